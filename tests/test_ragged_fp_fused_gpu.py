"""PointnetFPModule.fused_ragged_train (opt-in): train() with a ragged unknown side on fp_interp_concat + the fused node with a
row mask (last_path "fused_train_ragged") instead of the compacting layer-by-layer path. The shapes, the padding fills and the
restatement are tests/test_ragged_modules_gpu.py::test_fp_train's: B 4, N 1024, lengths (1024, 700, 300, 64), 64 known points,
C2 32, 6 skip channels, stack [64, 32]; the padding rows of xyz1 are NaN.

One difference from that test: the restatement's layer stack runs in float64 (its three_nn and interpolation stay the fp32
operators). A conv bias under batch normalisation has a gradient of exactly zero, which is what the node returns; the fp32
layer-by-layer stack returns its own rounding noise there (2.5e-5 measured at this shape, above the 1e-5 bound), so an fp32
restatement can only be met by a path that repeats its rounding. The bound stays 1e-5 of each tensor's scale."""
import copy

import numpy as np
import pytest
import torch

from test_ragged_modules_gpu import B, LENGTHS, N, _fp, _fp_inputs, case  # noqa: F401  (case: the module's fixture)

pytestmark = pytest.mark.gpu


def _check(cuda, case, index_plans):
    import pointnet2_amd as P
    mod = _fp(cuda).train()
    mod.fused_ragged_train = True
    mod.index_plans = index_plans
    ref = copy.deepcopy(mod).train().double()
    x1, x2, p1, p2 = _fp_inputs(case, cuda)
    total = sum(LENGTHS)
    torch.manual_seed(78)
    wout = torch.randn(total, 32, device=cuda)
    valid = torch.zeros(B, N, dtype=torch.bool, device=cuda)
    for i, ni in enumerate(LENGTHS):
        valid[i, :ni] = True

    p1a, p2a = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    out = mod(x1, x2, p1a, p2a, lengths1=LENGTHS)
    assert mod.last_path == "fused_train_ragged"
    assert int((out[~valid] != 0).sum()) == 0
    (out[valid] * wout).sum().backward()

    p1b, p2b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    rows = []
    for i, ni in enumerate(LENGTHS):
        d, ix = P.three_nn(x1[i:i + 1, :ni].contiguous(), x2[i:i + 1])
        inv = 1.0 / torch.clamp(d, min=1e-10)
        w = inv / inv.sum(dim=2, keepdim=True)
        rows.append(torch.cat([P.three_interpolate(p2b[i:i + 1], ix, w), p1b[i:i + 1, :ni]], dim=2)[0])
    X = torch.cat(rows, dim=0)                                              # (total, C)
    y = ref.mlp(X.double().t().unsqueeze(0).unsqueeze(3))[0, :, :, 0].t()   # (1, C, total, 1) -> (total, C_out), float64
    (y * wout.double()).sum().backward()

    def close(got, want, what):
        got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
        err, bound = np.abs(got - want).max(), 1e-5 * max(1.0, np.abs(want).max())
        print("%s: max error %.3e (bound %.3e)" % (what, err, bound))
        assert err <= bound, what

    close(out[valid], y, "output")
    close(p1a.grad[valid], p1b.grad[valid], "grad points1")
    assert int((p1a.grad[~valid] != 0).sum()) == 0 and torch.isfinite(p1a.grad).all()
    close(p2a.grad, p2b.grad, "grad points2")
    for (name, pa), pb in zip(mod.named_parameters(), ref.parameters()):
        close(pa.grad, pb.grad, "grad " + name)
    for ma, mb in zip(mod.modules(), ref.modules()):
        if isinstance(ma, torch.nn.BatchNorm2d):
            assert int(ma.num_batches_tracked) == 1                          # updated once
            close(ma.running_mean, mb.running_mean, "running_mean")
            close(ma.running_var, mb.running_var, "running_var")


def test_fp_train_fused_ragged(cuda, case):
    _check(cuda, case, index_plans=False)


def test_fp_train_fused_ragged_with_index_plans(cuda, case):
    """the planned scatter of the interpolation gradient behind the masked node"""
    _check(cuda, case, index_plans=True)


def test_flag_off_keeps_the_unfused_path(cuda, case):
    mod = _fp(cuda).train()
    assert mod.fused_ragged_train is False
    x1, x2, p1, p2 = _fp_inputs(case, cuda)
    mod(x1, x2, p1, p2, lengths1=LENGTHS)
    assert mod.last_path == "unfused_ragged"


def test_eval_is_unchanged_by_the_flag(cuda, case):
    x1, x2, p1, p2 = _fp_inputs(case, cuda)
    outs = []
    for flag in (False, True):
        mod = _fp(cuda).eval()
        mod.fused_ragged_train = flag
        with torch.no_grad():
            outs.append(mod(x1, x2, p1, p2, lengths1=LENGTHS))
        assert mod.last_path != "fused_train_ragged"
    assert torch.equal(outs[0], outs[1])
