"""Ragged batches through the modules (PointnetSAModule / PointnetSAModuleMSG .geometry(..., lengths=) and
.forward(..., lengths=), PointnetFPModule.forward(..., lengths1=)) on the GPU.

One shape throughout: b = 4 clouds padded to n = 1024 with lengths (1024, 700, 300, 64), npoint 64, nsample 16, layer stack
(32, 32, 64), 6 feature channels. The geometry a ragged level must produce is the CPU oracle's on every slice
xyz[i:i+1, :lengths[i]], computed once for the module."""
import copy

import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

B, N, LENGTHS = 4, 1024, [1024, 700, 300, 64]
NPOINT, RADIUS, NSAMPLE, WIDTHS, CFEAT = 64, 0.2, 16, [32, 32, 64], 6
MSG_RADII, MSG_NSAMPLES = [0.2, 0.4], [16, 32]


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bound(want):
    """the bound of tests/test_modules_gpu.py: 1e-5 of the output scale"""
    return 1e-5 * max(1.0, float(np.abs(want).max()))


@pytest.fixture(scope="module")
def case(oracle):
    """clouds, features and the per-slice oracle geometry (never changed by a test)"""
    xyz = S.sphere_clouds(B, N, 71)
    feats = np.random.default_rng(72).standard_normal((B, N, CFEAT)).astype(np.float32)
    fps, new_xyz, idx = [], [], {r: [] for r in MSG_RADII}
    for i, ni in enumerate(LENGTHS):
        sl = xyz[i:i + 1, :ni]
        f = oracle.farthest_point_sample(NPOINT, sl)
        q = oracle.gather_point(sl, f)
        fps.append(f[0]); new_xyz.append(q[0])
        for r, k in zip(MSG_RADII, MSG_NSAMPLES):
            idx[r].append(oracle.query_ball_point(r, k, sl, q)[0][0])
    return {"xyz": xyz, "feats": feats, "fps": np.stack(fps), "new_xyz": np.stack(new_xyz),
            "idx": {r: np.stack(v) for r, v in idx.items()}}


def _padded(a, fill, seed=0):
    """rows at or beyond the lengths: NaN, zeros, or finite random values"""
    out = a.copy()
    rng = np.random.default_rng(seed)
    for i, ni in enumerate(LENGTHS):
        if fill == "nan":
            out[i, ni:] = np.nan
        elif fill == "zero":
            out[i, ni:] = 0.0
        else:
            out[i, ni:] = rng.standard_normal(out[i, ni:].shape).astype(np.float32)
    return out


def _sa(cuda, **kw):
    from pointnet2_amd.pointnet_util import PointnetSAModule
    torch.manual_seed(73)
    return PointnetSAModule(CFEAT, NPOINT, RADIUS, NSAMPLE, WIDTHS, **kw).to(cuda)


def _oracle_geometry(case, cuda, radii=None):
    from pointnet2_amd.geometry import SAGeometry
    idx = [_dev(case["idx"][r], cuda) for r in radii] if radii else _dev(case["idx"][RADIUS], cuda)
    return SAGeometry(_dev(case["new_xyz"], cuda), idx, _dev(case["fps"], cuda))


def test_sa_geometry_is_the_oracles_per_slice(cuda, case):
    mod = _sa(cuda)
    x = _dev(_padded(case["xyz"], "nan"), cuda)
    g = mod.geometry(x, lengths=LENGTHS)
    assert np.array_equal(g.fps_idx.cpu().numpy(), case["fps"])
    assert np.array_equal(g.new_xyz.cpu().numpy(), case["new_xyz"])
    assert np.array_equal(g.idx.cpu().numpy(), case["idx"][RADIUS])
    gp = mod.geometry(x, plans=True, lengths=torch.tensor(LENGTHS, device=cuda))
    assert gp.plan is not None and torch.equal(gp.idx, g.idx)


def test_sa_forward_equals_the_geometry_route(cuda, case):
    """forward(lengths=) == forward(geometry=<the oracle's per-slice geometry>), bit for bit, on every stack path"""
    x = _dev(_padded(case["xyz"], "nan"), cuda)
    pts = _dev(_padded(case["feats"], "random", 1), cuda)
    g = _oracle_geometry(case, cuda)
    mod = _sa(cuda).eval()
    with torch.no_grad():
        a = mod(x, pts, lengths=LENGTHS)
        assert mod.last_path == "fused"
        b = mod(x, pts, geometry=g)
        assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.isfinite(a[1]).all()
        mod.fused_mlp = False
        a = mod(x, pts, lengths=LENGTHS)
        assert mod.last_path == "unfused"
        b = mod(x, pts, geometry=g)
        assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.isfinite(a[1]).all()
    mod = _sa(cuda).train()
    x = _dev(_padded(case["xyz"], "random", 7), cuda)                         # the training node wants finite padding rows
    a = mod(x, pts, lengths=LENGTHS)
    assert mod.last_path == "fused_train"
    b = mod(x, pts, geometry=g)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.isfinite(a[1]).all()


def test_sa_eval_against_the_single_cloud_module_and_float64(cuda, case, oracle):
    from oracle import sa_module as OM
    mod = _sa(cuda).eval()
    x = _dev(_padded(case["xyz"], "nan"), cuda)
    pts = _dev(_padded(case["feats"], "random", 2), cuda)
    with torch.no_grad():
        new_xyz, out, idx = mod(x, pts, lengths=LENGTHS)
        for i, ni in enumerate(LENGTHS):
            sx, so, si = mod(x[i:i + 1, :ni].contiguous(), pts[i:i + 1, :ni].contiguous())
            assert torch.equal(new_xyz[i:i + 1], sx) and torch.equal(idx[i:i + 1], si)
            want = so.double().cpu().numpy()
            err = np.abs(out[i:i + 1].double().cpu().numpy() - want).max()
            print("cloud %d: max |ragged - single cloud| = %.3e (bound %.3e)" % (i, err, _bound(want)))
            assert err <= _bound(want)
    # the float64 restatement of the learned part, fed with the oracle's grouped tensors
    widx = case["idx"][RADIUS]
    gxyz = np.stack([case["xyz"][i][widx[i]] for i in range(B)]) - case["new_xyz"][:, :, None, :]
    gfeat = np.stack([case["feats"][i][widx[i]] for i in range(B)])
    want = OM.sa_learned_part(gxyz, np.concatenate([gxyz, gfeat], axis=-1), OM.layers_of(mod.mlp.net), "max")
    err = np.abs(out.double().cpu().numpy() - want).max()
    print("max |ragged - float64| = %.3e (bound %.3e)" % (err, _bound(want)))
    assert err <= _bound(want)


def test_sa_padding_invariance_in_training(cuda, case):
    """train(), deterministic mode, coordinate gradients from the fused node: outputs and every gradient are bit-identical
    between zero padding and finite random padding (coordinates and features); the padding rows' own gradients are zero."""
    import pointnet2_amd as P
    torch.manual_seed(74)
    wout = torch.randn(B, NPOINT, WIDTHS[-1], device=cuda)
    was = P.is_deterministic()
    P.set_deterministic(True)
    res = {}
    try:
        for fill in ("zero", "random"):
            mod = _sa(cuda).train()
            mod.fused_xyz_grad = True
            x = _dev(_padded(case["xyz"], fill, 3), cuda).requires_grad_(True)
            pts = _dev(_padded(case["feats"], fill, 4), cuda).requires_grad_(True)
            _, out, _ = mod(x, pts, lengths=LENGTHS)
            (out * wout).sum().backward()
            print(fill, "padding: path", mod.last_path)
            res[fill] = (out.detach(), x.grad, pts.grad, [p.grad for p in mod.parameters()])
    finally:
        P.set_deterministic(was)
    a, b = res["zero"], res["random"]
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert len(a[3]) == len(b[3]) > 0 and all(torch.equal(u, v) for u, v in zip(a[3], b[3]))
    assert all(torch.isfinite(t).all() for t in (b[0], b[1], b[2]))
    assert float(b[1].abs().sum()) > 0 and float(b[2].abs().sum()) > 0
    for i, ni in enumerate(LENGTHS):
        assert int((b[1][i, ni:] != 0).sum()) == 0 and int((b[2][i, ni:] != 0).sum()) == 0


def test_msg_module(cuda, case):
    from pointnet2_amd.pointnet_util import PointnetSAModuleMSG
    torch.manual_seed(75)
    mod = PointnetSAModuleMSG(CFEAT, NPOINT, MSG_RADII, MSG_NSAMPLES, [WIDTHS, WIDTHS]).to(cuda).eval()
    x = _dev(_padded(case["xyz"], "nan"), cuda)
    pts = _dev(_padded(case["feats"], "random", 5), cuda)
    g = mod.geometry(x, lengths=LENGTHS)
    assert np.array_equal(g.new_xyz.cpu().numpy(), case["new_xyz"]) and np.array_equal(g.fps_idx.cpu().numpy(), case["fps"])
    for r, idx in zip(MSG_RADII, g.idx):
        assert np.array_equal(idx.cpu().numpy(), case["idx"][r]), r
    with torch.no_grad():
        a = mod(x, pts, lengths=LENGTHS)
        b = mod(x, pts, geometry=_oracle_geometry(case, cuda, MSG_RADII))
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.isfinite(a[1]).all()
    mod.train()
    x = _dev(_padded(case["xyz"], "random", 8), cuda)                         # the training node wants finite padding rows
    a = mod(x, pts, lengths=LENGTHS)
    b = mod(x, pts, geometry=_oracle_geometry(case, cuda, MSG_RADII))
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.isfinite(a[1]).all()


def test_group_all_with_lengths_is_refused(cuda, case):
    mod = _sa(cuda, group_all=True).eval()
    x, pts = _dev(case["xyz"], cuda), _dev(case["feats"], cuda)
    with pytest.raises(ValueError):
        mod(x, pts, lengths=LENGTHS)
    with pytest.raises(ValueError):
        mod.geometry(x, lengths=LENGTHS)


# ---------------------------------------------------------------------------------------------------- feature propagation
C2 = 32


def _fp(cuda):
    from pointnet2_amd.pointnet_util import PointnetFPModule
    torch.manual_seed(76)
    return PointnetFPModule(C2 + CFEAT, [64, 32]).to(cuda)


def _fp_inputs(case, cuda):
    x1 = _dev(_padded(case["xyz"], "nan"), cuda)
    x2 = _dev(case["new_xyz"], cuda)                                         # the known side: a previous level's dense output
    p1 = _dev(_padded(case["feats"], "random", 6), cuda)
    p2 = _dev(np.random.default_rng(77).standard_normal((B, NPOINT, C2)).astype(np.float32), cuda)
    return x1, x2, p1, p2


def test_fp_eval(cuda, case):
    mod = _fp(cuda).eval()
    x1, x2, p1, p2 = _fp_inputs(case, cuda)
    with torch.no_grad():
        out = mod(x1, x2, p1, p2, lengths1=LENGTHS)
        assert torch.isfinite(out).all()
        for i, ni in enumerate(LENGTHS):
            assert int((out[i, ni:] != 0).sum()) == 0                       # exactly zero beyond the length
            want = mod(x1[i:i + 1, :ni].contiguous(), x2[i:i + 1], p1[i:i + 1, :ni].contiguous(), p2[i:i + 1]).double().cpu().numpy()
            err = np.abs(out[i:i + 1, :ni].double().cpu().numpy() - want).max()
            print("cloud %d: max |ragged - single cloud| = %.3e (bound %.3e)" % (i, err, _bound(want)))
            assert err <= _bound(want)


def test_fp_train(cuda, case):
    """train(): batch statistics over the valid rows only. Restatement: per-slice three_nn + interpolation, the valid rows of
    all clouds concatenated, the module's own layer stack in train mode on (1, C, total, 1). Output and the gradients with
    respect to points1, points2 and the weights within 1e-5 of each tensor's scale; running statistics updated once."""
    import pointnet2_amd as P
    mod = _fp(cuda).train()
    ref = copy.deepcopy(mod).train()
    x1, x2, p1, p2 = _fp_inputs(case, cuda)
    total = sum(LENGTHS)
    torch.manual_seed(78)
    wout = torch.randn(total, 32, device=cuda)
    valid = torch.zeros(B, N, dtype=torch.bool, device=cuda)
    for i, ni in enumerate(LENGTHS):
        valid[i, :ni] = True

    p1a, p2a = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    out = mod(x1, x2, p1a, p2a, lengths1=LENGTHS)
    assert mod.last_path == "unfused_ragged"
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
    y = ref.mlp(X.t().unsqueeze(0).unsqueeze(3))[0, :, :, 0].t()            # (1, C, total, 1) -> (total, C_out)
    (y * wout).sum().backward()

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
