"""The modules' merged routes against the operator sequence written out here.

PointnetSAModule.forward and PointnetFPModule.forward resolve a geometry and hand it to the one function that runs the layer
stack on it, so "forward equals the geometry route" compares a thing with itself. These tests state each route independently,
in the style of tests/test_modules_gpu.py::test_level_entry_points_equal_the_operator_sequence: the public operators, then
the stack entry, on a copy of the module's weights. In deterministic mode outputs and every gradient must be the same bits.

Shapes as in tests/test_module_call_census_gpu.py (b = 4, n = 256, npoint 64, nsample 32, 16 channels, stack (16, 16, 32); FP:
256 unknown and 64 known points, c2 = 32, c1 = 16, stack (32, 32))."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, NPOINT, RADIUS, NSAMPLE, CFEAT, STACK = 4, 256, 64, 0.3, 32, 16, [16, 16, 32]
FP_M, FP_C2, FP_C1, FP_STACK = 64, 32, 16, [32, 32]


@pytest.fixture(scope="module")
def inputs(cuda):
    """coordinates, features, the FP level's known features and one weighting per output (never changed by a test)"""
    gen = torch.Generator().manual_seed(11)
    return {"xyz": torch.rand(B, N, 3, generator=gen).to(cuda),
            "feats": torch.randn(B, N, CFEAT, generator=gen).to(cuda),
            "feats2": torch.randn(B, FP_M, FP_C2, generator=gen).to(cuda),
            "w_sa": torch.randn(B, NPOINT, STACK[-1], generator=gen).to(cuda),
            "w_fp": torch.randn(B, N, FP_STACK[-1], generator=gen).to(cuda)}


@pytest.fixture
def deterministic():
    from pointnet2_amd import _tensors
    old = _tensors._deterministic
    _tensors.set_deterministic(True)
    yield
    _tensors.set_deterministic(old)


def _same_gradients(mod, ref, got_inputs, want_inputs):
    for a, b in zip(got_inputs, want_inputs):
        assert a.grad is not None and torch.equal(a.grad, b.grad)
    for (name, p), q in zip(mod.named_parameters(), ref.parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), name


@pytest.mark.parametrize("xyz_grad", [False, True])
@pytest.mark.parametrize("knn", [False, True])
def test_sa_train_equals_geometry_gather_node(cuda, inputs, deterministic, knn, xyz_grad):
    """sample_and_group_xyz (or FPS + gather and knn_point) -> [gather_point] -> sa_mlp_train"""
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    from pointnet2_amd.tf_grouping import knn_point, sample_and_group_xyz
    from pointnet2_amd.tf_sampling import farthest_point_sample_gather, gather_point
    torch.manual_seed(3)
    mod = U.PointnetSAModule(CFEAT, NPOINT, RADIUS, NSAMPLE, STACK, knn=knn).to(cuda).train()
    mod.fused_xyz_grad = xyz_grad
    ref = copy.deepcopy(mod)
    x, f = inputs["xyz"].clone().requires_grad_(xyz_grad), inputs["feats"].clone().requires_grad_(True)
    new_xyz, out, idx = mod(x, f)
    assert mod.last_path == "fused_train"
    (out * inputs["w_sa"]).sum().backward()

    rx, rf = inputs["xyz"].clone().requires_grad_(xyz_grad), inputs["feats"].clone().requires_grad_(True)
    if knn:
        fps_idx, want_xyz = farthest_point_sample_gather(NPOINT, rx)
        _, want_idx = knn_point(NSAMPLE, rx, want_xyz)
    else:
        fps_idx, want_xyz, want_idx, _, _ = sample_and_group_xyz(NPOINT, RADIUS, NSAMPLE, rx, True)
    if xyz_grad:
        want_xyz = gather_point(rx, fps_idx)
    want, _ = train_mlp.sa_mlp_train(ref.mlp.net, rx, want_xyz, rf, want_idx, True, "max", xyz_grad=xyz_grad)
    (want * inputs["w_sa"]).sum().backward()
    assert torch.equal(new_xyz, want_xyz) and torch.equal(idx, want_idx) and torch.equal(out, want)
    _same_gradients(mod, ref, [x, f] if xyz_grad else [f], [rx, rf] if xyz_grad else [rf])
    for a, b in zip(mod.buffers(), ref.buffers()):                      # running statistics, batch counters
        assert torch.equal(a, b)


@pytest.mark.parametrize("knn,pooling", [(True, "max"), (False, "avg")])
def test_sa_eval_equals_sampling_grouping_pool_kernel(cuda, inputs, knn, pooling):
    """FPS + gather -> knn_point or ball query -> sa_mlp_pool"""
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import sa_mlp
    from pointnet2_amd.tf_grouping import knn_point, query_ball_point
    from pointnet2_amd.tf_sampling import farthest_point_sample_gather
    torch.manual_seed(4)
    mod = U.PointnetSAModule(CFEAT, NPOINT, RADIUS, NSAMPLE, STACK, knn=knn, pooling=pooling).to(cuda).eval()
    x, f = inputs["xyz"], inputs["feats"]
    with torch.no_grad():
        new_xyz, out, idx = mod(x, f)
        assert mod.last_path == "fused"
        _, want_xyz = farthest_point_sample_gather(NPOINT, x)
        if knn:
            _, want_idx = knn_point(NSAMPLE, x, want_xyz)
        else:
            want_idx, _ = query_ball_point(RADIUS, NSAMPLE, x, want_xyz)
        want = sa_mlp.sa_mlp_pool(x, want_xyz, f, want_idx, mod._packed(cuda), pooling)
    assert torch.equal(new_xyz, want_xyz) and torch.equal(idx, want_idx) and torch.equal(out, want)


@pytest.mark.parametrize("form", ["node", "concat", "frozen"])
def test_fp_train_equals_three_nn_then_the_stack_entry(cuda, inputs, deterministic, monkeypatch, form):
    """three_nn -> fp_level_train, or fp_interp_concat -> fp_mlp_train (batch or frozen statistics)"""
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    from pointnet2_amd.tf_interpolate import fp_interp_concat, three_nn
    if form == "node":
        monkeypatch.setattr(train_mlp, "FP_NODE_MIN_SAVED", 0)
    torch.manual_seed(5)
    mod = U.PointnetFPModule(FP_C2 + FP_C1, FP_STACK).to(cuda)
    mod = mod.eval() if form == "frozen" else mod.train()
    mod.fused_frozen_bn = form == "frozen"
    ref = copy.deepcopy(mod)
    x, known = inputs["xyz"], inputs["xyz"][:, :FP_M].contiguous()
    f1, f2 = inputs["feats"].clone().requires_grad_(True), inputs["feats2"].clone().requires_grad_(True)
    out = mod(x, known, f1, f2)
    assert mod.last_path == ("fused_frozen" if form == "frozen" else "fused_train")
    (out * inputs["w_fp"]).sum().backward()

    r1, r2 = inputs["feats"].clone().requires_grad_(True), inputs["feats2"].clone().requires_grad_(True)
    dist, idx = three_nn(x, known)
    if form == "node":
        want = train_mlp.fp_level_train(ref.mlp.net, r2, r1, idx, dist)
    else:
        rows, _ = fp_interp_concat(r2, r1, idx, dist)
        want = train_mlp.fp_mlp_train(ref.mlp.net, rows, cin=FP_C2 + FP_C1, frozen=form == "frozen")
    (want * inputs["w_fp"]).sum().backward()
    assert torch.equal(out, want)
    _same_gradients(mod, ref, [f1, f2], [r1, r2])
    for a, b in zip(mod.buffers(), ref.buffers()):
        assert torch.equal(a, b)
