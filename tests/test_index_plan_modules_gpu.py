"""Index plans from the operators up to the modules (pointnet2_amd/index_plan.py): with a plan -- given by the caller, built by
the module where idx is born (index_plans = True) or carried by a geometry computed ahead (GeometryAhead(..., plans=True)) --
the gradients are those of the calls without one: bit for bit in the reproducible mode, within the training tests' bounds in
the default mode."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture()
def deterministic():
    import pointnet2_amd as P
    P.set_deterministic(True)
    yield P
    P.set_deterministic(False)


def _padded_idx(b, n, m, ns, dev, seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    idx = torch.sort(torch.randint(0, n, (b, m, ns), generator=g), dim=2)[0]
    k = torch.randint(1, ns + 1, (b, m, 1), generator=g)
    idx = torch.where(torch.arange(ns).view(1, 1, ns) >= k, idx[:, :, :1], idx)            # the first hit repeated
    return idx.to(torch.int32).to(dev)


@pytest.mark.parametrize("c", [3, 64])
def test_group_point_with_a_plan(cuda, deterministic, c):
    P = deterministic
    b, n, m, ns = 4, 300, 40, 16
    idx = _padded_idx(b, n, m, ns, cuda, 1)
    g = torch.randn(b, m, ns, c, device=cuda)
    plan = P.index_plan(idx, n, "group")
    assert (plan.b, plan.rows, plan.entries, plan.kind, plan.sorted) == (b, n, m * ns, "group", True)
    grads = []
    for p in (None, plan, plan):
        pts = torch.zeros(b, n, c, device=cuda, requires_grad=True)
        out = P.group_point(pts, idx, plan=p)
        out.backward(g)
        grads.append(pts.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    pts = torch.zeros(b, n, c, device=cuda, requires_grad=True)
    for bad in (P.index_plan(idx, n + 1, "group"), P.index_plan(idx[:, :, :3].contiguous(), n, "interpolate"),
                P.index_plan(idx[:, :-1].contiguous(), n, "group")):
        with pytest.raises(ValueError):
            P.group_point(pts, idx, plan=bad)


@pytest.mark.parametrize("c", [3, 36])
def test_three_interpolate_with_a_plan(cuda, deterministic, c):
    P = deterministic
    b, n, m = 4, 500, 60
    idx = torch.randint(0, m, (b, n, 3), device=cuda, dtype=torch.int32)
    w = torch.rand(b, n, 3, device=cuda)
    g = torch.randn(b, n, c, device=cuda)
    plan = P.index_plan(idx, m, "interpolate")
    grads = []
    for p in (None, plan, plan):
        pts = torch.zeros(b, m, c, device=cuda, requires_grad=True)
        P.three_interpolate(pts, idx, w, plan=p).backward(g)
        grads.append(pts.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    pts = torch.zeros(b, m, c, device=cuda, requires_grad=True)
    for bad in (P.index_plan(idx, m + 1, "interpolate"), P.index_plan(idx, m, "group"),
                P.index_plan(idx[:, :-1].contiguous(), m, "interpolate")):
        with pytest.raises(ValueError):
            P.three_interpolate(pts, idx, w, plan=bad)


def test_default_mode_operators_with_a_plan(cuda):
    """Default mode: the planned reduce is deterministic too (no float atomics), and close to the unplanned gradient."""
    import pointnet2_amd as P
    b, n, m, ns, c = 4, 300, 40, 16, 64
    idx = _padded_idx(b, n, m, ns, cuda, 2)
    g = torch.randn(b, m, ns, c, device=cuda)
    plan = P.index_plan(idx, n, "group")
    assert plan.sorted is False
    grads = []
    for p in (None, plan, plan):
        pts = torch.zeros(b, n, c, device=cuda, requires_grad=True)
        P.group_point(pts, idx, plan=p).backward(g)
        grads.append(pts.grad)
    assert torch.equal(grads[1], grads[2])
    assert float((grads[0] - grads[1]).abs().max()) <= 1e-5 * float(grads[0].abs().max())


# ---- levels: (kind of SA level, feature channels, l1_per_point, coordinate gradient, FP path) ----
LEVELS = {
    "sa_python_scatter": ("sa", 6, False, False, "concat"),       # the issue's level: 6 channels, the scatter of train_mlp.py
    "sa_per_point_asked": ("sa", 6, True, False, "node"),         # the same with l1_per_point asked for (6 channels: never taken)
    "sa_c_scatter": ("sa", 8, True, False, "node"),               # 8 channels: layer 1 per point, the scatter inside the C call
    "sa_c_scatter_off": ("sa", 8, False, False, "concat"),
    "sa_xyz": ("sa", 6, False, True, "node"),                     # fused_xyz_grad: two reductions from one inversion
    "sa_xyz_per_point": ("sa", 8, True, True, "concat"),
    "msg": ("msg", 6, False, False, "concat"),
    "msg_xyz": ("msg", 6, False, True, "node"),
}


class _Net(torch.nn.Module):
    """One SA (or MSG) level and the FP level that brings its features back onto the input points."""

    def __init__(self, kind, cfeat):
        import pointnet2_amd.pointnet_util as U
        super().__init__()
        if kind == "sa":
            self.sa = U.PointnetSAModule(cfeat, 64, 0.3, 32, [16, 16, 32])
            c2 = 32
        else:
            self.sa = U.PointnetSAModuleMSG(cfeat, 64, [0.2, 0.4], [16, 32], [[16, 16, 32], [16, 16, 32]])
            c2 = 64
        self.fp = U.PointnetFPModule(c2 + cfeat, [32, 32])

    def forward(self, xyz, feats, geometry=None):
        out = self.sa(xyz, feats, geometry=None if geometry is None else geometry.sa[0])
        new_xyz, f1 = out[0], out[1]
        return self.fp(xyz, new_xyz, feats, f1, geometry=None if geometry is None else geometry.fp[0])


def _run(net, xyz0, feats0, weight, want_xyz, geometry=None):
    net.zero_grad(set_to_none=True)
    xyz = xyz0.clone().requires_grad_(want_xyz)
    feats = feats0.clone().requires_grad_(True)
    out = net(xyz, feats, geometry)
    (out * weight).sum().backward()
    grads = {"out": out.detach(), "feats": feats.grad}
    if want_xyz:
        grads["xyz"] = xyz.grad
    for name, p in net.named_parameters():
        grads[name] = p.grad.clone()
    return grads


def _three_ways(cuda, level, monkeypatch):
    from pointnet2_amd import train_mlp
    from pointnet2_amd.geometry import GeometryAhead
    kind, cfeat, per_point, want_xyz, fp_path = LEVELS[level]
    monkeypatch.setattr(train_mlp, "FP_NODE_MIN_SAVED", 0 if fp_path == "node" else 1 << 60)
    torch.manual_seed(7)
    net = _Net(kind, cfeat).to(cuda).train()
    net.sa.fused_xyz_grad = want_xyz
    b, n = 4, 256
    xyz = torch.rand(b, n, 3, device=cuda)
    feats = torch.randn(b, n, cfeat, device=cuda)
    weight = torch.randn(b, n, 32, device=cuda)
    state = copy.deepcopy(net.state_dict())
    results = {}
    with train_mlp.options(l1_per_point=per_point):
        for way in ("none", "module", "geometry", "static"):
            net.load_state_dict(state)                                     # the running statistics of every run start alike
            net.sa.index_plans = net.fp.index_plans = way == "module"
            g = None
            if way in ("geometry", "static"):
                ahead = GeometryAhead([net.sa], [(0, 1)], plans=True)
                g = ahead.submit(xyz)
                assert g.sa[0].plan is not None and g.fp[0].plan is not None
                if way == "static":
                    # a static geometry refilled from a fresh one (of other coordinates first, so that copy_ has to bring the plans over)
                    for lvl in list(g.sa) + list(g.fp):
                        lvl.wait()
                    static = ahead.compute(torch.rand(b, n, 3, device=cuda)).static_copy()
                    assert len(static.tensors()) == len(g.tensors())
                    g = static.copy_(g)
            results[way] = _run(net, xyz, feats, weight, want_xyz, g)
            assert net.sa.last_path == "fused_train" and net.fp.last_path == "fused_train"
    return results


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_levels_reproducible_mode(cuda, deterministic, monkeypatch, level):
    res = _three_ways(cuda, level, monkeypatch)
    for way in ("module", "geometry", "static"):
        for name, want in res["none"].items():
            assert torch.equal(res[way][name], want), (way, name)


@pytest.mark.parametrize("level", sorted(LEVELS))
def test_levels_default_mode(cuda, monkeypatch, level):
    """The bounds tests/test_train_mlp_gpu.py applies to the same tensors: 2e-3 (single-scale level) / 5e-3 (MSG and FP) of the
    gradient's norm; the forward does not depend on a plan at all."""
    res = _three_ways(cuda, level, monkeypatch)
    for way in ("module", "geometry", "static"):
        for name, want in res["none"].items():
            got = res[way][name]
            if name == "out":
                assert torch.equal(got, want), way
                continue
            bound = 2e-3 if name.startswith("sa.mlp.") and LEVELS[level][0] == "sa" else 5e-3
            norm = float(want.norm())
            if norm < 1e-6:                                                # conv biases under batch norm: zero
                assert float(got.abs().max()) <= 1e-6, (way, name)
                continue
            err = float((got - want).norm()) / norm
            print("%s %s %s: %.2e" % (level, way, name, err))
            assert err <= bound, (way, name, err)


def test_training_nodes_refuse_a_wrong_plan(cuda):
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    torch.manual_seed(3)
    b, n, m, ns = 4, 256, 64, 32
    sa = U.PointnetSAModule(8, m, 0.3, ns, [16, 16, 32]).to(cuda).train()
    xyz = torch.rand(b, n, 3, device=cuda)
    g = sa.geometry(xyz, plans=True)
    assert g.plan is not None and g.plan.kind == "group" and len(g._tensors) == 4
    feats = torch.randn(b, n, 8, device=cuda, requires_grad=True)
    interp = P.index_plan(g.idx[:, :, :3].contiguous(), n, "interpolate")
    with pytest.raises(ValueError):
        train_mlp.sa_mlp_train(sa.mlp.net, xyz, g.new_xyz, feats, g.idx, plan=interp)
    with pytest.raises(ValueError):
        train_mlp.sa_mlp_train(sa.mlp.net, xyz, g.new_xyz, feats, g.idx, plan=P.index_plan(g.idx, n + 1, "group"))
    fp = U.PointnetFPModule(32 + 8, [32, 32]).to(cuda).train()
    dist, idx = P.three_nn(xyz, g.new_xyz)
    p2 = torch.randn(b, m, 32, device=cuda, requires_grad=True)
    with pytest.raises(ValueError):
        train_mlp.fp_level_train(fp.mlp.net, p2, feats, idx, dist, plan=g.plan)
    with pytest.raises(ValueError):
        train_mlp.fp_level_train(fp.mlp.net, p2, feats, idx, dist, plan=P.index_plan(idx, m + 1, "interpolate"))
