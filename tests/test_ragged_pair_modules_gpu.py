"""Per-cloud sample counts and a ragged known side through the modules (PointnetSAModule / PointnetSAModuleMSG
.geometry(..., lengths=, npoints=) and .forward(..., lengths=, npoints=), PointnetFPModule.forward(..., lengths1=, lengths2=))
on the GPU.

Shapes: b = 4 clouds padded to n = 1024 with lengths (1024, 700, 300, 40); level 1 npoint 128 with npoints (128, 96, 40, 8);
level 2 npoint 32 with npoints (32, 24, 10, 2); stacks as in test_ragged_modules_gpu.py. The geometry a level must produce is
the CPU oracle's on every slice, extended by the operators' fills (sample 0 as the centroid, a group of point 0)."""
import copy

import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

B, N, LENGTHS = 4, 1024, [1024, 700, 300, 40]
NPOINT1, NPOINTS1 = 128, [128, 96, 40, 8]
NPOINT2, NPOINTS2 = 32, [32, 24, 10, 2]
RADIUS, NSAMPLE, WIDTHS, CFEAT = 0.2, 16, [32, 32, 64], 6
MSG_RADII, MSG_NSAMPLES = [0.2, 0.4], [16, 32]


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _bound(want):
    """the bound of tests/test_modules_gpu.py: 1e-5 of the output scale"""
    return 1e-5 * max(1.0, float(np.abs(want).max()))


def _close(got, want, what):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    err = np.abs(got - want).max() if got.size else 0.0
    print("%s: max error %.3e (bound %.3e)" % (what, err, _bound(want)))
    assert err <= _bound(want), what


@pytest.fixture(scope="module")
def case(oracle):
    """clouds, features and the per-slice oracle geometry of level 1 extended by the fills (never changed by a test)"""
    xyz = S.sphere_clouds(B, N, 71)
    feats = np.random.default_rng(72).standard_normal((B, N, CFEAT)).astype(np.float32)
    fps = np.zeros((B, NPOINT1), dtype=np.int32)
    idx = {r: np.zeros((B, NPOINT1, k), dtype=np.int32) for r, k in zip(MSG_RADII, MSG_NSAMPLES)}
    for i, (ni, mi) in enumerate(zip(LENGTHS, NPOINTS1)):
        sl = xyz[i:i + 1, :ni]
        fps[i, :mi] = oracle.farthest_point_sample(mi, sl)[0]
        q = oracle.gather_point(sl, fps[i:i + 1, :mi])
        for r, k in zip(MSG_RADII, MSG_NSAMPLES):
            idx[r][i, :mi] = oracle.query_ball_point(r, k, sl, q)[0][0]
    new_xyz = np.stack([xyz[i][fps[i]] for i in range(B)])
    return {"xyz": xyz, "feats": feats, "fps": fps, "new_xyz": new_xyz, "idx": idx}


def _padded(a, fill, seed=0, lengths=LENGTHS):
    """rows at or beyond the lengths: NaN, zeros, or finite random values"""
    out = a.copy()
    rng = np.random.default_rng(seed)
    for i, ni in enumerate(lengths):
        if fill == "nan":
            out[i, ni:] = np.nan
        elif fill == "zero":
            out[i, ni:] = 0.0
        else:
            out[i, ni:] = rng.standard_normal(out[i, ni:].shape).astype(np.float32)
    return out


def _valid(counts, m, cuda):
    v = torch.zeros(len(counts), m, dtype=torch.bool, device=cuda)
    for i, c in enumerate(counts):
        v[i, :c] = True
    return v


def _sa(cuda, **kw):
    from pointnet2_amd.pointnet_util import PointnetSAModule
    torch.manual_seed(73)
    return PointnetSAModule(CFEAT, NPOINT1, RADIUS, NSAMPLE, WIDTHS, **kw).to(cuda)


def _msg(cuda):
    from pointnet2_amd.pointnet_util import PointnetSAModuleMSG
    torch.manual_seed(75)
    return PointnetSAModuleMSG(CFEAT, NPOINT1, MSG_RADII, MSG_NSAMPLES, [WIDTHS, WIDTHS]).to(cuda)


def _oracle_geometry(case, cuda, radii=None):
    from pointnet2_amd.geometry import SAGeometry
    idx = [_dev(case["idx"][r], cuda) for r in radii] if radii else _dev(case["idx"][RADIUS], cuda)
    return SAGeometry(_dev(case["new_xyz"], cuda), idx, _dev(case["fps"], cuda))


def _with_npoint(mod, m, fn):
    """fn() with mod.npoint = m (the single-cloud module of a cloud with m valid centroids)"""
    was = mod.npoint
    mod.npoint = m
    try:
        return fn()
    finally:
        mod.npoint = was


# --------------------------------------------------------------------------------------------------------------- geometry
def test_sa_geometry_is_the_oracles_per_slice_extended_by_the_fills(cuda, case):
    mod = _sa(cuda)
    x = _dev(_padded(case["xyz"], "nan"), cuda)
    g = mod.geometry(x, lengths=LENGTHS, npoints=NPOINTS1)
    assert np.array_equal(g.fps_idx.cpu().numpy(), case["fps"])
    assert np.array_equal(g.new_xyz.cpu().numpy().view(np.uint32), case["new_xyz"].view(np.uint32))
    assert np.array_equal(g.idx.cpu().numpy(), case["idx"][RADIUS])
    gp = mod.geometry(x, plans=True, lengths=torch.tensor(LENGTHS, device=cuda), npoints=torch.tensor(NPOINTS1, device=cuda))
    assert gp.plan is not None and torch.equal(gp.idx, g.idx)
    knn = _sa(cuda, knn=True)
    gk = knn.geometry(x, lengths=LENGTHS, npoints=NPOINTS1)
    assert torch.equal(gk.new_xyz, g.new_xyz)
    for i, (ni, mi) in enumerate(zip(LENGTHS, NPOINTS1)):
        assert int(gk.idx[i].max()) < ni and int(gk.idx[i, mi:].abs().sum()) == 0


def test_msg_geometry_one_launch_or_one_per_radius(cuda, case):
    mod = _msg(cuda)
    x = _dev(_padded(case["xyz"], "nan"), cuda)
    g = mod.geometry(x, lengths=LENGTHS, npoints=NPOINTS1)
    mod.ragged_one_launch = True
    g1 = mod.geometry(x, lengths=LENGTHS, npoints=NPOINTS1)
    assert np.array_equal(g.new_xyz.cpu().numpy(), case["new_xyz"]) and np.array_equal(g.fps_idx.cpu().numpy(), case["fps"])
    assert torch.equal(g.new_xyz, g1.new_xyz) and torch.equal(g.fps_idx, g1.fps_idx)
    for r, idx, idx1 in zip(MSG_RADII, g.idx, g1.idx):
        assert np.array_equal(idx.cpu().numpy(), case["idx"][r]), r
        assert torch.equal(idx, idx1), r


# ---------------------------------------------------------------------------------------------------------------- SA eval
def test_sa_eval(cuda, case):
    """forward(lengths=, npoints=) == forward(geometry=<the oracle's geometry>) on the rows below m_c, bit for bit, on the fused
    and the unfused stack path; exact zeros beyond; per cloud within the module bound of the single-cloud module"""
    x = _dev(_padded(case["xyz"], "nan"), cuda)
    pts = _dev(_padded(case["feats"], "random", 1), cuda)
    g = _oracle_geometry(case, cuda)
    valid = _valid(NPOINTS1, NPOINT1, cuda)
    mod = _sa(cuda).eval()
    with torch.no_grad():
        for fused, path in ((True, "fused"), (False, "unfused")):
            mod.fused_mlp = fused
            new_xyz, out, idx = mod(x, pts, lengths=LENGTHS, npoints=NPOINTS1)
            assert mod.last_path == path
            gx, gout, gidx = mod(x, pts, geometry=g)
            assert torch.equal(new_xyz, gx) and torch.equal(idx, gidx)
            assert torch.equal(out[valid], gout[valid]) and torch.isfinite(out).all()
            assert int((out[~valid] != 0).sum()) == 0
            for i, (ni, mi) in enumerate(zip(LENGTHS, NPOINTS1)):
                sx, so, si = _with_npoint(mod, mi, lambda: mod(x[i:i + 1, :ni].contiguous(), pts[i:i + 1, :ni].contiguous()))
                assert torch.equal(new_xyz[i:i + 1, :mi], sx) and torch.equal(idx[i:i + 1, :mi], si)
                _close(out[i:i + 1, :mi], so, "%s cloud %d: ragged - single cloud" % (path, i))


def test_sa_eval_counts_without_lengths(cuda, case):
    mod = _sa(cuda).eval()
    x, pts = _dev(case["xyz"], cuda), _dev(case["feats"], cuda)
    with torch.no_grad():
        a = mod(x, pts, npoints=NPOINTS1)
        b = mod(x, pts, lengths=[N] * B, npoints=NPOINTS1)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert int((a[1][~_valid(NPOINTS1, NPOINT1, cuda)] != 0).sum()) == 0


def test_msg_eval(cuda, case):
    x = _dev(_padded(case["xyz"], "nan"), cuda)
    pts = _dev(_padded(case["feats"], "random", 5), cuda)
    g = _oracle_geometry(case, cuda, MSG_RADII)
    valid = _valid(NPOINTS1, NPOINT1, cuda)
    mod = _msg(cuda).eval()
    with torch.no_grad():
        for fused, path in ((True, "fused"), (False, "unfused")):
            mod.fused_mlp = fused
            mod.ragged_one_launch = False
            new_xyz, out = mod(x, pts, lengths=LENGTHS, npoints=NPOINTS1)
            assert mod.last_path == path
            mod.ragged_one_launch = True
            one = mod(x, pts, lengths=LENGTHS, npoints=NPOINTS1)
            assert torch.equal(new_xyz, one[0]) and torch.equal(out, one[1])
            gx, gout = mod(x, pts, geometry=g)
            assert torch.equal(new_xyz, gx) and torch.equal(out[valid], gout[valid]) and torch.isfinite(out).all()
            assert int((out[~valid] != 0).sum()) == 0
            for i, (ni, mi) in enumerate(zip(LENGTHS, NPOINTS1)):
                sx, so = _with_npoint(mod, mi, lambda: mod(x[i:i + 1, :ni].contiguous(), pts[i:i + 1, :ni].contiguous()))
                assert torch.equal(new_xyz[i:i + 1, :mi], sx)
                _close(out[i:i + 1, :mi], so, "%s cloud %d: ragged - single cloud" % (path, i))


# --------------------------------------------------------------------------------------------------------------- SA train
@pytest.mark.parametrize("pooling,mlp2", [("max", None), ("avg", None), ("weighted_avg", None), ("max_and_avg", [32])])
def test_sa_train(cuda, case, pooling, mlp2):
    """train(): batch statistics over the valid groups only, last_path "unfused_ragged". Zero against random finite padding
    (features and the padding rows of xyz): output and gradients bit-identical, padding rows exact zeros. Restatement (max
    pooling): the valid groups gathered from the oracle geometry, the module's own stack in float64 on (1, C, total, nsample),
    pooled; running statistics updated once."""
    import pointnet2_amd as P
    torch.manual_seed(74)
    cout = (mlp2 or WIDTHS)[-1]
    wout = torch.randn(B, NPOINT1, cout, device=cuda)
    valid = _valid(NPOINTS1, NPOINT1, cuda)
    was, was_cudnn = P.is_deterministic(), torch.backends.cudnn.deterministic
    P.set_deterministic(True)
    torch.backends.cudnn.deterministic = True
    res = {}
    try:
        for fill in ("zero", "random"):
            mod = _sa(cuda, pooling=pooling, mlp2=mlp2).train()
            ref = copy.deepcopy(mod).double()
            x = _dev(_padded(case["xyz"], fill, 3), cuda).requires_grad_(True)
            pts = _dev(_padded(case["feats"], fill, 4), cuda).requires_grad_(True)
            _, out, _ = mod(x, pts, lengths=LENGTHS, npoints=NPOINTS1)
            assert mod.last_path == "unfused_ragged"
            (out * wout).sum().backward()
            res[fill] = (out.detach(), x.grad, pts.grad, [p.grad for p in mod.parameters()], mod)
    finally:
        P.set_deterministic(was)
        torch.backends.cudnn.deterministic = was_cudnn
    a, b = res["zero"], res["random"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert len(a[3]) == len(b[3]) > 0 and all(torch.equal(u, v) for u, v in zip(a[3], b[3]))
    assert all(torch.isfinite(t).all() for t in (b[0], b[1], b[2]))
    assert float(b[1].abs().sum()) > 0 and float(b[2].abs().sum()) > 0
    assert int((b[0][~valid] != 0).sum()) == 0                               # padding centroid rows: exact zeros
    for i, ni in enumerate(LENGTHS):                                         # padding points: exactly zero gradients
        assert int((b[1][i, ni:] != 0).sum()) == 0 and int((b[2][i, ni:] != 0).sum()) == 0
    mod = b[4]
    for bn in mod.modules():
        if isinstance(bn, torch.nn.BatchNorm2d):
            assert int(bn.num_batches_tracked) == 1                          # updated once
    if pooling != "max":
        return
    widx = case["idx"][RADIUS]
    gxyz = np.stack([case["xyz"][i][widx[i]] for i in range(B)]) - case["new_xyz"][:, :, None, :]
    gfeat = np.stack([case["feats"][i][widx[i]] for i in range(B)])
    grouped = np.concatenate([gxyz, gfeat], axis=-1).reshape(B * NPOINT1, NSAMPLE, 3 + CFEAT)
    rows = np.flatnonzero(valid.cpu().numpy().reshape(-1))
    X = torch.from_numpy(grouped[rows]).double().to(cuda)                    # (total, nsample, C)
    y = ref.train().mlp(X.permute(2, 0, 1).unsqueeze(0)).max(dim=3)[0][0].t()    # (1, C, total, nsample) -> (total, C')
    _close(b[0][valid], y, "output against the float64 restatement")
    for ma, mb in zip(mod.modules(), ref.modules()):
        if isinstance(ma, torch.nn.BatchNorm2d):
            _close(ma.running_mean, mb.running_mean, "running_mean")
            _close(ma.running_var, mb.running_var, "running_var")


def test_msg_train(cuda, case):
    x = _dev(_padded(case["xyz"], "random", 8), cuda)
    valid = _valid(NPOINTS1, NPOINT1, cuda)
    outs = []
    for fill in ("zero", "random"):
        mod = _msg(cuda).train()
        pts = _dev(_padded(case["feats"], fill, 5), cuda).requires_grad_(True)
        new_xyz, out = mod(x, pts, lengths=LENGTHS, npoints=NPOINTS1)
        assert mod.last_path == "unfused_ragged"
        out.sum().backward()
        outs.append((out.detach(), pts.grad))
        assert int((out[~valid] != 0).sum()) == 0 and torch.isfinite(out).all()
        for i, ni in enumerate(LENGTHS):
            assert int((pts.grad[i, ni:] != 0).sum()) == 0
    assert torch.equal(outs[0][0], outs[1][0])
    with pytest.raises(ValueError):
        _sa(cuda, group_all=True).geometry(x, npoints=NPOINTS1)


# ---------------------------------------------------------------------------------------------------------- chained levels
def _net(cuda):
    from pointnet2_amd.pointnet_util import PointnetFPModule, PointnetSAModule
    torch.manual_seed(79)
    sa1 = PointnetSAModule(CFEAT, NPOINT1, 0.2, 16, [32, 32, 64])
    sa2 = PointnetSAModule(64, NPOINT2, 0.4, 16, [64, 64, 128])
    fp1 = PointnetFPModule(128 + 64, [64, 64])
    fp2 = PointnetFPModule(64 + CFEAT, [64, 32])
    return [m.to(cuda) for m in (sa1, sa2, fp1, fp2)]


def _run(net, x, pts, lengths=None, np1=None, np2=None):
    sa1, sa2, fp1, fp2 = net
    l1_xyz, l1_pts, _ = sa1(x, pts, lengths=lengths, npoints=np1)
    l2_xyz, l2_pts, _ = sa2(l1_xyz, l1_pts, lengths=np1, npoints=np2)
    up1 = fp1(l1_xyz, l2_xyz, l1_pts, l2_pts, lengths1=np1, lengths2=np2)
    up0 = fp2(x, l1_xyz, pts, up1, lengths1=lengths, lengths2=np1)
    return l1_pts, l2_pts, up1, up0


def test_chained_levels_eval(cuda, case):
    """SA1 -> SA2 -> FP -> FP with npoints handed on as the next level's lengths: NaN in every padding row of xyz, random finite
    padding in the features; every output finite, zero beyond the lengths, per cloud within the module bound of the four
    modules run on the single cloud with npoint = m_c at each SA level"""
    net = [m.eval() for m in _net(cuda)]
    x = _dev(_padded(case["xyz"], "nan"), cuda)
    pts = _dev(_padded(case["feats"], "random", 9), cuda)
    with torch.no_grad():
        outs = _run(net, x, pts, LENGTHS, NPOINTS1, NPOINTS2)
        for out, counts in zip(outs, (NPOINTS1, NPOINTS2, NPOINTS1, LENGTHS)):
            assert torch.isfinite(out).all()
            assert int((out[~_valid(counts, out.shape[1], cuda)] != 0).sum()) == 0
        for i, (ni, m1, m2) in enumerate(zip(LENGTHS, NPOINTS1, NPOINTS2)):
            sa1, sa2 = net[0], net[1]
            sx, sp = x[i:i + 1, :ni].contiguous(), pts[i:i + 1, :ni].contiguous()
            was = sa1.npoint, sa2.npoint
            sa1.npoint, sa2.npoint = m1, m2
            try:
                single = _run(net, sx, sp)
            finally:
                sa1.npoint, sa2.npoint = was
            for name, out, want, c in zip(("l1", "l2", "up1", "up0"), outs, single, (m1, m2, m1, ni)):
                _close(out[i:i + 1, :c], want, "cloud %d %s: ragged - single cloud" % (i, name))


@pytest.mark.parametrize("fused_last", [False, True])
def test_chained_levels_train(cuda, case, fused_last):
    """train(): the default routes, then fused_ragged_train on the last FP level. Finite outputs; zero against random finite
    padding bit-identical; the gradient of points2 exactly zero on the known side's padding rows (every FP level)."""
    import pointnet2_amd as P
    was, was_cudnn = P.is_deterministic(), torch.backends.cudnn.deterministic
    P.set_deterministic(True)
    torch.backends.cudnn.deterministic = True
    res = []
    try:
        for fill in ("zero", "random"):
            net = [m.train() for m in _net(cuda)]
            net[3].fused_ragged_train = fused_last
            x = _dev(_padded(case["xyz"], fill, 3), cuda)
            pts = _dev(_padded(case["feats"], fill, 4), cuda)
            l1_pts, l2_pts, up1, up0 = _run(net, x, pts, LENGTHS, NPOINTS1, NPOINTS2)
            print("paths:", [m.last_path for m in net])
            l2_pts.retain_grad(); up1.retain_grad()
            up0.sum().backward()
            res.append((up0.detach(), up1.detach(), l2_pts.grad, up1.grad))
    finally:
        P.set_deterministic(was)
        torch.backends.cudnn.deterministic = was_cudnn
    a, b = res
    assert all(torch.isfinite(t).all() for t in b)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert int((b[2][~_valid(NPOINTS2, NPOINT2, cuda)] != 0).sum()) == 0     # points2 of the first FP level: SA2's padding rows
    assert int((b[3][~_valid(NPOINTS1, NPOINT1, cuda)] != 0).sum()) == 0     # points2 of the last FP level: level 1's padding rows
    assert float(b[2].abs().sum()) > 0 and float(b[3].abs().sum()) > 0


def test_fp_known_side_only(cuda, case):
    """lengths2 without lengths1: a dense unknown side; the dense routes behind the two-sided three_nn"""
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import PointnetFPModule
    torch.manual_seed(76)
    mod = PointnetFPModule(32 + CFEAT, [64, 32]).to(cuda).eval()
    x1, p1 = _dev(case["xyz"], cuda), _dev(case["feats"], cuda)
    x2 = _dev(_padded(case["new_xyz"], "nan", lengths=NPOINTS1), cuda)
    p2 = _dev(_padded(np.random.default_rng(77).standard_normal((B, NPOINT1, 32)).astype(np.float32), "random", 2, lengths=NPOINTS1), cuda)
    with torch.no_grad():
        out = mod(x1, x2, p1, p2, lengths2=NPOINTS1)
        assert torch.isfinite(out).all()
        for i, mi in enumerate(NPOINTS1):
            want = mod(x1[i:i + 1], x2[i:i + 1, :mi].contiguous(), p1[i:i + 1], p2[i:i + 1, :mi].contiguous())
            _close(out[i:i + 1], want, "cloud %d: ragged known side - single cloud" % i)
