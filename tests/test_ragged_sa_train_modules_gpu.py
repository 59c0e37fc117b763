"""The SA modules' two opt-in flags for ragged training on the GPU (pointnet_util.py): fused_ragged_train -- train() with npoints=
on the fused node with a row mask (train_mlp.sa_mlp_train(..., counts=); last_path "fused_train_ragged") instead of the
compacting layer-by-layer path ("unfused_ragged") -- and ragged_group_all -- a group_all level that accepts lengths=.

Shapes: b = 4 clouds padded to n = 256 with lengths (256, 200, 40, 130); npoint 32 with npoints (32, 17, 1, 24), nsample 16
(and 32 for the second MSG radius), 8 feature channels, stack 32 -> 32 -> 64; the group_all level behind it takes the 32 rows of
64 channels with lengths = npoints. Padding rows hold NaN. Bounds: 1e-5 of each tensor's scale (the nodes' own), and for eval the
bound of tests/test_ragged_modules_gpu.py (1e-5 of the output scale, at least 1e-5)."""
import copy

import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

B, N, LENGTHS = 4, 256, [256, 200, 40, 130]
NPOINT, NPOINTS = 32, [32, 17, 1, 24]
RADIUS, NSAMPLE, WIDTHS, CFEAT = 0.3, 16, [32, 32, 64], 8
MSG_RADII, MSG_NSAMPLES = [0.3, 0.5], [16, 32]
ALL_WIDTHS = [64, 128]
TOL = 1e-5


def _bound(want):
    """the bound of tests/test_ragged_modules_gpu.py: 1e-5 of the output scale"""
    return 1e-5 * max(1.0, float(want.abs().max()))


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-30, float(b.abs().max())))


def _i32(v, cuda):
    return torch.tensor(v, dtype=torch.int32, device=cuda)


def _inputs(cuda, cfeat=CFEAT, n=N, lengths=LENGTHS, seed=91):
    """clouds and features with NaN at and beyond the lengths"""
    xyz = torch.from_numpy(S.sphere_clouds(B, n, seed)).to(cuda)
    pts = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal((B, n, cfeat)).astype(np.float32)).to(cuda)
    for i, k in enumerate(lengths):
        xyz[i, k:], pts[i, k:] = float("nan"), float("nan")
    return xyz, pts


def _sa(cuda, **kw):
    from pointnet2_amd.pointnet_util import PointnetSAModule
    torch.manual_seed(93)
    return PointnetSAModule(CFEAT, NPOINT, RADIUS, NSAMPLE, WIDTHS, **kw).to(cuda)


def _msg(cuda):
    from pointnet2_amd.pointnet_util import PointnetSAModuleMSG
    torch.manual_seed(95)
    return PointnetSAModuleMSG(CFEAT, NPOINT, MSG_RADII, MSG_NSAMPLES, [WIDTHS, WIDTHS]).to(cuda)


def _group_all(cuda, c=WIDTHS[-1], **kw):
    from pointnet2_amd.pointnet_util import PointnetSAModule
    torch.manual_seed(97)
    return PointnetSAModule(c, None, None, None, ALL_WIDTHS, group_all=True, **kw).to(cuda)


def _train_both(mod, call, gout, want_path):
    """the module with the flag off ("unfused_ragged") and on (want_path) from the same weights -> the two result lists:
    output, the features' gradient, every parameter's gradient, every buffer; and which entries are conv biases"""
    res = []
    for flag in (False, True):
        cur = copy.deepcopy(mod).train()
        cur.fused_ragged_train = flag
        out, pts = call(cur)
        assert cur.last_path == (want_path if flag else "unfused_ragged"), cur.last_path
        (out * gout).sum().backward()
        res.append([out.detach(), pts.grad] + [p.grad for p in cur.parameters()] + [t.detach().clone() for t in cur.buffers()])
    conv_bias = {id(m.bias) for m in mod.modules() if isinstance(m, torch.nn.Conv2d) and m.bias is not None}
    res.append([False, False] + [id(p) in conv_bias for p in mod.parameters()] + [False] * len(list(mod.buffers())))
    return res


def _compare(res):
    """1e-5 of each tensor's scale. A conv bias in front of a batch norm has the gradient ZERO (the normalisation removes any
    per-channel constant): the node returns exact zeros, autograd's layer-by-layer sum of dz is rounding noise around zero --
    both are held to 1e-5 of the scale of the per-channel sum beside it, the gradient of the batch norm's own bias (two
    entries on)."""
    off, on, is_conv_bias = res
    assert len(off) == len(on) == len(is_conv_bias)
    errs = {}
    for i, (u, v) in enumerate(zip(on, off)):
        assert (u is None) == (v is None), i
        if u is None:
            continue
        assert bool(torch.isfinite(u.float()).all()), i
        if is_conv_bias[i]:
            scale = float(off[i + 2].double().abs().max())
            assert float(u.abs().max()) == 0.0 and float(v.abs().max()) <= TOL * scale, i
            continue
        errs[i] = _rel(u, v)
    print(" ".join("%d=%.1e" % kv for kv in errs.items()), flush=True)
    assert max(errs.values()) <= TOL, errs


def test_sa_module_takes_the_masked_node_and_matches_its_compacting_path(cuda):
    xyz, feats = _inputs(cuda)
    mod = _sa(cuda)
    lens, cnts = _i32(LENGTHS, cuda), _i32(NPOINTS, cuda)
    g = mod.geometry(xyz, lengths=lens, npoints=cnts)
    gout = torch.randn(B, NPOINT, WIDTHS[-1], device=cuda)
    gout[2, 1:] = float("nan")                                         # a padding centroid's output gradient may hold anything

    def call(cur):
        pts = feats.clone().requires_grad_(True)
        _, out, _ = cur(xyz, pts, geometry=g, lengths=lens, npoints=cnts)
        return out, pts
    res = _train_both(mod, call, torch.nan_to_num(gout, nan=0.0), "fused_train_ragged")
    _compare(res)
    # NaN on a padding group's output gradient: the node is indifferent, bit for bit (the compacting path never sees those rows)
    cur = copy.deepcopy(mod).train()
    cur.fused_ragged_train = True
    out, pts = call(cur)
    (out * torch.nan_to_num(gout, nan=0.0)).sum().backward()
    cur2 = copy.deepcopy(mod).train()
    cur2.fused_ragged_train = True
    out2, pts2 = call(cur2)
    (out2 * torch.ones_like(gout)).backward(gout)                      # the NaN rows go in as they are
    assert torch.equal(out, out2) and bool(torch.isfinite(pts2.grad).all())
    valid = torch.arange(NPOINT, device=cuda).view(1, -1) < cnts.view(-1, 1)
    assert int((out[~valid] != 0).sum()) == 0
    for i, k in enumerate(LENGTHS):
        assert int((pts2.grad[i, k:] != 0).sum()) == 0
    for p, q in zip(cur.parameters(), cur2.parameters()):
        assert torch.equal(p.grad, q.grad)                             # (fixed summation orders: the same bits)


def test_sa_module_keeps_the_compacting_path_where_the_node_is_not_offered(cuda):
    xyz, feats = _inputs(cuda)
    lens, cnts = _i32(LENGTHS, cuda), _i32(NPOINTS, cuda)
    for kw in (dict(pooling="avg"), dict(mlp2=[32])):
        mod = _sa(cuda, **kw).train()
        mod.fused_ragged_train = True
        mod(xyz, feats, lengths=lens, npoints=cnts)
        assert mod.last_path == "unfused_ragged", kw
    mod = _sa(cuda).train()                                            # the default: flag off
    assert mod.fused_ragged_train is False and mod.ragged_group_all is False and _msg(cuda).fused_ragged_train is False
    mod(xyz, feats, lengths=lens, npoints=cnts)
    assert mod.last_path == "unfused_ragged"


def test_msg_module_takes_one_masked_node_per_scale(cuda):
    xyz, feats = _inputs(cuda)
    mod = _msg(cuda)
    lens, cnts = _i32(LENGTHS, cuda), _i32(NPOINTS, cuda)
    g = mod.geometry(xyz, lengths=lens, npoints=cnts)
    gout = torch.randn(B, NPOINT, 2 * WIDTHS[-1], device=cuda)

    def call(cur):
        pts = feats.clone().requires_grad_(True)
        _, out = cur(xyz, pts, geometry=g, lengths=lens, npoints=cnts)
        return out, pts
    _compare(_train_both(mod, call, gout, "fused_train_ragged"))


def test_group_all_eval_equals_the_module_on_each_slice(cuda):
    xyz, feats = _inputs(cuda, cfeat=WIDTHS[-1], n=NPOINT, lengths=NPOINTS)
    lens = _i32(NPOINTS, cuda)
    for pooling in ("max", "avg", "weighted_avg", "max_and_avg"):
        mod = _group_all(cuda, pooling=pooling).eval()
        with pytest.raises(ValueError):
            mod(xyz, feats, lengths=lens)                              # the default still refuses
        mod.ragged_group_all = True
        with torch.no_grad():
            new_xyz, got, _ = mod(xyz, feats, lengths=lens)
            assert mod.last_path == "unfused" and tuple(new_xyz.shape) == (B, 1, 3) and got.shape[:2] == (B, 1)
            for i, k in enumerate(NPOINTS):
                _, want, _ = mod(xyz[i:i + 1, :k].contiguous(), feats[i:i + 1, :k].contiguous())
                err = float((got[i:i + 1] - want).abs().max())
                assert err <= _bound(want), (pooling, i, err)


def test_group_all_train_node_matches_the_compacting_fallback(cuda):
    xyz, feats = _inputs(cuda, cfeat=WIDTHS[-1], n=NPOINT, lengths=NPOINTS)
    lens = _i32(NPOINTS, cuda)
    mod = _group_all(cuda)
    mod.ragged_group_all = True
    gout = torch.randn(B, 1, ALL_WIDTHS[-1], device=cuda)

    def call(cur):
        pts = feats.clone().requires_grad_(True)
        _, out, _ = cur(xyz, pts, lengths=lens)
        assert tuple(out.shape) == (B, 1, ALL_WIDTHS[-1])
        return out, pts
    res = _train_both(mod, call, gout, "fused_train_ragged")
    _compare(res)
    for i, k in enumerate(NPOINTS):                                    # rows beyond a length: exactly zero gradients, both ways
        assert int((res[0][1][i, k:] != 0).sum()) == 0 and int((res[1][1][i, k:] != 0).sum()) == 0
    # every pooling mode has the compacting fallback; only max has the node
    for pooling in ("avg", "weighted_avg", "max_and_avg"):
        cur = _group_all(cuda, pooling=pooling).train()
        cur.ragged_group_all = cur.fused_ragged_train = True
        _, out, _ = cur(xyz, feats, lengths=lens)
        assert cur.last_path == "unfused_ragged" and bool(torch.isfinite(out).all())


def test_two_level_chain_runs_without_a_host_synchronisation(cuda):
    """SA with lengths and npoints, then group_all with lengths = npoints, both flags on: forward + backward enqueue only."""
    xyz, feats = _inputs(cuda)
    lens, cnts = _i32(LENGTHS, cuda), _i32(NPOINTS, cuda)
    sa, top = _sa(cuda).train(), _group_all(cuda).train()
    sa.fused_ragged_train = top.fused_ragged_train = top.ragged_group_all = True
    gout = torch.randn(B, 1, ALL_WIDTHS[-1], device=cuda)

    def step():
        pts = feats.clone().requires_grad_(True)
        new_xyz, mid, _ = sa(xyz, pts, lengths=lens, npoints=cnts)
        _, out, _ = top(new_xyz, mid, lengths=cnts)
        assert sa.last_path == "fused_train_ragged" and top.last_path == "fused_train_ragged"
        (out * gout).sum().backward()
        return out, pts.grad

    step()                                                              # warm: code objects loaded, workspaces sized
    torch.cuda.synchronize()
    for p in list(sa.parameters()) + list(top.parameters()):
        p.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, gpts = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gpts).all())
    assert float(out.abs().sum()) > 0 and float(gpts.abs().sum()) > 0
    for i, k in enumerate(LENGTHS):
        assert int((gpts[i, k:] != 0).sum()) == 0
    # the same chain with the flags off (compacting, synchronising) from the same weights agrees at the nodes' bound
    sa2, top2 = copy.deepcopy(sa), copy.deepcopy(top)
    sa2.fused_ragged_train = top2.fused_ragged_train = False
    for p in list(sa2.parameters()) + list(top2.parameters()):
        p.grad = None
    sa.zero_grad(), top.zero_grad()
    out1, g1 = step()
    pts = feats.clone().requires_grad_(True)
    new_xyz, mid, _ = sa2(xyz, pts, lengths=lens, npoints=cnts)
    _, out2, _ = top2(new_xyz, mid, lengths=cnts)
    assert sa2.last_path == "unfused_ragged" and top2.last_path == "unfused_ragged"
    (out2 * gout).sum().backward()
    assert _rel(out1, out2) <= TOL and _rel(g1, pts.grad) <= TOL, (_rel(out1, out2), _rel(g1, pts.grad))
