"""CPU tests of the training node on the GROUPED rows of a ragged batch (pn2_mlp_train_*_group_ragged, include/pn2ops.h,
csrc/train_mlp_ragged_group.hip): declared and exported, arguments refused before anything is launched, the support and workspace
queries and their Python mirror, the combinations sa_mlp_train(counts=) refuses, and the modules' two opt-in flags -- off by
default, and on CPU tensors the fallbacks."""
import ctypes

import pytest

from test_abi import _declared

NEW = ("pn2_mlp_train_group_ragged_supported", "pn2_mlp_train_ws_bytes_group_ragged", "pn2_mlp_train_forward_group_ragged",
       "pn2_mlp_train_backward_group_ragged", "pn2_mlp_train_group_ragged_plan")
PN2_E_NULL, PN2_E_ARG = -1, -3
FAKE = 0x1000                                                  # never dereferenced: every call below fails its checks first
# the GPU cases (a) and (d): b, n, m, nsample, cfeat, has_idx; the stack
DIMS_A, WIDTHS_A = (4, 256, 32, 16, 8, 1), (11, 32, 32, 64)
DIMS_D, WIDTHS_D = (4, 128, 1, 128, 64, 0), (67, 128, 256)


def _lib():
    from pointnet2_amd import _C
    return _C.lib()


def _w(*v):
    return (ctypes.c_int * len(v))(*v)


def _rows(d):
    return d[0] * d[2] * d[3]


def _layers(*widths):
    from pointnet2_amd.train_mlp import BnLayer
    arr = (BnLayer * (len(widths) - 1))()
    for l in range(len(widths) - 1):
        L = arr[l]
        L.cin, L.cout = widths[l], widths[l + 1]
        L.weight = L.gamma = L.beta = L.save = L.z = L.grad_weight = L.grad_gamma = L.grad_beta = FAKE
        L.w_stride_k, L.w_stride_n = 1, widths[l]
        L.eps = 1e-5
    return arr


def _group(d, points=FAKE, idx=FAKE):
    from pointnet2_amd.train_mlp import GroupSrc
    g = GroupSrc()
    g.b, g.n, g.m, g.nsample, g.cfeat, g.xyz_first = d[0], d[1], d[2], d[3], d[4], 1
    g.xyz, g.new_xyz = FAKE, FAKE if d[5] else None
    g.points = points if d[4] else None
    g.idx = idx if d[5] else None
    return g


def _fwd(lib, d, widths, rows=None, group="dims", pool_rows=None, counts=FAKE, out=FAKE, argsel=FAKE, mask=FAKE, ws=FAKE, layers="w"):
    grp = ctypes.byref(_group(d)) if group == "dims" else group
    return lib.pn2_mlp_train_forward_group_ragged(_rows(d) if rows is None else rows, len(widths) - 1,
                                                  _layers(*widths) if layers == "w" else layers, grp,
                                                  d[3] if pool_rows is None else pool_rows, counts, out, argsel, mask, ws, None, None)


def _bwd(lib, d, widths, rows=None, group="dims", pool_rows=None, counts=FAKE, out=FAKE, argsel=FAKE, gout=FAKE, grows=FAKE, mask=FAKE,
         ws=FAKE, layers="w"):
    grp = ctypes.byref(_group(d)) if group == "dims" else group
    return lib.pn2_mlp_train_backward_group_ragged(_rows(d) if rows is None else rows, len(widths) - 1,
                                                   _layers(*widths) if layers == "w" else layers, grp,
                                                   d[3] if pool_rows is None else pool_rows, counts, out, argsel, gout, grows, 1, mask,
                                                   ws, None, None)


def test_entries_declared_and_exported():
    from pointnet2_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    names = _declared()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _C.EXPORTED, n


def test_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib()
    for d, widths in ((DIMS_A, WIDTHS_A), (DIMS_D, WIDTHS_D)):
        for call in (_fwd, _bwd):
            assert call(lib, d, widths, counts=None) == PN2_E_NULL
            assert call(lib, d, widths, mask=None) == PN2_E_NULL
            assert call(lib, d, widths, group=None) == PN2_E_NULL
            assert call(lib, d, widths, layers=None) == PN2_E_NULL
            assert call(lib, d, widths, rows=_rows(d) + 32) == PN2_E_ARG          # the dims do not describe the rows
            assert call(lib, d, widths, pool_rows=2 * d[3]) == PN2_E_ARG          # the pool group is not the level's
            assert call(lib, d, widths, pool_rows=0) == PN2_E_ARG
            assert call(lib, d, (widths[0] + 1,) + widths[1:]) == PN2_E_ARG       # cin_1 != 3 + cfeat
            assert call(lib, d, widths[:-1] + (widths[-1] + 2,)) == PN2_E_ARG     # a cout that is no multiple of 4
            assert call(lib, d, widths, ws=None) == PN2_E_NULL                     # the dense entries' checks behind them
            assert call(lib, d, widths, out=None) == PN2_E_NULL
            assert call(lib, d, widths, argsel=None) == PN2_E_NULL
        assert _bwd(lib, d, widths, gout=None) == PN2_E_NULL
    # groups of 24 rows: the dense node takes 16 or a multiple of 32; 40 rows in all: not a multiple of 32
    assert _fwd(lib, (4, 256, 32, 24, 8, 1), WIDTHS_A) == PN2_E_ARG
    assert _fwd(lib, (1, 40, 1, 40, 8, 0), WIDTHS_A) == PN2_E_ARG
    # group_all means m == 1 and nsample == n
    assert _fwd(lib, (4, 256, 1, 128, 64, 0), WIDTHS_D) == PN2_E_ARG


def test_supported_and_workspace_are_consistent():
    lib = _lib()
    good = [(DIMS_A, WIDTHS_A), (DIMS_D, WIDTHS_D), ((3, 256, 16, 32, 0, 1), (3, 32, 64)), (DIMS_A, (11, 32)),
            ((4, 512, 128, 32, 128, 1), (131, 256))]
    bad = [((4, 256, 32, 24, 8, 1), WIDTHS_A), ((1, 40, 1, 40, 8, 0), WIDTHS_A), ((4, 256, 1, 128, 64, 0), WIDTHS_D),
           (DIMS_A, (12, 32, 32, 64)), (DIMS_A, (11, 32, 30)), ((0, 256, 32, 16, 8, 1), WIDTHS_A), ((4, 256, 32, 16, -1, 1), WIDTHS_A)]
    for cases, want in ((good, 1), (bad, 0)):
        for d, widths in cases:
            nl, rows = len(widths) - 1, _rows(d)
            assert lib.pn2_mlp_train_group_ragged_supported(rows, nl, _w(*widths), d[3], _w(*d)) == want, (d, widths)
            for backward in (0, 1):
                nbytes = lib.pn2_mlp_train_ws_bytes_group_ragged(rows, nl, _w(*widths), d[3], backward, _w(*d), None)
                assert (nbytes > 0) if want else (nbytes == -1), (d, widths, backward)
            count = lib.pn2_mlp_train_group_ragged_plan(rows, nl, _w(*widths), d[3], _w(*d), None, None, 0)
            assert (count == 2 * nl + (nl if d[4] else nl - 1)) if want else (count == PN2_E_ARG), (d, widths, count)
    assert lib.pn2_mlp_train_group_ragged_supported(_rows(DIMS_A), 3, None, 16, _w(*DIMS_A)) == 0
    assert lib.pn2_mlp_train_group_ragged_supported(_rows(DIMS_A), 3, _w(*WIDTHS_A), 16, None) == 0
    assert lib.pn2_mlp_train_group_ragged_supported(_rows(DIMS_A), 9, _w(*([11] + [32] * 9)), 16, _w(*DIMS_A)) == 0
    assert lib.pn2_mlp_train_group_ragged_plan(_rows(DIMS_A), 3, None, 16, _w(*DIMS_A), None, None, 0) == PN2_E_NULL


def test_python_supported_mirrors_the_c_query():
    from pointnet2_amd import train_mlp
    from pointnet2_amd.pointnet_util import _SharedMLP
    lib = _lib()
    for d, widths in ((DIMS_A, WIDTHS_A), (DIMS_D, WIDTHS_D), ((4, 256, 32, 24, 8, 1), WIDTHS_A), ((1, 40, 1, 40, 8, 0), WIDTHS_A)):
        net = _SharedMLP(widths[0], list(widths[1:])).train().net
        want = lib.pn2_mlp_train_group_ragged_supported(_rows(d), len(widths) - 1, _w(*widths), d[3], _w(*d)) == 1
        assert train_mlp.group_ragged_supported(net, d[0], d[1], d[2], d[3], d[4], bool(d[5])) is want, (d, widths)
    net = _SharedMLP(11, [32, 64])
    assert not train_mlp.group_ragged_supported(net.eval().net, *DIMS_A[:5])          # batch statistics only
    assert not train_mlp.group_ragged_supported(_SharedMLP(11, [32, 64], bn=False).train().net, *DIMS_A[:5])


def test_sa_mlp_train_refuses_counts_with_the_excluded_combinations():
    import torch
    from pointnet2_amd import train_mlp
    from pointnet2_amd.pointnet_util import _SharedMLP
    net = _SharedMLP(11, [32, 64]).train().net
    xyz, pts = torch.zeros(4, 256, 3), torch.zeros(4, 256, 8)
    new_xyz, idx = torch.zeros(4, 32, 3), torch.zeros(4, 32, 16, dtype=torch.int32)
    counts = torch.tensor([32, 17, 1, 24], dtype=torch.int32)
    for kw, word in ((dict(pooling="avg"), "pooling"), (dict(pooling="max_and_avg"), "pooling"), (dict(xyz_grad=True), "xyz_grad"),
                     (dict(frozen=True), "frozen")):
        with pytest.raises(ValueError, match=word):
            train_mlp.sa_mlp_train(net, xyz, new_xyz, pts, idx, counts=counts, **kw)


def test_module_flags_default_off_and_group_all_still_refuses_lengths():
    import torch
    from pointnet2_amd.pointnet_util import PointnetSAModule, PointnetSAModuleMSG
    sa = PointnetSAModule(8, 32, 0.2, 16, [32, 64])
    msg = PointnetSAModuleMSG(8, 32, [0.1, 0.2], [16, 32], [[32, 64], [32, 64]])
    ga = PointnetSAModule(8, None, None, None, [32, 64], group_all=True)
    assert sa.fused_ragged_train is False and msg.fused_ragged_train is False and ga.fused_ragged_train is False
    assert sa.ragged_group_all is False and ga.ragged_group_all is False
    xyz, pts, lens = torch.rand(2, 32, 3), torch.randn(2, 32, 8), torch.tensor([32, 5], dtype=torch.int32)
    with pytest.raises(ValueError, match="group_all with lengths: the group would contain the padding rows"):
        ga(xyz, pts, lengths=lens)
    with pytest.raises(ValueError, match="group_all with lengths: the group would contain the padding rows"):
        ga.geometry(xyz, lengths=lens)
    ga.ragged_group_all = True
    assert ga.geometry(xyz, lengths=lens) is None
    for call in (lambda: ga(xyz, pts, npoints=lens), lambda: ga.geometry(xyz, npoints=lens), lambda: ga(xyz, pts, lengths=lens, npoints=lens)):
        with pytest.raises(ValueError, match="group_all with lengths"):                 # npoints stays refused
            call()


@pytest.mark.parametrize("pooling", ["max", "avg", "weighted_avg", "max_and_avg"])
def test_ragged_group_all_on_cpu_tensors_takes_the_fallbacks(pooling):
    """CPU tensors with both flags on: eval() equals the module on each cloud's slice; train() takes the compacting fallback,
    whose result is the stack in train mode on the concatenated valid rows, pooled per cloud. NaN on the padding rows."""
    import copy
    import torch
    from pointnet2_amd.pointnet_util import PointnetSAModule
    torch.manual_seed(3)
    b, n, c = 3, 32, 8
    lens = [32, 7, 1]
    mod = PointnetSAModule(c, None, None, None, [16, 32], group_all=True, pooling=pooling)
    mod.ragged_group_all = mod.fused_ragged_train = True
    xyz, pts = torch.rand(b, n, 3), torch.randn(b, n, c)
    for i, k in enumerate(lens):
        xyz[i, k:], pts[i, k:] = float("nan"), float("nan")
    lengths = torch.tensor(lens, dtype=torch.int32)
    mod.eval()
    _, got, _ = mod(xyz, pts, lengths=lengths)
    assert mod.last_path == "unfused" and tuple(got.shape) == (b, 1, mod.mlp.c_out * (2 if pooling == "max_and_avg" else 1))
    for i, k in enumerate(lens):
        _, want, _ = mod(xyz[i:i + 1, :k], pts[i:i + 1, :k])
        assert torch.allclose(got[i:i + 1], want, rtol=1e-5, atol=1e-6), (pooling, i)
    # train: against the stack on the concatenated valid rows
    mod.train()
    ref = copy.deepcopy(mod)
    p = pts.clone().requires_grad_(True)
    _, got, _ = mod(xyz, p, lengths=lengths)
    assert mod.last_path == "unfused_ragged"
    got.square().sum().backward()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(p.grad).all())
    for i, k in enumerate(lens):
        assert float(p.grad[i, k:].abs().max() if k < n else 0.0) == 0.0
    rows = torch.cat([torch.cat([xyz[i, :k], pts[i, :k]], dim=1) for i, k in enumerate(lens)], dim=0)      # (total, 3 + c)
    y = ref.mlp(rows.t().reshape(1, 3 + c, -1, 1))[0, :, :, 0].t()                                       # (total, C')
    start, want = 0, []
    for i, k in enumerate(lens):
        h = y[start:start + k]
        w = torch.exp(-5 * xyz[i, :k].norm(dim=1, keepdim=True))
        pooled = {"max": lambda: h.max(dim=0)[0], "avg": lambda: h.mean(dim=0), "weighted_avg": lambda: (h * w / w.sum()).sum(dim=0),
                  "max_and_avg": lambda: torch.cat([h.mean(dim=0), h.max(dim=0)[0]])}[pooling]()
        want.append(pooled)
        start += k
    assert torch.allclose(got[:, 0], torch.stack(want), rtol=1e-5, atol=1e-6)
    for u, v in zip(mod.buffers(), ref.buffers()):
        assert torch.allclose(u.float(), v.float(), rtol=1e-6, atol=1e-7)                    # running statistics of the valid rows
