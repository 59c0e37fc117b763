"""CPU tests of the coordinate-gradient entries of the SA training node (pn2_mlp_train_*_xyz, include/pn2ops.h): declared and
exported, arguments refused before anything is launched, the support query against pn2_mlp_train_pool_supported, the workspace."""
import ctypes

from test_abi import _declared

NEW = ("pn2_mlp_train_xyz_supported", "pn2_mlp_train_ws_bytes_xyz", "pn2_mlp_train_backward_xyz")
PN2_E_NULL, PN2_E_ARG = -1, -3
FAKE = 0x1000                                                  # never dereferenced: every call below fails its checks first


def _lib():
    from pointnet2_amd import _C
    return _C.lib()


def _w(*widths):
    return (ctypes.c_int * len(widths))(*widths)


def _gd(*v):
    return (ctypes.c_int * 6)(*v)


def _layers(*widths):
    from pointnet2_amd.train_mlp import BnLayer
    arr = (BnLayer * (len(widths) - 1))()
    for l in range(len(widths) - 1):
        L = arr[l]
        L.cin, L.cout = widths[l], widths[l + 1]
        L.weight = L.gamma = L.beta = L.save = L.z = L.grad_weight = L.grad_gamma = L.grad_beta = FAKE
        L.w_stride_k, L.w_stride_n = 1, widths[l]
    return arr


def _group(b=2, n=256, m=64, ns=32, centroid=True):
    from pointnet2_amd.train_mlp import GroupSrc
    g = GroupSrc()
    g.b, g.n, g.m, g.nsample, g.cfeat, g.xyz_first = b, n, m, ns, 0, 1
    g.xyz, g.idx, g.new_xyz, g.points = FAKE, FAKE, (FAKE if centroid else None), None
    return g


def _bwd(lib, group, pooling, grad_xyz, grad_new_xyz, rows=2 * 64 * 32):
    f = ctypes.c_void_p(FAKE)
    return lib.pn2_mlp_train_backward_xyz(rows, 3, _layers(3, 32, 32, 64), group, 32, pooling, f, f, f, None, f, None, None,
                                          grad_xyz, grad_new_xyz, 0, f, None, None)


def test_xyz_entries_declared_and_exported():
    from pointnet2_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    names = _declared()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _C.EXPORTED, n


def test_xyz_backward_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    f = ctypes.c_void_p(FAKE)
    g = _group()
    assert _bwd(lib, ctypes.byref(g), 2, f, f) == PN2_E_ARG                # weighted_avg: no coordinate gradient
    for bad in (-1, 4):
        assert _bwd(lib, ctypes.byref(g), bad, f, f) == PN2_E_ARG
    for pooling in (0, 1, 3):
        assert _bwd(lib, None, pooling, f, f) == PN2_E_NULL                # no group
        assert _bwd(lib, ctypes.byref(g), pooling, f, None) == PN2_E_NULL  # a centroid without a place for its gradient
        assert _bwd(lib, ctypes.byref(g), pooling, None, f) == PN2_E_NULL  # the centroid's gradient alone
        nc = _group(centroid=False)
        assert _bwd(lib, ctypes.byref(nc), pooling, f, f) == PN2_E_ARG     # a gradient for a centroid that is not there
    # both new pointers NULL: pn2_mlp_train_backward_pool's own checks
    assert _bwd(lib, None, 1, None, None) == PN2_E_NULL
    assert _bwd(lib, None, 7, None, None) == PN2_E_ARG


def test_xyz_supported_follows_pool_supported():
    lib = _lib()
    shapes = [(4 * 256 * 32, (3, 64, 64, 128), 32, (4, 1024, 256, 32, 0, 1)),
              (4 * 256 * 16, (6, 32, 32, 64), 16, (4, 1024, 256, 16, 3, 1)),
              (4 * 256 * 64, (131, 128, 256), 64, (4, 512, 256, 64, 128, 1)),
              (4 * 128, (259, 256, 512, 1024), 128, (4, 128, 1, 128, 256, 0)),          # group_all
              (4 * 256 * 24, (3, 64, 64, 128), 24, (4, 1024, 256, 24, 0, 1)),           # nsample 24
              (4 * 256 * 32, (3, 64, 66), 32, (4, 1024, 256, 32, 0, 1)),                # width % 4
              (4 * 256 * 32 + 32, (3, 32, 64), 64, (4, 1024, 256, 32, 0, 1))]           # rows % nsample
    seen = set()
    for rows, widths, ns, gd in shapes:
        for mode in (0, 1, 3):
            want = lib.pn2_mlp_train_pool_supported(rows, len(widths) - 1, _w(*widths), ns, mode)
            assert lib.pn2_mlp_train_xyz_supported(rows, len(widths) - 1, _w(*widths), ns, mode, _gd(*gd)) == want
            assert lib.pn2_mlp_train_xyz_supported(rows, len(widths) - 1, _w(*widths), ns, mode, None) == want
            seen.add(want)
        assert lib.pn2_mlp_train_xyz_supported(rows, len(widths) - 1, _w(*widths), ns, 2, _gd(*gd)) == 0
    assert seen == {0, 1}
    rows, widths = 4 * 256 * 32, (3, 64, 64, 128)
    assert lib.pn2_mlp_train_xyz_supported(rows, 3, _w(*widths), 32, 0, _gd(4, 1024, 256, 32, 3, 1)) == 0    # widths[0] != 3 + cfeat
    assert lib.pn2_mlp_train_xyz_supported(rows, 3, _w(*widths), 32, 0, _gd(2, 1024, 256, 32, 0, 1)) == 0    # b m ns != rows


def test_xyz_workspace_holds_the_pool_workspace():
    lib = _lib()
    for rows, widths, ns, gd in ((4 * 256 * 32, (3, 64, 64, 128), 32, (4, 1024, 256, 32, 0, 1)),
                                 (4 * 256 * 32, (67, 64, 64, 128), 32, (4, 1024, 256, 32, 64, 1)),
                                 (4 * 128, (259, 256, 512, 1024), 128, (4, 128, 1, 128, 256, 0))):
        for mode in (0, 1, 3):
            base = lib.pn2_mlp_train_ws_bytes_pool(rows, len(widths) - 1, _w(*widths), ns, mode, 1, _gd(*gd), None)
            got = lib.pn2_mlp_train_ws_bytes_xyz(rows, len(widths) - 1, _w(*widths), ns, mode, _gd(*gd), None)
            assert base > 0 and got >= base
            if gd[5]:
                assert got >= base + rows * 12                 # the rows' g (rows, 3)
        assert lib.pn2_mlp_train_ws_bytes_xyz(rows, len(widths) - 1, _w(*widths), ns, 2, _gd(*gd), None) < 0
        assert lib.pn2_mlp_train_ws_bytes_xyz(rows, len(widths) - 1, _w(*widths), ns, 0, None, None) < 0


def test_python_xyz_grad_supported():
    from pointnet2_amd import train_mlp
    from pointnet2_amd.pointnet_util import PointnetSAModule, PointnetSAModuleMSG, _SharedMLP
    net = _SharedMLP(3, [32, 32, 64]).train().net
    for mode in ("max", "avg", "max_and_avg"):
        assert train_mlp.xyz_grad_supported(net, 2 * 64 * 32, 32, mode, 2, 256, 64, 0)
        assert not train_mlp.xyz_grad_supported(net, 2 * 64 * 24, 24, mode, 2, 256, 64, 0)
        assert not train_mlp.xyz_grad_supported(net, 2 * 64 * 32, 32, mode, 2, 256, 64, 5)       # the stack expects 3 channels
    assert not train_mlp.xyz_grad_supported(net, 2 * 64 * 32, 32, "weighted_avg", 2, 256, 64, 0)
    assert not train_mlp.xyz_grad_supported(_SharedMLP(3, [32, 64], bn=False).train().net, 2 * 64 * 32, 32, "max", 2, 256, 64, 0)
    assert PointnetSAModule(0, 64, 0.3, 32, [32, 64]).fused_xyz_grad is False
    assert PointnetSAModuleMSG(0, 64, [0.1, 0.2], [16, 32], [[32, 64], [32, 64]]).fused_xyz_grad is False
