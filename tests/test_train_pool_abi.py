"""CPU tests of the pooling entries of the training node (pn2_mlp_train_*_pool, include/pn2ops.h): declared and exported,
arguments refused before anything is launched, and the support query's answers."""
import ctypes

import torch.nn as nn

from test_abi import _declared

NEW = ("pn2_mlp_train_pool_supported", "pn2_mlp_train_ws_bytes_pool", "pn2_mlp_train_forward_pool",
       "pn2_mlp_train_backward_pool")
PN2_E_NULL, PN2_E_ARG = -1, -3


def _lib():
    from pointnet2_amd import _C
    return _C.lib()


def _w(*widths):
    return (ctypes.c_int * len(widths))(*widths)


def test_pool_entries_declared_and_exported():
    from pointnet2_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    names = _declared()
    for n in NEW:
        assert n in names, n
        assert hasattr(lib, n), n
        assert n in _C.EXPORTED, n
    assert _C.version().startswith("pn2ops 0.3.0")
    import pointnet2_amd
    assert pointnet2_amd.__version__ == "0.3.0"


def test_bad_pooling_is_an_argument_error():
    lib = _lib()
    for bad in (-1, 4, 99):
        assert lib.pn2_mlp_train_forward_pool(1024, 1, None, None, 32, bad, None, None, None, None, None, None, None) == PN2_E_ARG
        assert lib.pn2_mlp_train_backward_pool(1024, 1, None, None, 32, bad, None, None, None, None, None, None, None, 0, None,
                                               None, None) == PN2_E_ARG
        assert lib.pn2_mlp_train_pool_supported(1024, 2, _w(3, 32, 64), 32, bad) == 0
        assert lib.pn2_mlp_train_ws_bytes_pool(1024, 2, _w(3, 32, 64), 32, bad, 0, None, None) < 0


def test_averaging_modes_need_a_grouped_input():
    lib = _lib()
    for mode in (1, 2, 3):
        assert lib.pn2_mlp_train_forward_pool(1024, 1, None, None, 32, mode, None, None, None, None, None, None, None) == PN2_E_NULL
        assert lib.pn2_mlp_train_backward_pool(1024, 1, None, None, 32, mode, None, None, None, None, None, None, None, 0, None,
                                               None, None) == PN2_E_NULL


def test_pool_supported_answers():
    lib = _lib()
    rows = 4 * 256 * 32
    for mode in range(4):
        assert lib.pn2_mlp_train_pool_supported(rows, 3, _w(3, 64, 64, 128), 32, mode) == 1
        assert lib.pn2_mlp_train_pool_supported(4 * 256 * 16, 3, _w(3, 64, 64, 128), 16, mode) == 1
        assert lib.pn2_mlp_train_pool_supported(4 * 256 * 64, 2, _w(131, 128, 256), 64, mode) == 1
        assert lib.pn2_mlp_train_pool_supported(4 * 256 * 24, 3, _w(3, 64, 64, 128), 24, mode) == 0     # nsample 24
        assert lib.pn2_mlp_train_pool_supported(rows, 2, _w(3, 64, 66), 32, mode) == 0                 # width % 4
        assert lib.pn2_mlp_train_pool_supported(rows, 9, _w(*([3] + [32] * 9)), 32, mode) == 0         # > 8 layers
        assert lib.pn2_mlp_train_pool_supported(rows + 32, 2, _w(3, 32, 64), 64, mode) == 0            # rows % nsample
    for mode in (1, 2, 3):
        assert lib.pn2_mlp_train_pool_supported(rows, 2, _w(3, 32, 64), 0, mode) == 0                  # no group size


def test_pool_workspaces():
    lib = _lib()
    rows, w = 4 * 256 * 32, _w(3, 64, 64, 128)
    gd = (ctypes.c_int * 6)(4, 1024, 256, 32, 0, 1)
    for bw in (0, 1):                                          # pooling 0: the _ex workspace
        assert lib.pn2_mlp_train_ws_bytes_pool(rows, 3, w, 32, 0, bw, gd, None) == lib.pn2_mlp_train_ws_bytes_ex(rows, 3, w, 32, bw, gd, None)
    f1 = lib.pn2_mlp_train_ws_bytes_pool(rows, 3, w, 32, 1, 0, gd, None)
    f3 = lib.pn2_mlp_train_ws_bytes_pool(rows, 3, w, 32, 3, 0, gd, None)
    assert f1 > 0 and f3 >= f1 + 256 * 4 * 128 * 4             # max_and_avg: the max half besides
    for mode in (1, 2, 3):                                     # backward: the dense top layer's workspace
        assert lib.pn2_mlp_train_ws_bytes_pool(rows, 3, w, 32, mode, 1, gd, None) == lib.pn2_mlp_train_ws_bytes_ex(rows, 3, w, 0, 1, gd, None)


def test_python_pool_supported():
    from pointnet2_amd import train_mlp
    from pointnet2_amd.pointnet_util import _SharedMLP
    net = _SharedMLP(3, [32, 32, 64]).train().net
    for mode in ("max", "avg", "weighted_avg", "max_and_avg"):
        assert train_mlp.pool_supported(net, 2 * 64 * 32, 32, mode)
        assert not train_mlp.pool_supported(net, 2 * 64 * 24, 24, mode)
    assert not train_mlp.pool_supported(net, 2 * 64 * 32, 32, "median")
    assert not train_mlp.pool_supported(_SharedMLP(3, [32, 64], bn=False).train().net, 2 * 64 * 32, 32, "avg")
    frozen = _SharedMLP(3, [32, 64]).train()
    frozen.net[1].eval()
    assert not train_mlp.pool_supported(frozen.net, 2 * 64 * 32, 32, "avg")
    assert isinstance(net[0], nn.Conv2d)
