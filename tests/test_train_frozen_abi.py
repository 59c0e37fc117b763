"""CPU tests of the frozen-statistics entries of the training node (pn2_mlp_train_*_frozen, include/pn2ops.h,
csrc/train_mlp_frozen.hip): declared and exported, the struct layout unchanged, arguments refused before anything is launched,
and the Python mirror train_mlp.frozen_supported beside an unchanged stack_supported."""
import ctypes
import os
import subprocess

from test_abi import ROOT, _declared

NEW = ("pn2_mlp_train_frozen_supported", "pn2_mlp_train_ws_bytes_frozen", "pn2_mlp_train_forward_frozen",
       "pn2_mlp_train_backward_frozen")
PN2_E_NULL, PN2_E_ARG = -1, -3
FAKE = 0x1000                                                  # never dereferenced: every call below fails its checks first


def _lib():
    from pointnet2_amd import _C
    return _C.lib()


def _layers(*widths, running=True):
    from pointnet2_amd.train_mlp import BnLayer
    arr = (BnLayer * (len(widths) - 1))()
    for l in range(len(widths) - 1):
        L = arr[l]
        L.cin, L.cout = widths[l], widths[l + 1]
        L.weight = L.gamma = L.beta = L.save = L.z = L.grad_weight = L.grad_gamma = L.grad_beta = FAKE
        if running:
            L.running_mean = L.running_var = FAKE
        L.w_stride_k, L.w_stride_n = 1, widths[l]
        L.eps = 1e-5
    return arr


def _group(b=2, n=256, m=64, ns=32, centroid=True):
    from pointnet2_amd.train_mlp import GroupSrc
    g = GroupSrc()
    g.b, g.n, g.m, g.nsample, g.cfeat, g.xyz_first = b, n, m, ns, 0, 1
    g.xyz, g.idx, g.new_xyz, g.points = FAKE, FAKE, (FAKE if centroid else None), None
    return g


def _fwd(lib, layers, group, pooling, rows=2 * 64 * 32, x=None, pool_rows=32):
    f = ctypes.c_void_p(FAKE)
    return lib.pn2_mlp_train_forward_frozen(rows, 3, layers, group, x, pool_rows, pooling, f, f, f, f, f, None, None)


def _bwd(lib, layers, group, pooling, grad_xyz=None, grad_new_xyz=None, rows=2 * 64 * 32, x=None, pool_rows=32):
    f = ctypes.c_void_p(FAKE)
    return lib.pn2_mlp_train_backward_frozen(rows, 3, layers, group, x, pool_rows, pooling, f, f, f, f, f, None, None, None,
                                             grad_xyz, grad_new_xyz, None, 0, f, None, None)


def test_frozen_entries_declared_and_exported():
    from pointnet2_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    names = _declared()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _C.EXPORTED, n


def test_header_compiles_and_bn_layer_keeps_its_size(tmp_path):
    """The conv-bias gradients travel as an argument of the backward entry: pn2_bn_layer did not grow."""
    from pointnet2_amd.train_mlp import BnLayer
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "pn2ops.h"\nint main(void) {\n'
                   '    int (*f)(long long, int, const pn2_bn_layer *, const pn2_group_src *, const float *, int, int, float *, int *,\n'
                   '             float *, float *, void *, const pn2_train_opts *, void *) = pn2_mlp_train_forward_frozen;\n'
                   '    (void)f;\n    printf("%zu\\n", sizeof(pn2_bn_layer));\n    return 0; }\n')
    exe = tmp_path / "size"
    from pointnet2_amd import _C
    libdir = os.path.dirname(_C.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lpn2ops", "-Wl,-rpath," + libdir], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert int(out) == ctypes.sizeof(BnLayer)


def test_frozen_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib()
    f = ctypes.c_void_p(FAKE)
    g = _group()
    ok, bare = _layers(3, 32, 32, 64), _layers(3, 32, 32, 64, running=False)
    for call in (_fwd, _bwd):
        assert call(lib, bare, ctypes.byref(g), 0) == PN2_E_NULL              # no running statistics
        for bad in (-1, 4):
            assert call(lib, ok, ctypes.byref(g), bad) == PN2_E_ARG           # pooling outside 0..3
        assert call(lib, ok, ctypes.byref(g), 0, rows=2 * 64 * 32 + 8) == PN2_E_ARG      # rows % 32
        assert call(lib, ok, None, 0, x=f, pool_rows=0, rows=2048 + 8) == PN2_E_ARG       # ... plain rows too
        assert call(lib, ok, None, 0, pool_rows=0) == PN2_E_NULL              # neither group nor x
        assert call(lib, ok, None, 1, x=f, pool_rows=0) == PN2_E_NULL         # an averaging mode without a group
    assert _bwd(lib, ok, ctypes.byref(g), 2, f, f) == PN2_E_ARG               # weighted_avg: no coordinate gradient
    assert _bwd(lib, ok, ctypes.byref(g), 0, None, f) == PN2_E_NULL           # the centroid's gradient alone
    assert _bwd(lib, ok, ctypes.byref(g), 0, f, None) == PN2_E_NULL           # a centroid without a place for its gradient
    nc = _group(centroid=False)
    assert _bwd(lib, ok, ctypes.byref(nc), 0, f, f) == PN2_E_ARG              # a gradient for a centroid that is not there


def test_frozen_supported_and_workspace_follow_the_pool_and_xyz_queries():
    lib = _lib()
    w = lambda *v: (ctypes.c_int * len(v))(*v)
    rows, widths, gd = 4 * 256 * 32, (3, 64, 64, 128), (ctypes.c_int * 6)(4, 1024, 256, 32, 0, 1)
    for mode in range(4):
        assert lib.pn2_mlp_train_frozen_supported(rows, 3, w(*widths), 32, mode, None, 0) == 1
        assert lib.pn2_mlp_train_frozen_supported(rows, 3, w(*widths), 32, mode, gd, 1) == (0 if mode == 2 else 1)
        assert lib.pn2_mlp_train_frozen_supported(4 * 256 * 24, 3, w(*widths), 24, mode, None, 0) == 0       # nsample 24
        for backward in (0, 1):
            assert lib.pn2_mlp_train_ws_bytes_frozen(rows, 3, w(*widths), 32, mode, backward, gd, 0, None) == \
                lib.pn2_mlp_train_ws_bytes_pool(rows, 3, w(*widths), 32, mode, backward, gd, None) > 0
        if mode != 2:
            assert lib.pn2_mlp_train_ws_bytes_frozen(rows, 3, w(*widths), 32, mode, 1, gd, 1, None) == \
                lib.pn2_mlp_train_ws_bytes_xyz(rows, 3, w(*widths), 32, mode, gd, None) > 0
    assert lib.pn2_mlp_train_frozen_supported(8192, 2, w(128, 128, 128), 0, 0, None, 0) == 1                 # plain rows
    assert lib.pn2_mlp_train_frozen_supported(8192 + 8, 2, w(128, 128, 128), 0, 0, None, 0) == 0


def test_python_frozen_supported_mirrors_stack_supported():
    import torch
    from pointnet2_amd import train_mlp
    from pointnet2_amd.pointnet_util import PointnetFPModule, PointnetSAModule, PointnetSAModuleMSG, _SharedMLP
    rows = 2 * 64 * 32
    frozen = _SharedMLP(3, [32, 32, 64]).eval().net
    assert train_mlp.frozen_supported(frozen, rows, 32, True)
    for mode in ("max", "avg", "weighted_avg", "max_and_avg"):
        assert train_mlp.frozen_supported(frozen, rows, 32, True, mode)
    assert train_mlp.frozen_supported(frozen, rows, 32, True, "max", (2, 256, 64, 0, True))
    assert not train_mlp.frozen_supported(frozen, rows, 32, True, "weighted_avg", (2, 256, 64, 0, True))
    assert not train_mlp.frozen_supported(frozen, 2 * 64 * 24, 24, True)
    assert not train_mlp.stack_supported(frozen, rows, 32, True)                  # unchanged: that is not the batch-statistics path
    live = _SharedMLP(3, [32, 32, 64]).train().net
    assert train_mlp.stack_supported(live, rows, 32, True) and not train_mlp.frozen_supported(live, rows, 32, True)
    mixed = _SharedMLP(3, [32, 32, 64]).train().net
    mixed[1].eval()                                                               # one batch norm frozen, two not
    assert not train_mlp.frozen_supported(mixed, rows, 32, True) and not train_mlp.stack_supported(mixed, rows, 32, True)
    untracked = _SharedMLP(3, [32, 64]).net
    for i, mod in enumerate(untracked):
        if isinstance(mod, torch.nn.BatchNorm2d):
            untracked[i] = torch.nn.BatchNorm2d(mod.num_features, track_running_stats=False)
    untracked.eval()
    assert not train_mlp.frozen_supported(untracked, rows, 32, True) and not train_mlp.stack_supported(untracked, rows, 32, True)
    assert not train_mlp.frozen_supported(_SharedMLP(3, [32, 64], bn=False).eval().net, rows, 32, True)
    plain = _SharedMLP(134, [128, 128]).eval().net                                # an odd FP width: zero-padded to 136
    assert train_mlp.frozen_supported(plain, 2 * 2048, 0, False) and not train_mlp.stack_supported(plain, 2 * 2048, 0, False)
    assert PointnetSAModule(0, 64, 0.3, 32, [32, 64]).fused_frozen_bn is False
    assert PointnetSAModuleMSG(0, 64, [0.1, 0.2], [16, 32], [[32, 64], [32, 64]]).fused_frozen_bn is False
    assert PointnetFPModule(64, [32, 32]).fused_frozen_bn is False
