"""CPU tests of the FP-level training node's C entries (pn2_mlp_train_*_fp, include/pn2ops.h): declared and exported, the ctypes
mirror of pn2_fp_src matches the C compiler's layout, arguments refused before anything is launched, the support query."""
import ctypes
import os
import subprocess

from test_abi import ROOT, _declared

NEW = ("pn2_mlp_train_fp_supported", "pn2_mlp_train_ws_bytes_fp", "pn2_mlp_train_forward_fp", "pn2_mlp_train_backward_fp")
PN2_E_NULL, PN2_E_ARG = -1, -3


def _lib():
    from pointnet2_amd import _C
    return _C.lib()


def _w(*widths):
    return (ctypes.c_int * len(widths))(*widths)


def _src(b=2, n=64, m=16, c2=32, c1=8):
    from pointnet2_amd.train_mlp import FpSrc
    s = FpSrc()
    s.b, s.n, s.m, s.c2, s.c1 = b, n, m, c2, c1
    fake = 0x1000                                              # never dereferenced: every case below fails its checks first
    s.points2, s.points1, s.idx, s.dist = fake, (fake if c1 else None), fake, fake
    return s


def _layers(*widths):
    from pointnet2_amd.train_mlp import BnLayer
    arr = (BnLayer * (len(widths) - 1))()
    for l in range(len(widths) - 1):
        L = arr[l]
        L.cin, L.cout = widths[l], widths[l + 1]
        L.weight = L.gamma = L.beta = L.save = L.z = L.grad_weight = L.grad_gamma = L.grad_beta = 0x1000
        L.w_stride_k, L.w_stride_n = 1, widths[l]
    return arr


def test_fp_entries_declared_and_exported():
    from pointnet2_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    names = _declared()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _C.EXPORTED, n


def test_fp_src_mirror_matches_the_header(tmp_path):
    from pointnet2_amd.train_mlp import FpSrc
    body = ['#include "pn2ops.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
            'printf("%zu", sizeof(pn2_fp_src));']
    body += ['printf(" %%zu", offsetof(pn2_fp_src, %s));' % f for f, _ in FpSrc._fields_]
    body += ['printf("\\n");', "return 0; }"]
    src = tmp_path / "fp.c"
    src.write_text("\n".join(body) + "\n")
    exe = tmp_path / "fp"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    parts = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert parts[0] == ctypes.sizeof(FpSrc)
    assert parts[1:] == [getattr(FpSrc, f).offset for f, _ in FpSrc._fields_]


def test_fp_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib()
    L = _layers(40, 32, 64)
    fake = ctypes.c_void_p(0x1000)
    fwd = lambda s, layers=L, nl=2: lib.pn2_mlp_train_forward_fp(nl, layers, s, fake, fake, fake, None, None)
    bwd = lambda s, layers=L, nl=2: lib.pn2_mlp_train_backward_fp(nl, layers, s, fake, fake, fake, fake, fake, 0, fake, None, None)
    for call in (fwd, bwd):
        assert call(None) == PN2_E_NULL                                              # no source
        assert call(ctypes.byref(_src(n=60))) == PN2_E_ARG                           # b n = 120: rows % 32
        assert call(ctypes.byref(_src(m=0))) == PN2_E_ARG                            # no known point with n > 0
        assert call(ctypes.byref(_src(c2=30))) == PN2_E_ARG                          # layer 1 expects 40 = c2 + c1, gets 38
        assert call(ctypes.byref(_src()), _layers(40, 32, 62)) == PN2_E_ARG          # width % 4
        assert call(ctypes.byref(_src()), None) == PN2_E_ARG                         # no layers
    s = _src()
    s.points2 = None
    assert fwd(ctypes.byref(s)) == PN2_E_NULL
    s = _src()
    s.points1 = None                                                                 # c1 = 8 without skip features
    assert fwd(ctypes.byref(s)) == PN2_E_NULL and bwd(ctypes.byref(s)) == PN2_E_NULL


def test_fp_supported_answers():
    lib = _lib()
    assert lib.pn2_mlp_train_fp_supported(8, 8192, 1024, 128, 0, 3, _w(128, 128, 128, 128)) == 1       # sem_seg FP4
    assert lib.pn2_mlp_train_fp_supported(16, 128, 1, 1024, 256, 2, _w(1280, 256, 256)) == 1           # part_seg FP1: m = 1
    assert lib.pn2_mlp_train_fp_supported(2, 64, 2, 29, 6, 2, _w(35, 64, 32)) == 1                     # odd widths, m = 2
    assert lib.pn2_mlp_train_fp_supported(2, 60, 2, 29, 6, 2, _w(35, 64, 32)) == 0                     # rows % 32
    assert lib.pn2_mlp_train_fp_supported(2, 64, 2, 29, 6, 2, _w(36, 64, 32)) == 0                     # widths mismatch
    assert lib.pn2_mlp_train_fp_supported(2, 64, 2, 32, 0, 2, _w(32, 96, 32)) == 0                     # layer 1: 24 threads a row
    assert lib.pn2_mlp_train_fp_supported(2, 64, 0, 32, 0, 2, _w(32, 64, 32)) == 0                     # m = 0
    assert lib.pn2_mlp_train_ws_bytes_fp(2, 64, 0, 32, 0, 2, _w(32, 64, 32), 0, None) < 0
    f = lib.pn2_mlp_train_ws_bytes_fp(8, 8192, 1024, 128, 0, 3, _w(128, 128, 128, 128), 0, None)
    b = lib.pn2_mlp_train_ws_bytes_fp(8, 8192, 1024, 128, 0, 3, _w(128, 128, 128, 128), 1, None)
    assert 0 < f < b


def test_python_fp_level_supported():
    from pointnet2_amd import train_mlp
    from pointnet2_amd.pointnet_util import _SharedMLP
    net = _SharedMLP(128 + 6, [128, 128, 128]).train().net
    assert train_mlp.fp_level_supported(net, 16, 2048, 512, 128, 6)
    assert not train_mlp.fp_level_supported(net, 16, 2047, 512, 128, 6)           # b n % 32
    assert not train_mlp.fp_level_supported(net, 16, 2048, 512, 128, 0)           # widths mismatch
    frozen = _SharedMLP(128, [128, 128]).train()
    frozen.net[1].eval()
    assert not train_mlp.fp_level_supported(frozen.net, 8, 8192, 1024, 128, 0)


def test_fp_node_size_rule_at_the_reference_levels():
    """The modules take the node where it measured faster (train_mlp.FP_NODE_MIN_SAVED): sem_seg FP4, part_seg FP3 and FP1."""
    from pointnet2_amd import train_mlp
    from pointnet2_amd.reference_configs import FP_LEVELS
    taken = {name for name, b, n, m, c2 in FP_LEVELS if train_mlp.fp_level_preferred(b, n, m, c2)}
    assert taken == {"cfg5 sem_seg FP4", "cfg4 part_seg FP3", "cfg4 part_seg FP1"}
