"""CPU tests of the FP training node with a ragged unknown side (pn2_mlp_train_*_fp_ragged, include/pn2ops.h,
csrc/train_mlp_fp.hip / train_mlp_fp_ragged.hip): declared and exported, pn2_fp_src unchanged, arguments refused before anything
is launched, the support and workspace queries, their Python mirror, and the module's opt-in attribute."""
import ctypes

from test_abi import _declared

NEW = ("pn2_mlp_train_fp_ragged_supported", "pn2_mlp_train_ws_bytes_fp_ragged", "pn2_mlp_train_forward_fp_ragged",
       "pn2_mlp_train_backward_fp_ragged")
PN2_E_NULL, PN2_E_ARG = -1, -3
FAKE = 0x1000                                                  # never dereferenced: every call below fails its checks first
CASE_A = (4, 1024, 256, 35, 6, (41, 64, 32))                   # b, n, m, c2, c1, widths: the GPU file's case A
CASE_B = (4, 200, 25, 32, 0, (32, 32, 32, 64))
CASE_C = (2, 96, 16, 16, 16, (32, 32))


def _lib():
    from pointnet2_amd import _C
    return _C.lib()


def _w(*v):
    return (ctypes.c_int * len(v))(*v)


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


def _src(b, n, m, c2, c1, **kw):
    from pointnet2_amd.train_mlp import FpSrc
    s = FpSrc()
    s.b, s.n, s.m, s.c2, s.c1 = b, n, m, c2, c1
    s.points2 = s.idx = s.dist = FAKE
    s.points1 = FAKE if c1 else None
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _fwd(lib, src, layers, nlayers=2, lengths=FAKE, out=FAKE, weight=FAKE, mask=FAKE, ws=FAKE):
    return lib.pn2_mlp_train_forward_fp_ragged(nlayers, layers, ctypes.byref(src) if src is not None else None, lengths, out, weight,
                                               mask, ws, None, None)


def _bwd(lib, src, layers, nlayers=2, lengths=FAKE, weight=FAKE, out=FAKE, gout=FAKE, g2=FAKE, g1=FAKE, mask=FAKE, ws=FAKE):
    return lib.pn2_mlp_train_backward_fp_ragged(nlayers, layers, ctypes.byref(src) if src is not None else None, lengths, weight, out,
                                                gout, g2, g1, 0, mask, ws, None, None)


def test_fp_ragged_entries_declared_and_exported():
    from pointnet2_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    names = _declared()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _C.EXPORTED, n


def test_fp_src_keeps_its_size():
    from pointnet2_amd.train_mlp import FpSrc
    assert ctypes.sizeof(FpSrc) == 64                          # the lengths and the mask travel as arguments


def test_fp_ragged_supported_and_workspace():
    lib = _lib()
    for b, n, m, c2, c1, widths in (CASE_A, CASE_B, CASE_C):
        nl = len(widths) - 1
        assert lib.pn2_mlp_train_fp_supported(b, n, m, c2, c1, nl, _w(*widths)) == 1
        assert lib.pn2_mlp_train_fp_ragged_supported(b, n, m, c2, c1, nl, _w(*widths)) == 1
        for backward in (0, 1):
            assert lib.pn2_mlp_train_ws_bytes_fp_ragged(b, n, m, c2, c1, nl, _w(*widths), backward, None) > 0
    b, n, m, c2, c1, widths = CASE_A
    assert lib.pn2_mlp_train_fp_ragged_supported(3, 100, m, c2, c1, 2, _w(*widths)) == 0          # b n % 32
    assert lib.pn2_mlp_train_ws_bytes_fp_ragged(3, 100, m, c2, c1, 2, _w(*widths), 0, None) == -1
    assert lib.pn2_mlp_train_fp_ragged_supported(0, n, m, c2, c1, 2, _w(*widths)) == 0
    # where the dense node says no: layer 1 of width 96 (no whole rows per workgroup of its vector pass), a width % 4, no widths
    for bad in ((41, 96, 32), (41, 64, 30), (40, 64, 32)):
        assert lib.pn2_mlp_train_fp_supported(b, n, m, c2, c1, 2, _w(*bad)) == 0
        assert lib.pn2_mlp_train_fp_ragged_supported(b, n, m, c2, c1, 2, _w(*bad)) == 0
        assert lib.pn2_mlp_train_ws_bytes_fp_ragged(b, n, m, c2, c1, 2, _w(*bad), 1, None) == -1
    assert lib.pn2_mlp_train_fp_ragged_supported(b, n, m, c2, c1, 2, None) == 0
    assert lib.pn2_mlp_train_fp_ragged_supported(b, n, m, c2, c1, 8, _w(*([41] + [32] * 8))) == 0     # at most 7 layers


def test_fp_ragged_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib()
    b, n, m, c2, c1, widths = CASE_A
    ok, src = _layers(*widths), _src(b, n, m, c2, c1)
    assert _fwd(lib, src, ok, lengths=None) == PN2_E_NULL                     # no lengths (forward reads them)
    for call in (_fwd, _bwd):
        assert call(lib, src, ok, mask=None) == PN2_E_NULL                    # no mask buffer
        assert call(lib, None, ok) == PN2_E_NULL                              # the dense entries' checks behind them
        assert call(lib, src, ok, ws=None) == PN2_E_NULL
        assert call(lib, src, ok, out=None) == PN2_E_NULL
        assert call(lib, _src(b, n, m, c2, c1, points2=None), ok) == PN2_E_NULL
        assert call(lib, _src(b, n, m, c2, c1, points1=None), ok) == PN2_E_NULL
        assert call(lib, _src(3, 100, m, c2, c1), ok) == PN2_E_ARG            # b n % 32
        assert call(lib, _src(0, n, m, c2, c1), ok) == PN2_E_ARG
        assert call(lib, _src(b, n, 0, c2, c1), ok) == PN2_E_ARG
        assert call(lib, _src(b, n, m, c2, 5), ok) == PN2_E_ARG               # cin_1 != c2 + c1
        assert call(lib, src, None) == PN2_E_ARG
        assert call(lib, src, _layers(41, 96, 32)) == PN2_E_ARG
        assert call(lib, src, _layers(41, 64, 30)) == PN2_E_ARG
        assert call(lib, _src(b, n, m, 41, 0, points1=FAKE), ok) == PN2_E_ARG  # skip features without channels
    assert _fwd(lib, src, ok, weight=None) == PN2_E_NULL
    assert _bwd(lib, src, ok, gout=None) == PN2_E_NULL
    assert _bwd(lib, src, ok, weight=None) == PN2_E_NULL
    assert _bwd(lib, _src(b, n, m, 41, 0), ok, g1=FAKE) == PN2_E_ARG
    # backward takes lengths for symmetry and does not look at it: a NULL there changes no answer
    assert _bwd(lib, src, ok, lengths=None, ws=None) == PN2_E_NULL and _bwd(lib, _src(3, 100, m, c2, c1), ok, lengths=None) == PN2_E_ARG


def test_python_fp_level_ragged_supported_mirrors_the_c_query():
    from pointnet2_amd import train_mlp
    from pointnet2_amd.pointnet_util import PointnetFPModule, _SharedMLP
    lib = _lib()
    for b, n, m, c2, c1, widths in (CASE_A, CASE_B, CASE_C, (3, 100, 20, 32, 8, (40, 32, 32)), (4, 256, 64, 64, 8, (72, 96, 32)),
                                    (16, 2048, 512, 128, 6, (134, 128, 128, 128))):
        net = _SharedMLP(c2 + c1, list(widths[1:])).train().net
        want = lib.pn2_mlp_train_fp_ragged_supported(b, n, m, c2, c1, len(widths) - 1, _w(*widths)) == 1
        assert train_mlp.fp_level_ragged_supported(net, b, n, m, c2, c1) is want, (b, n, m, c2, c1, widths)
        assert want == (train_mlp.fp_level_supported(net, b, n, m, c2, c1) and (b * n) % 32 == 0)
    assert train_mlp.fp_level_ragged_supported(_SharedMLP(41, [64, 32]).train().net, *CASE_A[:5])
    assert not train_mlp.fp_level_ragged_supported(_SharedMLP(41, [64, 32]).eval().net, *CASE_A[:5])      # batch statistics only
    assert not train_mlp.fp_level_ragged_supported(_SharedMLP(41, [64, 32]).train().net, 4, 1024, 256, 35, 5)
    assert PointnetFPModule(41, [64, 32]).fused_ragged_node is False
