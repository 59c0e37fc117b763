"""CPU tests of the ragged-rows entries of the training node (pn2_mlp_train_*_ragged, include/pn2ops.h,
csrc/train_mlp_ragged.hip): declared and exported, the struct layouts unchanged, arguments refused before anything is launched,
the support and workspace queries, their Python mirror, and the module's opt-in flag, which changes nothing on CPU tensors."""
import ctypes
import os
import subprocess

from test_abi import ROOT, _declared

NEW = ("pn2_mlp_train_ragged_supported", "pn2_mlp_train_ws_bytes_ragged", "pn2_mlp_train_forward_ragged",
       "pn2_mlp_train_backward_ragged")
PN2_E_NULL, PN2_E_ARG = -1, -3
FAKE = 0x1000                                                  # never dereferenced: every call below fails its checks first
WIDTHS_A, WIDTHS_B = (40, 64, 32), (32, 32, 32, 64)            # the GPU cases' stacks (38 inputs enter zero-padded to 40)


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


def _fwd(lib, b, n, lengths, layers, nlayers=2, x=FAKE, out=FAKE, mask=FAKE, ws=FAKE):
    return lib.pn2_mlp_train_forward_ragged(b, n, lengths, nlayers, layers, x, out, mask, ws, None, None)


def _bwd(lib, b, n, lengths, layers, nlayers=2, x=FAKE, out=FAKE, gout=FAKE, gx=FAKE, mask=FAKE, ws=FAKE):
    return lib.pn2_mlp_train_backward_ragged(b, n, lengths, nlayers, layers, x, out, gout, gx, mask, ws, None, None)


def test_ragged_entries_declared_and_exported():
    from pointnet2_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    names = _declared()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _C.EXPORTED, n


def test_header_compiles_as_c99_and_the_structs_keep_their_sizes(tmp_path):
    """The mask and the lengths travel as arguments: neither pn2_bn_layer nor pn2_train_opts grew."""
    from pointnet2_amd.train_mlp import BnLayer, TrainOpts
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "pn2ops.h"\nint main(void) {\n'
                   '    int (*f)(int, int, const int *, int, const pn2_bn_layer *, const float *, float *, void *, void *,\n'
                   '             const pn2_train_opts *, void *) = pn2_mlp_train_forward_ragged;\n'
                   '    int (*g)(int, int, const int *, int, const pn2_bn_layer *, const float *, const float *, const float *,\n'
                   '             float *, const void *, void *, const pn2_train_opts *, void *) = pn2_mlp_train_backward_ragged;\n'
                   '    int (*s)(int, int, int, const int *) = pn2_mlp_train_ragged_supported;\n'
                   '    long long (*w)(int, int, int, const int *, int, const pn2_train_opts *) = pn2_mlp_train_ws_bytes_ragged;\n'
                   '    (void)f; (void)g; (void)s; (void)w;\n'
                   '    printf("%zu %zu\\n", sizeof(pn2_bn_layer), sizeof(pn2_train_opts));\n    return 0; }\n')
    exe = tmp_path / "size"
    from pointnet2_amd import _C
    libdir = os.path.dirname(_C.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lpn2ops", "-Wl,-rpath," + libdir], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(BnLayer) == 128
    assert int(out[1]) == ctypes.sizeof(TrainOpts) == 48


def test_ragged_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib()
    ok = _layers(*WIDTHS_A)
    for call in (_fwd, _bwd):
        assert call(lib, 4, 1024, None, ok) == PN2_E_NULL                     # no lengths
        assert call(lib, 4, 1024, FAKE, ok, mask=None) == PN2_E_NULL          # no mask buffer
        assert call(lib, 3, 100, FAKE, ok) == PN2_E_ARG                       # b n % 32
        assert call(lib, 0, 1024, FAKE, ok) == PN2_E_ARG and call(lib, 4, -32, FAKE, ok) == PN2_E_ARG
        assert call(lib, 4, 1024, FAKE, ok, x=None) == PN2_E_NULL             # the dense entries' checks behind them
        assert call(lib, 4, 1024, FAKE, ok, ws=None) == PN2_E_NULL
        assert call(lib, 4, 1024, FAKE, None) == PN2_E_ARG
        assert call(lib, 4, 1024, FAKE, _layers(38, 64, 32)) == PN2_E_ARG     # plain rows are read 16 bytes at a time
        assert call(lib, 4, 1024, FAKE, _layers(40, 64, 30)) == PN2_E_ARG
    assert _bwd(lib, 4, 1024, FAKE, ok, gout=None) == PN2_E_NULL


def test_ragged_supported_and_workspace():
    lib = _lib()
    for b, n in ((4, 200), (4, 1024)):
        for widths in (WIDTHS_A, WIDTHS_B):
            nl = len(widths) - 1
            assert lib.pn2_mlp_train_ragged_supported(b, n, nl, _w(*widths)) == 1
            for backward in (0, 1):
                assert lib.pn2_mlp_train_ws_bytes_ragged(b, n, nl, _w(*widths), backward, None) > 0
    for widths in (WIDTHS_A, WIDTHS_B):
        nl = len(widths) - 1
        assert lib.pn2_mlp_train_ragged_supported(3, 100, nl, _w(*widths)) == 0
        for backward in (0, 1):
            assert lib.pn2_mlp_train_ws_bytes_ragged(3, 100, nl, _w(*widths), backward, None) == -1
    assert lib.pn2_mlp_train_ragged_supported(4, 1024, 2, _w(38, 64, 32)) == 0      # the caller pads (fp_mlp_train does)
    assert lib.pn2_mlp_train_ragged_supported(4, 1024, 2, _w(40, 64, 30)) == 0
    assert lib.pn2_mlp_train_ragged_supported(4, 1024, 2, None) == 0
    assert lib.pn2_mlp_train_ragged_supported(4, 1024, 9, _w(*([32] * 10))) == 0
    assert lib.pn2_mlp_train_ragged_supported(1 << 16, 1 << 15, 2, _w(*WIDTHS_A)) == 0       # 2^31 rows


def test_python_ragged_supported_mirrors_the_c_query():
    from pointnet2_amd import train_mlp
    from pointnet2_amd.pointnet_util import PointnetFPModule, _SharedMLP
    lib = _lib()
    for cin, mlp in ((38, [64, 32]), (32, [32, 32, 64]), (134, [128, 128])):
        net = _SharedMLP(cin, mlp).train().net
        widths = [(cin + 3) // 4 * 4] + mlp
        for b, n in ((4, 200), (4, 1024), (3, 100), (16, 2048)):
            want = lib.pn2_mlp_train_ragged_supported(b, n, len(mlp), _w(*widths)) == 1
            assert train_mlp.ragged_supported(net, b, n) is want, (cin, mlp, b, n)
            assert want == ((b * n) % 32 == 0)
    assert not train_mlp.ragged_supported(_SharedMLP(32, [32, 30]).train().net, 4, 1024)
    assert not train_mlp.ragged_supported(_SharedMLP(32, [32, 32]).eval().net, 4, 1024)      # batch statistics only
    assert not train_mlp.ragged_supported(_SharedMLP(32, [32, 32], bn=False).train().net, 4, 1024)
    assert PointnetFPModule(64, [32, 32]).fused_ragged_train is False


def test_fp_mlp_train_refuses_lengths_with_frozen_statistics():
    import pytest
    import torch
    from pointnet2_amd import train_mlp
    from pointnet2_amd.pointnet_util import _SharedMLP
    net = _SharedMLP(32, [32, 32]).eval().net
    with pytest.raises(ValueError):
        train_mlp.fp_mlp_train(net, torch.zeros(4, 64, 32), frozen=True, lengths=torch.tensor([64, 3, 2, 1], dtype=torch.int32))


def test_flag_on_cpu_tensors_keeps_the_unfused_path(monkeypatch):
    """With the flag on, CPU tensors take "unfused_ragged" and give the flag-off tensors. (The operators have no CPU form:
    three_nn's result is handed in as a geometry and three_interpolate is stood in for by its definition in torch.)"""
    import copy
    import torch
    from pointnet2_amd import pointnet_util
    from pointnet2_amd.pointnet_util import FPGeometry, PointnetFPModule

    def interpolate(points, idx, weight, plan=None):
        rows = torch.gather(points.unsqueeze(1).expand(-1, idx.shape[1], -1, -1), 2,
                            idx.long().unsqueeze(3).expand(-1, -1, -1, points.shape[2]))          # (b, n, 3, c)
        return (rows * weight.unsqueeze(3)).sum(dim=2)
    monkeypatch.setattr(pointnet_util, "three_interpolate", interpolate)
    torch.manual_seed(0)
    b, n, m, c2, c1 = 2, 48, 16, 8, 6
    lens = torch.tensor([48, 20], dtype=torch.int32)
    xyz1, xyz2 = torch.rand(b, n, 3), torch.rand(b, m, 3)
    p1, p2 = torch.randn(b, n, c1), torch.randn(b, m, c2)
    idx = torch.cdist(xyz1, xyz2).topk(3, dim=2, largest=False)
    geo = FPGeometry((idx.values ** 2).contiguous(), idx.indices.to(torch.int32).contiguous(), None)
    mod = PointnetFPModule(c2 + c1, [16, 8]).train()
    outs = []
    for flag in (False, True):
        cur = copy.deepcopy(mod)
        cur.fused_ragged_train = flag
        a1, a2 = p1.clone().requires_grad_(), p2.clone().requires_grad_()
        out = cur(xyz1, xyz2, a1, a2, geometry=geo, lengths1=lens)
        assert cur.last_path == "unfused_ragged"
        out.square().sum().backward()
        outs.append([out.detach(), a1.grad, a2.grad] + [p.grad for p in cur.parameters()] + [t.clone() for t in cur.buffers()])
    for u, v in zip(*outs):
        assert torch.equal(u, v)
