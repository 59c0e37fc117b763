"""CPU tests of the large-cloud FPS entries (include/pn2ops.h: pn2_fps_large_ws_bytes, pn2_fps_large_supported,
pn2_fps_large_pays, pn2_farthest_point_sample_large, pn2_farthest_point_sample_large_ex): declared, exported and bound; the
host-side validation answers before any device call, in the dense entry's order, so host memory stands in for every device
pointer and nothing is launched. The entries that existed before keep their behaviour beyond 16384 points."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pn2_fps_large_ws_bytes", "pn2_fps_large_supported", "pn2_fps_large_pays", "pn2_farthest_point_sample_large",
         "pn2_farthest_point_sample_large_ex"]
OK, E_NULL, E_SHAPE, E_ARG, E_TOO_LARGE = 0, -1, -2, -3, -4
LO, HI = 16384, 1048576                                   # the envelope: LO < n <= HI


def test_declared_exported_and_bound():
    from pointnet2_amd import _C
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pn2ops.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pn2_[a-z0-9_]+)\s*\(", txt))
    lib = ctypes.CDLL(_C.LIB_PATH)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert n in declared and hasattr(lib, n) and n in _C.EXPORTED, n
        assert n in integration, n
    plain, ex = _C._SIGNATURES["pn2_farthest_point_sample_large"], _C._SIGNATURES["pn2_farthest_point_sample_large_ex"]
    assert ex == [ctypes.c_int] + plain                    # group_len in front, nothing else differs
    assert _C._RESTYPES["pn2_fps_large_ws_bytes"] is ctypes.c_longlong


class _Mem:
    def __init__(self):
        self.f = (ctypes.c_float * 256)()
        self.i = (ctypes.c_int * 256)()
        self.w = (ctypes.c_char * 64)()
        self.F, self.I = ctypes.addressof(self.f), ctypes.addressof(self.i)
        self.W = (ctypes.addressof(self.w) + 15) & ~15     # 16-byte aligned


@pytest.fixture(scope="module")
def mem():
    return _Mem()


def large(mem, group_len=None, b=1, n=20000, m=4, inp="F", ws="W", out="I"):
    """Only ever called with arguments the entry must refuse (or that leave nothing to do): no launch."""
    from pointnet2_amd import _C
    p = dict(I=mem.I, F=mem.F, W=mem.W, N=None)
    if group_len is None:
        return _C.lib().pn2_farthest_point_sample_large(b, n, m, p[inp], p[ws], p[out], mem.F, None)
    return _C.lib().pn2_farthest_point_sample_large_ex(group_len, b, n, m, p[inp], p[ws], p[out], mem.F, None)


@pytest.mark.parametrize("group_len", [None, 64, 128, 256, 7])
def test_codes_in_the_dense_entrys_order(mem, group_len):
    # nothing to do: before the extents, the pointers, the envelope and group_len
    assert large(mem, group_len, b=0) == OK
    assert large(mem, group_len, m=0) == OK
    assert large(mem, group_len, m=-3) == OK
    assert large(mem, group_len, m=0, n=0) == OK
    assert large(mem, group_len, b=0, inp="N", ws="N", out="N") == OK
    assert large(mem, group_len, b=0, n=5) == OK
    # extents: before the pointers and the envelope
    assert large(mem, group_len, n=0) == E_SHAPE
    assert large(mem, group_len, n=-1) == E_SHAPE
    assert large(mem, group_len, b=-1) == E_SHAPE
    assert large(mem, group_len, n=0, inp="N") == E_SHAPE
    # pointers: before the envelope
    assert large(mem, group_len, inp="N") == E_NULL
    assert large(mem, group_len, out="N") == E_NULL
    assert large(mem, group_len, ws="N") == E_NULL
    assert large(mem, group_len, n=8, ws="N") == E_NULL
    assert large(mem, group_len, n=HI + 1, out="N") == E_NULL
    # the envelope and the int32 extents: before group_len
    assert large(mem, group_len, n=8) == E_TOO_LARGE
    assert large(mem, group_len, n=LO) == E_TOO_LARGE
    assert large(mem, group_len, n=HI + 1) == E_TOO_LARGE
    assert large(mem, group_len, b=1000, n=HI) == E_TOO_LARGE          # b n 3 beyond int32
    assert large(mem, group_len, b=2, n=20000, m=400000000) == E_TOO_LARGE   # b m 3 beyond int32


@pytest.mark.parametrize("group_len", [0, -1, 7, 32, 63, 65, 192, 512])
def test_a_group_len_outside_the_three_values(mem, group_len):
    assert large(mem, group_len) == E_ARG
    assert large(mem, group_len, n=LO + 1) == E_ARG
    assert large(mem, group_len, n=HI) == E_ARG
    assert large(mem, group_len, n=LO) == E_TOO_LARGE                  # the envelope is answered first
    assert large(mem, group_len, ws="N") == E_NULL                      # ... and so are the pointers


def test_at_most_4096_groups_per_cloud(mem):
    """Four box slots per lane: group_len 64 reaches 262144 points, 128 reaches 524288, 256 the whole envelope. Refused before
    anything is launched, like the envelope itself."""
    assert large(mem, 64, n=64 * 4096 + 1) == E_TOO_LARGE
    assert large(mem, 128, n=128 * 4096 + 1) == E_TOO_LARGE
    assert large(mem, 64, n=HI) == E_TOO_LARGE


def test_a_misaligned_workspace_is_refused(mem):
    from pointnet2_amd import _C
    assert _C.lib().pn2_farthest_point_sample_large(1, 20000, 4, mem.F, mem.W + 4, mem.I, mem.F, None) == E_ARG


def test_supported_pays_and_the_workspace_size():
    from pointnet2_amd import _C
    lib = _C.lib()
    assert [lib.pn2_fps_large_supported(n, 64) for n in (LO, LO + 1, HI, HI + 1)] == [0, 1, 1, 0]
    assert lib.pn2_fps_large_supported(20000, 0) == 0 and lib.pn2_fps_large_supported(0, 4) == 0
    for n in (1, 8, LO, HI + 1, -5):
        assert lib.pn2_fps_large_ws_bytes(2, n) == 0
        assert lib.pn2_fps_large_pays(n, 1024) == 0                     # the rule never says 1 outside the envelope
    assert lib.pn2_fps_large_ws_bytes(0, 20000) == 0 and lib.pn2_fps_large_ws_bytes(-1, 20000) == 0
    for b, n in ((1, LO + 1), (2, 20000), (8, HI), (100, HI)):
        assert lib.pn2_fps_large_ws_bytes(b, n) == 20 * b * n           # 16-byte record + running distance per point; no int32 wrap
    for n in (LO + 1, 20000, 131072, HI):
        for m in (1, 64, 1024, 4096):
            assert lib.pn2_fps_large_pays(n, m) in (0, 1)
            assert lib.pn2_fps_large_pays(n, m) <= lib.pn2_fps_large_supported(n, m)


def test_the_existing_entries_keep_their_behaviour(mem):
    from pointnet2_amd import _C
    lib = _C.lib()
    assert lib.pn2_fps_temp_floats(2, 20000) == 40000
    assert lib.pn2_fps_temp_floats(2, LO) == 0
    assert lib.pn2_farthest_point_sample(1, 20000, 4, mem.F, None, mem.I, None) == E_NULL      # still the kernel that needs temp
    assert lib.pn2_farthest_point_sample_ragged(1, LO + 1, 4, mem.F, mem.I, mem.I, mem.F, None) == E_TOO_LARGE
    assert lib.pn2_farthest_point_sample_ragged_counts(1, LO + 1, 4, mem.F, mem.I, mem.I, mem.I, mem.F, None) == E_TOO_LARGE
    assert lib.pn2_farthest_point_sample_ragged_variant(0, 1, LO + 1, 4, mem.F, mem.I, None, mem.I, mem.F, None) == E_TOO_LARGE
    assert lib.pn2_farthest_point_sample_ordered(1, LO + 1, 4, mem.F, mem.I, mem.F, mem.I, None) == E_TOO_LARGE


def test_the_python_switch():
    import pointnet2_amd as P
    from pointnet2_amd import tf_sampling
    assert P.set_fps_large is tf_sampling.set_fps_large
    try:
        for mode in (True, False, None):
            P.set_fps_large(mode)
            assert tf_sampling._FPS_LARGE[0] is mode
        with pytest.raises(ValueError):
            P.set_fps_large(1)
    finally:
        P.set_fps_large(None)
