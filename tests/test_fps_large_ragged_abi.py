"""CPU tests of the ragged large-cloud FPS entries (include/pn2ops.h: pn2_farthest_point_sample_large_ragged,
pn2_farthest_point_sample_large_ragged_ex): declared, exported, bound and named in INTEGRATION.md; the host-side validation answers
before any device call and in the documented order, so host memory stands in for every device pointer and nothing is launched (as
in tests/test_fps_large_abi.py); the entries that existed before keep their behaviour; the Python switch exists, is off by default
and takes bools only."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pn2_farthest_point_sample_large_ragged", "pn2_farthest_point_sample_large_ragged_ex"]
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
    plain, ex = _C._SIGNATURES[NAMES[0]], _C._SIGNATURES[NAMES[1]]
    assert ex == [ctypes.c_int, ctypes.c_int] + plain      # kernel and group_len in front, nothing else differs
    assert plain == [ctypes.c_int] * 3 + [ctypes.c_void_p] * 7


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


def ragged(mem, kernel=None, group_len=256, b=1, n=20000, m=4, inp="F", lengths="I", npoints="I", ws="W", out="I"):
    """Only ever called with arguments the entry must refuse (or that leave nothing to do): no launch. kernel None = the plain
    entry."""
    from pointnet2_amd import _C
    p = dict(I=mem.I, F=mem.F, W=mem.W, M=mem.W + 4, N=None)
    if kernel is None:
        return _C.lib().pn2_farthest_point_sample_large_ragged(b, n, m, p[inp], p[lengths], p[npoints], p[ws], p[out], mem.F, None)
    return _C.lib().pn2_farthest_point_sample_large_ragged_ex(kernel, group_len, b, n, m, p[inp], p[lengths], p[npoints], p[ws], p[out],
                                                              mem.F, None)


# (kernel, group_len): the plain entry, every kernel, and values the fifth check refuses -- the earlier checks answer first
@pytest.mark.parametrize("kernel,group_len", [(None, 256), (0, 256), (1, 64), (2, 128), (7, 256), (-1, 64), (2, 7), (1, 0)])
def test_codes_in_the_documented_order(mem, kernel, group_len):
    def call(**kw):
        return ragged(mem, kernel, group_len, **kw)
    # 1 nothing to do: before the extents, the pointers, the envelope, kernel and group_len
    assert call(b=0) == OK
    assert call(m=0) == OK
    assert call(m=-3) == OK
    assert call(m=0, n=0) == OK
    assert call(b=0, inp="N", lengths="N", npoints="N", ws="N", out="N") == OK
    assert call(b=0, n=5) == OK
    # 2 extents: before the pointers and the envelope
    assert call(n=0) == E_SHAPE
    assert call(n=-1) == E_SHAPE
    assert call(b=-1) == E_SHAPE
    assert call(n=0, inp="N", lengths="N") == E_SHAPE
    # 3 pointers: before the envelope
    assert call(inp="N") == E_NULL
    assert call(out="N") == E_NULL
    assert call(ws="N") == E_NULL
    assert call(lengths="N") == E_NULL
    assert call(n=8, lengths="N") == E_NULL
    assert call(n=HI + 1, ws="N") == E_NULL
    # 4 the envelope and the int32 extents: before kernel, group_len and the alignment
    assert call(n=8) == E_TOO_LARGE
    assert call(n=LO) == E_TOO_LARGE
    assert call(n=HI + 1) == E_TOO_LARGE
    assert call(n=LO, ws="M") == E_TOO_LARGE
    assert call(b=1000, n=HI) == E_TOO_LARGE                            # b n 3 beyond int32
    assert call(b=2, n=20000, m=400000000) == E_TOO_LARGE               # b m 3 beyond int32
    # npoints may be NULL: the checks go on to the next answer
    assert call(npoints="N", n=LO) == E_TOO_LARGE


@pytest.mark.parametrize("kernel,group_len", [(-1, 256), (3, 256), (7, 64), (0, 0), (1, 63), (2, 192), (0, 512), (1, -1), (5, 5)])
def test_a_kernel_or_group_len_out_of_range(mem, kernel, group_len):
    assert ragged(mem, kernel, group_len) == E_ARG
    assert ragged(mem, kernel, group_len, n=LO + 1, npoints="N") == E_ARG
    assert ragged(mem, kernel, group_len, n=HI) == E_ARG
    assert ragged(mem, kernel, group_len, ws="M") == E_ARG               # ... before the group count and the alignment
    assert ragged(mem, kernel, group_len, n=LO) == E_TOO_LARGE           # the envelope is answered first
    assert ragged(mem, kernel, group_len, lengths="N") == E_NULL         # ... and so are the pointers


def test_at_most_4096_groups_where_the_tier_would_run(mem):
    """Four box slots per lane. Kernel 2 runs the tier, kernel 0 where pn2_fps_large_pays(n, m) on the padded extents says so;
    kernel 1 never does, so its next answer is the alignment check's."""
    from pointnet2_amd import _C
    n64, n128 = 64 * 4096 + 1, 128 * 4096 + 1
    assert _C.lib().pn2_fps_large_pays(n64, 64) == 1 and _C.lib().pn2_fps_large_pays(n64, 4) == 0
    assert ragged(mem, 2, 64, n=n64) == E_TOO_LARGE
    assert ragged(mem, 2, 128, n=n128) == E_TOO_LARGE
    assert ragged(mem, 2, 64, n=HI) == E_TOO_LARGE
    assert ragged(mem, 2, 64, n=n64, ws="M") == E_TOO_LARGE              # before the alignment
    assert ragged(mem, 0, 64, n=n64, m=64) == E_TOO_LARGE                # the rule sends (n, 64) to the tier
    assert ragged(mem, 0, 64, n=n64, m=4, ws="M") == E_ARG               # ... and (n, 4) to the global-memory kernel: no group limit
    assert ragged(mem, 1, 64, n=n64, m=64, ws="M") == E_ARG


@pytest.mark.parametrize("kernel", [None, 0, 1, 2])
def test_a_misaligned_workspace_is_refused_last(mem, kernel):
    assert ragged(mem, kernel, ws="M") == E_ARG
    assert ragged(mem, kernel, ws="M", npoints="N") == E_ARG


def test_the_existing_entries_keep_their_behaviour(mem):
    from pointnet2_amd import _C
    lib = _C.lib()
    assert lib.pn2_farthest_point_sample_ragged(1, LO + 1, 4, mem.F, mem.I, mem.I, mem.F, None) == E_TOO_LARGE
    assert lib.pn2_farthest_point_sample_ragged_counts(1, LO + 1, 4, mem.F, mem.I, mem.I, mem.I, mem.F, None) == E_TOO_LARGE
    assert lib.pn2_farthest_point_sample_ragged_variant(0, 1, LO + 1, 4, mem.F, mem.I, None, mem.I, mem.F, None) == E_TOO_LARGE
    assert lib.pn2_farthest_point_sample_large(1, LO, 4, mem.F, mem.W, mem.I, mem.F, None) == E_TOO_LARGE
    assert lib.pn2_farthest_point_sample_large_ex(7, 1, 20000, 4, mem.F, mem.W, mem.I, mem.F, None) == E_ARG
    assert lib.pn2_fps_large_ws_bytes(2, 20000) == 20 * 2 * 20000        # the ragged entries' workspace: the padded n


def test_the_python_switch():
    import pointnet2_amd as P
    from pointnet2_amd import tf_sampling
    assert P.set_fps_ragged_large is tf_sampling.set_fps_ragged_large
    assert tf_sampling._FPS_RAGGED_LARGE[0] is False                    # opt-in
    assert tf_sampling.FPS_RAGGED_MAX_POINTS == LO and tf_sampling.FPS_RAGGED_LARGE_MAX_POINTS == HI
    try:
        P.set_fps_ragged_large(True)
        assert tf_sampling._FPS_RAGGED_LARGE[0] is True
        P.set_fps_ragged_large()
        assert tf_sampling._FPS_RAGGED_LARGE[0] is False
        for bad in (1, 0, None, "on"):
            with pytest.raises(ValueError):
                P.set_fps_ragged_large(bad)
        assert tf_sampling._FPS_RAGGED_LARGE[0] is False
    finally:
        P.set_fps_ragged_large(False)
