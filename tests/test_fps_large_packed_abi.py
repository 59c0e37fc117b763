"""CPU tests of the packed large-cloud FPS entries (include/pn2ops.h: pn2_fps_large_packed_ws_bytes,
pn2_farthest_point_sample_large_packed, pn2_farthest_point_sample_large_packed_ex): declared, exported, bound and named in
INTEGRATION.md; the host-side validation answers before any device call and in the documented order, so host memory stands in for
every device pointer and nothing is launched (as in tests/test_fps_large_ragged_abi.py); the register-tier packed entry keeps its
limit; the Python route refuses on CPU tensors before a device is needed."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pn2_farthest_point_sample_large_packed", "pn2_farthest_point_sample_large_packed_ex", "pn2_fps_large_packed_ws_bytes"]
OK, E_NULL, E_SHAPE, E_ARG, E_TOO_LARGE = 0, -1, -2, -3, -4
LO, HI = 16384, 1048576                                   # the envelope: LO < nmax <= HI
BIG = 2 ** 31 // 3 + 1                                    # total 3 > INT_MAX


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
    assert ex == [ctypes.c_int] * 3 + plain                # kernel, group_len and short_max in front, nothing else differs
    i, p = ctypes.c_int, ctypes.c_void_p
    assert plain == [i, i, i, i, p, p, i, p, p, p, p]      # b, total, nmax, m, inp, offsets, global_idx, ws, out, out_xyz, stream
    assert _C._SIGNATURES[NAMES[2]] == [i] and _C._RESTYPES[NAMES[2]] is ctypes.c_longlong


def test_the_workspace_follows_the_flat_array():
    from pointnet2_amd import _C
    lib = _C.lib()
    assert lib.pn2_fps_large_packed_ws_bytes(26000) == 20 * 26000
    assert lib.pn2_fps_large_packed_ws_bytes(1) == 20                        # no envelope: total may be below nmax
    assert lib.pn2_fps_large_packed_ws_bytes(0) == 0 and lib.pn2_fps_large_packed_ws_bytes(-5) == 0
    assert lib.pn2_fps_large_packed_ws_bytes(2 ** 31 - 1) == 20 * (2 ** 31 - 1)   # 64-bit


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


def packed(mem, kernel=None, group_len=256, short_max=-1, b=1, total=30000, nmax=20000, m=4, inp="F", offsets="I", ws="W", out="I",
           global_idx=0):
    """Only ever called with arguments the entry must refuse (or that leave nothing to do): no launch. kernel None = the plain
    entry."""
    from pointnet2_amd import _C
    p = dict(I=mem.I, F=mem.F, W=mem.W, M=mem.W + 4, N=None)
    tail = (b, total, nmax, m, p[inp], p[offsets], global_idx, p[ws], p[out], mem.F, None)
    if kernel is None:
        return _C.lib().pn2_farthest_point_sample_large_packed(*tail)
    return _C.lib().pn2_farthest_point_sample_large_packed_ex(kernel, group_len, short_max, *tail)


# (kernel, group_len, short_max): the plain entry, every kernel, and values the fifth check refuses -- the earlier checks answer first
@pytest.mark.parametrize("kernel,group_len,short_max", [(None, 256, -1), (0, 256, -1), (1, 64, 0), (2, 128, 8192), (2, 256, 1), (7, 256, -1),
                                                        (-1, 64, 0), (2, 7, 0), (1, 0, -1), (2, 256, -2), (2, 256, 8193)])
def test_codes_in_the_documented_order(mem, kernel, group_len, short_max):
    def call(**kw):
        return packed(mem, kernel, group_len, short_max, **kw)
    # 1 nothing to do: before the extents, the pointers, the envelope and the three choices
    assert call(b=0) == OK
    assert call(m=0) == OK
    assert call(m=-3) == OK
    assert call(m=0, nmax=0, total=0) == OK
    assert call(b=0, inp="N", offsets="N", ws="N", out="N") == OK
    assert call(b=0, nmax=5) == OK
    # 2 extents: before the pointers and the envelope
    assert call(nmax=0) == E_SHAPE
    assert call(nmax=-1) == E_SHAPE
    assert call(b=-1) == E_SHAPE
    assert call(total=0) == E_SHAPE
    assert call(total=-4) == E_SHAPE
    assert call(total=0, inp="N", offsets="N") == E_SHAPE
    # 3 pointers: before the envelope
    assert call(inp="N") == E_NULL
    assert call(out="N") == E_NULL
    assert call(ws="N") == E_NULL
    assert call(offsets="N") == E_NULL
    assert call(nmax=8, offsets="N") == E_NULL
    assert call(nmax=HI + 1, ws="N") == E_NULL
    # 4 the envelope and the int32 extents: before kernel, group_len, short_max and the alignment
    assert call(nmax=8) == E_TOO_LARGE
    assert call(nmax=LO) == E_TOO_LARGE
    assert call(nmax=HI + 1) == E_TOO_LARGE
    assert call(nmax=LO, ws="M") == E_TOO_LARGE
    assert call(total=BIG) == E_TOO_LARGE                               # total 3 beyond int32
    assert call(b=2, m=400000000) == E_TOO_LARGE                        # b m 3 beyond int32
    assert call(total=5, nmax=LO) == E_TOO_LARGE                        # total below nmax is no error of its own


@pytest.mark.parametrize("kernel,group_len,short_max", [(-1, 256, -1), (3, 256, 0), (7, 64, 8192), (0, 0, -1), (1, 63, 0), (2, 192, 0),
                                                        (0, 512, -1), (1, -1, 0), (5, 5, 5),
                                                        (2, 256, -2), (2, 256, 8193), (0, 64, -2), (1, 128, 8193), (2, 64, 1 << 20)])
def test_a_kernel_group_len_or_short_max_out_of_range(mem, kernel, group_len, short_max):
    """short_max: -1 (the rule), 0 (never) and 1 .. 8192 are the values; -2 and 8193 are refused -- from kernel 1 too, which
    ignores only a VALID value."""
    assert packed(mem, kernel, group_len, short_max) == E_ARG
    assert packed(mem, kernel, group_len, short_max, nmax=LO + 1, total=7) == E_ARG
    assert packed(mem, kernel, group_len, short_max, nmax=HI) == E_ARG        # ... before the group count
    assert packed(mem, kernel, group_len, short_max, ws="M") == E_ARG         # ... and the alignment
    assert packed(mem, kernel, group_len, short_max, nmax=LO) == E_TOO_LARGE  # the envelope is answered first
    assert packed(mem, kernel, group_len, short_max, offsets="N") == E_NULL   # ... and so are the pointers


@pytest.mark.parametrize("short_max", [-1, 0, 1, 1024, 8192])
def test_every_valid_short_max_goes_on_to_the_alignment_check(mem, short_max):
    for kernel in (0, 1, 2):
        assert packed(mem, kernel, 256, short_max, ws="M") == E_ARG
        # ... behind the group limit, which a valid short_max does not move: kernel 1 has none
        assert packed(mem, kernel, 64, short_max, nmax=64 * 4096 + 1, total=300000, m=64, ws="M") == (E_ARG if kernel == 1 else E_TOO_LARGE)


def test_at_most_4096_groups_where_the_tier_would_run(mem):
    """Four box slots per lane. Kernel 2 runs the tier, kernel 0 where pn2_fps_large_pays(nmax, m) says so; kernel 1 never does,
    so its next answer is the alignment check's."""
    from pointnet2_amd import _C
    n64, n128 = 64 * 4096 + 1, 128 * 4096 + 1
    assert _C.lib().pn2_fps_large_pays(n64, 64) == 1 and _C.lib().pn2_fps_large_pays(n64, 4) == 0
    assert packed(mem, 2, 64, nmax=n64) == E_TOO_LARGE
    assert packed(mem, 2, 128, nmax=n128) == E_TOO_LARGE
    assert packed(mem, 2, 64, nmax=HI) == E_TOO_LARGE
    assert packed(mem, 2, 64, nmax=n64, total=100) == E_TOO_LARGE             # on nmax, whatever the flat array holds
    assert packed(mem, 2, 64, nmax=n64, ws="M") == E_TOO_LARGE                # before the alignment
    assert packed(mem, 0, 64, nmax=n64, m=64) == E_TOO_LARGE                  # the rule sends (nmax, 64) to the tier
    assert packed(mem, 0, 64, nmax=n64, m=4, ws="M") == E_ARG                 # ... and (nmax, 4) to the global-memory kernel: no group limit
    assert packed(mem, 1, 64, nmax=n64, m=64, ws="M") == E_ARG
    assert packed(mem, 2, 256, nmax=HI, ws="M") == E_ARG                      # 4096 groups of 256: inside


@pytest.mark.parametrize("kernel", [None, 0, 1, 2])
def test_a_misaligned_workspace_is_refused_last(mem, kernel):
    assert packed(mem, kernel, ws="M") == E_ARG
    assert packed(mem, kernel, ws="M", global_idx=1) == E_ARG


def test_the_register_tier_entry_keeps_its_limit(mem):
    from pointnet2_amd import _C
    fn = _C.lib().pn2_farthest_point_sample_packed
    assert fn(0, 1, 8, LO + 1, 4, mem.F, mem.I, 0, mem.I, None, None) == E_TOO_LARGE
    assert fn(0, 1, 30000, 20000, 4, mem.F, mem.I, 1, mem.I, mem.F, None) == E_TOO_LARGE


def test_the_python_route_refuses_on_cpu_tensors():
    """Switch off: the old ValueError. Switch on: max_points beyond 1048576 is refused by name; a forced tier keeps the 16384
    limit. All before a device is needed."""
    import pointnet2_amd as P
    from pointnet2_amd import tf_sampling as T
    flat, offs = torch.zeros(8, 3), [0, 3, 8]
    before = (T._FPS_RAGGED_LARGE[0], T._FPS_VARIANT[0])
    try:
        P.set_fps_ragged_large(False)
        for fn in (P.farthest_point_sample, P.farthest_point_sample_gather):
            with pytest.raises(ValueError, match="at most 16384 points per cloud"):
                fn(4, flat, offsets=offs, max_points=16385)
            with pytest.raises(ValueError, match="offsets|max_points"):
                fn(4, flat, offsets=offs, max_points=20000)
        P.set_fps_ragged_large(True)
        for fn in (P.farthest_point_sample, P.farthest_point_sample_gather):
            with pytest.raises(ValueError, match="at most 1048576 points per cloud"):
                fn(4, flat, offsets=offs, max_points=HI + 1)
        for variant in (1, 2, 3):
            T.set_fps_variant(variant)
            with pytest.raises(ValueError, match="at most 16384 points per cloud"):
                P.farthest_point_sample(4, flat, offsets=offs, max_points=20000)
        T.set_fps_variant(0)
        with pytest.raises(ValueError, match="npoints"):                      # still not offered with offsets
            P.farthest_point_sample(4, flat, offsets=offs, max_points=20000, npoints=[2, 2])
    finally:
        P.set_fps_ragged_large(before[0])
        T.set_fps_variant(before[1])
    assert "both" in T.set_fps_ragged_large.__doc__.lower()                   # the switch covers both variable-size layouts
