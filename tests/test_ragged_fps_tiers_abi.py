"""CPU tests of pn2_farthest_point_sample_ragged_variant (include/pn2ops.h): the ragged FPS entries with the tier chosen by the
caller. Declared, exported and bound; the host-side validation answers before any device call -- variant first, then the order and
codes of pn2_farthest_point_sample_ragged, then the forced tier's rank-slot envelope of the PADDED n --, so host memory stands in
for every device pointer. The Python switch set_fps_variant says that it covers ragged calls."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pn2_farthest_point_sample_ragged_variant"
OK, E_NULL, E_SHAPE, E_ARG, E_TOO_LARGE = 0, -1, -2, -3, -4
AUTO, FULL, PRUNED, BATCH = 0, 1, 2, 3


def test_declared_exported_and_bound():
    from pointnet2_amd import _C
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pn2ops.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pn2_[a-z0-9_]+)\s*\(", txt))
    assert NAME in declared
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), NAME)
    assert NAME in _C.EXPORTED
    counts = _C._SIGNATURES["pn2_farthest_point_sample_ragged_counts"]
    assert _C._SIGNATURES[NAME] == [ctypes.c_int] + counts                    # the variant in front, nothing else differs
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_header_no_longer_says_register_tier_only():
    txt = open(os.path.join(ROOT, "include", "pn2ops.h")).read()
    assert "pn2_farthest_point_sample_ragged: the register tier only" not in txt


class _Mem:
    def __init__(self):
        self.f = (ctypes.c_float * 256)()
        self.i = (ctypes.c_int * 256)()
        self.F, self.I = ctypes.addressof(self.f), ctypes.addressof(self.i)


@pytest.fixture(scope="module")
def mem():
    return _Mem()


def fps(mem, variant=AUTO, b=1, n=8, m=4, inp="F", lengths="I", npoints="I", out="I"):
    from pointnet2_amd import _C
    p = dict(I=mem.I, F=mem.F, N=None)
    return _C.lib().pn2_farthest_point_sample_ragged_variant(variant, b, n, m, p[inp], p[lengths], p[npoints], p[out], mem.F, None)


@pytest.mark.parametrize("variant", [-1, 4, 17])
def test_a_variant_out_of_range_is_answered_first(mem, variant):
    assert fps(mem, variant) == E_ARG
    assert fps(mem, variant, b=0) == E_ARG                 # ahead of "nothing to do"
    assert fps(mem, variant, m=0) == E_ARG
    assert fps(mem, variant, n=0) == E_ARG                 # ahead of the extents
    assert fps(mem, variant, lengths="N") == E_ARG         # ahead of the pointers
    assert fps(mem, variant, n=16385) == E_ARG


@pytest.mark.parametrize("variant", [AUTO, FULL, PRUNED, BATCH])
def test_then_the_order_and_codes_of_the_ragged_entry(mem, variant):
    assert fps(mem, variant, b=0) == OK
    assert fps(mem, variant, m=0) == OK
    assert fps(mem, variant, m=-2) == OK
    assert fps(mem, variant, b=0, lengths="N", inp="N") == OK      # nothing to do is answered before the pointers
    assert fps(mem, variant, m=0, n=0) == OK                       # ... and before the extents
    assert fps(mem, variant, n=0) == E_SHAPE
    assert fps(mem, variant, n=-1) == E_SHAPE
    assert fps(mem, variant, b=-1) == E_SHAPE
    assert fps(mem, variant, n=0, lengths="N") == E_SHAPE          # extents before pointers
    assert fps(mem, variant, lengths="N") == E_NULL
    assert fps(mem, variant, inp="N") == E_NULL
    assert fps(mem, variant, out="N") == E_NULL
    assert fps(mem, variant, n=16385) == E_TOO_LARGE
    assert fps(mem, variant, n=16385, lengths="N") == E_NULL       # pointers before the envelope
    assert fps(mem, variant, n=20000, npoints="N") == E_TOO_LARGE  # npoints may be NULL: m samples from every cloud


def test_a_forced_tier_outside_its_rank_slot_envelope(mem):
    """ranks = 512 ceil(n / 512) of the PADDED n: pruned 2049..8192, batched 513..8192; no launch is made for these"""
    for n in (8, 512, 1024, 2048, 8193, 16384):
        assert fps(mem, PRUNED, n=n) == E_ARG
    for n in (8, 512, 8193, 16384):
        assert fps(mem, BATCH, n=n) == E_ARG
    assert fps(mem, PRUNED, n=8193, npoints="N") == E_ARG


def test_the_existing_entries_keep_their_codes(mem):
    from pointnet2_amd import _C
    lib = _C.lib()
    assert lib.pn2_farthest_point_sample_ragged(1, 16385, 4, mem.F, mem.I, mem.I, mem.F, None) == E_TOO_LARGE
    assert lib.pn2_farthest_point_sample_ragged(1, 8, 4, mem.F, None, mem.I, mem.F, None) == E_NULL
    assert lib.pn2_farthest_point_sample_ragged_counts(1, 8, 4, mem.F, mem.I, None, mem.I, mem.F, None) == E_NULL
    assert lib.pn2_farthest_point_sample_ragged_counts(0, 8, 4, mem.F, mem.I, None, mem.I, mem.F, None) == OK


def test_set_fps_variant_covers_ragged_calls():
    from pointnet2_amd import tf_sampling
    doc = tf_sampling.set_fps_variant.__doc__
    assert "lengths=" in doc and "npoints=" in doc and "Does not apply" not in doc
    assert NAME in doc
