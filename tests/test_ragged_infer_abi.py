"""CPU tests of the ragged inference entries (include/pn2ops.h "ragged inference"): the fused MLPs with count arrays and the
one-call ragged levels. Declared, exported and bound; each signature is its dense twin's plus the count pointers at the stated
positions; the host-side validation answers before any device call, so host memory stands in for every device pointer."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pn2_sa_mlp3_maxpool_ragged", "pn2_fp_mlp_ragged", "pn2_sa_level_ragged", "pn2_fp_level_ragged"]
OK, E_NULL, E_SHAPE, E_ARG, E_TOO_LARGE = 0, -1, -2, -3, -4
VP = ctypes.c_void_p


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(name):
    from pointnet2_amd import _C
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pn2ops.h")).read(), flags=re.S)
    assert name in set(re.findall(r"\b(pn2_[a-z0-9_]+)\s*\(", txt))
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)
    assert name in _C.EXPORTED


def test_signatures_are_the_dense_twins_plus_the_counts():
    from pointnet2_amd import _C
    sig = _C._SIGNATURES
    ex = sig["pn2_sa_mlp3_maxpool_ex"]               # (b, n, m, nsample, cfeat, xyz | new_xyz | points, idx, ...)
    assert sig["pn2_sa_mlp3_maxpool_ragged"] == ex[:6] + [VP] + ex[6:7] + [VP] + ex[7:]      # lengths after xyz, npoints after new_xyz
    fp = sig["pn2_fp_mlp"]                           # (b, n, m, c2, c1, points2, points1 | idx, dist, ...)
    assert sig["pn2_fp_mlp_ragged"] == fp[:7] + [VP] + fp[7:]                                # lengths1 after points1
    lvl = sig["pn2_sa_level"]                        # (b, n, m, radius, nsample, cfeat, xyz, points, ws_sample, generation, fps_temp, c1, ...)
    assert sig["pn2_sa_level_ragged"] == lvl[:7] + [VP, VP] + lvl[7:8] + lvl[11:]            # + lengths, npoints; no workspace, generation, temp
    fl = sig["pn2_fp_level"]                         # (b, n, m, c2, c1, xyz1 | xyz2 | points2, ...)
    assert sig["pn2_fp_level_ragged"] == fl[:6] + [VP] + fl[6:7] + [VP] + fl[7:]             # lengths1 after xyz1, lengths2 after xyz2


class _Mem:
    def __init__(self):
        self.f = (ctypes.c_float * 256)()
        self.i = (ctypes.c_int * 256)()
        self.F, self.I = ctypes.addressof(self.f), ctypes.addressof(self.i)


@pytest.fixture(scope="module")
def mem():
    return _Mem()


def sa(mem, b=1, n=8, m=4, nsample=4, lengths="I", npoints="I", group_all=False, widths=(64, 64, 128), variant=0):
    from pointnet2_amd import _C
    p = dict(I=mem.I, N=None)
    new_xyz, idx = (None, None) if group_all else (mem.F, mem.I)
    if group_all:
        m, nsample = 1, n
    return _C.lib().pn2_sa_mlp3_maxpool_ragged(b, n, m, nsample, 0, mem.F, p[lengths], new_xyz, p[npoints], None, idx, widths[0],
                                               widths[1], widths[2], mem.F, mem.F, mem.F, mem.F, variant, None)


def test_sa_mlp_ragged_codes(mem):
    assert sa(mem, npoints="N") == E_NULL                                   # the grouped form needs npoints
    assert sa(mem, lengths="N", b=0) == OK
    assert sa(mem, group_all=True, lengths="N", npoints="N", widths=(256, 256, 512)) == E_NULL      # group_all needs lengths
    assert sa(mem, group_all=True, widths=(256, 256, 512)) == E_ARG          # ... and takes no npoints
    assert sa(mem, nsample=0) == E_ARG
    assert sa(mem, n=0) == E_SHAPE
    assert sa(mem, n=0, npoints="N") == E_SHAPE                             # extents before pointers, as in the dense entry
    assert sa(mem, b=0, lengths="N", npoints="N") == OK                     # nothing to do is answered first
    assert sa(mem, m=0, npoints="N") == OK
    assert sa(mem, variant=4) == E_ARG
    assert sa(mem, widths=(2048, 2048, 2048)) == E_TOO_LARGE                # no kernel for the stack, as in the dense entry


def fp(mem, b=1, n=8, m=4, lengths1="I", kind=0):
    from pointnet2_amd import _C
    p = dict(I=mem.I, N=None)
    widths = (ctypes.c_int * 2)(128, 128)
    return _C.lib().pn2_fp_mlp_ragged(b, n, m, 16, 0, mem.F, None, p[lengths1], mem.I, mem.F, 2, widths, kind, mem.F, mem.F, mem.F,
                                      mem.F, None)


def test_fp_mlp_ragged_codes(mem):
    assert fp(mem, lengths1="N") == E_NULL
    assert fp(mem, lengths1="N", kind=1) == E_NULL
    assert fp(mem, m=0) == E_SHAPE
    assert fp(mem, kind=2) == E_ARG
    assert fp(mem, b=0, lengths1="N") == OK


def sa_level(mem, b=1, n=8, m=4, radius=0.2, nsample=4, lengths="I", npoints="I"):
    from pointnet2_amd import _C
    p = dict(I=mem.I, N=None)
    return _C.lib().pn2_sa_level_ragged(b, n, m, radius, nsample, 0, mem.F, p[lengths], p[npoints], None, 64, 64, 128, mem.F, mem.F,
                                        mem.I, mem.F, mem.I, mem.I, mem.F, mem.F, None, None)


def fp_level(mem, b=1, n=8, m=4, lengths1="I", lengths2="I"):
    from pointnet2_amd import _C
    p = dict(I=mem.I, N=None)
    widths = (ctypes.c_int * 2)(128, 128)
    return _C.lib().pn2_fp_level_ragged(b, n, m, 16, 0, mem.F, p[lengths1], mem.F, p[lengths2], mem.F, None, 2, widths, 0, mem.F, mem.F,
                                        mem.F, mem.I, mem.F, mem.F, None)


def test_level_entries_return_their_first_failing_parts_code(mem):
    assert sa_level(mem, lengths="N") == E_NULL          # FPS with counts
    assert sa_level(mem, npoints="N") == E_NULL
    assert sa_level(mem, n=0) == E_SHAPE
    assert sa_level(mem, n=16385) == E_TOO_LARGE
    assert sa_level(mem, b=0) == OK                      # every part has nothing to do
    assert fp_level(mem, lengths1="N") == E_NULL         # three_nn on both ragged sides
    assert fp_level(mem, lengths2="N") == E_NULL
    assert fp_level(mem, n=0) == E_SHAPE
    assert fp_level(mem, b=0) == OK
