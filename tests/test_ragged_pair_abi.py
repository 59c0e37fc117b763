"""CPU tests of the two-sided ragged entries (include/pn2ops.h "ragged batches, the second side"): per-cloud sample counts of
FPS and a ragged query / known side of the pair operators. Declared, exported and bound; the host-side validation answers with
the one-sided twin's codes before any device call, so host memory stands in for every device pointer; the Python operators
refuse a wrong shape of `lengths2` / `npoints` with a ValueError naming the keyword before anything else."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pn2_farthest_point_sample_ragged_counts", "pn2_query_ball_group_xyz_ragged_pair", "pn2_query_ball_group_xyz_msg_ragged_pair",
         "pn2_knn_point_ragged_pair", "pn2_three_nn_ragged_pair"]
TWINS = ["pn2_farthest_point_sample_ragged", "pn2_query_ball_group_xyz_ragged", "pn2_query_ball_group_xyz_msg_ragged",
         "pn2_knn_point_ragged", "pn2_three_nn_ragged"]
COUNT_AT = [5, 8, 9, 7, 6]                  # position of the second count array in the argument list
OK, E_NULL, E_SHAPE, E_ARG, E_TOO_LARGE = 0, -1, -2, -3, -4


@pytest.mark.parametrize("name,twin,at", list(zip(NAMES, TWINS, COUNT_AT)))
def test_declared_exported_and_bound(name, twin, at):
    from pointnet2_amd import _C
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pn2ops.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pn2_[a-z0-9_]+)\s*\(", txt))
    assert name in declared
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), name)
    assert name in _C.EXPORTED
    one = _C._SIGNATURES[twin]
    assert _C._SIGNATURES[name] == one[:at] + [ctypes.c_void_p] + one[at:]        # one more device pointer, nothing else differs


class _Mem:
    def __init__(self):
        self.f = (ctypes.c_float * 256)()
        self.i = (ctypes.c_int * 256)()
        self.F, self.I = ctypes.addressof(self.f), ctypes.addressof(self.i)


@pytest.fixture(scope="module")
def mem():
    return _Mem()


def fps(mem, b=1, n=8, m=4, lengths="I", npoints="I"):
    from pointnet2_amd import _C
    p = dict(I=mem.I, N=None)
    return _C.lib().pn2_farthest_point_sample_ragged_counts(b, n, m, mem.F, p[lengths], p[npoints], mem.I, mem.F, None)


def test_fps_counts_codes(mem):
    assert fps(mem, npoints="N") == E_NULL
    assert fps(mem, lengths="N") == E_NULL
    assert fps(mem, n=0) == E_SHAPE
    assert fps(mem, n=-1) == E_SHAPE
    assert fps(mem, b=-1) == E_SHAPE
    assert fps(mem, n=16385) == E_TOO_LARGE
    assert fps(mem, b=0) == OK
    assert fps(mem, b=0, npoints="N") == OK                 # nothing to do is answered first, as in the twin
    assert fps(mem, m=0) == OK


def bq(mem, b=1, n=8, m=4, radius=0.2, nsample=4, lengths1="I", lengths2="I", kernel=0, qpb=0):
    from pointnet2_amd import _C
    p = dict(I=mem.I, N=None)
    return _C.lib().pn2_query_ball_group_xyz_ragged_pair(b, n, m, radius, nsample, mem.F, p[lengths1], mem.F, p[lengths2], 1, mem.I, mem.I,
                                                         mem.F, kernel, qpb, None)


def test_ball_query_pair_codes(mem):
    assert bq(mem, lengths2="N") == E_NULL
    assert bq(mem, lengths1="N") == E_NULL
    assert bq(mem, n=0) == E_SHAPE
    assert bq(mem, radius=0.0) == E_ARG
    assert bq(mem, radius=-1.0) == E_ARG
    assert bq(mem, nsample=0) == E_ARG
    assert bq(mem, kernel=-1) == E_ARG
    assert bq(mem, kernel=4) == E_ARG
    assert bq(mem, qpb=-1) == E_ARG
    assert bq(mem, b=0) == OK
    assert bq(mem, m=0) == OK
    assert bq(mem, n=0, lengths2="N") == E_SHAPE            # extents before pointers, as in the twin


def msg(mem, b=1, n=8, m=4, radii=(0.2, 0.4), nsamples=(4, 8), lengths1="I", lengths2="I"):
    from pointnet2_amd import _C
    p = dict(I=mem.I, N=None)
    k = len(radii)
    r = (ctypes.c_float * k)(*radii)
    s = (ctypes.c_int * k)(*nsamples)
    pi = (ctypes.c_void_p * k)(*[mem.I] * k)
    pg = (ctypes.c_void_p * k)(*[mem.F] * k)
    return _C.lib().pn2_query_ball_group_xyz_msg_ragged_pair(b, n, m, k, r, s, mem.F, p[lengths1], mem.F, p[lengths2], 1, pi, pi, pg, None)


def test_msg_pair_codes(mem):
    assert msg(mem, lengths2="N") == E_NULL
    assert msg(mem, lengths1="N") == E_NULL
    assert msg(mem, n=0) == E_SHAPE
    assert msg(mem, radii=(0.2, 0.0)) == E_ARG
    assert msg(mem, nsamples=(4, 0)) == E_ARG
    assert msg(mem, b=0) == OK
    assert msg(mem, m=0, lengths2="N") == OK
    assert msg(mem, n=8193) == E_TOO_LARGE


def knn(mem, b=1, n=8, m=4, k=2, lengths1="I", lengths2="I"):
    from pointnet2_amd import _C
    p = dict(I=mem.I, N=None)
    return _C.lib().pn2_knn_point_ragged_pair(b, n, m, k, mem.F, p[lengths1], mem.F, p[lengths2], mem.F, mem.I, None)


def test_knn_pair_codes(mem):
    assert knn(mem, lengths2="N") == E_NULL
    assert knn(mem, lengths1="N") == E_NULL
    assert knn(mem, n=0) == E_SHAPE
    assert knn(mem, k=0) == E_ARG
    assert knn(mem, k=-3) == E_ARG
    assert knn(mem, k=9) == E_TOO_LARGE                     # k > n
    assert knn(mem, n=14337) == E_TOO_LARGE                 # the LDS envelope
    assert knn(mem, b=0) == OK
    assert knn(mem, m=0) == OK


def nn3(mem, b=1, n=8, m=4, variant=0, lengths1="I", lengths2="I"):
    from pointnet2_amd import _C
    p = dict(I=mem.I, N=None)
    return _C.lib().pn2_three_nn_ragged_pair(b, n, m, mem.F, p[lengths1], mem.F, p[lengths2], mem.F, mem.I, variant, None)


def test_three_nn_pair_codes(mem):
    assert nn3(mem, lengths2="N") == E_NULL
    assert nn3(mem, lengths1="N") == E_NULL
    assert nn3(mem, n=0) == E_SHAPE
    assert nn3(mem, variant=-1) == E_ARG
    assert nn3(mem, variant=3) == E_ARG
    assert nn3(mem, variant=2, m=63) == E_ARG               # the cell list exists for 64..8192 PADDED known points
    assert nn3(mem, variant=2, m=8193) == E_ARG
    assert nn3(mem, b=0) == OK


BAD = [([1, 2, 3], "a wrong length"), (torch.zeros(2, 1, dtype=torch.int32), "2-D"), (torch.ones(2), "float"), (5, "a scalar")]


@pytest.mark.parametrize("bad", [b for b, _ in BAD], ids=[i for _, i in BAD])
def test_python_wrappers_refuse_a_wrong_count_shape(bad):
    """b = 2; the check comes before any look at the other tensors (CPU tensors would be refused next), so no GPU is needed"""
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import sample_and_group, three_nn_weights
    x1, x2 = torch.zeros(2, 8, 3), torch.zeros(2, 4, 3)
    calls = {
        "npoints": [lambda: P.farthest_point_sample(4, x1, npoints=bad),
                    lambda: P.farthest_point_sample_gather(4, x1, npoints=bad),
                    lambda: P.farthest_point_sample(4, x1, lengths=[8, 8], npoints=bad),
                    lambda: P.sample_and_group_xyz(4, 0.2, 4, x1, npoints=bad),
                    lambda: sample_and_group(4, 0.2, 4, x1, None, npoints=bad)],
        "lengths2": [lambda: P.query_ball_point(0.2, 4, x1, x2, lengths2=bad),
                     lambda: P.query_ball_group_xyz(0.2, 4, x1, x2, lengths2=bad),
                     lambda: P.query_ball_group_xyz_msg([0.2, 0.4], [4, 4], x1, x2, lengths2=bad),
                     lambda: P.knn_point(2, x1, x2, lengths2=bad),
                     lambda: P.knn_point(2, x1, x2, lengths1=[8, 8], lengths2=bad),
                     lambda: P.three_nn(x1, x2, lengths2=bad),
                     lambda: three_nn_weights(x1, x2, lengths2=bad)],
    }
    for keyword, fns in calls.items():
        for fn in fns:
            with pytest.raises(ValueError, match=keyword):
                fn()
