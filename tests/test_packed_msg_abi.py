"""CPU tests of the packed multi-radius entry (include/pn2ops.h "packed batches": pn2_query_ball_group_xyz_msg_packed):
declared and exported, the host-side validation answers before any GPU call in the order the header states, the Python front's
refusals that need no device, and the module's opt-in."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pn2_query_ball_group_xyz_msg_packed"
OK, E_NULL, E_SHAPE, E_ARG, E_TOO_LARGE = 0, -1, -2, -3, -4
BIG = 2 ** 31 // 3 + 1                                        # total 3 > INT_MAX


def test_declared_and_exported():
    from pointnet2_amd import _C
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pn2ops.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pn2_[a-z0-9_]+)\s*\(", txt))
    lib = ctypes.CDLL(_C.LIB_PATH)
    assert NAME in declared and hasattr(lib, NAME) and NAME in _C.EXPORTED


@pytest.fixture(scope="module")
def bufs():
    """Host memory standing in for the device pointers: the calls below return before anything would touch it."""
    f = (ctypes.c_float * 64)()
    i = (ctypes.c_int * 64)()
    keep = [f, i]

    def floats(*v):
        keep.append((ctypes.c_float * len(v))(*v))
        return keep[-1]

    def ints(*v):
        keep.append((ctypes.c_int * len(v))(*v))
        return keep[-1]

    def ptrs(*v):
        keep.append((ctypes.c_void_p * len(v))(*v))
        return keep[-1]
    return ctypes.addressof(f), ctypes.addressof(i), floats, ints, ptrs, keep


def test_validation(bufs):
    """(b, total, nmax, m, nscales, radii, nsamples, xyz1, offsets1, xyz2, subtract, global_idx, idx, pts_cnt, grouped, stream):
    the order of pn2_query_ball_group_xyz_msg_ragged with offsets1 where lengths1 stood, the extents of
    pn2_query_ball_group_xyz_packed"""
    from pointnet2_amd import _C
    F, I, floats, ints, ptrs, _ = bufs
    fn = _C.lib().pn2_query_ball_group_xyz_msg_packed
    R2, N2 = floats(0.1, 0.2), ints(4, 8)
    PI, PC, PG = ptrs(I, I), ptrs(I, I), ptrs(F, F)
    assert fn(1, 8, 8, 4, 0, R2, N2, F, I, F, 1, 0, PI, PC, PG, None) == E_ARG          # nscales outside 1..4, checked first
    assert fn(-1, 0, 0, -1, 5, R2, N2, F, I, F, 1, 0, PI, PC, PG, None) == E_ARG
    assert fn(1, 8, 8, 4, 2, None, N2, F, I, F, 1, 0, PI, PC, PG, None) == E_ARG
    assert fn(1, 8, 8, 4, 2, R2, None, F, I, F, 1, 0, PI, PC, PG, None) == E_ARG
    assert fn(-1, 8, 8, 4, 2, R2, N2, F, I, F, 1, 0, PI, PC, PG, None) == E_SHAPE
    assert fn(1, 8, 0, 4, 2, R2, N2, F, I, F, 1, 0, PI, PC, PG, None) == E_SHAPE
    assert fn(1, 8, 8, -1, 2, R2, N2, F, I, F, 1, 0, PI, PC, PG, None) == E_SHAPE
    assert fn(-1, 8, 8, 4, 2, floats(0.1, 0.0), N2, F, I, F, 1, 0, PI, PC, PG, None) == E_SHAPE   # extents before attributes' values
    assert fn(1, 8, 8, 4, 2, floats(0.1, 0.0), N2, F, I, F, 1, 0, PI, PC, PG, None) == E_ARG
    assert fn(1, 8, 8, 4, 2, floats(-1.0, 0.2), N2, F, I, F, 1, 0, PI, PC, PG, None) == E_ARG
    assert fn(1, 8, 8, 4, 2, R2, ints(4, 0), F, I, F, 1, 0, PI, PC, PG, None) == E_ARG
    assert fn(0, 8, 8, 4, 2, R2, N2, None, None, None, 1, 0, None, None, None, None) == OK   # b = 0 before any pointer is looked at
    assert fn(1, 8, 8, 0, 2, R2, N2, None, None, None, 1, 0, None, None, None, None) == OK   # m = 0 likewise
    assert fn(0, 0, 8, 4, 2, R2, N2, None, None, None, 1, 0, None, None, None, None) == OK   # ... and before total
    assert fn(1, 0, 8, 4, 2, R2, N2, F, I, F, 1, 0, PI, PC, PG, None) == E_SHAPE        # an empty flat array
    assert fn(1, 8, 9, 4, 2, R2, N2, F, I, F, 1, 0, PI, PC, PG, None) == E_SHAPE        # nmax bounds a cloud: never above total
    assert fn(1, 0, 8, 4, 2, R2, N2, F, None, F, 1, 0, PI, PC, PG, None) == E_SHAPE     # total before the offsets
    assert fn(1, 8, 8, 4, 2, R2, N2, F, None, F, 1, 0, PI, PC, PG, None) == E_NULL      # NULL offsets
    assert fn(1, 8, 8, 4, 2, R2, N2, None, None, None, 1, 0, None, None, None, None) == E_NULL
    assert fn(1, 8, 8, 4, 2, R2, N2, F, I, F, 1, 0, None, PC, None, None) == E_NULL     # neither idx nor grouped_xyz
    assert fn(1, 8, 8, 4, 2, R2, N2, F, I, F, 1, 0, ptrs(I, None), PC, ptrs(F, None), None) == E_NULL   # ... for one scale
    assert fn(1, 8, 8, 4, 2, R2, N2, F, None, F, 1, 0, None, PC, None, None) == E_NULL
    assert fn(1, 9000, 8193, 4, 2, R2, N2, F, I, F, 1, 0, PI, PC, PG, None) == E_TOO_LARGE      # beyond the cell kernels' point limit
    assert fn(1, 9000, 8193, 4, 2, R2, N2, F, I, F, 1, 0, None, PC, None, None) == E_NULL      # ... behind the output pointers
    assert fn(1, 8192, 8192, 64, 3, floats(0.1, 0.2, 0.4), ints(16, 32, 127), F, I, F, 1, 0, ptrs(I, I, I), None, ptrs(F, F, F),
              None) == E_TOO_LARGE                                                    # no LDS geometry fits
    assert fn(1, BIG, 8, 4, 2, R2, N2, F, I, F, 1, 0, PI, PC, PG, None) == E_TOO_LARGE         # total 3 > INT_MAX
    assert fn(1, BIG, 8, 4, 2, R2, N2, None, I, None, 1, 0, PI, PC, PG, None) == E_TOO_LARGE   # ... before xyz1 / xyz2
    assert fn(1, 8, 8, 4, 2, R2, N2, None, I, F, 1, 0, PI, PC, PG, None) == E_NULL
    assert fn(1, 8, 8, 4, 2, R2, N2, F, I, None, 1, 0, PI, None, PG, None) == E_NULL


def test_plan_describes_the_packed_launch():
    """the plan entry answers for (b, nmax, m): what the packed entry refuses with PN2_E_TOO_LARGE it reports as -4"""
    from pointnet2_amd.tf_grouping import query_ball_group_xyz_msg_plan as plan
    assert plan([0.1, 0.2, 0.4], [16, 32, 127], 1, 8192, 64)["rc"] == E_TOO_LARGE
    assert plan([0.1, 0.2], [4, 8], 1, 8193, 4)["rc"] == E_TOO_LARGE
    assert plan([0.1, 0.2, 0.4], [16, 32, 126], 4, 8192, 704)["threads"] == 512


def test_front_refusals_need_no_device():
    import pointnet2_amd as P
    flat, q = torch.rand(10, 3), torch.rand(2, 4, 3)
    offs = torch.tensor([0, 6, 10], dtype=torch.int32)
    R, K = [0.2, 0.4], [4, 8]
    with pytest.raises(ValueError, match="offsets and lengths are two layouts"):
        P.query_ball_group_xyz_msg(R, K, flat, q, offsets=offs, max_points=6, lengths1=[6, 4])
    with pytest.raises(ValueError, match="lengths2=.*not offered with offsets"):
        P.query_ball_group_xyz_msg(R, K, flat, q, offsets=offs, max_points=6, lengths2=[4, 4])
    with pytest.raises(ValueError, match="needs max_points"):
        P.query_ball_group_xyz_msg(R, K, flat, q, offsets=offs)
    with pytest.raises(ValueError, match="host int, not a tensor"):
        P.query_ball_group_xyz_msg(R, K, flat, q, offsets=offs, max_points=torch.tensor(6))
    with pytest.raises(ValueError, match=r"one flat \(total, 3\) array"):
        P.query_ball_group_xyz_msg(R, K, flat.view(2, 5, 3), q, offsets=offs, max_points=6)
    with pytest.raises(ValueError, match="offsets"):
        P.query_ball_group_xyz_msg(R, K, flat, q, offsets=torch.tensor([0, 3, 6, 10], dtype=torch.int32), max_points=6)
    # the same messages, in the same order, as the single-radius front's
    for kw in (dict(max_points=6, lengths1=[6, 4]), dict(max_points=6, lengths2=[4, 4]), dict()):
        with pytest.raises(ValueError) as one:
            P.query_ball_group_xyz(0.2, 4, flat, q, offsets=offs, **kw)
        with pytest.raises(ValueError) as msg:
            P.query_ball_group_xyz_msg(R, K, flat, q, offsets=offs, **kw)
        assert str(one.value).replace("query_ball_group_xyz", "query_ball_group_xyz_msg") == str(msg.value)


def test_module_opt_in_is_off_by_default():
    import pointnet2_amd.pointnet_util as U
    mod = U.PointnetSAModuleMSG(6, 16, [0.3, 0.5], [16, 32], [[32, 32, 64], [32, 48, 64]])
    assert mod.packed_batches is False
    flat, offs = torch.rand(10, 3), torch.tensor([0, 6, 10], dtype=torch.int32)
    with pytest.raises(ValueError, match="offsets"):
        mod(flat, None, offsets=offs, max_points=6)
    with pytest.raises(ValueError, match="offsets"):
        mod.packed_geometry(flat, offs, 6)
