"""CPU tests of the ragged-batch entries of the C ABI (include/pn2ops.h "ragged batches": pn2_farthest_point_sample_ragged,
pn2_query_ball_group_xyz_ragged, pn2_knn_point_ragged, pn2_three_nn_ragged): declared and exported, the host-side validation
answers before any GPU call, the Python wrappers refuse a wrong lengths shape, check_lengths refuses bad values."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pn2_farthest_point_sample_ragged", "pn2_query_ball_group_xyz_ragged", "pn2_knn_point_ragged", "pn2_three_nn_ragged"]
OK, E_NULL, E_SHAPE, E_ARG, E_TOO_LARGE = 0, -1, -2, -3, -4


def test_declared_and_exported():
    from pointnet2_amd import _C
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pn2ops.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pn2_[a-z0-9_]+)\s*\(", txt))
    lib = ctypes.CDLL(_C.LIB_PATH)
    for n in NAMES:
        assert n in declared and hasattr(lib, n) and n in _C.EXPORTED, n


@pytest.fixture(scope="module")
def bufs():
    """Host memory standing in for the device pointers: the calls below return before anything would touch it."""
    f = (ctypes.c_float * 64)()
    i = (ctypes.c_int * 64)()
    return ctypes.addressof(f), ctypes.addressof(i), (f, i)


def test_fps_validation(bufs):
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_farthest_point_sample_ragged
    assert fn(1, 8, 4, F, None, I, None, None) == E_NULL                    # NULL lengths
    assert fn(1, 8, 4, None, I, I, None, None) == E_NULL
    assert fn(1, 0, 4, F, I, I, None, None) == E_SHAPE
    assert fn(1, -3, 4, F, I, I, None, None) == E_SHAPE
    assert fn(1, 16385, 4, F, I, I, None, None) == E_TOO_LARGE              # beyond the register tier
    assert fn(0, 8, 4, F, I, I, None, None) == OK
    assert fn(0, 8, 4, None, None, None, None, None) == OK


def test_ball_query_validation(bufs):
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_query_ball_group_xyz_ragged
    assert fn(1, 8, 4, 0.2, 4, F, None, F, 1, I, I, F, 0, 0, None) == E_NULL     # NULL lengths
    assert fn(1, 0, 4, 0.2, 4, F, I, F, 1, I, I, F, 0, 0, None) == E_SHAPE
    assert fn(1, 8, 4, 0.0, 4, F, I, F, 1, I, I, F, 0, 0, None) == E_ARG
    assert fn(1, 8, 4, -1.0, 4, F, I, F, 1, I, I, F, 0, 0, None) == E_ARG
    assert fn(1, 8, 4, 0.2, 0, F, I, F, 1, I, I, F, 0, 0, None) == E_ARG
    assert fn(1, 8, 4, 0.2, 4, F, I, F, 1, I, I, F, 4, 0, None) == E_ARG         # kernel code outside 0..3
    assert fn(0, 8, 4, 0.2, 4, F, I, F, 1, I, I, F, 0, 0, None) == OK


def test_knn_validation(bufs):
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_knn_point_ragged
    assert fn(1, 8, 4, 2, F, None, F, F, I, None) == E_NULL                  # NULL lengths
    assert fn(1, 0, 4, 2, F, I, F, F, I, None) == E_SHAPE
    assert fn(1, 8, 4, 0, F, I, F, F, I, None) == E_ARG
    assert fn(1, 14337, 4, 2, F, I, F, F, I, None) == E_TOO_LARGE
    assert fn(1, 8, 4, 9, F, I, F, F, I, None) == E_TOO_LARGE                # k > the padded n
    assert fn(0, 8, 4, 2, F, I, F, F, I, None) == OK


def test_three_nn_validation(bufs):
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_three_nn_ragged
    assert fn(1, 8, 4, F, None, F, F, I, 0, None) == E_NULL                  # NULL lengths
    assert fn(1, 0, 4, F, I, F, F, I, 0, None) == E_SHAPE
    assert fn(1, 8, 4, F, I, F, F, I, 3, None) == E_ARG                      # variant outside 0..2
    assert fn(1, 8, 4, F, I, F, F, I, 2, None) == E_ARG                      # no cell list below 64 known points
    assert fn(0, 8, 4, F, I, F, F, I, 0, None) == OK


def test_python_wrappers_refuse_a_wrong_lengths_shape():
    """The lengths shape is checked before anything else, so this needs no GPU: (b,) is the only shape."""
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import sample_and_group, three_nn_weights
    xyz, q = torch.zeros(2, 8, 3), torch.zeros(2, 4, 3)
    for bad in ([1, 2, 3], torch.tensor([[1, 2]]), torch.tensor([1.0, 2.0]), torch.tensor(3)):
        calls = [lambda: P.farthest_point_sample(4, xyz, lengths=bad),
                 lambda: P.farthest_point_sample_gather(4, xyz, lengths=bad),
                 lambda: P.query_ball_point(0.2, 4, xyz, q, lengths1=bad),
                 lambda: P.query_ball_group_xyz(0.2, 4, xyz, q, lengths1=bad),
                 lambda: P.knn_point(2, xyz, q, lengths1=bad),
                 lambda: P.three_nn(xyz, q, lengths1=bad),
                 lambda: three_nn_weights(xyz, q, lengths1=bad),
                 lambda: P.sample_and_group_xyz(4, 0.2, 4, xyz, lengths=bad),
                 lambda: sample_and_group(4, 0.2, 4, xyz, None, lengths=bad)]
        for call in calls:
            with pytest.raises(ValueError, match="lengths"):
                call()


def test_operator_fronts_complain_in_the_promised_order():
    """What a front says when several things are wrong at once, on CPU tensors (every call ends in a complaint before a device
    is touched): radius and nsample first of all, then a wrong lengths shape (lengths2 included, every counted front), and only
    then that there is no CPU path."""
    import pointnet2_amd as P
    xyz, q, bad, good = torch.zeros(2, 8, 3), torch.zeros(2, 4, 3), [1, 2, 3], [8, 8]
    for front in (P.query_ball_point, P.query_ball_group_xyz):
        for kw in ({"lengths1": bad}, {"offsets": [0, 8], "max_points": 8}):
            with pytest.raises(ValueError, match="positive radius"):
                front(0.0, 0, xyz, q, **kw)
            with pytest.raises(ValueError, match="positive nsample"):
                front(0.2, 0, xyz, q, **kw)
    with pytest.raises(ValueError, match="positive radius"):
        P.query_ball_group_xyz_msg([0.2, -1.0], [4, 4], xyz, q, lengths1=bad)
    with pytest.raises(ValueError, match="positive nsample"):
        P.query_ball_group_xyz_msg([0.2, 0.3], [4, 0], xyz, q, lengths1=bad)
    counted = [lambda **kw: P.query_ball_point(0.2, 4, xyz, q, **kw), lambda **kw: P.query_ball_group_xyz(0.2, 4, xyz, q, **kw),
               lambda **kw: P.query_ball_group_xyz_msg([0.2, 0.3], [4, 4], xyz, q, **kw), lambda **kw: P.knn_point(2, xyz, q, **kw),
               lambda **kw: P.three_nn(xyz, q, **kw)]
    for front in counted:
        with pytest.raises(ValueError, match=r"lengths1 must have shape \(batch_size,\) = \(2,\)"):
            front(lengths1=bad, lengths2=bad)
        with pytest.raises(ValueError, match=r"lengths2 must have shape \(batch_size,\) = \(2,\)"):
            front(lengths1=good, lengths2=bad)
        with pytest.raises(ValueError, match="xyz1 must live on a ROCm device"):
            front(lengths1=good, lengths2=good)
    with pytest.raises(ValueError, match="lengths2=. is not offered with offsets"):
        P.query_ball_point(0.2, 4, torch.zeros(8, 3), q, offsets=[0, 3, 8], max_points=5, lengths2=good)


def test_pair_counts_is_the_rule_for_the_counted_entry():
    """The one statement of which counted entry a call takes and with which count arrays (host logic; CPU tensors do)."""
    from pointnet2_amd._tensors import pair_counts
    cpu, l1, l2 = torch.device("cpu"), torch.tensor([5, 3], dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32)
    assert pair_counts(None, None, 2, 5, 4, cpu) == ("", None, None, (), ())
    suffix, c1, c2, p1, p2 = pair_counts(l1, None, 2, 5, 4, cpu)
    assert suffix == "_ragged" and c1 is l1 and c2 is None and p1 == (l1.data_ptr(),) and p2 == ()   # int32 in place: handed on
    suffix, c1, c2, p1, p2 = pair_counts(None, l2, 2, 5, 4, cpu)
    assert suffix == "_ragged_pair" and c1.tolist() == [5, 5] and c1.dtype == torch.int32 and c2 is l2
    assert p1 == (c1.data_ptr(),) and p2 == (l2.data_ptr(),)
    suffix, c1, c2, p1, p2 = pair_counts(l1, l2, 2, 5, 4, cpu)
    assert suffix == "_ragged_pair" and c1 is l1 and c2 is l2 and p1 == (l1.data_ptr(),) and p2 == (l2.data_ptr(),)
    suffix, c1, c2, p1, p2 = pair_counts(l1, None, 2, 5, 4, cpu, both=True)          # an entry with no unpaired variant
    assert suffix == "_ragged_pair" and c1 is l1 and c2.tolist() == [4, 4] and p2 == (c2.data_ptr(),)
    with pytest.raises(ValueError, match="npoints must have shape"):
        pair_counts(l1, [1, 2, 3], 2, 5, 4, cpu, ("lengths", "npoints"))


def test_check_lengths():
    import pointnet2_amd as P
    got = P.check_lengths(torch.tensor([1, 8, 5], dtype=torch.int64), 8)
    assert got.dtype == torch.int32 and got.tolist() == [1, 8, 5]
    assert P.check_lengths([8, 1], 8, b=2).tolist() == [8, 1]
    for bad in ([0, 3], [9, 3], torch.tensor([1.0, 2.0]), torch.tensor([[1, 2]]), [-1]):
        with pytest.raises(ValueError):
            P.check_lengths(bad, 8)
    with pytest.raises(ValueError):
        P.check_lengths([1, 2], 8, b=3)                                      # a wrong size
