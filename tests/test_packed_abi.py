"""CPU tests of the packed-batch entries of the C ABI (include/pn2ops.h "packed batches": pn2_farthest_point_sample_packed,
pn2_query_ball_group_xyz_packed, pn2_three_nn_packed): declared and exported, the host-side validation answers before any GPU
call in the order the header states, the Python helpers of the layout (packed_offsets, check_offsets, pack_batch,
unpack_batch) and the wrappers' refusals that need no device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pn2_farthest_point_sample_packed", "pn2_query_ball_group_xyz_packed", "pn2_three_nn_packed"]
OK, E_NULL, E_SHAPE, E_ARG, E_TOO_LARGE = 0, -1, -2, -3, -4
BIG = 2 ** 31 // 3 + 1                                        # total 3 > INT_MAX


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
    """(variant, b, total, nmax, m, inp, offsets, global_idx, out, out_xyz, stream)"""
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_farthest_point_sample_packed
    assert fn(4, 1, 8, 8, 4, F, I, 0, I, None, None) == E_ARG                # variant outside 0..3, checked first
    assert fn(-1, 0, 8, 8, 4, None, None, 0, None, None, None) == E_ARG
    assert fn(0, 0, 8, 8, 4, None, None, 0, None, None, None) == OK          # b = 0 before any pointer is looked at
    assert fn(0, 1, 8, 8, 0, None, None, 0, None, None, None) == OK          # m = 0 likewise
    assert fn(0, -1, 8, 8, 4, F, I, 0, I, None, None) == E_SHAPE
    assert fn(0, 1, 8, 0, 4, F, I, 0, I, None, None) == E_SHAPE
    assert fn(0, 1, 0, 8, 4, F, I, 0, I, None, None) == E_SHAPE              # an empty flat array
    assert fn(0, 1, 8, 8, 4, F, None, 0, I, None, None) == E_NULL            # NULL offsets
    assert fn(0, 1, 8, 8, 4, None, I, 0, I, None, None) == E_NULL
    assert fn(0, 1, 8, 8, 4, F, I, 1, None, None, None) == E_NULL
    assert fn(0, 1, 8, 16385, 4, F, I, 0, I, None, None) == E_TOO_LARGE      # beyond the register tiers
    assert fn(0, 1, BIG, 8, 4, F, I, 0, I, None, None) == E_TOO_LARGE        # total 3 > INT_MAX
    assert fn(2, 1, 8, 8, 4, F, I, 0, I, None, None) == E_ARG                # the pruned tier below its rank-slot envelope
    assert fn(3, 1, 9000, 9000, 4, F, I, 0, I, None, None) == E_ARG          # the batched tier above it


def test_ball_query_validation(bufs):
    """(b, total, nmax, m, radius, nsample, xyz1, offsets1, xyz2, subtract, global_idx, idx, pts_cnt, grouped, kernel, qpb, stream)"""
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_query_ball_group_xyz_packed
    assert fn(1, 8, 8, 4, 0.2, 4, F, I, F, 1, 0, I, I, F, 4, 0, None) == E_ARG        # kernel code outside 0..3
    assert fn(1, 8, 8, 4, 0.2, 4, F, I, F, 1, 0, I, I, F, 0, -1, None) == E_ARG
    assert fn(1, 8, 8, 4, 0.0, 4, F, I, F, 1, 0, I, I, F, 0, 0, None) == E_ARG
    assert fn(1, 8, 8, 4, -1.0, 4, F, I, F, 1, 0, I, I, F, 0, 0, None) == E_ARG
    assert fn(1, 8, 8, 4, 0.2, 0, F, I, F, 1, 0, I, I, F, 0, 0, None) == E_ARG
    assert fn(-1, 8, 8, 4, 0.2, 4, F, I, F, 1, 0, I, I, F, 0, 0, None) == E_SHAPE
    assert fn(1, 8, 0, 4, 0.2, 4, F, I, F, 1, 0, I, I, F, 0, 0, None) == E_SHAPE
    assert fn(1, 8, 8, -1, 0.2, 4, F, I, F, 1, 0, I, I, F, 0, 0, None) == E_SHAPE
    assert fn(0, 8, 8, 4, 0.2, 4, None, None, None, 1, 0, None, None, None, 0, 0, None) == OK
    assert fn(1, 8, 8, 0, 0.2, 4, None, None, None, 1, 0, None, None, None, 0, 0, None) == OK
    assert fn(1, 0, 8, 4, 0.2, 4, F, I, F, 1, 0, I, I, F, 0, 0, None) == E_SHAPE
    assert fn(1, 8, 8, 4, 0.2, 4, F, None, F, 1, 0, I, I, F, 0, 0, None) == E_NULL    # NULL offsets
    assert fn(1, 8, 8, 4, 0.2, 4, None, I, F, 1, 0, I, I, F, 0, 0, None) == E_NULL
    assert fn(1, 8, 8, 4, 0.2, 4, F, I, None, 1, 0, I, I, F, 0, 0, None) == E_NULL
    assert fn(1, 8, 8, 4, 0.2, 4, F, I, F, 0, 1, None, I, None, 0, 0, None) == E_NULL  # neither idx nor grouped_xyz
    assert fn(1, BIG, 8, 4, 0.2, 4, F, I, F, 1, 0, I, I, F, 0, 0, None) == E_TOO_LARGE


def test_three_nn_validation(bufs):
    """(b, total, nmax, m, xyz1, offsets1, xyz2, lengths2, global_idx, dist, idx, variant, stream)"""
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_three_nn_packed
    assert fn(1, 8, 8, 4, F, I, F, None, 0, F, I, 3, None) == E_ARG          # variant outside 0..2
    assert fn(-1, 8, 8, 4, F, I, F, None, 0, F, I, 0, None) == E_SHAPE
    assert fn(1, 8, 0, 4, F, I, F, None, 0, F, I, 0, None) == E_SHAPE
    assert fn(1, 8, 8, -1, F, I, F, None, 0, F, I, 0, None) == E_SHAPE
    assert fn(0, 8, 8, 4, None, None, None, None, 0, None, None, 0, None) == OK
    assert fn(1, 0, 8, 4, F, I, F, None, 0, F, I, 0, None) == E_SHAPE
    assert fn(1, 8, 8, 4, F, None, F, None, 0, F, I, 0, None) == E_NULL      # NULL offsets
    assert fn(1, BIG, 8, 4, F, I, F, None, 0, F, I, 0, None) == E_TOO_LARGE
    assert fn(1, 8, 8, 4, None, I, F, None, 0, F, I, 0, None) == E_NULL
    assert fn(1, 8, 8, 4, F, I, None, None, 0, F, I, 0, None) == E_NULL
    assert fn(1, 8, 8, 4, F, I, F, None, 1, None, I, 0, None) == E_NULL
    assert fn(1, 8, 8, 4, F, I, F, None, 0, F, I, 2, None) == E_ARG          # no cell list below 64 known points


def test_pack_batch_round_trip():
    import pointnet2_amd as P
    torch.manual_seed(0)
    padded = torch.rand(4, 9, 3)
    lengths = [9, 1, 4, 7]
    flat, offsets = P.pack_batch(padded, lengths)
    assert flat.shape == (21, 3) and offsets.dtype == torch.int32 and offsets.tolist() == [0, 9, 10, 14, 21]
    for c, n in enumerate(lengths):
        assert torch.equal(flat[offsets[c]:offsets[c + 1]], padded[c, :n])
    back, lens = P.unpack_batch(flat, offsets, n=9, fill=-1.0)
    assert lens.dtype == torch.int32 and lens.tolist() == lengths
    for c, n in enumerate(lengths):
        assert torch.equal(back[c, :n], padded[c, :n]) and bool((back[c, n:] == -1.0).all())
    assert P.unpack_batch(flat, offsets)[0].shape == (4, 9, 3)               # n defaults to the longest cloud
    f2, o2 = P.pack_batch(*P.unpack_batch(flat, offsets))
    assert torch.equal(f2, flat) and torch.equal(o2, offsets)
    with pytest.raises(ValueError):
        P.unpack_batch(flat, offsets, n=8)                                   # below the longest cloud
    with pytest.raises(ValueError):
        P.pack_batch(padded, [9, 0, 4, 7])                                   # check_lengths' rules
    with pytest.raises(ValueError):
        P.pack_batch(padded[0], [9])


def test_packed_offsets_errors():
    import pointnet2_amd as P
    cpu = torch.device("cpu")
    got = P.packed_offsets([0, 3, 8], cpu)
    assert got.dtype == torch.int32 and got.tolist() == [0, 3, 8]
    assert P.packed_offsets(torch.tensor([0, 3, 8]), cpu, b=2).dtype == torch.int32     # int64 is converted
    for bad in (torch.tensor([0.0, 3.0]), torch.tensor([[0, 3]]), torch.tensor(3), "abc", []):
        with pytest.raises(ValueError, match="offsets"):
            P.packed_offsets(bad, cpu)
    with pytest.raises(ValueError, match="offsets"):
        P.packed_offsets([0, 3, 8], cpu, b=3)                                # (b + 1,) is the only shape


def test_check_offsets():
    import pointnet2_amd as P
    got = P.check_offsets(torch.tensor([0, 3, 8], dtype=torch.int64), 8, 5)
    assert got.dtype == torch.int32 and got.tolist() == [0, 3, 8]
    assert P.check_offsets([0, 8], 8).tolist() == [0, 8]
    for bad, total, nmax in (([1, 3, 8], 8, None), ([0, 3, 7], 8, None), ([0, 3, 3, 8], 8, None), ([0, 5, 3, 8], 8, None),
                             ([0, 3, 8], 8, 4), ([0], 8, None), (torch.tensor([0.0, 8.0]), 8, None), ([0, 8], 0, None)):
        with pytest.raises(ValueError):
            P.check_offsets(bad, total, nmax)


def test_python_wrappers_refuse_before_any_launch():
    """offsets with lengths, a missing or tensor-valued max_points, a coordinate argument that is not (total, 3), a wrong
    offsets shape: all ValueError, checked before a device is needed."""
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import sample_and_group
    flat, q, offs = torch.zeros(8, 3), torch.zeros(2, 4, 3), [0, 3, 8]
    calls = [lambda: P.farthest_point_sample(4, flat, offsets=offs, max_points=5, lengths=[3, 5]),
             lambda: P.farthest_point_sample_gather(4, flat, offsets=offs, max_points=5, lengths=[3, 5]),
             lambda: P.query_ball_point(0.2, 4, flat, q, offsets=offs, max_points=5, lengths1=[3, 5]),
             lambda: P.query_ball_group_xyz(0.2, 4, flat, q, offsets=offs, max_points=5, lengths1=[3, 5]),
             lambda: P.three_nn(flat, q, offsets1=offs, max_points1=5, lengths1=[3, 5]),
             lambda: sample_and_group(4, 0.2, 4, flat, None, offsets=offs, max_points=5, lengths=[3, 5]),
             lambda: P.farthest_point_sample(4, flat, offsets=offs),                                  # max_points is required
             lambda: P.query_ball_point(0.2, 4, flat, q, offsets=offs),
             lambda: P.three_nn(flat, q, offsets1=offs),
             lambda: P.farthest_point_sample(4, flat, offsets=offs, max_points=torch.tensor(5)),      # a host int
             lambda: P.farthest_point_sample(4, flat.view(1, 8, 3), offsets=offs, max_points=5),      # (total, 3)
             lambda: P.query_ball_point(0.2, 4, flat, q, offsets=[0, 8], max_points=8),               # (b + 1,) against xyz2's b
             lambda: P.three_nn(flat, q, offsets1=[0, 2, 5, 8], max_points1=8),
             lambda: P.farthest_point_sample(4, flat, offsets=offs, max_points=16385),
             lambda: sample_and_group(4, 0.2, 4, flat, None, knn=True, offsets=offs, max_points=5)]
    for call in calls:
        with pytest.raises(ValueError, match="offsets|max_points"):          # (not the "no CPU path" message: checked before it)
            call()
