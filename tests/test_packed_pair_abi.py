"""CPU tests of the second side of packed batches (include/pn2ops.h "the second side, packed":
pn2_farthest_point_sample_packed_counts, pn2_query_ball_group_xyz_packed_pair, pn2_query_ball_group_xyz_msg_packed_pair,
pn2_knn_point_packed): declared and exported, the host-side validation answers before any GPU call in the order the header
states, and the Python switch set_packed_pairs -- off, every refusal stands word for word; on, the same calls get past it to the
first check that needs a device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pn2_farthest_point_sample_packed_counts", "pn2_query_ball_group_xyz_packed_pair", "pn2_query_ball_group_xyz_msg_packed_pair",
         "pn2_knn_point_packed"]
OK, E_NULL, E_SHAPE, E_ARG, E_TOO_LARGE = 0, -1, -2, -3, -4
BIG = 2 ** 31 // 3 + 1                                        # total 3 > INT_MAX
NO_DEVICE = "must live on a ROCm device"


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


def test_fps_counts_validation(bufs):
    """(variant, b, total, nmax, m, inp, offsets, npoints, global_idx, out, out_xyz, stream): pn2_farthest_point_sample_packed's
    order, npoints required beside the offsets"""
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_farthest_point_sample_packed_counts
    assert fn(4, 1, 8, 8, 4, F, I, I, 0, I, None, None) == E_ARG             # variant outside 0..3, checked first
    assert fn(-1, 0, 8, 8, 4, None, None, None, 0, None, None, None) == E_ARG
    assert fn(0, 0, 8, 8, 4, None, None, None, 0, None, None, None) == OK    # b = 0 before any pointer is looked at
    assert fn(0, 1, 8, 8, 0, None, None, None, 0, None, None, None) == OK    # m = 0 likewise
    assert fn(0, -1, 8, 8, 4, F, I, I, 0, I, None, None) == E_SHAPE
    assert fn(0, 1, 8, 0, 4, F, I, I, 0, I, None, None) == E_SHAPE
    assert fn(0, 1, 0, 8, 4, F, I, I, 0, I, None, None) == E_SHAPE           # an empty flat array
    assert fn(0, 1, 8, 8, 4, F, None, I, 0, I, None, None) == E_NULL         # NULL offsets
    assert fn(0, 1, 8, 8, 4, F, I, None, 0, I, None, None) == E_NULL         # NULL npoints: required here
    assert fn(0, 1, 8, 8, 4, None, I, I, 0, I, None, None) == E_NULL
    assert fn(0, 1, 8, 8, 4, F, I, I, 1, None, None, None) == E_NULL
    assert fn(0, 1, 8, 16385, 4, F, I, I, 0, I, None, None) == E_TOO_LARGE   # beyond the register tiers
    assert fn(0, 1, 8, 16385, 4, F, I, None, 0, I, None, None) == E_NULL     # ... behind the pointers
    assert fn(0, 1, BIG, 8, 4, F, I, I, 0, I, None, None) == E_TOO_LARGE     # total 3 > INT_MAX
    assert fn(2, 1, 8, 8, 4, F, I, I, 0, I, None, None) == E_ARG             # the pruned tier below its rank-slot envelope
    assert fn(3, 1, 9000, 9000, 4, F, I, I, 0, I, None, None) == E_ARG       # the batched tier above it
    one_sided = _C.lib().pn2_farthest_point_sample_packed                   # the existing entry keeps its envelope
    assert one_sided(0, 1, 8, 16385, 4, F, I, 0, I, None, None) == E_TOO_LARGE


def test_ball_query_pair_validation(bufs):
    """(b, total, nmax, m, radius, nsample, xyz1, offsets1, xyz2, lengths2, subtract, global_idx, idx, pts_cnt, grouped, kernel, qpb,
    stream)"""
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_query_ball_group_xyz_packed_pair
    assert fn(1, 8, 8, 4, 0.2, 4, F, I, F, I, 1, 0, I, I, F, 4, 0, None) == E_ARG        # kernel code outside 0..3
    assert fn(1, 8, 8, 4, 0.2, 4, F, I, F, I, 1, 0, I, I, F, 0, -1, None) == E_ARG
    assert fn(1, 8, 8, 4, 0.0, 4, F, I, F, I, 1, 0, I, I, F, 0, 0, None) == E_ARG
    assert fn(1, 8, 8, 4, 0.2, 0, F, I, F, I, 1, 0, I, I, F, 0, 0, None) == E_ARG
    assert fn(-1, 8, 8, 4, 0.2, 4, F, I, F, I, 1, 0, I, I, F, 0, 0, None) == E_SHAPE
    assert fn(1, 8, 0, 4, 0.2, 4, F, I, F, I, 1, 0, I, I, F, 0, 0, None) == E_SHAPE
    assert fn(1, 8, 8, -1, 0.2, 4, F, I, F, I, 1, 0, I, I, F, 0, 0, None) == E_SHAPE
    assert fn(0, 8, 8, 4, 0.2, 4, None, None, None, None, 1, 0, None, None, None, 0, 0, None) == OK
    assert fn(1, 8, 8, 0, 0.2, 4, None, None, None, None, 1, 0, None, None, None, 0, 0, None) == OK
    assert fn(1, 0, 8, 4, 0.2, 4, F, I, F, I, 1, 0, I, I, F, 0, 0, None) == E_SHAPE
    assert fn(1, 8, 8, 4, 0.2, 4, F, None, F, I, 1, 0, I, I, F, 0, 0, None) == E_NULL    # NULL offsets
    assert fn(1, 8, 8, 4, 0.2, 4, F, I, F, None, 1, 0, I, I, F, 0, 0, None) == E_NULL    # NULL lengths2: required here
    assert fn(1, 8, 8, 4, 0.2, 4, None, I, F, I, 1, 0, I, I, F, 0, 0, None) == E_NULL
    assert fn(1, 8, 8, 4, 0.2, 4, F, I, None, I, 1, 0, I, I, F, 0, 0, None) == E_NULL
    assert fn(1, 8, 8, 4, 0.2, 4, F, I, F, I, 0, 1, None, I, None, 0, 0, None) == E_NULL  # neither idx nor grouped_xyz
    assert fn(1, BIG, 8, 4, 0.2, 4, F, I, F, I, 1, 0, I, I, F, 0, 0, None) == E_TOO_LARGE


def test_multi_radius_pair_validation(bufs):
    """(b, total, nmax, m, nscales, radii, nsamples, xyz1, offsets1, xyz2, lengths2, subtract, global_idx, idx, pts_cnt, grouped,
    stream): pn2_query_ball_group_xyz_msg_packed's order"""
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_query_ball_group_xyz_msg_packed_pair
    radii, nss = (ctypes.c_float * 2)(0.1, 0.2), (ctypes.c_int * 2)(4, 8)
    bad_r, bad_ns = (ctypes.c_float * 2)(0.1, 0.0), (ctypes.c_int * 2)(4, 0)
    pi, pf = (ctypes.c_void_p * 2)(I, I), (ctypes.c_void_p * 2)(F, F)
    none = (ctypes.c_void_p * 2)(None, None)
    assert fn(1, 8, 8, 4, 0, radii, nss, F, I, F, I, 1, 0, pi, pi, pf, None) == E_ARG    # nscales outside 1..4
    assert fn(1, 8, 8, 4, 5, radii, nss, F, I, F, I, 1, 0, pi, pi, pf, None) == E_ARG
    assert fn(1, 8, 8, 4, 2, None, nss, F, I, F, I, 1, 0, pi, pi, pf, None) == E_ARG
    assert fn(-1, 8, 8, 4, 2, radii, nss, F, I, F, I, 1, 0, pi, pi, pf, None) == E_SHAPE
    assert fn(1, 8, 0, 4, 2, radii, nss, F, I, F, I, 1, 0, pi, pi, pf, None) == E_SHAPE
    assert fn(1, 8, 8, 4, 2, bad_r, nss, F, I, F, I, 1, 0, pi, pi, pf, None) == E_ARG
    assert fn(1, 8, 8, 4, 2, radii, bad_ns, F, I, F, I, 1, 0, pi, pi, pf, None) == E_ARG
    assert fn(0, 8, 8, 4, 2, radii, nss, None, None, None, None, 1, 0, None, None, None, None) == OK
    assert fn(1, 8, 8, 0, 2, radii, nss, None, None, None, None, 1, 0, None, None, None, None) == OK
    assert fn(1, 0, 8, 4, 2, radii, nss, F, I, F, I, 1, 0, pi, pi, pf, None) == E_SHAPE  # total <= 0
    assert fn(1, 8, 9, 4, 2, radii, nss, F, I, F, I, 1, 0, pi, pi, pf, None) == E_SHAPE  # nmax > total
    assert fn(1, 8, 8, 4, 2, radii, nss, F, None, F, I, 1, 0, pi, pi, pf, None) == E_NULL   # NULL offsets
    assert fn(1, 8, 8, 4, 2, radii, nss, F, I, F, None, 1, 0, pi, pi, pf, None) == E_NULL   # NULL lengths2: required here
    assert fn(1, 8, 8, 4, 2, radii, nss, F, I, F, I, 1, 0, none, pi, none, None) == E_NULL  # a scale with neither idx nor grouped_xyz
    assert fn(1, 9000, 9000, 4, 2, radii, nss, F, I, F, I, 1, 0, pi, pi, pf, None) == E_TOO_LARGE   # above the cell kernels' point limit
    assert fn(1, 8, 8, 4, 2, radii, nss, None, I, F, I, 1, 0, pi, pi, pf, None) == E_NULL
    assert fn(1, 8, 8, 4, 2, radii, nss, F, I, None, I, 1, 0, pi, pi, pf, None) == E_NULL


def test_knn_validation(bufs):
    """(b, total, nmax, m, k, xyz1, offsets1, xyz2, lengths2, global_idx, val, idx, stream): knn_entry's order with nmax where n
    stood; lengths2 may be NULL"""
    from pointnet2_amd import _C
    F, I, _ = bufs
    fn = _C.lib().pn2_knn_point_packed
    assert fn(1, 8, 8, 4, 0, F, I, F, None, 0, F, I, None) == E_ARG           # k <= 0, checked first
    assert fn(-1, 8, 8, 4, 2, F, I, F, None, 0, F, I, None) == E_SHAPE
    assert fn(1, 8, 0, 4, 2, F, I, F, None, 0, F, I, None) == E_SHAPE
    assert fn(1, 8, 8, -1, 2, F, I, F, None, 0, F, I, None) == E_SHAPE
    assert fn(0, 8, 8, 4, 2, None, None, None, None, 0, None, None, None) == OK
    assert fn(1, 8, 8, 0, 2, None, None, None, None, 0, None, None, None) == OK
    assert fn(1, 0, 8, 4, 2, F, I, F, None, 0, F, I, None) == E_SHAPE         # total <= 0, behind the early PN2_OK
    assert fn(0, 0, 8, 4, 2, F, I, F, None, 0, F, I, None) == OK
    assert fn(1, 8, 8, 4, 2, None, I, F, None, 0, F, I, None) == E_NULL
    assert fn(1, 8, 8, 4, 2, F, None, F, None, 0, F, I, None) == E_NULL       # NULL offsets
    assert fn(1, 8, 8, 4, 2, F, I, None, None, 0, F, I, None) == E_NULL
    assert fn(1, 8, 8, 4, 2, F, I, F, None, 0, None, I, None) == E_NULL
    assert fn(1, 8, 8, 4, 2, F, I, F, None, 0, F, None, None) == E_NULL
    assert fn(1, 8, 8, 4, 9, F, I, F, None, 0, F, I, None) == E_TOO_LARGE     # k > nmax
    assert fn(1, 20000, 14337, 4, 2, F, I, F, None, 0, F, I, None) == E_TOO_LARGE
    assert fn(1, BIG, 8, 4, 2, F, I, F, None, 0, F, I, None) == E_TOO_LARGE   # total 3 > INT_MAX


def _calls():
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import sample_and_group
    flat, q, offs = torch.zeros(8, 3), torch.zeros(2, 4, 3), [0, 3, 8]
    return [("npoints=. are not offered with offsets", lambda: P.farthest_point_sample(4, flat, offsets=offs, max_points=5, npoints=[2, 4])),
            ("lengths2=. is not offered with offsets", lambda: P.query_ball_point(0.2, 4, flat, q, offsets=offs, max_points=5, lengths2=[2, 4])),
            ("lengths2=. is not offered with offsets",
             lambda: P.query_ball_group_xyz_msg([0.1, 0.2], [4, 8], flat, q, offsets=offs, max_points=5, lengths2=[2, 4])),
            ("knn is not offered with offsets", lambda: sample_and_group(4, 0.2, 4, flat, None, knn=True, offsets=offs, max_points=5)),
            ("offsets and lengths / npoints are two layouts",
             lambda: sample_and_group(4, 0.2, 4, flat, None, offsets=offs, max_points=5, npoints=[2, 4]))]


@pytest.fixture
def pairs_on():
    import pointnet2_amd as P
    from pointnet2_amd import _tensors
    before = _tensors.packed_pairs()
    P.set_packed_pairs(True)
    try:
        yield
    finally:
        P.set_packed_pairs(before)


def test_the_switch_is_off_by_default_and_every_refusal_stands():
    from pointnet2_amd import _tensors
    assert _tensors.packed_pairs() is False
    for message, call in _calls():
        with pytest.raises(ValueError, match=message):
            call()


def test_with_the_switch_on_the_same_calls_reach_the_device_check(pairs_on):
    for _, call in _calls():
        with pytest.raises(ValueError, match=NO_DEVICE):
            call()


def test_set_packed_pairs_takes_a_bool_only():
    import pointnet2_amd as P
    from pointnet2_amd import _tensors
    before = _tensors.packed_pairs()
    try:
        for bad in (1, 0, None, "yes", torch.tensor(True)):
            with pytest.raises(ValueError, match="bool"):
                P.set_packed_pairs(bad)
        assert _tensors.packed_pairs() is before
        P.set_packed_pairs(True)
        assert _tensors.packed_pairs() is True
        P.set_packed_pairs(False)
        assert _tensors.packed_pairs() is False
    finally:
        P.set_packed_pairs(before)


def test_knn_point_takes_offsets_without_the_switch():
    """a new keyword of knn_point: offered whatever the switch says; on CPU tensors it reaches the device check"""
    import pointnet2_amd as P
    from pointnet2_amd import _tensors
    assert _tensors.packed_pairs() is False
    flat, q, offs = torch.zeros(8, 3), torch.zeros(2, 4, 3), [0, 3, 8]
    with pytest.raises(ValueError, match=NO_DEVICE):
        P.knn_point(2, flat, q, offsets=offs, max_points=5)
    with pytest.raises(ValueError, match=NO_DEVICE):
        P.knn_point(2, flat, q, lengths2=[4, 1], offsets=offs, max_points=5, global_idx=True)


def test_wrong_arguments_raise_before_any_launch(pairs_on):
    """shapes of the counts, the two layouts together, a missing max_points, kNN's envelope: ValueError with no device in sight"""
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import PointnetFPModule, PointnetSAModule, PointnetSAModuleMSG, sample_and_group
    flat, q, offs = torch.zeros(8, 3), torch.zeros(2, 4, 3), [0, 3, 8]
    shape = [(lambda: P.farthest_point_sample(4, flat, offsets=offs, max_points=5, npoints=[2, 4, 1]), "npoints"),
             (lambda: P.farthest_point_sample_gather(4, flat, offsets=offs, max_points=5, npoints=[[2, 4]]), "npoints"),
             (lambda: P.query_ball_point(0.2, 4, flat, q, offsets=offs, max_points=5, lengths2=[2, 4, 1]), "lengths2"),
             (lambda: P.query_ball_group_xyz(0.2, 4, flat, q, offsets=offs, max_points=5, lengths2=[4]), "lengths2"),
             (lambda: P.query_ball_group_xyz_msg([0.1], [4], flat, q, offsets=offs, max_points=5, lengths2=[2, 4, 1]), "lengths2"),
             (lambda: P.knn_point(2, flat, q, offsets=offs, max_points=5, lengths2=[2, 4, 1]), "lengths2"),
             (lambda: sample_and_group(4, 0.2, 4, flat, None, offsets=offs, max_points=5, npoints=[2, 4, 1]), "npoints")]
    for call, name in shape:
        with pytest.raises(ValueError, match=name + " must have shape"):
            call()
    with pytest.raises(ValueError, match="npoints must be int32 or int64"):
        P.farthest_point_sample(4, flat, offsets=offs, max_points=5, npoints=torch.tensor([2.0, 4.0]))
    layouts = [lambda: P.knn_point(2, flat, q, lengths1=[3, 5], offsets=offs, max_points=5),
               lambda: P.farthest_point_sample(4, flat, offsets=offs, max_points=5, lengths=[3, 5], npoints=[2, 4]),
               lambda: P.query_ball_point(0.2, 4, flat, q, offsets=offs, max_points=5, lengths1=[3, 5], lengths2=[2, 4]),
               lambda: sample_and_group(4, 0.2, 4, flat, None, offsets=offs, max_points=5, lengths=[3, 5], npoints=[2, 4])]
    for call in layouts:
        with pytest.raises(ValueError, match="two layouts"):
            call()
    for call in (lambda: P.knn_point(2, flat, q, offsets=offs),
                 lambda: P.farthest_point_sample(4, flat, offsets=offs, npoints=[2, 4]),
                 lambda: P.query_ball_point(0.2, 4, flat, q, offsets=offs, lengths2=[2, 4])):
        with pytest.raises(ValueError, match="max_points"):
            call()
    with pytest.raises(ValueError, match="at most 14336 points per cloud"):
        P.knn_point(2, flat, q, offsets=offs, max_points=14337)
    with pytest.raises(ValueError, match="k <= max_points"):
        P.knn_point(6, flat, q, offsets=offs, max_points=5)               # no matrix form to fall back to
    with pytest.raises(ValueError, match="3-D points"):
        P.knn_point(2, flat, torch.zeros(2, 4, 2), offsets=offs, max_points=5)
    with pytest.raises(ValueError, match="npoints"):                     # counts stop at the register tiers, whatever the large switch says
        P.farthest_point_sample(4, flat, offsets=offs, max_points=16385, npoints=[2, 4])
    # still refused with offsets, switch or no switch
    sa = PointnetSAModule(0, 4, 0.2, 4, [8], group_all=True)
    with pytest.raises(ValueError, match="group_all is not offered with offsets"):
        sa(flat, None, offsets=offs, max_points=5)
    sa = PointnetSAModule(0, 4, 0.2, 4, [8])
    with pytest.raises(ValueError, match="two layouts"):
        sa(flat, None, offsets=offs, max_points=5, lengths=[3, 5])
    sa.fused_xyz_grad = True
    with pytest.raises(ValueError, match="fused_xyz_grad is not offered with offsets"):
        sa(flat, None, offsets=offs, max_points=5, npoints=[2, 4])
    msg = PointnetSAModuleMSG(0, 4, [0.1, 0.2], [4, 8], [[8], [8]])
    msg.packed_batches = True
    with pytest.raises(ValueError, match="two layouts"):
        msg(flat, None, offsets=offs, max_points=5, npoints=[2, 4])
    fp = PointnetFPModule(4, [8])
    with pytest.raises(ValueError, match="two layouts"):
        fp(flat, q, None, torch.zeros(2, 4, 4), offsets1=offs, max_points1=5, lengths1=[3, 5], lengths2=[2, 4])


def test_modules_refuse_with_the_switch_off():
    from pointnet2_amd import _tensors
    from pointnet2_amd.pointnet_util import PointnetFPModule, PointnetSAModule
    assert _tensors.packed_pairs() is False
    flat, q, offs = torch.zeros(8, 3), torch.zeros(2, 4, 3), [0, 3, 8]
    with pytest.raises(ValueError, match="knn is not offered with offsets"):
        PointnetSAModule(0, 4, 0.2, 4, [8], knn=True)(flat, None, offsets=offs, max_points=5)
    with pytest.raises(ValueError, match="offsets and lengths / npoints are two layouts"):
        PointnetSAModule(0, 4, 0.2, 4, [8])(flat, None, offsets=offs, max_points=5, npoints=[2, 4])
    with pytest.raises(ValueError, match="offsets1 and lengths1 / lengths2 are two layouts"):
        PointnetFPModule(4, [8])(flat, q, None, torch.zeros(2, 4, 4), offsets1=offs, max_points1=5, lengths2=[2, 4])
