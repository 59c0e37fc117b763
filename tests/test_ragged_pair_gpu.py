"""The second side of ragged batches on the GPU: per-cloud sample counts of FPS (`npoints`) and a ragged query / known side of
the pair operators (`lengths2`); include/pn2ops.h "ragged batches, the second side".

THE PAIR SLICE RULE: for cloud c and rows j < m_c the result is bit- and index-identical to the dense operator on
(xyz1[c, :n_c], xyz2[c, :m_c]) alone; rows j >= m_c hold fixed fills. Expectations come from the CPU oracle applied to every
slice pair, computed once per case and shared by the paddings. Every case runs with two paddings of BOTH padded tensors -- the
rows of xyz1 at or beyond n_c and the rows of xyz2 at or beyond m_c, which the kernels must never read: (a) NaN and (b)
adversarial finite values (the cloud's own first points / queries; for FPS points offset by 1e3)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

PADDINGS = ["nan", "adversarial"]


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def padded(xyz, lengths, padding, offset=None):
    """xyz (b, n, 3) with the rows at or beyond lengths[i] replaced: NaN, or -- adversarial -- the cloud's own first rows
    (offset None) / its own rows moved by `offset`."""
    out = xyz.copy()
    n = xyz.shape[1]
    for i, ni in enumerate(lengths):
        if ni >= n:
            continue
        if padding == "nan":
            out[i, ni:] = np.nan
        elif offset is None:
            out[i, ni:] = xyz[i, np.arange(n - ni) % ni]
        else:
            out[i, ni:] = xyz[i, ni:] + np.float32(offset)
    return out


def lens_t(lengths, cuda):
    return torch.tensor(lengths, dtype=torch.int32, device=cuda)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------- FPS
FPS_CASES = {
    # Q_c = 3,3,2,2,1,1,1,1; m_c > n_c twice (37 points -> 64 samples, 1 point -> 5 samples)
    "q33221111": (S.sphere_clouds, 1100, [1100, 1025, 1024, 513, 512, 511, 37, 1], 64, [64, 1, 63, 64, 17, 2, 64, 5]),
    "512x8": (S.uniform_clouds, 4096, [4096, 3000, 2049, 2048, 100], 128, [128, 1, 127, 64, 128]),
    "lattice_ties": (S.lattice_clouds, 1500, [1500, 1000, 700], 500, [500, 499, 3]),
    "duplicated_ties": (S.duplicated_clouds, 1500, [1500, 1000, 700], 500, [500, 499, 3]),
}


def fps_want(xyz, lengths, m, npoints):
    """per slice the oracle's first m_c samples; rows from m_c on repeat row 0 -> idx (b, m), new_xyz (b, m, 3)"""
    import oracle as O
    wi = np.zeros((len(lengths), m), dtype=np.int32)
    wx = np.zeros((len(lengths), m, 3), dtype=np.float32)
    for i, (ni, mi) in enumerate(zip(lengths, npoints)):
        wi[i, :mi] = O.farthest_point_sample(mi, xyz[i:i + 1, :ni])[0]
        wi[i, mi:] = wi[i, 0]
        wx[i] = xyz[i][wi[i]]
    return wi, wx


@functools.lru_cache(maxsize=None)
def fps_case(name):
    gen, n, lengths, m, npoints = FPS_CASES[name]
    xyz = gen(len(lengths), n, 11)
    return (xyz, lengths, m, npoints) + fps_want(xyz, lengths, m, npoints)


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("name", sorted(FPS_CASES))
def test_fps_counts(cuda, oracle, name, padding):
    import pointnet2_amd as P
    xyz, lengths, m, npoints, wi, wx = fps_case(name)
    x = dev(padded(xyz, lengths, padding, offset=1e3), cuda)
    lens, cnts = lens_t(lengths, cuda), lens_t(npoints, cuda)
    idx, new_xyz = P.farthest_point_sample_gather(m, x, lengths=lens, npoints=cnts)
    got = host(idx)
    assert (got < np.asarray(lengths)[:, None]).all() and (got >= 0).all()
    assert wi[:, 0].max() == 0                                               # sample 0 is point 0
    assert np.array_equal(got, wi)                                           # rows < m_c: the slice's; rows >= m_c: row 0
    assert np.array_equal(bits(host(new_xyz)), bits(wx))
    for form in (cnts, list(npoints), cnts.long()):                         # int32 tensor, sequence, int64 tensor
        assert np.array_equal(host(P.farthest_point_sample(m, x, lengths=lens, npoints=form)), wi)


@pytest.mark.parametrize("name", sorted(FPS_CASES))
def test_fps_full_counts_is_the_one_sided_call(cuda, name):
    import pointnet2_amd as P
    xyz, lengths, m, _, _, _ = fps_case(name)
    x = dev(padded(xyz, lengths, "nan"), cuda)
    idx, new_xyz = P.farthest_point_sample_gather(m, x, lengths=lengths, npoints=[m] * len(lengths))
    oidx, oxyz = P.farthest_point_sample_gather(m, x, lengths=lengths)
    assert torch.equal(idx, oidx) and torch.equal(new_xyz, oxyz)
    assert torch.equal(P.farthest_point_sample(m, x, lengths=lengths, npoints=[m] * len(lengths)), oidx)


def test_fps_counts_without_lengths_means_full_lengths(cuda, oracle):
    import pointnet2_amd as P
    xyz = S.sphere_clouds(3, 700, 12)
    npoints = [40, 1, 17]
    wi, wx = fps_want(xyz, [700] * 3, 40, npoints)
    idx, new_xyz = P.farthest_point_sample_gather(40, dev(xyz, cuda), npoints=npoints)
    assert np.array_equal(host(idx), wi) and np.array_equal(bits(host(new_xyz)), bits(wx))


def test_fps_counts_are_clamped_on_the_device(cuda):
    """0, a negative count and m + 7: the bits of the clamped counts (memory safety only; check_lengths validates)"""
    import pointnet2_amd as P
    xyz, lengths, m, _, _, _ = fps_case("q33221111")
    x = dev(padded(xyz, lengths, "nan"), cuda)
    raw = [0, -5, m + 7, 64, 17, 2, 64, 5]
    clamped = [min(max(v, 1), m) for v in raw]
    got = P.farthest_point_sample_gather(m, x, lengths=lengths, npoints=lens_t(raw, cuda))
    want = P.farthest_point_sample_gather(m, x, lengths=lengths, npoints=clamped)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError):
        P.check_lengths(raw, m)


# ----------------------------------------------------------------------------------------------------------- ball query
# Launch geometry at these shapes (launch_bq, bq_use_cells / bq_cells_pick / launch_bq_cells, msg_plan; b = 5, n = 2500):
#   m = 128: sweep (kernel 0 -- b m < 8192 -- and 1): qpb 16, gx 8; cell list kernel 2: 512 threads, 16 lanes per query, qpb 32,
#            4 parts; kernel 3: 512 threads, 8 lanes per query, qpb 64, 2 parts; multi-radius (0.1, 0.2, 0.4): swept, qpb 16.
#            With lengths2 = [128, 127, 33, 7, 1] cloud 2 has a workgroup that straddles m_c = 33 under every qpb (32..47,
#            32..63, 0..63) and workgroups of fill rows alone behind it; clouds 3 and 4 straddle in their first workgroup;
#            cloud 1 (127) straddles in its last.
#   m = 640: sweep qpb 16, gx 40; cell list kernel 2: qpb 32, 20 parts.
BQ_N, BQ_LENGTHS1 = 2500, [2500, 2048, 700, 63, 1]
BQ_SHAPES = {128: [128, 127, 33, 7, 1], 640: [640, 65, 1, 64, 600]}
BQ_PARAMS = [(0.2, 32), (0.4, 16)]
MSG_SCALES = [(0.1, 8), (0.2, 16), (0.4, 32)]


@functools.lru_cache(maxsize=None)
def bq_cloud(m):
    """the clouds and, per slice, its own first m_c farthest-point samples as queries (rows beyond: zeros, replaced by the padding)"""
    import oracle as O
    xyz = S.uniform_clouds(len(BQ_LENGTHS1), BQ_N, 21)
    q = np.zeros((len(BQ_LENGTHS1), m, 3), dtype=np.float32)
    for i, (ni, mi) in enumerate(zip(BQ_LENGTHS1, BQ_SHAPES[m])):
        sl = xyz[i:i + 1, :ni]
        q[i, :mi] = O.gather_point(sl, O.farthest_point_sample(mi, sl))[0]
    return xyz, q


def bq_want(xyz, q, lengths1, lengths2, radius, nsample):
    """the oracle per slice pair, extended by the fills -> idx, pts_cnt, grouped (centred), grouped (raw)"""
    import oracle as O
    b, m = q.shape[0], q.shape[1]
    wi = np.zeros((b, m, nsample), dtype=np.int32)
    wc = np.zeros((b, m), dtype=np.int32)
    wg = np.zeros((b, m, nsample, 3), dtype=np.float32)
    wr = np.zeros((b, m, nsample, 3), dtype=np.float32)
    for i, (ni, mi) in enumerate(zip(lengths1, lengths2)):
        sl, qi = xyz[i:i + 1, :ni], q[i:i + 1, :mi]
        ii, ci = O.query_ball_point(radius, nsample, sl, qi)
        wi[i, :mi], wc[i, :mi] = ii[0], ci[0]
        wr[i, :mi] = O.group_point(sl, ii)[0]
        wg[i, :mi] = wr[i, :mi] - qi[0][:, None, :]
    return wi, wc, wg, wr


@functools.lru_cache(maxsize=None)
def bq_case(m, radius, nsample):
    xyz, q = bq_cloud(m)
    return (xyz, q) + bq_want(xyz, q, BQ_LENGTHS1, BQ_SHAPES[m], radius, nsample)


def bq_inputs(m, padding, cuda):
    xyz, q = bq_cloud(m)
    return (dev(padded(xyz, BQ_LENGTHS1, padding), cuda), dev(padded(q, BQ_SHAPES[m], padding), cuda), lens_t(BQ_LENGTHS1, cuda),
            lens_t(BQ_SHAPES[m], cuda))


def check_bq(idx, cnt, grp, raw, want, lengths1, lengths2):
    wi, wc, wg, wr = want
    if idx is not None:
        assert (host(idx) < np.asarray(lengths1)[:, None, None]).all() and (host(idx) >= 0).all()
        assert np.array_equal(host(idx), wi)
    assert np.array_equal(host(cnt), wc)
    for got, w in ((grp, wg), (raw, wr)):
        if got is None:
            continue
        g = host(got)
        for i, mi in enumerate(lengths2):
            assert np.array_equal(g[i, :mi], w[i, :mi]), i
            assert not bits(g[i, mi:]).any(), i                              # the fill: +0.0, bit for bit


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
@pytest.mark.parametrize("radius,nsample", BQ_PARAMS)
def test_ball_query_pair(cuda, oracle, radius, nsample, kernel, padding):
    import pointnet2_amd as P
    from pointnet2_amd import tf_grouping
    want = bq_case(128, radius, nsample)[2:]
    x, qd, l1, l2 = bq_inputs(128, padding, cuda)
    before = list(tf_grouping._BQ_KERNEL)
    tf_grouping.set_ball_query_kernel(kernel)
    try:
        idx, cnt, grp = P.query_ball_group_xyz(radius, nsample, x, qd, True, lengths1=l1, lengths2=l2)
        idx2, cnt2 = P.query_ball_point(radius, nsample, x, qd, lengths1=l1, lengths2=l2)
        none, cnt3, raw = P.query_ball_group_xyz(radius, nsample, x, qd, False, want_idx=False, lengths1=l1, lengths2=l2)
    finally:
        tf_grouping.set_ball_query_kernel(*before)
    assert none is None
    check_bq(idx, cnt, grp, raw, want, BQ_LENGTHS1, BQ_SHAPES[128])
    check_bq(idx2, cnt2, None, None, want, BQ_LENGTHS1, BQ_SHAPES[128])
    assert np.array_equal(host(cnt3), want[1])


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("kernel", [1, 2])
def test_ball_query_pair_many_workgroups_per_cloud(cuda, oracle, kernel, padding):
    """m = 640: gx = 40 in the sweep kernel, 20 parts in the cell-list kernel"""
    import pointnet2_amd as P
    from pointnet2_amd import tf_grouping
    want = bq_case(640, 0.2, 32)[2:]
    x, qd, l1, l2 = bq_inputs(640, padding, cuda)
    before = list(tf_grouping._BQ_KERNEL)
    tf_grouping.set_ball_query_kernel(kernel)
    try:
        idx, cnt, grp = P.query_ball_group_xyz(0.2, 32, x, qd, True, lengths1=l1, lengths2=l2)
    finally:
        tf_grouping.set_ball_query_kernel(*before)
    check_bq(idx, cnt, grp, None, want, BQ_LENGTHS1, BQ_SHAPES[640])


def test_ball_query_one_side_given_the_other_is_dense(cuda):
    import pointnet2_amd as P
    x, qd, l1, l2 = bq_inputs(128, "nan", cuda)
    full1, full2 = [BQ_N] * len(BQ_LENGTHS1), [128] * len(BQ_LENGTHS1)
    xd = dev(bq_cloud(128)[0], cuda)                                         # no padding in xyz1: its side is dense here
    a = P.query_ball_group_xyz(0.2, 32, xd, qd, True, lengths2=l2)
    b = P.query_ball_group_xyz(0.2, 32, xd, qd, True, lengths1=full1, lengths2=l2)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    qfull = dev(padded(bq_cloud(128)[1], BQ_SHAPES[128], "adversarial"), cuda)   # every query row valid
    c = P.query_ball_group_xyz(0.2, 32, x, qfull, True, lengths1=l1, lengths2=full2)
    d = P.query_ball_group_xyz(0.2, 32, x, qfull, True, lengths1=l1)
    assert all(torch.equal(s, t) for s, t in zip(c, d))


def test_ball_query_counts_are_clamped_on_the_device(cuda):
    import pointnet2_amd as P
    x, qd, l1, _ = bq_inputs(128, "adversarial", cuda)
    raw = [0, -3, 128 + 7, 7, 1]
    clamped = [min(max(v, 1), 128) for v in raw]
    got = P.query_ball_group_xyz(0.2, 32, x, qd, True, lengths1=l1, lengths2=lens_t(raw, cuda))
    want = P.query_ball_group_xyz(0.2, 32, x, qd, True, lengths1=l1, lengths2=clamped)
    assert all(torch.equal(s, t) for s, t in zip(got, want))


# --------------------------------------------------------------------------------------------------------- multi-radius
MSG_SWEPT = (300, [300, 63, 1], 64, [64, 5, 1])          # n, lengths1, m, lengths2: b m = 192, qpb 16, 4 parts, never binned


@functools.lru_cache(maxsize=None)
def msg_swept_cloud():
    import oracle as O
    n, l1, m, l2 = MSG_SWEPT
    xyz = S.uniform_clouds(len(l1), n, 24)
    q = np.zeros((len(l1), m, 3), dtype=np.float32)
    for i, (ni, mi) in enumerate(zip(l1, l2)):
        q[i, :mi] = O.gather_point(xyz[i:i + 1, :ni], O.farthest_point_sample(mi, xyz[i:i + 1, :ni]))[0]
    return xyz, q


@functools.lru_cache(maxsize=None)
def msg_want(shape):
    if shape == "swept":
        (xyz, q), l1, l2 = msg_swept_cloud(), MSG_SWEPT[1], MSG_SWEPT[3]
    else:
        (xyz, q), l1, l2 = bq_cloud(128), BQ_LENGTHS1, BQ_SHAPES[128]
    return xyz, q, l1, l2, [bq_want(xyz, q, l1, l2, r, k) for r, k in MSG_SCALES]


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("shape", ["clouds", "swept"])
def test_multi_radius_pair(cuda, oracle, shape, padding):
    import pointnet2_amd as P
    xyz, q, l1, l2, wants = msg_want(shape)
    plan = P.tf_grouping.query_ball_group_xyz_msg_plan([r for r, _ in MSG_SCALES], [k for _, k in MSG_SCALES], len(l1), xyz.shape[1],
                                                       q.shape[1])
    assert plan["rc"] == 0 and plan["qpb"] == 16 and plan["use_cells"] == 0       # the geometry the comment above states
    x, qd = dev(padded(xyz, l1, padding), cuda), dev(padded(q, l2, padding), cuda)
    a, c = lens_t(l1, cuda), lens_t(l2, cuda)
    for subtract in (True, False):
        one = P.query_ball_group_xyz_msg([r for r, _ in MSG_SCALES], [k for _, k in MSG_SCALES], x, qd, subtract, lengths1=a, lengths2=c)
        for (r, k), (idx, cnt, grp), want in zip(MSG_SCALES, one, wants):
            pidx, pcnt, pgrp = P.query_ball_group_xyz(r, k, x, qd, subtract, lengths1=a, lengths2=c)
            assert torch.equal(idx, pidx) and torch.equal(cnt, pcnt), r
            assert np.array_equal(bits(host(grp)), bits(host(pgrp))), r
            check_bq(idx, cnt, grp if subtract else None, None if subtract else grp, want, l1, l2)


def test_multi_radius_pair_binned(cuda, oracle):
    """a launch large enough for the cell list (n >= 1024, b m nscales >= 8192): per-radius pair launches are the reference,
    themselves checked against the oracle above"""
    import pointnet2_amd as P
    b, n, m = 6, 2048, 512
    l1, l2 = [2048, 1500, 1024, 64, 63, 1], [512, 300, 1, 512, 33, 2]
    plan = P.tf_grouping.query_ball_group_xyz_msg_plan([0.1, 0.2, 0.4], [8, 16, 32], b, n, m)
    assert plan["use_cells"] == 1
    xyz = S.sphere_clouds(b, n, 25)
    x = dev(padded(xyz, l1, "nan"), cuda)
    _, q = P.farthest_point_sample_gather(m, x, lengths=l1, npoints=l2)
    for i, mi in enumerate(l2):
        q[i, mi:] = float("nan")
    one = P.query_ball_group_xyz_msg([0.1, 0.2, 0.4], [8, 16, 32], x, q, True, lengths1=l1, lengths2=l2)
    for (r, k), (idx, cnt, grp) in zip(MSG_SCALES, one):
        pidx, pcnt, pgrp = P.query_ball_group_xyz(r, k, x, q, True, lengths1=l1, lengths2=l2)
        assert torch.equal(idx, pidx) and torch.equal(cnt, pcnt) and np.array_equal(bits(host(grp)), bits(host(pgrp))), r
        assert torch.isfinite(grp).all()
        for i, (ni, mi) in enumerate(zip(l1, l2)):
            assert int(idx[i].max()) < ni and not bits(host(grp[i, mi:])).any() and int(cnt[i, mi:].sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ kNN
KNN_N, KNN_LENGTHS1, KNN_M, KNN_LENGTHS2 = 1500, [1500, 600, 40], 64, [64, 9, 1]


@functools.lru_cache(maxsize=None)
def knn_case(k):
    """built as tests/test_ragged_gpu.py's knn_case, per slice pair: the fp32 distance matrix, the oracle's swap rounds, the
    first k columns; k > n_c: the entries from n_c on repeat entry 0; rows from m_c on: idx 0, val +0.0"""
    import oracle as O
    rng = np.random.default_rng(31)
    xyz = S.sphere_clouds(len(KNN_LENGTHS1), KNN_N, 32)
    q = np.zeros((len(KNN_LENGTHS1), KNN_M, 3), dtype=np.float32)
    wi = np.zeros((len(KNN_LENGTHS1), KNN_M, k), dtype=np.int32)
    wv = np.zeros((len(KNN_LENGTHS1), KNN_M, k), dtype=np.float32)
    for i, (ni, mi) in enumerate(zip(KNN_LENGTHS1, KNN_LENGTHS2)):
        sl = xyz[i:i + 1, :ni]
        q[i, :mi] = sl[0, rng.integers(0, ni, size=mi)]
        q[i, :mi:2] += rng.normal(0, 0.05, size=q[i, :mi:2].shape).astype(np.float32)
        dx = sl[:, None, :, 0] - q[i, :mi][None, :, None, 0]
        dy = sl[:, None, :, 1] - q[i, :mi][None, :, None, 1]
        dz = sl[:, None, :, 2] - q[i, :mi][None, :, None, 2]
        d = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
        kk = min(k, ni)
        oi, ov = O.select_top_k(kk, d)
        wi[i, :mi, :kk], wv[i, :mi, :kk] = oi[0, :, :kk], ov[0, :, :kk]
        wi[i, :mi, kk:], wv[i, :mi, kk:] = oi[0, :, :1], ov[0, :, :1]
    return xyz, q, wi, wv


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("k", [8, 32, 48])                                 # 48 > n_c = 40: the repeat-entry-0 rule
def test_knn_pair(cuda, oracle, k, padding):
    import pointnet2_amd as P
    xyz, q, wi, wv = knn_case(k)
    val, idx = P.knn_point(k, dev(padded(xyz, KNN_LENGTHS1, padding), cuda), dev(padded(q, KNN_LENGTHS2, padding), cuda),
                           lengths1=lens_t(KNN_LENGTHS1, cuda), lengths2=lens_t(KNN_LENGTHS2, cuda))
    assert (host(idx) < np.asarray(KNN_LENGTHS1)[:, None, None]).all() and (host(idx) >= 0).all()
    assert np.array_equal(host(idx), wi) and np.array_equal(bits(host(val)), bits(wv))
    for i, mi in enumerate(KNN_LENGTHS2):                                    # the fill rows, exactly
        assert not host(idx)[i, mi:].any() and not bits(host(val)[i, mi:]).any()


# ------------------------------------------------------------------------------------------------------------- three_nn
NN_CASES = {
    "m1024": (2000, [2000, 1500, 129, 128, 1, 7, 64], 1024, [1024, 700, 64, 63, 3, 2, 1], [0, 1, 2]),
    "m40": (2000, [2000, 1500, 129, 128, 1, 7, 64], 40, [40, 3, 2, 1, 40, 17, 5], [0, 1]),
}


@functools.lru_cache(maxsize=None)
def nn_case(name):
    import oracle as O
    n, l1, m, l2, _ = NN_CASES[name]
    unknown = S.uniform_clouds(len(l1), n, 41)
    known = S.uniform_clouds(len(l1), m, 42)
    wd = np.zeros((len(l1), n, 3), dtype=np.float32)                        # rows beyond lengths1: zeros
    wi = np.zeros((len(l1), n, 3), dtype=np.int32)
    for i, (ni, mi) in enumerate(zip(l1, l2)):
        d, ix = O.three_nn(unknown[i:i + 1, :ni], known[i:i + 1, :mi])
        wd[i, :ni], wi[i, :ni] = d[0], ix[0]
    return unknown, known, wd, wi


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("name", sorted(NN_CASES))
def test_three_nn_pair(cuda, oracle, name, padding):
    import pointnet2_amd as P
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    from pointnet2_amd.pointnet_util import three_nn_weights
    n, l1, m, l2, variants = NN_CASES[name]
    unknown, known, wd, wi = nn_case(name)
    assert np.isinf(wd).any()                                                # m_c < 3: the dense operator's +inf / index 0 entries
    x1, x2 = dev(padded(unknown, l1, padding), cuda), dev(padded(known, l2, padding), cuda)
    a, c = lens_t(l1, cuda), lens_t(l2, cuda)
    for variant in variants:
        d = torch.full((len(l1), n, 3), -7.0, device=cuda)
        ix = torch.full((len(l1), n, 3), -7, dtype=torch.int32, device=cuda)
        rc = _C.lib().pn2_three_nn_ragged_pair(len(l1), n, m, ptr(x1), ptr(a), ptr(x2), ptr(c), ptr(d), ptr(ix), variant, stream_ptr(cuda))
        assert rc == 0
        assert (host(ix) < np.maximum(np.asarray(l2), 1)[:, None, None]).all() and (host(ix) >= 0).all(), variant
        assert np.array_equal(host(ix), wi) and np.array_equal(bits(host(d)), bits(wd)), variant
    dist, idx = P.three_nn(x1, x2, lengths1=a, lengths2=c)
    assert np.array_equal(host(idx), wi) and np.array_equal(bits(host(dist)), bits(wd))
    widx, w = three_nn_weights(x1, x2, lengths1=a, lengths2=c)
    assert torch.isfinite(w).all() and np.array_equal(host(widx), wi)


def test_three_nn_known_side_only(cuda, oracle):
    """lengths2 without lengths1: a dense unknown side behind the pair entry"""
    import pointnet2_amd as P
    n, l1, m, l2, _ = NN_CASES["m1024"]
    unknown, known, _, _ = nn_case("m1024")
    x1, x2 = dev(unknown, cuda), dev(padded(known, l2, "nan"), cuda)
    dist, idx = P.three_nn(x1, x2, lengths2=l2)
    for i, mi in enumerate(l2):
        d, ix = oracle.three_nn(unknown[i:i + 1], known[i:i + 1, :mi])
        assert np.array_equal(host(idx[i]), ix[0]) and np.array_equal(bits(host(dist[i])), bits(d[0])), i


# ------------------------------------------------------------------------------------------------------ sample_and_group
SG_LENGTHS, SG_NPOINTS = [1024, 700, 300, 64], [64, 40, 7, 1]


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("knn", [False, True])
@pytest.mark.parametrize("with_points", [False, True])
def test_sample_and_group_counts(cuda, knn, with_points, padding):
    """against the composition of the pair operators checked above; idx never names a padding row, so NaN padding in xyz and
    in the features reaches no output"""
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import sample_and_group
    xyz = S.sphere_clouds(4, 1024, 51)
    x = dev(padded(xyz, SG_LENGTHS, padding), cuda)
    feats = np.random.default_rng(52).random((4, 1024, 6), dtype=np.float32)
    for i, ni in enumerate(SG_LENGTHS):
        feats[i, ni:] = np.nan if padding == "nan" else 1e6
    pts = dev(feats, cuda) if with_points else None
    new_xyz, new_points, idx, grouped_xyz = sample_and_group(64, 0.2, 16, x, pts, knn=knn, lengths=SG_LENGTHS, npoints=SG_NPOINTS)
    fps, wxyz = P.farthest_point_sample_gather(64, x, lengths=SG_LENGTHS, npoints=SG_NPOINTS)
    if knn:
        _, widx = P.knn_point(16, x, wxyz, lengths1=SG_LENGTHS, lengths2=SG_NPOINTS)
    else:
        widx, _ = P.query_ball_point(0.2, 16, x, wxyz, lengths1=SG_LENGTHS, lengths2=SG_NPOINTS)
    assert torch.equal(new_xyz, wxyz) and torch.equal(idx, widx)
    assert (host(idx) < np.asarray(SG_LENGTHS)[:, None, None]).all()
    wg = P.group_point(x, widx) - wxyz.unsqueeze(2)
    assert torch.equal(grouped_xyz, wg) and torch.isfinite(grouped_xyz).all()
    for i, mi in enumerate(SG_NPOINTS):                                      # padding centroids: sample 0, group of point 0
        assert not host(idx)[i, mi:].any() and not host(grouped_xyz)[i, mi:].any()
        assert torch.equal(new_xyz[i, mi:], new_xyz[i, :1].expand(64 - mi, 3))
    want = torch.cat([wg, P.group_point(pts, widx)], dim=-1) if with_points else wg
    assert torch.equal(new_points, want) and torch.isfinite(new_points).all()


# -------------------------------------------------------------------------------------------------------------- capture
def test_capture_and_replay_with_new_counts(cuda):
    """sample_and_group_xyz(lengths=, npoints=) captured once; both count arrays are overwritten in place; the replay gives the
    eager call's bits at the new counts (the host never read them). Rows beyond the LARGER length hold NaN."""
    import pointnet2_amd as P
    first, second = ([1024, 700, 300, 64], [64, 40, 7, 1]), ([900, 1024, 64, 250], [3, 64, 64, 20])
    xyz = S.sphere_clouds(4, 1024, 53)
    x = dev(padded(xyz, [max(a, b) for a, b in zip(first[0], second[0])], "nan"), cuda)
    lens, cnts = lens_t(first[0], cuda), lens_t(first[1], cuda)

    def step():
        return P.sample_and_group_xyz(64, 0.2, 16, x, True, lengths=lens, npoints=cnts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        old = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    lens.copy_(lens_t(second[0], cuda))
    cnts.copy_(lens_t(second[1], cuda))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in captured]
    want = step()
    assert not all(torch.equal(g, o) for g, o in zip(got, old))              # the replay did see the new counts
    for g, w in zip(got, want):
        assert np.array_equal(bits(host(g)) if g.dtype == torch.float32 else host(g), bits(host(w)) if w.dtype == torch.float32 else host(w))
    assert all(torch.isfinite(g).all() for g in got if g.dtype == torch.float32)
