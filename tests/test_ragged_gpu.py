"""Ragged batches through the Python operators on the GPU (lengths / lengths1 keywords; include/pn2ops.h "ragged batches").

THE SLICE RULE: for cloud i the result is bit- and index-identical to the dense operator on xyz[i:i+1, :lengths[i]]. The
expectations therefore come from the CPU oracle applied to every slice, computed once per case and shared by the paddings.
Every case runs with two paddings of the rows at or beyond lengths[i], which the kernels must never read: (a) NaN, and (b)
adversarial finite values -- for FPS points offset by 1e3 (picked at once if read), for ball query / kNN / three_nn copies of
the cloud's own first points (they would enter the balls and neighbour lists if read). Every idx must be < lengths[i]."""
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
    """xyz (b, n, 3) with the rows at or beyond lengths[i] replaced: NaN, or -- adversarial -- the cloud's own first points
    (offset None) / its own points moved by `offset` (FPS: far away, so they would win the first rounds)."""
    out = xyz.copy()
    n = xyz.shape[1]
    for i, ni in enumerate(lengths):
        if ni == n:
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


# ------------------------------------------------------------------------------------------------------------------- FPS
FPS_CASES = {
    "q3322111_m_gt_n": (S.sphere_clouds, 1100, [1100, 1025, 1024, 513, 512, 511, 37, 1], 64),     # Q_i = 3,3,2,2,1,1,1,1; m > n_i twice
    "512x8": (S.uniform_clouds, 4096, [4096, 3000, 2049, 2048, 100], 128),
    "no_lds_mirror": (S.uniform_clouds, 8200, [8200, 5000], 32),
    "lattice_ties": (S.lattice_clouds, 1500, [1500, 1000, 700], 500),
    "duplicated_ties": (S.duplicated_clouds, 1500, [1500, 1000, 700], 500),
}


@functools.lru_cache(maxsize=None)
def fps_case(name):
    import oracle as O
    gen, n, lengths, m = FPS_CASES[name]
    xyz = gen(len(lengths), n, 11)
    want = np.stack([O.farthest_point_sample(m, xyz[i:i + 1, :ni])[0] for i, ni in enumerate(lengths)])
    return xyz, lengths, m, want


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("name", sorted(FPS_CASES))
def test_fps_ragged(cuda, oracle, name, padding):
    import pointnet2_amd as P
    xyz, lengths, m, want = fps_case(name)
    x = dev(padded(xyz, lengths, padding, offset=1e3), cuda)
    lens = lens_t(lengths, cuda)
    idx, new_xyz = P.farthest_point_sample_gather(m, x, lengths=lens)
    got = host(idx)
    assert (got < np.asarray(lengths)[:, None]).all() and (got >= 0).all()
    assert np.array_equal(got, want)
    gathered = np.stack([xyz[i][want[i]] for i in range(len(lengths))])
    assert np.array_equal(host(new_xyz), gathered)                         # out_xyz: the gathered slice, bit for bit
    assert np.array_equal(host(P.farthest_point_sample(m, x, lengths=lens)), want)
    assert np.array_equal(host(P.farthest_point_sample(m, x, lengths=list(lengths))), want)      # a sequence, int64 tensor
    assert np.array_equal(host(P.farthest_point_sample(m, x, lengths=lens.long())), want)


def test_fps_ragged_full_lengths_is_the_dense_operator(cuda):
    import pointnet2_amd as P
    x = dev(S.sphere_clouds(3, 1100, 12), cuda)
    idx, new_xyz = P.farthest_point_sample_gather(64, x, lengths=[1100] * 3)
    didx, dxyz = P.farthest_point_sample_gather(64, x)
    assert torch.equal(idx, didx) and torch.equal(new_xyz, dxyz)


def test_fps_ragged_envelope(cuda):
    import pointnet2_amd as P
    x = torch.zeros(1, 16385, 3, device=cuda)
    with pytest.raises(ValueError):
        P.farthest_point_sample(4, x, lengths=[16385])


# ----------------------------------------------------------------------------------------------------------- ball query
BQ_N, BQ_LENGTHS, BQ_M = 2500, [2500, 2048, 700, 63, 1], 128
BQ_PARAMS = [(0.2, 32), (0.4, 16)]


@functools.lru_cache(maxsize=None)
def bq_case(radius, nsample):
    """queries = each slice's own farthest-point samples; -> xyz, queries, idx, pts_cnt, grouped (centred) per the oracle"""
    import oracle as O
    xyz = S.uniform_clouds(len(BQ_LENGTHS), BQ_N, 21)
    q, idx, cnt, grp = [], [], [], []
    for i, ni in enumerate(BQ_LENGTHS):
        sl = xyz[i:i + 1, :ni]
        qi = O.gather_point(sl, O.farthest_point_sample(BQ_M, sl))
        ii, ci = O.query_ball_point(radius, nsample, sl, qi)
        q.append(qi[0]); idx.append(ii[0]); cnt.append(ci[0])
        grp.append(O.group_point(sl, ii)[0] - qi[0][:, None, :])
    return xyz, np.stack(q), np.stack(idx), np.stack(cnt), np.stack(grp)


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
@pytest.mark.parametrize("radius,nsample", BQ_PARAMS)
def test_ball_query_ragged(cuda, oracle, radius, nsample, kernel, padding):
    import pointnet2_amd as P
    from pointnet2_amd import tf_grouping
    xyz, q, widx, wcnt, wgrp = bq_case(radius, nsample)
    x, qd, lens = dev(padded(xyz, BQ_LENGTHS, padding), cuda), dev(q, cuda), lens_t(BQ_LENGTHS, cuda)
    before = list(tf_grouping._BQ_KERNEL)
    P.tf_grouping.set_ball_query_kernel(kernel)
    try:
        idx, cnt, grp = P.query_ball_group_xyz(radius, nsample, x, qd, True, lengths1=lens)
        idx2, cnt2 = P.query_ball_point(radius, nsample, x, qd, lengths1=lens)
        _, _, raw = P.query_ball_group_xyz(radius, nsample, x, qd, False, want_idx=False, lengths1=lens)
    finally:
        P.tf_grouping.set_ball_query_kernel(*before)
    assert (host(idx) < np.asarray(BQ_LENGTHS)[:, None, None]).all() and (host(idx) >= 0).all()
    assert np.array_equal(host(idx), widx) and np.array_equal(host(cnt), wcnt)
    assert np.array_equal(host(grp), wgrp)
    assert np.array_equal(host(idx2), widx) and np.array_equal(host(cnt2), wcnt)
    assert np.array_equal(host(raw), np.stack([xyz[i][widx[i]] for i in range(len(BQ_LENGTHS))]))    # without the centroid


@pytest.mark.parametrize("kernel", [0, 2])
def test_ball_query_ragged_empty_balls(cuda, kernel):
    """queries far from the cloud: empty balls, rows of zeros -- whatever the dense operator answers on the slice"""
    import pointnet2_amd as P
    xyz = S.uniform_clouds(3, 600, 22)
    lengths = [600, 200, 30]
    q = (S.uniform_clouds(3, 16, 23) + np.float32(10.0)).astype(np.float32)
    x, qd = dev(padded(xyz, lengths, "nan"), cuda), dev(q, cuda)
    P.tf_grouping.set_ball_query_kernel(kernel)
    try:
        idx, cnt, grp = P.query_ball_group_xyz(0.2, 8, x, qd, True, lengths1=lengths)
        for i, ni in enumerate(lengths):
            di, dc, dg = P.query_ball_group_xyz(0.2, 8, x[i:i + 1, :ni].contiguous(), qd[i:i + 1], True)
            assert torch.equal(idx[i:i + 1], di) and torch.equal(cnt[i:i + 1], dc) and torch.equal(grp[i:i + 1], dg)
    finally:
        P.tf_grouping.set_ball_query_kernel(0)
    assert int(cnt.sum()) == 0 and int(idx.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ kNN
KNN_N, KNN_LENGTHS, KNN_M = 1500, [1500, 600, 40], 64


@functools.lru_cache(maxsize=None)
def knn_case(k):
    """the expectation of tests/test_parity_gpu.py::test_knn_point_native_ties_and_shapes, per slice: the fp32 distance
    matrix, the oracle's swap rounds, the first k columns; k > n_i: the row's entries from n_i on repeat entry 0"""
    import oracle as O
    rng = np.random.default_rng(31)
    xyz = S.sphere_clouds(len(KNN_LENGTHS), KNN_N, 32)
    q = np.empty((len(KNN_LENGTHS), KNN_M, 3), dtype=np.float32)
    wi = np.empty((len(KNN_LENGTHS), KNN_M, k), dtype=np.int32)
    wv = np.empty((len(KNN_LENGTHS), KNN_M, k), dtype=np.float32)
    for i, ni in enumerate(KNN_LENGTHS):
        sl = xyz[i:i + 1, :ni]
        q[i] = sl[0, rng.integers(0, ni, size=KNN_M)]
        q[i, ::2] += rng.normal(0, 0.05, size=q[i, ::2].shape).astype(np.float32)
        dx = sl[:, None, :, 0] - q[i][None, :, None, 0]
        dy = sl[:, None, :, 1] - q[i][None, :, None, 1]
        dz = sl[:, None, :, 2] - q[i][None, :, None, 2]
        d = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
        oi, ov = O.select_top_k(min(k, ni), d)
        kk = min(k, ni)
        wi[i, :, :kk], wv[i, :, :kk] = oi[0, :, :kk], ov[0, :, :kk]
        wi[i, :, kk:], wv[i, :, kk:] = oi[0, :, :1], ov[0, :, :1]
    return xyz, q, wi, wv


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("k", [8, 32, 48])                                 # 48 > n_i = 40: the repeat-entry-0 rule
def test_knn_ragged(cuda, oracle, k, padding):
    import pointnet2_amd as P
    xyz, q, wi, wv = knn_case(k)
    val, idx = P.knn_point(k, dev(padded(xyz, KNN_LENGTHS, padding), cuda), dev(q, cuda), lengths1=lens_t(KNN_LENGTHS, cuda))
    assert (host(idx) < np.asarray(KNN_LENGTHS)[:, None, None]).all() and (host(idx) >= 0).all()
    assert np.array_equal(host(idx), wi) and np.array_equal(host(val), wv)
    if k > min(KNN_LENGTHS):
        i, ni = len(KNN_LENGTHS) - 1, KNN_LENGTHS[-1]
        assert (host(idx)[i, :, ni:] == host(idx)[i, :, :1]).all() and (host(val)[i, :, ni:] == host(val)[i, :, :1]).all()


def test_knn_ragged_envelope(cuda):
    import pointnet2_amd as P
    with pytest.raises(ValueError):                                         # not 3-D points
        P.knn_point(2, torch.zeros(1, 8, 2, device=cuda), torch.zeros(1, 4, 2, device=cuda), lengths1=[8])
    with pytest.raises(ValueError):                                         # beyond the one-kernel envelope
        P.knn_point(2, torch.zeros(1, 14337, 3, device=cuda), torch.zeros(1, 4, 3, device=cuda), lengths1=[100])


# ------------------------------------------------------------------------------------------------------------- three_nn
NN_N, NN_LENGTHS = 3000, [3000, 1024, 5]


@functools.lru_cache(maxsize=None)
def nn_case(m):
    import oracle as O
    unknown = S.uniform_clouds(len(NN_LENGTHS), NN_N, 41)
    known = S.uniform_clouds(len(NN_LENGTHS), m, 42)
    wd = np.zeros((len(NN_LENGTHS), NN_N, 3), dtype=np.float32)             # rows beyond the length: zeros
    wi = np.zeros((len(NN_LENGTHS), NN_N, 3), dtype=np.int32)
    for i, ni in enumerate(NN_LENGTHS):
        d, ix = O.three_nn(unknown[i:i + 1, :ni], known[i:i + 1])
        wd[i, :ni], wi[i, :ni] = d[0], ix[0]
    return unknown, known, wd, wi


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("m", [2, 64, 512])
def test_three_nn_ragged(cuda, oracle, m, padding):
    import pointnet2_amd as P
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    unknown, known, wd, wi = nn_case(m)
    x1, x2, lens = dev(padded(unknown, NN_LENGTHS, padding), cuda), dev(known, cuda), lens_t(NN_LENGTHS, cuda)
    dist, idx = P.three_nn(x1, x2, lengths1=lens)
    assert np.array_equal(host(idx), wi) and np.array_equal(host(dist), wd)       # +inf where a neighbour is missing (m = 2)
    for variant in ([1, 2] if m >= 64 else [1]):                            # the sweep and the cell list, forced
        d = torch.full((len(NN_LENGTHS), NN_N, 3), -7.0, device=cuda)
        ix = torch.full((len(NN_LENGTHS), NN_N, 3), -7, dtype=torch.int32, device=cuda)
        rc = _C.lib().pn2_three_nn_ragged(len(NN_LENGTHS), NN_N, m, ptr(x1), ptr(lens), ptr(x2), ptr(d), ptr(ix), variant, stream_ptr(cuda))
        assert rc == 0
        assert np.array_equal(host(ix), wi) and np.array_equal(host(d), wd), variant
    from pointnet2_amd.pointnet_util import three_nn_weights
    widx, w = three_nn_weights(x1, x2, lengths1=lens)
    assert torch.isfinite(w).all() and np.array_equal(host(widx), wi)


# ------------------------------------------------------------------------------------------------------ sample_and_group
@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("knn", [False, True])
@pytest.mark.parametrize("with_points", [False, True])
def test_sample_and_group_ragged(cuda, knn, with_points, padding):
    """against the composition of the ragged operators checked above (idx never names a padding row, so NaN padding in xyz
    and in the features reaches no output)"""
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import sample_and_group
    lengths = [1024, 700, 300, 64]
    xyz = S.sphere_clouds(4, 1024, 51)
    x = dev(padded(xyz, lengths, padding), cuda)
    feats = np.random.default_rng(52).random((4, 1024, 6), dtype=np.float32)
    for i, ni in enumerate(lengths):
        feats[i, ni:] = np.nan if padding == "nan" else 1e6
    pts = dev(feats, cuda) if with_points else None
    new_xyz, new_points, idx, grouped_xyz = sample_and_group(64, 0.2, 16, x, pts, knn=knn, lengths=lengths)
    fps, wxyz = P.farthest_point_sample_gather(64, x, lengths=lengths)
    if knn:
        _, widx = P.knn_point(16, x, wxyz, lengths1=lengths)
    else:
        widx, _ = P.query_ball_point(0.2, 16, x, wxyz, lengths1=lengths)
    assert torch.equal(new_xyz, wxyz) and torch.equal(idx, widx)
    assert (host(idx) < np.asarray(lengths)[:, None, None]).all()
    wg = P.group_point(x, widx) - wxyz.unsqueeze(2)
    assert torch.equal(grouped_xyz, wg) and torch.isfinite(grouped_xyz).all()
    want = torch.cat([wg, P.group_point(pts, widx)], dim=-1) if with_points else wg
    assert torch.equal(new_points, want) and torch.isfinite(new_points).all()


# ------------------------------------------------------------------------------------------------------------- gradients
def test_group_point_gradient_on_ragged_geometry(cuda, oracle):
    """group_point on a ragged level's idx, deterministic mode. The gradient into `points` is exactly zero on the padding rows.
    On the valid rows it is the gradient of the slice: bit for bit the CPU oracle's (this call -- 4 clouds, 1024 rows, 1024
    references each -- is one the segmented reduction sums in the CPU loop's order, INTEGRATION.md C'', and that order does
    not depend on the batch), and equal to the dense operator run on the slice alone within fp32 summation error: a
    one-cloud call is documented to take the fixed-point sums (b < 4), i.e. the exactly rounded sum, from which a sequential
    fp32 sum of r addends differs by at most r 2^-24 sum|addend|; one more 2^-24 sum|addend| covers the final rounding."""
    import pointnet2_amd as P
    lengths = [1024, 700, 300, 64]
    x = dev(padded(S.sphere_clouds(4, 1024, 61), lengths, "nan"), cuda)
    _, q = P.farthest_point_sample_gather(64, x, lengths=lengths)
    idx, _ = P.query_ball_point(0.2, 16, x, q, lengths1=lengths)
    torch.manual_seed(62)
    pts = torch.randn(4, 1024, 16, device=cuda, requires_grad=True)
    w = torch.randn(4, 64, 16, 16, device=cuda)
    was = P.is_deterministic()
    P.set_deterministic(True)
    try:
        (P.group_point(pts, idx) * w).sum().backward()
        for i, ni in enumerate(lengths):
            assert int((pts.grad[i, ni:] != 0).sum()) == 0                  # exactly zero on the padding rows
            idx_i, w_i = host(idx[i:i + 1]), host(w[i:i + 1])
            want = oracle.group_point_grad((1, ni, 16), idx_i, w_i)
            assert np.array_equal(host(pts.grad[i:i + 1, :ni]), want), i
            sl = pts.detach()[i:i + 1, :ni].clone().requires_grad_(True)
            (P.group_point(sl, idx[i:i + 1].contiguous()) * w[i:i + 1]).sum().backward()
            refs = np.bincount(idx_i.reshape(-1), minlength=ni).astype(np.float64)[None, :, None]
            bound = (refs + 1.0) * 2.0 ** -24 * oracle.group_point_grad((1, ni, 16), idx_i, np.abs(w_i)).astype(np.float64)
            diff = np.abs(host(sl.grad).astype(np.float64) - want)
            print("cloud %d: max |slice grad - batch grad| = %.3e, largest share of its bound %.3f"
                  % (i, diff.max(), (diff / np.maximum(bound, 1e-300)).max()))
            assert (diff <= bound).all(), i
    finally:
        P.set_deterministic(was)
