"""The second side of packed batches through the Python operators on the GPU (set_packed_pairs(True); include/pn2ops.h "the second
side, packed"): per-cloud sample counts in FPS, a ragged query side in the ball queries, packed kNN, sample_and_group on both.

THE PAIR SLICE RULE COMBINED WITH THE SLICE RULE, PACKED: for cloud c with m_c valid rows on the second side, rows j < m_c are
bit- and index-identical to the dense operator on (flat[offsets[c] : offsets[c + 1]], xyz2[c, :m_c]) alone; rows j >= m_c hold
the padded twin's fills, with offsets[c] where the local form writes index 0. The expectations come from the CPU oracle applied
per slice pair, computed once per case (shared with the one-sided packed tests and the padded pair tests where the shapes are
theirs); every case is also compared with the _ragged_counts / _ragged_pair operator on the NaN-padded copy. All comparisons are
exact. The query rows at or beyond m_c hold NaN: a read of one would reach an output.

Every cloud is drawn in the same unit cube or sphere, so a read across a cloud boundary changes a result. Each set of counts runs
in the order given and in a rotation whose slab starts are no multiple of 4 (asserted)."""
import functools

import numpy as np
import pytest
import torch

import test_packed_gpu as TP
import test_packed_msg_gpu as PM
import test_ragged_pair_gpu as RP
from test_packed_gpu import bits, dev, host, packed, padded, rotate, starts_are_unaligned

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def pairs_on():
    import pointnet2_amd as P
    from pointnet2_amd import _tensors
    before = _tensors.packed_pairs()
    P.set_packed_pairs(True)
    try:
        yield
    finally:
        P.set_packed_pairs(before)


def counts_t(counts, cuda):
    return torch.tensor(list(counts), dtype=torch.int32, device=cuda)


# ------------------------------------------------------------------------------------------------------------------- FPS
FPS_M, FPS_NPOINTS = TP.FPS_M, (64, 17, 40, 5)              # clouds (1100, 513, 40, 1): m_c < n_c, m_c < n_c, m_c = n_c, m_c > n_c = 1


def fps_want(cl, want, npoints, offs_h, global_idx):
    """the oracle's first m_c samples of each slice, then the fill: index 0 (offsets[c]) and the cloud's first point"""
    wi = np.zeros((len(cl), FPS_M), dtype=np.int32)
    wx = np.zeros((len(cl), FPS_M, 3), dtype=np.float32)
    for c, (pts, w, mc) in enumerate(zip(cl, want, npoints)):
        wi[c, :mc] = w[:mc]
        wx[c] = pts[wi[c]]
        if global_idx:
            wi[c] += offs_h[c]
    return wi, wx


@pytest.mark.parametrize("by", [0, 1])
@pytest.mark.parametrize("tier,variant,nmax,counts", TP.FPS_TIERS, ids=[t[0] for t in TP.FPS_TIERS])
def test_fps_packed_counts_every_tier(cuda, oracle, tier, variant, nmax, counts, by):
    import pointnet2_amd as P
    from pointnet2_amd import tf_sampling
    cl, want = TP.fps_case(counts, FPS_M, 71)                                # the one-sided test's clouds and oracle samples
    cl, want, npoints = rotate(cl, by), rotate(want, by), rotate(FPS_NPOINTS, by)
    flat, offs, offs_h = packed(cl, cuda)
    assert by == 0 or starts_are_unaligned(offs_h)
    cnts = counts_t(npoints, cuda)
    xp, lens = padded(cl, nmax, cuda)
    tf_sampling.set_fps_variant(variant)
    try:
        idx, new_xyz = P.farthest_point_sample_gather(FPS_M, flat, offsets=offs, max_points=nmax, npoints=cnts)
        gidx, gxyz = P.farthest_point_sample_gather(FPS_M, flat, offsets=offs, max_points=nmax, npoints=cnts, global_idx=True)
        only = P.farthest_point_sample(FPS_M, flat, offsets=offs, max_points=nmax, npoints=cnts)
        gonly = P.farthest_point_sample(FPS_M, flat, offsets=offs, max_points=nmax, npoints=cnts, global_idx=True)
        ridx, rxyz = P.farthest_point_sample_gather(FPS_M, xp, lengths=lens, npoints=cnts)   # the _ragged_counts entry, padded copy
    finally:
        tf_sampling.set_fps_variant(0)
    wi, wx = fps_want(cl, want, npoints, offs_h, False)
    gi, _ = fps_want(cl, want, npoints, offs_h, True)
    assert np.array_equal(host(idx), wi) and np.array_equal(host(bits(new_xyz)), wx.view(np.int32))
    assert np.array_equal(host(gidx), gi) and torch.equal(bits(gxyz), bits(new_xyz))
    assert torch.equal(only, idx) and torch.equal(gonly, gidx)
    assert torch.equal(idx, ridx) and torch.equal(bits(new_xyz), bits(rxyz))
    for c, mc in enumerate(npoints):                                         # the fill rows, spelled out
        assert not host(idx)[c, mc:].any() and (host(gidx)[c, mc:] == offs_h[c]).all()
        assert np.array_equal(host(new_xyz)[c, mc:], np.broadcast_to(cl[c][0], (FPS_M - mc, 3)))
    lo, hi = np.asarray(offs_h[:-1])[:, None], np.asarray(offs_h[1:])[:, None]
    assert (host(gidx) >= lo).all() and (host(gidx) < hi).all()              # every stored index names a row of its own cloud
    assert not getattr(new_xyz, "_pn2_fps_ordered", False)                   # fill rows break the farthest-point order


def test_fps_packed_counts_are_clamped_on_the_device(cuda, oracle):
    import pointnet2_amd as P
    cl, _ = TP.fps_case(TP.FPS_COUNTS, FPS_M, 71)
    flat, offs, offs_h = packed(cl, cuda)
    raw = [0, FPS_M + 5, -2, 7]
    clamped = [min(max(v, 1), FPS_M) for v in raw]
    for global_idx in (False, True):
        got = P.farthest_point_sample_gather(FPS_M, flat, offsets=offs, max_points=1100, npoints=counts_t(raw, cuda), global_idx=global_idx)
        want = P.farthest_point_sample_gather(FPS_M, flat, offsets=offs, max_points=1100, npoints=counts_t(clamped, cuda),
                                              global_idx=global_idx)
        assert torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1]))
        local = host(got[0]) - (np.asarray(offs_h[:-1])[:, None] if global_idx else 0)
        assert (local >= 0).all() and (local < np.asarray(TP.FPS_COUNTS)[:, None]).all()     # nothing out of range
    full = P.farthest_point_sample_gather(FPS_M, flat, offsets=offs, max_points=1100)
    assert torch.equal(got[0][1] - offs_h[1], full[0][1])                    # m + 5 computes on m: the one-sided rows


# ----------------------------------------------------------------------------------------------------------- ball query
BQ_LENGTHS2 = (32, 1, 17, 5)                                 # clouds (300, 64, 2048, 63), m = 32, the last 8 queries far away


def nan_beyond(q, lengths2, cuda):
    """the queries on the device with NaN in the rows at or beyond each count: never read"""
    qd = dev(q, cuda).clone()
    for c, mc in enumerate(lengths2):
        qd[c, mc:] = float("nan")
    return qd


def check_pair(outs, want, lengths2, base, none_idx=False):
    """outs: idx (minus base compared), pts_cnt, grouped; want: the oracle's idx, cnt, grouped for all m rows (those below m_c
    are the slice pair's: a query's row depends on no other query)"""
    idx, cnt, grp = outs
    widx, wcnt, wgrp = want
    assert (idx is None) == none_idx
    for c, mc in enumerate(lengths2):
        if idx is not None:
            local = host(idx[c]) - (base[c] if base is not None else 0)
            assert np.array_equal(local[:mc], widx[c, :mc]) and not local[mc:].any(), c
        assert np.array_equal(host(cnt[c, :mc]), wcnt[c, :mc]) and not host(cnt[c, mc:]).any(), c
        assert np.array_equal(host(grp[c, :mc]), wgrp[c, :mc]) and not host(bits(grp[c, mc:])).any(), c   # the fill: +0.0, bit for bit


def same_triple(a, b, shift=None):
    ia = a[0] if shift is None or a[0] is None else a[0] - shift
    return (ia is None) == (b[0] is None) and (ia is None or torch.equal(ia, b[0])) and torch.equal(a[1], b[1]) and \
        torch.equal(bits(a[2]), bits(b[2]))


@pytest.mark.parametrize("by", [0, 3])
@pytest.mark.parametrize("global_idx", [0, 1])
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("radius", TP.BQ_RADII)
def test_ball_query_packed_pair(cuda, oracle, radius, kernel, global_idx, by):
    import pointnet2_amd as P
    from pointnet2_amd import tf_grouping
    cl, out = TP.bq_case(TP.BQ_COUNTS, TP.BQ_M, radius, TP.BQ_NS, 73)        # the one-sided test's clouds, queries and oracle rows
    cl, out, l2 = rotate(cl, by), rotate(out, by), rotate(BQ_LENGTHS2, by)
    q, widx, wcnt, wgrp, wraw = (np.stack([o[k] for o in out]) for k in range(5))
    flat, offs, offs_h = packed(cl, cuda)
    assert by != 3 or starts_are_unaligned(offs_h)
    qd, cnts = nan_beyond(q, l2, cuda), counts_t(l2, cuda)
    xp, lens = padded(cl, TP.BQ_NMAX, cuda)
    base = offs_h[:-1] if global_idx else None
    kw = dict(offsets=offs, max_points=TP.BQ_NMAX, lengths2=cnts, global_idx=bool(global_idx))
    before = list(tf_grouping._BQ_KERNEL)
    tf_grouping.set_ball_query_kernel(kernel)
    try:
        fused = P.query_ball_group_xyz(radius, TP.BQ_NS, flat, qd, True, **kw)
        idx2, cnt2 = P.query_ball_point(radius, TP.BQ_NS, flat, qd, **kw)
        raw = P.query_ball_group_xyz(radius, TP.BQ_NS, flat, qd, False, want_idx=False, **kw)
        twin = P.query_ball_group_xyz(radius, TP.BQ_NS, xp, qd, True, lengths1=lens, lengths2=cnts)   # the _ragged_pair entry
    finally:
        tf_grouping.set_ball_query_kernel(*before)
    check_pair(fused, (widx, wcnt, wgrp), l2, base)
    check_pair(raw, (widx, wcnt, wraw), l2, base, none_idx=True)
    assert torch.equal(idx2, fused[0]) and torch.equal(cnt2, fused[1])
    assert same_triple(fused, twin, offs[:-1, None, None] if global_idx else None)
    lo, hi = np.asarray(offs_h[:-1])[:, None, None], np.asarray(offs_h[1:])[:, None, None]
    if global_idx:
        assert (host(fused[0]) >= lo).all() and (host(fused[0]) < hi).all()  # fill rows included: offsets[c], the cloud's own first row


@pytest.mark.parametrize("global_idx", [0, 1])
@pytest.mark.parametrize("kernel", [1, 2])
def test_ball_query_packed_pair_many_workgroups_per_cloud(cuda, oracle, kernel, global_idx):
    """The padded pair test's m = 640 case, packed: b m = 3200 gives the sweep kernel 16 queries per workgroup (40 per cloud)
    and the cell-list kernel 64 (10 per cloud). With lengths2 = (640, 65, 1, 64, 600) cloud 1 has workgroups of valid rows only,
    one of both kinds and -- from row 80 / 128 on -- workgroups of fill rows alone, which leave before the staging; cloud 3 (64)
    ends on a workgroup boundary of both kernels."""
    import pointnet2_amd as P
    from pointnet2_amd import tf_grouping
    xyz, q, wi, wc, wg, _ = RP.bq_case(640, 0.2, 32)
    l1, l2 = RP.BQ_LENGTHS1, RP.BQ_SHAPES[640]
    assert 640 >= 3 * 64 and l2[1] == 65
    cl = [xyz[c, :n] for c, n in enumerate(l1)]
    flat, offs, offs_h = packed(cl, cuda)
    qd, cnts = nan_beyond(q, l2, cuda), counts_t(l2, cuda)
    before = list(tf_grouping._BQ_KERNEL)
    tf_grouping.set_ball_query_kernel(kernel)
    try:
        got = P.query_ball_group_xyz(0.2, 32, flat, qd, True, offsets=offs, max_points=RP.BQ_N, lengths2=cnts, global_idx=bool(global_idx))
        twin = P.query_ball_group_xyz(0.2, 32, padded(cl, RP.BQ_N, cuda)[0], qd, True, lengths1=counts_t(l1, cuda), lengths2=cnts)
    finally:
        tf_grouping.set_ball_query_kernel(*before)
    check_pair(got, (wi, wc, wg), l2, offs_h[:-1] if global_idx else None)
    assert same_triple(got, twin, offs[:-1, None, None] if global_idx else None)


@pytest.mark.parametrize("global_idx", [0, 1])
def test_ball_query_packed_pair_global_memory_sweep(cuda, oracle, global_idx):
    """max_points above the LDS sweep's cloud size, as in the one-sided test"""
    import pointnet2_amd as P
    from pointnet2_amd import tf_grouping
    counts, m, l2 = (33, 9700, 7), 8 + TP.BQ_FAR, (16, 3, 1)
    cl, out = TP.bq_case(counts, m, 0.1, 16, 74)
    q, widx, wcnt, wgrp, _ = (np.stack([o[k] for o in out]) for k in range(5))
    flat, offs, offs_h = packed(cl, cuda)
    qd, cnts = nan_beyond(q, l2, cuda), counts_t(l2, cuda)
    before = list(tf_grouping._BQ_KERNEL)
    try:
        for kernel in (0, 1):
            tf_grouping.set_ball_query_kernel(kernel)
            got = P.query_ball_group_xyz(0.1, 16, flat, qd, True, offsets=offs, max_points=9700, lengths2=cnts, global_idx=bool(global_idx))
            check_pair(got, (widx, wcnt, wgrp), l2, offs_h[:-1] if global_idx else None)
    finally:
        tf_grouping.set_ball_query_kernel(*before)


def test_ball_query_packed_pair_full_counts_is_the_one_sided_call(cuda):
    import pointnet2_amd as P
    cl, out = TP.bq_case(TP.BQ_COUNTS, TP.BQ_M, 0.4, TP.BQ_NS, 73)
    flat, offs, _ = packed(cl, cuda)
    qd = dev(np.stack([o[0] for o in out]), cuda)
    a = P.query_ball_group_xyz(0.4, TP.BQ_NS, flat, qd, True, offsets=offs, max_points=TP.BQ_NMAX, global_idx=True,
                               lengths2=[TP.BQ_M] * len(cl))
    b = P.query_ball_group_xyz(0.4, TP.BQ_NS, flat, qd, True, offsets=offs, max_points=TP.BQ_NMAX, global_idx=True)
    assert same_triple(a, b)


# --------------------------------------------------------------------------------------------------------- multi-radius
MSG_CASES = [("binned_mixed", (704, 1, 300, 64)), ("swept", (100, 1))]       # lengths2 includes 1 and m


def run_msg_pair(cuda, oracle, key, scales, lengths, lengths2, max_points=None):
    import pointnet2_amd as P
    import ball_msg_cases as M
    radii, nss = [s[0] for s in scales], [s[1] for s in scales]
    nmax = M.INPUTS[key][1] if max_points is None else max_points
    assert max(lengths2) == M.INPUTS[key][2] and min(lengths2) == 1
    for clouds, counts in PM._orders(lengths):
        flat, qd, offs, xp, qs, offsets = PM._batch(key, clouds, counts, cuda)
        l2 = [lengths2[c] for c in clouds]
        qd = nan_beyond(qs, l2, cuda)
        lens, cnts = counts_t(counts, cuda), counts_t(l2, cuda)
        twin = P.query_ball_group_xyz_msg(radii, nss, xp, qd, True, lengths1=lens, lengths2=cnts)
        for global_idx in (False, True):
            outs = P.query_ball_group_xyz_msg(radii, nss, flat, qd, True, offsets=offs, max_points=nmax, lengths2=cnts, global_idx=global_idx)
            assert len(outs) == len(scales)
            shift = offs[:-1].view(-1, 1, 1) if global_idx else None
            for (r, k), got, tw in zip(scales, outs, twin):
                want = [PM._want(oracle, key, c, n, r, k) for c, n in zip(clouds, counts)]       # all m rows of each slice, cached
                widx, wcnt, wraw = (np.stack([w[j] for w in want]) for j in range(3))
                check_pair(got, (widx, wcnt, wraw - qs[:, :, None, :]), l2, offsets[:-1] if global_idx else None)
                one = P.query_ball_group_xyz(r, k, flat, qd, True, offsets=offs, max_points=nmax, lengths2=cnts, global_idx=global_idx)
                assert same_triple(got, one), (key, r, global_idx)
                assert same_triple(got, tw, shift), (key, r, global_idx)


@pytest.mark.parametrize("name,lengths2", MSG_CASES, ids=[c[0] for c in MSG_CASES])
def test_multi_radius_packed_pair(cuda, oracle, name, lengths2):
    import ragged_msg_cases as R
    _, key, scales, lengths, _ = R.CASES[R.IDS.index(name)]
    run_msg_pair(cuda, oracle, key, scales, lengths, lengths2)


def test_multi_radius_packed_pair_five_radii_take_the_per_radius_operator(cuda, oracle):
    """more radii than the one launch holds: the front falls back to the single-radius packed pair operator per radius"""
    five = [(0.05, 8), (0.1, 16), (0.2, 32), (0.3, 16), (0.4, 64)]
    run_msg_pair(cuda, oracle, "small", five, [600, 37], (100, 1))


# ------------------------------------------------------------------------------------------------------------------ kNN
KNN_COUNTS, KNN_SAME, KNN_NMAX, KNN_M = (1500, 600, 40, 1), 1100, 1500, 64
KNN_LENGTHS2 = (64, 9, 1, 33, 64)
KNN_KS = [8, 32, 48]                                         # 48 > 40: the repeat-entry-0 rule; <= 40 / > 40: both ways to the threshold.
# KNN_SAME > kKnnCap = 1024 (csrc/topk.hip): a cloud of identical points ties more candidates than the replay holds -- the literal rounds


@functools.lru_cache(maxsize=None)
def knn_clouds():
    from pointnet2_amd import synthetic as S
    rng = np.random.default_rng(81)
    sphere = S.sphere_clouds(len(KNN_COUNTS), max(KNN_COUNTS), 82)
    cl = [np.ascontiguousarray(sphere[c, :n]) for c, n in enumerate(KNN_COUNTS)]
    cl.append(np.tile(sphere[0, 7:8], (KNN_SAME, 1)))                        # 1100 copies of one point of the sphere: > kKnnCap ties
    q = []
    for pts in cl:
        qc = pts[rng.integers(0, len(pts), size=KNN_M)].copy()
        qc[::2] += rng.normal(0, 0.05, size=qc[::2].shape).astype(np.float32)
        q.append(qc)
    return cl, np.stack(q)


@functools.lru_cache(maxsize=None)
def knn_case(k):
    """as knn_case of tests/test_ragged_pair_gpu.py, per slice: the fp32 distance matrix, the oracle's swap rounds, the first k
    columns; k > n_c: the entries from n_c on repeat entry 0. All m rows (a query's row depends on no other query)."""
    import oracle as O
    cl, q = knn_clouds()
    wi = np.zeros((len(cl), KNN_M, k), dtype=np.int32)
    wv = np.zeros((len(cl), KNN_M, k), dtype=np.float32)
    for c, pts in enumerate(cl):
        sl = pts[None]
        dx = sl[:, None, :, 0] - q[c][None, :, None, 0]
        dy = sl[:, None, :, 1] - q[c][None, :, None, 1]
        dz = sl[:, None, :, 2] - q[c][None, :, None, 2]
        d = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
        kk = min(k, len(pts))
        oi, ov = O.select_top_k(kk, d)
        wi[c, :, :kk], wv[c, :, :kk] = oi[0, :, :kk], ov[0, :, :kk]
        wi[c, :, kk:], wv[c, :, kk:] = oi[0, :, :1], ov[0, :, :1]
    return wi, wv


@pytest.mark.parametrize("by", [0, 3])
@pytest.mark.parametrize("global_idx", [0, 1])
@pytest.mark.parametrize("ragged_queries", [False, True])
@pytest.mark.parametrize("k", KNN_KS)
def test_knn_packed(cuda, oracle, k, ragged_queries, global_idx, by):
    import pointnet2_amd as P
    cl, q = knn_clouds()
    wi, wv = knn_case(k)
    order = rotate(list(range(len(cl))), by)
    cl, q, wi, wv = [cl[c] for c in order], q[order], wi[order], wv[order]
    l2 = [KNN_LENGTHS2[c] for c in order] if ragged_queries else [KNN_M] * len(cl)
    flat, offs, offs_h = packed(cl, cuda)
    assert by == 0 or starts_are_unaligned(offs_h)                          # (1, 1100, 1500, 600, 40): 1, 1101, 2601, 3201
    qd = nan_beyond(q, l2, cuda)
    cnts = counts_t(l2, cuda) if ragged_queries else None
    val, idx = P.knn_point(k, flat, qd, lengths2=cnts, offsets=offs, max_points=KNN_NMAX, global_idx=bool(global_idx))
    assert tuple(val.shape) == (len(cl), KNN_M, k) and tuple(idx.shape) == (len(cl), KNN_M, k)
    xp, lens = padded(cl, KNN_NMAX, cuda)
    rval, ridx = P.knn_point(k, xp, qd, lengths1=lens, lengths2=cnts)        # the _ragged / _ragged_pair entry on the padded copy
    base = np.asarray(offs_h[:-1])[:, None, None] if global_idx else 0
    local = host(idx) - base
    for c, mc in enumerate(l2):
        assert np.array_equal(local[c, :mc], wi[c, :mc]), c
        assert np.array_equal(host(bits(val[c, :mc])), wv[c, :mc].view(np.int32)), c
        assert not local[c, mc:].any() and not host(bits(val[c, mc:])).any(), c                  # the fill: idx 0 (offsets[c]), +0.0
        if len(cl[c]) == 1:
            assert not local[c].any()                                        # every entry is entry 0
        if len(cl[c]) < k:
            assert (local[c, :mc, len(cl[c]):] == local[c, :mc, :1]).all()   # the repeat-entry-0 rule
    assert (local >= 0).all() and (local < np.asarray([len(p) for p in cl])[:, None, None]).all()
    assert np.array_equal(local, host(ridx)) and torch.equal(bits(val), bits(rval))


# ------------------------------------------------------------------------------------------------------ sample_and_group
SG_COUNTS, SG_NPOINTS = (97, 33, 64, 1), (16, 5, 1, 9)


@pytest.mark.parametrize("knn", [False, True])
@pytest.mark.parametrize("with_points", [False, True])
def test_sample_and_group_packed_counts_equals_the_padded_call(cuda, knn, with_points):
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import sample_and_group
    cl = TP.clouds(SG_COUNTS, 83)
    flat, offs, _ = packed(cl, cuda)
    feats = torch.rand(flat.shape[0], 6, device=cuda) if with_points else None
    xp, lens = padded(cl, 97, cuda, fill=0.0)
    fp = P.unpack_batch(feats, offs, n=97)[0] if with_points else None
    cnts = counts_t(SG_NPOINTS, cuda)
    new_xyz, new_points, idx, grouped_xyz = sample_and_group(16, 0.3, 8, flat, feats, knn=knn, offsets=offs, max_points=97, npoints=cnts)
    wxyz, wpoints, widx, wgrouped = sample_and_group(16, 0.3, 8, xp, fp, knn=knn, lengths=lens, npoints=cnts)
    assert torch.equal(bits(new_xyz), bits(wxyz)) and torch.equal(bits(grouped_xyz), bits(wgrouped))
    assert torch.equal(bits(new_points), bits(wpoints))
    assert torch.equal(idx, widx + offs[:-1, None, None])                    # idx is global, the fill rows offsets[c]
    for c, mc in enumerate(SG_NPOINTS):
        assert not host(widx)[c, mc:].any() and not host(bits(grouped_xyz[c, mc:])).any()
    # knn without counts: the one-sided packed kNN in the ball query's place
    if knn:
        a = sample_and_group(16, 0.3, 8, flat, feats, knn=True, offsets=offs, max_points=97)
        w = sample_and_group(16, 0.3, 8, xp, fp, knn=True, lengths=lens)
        assert torch.equal(bits(a[0]), bits(w[0])) and torch.equal(bits(a[1]), bits(w[1])) and torch.equal(a[2], w[2] + offs[:-1, None, None])


# -------------------------------------------------------------------------------------------------------------- capture
def test_capture_and_replay_with_new_offsets_and_counts(cuda):
    """FPS with counts + ball query pair + kNN captured into one graph on one stream; offsets and npoints are overwritten in place
    (another partition of the same rows, other counts); the replay gives the eager call's bits on the new values."""
    import pointnet2_amd as P
    first, second = ((97, 33, 64), (16, 5, 1)), ((40, 121, 33), (3, 16, 9))
    flat = dev(np.concatenate(TP.clouds((194,), 84)), cuda)
    offs = dev(np.concatenate([[0], np.cumsum(first[0])]).astype(np.int32), cuda)
    cnts = counts_t(first[1], cuda)

    def step():
        fps, new_xyz = P.farthest_point_sample_gather(16, flat, offsets=offs, max_points=128, npoints=cnts, global_idx=True)
        idx, cnt, grp = P.query_ball_group_xyz(0.3, 8, flat, new_xyz, True, offsets=offs, max_points=128, lengths2=cnts, global_idx=True)
        val, kidx = P.knn_point(8, flat, new_xyz, lengths2=cnts, offsets=offs, max_points=128, global_idx=True)
        return fps, new_xyz, idx, cnt, grp, val, kidx
    side = torch.cuda.Stream()                                               # warm on a side stream, as a capture wants it
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        old = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    offs.copy_(dev(np.concatenate([[0], np.cumsum(second[0])]).astype(np.int32), cuda))
    cnts.copy_(counts_t(second[1], cuda))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in captured]
    want = step()
    assert sum(first[0]) == sum(second[0])
    assert not any(torch.equal(a, b) for a, b in zip(got[:3], old[:3]))      # the replay did see the new values
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want))
