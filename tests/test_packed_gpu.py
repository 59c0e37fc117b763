"""Packed batches through the Python operators on the GPU (offsets= / max_points=; include/pn2ops.h "packed batches").

THE SLICE RULE, PACKED: for cloud c the result is bit- and index-identical to the dense operator on
flat[offsets[c] : offsets[c + 1]] alone. The expectations come from the CPU oracle applied to every slice, computed once per
case; every case is also compared with the `_ragged` operator on the same clouds padded. All comparisons are exact
(torch.equal / np.array_equal on int32 views of the floats).

Every cloud is drawn in the same unit cube, so a read across a cloud boundary lands on points that WOULD enter the
neighbour's balls, neighbour lists and arg-max rounds: it changes a result. Each set of counts runs in the order given and
in a rotation of it chosen so that every slab behind the first starts at a row that is odd or no multiple of 4 (offsets[0] is
0 by definition; the test asserts the starts); the expectation of a cloud does not depend on where it lies."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def clouds(counts, seed):
    """One uniform cloud per count, all in [0, 1)^3."""
    rng = np.random.default_rng(seed)
    return [rng.random((n, 3), dtype=np.float32) for n in counts]


def rotate(items, by):
    return list(items[by:]) + list(items[:by])


def packed(cl, cuda):
    """-> flat (total, 3), offsets (b + 1,) int32 on the device, offsets as a host list"""
    offs = np.concatenate([[0], np.cumsum([len(c) for c in cl])]).astype(np.int32)
    return dev(np.concatenate(cl), cuda), dev(offs, cuda), offs.tolist()


def padded(cl, n, cuda, fill=np.nan):
    out = np.full((len(cl), n, 3), fill, dtype=np.float32)
    for i, c in enumerate(cl):
        out[i, :len(c)] = c
    return dev(out, cuda), torch.tensor([len(c) for c in cl], dtype=torch.int32, device=cuda)


def starts_are_unaligned(offs):
    return all(o % 4 != 0 for o in offs[1:-1])


# ------------------------------------------------------------------------------------------------------------------- FPS
FPS_COUNTS, FPS_M = (1100, 513, 40, 1), 64                   # Q_c = 3, 2, 1, 1; m > n_c twice
FPS_AUTO_COUNTS, FPS_AUTO_M = (5, 130, 77), 16               # m > n_c once


@functools.lru_cache(maxsize=None)
def fps_case(counts, m, seed):
    import oracle as O
    cl = clouds(counts, seed)
    want = [O.farthest_point_sample(m, c[None])[0] for c in cl]
    return cl, want


# variant (tf_sampling.FPS_*), max_points. The pruned tier exists from 2049 rank slots on, so it runs the same clouds under
# the bound 2049 -- max_points is a bound, not the longest cloud -- and once more on a cloud that needs its size.
FPS_TIERS = [("register", 1, 1100, FPS_COUNTS), ("batched", 3, 1100, FPS_COUNTS), ("pruned", 2, 2049, FPS_COUNTS),
             ("pruned_2100", 2, 2100, (2100, 513, 40, 1)), ("batched_2100", 3, 2100, (2100, 513, 40, 1)),
             ("auto", 0, 1100, FPS_COUNTS)]


@pytest.mark.parametrize("by", [0, 1])
@pytest.mark.parametrize("tier,variant,nmax,counts", FPS_TIERS, ids=[t[0] for t in FPS_TIERS])
def test_fps_packed_every_tier(cuda, oracle, tier, variant, nmax, counts, by):
    import pointnet2_amd as P
    from pointnet2_amd import tf_sampling
    cl, want = fps_case(counts, FPS_M, 71)
    cl, want = rotate(cl, by), np.stack(rotate(want, by))
    flat, offs, offs_h = packed(cl, cuda)
    assert by == 0 or starts_are_unaligned(offs_h)                          # 513, 553, 554
    xp, lens = padded(cl, nmax, cuda)
    tf_sampling.set_fps_variant(variant)
    try:
        idx, new_xyz = P.farthest_point_sample_gather(FPS_M, flat, offsets=offs, max_points=nmax)
        gidx, gxyz = P.farthest_point_sample_gather(FPS_M, flat, offsets=offs, max_points=nmax, global_idx=True)
        only = P.farthest_point_sample(FPS_M, flat, offsets=offs, max_points=nmax)
        ridx, rxyz = P.farthest_point_sample_gather(FPS_M, xp, lengths=lens)       # the _ragged entry on the padded copy
    finally:
        tf_sampling.set_fps_variant(0)
    assert np.array_equal(host(idx), want)
    assert np.array_equal(host(new_xyz), np.stack([c[w] for c, w in zip(cl, want)]))
    assert torch.equal(idx, only) and torch.equal(idx, ridx) and torch.equal(bits(new_xyz), bits(rxyz))
    assert torch.equal(gidx, idx + offs[:-1, None]) and torch.equal(bits(gxyz), bits(new_xyz))     # global = local + offsets[c]
    assert torch.equal(flat[gidx.long()], new_xyz)


@pytest.mark.parametrize("by", [0, 1, 2])
def test_fps_packed_automatic_rule_small_clouds(cuda, oracle, by):
    import pointnet2_amd as P
    cl, want = fps_case(FPS_AUTO_COUNTS, FPS_AUTO_M, 72)
    cl, want = rotate(cl, by), np.stack(rotate(want, by))
    flat, offs, _ = packed(cl, cuda)
    idx, new_xyz = P.farthest_point_sample_gather(FPS_AUTO_M, flat, offsets=offs.long(), max_points=130)   # int64 offsets are converted
    assert np.array_equal(host(idx), want)
    assert np.array_equal(host(new_xyz), np.stack([c[w] for c, w in zip(cl, want)]))
    for c in range(3):                                                       # the dense operator on the slice, npoint > n included
        lo, hi = int(offs[c]), int(offs[c + 1])
        di, dx = P.farthest_point_sample_gather(FPS_AUTO_M, flat[lo:hi].unsqueeze(0).contiguous())
        assert torch.equal(idx[c:c + 1], di) and torch.equal(bits(new_xyz[c:c + 1]), bits(dx))


# ----------------------------------------------------------------------------------------------------------- ball query
BQ_COUNTS, BQ_NMAX, BQ_M, BQ_NS = (300, 64, 2048, 63), 2048, 32, 16
BQ_RADII = [0.08, 0.4]                                       # sparse balls (some hold < nsample points); crowded balls (rows padded with duplicates never, full rows always)
BQ_FAR = 8                                                   # the last queries of every cloud lie outside the cube: empty balls


@functools.lru_cache(maxsize=None)
def bq_case(counts, m, radius, nsample, seed):
    """queries: m - BQ_FAR of the cloud's own farthest-point samples (repeated where the cloud is smaller), then BQ_FAR far away"""
    import oracle as O
    cl = clouds(counts, seed)
    out = []
    for c in cl:
        sl = c[None]
        q = O.gather_point(sl, O.farthest_point_sample(m, sl)).copy()
        q[0, m - BQ_FAR:] += np.float32(10.0)
        ii, ci = O.query_ball_point(radius, nsample, sl, q)
        out.append((q[0], ii[0], ci[0], O.group_point(sl, ii)[0] - q[0][:, None, :], O.group_point(sl, ii)[0]))
    return cl, out


def run_ball_query(cuda, counts, nmax, m, radius, nsample, kernel, global_idx, by, seed):
    import pointnet2_amd as P
    from pointnet2_amd import tf_grouping
    cl, out = bq_case(counts, m, radius, nsample, seed)
    cl, out = rotate(cl, by), rotate(out, by)
    q, widx, wcnt, wgrp, wraw = (np.stack([o[k] for o in out]) for k in range(5))
    flat, offs, offs_h = packed(cl, cuda)
    assert by != 3 or starts_are_unaligned(offs_h)                          # (63, 300, 64, 2048): 63, 363, 427
    qd = dev(q, cuda)
    xp, lens = padded(cl, nmax, cuda)
    base = offs[:-1, None, None] if global_idx else 0
    before = list(tf_grouping._BQ_KERNEL)
    tf_grouping.set_ball_query_kernel(kernel)
    try:
        idx, cnt, grp = P.query_ball_group_xyz(radius, nsample, flat, qd, True, offsets=offs, max_points=nmax, global_idx=global_idx)
        idx2, cnt2 = P.query_ball_point(radius, nsample, flat, qd, offsets=offs, max_points=nmax, global_idx=global_idx)
        none, _, raw = P.query_ball_group_xyz(radius, nsample, flat, qd, False, want_idx=False, offsets=offs, max_points=nmax,
                                              global_idx=global_idx)
        ridx, rcnt, rgrp = P.query_ball_group_xyz(radius, nsample, xp, qd, True, lengths1=lens)     # the _ragged entry, padded copy
    finally:
        tf_grouping.set_ball_query_kernel(*before)
    assert none is None
    assert np.array_equal(host(idx - base), widx) and np.array_equal(host(cnt), wcnt) and np.array_equal(host(grp), wgrp)
    assert torch.equal(idx2, idx) and torch.equal(cnt2, cnt)
    assert np.array_equal(host(raw), wraw)                                   # without the centroid
    assert torch.equal(idx - base, ridx) and torch.equal(cnt, rcnt) and torch.equal(bits(grp), bits(rgrp))
    assert int(cnt[:, m - BQ_FAR:].sum()) == 0 and int((idx - base)[:, m - BQ_FAR:].abs().sum()) == 0   # empty balls: zeros (+ offsets[c])
    if global_idx:                                                           # rows of the flat array: they gather the same points
        assert torch.equal(flat[idx.long()] - qd.unsqueeze(2), grp)
    return wcnt


@pytest.mark.parametrize("by", [0, 3])
@pytest.mark.parametrize("global_idx", [0, 1])
@pytest.mark.parametrize("kernel", [1, 2])                                 # 1: the sweep in LDS; 2: the cell list (the 63-point cloud takes the sweep body inside it)
@pytest.mark.parametrize("radius", BQ_RADII)
def test_ball_query_packed(cuda, oracle, radius, kernel, global_idx, by):
    wcnt = run_ball_query(cuda, BQ_COUNTS, BQ_NMAX, BQ_M, radius, BQ_NS, kernel, global_idx, by, 73)
    near = wcnt[:, :BQ_M - BQ_FAR]
    if radius == BQ_RADII[0]:
        assert (near < BQ_NS).any() and (near >= 1).all()                   # rows padded with duplicates of the first hit
    else:
        assert (near == BQ_NS).any()                                        # crowded balls: the sweep stops at nsample


@pytest.mark.parametrize("global_idx", [0, 1])
def test_ball_query_packed_global_memory_sweep(cuda, oracle, global_idx):
    """nmax above the LDS sweep's cloud size: the sweep that reads the cloud from global memory; the second cloud starts at
    row 9700 + ... of the flat array"""
    run_ball_query(cuda, (33, 9700, 7), 9700, 8 + BQ_FAR, 0.1, 16, 0, global_idx, 0, 74)
    run_ball_query(cuda, (33, 9700, 7), 9700, 8 + BQ_FAR, 0.1, 16, 1, global_idx, 0, 74)


# ------------------------------------------------------------------------------------------------------------- three_nn
NN_COUNTS, NN_M = (1, 2, 130, 257), 64


@functools.lru_cache(maxsize=None)
def nn_case(lengths2):
    import oracle as O
    unknown = clouds(NN_COUNTS, 75)
    known = np.random.default_rng(76).random((len(NN_COUNTS), NN_M, 3), dtype=np.float32)
    wd, wi = [], []
    for c, u in enumerate(unknown):
        mk = NN_M if lengths2 is None else lengths2[c]
        d, ix = O.three_nn(u[None], known[c:c + 1, :mk])
        wd.append(d[0]); wi.append(ix[0])
    return unknown, known, wd, wi


@pytest.mark.parametrize("by", [0, 1])
@pytest.mark.parametrize("variant", [1, 2])                                # the sweep, the cell list
@pytest.mark.parametrize("lengths2", [None, (64, 2, 1, 30)], ids=["dense_known", "ragged_known"])
def test_three_nn_packed(cuda, oracle, lengths2, variant, by):
    import pointnet2_amd as P
    from pointnet2_amd import tf_interpolate
    unknown, known, wd, wi = nn_case(lengths2)
    order = rotate(list(range(len(NN_COUNTS))), by)
    cl = [unknown[c] for c in order]
    kn = dev(known[order], cuda)
    if lengths2 is not None:                                               # the known rows beyond a count are never read
        for r, c in enumerate(order):
            kn[r, lengths2[c]:] = float("nan")
    l2 = None if lengths2 is None else torch.tensor([lengths2[c] for c in order], dtype=torch.int32, device=cuda)
    flat, offs, offs_h = packed(cl, cuda)
    assert by != 0 or starts_are_unaligned(offs_h)                          # (1, 2, 130, 257): 1, 3, 133
    want_d, want_i = np.concatenate([wd[c] for c in order]), np.concatenate([wi[c] for c in order])
    xp, lens = padded(cl, max(NN_COUNTS), cuda)
    tf_interpolate._NN_PACKED_VARIANT[0] = variant
    try:
        dist, idx = P.three_nn(flat, kn, offsets1=offs, max_points1=max(NN_COUNTS), lengths2=l2)
        gdist, gidx = P.three_nn(flat, kn, offsets1=offs, max_points1=max(NN_COUNTS), lengths2=l2, global_idx=True)
    finally:
        tf_interpolate._NN_PACKED_VARIANT[0] = 0
    assert dist.shape == (flat.shape[0], 3) and idx.shape == (flat.shape[0], 3)
    assert np.array_equal(host(idx), want_i)
    assert np.array_equal(host(bits(dist)), want_d.view(np.int32))           # +inf where a cloud has fewer than three known points
    if lengths2 is not None:
        assert np.isinf(host(dist)).any()
    # global: local + c m on every row of cloud c
    cloud_of_row = torch.repeat_interleave(torch.arange(len(cl), device=cuda), torch.tensor([len(c) for c in cl], device=cuda))
    assert torch.equal(gidx, idx + (cloud_of_row * NN_M).to(torch.int32)[:, None]) and torch.equal(bits(gdist), bits(dist))
    # the _ragged entries on the padded copy (their variant is the library's choice: results never depend on it)
    rd, ri = P.three_nn(xp, kn, lengths1=lens, lengths2=l2)
    for r in range(len(cl)):
        lo, hi = offs_h[r], offs_h[r + 1]
        assert torch.equal(idx[lo:hi], ri[r, :hi - lo]) and torch.equal(bits(dist[lo:hi]), bits(rd[r, :hi - lo]))


# ------------------------------------------------------------------------------------------------------ sample_and_group
def test_sample_and_group_packed_equals_the_padded_call(cuda):
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import sample_and_group
    counts = (97, 33, 64)
    cl = clouds(counts, 77)
    flat, offs, offs_h = packed(cl, cuda)
    feats = torch.rand(flat.shape[0], 6, device=cuda)
    xp, lens = padded(cl, 97, cuda, fill=0.0)
    fp, _ = P.unpack_batch(feats, offs, n=97)
    new_xyz, new_points, idx, grouped_xyz = sample_and_group(16, 0.3, 8, flat, feats, offsets=offs, max_points=97)
    wxyz, wpoints, widx, wgrouped = sample_and_group(16, 0.3, 8, xp, fp, lengths=lens)
    assert torch.equal(bits(new_xyz), bits(wxyz)) and torch.equal(bits(grouped_xyz), bits(wgrouped))
    assert torch.equal(bits(new_points), bits(wpoints))
    assert torch.equal(idx, widx + offs[:-1, None, None])                    # idx is global
    only_xyz = sample_and_group(16, 0.3, 8, flat, None, offsets=offs, max_points=97)[1]
    assert torch.equal(bits(only_xyz), bits(grouped_xyz))


def test_sample_and_group_packed_graph_replay_follows_offsets(cuda):
    """Captured once, replayed after offsets changed IN PLACE to another partition of the same rows: the host never read them."""
    from pointnet2_amd.pointnet_util import sample_and_group
    first, second = (97, 33, 64), (40, 121, 33)
    flat = dev(np.concatenate(clouds((194,), 78)), cuda)
    feats = torch.rand(194, 5, device=cuda)
    offs = dev(np.array([0, 97, 130, 194], dtype=np.int32), cuda)

    def step():
        return sample_and_group(16, 0.3, 8, flat, feats, offsets=offs, max_points=128)
    side = torch.cuda.Stream()                                               # warm on a side stream, as a capture wants it
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        old = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    offs.copy_(dev(np.concatenate([[0], np.cumsum(second)]).astype(np.int32), cuda))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in captured]
    want = step()
    assert sum(first) == sum(second)
    assert not all(torch.equal(a, b) for a, b in zip(got, old))               # the replay did see the new partition
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want))
