"""The algorithm behind pn2_knn_point (csrc/topk.hip), as a numpy model on the CPU: replaying the
reference's k swap rounds (tf_grouping_g.cu:83-123) on the candidate set {value <= tau}, tau >= v_k, with
slot tracking, gives exactly the first k outputs of the literal selection sort -- for ANY such tau
(including the loose bound from the per-lane minima) and on arrays full of exact ties. The HIP kernel is
checked against the oracle on the GPU (tests/test_parity_gpu.py); this pins the reasoning itself.

The second half models the kernel's own choice of tau on fp32 rows (kernel_tau) and evaluates it on every row of the edge-case
table (knn_edge_cases.py): which side of kKnnCap a case lands on is a condition on its inputs, asserted here without a GPU and
relied on by tests/test_knn_edge_gpu.py."""
import functools

import numpy as np

import knn_edge_cases as E


def literal_rounds(v, k):
    v = v.copy()
    idx = np.arange(len(v))
    for s in range(k):
        mn = s
        for t in range(s + 1, len(v)):
            if v[t] < v[mn]:
                mn = t
        if mn != s:
            v[mn], v[s] = v[s], v[mn]
            idx[mn], idx[s] = idx[s], idx[mn]
    return v[:k].copy(), idx[:k].copy()


def replay_on_candidates(v, k, tau):
    cand = [i for i in range(len(v)) if v[i] <= tau]
    pos = {c: c for c in cand}                       # current slot of every live candidate
    out_v, out_i = [], []
    for s in range(k):
        win = min(pos, key=lambda c: (v[c], pos[c]))
        q = pos.pop(win)
        out_v.append(v[win])
        out_i.append(win)
        if q != s:                                   # the swap: whoever sits at slot s moves to slot q
            for c in pos:
                if pos[c] == s:
                    pos[c] = q
    return np.array(out_v), np.array(out_i)


def lane_minima_bound(v, k):
    """k-th smallest of the 64 strided per-lane minima (what the kernel uses for k <= 40)."""
    mins = sorted(v[l::64].min() for l in range(min(64, len(v))))
    return mins[k - 1]


def test_replay_equals_literal_selection_sort_for_any_valid_tau():
    rng = np.random.default_rng(0)
    for trial in range(1500):
        n = int(rng.integers(2, 90))
        k = int(rng.integers(1, n + 1))
        v = rng.integers(0, int(rng.integers(1, 8)), size=n).astype(np.float64)      # heavy ties
        vk = np.sort(v)[k - 1]
        want = literal_rounds(v, k)
        for tau in (vk, vk + 0.5, vk + 3.0, v.max()):
            got = replay_on_candidates(v, k, tau)
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]), (trial, tau)


def test_lane_minima_bound_is_a_valid_threshold():
    rng = np.random.default_rng(1)
    for trial in range(300):
        n = int(rng.integers(64, 700))
        k = int(rng.integers(1, 41))
        v = np.round(rng.random(n) * rng.choice([4, 50, 1000])) / 7.0
        tau = lane_minima_bound(v, k)
        assert tau >= np.sort(v)[k - 1]
        want = literal_rounds(v, k)
        got = replay_on_candidates(v, k, tau)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]), trial


# ---- the kernel's tau on fp32 rows, and the edge-case table ---------------------------------------------------------------------
def key32(d):
    """orderable() of csrc/topk.hip: uint32 keys whose unsigned order is the floats' `<` order (-0 folded into +0; no NaN here)"""
    d = np.asarray(d, dtype=np.float32)
    assert not np.isnan(d).any()
    u = np.where(d == 0, np.float32(0), d).astype(np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def histogram_bound(v, k):
    """the kernel's tau for more than 40 rounds: the 16-bit prefix of the key of v_k, the low 16 bits set"""
    return np.uint32(np.sort(key32(v))[k - 1] | np.uint32(0xffff))


def histogram_bound_two_passes(v, k):
    """the same bound the way the kernel finds it: the 256-bin histogram of key bits 31..24, the bin in which the cumulative
    count reaches k (knn_find_bin: excl < want <= incl), then bits 23..16 inside that bin for the k - before remaining"""
    keys = key32(v)

    def find_bin(hist, want):
        incl = np.cumsum(hist)
        b = int(np.nonzero((incl - hist < want) & (want <= incl))[0][0])
        return b, int(incl[b] - hist[b])

    b1, before1 = find_bin(np.bincount(keys >> 24, minlength=256), k)
    inside = keys[(keys >> 24) == b1]
    b2, _ = find_bin(np.bincount((inside >> 16) & 255, minlength=256), k - before1)
    return np.uint32((b1 << 24) | (b2 << 16) | 0xffff)


def kernel_tau(v, k):
    """tau as knn_wave_body chooses it (rounds = min(k, n) <= 40: the lane minima), as a key"""
    rounds = min(k, len(v))
    return np.uint32(lane_minima_bound(key32(v), rounds)) if rounds <= 40 else histogram_bound(v, rounds)


def candidates(v, k):
    """|C| of a row"""
    return int((key32(v) <= kernel_tau(v, k)).sum())


@functools.lru_cache(maxsize=None)
def _rows(name):
    """(b * m, n) distance rows of a table input, read-only"""
    xyz, q = E.INPUTS[name][3]()
    b, n, m, _ = E.INPUTS[name]
    assert xyz.shape == (b, n, 3) and q.shape == (b, m, 3) and xyz.dtype == q.dtype == np.float32
    assert not np.isnan(xyz).any() and not np.isnan(q).any()
    d = E.dist_matrix(xyz, q).reshape(b * m, n)
    d.setflags(write=False)
    return d


def test_histogram_bound_is_what_the_two_passes_find():
    rng = np.random.default_rng(2)
    for trial in range(300):
        n = int(rng.integers(1, 400))
        k = int(rng.integers(1, n + 1))
        v = (rng.random(n, dtype=np.float32) * np.float32(rng.choice([1e-42, 1e-3, 1.0, 1e30]))).astype(np.float32)
        v[rng.random(n) < 0.2] = rng.choice([0.0, np.inf, 1.0])
        assert histogram_bound(v, k) == histogram_bound_two_passes(v, k), trial
        assert histogram_bound(v, k) >= np.sort(key32(v))[k - 1]
    for name, ks in (("ladder", (41, 60)), ("denormal", (64, 128)), ("inf_block", (160, 300)), ("shell_900", (64,))):
        for row in _rows(name):
            for k in ks:
                assert histogram_bound(row, k) == histogram_bound_two_passes(row, k), (name, k)


def test_replay_with_the_kernels_tau_equals_literal_rounds_on_table_rows():
    """ties, +Inf, denormals, n < 64, both tau paths, a full candidate table"""
    picks = [("ladder", (1, 40, 41, 60)), ("tiny_1", (1,)), ("tiny_2", (2,)), ("tiny_41", (40, 41)), ("tiny_63", (40, 41, 63)),
             ("tiny_65", (2, 40, 41, 65)), ("inf_block", (32, 160, 300)), ("denormal", (16, 64)), ("shell_900", (16, 64)),
             ("dup_1024", (8, 41))]
    for name, ks in picks:
        rows = _rows(name)
        for row in (rows[0], rows[-1]):
            keys = key32(row).astype(np.int64)
            for k in ks:
                want_v, want_i = literal_rounds(row.astype(np.float64), k)
                got_k, got_i = replay_on_candidates(keys, k, int(kernel_tau(row, k)))
                assert np.array_equal(got_i, want_i), (name, k)
                assert np.array_equal(got_k, key32(want_v.astype(np.float32)).astype(np.int64)), (name, k)


def test_every_table_case_lands_on_its_side_of_the_cap():
    """A condition on the INPUTS of knn_edge_cases.py: if a case misses its side, its input is wrong."""
    assert len(set(E.IDS)) == len(E.IDS) and set(E._K) == set(E.INPUTS)
    for cid, name, k in E.CASES:
        b, n, m, _ = E.INPUTS[name]
        assert b <= 2 and (m <= 16 or n <= 4096) and n <= E.ENVELOPE and 1 <= k <= n, cid
        assert b * m * n * min(k, n) <= 3e7, cid                  # comparisons of the serial oracle
        counts = [candidates(row, k) for row in _rows(name)]
        assert min(counts) >= k, cid                              # tau >= v_k
        if name in E.EXACTLY:
            assert set(counts) == {E.EXACTLY[name]}, (cid, counts)
        if E.above_cap(name, k):
            assert min(counts) > E.CAP, (cid, counts)
        else:
            assert max(counts) <= E.CAP, (cid, counts)
    # what single inputs are there for
    assert all((key32(r[l::64]).min() == 0x80000000) for name in E.EXACTLY for r in _rows(name) for l in range(64))
    shell = _rows("shell_900")[0]
    assert len(set(key32(shell) >> 16)) == 2 and set(key32(shell) >> 24) == {0xbf}           # straddles one second-level edge
    ladder = _rows("ladder")
    assert all(len(set(key32(r) >> 24)) == 60 for r in ladder) and (np.sort(ladder[0]) == np.ldexp(1.0, -2 * np.arange(59, -1, -1))).all()
    inf = _rows("inf_block")
    assert all(int(np.isinf(r).sum()) == 150 for r in inf)
    den = _rows("denormal")
    assert all(r.view(np.uint32).max() < 0x00100000 for r in den)        # denormal fp32, hence denormal fp64 keys
    assert (den[0] == 0).sum() >= 40 and set(key32(den[0]) >> 24) == {0x80} and (den[0] > 0).sum() > 400
    assert [8 * E.INPUTS[i][1] + 13312 for i in ("lds_mid", "lds_max")] == [78848, 128000]


def test_ragged_slices_land_on_their_side_of_the_cap():
    """rag_dup: the full cloud replays a full table, the 1025-point cloud takes the literal rounds (query 0 of each)"""
    n, lengths, m, build = E.RAGGED["rag_dup"]
    xyz, q = build()
    assert xyz.shape == (3, n, 3) and q.shape == (3, m, 3) and not np.isnan(xyz).any()
    for k in E.RAGGED_K:
        d0 = E.dist_matrix(xyz[0:1, :2048], q[0:1])[0, 0]
        d1 = E.dist_matrix(xyz[1:2, :1025], q[1:2])[0, 0]
        assert candidates(d0, k) == 1024 and candidates(d1, k) == 1025, k
    n, lengths, m, build = E.RAGGED["rag_max"]
    assert (n, lengths) == (E.ENVELOPE, [E.ENVELOPE, 63]) and build()[0].shape == (2, n, 3)
