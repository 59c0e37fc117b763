"""The packed multi-radius ball query (query_ball_group_xyz_msg(..., offsets=, max_points=), pn2_query_ball_group_xyz_msg_packed)
on packed batches built from the inputs and lengths of ragged_msg_cases.py (GPU).

THE SLICE RULE, PACKED: for cloud c and every radius, idx - offsets[c] (global_idx; idx itself without), pts_cnt and grouped_xyz
are what the dense operator returns for flat[offsets[c] : offsets[c + 1]] alone. So for every case, scale and cloud the results
equal the CPU oracle on the slice (computed once per (input, cloud, count, radius, nsample)), the single-radius packed operator
called per radius, and the ragged multi-radius operator on the NaN-padded copy of the same clouds. Every cloud of an input lies
in the same cube, so a read across a slab boundary would change a result. Each set of counts runs in the given order and in an
ORDER whose slab starts are all no multiple of 4 (a slab may start at any row): a rotation of the clouds where one exists, else
the given order with the first cloud one point shorter. The kernel is never its own expectation."""
import ctypes

import numpy as np
import pytest
import torch

import ball_msg_cases as M
import ragged_msg_cases as R

pytestmark = pytest.mark.gpu

_inputs, _wanted = {}, {}


def _input(key):
    if key not in _inputs:
        xyz, q = M.INPUTS[key][3]()
        b, n, m, _ = M.INPUTS[key]
        assert xyz.shape == (b, n, 3) and q.shape == (b, m, 3) and xyz.dtype == q.dtype == np.float32
        xyz.setflags(write=False)
        q.setflags(write=False)
        _inputs[key] = (xyz, q)
    return _inputs[key]


def _oracle_slice(oracle, sl, q, radius, ns):
    """(idx, cnt, group_point(slice, idx)) of the oracle for one cloud: sl (nc, 3), q (m, 3)"""
    sl = np.ascontiguousarray(sl[None])
    i, k = oracle.query_ball_point(radius, ns, sl, np.ascontiguousarray(q[None]))
    return i[0], k[0], oracle.group_point(sl, i)[0]


def _want(oracle, key, cloud, nc, radius, ns):
    """the oracle on the first nc points of cloud `cloud` of an input, against that cloud's queries; computed once, read-only"""
    k = (key, cloud, nc, radius, ns)
    if k not in _wanted:
        xyz, q = _input(key)
        out = _oracle_slice(oracle, xyz[cloud, :nc], q[cloud], radius, ns)
        for a in out:
            a.setflags(write=False)
        _wanted[k] = out
    return _wanted[k]


def _orders(lengths):
    """[(clouds, counts)]: the given order, and the order with every slab start (but the first, 0) no multiple of 4"""
    b = len(lengths)
    given = (list(range(b)), list(lengths))
    for k in range(1, b):
        clouds = [(p + k) % b for p in range(b)]
        counts = [lengths[c] for c in clouds]
        if all(s % 4 for s in np.cumsum(counts)[:-1]):
            return [given, (clouds, counts)]
    counts = [lengths[0] - 1] + list(lengths[1:])
    return [given, (list(range(b)), counts)]


def _odd_starts(counts):
    return all(s % 4 for s in np.cumsum(counts)[:-1])


def test_the_orders_have_the_starts_they_promise():
    clouds, counts = _orders(R.MIXED)[1]
    assert clouds == [3, 0, 1, 2] and counts == [63, 3000, 1500, 64]           # rotated by 3
    assert np.cumsum([0] + counts)[1:-1].tolist() == [63, 3063, 4563]
    giveup = dict((c[0], c[3]) for c in R.CASES)["giveup_mixed"]
    assert all(k % 4 == 0 for k in giveup)                                    # no rotation helps: the first cloud loses a point
    clouds, counts = _orders(giveup)[1]
    assert clouds == [0, 1, 2, 3] and counts == [giveup[0] - 1] + giveup[1:]
    for case in R.CASES:
        (c0, k0), (c1, k1) = _orders(case[3])
        assert k0 == list(case[3]) and sorted(c1) == c0 and _odd_starts(k1) and len(k1) > 1, case[0]


def _dev(a, cuda):
    return torch.tensor(a, device=cuda)                          # a copy: the shared inputs are read-only


def _host(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_outs(a, b, shift=None):
    """two results of the operator, every scale: idx (or None both; a's minus shift), pts_cnt, grouped_xyz bit for bit"""
    def same_idx(i1, i2):
        if i1 is None or i2 is None:
            return i1 is None and i2 is None
        return torch.equal(i1 if shift is None else i1 - shift, i2)
    return len(a) == len(b) and all(same_idx(i1, i2) and torch.equal(c1, c2) and _same_bits(g1, g2)
                                    for (i1, c1, g1), (i2, c2, g2) in zip(a, b))


def _batch(key, clouds, counts, cuda):
    """the packed batch of xyz[clouds[p], :counts[p]], its queries, its offsets and its NaN-padded copy"""
    xyz, q = _input(key)
    n = xyz.shape[1]
    flat = np.concatenate([xyz[c, :k] for c, k in zip(clouds, counts)])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    padded = np.full((len(clouds), n, 3), np.nan, dtype=np.float32)
    for p, (c, k) in enumerate(zip(clouds, counts)):
        padded[p, :k] = xyz[c, :k]
    qs = np.ascontiguousarray(q[clouds])
    return _dev(flat, cuda), _dev(qs, cuda), _dev(offsets, cuda), _dev(padded, cuda), qs, offsets


def _check_against_oracle(oracle, key, scales, clouds, counts, offsets, flat, qs, outs, subtract, want_idx, global_idx, tag):
    for (radius, ns), (idx, cnt, grouped) in zip(scales, outs):
        want = [_want(oracle, key, c, k, radius, ns) for c, k in zip(clouds, counts)]
        widx, wcnt, wgrp = (np.stack([w[j] for w in want]) for j in range(3))
        assert np.array_equal(_host(cnt), wcnt), (tag, radius)
        centred = wgrp - qs[:, :, None, :] if subtract else wgrp
        got_g = _host(grouped)
        assert np.array_equal(got_g, centred), (tag, radius)
        if not want_idx:
            assert idx is None, (tag, radius)
            continue
        got = _host(idx)
        lo = offsets[:-1, None, None] if global_idx else 0
        assert (got >= lo).all() and (got < lo + np.asarray(counts)[:, None, None]).all(), (tag, radius)   # inside its own slab
        assert np.array_equal(got - lo, widx), (tag, radius)
        if global_idx:                                              # the indices are rows of the flat array
            rows = _host(flat)[got]
            assert np.array_equal(rows - qs[:, :, None, :] if subtract else rows, got_g), (tag, radius)


def _run_case(P, cuda, oracle, name, key, scales, lengths, opts, max_points=None):
    subtract, want_idx = opts.get("subtract", True), opts.get("want_idx", True)
    radii, nss = [s[0] for s in scales], [s[1] for s in scales]
    nmax = M.INPUTS[key][1] if max_points is None else max_points   # the padded n of the ragged test: a bound on every count
    results = []
    for clouds, counts in _orders(lengths):
        flat, qd, offs, padded, qs, offsets = _batch(key, clouds, counts, cuda)
        lens = torch.tensor(counts, dtype=torch.int32, device=cuda)
        ragged = P.query_ball_group_xyz_msg(radii, nss, padded, qd, subtract, want_idx=want_idx, lengths1=lens)
        for global_idx in (False, True):
            tag = (name, tuple(counts), global_idx)
            outs = P.query_ball_group_xyz_msg(radii, nss, flat, qd, subtract, want_idx=want_idx, offsets=offs, max_points=nmax,
                                              global_idx=global_idx)
            assert len(outs) == len(scales)
            for (r, k), (idx, cnt, grouped) in zip(scales, outs):
                b, m = qd.shape[0], qd.shape[1]
                assert (idx is None or tuple(idx.shape) == (b, m, k)) and tuple(cnt.shape) == (b, m) and tuple(grouped.shape) == (b, m, k, 3)
            _check_against_oracle(oracle, key, scales, clouds, counts, offsets, flat, qs, outs, subtract, want_idx, global_idx, tag)
            per_radius = [P.query_ball_group_xyz(r, k, flat, qd, subtract, want_idx=want_idx, offsets=offs, max_points=nmax,
                                                 global_idx=global_idx) for r, k in scales]
            assert _same_outs(outs, per_radius), tag
            assert _same_outs(outs, ragged, offs[:-1].view(-1, 1, 1) if global_idx else None), tag
            results.append(outs)
    return results


@pytest.mark.parametrize("name,key,scales,lengths,opts", R.CASES, ids=R.IDS)
def test_packed_msg_is_the_oracle_per_slice_and_both_sibling_operators(cuda, oracle, name, key, scales, lengths, opts):
    import pointnet2_amd as P
    from pointnet2_amd.tf_grouping import query_ball_group_xyz_msg_plan
    plan = query_ball_group_xyz_msg_plan([s[0] for s in scales], [s[1] for s in scales], len(lengths), M.INPUTS[key][1], M.INPUTS[key][2])
    assert (plan["rc"] == -4) == (name == "fallback_127"), plan     # the per-radius packed fallback is taken there, and only there
    _run_case(P, cuda, oracle, name, key, scales, lengths, opts)


def test_the_cases_the_branches_need_are_present():
    assert {"binned_mixed", "tiny_clouds", "third_geometry", "giveup_mixed", "swept", "m_7", "odd_n_5000", "no_idx_binned", "no_idx_swept",
            "no_subtract_binned", "no_subtract_swept", "radii_one", "radii_four", "radii_permuted", "fallback_127"} <= set(R.IDS)


def test_max_points_is_a_bound(cuda, oracle):
    """binned_mixed once more under max_points = 3001: the host plans for another extent, the results are the same bits"""
    import pointnet2_amd as P
    name, key, scales, lengths, opts = R.CASES[R.IDS.index("binned_mixed")]
    assert max(lengths) == 3000
    exact = _run_case(P, cuda, oracle, name, key, scales, lengths, opts)
    loose = _run_case(P, cuda, oracle, name, key, scales, lengths, opts, max_points=3001)
    assert len(exact) == len(loose) == 4 and all(_same_outs(a, b) for a, b in zip(exact, loose))


@pytest.mark.parametrize("key,scales,lengths", R.NULL_CNT_CASES, ids=[c[0] for c in R.NULL_CNT_CASES])
@pytest.mark.parametrize("cnt_form", ["no_array", "null_entries"])
def test_null_pts_cnt_at_the_c_abi(cuda, oracle, key, scales, lengths, cnt_form):
    """pts_cnt may be missing as a whole or per scale. The outputs are filled with values no result can hold first: every entry
    must be overwritten -- also the rows of short clouds -- and must equal the oracle's."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import on_device, stream_ptr
    clouds, counts = _orders(lengths)[1]
    flat, qd, offs, _, qs, offsets = _batch(key, clouds, counts, cuda)
    b, m, k = len(counts), qd.shape[1], len(scales)
    idx = [torch.full((b, m, ns), -77, dtype=torch.int32, device=cuda) for _, ns in scales]
    grp = [torch.full((b, m, ns, 3), 1e30, dtype=torch.float32, device=cuda) for _, ns in scales]
    radii = (ctypes.c_float * k)(*[s[0] for s in scales])
    nss = (ctypes.c_int * k)(*[s[1] for s in scales])
    pi = (ctypes.c_void_p * k)(*[t.data_ptr() for t in idx])
    pg = (ctypes.c_void_p * k)(*[t.data_ptr() for t in grp])
    pc = None if cnt_form == "no_array" else (ctypes.c_void_p * k)(*([None] * k))
    with on_device(cuda):
        rc = _C.lib().pn2_query_ball_group_xyz_msg_packed(b, int(flat.shape[0]), M.INPUTS[key][1], m, k, radii, nss, flat.data_ptr(),
                                                          offs.data_ptr(), qd.data_ptr(), 1, 1, pi, pc, pg, stream_ptr(cuda))
    assert rc == 0
    torch.cuda.synchronize()
    for (radius, ns), i, g in zip(scales, idx, grp):
        assert not bool((i == -77).any()) and not bool((g == 1e30).any()), (key, radius)
        want = [_want(oracle, key, c, kc, radius, ns) for c, kc in zip(clouds, counts)]
        widx, wgrp = np.stack([w[0] for w in want]), np.stack([w[2] for w in want])
        assert np.array_equal(_host(i) - offsets[:-1, None, None], widx), (key, radius)
        assert np.array_equal(_host(g), wgrp - qs[:, :, None, :]), (key, radius)


def test_capture_and_replay_with_new_offsets(cuda, oracle):
    """One call captured on a single stream at counts (3000, 1500, 64, 63); offsets is overwritten in place to counts (63, 64,
    1500, 3000) of the SAME flat array -- total and max_points are host values and stay --; the replay gives the oracle's
    results for the new slices (the host never read the offsets, nothing in the launch depends on them)."""
    import pointnet2_amd as P
    key, scales = "edge_base", M.THREE
    first, second = list(R.MIXED), list(reversed(R.MIXED))
    assert first == [3000, 1500, 64, 63] and second == [63, 64, 1500, 3000]
    flat, qd, offs, _, qs, _ = _batch(key, [0, 1, 2, 3], first, cuda)
    new_offsets = np.concatenate([[0], np.cumsum(second)]).astype(np.int32)
    radii, nss = [s[0] for s in scales], [s[1] for s in scales]

    def step():
        return P.query_ball_group_xyz_msg(radii, nss, flat, qd, True, offsets=offs, max_points=3000, global_idx=True)
    side = torch.cuda.Stream()                                               # warm on a side stream, as a capture wants it
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        old = [tuple(t.clone() for t in out) for out in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    offs.copy_(_dev(new_offsets, cuda))
    graph.replay()
    torch.cuda.synchronize()
    got = [tuple(t.clone() for t in out) for out in captured]
    assert not _same_outs(got, old)                                          # the replay did see the new offsets
    flat_h = _host(flat)
    for (radius, ns), (idx, cnt, grouped) in zip(scales, got):
        for c in range(4):
            lo, hi = int(new_offsets[c]), int(new_offsets[c + 1])
            widx, wcnt, wgrp = _oracle_slice(oracle, flat_h[lo:hi], qs[c], radius, ns)
            assert np.array_equal(_host(idx[c]) - lo, widx) and np.array_equal(_host(cnt[c]), wcnt), (radius, c)
            assert np.array_equal(_host(grouped[c]), wgrp - qs[c][:, None, :]), (radius, c)
