"""The ragged multi-radius ball query (query_ball_group_xyz_msg(..., lengths1=), pn2_query_ball_group_xyz_msg_ragged) at the
cases of ragged_msg_cases.py (GPU).

THE SLICE RULE: for cloud c and every radius, idx, pts_cnt and grouped_xyz are what the dense operator returns for
xyz1[c, :lengths1[c]] alone. So for every case, scale and cloud: idx and pts_cnt equal the CPU oracle on the slice, grouped_xyz
equals oracle.group_point(slice, idx) [- centroid] bit for bit, all three equal the single-radius ragged operator called per
radius, and the results under the two paddings of the rows at or beyond a length (NaN; copies of the queries) are the same
bits. The kernel is never its own expectation; the oracle's answer for an (input, lengths, radius, nsample) is computed once."""
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


def _want(oracle, key, lengths, radius, ns):
    """(idx, cnt, group_point(slice, idx)) of the oracle on every cloud's slice, stacked; read-only"""
    k = (key, tuple(lengths), radius, ns)
    if k not in _wanted:
        xyz, q = _input(key)
        idx, cnt, grp = [], [], []
        for c, nc in enumerate(lengths):
            sl = np.ascontiguousarray(xyz[c:c + 1, :nc])
            i, k_ = oracle.query_ball_point(radius, ns, sl, np.ascontiguousarray(q[c:c + 1]))
            idx.append(i[0]); cnt.append(k_[0]); grp.append(oracle.group_point(sl, i)[0])
        out = (np.stack(idx), np.stack(cnt), np.stack(grp))
        for a in out:
            a.setflags(write=False)
        _wanted[k] = out
    return _wanted[k]


def _dev(a, cuda):
    return torch.tensor(a, device=cuda)                          # a copy: the shared inputs are read-only


def _host(t):
    return t.detach().cpu().numpy()


def _lens(lengths, cuda):
    return torch.tensor(lengths, dtype=torch.int32, device=cuda)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_outs(a, b):
    """two results of the operator, every scale: idx (or None both), pts_cnt, grouped_xyz bit for bit"""
    return len(a) == len(b) and all(
        ((i1 is None and i2 is None) or torch.equal(i1, i2)) and torch.equal(c1, c2) and _same_bits(g1, g2)
        for (i1, c1, g1), (i2, c2, g2) in zip(a, b))


def _run(P, cuda, key, scales, lengths, padding="nan", subtract=True, want_idx=True, given=None):
    """given: the lengths handed to the operator where they differ from the ones the padding is written for"""
    xyz, q = _input(key)
    x, qd = _dev(R.padded(xyz, q, lengths, padding), cuda), _dev(q, cuda)
    lens = _lens(lengths if given is None else given, cuda)
    outs = P.query_ball_group_xyz_msg([s[0] for s in scales], [s[1] for s in scales], x, qd, subtract, want_idx=want_idx,
                                      lengths1=lens)
    assert len(outs) == len(scales)
    return x, qd, lens, outs


def _check_against_oracle(oracle, key, scales, lengths, outs, subtract, want_idx, tag):
    _, q = _input(key)
    for (radius, ns), (idx, cnt, grouped) in zip(scales, outs):
        widx, wcnt, wgrp = _want(oracle, key, lengths, radius, ns)
        assert np.array_equal(_host(cnt), wcnt), (tag, radius)
        if want_idx:
            got = _host(idx)
            assert (got >= 0).all() and (got < np.asarray(lengths)[:, None, None]).all(), (tag, radius)
            assert np.array_equal(got, widx), (tag, radius)
        else:
            assert idx is None, (tag, radius)
        want = wgrp - q[:, :, None, :] if subtract else wgrp
        assert np.array_equal(_host(grouped), want), (tag, radius)


@pytest.mark.parametrize("name,key,scales,lengths,opts", R.CASES, ids=R.IDS)
def test_ragged_msg_is_the_oracle_per_slice_and_the_single_radius_operator(cuda, oracle, name, key, scales, lengths, opts):
    import pointnet2_amd as P
    subtract, want_idx = opts.get("subtract", True), opts.get("want_idx", True)
    results = {}
    for padding in R.PADDINGS:
        x, qd, lens, outs = _run(P, cuda, key, scales, lengths, padding, subtract, want_idx)
        _check_against_oracle(oracle, key, scales, lengths, outs, subtract, want_idx, (name, padding))
        per_radius = [P.query_ball_group_xyz(r, k, x, qd, subtract, want_idx=want_idx, lengths1=lens) for r, k in scales]
        assert _same_outs(outs, per_radius), (name, padding)
        results[padding] = outs
    assert _same_outs(results["nan"], results["adversarial"]), name


@pytest.mark.parametrize("key,scales", R.FULL_LENGTH_CASES, ids=[c[0] for c in R.FULL_LENGTH_CASES])
def test_full_lengths_are_the_dense_launch(cuda, key, scales):
    """(the dense launch itself is checked against the oracle in test_ball_msg_gpu.py)"""
    import pointnet2_amd as P
    b, n, m, _ = M.INPUTS[key]
    x, qd, _, outs = _run(P, cuda, key, scales, [n] * b)
    dense = P.query_ball_group_xyz_msg([s[0] for s in scales], [s[1] for s in scales], x, qd, True)
    assert _same_outs(outs, dense)


def test_bad_lengths_are_clamped_on_the_device(cuda, oracle):
    """0, -3 and n + 7 compute on 1, 1 and n (the operators never look at the values: check_lengths does, where a batch is
    built); the padding is written for the clamped lengths, NaN beyond them."""
    import pointnet2_amd as P
    key, scales, given, clamped = R.BAD_LENGTHS
    _, _, _, outs = _run(P, cuda, key, scales, clamped, given=given)
    _check_against_oracle(oracle, key, scales, clamped, outs, True, True, "clamped")
    _, _, _, ref = _run(P, cuda, key, scales, clamped)
    assert _same_outs(outs, ref)


@pytest.mark.parametrize("key,scales,lengths", R.NULL_CNT_CASES, ids=[c[0] for c in R.NULL_CNT_CASES])
@pytest.mark.parametrize("cnt_form", ["no_array", "null_entries"])
def test_null_pts_cnt_at_the_c_abi(cuda, oracle, key, scales, lengths, cnt_form):
    """pts_cnt may be missing as a whole or per scale. The outputs are filled with values no result can hold first: every entry
    must be overwritten -- also the rows of short clouds -- and must equal the oracle's."""
    import pointnet2_amd as P
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import on_device, stream_ptr
    xyz, q = _input(key)
    x, qd, lens = _dev(R.padded(xyz, q, lengths, "nan"), cuda), _dev(q, cuda), _lens(lengths, cuda)
    b, n, m, _ = M.INPUTS[key]
    k = len(scales)
    idx = [torch.full((b, m, ns), -77, dtype=torch.int32, device=cuda) for _, ns in scales]
    grp = [torch.full((b, m, ns, 3), 1e30, dtype=torch.float32, device=cuda) for _, ns in scales]
    radii = (ctypes.c_float * k)(*[s[0] for s in scales])
    nss = (ctypes.c_int * k)(*[s[1] for s in scales])
    pi = (ctypes.c_void_p * k)(*[t.data_ptr() for t in idx])
    pg = (ctypes.c_void_p * k)(*[t.data_ptr() for t in grp])
    pc = None if cnt_form == "no_array" else (ctypes.c_void_p * k)(*([None] * k))
    with on_device(cuda):
        rc = _C.lib().pn2_query_ball_group_xyz_msg_ragged(b, n, m, k, radii, nss, x.data_ptr(), lens.data_ptr(), qd.data_ptr(), 1, pi,
                                                          pc, pg, stream_ptr(cuda))
    assert rc == 0
    torch.cuda.synchronize()
    for (radius, ns), i, g in zip(scales, idx, grp):
        assert not bool((i == -77).any()) and not bool((g == 1e30).any()), (key, radius)
        widx, _, wgrp = _want(oracle, key, lengths, radius, ns)
        assert np.array_equal(_host(i), widx) and np.array_equal(_host(g), wgrp - q[:, :, None, :]), (key, radius)


def test_capture_and_replay_with_new_lengths(cuda, oracle):
    """One call captured on a single stream; lengths1 is overwritten in place; the replay gives the eager call's bits at the new
    lengths (the host never read the lengths, nothing in the launch depends on them). The padding rows hold NaN beyond the
    LARGER of the two lengths of a cloud and the cloud's own points below, so both lengths see their slice."""
    import pointnet2_amd as P
    key, scales, first, second = R.CAPTURE
    xyz, q = _input(key)
    x, qd = _dev(R.padded(xyz, q, [max(a, b) for a, b in zip(first, second)], "nan"), cuda), _dev(q, cuda)
    lens = _lens(first, cuda)
    radii, nss = [s[0] for s in scales], [s[1] for s in scales]

    def step():
        return P.query_ball_group_xyz_msg(radii, nss, x, qd, True, lengths1=lens)
    side = torch.cuda.Stream()                                               # warm on a side stream, as a capture wants it
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        old = [tuple(t.clone() for t in out) for out in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    lens.copy_(_lens(second, cuda))
    graph.replay()
    torch.cuda.synchronize()
    got = [tuple(t.clone() for t in out) for out in captured]
    want = step()
    assert not _same_outs(got, old)                                          # the replay did see the new lengths
    assert _same_outs(got, want)
    _check_against_oracle(oracle, key, scales, second, got, True, True, "replay")
