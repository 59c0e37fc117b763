"""The multi-radius ball query (pn2_query_ball_group_xyz_msg) at the cases of ball_msg_cases.py (GPU): every launch geometry,
clouds whose binning gives up inside a binned launch, non-finite / far-away inputs, extreme radii, every order and number of
radii, the output forms, both sides of the use_cells threshold and query counts below the workgroup's granule. What each case
launches is pinned host-side by test_ball_msg_plan.py.

For every case and every scale: idx and pts_cnt equal the CPU oracle (the restatement pinned to the reference), grouped_xyz
equals oracle.group_point(xyz, idx) [- centroid] bit for bit, and all three equal the single-radius operators called per radius.
The kernel is never its own expectation. The oracle's answer for an (input, radius, nsample) is computed once and shared."""
import ctypes

import numpy as np
import pytest
import torch

import ball_msg_cases as M

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


def _want(oracle, key, radius, ns):
    """(idx, cnt, group_point(xyz, idx)) of the oracle, read-only"""
    k = (key, radius, ns)
    if k not in _wanted:
        xyz, q = _input(key)
        with np.errstate(invalid="ignore", over="ignore"):
            idx, cnt = oracle.query_ball_point(radius, ns, xyz, q)
            grouped = oracle.group_point(xyz, idx)
        for a in (idx, cnt, grouped):
            a.setflags(write=False)
        _wanted[k] = (idx, cnt, grouped)
    return _wanted[k]


def _dev(a, cuda):
    return torch.tensor(a, device=cuda)                          # a copy: the shared inputs are read-only


def _host(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_scale(P, oracle, key, x, qd, radius, ns, out, subtract, want_idx, tag):
    xyz, q = _input(key)
    idx, cnt, grouped = out
    widx, wcnt, wgrp = _want(oracle, key, radius, ns)
    assert np.array_equal(_host(cnt), wcnt), tag
    if want_idx:
        assert np.array_equal(_host(idx), widx), tag
    else:
        assert idx is None, tag
    with np.errstate(invalid="ignore", over="ignore"):
        want = wgrp - q[:, :, None, :] if subtract else wgrp
    assert np.array_equal(_host(grouped), want, equal_nan=True), tag
    # ... and the single-radius operators, called per radius
    i1, c1 = P.query_ball_point(radius, ns, x, qd)
    i2, c2, g2 = P.query_ball_group_xyz(radius, ns, x, qd, subtract)
    assert torch.equal(c1, cnt) and torch.equal(c2, cnt), tag
    if want_idx:
        assert torch.equal(i1, idx) and torch.equal(i2, idx), tag
    assert _same_bits(g2, grouped), tag


def _run(P, cuda, key, scales, subtract=True, want_idx=True):
    xyz, q = _input(key)
    x, qd = _dev(xyz, cuda), _dev(q, cuda)
    outs = P.query_ball_group_xyz_msg([s[0] for s in scales], [s[1] for s in scales], x, qd, subtract, want_idx=want_idx)
    assert len(outs) == len(scales)
    return x, qd, outs


@pytest.mark.parametrize("name,key,scales,opts", M.CASES, ids=M.IDS)
def test_msg_matches_oracle_and_single_radius_operators(cuda, oracle, name, key, scales, opts):
    import pointnet2_amd as P
    subtract, want_idx = opts.get("subtract", True), opts.get("want_idx", True)
    x, qd, outs = _run(P, cuda, key, scales, subtract, want_idx)
    for (radius, ns), out in zip(scales, outs):
        _check_scale(P, oracle, key, x, qd, radius, ns, out, subtract, want_idx, (name, radius, ns))


def test_msg_order_of_radii_does_not_matter(cuda):
    """Every order of one radius list: each scale's outputs are those of the ascending call, bit for bit (the cells are sized
    for the second smallest radius wherever it stands in the list)."""
    import pointnet2_amd as P
    asc_case = M.CASES[M.IDS.index(M.ASCENDING)]
    _, _, asc_outs = _run(P, cuda, asc_case[1], asc_case[2])
    asc = dict(zip(asc_case[2], asc_outs))
    for name, key, scales, _ in M.PERMUTATIONS:
        _, _, outs = _run(P, cuda, key, scales)
        for scale, (idx, cnt, grouped) in zip(scales, outs):
            a_idx, a_cnt, a_grp = asc[scale]
            assert torch.equal(idx, a_idx) and torch.equal(cnt, a_cnt) and _same_bits(grouped, a_grp), (name, scale)


@pytest.mark.parametrize("key", M.NULL_CNT_INPUTS)
@pytest.mark.parametrize("cnt_form", ["no_array", "null_entries"])
def test_msg_null_pts_cnt_at_the_c_abi(cuda, key, cnt_form):
    """pts_cnt may be missing as a whole or per scale. The outputs are filled with values no result can hold first: every entry
    must be overwritten and must equal the full call's (itself checked against the oracle above)."""
    import pointnet2_amd as P
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import on_device, stream_ptr
    scales = M.THREE
    x, qd, full = _run(P, cuda, key, scales)
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
        rc = _C.lib().pn2_query_ball_group_xyz_msg(b, n, m, k, radii, nss, x.data_ptr(), qd.data_ptr(), 1, pi, pc, pg,
                                                   stream_ptr(cuda))
    assert rc == 0
    torch.cuda.synchronize()
    for scale, (f_idx, _, f_grp), i, g in zip(scales, full, idx, grp):
        assert not bool((i == -77).any()) and not bool((g == 1e30).any()), (key, scale)
        assert torch.equal(i, f_idx) and _same_bits(g, f_grp), (key, scale)
