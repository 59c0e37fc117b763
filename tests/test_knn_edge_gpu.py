"""kNN and the selection sort (csrc/topk.hip) at the cases of knn_edge_cases.py (GPU): both tau paths from either side of the
switch at 40 rounds, the replay on a full candidate table and the literal rounds one candidate later, the literal rounds from
distinct values and for more than 1024 rounds, fewer points than lanes, histogram bin edges, +Inf and denormal distances, dynamic
LDS up to the envelope's edge, the ragged twin at lengths 1, 63 and 14336, the matrix path of knn_point, the wave kernel's long
rows and rows holding NaN in both selection-sort kernels. Where each case goes is pinned host-side by test_knn_replay_model.py.

Every comparison is exact: indices with array_equal, values as uint32 bit patterns (+Inf, -0 and NaN payloads count). The
expectation is the project's definition of knn_point -- the fp32 matrix ((dx dx + dy dy) + dz dz) in numpy, the oracle's
selection sort, the first k columns -- computed once per (input, k). The kernel is never its own expectation."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import knn_edge_cases as E
from test_ragged_gpu import PADDINGS, padded

pytestmark = pytest.mark.gpu


def dev(a, cuda):
    return torch.tensor(a, device=cuda)                          # a copy: the shared inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _input(name):
    xyz, q = E.INPUTS[name][3]()
    d = E.dist_matrix(xyz, q)
    for a in (xyz, q, d):
        a.setflags(write=False)
    return xyz, q, d


@functools.lru_cache(maxsize=None)
def _want(name, k):
    import oracle as O
    wi, wo = O.select_top_k(k, _input(name)[2])
    wi, wo = wi[:, :, :k].copy(), wo[:, :, :k].copy()
    wi.setflags(write=False)
    wo.setflags(write=False)
    return wi, wo


@pytest.mark.parametrize("cid,name,k", E.CASES, ids=E.IDS)
def test_knn_dense_table(cuda, oracle, cid, name, k):
    import pointnet2_amd as P
    xyz, q, _ = _input(name)
    b, n, m, _ = E.INPUTS[name]
    wi, wo = _want(name, k)
    val, idx = P.knn_point(k, dev(xyz, cuda), dev(q, cuda))
    assert val.shape == idx.shape == (b, m, k)
    assert np.array_equal(host(idx), wi), cid
    assert np.array_equal(bits(host(val)), bits(wo)), cid


@functools.lru_cache(maxsize=None)
def _ragged_case(name, k):
    """per slice the dense definition (tests/test_ragged_gpu.py::knn_case); k > n_i: the entries from n_i on repeat entry 0"""
    import oracle as O
    n, lengths, m, build = E.RAGGED[name]
    xyz, q = build()
    wi = np.empty((len(lengths), m, k), dtype=np.int32)
    wv = np.empty((len(lengths), m, k), dtype=np.float32)
    for i, ni in enumerate(lengths):
        kk = min(k, ni)
        oi, ov = O.select_top_k(kk, E.dist_matrix(xyz[i:i + 1, :ni], q[i:i + 1]))
        wi[i, :, :kk], wv[i, :, :kk] = oi[0, :, :kk], ov[0, :, :kk]
        wi[i, :, kk:], wv[i, :, kk:] = oi[0, :, :1], ov[0, :, :1]
    return xyz, q, wi, wv


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("k", E.RAGGED_K)
@pytest.mark.parametrize("name", sorted(E.RAGGED))
def test_knn_ragged_twin(cuda, oracle, name, k, padding):
    import pointnet2_amd as P
    n, lengths, m, _ = E.RAGGED[name]
    xyz, q, wi, wv = _ragged_case(name, k)
    x = dev(padded(xyz, lengths, padding), cuda)
    val, idx = P.knn_point(k, x, dev(q, cuda), lengths1=torch.tensor(lengths, dtype=torch.int32, device=cuda))
    assert (host(idx) < np.asarray(lengths)[:, None, None]).all() and (host(idx) >= 0).all()
    assert np.array_equal(host(idx), wi), (name, k, padding)
    assert np.array_equal(bits(host(val)), bits(wv)), (name, k, padding)
    for i, ni in enumerate(lengths):
        if k > ni:
            assert (host(idx)[i, :, ni:] == host(idx)[i, :, :1]).all() and (bits(host(val))[i, :, ni:] == bits(host(val))[i, :, :1]).all()


@pytest.mark.parametrize("name", sorted(E.MATRIX))
def test_knn_matrix_path(cuda, oracle, name):
    """c != 3, or n past the envelope: torch elementwise ops (differences, squares, a left-to-right sum over c) + select_top_k"""
    import pointnet2_amd as P
    c, n, m, k = E.MATRIX[name]
    xyz, q = E.matrix_input(name)
    assert xyz.shape[1:] == (n, c) and q.shape[1:] == (m, c)
    wi, wo = oracle.select_top_k(k, E.dist_matrix(xyz, q))
    val, idx = P.knn_point(k, dev(xyz, cuda), dev(q, cuda))
    assert val.shape == idx.shape == (xyz.shape[0], m, k)
    assert np.array_equal(host(idx), wi[:, :, :k]), name
    assert np.array_equal(bits(host(val)), bits(wo[:, :, :k])), name
    if c == 3:                                                   # ... exactly as the one-kernel path does one point earlier
        xyz, q = xyz[:, :E.ENVELOPE].copy(), q
        wi, wo = oracle.select_top_k(k, E.dist_matrix(xyz, q))
        val, idx = P.knn_point(k, dev(xyz, cuda), dev(q, cuda))
        assert np.array_equal(host(idx), wi[:, :, :k]) and np.array_equal(bits(host(val)), bits(wo[:, :, :k]))


def test_knn_envelope_at_the_c_abi(cuda):
    """one point past the envelope is refused at the C ABI, dense and ragged (k > n: tests/test_abi.py)"""
    from pointnet2_amd import _C
    lib = _C.lib()
    one = ctypes.c_void_p(16)                                    # any non-null pointer: never dereferenced
    assert lib.pn2_knn_point(1, E.ENVELOPE + 1, 4, 2, one, one, one, one, None) == -4
    assert lib.pn2_knn_point_ragged(1, E.ENVELOPE + 1, 4, 2, one, one, one, one, one, None) == -4
    assert lib.pn2_knn_point(0, E.ENVELOPE, 4, 2, None, None, None, None, None) == 0           # inside: an empty batch is fine


@pytest.mark.parametrize("b,m,n,k", E.SORT_LONG, ids=["n%d-k%d" % (c[2], c[3]) for c in E.SORT_LONG])
def test_selection_sort_long_rows(cuda, oracle, b, m, n, k):
    """the wave kernel above 64 KiB of LDS (8 n bytes, up to 128 KiB at n = 16384) and the first row length of the serial kernel;
    the whole (b, m, n) outputs: the tail beyond k is part of the contract"""
    import pointnet2_amd as P
    dist = E.sort_long_input(b, m, n, k)
    assert not np.isnan(dist).any()
    outi, out = P.select_top_k(k, dev(dist, cuda))
    wi, wo = oracle.select_top_k(k, dist)
    assert np.array_equal(host(outi), wi), (n, k)
    assert np.array_equal(bits(host(out)), bits(wo)), (n, k)


@pytest.mark.parametrize("n", E.NAN_N, ids=["wave", "serial"])
def test_selection_sort_nan_rows(cuda, oracle, n):
    """The reference compares with `<` (tf_grouping_g.cu:83-123): a NaN in the unsorted tail is never selected, and a round whose
    slot holds a NaN swaps nothing -- for NaN of either sign, in both kernels."""
    import pointnet2_amd as P
    assert (n <= E.SORT_MAX_LDS_N) == (n == E.NAN_N[0])
    dist = E.sort_nan_input(n)
    outi, out = P.select_top_k(E.NAN_K, dev(dist, cuda))
    wi, wo = oracle.select_top_k(E.NAN_K, dist)
    assert bits(wo)[0, E.NAN_ROWS.index("slot3_neg"), 3] == E.NEG_NAN                          # the oracle itself: it stays
    gi, gv = host(outi), bits(host(out))
    wrong = [row for r, row in enumerate(E.NAN_ROWS)
             if not (np.array_equal(gi[0, r], wi[0, r]) and np.array_equal(gv[0, r], bits(wo)[0, r]))]
    assert not wrong, (n, wrong)
