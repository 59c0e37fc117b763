"""The fused inference MLP kernels (csrc/sa_mlp.hip, sa_mlp_stream.hip, coop_mlp.hip, fp_mlp.hip) on inputs whose float64
result is exactly representable and which the six-term bf16 scheme, if complete and correctly packed, must reproduce BIT FOR
BIT (tests/mlp_exact_cases.py states and asserts the conditions). No tolerance: np.array_equal against the plain float64
evaluation. A lost 2^-16-order term, a level plane of one tile pair stored at the wrong place, a wrong masked tail or a wrong
bias on a few small channels -- all inside the 5e-6 / 1e-5 bounds of the float64 tests of these kernels -- is a hard mismatch
here. Public Python entry points only; every kernel family is asserted by the kind the library reports."""
import ctypes

import numpy as np
import pytest
import torch

import mlp_exact_cases as C

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _assert_bits(got, want, q, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    g, w = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    bad = np.argwhere(g != w)
    r, c = (int(v) for v in bad[0])
    pytest.fail("%s: %d of %d values differ; first at (row %d, channel %d): got %s, want %s, got - want = %g x 2^-%d"
                % (what, len(bad), g.size, r, c, float(g[r, c]).hex(), float(w[r, c]).hex(),
                   (float(g[r, c]) - float(w[r, c])) * 2.0 ** q, q))


def _sa_family(packed, case, b, n, m, ns):
    from pointnet2_amd import _C
    fam = packed.kind
    if fam == "cooperative" and _C.lib().pn2_sa_mlp3_ws_bytes(b, n, m, packed.cin, *packed.widths, ns) > 0:
        fam = "cooperative_gemm"                      # only the GEMM last layer needs scratch among the cooperative stacks
    return fam


def _run_sa(case, cuda, want_family):
    from pointnet2_amd import sa_mlp
    b, n = case["xyz"].shape[:2]
    group_all = case["family"] == "group_all"
    m, ns = (1, n) if group_all else case["idx"].shape[1:]
    packed = sa_mlp.PackedMLP3(case["layers"], cuda, ns, xyz_first=case["xyz_first"])
    assert _sa_family(packed, case, b, n, m, ns) == want_family
    args = [_dev(case[k], cuda) for k in ("xyz", "new_xyz", "points", "idx")]
    outs = []
    try:
        for variant in ((0, 1, 2, 3) if want_family == "resident" else (0,)):      # 2, 3: two items per wave where it applies
            sa_mlp.set_resident_variant(variant)
            outs.append((variant, sa_mlp.sa_mlp_maxpool(args[0], args[1], args[2], args[3], packed).cpu().numpy()))
    finally:
        sa_mlp.set_resident_variant(0)
    return outs


@pytest.mark.parametrize("cid", C.SA_IDS)
def test_sa_stack_is_exact(cuda, cid):
    case = C.get_case(cid)
    want, q = C.expected(cid)
    for variant, got in _run_sa(case, cuda, cid.split("-")[0]):
        _assert_bits(got, want, q, "%s (resident variant %d)" % (cid, variant))


@pytest.mark.parametrize("cid", C.GROUP_ALL_IDS)
def test_group_all_stack_is_exact(cuda, cid):
    case = C.get_case(cid)
    want, q = C.expected(cid)
    (_, got), = _run_sa(case, cuda, "cooperative_gemm")
    _assert_bits(got, want, q, cid)


def _fp_kinds(c2, c1, widths):
    from pointnet2_amd import _C
    warr = (ctypes.c_int * len(widths))(*widths)
    kinds = [k for k in (0, 1) if _C.lib().pn2_fp_mlp_config(c2, c1, len(widths), warr, k, None, None, None) == 0]
    assert kinds, "no fused kernel for the stack"
    return kinds


@pytest.mark.parametrize("cid", C.FP_IDS)
def test_fp_stack_is_exact(cuda, cid):
    from pointnet2_amd import sa_mlp
    case = C.get_case(cid)
    want, q = C.expected(cid)
    assert (case["idx"].shape[0] * case["idx"].shape[1]) % 32 != 0
    p2, p1, idx, dist = (_dev(case[k], cuda) for k in ("points2", "points1", "idx", "dist"))
    for kind in _fp_kinds(case["c2"], case["c1"], case["widths"]):
        packed = sa_mlp.PackedFPMLP(case["layers"], case["c2"], case["c1"], cuda, kind)
        _assert_bits(sa_mlp.fp_mlp(p2, p1, idx, dist, packed), want, q, "%s (%s)" % (cid, ("streamed", "cooperative")[kind]))


def test_case_table_is_complete():
    """Every family / probe kind / probe layer combination is in the table (a renamed id would silently drop one)."""
    for fam, cfeat, widths, ns in C.SA_STACKS:
        for kind, layer in C.PROBES:
            assert C.sa_id(fam, cfeat, widths, ns, kind, layer) in C.CASES
    assert {f for f, *_ in C.FEATURES_FIRST} == {f for f, *_ in C.SA_STACKS}
    assert len(C.GROUP_ALL_IDS) == len(C.GROUP_ALL) * len(C.PROBES)
    assert len(C.FP_IDS) == sum(len(w) * 3 for _, _, w in C.FP_STACKS)
    known = {C.CASES[i][1]["m"] for i in C.FP_IDS}
    assert known == set(C.FP_KNOWN)


# ---- the one-C-call level entry points feed the same kernels ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["w_rich", "x_rich", "cross"])
def test_sa_level_call_is_exact(cuda, kind):
    """sa_mlp.sa_level on a tiny cloud whose every ball holds the whole cloud (nsample = n): sampling and grouping inside the
    call, then the same kernel -- equal to the operator path on the call's own new_xyz / idx, which is exact."""
    from pointnet2_amd import sa_mlp
    cfeat, widths, ns, m = 6, (64, 96, 128), 32, 5
    case = dict(C.build_sa(cfeat, widths, ns, kind, 1, seed=200, b=3, m=m, n=ns))
    packed = sa_mlp.PackedMLP3(case["layers"], cuda, ns)
    xyz, points = _dev(case["xyz"], cuda), _dev(case["points"], cuda)
    new_xyz, out, idx = sa_mlp.sa_level(m, 100.0, ns, xyz, points, packed)[:3]
    case["new_xyz"], case["idx"] = new_xyz.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(np.sort(case["idx"], axis=2), np.broadcast_to(np.arange(ns, dtype=np.int32), case["idx"].shape))
    want, q = C.check_exact(case)
    _assert_bits(out, want, q, "sa_level " + kind)
    _assert_bits(sa_mlp.sa_mlp_maxpool(xyz, new_xyz, points, idx, packed), want, q, "operator path " + kind)


@pytest.mark.parametrize("kind", ["w_rich", "x_rich", "cross"])
def test_fp_level_call_is_exact(cuda, kind):
    """sa_mlp.fp_level with geometry that makes three_nn return squared distances (1, 2, 2) for every unknown point: its three
    known points sit at +(1,0,0), +(1,1,0), +(1,0,1), the next point's 8 away."""
    import pointnet2_amd as P
    from pointnet2_amd import sa_mlp
    c2, c1, widths, b, n = 128, 6, (128, 128, 128), 3, 11
    xyz1 = np.zeros((b, n, 3), np.float32)
    xyz1[:, :, 0] = 8.0 * np.arange(n)
    xyz2 = (xyz1[:, :, None, :] + np.array([[1, 0, 0], [1, 1, 0], [1, 0, 1]], np.float32)).reshape(b, 3 * n, 3)
    case = dict(C.build_fp(c2, c1, widths, kind, 1, m=3 * n, n=n, b=b, seed=300))
    x1, x2, p1, p2 = _dev(xyz1, cuda), _dev(xyz2, cuda), _dev(case["points1"], cuda), _dev(case["points2"], cuda)
    dist, idx = P.three_nn(x1, x2)
    case["dist"], case["idx"] = dist.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(case["dist"], np.broadcast_to(np.array([1, 2, 2], np.float32), (b, n, 3)))
    want, q = C.check_exact(case)
    for k in _fp_kinds(c2, c1, widths):
        packed = sa_mlp.PackedFPMLP(case["layers"], c2, c1, cuda, k)
        _assert_bits(sa_mlp.fp_level(x1, x2, p1, p2, packed), want, q, "fp_level %s kind %d" % (kind, k))
        _assert_bits(sa_mlp.fp_mlp(p2, p1, idx, dist, packed), want, q, "operator path %s kind %d" % (kind, k))
