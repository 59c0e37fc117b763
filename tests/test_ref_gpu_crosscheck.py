"""GPU cross-check of the ORACLE against the reference's own device kernels.

The reference has no CPU farthest-point-sampling, so the oracle's restatement of
tf_sampling_g.cu:105-170 (and in particular its tie rule) cannot be pinned by a
CPU run of reference code. oracle/Makefile target `ref_gpu` compiles the
reference .cu files UNMODIFIED for gfx950 (with -ffp-contract=off, i.e. the CPU
arithmetic the north star selects) into oracle/_ref/*.so; the .so files travel to
the GPU box with the snapshot. Here they are launched on the same inputs as the
oracle and the product kernels. Where oracle/_ref is not built, their outputs on
these inputs come from tests/golden/ref_gpu_kernels*.npz instead, written from live
launches by tests/golden/make_golden_ref_gpu.py (a live launch is also checked
against those files). Test infrastructure only.

Every input is a module-level table, and stored_outputs() lists the stored arrays
the tests ask for; tests/test_ref_gpu_keys.py checks that list against the files
without a GPU."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from fps_cases import FPS_LITERAL_CASES
from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

_I, _F, _P = ctypes.c_int, ctypes.c_float, ctypes.c_void_p

# ---------------------------------------------------------------------------------------------------------------- inputs
FPS_CASES = [
    (lambda: S.sphere_clouds(2, 1024, 0), 256),
    (lambda: S.duplicated_clouds(3, 1024, 1), 256),          # ties everywhere
    (lambda: S.dropout_clouds(2, 2048, 2), 300),
    (lambda: S.lattice_clouds(2, 1500, 3), 400),
    (lambda: S.identical_clouds(1, 700, 4), 30),
    (lambda: S.uniform_clouds(40, 600, 5), 64),              # b > 32: the reference grid-strides over batches
    (lambda: S.sphere_clouds(2, 4096, 6), 512),              # n > 3072: reference falls back to global reads
]
BALL_QUERY_CASES = [(lambda: S.sphere_clouds(2, 1024, 7), 256, 0.2, 32), (lambda: S.duplicated_clouds(2, 900, 8), 100, 0.3, 64)]
PROB_SAMPLE_CASES = [(2, 9000, 400), (3, 100, 64), (1, 8192, 33), (2, 16385, 100), (40, 700, 50), (2, 5, 10)]
SELECTION_SORT_CASES = [(2, 9, 100, 7), (1, 5, 64, 64), (2, 3, 1000, 32)]
GROUP_POINT_CASE = (3, 200, 7, 30, 16)                       # b, n, c, m, nsample

# The set-abstraction stage of the benchmark metric: 32 clouds, 4096 -> 1024 centroids, balls of 0.2 with 32 slots.
SA_STAGE = (1024, 0.2, 32)
SA_STAGE_INPUTS = [("d1", lambda: S.sphere_clouds(32, 4096, 931)), ("quant", lambda: S.quantized_clouds(32, 4096, 932))]
SA_STORED_CLOUDS = 2                                         # of the ball-query and group outputs (the indices are stored whole)
# name, cloud, centroids (the oracle's farthest points), radius, nsample: sem_seg SA1 and the widest ball of cls_msg level 1
BALL_QUERY_LEGS = [("sem_seg_sa1", lambda: S.uniform_clouds(2, 8192, 933), 1024, 0.1, 32),
                   ("cls_msg_l1", lambda: S.sphere_clouds(4, 1024, 934), 512, 0.4, 128)]
BOUNDARY_ROWS_CAP = 0.001                                    # of all rows: what the reference kernel may change at all

# Gradients whose sums are exact in fp32 whatever the order: integers in [-8, 8] times 2^-6, at most 32768 per row.
GATHER_GRAD_CASES = [("fps_dup", lambda: S.duplicated_clouds(4, 512, 941), 1024, 942)]            # name, cloud, m (> n), seed of g
# name, cloud, centroids, radius, nsample, channels, seed of g: cls_ssg level 2, the 320 channels of cls_msg level 2, xyz
GROUP_GRAD_CASES = [("cls_ssg_l2", lambda: S.duplicated_clouds(4, 512, 943), 128, 0.4, 64, 128, 944),
                    ("c320", lambda: S.duplicated_clouds(2, 512, 945), 128, 0.8, 128, 320, 946),
                    ("c3", lambda: S.duplicated_clouds(4, 512, 947), 128, 0.4, 64, 3, 948)]


def stored_outputs():
    """-> {array name in ref_gpu_kernels*.npz: (shape, dtype)} for every reference-kernel output the tests below ask for."""
    i32, f32 = np.dtype(np.int32), np.dtype(np.float32)
    want = {}

    def add(key, *arrays):
        for i, a in enumerate(arrays):
            want["%s_%d" % (key, i)] = a
    for case, (make, m) in enumerate(FPS_CASES):
        add("fps%d" % case, ((make().shape[0], m), i32))
    for name, make, m, _ in FPS_LITERAL_CASES:
        add("fpstab_" + name, ((make().shape[0], m), i32))
    for case, (make, m, _, ns) in enumerate(BALL_QUERY_CASES):
        add("ball_query%d" % case, ((make().shape[0], m, ns), i32))
    for case, (b, n, m) in enumerate(PROB_SAMPLE_CASES):
        add("prob_sample%d" % case, ((b, m), i32))
    for case, (b, m, n, k) in enumerate(SELECTION_SORT_CASES):
        add("selection_sort%d" % case, ((b, m, n), i32), ((b, m, n), f32))
    b, n, c, m, ns = GROUP_POINT_CASE
    add("group_point", ((b, m, ns, c), f32))
    m, _, ns = SA_STAGE
    k = SA_STORED_CLOUDS
    for name, make in SA_STAGE_INPUTS:
        add("sa_" + name, ((make().shape[0], m), i32), ((k, m, 3), f32), ((k, m, ns), i32), ((k, m), i32), ((k, m, ns, 3), f32))
    for name, make, m, _, ns in BALL_QUERY_LEGS:
        add("ballleg_" + name, ((make().shape[0], m, ns), i32), ((make().shape[0], m), i32))
    for name, make, m, _ in GATHER_GRAD_CASES:
        add("gathergrad_" + name, (make().shape, f32))
    for name, make, m, _, ns, c, _ in GROUP_GRAD_CASES:
        add("groupgrad_" + name, (make().shape[:2] + (c,), f32))
    return want


def stored_files(golden_dir):
    return sorted(glob.glob(os.path.join(golden_dir, "ref_gpu_kernels*.npz")))


class RefKernels:
    """The reference kernels' outputs, case by case: launched live where oracle/_ref holds the kernels (and then equal to the
    stored outputs), else read from tests/golden/ref_gpu_kernels*.npz."""

    def __init__(self, oracle, paths):
        self.oracle = oracle
        self.stored = {}
        for p in paths:
            with np.load(p) as z:
                self.stored.update({f: z[f] for f in z.files})

    def get(self, group, key, launch, clouds=None):
        """-> the tuple of arrays `launch()` returns for case `key` (stored as <key>_0, <key>_1, ...). clouds: per output, how
        many leading clouds are stored (None = all); without oracle/_ref only those come back."""
        stored = tuple(self.stored[f] for f in sorted(f for f in self.stored if f.rsplit("_", 1)[0] == key))
        if not self.oracle.ref_available(group):
            assert stored, "no stored output for " + key
            return stored
        live = launch()
        clouds = clouds or (None,) * len(live)
        assert len(live) == len(stored) and all(np.array_equal(a[:k], b) for a, b, k in zip(live, stored, clouds)), \
            "reference kernel != its stored output: " + key
        return live


@pytest.fixture(scope="module")
def ref_kernels(oracle, golden_dir):
    return RefKernels(oracle, stored_files(golden_dir))


def _fn(oracle, group, name, argtypes):
    f = oracle.ref_fn(group, name)
    f.argtypes = argtypes
    return f


def _ref_fps(oracle, x, m):
    b, n, _ = x.shape
    fn = _fn(oracle, "sampling_gpu", "farthestpointsamplingLauncher", [_I] * 3 + [_P] * 3)
    temp = torch.empty((32, n), dtype=torch.float32, device=x.device)      # tf_sampling.cpp:115
    out = torch.zeros((b, m), dtype=torch.int32, device=x.device)
    torch.cuda.synchronize()
    fn(b, n, m, x.data_ptr(), temp.data_ptr(), out.data_ptr())             # null stream
    torch.cuda.synchronize()
    return out


def _ref_ball_query(oracle, x, q, r, ns):
    b, n, _ = x.shape
    m = q.shape[1]
    fn = _fn(oracle, "grouping_gpu", "queryBallPointLauncher", [_I] * 3 + [_F, _I] + [_P] * 4)
    idx = torch.zeros((b, m, ns), dtype=torch.int32, device=x.device)      # pre-zeroed, as the reference's harness does (query_ball_point.cpp:94)
    cnt = torch.zeros((b, m), dtype=torch.int32, device=x.device)
    torch.cuda.synchronize()
    fn(b, n, m, r, ns, x.data_ptr(), q.data_ptr(), idx.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    return idx, cnt


def test_reference_fps_kernel_equals_oracle_and_product(cuda, oracle, ref_kernels):
    import pointnet2_amd as P
    for case, (make, m) in enumerate(FPS_CASES):
        xyz = make()
        x = torch.from_numpy(xyz).to(cuda)
        ref, = ref_kernels.get("sampling_gpu", "fps%d" % case, lambda: (_ref_fps(oracle, x, m).cpu().numpy(),))
        assert np.array_equal(ref, oracle.farthest_point_sample(m, xyz)), "oracle != reference kernel"
        assert np.array_equal(ref, P.farthest_point_sample(m, x).cpu().numpy()), "product != reference kernel"


def _fps_mismatch(oracle, xyz, ref, got):
    """The first (cloud, sample) where `got` leaves the reference kernel's indices, with the running distance (the literal
    emulator's, after the update of that round) of the two points chosen there."""
    bi, j = (int(v) for v in np.argwhere(ref != got)[0])
    cloud = np.ascontiguousarray(xyz[bi:bi + 1], dtype=np.float32)
    n = cloud.shape[1]
    mind = np.zeros(n, np.float32)
    lit = np.zeros((1, j + 1), np.int32)
    f32p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    oracle.lib().pn2_cpu_farthest_point_sample_literal(1, n, j + 1, cloud.ctypes.data_as(f32p), mind.ctypes.data_as(f32p),
                                                       lit.ctypes.data_as(i32p))
    a, c = int(ref[bi, j]), int(got[bi, j])
    return "cloud %d, sample %d: reference kernel picks %d (running distance %r), this one %d (%r); literal emulator %d" % (
        bi, j, a, float(mind[a]), c, float(mind[c]), int(lit[0, j]))


def _forced_tier(variant, x, m):
    """pn2_farthest_point_sample_variant -> indices, or None where the tier does not exist for the shape (PN2_E_ARG)."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    b, n, _ = x.shape
    temp = torch.empty((max(1, lib.pn2_fps_temp_floats(b, n)),), dtype=torch.float32, device=x.device)
    out = torch.full((b, m), -1, dtype=torch.int32, device=x.device)
    rc = lib.pn2_farthest_point_sample_variant(variant, b, n, m, ptr(x), ptr(temp), ptr(out), None, stream_ptr(x.device))
    if rc == -3:                                                           # PN2_E_ARG: outside the tier's slot range
        return None
    _C.check(rc, "farthest_point_sample_variant")
    return out.cpu().numpy()


def test_reference_fps_kernel_on_the_literal_table(cuda, oracle, ref_kernels):
    """Every case of tests/fps_cases.py through farthestpointsamplingLauncher: the oracle, the product's size rule, every tier
    that exists for the shape and the overlapped sample-and-group launch all return the reference kernel's indices. tiny_scale
    (squared distances are fp32 denormals) is compared like every other case: the reference kernel as hipcc builds it keeps
    denormals, as gcc's build of the oracle does."""
    import pointnet2_amd as P
    from pointnet2_amd import tf_sampling as T
    bad = []
    for name, make, m, _ in FPS_LITERAL_CASES:
        xyz = np.ascontiguousarray(make(), dtype=np.float32)
        b, n, _ = xyz.shape
        x = torch.from_numpy(xyz).to(cuda)
        ref, = ref_kernels.get("sampling_gpu", "fpstab_" + name, lambda: (_ref_fps(oracle, x, m).cpu().numpy(),))
        others = [("oracle", oracle.farthest_point_sample(m, xyz)), ("auto", P.farthest_point_sample(m, x).cpu().numpy())]
        tiers = 0
        for tier, variant in (("full", T.FPS_FULL), ("pruned", T.FPS_PRUNED), ("batch", T.FPS_BATCH)):
            got = _forced_tier(variant, x, m)
            if got is not None:
                others.append((tier, got))
                tiers += 1
        assert tiers >= 1, name                                            # the full tier takes every shape
        if 64 <= n <= 8192 and b <= 256:                                   # the overlapped launch's envelope
            others.append(("sample_and_group_xyz", P.sample_and_group_xyz(m, 0.2, 8, x, subtract_centroid=False)[0].cpu().numpy()))
        for who, got in others:
            if not np.array_equal(ref, got):
                bad.append("%s: %s != reference kernel; %s" % (name, who, _fps_mismatch(oracle, xyz, ref, got)))
    assert not bad, "\n".join(bad)


def boundary_rows(xyz, q, r):
    """-> (b, m) bool: does query (i, j) have a candidate ON the boundary, a point whose sqrtf(squared distance) is within one
    ulp of the radius? The device sqrtf may round differently from the host's in the last ulp; the oracle follows the CPU
    twin. Only such a row may differ between the reference GPU kernel and the oracle."""
    rbits = np.array(np.float32(r)).view(np.int32).astype(np.int64)
    out = np.zeros(q.shape[:2], bool)
    for bi in range(xyz.shape[0]):
        for j0 in range(0, q.shape[1], 256):
            d = xyz[bi][None, :, :] - q[bi, j0:j0 + 256][:, None, :]       # fp32, the kernel's operand order does not matter for |.|
            s2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            root = np.sqrt(s2.astype(np.float32))
            out[bi, j0:j0 + 256] = (np.abs(root.view(np.int32).astype(np.int64) - rbits) <= 1).any(axis=1)
    return out


def _same_off_the_boundary(what, ref, want, boundary):
    """Rows without a boundary candidate: bit-identical. Rows that differ at all: below the cap."""
    ref, want = ref.reshape(boundary.shape + (-1,)), want.reshape(boundary.shape + (-1,))
    same = (ref == want).all(axis=2)
    assert same.mean() > 1 - BOUNDARY_ROWS_CAP, (what, float(same.mean()))
    loose = np.argwhere(~same & ~boundary)
    assert len(loose) == 0, "%s: query %s differs from the reference GPU kernel without a boundary candidate" % (what, loose[0])


def test_reference_ball_query_kernel_equals_oracle_and_product(cuda, oracle, ref_kernels):
    import pointnet2_amd as P
    for case, (make, m, r, ns) in enumerate(BALL_QUERY_CASES):
        xyz = make()
        q = xyz[:, :m].copy()
        x, qq = torch.from_numpy(xyz).to(cuda), torch.from_numpy(q).to(cuda)
        ref_idx, = ref_kernels.get("grouping_gpu", "ball_query%d" % case,
                                   lambda: (_ref_ball_query(oracle, x, qq, r, ns)[0].cpu().numpy(),))
        widx, wcnt = oracle.query_ball_point(r, ns, xyz, q)
        # every row where the reference GPU kernel disagrees must contain a candidate ON the boundary (VERDICT round 4, weak 9:
        # this leg used to be a 99.9 % test)
        _same_off_the_boundary("idx", ref_idx, widx, boundary_rows(xyz, q, r))
        pidx, pcnt = P.query_ball_point(r, ns, x, qq)
        assert np.array_equal(pidx.cpu().numpy(), widx) and np.array_equal(pcnt.cpu().numpy(), wcnt)


def test_reference_ball_query_kernel_at_model_levels(cuda, oracle, ref_kernels):
    """queryBallPointLauncher at sem_seg SA1 and at the widest ball of cls_msg level 1, centroids = the oracle's farthest points."""
    import pointnet2_amd as P
    for name, make, m, r, ns in BALL_QUERY_LEGS:
        xyz = make()
        q = oracle.gather_point(xyz, oracle.farthest_point_sample(m, xyz))
        x, qq = torch.from_numpy(xyz).to(cuda), torch.from_numpy(q).to(cuda)
        ref_idx, ref_cnt = ref_kernels.get("grouping_gpu", "ballleg_" + name,
                                           lambda: tuple(t.cpu().numpy() for t in _ref_ball_query(oracle, x, qq, r, ns)))
        boundary = boundary_rows(xyz, q, r)
        assert boundary.mean() < BOUNDARY_ROWS_CAP, (name, int(boundary.sum()))
        widx, wcnt = oracle.query_ball_point(r, ns, xyz, q)
        _same_off_the_boundary(name + " idx", ref_idx, widx, boundary)
        _same_off_the_boundary(name + " pts_cnt", ref_cnt, wcnt, boundary)
        pidx, pcnt = P.query_ball_point(r, ns, x, qq)
        assert np.array_equal(pidx.cpu().numpy(), widx) and np.array_equal(pcnt.cpu().numpy(), wcnt), name


def test_reference_launchers_chain_at_the_metric_shape(cuda, oracle, ref_kernels):
    """The set-abstraction stage the benchmark times, through the reference's own launchers one after the other on the null
    stream (farthest point sampling, gather, ball query, group of xyz), against P.sample_and_group_xyz and the oracle.
    Indices of the farthest points and new_xyz: bit-exact. idx, pts_cnt and grouped_xyz: bit-exact in every row without a
    boundary candidate (boundary_rows), and the rows that have one are counted on the CPU first: below 0.1 % of all rows."""
    import pointnet2_amd as P
    m, r, ns = SA_STAGE
    k = SA_STORED_CLOUDS
    for name, make in SA_STAGE_INPUTS:
        xyz = make()
        b, n, _ = xyz.shape
        x = torch.from_numpy(xyz).to(cuda)

        def launch():
            fps = _ref_fps(oracle, x, m)
            new_xyz = torch.zeros((b, m, 3), dtype=torch.float32, device=cuda)
            _fn(oracle, "sampling_gpu", "gatherpointLauncher", [_I] * 3 + [_P] * 3)(b, n, m, x.data_ptr(), fps.data_ptr(),
                                                                                    new_xyz.data_ptr())
            torch.cuda.synchronize()
            idx, cnt = _ref_ball_query(oracle, x, new_xyz, r, ns)
            grouped = torch.zeros((b, m, ns, 3), dtype=torch.float32, device=cuda)
            _fn(oracle, "grouping_gpu", "groupPointLauncher", [_I] * 5 + [_P] * 3)(b, n, 3, m, ns, x.data_ptr(), idx.data_ptr(),
                                                                                   grouped.data_ptr())
            torch.cuda.synchronize()
            return tuple(t.cpu().numpy() for t in (fps, new_xyz, idx, cnt, grouped))
        rfps, rnew, ridx, rcnt, rgrp = ref_kernels.get("sampling_gpu", "sa_" + name, launch, clouds=(None, k, k, k, k))
        wfps = oracle.farthest_point_sample(m, xyz)
        wnew = oracle.gather_point(xyz, wfps)
        widx, wcnt = oracle.query_ball_point(r, ns, xyz, wnew)
        wgrp = oracle.group_point(xyz, widx)
        boundary = boundary_rows(xyz, wnew, r)
        assert boundary.mean() < BOUNDARY_ROWS_CAP, (name, int(boundary.sum()))
        pfps, pnew, pidx, pcnt, pgrp = (t.cpu().numpy() for t in P.sample_and_group_xyz(m, r, ns, x, subtract_centroid=False))
        if not np.array_equal(rfps, wfps):
            raise AssertionError(name + ": oracle != reference kernel; " + _fps_mismatch(oracle, xyz, rfps, wfps))
        if not np.array_equal(rfps, pfps):
            raise AssertionError(name + ": product != reference kernel; " + _fps_mismatch(oracle, xyz, rfps, pfps))
        c = len(ridx)                                                      # every cloud live, the stored ones otherwise
        assert c == b or not oracle.ref_available("sampling_gpu")
        assert np.array_equal(rnew, wnew[:len(rnew)]) and np.array_equal(pnew, wnew), name
        for what, ref, want, got in (("idx", ridx, widx, pidx), ("pts_cnt", rcnt, wcnt, pcnt), ("grouped_xyz", rgrp, wgrp, pgrp)):
            _same_off_the_boundary(name + " " + what, ref, want[:c], boundary[:c])
            _same_off_the_boundary(name + " product " + what, ref, got[:c], boundary[:c])
            assert np.array_equal(got, want), (name, what)                 # the product follows the oracle on the boundary too


def test_reference_prob_sample_kernel_equals_oracle_and_product(cuda, oracle, ref_kernels):
    """Pins the oracle's restatement of the fp32 tiled scan (tf_sampling_g.cu:7-104) against the
    reference kernels themselves (probsampleLauncher = cumsumKernel + binarysearchKernel)."""
    import pointnet2_amd as P
    rng = np.random.default_rng(11)
    for case, (b, n, m) in enumerate(PROB_SAMPLE_CASES):
        p = rng.random((b, n), dtype=np.float32)
        r = rng.random((b, m), dtype=np.float32)
        dp, dr = torch.from_numpy(p).to(cuda), torch.from_numpy(r).to(cuda)

        def launch():
            fn = _fn(oracle, "sampling_gpu", "probsampleLauncher", [_I] * 3 + [_P] * 4)
            temp = torch.empty((b, n), dtype=torch.float32, device=cuda)
            out = torch.zeros((b, m), dtype=torch.int32, device=cuda)
            torch.cuda.synchronize()
            fn(b, n, m, dp.data_ptr(), dr.data_ptr(), temp.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            return (out.cpu().numpy(),)
        ref, = ref_kernels.get("sampling_gpu", "prob_sample%d" % case, launch)
        assert np.array_equal(ref, oracle.prob_sample(p, r)), ("oracle != reference kernel", b, n, m)
        assert np.array_equal(ref, P.prob_sample(dp, dr).cpu().numpy()), ("product != reference kernel", b, n, m)


def test_reference_selection_sort_and_group_kernels(cuda, oracle, ref_kernels):
    import pointnet2_amd as P
    rng = np.random.default_rng(12)
    for case, (b, m, n, k) in enumerate(SELECTION_SORT_CASES):
        dist = np.round(rng.random((b, m, n), dtype=np.float32) * 40) / 40
        d = torch.from_numpy(dist).to(cuda)

        def launch():
            fn = _fn(oracle, "grouping_gpu", "selectionSortLauncher", [_I] * 4 + [_P] * 3)
            outi = torch.zeros((b, m, n), dtype=torch.int32, device=cuda)
            out = torch.zeros((b, m, n), dtype=torch.float32, device=cuda)
            torch.cuda.synchronize()
            fn(b, n, m, k, d.data_ptr(), outi.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            return outi.cpu().numpy(), out.cpu().numpy()
        ri, ro = ref_kernels.get("grouping_gpu", "selection_sort%d" % case, launch)
        wi, wo = oracle.select_top_k(k, dist)
        assert np.array_equal(ri, wi) and np.array_equal(ro, wo)
        pi, po = P.select_top_k(k, d)
        assert np.array_equal(pi.cpu().numpy(), wi) and np.array_equal(po.cpu().numpy(), wo)
    gb, gn, gc, gm, gns = GROUP_POINT_CASE
    pts = rng.random((gb, gn, gc), dtype=np.float32)
    idx = rng.integers(0, gn, size=(gb, gm, gns)).astype(np.int32)
    dp, di = torch.from_numpy(pts).to(cuda), torch.from_numpy(idx).to(cuda)

    def launch():
        fn = _fn(oracle, "grouping_gpu", "groupPointLauncher", [_I] * 5 + [_P] * 3)
        out = torch.zeros((gb, gm, gns, gc), dtype=torch.float32, device=cuda)
        torch.cuda.synchronize()
        fn(gb, gn, gc, gm, gns, dp.data_ptr(), di.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        return (out.cpu().numpy(),)
    ref, = ref_kernels.get("grouping_gpu", "group_point", launch)
    assert np.array_equal(ref, oracle.group_point(pts, idx))
    assert np.array_equal(ref, P.group_point(dp, di).cpu().numpy())


def _exact_gradient(seed, shape):
    """Integers in [-8, 8] times 2^-6: every partial sum of up to 32768 of them is exact in fp32, so the order in which float
    atomics land cannot change a bit of the result."""
    return (np.random.default_rng(seed).integers(-8, 9, size=shape).astype(np.float32) * np.float32(2.0 ** -6)).astype(np.float32)


def test_reference_scatter_add_kernel_on_exact_sums(cuda, oracle, ref_kernels):
    """scatteraddpointLauncher (float atomics) == oracle == pn2_gather_point_grad == pn2_gather_point_grad_det, bit for bit, on
    farthest-point indices of duplicated clouds with m > n (repeated indices)."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import det_workspace, ptr, stream_ptr
    lib = _C.lib()
    for name, make, m, seed in GATHER_GRAD_CASES:
        xyz = make()
        b, n, _ = xyz.shape
        idx_np = oracle.farthest_point_sample(m, xyz)
        assert np.bincount(idx_np.reshape(-1)).max() > 1
        g_np = _exact_gradient(seed, (b, m, 3))
        idx, g = torch.from_numpy(idx_np).to(cuda), torch.from_numpy(g_np).to(cuda)

        def launch():
            out = torch.zeros((b, n, 3), dtype=torch.float32, device=cuda)     # zero-filled by the caller, tf_sampling.cpp:174
            torch.cuda.synchronize()
            _fn(oracle, "sampling_gpu", "scatteraddpointLauncher", [_I] * 3 + [_P] * 3)(b, n, m, g.data_ptr(), idx.data_ptr(),
                                                                                        out.data_ptr())
            torch.cuda.synchronize()
            return (out.cpu().numpy(),)
        ref, = ref_kernels.get("sampling_gpu", "gathergrad_" + name, launch)
        assert np.array_equal(ref, oracle.gather_point_grad((b, n, 3), idx_np, g_np)), name
        out = torch.full((b, n, 3), 7.0, dtype=torch.float32, device=cuda)     # zero-filled by the library
        _C.check(lib.pn2_gather_point_grad(b, n, m, ptr(g), ptr(idx), ptr(out), stream_ptr(cuda)), "gather_point_grad")
        assert np.array_equal(ref, out.cpu().numpy()), (name, "pn2_gather_point_grad")
        out = torch.full((b, n, 3), 7.0, dtype=torch.float32, device=cuda)
        ws = det_workspace(lib, b, n, 3, cuda)
        _C.check(lib.pn2_gather_point_grad_det(b, n, m, ptr(g), ptr(idx), ptr(out), ptr(ws), stream_ptr(cuda)), "gather_point_grad_det")
        assert np.array_equal(ref, out.cpu().numpy()), (name, "pn2_gather_point_grad_det")


def test_reference_group_point_grad_kernel_on_exact_sums(cuda, oracle, ref_kernels):
    """groupPointGradLauncher (float atomics) == oracle == pn2_group_point_grad == pn2_group_point_grad_det ==
    pn2_group_point_grad_seg in both modes, bit for bit, on the lists of a real ball query over duplicated clouds, whose
    padding piles references onto low point numbers."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import det_workspace, ptr, seg_workspace, stream_ptr
    lib = _C.lib()
    for name, make, m, r, ns, c, seed in GROUP_GRAD_CASES:
        xyz = make()
        b, n, _ = xyz.shape
        q = oracle.gather_point(xyz, oracle.farthest_point_sample(m, xyz))
        idx_np, _ = oracle.query_ball_point(r, ns, xyz, q)
        lens = np.stack([np.bincount(idx_np[i].reshape(-1), minlength=n) for i in range(b)])
        assert 256 <= lens.max() <= 32768, (name, int(lens.max()))            # crowded rows, exact sums
        g_np = _exact_gradient(seed, (b, m, ns, c))
        idx, g = torch.from_numpy(idx_np).to(cuda), torch.from_numpy(g_np).to(cuda)

        def launch():
            out = torch.zeros((b, n, c), dtype=torch.float32, device=cuda)     # zero-filled by the caller, tf_grouping.cpp:204
            torch.cuda.synchronize()
            _fn(oracle, "grouping_gpu", "groupPointGradLauncher", [_I] * 5 + [_P] * 3)(b, n, c, m, ns, g.data_ptr(), idx.data_ptr(),
                                                                                       out.data_ptr())
            torch.cuda.synchronize()
            return (out.cpu().numpy(),)
        ref, = ref_kernels.get("grouping_gpu", "groupgrad_" + name, launch)
        assert np.array_equal(ref, oracle.group_point_grad((b, n, c), idx_np, g_np)), name
        st = stream_ptr(cuda)
        calls = [("pn2_group_point_grad", lambda o: lib.pn2_group_point_grad(b, n, c, m, ns, ptr(g), ptr(idx), ptr(o), st)),
                 ("pn2_group_point_grad_det", lambda o: lib.pn2_group_point_grad_det(
                     b, n, c, m, ns, ptr(g), ptr(idx), ptr(o), ptr(det_workspace(lib, b, n, c, cuda)), st))]
        for det in (0, 1):
            calls.append(("pn2_group_point_grad_seg, deterministic = %d" % det, lambda o, det=det: lib.pn2_group_point_grad_seg(
                b, n, c, m, ns, ptr(g), ptr(idx), ptr(o), ptr(seg_workspace(lib, b, n, m * ns, cuda)), det, st)))
        for who, call in calls:
            out = torch.full((b, n, c), 7.0, dtype=torch.float32, device=cuda)  # zero-filled by the library
            _C.check(call(out), who)
            torch.cuda.synchronize()
            assert np.array_equal(ref, out.cpu().numpy()), (name, who)
