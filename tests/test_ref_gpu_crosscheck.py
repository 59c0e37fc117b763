"""GPU cross-check of the ORACLE against the reference's own device kernels.

The reference has no CPU farthest-point-sampling, so the oracle's restatement of
tf_sampling_g.cu:105-170 (and in particular its tie rule) cannot be pinned by a
CPU run of reference code. oracle/Makefile target `ref_gpu` compiles the
reference .cu files UNMODIFIED for gfx950 (with -ffp-contract=off, i.e. the CPU
arithmetic the north star selects) into oracle/_ref/*.so; the .so files travel to
the GPU box with the snapshot. Here they are launched on the same inputs as the
oracle and the product kernels. Where oracle/_ref is not built, their outputs on
these inputs come from tests/golden/ref_gpu_kernels.npz instead, written from live
launches by tests/golden/make_golden_ref_gpu.py (a live launch is also checked
against that file). Test infrastructure only."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu


class RefKernels:
    """The reference kernels' outputs, case by case: launched live where oracle/_ref holds the kernels (and then equal to the
    stored outputs), else read from tests/golden/ref_gpu_kernels.npz."""

    def __init__(self, oracle, path):
        self.oracle = oracle
        self.stored = np.load(path)

    def get(self, group, key, launch):
        """-> the tuple of arrays `launch()` returns for case `key` (stored as <key>_0, <key>_1, ...)."""
        stored = tuple(self.stored[f] for f in sorted(f for f in self.stored.files if f.rsplit("_", 1)[0] == key))
        if not self.oracle.ref_available(group):
            assert stored, "no stored output for " + key
            return stored
        live = launch()
        assert len(live) == len(stored) and all(np.array_equal(a, b) for a, b in zip(live, stored)), \
            "reference kernel != its stored output: " + key
        return live


@pytest.fixture(scope="module")
def ref_kernels(oracle, golden_dir):
    return RefKernels(oracle, os.path.join(golden_dir, "ref_gpu_kernels.npz"))


def _fn(oracle, group, name, argtypes):
    f = oracle.ref_fn(group, name)
    f.argtypes = argtypes
    return f


def test_reference_fps_kernel_equals_oracle_and_product(cuda, oracle, ref_kernels):
    import pointnet2_amd as P
    for case, (xyz, m) in enumerate([
        (S.sphere_clouds(2, 1024, 0), 256),
        (S.duplicated_clouds(3, 1024, 1), 256),          # ties everywhere
        (S.dropout_clouds(2, 2048, 2), 300),
        (S.lattice_clouds(2, 1500, 3), 400),
        (S.identical_clouds(1, 700, 4), 30),
        (S.uniform_clouds(40, 600, 5), 64),              # b > 32: the reference grid-strides over batches
        (S.sphere_clouds(2, 4096, 6), 512),              # n > 3072: reference falls back to global reads
    ]):
        b, n, _ = xyz.shape
        x = torch.from_numpy(xyz).to(cuda)

        def launch():
            fn = _fn(oracle, "sampling_gpu", "farthestpointsamplingLauncher", [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3)
            temp = torch.empty((32, n), dtype=torch.float32, device=cuda)      # tf_sampling.cpp:115
            out = torch.zeros((b, m), dtype=torch.int32, device=cuda)
            torch.cuda.synchronize()
            fn(b, n, m, x.data_ptr(), temp.data_ptr(), out.data_ptr())         # null stream
            torch.cuda.synchronize()
            return (out.cpu().numpy(),)
        ref, = ref_kernels.get("sampling_gpu", "fps%d" % case, launch)
        assert np.array_equal(ref, oracle.farthest_point_sample(m, xyz)), "oracle != reference kernel"
        assert np.array_equal(ref, P.farthest_point_sample(m, x).cpu().numpy()), "product != reference kernel"


def test_reference_ball_query_kernel_equals_oracle_and_product(cuda, oracle, ref_kernels):
    import pointnet2_amd as P
    for case, (xyz, m, r, ns) in enumerate([(S.sphere_clouds(2, 1024, 7), 256, 0.2, 32), (S.duplicated_clouds(2, 900, 8), 100, 0.3, 64)]):
        b, n, _ = xyz.shape
        q = xyz[:, :m].copy()
        x, qq = torch.from_numpy(xyz).to(cuda), torch.from_numpy(q).to(cuda)

        def launch():
            fn = _fn(oracle, "grouping_gpu", "queryBallPointLauncher",
                     [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 4)
            idx = torch.zeros((b, m, ns), dtype=torch.int32, device=cuda)
            cnt = torch.zeros((b, m), dtype=torch.int32, device=cuda)
            torch.cuda.synchronize()
            fn(b, n, m, r, ns, x.data_ptr(), qq.data_ptr(), idx.data_ptr(), cnt.data_ptr())
            torch.cuda.synchronize()
            return (idx.cpu().numpy(),)
        ref_idx, = ref_kernels.get("grouping_gpu", "ball_query%d" % case, launch)
        widx, wcnt = oracle.query_ball_point(r, ns, xyz, q)
        # the device sqrtf may round differently from the host's in the last ulp; the oracle follows the CPU twin. Every row
        # where the reference GPU kernel disagrees must therefore contain a candidate ON the boundary: a point whose
        # sqrtf(squared distance) is within one ulp of the radius (this leg used to be a 99.9 % test)
        same = (ref_idx == widx).all(axis=2)
        assert same.mean() > 0.999
        r32 = np.float32(r)
        for bi, j in np.argwhere(~same):
            d = xyz[bi] - q[bi, j]                                     # fp32, the kernel's operand order does not matter for |.|
            s2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            root = np.sqrt(s2.astype(np.float32))
            ulps = np.abs(root.view(np.int32).astype(np.int64) - np.array(r32).view(np.int32).astype(np.int64))
            assert (ulps <= 1).any(), "query (%d, %d) differs from the reference GPU kernel without a boundary candidate" % (bi, j)
        pidx, pcnt = P.query_ball_point(r, ns, x, qq)
        assert np.array_equal(pidx.cpu().numpy(), widx) and np.array_equal(pcnt.cpu().numpy(), wcnt)


def test_reference_prob_sample_kernel_equals_oracle_and_product(cuda, oracle, ref_kernels):
    """Pins the oracle's restatement of the fp32 tiled scan (tf_sampling_g.cu:7-104) against the
    reference kernels themselves (probsampleLauncher = cumsumKernel + binarysearchKernel)."""
    import pointnet2_amd as P
    rng = np.random.default_rng(11)
    for case, (b, n, m) in enumerate([(2, 9000, 400), (3, 100, 64), (1, 8192, 33), (2, 16385, 100), (40, 700, 50), (2, 5, 10)]):
        p = rng.random((b, n), dtype=np.float32)
        r = rng.random((b, m), dtype=np.float32)
        dp, dr = torch.from_numpy(p).to(cuda), torch.from_numpy(r).to(cuda)

        def launch():
            fn = _fn(oracle, "sampling_gpu", "probsampleLauncher", [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4)
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
    for case, (b, m, n, k) in enumerate([(2, 9, 100, 7), (1, 5, 64, 64), (2, 3, 1000, 32)]):
        dist = np.round(rng.random((b, m, n), dtype=np.float32) * 40) / 40
        d = torch.from_numpy(dist).to(cuda)

        def launch():
            fn = _fn(oracle, "grouping_gpu", "selectionSortLauncher", [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3)
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
    pts = rng.random((3, 200, 7), dtype=np.float32)
    idx = rng.integers(0, 200, size=(3, 30, 16)).astype(np.int32)
    dp, di = torch.from_numpy(pts).to(cuda), torch.from_numpy(idx).to(cuda)

    def launch():
        fn = _fn(oracle, "grouping_gpu", "groupPointLauncher", [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3)
        out = torch.zeros((3, 30, 16, 7), dtype=torch.float32, device=cuda)
        torch.cuda.synchronize()
        fn(3, 200, 7, 30, 16, dp.data_ptr(), di.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        return (out.cpu().numpy(),)
    ref, = ref_kernels.get("grouping_gpu", "group_point", launch)
    assert np.array_equal(ref, oracle.group_point(pts, idx))
    assert np.array_equal(ref, P.group_point(dp, di).cpu().numpy())
