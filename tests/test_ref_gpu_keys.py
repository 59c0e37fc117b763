"""The stored outputs of the reference's device kernels (tests/golden/ref_gpu_kernels*.npz) hold every array that
tests/test_ref_gpu_crosscheck.py asks for, with the shape and type its case tables give: a table changed without
tests/golden/make_golden_ref_gpu.py run again fails here, without a GPU. The boundary-candidate rows of every ball-query input
of that module are counted here too: they bound what the reference kernel may change."""
import os

import numpy as np

import test_ref_gpu_crosscheck as T


def test_stored_reference_outputs_cover_every_case(golden_dir):
    files = T.stored_files(golden_dir)
    assert files
    have = {}
    for p in files:
        assert os.path.getsize(p) <= 1019256, p                      # the largest fixture before these
        with np.load(p) as z:
            for f in z.files:
                assert f not in have, f
                have[f] = (z[f].shape, z[f].dtype)
    want = T.stored_outputs()
    assert sorted(have) == sorted(want), sorted(set(have) ^ set(want))
    for key, (shape, dtype) in want.items():
        assert have[key] == (tuple(shape), dtype), (key, have[key], shape, dtype)
    kernels = T.RefKernels(None, files)                               # and the keys come back in output order
    for key in {k.rsplit("_", 1)[0] for k in want}:
        assert [kernels.stored[f].shape for f in sorted(f for f in kernels.stored if f.rsplit("_", 1)[0] == key)] == \
            [tuple(want["%s_%d" % (key, i)][0]) for i in range(sum(k.rsplit("_", 1)[0] == key for k in want))], key


def test_boundary_candidate_rows_stay_below_the_cap(oracle):
    m, r, ns = T.SA_STAGE
    inputs = [("sa_" + name, make, m, r) for name, make in T.SA_STAGE_INPUTS] + [(name, make, lm, lr) for name, make, lm, lr, _ in T.BALL_QUERY_LEGS]
    for name, make, m, r in inputs:
        xyz = make()
        q = oracle.gather_point(xyz, oracle.farthest_point_sample(m, xyz))
        rows = T.boundary_rows(xyz, q, r)
        print("%s: %d of %d rows have a boundary candidate" % (name, int(rows.sum()), rows.size))
        assert rows.mean() < T.BOUNDARY_ROWS_CAP, (name, int(rows.sum()), rows.size)
