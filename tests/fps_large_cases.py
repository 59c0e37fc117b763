"""The clouds of the large-cloud farthest-point-sampling tier (csrc/fps_large.hip), shared by its CPU model
(tests/test_fps_large_model.py) and its device tests (tests/test_fps_large_gpu.py): one table, so that every cloud the kernel is
checked on is a cloud the numpy restatement of its rule has reproduced the oracle on.

A case is (name, make, npoint, group_len). make() -> (b, n, 3) float32 with 16384 < n; group_len is the L the CPU model runs
with (the device tests run every L on every case)."""
import numpy as np

from pointnet2_amd import synthetic as S


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def islands(c, shift):
    """The second half of every cloud moved ~shift away along x: the squared distance between the halves overflows to inf, which
    the reference's min() against the 1e38 start value turns into 1e38 (tf_sampling_g.cu:118,143)."""
    c = np.array(c, dtype=np.float32)
    c[:, c.shape[1] // 2:, 0] += np.float32(shift)
    return c


LARGE_CASES = [
    ("uniform20000", lambda: S.uniform_clouds(1, 20000, 1201), 400, 256),
    ("sphere16385", lambda: S.sphere_clouds(1, 16385, 1202), 300, 256),          # a one-record last group
    ("dropout20000", lambda: S.dropout_clouds(1, 20000, 1203), 300, 256),        # 87 % of the cloud on one spot
    ("lattice17000", lambda: S.lattice_clouds(1, 17000, 1204), 400, 128),        # 216 distinct points: exact ties everywhere
    ("duplicated18000", lambda: S.duplicated_clouds(1, 18000, 1205), 300, 64),
    ("quantized20000", lambda: S.quantized_clouds(1, 20000, 1206), 300, 256),
    ("identical16500", lambda: S.identical_clouds(1, 16500, 1207), 40, 256),     # nothing can be pruned
    ("uniform70000", lambda: S.uniform_clouds(1, 70000, 1208), 200, 64),         # 1094 groups: more than one group per thread
    ("islands_3e19", lambda: islands(S.uniform_clouds(1, 20000, 1209), 3e19), 200, 256),
    ("tiny_scale", lambda: _f32(S.sphere_clouds(1, 20000, 1210) * np.float32(1e-18)), 200, 256),   # squares are denormals
]

LARGE_NAMES = [c[0] for c in LARGE_CASES]
