"""The clouds of the large-cloud farthest-point-sampling tier (csrc/fps_large.hip), shared by its CPU model
(tests/test_fps_large_model.py) and its device tests (tests/test_fps_large_gpu.py): one table, so that every cloud the kernel is
checked on is a cloud the numpy restatement of its rule has reproduced the oracle on.

A case is (name, make, npoint, group_len). make() -> (b, n, 3) float32 with 16384 < n; group_len is the L the CPU model runs
with. The device tests run every L on every case of LARGE_CASES, and a case of FULL_TABLE_CASES at its own L and every larger
one (a smaller L would need more than the 4096 groups the kernel has box slots for)."""
import numpy as np

from fps_cases import NAN, INF, X, Y, denormal_z, poke
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
    # non-finite coordinates inside the cloud (tests/fps_cases.py): the first such point in (k mod 512, k) order is picked in
    # round 1 and in every round after it, at value 1e38. Its box distance is inf (an infinite coordinate: every finite box is
    # skipped) or NaN (a NaN coordinate: nothing is skipped) in every round; boxes leave their NaN members out.
    ("nonfinite_20000", lambda: poke(S.uniform_clouds(1, 20000, 1402), [(16400, X, -INF), (19999, Y, NAN)]), 100, 256),
    ("first_nan_20000", lambda: poke(S.uniform_clouds(1, 20000, 1403), [(0, X, NAN)]), 100, 128),            # every sample is 0
    ("quarter_nan_20000", lambda: poke(S.uniform_clouds(1, 20000, 1404), [(k, X, NAN) for k in range(1, 20000, 4)]), 100, 64),
    # an axis whose extent is a denormal: the scale 32 / extent overflows, every point in bin 0 of that axis
    ("denormal_extent_20000", lambda: denormal_z(S.uniform_clouds(1, 20000, 1405)), 200, 256),
]

LARGE_NAMES = [c[0] for c in LARGE_CASES]

# The whole table of box and key slots: lane l of wave w keeps group w + 16 (64 i + l) in slot i < 4, so slot i starts at group
# 1024 i. 4096 groups need 4096 L points and nothing smaller reaches slot 3; npoint of tens keeps a device run in milliseconds.
# (name, make, npoint, group_len, groups)
FULL_TABLE_CASES = [
    ("full_table_64", lambda: S.uniform_clouds(2, 262144, 1401), 64, 64, 4096),
    ("full_table_128", lambda: S.sphere_clouds(1, 524288, 1401), 64, 128, 4096),
    ("full_table_256", lambda: S.uniform_clouds(1, 1048576, 1401), 48, 256, 4096),
    ("slot2_first_group", lambda: S.uniform_clouds(1, 131073, 1411), 64, 64, 2049),   # one group in slot 2, holding one record
]

FULL_TABLE_NAMES = [c[0] for c in FULL_TABLE_CASES]
