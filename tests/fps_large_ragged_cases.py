"""The ragged batches of the large-cloud farthest-point-sampling entry (pn2_farthest_point_sample_large_ragged, DESIGN.md 4.1e
"with lengths"), shared by the CPU model test (tests/test_fps_large_ragged_model.py) and the device tests
(tests/test_fps_large_ragged_gpu.py): one table, so that the short slices the device is checked on are slices the numpy
restatement of the grouping rule has reproduced the oracle on.

A case is name -> (generator, seed, padded n, lengths or None (= every cloud full), npoint, npoints or None). Padded n of
16385 .. 20000 and npoint of 40 .. 300 keep the oracle and the launch in the millisecond range; TABLE_CASES, of the same form,
is the one batch that needs 262144 points."""
import functools

import numpy as np

from fps_cases import NAN, INF, X, Y, Z, poke
from pointnet2_amd import synthetic as S


def nonfinite_clouds(b, n, seed):
    """Five uniform clouds with non-finite coordinates placed against the lengths of the "nonfinite" case below: several kinds
    inside cloud 0; the ONLY one of cloud 1 just below its length and that of cloud 2 just beyond (so cloud 2 is a finite cloud:
    the point is padding); cloud 3 starts on a NaN point (every sample 0); cloud 4 has +inf in the last point of a slice of
    256 x 64 + 1 records."""
    assert b == 5 and n == 17000
    c = S.uniform_clouds(b, n, seed)
    for cloud_no, k, axis, value in [(0, 16400, X, -INF), (0, 9000, Y, NAN), (0, 37, Z, INF), (1, 4999, Y, NAN), (2, 700, X, NAN),
                                     (3, 0, X, NAN), (4, 16384, Z, INF)]:
        c[cloud_no] = poke(c[cloud_no:cloud_no + 1], [(k, axis, value)])[0]
    return c


CASES = {
    # group boundaries at every group length (16640 = 65 x 256), the dense envelope's edge, fewer than 16 groups, one group, one
    # record, and exhausted clouds (m > n_c)
    "boundaries": (S.uniform_clouds, 1301, 17000, [17000, 16641, 16640, 16639, 16385, 9000, 257, 256, 65, 64, 2, 1], 96, None),
    # ties
    "lattice": (S.lattice_clouds, 1302, 17000, [17000, 5000, 700], 300, None),
    "duplicated": (S.duplicated_clouds, 1303, 17000, [17000, 5000, 700], 300, None),
    "identical": (S.identical_clouds, 1304, 17000, [16500, 600, 1], 40, None),
    # per-cloud sample counts, with and without lengths
    "counts": (S.sphere_clouds, 1305, 20000, [20000, 37, 16385, 600], 128, [1, 2, 127, 128]),
    "counts_full": (S.sphere_clouds, 1305, 20000, None, 128, [1, 2, 127, 128]),
    # non-finite points INSIDE the valid lengths (nonfinite_clouds above); the one at [2, 700] is beyond its cloud's length
    "nonfinite": (nonfinite_clouds, 1306, 17000, [17000, 5000, 700, 300, 16385], 96, None),
}

# The whole group table beside shorter slices (group length 64): one workgroup uses all four box slots per lane, its neighbours
# three of them (2049 groups: one record in slot 2), two (1094 groups) and not even one whole wave (1 record). Run by the
# global-memory kernel and by the tier at group length 64 only (any larger one leaves slots empty), under NaN padding.
TABLE_CASES = {
    "full_table": (S.uniform_clouds, 1421, 262144, [262144, 131073, 70000, 1], 64, None),
}
_ALL = {**CASES, **TABLE_CASES}

# the CPU model's slices: below the dense envelope of the tier, around one group and around 16 groups of every group length
MODEL_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 3000]
MODEL_M = 96
MODEL_KINDS = {"uniform": "boundaries", "lattice": "lattice", "identical": "identical", "nonfinite": "nonfinite"}


@functools.lru_cache(maxsize=None)
def cloud(name):
    """(b, padded n, 3) float32 of the case, read-only."""
    gen, seed, n, lengths, _, npoints = _ALL[name]
    xyz = np.ascontiguousarray(gen(len(lengths if lengths is not None else npoints), n, seed), dtype=np.float32)
    xyz.setflags(write=False)
    return xyz


def lengths_of(name):
    _, _, n, lengths, _, npoints = _ALL[name]
    return list(lengths) if lengths is not None else [n] * len(npoints)


def slice_rule(oracle, xyz, lengths, m, npoints=None):
    """THE SLICE RULE (tests/test_ragged_fps_tiers_gpu.py, case()): cloud i's rows are the oracle's on xyz[i:i+1, :lengths[i]],
    truncated to npoints[i]; the rows from there on are index 0."""
    want = np.zeros((len(lengths), m), dtype=np.int32)
    for i, ni in enumerate(lengths):
        mi = m if npoints is None else npoints[i]
        want[i, :mi] = oracle.farthest_point_sample(m, np.ascontiguousarray(xyz[i:i + 1, :ni]))[0][:mi]
    return want


@functools.lru_cache(maxsize=None)
def expected(name):
    """The case's expectation, computed once and shared by the paddings, the kernels and the group lengths."""
    import oracle as O
    _, _, _, _, m, npoints = _ALL[name]
    want = slice_rule(O, cloud(name), lengths_of(name), m, npoints)
    want.setflags(write=False)
    return want


def model_slices(kind):
    """[(n_c, slice)]: the first n_c points of the clouds of the device case of that kind, one cloud after the other."""
    xyz = cloud(MODEL_KINDS[kind])
    return [(nc, xyz[j % xyz.shape[0], :nc]) for j, nc in enumerate(MODEL_SIZES)]
