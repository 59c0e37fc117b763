"""The farthest-point-sampling case table shared by tests/golden/make_golden.py (which records the literal emulator's indices
into tests/golden/fps_literal.npz), tests/test_oracle.py (oracle restatement == literal emulator, CPU), test_fps_golden in
tests/test_parity_gpu.py (product == literal emulator) and tests/test_ref_gpu_crosscheck.py (the reference's own kernel ==
oracle == every product tier). One table, so that every input the product's tiers are checked on is also an input the
literal emulator and the reference kernel have seen.

A case is (name, make, npoint, stores_xyz). make() -> (b, n, 3) float32. The six cases of the first fixture keep their
coordinates in the npz; the others store indices only, the cloud is regenerated from pointnet2_amd/synthetic.py and a CRC32
of its bytes (crc32_of) is stored beside the indices, so that a silent change of a generator fails loudly.

The comment of each case says which tier PN2_FPS_AUTO takes for it (include/pn2ops.h): rank slots = 512 * ceil(n / 512);
batched at 513..8192 slots with npoint >= 256, pruned at 4097..8192 slots with 128 <= npoint < 256, the register (full)
tier otherwise up to 16384 points, the global-memory kernel beyond."""
import zlib

import numpy as np

from pointnet2_amd import synthetic as S


def crc32_of(xyz):
    a = np.ascontiguousarray(xyz, dtype=np.float32)
    return np.uint32(zlib.crc32(a.tobytes()) & 0xffffffff)


def islands(c, shift):
    """The second half of every cloud moved ~shift away along x: from 1.85e19 on, the squared distance between the halves
    overflows to inf, which the reference's min() against the 1e38 start value turns into 1e38 (tf_sampling_g.cu:118,143)."""
    c = np.array(c, dtype=np.float32)
    c[:, c.shape[1] // 2:, 0] += np.float32(shift)
    return c


def poke(c, points):
    """Every cloud with coordinate `axis` of point k set to `value`, for (k, axis, value) in points."""
    c = np.array(c, dtype=np.float32)
    for k, axis, value in points:
        c[:, k, axis] = np.float32(value)
    return c


def denormal_z(c):
    """z of point k = float32((k % 701) * 1e-42): 701 distinct denormals, an extent of 7e-40 whose reciprocal overflows fp32 (the
    bin scale of a grouping prologue is cells / extent)."""
    c = np.array(c, dtype=np.float32)
    c[:, :, 2] = ((np.arange(c.shape[1]) % 701) * 1e-42).astype(np.float32)
    return c


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


NAN, INF = float("nan"), float("inf")
X, Y, Z = 0, 1, 2


FPS_LITERAL_CASES = [
    # ---- the first fixture's six (coordinates stored)
    ("d1", lambda: S.sphere_clouds(2, 1024, 31), 256, True),
    ("dup", lambda: S.duplicated_clouds(2, 700, 32), 300, True),
    ("drop", lambda: S.dropout_clouds(2, 1024, 33), 200, True),
    ("same", lambda: S.identical_clouds(1, 600, 34), 40, True),
    ("lattice", lambda: S.lattice_clouds(2, 1500, 35), 400, True),
    ("small", lambda: S.uniform_clouds(2, 37, 36), 37, True),
    # ---- sizes at the tier boundaries, npoint >= 256: the batched tier
    ("n513", lambda: S.sphere_clouds(2, 513, 901), 260, False),                 # 1024 slots, one real point in the second rank
    ("n2049", lambda: S.sphere_clouds(2, 2049, 902), 300, False),               # 2560 slots
    ("n4096", lambda: S.uniform_clouds(2, 4096, 903), 512, False),
    ("n8192", lambda: S.uniform_clouds(2, 8192, 904), 1024, False),             # sem_seg SA1
    # ---- 4097..8192 slots, 128 <= npoint < 256: the pruned tier
    ("pruned8192", lambda: S.sphere_clouds(2, 8192, 905), 200, False),
    ("pruned5000", lambda: S.uniform_clouds(2, 5000, 906), 128, False),
    # ---- the register tier without LDS coordinates, and the global-memory kernel
    ("n12000", lambda: S.uniform_clouds(2, 12000, 907), 64, False),
    ("n20000", lambda: S.uniform_clouds(2, 20000, 908), 48, False),
    # ---- exact ties everywhere
    ("lattice4096", lambda: S.lattice_clouds(2, 4096, 909), 900, False),        # 216 distinct points: all distances 0 after them
    ("lattice6000", lambda: S.lattice_clouds(2, 6000, 910), 600, False),
    ("dup8192", lambda: S.duplicated_clouds(2, 8192, 911), 700, False),
    ("quant4096", lambda: S.quantized_clouds(2, 4096, 912), 1024, False),
    ("quant16_8192", lambda: S.quantized_clouds(2, 8192, 913, 1.0 / 16), 512, False),
    ("drop4096", lambda: S.dropout_clouds(2, 4096, 914), 600, False),           # 87 % of the cloud on one spot
    ("same3000", lambda: S.identical_clouds(2, 3000, 915), 260, False),
    # ---- degenerate boxes
    ("flat4096", lambda: _f32(S.sphere_clouds(2, 4096, 916) * np.array([1.0, 1.0, 0.0], np.float32)), 512, False),
    ("line4096", lambda: _f32(S.sphere_clouds(2, 4096, 917) * np.array([1.0, 0.0, 0.0], np.float32)), 300, False),
    # ---- the ends of the fp32 range
    ("far_offset", lambda: _f32(S.sphere_clouds(2, 4096, 918) * np.float32(1e-3) + np.float32(100.0)), 400, False),
    ("tiny_scale", lambda: _f32(S.sphere_clouds(2, 4096, 919) * np.float32(1e-18)), 300, False),    # squares are denormals
    ("islands_3e19", lambda: islands(S.sphere_clouds(2, 4096, 920), 3e19), 300, False),
    ("islands_2p5e19_8192", lambda: islands(S.uniform_clouds(2, 8192, 921), 2.5e19), 200, False),   # pruned tier
    # ---- more samples than points, every point sampled
    ("m_gt_n_2500", lambda: S.duplicated_clouds(2, 2500, 922), 2600, False),
    ("n37_all", lambda: S.uniform_clouds(2, 37, 923), 37, False),
    # ---- the metric shape, B = 32
    ("metric32", lambda: S.sphere_clouds(32, 4096, 924), 1024, False),
    # ---- non-finite coordinates inside the cloud. Such a point keeps its start distance 1e38 for ever (its distance to anything,
    # itself included, is NaN or inf, and min() keeps the other operand): round 1 picks the non-finite point with the smallest
    # (k mod 512, k), every later round picks it again, and no running distance changes.
    ("nan_one_4096", lambda: poke(S.uniform_clouds(2, 4096, 1501), [(700, Y, NAN)]), 512, False),               # batched
    ("nonfinite_ties_4096", lambda: poke(S.sphere_clouds(2, 4096, 1502),                 # batched; 518 and 1030 are both 6 mod 512
                                         [(700, X, NAN), (1030, Z, INF), (3000, Y, -INF), (518, X, INF)]), 300, False),
    ("nan_first_2049", lambda: poke(S.sphere_clouds(2, 2049, 1503), [(0, X, NAN)]), 300, False),                # batched; all 0
    ("nonfinite_8192_pruned", lambda: poke(S.uniform_clouds(2, 8192, 1504), [(5000, X, INF), (4100, Y, NAN)]), 200, False),  # pruned
    ("nan_12000", lambda: poke(S.uniform_clouds(2, 12000, 1505), [(11999, Z, NAN)]), 64, False),                # register
    ("nonfinite_20000", lambda: poke(S.uniform_clouds(2, 20000, 1506), [(16400, X, -INF), (19999, Y, NAN)]), 48, False),  # global
    ("inf_small37", lambda: poke(S.uniform_clouds(2, 37, 1507), [(36, X, INF)]), 37, False),                    # register
    ("quarter_nan_4096", lambda: poke(S.uniform_clouds(2, 4096, 1508), [(k, X, NAN) for k in range(1, 4096, 4)]), 400, False),  # batched
    # ---- an axis whose extent is a denormal: the bin scale of the grouping prologues overflows
    ("denormal_extent_4096", lambda: denormal_z(S.uniform_clouds(2, 4096, 1509)), 512, False),                  # batched
    ("denormal_extent_8192", lambda: denormal_z(S.uniform_clouds(2, 8192, 1510)), 200, False),                  # pruned
]

FPS_LITERAL_NAMES = [c[0] for c in FPS_LITERAL_CASES]


def load_case(g, name):
    """-> (xyz, literal indices) of a case from the loaded fps_literal.npz; checks the regenerated input's CRC32."""
    _, make, m, stores_xyz = FPS_LITERAL_CASES[FPS_LITERAL_NAMES.index(name)]
    want = g[name + "_idx"]
    xyz = g[name + "_xyz"] if stores_xyz else _f32(make())
    if not stores_xyz:
        assert int(g[name + "_crc"]) == int(crc32_of(xyz)), \
            "%s: synthetic.py no longer generates the cloud fps_literal.npz was recorded on" % name
    assert want.shape == (xyz.shape[0], m) and want.dtype == np.int32, name
    return xyz, want
