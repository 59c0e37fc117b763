"""The multi-radius ball query (pn2_query_ball_group_xyz_msg, csrc/ball_query_msg.hip) on edge clouds and at every launch
geometry: one case table, shared by the host-only test of what each case launches (test_ball_msg_plan.py, through
tf_grouping.query_ball_group_xyz_msg_plan) and by the GPU test that runs them (test_ball_msg_gpu.py).

INPUTS: name -> (b, n, m, builder); the builder returns (xyz (b,n,3), queries (b,m,3)) float32, the same arrays at every call.
Queries are points of the cloud, every third one moved by N(0, 0.7 r) -- r: the `jitter` radius of the input.
CASES: (name, input, scales [(radius, nsample), ...], options). Options: subtract / want_idx (the operator's arguments).
Several cases share an input, so the oracle's answer for an (input, radius, nsample) is computed once.

Which branch a cloud takes on the device (list, sweep, wide run) cannot be read back; the inputs are built so that the code's own
rules send them there, and each comment names the rule. Host rules (msg_plan): use_cells = n >= 1024 and b m nscales >= 8192;
geometry {512 threads, 80 KiB}, else {1024, 160 KiB}, else {512, 160 KiB}; qpb = ceil(b m / 256) (binned; / 512 swept) rounded
up to the workgroup's granule (2 queries per wave); lanes per query of a radius: the smallest of 8, 16, 32 that fits the LDS,
keeps waves * 64 / lpq <= qpb and is >= 16 beyond the bin radius. Device rules (bq_build_grid): a cloud leaves the list for the
sweep with more than max(128, n / 16) copies of point 0, with fewer than 64 cells, or with more than max(128, n / 16) points
in one cell; a radius leaves it when its block of visited cells covers half of the grid or more.

Sizes: b <= 4, m <= 704, n <= 8192, so a case costs the serial oracle at most 70 M distances per radius. Four kinds of case
have to exceed that, each as little as its rule allows:
  wide_run          m = 1024 (three clouds): the shape the wide-run case was specified at;
  thr_1024_8191     b m nscales = 8191 is prime: one cloud, one radius, m = 8191 (n = 1024: 8 M distances);
  denormal_binned   two radii are binned from b m >= 4096 on: m = 1024;
  lanes_8_16        8 (16) lanes per query need qpb >= 64 (32), that is b m >= 12289 (4097): b = 18 at n = 2048.
"""
import itertools

import numpy as np

from pointnet2_amd import synthetic as S

F = np.float32
CLS_MSG = [(0.1, 16), (0.2, 32), (0.4, 128)]            # pointnet2_cls_msg.py:27
THREE = [(0.1, 16), (0.2, 32), (0.4, 64)]


def queries(xyz, m, r, seed, base=None):
    """m points of the cloud per batch entry (of `base` when xyz itself holds non-finite points), every third one jittered"""
    rng = np.random.default_rng(seed)
    src = xyz if base is None else base
    b, n, _ = src.shape
    pick = rng.integers(0, n, size=(b, m))
    q = np.take_along_axis(src, pick[:, :, None].repeat(3, axis=2), axis=1).copy()
    q[:, ::3] += rng.normal(0, r * 0.7, size=q[:, ::3].shape).astype(F)
    return q


def _plain(gen, b, n, m, seed, r=0.2, scale=1.0):
    def build():
        xyz = (gen(b, n, seed) * F(scale)).astype(F)
        return xyz, queries(xyz, m, r, seed + 1)
    return (b, n, m, build)


def _cat(parts, m, seed, r=0.2):
    """one batch out of several generators' clouds: parts = [(gen, clouds, n, seed), ...]"""
    b, n = sum(p[1] for p in parts), parts[0][2]

    def build():
        xyz = np.concatenate([gen(k, nn, sd) for gen, k, nn, sd in parts], axis=0).astype(F)
        return xyz, queries(xyz, m, r, seed)
    return (b, n, m, build)


def crowded_not_at_point0(b, n, seed):
    """Half of every cloud copied onto ONE point that is not point 0 (the second half onto the last point): bq_build_grid's
    count of copies of point 0 sees one, the crowded-cell test after the counting sort sees n / 2 > max(128, n / 16)."""
    xyz = S.uniform_clouds(b, n, seed)
    xyz[:, n // 2:] = xyz[:, n - 1:n]
    return xyz


def planar_clouds(b, n, seed):
    xyz = S.uniform_clouds(b, n, seed)
    xyz[:, :, 2] = F(0.25)
    return xyz


def linear_clouds(b, n, seed):
    xyz = S.uniform_clouds(b, n, seed)
    xyz[:, :, 1] = F(-1.0)
    xyz[:, :, 2] = F(7.0)
    return xyz


def _mixed_giveup():
    def build():
        n = 4096
        xyz = np.concatenate([S.uniform_clouds(1, n, 410), S.dropout_clouds(1, n, 411), S.identical_clouds(1, n, 412),
                              crowded_not_at_point0(1, n, 413)], axis=0).astype(F)
        return xyz, queries(xyz, 704, 0.2, 414)
    return (4, 4096, 704, build)


# ---- case 5: edge inputs, b 4, n 3000, m 704 -- three radii are a binned launch (8448 >= 8192)
def _edge(kind, m=704):
    b, n = 4, 3000

    def build():
        base = S.uniform_clouds(b, n, 3)
        if kind == "nonfinite":                                  # points: never hit, cell 0; queries: the full-visit path, no hit
            xyz = base.copy()
            xyz[:, 5, 0] = np.nan
            xyz[:, 77, 1] = np.inf
            xyz[:, 300, 2] = -np.inf
            q = queries(xyz, m, 0.2, 500, base=base)
            q[:, 3, 1] = np.nan
            q[:, 9, 0] = np.inf
            q[:, 10, 2] = -np.inf
            return xyz, q
        if kind == "far":                                        # |q| > 4096 r: the query visits the whole list
            q = queries(base, m, 0.2, 501)
            q[:, ::4] *= F(1e6)
            q[:, 1::4] += F(1e3)
            return base, q
        if kind == "offset":                                     # every |q| > 4096 r for r <= 0.4: every query visits everything
            xyz = (base + F(4000.0)).astype(F)
            return xyz, queries(xyz, m, 0.2, 502)
        return base, queries(base, m, 0.2, 503)                  # "base": ordinary points under extreme radii
    return (b, n, m, build)


INPUTS = {
    # 1. n = 8192: only {512 threads, 160 KiB} holds the cloud beside eight waves' areas
    "cube_8192": _plain(S.uniform_clouds, 2, 8192, 512, 100),
    "sphere_8192": _plain(S.sphere_clouds, 2, 8192, 512, 102),
    "both_8192": _cat([(S.uniform_clouds, 2, 8192, 104), (S.sphere_clouds, 2, 8192, 105)], 704, 106),
    # 2. odd n, {1024, 160 KiB}, 22 parts of 32 with a last part of 28
    "cube_5000": _plain(S.uniform_clouds, 4, 5000, 700, 200),
    # 3. m = 690 = 43 x 16 + 2: the last workgroup of a cloud owns two queries, one wave's worth
    "sphere_2048": _plain(S.sphere_clouds, 4, 2048, 690, 300),
    # 4. binning gives up for some clouds of a binned launch
    "mixed_giveup": _mixed_giveup(),
    "duplicated": _plain(S.duplicated_clouds, 4, 4096, 704, 420),
    "lattice": _plain(S.lattice_clouds, 4, 4096, 704, 422),
    "planar": _plain(planar_clouds, 4, 4096, 704, 424),
    "linear": _plain(linear_clouds, 4, 4096, 704, 426),
    # 5. edge inputs
    "edge_nonfinite": _edge("nonfinite"),
    "edge_far": _edge("far"),
    "edge_offset": _edge("offset"),
    "edge_base": _edge("base"),
    "edge_base_1024": _edge("base", 1024),
    # 6. radius lists
    "sphere_4096": _plain(S.sphere_clouds, 4, 4096, 704, 600),
    # 7. extent 6: cells of 0.5 (extent / 12), a ball of 1.0 reaches 5 or 6 of 12 cells per axis
    "sphere_x3": _plain(S.sphere_clouds, 3, 4096, 1024, 700, scale=3.0),
    # 8. output forms: the binned shape is sphere_2048
    "small": _plain(S.sphere_clouds, 2, 600, 100, 800),
    # 9. use_cells threshold
    "thr_1023": _plain(S.sphere_clouds, 4, 1023, 512, 900),
    "thr_1024": _plain(S.sphere_clouds, 4, 1024, 512, 902),
    "thr_1024_8191": _plain(S.sphere_clouds, 1, 1024, 8191, 904),
    # 10. m below the workgroup's granule (16 queries): one part, one or four waves with work
    "m1": _plain(S.uniform_clouds, 3, 300, 1, 1000),
    "m7": _plain(S.uniform_clouds, 3, 1500, 7, 1002),
    # 11. qpb = 64: eight waves of eight queries
    "sphere_2048_b18": _plain(S.sphere_clouds, 18, 2048, 700, 1100),
}

FOUR = [(0.05, 8), (0.1, 16), (0.2, 32), (0.4, 64)]
PERMUTED = [(0.4, 128), (0.1, 16), (0.2, 32)]                   # every order of it is a case

CASES = [
    # 1. The third geometry. nsample 127 at n = 8192 needs 3104 bytes per wave (row buffers are padded to 16 bytes) of the
    # 3102 there are: refused like 128, the operator launches per radius -- same results asked. 126 is the largest that runs.
    ("g3_cube_127", "cube_8192", [(0.1, 16), (0.2, 32), (0.4, 127)], {}),
    ("g3_sphere_127", "sphere_8192", [(0.1, 16), (0.2, 32), (0.4, 127)], {}),
    ("g3_cube_126", "cube_8192", [(0.1, 16), (0.2, 32), (0.4, 126)], {}),
    ("g3_sphere_126", "sphere_8192", [(0.1, 16), (0.2, 32), (0.4, 126)], {}),
    ("g3_cube_two", "cube_8192", [(0.15, 8), (0.3, 64)], {}),
    ("g3_sphere_two", "sphere_8192", [(0.15, 8), (0.3, 64)], {}),
    # ... and binned (4 x 704 x 3 = 8448): the cube's 0.4 covers the grid and is swept behind the list passes, the sphere's stays
    ("g3_binned", "both_8192", [(0.1, 16), (0.2, 32), (0.4, 126)], {}),
    # 2.
    ("odd_n_5000", "cube_5000", CLS_MSG, {}),
    # 3.
    ("short_last_part", "sphere_2048", THREE, {}),
    # 4. cloud 0 stays on the list; 1: copies of point 0 (87 %); 2: copies of point 0 (all; zero extent: one cell);
    # 3: one crowded cell. Then whole batches of: duplicated points (binned: four copies per point crowd no cell), a lattice
    # (extent 0.625: 4 x 4 x 4 cells at 0.2, the least that are kept), a plane (5 x 5 x 1 cells < 64), a line (5 x 1 x 1).
    ("giveup_mixed", "mixed_giveup", THREE, {}),
    ("giveup_duplicated", "duplicated", THREE, {}),
    ("giveup_lattice", "lattice", THREE, {}),
    ("giveup_planar", "planar", THREE, {}),
    ("giveup_linear", "linear", THREE, {}),
    # 5.
    ("edge_nonfinite", "edge_nonfinite", THREE, {}),
    ("edge_far_queries", "edge_far", THREE, {}),
    ("edge_offset_cloud", "edge_offset", THREE, {}),
    # binned at 0.2: 1e-6 far below the cells; 1e30 (threshold +inf: every finite point hits) covers the grid and is swept
    ("edge_radii_tiny_huge", "edge_base", [(1e-6, 8), (0.2, 32), (1e30, 64)], {}),
    # a denormal bin radius: cells of extent / 12, 0.1 is a wide run (sy, sz = 2 or 3). Two radii at m = 704 are swept ...
    ("edge_radii_denormal", "edge_base", [(1e-40, 8), (0.1, 16)], {}),
    ("denormal_binned", "edge_base_1024", [(1e-40, 8), (0.1, 16)], {}),      # ... at m = 1024 binned
    # 6. (the six orders of PERMUTED follow below)
    ("radii_equal", "sphere_4096", [(0.2, 16), (0.2, 64)], {}),
    ("radii_one", "sphere_4096", [(0.2, 32)], {}),
    ("radii_four", "sphere_4096", FOUR, {}),
    ("radii_small_first", "sphere_4096", [(0.01, 4), (0.3, 32), (0.35, 48)], {}),
    # 7. (5 / 12)^3 of the grid: on the list, sy = sz = 4 or 5 -- wide runs over 5 or 6 slabs
    ("wide_run", "sphere_x3", [(0.1, 8), (0.2, 16), (1.0, 64)], {}),
    # 8.
    ("no_idx_binned", "sphere_2048", THREE, {"want_idx": False}),
    ("no_idx_swept", "small", THREE, {"want_idx": False}),
    ("no_subtract_binned", "sphere_2048", THREE, {"subtract": False}),
    ("no_subtract_swept", "small", THREE, {"subtract": False}),
    # 9. 4 x 512 x 4 = 8192: n = 1023 swept, n = 1024 binned; 1 x 8191 x 1: n = 1024 swept
    ("thr_n1023", "thr_1023", FOUR, {}),
    ("thr_n1024", "thr_1024", FOUR, {}),
    ("thr_8191", "thr_1024_8191", [(0.2, 32)], {}),
    # 10.
    ("m_1", "m1", THREE, {}),
    ("m_7", "m7", THREE, {}),
    # 11. 8 lanes per query at 0.1 (nsample 32 at 0.2 does not fit eight row buffers: 16), 16 beyond the bin radius
    ("lanes_8_16", "sphere_2048_b18", THREE, {}),
]
PERMUTATIONS = [("radii_perm_%d%d%d" % order, "sphere_4096", [PERMUTED[i] for i in order], {})
                for order in itertools.permutations(range(3))]
CASES += PERMUTATIONS
ASCENDING = "radii_perm_120"                                     # (0.1, 16), (0.2, 32), (0.4, 128)

# 8, at the C ABI: pts_cnt pointers null (tested apart: the operator always passes them)
NULL_CNT_INPUTS = ("sphere_2048", "small")

IDS = [c[0] for c in CASES]


def plan_of(case):
    """what the case launches (tf_grouping.query_ball_group_xyz_msg_plan)"""
    from pointnet2_amd import tf_grouping
    _, key, scales, _ = case
    b, n, m, _ = INPUTS[key]
    return tf_grouping.query_ball_group_xyz_msg_plan([s[0] for s in scales], [s[1] for s in scales], b, n, m)
