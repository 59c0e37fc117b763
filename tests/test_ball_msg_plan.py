"""What the multi-radius ball query launches at the cases of ball_msg_cases.py -- asked of the launcher's own decision function
through pn2_query_ball_group_xyz_msg_plan (tf_grouping.query_ball_group_xyz_msg_plan): host logic, no device.

(a) the table reaches each of the three launch geometries, both values of use_cells, 8, 16 and 32 lanes per query, a cloud cut
    into parts with a short last one, and a qpb clipped to m; what single cases are there for is pinned case by case, so that
    shrinking one below a rule's threshold fails here and not silently on the GPU;
(b) the LDS arithmetic at n = 8192: a wave's area at 32 lanes per query is 2 nwin 512 + 4 roundup4(2 nsample) + 32 bytes, and
    {512 threads, 160 KiB} leaves (163840 - 16 n - 4 * 1732 - 1024) / 8 = 3102 of them: nsample 126 (3088) runs there, 127 and
    128 (3104) are refused -- the row buffers' padding to 16 bytes is what 127 does not survive (include/pn2ops.h documents the
    refusal from 127 on);
(c) the bin radius: a function of the SET of radii -- the second smallest of three or four, the smallest of one or two;
(d) the entry is exported and returns the launcher's argument errors."""
import ctypes
import itertools

import pytest

import ball_msg_cases as M
from pointnet2_amd import tf_grouping

G1, G2, G3 = (512, 80 * 1024), (1024, 160 * 1024), (512, 160 * 1024)


def _plans():
    return {c[0]: M.plan_of(c) for c in M.CASES}


def _geom(p):
    return (p["threads"], p["lds_cap"])


def _shape(name):
    case = M.CASES[M.IDS.index(name)]
    return M.INPUTS[case[1]][:3]


def test_the_table_stays_inside_the_envelope():
    assert len(set(M.IDS)) == len(M.IDS)
    big = {"wide_run", "thr_8191", "denormal_binned", "lanes_8_16"}          # see ball_msg_cases.py: Sizes
    for name, key, scales, _ in M.CASES:
        b, n, m, _ = M.INPUTS[key]
        assert n <= 8192 and 1 <= len(scales) <= 4 and all(r > 0 and ns > 0 for r, ns in scales), name
        if name not in big:
            assert b <= 4 and m <= 704, name
        assert b * m * n * len(scales) <= 2.2e8, name             # distances the serial oracle evaluates at most


def test_table_reaches_every_geometry_and_rule():
    plans = _plans()
    launched = {k: p for k, p in plans.items() if p["rc"] == 0}
    refused = sorted(k for k, p in plans.items() if p["rc"] != 0)
    assert refused == ["g3_cube_127", "g3_sphere_127"]           # (b): the operator's per-radius path, same results asked
    assert all(plans[k]["rc"] == -4 and plans[k]["threads"] == 0 for k in refused)
    for k, p in launched.items():
        assert _geom(p) in (G1, G2, G3), k
        assert 0 < p["lds_bytes"] <= p["lds_cap"] <= 160 * 1024, (k, p)
        assert all(l in (8, 16, 32) for l in p["lpq"]), (k, p)
        b, n, m = _shape(k)
        gran = p["threads"] // 64 * 2
        assert p["qpb"] % gran == 0 and p["parts"] == -(-m // p["qpb"]), (k, p)
    assert {_geom(p) for p in launched.values()} == {G1, G2, G3}
    assert {p["use_cells"] for p in launched.values()} == {0, 1}
    assert {l for p in launched.values() for l in p["lpq"]} == {8, 16, 32}
    short = [k for k, p in launched.items() if p["parts"] > 1 and _shape(k)[2] % p["qpb"] != 0]
    assert "short_last_part" in short and "odd_n_5000" in short and "lanes_8_16" in short
    clipped = [k for k, p in launched.items() if p["qpb"] > _shape(k)[2]]          # m below the granule: one part, qpb > m
    assert {"m_1", "m_7"} <= set(clipped) and all(launched[k]["parts"] == 1 for k in clipped)


def test_each_case_launches_what_it_is_there_for():
    plans = _plans()

    def is_(name, geom, use_cells, **more):
        p = plans[name]
        assert p["rc"] == 0 and _geom(p) == geom and p["use_cells"] == use_cells, (name, p)
        for key, want in more.items():
            assert p[key] == want, (name, key, p)

    for name in ("g3_cube_126", "g3_sphere_126", "g3_cube_two", "g3_sphere_two"):
        is_(name, G3, 0, qpb=16, parts=32)
    is_("g3_binned", G3, 1, qpb=16, parts=44, lpq=[32, 32, 32])
    is_("odd_n_5000", G2, 1, qpb=32, parts=22, lpq=[32, 32, 32])                   # 700 = 21 x 32 + 28
    is_("short_last_part", G1, 1, qpb=16, parts=44)                                # 690 = 43 x 16 + 2
    for name in ("giveup_mixed", "giveup_duplicated", "giveup_lattice", "giveup_planar", "giveup_linear", "edge_nonfinite",
                 "edge_far_queries", "edge_offset_cloud", "edge_radii_tiny_huge", "denormal_binned", "radii_four",
                 "radii_small_first", "wide_run", "no_idx_binned", "no_subtract_binned", "thr_n1024", "lanes_8_16") \
            + tuple(c[0] for c in M.PERMUTATIONS):
        assert plans[name]["use_cells"] == 1 and plans[name]["rc"] == 0, name
    for name in ("edge_radii_denormal", "radii_equal", "radii_one", "no_idx_swept", "no_subtract_swept", "thr_n1023", "thr_8191",
                 "m_1", "m_7"):
        assert plans[name]["use_cells"] == 0 and plans[name]["rc"] == 0, name
    is_("lanes_8_16", G1, 1, qpb=64, parts=11, lpq=[8, 16, 16])                    # 700 = 10 x 64 + 60
    is_("m_1", G1, 0, qpb=16, parts=1)
    is_("m_7", G1, 0, qpb=16, parts=1)
    # a permuted radius list keeps each radius' lanes and the launch
    asc = plans[M.ASCENDING]
    for name, _, scales, _ in M.PERMUTATIONS:
        p = plans[name]
        assert {k: p[k] for k in p if k != "lpq"} == {k: asc[k] for k in asc if k != "lpq"}, name
        assert dict(zip(scales, p["lpq"])) == dict(zip(M.CASES[M.IDS.index(M.ASCENDING)][2], asc["lpq"])), name


def test_use_cells_threshold_from_both_sides():
    plan = tf_grouping.query_ball_group_xyz_msg_plan
    four_r, four_ns = [s[0] for s in M.FOUR], [s[1] for s in M.FOUR]
    assert plan(four_r, four_ns, 4, 1024, 512)["use_cells"] == 1                    # n = 1024, b m nscales = 8192
    assert plan(four_r, four_ns, 4, 1023, 512)["use_cells"] == 0                    # n one short
    assert plan([0.2], [32], 1, 1024, 8191)["use_cells"] == 0                       # b m nscales one short
    assert plan([0.2], [32], 1, 1024, 8192)["use_cells"] == 1
    assert plan(four_r[:3], four_ns[:3], 4, 1024, 512)["use_cells"] == 0            # 6144


def test_lds_at_8192_points():
    plan = tf_grouping.query_ball_group_xyz_msg_plan
    radii = [0.1, 0.2, 0.4]
    budget = (160 * 1024 - 16 * 8192 - 4 * 1732 - 1024) // 8
    assert budget == 3102

    def wave(ns):                                                # bq_cells_wave_bytes(8192, ns, 32)
        return 2 * 2 * 512 + 4 * ((2 * ns + 3) // 4 * 4) + 2 * 16

    assert wave(126) == 3088 and wave(127) == wave(128) == 3104
    for b, m in ((2, 512), (4, 704)):
        p = plan(radii, [16, 32, 126], b, 8192, m)
        assert p["rc"] == 0 and _geom(p) == G3 and p["lpq"] == [32, 32, 32], p
        assert p["lds_bytes"] == 16 * 8192 + 4 * 1732 + 8 * wave(126) + 1024 <= 160 * 1024
        for ns in (127, 128):
            p = plan(radii, [16, 32, ns], b, 8192, m)
            assert p["rc"] == -4 and p["threads"] == 0 and p["lds_bytes"] == 0, (ns, p)
    for ns in range(1, 127):                                     # every smaller nsample runs, never above 160 KiB
        p = plan(radii, [16, 32, ns], 2, 8192, 512)
        assert p["rc"] == 0 and _geom(p) == G3 and p["lds_bytes"] <= 160 * 1024, (ns, p)
    assert plan(radii, [16, 32, 64], 2, 8193, 512)["rc"] == -4                      # beyond the cell list's envelope
    # the requested LDS over a sweep of shapes: never above the chosen geometry's cap
    for n in (1, 64, 1000, 1024, 2048, 3000, 4096, 4097, 5000, 6000, 8000, 8192):
        for ns in (1, 8, 16, 33, 64, 100, 128, 200, 256):
            for b, m in ((1, 1), (4, 704), (32, 1024)):
                p = plan(radii, [8, 16, ns], b, n, m)
                assert p["rc"] in (0, -4), p
                if p["rc"] == 0:
                    assert 0 < p["lds_bytes"] <= p["lds_cap"] and _geom(p) in (G1, G2, G3), (n, ns, b, m, p)


def test_bin_radius_is_a_function_of_the_set_of_radii():
    plan = tf_grouping.query_ball_group_xyz_msg_plan
    f32 = lambda v: ctypes.c_float(v).value
    lists = {
        1: [(0.2, 32)],
        2: [(0.3, 64), (0.15, 8)],
        3: M.PERMUTED,
        4: M.FOUR,
    }
    for k, scales in lists.items():
        want = f32(sorted(s[0] for s in scales)[1 if k >= 3 else 0])
        for order in itertools.permutations(scales):
            p = plan([s[0] for s in order], [s[1] for s in order], 4, 4096, 704)
            assert p["rc"] == 0 and p["bin_radius"] == want, (order, p)
    # equal radii: the second smallest of (0.2, 0.2, 0.4) is 0.2; of (0.1, 0.4, 0.4) 0.4
    assert plan([0.2, 0.4, 0.2], [8, 8, 8], 4, 4096, 704)["bin_radius"] == f32(0.2)
    assert plan([0.4, 0.1, 0.4], [8, 8, 8], 4, 4096, 704)["bin_radius"] == f32(0.4)
    assert plan([0.2, 0.2], [16, 64], 4, 4096, 704)["bin_radius"] == f32(0.2)
    # reported for an empty call and for a refused one too
    assert plan([0.3, 0.1, 0.2], [8, 8, 8], 0, 4096, 704) == dict(rc=0, threads=0, lds_cap=0, lds_bytes=0, use_cells=0, qpb=0,
                                                                  parts=0, lpq=[0, 0, 0], bin_radius=f32(0.2))
    assert plan([0.3, 0.1, 0.2], [8, 8, 128], 2, 8192, 512)["bin_radius"] == f32(0.2)


def test_plan_entry_is_exported_and_validates_like_the_launcher():
    from pointnet2_amd import _C
    assert "pn2_query_ball_group_xyz_msg_plan" in _C.EXPORTED and hasattr(ctypes.CDLL(_C.LIB_PATH), "pn2_query_ball_group_xyz_msg_plan")
    lib = _C.lib()
    one = ctypes.c_void_p(16)                                    # any non-null pointer: never dereferenced
    out = (ctypes.c_void_p * 2)(16, 16)
    radii = (ctypes.c_float * 2)(0.1, 0.2)
    nss = (ctypes.c_int * 2)(4, 4)
    info = (ctypes.c_int * 10)(*([-7] * 10))

    def both(b, n, m, k, r, s):
        rc = lib.pn2_query_ball_group_xyz_msg_plan(b, n, m, k, r, s, info, None)
        assert rc == lib.pn2_query_ball_group_xyz_msg(b, n, m, k, r, s, one, one, 1, out, None, out, None)
        return rc

    assert both(1, 8, 4, 0, radii, nss) == -3                    # no scale
    assert both(1, 8, 4, 5, radii, nss) == -3                    # > 4 scales
    assert both(1, 8, 4, 2, None, nss) == -3 and both(1, 8, 4, 2, radii, None) == -3
    assert both(-1, 8, 4, 2, radii, nss) == -2 and both(1, 0, 4, 2, radii, nss) == -2 and both(1, 8, -1, 2, radii, nss) == -2
    nss[1] = 0
    assert both(1, 8, 4, 2, radii, nss) == -3                    # nsample 0
    nss[1] = 4
    radii[0] = 0.0
    assert both(1, 8, 4, 2, radii, nss) == -3                    # radius 0
    radii[0] = float("nan")
    assert both(1, 8, 4, 2, radii, nss) == -3
    assert list(info) == [-7] * 10                               # nothing is written about such arguments
    radii[0] = 0.1
    assert both(1, 8200, 4, 2, radii, nss) == -4                 # n beyond the envelope
    assert both(1 << 20, 4096, 1 << 20, 2, radii, nss) == -4     # b m nsample beyond 2^40
    nss[1] = 128
    assert both(2, 8192, 512, 2, radii, nss) == -4               # no geometry
    assert both(0, 8, 4, 2, radii, nss) == 0 and both(1, 8, 0, 2, radii, nss) == 0   # empty: nothing to launch
    assert list(info)[:6] == [0] * 6
    # null info / bin_radius are allowed
    assert lib.pn2_query_ball_group_xyz_msg_plan(1, 8, 4, 2, radii, nss, None, None) == 0
    with pytest.raises(ValueError, match="PN2_E_ARG"):
        tf_grouping.query_ball_group_xyz_msg_plan([0.1, -1.0], [4, 4], 1, 8, 4)
