"""The ragged multi-radius ball query (pn2_query_ball_group_xyz_msg_ragged, csrc/ball_query_msg.hip): one case table for
test_ragged_msg_gpu.py. The inputs are those of ball_msg_cases.py (imported, not copied) with per-cloud lengths laid over them.

CASES: (name, input, scales [(radius, nsample), ...], lengths, options). Options: subtract / want_idx (the operator's arguments).
Each case is the smallest shape of ball_msg_cases.py that reaches its branch. The HOST decides from the padded n (msg_plan:
use_cells = n >= 1024 and b m nscales >= 8192, the geometry, lanes per query); on the DEVICE a cloud below 64 points is swept
without binning, a larger one bins its own n_c points, bq_build_grid's give-up rules (copies of point 0, fewer than 64 cells, a
crowded cell) and the half-of-the-grid rule then apply to that cloud's grid. Which branch a cloud took cannot be read back; the
lengths are chosen so that the code's own rules send the clouds there, and each comment names the rule.

Cost for the serial oracle: m sum(lengths) distances per radius, at most 704 x 20580 = 14.5 M (third_geometry) -- below the
70 M per radius that ball_msg_cases.py allows itself.
"""
import numpy as np

import ball_msg_cases as M

PADDINGS = ("nan", "adversarial")

G3 = [(0.1, 16), (0.2, 32), (0.4, 126)]
MIXED = [3000, 1500, 64, 63]

CASES = [
    # binned launch (4 x 704 x 3 = 8448, n = 3000): a full cloud; 1500 points: a cloud the single-radius dispatch would sweep
    # (its cell list starts at 2048 points), binned here; 64 / 63: the two sides of the n_c < 64 rule
    ("binned_mixed", "edge_base", M.THREE, MIXED, {}),
    # one- and two-point clouds (swept: the first hit pads every slot, empty balls give zero rows and pts_cnt 0); 129: the sweep
    # copy's pad crosses 128
    ("tiny_clouds", "edge_base", M.THREE, [3000, 1, 2, 129], {}),
    # {512 threads, 160 KiB}, binned: clouds 0, 1 cubes (0.4 covers the grid: swept behind the list passes), 2, 3 spheres
    # (cloud 2: 0.4 stays on the list); 8191 / 4097: two bitmap windows, one more point than one; 100: one window
    ("third_geometry", "both_8192", G3, [8192, 8191, 4097, 100], {}),
    # clouds that give up binning inside a binned ragged launch, shortened: 0 stays on the list; 1: copies of point 0; 2: one
    # point repeated (zero extent); 3: points 2048.. are copies of one point that is not point 0 -- 952 in one cell > 3000 / 16
    ("giveup_mixed", "mixed_giveup", M.THREE, [4096, 4000, 2500, 3000], {}),
    # swept launch (n = 600 < 1024)
    ("swept", "small", M.THREE, [600, 37], {}),
    # m below the workgroup's granule: one part, four waves with work
    ("m_7", "m7", M.THREE, [1500, 700, 5], {}),
    # odd n at {1024 threads, 160 KiB}; 2049 / 1023: around the dense use_cells threshold's powers of two
    ("odd_n_5000", "cube_5000", M.CLS_MSG, [5000, 4999, 2049, 1023], {}),
    # output forms, binned and swept
    ("no_idx_binned", "edge_base", M.THREE, MIXED, {"want_idx": False}),
    ("no_idx_swept", "small", M.THREE, [600, 37], {"want_idx": False}),
    ("no_subtract_binned", "edge_base", M.THREE, MIXED, {"subtract": False}),
    ("no_subtract_swept", "small", M.THREE, [600, 37], {"subtract": False}),
    # radius lists: one radius (swept: 4 x 704 x 1 < 8192), four, and an order with the largest radius first
    ("radii_one", "sphere_4096", [(0.2, 32)], [4096, 3000, 2000, 1000], {}),
    ("radii_four", "sphere_4096", M.FOUR, [4096, 3000, 2000, 1000], {}),
    ("radii_permuted", "sphere_4096", M.PERMUTED, [4096, 3000, 2000, 1000], {}),
    # the Python operator's fallback: no LDS geometry holds nsample 127 at n = 8192 (code -4) -- one ragged launch per radius
    ("fallback_127", "cube_8192", [(0.1, 16), (0.2, 32), (0.4, 127)], [8192, 5000], {}),
]
IDS = [c[0] for c in CASES]

# with every length equal to n the launch must give the dense launch's bits: one binned, one swept
FULL_LENGTH_CASES = [("edge_base", M.THREE), ("small", M.THREE)]
# pts_cnt missing at the C ABI, as a whole and per scale: one binned, one swept
NULL_CNT_CASES = [("edge_base", M.THREE, MIXED), ("small", M.THREE, [600, 37])]
# lengths the kernels clamp into 1..n for memory safety: (as given, as computed on)
BAD_LENGTHS = ("edge_base", M.THREE, [0, -3, 3007, 1500], [1, 1, 3000, 1500])
# capture and replay: captured at the first lengths, replayed at the second
CAPTURE = ("edge_base", M.THREE, MIXED, [700, 3000, 2999, 65])


def padded(xyz, q, lengths, padding):
    """xyz (b, n, 3) with the rows at or beyond lengths[c] replaced: NaN, or -- adversarial -- copies of the cloud's own queries:
    points at distance 0 of a query, inside every ball, that would enter the results if they were read."""
    out = xyz.copy()
    n, m = xyz.shape[1], q.shape[1]
    for c, nc in enumerate(lengths):
        if nc >= n:
            continue
        if padding == "nan":
            out[c, nc:] = np.nan
        else:
            out[c, nc:] = q[c, np.arange(n - nc) % m]
    return out
