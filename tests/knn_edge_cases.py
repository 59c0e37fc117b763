"""kNN (pn2_knn_point / pn2_knn_point_ragged) and the selection sort (pn2_selection_sort), csrc/topk.hip, on edge rows: one case
table, shared by the host-only model of where each case goes (test_knn_replay_model.py) and by the GPU test that runs them
(test_knn_edge_gpu.py).

INPUTS: name -> (b, n, m, builder); the builder returns (xyz (b,n,3), queries (b,m,3)) float32, the same arrays at every call.
Unless an input fixes its queries, they are points of the cloud with every other one moved by N(0, 0.05).
CASES: (id, input, k). RAGGED: name -> (n, lengths, m, builder), run at RAGGED_K. No input holds a NaN.

Which path a row takes on the device cannot be read back; the inputs are built so that the kernel's own rules send them there,
and each comment names the rule. The rules of knn_wave_body (rounds = min(k, n)):
  tau     rounds <= 40: the rounds-th smallest of the 64 lanes' minima (lane l owns slots l, l + 64, ...; a lane without a
          slot holds the key 0xffffffff); beyond: key(v_k) | 0xffff, from two 256-bin histograms (key bits 31..24, 23..16).
  C       the slots whose key is <= tau. |C| <= kKnnCap = 1024: the swap rounds are replayed on C, keys read as fp64.
          |C| > 1024: the literal rounds on the row.
  LDS     8 n + 13312 bytes; above 64 KiB (n >= 6529) the launch needs the dynamic-LDS attribute.
test_knn_replay_model.py evaluates these rules on every row of the table and asserts the side of the cap named here.

Sizes: b <= 2, and m <= 16 where n > 4096; the serial oracle costs b m n min(k, n) comparisons, at most 15 M per case.
"""
import numpy as np

from pointnet2_amd import synthetic as S

F = np.float32
CAP = 1024                                                       # kKnnCap
ENVELOPE = 14336                                                 # pn2_knn_point: n beyond it is PN2_E_TOO_LARGE


def queries(xyz, m, seed):
    """m points of the cloud per batch entry, every other one jittered (test_parity_gpu.py::test_knn_point_native_ties_and_shapes)"""
    rng = np.random.default_rng(seed)
    b, n, _ = xyz.shape
    pick = rng.integers(0, n, size=(b, m))
    q = np.take_along_axis(xyz, pick[:, :, None].repeat(3, axis=2), axis=1).copy()
    q[:, ::2] += rng.normal(0, 0.05, size=q[:, ::2].shape).astype(F)
    return q.astype(F)


def _plain(gens, n, m, seed):
    """cloud i from gens[i]"""
    def build():
        xyz = np.concatenate([g(1, n, seed + i) for i, g in enumerate(gens)], axis=0).astype(F)
        return xyz, queries(xyz, m, seed + 50)
    return (len(gens), n, m, build)


DUP_POINT = np.array([0.5, 0.25, 0.75], dtype=F)


def dup_cloud(n, copies, seed, scattered):
    """`copies` points equal DUP_POINT (the first ones, or -- scattered -- at random slots: then every round of the replay swaps
    and hands a slot over), the rest uniform in [2, 3)^3: from DUP_POINT exactly `copies` distances are 0 and none is tiny."""
    rng = np.random.default_rng(seed)
    xyz = (rng.random((n, 3), dtype=F) + F(2.0)).astype(F)
    at = np.sort(rng.permutation(n)[:copies]) if scattered else np.arange(copies)
    xyz[at] = DUP_POINT
    return xyz


def _dup(copies):
    def build():
        xyz = np.stack([dup_cloud(2048, copies, 100 + copies, False), dup_cloud(2048, copies, 200 + copies, True)])
        return xyz, np.broadcast_to(DUP_POINT, (2, 2, 3)).copy()
    return (2, 2048, 2, build)


def _shell(n):
    """unit directions times 1 +- 1e-6 around the query: squared distances 1 +- 2e-6, some thirty fp32 values on either side of
    1.0, where the key changes its second byte (0xbf7fxxxx | 0xbf80xxxx)"""
    def build():
        rng = np.random.default_rng(300 + n)
        q = np.array([[0.25, -0.5, 0.125]], dtype=np.float64)
        v = rng.standard_normal((n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v *= 1.0 + rng.uniform(-1e-6, 1e-6, size=(n, 1))
        return (v + q).astype(F)[None], q.astype(F)[None]
    return (1, n, 1, build)


def _ladder():
    def build():
        x = np.zeros((2, 60, 3), dtype=F)
        x[0, :, 0] = np.ldexp(F(1.0), -np.arange(60))            # 2^-e: the nearest point is the last
        x[1, :, 0] = x[0, np.random.default_rng(400).permutation(60), 0]
        return x, np.zeros((2, 1, 3), dtype=F)
    return (2, 60, 1, build)


def _tiny(n):
    def build():
        xyz = S.lattice_clouds(2, n, 500 + n)
        return xyz, queries(xyz, 4, 550 + n)
    return (2, n, 4, build)


def _inf_block():
    def build():
        xyz = S.uniform_clouds(1, 300, 600)
        xyz[0, 100:250, 0] = F(3e19)                             # (3e19)^2 overflows fp32
        return xyz, np.array([[[0, 0, 0], [0.5, 0.5, 0.5]]], dtype=F)
    return (1, 300, 2, build)


def _denormal():
    def build():
        rng = np.random.default_rng(700)
        xyz = (S.lattice_clouds(1, 500, 701) * F(1e-20)).astype(F)
        q0, q1 = xyz[0, 7].copy(), xyz[0, 11].copy()
        assert not np.array_equal(q0, q1)
        xyz[0, np.sort(rng.permutation(500)[:40])] = q0         # exact zeros beside distances around 1e-40
        return xyz, np.stack([q0, q1])[None]
    return (1, 500, 2, build)


INPUTS = {
    # dup_*: every lane owns a copy, so all 64 lane minima are 0; v_k = 0 and key(0) | 0xffff admits denormals only: |C| is
    # the number of copies on both tau paths. 1024: the replay on a full candidate table; 1025: the literal rounds.
    "dup_1024": _dup(1024),
    "dup_1025": _dup(1025),
    # shell_*: at k = 64 tau = 0xbf7fffff takes the half of the shell below 1.0: ~450 of 900 (replay), ~1500 of 3000 (the
    # literal rounds, reached from distinct values). At k = 16 the lane minima keep |C| at a few dozen.
    "shell_900": _shell(900),
    "shell_3000": _shell(3000),
    # ladder: exact distances 2^-2e, e = 0..59, one per first-level bin; n < 64 on both tau paths and k = n
    "ladder": _ladder(),
    # tiny_*: lanes without a slot in the rank vote (n < 64), the histograms over fewer elements than lanes, lattice ties
    **{"tiny_%d" % n: _tiny(n) for n in (1, 2, 41, 63, 64, 65)},
    # big_k: |C| >= k > 1024, the literal rounds for more than 1024 rounds
    "big_k": _plain([S.uniform_clouds], 1500, 3, 800),
    # inf_block: 150 distances are +Inf (key 0xff800000, tied among themselves), 150 finite: k = 160, 200 end inside the block
    # (tau = 0xff80ffff: every slot is a candidate), 300 = n goes past it, 32 stays before it
    "inf_block": _inf_block(),
    # denormal: value bits below 0x00100000 -- the fp64 keys of the replay are denormal doubles -- and every element in the
    # first-level bin 0x80
    "denormal": _denormal(),
    # lds_*: 8 n + 13312 = 78,848 and 128,000 bytes (the envelope's edge); cloud 1 is full of ties
    "lds_mid": _plain([S.sphere_clouds, S.duplicated_clouds], 8192, 8, 900),
    "lds_max": _plain([S.sphere_clouds, S.duplicated_clouds], ENVELOPE, 8, 910),
    # switch: rounds = 40 | 41 on ordinary data
    "switch": _plain([S.uniform_clouds, S.uniform_clouds], 4096, 16, 920),
}

_K = {
    "dup_1024": (8, 40, 41, 64), "dup_1025": (8, 40, 41, 64),
    "shell_900": (16, 64), "shell_3000": (16, 64),
    "ladder": (1, 30, 40, 41, 60),
    **{"tiny_%d" % n: tuple(k for k in sorted({1, 2, 40, 41, n}) if k <= n) for n in (1, 2, 41, 63, 64, 65)},
    "big_k": (1025, 1100, 1500),
    "inf_block": (32, 160, 200, 300),
    "denormal": (16, 64, 128),
    "lds_mid": (16, 64), "lds_max": (16, 64),
    "switch": (39, 40, 41, 42),
}
CASES = [("%s-k%d" % (name, k), name, k) for name in INPUTS for k in _K[name]]
IDS = [c[0] for c in CASES]

# ---- the side of the cap each case is there for (asserted on every row by test_knn_replay_model.py)
EXACTLY = {"dup_1024": 1024, "dup_1025": 1025}                   # |C| on every row, at every k


def above_cap(name, k):
    """True: |C| > CAP on every row (the literal rounds); False: |C| <= CAP on every row (the replay)"""
    return name == "dup_1025" or name == "big_k" or (name == "shell_3000" and k == 64)


# ---- ragged twin: (padded n, lengths, m, builder -> (xyz (b,n,3), q (b,m,3))); rows at or beyond a length are placeholders,
# replaced by the test's paddings
def _rag_max():
    def build():
        xyz = S.sphere_clouds(2, ENVELOPE, 1000)
        q = queries(xyz, 8, 1001)
        q[1] = queries(xyz[1:, :63], 8, 1002)[0]
        return xyz, q
    return (ENVELOPE, [ENVELOPE, 63], 8, build)


def _rag_dup():
    """cloud 0 is dup_1024 (1024 copies of 2048: the replay on a full table), cloud 1 dup_1025 at its own length (1025 copies of
    1025: the literal rounds), cloud 2 one point. Query 0 is DUP_POINT, query 1 a jittered point of the slice."""
    def build():
        xyz = np.zeros((3, 2048, 3), dtype=F)
        xyz[0] = dup_cloud(2048, 1024, 1100, True)
        xyz[1, :1025] = dup_cloud(1025, 1025, 1101, False)
        xyz[2, 0] = (0.125, 0.5, -0.25)
        q = np.empty((3, 2, 3), dtype=F)
        q[:, 0] = DUP_POINT
        for i, ni in enumerate((2048, 1025, 1)):
            q[i, 1] = queries(xyz[i:i + 1, :ni], 1, 1110 + i)[0, 0]
        return xyz, q
    return (2048, [2048, 1025, 1], 2, build)


RAGGED = {"rag_max": _rag_max(), "rag_dup": _rag_dup()}
RAGGED_K = (8, 41, 64)                                           # 64 > 63 and every k > 1: the row repeats entry 0

# ---- the matrix path of tf_grouping.knn_point (c != 3 or n > ENVELOPE): (c, n, m, k)
MATRIX = {"c2": (2, 200, 9, 7), "c5": (5, 200, 9, 7), "c3_past_envelope": (3, ENVELOPE + 1, 4, 16)}


def matrix_input(name):
    """lattice coordinates (ties) for c = 2, 5; an ordinary cloud one point past the envelope for c = 3"""
    c, n, m, _ = MATRIX[name]
    if c == 3:
        xyz = S.sphere_clouds(1, n, 1200)
        return xyz, queries(xyz, m, 1201)
    rng = np.random.default_rng(1210 + c)
    xyz = (rng.integers(0, 6, size=(2, n, c)).astype(F) * F(0.125)).astype(F)
    q = xyz[:, rng.integers(0, n, size=m)].copy()
    q[:, ::2] += (rng.integers(-1, 2, size=q[:, ::2].shape).astype(F) * F(0.125))      # still on the lattice
    return xyz, q.astype(F)


def dist_matrix(xyz, q):
    """(b, m, n) fp32: the c squares summed left to right, every operation rounded to fp32 -- for c = 3 the
    ((dx dx + dy dy) + dz dz) of knn_point's definition"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        d = None
        for ch in range(xyz.shape[2]):
            diff = (xyz[:, None, :, ch] - q[:, :, None, ch]).astype(F)
            sq = (diff * diff).astype(F)
            d = sq if d is None else (d + sq).astype(F)
    return d


# ---- selection sort
SORT_LONG = [(1, 3, 8193, 33), (1, 2, 16384, 64), (1, 2, 16384, 2000), (1, 2, 16385, 33)]     # (b, m, n, k)
SORT_MAX_LDS_N = 16384                                           # kSortMaxLdsN: longer rows take the serial kernel
POS_NAN, NEG_NAN = 0x7fc00000, 0xffc00000
NAN_N, NAN_K = (100, 16400), 10
NAN_ROWS = ["control"] + ["%s_%s" % (where, sign) for where in ("slot0", "slot3", "tail", "all") for sign in ("pos", "neg")]


def quantised(shape, rng):
    """many exact ties, some negatives (test_parity_gpu.py::test_selection_sort_golden_and_random)"""
    return (np.round(rng.random(shape, dtype=F) * 50) / 50 - F(0.3)).astype(F)


def sort_long_input(b, m, n, k):
    """quantised ties; row 0 starts (0, -0, 0); the last row holds +-Inf, denormals of both signs and +-0, before and beyond k"""
    rng = np.random.default_rng(1300 + n + k)
    dist = quantised((b, m, n), rng)
    dist[0, 0, :3] = [0.0, -0.0, 0.0]
    special = np.array([np.inf, -np.inf, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 0.0, -0.0], dtype=F)
    row = dist[b - 1, m - 1]
    at = rng.permutation(n)[:64]
    row[at] = np.tile(special, 8)
    row[[1, 2, 5, 6]] = [-0.0, 0.0, -np.inf, -np.inf]
    return dist


def sort_nan_input(n):
    """(1, len(NAN_ROWS), n): the same quantised row with NaN of either sign at slot 0, at slot 3 (< k), only beyond k (at a few
    slots, the row's last among them), everywhere -- and without any, as control"""
    rng = np.random.default_rng(1400 + n)
    base = quantised((n,), rng)
    bits = np.tile(base.view(np.uint32), (len(NAN_ROWS), 1))
    for r, name in enumerate(NAN_ROWS):
        if name == "control":
            continue
        where, sign = name.split("_")
        nan = POS_NAN if sign == "pos" else NEG_NAN
        at = {"slot0": [0], "slot3": [3], "tail": [NAN_K, NAN_K + 7, n // 2, n - 1], "all": list(range(n))}[where]
        bits[r, at] = nan
    return bits.view(F)[None].copy()
