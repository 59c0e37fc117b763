"""Exact-arithmetic probe cases for the fused inference MLP kernels (csrc/sa_mlp.hip, sa_mlp_stream.hip, coop_mlp.hip,
fp_mlp.hip), shared by tests/test_mlp_exact_model.py (numpy model of the six-term scheme, CPU) and
tests/test_mlp_exact_gpu.py (the kernels). Plain helper module, deterministic (seeded numpy).

The kernels evaluate an fp32 product on the bf16 matrix pipe: both operands are split into three bf16 levels by
round-to-nearest-even and the (weight level, activation level) terms TERMS are kept; (1,2), (2,1) and (2,2) are dropped.
The inputs built here make that scheme EXACT, so the comparison is np.array_equal against a float64 evaluation:
  * a product x.w loses nothing when its dropped terms are zero: x has one level and w is anything, both have at most two
    levels, or w has one level and x is anything;
  * a bf16 x bf16 product is exact in the fp32 accumulator; a dot product plus bias is exact in ANY order and grouping
    when every term is a multiple of one 2^-q and sum |terms| + |bias| < 2^(24-q): every partial sum is then a multiple
    of 2^-q below 2^24 of them, i.e. an fp32 value;
  * ReLU, max-pooling, bias + ReLU after the max and selection are exact.
check_exact() asserts these conditions on the case itself (a condition on the inputs, not a measurement) and returns the
float64 result as float32.

Value classes: plain = small integers (one level); two_level = +-(1 + a 2^-9); rich = +-(1 + a 2^-9 + c 2^-17), a, c in
{1, 3} (needs all three levels). One PROBE layer per case:
  w_rich  plain activations into a dense rich weight matrix: terms (0,0), (1,0), (2,0), every packed plane of every pair;
  x_rich  rich activations into a one-level layer: terms (0,1), (0,2). At layer 1 the inputs themselves are rich, at layer
          L > 1 layer L - 1 is the dense rich one;
  cross   two_level activations into dense two_level weights: term (1,1) (at L > 1 layer L - 1 routes with two_level weights).
Every other layer ROUTES: each input row feeds exactly one output column with a weight of +-1 or 2 (random, the live channels
dealt round the 32-channel tiles of the output, so every tile of the activations is used; ceil(K / N) rows per column where
N < K, columns without a row are bias-only where N > K). Routing never increases the number of non-zero activations, which
is what keeps the sums of the probe layer inside the budget."""
import functools

import numpy as np

TERMS = [(0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0)]          # (weight level, activation level), mma_x6's order
INF = np.float32(np.inf)
DIST_ROWS = np.array([[1, INF, INF], [1, 1, INF], [1, 2, 2]], np.float32)     # weights (1,0,0), (1/2,1/2,0), (1/2,1/4,1/4)


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------
def bf16_levels(x):
    """The three round-to-nearest-even bf16 levels of float32 values (split_act / mlp_split_weight), as float64 arrays."""
    r = np.ascontiguousarray(x, dtype=np.float32)
    levels = []
    for _ in range(3):
        u = r.view(np.uint32).astype(np.uint64)
        hi = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32).reshape(r.shape)
        levels.append(hi.astype(np.float64))
        r = (r - hi).astype(np.float32)
    return levels


def low_bit(a):
    """Smallest q >= 0 with every value of a a multiple of 2^-q."""
    a = np.asarray(a, np.float64)
    a = a[np.isfinite(a) & (a != 0)]
    if not a.size:
        return 0
    m, e = np.frexp(a)                                               # a = mi 2^(e - 53), mi a 53-bit integer
    mi = np.abs(np.ldexp(m, 53)).astype(np.int64)
    tz = np.frexp((mi & -mi).astype(np.float64))[1] - 1              # trailing zeros of mi
    return max(0, int((53 - tz - e).max()))


def _is_f32(a):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(a, np.float64).astype(np.float32).astype(np.float64))


def mm(x, w):
    """x @ w in float64. Every term and partial sum of a case is exact in float64 (53 bits against the 24 of the budget), so
    the order is free; the routing layers (one non-zero per weight row) and sparse activations are taken the cheap way."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    per_row = np.count_nonzero(w, axis=1)
    if per_row.max(initial=0) <= 1:
        out = np.zeros((x.shape[0], w.shape[1]))
        rows = np.flatnonzero(per_row)
        cols = np.argmax(w[rows] != 0, axis=1)
        order = np.argsort(cols, kind="stable")
        rows, cols = rows[order], cols[order]
        rank = np.arange(len(cols)) - np.searchsorted(cols, cols)          # position of the row within its column
        for r in range(int(rank.max(initial=-1)) + 1):
            s = rank == r
            out[:, cols[s]] += x[:, rows[s]] * w[rows[s], cols[s]]
        return out
    nnz = int(np.count_nonzero(x, axis=1).max(initial=0))
    if nnz * 8 <= x.shape[1]:
        order = np.argsort(x == 0, axis=1, kind="stable")[:, :nnz]         # the non-zero columns of every row first
        vals = np.take_along_axis(x, order, axis=1)
        out = np.zeros((x.shape[0], w.shape[1]))
        for s in range(nnz):
            out += vals[:, s, None] * w[order[:, s]]
        return out
    return x @ w


def _check_products(x, w, what):
    """Every x[r, k] . w[k, n] is exact in the six kept terms: the dropped (weight level, activation level) terms vanish.
    Returns (sum of |levels| of x, of w): what the absolute-sum condition is taken over (the levels of a value can differ
    in sign, so their absolute sum can exceed the value's)."""
    assert _is_f32(x) and _is_f32(w), what
    xl, wl = bf16_levels(x), bf16_levels(w)
    xk, wk = [v.any(axis=0) for v in xl], [v.any(axis=1) for v in wl]                             # per contraction index k
    for i, j in ((1, 2), (2, 1), (2, 2)):
        assert not (xk[j] & wk[i]).any(), "%s: dropped term (%d,%d) is not zero" % (what, i, j)
    return np.abs(xl[0]) + np.abs(xl[1]) + np.abs(xl[2]), np.abs(wl[0]) + np.abs(wl[1]) + np.abs(wl[2])


# ---- values -----------------------------------------------------------------------------------------------------------------
def _signs(rng, shape):
    return rng.choice(np.array([-1.0, 1.0]), size=shape)


def values(rng, cls, shape):
    if cls == "unit":
        return _signs(rng, shape)
    if cls == "plain":
        return _signs(rng, shape) * rng.choice(np.array([1.0, 2.0]), size=shape, p=[0.7, 0.3])
    a = rng.choice(np.array([1.0, 3.0]), size=shape)
    if cls == "two_level":
        return _signs(rng, shape) * (1 + a * 2.0 ** -9)
    assert cls == "rich"
    c = rng.choice(np.array([1.0, 3.0]), size=shape)
    return _signs(rng, shape) * (1 + a * 2.0 ** -9 + c * 2.0 ** -17)


def _sparse_rows(rng, rows, width, nnz, cls):
    """(rows, width) with at most nnz non-zero entries per row, of class cls. Row r puts them into the 32-channel tiles
    r nnz, r nnz + 1, .. (cyclically), so that few rows still reach every tile."""
    out = np.zeros((rows, width))
    if width == 0:
        return out
    tiles = -(-width // 32)
    nnz = min(nnz, width)
    tile = (np.arange(rows)[:, None] * nnz + np.arange(nnz)[None, :]) % tiles
    size = np.minimum(32, width - 32 * tile)
    cols = 32 * tile + (rng.integers(0, 32, (rows, nnz)) + np.arange(nnz)[None, :] // tiles) % size
    out[np.arange(rows)[:, None], cols] = values(rng, cls, (rows, nnz))
    return out


def _route(rng, x, n, cls, after_probe):
    """Each input channel of x (rows, k) feeds one output column. Before the probe layer: weights +-1 / 2, at most three biased
    columns (the number of non-zero activations must not grow). Behind it: mostly +1, so that ReLU keeps the probe's channels
    visible, and -1 together with a positive bias. The channels that are non-zero somewhere go first and are dealt round the
    32-column tiles of the output with a sign that keeps them alive, so that every contraction tile of the NEXT layer carries
    a live activation wherever there are enough live channels (a tile of dead channels would hide its weight planes)."""
    k = x.shape[1]
    w, b = np.zeros((k, n)), np.zeros(n)
    tiles = [rng.permutation(np.arange(t, min(t + 32, n))) for t in range(0, n, 32)]
    seq = np.array([t[r] for r in range(32) for t in tiles if r < len(t)])            # column r of every tile, r = 0, 1, ..
    live = (x != 0).any(axis=0)
    rows = np.concatenate([rng.permutation(np.flatnonzero(live)), rng.permutation(np.flatnonzero(~live))])
    col = seq[np.arange(k) % n]
    if cls == "plain":
        wt = rng.choice(np.array([1.0, -1.0, 2.0]), size=k, p=[0.85, 0.15, 0.0] if after_probe else [0.75, 0.15, 0.10])
    else:
        wt = values(rng, cls, k)
    first = np.arange(k) < len(tiles)                                                 # the first channel of every tile stays alive
    sign = np.where((x[:, rows] * wt > 0).any(axis=0), 1.0, -1.0)
    wt = np.where(first, wt * sign, wt)
    w[rows, col] = wt
    nlive = int(live.sum())
    for i in range(nlive, min(2 * len(tiles), n) if nlive else 0):                    # fewer live channels than two per tile: a
        r = rows[i % nlive]                                                           # live channel also feeds the tiles left over
        w[r, seq[i]] = abs(wt[i % nlive]) * (1.0 if (x[:, r] > 0).any() else -1.0)
    if after_probe:
        neg = np.unique(col[wt < 0])
        b[neg] = 2.0
        b[rng.choice(n, size=max(1, n // 8), replace=False)] += rng.choice(np.array([-1.0, 1.0]), size=max(1, n // 8))
    else:
        b[rng.choice(n, size=min(3, n), replace=False)] = rng.choice(np.array([-1.0, 1.0]), size=min(3, n))
    return w, b


def _input_class(kind, layer):
    """The value class the layer-1 INPUTS need."""
    return {"w_rich": "plain", "x_rich": "rich", "cross": "two_level"}[kind] if layer == 1 else "plain"


def _layers(rng, x, widths, kind, layer):
    """x (rows, K) float64: the rows layer 1 sees -> [(W float32, b float32)] with the probe of `kind` at 1-based `layer`."""
    nl = len(widths)
    assert 1 <= layer <= nl
    dense = {"w_rich": layer, "x_rich": layer - 1, "cross": layer}[kind]         # 0: none (x_rich at layer 1)
    dense_cls = "two_level" if kind == "cross" else "rich"
    out = []
    for j in range(1, nl + 1):
        k, n = x.shape[1], widths[j - 1]
        if j == dense:
            w = values(rng, dense_cls, (k, n))
            b = np.where(rng.random(n) < 0.5, values(rng, dense_cls, n), rng.integers(-1, 3, n).astype(np.float64))
        elif kind == "cross" and j == layer - 1:
            w, b = _route(rng, x, n, "two_level", False)
        else:
            w, b = _route(rng, x, n, "plain", j > dense if dense else j > 1)
        out.append((w.astype(np.float32), b.astype(np.float32)))
        x = np.maximum(mm(x, w) + b, 0.0)
    return out


def _fraction(rng, cls, shape):
    """What makes an integer coordinate two_level / rich (half of the coordinates keep their integer)."""
    if cls == "plain":
        return np.zeros(shape)
    f = rng.choice(np.array([1.0, 3.0]), size=shape) * 2.0 ** -9
    if cls == "rich":
        f = f + rng.choice(np.array([1.0, 3.0]), size=shape) * 2.0 ** -17
    return f * (rng.random(shape) < 0.5)


# ---- builders ---------------------------------------------------------------------------------------------------------------
def build_sa(cfeat, widths, ns, kind, layer, xyz_first=True, seed=0, b=3, m=23, n=None, group_all=False):
    """A grouped SA stack: integer xyz and centroids (their difference is an exact small integer), sparse feature rows, idx
    mixing groups of distinct rows with groups padded by repeats of the first hit. group_all: no centroid, the group is the
    cloud (m = 1, ns = n)."""
    if group_all:
        m, ns = 1, n
    elif n is None:
        n = max(64, ns + 11)
    rng = np.random.default_rng([seed, cfeat, ns, layer] + list(widths))
    in_cls = _input_class(kind, layer)
    xyz = rng.integers(0, 3, (b, n, 3)).astype(np.float64) + _fraction(rng, in_cls, (b, n, 3))
    new_xyz = None if group_all else rng.integers(0, 3, (b, m, 3)).astype(np.float64)
    points = _sparse_rows(rng, b * n, cfeat, 8 if group_all else 3, in_cls).reshape(b, n, cfeat) if cfeat else None     # (few groups: more per row)
    idx = None
    if not group_all:
        idx = np.empty((b, m, ns), np.int32)
        for g in range(b * m):
            if g % 2 == 0 and ns <= n:
                row = rng.permutation(n)[:ns]
            else:                                                     # k distinct hits, then the first one repeated
                k = int(rng.integers(1, min(ns, n) + 1))
                row = np.concatenate([rng.permutation(n)[:k], np.zeros(ns - k, np.int64)])
                row[k:] = row[0]
            idx[g // m, g % m] = row
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    case = dict(family="group_all" if group_all else "sa", kind=kind, layer=layer, cfeat=cfeat, widths=tuple(widths), ns=ns,
                xyz_first=bool(xyz_first), xyz=f32(xyz), new_xyz=f32(new_xyz), points=f32(points), idx=idx)
    case["layers"] = _layers(rng, first_input(case), widths, kind, layer)
    return case


def build_fp(c2, c1, widths, kind, layer, m=3, n=77, b=3, seed=0):
    """A feature-propagation stack: sparse known / skip features, dist rows from DIST_ROWS (m = 1: (1, inf, inf) only)."""
    rng = np.random.default_rng([seed, c2, c1, m, layer] + list(widths))
    in_cls = _input_class(kind, layer)
    if in_cls == "plain":
        in_cls = "unit"                                               # +-1: the interpolation weights cost two bits of the budget
    # a rich first layer: few known rows must still reach every contraction tile of W1a
    nnz2 = max(2, -(-(-(-c2 // 32)) // (b * m))) if (kind, layer) == ("w_rich", 1) else 2
    points2 = _sparse_rows(rng, b * m, c2, nnz2, in_cls).reshape(b, m, c2)
    points1 = _sparse_rows(rng, b * n, c1, 2, in_cls).reshape(b, n, c1) if c1 else None
    idx = rng.integers(0, m, (b, n, 3)).astype(np.int32)
    dist = DIST_ROWS[np.zeros((b, n), np.int64) if m == 1 else rng.integers(0, 3, (b, n))]
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    case = dict(family="fp", kind=kind, layer=layer, c2=c2, c1=c1, widths=tuple(widths), points2=f32(points2),
                points1=f32(points1), idx=idx, dist=np.ascontiguousarray(dist, dtype=np.float32))
    case["layers"] = _layers(rng, first_input(case), widths, kind, layer)
    return case


# ---- float64 evaluation and the exactness conditions ------------------------------------------------------------------------
def fp_weights(dist):
    """pointnet_util.py:212-215 in float64 (exact for DIST_ROWS)."""
    inv = 1.0 / np.maximum(dist.astype(np.float64), 1e-10)
    return inv / inv.sum(axis=-1, keepdims=True)


def first_input(case):
    """The rows layer 1 sees, in the order of ITS weight rows, float64: SA (b m ns, 3 + cfeat), group_all (b n, ..), FP (b n, c2 + c1)."""
    if case["family"] == "fp":
        p2, idx, w = case["points2"].astype(np.float64), case["idx"].astype(np.int64), fp_weights(case["dist"])
        b, n = idx.shape[:2]
        x = sum(np.take_along_axis(p2, np.repeat(idx[:, :, j, None], p2.shape[2], axis=2), axis=1) * w[:, :, j, None] for j in range(3))
        if case["points1"] is not None:
            x = np.concatenate([x, case["points1"].astype(np.float64)], axis=2)
        return x.reshape(b * n, -1)
    xyz = case["xyz"].astype(np.float64)
    b, n = xyz.shape[:2]
    if case["family"] == "group_all":
        parts = [xyz] + ([case["points"].astype(np.float64)] if case["points"] is not None else [])
        return np.concatenate(parts if case["xyz_first"] else parts[::-1], axis=2).reshape(b * n, -1)
    idx = case["idx"].astype(np.int64)
    m, ns = idx.shape[1:]
    bi = np.arange(b)[:, None, None]
    parts = [xyz[bi, idx] - case["new_xyz"].astype(np.float64)[:, :, None, :]]
    if case["points"] is not None:
        parts.append(case["points"].astype(np.float64)[bi, idx])
    return np.concatenate(parts if case["xyz_first"] else parts[::-1], axis=3).reshape(b * m * ns, -1)


def pool(case, rows):
    """(rows, c) -> the entry point's output shape: max over the group (SA, group_all), nothing (FP)."""
    if case["family"] == "fp":
        b, n = case["idx"].shape[:2]
        return rows.reshape(b, n, -1)
    if case["family"] == "group_all":
        b, n = case["xyz"].shape[:2]
        return rows.reshape(b, n, -1).max(axis=1, keepdims=True)
    b, m, ns = case["idx"].shape
    return rows.reshape(b, m, ns, -1).max(axis=2)


def evaluate(case):
    """Plain float64: [(X_j, pre_j)] of every layer (pre = X W + b, before ReLU) and the pooled output."""
    x = first_input(case)
    trace = []
    for w, bias in case["layers"]:
        pre = mm(x, w) + bias.astype(np.float64)
        trace.append((x, pre))
        x = np.maximum(pre, 0.0)
    return trace, pool(case, x)


def _check_sum(terms_abs, q, what):
    worst = float(terms_abs.max()) if terms_abs.size else 0.0
    assert worst < 2.0 ** (24 - q), "%s: sum |terms| + |bias| = %g is not below 2^(24 - %d)" % (what, worst, q)


def check_exact(case):
    """Assert the conditions under which ANY complete six-term evaluation reproduces float64 bit for bit, layer by layer (see
    the module docstring); return (expected output float32, q of the last layer)."""
    trace, out = evaluate(case)
    q = 0
    for j, ((x, pre), (w, bias)) in enumerate(zip(trace, case["layers"])):
        what = "layer %d" % (j + 1)
        w64, b64 = w.astype(np.float64), bias.astype(np.float64)
        if j == 0 and case["family"] == "fp":
            # the kernel's grouping: Q = points2 . W1a per known point (its own sum), then w1 Q1 + w2 Q2 + w3 Q3 in fp32
            # (the interpolation weights cost low bits: 2 for (1/2, 1/4, 1/4)), + bias + the skip part on the matrix pipe
            c2 = case["c2"]
            p2 = case["points2"].astype(np.float64).reshape(-1, c2)
            ax, aw = _check_products(p2, w64[:c2], what + " (known features)")
            qq = low_bit(p2) + low_bit(w64[:c2])
            absq = mm(ax, aw)
            _check_sum(absq, qq, what + " Q")
            wi, idx = fp_weights(case["dist"]), case["idx"].astype(np.int64)
            b, n = idx.shape[:2]
            absq = absq.reshape(b, -1, absq.shape[1])
            total = sum(np.take_along_axis(absq, np.repeat(idx[:, :, k, None], absq.shape[2], axis=2), axis=1) * wi[:, :, k, None]
                        for k in range(3)).reshape(b * n, -1)
            q = qq + low_bit(wi)
            if case["c1"]:
                p1 = x[:, c2:]
                ax, aw = _check_products(p1, w64[c2:], what + " (skip link)")
                q = max(q, low_bit(p1) + low_bit(w64[c2:]))
                total = total + mm(ax, aw)
        else:
            ax, aw = _check_products(x, w64, what)
            q = low_bit(x) + low_bit(w64)
            total = mm(ax, aw)
        q = max(q, low_bit(b64))
        _check_sum(total + np.abs(b64), q, what)
        assert low_bit(pre) <= q and _is_f32(x) and _is_f32(pre), what
    assert _is_f32(out)
    return out.astype(np.float32), q


# ---- the case table ---------------------------------------------------------------------------------------------------------
PROBES = [(k, l) for k in ("w_rich", "x_rich", "cross") for l in (1, 2, 3)]

# (family the library must choose, cfeat, widths, nsample); the first of each family also runs with xyz_first=False
SA_STACKS = [("resident", 0, (64, 64, 128), 32), ("resident", 0, (32, 32, 64), 16), ("resident", 6, (64, 96, 128), 32),
             ("resident", 1, (17, 33, 65), 16), ("resident", 0, (24, 40, 100), 128),
             ("streamed", 64, (64, 64, 128), 32), ("streamed", 128, (128, 128, 256), 64), ("streamed", 320, (128, 128, 256), 32),
             ("streamed", 61, (100, 120, 200), 32),
             ("cooperative", 256, (256, 256, 512), 32), ("cooperative", 61, (200, 256, 500), 40), ("cooperative", 128, (128, 128, 256), 16),
             ("cooperative_gemm", 6, (200, 400, 900), 150), ("cooperative_gemm", 64, (256, 512, 1024), 32)]
FEATURES_FIRST = [("resident", 6, (64, 96, 128), 32), ("streamed", 64, (64, 64, 128), 32), ("cooperative", 256, (256, 256, 512), 32),
                  ("cooperative_gemm", 64, (256, 512, 1024), 32)]
GROUP_ALL = [(2, 33, 5), (3, 100, 256), (2, 128, 640)]                  # (b, n, cfeat), widths (256, 512, 1024)
GROUP_ALL_WIDTHS = (256, 512, 1024)
# (c2, c1, widths): the sets of tests/test_fp_mlp_gpu.py's CASES -- (128, 0, ..): no skip link; (128, 6), (20, 5), (8, 3): c1 % 4 != 0
FP_STACKS = [(1024, 256, (256, 256)), (256, 128, (256, 128)), (128, 6, (128, 128, 128)), (512, 256, (256, 256)),
             (256, 128, (256, 256)), (256, 64, (256, 128)), (128, 0, (128, 128, 128)), (20, 5, (40, 100)), (8, 3, (32, 48, 16))]
FP_KNOWN = (1, 2, 3, 17)                                                # m, cycled over the cases


def sa_id(fam, cfeat, widths, ns, kind, layer, xyz_first=True):
    return "%s-c%d-%s-ns%d-%s@%d%s" % (fam, cfeat, "x".join(map(str, widths)), ns, kind, layer, "" if xyz_first else "-featfirst")


def case_table():
    """{id: (builder, kwargs)} of every case; build with get_case(id)."""
    table = {}
    for i, (fam, cfeat, widths, ns) in enumerate(SA_STACKS):
        for kind, layer in PROBES:
            table[sa_id(fam, cfeat, widths, ns, kind, layer)] = (build_sa, dict(cfeat=cfeat, widths=widths, ns=ns, kind=kind, layer=layer, seed=i))
    for i, (fam, cfeat, widths, ns) in enumerate(FEATURES_FIRST):
        for kind, layer in (("w_rich", 1), ("x_rich", 1), ("cross", 1)):          # the order only concerns layer 1
            table[sa_id(fam, cfeat, widths, ns, kind, layer, False)] = (build_sa, dict(cfeat=cfeat, widths=widths, ns=ns, kind=kind, layer=layer,
                                                                                     xyz_first=False, seed=50 + i))
    for i, (b, n, cfeat) in enumerate(GROUP_ALL):
        for kind, layer in PROBES:
            table["group_all-b%d-n%d-c%d-%s@%d" % (b, n, cfeat, kind, layer)] = (build_sa, dict(cfeat=cfeat, widths=GROUP_ALL_WIDTHS, ns=None, kind=kind, layer=layer,
                                                                                               seed=70 + i, b=b, n=n, group_all=True))
    k = 0
    for i, (c2, c1, widths) in enumerate(FP_STACKS):
        for kind, layer in PROBES:
            if layer > len(widths):
                continue
            m = FP_KNOWN[k % len(FP_KNOWN)]
            k += 1
            table["fp-%d+%d-%s-m%d-%s@%d" % (c2, c1, "x".join(map(str, widths)), m, kind, layer)] = (build_fp, dict(c2=c2, c1=c1, widths=widths, kind=kind, layer=layer,
                                                                                                                 m=m, seed=90 + i))
    return table


CASES = case_table()
SA_IDS = [k for k, v in CASES.items() if v[0] is build_sa and not v[1].get("group_all")]
GROUP_ALL_IDS = [k for k, v in CASES.items() if v[1].get("group_all")]
FP_IDS = [k for k, v in CASES.items() if v[0] is build_fp]


@functools.lru_cache(maxsize=None)
def get_case(case_id):
    fn, kw = CASES[case_id]
    return fn(**kw)


@functools.lru_cache(maxsize=None)
def expected(case_id):
    """(want float32, q): computed once per session, read-only."""
    want, q = check_exact(get_case(case_id))
    want.setflags(write=False)
    return want, q
