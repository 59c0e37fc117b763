"""A numpy model of the fused inference MLPs' arithmetic on the exact-arithmetic probe cases (tests/mlp_exact_cases.py; CPU,
no device work): round-to-nearest-even three-level bf16 split of both operands, the six kept terms in mma_x6's order, one
fp32 rounding per matrix instruction (a K16 block: 16 exact bf16 x bf16 products added to the fp32 accumulator), the
contraction padded to 32-channel tiles as the packers pad it, the kernels' own grouping of layer 1 (feature-propagation:
Q = points2 . W1a per known point, interpolated in fp32, then the skip link; streamed SA stacks: features and xyz as separate
tiles), bias and ReLU after the pooling in the last layer.

What it shows: (1) on every case the scheme reproduces the float64 evaluation bit for bit, so a complete and correctly packed
kernel has to; (2) the cases SEE what they are meant to see -- dropping any one of the six terms, or zeroing any one level
plane of any one 32x32 tile pair of a probe layer, changes the pooled output of a case aimed at it. The layout itself
(which word of the packed array holds which plane) is tests/test_sa_mlp_pack.py's subject; the kernels are
tests/test_mlp_exact_gpu.py's."""
import ctypes

import numpy as np
import pytest

import mlp_exact_cases as C

_MODEL_ROWS = 384                                     # grouped rows the model walks per case (whole groups; FP: all rows)


def _pad32(a, axis):
    extra = -a.shape[axis] % 32
    if not extra:
        return a
    width = [(0, 0)] * a.ndim
    width[axis] = (0, extra)
    return np.pad(a, width)


def _accumulate(acc, x, w, terms, zero_plane=None):
    """acc (rows, N) float32 += x (rows, K) . w (K, N): per K16 block the kept terms in order, one rounding per term (one MFMA).
    zero_plane = (t, u, level): that level of the 32x32 weight tile (output tile t, contraction tile u) is zero."""
    xl = [_pad32(l, 1) for l in C.bf16_levels(x)]
    wl = [_pad32(l, 0) for l in C.bf16_levels(w)]
    if zero_plane is not None:
        t, u, level = zero_plane
        wl[level] = wl[level].copy()
        wl[level][32 * u:32 * u + 32, 32 * t:32 * t + 32] = 0.0
    for k0 in range(0, xl[0].shape[1], 16):
        for i, j in terms:
            a, bw = xl[j][:, k0:k0 + 16], wl[i][k0:k0 + 16]
            if a.any() and bw.any():                                  # (an all-zero operand adds exact zeros)
                acc = (acc.astype(np.float64) + a @ bw).astype(np.float32)
    return acc


def _groups(case):
    """(number of groups the model walks, rows per group)."""
    if case["family"] == "fp":
        return case["idx"].shape[0] * case["idx"].shape[1], 1
    if case["family"] == "group_all":
        return case["xyz"].shape[0], case["xyz"].shape[1]
    b, m, ns = case["idx"].shape
    return min(b * m, max(2, _MODEL_ROWS // ns)), ns


def _layer1_parts(case, rows):
    """[(x, w)] of layer 1 in the order and the tiling the kernel family accumulates them (bias first, see _forward)."""
    w = case["layers"][0][0].astype(np.float64)
    x = C.first_input(case)[:rows]
    if case["family"] == "fp":
        return [(x[:, case["c2"]:], w[case["c2"]:])] if case["c1"] else []          # the known features go through Q
    from pointnet2_amd import sa_mlp
    cfeat = case["cfeat"]
    fx, ff = (slice(0, 3), slice(3, None)) if case["xyz_first"] else (slice(cfeat, None), slice(0, cfeat))
    kind = sa_mlp.kind(3 + cfeat, case["widths"], case["ns"])
    if kind == "streamed":                                             # per-point feature tiles, then the xyz pair
        return [(x[:, ff], w[ff]), (x[:, fx], w[fx])]
    if kind == "cooperative":                                          # channel order [features, xyz]
        return [(np.concatenate([x[:, ff], x[:, fx]], axis=1), np.concatenate([w[ff], w[fx]], axis=0))]
    return [(np.concatenate([x[:, fx], x[:, ff]], axis=1), np.concatenate([w[fx], w[ff]], axis=0))]   # resident: one tile


def _fp_q(case, terms, zero_plane=None):
    """Q = points2 . W1a (no bias) per known point, then tf_interpolate's (p1 w1 + p2 w2) + p3 w3 in fp32 per unknown point."""
    c2 = case["c2"]
    p2 = case["points2"].astype(np.float64).reshape(-1, c2)
    w = case["layers"][0][0].astype(np.float64)[:c2]
    q = _accumulate(np.zeros((p2.shape[0], w.shape[1]), np.float32), p2, w, terms, zero_plane)
    b, n = case["idx"].shape[:2]
    q = q.reshape(b, -1, q.shape[1])
    wi = C.fp_weights(case["dist"]).astype(np.float32)
    rows = [np.take_along_axis(q, np.repeat(case["idx"][:, :, k, None].astype(np.int64), q.shape[2], axis=2), axis=1) * wi[:, :, k, None]
            for k in range(3)]                                        # float32 products
    return ((rows[0] + rows[1]) + rows[2]).reshape(b * n, -1)          # float32 sums, the reference's order


def _forward(case, terms=C.TERMS, zero_plane=None):
    """The model's pooled output on the first _groups(case) groups. zero_plane = (layer (0-based), part, t, u, level); part -1:
    the known-feature rows of a feature-propagation layer 1."""
    groups, per = _groups(case)
    rows = groups * per
    zp = lambda layer, part: zero_plane[2:] if zero_plane is not None and zero_plane[:2] == (layer, part) else None
    nl = len(case["layers"])
    act = None
    for j, (w, bias) in enumerate(case["layers"]):
        last = j == nl - 1
        n = w.shape[1]
        acc = np.zeros((rows, n), np.float32) if last else np.broadcast_to(bias, (rows, n)).copy()
        if j == 0:
            if case["family"] == "fp":
                with np.errstate(invalid="ignore"):
                    acc = acc + _fp_q(case, terms, zp(0, -1))[:rows]                          # float32 add
            for part, (x, wpart) in enumerate(_layer1_parts(case, rows)):
                acc = _accumulate(acc, x, wpart, terms, zp(0, part))
        else:
            acc = _accumulate(acc, act, w.astype(np.float64), terms, zp(j, 0))
        if not last:
            act = np.maximum(acc, np.float32(0)).astype(np.float64)
    if case["family"] == "fp":
        return np.maximum(acc + bias, np.float32(0))                   # float32: bias + ReLU, plain store
    pooled = acc.reshape(groups, per, -1).max(axis=1)
    return np.maximum(pooled + bias, np.float32(0))                    # bias + ReLU once, after the max


def _want(case_id):
    case = C.get_case(case_id)
    want, _ = C.expected(case_id)
    groups, _ = _groups(case)
    return want.reshape(-1, want.shape[-1])[:groups]


@pytest.mark.parametrize("cid", list(C.CASES))
def test_model_equals_float64(cid):
    """check_exact's conditions hold and the six-term model equals the float64 evaluation bit for bit."""
    got = _forward(C.get_case(cid))
    assert got.dtype == np.float32 and np.array_equal(got, _want(cid))


# small stacks of every family for the mutation legs
_SMALL = ["resident-c0-32x32x64-ns16", "resident-c6-64x96x128-ns32", "streamed-c61-100x120x200-ns32",
          "cooperative-c128-128x128x256-ns16", "fp-20+5-40x100", "fp-8+3-32x48x16", "fp-128+0-128x128x128"]


def _ids(prefix, kind, layer):
    return [i for i in C.CASES if i.startswith(prefix) and i.endswith("%s@%d" % (kind, layer))]


@pytest.mark.parametrize("layer", [1, 2, 3])
@pytest.mark.parametrize("term", C.TERMS, ids=["w%dx%d" % t for t in C.TERMS])
def test_every_term_is_seen(term, layer):
    """Without any one of the six terms the model no longer gives the float64 result on the cases aimed at that term: the
    weight-side terms (0,0), (1,0), (2,0) on w_rich, (0,1) and (0,2) on x_rich, (1,1) on cross -- at every probe layer."""
    kind = "w_rich" if term[1] == 0 else ("cross" if term == (1, 1) else "x_rich")
    ids = [i for p in _SMALL for i in _ids(p, kind, layer)]
    assert ids
    terms = [t for t in C.TERMS if t != term]
    seen = [i for i in ids if not np.array_equal(_forward(C.get_case(i), terms), _want(i))]
    assert seen, "no %s case at layer %d notices the loss of term %r" % (kind, layer, term)
    assert len(seen) == len(ids), sorted(set(ids) - set(seen))        # in fact each of them does


# ---- one level plane of one tile pair ---------------------------------------------------------------------------------------
def _plane_delta(xl, wl, ncols, t, u, level):
    """What the plane contributes to the pre-activations of output tile t: rows x (columns of the tile). xl, wl: padded levels."""
    wt = wl[level][32 * u:32 * u + 32, 32 * t:32 * t + 32]
    return sum(xl[j][:, 32 * u:32 * u + 32] @ wt for i, j in C.TERMS if i == level)[:, :min(32, ncols - 32 * t)]


def _output_changes(case, trace, layer, cols, new_pre):
    """Does the pooled float64 output change when pre-activation columns `cols` of `layer` become new_pre? Only the columns a
    change reaches are recomputed (the layers behind a probe route: one column per row)."""
    for j in range(layer + 1, len(case["layers"])):
        d = np.maximum(new_pre, 0.0) - np.maximum(trace[j - 1][1][:, cols], 0.0)
        if not d.any():
            return False
        wsub = case["layers"][j][0].astype(np.float64)[cols]
        nz = np.flatnonzero(wsub.any(axis=0))
        new_pre, cols = trace[j][1][:, nz] + d @ wsub[:, nz], nz
    return not np.array_equal(C.pool(case, np.maximum(new_pre, 0.0)), C.pool(case, np.maximum(trace[-1][1][:, cols], 0.0)))


def _probe_parts(case, layer):
    """[(part, x, w, lift)] of the probe layer: lift maps a delta on the part's rows to the layer's rows (interpolation for Q)."""
    if layer > 0:
        x = np.maximum(C.evaluate(case)[0][layer - 1][1], 0.0)
        return [(0, x, case["layers"][layer][0].astype(np.float64), lambda d: d)]
    rows = C.first_input(case).shape[0]
    parts = [(p, x, w, lambda d: d) for p, (x, w) in enumerate(_layer1_parts(case, rows))]
    if case["family"] == "fp":
        c2, idx, wi = case["c2"], case["idx"].astype(np.int64), C.fp_weights(case["dist"])
        b, n = idx.shape[:2]

        def lift(d):
            d = d.reshape(b, -1, d.shape[1])
            return sum(np.take_along_axis(d, np.repeat(idx[:, :, k, None], d.shape[2], axis=2), axis=1) * wi[:, :, k, None]
                       for k in range(3)).reshape(b * n, -1)
        parts.append((-1, case["points2"].astype(np.float64).reshape(-1, c2), case["layers"][0][0].astype(np.float64)[:c2], lift))
    return parts


def _planes(case, layer):
    for part, x, w, lift in _probe_parts(case, layer):
        xl = [_pad32(l, 1) for l in C.bf16_levels(x)]
        wl = [_pad32(_pad32(l, 0), 1) for l in C.bf16_levels(w)]
        for t in range(-(-w.shape[1] // 32)):
            for u in range(-(-w.shape[0] // 32)):
                for level in range(3):
                    yield part, xl, wl, w.shape[1], lift, t, u, level


_W_RICH = [i for i in C.CASES if "-w_rich@" in i]


@pytest.mark.parametrize("cid", _W_RICH)
def test_every_weight_plane_is_seen(cid):
    """Zeroing any one level plane of any one tile pair of the rich layer changes the case's output: all of them for stacks up
    to 256 wide, a seeded third of the tile pairs for the wider ones. (Exact arithmetic: the output without the plane is the
    float64 output minus the plane's own contribution, pushed through the layers behind it.)"""
    case = C.get_case(cid)
    layer = int(cid.split("@")[1].split("-")[0]) - 1
    trace, _ = C.evaluate(case)
    wide = max(case["widths"]) > 256
    pairs = [(part, t, u) for part, _, w, _ in _probe_parts(case, layer)
             for t in range(-(-w.shape[1] // 32)) for u in range(-(-w.shape[0] // 32))]
    if wide:
        pick = np.random.default_rng(len(cid)).choice(len(pairs), size=-(-len(pairs) // 3), replace=False)
        pairs = [pairs[i] for i in pick]
    pairs = set(pairs)
    missed, tried = [], 0
    for part, xl, wl, ncols, lift, t, u, level in _planes(case, layer):
        if (part, t, u) not in pairs:
            continue
        tried += 1
        cols = np.arange(32 * t, min(32 * t + 32, ncols))
        new_pre = trace[layer][1][:, cols] - lift(_plane_delta(xl, wl, ncols, t, u, level))
        if not _output_changes(case, trace, layer, cols, new_pre):
            missed.append((part, t, u, level))
    assert tried and not missed, "%d of %d planes unseen: %r" % (len(missed), tried, missed[:8])


@pytest.mark.parametrize("cid", ["resident-c6-64x96x128-ns32-w_rich@2", "streamed-c61-100x120x200-ns32-w_rich@1",
                                 "cooperative-c128-128x128x256-ns16-w_rich@3", "fp-20+5-40x100-m1-w_rich@1", "fp-8+3-32x48x16-m17-w_rich@2"])
def test_plane_shortcut_is_the_model(cid):
    """The shortcut of test_every_weight_plane_is_seen against the model itself with the plane zeroed, on a few planes."""
    case = C.get_case(cid)
    layer = int(cid.split("@")[1]) - 1
    trace, _ = C.evaluate(case)
    groups, _ = _groups(case)
    base = _want(cid)
    planes = list(_planes(case, layer))
    for part, xl, wl, ncols, lift, t, u, level in planes[::max(1, len(planes) // 7)]:
        got = _forward(case, zero_plane=(layer, part, t, u, level))
        cols = np.arange(32 * t, min(32 * t + 32, ncols))
        new_pre = trace[layer][1][:, cols] - lift(_plane_delta(xl, wl, ncols, t, u, level))
        full = [tr[1].copy() for tr in trace]
        full[layer][:, cols] = new_pre
        act = np.maximum(full[layer], 0.0)
        for j in range(layer + 1, len(case["layers"])):
            act = np.maximum(act @ case["layers"][j][0].astype(np.float64) + case["layers"][j][1], 0.0)
        want = C.pool(case, act)
        want = want.reshape(-1, want.shape[-1])[:groups]
        assert np.array_equal(got, want.astype(np.float32)) and np.array_equal(want, want.astype(np.float32))
        assert not np.array_equal(got, base)


# ---- the host split behind the pack entry points ----------------------------------------------------------------------------
def _decode_pair(words):
    """One packed tile pair [e][level][lane][8 bf16] -> three (32, 32) planes [k][n] (tests/test_sa_mlp_pack.py's decode)."""
    raw = (np.ascontiguousarray(words).view(np.uint16).reshape(2, 3, 64, 8).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    planes = np.zeros((3, 32, 32))
    for e in range(2):
        for lane in range(64):
            for j in range(8):
                v = 8 * e + j
                k = 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3)
                planes[:, k, lane & 31] = raw[e, :, lane, j]
    return planes


def test_packed_planes_of_a_rich_matrix_sum_back_exactly():
    """mlp_split_weight through pn2_sa_mlp3_pack and pn2_fp_mlp_pack: the three stored planes of a rich 32x32 tile are the
    round-to-nearest-even levels and sum to the matrix exactly."""
    from pointnet2_amd import _C
    lib = _C.lib()
    rng = np.random.default_rng(11)
    w = C.values(rng, "rich", (32, 32)).astype(np.float32)
    zeros = np.zeros(32, np.float32)
    levels = np.stack(C.bf16_levels(w))
    assert all(levels[l].any() for l in range(3))

    info = (ctypes.c_int * 4)()
    wf, bf = ctypes.c_longlong(), ctypes.c_longlong()
    assert lib.pn2_sa_mlp3_config(32, 32, 32, 32, 32, info, ctypes.byref(wf), ctypes.byref(bf)) == 0 and info[0] == 0
    wp, bp = np.empty(wf.value, np.float32), np.empty(bf.value, np.float32)
    assert lib.pn2_sa_mlp3_pack(32, 32, 32, 32, 32, 1, w.ctypes.data, zeros.ctypes.data, w.ctypes.data, zeros.ctypes.data,
                                w.ctypes.data, zeros.ctypes.data, wp.ctypes.data, bp.ctypes.data) == 0
    planes = _decode_pair(wp[1536:2 * 1536])                          # layer 2: no row permutation
    assert np.array_equal(planes, levels) and np.array_equal(planes.sum(axis=0), w.astype(np.float64))

    widths = (ctypes.c_int * 2)(32, 32)
    for kind in (0, 1):
        assert lib.pn2_fp_mlp_config(32, 0, 2, widths, kind, info, ctypes.byref(wf), ctypes.byref(bf)) == 0 and info[0] == 0
        wp, bp = np.empty(wf.value, np.float32), np.empty(bf.value, np.float32)
        wptr = (ctypes.c_void_p * 2)(w.ctypes.data, w.ctypes.data)
        bptr = (ctypes.c_void_p * 2)(zeros.ctypes.data, zeros.ctypes.data)
        assert lib.pn2_fp_mlp_pack(32, 0, 2, widths, kind, wptr, bptr, wp.ctypes.data, bp.ctypes.data) == 0
        # no skip link: the main stream starts with layer 2's pair (t = 0, u = 0) in both kernels' orders
        planes = _decode_pair(wp[:1536])
        assert np.array_equal(planes, levels) and np.array_equal(planes.sum(axis=0), w.astype(np.float64))
        # the per-point kernel's stream of the known-feature rows of layer 1 sits behind the main stream: its first pair
        npoint = ((32 + 31) // 32) * info[1]
        planes = _decode_pair(wp[wp.size - npoint * 1536:][:1536])
        assert np.array_equal(planes, levels)
