"""Gradients of the scatter-add operators (group_point, gather_point, three_interpolate) at every SA and FP level of the reference
configurations, at the configuration's own batch, and at the edges of the segmented reduction's dispatch (csrc/seg_grad.hip).

Every gradient runs through autograd (or the C ABI where a pointer matters) in both modes and is checked against a float64
scatter-add on the device:
  * default mode: every element within mag * 2^-24 * max(count, 2) of the exact sum (mag = sum of |addend|, count = entries
    of the row) -- the bound of a sequential fp32 sum;
  * reproducible mode: two calls give identical bits, and every row equals one of two restatements BIT FOR BIT:
      - rows inside the sorted envelope -- at least 4 clouds, rows per cloud <= SEG_LDS_ROWS, rows + entries per cloud <=
        SEG_FIT_INTS (counters and list in 144 KiB of LDS), segment of at most SEG_SORT_MAX entries -- equal the reference's CPU
        loop (oracle.group_point_grad / three_interpolate_grad: ascending entry order);
      - every other row of the segmented reduction equals oracle.fixed_point_grad (64-bit fixed point, one scale per element
        from the largest addend of its own segment);
      - the calls that do not take the segmented reduction (fewer than 16 channels with fewer than 4 clouds or more than
        SEG_LDS_ROWS rows per cloud, and every gather_point) use det_grad.hip: the same fixed-point sum with ONE scale per
        call, from the largest |grad_out| (and |weight|) of the whole call; restated with oracle.fixed_point_grad(shift=k).
    The test derives the kind of every row from these documented conditions and asserts which kinds occur.
The bit-exact CPU comparisons take every cloud up to 64 MB of addends, else three clouds (those holding fixed-point rows
first); the float64 bound covers every cloud."""
import numpy as np
import pytest
import torch

from pointnet2_amd import reference_configs as RC
from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

# The reproducible mode's envelope (README.md "Reproducible gradients"; csrc/seg_grad.hip kSegLdsRows, the 144 KiB LDS fit,
# kSegSortMax) and the segmented reduction's dispatch (_tensors.use_segmented_grad), restated here on purpose.
SEG_LDS_ROWS = 24576
SEG_FIT_INTS = 36864
SEG_SORT_MAX = 1024
SEG_MIN_CHANNELS = 16
BIT_CHECK_BYTES = 64 << 20


def _ceil_log2(v):
    return (int(v) - 1).bit_length() if v > 1 else 0


def _exp_field(x):
    return int(np.float32(x).view(np.uint32)) >> 23 & 0xff


def _cloud(label, b, n, seed):
    return S.uniform_clouds(b, n, seed) if "sem_seg" in label else S.sphere_clouds(b, n, seed)


def _grad_out(shape, seed, dev):
    """standard normals, every row (last axis) scaled by 10 ** U(-3, 3)"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    g = torch.randn(shape, generator=gen, device=dev)
    scale = 10.0 ** (torch.rand(tuple(shape[:-1]) + (1,), generator=gen, device=dev) * 6.0 - 3.0)
    return (g * scale).contiguous()


def _reference(rows, target, addend):
    """float64 scatter-add on the device: target (b, e) row numbers, addend (b, e, c) -> sum, sum of |addend| (b, rows, c)
    and the entries per row (b, rows, 1)."""
    b, e, c = addend.shape
    dev = addend.device
    flat = (target.long() + torch.arange(b, device=dev)[:, None] * rows).reshape(-1)
    a = addend.reshape(-1, c)
    want = torch.zeros(b * rows, c, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(want)
    step = max(1, (1 << 24) // c)
    for s in range(0, flat.numel(), step):
        part = a[s:s + step].double()
        want.index_add_(0, flat[s:s + step], part)
        mag.index_add_(0, flat[s:s + step], part.abs_())
    cnt = torch.bincount(flat, minlength=b * rows).double()
    return want.view(b, rows, c), mag.view(b, rows, c), cnt.view(b, rows, 1)


def _assert_bound(got, ref, what, resolution=0.0):
    want, mag, cnt = ref
    tol = mag * 2.0 ** -24 * cnt.clamp(min=2) + cnt * resolution + 1e-30
    err = (got.double() - want).abs()
    bad = ~(err <= tol)                                              # NaN fails too
    assert not bool(bad.any()), "%s: %d elements outside the bound, worst err/tol %.3g" % (
        what, int(bad.sum()), float(torch.nan_to_num(err / tol, nan=float("inf")).max()))


class Case:
    """One gradient: `run(det)` returns it (b, rows, c); target (b, e) / addend (b, e, c) are its scatter-add on the device;
    `cpu_loop(sel)` the reference CPU loop's result for clouds `sel` (float32); grad_out / weight feed det_grad.hip's scale."""

    def __init__(self, b, rows, c, target, addend, run, cpu_loop, grad_out, weight=None, has_segmented_form=True):
        self.b, self.rows, self.c = b, rows, c
        self.has_segmented_form = has_segmented_form
        self.entries = target.shape[1]
        self.target, self.addend, self.run, self.cpu_loop = target, addend, run, cpu_loop
        self.grad_out, self.weight = grad_out, weight

    def segmented(self):
        return self.has_segmented_form and (self.c >= SEG_MIN_CHANNELS or (self.b >= 4 and self.rows <= SEG_LDS_ROWS))

    def inside_envelope(self):
        return self.b >= 4 and self.rows <= SEG_LDS_ROWS and self.rows + self.entries <= SEG_FIT_INTS

    def tensor_shift(self):
        """det_grad.hip: k = 62 - ceil(log2 entries) - (e(max |grad_out|) - 126) - (e(max |weight|, or 1.0) - 126)"""
        gmax = float(self.grad_out.abs().max()) if self.grad_out.numel() else 0.0
        wmax = float(self.weight.abs().max()) if self.weight is not None else 0.0
        return 62 - _ceil_log2(self.entries) - (_exp_field(gmax) - 126) - (_exp_field(wmax if wmax > 0 else 1.0) - 126)


def _run_modes(fn, shape, dev):
    """fn(leaf) -> output; once(det, g): the gradient of leaf (zeros of `shape`) for grad_out g, in the given mode"""
    import pointnet2_amd as P

    def once(det, g):
        leaf = torch.zeros(shape, device=dev, requires_grad=True)
        P.set_deterministic(det)
        try:
            fn(leaf).backward(g)
        finally:
            P.set_deterministic(False)
        return leaf.grad.detach()
    return once


def _check(case, oracle, expect, what):
    """Both modes against the float64 scatter-add, reproducibility, and the row kinds of the reproducible mode: `expect` is
    the set of kinds that must occur among the non-empty rows -- "cpu" (CPU loop order), "fixed" (per-element fixed point),
    "tensor" (det_grad.hip)."""
    b, rows = case.b, case.rows
    ref = _reference(rows, case.target, case.addend)
    lens = ref[2].view(b, rows).cpu().numpy().astype(np.int64)
    _assert_bound(case.run(False), ref, what + " default mode")
    d1 = case.run(True)
    d2 = case.run(True)
    assert torch.equal(d1.view(torch.int32), d2.view(torch.int32)), what + " reproducible mode: two calls differ"

    shift, resolution = None, 0.0
    cpu_rows = np.zeros((b, rows), bool)
    if not case.segmented():
        shift = case.tensor_shift()
        resolution = 2.0 ** -(shift + 1)
        kinds = {"tensor"}
    else:
        if case.inside_envelope():
            cpu_rows = lens <= SEG_SORT_MAX
        kinds = set()
        if (cpu_rows & (lens > 0)).any():
            kinds.add("cpu")
        if (~cpu_rows & (lens > 0)).any():
            kinds.add("fixed")
    assert kinds == set(expect), (what, sorted(kinds), sorted(expect))
    _assert_bound(d1, ref, what + " reproducible mode", resolution)

    per_cloud = case.entries * case.c * 4
    fixed_clouds = np.nonzero((~cpu_rows & (lens > 0)).any(axis=1))[0] if shift is None else np.zeros(0, np.int64)
    if b * per_cloud <= BIT_CHECK_BYTES:
        sel = list(range(b))
    else:
        sel = [0] + [int(i) for i in fixed_clouds if i != 0][:2]
        sel += [i for i in range(1, b) if i not in sel][:3 - len(sel)]
        sel = sorted(sel)
    got = d1[sel].cpu().numpy()
    target = case.target[sel].cpu().numpy()
    addend = case.addend[sel].cpu().numpy()
    cpu = case.cpu_loop(sel) if cpu_rows[sel].any() else None
    for j, i in enumerate(sel):
        want = oracle.fixed_point_grad(rows, target[j], addend[j], shift=shift)
        if cpu is not None:
            want = np.where(cpu_rows[i][:, None], cpu[j], want)
        bad = np.nonzero((got[j].view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, "%s reproducible mode, cloud %d: %d rows not bit-identical (%d of them CPU-order rows), rows %s" % (
            what, i, bad.size, int(cpu_rows[i][bad].sum()), bad[:8].tolist())


def _group_case(P, oracle, xyz_or_feats, idx, seed, dev):
    """group_point's gradient with respect to `xyz_or_feats` (b, n, c) through autograd, idx (b, m, ns) on the device"""
    b, n, c = xyz_or_feats.shape
    _, m, ns = idx.shape
    g = _grad_out((b, m, ns, c), seed, dev)
    once = _run_modes(lambda leaf: P.group_point(leaf, idx), (b, n, c), dev)
    idx_h = idx.cpu().numpy()

    def cpu_loop(sel):
        return oracle.group_point_grad((len(sel), n, c), idx_h[sel], g[sel].cpu().numpy())
    return Case(b, n, c, idx.reshape(b, -1), g.reshape(b, -1, c), lambda det: once(det, g), cpu_loop, g)


# ------------------------------------------------------------------------------------------------ reference configurations
# The kind of row the reproducible mode gives at each configuration shape (derived from the envelope, asserted by the test):
#   cfg1 (b = 2, no features: grouped xyz, c = 3): det_grad.hip, one scale per call;
#   cls_msg L1 r = 0.4 / ns = 128 (4096 + 65536) and sem_seg SA1 (8192 + 32768): the list does not fit -> fixed point;
#   cls_msg L2 r = 0.8 / ns = 128: padding piles more than 1024 references on a few low point numbers -> both kinds;
#   the metric shape: 4096 + 32768 = 36864 exactly, the fit boundary -> CPU order;
#   every other SA and FP level: CPU order. gather_point's gradient is always det_grad.hip.
SA_CASES = [(lv, s) for lv in RC.SA_LEVELS for s in range(len(lv[4]))]
SA_EXPECT = {("cfg1 SA", 0): {"tensor"}, ("cfg3 cls_msg L1", 2): {"fixed"}, ("cfg5 sem_seg SA1", 0): {"fixed"},
             ("cfg3 cls_msg L2", 2): {"cpu", "fixed"}}


@pytest.mark.parametrize("level,scale", SA_CASES, ids=["%s r%g ns%d" % (lv[0], lv[4][s][0], lv[4][s][1]) for lv, s in SA_CASES])
def test_sa_level_gradients_at_config_shape(cuda, oracle, level, scale):
    import pointnet2_amd as P
    label, b, n, npoint, scales, c = level
    radius, ns = scales[scale]
    xyz = _cloud(label, b, n, 1100 + len(label))
    x = torch.from_numpy(xyz).to(cuda)
    fps = P.farthest_point_sample(npoint, x)
    new_xyz = P.gather_point(x, fps)
    idx, _ = P.query_ball_point(radius, ns, x, new_xyz)
    expect = SA_EXPECT.get((label, scale), {"cpu"})
    if label.startswith("metric"):
        assert n + npoint * ns == SEG_FIT_INTS                     # the metric shape sits exactly on the fit boundary
    what = "%s r=%g ns=%d" % (label, radius, ns)
    if c:
        feats = torch.zeros(b, n, c, device=cuda)
        _check(_group_case(P, oracle, feats, idx, 10 * scale + 1, cuda), oracle, expect, what + " group_point c=%d" % c)
    _check(_group_case(P, oracle, x, idx, 10 * scale + 2, cuda), oracle, expect, what + " group_point xyz")
    if scale == 0:
        g = _grad_out((b, npoint, 3), 3, cuda)
        once = _run_modes(lambda leaf: P.gather_point(leaf, fps), (b, n, 3), cuda)
        case = Case(b, n, 3, fps, g, lambda det: once(det, g), None, g, has_segmented_form=False)
        _check(case, oracle, {"tensor"}, what + " gather_point")


FP_IDS = [lv[0] for lv in RC.FP_LEVELS]


def _interp_case(P, oracle, known_feats_shape, nidx, w, seed, dev):
    b, m, c = known_feats_shape
    n = nidx.shape[1]
    g = _grad_out((b, n, c), seed, dev)
    addend = (g[:, :, None, :] * w[:, :, :, None]).reshape(b, 3 * n, c)     # fp32 products, as the reference forms them
    once = _run_modes(lambda leaf: P.three_interpolate(leaf, nidx, w), (b, m, c), dev)
    idx_h, w_h = nidx.cpu().numpy(), w.cpu().numpy()

    def cpu_loop(sel):
        return oracle.three_interpolate_grad((len(sel), m, c), idx_h[sel], w_h[sel], g[sel].cpu().numpy())
    return Case(b, m, c, nidx.reshape(b, -1), addend, lambda det: once(det, g), cpu_loop, g, w)


@pytest.mark.parametrize("level", RC.FP_LEVELS, ids=FP_IDS)
def test_fp_level_gradient_at_config_shape(cuda, oracle, level):
    """three_interpolate's gradient with the level's inverse-distance weights (pointnet_util.py:211-216); part_seg FP1 is ONE
    target row per cloud (m = 1) whose two missing neighbours carry weight 0."""
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import three_nn_weights
    label, b, n, m, c = level
    u = torch.from_numpy(_cloud(label, b, n, 1200 + len(label))).to(cuda)
    k = torch.zeros(b, 1, 3, device=cuda) if m == 1 else P.gather_point(u, P.farthest_point_sample(m, u))
    nidx, w = three_nn_weights(u, k)
    _check(_interp_case(P, oracle, (b, m, c), nidx, w, 7, cuda), oracle, {"cpu"}, label + " three_interpolate c=%d" % c)


# ------------------------------------------------------------------------------------------ edges of the envelope / dispatch
def _random_idx(rng, b, n, m, ns, crowd=None):
    idx = rng.integers(0, n, size=(b, m, ns)).astype(np.int32)
    if crowd:                                                       # a few low point numbers collect many references
        idx[:, :, ::3] = rng.integers(0, min(crowd, n), size=idx[:, :, ::3].shape)
    return idx


def _group_check(cuda, oracle, idx_np, n, c, expect, what, seed=1):
    import pointnet2_amd as P
    b = idx_np.shape[0]
    idx = torch.from_numpy(np.ascontiguousarray(idx_np, dtype=np.int32)).to(cuda)
    _check(_group_case(P, oracle, torch.zeros(b, n, c, device=cuda), idx, seed, cuda), oracle, expect, what)


@pytest.mark.parametrize("b,expect", [(3, {"fixed"}), (4, {"cpu"})])
def test_envelope_clouds_3_vs_4(cuda, oracle, b, expect):
    idx = _random_idx(np.random.default_rng(b), b, 700, 90, 16, crowd=8)
    _group_check(cuda, oracle, idx, 700, 24, expect, "b=%d" % b)


@pytest.mark.parametrize("rows,c,expect", [(24576, 3, {"cpu"}), (24577, 3, {"tensor"}), (24576, 16, {"cpu"}),
                                           (24577, 16, {"fixed"})])
def test_envelope_rows_lds_boundary(cuda, oracle, rows, c, expect):
    """rows per cloud = kSegLdsRows and one more: with c < 16 the boundary also moves the call to det_grad.hip"""
    idx = _random_idx(np.random.default_rng(rows + c), 4, rows, 64, 32, crowd=40)
    idx[:, 0, :] = rows - 1                                         # the last row is a target
    _group_check(cuda, oracle, idx, rows, c, expect, "rows=%d c=%d" % (rows, c))


@pytest.mark.parametrize("rows,expect", [(4096, {"cpu"}), (4097, {"fixed"})])
def test_envelope_lds_fit_boundary(cuda, oracle, rows, expect):
    """rows + entries = 36864 (the metric shape's own sum: counters and list fill 144 KiB exactly) and 36865"""
    idx = _random_idx(np.random.default_rng(rows), 4, rows, 1024, 32, crowd=30)
    assert rows + idx.shape[1] * idx.shape[2] in (SEG_FIT_INTS, SEG_FIT_INTS + 1)
    _group_check(cuda, oracle, idx, rows, 16, expect, "rows+entries=%d" % (rows + 32768))


@pytest.mark.parametrize("c", [20, 3])
def test_envelope_sort_tiers(cuda, oracle, c):
    """segments of 32 / 33 entries (one-thread insertion sort / 16-lane rank sort), 128 / 129 (16 lanes / one wave) and
    1024 / 1025 (one wave / not sorted: the fixed-point sum)"""
    rng = np.random.default_rng(c)
    b, n, m, ns = 4, 3000, 160, 32
    special = {10: 32, 11: 33, 12: 128, 13: 129, 14: 1024, 15: 1025}
    idx = np.empty((b, m * ns), np.int32)
    for i in range(b):
        fill = np.concatenate([np.full(k, p, np.int32) for p, k in special.items()])
        rest = rng.integers(16, n, size=m * ns - fill.size).astype(np.int32)
        idx[i] = rng.permutation(np.concatenate([fill, rest]))
    lens = np.bincount(idx[0], minlength=n)
    assert all(lens[p] == k for p, k in special.items())
    _group_check(cuda, oracle, idx.reshape(b, m, ns), n, c, {"cpu", "fixed"}, "sort tiers c=%d" % c)


@pytest.mark.parametrize("b,c,long_row,expect", [(3, 24, False, {"fixed"}), (4, 24, True, {"cpu", "fixed"}), (2, 3, False, {"tensor"})])
def test_reproducible_mode_on_cancelling_segments(cuda, oracle, b, c, long_row, expect):
    """Segments whose two largest addends cancel exactly (+2^20, -2^20) beside addends of ~2^-30: the fixed-point sum keeps
    only multiples of its unit 2^-k, and with the large pair gone the result shows every one of those roundings. With
    normally distributed gradients the unit lies far below the result's own fp32 rounding and a wrong scale goes unseen.
    b = 3: the inversion without LDS (every row fixed point); b = 4: one row of 1100 references beyond the sort beside sorted
    rows; b = 2, c = 3: det_grad.hip, one scale for the call."""
    import pointnet2_amd as P
    rng = np.random.default_rng(b * 10 + c)
    n, m, ns = 200, 64, 48
    idx = rng.integers(0, n, size=(b, m * ns)).astype(np.int32)
    if long_row:
        idx[:, :1100] = 7
        idx = np.stack([rng.permutation(r) for r in idx])
    g = (rng.standard_normal((b, m * ns, c)) * 2.0 ** -30).astype(np.float32)
    for i in range(b):
        order = np.argsort(idx[i], kind="stable")
        first = np.searchsorted(idx[i][order], np.arange(n))
        cnt = np.bincount(idx[i], minlength=n)
        pair = cnt >= 2
        g[i, order[first[pair]]] = 2.0 ** 20
        g[i, order[first[pair] + 1]] = -(2.0 ** 20)
    idx_t = torch.from_numpy(idx.reshape(b, m, ns)).to(cuda)
    g_t = torch.from_numpy(g.reshape(b, m, ns, c)).to(cuda)
    once = _run_modes(lambda leaf: P.group_point(leaf, idx_t), (b, n, c), cuda)
    case = Case(b, n, c, idx_t.reshape(b, -1), g_t.reshape(b, -1, c), lambda det: once(det, g_t),
                lambda sel: oracle.group_point_grad((len(sel), n, c), idx.reshape(b, m, ns)[sel], g.reshape(b, m, ns, c)[sel]), g_t)
    _check(case, oracle, expect, "cancelling segments b=%d c=%d" % (b, c))


@pytest.mark.parametrize("n,m,expect", [(1, 16, {"cpu"}), (2, 16, {"cpu"}), (1, 40, {"fixed"})])
def test_one_and_two_rows_per_cloud(cuda, oracle, n, m, expect):
    """rows per cloud 1 and 2: the fallback of seg_long_blocks (nothing to spread) and rows long enough for the default mode's
    whole-workgroup sums; 1280 references on one row are beyond the sort"""
    idx = np.random.default_rng(n * m).integers(0, n, size=(4, m, 32)).astype(np.int32)
    _group_check(cuda, oracle, idx, n, 64, expect, "rows=%d entries=%d" % (n, m * 32))


@pytest.mark.parametrize("c", [6, 512, 1023, 1024])
def test_channel_counts(cuda, oracle, c):
    """c = 6 (one channel per lane), 512 (both float4s of a lane in one sweep), 1023 (not a multiple of 4: no float4 rows,
    64 lanes, 16 column sweeps), 1024 (two sweeps of two float4s); ball-query-shaped lists with long rows"""
    rng = np.random.default_rng(c)
    b, n, m, ns = 4, 300, 64, 32
    idx = np.empty((b, m, ns), np.int32)
    for i in range(b):
        for j in range(m):
            k = int(rng.integers(1, ns + 1))
            row = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)
            idx[i, j, :k] = row
            idx[i, j, k:] = row[0]                                  # padding repeats the first hit (tf_grouping_g.cu:24-31)
    _group_check(cuda, oracle, idx, n, c, {"cpu"}, "c=%d" % c)


def _abi_group_case(oracle, cuda, b, n, m, ns, c, offset_out, offset_points, seed):
    """group_point's gradient through pn2_group_point_grad_seg with grad_out and/or grad_points 4 bytes past a 16-byte
    boundary (no float4 rows); grad_points starts as NaN so that an element left unwritten fails"""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import seg_workspace
    lib = _C.lib()
    idx_np = _random_idx(np.random.default_rng(seed), b, n, m, ns, crowd=10)
    idx = torch.from_numpy(idx_np).to(cuda)
    g = _grad_out((b, m, ns, c), seed, cuda)
    go_buf = torch.empty(g.numel() + 4, device=cuda)
    go = go_buf[1:1 + g.numel()] if offset_out else go_buf[:g.numel()]
    go.copy_(g.reshape(-1))
    ws = seg_workspace(lib, b, n, m * ns, cuda)

    def run(det):
        gp_buf = torch.full((b * n * c + 4,), float("nan"), device=cuda)
        gp = gp_buf[1:1 + b * n * c] if offset_points else gp_buf[:b * n * c]
        assert (go.data_ptr() % 16 == 4) == offset_out and (gp.data_ptr() % 16 == 4) == offset_points
        _C.check(lib.pn2_group_point_grad_seg(b, n, c, m, ns, go.data_ptr(), idx.data_ptr(), gp.data_ptr(), ws.data_ptr(),
                                              1 if det else 0, torch.cuda.current_stream(cuda).cuda_stream), "group_point_grad")
        torch.cuda.synchronize(cuda)
        return gp.view(b, n, c).clone()

    def cpu_loop(sel):
        return oracle.group_point_grad((len(sel), n, c), idx_np[sel], g[sel].cpu().numpy())
    return Case(b, n, c, idx.reshape(b, -1), g.reshape(b, -1, c), run, cpu_loop, g)


@pytest.mark.parametrize("c", [64, 320])
@pytest.mark.parametrize("where", ["grad_out", "grad_points", "both"])
def test_unaligned_pointers(cuda, oracle, where, c):
    case = _abi_group_case(oracle, cuda, 4, 500, 64, 16, c, where != "grad_points", where != "grad_out", c + len(where))
    _check(case, oracle, {"cpu"}, "unaligned %s c=%d" % (where, c))


def test_no_entries_zero_fill(cuda):
    """m = 0 or nsample = 0 (group_point) and n = 0 (three_interpolate): the gradient is all zeros, both modes"""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import seg_workspace
    lib = _C.lib()
    st = torch.cuda.current_stream(cuda).cuda_stream
    dummy_f = torch.zeros(16, device=cuda)
    dummy_i = torch.zeros(16, dtype=torch.int32, device=cuda)
    b, n, c = 4, 100, 32
    for det in (0, 1):
        for m, ns in ((0, 16), (8, 0)):
            gp = torch.full((b, n, c), float("nan"), device=cuda)
            ws = seg_workspace(lib, b, n, m * ns, cuda)
            _C.check(lib.pn2_group_point_grad_seg(b, n, c, m, ns, dummy_f.data_ptr(), dummy_i.data_ptr(), gp.data_ptr(),
                                                  ws.data_ptr(), det, st), "group_point_grad")
            torch.cuda.synchronize(cuda)
            assert torch.equal(gp.view(torch.int32), torch.zeros_like(gp.view(torch.int32))), (det, m, ns)
        gk = torch.full((b, 10, c), float("nan"), device=cuda)
        ws = seg_workspace(lib, b, 10, 0, cuda)
        _C.check(lib.pn2_three_interpolate_grad_seg(b, 0, c, 10, dummy_f.data_ptr(), dummy_i.data_ptr(), dummy_f.data_ptr(),
                                                    gk.data_ptr(), ws.data_ptr(), det, st), "three_interpolate_grad")
        torch.cuda.synchronize(cuda)
        assert torch.equal(gk.view(torch.int32), torch.zeros_like(gk.view(torch.int32))), det


@pytest.mark.parametrize("m,n,c,expect", [(1, 300, 32, {"cpu"}), (2, 300, 32, {"cpu"}), (1, 600, 32, {"fixed"}),
                                          (2, 600, 32, {"cpu", "fixed"}), (2, 300, 8, {"cpu"})])
def test_interpolate_one_or_two_known_points(cuda, oracle, m, n, c, expect):
    """m = 1 and 2: three_nn's missing neighbours are index 0 with weight 0 (inverse of an infinite distance), so row 0 collects
    every unknown point's third (and second) reference; beyond 1024 of them it is not sorted"""
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import three_nn_weights
    u = torch.from_numpy(S.sphere_clouds(4, n, 60 + m)).to(cuda)
    k = P.gather_point(u, P.farthest_point_sample(m, u)) if m > 1 else u[:, :1].contiguous()
    nidx, w = three_nn_weights(u, k)
    assert bool((w[:, :, 2] == 0).all()) and (m == 1) == bool((w[:, :, 1] == 0).all())
    _check(_interp_case(P, oracle, (4, m, c), nidx, w, m * n + c, cuda), oracle, expect, "three_interpolate m=%d n=%d c=%d" % (m, n, c))


# ------------------------------------------------------------------------------------- bench.py's gradient rows, as it calls them
def _bench_group_inputs(cuda, b, n, m, r, ns, c, seed):
    import pointnet2_amd as P
    xyz = torch.from_numpy(S.sphere_clouds(b, n, seed)).to(cuda)
    _, new_xyz = P.farthest_point_sample_gather(m, xyz)
    idx, _ = P.query_ball_point(r, ns, xyz, new_xyz)
    pts = torch.randn(b, n, c, device=cuda)
    return idx, P.group_point(pts, idx)                             # bench's grad_out is the forward's output buffer


@pytest.mark.parametrize("b,n,m,r,ns,c,seed", [(32, 512, 128, 0.4, 64, 128, 31), (32, 512, 128, 0.8, 128, 320, 32)],
                         ids=["group_point_c128_cls_ssg_L2_grad", "group_point_c320_cls_msg_L2_grad"])
def test_bench_group_point_grad_rows(cuda, b, n, m, r, ns, c, seed):
    """pn2_group_point_grad_seg exactly as the benchmark's gradient rows time it: C ABI, one preallocated workspace reused by
    every call, deterministic = 0; every call's output against the float64 scatter-add"""
    from pointnet2_amd import _C
    lib = _C.lib()
    idx, out = _bench_group_inputs(cuda, b, n, m, r, ns, c, seed)
    ws = torch.empty(((lib.pn2_seg_grad_ws_bytes(b, n, m * ns) + 7) // 8,), dtype=torch.int64, device=cuda)
    ref = _reference(n, idx.reshape(b, -1), out.reshape(b, -1, c))
    st = torch.cuda.current_stream(cuda).cuda_stream
    for call in range(3):
        gp = torch.full((b, n, c), float("nan"), device=cuda)
        _C.check(lib.pn2_group_point_grad_seg(b, n, c, m, ns, out.data_ptr(), idx.data_ptr(), gp.data_ptr(), ws.data_ptr(), 0, st),
                 "group_point_grad")
        torch.cuda.synchronize(cuda)
        _assert_bound(gp, ref, "bench row c=%d call %d" % (c, call))


def test_bench_three_interpolate_grad_row(cuda):
    """pn2_three_interpolate_grad_seg at sem_seg FP4 as the benchmark calls it (known = the first m unknown points, weights
    1 / clamp(dist) normalised, grad_out = the forward's output buffer, one workspace, deterministic = 0)"""
    import pointnet2_amd as P
    from pointnet2_amd import _C
    lib = _C.lib()
    b, n, m, c = 8, 8192, 1024, 128
    unknown = torch.from_numpy(S.uniform_clouds(b, n, 91)).to(cuda)
    known = unknown[:, :m].contiguous()
    dist, idx = P.three_nn(unknown, known)
    w = 1.0 / torch.clamp(dist, min=1e-10)
    w = (w / w.sum(dim=2, keepdim=True)).contiguous()
    pts = torch.randn(b, m, c, device=cuda)
    out = P.three_interpolate(pts, idx, w)
    ws = torch.empty(((lib.pn2_seg_grad_ws_bytes(b, m, 3 * n) + 7) // 8,), dtype=torch.int64, device=cuda)
    ref = _reference(m, idx.reshape(b, -1), (out[:, :, None, :] * w[:, :, :, None]).reshape(b, 3 * n, c))
    st = torch.cuda.current_stream(cuda).cuda_stream
    for call in range(3):
        gp = torch.full((b, m, c), float("nan"), device=cuda)
        _C.check(lib.pn2_three_interpolate_grad_seg(b, n, c, m, out.data_ptr(), idx.data_ptr(), w.data_ptr(), gp.data_ptr(),
                                                    ws.data_ptr(), 0, st), "three_interpolate_grad")
        torch.cuda.synchronize(cuda)
        _assert_bound(gp, ref, "bench row three_interpolate call %d" % call)
