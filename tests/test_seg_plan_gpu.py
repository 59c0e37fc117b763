"""Index plans through the C ABI (include/pn2ops.h "index plans", csrc/seg_grad.hip) on the GPU: the contents of a built plan
against numpy, the planned gradients against the unplanned ones (reproducible mode: bit for bit) and against a float64 scatter
(default mode: the bound of tests/test_det_grad_gpu.py's segmented test), the two walks of the default mode's long-row part
against each other, and a plan's bytes before and after the gradients that read it.

Shapes: the smallest that reach every branch of the inversion's host logic (which kernel builds the plan). Index patterns: what
decides where the long rows are (the stride walk assumes the low point numbers; the table walk assumes nothing). Channel counts:
every lane layout of the reduce kernels."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# name: (b, rows, groups, group size): entries = groups * size
GROUP_SHAPES = {
    "A": (4, 500, 70, 16),        # LDS list, KEEP = 1
    "B": (4, 1024, 625, 32),      # LDS list, KEEP = 3
    "C": (4, 600, 625, 64),       # counters in LDS, list global
    "D": (3, 500, 70, 16),        # b < 4: count / scan / fill
    "E": (4, 25000, 94, 32),      # rows > 24576: count / scan / fill
}
# (b, n unknown, m known): rows = m, entries = 3 n
INTERP_SHAPES = {"I": (4, 700, 90), "J": (3, 700, 90), "K": (4, 64, 2)}
PATTERNS = ("uniform", "padded", "third", "congruent", "big")
CHANNELS = (3, 16, 64, 128, 130, 256, 320)


def _lib():
    from pointnet2_amd import _C
    return _C.lib()


def _check(rc):
    from pointnet2_amd import _C
    _C.check(rc, "seg plan test")


def _long_rule(rows, entries, c, out_rows):
    lf, lb = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib().pn2_seg_grad_plan(rows, entries, c, out_rows, ctypes.byref(lf), ctypes.byref(lb)) == 0
    return lf.value, lb.value


def _targets(pattern, b, rows, groups, size, seed):
    """(b, groups * size) int32 target rows, or None where the shape cannot hold the pattern."""
    rng = np.random.default_rng(seed)
    entries = groups * size
    t = rng.integers(0, rows, size=(b, groups, size)).astype(np.int32)
    if pattern == "uniform":
        pass
    elif pattern == "padded":
        # ball-query lists: k hits ascending, then the FIRST hit repeated; first hits at the low row numbers (tf_grouping_g.cu:24-31)
        low = max(1, rows // 40)
        first = rng.integers(0, low, size=(b, groups, 1))
        rest = np.sort(rng.integers(first + 1 if rows > 1 else 0, max(rows, 2), size=(b, groups, size)) % rows, axis=2)
        k = rng.integers(1, size + 1, size=(b, groups, 1))
        pos = np.arange(size).reshape(1, 1, size)
        t = np.where((pos == 0) | (pos >= k), first, rest).astype(np.int32)
    elif pattern == "third":
        hot, dead = 11 % rows, 5 % rows
        if dead == hot:
            dead = (hot + 1) % rows
        t = t.reshape(b, entries)
        t[:, ::3] = hot                                            # a third of all references on one row ...
        t[t == dead] = hot                                         # ... and a row nobody references
    elif pattern == "congruent":
        # long rows ONLY at flat row numbers congruent modulo the stride of the stride walk: all of them are one workgroup's
        long_from, stride = _long_rule(rows, entries, 128, b * rows)
        t = t.reshape(b, entries)
        for i in range(b):
            own = np.array([r for r in range(rows) if (i * rows + r) % stride == 0] or [0], dtype=np.int32)
            t[i, : entries // 2] = own[np.arange(entries // 2) % len(own)]
            cnt = np.bincount(t[i], minlength=rows)
            stray = (cnt >= long_from) & ~np.isin(np.arange(rows), own)
            t[i, stray[t[i]]] = own[0]
    elif pattern == "big":
        if entries < 1100:
            return None
        t = t.reshape(b, entries)
        t[:, 10:1110] = 3 % rows                                   # one row with more than 1024 references: beyond the sorted envelope
    return np.ascontiguousarray(t.reshape(b, entries))


class _Case:
    """One (shape, pattern): the index tensor on the device, both plans, and what numpy knows about them."""

    def __init__(self, kind, name, pattern, dev):
        self.kind, self.dev = kind, dev
        if kind == "group":
            self.b, self.rows, self.groups, self.size = GROUP_SHAPES[name]
            self.src_div = 1
        else:
            self.b, n, self.rows = INTERP_SHAPES[name]
            self.groups, self.size, self.src_div = n, 3, 3
        self.entries = self.groups * self.size
        t = _targets(pattern, self.b, self.rows, self.groups, self.size, seed=sum(map(ord, name + pattern)))
        assert t is not None
        self.t = t
        self.idx = torch.from_numpy(t).to(dev)
        self.cnt = np.stack([np.bincount(t[i], minlength=self.rows) for i in range(self.b)])
        self.weight = torch.rand((self.b, self.entries), device=dev) if kind == "interpolate" else None
        lib = _lib()
        self.nbytes = lib.pn2_seg_plan_bytes(self.b, self.rows, self.entries)
        self.plans = {}
        for srt in (0, 1):
            plan = torch.full(((self.nbytes + 3) // 4,), -0x55555556, dtype=torch.int32, device=dev)    # a build may rely on no initial value
            self.build(plan, srt)
            self.plans[srt] = plan
        torch.cuda.synchronize(dev)
        self.snapshot = {s: p.clone() for s, p in self.plans.items()}

    def build(self, plan, srt):
        lib = _lib()
        if self.kind == "group":
            _check(lib.pn2_group_point_plan(self.b, self.rows, self.groups, self.size, self.idx.data_ptr(), srt, plan.data_ptr(), None))
        else:
            _check(lib.pn2_three_interpolate_plan(self.b, self.groups, self.rows, self.idx.data_ptr(), srt, plan.data_ptr(), None))

    def grad_out(self, c, seed=0):
        g = torch.Generator(device=self.dev)
        g.manual_seed(1000 * c + seed)
        srows = self.entries // self.src_div
        v = torch.randn((self.b, srows, c), device=self.dev, generator=g)
        scale = 10.0 ** torch.randint(-3, 3, (self.b, srows, 1), device=self.dev, generator=g).float()
        return (v * scale).contiguous()

    def planned(self, c, go, srt, det, variant=None, out=None):
        lib = _lib()
        out = torch.full((self.b, self.rows, c), float("nan"), device=self.dev) if out is None else out
        plan = self.plans[srt].data_ptr()
        if self.kind == "group":
            if variant is None:
                _check(lib.pn2_group_point_grad_planned(self.b, self.rows, c, self.groups, self.size, go.data_ptr(), plan, out.data_ptr(), det, None))
            else:
                _check(lib.pn2_group_point_grad_planned_ex(self.b, self.rows, c, self.groups, self.size, go.data_ptr(), plan, out.data_ptr(),
                                                           det, variant, None))
        elif variant is None:
            _check(lib.pn2_three_interpolate_grad_planned(self.b, self.groups, c, self.rows, go.data_ptr(), plan, self.weight.data_ptr(),
                                                          out.data_ptr(), det, None))
        else:
            _check(lib.pn2_three_interpolate_grad_planned_ex(self.b, self.groups, c, self.rows, go.data_ptr(), plan, self.weight.data_ptr(),
                                                             out.data_ptr(), det, variant, None))
        return out

    def unplanned(self, c, go, det):
        lib = _lib()
        out = torch.full((self.b, self.rows, c), float("nan"), device=self.dev)
        ws = torch.empty(((lib.pn2_seg_grad_ws_bytes(self.b, self.rows, self.entries) + 7) // 8,), dtype=torch.int64, device=self.dev)
        if self.kind == "group":
            _check(lib.pn2_group_point_grad_seg(self.b, self.rows, c, self.groups, self.size, go.data_ptr(), self.idx.data_ptr(), out.data_ptr(),
                                                ws.data_ptr(), det, None))
        else:
            _check(lib.pn2_three_interpolate_grad_seg(self.b, self.groups, c, self.rows, go.data_ptr(), self.idx.data_ptr(),
                                                      self.weight.data_ptr(), out.data_ptr(), ws.data_ptr(), det, None))
        return out

    def exact(self, c, go):
        """float64 scatter of the fp32 addends (three_interpolate: the products rounded to fp32, as the operator forms them) and of
        their magnitudes."""
        src = torch.arange(self.entries, device=self.dev) // self.src_div
        add = go[:, src, :]
        if self.weight is not None:
            add = add * self.weight.unsqueeze(2)
        add = add.double()
        # fp64 atomics on ONE address serialise (a row with a third of all references): spread every row over `fold` slots first
        fold = 64 if self.rows <= 2048 else 1
        slot = (self.idx.long() + self.rows * (torch.arange(self.entries, device=self.dev) % fold)).contiguous()
        want = torch.zeros((self.b, fold * self.rows, c), dtype=torch.float64, device=self.dev)
        mag = torch.zeros_like(want)
        for i in range(self.b):
            want[i].index_add_(0, slot[i], add[i])
            mag[i].index_add_(0, slot[i], add[i].abs())
        want = want.view(self.b, fold, self.rows, c).sum(dim=1)
        mag = mag.view(self.b, fold, self.rows, c).sum(dim=1)
        return want, mag


@functools.lru_cache(maxsize=None)
def _case(kind, name, pattern, dev_index):
    return _Case(kind, name, pattern, torch.device("cuda", dev_index))


def _cases():
    out = []
    for name, (b, rows, groups, size) in GROUP_SHAPES.items():
        out += [("group", name, p) for p in PATTERNS if p != "big" or groups * size >= 1100]
    for name, (b, n, m) in INTERP_SHAPES.items():
        out += [("interpolate", name, p) for p in PATTERNS if p != "big" or 3 * n >= 1100]
    return out


CASES = _cases()


def _get(cuda, kind, name, pattern):
    return _case(kind, name, pattern, cuda.index if cuda.index is not None else torch.cuda.current_device())


@pytest.mark.parametrize("kind,name,pattern", CASES)
def test_plan_contents(cuda, kind, name, pattern):
    """start = the exclusive scan of the counts; every segment of list holds exactly the entries that name its row, ascending where
    the row is flagged sorted; the table holds exactly the rows of long_from references or more."""
    cs = _get(cuda, kind, name, pattern)
    off = (ctypes.c_longlong * 5)()
    lf, cap = ctypes.c_int(0), ctypes.c_longlong(0)
    assert _lib().pn2_seg_plan_layout(cs.b, cs.rows, cs.entries, off, ctypes.byref(lf), ctypes.byref(cap)) == 0
    assert lf.value == _long_rule(cs.rows, cs.entries, 64, cs.b * cs.rows)[0]
    b, rows, entries, cap = cs.b, cs.rows, cs.entries, cap.value
    order = np.argsort(cs.t, axis=1, kind="stable")                        # entries by target row, ascending inside a row
    want_start = np.concatenate([np.zeros((b, 1), np.int64), np.cumsum(cs.cnt, axis=1)], axis=1)
    envelope = b >= 4 and rows <= 24576 and rows + entries <= 36864       # where a sorted build sorts (include/pn2ops.h)
    for srt in (0, 1):
        words = cs.plans[srt].cpu().numpy()

        def part(k, count):
            return words[off[k] // 4: off[k] // 4 + count]

        start = part(0, b * (rows + 1)).reshape(b, rows + 1)
        flags = part(1, b * rows).reshape(b, rows)
        lst = part(2, b * entries).reshape(b, entries)
        long_count = part(3, b)
        long_rows = part(4, b * cap).reshape(b, cap)
        assert np.array_equal(start, want_start)
        assert np.array_equal(np.sort(lst, axis=1), np.broadcast_to(np.arange(entries), (b, entries)))      # a permutation per cloud
        assert np.array_equal(np.take_along_axis(cs.t, lst, axis=1), np.sort(cs.t, axis=1))                 # grouped by row
        if srt and envelope:
            assert np.array_equal(flags != 0, cs.cnt <= 1024)
        else:
            assert not flags.any()
        in_sorted_row = np.repeat(flags.reshape(-1) != 0, cs.cnt.reshape(-1)).reshape(b, entries)           # per list position
        assert np.array_equal(lst[in_sorted_row], order[in_sorted_row])
        for i in range(b):
            want_long = np.flatnonzero(cs.cnt[i] >= lf.value)
            assert long_count[i] == len(want_long) <= cap
            assert np.array_equal(np.sort(long_rows[i, : long_count[i]]), want_long)


@pytest.mark.parametrize("kind,name,pattern", CASES)
def test_planned_gradients(cuda, kind, name, pattern):
    """Every channel count: the reproducible mode from a sorted plan is the unplanned reproducible gradient bit for bit; the default
    mode is within the sequential-sum bound of the float64 scatter, the same bits from both walks and on every call, exactly
    zero on unreferenced rows; and the plans' bytes are what they were before."""
    cs = _get(cuda, kind, name, pattern)
    empty = torch.from_numpy(cs.cnt == 0).to(cuda)
    cnt = torch.from_numpy(np.maximum(cs.cnt, 2).astype(np.float64)).to(cuda).unsqueeze(2)
    for c in CHANNELS:
        go = cs.grad_out(c)
        # reproducible mode
        ref = cs.unplanned(c, go, 1)
        got = cs.planned(c, go, 1, 1)
        assert torch.equal(got, ref), (c, "reproducible")
        loose = cs.planned(c, go, 0, 1)                                    # unsorted plan: fixed point on every row, still reproducible
        assert torch.equal(loose, cs.planned(c, go, 0, 1)), (c, "reproducible from an unsorted plan")
        # default mode
        want, mag = cs.exact(c, go)
        tol = mag * 2.0 ** -24 * cnt + 1e-30
        v1 = cs.planned(c, go, 0, 0, variant=1)
        v2 = cs.planned(c, go, 0, 0, variant=2)
        v0 = cs.planned(c, go, 0, 0)
        again = cs.planned(c, go, 0, 0)
        err = (v0.double() - want).abs()
        print("%s %s %s c=%d: max err / bound = %.3f" % (kind, name, pattern, c, float((err / tol).max())))
        assert bool((err <= tol).all()), (c, "default")
        assert torch.equal(v1, v2), (c, "stride walk vs table walk")
        assert torch.equal(v0, v2) and torch.equal(v0, again), (c, "default, call to call")
        assert bool((((loose.double() - want).abs()) <= tol).all()), (c, "fixed point")
        if empty.any():
            assert torch.count_nonzero(v0[empty]) == 0 and torch.count_nonzero(got[empty]) == 0
        # a sorted plan serves the default mode too
        s0 = cs.planned(c, go, 1, 0)
        assert bool(((s0.double() - want).abs() <= tol).all()), (c, "default from a sorted plan")
    torch.cuda.synchronize(cuda)
    for srt in (0, 1):
        assert torch.equal(cs.plans[srt], cs.snapshot[srt]), "a gradient call wrote into its plan"


@pytest.mark.parametrize("kind,name", [("group", "A"), ("interpolate", "I")])
def test_one_plan_two_gradients(cuda, kind, name):
    """What the training node with coordinate gradients does: a 3-channel and a 64-channel reduction from the same plan."""
    cs = _get(cuda, kind, name, "padded")
    g3, g64 = cs.grad_out(3, seed=5), cs.grad_out(64, seed=5)
    a3, a64 = cs.planned(3, g3, 1, 1), cs.planned(64, g64, 1, 1)
    assert torch.equal(a3, cs.unplanned(3, g3, 1))
    assert torch.equal(a64, cs.unplanned(64, g64, 1))
    assert torch.equal(cs.plans[1], cs.snapshot[1])


@pytest.mark.parametrize("kind,name", [("group", "B"), ("interpolate", "I")])
def test_unaligned_gradient(cuda, kind, name):
    """grad_out 4 bytes past a 16-byte boundary: the scalar-lane kernels, same values."""
    cs = _get(cuda, kind, name, "third")
    c = 64
    go = cs.grad_out(c)
    flat = torch.empty(go.numel() + 4, device=cuda)
    shifted = flat[1: 1 + go.numel()].view(go.shape)
    assert shifted.data_ptr() % 16 == 4
    shifted.copy_(go)
    assert torch.equal(cs.planned(c, shifted, 1, 1), cs.unplanned(c, go, 1))
    want, mag = cs.exact(c, go)
    cnt = torch.from_numpy(np.maximum(cs.cnt, 2).astype(np.float64)).to(cuda).unsqueeze(2)
    got = cs.planned(c, shifted, 0, 0)
    assert bool(((got.double() - want).abs() <= mag * 2.0 ** -24 * cnt + 1e-30).all())
    assert torch.equal(got, cs.planned(c, shifted, 0, 0, variant=1))


def test_rebuilding_into_the_same_memory(cuda):
    """A plan is rebuilt in place when idx is rewritten (a static geometry's copy_ / a captured build)."""
    cs = _get(cuda, "group", "A", "uniform")
    other = _Case("group", "A", "third", cuda)
    other.build(cs.plans[1], 1)                                           # cs.idx -> other.idx, same memory
    try:
        go = other.grad_out(64)
        saved, other.plans[1] = other.plans[1], cs.plans[1]
        assert torch.equal(other.planned(64, go, 1, 1), other.unplanned(64, go, 1))
        other.plans[1] = saved
    finally:
        cs.build(cs.plans[1], 1)
        torch.cuda.synchronize(cuda)


def test_argument_errors_and_empty_shapes(cuda):
    lib = _lib()
    cs = _get(cuda, "group", "A", "uniform")
    b, n, m, ns, c = cs.b, cs.rows, cs.groups, cs.size, 16
    go = cs.grad_out(c)
    out = torch.full((b, n, c), 7.0, device=cuda)
    plan = cs.plans[1].data_ptr()
    assert lib.pn2_group_point_grad_planned(b, n, c, m, ns, go.data_ptr(), None, out.data_ptr(), 0, None) == -1
    assert lib.pn2_group_point_grad_planned(b, n, 0, m, ns, go.data_ptr(), plan, out.data_ptr(), 0, None) == -2
    assert lib.pn2_group_point_grad_planned(b, -n, c, m, ns, go.data_ptr(), plan, out.data_ptr(), 0, None) == -2
    assert lib.pn2_group_point_grad_planned(b, n, c, -m, ns, go.data_ptr(), plan, out.data_ptr(), 0, None) == -2
    assert lib.pn2_group_point_grad_planned_ex(b, n, c, m, ns, go.data_ptr(), plan, out.data_ptr(), 0, 3, None) == -3
    assert lib.pn2_three_interpolate_grad_planned(b, 10, c, 0, go.data_ptr(), plan, go.data_ptr(), out.data_ptr(), 0, None) == -2
    assert lib.pn2_three_interpolate_grad_planned(b, 10, c, 5, go.data_ptr(), None, go.data_ptr(), out.data_ptr(), 0, None) == -1
    assert lib.pn2_group_point_plan(b, n, m, ns, cs.idx.data_ptr(), 0, None, None) == -1
    assert lib.pn2_three_interpolate_plan(b, 10, 0, cs.idx.data_ptr(), 0, plan, None) == -2
    torch.cuda.synchronize(cuda)
    assert bool((out == 7.0).all())                                        # nothing was launched
    assert lib.pn2_group_point_grad_planned(0, n, c, m, ns, None, None, None, 0, None) == 0
    assert lib.pn2_three_interpolate_grad_planned(0, 10, c, 5, None, None, None, None, 0, None) == 0
    assert bool((out == 7.0).all())
    # no references: the output is zero-filled and no plan is read
    _check(lib.pn2_group_point_grad_planned(b, n, c, 0, ns, None, None, out.data_ptr(), 0, None))
    assert torch.count_nonzero(out) == 0
    out.fill_(7.0)
    _check(lib.pn2_three_interpolate_grad_planned(b, 0, c, n, None, None, None, out.data_ptr(), 1, None))
    assert torch.count_nonzero(out) == 0
