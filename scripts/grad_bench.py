"""Gradient kernels: fp32-atomic scatter-add vs the reproducible fixed-point variant (pn2_*_grad_det).
Algorithmic bytes = grad_out read once + result written once. Development / measurement aid.

--plans [--baseline-lib PATH] [--out FILE]: the index-plan columns (include/pn2ops.h "index plans") at the rows DESIGN.md 4.3
quotes: pn2_*_grad_seg (inversion + reduce), the plan build alone, the planned reduce alone (the library's choice, the stride
walk, the table walk), both modes; and the same from another build of the library (--baseline-lib: the parent commit's, for a
comparison inside one session). Every figure is the median of --rounds windows of --iters calls, the variants taking turns."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import pointnet2_amd as P
from pointnet2_amd import _C
from pointnet2_amd._tensors import det_workspace, seg_workspace

dev = torch.device("cuda:0")
L = _C.lib()


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def group_case(name, b, n, c, m, ns, r):
    xyz = torch.rand(b, n, 3, device=dev)
    q = P.gather_point(xyz, P.farthest_point_sample(m, xyz))
    idx, _ = P.query_ball_point(r, ns, xyz, q)
    g = torch.randn(b, m, ns, c, device=dev)
    out = torch.empty(b, n, c, device=dev)
    ws = det_workspace(L, b, n, c, dev)
    t0 = timeit(lambda: L.pn2_group_point_grad(b, n, c, m, ns, g.data_ptr(), idx.data_ptr(), out.data_ptr(), None))
    t1 = timeit(lambda: L.pn2_group_point_grad_det(b, n, c, m, ns, g.data_ptr(), idx.data_ptr(), out.data_ptr(), ws.data_ptr(), None))
    byt = 4.0 * (g.numel() + out.numel())
    ws2 = seg_workspace(L, b, n, m * ns, dev)
    t2 = timeit(lambda: L.pn2_group_point_grad_seg(b, n, c, m, ns, g.data_ptr(), idx.data_ptr(), out.data_ptr(), ws2.data_ptr(), 0, None))
    t3 = timeit(lambda: L.pn2_group_point_grad_seg(b, n, c, m, ns, g.data_ptr(), idx.data_ptr(), out.data_ptr(), ws2.data_ptr(), 1, None))
    print("%-46s atomics %7.1f us (%5.0f GB/s) | fixed-point atomics %7.1f | segmented %7.1f us (%5.0f GB/s) | segmented reproducible %7.1f us (%5.0f GB/s)"
          % (name, t0, byt / t0 / 1e3, t1, t2, byt / t2 / 1e3, t3, byt / t3 / 1e3), flush=True)


def interp_case(name, b, n, c, m):
    xyz1, xyz2 = torch.rand(b, n, 3, device=dev), torch.rand(b, m, 3, device=dev)
    d, idx = P.three_nn(xyz1, xyz2)
    w = torch.rand(b, n, 3, device=dev)
    g = torch.randn(b, n, c, device=dev)
    out = torch.empty(b, m, c, device=dev)
    ws = det_workspace(L, b, m, c, dev)
    t0 = timeit(lambda: L.pn2_three_interpolate_grad(b, n, c, m, g.data_ptr(), idx.data_ptr(), w.data_ptr(), out.data_ptr(), None))
    t1 = timeit(lambda: L.pn2_three_interpolate_grad_det(b, n, c, m, g.data_ptr(), idx.data_ptr(), w.data_ptr(), out.data_ptr(), ws.data_ptr(), None))
    byt = 4.0 * (g.numel() + out.numel())
    ws2 = seg_workspace(L, b, m, 3 * n, dev)
    t2 = timeit(lambda: L.pn2_three_interpolate_grad_seg(b, n, c, m, g.data_ptr(), idx.data_ptr(), w.data_ptr(), out.data_ptr(), ws2.data_ptr(), 0, None))
    t3 = timeit(lambda: L.pn2_three_interpolate_grad_seg(b, n, c, m, g.data_ptr(), idx.data_ptr(), w.data_ptr(), out.data_ptr(), ws2.data_ptr(), 1, None))
    print("%-46s atomics %7.1f us (%5.0f GB/s) | fixed-point atomics %7.1f | segmented %7.1f us (%5.0f GB/s) | segmented reproducible %7.1f us (%5.0f GB/s)"
          % (name, t0, byt / t0 / 1e3, t1, t2, byt / t2 / 1e3, t3, byt / t3 / 1e3), flush=True)


# ---- index plans ---------------------------------------------------------------------------------------------------------------
def _window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def _take_turns(calls, iters, rounds):
    """calls: {name: fn} -> {name: [us per call of every round]}; the variants alternate inside a round."""
    for fn in calls.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            times[k].append(_window(fn, iters))
    return times


def _congruent_idx(b, n, m, ns, c):
    """Long rows only at flat row numbers congruent modulo the stride walk's stride: its worst case (tests/test_seg_plan_gpu.py)."""
    import numpy as np
    lf, lb = ctypes.c_int(0), ctypes.c_int(0)
    L.pn2_seg_grad_plan(n, m * ns, c, b * n, ctypes.byref(lf), ctypes.byref(lb))
    rng = np.random.default_rng(0)
    t = rng.integers(0, n, size=(b, m * ns)).astype(np.int32)
    for i in range(b):
        own = np.array([r for r in range(n) if (i * n + r) % lb.value == 0] or [0], dtype=np.int32)
        t[i, : m * ns // 2] = own[np.arange(m * ns // 2) % len(own)]
        cnt = np.bincount(t[i], minlength=n)
        stray = (cnt >= lf.value) & ~np.isin(np.arange(n), own)
        t[i, stray[t[i]]] = own[0]
    return torch.from_numpy(t.reshape(b, m, ns)).to(dev)


def plan_case(name, kind, b, n, c, m, ns, r, base, args, log, idx=None):
    """kind "group": points (b,n,c) <- (m,ns); "interp": known (b,m,c) <- n unknown points."""
    if kind == "group":
        if idx is None:
            xyz = torch.rand(b, n, 3, device=dev)
            idx, _ = P.query_ball_point(r, ns, xyz, P.gather_point(xyz, P.farthest_point_sample(m, xyz)))
        rows, entries = n, m * ns
        g = torch.randn(b, m, ns, c, device=dev)
        w = None
    else:
        _, idx = P.three_nn(torch.rand(b, n, 3, device=dev), torch.rand(b, m, 3, device=dev))
        rows, entries = m, 3 * n
        g = torch.randn(b, n, c, device=dev)
        w = torch.rand(b, n, 3, device=dev)
    out = torch.empty(b, rows, c, device=dev)
    ws = seg_workspace(L, b, rows, entries, dev)
    plans = {d: torch.empty(((L.pn2_seg_plan_bytes(b, rows, entries) + 3) // 4,), dtype=torch.int32, device=dev) for d in (0, 1)}
    gp, ip, op, wsp, wp = g.data_ptr(), idx.data_ptr(), out.data_ptr(), ws.data_ptr(), (w.data_ptr() if w is not None else None)

    def seg(lib, det):
        if kind == "group":
            return lambda: lib.pn2_group_point_grad_seg(b, n, c, m, ns, gp, ip, op, wsp, det, None)
        return lambda: lib.pn2_three_interpolate_grad_seg(b, n, c, m, gp, ip, wp, op, wsp, det, None)

    def build(det):
        pp = plans[det].data_ptr()
        if kind == "group":
            return lambda: L.pn2_group_point_plan(b, n, m, ns, ip, det, pp, None)
        return lambda: L.pn2_three_interpolate_plan(b, n, m, ip, det, pp, None)

    def planned(det, variant):
        pp = plans[det].data_ptr()
        if kind == "group":
            return lambda: L.pn2_group_point_grad_planned_ex(b, n, c, m, ns, gp, pp, op, det, variant, None)
        return lambda: L.pn2_three_interpolate_grad_planned_ex(b, n, c, m, gp, pp, wp, op, det, variant, None)

    for det in (0, 1):
        assert build(det)() == 0
        calls = {}
        if base is not None:
            calls["parent seg"] = seg(base, det)
        calls["seg"] = seg(L, det)
        calls["build"] = build(det)
        calls["planned"] = planned(det, 0)
        if det == 0:
            calls["stride walk"] = planned(0, 1)
            calls["table walk"] = planned(0, 2)
            calls["table walk again"] = planned(0, 2)             # the spread of two runs of the same variant
        for fn in calls.values():
            assert fn() == 0
        times = _take_turns(calls, args.iters, args.rounds)
        med = {k: statistics.median(v) for k, v in times.items()}
        line = "%-44s %-12s " % (name, "reproducible" if det else "default") + " | ".join("%s %6.1f" % (k, v) for k, v in med.items())
        if base is not None:
            line += " | accept planned <= parent - build / 2 = %.1f: %s" % (med["parent seg"] - 0.5 * med["build"],
                                                                           "yes" if med["planned"] <= med["parent seg"] - 0.5 * med["build"] else "NO")
        print(line, flush=True)
        if log is not None:
            log.write(line + "\n")
            for k, v in times.items():
                log.write("    %-18s %s\n" % (k, " ".join("%.2f" % x for x in v)))
            log.flush()


def plan_rows(args):
    base = None
    if args.baseline_lib:
        base = ctypes.CDLL(args.baseline_lib)                          # (int arguments and pointers as Python ints: set the pointer types)
        vp, i = ctypes.c_void_p, ctypes.c_int
        base.pn2_group_point_grad_seg.argtypes = [i, i, i, i, i, vp, vp, vp, vp, i, vp]
        base.pn2_three_interpolate_grad_seg.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, i, vp]
    log = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        log = open(args.out, "w")
        log.write("# us per call, median of %d windows of %d calls (raw windows indented below each row); %s\n"
                  % (args.rounds, args.iters, _C.version()))
    plan_case("group_grad cls_ssg L2 (32,512,128)<-(128,64)", "group", 32, 512, 128, 128, 64, 0.4, base, args, log)
    plan_case("group_grad cls_msg L2 (32,512,320)<-(128,128)", "group", 32, 512, 320, 128, 128, 0.8, base, args, log)
    plan_case("interp_grad sem_seg FP4 (8,1024,128)<-8192", "interp", 8, 8192, 128, 1024, 0, 0.0, base, args, log)
    plan_case("group_grad congruent rows (32,512,128)<-(128,64)", "group", 32, 512, 128, 128, 64, 0.4, base, args, log,
              idx=_congruent_idx(32, 512, 128, 64, 128))
    plan_case("group_grad metric xyz (32,4096,3)<-(1024,32)", "group", 32, 4096, 3, 1024, 32, 0.2, base, args, log)
    if log is not None:
        log.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", action="store_true")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.plans:
        plan_rows(args)
        sys.exit(0)
    group_case("group_grad metric xyz (32,4096,3)<-(1024,32)", 32, 4096, 3, 1024, 32, 0.2)
    group_case("group_grad cls_ssg L2 (32,512,128)<-(128,64)", 32, 512, 128, 128, 64, 0.4)
    group_case("group_grad (32,4096,128)<-(1024,32)", 32, 4096, 128, 1024, 32, 0.2)
    group_case("group_grad cls_msg L2 (32,512,320)<-(128,128)", 32, 512, 320, 128, 128, 0.8)
    interp_case("interp_grad sem_seg FP4 (8,1024,128)<-8192", 8, 8192, 128, 1024)
    interp_case("interp_grad part_seg FP3 (16,512,128)<-2048", 16, 2048, 128, 512)
