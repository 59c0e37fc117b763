"""The two-sided ragged entries (pn2_*_ragged_counts / pn2_*_ragged_pair) against their one-sided twins, same process, same
tensors. Measurement aid; needs the GPU.

    python scripts/ragged_pair_bench.py [--samples 20] [--reps 3] [--inner 10] [--parent-lib libpn2ops.so] [--json FILE]

Method (that of scripts/ragged_msg_bench.py): the C entries are called directly on preallocated outputs; one SAMPLE is `inner`
back-to-back calls of a route between two device events, divided by `inner`; one repetition of a route is the MEDIAN of
`samples` samples behind a warm-up; the routes of a shape ALTERNATE, `reps` repetitions each. Reported per route: the median of
its repetitions' medians and their spread (min .. max). A difference smaller than the spread is not a difference.

--parent-lib: a second build of the library (the parent commit's) whose ONE-SIDED ragged entries are the baseline; without it
the baseline is this library's own one-sided entries.

Per operator (FPS, single- and multi-radius ball query, kNN, three_nn) and shape (reference_configs.py: cls_msg level 1 at
b 32, sem_seg SA1 / FP4 at b 8):
  (a) full counts: the pair entry with every count at its maximum against the one-sided entry; outputs compared bit for bit
      first.
  (b) the pair entry with lengths uniform in n/2 .. n and counts uniform in m/2 .. m (seed fixed), against (a)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import pointnet2_amd as P
from pointnet2_amd import _C
from pointnet2_amd import synthetic as S
from pointnet2_amd._tensors import stream_ptr

#          title, b, n, m, scales [(radius, nsample)], k of kNN
SA_SHAPES = [("cls_msg level 1", 32, 4096, 512, [(0.1, 16), (0.2, 32), (0.4, 128)], 32),
             ("sem_seg SA1", 8, 8192, 1024, [(0.1, 32)], 32)]
#          title, b, unknown n, known m
FP_SHAPES = [("cls_msg level 1 as an FP level", 32, 4096, 512), ("sem_seg FP4", 8, 8192, 1024)]


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("pn2_farthest_point_sample_ragged", "pn2_query_ball_group_xyz_ragged", "pn2_query_ball_group_xyz_msg_ragged",
                 "pn2_knn_point_ragged", "pn2_three_nn_ragged"):
        getattr(lib, name).argtypes = _C._SIGNATURES[name]
        getattr(lib, name).restype = ctypes.c_int
    return lib


def check(rc):
    if rc != 0:
        raise SystemExit("a launch failed with code %d" % rc)


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner                     # microseconds per call of the route


def measure(rts, a):
    meds = {name: [] for name in rts}
    for _ in range(a.reps):                                       # alternate the routes
        for name, fn in rts.items():
            for _ in range(3):
                sample(fn, a.inner)                               # warm
            meds[name].append(statistics.median(sample(fn, a.inner) for _ in range(a.samples)))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in meds.items()}


def same_bits(a, b):
    return all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


def i32(v, dev):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device=dev)


def nan_beyond(t, counts):
    t = t.clone()
    for c, nc in enumerate(counts):
        t[c, int(nc):] = float("nan")
    return t


def sa_routes(base, b, n, m, scales, k, xyz, dev):
    """name -> {route: call}, and the bit comparison of the full-count pair route with the one-sided route"""
    lib, st = _C.lib(), stream_ptr(dev)
    rng = np.random.default_rng(7)
    full_n, full_m = i32(np.full(b, n), dev), i32(np.full(b, m), dev)
    rag_n, rag_m = rng.integers(n // 2, n + 1, size=b), rng.integers(m // 2, m + 1, size=b)
    xr = nan_beyond(xyz, rag_n)
    ln, lm = i32(rag_n, dev), i32(rag_m, dev)
    _, q = P.farthest_point_sample_gather(m, xyz)
    _, qr = P.farthest_point_sample_gather(m, xr, lengths=ln, npoints=lm)
    qr = nan_beyond(qr, rag_m)
    ops, same = {}, {}

    def outs(*shapes):
        return [torch.empty(s, dtype=d, device=dev) for s, d in shapes]
    I, F = torch.int32, torch.float32
    # FPS
    o1, o2, o3 = (outs(((b, m), I), ((b, m, 3), F)) for _ in range(3))
    ops["FPS"] = {
        "one-sided (baseline)": lambda: check(base.pn2_farthest_point_sample_ragged(b, n, m, xyz.data_ptr(), full_n.data_ptr(), o1[0].data_ptr(), o1[1].data_ptr(), st)),
        "pair, full counts": lambda: check(lib.pn2_farthest_point_sample_ragged_counts(b, n, m, xyz.data_ptr(), full_n.data_ptr(), full_m.data_ptr(), o2[0].data_ptr(), o2[1].data_ptr(), st)),
        "pair, ragged counts": lambda: check(lib.pn2_farthest_point_sample_ragged_counts(b, n, m, xr.data_ptr(), ln.data_ptr(), lm.data_ptr(), o3[0].data_ptr(), o3[1].data_ptr(), st)),
    }
    same["FPS"] = (o1, o2)
    # single-radius ball query: the level's first scale
    r0, ns0 = scales[0]
    g1, g2, g3 = (outs(((b, m, ns0), I), ((b, m), I), ((b, m, ns0, 3), F)) for _ in range(3))
    ops["ball query (%.1f, %d)" % (r0, ns0)] = {
        "one-sided (baseline)": lambda: check(base.pn2_query_ball_group_xyz_ragged(b, n, m, r0, ns0, xyz.data_ptr(), full_n.data_ptr(), q.data_ptr(), 1, g1[0].data_ptr(), g1[1].data_ptr(), g1[2].data_ptr(), 0, 0, st)),
        "pair, full counts": lambda: check(lib.pn2_query_ball_group_xyz_ragged_pair(b, n, m, r0, ns0, xyz.data_ptr(), full_n.data_ptr(), q.data_ptr(), full_m.data_ptr(), 1, g2[0].data_ptr(), g2[1].data_ptr(), g2[2].data_ptr(), 0, 0, st)),
        "pair, ragged counts": lambda: check(lib.pn2_query_ball_group_xyz_ragged_pair(b, n, m, r0, ns0, xr.data_ptr(), ln.data_ptr(), qr.data_ptr(), lm.data_ptr(), 1, g3[0].data_ptr(), g3[1].data_ptr(), g3[2].data_ptr(), 0, 0, st)),
    }
    same["ball query (%.1f, %d)" % (r0, ns0)] = (g1, g2)
    # multi-radius ball query
    if len(scales) > 1:
        kk = len(scales)
        radii = (ctypes.c_float * kk)(*[r for r, _ in scales])
        nss = (ctypes.c_int * kk)(*[s for _, s in scales])
        sets = [[outs(((b, m, s), I), ((b, m), I), ((b, m, s, 3), F)) for _, s in scales] for _ in range(3)]
        tabs = [[(ctypes.c_void_p * kk)(*[o[j].data_ptr() for o in st_]) for j in range(3)] for st_ in sets]
        ops["multi-radius ball query"] = {
            "one-sided (baseline)": lambda: check(base.pn2_query_ball_group_xyz_msg_ragged(b, n, m, kk, radii, nss, xyz.data_ptr(), full_n.data_ptr(), q.data_ptr(), 1, tabs[0][0], tabs[0][1], tabs[0][2], st)),
            "pair, full counts": lambda: check(lib.pn2_query_ball_group_xyz_msg_ragged_pair(b, n, m, kk, radii, nss, xyz.data_ptr(), full_n.data_ptr(), q.data_ptr(), full_m.data_ptr(), 1, tabs[1][0], tabs[1][1], tabs[1][2], st)),
            "pair, ragged counts": lambda: check(lib.pn2_query_ball_group_xyz_msg_ragged_pair(b, n, m, kk, radii, nss, xr.data_ptr(), ln.data_ptr(), qr.data_ptr(), lm.data_ptr(), 1, tabs[2][0], tabs[2][1], tabs[2][2], st)),
        }
        same["multi-radius ball query"] = ([t for o in sets[0] for t in o], [t for o in sets[1] for t in o])
    # kNN
    k1, k2, k3 = (outs(((b, m, k), F), ((b, m, k), I)) for _ in range(3))
    ops["kNN (k %d)" % k] = {
        "one-sided (baseline)": lambda: check(base.pn2_knn_point_ragged(b, n, m, k, xyz.data_ptr(), full_n.data_ptr(), q.data_ptr(), k1[0].data_ptr(), k1[1].data_ptr(), st)),
        "pair, full counts": lambda: check(lib.pn2_knn_point_ragged_pair(b, n, m, k, xyz.data_ptr(), full_n.data_ptr(), q.data_ptr(), full_m.data_ptr(), k2[0].data_ptr(), k2[1].data_ptr(), st)),
        "pair, ragged counts": lambda: check(lib.pn2_knn_point_ragged_pair(b, n, m, k, xr.data_ptr(), ln.data_ptr(), qr.data_ptr(), lm.data_ptr(), k3[0].data_ptr(), k3[1].data_ptr(), st)),
    }
    same["kNN (k %d)" % k] = (k1, k2)
    keep = (full_n, full_m, ln, lm, xr, q, qr)                     # the closures hold raw pointers: keep the tensors alive
    return ops, same, {"mean_length": float(rag_n.mean()), "mean_count": float(rag_m.mean()), "max_count": int(rag_m.max())}, keep


def fp_routes(base, b, n, m, dev):
    lib, st = _C.lib(), stream_ptr(dev)
    rng = np.random.default_rng(8)
    unknown = torch.from_numpy(S.uniform_clouds(b, n, 3)).to(dev)
    known = torch.from_numpy(S.uniform_clouds(b, m, 4)).to(dev)
    full_n, full_m = i32(np.full(b, n), dev), i32(np.full(b, m), dev)
    rag_n, rag_m = rng.integers(n // 2, n + 1, size=b), rng.integers(m // 2, m + 1, size=b)
    ur, kr = nan_beyond(unknown, rag_n), nan_beyond(known, rag_m)
    ln, lm = i32(rag_n, dev), i32(rag_m, dev)
    o = [[torch.empty((b, n, 3), dtype=torch.float32, device=dev), torch.empty((b, n, 3), dtype=torch.int32, device=dev)] for _ in range(3)]
    ops = {"three_nn": {
        "one-sided (baseline)": lambda: check(base.pn2_three_nn_ragged(b, n, m, unknown.data_ptr(), full_n.data_ptr(), known.data_ptr(), o[0][0].data_ptr(), o[0][1].data_ptr(), 0, st)),
        "pair, full counts": lambda: check(lib.pn2_three_nn_ragged_pair(b, n, m, unknown.data_ptr(), full_n.data_ptr(), known.data_ptr(), full_m.data_ptr(), o[1][0].data_ptr(), o[1][1].data_ptr(), 0, st)),
        "pair, ragged counts": lambda: check(lib.pn2_three_nn_ragged_pair(b, n, m, ur.data_ptr(), ln.data_ptr(), kr.data_ptr(), lm.data_ptr(), o[2][0].data_ptr(), o[2][1].data_ptr(), 0, st)),
    }}
    keep = (unknown, known, full_n, full_m, ur, kr, ln, lm)
    return ops, {"three_nn": (o[0], o[1])}, {"mean_length": float(rag_n.mean()), "mean_count": float(rag_m.mean())}, keep


def report(title, b, n, m, ops, same, info, a, results):
    for op, rts in ops.items():
        for fn in rts.values():
            fn()
        torch.cuda.synchronize()
        identical = same_bits(*same[op])
        res = measure(rts, a)
        results.append(dict(shape=title, b=b, n=n, m=m, op=op, identical_full_counts=identical, routes=res, **info))
        print("%s (b %d, n %d, m %d) %s: full-count outputs identical to the one-sided entry: %s" % (title, b, n, m, op, identical),
              flush=True)
        for name, r in res.items():
            print("    %-24s %8.1f us   (repetitions %.1f .. %.1f)" % (name, r["median_us"], r["min_us"], r["max_us"]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_pair_bench.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    base = bind(a.parent_lib) if a.parent_lib else _C.lib()
    print("baseline: %s" % ("the one-sided entries of " + a.parent_lib if a.parent_lib else "this library's one-sided entries"))
    results = []
    for title, b, n, m, scales, k in SA_SHAPES:
        xyz = torch.from_numpy(S.sphere_clouds(b, n, 1)).to(dev)
        ops, same, info, keep = sa_routes(base, b, n, m, scales, k, xyz, dev)
        report(title, b, n, m, ops, same, info, a, results)
    for title, b, n, m in FP_SHAPES:
        ops, same, info, keep = fp_routes(base, b, n, m, dev)
        report(title, b, n, m, ops, same, info, a, results)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"samples": a.samples, "reps": a.reps, "inner": a.inner, "parent_lib": bool(a.parent_lib), "results": results},
                      f, indent=1)


if __name__ == "__main__":
    main()
