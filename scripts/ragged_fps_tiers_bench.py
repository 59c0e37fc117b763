"""Ragged farthest-point sampling per tier (pn2_farthest_point_sample_ragged_variant) against the dense operator and against the
ragged entry of the parent commit's library. Measurement aid; needs the GPU.

    python scripts/ragged_fps_tiers_bench.py [parent-lib] [--samples 20] [--reps 3] [--inner 3] [--json FILE]

parent-lib: a second build of the library (the parent commit's) whose pn2_farthest_point_sample_ragged / _ragged_counts are the
"parent" leg; without it that leg is this library's PN2_FPS_FULL, the kernel the parent launches.

Method (that of profiles/ragged/README.md and scripts/ragged_pair_bench.py): the C entries are called directly on preallocated
outputs; one SAMPLE is `inner` back-to-back calls of a leg between two device events, divided by `inner`; one repetition of a
leg is the MEDIAN of `samples` samples behind a warm-up; the legs of a setting ALTERNATE in one process, `reps` repetitions
each. Reported per leg: the median of its repetitions' medians and their spread (min .. max). A difference smaller than the
spread is not a difference.

Shapes: the metric shape (32 x 4096 -> 1024), sem_seg SA1 (8 x 8192 -> 1024) and 8 x 8192 -> 200, where the size rule takes
the pruned tier; sphere_clouds. Length settings (seed fixed):
every length = n; lengths uniform in n/2 .. n; lengths uniform in 64 .. n; every length = n with npoints uniform in m/2 .. m.
Legs: the dense operator (the full clouds: what the batch would cost padded by resampling); the parent's ragged entry; this
tree's ragged entry once per variant. Before timing, every variant's outputs are compared with PN2_FPS_FULL's bit for bit."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pointnet2_amd import _C
from pointnet2_amd import synthetic as S
from pointnet2_amd._tensors import stream_ptr

# the third shape is where the size rule takes the PRUNED tier (8192 rank slots, 128 <= m < 256)
SHAPES = [("metric shape", 32, 4096, 1024), ("sem_seg SA1", 8, 8192, 1024), ("8192 -> 200 (AUTO = pruned)", 8, 8192, 200)]
VARIANTS = [("AUTO", 0), ("FULL", 1), ("PRUNED", 2), ("BATCH", 3)]


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("pn2_farthest_point_sample_ragged", "pn2_farthest_point_sample_ragged_counts"):
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
    return e0.elapsed_time(e1) * 1e3 / inner                     # microseconds per call of the leg


def measure(legs, a):
    meds = {name: [] for name in legs}
    for _ in range(a.reps):                                       # alternate the legs
        for name, fn in legs.items():
            for _ in range(3):
                sample(fn, a.inner)                               # warm
            meds[name].append(statistics.median(sample(fn, a.inner) for _ in range(a.samples)))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in meds.items()}


def i32(v, dev):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device=dev)


def settings(b, n, m):
    rng = np.random.default_rng(7)
    full_n, full_m = np.full(b, n), np.full(b, m)
    return [("every length = n", full_n, None),
            ("lengths U[n/2, n]", rng.integers(n // 2, n + 1, size=b), None),
            ("lengths U[64, n]", rng.integers(64, n + 1, size=b), None),
            ("every length = n, npoints U[m/2, m]", full_n, rng.integers(m // 2, m + 1, size=b))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_lib", nargs="?", default=None)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_fps_tiers_bench.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    lib, st = _C.lib(), stream_ptr(dev)
    parent = bind(a.parent_lib) if a.parent_lib else None
    print("parent leg: %s" % ("the ragged entries of " + a.parent_lib if parent else "none given: this library's PN2_FPS_FULL stands in"))
    results = []
    for title, b, n, m in SHAPES:
        xyz = torch.from_numpy(S.sphere_clouds(b, n, 1)).to(dev)
        for setting, lens, cnts in settings(b, n, m):
            x = xyz.clone()
            for c, nc in enumerate(lens):
                x[c, int(nc):] = float("nan")                     # rows at or beyond a length are never read
            ln = i32(lens, dev)
            lm = i32(cnts, dev) if cnts is not None else None
            pm = lm.data_ptr() if lm is not None else None
            outs = {name: (torch.empty((b, m), dtype=torch.int32, device=dev), torch.empty((b, m, 3), dtype=torch.float32, device=dev))
                    for name in ["dense", "parent"] + [v for v, _ in VARIANTS]}
            legs = {}
            od = outs["dense"]
            legs["dense operator (full clouds)"] = lambda od=od: check(lib.pn2_farthest_point_sample_gather(
                b, n, m, xyz.data_ptr(), None, od[0].data_ptr(), od[1].data_ptr(), st))
            op = outs["parent"]
            if parent is None:
                legs["parent: this library's FULL"] = lambda op=op: check(lib.pn2_farthest_point_sample_ragged_variant(
                    1, b, n, m, x.data_ptr(), ln.data_ptr(), pm, op[0].data_ptr(), op[1].data_ptr(), st))
            elif lm is None:
                legs["parent's ragged entry"] = lambda op=op: check(parent.pn2_farthest_point_sample_ragged(
                    b, n, m, x.data_ptr(), ln.data_ptr(), op[0].data_ptr(), op[1].data_ptr(), st))
            else:
                legs["parent's ragged entry"] = lambda op=op: check(parent.pn2_farthest_point_sample_ragged_counts(
                    b, n, m, x.data_ptr(), ln.data_ptr(), pm, op[0].data_ptr(), op[1].data_ptr(), st))
            for vname, v in VARIANTS:
                o = outs[vname]
                legs["ragged " + vname] = lambda o=o, v=v: check(lib.pn2_farthest_point_sample_ragged_variant(
                    v, b, n, m, x.data_ptr(), ln.data_ptr(), pm, o[0].data_ptr(), o[1].data_ptr(), st))
            for fn in legs.values():
                fn()
            torch.cuda.synchronize()
            ref = outs["FULL"]
            identical = all(torch.equal(outs[k][0], ref[0]) and torch.equal(outs[k][1].view(torch.int32), ref[1].view(torch.int32))
                            for k in ["parent"] + [v for v, _ in VARIANTS])
            res = measure(legs, a)
            info = dict(shape=title, b=b, n=n, m=m, setting=setting, mean_length=float(np.mean(lens)), min_length=int(np.min(lens)),
                        mean_npoints=float(np.mean(cnts)) if cnts is not None else float(m), identical_to_full=identical, legs=res)
            results.append(info)
            print("%s (b %d, n %d, m %d), %s [mean length %.0f, min %d]: every ragged leg identical to FULL: %s"
                  % (title, b, n, m, setting, info["mean_length"], info["min_length"], identical), flush=True)
            for name, r in res.items():
                print("    %-30s %8.1f us   (repetitions %.1f .. %.1f)" % (name, r["median_us"], r["min_us"], r["max_us"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"samples": a.samples, "reps": a.reps, "inner": a.inner, "parent_lib": bool(a.parent_lib), "results": results},
                      f, indent=1)


if __name__ == "__main__":
    main()
