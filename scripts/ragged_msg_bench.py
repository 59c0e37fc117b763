"""Multi-radius grouping on a ragged batch: ONE pn2_query_ball_group_xyz_msg_ragged launch against the per-radius route (one
pn2_query_ball_group_xyz_ragged per radius), same process, same tensors. Measurement aid; needs the GPU.

    python scripts/ragged_msg_bench.py [--samples 20] [--reps 3] [--inner 10] [--json FILE]

Method: the C entries are called directly on preallocated outputs (no allocation, no Python operator in the window). One
SAMPLE is `inner` back-to-back calls of a route between two device events, divided by `inner` (a single call of 30 us would
measure the event pair). One repetition of a route is the MEDIAN of `samples` samples behind a warm-up; the routes of a shape
ALTERNATE, `reps` repetitions each. Reported per route: the median of its repetitions' medians and their spread (min .. max).
A difference smaller than the spread is not a difference.

Shapes (pointnet2_cls_msg.py:27-28): level 1 b 32, n 4096, m 512, radii 0.1 / 0.2 / 0.4, nsample 16 / 32 / 128, on
sphere-surface clouds and on uniform cubes; level 2 n 512, m 128, radii 0.2 / 0.4 / 0.8, nsample 32 / 64 / 128 (a swept launch).
Queries: the ragged farthest-point samples of each cloud. Lengths: drawn uniformly in [n / 2, n] (seed fixed), and a second run
with every length n, next to the DENSE multi-radius launch -- the price of the ragged wrapper. Before anything is timed the
routes' outputs are compared bit for bit."""
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

SHAPES = [
    ("cls_msg level 1, sphere surface", S.sphere_clouds, 32, 4096, 512, [0.1, 0.2, 0.4], [16, 32, 128]),
    ("cls_msg level 1, uniform cube", S.uniform_clouds, 32, 4096, 512, [0.1, 0.2, 0.4], [16, 32, 128]),
    ("cls_msg level 2 (swept)", S.sphere_clouds, 32, 512, 128, [0.2, 0.4, 0.8], [32, 64, 128]),
]


def outputs(b, m, nsamples, dev):
    return [(torch.empty((b, m, k), dtype=torch.int32, device=dev), torch.empty((b, m), dtype=torch.int32, device=dev),
             torch.empty((b, m, k, 3), dtype=torch.float32, device=dev)) for k in nsamples]


def routes(b, n, m, radii_l, nsamples_l, x, q, lens, dev, dense):
    """name -> (call(), outputs). Every route owns its outputs."""
    lib, st, k = _C.lib(), stream_ptr(dev), len(radii_l)
    radii = (ctypes.c_float * k)(*radii_l)
    nss = (ctypes.c_int * k)(*nsamples_l)

    def tables(outs):
        return [(ctypes.c_void_p * k)(*[o[j].data_ptr() for o in outs]) for j in range(3)]

    def check(rc):
        if rc != 0:
            raise SystemExit("a launch failed with code %d" % rc)
    out = {}
    o_one = outputs(b, m, nsamples_l, dev)
    pi, pc, pg = tables(o_one)
    out["one ragged multi-radius launch"] = (lambda: check(lib.pn2_query_ball_group_xyz_msg_ragged(
        b, n, m, k, radii, nss, x.data_ptr(), lens.data_ptr(), q.data_ptr(), 1, pi, pc, pg, st)), o_one)
    o_per = outputs(b, m, nsamples_l, dev)

    def per_radius():
        for r, ns, (i, c, g) in zip(radii_l, nsamples_l, o_per):
            check(lib.pn2_query_ball_group_xyz_ragged(b, n, m, r, ns, x.data_ptr(), lens.data_ptr(), q.data_ptr(), 1, i.data_ptr(),
                                                      c.data_ptr(), g.data_ptr(), 0, 0, st))
    out["one ragged launch per radius"] = (per_radius, o_per)
    if dense:
        o_dense = outputs(b, m, nsamples_l, dev)
        di, dc, dg = tables(o_dense)
        out["dense multi-radius launch"] = (lambda: check(lib.pn2_query_ball_group_xyz_msg(
            b, n, m, k, radii, nss, x.data_ptr(), q.data_ptr(), 1, di, dc, dg, st)), o_dense)
    return out


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
        for name, (fn, _) in rts.items():
            for _ in range(3):
                sample(fn, a.inner)                               # warm
            meds[name].append(statistics.median(sample(fn, a.inner) for _ in range(a.samples)))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in meds.items()}


def same_bits(rts):
    ref = next(iter(rts.values()))[1]
    for fn, _ in rts.values():
        fn()
    torch.cuda.synchronize()
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for _, outs in rts.values() for o, r in zip(outs, ref)
               for a, b in zip(o, r))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_msg_bench.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    results = []
    for title, gen, b, n, m, radii, nsamples in SHAPES:
        xyz = torch.from_numpy(gen(b, n, 1)).to(dev)
        rng = np.random.default_rng(7)
        for kind, lengths in (("lengths in [n/2, n]", rng.integers(n // 2, n + 1, size=b)), ("every length n", np.full(b, n))):
            lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
            x = xyz.clone()
            for c, nc in enumerate(lengths):
                x[c, int(nc):] = float("nan")
            _, q = P.farthest_point_sample_gather(m, x, lengths=lens)
            rts = routes(b, n, m, radii, nsamples, x, q, lens, dev, dense=kind == "every length n")
            same = same_bits(rts)
            res = measure(rts, a)
            results.append({"shape": title, "b": b, "n": n, "m": m, "radii": radii, "nsamples": nsamples, "lengths": kind,
                            "mean_length": float(np.mean(lengths)), "identical_outputs": same, "routes": res})
            print("%s, %s (mean %.0f): outputs identical: %s" % (title, kind, float(np.mean(lengths)), same), flush=True)
            for name, r in res.items():
                print("    %-34s %7.1f us   (repetitions %.1f .. %.1f)" % (name, r["median_us"], r["min_us"], r["max_us"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"samples": a.samples, "reps": a.reps, "inner": a.inner, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
