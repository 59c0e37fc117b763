"""Training-mode set-abstraction levels on a RAGGED batch, after sampling and grouping: what PointnetSAModule.train() takes with
npoints= today -- the compacting layer-by-layer path, last_path "unfused_ragged", unchanged by the flag -- against the opt-in
fused node with a row mask (fused_ragged_train: train_mlp.sa_mlp_train(..., counts=), "fused_train_ragged"), and, as the price of
the mask and of its one fixed organisation, the dense fused node (sa_mlp_train without counts on the same padded tensors, every
row taken as valid: other statistics, reported only). For the group_all level (ragged_group_all) "unfused_ragged" is the
compacting fallback that came with the flag.
One warm forward + backward per step, HIP events around the step, median of --iters after --warmup; the paths alternate, --reps
times each, in one process: the spread of a path's medians is its run-to-run noise here.
The two SA levels of the classification network behind a ragged first level (models/pointnet2_cls_ssg.py:27-28):
cls_ssg L2 (b 32, n 512 -> m 128, nsample 64, 128 features, 131 -> 128 -> 128 -> 256; lengths in n/2..n, npoints in m/2..m) and
cls_ssg L3 (group_all, b 32, n 128, 256 features, 259 -> 256 -> 512 -> 1024; lengths in n/2..n); counts drawn once, seed 0.
    python scripts/sa_ragged_train_bench.py [--iters 20] [--warmup 5] [--reps 3] [--paths a,b,..] [--out DIR]
Prints one JSON line per level (per path also peak_bytes: torch.cuda.max_memory_allocated over one more step, above what was
allocated before it); --out: also DIR/results.json."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pointnet2_amd.pointnet_util as U  # noqa: E402
from pointnet2_amd import train_mlp  # noqa: E402

# name, b, n, m (None: group_all), radius, nsample, cfeat, widths
LEVELS = (("cls_ssg L2", 32, 512, 128, 0.4, 64, 128, [128, 128, 256]),
          ("cls_ssg L3", 32, 128, None, None, None, 256, [256, 512, 1024]))
PATHS = ("unfused_ragged", "fused_train_ragged", "dense")


def step_times_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--paths", default=",".join(PATHS), help="the paths to time, of " + ", ".join(PATHS))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    paths = tuple(k for k in PATHS if k in a.paths.split(","))
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    for name, b, n, m, radius, ns, cfeat, widths in LEVELS:
        group_all = m is None
        lengths = torch.randint(n // 2, n + 1, (b,), generator=g, dtype=torch.int32)
        lens = lengths.to(dev)
        mod = U.PointnetSAModule(cfeat, m, radius, ns, widths, group_all=group_all).to(dev).train()
        mod.ragged_group_all = True
        xyz = torch.rand((b, n, 3), generator=g).to(dev)
        pts = torch.randn((b, n, cfeat), generator=g).to(dev).requires_grad_(True)
        params = list(mod.parameters()) + [pts]
        taken = {}
        if group_all:
            npoints, cnts, geo = None, None, None
            gout = torch.randn((b, 1, widths[-1]), generator=g).to(dev)
            valid_rows, all_rows = int(lengths.sum()), b * n
        else:
            npoints = torch.randint(m // 2, m + 1, (b,), generator=g, dtype=torch.int32)
            cnts = npoints.to(dev)
            geo = mod.geometry(xyz, lengths=lens, npoints=cnts)
            gout = torch.randn((b, m, widths[-1]), generator=g).to(dev)
            valid_rows, all_rows = int(npoints.sum()) * ns, b * m * ns

        def module(flag):
            def fn():
                mod.fused_ragged_train = flag
                if group_all:
                    _, out, _ = mod(xyz, pts, lengths=lens)
                else:
                    _, out, _ = mod(xyz, pts, geometry=geo, lengths=lens, npoints=cnts)
                taken[flag] = mod.last_path
                torch.autograd.grad(out, params, gout)
            return fn

        def dense():
            if group_all:
                out, _ = train_mlp.sa_mlp_train(mod.mlp.net, xyz, None, pts, None)
            else:
                out, _ = train_mlp.sa_mlp_train(mod.mlp.net, xyz, geo.new_xyz, pts, geo.idx)
            torch.autograd.grad(out, params, gout)

        fns = dict(zip(PATHS, (module(False), module(True), dense)))
        medians = {k: [] for k in paths}
        samples = {k: [] for k in paths}
        for _ in range(a.reps):                                   # the paths alternated
            for key in paths:
                t = step_times_ms(fns[key], a.iters, a.warmup)
                medians[key].append(round(statistics.median(t), 4))
                samples[key] += [round(v, 4) for v in t]
        want = {False: "unfused_ragged", True: "fused_train_ragged"}
        assert all(want[k] == v for k, v in taken.items()), taken
        peaks = {}
        for key in paths:                                         # warm by now: the peak of one more step
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fns[key]()
            torch.cuda.synchronize()
            peaks[key] = torch.cuda.max_memory_allocated() - base
        row = {"level": name, "b": b, "n": n, "m": m, "nsample": ns, "cfeat": cfeat, "widths": widths, "lengths": lengths.tolist(),
               "npoints": npoints.tolist() if npoints is not None else None, "valid_rows": valid_rows, "rows": all_rows,
               "iters": a.iters, "warmup": a.warmup, "reps": a.reps}
        for key in paths:
            row[key] = {"median_ms": round(statistics.median(medians[key]), 4), "medians_ms": medians[key],
                        "min_ms": min(samples[key]), "max_ms": max(samples[key]),
                        "spread_of_medians_ms": round(max(medians[key]) - min(medians[key]), 4), "peak_bytes": peaks[key]}

        def ratio(name, num, den):
            if num in row and den in row:
                row[name] = round(row[num]["median_ms"] / row[den]["median_ms"], 3)
        ratio("speedup_over_unfused", "unfused_ragged", "fused_train_ragged")
        ratio("mask_price", "fused_train_ragged", "dense")
        print(json.dumps(row), flush=True)
        rows.append(row)
        del mod, pts
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "results.json"), "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
