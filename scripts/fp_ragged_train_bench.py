"""Training-mode feature-propagation level with a RAGGED unknown side, after three_nn: what PointnetFPModule.train() takes
with lengths1= today -- the compacting layer-by-layer path, last_path "unfused_ragged" -- against the opt-in route
(fused_ragged_train: fp_interp_concat + the fused node with a row mask, "fused_train_ragged"), the ONE-NODE form with the mask
inside (fused_ragged_node as well: fp_level_train(..., lengths=), "fused_train_ragged_node"), and, as the price of the mask, the
dense route (fp_interp_concat + fp_mlp_train on the same padded tensors, every row taken as valid: other statistics, reported
only). One warm forward + backward per step, HIP events around the step, median of --iters after --warmup; the paths
alternate, --reps times each, in one process: the spread of a path's medians is its run-to-run noise here.
The two ragged last levels of the segmentation networks: sem_seg FP4 (b 8, n 8192, m 1024, 128 -> 128 -> 128 -> 128) and
part_seg FP3 (b 16, n 2048, m 512, 128 + 6 -> 128 -> 128 -> 128); lengths drawn once, seed 0, between n / 2 and n.
    python scripts/fp_ragged_train_bench.py [--iters 20] [--warmup 5] [--reps 3] [--paths a,b,..] [--out DIR]
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
from pointnet2_amd.geometry import FPGeometry  # noqa: E402
from pointnet2_amd.tf_interpolate import fp_interp_concat, three_nn  # noqa: E402

# name, b, n, m, c2, c1, widths (models/pointnet2_sem_seg.py:37, models/pointnet2_part_seg.py:33)
LEVELS = (("sem_seg FP4", 8, 8192, 1024, 128, 0, [128, 128, 128]),
          ("part_seg FP3", 16, 2048, 512, 128, 6, [128, 128, 128]))
PATHS = ("unfused_ragged", "fused_train_ragged", "fused_train_ragged_node", "dense")


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
    for name, b, n, m, c2, c1, widths in LEVELS:
        lengths = torch.randint(n // 2, n + 1, (b,), generator=g, dtype=torch.int32)
        lens = lengths.to(dev)
        mod = U.PointnetFPModule(c2 + c1, widths).to(dev).train()
        xyz1 = torch.rand((b, n, 3), generator=g).to(dev)
        xyz2 = xyz1[:, :m].contiguous()
        p2 = torch.randn((b, m, c2), generator=g).to(dev).requires_grad_(True)
        p1 = torch.randn((b, n, c1), generator=g).to(dev).requires_grad_(True) if c1 else None
        dist, idx = three_nn(xyz1, xyz2, lengths1=lens)
        geo = FPGeometry(dist, idx)
        gout = torch.randn((b, n, widths[-1]), generator=g).to(dev)
        params = list(mod.parameters()) + [p2] + ([p1] if p1 is not None else [])
        taken = {}

        def module(flag, node=False):
            def fn():
                mod.fused_ragged_train, mod.fused_ragged_node = flag, node
                out = mod(xyz1, xyz2, p1, p2, geometry=geo, lengths1=lens)
                taken[(flag, node)] = mod.last_path
                torch.autograd.grad(out, params, gout)
            return fn

        def dense():
            x, _ = fp_interp_concat(p2, p1, idx, dist)
            torch.autograd.grad(train_mlp.fp_mlp_train(mod.mlp.net, x, cin=c2 + c1), params, gout)

        fns = dict(zip(PATHS, (module(False), module(True), module(True, True), dense)))
        medians = {k: [] for k in paths}
        samples = {k: [] for k in paths}
        for _ in range(a.reps):                                   # the paths alternated
            for key in paths:
                t = step_times_ms(fns[key], a.iters, a.warmup)
                medians[key].append(round(statistics.median(t), 4))
                samples[key] += [round(v, 4) for v in t]
        want = {(False, False): "unfused_ragged", (True, False): "fused_train_ragged", (True, True): "fused_train_ragged_node"}
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
        row = {"level": name, "b": b, "n": n, "m": m, "c2": c2, "c1": c1, "widths": widths, "lengths": lengths.tolist(),
               "valid_rows": int(lengths.sum()), "rows": b * n, "iters": a.iters, "warmup": a.warmup, "reps": a.reps}
        for key in paths:
            row[key] = {"median_ms": round(statistics.median(medians[key]), 4), "medians_ms": medians[key],
                        "min_ms": min(samples[key]), "max_ms": max(samples[key]),
                        "spread_of_medians_ms": round(max(medians[key]) - min(medians[key]), 4), "peak_bytes": peaks[key]}
        def ratio(name, num, den):
            if num in row and den in row:
                row[name] = round(row[num]["median_ms"] / row[den]["median_ms"], 3)
        ratio("speedup_over_unfused", "unfused_ragged", "fused_train_ragged")
        ratio("node_over_two_launch", "fused_train_ragged", "fused_train_ragged_node")
        ratio("mask_price", "fused_train_ragged", "dense")
        print(json.dumps(row), flush=True)
        rows.append(row)
        del mod, p2, p1
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "results.json"), "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
