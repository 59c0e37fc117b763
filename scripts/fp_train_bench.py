"""Training-mode feature-propagation level (utils/pointnet_util.py:211-226) after three_nn: the FP node with layer 1 per known
point (train_mlp.fp_level_train, csrc/train_mlp_fp.hip) vs the current path (fp_interp_concat + fp_mlp_train: the (b, n, pitch)
input written, then the stack on plain rows), and which of the two PointnetFPModule.train() takes. Forward + backward per iteration, HIP events, median over --iters after
--warmup; peak memory of one forward + backward (torch.cuda.max_memory_allocated). The seven FP levels of
reference_configs.FP_LEVELS with their real widths and skip channels. Writes JSON lines.
    python scripts/fp_train_bench.py [--iters 20] [--warmup 5] [--levels FP4,FP1] [--once node|current]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pointnet2_amd.pointnet_util as U  # noqa: E402
from pointnet2_amd import train_mlp  # noqa: E402
from pointnet2_amd.reference_configs import FP_LEVELS  # noqa: E402
from pointnet2_amd.tf_interpolate import fp_interp_concat, three_nn  # noqa: E402

# level name -> (layer widths, skip channels c1): models/pointnet2_part_seg.py:31-33, models/pointnet2_sem_seg.py:34-37
STACKS = {
    "cfg4 part_seg FP1": ([256, 256], 256),
    "cfg4 part_seg FP2": ([256, 128], 128),
    "cfg4 part_seg FP3": ([128, 128, 128], 6),
    "cfg5 sem_seg FP1": ([256, 256], 256),
    "cfg5 sem_seg FP2": ([256, 256], 128),
    "cfg5 sem_seg FP3": ([256, 128], 64),
    "cfg5 sem_seg FP4": ([128, 128, 128], 0),
}


def median_ms(fn, iters, warmup):
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
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--levels", default="")
    ap.add_argument("--once", choices=("node", "current"),
                    help="two forward + backward steps of that path, no timing (a profiler run: the second step is the warm one)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    for name, b, n, m, c2 in FP_LEVELS:
        if a.levels and not any(k in name for k in a.levels.split(",")):
            continue
        widths, c1 = STACKS[name]
        net = U._SharedMLP(c2 + c1, widths, bn=True).to(dev).train().net
        xyz1 = torch.rand((b, n, 3), generator=g).to(dev)
        xyz2 = xyz1[:, :m].contiguous() if m > 1 else torch.rand((b, m, 3), generator=g).to(dev)
        p2 = torch.randn((b, m, c2), generator=g).to(dev).requires_grad_(True)
        p1 = torch.randn((b, n, c1), generator=g).to(dev).requires_grad_(True) if c1 else None
        dist, idx = three_nn(xyz1, xyz2)
        gout = torch.randn((b, n, widths[-1]), generator=g).to(dev)
        params = list(net.parameters()) + [p2] + ([p1] if p1 is not None else [])

        def node():
            torch.autograd.grad(train_mlp.fp_level_train(net, p2, p1, idx, dist), params, gout)

        def current():
            x, _ = fp_interp_concat(p2, p1, idx, dist)
            torch.autograd.grad(train_mlp.fp_mlp_train(net, x, cin=c2 + c1), params, gout)
        if a.once:
            for _ in range(2):
                (node if a.once == "node" else current)()
            torch.cuda.synchronize()
            continue
        row = {"level": name, "b": b, "n": n, "m": m, "c2": c2, "c1": c1, "widths": widths, "iters": a.iters,
               "node_supported": train_mlp.fp_level_supported(net, b, n, m, c2, c1),
               "module_takes": "node" if train_mlp.fp_level_supported(net, b, n, m, c2, c1) and
                               train_mlp.fp_level_preferred(b, n, m, c2) else "current"}
        for key, fn in (("node", node), ("current", current)):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            row[key + "_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
        # the two paths alternated, twice each: run-to-run noise shows as the spread of the two medians
        for rep in range(2):
            for key, fn in (("node", node), ("current", current)):
                row["%s_fwd_bwd_ms_%d" % (key, rep)] = round(median_ms(fn, a.iters, a.warmup), 4)
        row["speedup"] = round(min(row["current_fwd_bwd_ms_0"], row["current_fwd_bwd_ms_1"]) /
                               min(row["node_fwd_bwd_ms_0"], row["node_fwd_bwd_ms_1"]), 3)
        print(json.dumps(row), flush=True)
        del net, p2, p1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
