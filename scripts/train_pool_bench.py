"""Training-mode SA level with the averaging pooling modes (avg / weighted_avg / max_and_avg, utils/pointnet_util.py:128-142):
the fused node (csrc/train_mlp.hip, pn2_mlp_train_*_pool) vs the layer-by-layer torch path of the same stack (group_point +
concat + conv/BN/ReLU + the pooling formula, autograd). Forward + backward per iteration, HIP events, median over
--iters iterations after --warmup; peak memory of one forward + backward (torch.cuda.max_memory_allocated). max pooling
is reported beside for reference. Writes JSON lines.
    python scripts/train_pool_bench.py [--iters 20] [--warmup 5] [--modes max,avg,weighted_avg,max_and_avg] [--levels metric,SA2]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pointnet2_amd.pointnet_util as U  # noqa: E402
from pointnet2_amd import train_mlp  # noqa: E402
from pointnet2_amd.tf_grouping import group_point  # noqa: E402

# name, b, n, m, ns, cfeat, widths
LEVELS = [
    ("metric B=32 4096->1024 ns=32 [64,64,128]", 32, 4096, 1024, 32, 0, [64, 64, 128]),
    ("cls_ssg SA2 B=32 512->128 ns=64 C=128 [128,128,256]", 32, 512, 128, 64, 128, [128, 128, 256]),
]


def pool_torch(x, gx, mode):
    """(b, C, m, ns) activations -> (b, m, C or 2 C): PointnetSAModule._stack_and_pool's formulas."""
    if mode == "max":
        x = x.max(dim=3)[0]
    elif mode == "avg":
        x = x.mean(dim=3)
    elif mode == "weighted_avg":
        w = torch.exp(-gx.norm(dim=-1) * 5)
        x = (x * (w / w.sum(dim=2, keepdim=True)).unsqueeze(1)).sum(dim=3)
    else:
        x = torch.cat([x.mean(dim=3), x.max(dim=3)[0]], dim=1)
    return x.permute(0, 2, 1)


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
    ap.add_argument("--modes", default="max,avg,weighted_avg,max_and_avg")
    ap.add_argument("--levels", default="metric,SA2")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    for name, b, n, m, ns, cfeat, widths in LEVELS:
        if not any(k in name for k in a.levels.split(",")):
            continue
        net = U._SharedMLP(3 + cfeat, widths, bn=True).to(dev).train()
        xyz = torch.rand((b, n, 3), generator=g).to(dev)
        feats = torch.randn((b, n, cfeat), generator=g).to(dev).requires_grad_(True) if cfeat else None
        new_xyz = xyz[:, :m].contiguous()
        idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(dev)
        params = list(net.parameters()) + ([feats] if feats is not None else [])
        for mode in a.modes.split(","):
            c = widths[-1] * (2 if mode == "max_and_avg" else 1)
            gw = torch.randn((b, m, c), generator=g).to(dev)

            def fused():
                out, _ = train_mlp.sa_mlp_train(net.net, xyz, new_xyz, feats, idx, True, pooling=mode)
                torch.autograd.grad(out, params, gw)

            def unfused():
                gx = group_point(xyz, idx) - new_xyz.unsqueeze(2)
                x = torch.cat([gx, group_point(feats, idx)], dim=-1) if feats is not None else gx
                out = pool_torch(net(x.permute(0, 3, 1, 2)), gx, mode)
                torch.autograd.grad(out, params, gw)
            row = {"level": name, "pooling": mode, "rows": b * m * ns, "iters": a.iters}
            for key, fn in (("fused", fused), ("layer_by_layer", unfused)):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fn()
                torch.cuda.synchronize()
                row[key + "_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
                row[key + "_fwd_bwd_ms"] = round(median_ms(fn, a.iters, a.warmup), 3)
            row["speedup"] = round(row["layer_by_layer_fwd_bwd_ms"] / row["fused_fwd_bwd_ms"], 2)
            print(json.dumps(row), flush=True)
        del net, xyz, feats
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
