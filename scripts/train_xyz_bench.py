"""Training-mode SA level whose xyz requires a gradient: what the coordinate gradients of the fused node cost and save.
Per level, forward + backward per iteration, HIP events, median over --iters iterations after --warmup, one process; peak memory
of one forward + backward (torch.cuda.max_memory_allocated):
    (a) layer_by_layer  group_point + concat + conv/BN/ReLU + max, autograd, xyz and new_xyz differentiable (what a module with
                        fused_xyz_grad off runs for such an xyz)
    (b) node_xyz        train_mlp.sa_mlp_train(..., xyz_grad=True): the fused node with grad_xyz and grad_new_xyz
    (c) node            the fused node, coordinates constant (no gradient to them)
    (d) node_xyz_plan   (b) with the level's index plan built in the forward (a module with index_plans = True): the two scatters
                        of the backward -- coordinates and features -- reduce from one inversion instead of inverting idx twice
    (e) node_xyz_given  (b) with a plan built beforehand (a geometry computed ahead with plans=True): no inversion in the iteration
(b) - (c) is the cost of the feature; (a) / (b) its gain. new_xyz is a leaf here: gather_point's own backward is the same launch
on every path. Writes JSON lines.
    python scripts/train_xyz_bench.py [--iters 20] [--warmup 5] [--levels metric,SA2] [--only b]   (--only: one path, for a profiler)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pointnet2_amd.pointnet_util as U  # noqa: E402
from pointnet2_amd import index_plan, train_mlp  # noqa: E402
from pointnet2_amd.tf_grouping import group_point  # noqa: E402

# name, b, n, m, ns, cfeat, widths, xyz_first
LEVELS = [
    ("metric B=32 4096->1024 ns=32 [64,64,128]", 32, 4096, 1024, 32, 0, [64, 64, 128], True),
    ("cls_ssg SA1 B=32 1024->512 ns=32 [64,64,128]", 32, 1024, 512, 32, 0, [64, 64, 128], True),
    ("cls_ssg SA2 B=32 512->128 ns=64 C=128 [128,128,256]", 32, 512, 128, 64, 128, [128, 128, 256], True),
    ("cls_ssg SA3 B=32 group_all 128 C=256 [256,512,1024]", 32, 128, 1, 128, 256, [256, 512, 1024], True),
    ("cls_msg SA1 s1 B=32 4096->512 ns=16 C=3 [32,32,64]", 32, 4096, 512, 16, 3, [32, 32, 64], False),
    ("cls_msg SA1 s2 B=32 4096->512 ns=32 C=3 [64,64,128]", 32, 4096, 512, 32, 3, [64, 64, 128], False),
    ("cls_msg SA1 s3 B=32 4096->512 ns=128 C=3 [64,96,128]", 32, 4096, 512, 128, 3, [64, 96, 128], False),
    ("sem_seg SA1 B=8 8192->1024 ns=32 [32,32,64]", 8, 8192, 1024, 32, 0, [32, 32, 64], True),
    ("sem_seg SA4 B=8 64->16 ns=32 C=256 [256,256,512]", 8, 64, 16, 32, 256, [256, 256, 512], True),
]


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
    ap.add_argument("--only", default="abc")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    for name, b, n, m, ns, cfeat, widths, xyz_first in LEVELS:
        if a.levels and not any(k in name for k in a.levels.split(",")):
            continue
        group_all = "group_all" in name
        net = U._SharedMLP(3 + cfeat, widths, bn=True).to(dev).train()
        xyz = torch.rand((b, n, 3), generator=g).to(dev).requires_grad_(True)
        feats = torch.randn((b, n, cfeat), generator=g).to(dev).requires_grad_(True) if cfeat else None
        new_xyz = None if group_all else xyz.detach()[:, :m].contiguous().requires_grad_(True)
        idx = None if group_all else torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(dev)
        if idx is not None:
            idx[:, :, ns // 2:] = idx[:, :, :1]                 # padded groups, like the ball query's
        params = list(net.parameters()) + ([feats] if feats is not None else [])
        coords = [xyz] + ([new_xyz] if new_xyz is not None else [])
        gw = torch.randn((b, m, widths[-1]), generator=g).to(dev)

        def node_xyz():
            out, _ = train_mlp.sa_mlp_train(net.net, xyz, new_xyz, feats, idx, xyz_first, xyz_grad=True)
            torch.autograd.grad(out, params + coords, gw)

        given = None if group_all else index_plan(idx, n, "group")

        def node_xyz_plan():
            out, _ = train_mlp.sa_mlp_train(net.net, xyz, new_xyz, feats, idx, xyz_first, xyz_grad=True,
                                            plan=None if group_all else index_plan(idx, n, "group"))
            torch.autograd.grad(out, params + coords, gw)

        def node_xyz_given():
            out, _ = train_mlp.sa_mlp_train(net.net, xyz, new_xyz, feats, idx, xyz_first, xyz_grad=True, plan=given)
            torch.autograd.grad(out, params + coords, gw)

        def node():
            out, _ = train_mlp.sa_mlp_train(net.net, xyz, new_xyz, feats, idx, xyz_first)
            torch.autograd.grad(out, params, gw)

        def layer_by_layer():
            if group_all:
                gx = xyz.unsqueeze(1)
                gf = feats.unsqueeze(1) if feats is not None else None
            else:
                gx = group_point(xyz, idx) - new_xyz.unsqueeze(2)
                gf = group_point(feats, idx) if feats is not None else None
            x = gx if gf is None else torch.cat([gx, gf] if xyz_first else [gf, gx], dim=-1)
            out = net(x.permute(0, 3, 1, 2)).max(dim=3)[0].permute(0, 2, 1)
            torch.autograd.grad(out, params + coords, gw)
        rows = b * m * ns
        gdims = (b, n, m, ns, cfeat, 0 if group_all else 1)
        row = {"level": name, "rows": rows, "iters": a.iters,
               "supported": train_mlp.xyz_grad_supported(net.net, rows, ns, "max", b, n, m, cfeat, not group_all), "group_dims": gdims}
        for tag, key, fn in (("a", "layer_by_layer", layer_by_layer), ("b", "node_xyz", node_xyz), ("c", "node", node),
                             ("d", "node_xyz_plan", node_xyz_plan), ("e", "node_xyz_given", node_xyz_given)):
            if tag not in a.only:
                continue
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            row[key + "_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            row[key + "_fwd_bwd_ms"] = round(median_ms(fn, a.iters, a.warmup), 3)
        if a.only == "abc":
            row["speedup_a_over_b"] = round(row["layer_by_layer_fwd_bwd_ms"] / row["node_xyz_fwd_bwd_ms"], 2)
            row["cost_b_minus_c_ms"] = round(row["node_xyz_fwd_bwd_ms"] - row["node_fwd_bwd_ms"], 3)
        print(json.dumps(row), flush=True)
        del net, xyz, feats
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
