"""Gradients through a level whose batch norms are frozen (eval(): running statistics): what the frozen-statistics node
(train_mlp.sa_mlp_train / fp_mlp_train(..., frozen=True), csrc/train_mlp_frozen.hip) costs and saves.
Per level, forward + backward per iteration, HIP events, median over --iters iterations after --warmup, one process; peak memory
of one forward + backward (torch.cuda.max_memory_allocated):
    (1) layer_by_layer   group_point + concat + conv / BN(eval) / ReLU + max, autograd: parameter and feature gradients (what a
                         module with fused_frozen_bn off runs)
    (2) node_frozen      the fused node with frozen statistics, the same gradients
    (3) node_batch       the existing batch-statistics node on the same shape (the batch norms in train()): the cost yardstick
    (4) saliency_lbl / saliency_node   (1) and (2) with ONLY xyz.requires_grad, every parameter frozen (grouped levels)
(3) runs twice (node_batch, node_batch_again): the spread of a repeated measurement in the same session. Writes JSON lines.
    python scripts/train_frozen_bench.py [--iters 20] [--warmup 5] [--levels metric,SA2] [--only 2] [--repeat 6]
    (--only: one path, for a profiler; --repeat: the selected paths several times in alternating order)"""
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

# name, b, n, m, ns, cfeat, widths, xyz_first (ns = 0: plain rows of an FP level, cfeat = its input width)
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
    ("sem_seg FP4 B=8 8192 rows C=128 [128,128,128]", 8, 8192, 0, 0, 128, [128, 128, 128], True),
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
    ap.add_argument("--only", default="1234")
    ap.add_argument("--repeat", type=int, default=1, help="measure the selected paths this many times, alternating their order "
                    "from pass to pass: <path>_repeats_ms lists every pass's median (the spread of one session)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    for name, b, n, m, ns, cfeat, widths, xyz_first in LEVELS:
        if a.levels and not any(k in name for k in a.levels.split(",")):
            continue
        plain, group_all = ns == 0, "group_all" in name
        net = U._SharedMLP(cfeat if plain else 3 + cfeat, widths, bn=True).to(dev)
        with torch.no_grad():
            for mod in net.net:
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.running_mean.normal_()
                    mod.running_var.uniform_(0.5, 1.5)
        wparams = list(net.parameters())
        if plain:
            x = torch.randn((b, n, cfeat), generator=g).to(dev).requires_grad_(True)
            gw = torch.randn((b, n, widths[-1]), generator=g).to(dev)
        else:
            xyz = torch.rand((b, n, 3), generator=g).to(dev)
            feats = torch.randn((b, n, cfeat), generator=g).to(dev).requires_grad_(True) if cfeat else None
            new_xyz = None if group_all else xyz[:, :m].contiguous()
            idx = None if group_all else torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(dev)
            if idx is not None:
                idx[:, :, ns // 2:] = idx[:, :, :1]                 # padded groups, like the ball query's
            gw = torch.randn((b, m, widths[-1]), generator=g).to(dev)

        def node(frozen, coords=None):
            if plain:
                out = train_mlp.fp_mlp_train(net.net, x, frozen=frozen)
                return torch.autograd.grad(out, wparams + [x], gw)
            if coords is not None:
                out, _ = train_mlp.sa_mlp_train(net.net, coords[0], coords[1] if len(coords) > 1 else None, feats, idx, xyz_first,
                                                xyz_grad=True, frozen=frozen)
                return torch.autograd.grad(out, coords, gw)
            out, _ = train_mlp.sa_mlp_train(net.net, xyz, new_xyz, feats, idx, xyz_first, frozen=frozen)
            return torch.autograd.grad(out, wparams + ([feats] if feats is not None else []), gw)

        def layer_by_layer(coords=None):
            if plain:
                out = net(x.permute(0, 2, 1).unsqueeze(2)).squeeze(2).permute(0, 2, 1)
                return torch.autograd.grad(out, wparams + [x], gw)
            cx = xyz if coords is None else coords[0]
            cn = new_xyz if coords is None or len(coords) < 2 else coords[1]
            if group_all:
                gx = cx.unsqueeze(1)
                gf = feats.unsqueeze(1) if feats is not None else None
            else:
                gx = group_point(cx, idx) - cn.unsqueeze(2)
                gf = group_point(feats, idx) if feats is not None else None
            inp = gx if gf is None else torch.cat([gx, gf] if xyz_first else [gf, gx], dim=-1)
            out = net(inp.permute(0, 3, 1, 2)).max(dim=3)[0].permute(0, 2, 1)
            return torch.autograd.grad(out, (wparams + ([feats] if feats is not None else [])) if coords is None else coords, gw)

        def set_params(flag):
            for p in wparams:
                p.requires_grad_(flag)
            if not plain and feats is not None:
                feats.requires_grad_(flag)
        coords = None
        if not plain:
            coords = [xyz.clone().requires_grad_(True)] + ([] if group_all else [new_xyz.clone().requires_grad_(True)])
        runs = [("1", "layer_by_layer", "eval", True, lambda: layer_by_layer()),
                ("2", "node_frozen", "eval", True, lambda: node(True)),
                ("3", "node_batch", "train", True, lambda: node(False)),
                ("3", "node_batch_again", "train", True, lambda: node(False))]
        if not plain:
            runs += [("4", "saliency_lbl", "eval", False, lambda: layer_by_layer(coords)),
                     ("4", "saliency_node", "eval", False, lambda: node(True, coords))]
        row = {"level": name, "rows": b * n if plain else b * m * ns, "iters": a.iters}
        for tag, key, mode, want_params, fn in runs:
            if tag not in a.only:
                continue
            net.train() if mode == "train" else net.eval()
            set_params(want_params)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            row[key + "_peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            row[key + "_fwd_bwd_ms"] = round(median_ms(fn, a.iters, a.warmup), 3)
            row.setdefault(key + "_repeats_ms", []).append(row[key + "_fwd_bwd_ms"]) if a.repeat > 1 else None
        for rep in range(1, a.repeat):                               # the same paths again, backwards on every other pass
            chosen = [r for r in runs if r[0] in a.only]
            for tag, key, mode, want_params, fn in (chosen[::-1] if rep % 2 else chosen):
                net.train() if mode == "train" else net.eval()
                set_params(want_params)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                row[key + "_repeats_ms"].append(round(median_ms(fn, a.iters, a.warmup), 3))
        if "layer_by_layer_fwd_bwd_ms" in row and "node_frozen_fwd_bwd_ms" in row:
            row["speedup_1_over_2"] = round(row["layer_by_layer_fwd_bwd_ms"] / row["node_frozen_fwd_bwd_ms"], 2)
        print(json.dumps(row), flush=True)
        del net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
