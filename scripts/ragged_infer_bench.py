"""Ragged inference: the modules' eval() routes with fused_ragged_eval on (the fused kernels with the counts inside, one C call
per level; include/pn2ops.h "ragged inference") against the default routes -- the parent commit's: the dense kernels on every
row and a torch.where behind them, a ragged group_all level layer by layer. Same process, same tensors. Measurement aid; needs
the GPU.

    python scripts/ragged_infer_bench.py [--samples 20] [--reps 3] [--inner 5] [--json FILE]
    python scripts/ragged_infer_bench.py --dense [--json FILE]      # the four dense eval forwards only (run per tree: before / after)

Method (that of scripts/ragged_pair_bench.py): one SAMPLE is `inner` back-to-back eager forwards of a route between two device
events, divided by `inner` (host time included: fewer calls per level is part of what is measured); one repetition of a route is
the MEDIAN of `samples` samples behind a warm-up; the routes of a shape ALTERNATE, `reps` repetitions each. Reported per route:
the median of its repetitions' medians and their spread (min .. max). A difference smaller than the spread is not a difference.
Before anything is timed the two routes' outputs are compared (bit for bit, except the group_all level, where the default route
is another evaluation order).

Shapes (reference_configs.py), b 32, lengths uniform in n/2 .. n, npoints uniform in m/2 .. m (seed fixed): the three cls_ssg
levels and the whole ragged cls_ssg eval forward; sem_seg SA1; sem_seg FP4 and part_seg FP3.
--dense: the four dense model forwards of scripts/model_forward_bench.py (fused, eager), median of `samples` -- the dense
instantiations and their launches are meant to be what they were; run it in the parent's tree and in this one, alternating."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import pointnet2_amd.pointnet_util as U
from pointnet2_amd import synthetic as S

dev = torch.device("cuda:0")
B = 32


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner                     # microseconds per forward


def measure(rts, a):
    meds = {name: [] for name in rts}
    for _ in range(a.reps):                                       # alternate the routes
        for name, fn in rts.items():
            for _ in range(3):
                sample(fn, a.inner)                               # warm
            meds[name].append(statistics.median(sample(fn, a.inner) for _ in range(a.samples)))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in meds.items()}


def counts(rng, hi):
    return torch.from_numpy(rng.integers(hi // 2, hi + 1, B).astype(np.int32)).to(dev)


def stir(mod):
    for bn in [x for x in mod.modules() if isinstance(x, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d))]:
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
    return mod.to(dev).eval()


def flagged(mods, flag):
    for m in mods:
        m.fused_ragged_eval = flag


def routes(mods, call, exact=True):
    """call() under both settings of the modules' flag -> {route: fn}, after comparing the outputs and checking the paths."""
    def run(flag):
        flagged(mods, flag)
        with torch.no_grad():
            return call()
    off, on = run(False), run(True)
    assert all(m.last_path == "fused_ragged" for m in mods), [m.last_path for m in mods]
    tensors = lambda r: [t for t in (r if isinstance(r, tuple) else (r,)) if t.dtype == torch.float32]
    for u, v in zip(tensors(off), tensors(on)):
        if exact:
            assert torch.equal(u, v)
        else:
            assert (u - v).abs().max().item() <= 2e-5 * max(1.0, u.abs().max().item())
    return {"default": lambda: run(False), "fused_ragged_eval": lambda: run(True)}


class RaggedClsSSG(torch.nn.Module):                  # scripts/model_forward_bench.py: ClsSSG, with the counts handed down
    def __init__(self):
        super().__init__()
        self.sa1 = U.PointnetSAModule(0, 512, 0.2, 32, [64, 64, 128])
        self.sa2 = U.PointnetSAModule(128, 128, 0.4, 64, [128, 128, 256])
        self.sa3 = U.PointnetSAModule(256, None, None, None, [256, 512, 1024], group_all=True)
        self.sa3.ragged_group_all = True
        self.fc = torch.nn.Sequential(torch.nn.Linear(1024, 512), torch.nn.BatchNorm1d(512), torch.nn.ReLU(), torch.nn.Linear(512, 256),
                                      torch.nn.BatchNorm1d(256), torch.nn.ReLU(), torch.nn.Linear(256, 40))

    def forward(self, xyz, l0, n1, n2):
        x1, f1, _ = self.sa1(xyz, None, lengths=l0, npoints=n1)
        x2, f2, _ = self.sa2(x1, f1, lengths=n1, npoints=n2)
        _, f3, _ = self.sa3(x2, f2, lengths=n2)
        return self.fc(f3.reshape(xyz.shape[0], -1))


def ragged(a):
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    out = {}

    def report(title, rts):
        r = measure(rts, a)
        out[title] = r
        d, f = r["default"], r["fused_ragged_eval"]
        print("%-34s default %8.1f us (%.1f .. %.1f)   fused_ragged_eval %8.1f us (%.1f .. %.1f)   x%.2f"
              % (title, d["median_us"], d["min_us"], d["max_us"], f["median_us"], f["min_us"], f["max_us"],
                 d["median_us"] / f["median_us"]), flush=True)

    # ---- cls_ssg: the three levels on their own inputs, then the whole forward
    net = stir(RaggedClsSSG())
    xyz = torch.from_numpy(S.sphere_clouds(B, 1024, 1)).to(dev)
    l0, n1, n2 = counts(rng, 1024), counts(rng, 512), counts(rng, 128)
    with torch.no_grad():
        x1, f1, _ = net.sa1(xyz, None, lengths=l0, npoints=n1)
        x2, f2, _ = net.sa2(x1, f1, lengths=n1, npoints=n2)
    report("cls_ssg SA1 1024 -> 512", routes([net.sa1], lambda: net.sa1(xyz, None, lengths=l0, npoints=n1)))
    report("cls_ssg SA2 512 -> 128", routes([net.sa2], lambda: net.sa2(x1, f1, lengths=n1, npoints=n2)))
    report("cls_ssg SA3 group_all 128", routes([net.sa3], lambda: net.sa3(x2, f2, lengths=n2), exact=False))
    report("cls_ssg ragged eval forward", routes([net.sa1, net.sa2, net.sa3], lambda: net(xyz, l0, n1, n2), exact=False))
    del net
    # ---- sem_seg SA1
    sa = stir(U.PointnetSAModule(0, 1024, 0.1, 32, [32, 32, 64]))
    xyz = torch.from_numpy(S.sphere_clouds(B, 8192, 2)).to(dev)
    l0, n1 = counts(rng, 8192), counts(rng, 1024)
    report("sem_seg SA1 8192 -> 1024", routes([sa], lambda: sa(xyz, None, lengths=l0, npoints=n1)))
    # ---- sem_seg FP4, part_seg FP3
    for title, n, m, c2, c1 in (("sem_seg FP4 1024 -> 8192", 8192, 1024, 128, 0), ("part_seg FP3 512 -> 2048", 2048, 512, 128, 6)):
        fp = stir(U.PointnetFPModule(c2 + c1, [128, 128, 128]))
        xyz1 = torch.from_numpy(S.sphere_clouds(B, n, 3)).to(dev)
        xyz2 = xyz1[:, :m].contiguous()
        p1 = torch.randn(B, n, c1, device=dev) if c1 else None
        p2 = torch.randn(B, m, c2, device=dev)
        l1, l2 = counts(rng, n), counts(rng, m)
        report(title, routes([fp], lambda: fp(xyz1, xyz2, p1, p2, lengths1=l1, lengths2=l2)))
    return out


def dense(a):
    import model_forward_bench as MB
    torch.manual_seed(0)
    out = {}
    for name, model, b, n, normals in [("cls_ssg B=32 N=1024", MB.ClsSSG(), 32, 1024, False), ("cls_msg B=32 N=4096", MB.ClsMSG(), 32, 4096, True),
                                       ("part_seg B=16 N=2048", MB.PartSeg(), 16, 2048, True), ("sem_seg B=8 N=8192", MB.SemSeg(), 8, 8192, False)]:
        model = model.to(dev).eval()
        cloud = S.sphere_clouds(b, n, 1)
        if normals:
            nrm = cloud / np.maximum(np.linalg.norm(cloud, axis=2, keepdims=True), 1e-9)
            cloud = np.concatenate([cloud, nrm.astype(np.float32)], axis=2)
        x = torch.from_numpy(cloud).to(dev)
        with torch.no_grad():
            for _ in range(3):
                sample(lambda: model(x), a.inner)
            out[name] = {"median_us": statistics.median(sample(lambda: model(x), a.inner) for _ in range(a.samples))}
        print("%-24s dense eval forward %9.1f us" % (name, out[name]["median_us"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    res = dense(a) if a.dense else ragged(a)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
