"""Packed batches (offsets= / max_points=, pn2_*_packed) against the padded layout (lengths=, pn2_*_ragged) on the SAME clouds,
same process. Measurement aid; needs the GPU.

    python scripts/packed_bench.py [--samples 20] [--reps 3] [--inner 10] [--parent-lib libpn2ops.so] [--json FILE] [--only SECTION]

Method (that of scripts/ragged_pair_bench.py): the C entries are called directly on preallocated outputs; one SAMPLE is `inner`
back-to-back calls of a route between two device events, divided by `inner` (FPS: 3 calls); one repetition of a route is the
MEDIAN of `samples` samples behind a warm-up; the routes ALTERNATE, `reps` repetitions each. Reported per route: the median of
its repetitions' medians and their spread (min .. max). A difference smaller than the spread is not a difference. Outputs of
the two layouts are compared bit for bit on the valid rows before anything is timed.

--parent-lib: a second build of the library (the parent commit's) whose `_ragged` entries are the padded baseline; without it
the baseline is this library's own `_ragged` entries (the same kernels: profiles/packed/README.md).

Operators, lengths uniform in n/2 .. n (seed fixed), the padded tensor sized by n:
  FPS + gather        32 x 4096 -> 1024 (the library's size rule on n / max_points = 4096: the batched tier)
  ball query + group  the same clouds and samples, radius 0.2, nsample 32 (kernel 0: the library's choice)
  three_nn            sem_seg FP4: 8 x 8192 unknown, 1024 known
  multi-radius group  cls_msg level 1: 32 x 4096, m 512, radii 0.1 / 0.2 / 0.4, nsample 16 / 32 / 128, on sphere-surface clouds
                      and on uniform cubes (those of scripts/ragged_msg_bench.py); queries: each cloud's farthest-point samples.
                      ONE pn2_query_ball_group_xyz_msg_packed launch against (a) what a packed user had before it, three
                      pn2_query_ball_group_xyz_packed launches, and (b) pn2_query_ball_group_xyz_msg_ragged on the padded copy
                      (both baselines from --parent-lib when given)
The second side, packed (--only pair, --only knn; profiles/packed_pair/README.md): FPS + gather with per-cloud sample counts,
the ball query with a ragged query side and kNN (8 x 4096 -> 1024 x 32) through the packed entries against the same clouds
padded through the _ragged_counts / _ragged_pair entries, counts uniform in m/2 .. m; then full counts against the one-sided
packed entries.
MSG level (cls_msg level 1 with 6 feature channels, stacks 32-32-64 / 64-64-128 / 64-96-128, uniform cubes): PointnetSAModuleMSG
with packed_batches on the packed batch against the padded lengths= forward with ragged_one_launch, eval() (no_grad) and train()
(forward + backward); both routes are this tree's Python.
Training level (sem_seg FP4, 128 -> 128 -> 128 -> 128, one warm forward + backward of PointnetFPModule per step, three_nn
included): the packed route -- `total` made a multiple of 32 by the last cloud's length, so the dense node runs on `total`
rows and nothing is masked -- against the padded route with fused_ragged_train (the masked node on b n rows); time and
torch.cuda.max_memory_allocated above what was allocated before the step. Both module routes are this tree's Python: the
padded route's code and kernels are the parent commit's, unchanged."""
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
import pointnet2_amd.pointnet_util as U
from pointnet2_amd import _C
from pointnet2_amd._tensors import stream_ptr


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("pn2_farthest_point_sample_ragged", "pn2_query_ball_group_xyz_ragged", "pn2_three_nn_ragged",
                 "pn2_query_ball_group_xyz_packed", "pn2_query_ball_group_xyz_msg_ragged", "pn2_farthest_point_sample_ragged_counts",
                 "pn2_query_ball_group_xyz_ragged_pair", "pn2_knn_point_ragged_pair", "pn2_knn_point_ragged",
                 "pn2_farthest_point_sample_packed"):
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


def measure(rts, samples, reps, inner):
    meds = {name: [] for name in rts}
    for _ in range(reps):                                         # alternate the routes
        for name, fn in rts.items():
            for _ in range(3):
                sample(fn, inner)                                 # warm
            meds[name].append(statistics.median(sample(fn, inner) for _ in range(samples)))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in meds.items()}


def bits(t):
    return t.contiguous().view(torch.int32)


def valid_rows(padded, lengths):
    return torch.cat([padded[c, :int(k)] for c, k in enumerate(lengths)])


def batch(b, n, seed, dev, multiple=1):
    """lengths uniform in n/2 .. n (the last one lowered so that the total is a multiple of `multiple`), the padded clouds
    (uniform in the unit cube, NaN beyond a length) and their packed twin"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(n // 2, n + 1, size=b)
    lengths[-1] -= int(lengths.sum()) % multiple
    xyz = torch.from_numpy(rng.random((b, n, 3), dtype=np.float32)).to(dev)
    for c, k in enumerate(lengths):
        xyz[c, int(k):] = float("nan")
    flat, offs = P.pack_batch(xyz, lengths.tolist())
    return lengths, xyz, torch.tensor(lengths, dtype=torch.int32, device=dev), flat, offs


def report(title, rts, identical, a, results, **info):
    res = measure(rts, a.samples, a.reps, info.pop("inner", a.inner))
    results.append(dict(op=title, identical_valid_rows=identical, routes=res, **info))
    print("%s: outputs identical on the valid rows: %s" % (title, identical), flush=True)
    for name, r in res.items():
        print("    %-28s %8.1f us   (repetitions %.1f .. %.1f)" % (name, r["median_us"], r["min_us"], r["max_us"]), flush=True)


def operators(base, a, dev, results):
    lib, st = _C.lib(), stream_ptr(dev)
    I, F = torch.int32, torch.float32
    # ---- FPS + gather and ball query + group: 32 x 4096 -> 1024
    b, n, m, radius, ns = 32, 4096, 1024, 0.2, 32
    lengths, xyz, lens, flat, offs = batch(b, n, 1, dev)
    total = int(flat.shape[0])
    o = [[torch.empty((b, m), dtype=I, device=dev), torch.empty((b, m, 3), dtype=F, device=dev)] for _ in range(2)]
    rts = {"padded (_ragged, baseline)": lambda: check(base.pn2_farthest_point_sample_ragged(b, n, m, xyz.data_ptr(), lens.data_ptr(), o[0][0].data_ptr(), o[0][1].data_ptr(), st)),
           "packed": lambda: check(lib.pn2_farthest_point_sample_packed(0, b, total, n, m, flat.data_ptr(), offs.data_ptr(), 0, o[1][0].data_ptr(), o[1][1].data_ptr(), st))}
    for fn in rts.values():
        fn()
    torch.cuda.synchronize()
    same = torch.equal(o[0][0], o[1][0]) and torch.equal(bits(o[0][1]), bits(o[1][1]))
    report("FPS + gather 32 x 4096 -> 1024", rts, same, a, results, b=b, n=n, m=m, total=total, mean_length=float(lengths.mean()), inner=3)
    q = o[1][1].clone()
    g = [[torch.empty((b, m, ns), dtype=I, device=dev), torch.empty((b, m), dtype=I, device=dev), torch.empty((b, m, ns, 3), dtype=F, device=dev)]
         for _ in range(2)]
    rts = {"padded (_ragged, baseline)": lambda: check(base.pn2_query_ball_group_xyz_ragged(b, n, m, radius, ns, xyz.data_ptr(), lens.data_ptr(), q.data_ptr(), 1, g[0][0].data_ptr(), g[0][1].data_ptr(), g[0][2].data_ptr(), 0, 0, st)),
           "packed": lambda: check(lib.pn2_query_ball_group_xyz_packed(b, total, n, m, radius, ns, flat.data_ptr(), offs.data_ptr(), q.data_ptr(), 1, 0, g[1][0].data_ptr(), g[1][1].data_ptr(), g[1][2].data_ptr(), 0, 0, st))}
    for fn in rts.values():
        fn()
    torch.cuda.synchronize()
    same = all(torch.equal(bits(u), bits(v)) for u, v in zip(g[0], g[1]))
    report("ball query + group r 0.2, nsample 32", rts, same, a, results, b=b, n=n, m=m, total=total)
    # ---- three_nn at sem_seg FP4
    b, n, m = 8, 8192, 1024
    lengths, xyz, lens, flat, offs = batch(b, n, 2, dev)
    total = int(flat.shape[0])
    known = torch.from_numpy(np.random.default_rng(3).random((b, m, 3), dtype=np.float32)).to(dev)
    pd, pi = torch.empty((b, n, 3), dtype=F, device=dev), torch.empty((b, n, 3), dtype=I, device=dev)
    fd, fi = torch.empty((total, 3), dtype=F, device=dev), torch.empty((total, 3), dtype=I, device=dev)
    rts = {"padded (_ragged, baseline)": lambda: check(base.pn2_three_nn_ragged(b, n, m, xyz.data_ptr(), lens.data_ptr(), known.data_ptr(), pd.data_ptr(), pi.data_ptr(), 0, st)),
           "packed": lambda: check(lib.pn2_three_nn_packed(b, total, n, m, flat.data_ptr(), offs.data_ptr(), known.data_ptr(), None, 0, fd.data_ptr(), fi.data_ptr(), 0, st))}
    for fn in rts.values():
        fn()
    torch.cuda.synchronize()
    same = torch.equal(valid_rows(pi, lengths), fi) and torch.equal(bits(valid_rows(pd, lengths)), bits(fd))
    report("three_nn sem_seg FP4 (8 x 8192, 1024 known)", rts, same, a, results, b=b, n=n, m=m, total=total, mean_length=float(lengths.mean()))


def pair_operators(base, a, dev, results, knn):
    """The second side, packed (pn2_farthest_point_sample_packed_counts, pn2_query_ball_group_xyz_packed_pair; knn:
    pn2_knn_point_packed) against what a user does without them: the same clouds padded through the _ragged_counts / _ragged_pair
    entries (from --parent-lib when given). Counts uniform in m/2 .. m, lengths uniform in n/2 .. n. Then full counts against the
    one-sided packed entries: the price of the second array."""
    lib, st = _C.lib(), stream_ptr(dev)
    I, F = torch.int32, torch.float32
    rng = np.random.default_rng(9)
    if knn:
        b, n, m, k = 8, 4096, 1024, 32
        lengths, xyz, lens, flat, offs = batch(b, n, 5, dev)
        total = int(flat.shape[0])
        cnts = torch.tensor(rng.integers(m // 2, m + 1, size=b), dtype=I, device=dev)
        full = torch.full((b,), m, dtype=I, device=dev)
        _, q = P.farthest_point_sample_gather(m, xyz, lengths=lens)
        o = [[torch.empty((b, m, k), dtype=F, device=dev), torch.empty((b, m, k), dtype=I, device=dev)] for _ in range(4)]
        rts = {"padded (_ragged_pair, baseline)": lambda: check(base.pn2_knn_point_ragged_pair(b, n, m, k, xyz.data_ptr(), lens.data_ptr(), q.data_ptr(), cnts.data_ptr(), o[0][0].data_ptr(), o[0][1].data_ptr(), st)),
               "packed, lengths2": lambda: check(lib.pn2_knn_point_packed(b, total, n, m, k, flat.data_ptr(), offs.data_ptr(), q.data_ptr(), cnts.data_ptr(), 0, o[1][0].data_ptr(), o[1][1].data_ptr(), st))}
        for fn in rts.values():
            fn()
        torch.cuda.synchronize()
        same = torch.equal(bits(o[0][0]), bits(o[1][0])) and torch.equal(o[0][1], o[1][1])
        report("kNN (8, 4096) -> (1024, 32), counts m/2 .. m", rts, same, a, results, b=b, n=n, m=m, total=total, inner=3)
        rts = {"padded (_ragged, baseline)": lambda: check(base.pn2_knn_point_ragged(b, n, m, k, xyz.data_ptr(), lens.data_ptr(), q.data_ptr(), o[0][0].data_ptr(), o[0][1].data_ptr(), st)),
               "packed, no lengths2": lambda: check(lib.pn2_knn_point_packed(b, total, n, m, k, flat.data_ptr(), offs.data_ptr(), q.data_ptr(), None, 0, o[2][0].data_ptr(), o[2][1].data_ptr(), st)),
               "packed, full lengths2": lambda: check(lib.pn2_knn_point_packed(b, total, n, m, k, flat.data_ptr(), offs.data_ptr(), q.data_ptr(), full.data_ptr(), 0, o[3][0].data_ptr(), o[3][1].data_ptr(), st))}
        for fn in rts.values():
            fn()
        torch.cuda.synchronize()
        same = all(torch.equal(bits(o[0][0]), bits(x[0])) and torch.equal(o[0][1], x[1]) for x in o[2:])
        report("kNN (8, 4096) -> (1024, 32), full counts", rts, same, a, results, b=b, n=n, m=m, total=total, inner=3)
        return
    b, n, m, radius, ns = 32, 4096, 1024, 0.2, 32
    lengths, xyz, lens, flat, offs = batch(b, n, 1, dev)
    total = int(flat.shape[0])
    cnts = torch.tensor(rng.integers(m // 2, m + 1, size=b), dtype=I, device=dev)
    full = torch.full((b,), m, dtype=I, device=dev)
    o = [[torch.empty((b, m), dtype=I, device=dev), torch.empty((b, m, 3), dtype=F, device=dev)] for _ in range(4)]
    rts = {"padded (_ragged_counts, baseline)": lambda: check(base.pn2_farthest_point_sample_ragged_counts(b, n, m, xyz.data_ptr(), lens.data_ptr(), cnts.data_ptr(), o[0][0].data_ptr(), o[0][1].data_ptr(), st)),
           "packed, npoints": lambda: check(lib.pn2_farthest_point_sample_packed_counts(0, b, total, n, m, flat.data_ptr(), offs.data_ptr(), cnts.data_ptr(), 0, o[1][0].data_ptr(), o[1][1].data_ptr(), st))}
    for fn in rts.values():
        fn()
    torch.cuda.synchronize()
    same = torch.equal(o[0][0], o[1][0]) and torch.equal(bits(o[0][1]), bits(o[1][1]))
    report("FPS + gather 32 x 4096 -> 1024, counts m/2 .. m", rts, same, a, results, b=b, n=n, m=m, total=total, inner=3)
    rts = {"packed, one-sided (baseline)": lambda: check(base.pn2_farthest_point_sample_packed(0, b, total, n, m, flat.data_ptr(), offs.data_ptr(), 0, o[2][0].data_ptr(), o[2][1].data_ptr(), st)),
           "packed, full npoints": lambda: check(lib.pn2_farthest_point_sample_packed_counts(0, b, total, n, m, flat.data_ptr(), offs.data_ptr(), full.data_ptr(), 0, o[3][0].data_ptr(), o[3][1].data_ptr(), st))}
    for fn in rts.values():
        fn()
    torch.cuda.synchronize()
    same = torch.equal(o[2][0], o[3][0]) and torch.equal(bits(o[2][1]), bits(o[3][1]))
    report("FPS + gather 32 x 4096 -> 1024, full counts", rts, same, a, results, b=b, n=n, m=m, total=total, inner=3)
    q = o[1][1].clone()
    g = [[torch.empty((b, m, ns), dtype=I, device=dev), torch.empty((b, m), dtype=I, device=dev), torch.empty((b, m, ns, 3), dtype=F, device=dev)]
         for _ in range(4)]
    rts = {"padded (_ragged_pair, baseline)": lambda: check(base.pn2_query_ball_group_xyz_ragged_pair(b, n, m, radius, ns, xyz.data_ptr(), lens.data_ptr(), q.data_ptr(), cnts.data_ptr(), 1, g[0][0].data_ptr(), g[0][1].data_ptr(), g[0][2].data_ptr(), 0, 0, st)),
           "packed, lengths2": lambda: check(lib.pn2_query_ball_group_xyz_packed_pair(b, total, n, m, radius, ns, flat.data_ptr(), offs.data_ptr(), q.data_ptr(), cnts.data_ptr(), 1, 0, g[1][0].data_ptr(), g[1][1].data_ptr(), g[1][2].data_ptr(), 0, 0, st))}
    for fn in rts.values():
        fn()
    torch.cuda.synchronize()
    same = all(torch.equal(bits(u), bits(v)) for u, v in zip(g[0], g[1]))
    report("ball query + group r 0.2, nsample 32, counts m/2 .. m", rts, same, a, results, b=b, n=n, m=m, total=total)
    rts = {"packed, one-sided (baseline)": lambda: check(base.pn2_query_ball_group_xyz_packed(b, total, n, m, radius, ns, flat.data_ptr(), offs.data_ptr(), q.data_ptr(), 1, 0, g[2][0].data_ptr(), g[2][1].data_ptr(), g[2][2].data_ptr(), 0, 0, st)),
           "packed, full lengths2": lambda: check(lib.pn2_query_ball_group_xyz_packed_pair(b, total, n, m, radius, ns, flat.data_ptr(), offs.data_ptr(), q.data_ptr(), full.data_ptr(), 1, 0, g[3][0].data_ptr(), g[3][1].data_ptr(), g[3][2].data_ptr(), 0, 0, st))}
    for fn in rts.values():
        fn()
    torch.cuda.synchronize()
    same = all(torch.equal(bits(u), bits(v)) for u, v in zip(g[2], g[3]))
    report("ball query + group r 0.2, nsample 32, full counts", rts, same, a, results, b=b, n=n, m=m, total=total)


def msg_operator(base, a, dev, results):
    """cls_msg level 1 on a packed batch: one packed multi-radius launch against the two routes the parent commit offers"""
    from pointnet2_amd import synthetic as S
    lib, st = _C.lib(), stream_ptr(dev)
    b, n, m, radii_l, nss_l = 32, 4096, 512, [0.1, 0.2, 0.4], [16, 32, 128]
    k = len(radii_l)
    radii, nss = (ctypes.c_float * k)(*radii_l), (ctypes.c_int * k)(*nss_l)
    for title, gen in (("sphere surface", S.sphere_clouds), ("uniform cube", S.uniform_clouds)):
        xyz = torch.from_numpy(gen(b, n, 1)).to(dev)
        lengths = np.random.default_rng(7).integers(n // 2, n + 1, size=b)
        lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
        for c, nc in enumerate(lengths):
            xyz[c, int(nc):] = float("nan")
        flat, offs = P.pack_batch(xyz, lengths.tolist())
        total = int(flat.shape[0])
        _, q = P.farthest_point_sample_gather(m, xyz, lengths=lens)
        outs = [[(torch.empty((b, m, ns), dtype=torch.int32, device=dev), torch.empty((b, m), dtype=torch.int32, device=dev),
                  torch.empty((b, m, ns, 3), dtype=torch.float32, device=dev)) for ns in nss_l] for _ in range(3)]
        tabs = [[(ctypes.c_void_p * k)(*[o[j].data_ptr() for o in out]) for j in range(3)] for out in outs]

        def per_radius():
            for r, ns, (i, c, g) in zip(radii_l, nss_l, outs[1]):
                check(base.pn2_query_ball_group_xyz_packed(b, total, n, m, r, ns, flat.data_ptr(), offs.data_ptr(), q.data_ptr(), 1, 0,
                                                           i.data_ptr(), c.data_ptr(), g.data_ptr(), 0, 0, st))
        rts = {"packed, one multi-radius launch": lambda: check(lib.pn2_query_ball_group_xyz_msg_packed(
                   b, total, n, m, k, radii, nss, flat.data_ptr(), offs.data_ptr(), q.data_ptr(), 1, 0, *tabs[0], st)),
               "(a) packed, one launch per radius": per_radius,
               "(b) padded, _msg_ragged": lambda: check(base.pn2_query_ball_group_xyz_msg_ragged(
                   b, n, m, k, radii, nss, xyz.data_ptr(), lens.data_ptr(), q.data_ptr(), 1, *tabs[2], st))}
        for fn in rts.values():
            fn()
        torch.cuda.synchronize()
        same = all(torch.equal(bits(u), bits(v)) for other in outs[1:] for o, r in zip(other, outs[0]) for u, v in zip(o, r))
        report("multi-radius group, cls_msg level 1, " + title, rts, same, a, results, b=b, n=n, m=m, total=total,
               mean_length=float(lengths.mean()))


def msg_level(a, dev, results):
    """PointnetSAModuleMSG at cls_msg level 1 with 6 feature channels: packed_batches against the padded lengths= forward"""
    from pointnet2_amd import synthetic as S
    b, n, m, cfeat = 32, 4096, 512, 6
    xyz = torch.from_numpy(S.uniform_clouds(b, n, 1)).to(dev)
    lengths = np.random.default_rng(7).integers(n // 2, n + 1, size=b)
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    feats = torch.randn((b, n, cfeat), generator=torch.Generator().manual_seed(11)).to(dev)
    flat, offs = P.pack_batch(xyz, lengths.tolist())
    fflat, _ = P.pack_batch(feats, lengths.tolist())
    torch.manual_seed(3)
    mod = U.PointnetSAModuleMSG(cfeat, m, [0.1, 0.2, 0.4], [16, 32, 128], [[32, 32, 64], [64, 64, 128], [64, 96, 128]]).to(dev)
    mod.packed_batches = mod.ragged_one_launch = True
    for mode in ("eval", "train"):
        mod.train(mode == "train")
        taken = {}

        def run(name, *args, **kw):
            if mode == "eval":
                with torch.no_grad():
                    _, out = mod(*args, **kw)
            else:
                _, out = mod(*args, **kw)
                torch.autograd.grad(out.sum(), list(mod.parameters()))
            taken[name] = mod.last_path
            return out
        fns = {"padded, lengths= (ragged_one_launch)": lambda: run("padded", xyz, feats, lengths=lens),
               "packed, packed_batches": lambda: run("packed", flat, fflat, offsets=offs, max_points=n)}
        op, of = [fn() for fn in fns.values()]
        torch.cuda.synchronize()
        diff = float((op - of).abs().max() / of.abs().max().clamp(min=1.0))
        meds = {key: [] for key in fns}
        for _ in range(a.reps):
            for key, fn in fns.items():
                for _ in range(5):
                    fn()
                meds[key].append(statistics.median(sample(fn, 1) for _ in range(a.samples)))
        row = dict(op="cls_msg level 1 MSG module, " + mode, b=b, n=n, m=m, total=int(flat.shape[0]), paths=dict(taken),
                   output_difference_of_scale=diff,
                   routes={key: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for key, v in meds.items()})
        results.append(row)
        print("cls_msg level 1 MSG module, %s (paths %s; outputs differ by %.2e of scale)" % (mode, taken, diff), flush=True)
        for key, r in row["routes"].items():
            print("    %-38s %8.1f us   (repetitions %.1f .. %.1f)" % (key, r["median_us"], r["min_us"], r["max_us"]), flush=True)


def training_level(a, dev, results):
    b, n, m, c2, widths = 8, 8192, 1024, 128, [128, 128, 128]
    lengths, xyz, lens, flat, offs = batch(b, n, 4, dev, multiple=32)
    xyz = torch.nan_to_num(xyz, nan=0.0)                          # (a training node may read a padding coordinate: finite)
    total = int(flat.shape[0])
    g = torch.Generator(device="cpu").manual_seed(5)
    mod = U.PointnetFPModule(c2, widths).to(dev).train()
    mod.fused_ragged_train = True
    xyz2 = torch.rand((b, m, 3), generator=g).to(dev)
    p2 = torch.randn((b, m, c2), generator=g).to(dev).requires_grad_(True)
    gout_p = torch.randn((b, n, widths[-1]), generator=g).to(dev)
    gout_f = valid_rows(gout_p, lengths).contiguous()
    params = list(mod.parameters()) + [p2]
    taken = {}

    def padded():
        out = mod(xyz, xyz2, None, p2, lengths1=lens)
        taken["padded"] = mod.last_path
        return out, torch.autograd.grad(out, params, gout_p)

    def packed():
        out = mod(flat, xyz2, None, p2, offsets1=offs, max_points1=n)
        taken["packed"] = mod.last_path
        return out, torch.autograd.grad(out, params, gout_f)
    fns = {"padded, fused_ragged_train": padded, "packed": packed}
    # the two routes compute the same level: compare before timing (two organisations of the same sums, not the same bits)
    (op, gp), (of, gf) = padded(), packed()
    torch.cuda.synchronize()
    def rel(u, v):                                                # of the tensor's scale (the conv biases' gradients are zero up to rounding)
        return float((u.detach() - v.detach()).abs().max() / v.detach().abs().max().clamp(min=1.0))
    names = ["out"] + [k for k, _ in mod.named_parameters()] + ["points2"]
    each = dict(zip(names, [rel(valid_rows(op, lengths), of)] + [rel(u, v) for u, v in zip(gp, gf)]))
    print("    differences, of each tensor's scale: " + ", ".join("%s %.1e" % kv for kv in each.items()), flush=True)
    worst = max(each.values())
    from pointnet2_amd import train_mlp
    taken["packed_one_node_form"] = bool(train_mlp.fp_level_preferred(1, total, b * m, c2) and
                                         train_mlp.fp_level_supported(mod.mlp.net, 1, total, b * m, c2, 0))
    meds, peaks = {k: [] for k in fns}, {}
    for _ in range(a.reps):
        for key, fn in fns.items():
            for _ in range(5):
                fn()
            meds[key].append(statistics.median(sample(fn, 1) for _ in range(a.samples)))
    for key, fn in fns.items():                                   # warm by now: the peak of one more step
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peaks[key] = torch.cuda.max_memory_allocated() - before
    row = dict(op="sem_seg FP4 training level", b=b, n=n, m=m, total=total, rows_padded=b * n, paths=taken,
               worst_relative_difference=worst,
               routes={k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "peak_bytes": peaks[k]} for k, v in meds.items()})
    results.append(row)
    print("sem_seg FP4 training level (total %d of %d padded rows; paths %s; worst difference of outputs and gradients, of each tensor's scale, %.2e)"
          % (total, b * n, taken, worst), flush=True)
    for k, r in row["routes"].items():
        print("    %-28s %8.1f us   (repetitions %.1f .. %.1f)   peak %6.1f MB" % (k, r["median_us"], r["min_us"], r["max_us"], r["peak_bytes"] / 1e6),
              flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, choices=["operators", "msg", "msg_level", "training", "pair", "knn"], help="one section alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("packed_bench.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    base = bind(a.parent_lib) if a.parent_lib else _C.lib()
    print("padded baseline: %s" % ("the _ragged entries of " + a.parent_lib if a.parent_lib else "this library's _ragged entries"))
    results = []
    for name, section in (("operators", lambda: operators(base, a, dev, results)), ("msg", lambda: msg_operator(base, a, dev, results)),
                          ("msg_level", lambda: msg_level(a, dev, results)), ("training", lambda: training_level(a, dev, results)),
                          ("pair", lambda: pair_operators(base, a, dev, results, False)),
                          ("knn", lambda: pair_operators(base, a, dev, results, True))):
        if a.only in (None, name):
            section()
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"samples": a.samples, "reps": a.reps, "inner": a.inner, "parent_lib": bool(a.parent_lib), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
