"""A/B timing of the large-cloud FPS tier (csrc/fps_large.hip) against the global-memory kernel of
pn2_farthest_point_sample_gather, in the same process on the same clouds, alternating. The table this prints is what
pn2_fps_large_pays is set from (profiles/fps_large/README.md).

One sample = device events around `reps` back-to-back calls, reps chosen so that a sample fills --fill seconds (at least one
call); a figure = the median of --samples samples after a warm-up call of each kernel (whose outputs must be identical). A
configuration that would run longer than --budget seconds per kernel takes fewer samples, never fewer than three; the number
taken is printed. --repeat measures every configuration that many times over and prints each median: their distance is the
spread a speed-up has to exceed.

    python scripts/fps_large_bench.py                                  # the whole sweep (long)
    python scripts/fps_large_bench.py --n 131072 --m 1024 --b 1 --kinds uniform,sphere --group-len 64,128,256 --repeat 2
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pointnet2_amd import _C, synthetic as S                     # noqa: E402
from pointnet2_amd._tensors import ptr, stream_ptr               # noqa: E402

KINDS = {"uniform": S.uniform_clouds, "sphere": S.sphere_clouds, "dropout": S.dropout_clouds, "identical": S.identical_clouds}


def ints(s):
    return [int(v) for v in s.split(",") if v]


def measure(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run_config(lib, dev, kind, b, n, m, group_len, args):
    x = torch.from_numpy(KINDS[kind](b, n, 77)).to(dev)
    st = stream_ptr(dev)
    temp = torch.empty((max(1, lib.pn2_fps_temp_floats(b, n)),), dtype=torch.float32, device=dev)
    ws = torch.empty((lib.pn2_fps_large_ws_bytes(b, n),), dtype=torch.uint8, device=dev)
    out = [torch.zeros((b, m), dtype=torch.int32, device=dev) for _ in range(2)]
    oxyz = [torch.zeros((b, m, 3), dtype=torch.float32, device=dev) for _ in range(2)]

    def generic():
        _C.check(lib.pn2_farthest_point_sample_gather(b, n, m, ptr(x), ptr(temp), ptr(out[0]), ptr(oxyz[0]), st), "generic")

    def large():
        _C.check(lib.pn2_farthest_point_sample_large_ex(group_len, b, n, m, ptr(x), ptr(ws), ptr(out[1]), ptr(oxyz[1]), st), "large")

    t1 = [measure(generic, 1) * 1e-3, measure(large, 1) * 1e-3]                       # warm-up, and the size of one call
    if not (torch.equal(out[0], out[1]) and torch.equal(oxyz[0], oxyz[1])):
        raise SystemExit("%s b=%d n=%d m=%d L=%d: the two kernels disagree" % (kind, b, n, m, group_len))
    reps = [max(1, int(args.fill / max(t, 1e-6))) for t in t1]
    samples = max(3, min(args.samples, int(args.budget / max(reps[0] * t1[0], reps[1] * t1[1], 1e-6))))
    medians = []
    for _ in range(args.repeat):
        tg, tl = [], []
        for _ in range(samples):
            tg.append(measure(generic, reps[0]))
            tl.append(measure(large, reps[1]))
        medians.append((float(np.median(tg)), float(np.median(tl))))
    return dict(kind=kind, b=b, n=n, m=m, group_len=group_len, samples=samples, reps=reps,
                generic_ms=[g for g, _ in medians], large_ms=[l for _, l in medians],
                ratio=medians[0][0] / medians[0][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=ints, default=[20000, 32768, 65536, 131072, 262144, 1048576])
    ap.add_argument("--m", type=ints, default=[64, 256, 1024, 4096])
    ap.add_argument("--b", type=ints, default=[1, 8])
    ap.add_argument("--kinds", default="uniform,sphere,dropout,identical")
    ap.add_argument("--group-len", type=ints, default=[256])
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--fill", type=float, default=0.2, help="seconds one sample should fill")
    ap.add_argument("--budget", type=float, default=8.0, help="seconds per kernel and configuration")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _C.lib()
    rows = []
    print("| cloud | b | n | m | L | generic ms | large ms | generic / large | samples |")
    print("|---|---|---|---|---|---|---|---|---|")
    for kind in args.kinds.split(","):
        for b in args.b:
            for n in args.n:
                for m in args.m:
                    for gl in args.group_len:
                        if not lib.pn2_fps_large_supported(n, m) or (n + gl - 1) // gl > 4096:
                            continue
                        r = run_config(lib, dev, kind, b, n, m, gl, args)
                        rows.append(r)
                        print("| %s | %d | %d | %d | %d | %s | %s | %.2f | %d |" % (
                            kind, b, n, m, gl, " / ".join("%.3f" % v for v in r["generic_ms"]),
                            " / ".join("%.3f" % v for v in r["large_ms"]), r["ratio"], r["samples"]), flush=True)
                        if args.out:
                            with open(args.out, "a") as f:
                                f.write(json.dumps(r) + "\n")
    return rows


if __name__ == "__main__":
    main()
