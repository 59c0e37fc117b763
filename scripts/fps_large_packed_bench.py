"""Timing of packed farthest-point sampling beyond 16384 points per cloud (pn2_farthest_point_sample_large_packed_ex) -- the sibling
of scripts/fps_large_ragged_bench.py; its tables are profiles/fps_large_packed/README.md (DESIGN.md 4.1e "packed").

Every row times its legs in ONE process, alternating: a sample = device events around one call of each leg in turn, a figure =
the median of --samples samples (20) after a warm-up call of every leg. Legs that must agree are compared first.

  (p) parity of the mode: 8 x 131072 -> 1024, lengths uniform in n/2 .. n; the packed entry (short_max = 0) against
      pn2_farthest_point_sample_large_ragged_ex on the NaN-padded copy of the same clouds, for kernel 2 and kernel 1;
  (s) the short body: b = 8 clouds of n_c in {1024, 2048, 4096, 8192} points inside nmax = 20000 and nmax = 131072, m in {256, 1024}:
      the tier with short_max = 8192, with short_max = 0, the padded entry (kernel 2) on the padded copy, and -- the floor --
      pn2_farthest_point_sample_packed with nmax = n_c.

    python scripts/fps_large_packed_bench.py [--samples 20] [--out rows.jsonl] [--rows ps]
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

KINDS = {"uniform": S.uniform_clouds, "sphere": S.sphere_clouds}


class Buffers:
    def __init__(self, dev, ws_bytes, b, m):
        self.ws = torch.empty((max(16, ws_bytes),), dtype=torch.uint8, device=dev)
        self.out = torch.zeros((b, m), dtype=torch.int32, device=dev)
        self.oxyz = torch.zeros((b, m, 3), dtype=torch.float32, device=dev)


def time_legs(legs, samples):
    """legs: {name: fn} -> {name: median ms}, alternating, one call per sample."""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(samples):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in times.items()}


def same(a, b, what):
    if not (torch.equal(a.out, b.out) and torch.equal(a.oxyz.view(torch.int32), b.oxyz.view(torch.int32))):
        raise SystemExit("%s: the legs disagree" % what)


def batch(dev, kind, seed, n, lengths):
    """-> flat (total, 3), offsets, the NaN-padded (b, n, 3) copy, lengths -- all on the device"""
    xyz = KINDS[kind](len(lengths), n, seed)
    flat = np.concatenate([xyz[i, :ni] for i, ni in enumerate(lengths)])
    for i, ni in enumerate(lengths):
        xyz[i, ni:] = np.nan
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return (torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(xyz).to(dev),
            torch.tensor(list(lengths), dtype=torch.int32, device=dev))


def packed_leg(lib, st, kernel, short_max, b, total, nmax, m, flat, offs, buf):
    return lambda: _C.check(lib.pn2_farthest_point_sample_large_packed_ex(kernel, 256, short_max, b, total, nmax, m, ptr(flat), ptr(offs), 0,
                                                                          ptr(buf.ws), ptr(buf.out), ptr(buf.oxyz), st), "packed kernel %d" % kernel)


def padded_leg(lib, st, kernel, b, n, m, x, lens, buf):
    return lambda: _C.check(lib.pn2_farthest_point_sample_large_ragged_ex(kernel, 256, b, n, m, ptr(x), ptr(lens), None, ptr(buf.ws),
                                                                          ptr(buf.out), ptr(buf.oxyz), st), "padded kernel %d" % kernel)


def row_p(lib, dev, kind, samples):
    b, n, m = 8, 131072, 1024
    st = stream_ptr(dev)
    lengths = np.random.default_rng(5).integers(n // 2, n + 1, size=b).tolist()
    flat, offs, x, lens = batch(dev, kind, 78, n, lengths)
    total = flat.shape[0]
    names = ("packed kernel 2", "padded kernel 2", "packed kernel 1", "padded kernel 1")
    bufs = {k: Buffers(dev, lib.pn2_fps_large_packed_ws_bytes(total) if k.startswith("packed") else lib.pn2_fps_large_ws_bytes(b, n), b, m)
            for k in names}
    legs = {"packed kernel 2": packed_leg(lib, st, 2, 0, b, total, n, m, flat, offs, bufs["packed kernel 2"]),
            "padded kernel 2": padded_leg(lib, st, 2, b, n, m, x, lens, bufs["padded kernel 2"]),
            "packed kernel 1": packed_leg(lib, st, 1, 0, b, total, n, m, flat, offs, bufs["packed kernel 1"]),
            "padded kernel 1": padded_leg(lib, st, 1, b, n, m, x, lens, bufs["padded kernel 1"])}
    t = time_legs(legs, samples)
    for k in names:
        same(bufs[k], bufs["padded kernel 2"], "(p) %s, %s" % (kind, k))
    return dict(row="p", kind=kind, b=b, n=n, n_c=0, m=m, lengths=lengths, ms=t)


def row_s(lib, dev, kind, nmax, nc, m, samples):
    b = 8
    st = stream_ptr(dev)
    flat, offs, x, lens = batch(dev, kind, 79, nmax, [nc] * b)
    total = flat.shape[0]
    names = ("short_max 8192", "short_max 0", "padded kernel 2", "register tier, nmax = n_c")
    bufs = {k: Buffers(dev, lib.pn2_fps_large_ws_bytes(b, nmax) if k.startswith("padded") else lib.pn2_fps_large_packed_ws_bytes(total), b, m)
            for k in names}
    reg = bufs["register tier, nmax = n_c"]
    legs = {"short_max 8192": packed_leg(lib, st, 2, 8192, b, total, nmax, m, flat, offs, bufs["short_max 8192"]),
            "short_max 0": packed_leg(lib, st, 2, 0, b, total, nmax, m, flat, offs, bufs["short_max 0"]),
            "padded kernel 2": padded_leg(lib, st, 2, b, nmax, m, x, lens, bufs["padded kernel 2"]),
            "register tier, nmax = n_c": lambda: _C.check(lib.pn2_farthest_point_sample_packed(0, b, total, nc, m, ptr(flat), ptr(offs), 0,
                                                                                               ptr(reg.out), ptr(reg.oxyz), st), "register tier")}
    t = time_legs(legs, samples)
    for k in names:
        same(bufs[k], reg, "(s) %s nmax=%d n_c=%d m=%d, %s" % (kind, nmax, nc, m, k))
    return dict(row="s", kind=kind, b=b, n=nmax, n_c=nc, m=m, ms=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    ap.add_argument("--rows", default="ps", help="which tables: p (parity), s (short body)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _C.lib()
    rows = []

    def add(r):
        rows.append(r)
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    if "p" in args.rows:
        for kind in KINDS:
            add(row_p(lib, dev, kind, args.samples))
    if "s" in args.rows:
        for kind in KINDS:
            for nmax in (20000, 131072):
                for m in (256, 1024):
                    for nc in (1024, 2048, 4096, 8192):
                        add(row_s(lib, dev, kind, nmax, nc, m, args.samples))
    print("| row | cloud | nmax | n_c | m | " + " | ".join(["leg", "ms"]) + " |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        for leg, ms in r["ms"].items():
            print("| %s | %s | %d | %d | %d | %s | %.3f |" % (r["row"], r["kind"], r["n"], r["n_c"], r["m"], leg, ms))
    return rows


if __name__ == "__main__":
    main()
