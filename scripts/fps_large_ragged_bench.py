"""Timing of ragged farthest-point sampling beyond 16384 padded points (pn2_farthest_point_sample_large_ragged_ex) -- the sibling
of scripts/fps_large_bench.py; its table is profiles/fps_large_ragged/README.md (DESIGN.md 4.1e "with lengths").

Every row times its legs in ONE process, alternating: a sample = device events around one call of each leg in turn, a figure =
the median of --samples samples (20) after a warm-up call of every leg. Legs that must agree are compared first.

  (a) full lengths: the ragged entry against the unchanged dense entries at 131072 -> 1024, b = 8 (what the counts cost);
  (b) partial lengths and counts: lengths uniform in n/2 .. n, npoints in m/2 .. m, kernel 2 against kernel 1;
  (c) short clouds in a large padding: clouds of 2048 points padded to 20000 against the register-tier ragged entry on the same
      clouds padded to 2048 (a launch cannot mix tiers: the price of the padding).

    python scripts/fps_large_ragged_bench.py [--samples 20] [--out rows.jsonl]
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
    def __init__(self, lib, dev, b, n, m):
        self.ws = torch.empty((max(16, lib.pn2_fps_large_ws_bytes(b, n)),), dtype=torch.uint8, device=dev)
        self.temp = torch.empty((max(1, lib.pn2_fps_temp_floats(b, n)),), dtype=torch.float32, device=dev)
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


def ragged_leg(lib, st, kernel, b, n, m, x, lens, cnts, buf):
    return lambda: _C.check(lib.pn2_farthest_point_sample_large_ragged_ex(kernel, 256, b, n, m, ptr(x), ptr(lens), ptr(cnts), ptr(buf.ws),
                                                                          ptr(buf.out), ptr(buf.oxyz), st), "ragged kernel %d" % kernel)


def row_a(lib, dev, kind, samples):
    b, n, m = 8, 131072, 1024
    st = stream_ptr(dev)
    x = torch.from_numpy(KINDS[kind](b, n, 77)).to(dev)
    lens = torch.full((b,), n, dtype=torch.int32, device=dev)
    cnts = torch.full((b,), m, dtype=torch.int32, device=dev)
    bufs = {k: Buffers(lib, dev, b, n, m) for k in ("dense tier", "ragged tier", "ragged tier, counts", "dense generic", "ragged generic")}
    legs = {
        "dense tier": lambda: _C.check(lib.pn2_farthest_point_sample_large(b, n, m, ptr(x), ptr(bufs["dense tier"].ws),
                                                                          ptr(bufs["dense tier"].out), ptr(bufs["dense tier"].oxyz), st), "dense tier"),
        "ragged tier": ragged_leg(lib, st, 2, b, n, m, x, lens, None, bufs["ragged tier"]),
        "ragged tier, counts": ragged_leg(lib, st, 2, b, n, m, x, lens, cnts, bufs["ragged tier, counts"]),
        "dense generic": lambda: _C.check(lib.pn2_farthest_point_sample_gather(b, n, m, ptr(x), ptr(bufs["dense generic"].temp),
                                                                               ptr(bufs["dense generic"].out), ptr(bufs["dense generic"].oxyz), st),
                                          "dense generic"),
        "ragged generic": ragged_leg(lib, st, 1, b, n, m, x, lens, None, bufs["ragged generic"]),
    }
    t = time_legs(legs, samples)
    for k in bufs:
        same(bufs[k], bufs["dense tier"], "(a) %s, %s" % (kind, k))
    return dict(row="a", kind=kind, b=b, n=n, m=m, ms=t)


def row_b(lib, dev, kind, samples):
    b, n, m = 8, 131072, 1024
    st = stream_ptr(dev)
    rng = np.random.default_rng(5)
    lengths = rng.integers(n // 2, n + 1, size=b).astype(np.int32)
    npoints = rng.integers(m // 2, m + 1, size=b).astype(np.int32)
    xyz = KINDS[kind](b, n, 78)
    for i, ni in enumerate(lengths):
        xyz[i, ni:] = np.nan
    x = torch.from_numpy(xyz).to(dev)
    lens, cnts = torch.from_numpy(lengths).to(dev), torch.from_numpy(npoints).to(dev)
    bufs = {k: Buffers(lib, dev, b, n, m) for k in ("kernel 1", "kernel 2")}
    legs = {"kernel 1": ragged_leg(lib, st, 1, b, n, m, x, lens, cnts, bufs["kernel 1"]),
            "kernel 2": ragged_leg(lib, st, 2, b, n, m, x, lens, cnts, bufs["kernel 2"])}
    t = time_legs(legs, samples)
    same(bufs["kernel 1"], bufs["kernel 2"], "(b) %s" % kind)
    return dict(row="b", kind=kind, b=b, n=n, m=m, lengths=lengths.tolist(), npoints=npoints.tolist(), ms=t)


def row_c(lib, dev, kind, m, samples):
    b, n, nc = 8, 20000, 2048
    st = stream_ptr(dev)
    small = KINDS[kind](b, nc, 79)
    big = np.full((b, n, 3), np.nan, dtype=np.float32)
    big[:, :nc] = small
    xs, xb = torch.from_numpy(small).to(dev), torch.from_numpy(big).to(dev)
    lens = torch.full((b,), nc, dtype=torch.int32, device=dev)
    bufs = {k: Buffers(lib, dev, b, n, m) for k in ("register tier, padded to 2048", "kernel 0", "kernel 1", "kernel 2")}
    reg = bufs["register tier, padded to 2048"]
    legs = {"register tier, padded to 2048": lambda: _C.check(lib.pn2_farthest_point_sample_ragged(b, nc, m, ptr(xs), ptr(lens), ptr(reg.out),
                                                                                                    ptr(reg.oxyz), st), "register tier")}
    for kernel in (0, 1, 2):
        legs["kernel %d" % kernel] = ragged_leg(lib, st, kernel, b, n, m, xb, lens, None, bufs["kernel %d" % kernel])
    t = time_legs(legs, samples)
    for k in bufs:
        same(bufs[k], reg, "(c) %s m=%d, %s" % (kind, m, k))
    return dict(row="c", kind=kind, b=b, n=n, n_c=nc, m=m, rule=int(lib.pn2_fps_large_pays(n, m)), ms=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON lines here")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _C.lib()
    rows = []
    for kind in KINDS:
        rows.append(row_a(lib, dev, kind, args.samples))
    for kind in KINDS:
        rows.append(row_b(lib, dev, kind, args.samples))
    for kind in KINDS:
        for m in (128, 512):
            rows.append(row_c(lib, dev, kind, m, args.samples))
    for r in rows:
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(r) + "\n")
    print("| row | cloud | b | n | m | leg | ms |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        for leg, ms in r["ms"].items():
            print("| %s | %s | %d | %d | %d | %s | %.3f |" % (r["row"], r["kind"], r["b"], r["n"], r["m"], leg, ms))
    return rows


if __name__ == "__main__":
    main()
