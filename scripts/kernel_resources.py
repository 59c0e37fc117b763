#!/usr/bin/env python3
"""Registers, LDS and scratch of every kernel of libpn2ops.so, from the compiler's own report -- no GPU needed.

    python scripts/kernel_resources.py [-j JOBS] [--csrc DIR] > listing.txt

Every object of pointnet2_amd/csrc/Makefile is compiled once more with its own flags (asked of `make -n`) plus
-Rpass-analysis=kernel-resource-usage, to /dev/null; one line per kernel, sorted, so two listings diff cleanly:

    source  kernel(demangled)  sgpr  vgpr  agpr  scratch[bytes/lane]  lds[bytes/block]  occupancy[waves/SIMD]
"""
import argparse
import concurrent.futures
import os
import re
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
        ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ"))


def commands(csrc):
    """The Makefile's compile commands of the library's objects (not the lab builds), as argument lists."""
    text = subprocess.run(["make", "-C", csrc, "-B", "-n", "../libpn2ops.so"], check=True, capture_output=True, text=True).stdout
    out = []
    for line in text.splitlines():
        args = shlex.split(line)
        if "-c" not in args or not any(a.endswith(".hip") for a in args):
            continue
        keep, skip = [], False
        for a in args:
            if skip:
                skip = False
            elif a == "-o":
                skip = True
            elif a not in ("-MMD", "-MP"):
                keep.append(a)
        out.append(keep + ["-Rpass-analysis=kernel-resource-usage", "-o", os.devnull])
    return out


def listing(csrc, args):
    src = next(a for a in args if a.endswith(".hip"))
    err = subprocess.run(args, cwd=csrc, capture_output=True, text=True)
    if err.returncode:
        sys.stderr.write(err.stderr)
        raise SystemExit("compiling %s failed" % src)
    rows, cur = [], None
    for line in err.stderr.splitlines():
        m = re.search(r"remark: (?:.*?: )?Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        for key, short in KEYS:
            m = re.search(r"remark: .*?\s" + re.escape(key) + r": (\S+)", line)
            if m and cur is not None:
                cur[short] = m.group(1)
    names = [r["name"] for r in rows]
    plain = subprocess.run(["c++filt", "-p"] + names, capture_output=True, text=True).stdout.splitlines() if names else []
    if len(plain) != len(names):
        plain = names
    return [(src, p if p else n, r) for p, n, r in zip(plain, names, rows)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--csrc", default=os.path.join(ROOT, "pointnet2_amd", "csrc"))
    a = ap.parse_args()
    with concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        per_file = list(pool.map(lambda c: listing(a.csrc, c), commands(a.csrc)))
    lines = []
    for rows in per_file:
        for src, name, r in rows:
            if "vgpr" not in r:                                   # device functions that are not kernels report nothing more
                continue
            lines.append("%s\t%s\tsgpr %s\tvgpr %s\tagpr %s\tscratch %s\tlds %s\tocc %s" % (
                src, name, r.get("sgpr"), r.get("vgpr"), r.get("agpr"), r.get("scratch"), r.get("lds"), r.get("occ")))
    print("\n".join(sorted(lines)))


if __name__ == "__main__":
    main()
