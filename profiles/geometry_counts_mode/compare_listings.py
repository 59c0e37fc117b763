#!/usr/bin/env python3
"""Compare two pairs of listings of scripts/kernel_text.py and scripts/kernel_resources.py over the five geometry files, the
second pair's kernel names mapped onto the retired names (README.md, "name map").

    python compare_listings.py A_text A_resources B_text B_resources

One line per kernel whose text hash or resources differ, then the totals."""
import re
import sys

FILES = ("ball_query.hip", "ball_query_msg.hip", "topk.hip", "interpolate.hip", "fps.hip")


def split(name):
    m = re.match(r"^(?:void )?pn2::(\w+)(?:<(.*)>)?(?:\(.*\))?$", name)
    if not m:
        return name, ()
    ta = tuple(t.strip() for t in m.group(2).split(",")) if m.group(2) and m.group(2).strip() else ()
    return m.group(1), ta


def old_key(name):
    """(retired kernel name, its template arguments) of a kernel of either tree"""
    k, ta = split(name)
    ncnt = sum(1 for t in ta if t == "int const*")
    ta = tuple(t for t in ta if t != "int const*")
    if k == "fps_reg_ragged_kernel" and len(ta) == 4:
        return ("fps_reg_ragged_counts_kernel" if ta[-1] == "true" else "fps_reg_ragged_kernel"), ta[:-1]
    suffix = {0: "", 1: "_ragged", 2: "_ragged_pair"}[ncnt]
    return (k[:-len("_kernel")] + suffix + "_kernel" if suffix else k), ta


def load(path):
    d = {}
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        if len(f) > 2 and f[0] in FILES:
            d[(f[0],) + old_key(f[1])] = (f[1], f[2:])
    return d


def main():
    at, ar, bt, br = map(load, sys.argv[1:5])
    print("kernels: %d / %d" % (len(at), len(bt)))
    same_t = same_r = 0
    for k in sorted(set(at) | set(bt)):
        if k not in at or k not in bt:
            print("UNMATCHED", k)
            continue
        st, sr = at[k][1] == bt[k][1], ar[k][1] == br[k][1]
        same_t += st
        same_r += sr
        if not st or not sr:
            print("%s\t%s -> %s\ttext %s (%s -> %s instructions)\t%s" % (
                k[0], at[k][0], bt[k][0], "same" if st else "DIFFERS", at[k][1][0], bt[k][1][0],
                "resources same" if sr else "RESOURCES %s -> %s" % (" ".join(ar[k][1]), " ".join(br[k][1]))))
    print("same text %d, same resources %d of %d" % (same_t, same_r, len(set(at) | set(bt))))


if __name__ == "__main__":
    main()
