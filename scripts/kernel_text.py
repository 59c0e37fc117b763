#!/usr/bin/env python3
"""A hash of every kernel's instruction text, from the compiler's own assembly -- no GPU needed. Companion of
kernel_resources.py: two listings diff cleanly, and an unchanged line means the kernel's code did not change.

    python scripts/kernel_text.py [-j JOBS] [--csrc DIR] > listing.txt

Every object of pointnet2_amd/csrc/Makefile is compiled once more with its own flags (asked of `make -n`), device side only,
to assembly. A kernel's text is what stands between its label and its .Lfunc_end label, without comments and blank lines;
basic-block labels carry the function's number within its file (.LBB<function>_<block>), which moves when another function
is added in front of it, so that number is dropped. The text runs on through the kernel's descriptor (.amdhsa_* : registers,
kernel-argument bytes), which names the kernel's own mangled symbol; that name is replaced by a placeholder and the section
directives around the descriptor (.text, or a template instantiation's own comdat section) are left out, so a kernel that
only changes its name or becomes a template (one that gains an empty parameter pack) keeps its hash. One line per kernel, sorted:

    source  kernel(demangled)  instructions  sha256 of the text
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources  # noqa: E402


def listing(csrc, args):
    src = next(a for a in args if a.endswith(".hip"))
    args = [a for a in args if not a.startswith("-Rpass-analysis")]
    args = args[:args.index("-o")] + ["--cuda-device-only", "-S", "-o", "-"]
    args.remove("-c")
    res = subprocess.run(args, cwd=csrc, capture_output=True, text=True)
    if res.returncode:
        sys.stderr.write(res.stderr)
        raise SystemExit("compiling %s failed" % src)
    lines = res.stdout.splitlines()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", res.stdout, re.M))
    rows, name, text = [], None, []
    for line in lines:
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in kernels:
            name, text = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            rows.append((name, text))
            name = None
            continue
        code = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).replace(name, "<kernel>").strip()
        if code and code != ".text" and not code.startswith(".section"):
            text.append(code)
    names = [n for n, _ in rows]
    plain = subprocess.run(["c++filt", "-p"] + names, capture_output=True, text=True).stdout.splitlines() if names else []
    if len(plain) != len(names):
        plain = names
    return ["%s\t%s\t%d\t%s" % (src, p or n, sum(1 for t in text if not t.endswith(":") and not t.startswith(".")),
                                hashlib.sha256("\n".join(text).encode()).hexdigest())
            for p, (n, text) in zip(plain, rows)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--csrc", default=os.path.join(kernel_resources.ROOT, "pointnet2_amd", "csrc"))
    a = ap.parse_args()
    with concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        per_file = list(pool.map(lambda c: listing(a.csrc, c), kernel_resources.commands(a.csrc)))
    print("\n".join(sorted(line for rows in per_file for line in rows)))


if __name__ == "__main__":
    main()
