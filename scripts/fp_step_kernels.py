"""Per-kernel breakdown of ONE warm training step of an FP level from a rocprofv3 kernel trace of
`scripts/fp_train_bench.py --levels LEVEL --once node|current` (two steps after three_nn; the second is summarised).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o step -- python scripts/fp_train_bench.py --levels FP4 --once node
    python scripts/fp_step_kernels.py DIR/step_kernel_trace.csv [...]
Prints, per trace, the kernels of the warm step (name, launches, summed duration) and the step's summed kernel time."""
import collections
import csv
import sys


def warm_step(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    last_nn = max(i for i, r in enumerate(rows) if "three_nn" in r["Kernel_Name"])
    after = rows[last_nn + 1:]
    if len(after) % 2:
        raise SystemExit("%s: %d kernels after three_nn, not two equal steps" % (path, len(after)))
    return after[len(after) // 2:]


def main():
    for path in sys.argv[1:]:
        step = warm_step(path)
        agg = collections.OrderedDict()
        for r in step:
            name = r["Kernel_Name"].split("(")[0]
            a = agg.setdefault(name, [0, 0])
            a[0] += 1
            a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        total = sum(d for _, d in agg.values())
        print("== %s: %d launches, kernel time %.1f us" % (path, len(step), total / 1e3))
        for name, (cnt, dur) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print("  %8.1f us  %2d x  %s" % (dur / 1e3, cnt, name))


if __name__ == "__main__":
    main()
