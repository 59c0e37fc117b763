"""Write tests/golden/operator_call_census.json: the C entries every operator call of tests/test_operator_call_census_gpu.py
reaches, in order, with their arguments, from that module's own case list. Run it on the commit whose behaviour is to be
pinned:

    python scripts/record_operator_call_census.py [output.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pytest  # noqa: E402
import torch  # noqa: E402

import test_operator_call_census_gpu as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    dev = torch.device("cuda:0")
    result = {}
    for case in T.CASES:
        mp = pytest.MonkeyPatch()
        try:
            result[case[0]] = T.census(case, dev, mp)
        finally:
            mp.undo()
        print("%-48s %s" % (case[0], " ".join(name for name, _ in result[case[0]])), flush=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
