"""Generates tests/golden/ref_gpu_kernels.npz: the outputs of the reference's own device kernels (oracle/_ref/libref_*_gpu.so,
oracle/Makefile target `ref_gpu`) on the inputs of tests/test_ref_gpu_crosscheck.py, so that its tests also run where
oracle/_ref is not built. Runs that module's tests with every reference kernel launched live and recorded; their checks
against the oracle and the product kernels hold while recording. Needs a GPU and oracle/_ref:

    python tests/golden/make_golden_ref_gpu.py [out.npz]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle as O  # noqa: E402
import test_ref_gpu_crosscheck as T  # noqa: E402


class Recorder:
    """RefKernels' interface: always launches the reference kernel, keeps its outputs as <key>_0, <key>_1, ..."""

    def __init__(self):
        self.out = {}

    def get(self, group, key, launch):
        assert O.ref_available(group), "oracle/_ref/%s not built" % group
        res = launch()
        for i, a in enumerate(res):
            self.out["%s_%d" % (key, i)] = a
        return res


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ref_gpu_kernels.npz")
    cuda = torch.device("cuda:0")
    O.lib()
    rec = Recorder()
    for name in sorted(n for n in dir(T) if n.startswith("test_")):
        getattr(T, name)(cuda, O, rec)
        print("recorded", name)
    np.savez_compressed(dst, **rec.out)
    print(dst, os.path.getsize(dst), "bytes,", len(rec.out), "arrays")


if __name__ == "__main__":
    main()
