"""Generates tests/golden/ref_gpu_kernels*.npz: the outputs of the reference's own device kernels (oracle/_ref/libref_*_gpu.so,
oracle/Makefile target `ref_gpu`) on the inputs of tests/test_ref_gpu_crosscheck.py, so that its tests also run where
oracle/_ref is not built. Runs that module's tests with every reference kernel launched live and recorded; their checks
against the oracle and the product kernels hold while recording. The arrays are dealt in recording order to
ref_gpu_kernels.npz, ref_gpu_kernels_1.npz, ... so that no file passes FILE_BYTES; the tests read all of them. Needs a GPU
and oracle/_ref:

    python tests/golden/make_golden_ref_gpu.py [directory]
"""
import glob
import os
import sys
import zlib

import numpy as np
import torch

FILE_BYTES = 900_000                      # per file, of deflated array bytes: below the largest fixture there is (1,019,256)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle as O  # noqa: E402
import test_ref_gpu_crosscheck as T  # noqa: E402


class Recorder:
    """RefKernels' interface: always launches the reference kernel, keeps its outputs as <key>_0, <key>_1, ..."""

    def __init__(self):
        self.out = {}

    def get(self, group, key, launch, clouds=None):
        assert O.ref_available(group), "oracle/_ref/%s not built" % group
        res = launch()
        for i, a in enumerate(res):
            self.out["%s_%d" % (key, i)] = a if clouds is None else a[:clouds[i]]
        return res


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else HERE
    cuda = torch.device("cuda:0")
    O.lib()
    rec = Recorder()
    for name in sorted(n for n in dir(T) if n.startswith("test_")):
        getattr(T, name)(cuda, O, rec)
        print("recorded", name)
    assert set(rec.out) == set(T.stored_outputs()), set(rec.out) ^ set(T.stored_outputs())
    files, room = [{}], FILE_BYTES
    for key, a in rec.out.items():
        size = len(zlib.compress(np.ascontiguousarray(a).tobytes(), 6)) + 256
        if size > room and files[-1]:
            files.append({})
            room = FILE_BYTES
        files[-1][key] = a
        room -= size
    for old in glob.glob(os.path.join(dst, "ref_gpu_kernels*.npz")):
        os.remove(old)
    for i, arrays in enumerate(files):
        path = os.path.join(dst, "ref_gpu_kernels%s.npz" % ("_%d" % i if i else ""))
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
