"""CPU tests of pn2_query_ball_group_xyz_msg_ragged (include/pn2ops.h "ragged batches"): the multi-radius ball query with
per-cloud point counts. Declared, exported and bound; the host-side validation answers before any device call, so host memory
(or NULL, where the dense entry allows it) stands in for every device pointer; the Python operator refuses a wrong lengths
shape before anything else."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pn2_query_ball_group_xyz_msg_ragged"
OK, E_NULL, E_SHAPE, E_ARG, E_TOO_LARGE = 0, -1, -2, -3, -4


def test_declared_exported_and_bound():
    from pointnet2_amd import _C
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pn2ops.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pn2_[a-z0-9_]+)\s*\(", txt))
    assert NAME in declared
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), NAME)
    assert NAME in _C.EXPORTED
    dense = _C._SIGNATURES["pn2_query_ball_group_xyz_msg"]
    assert _C._SIGNATURES[NAME] == dense[:7] + [ctypes.c_void_p] + dense[7:]      # lengths1 behind xyz1, nothing else differs


class _Call:
    """One call description; every test changes one thing about a call that would be launched."""

    def __init__(self):
        self.keep = []
        self.f = (ctypes.c_float * 64)()
        self.i = (ctypes.c_int * 64)()
        self.args = dict(b=1, n=8, m=4, radii=[0.2, 0.4], nsamples=[4, 8], xyz1=ctypes.addressof(self.f),
                         lengths1=ctypes.addressof(self.i), xyz2=ctypes.addressof(self.f), idx="all", cnt="all", grouped="all")

    def __call__(self, **changes):
        from pointnet2_amd import _C
        a = dict(self.args, **changes)
        k = a.get("nscales", len(a["radii"]))
        radii = (ctypes.c_float * max(len(a["radii"]), 1))(*a["radii"])
        nss = (ctypes.c_int * max(len(a["nsamples"]), 1))(*a["nsamples"])

        def table(form, base):
            if form is None:
                return None
            entries = [base if (form == "all" or i not in form) else None for i in range(max(len(a["radii"]), 1))]
            return (ctypes.c_void_p * len(entries))(*entries)
        pi = table(a["idx"], ctypes.addressof(self.i))
        pc = table(a["cnt"], ctypes.addressof(self.i))
        pg = table(a["grouped"], ctypes.addressof(self.f))
        return _C.lib().pn2_query_ball_group_xyz_msg_ragged(a["b"], a["n"], a["m"], k, radii, nss, a["xyz1"], a["lengths1"], a["xyz2"],
                                                            1, pi, pc, pg, None)


@pytest.fixture(scope="module")
def call():
    return _Call()


def test_null_lengths(call):
    assert call(lengths1=None) == E_NULL
    assert call(lengths1=None, xyz1=None, xyz2=None) == E_NULL


def test_attributes(call):
    assert call(nscales=0) == E_ARG
    assert call(radii=[0.1] * 5, nsamples=[4] * 5) == E_ARG                  # five scales
    assert call(radii=[0.2, 0.0]) == E_ARG
    assert call(radii=[-1.0, 0.4]) == E_ARG
    assert call(radii=[float("nan"), 0.4]) == E_ARG
    assert call(nsamples=[4, 0]) == E_ARG
    assert call(nsamples=[-2, 8]) == E_ARG
    # ... with null data pointers too: the attributes are looked at first
    assert call(nscales=0, xyz1=None, xyz2=None, lengths1=None) == E_ARG
    assert call(nsamples=[4, 0], xyz1=None, xyz2=None) == E_ARG


def test_extents(call):
    assert call(n=0) == E_SHAPE
    assert call(b=-1) == E_SHAPE
    assert call(n=8193) == E_TOO_LARGE
    assert call(n=8193, xyz1=None, xyz2=None) == E_TOO_LARGE                 # before the data pointers are looked at
    assert call(n=8192, radii=[0.1, 0.2, 0.4], nsamples=[16, 32, 127]) == E_TOO_LARGE    # no LDS geometry (the dense entry's case)


def test_nothing_to_do(call):
    assert call(b=0) == OK
    assert call(m=0) == OK
    assert call(b=0, xyz1=None, xyz2=None, lengths1=None) == OK


def test_missing_outputs(call):
    assert call(idx={1}, grouped={1}) == E_NULL                              # scale 1 has neither idx nor grouped_xyz
    assert call(idx=None, grouped=None) == E_NULL
    assert call(idx=None, grouped={0}) == E_NULL
    assert call(idx={0}, grouped={1}, n=8193) == E_TOO_LARGE                 # one of the two per scale is enough: the next check answers
    assert call(cnt=None, n=8193) == E_TOO_LARGE
    assert call(xyz1=None) == E_NULL
    assert call(xyz2=None) == E_NULL


def test_python_operator_refuses_a_wrong_lengths_shape():
    import pointnet2_amd as P
    xyz, q = torch.zeros(2, 8, 3), torch.zeros(2, 4, 3)
    for bad in ([1, 2, 3], torch.tensor([[1, 2]]), torch.tensor([1.0, 2.0]), torch.tensor(3)):
        with pytest.raises(ValueError, match="lengths"):
            P.query_ball_group_xyz_msg([0.2, 0.4], [4, 8], xyz, q, lengths1=bad)


def test_module_attribute_defaults_to_off():
    from pointnet2_amd.pointnet_util import PointnetSAModuleMSG
    assert PointnetSAModuleMSG(0, 4, [0.2, 0.4], [4, 8], [[8], [8]]).ragged_one_launch is False
