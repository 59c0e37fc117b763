"""PointnetSAModuleMSG.ragged_one_launch on the GPU: geometry(xyz, lengths=) runs ragged FPS + gather and then ONE ragged
multi-radius launch for all radii instead of one ragged ball query per radius.

The shapes of test_ragged_modules_gpu.py's MSG module -- b = 4 clouds padded to n = 1024, lengths (1024, 700, 300, 64), npoint
64 -- with a third radius. The default route (itself checked against the per-slice oracle there) is the expectation: the
attribute must change which C entries are called and nothing else, so geometry, eval() output and train() output and gradients
are compared bit for bit. The counting proxy over _C.lib is the one of test_module_call_census_gpu.py."""
import collections
import json
import os

import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

B, N, LENGTHS = 4, 1024, [1024, 700, 300, 64]
NPOINT, WIDTHS, CFEAT = 64, [32, 32, 64], 6
MSG_RADII, MSG_NSAMPLES = [0.2, 0.4, 0.8], [16, 32, 64]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "module_call_census.json")
ONE, PER_RADIUS = "pn2_query_ball_group_xyz_msg_ragged", "pn2_query_ball_group_xyz_ragged"


def _padded(a, fill, seed=0):
    out = a.copy()
    rng = np.random.default_rng(seed)
    for i, ni in enumerate(LENGTHS):
        out[i, ni:] = np.nan if fill == "nan" else rng.standard_normal(out[i, ni:].shape).astype(np.float32)
    return out


@pytest.fixture(scope="module")
def data(cuda):
    xyz = S.sphere_clouds(B, N, 71)
    feats = np.random.default_rng(72).standard_normal((B, N, CFEAT)).astype(np.float32)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return {"xyz_nan": dev(_padded(xyz, "nan")), "xyz_finite": dev(_padded(xyz, "random", 8)), "feats": dev(_padded(feats, "random", 5))}


def _pair(cuda):
    """the same module twice (same seed, same weights): the default route and the one-launch route"""
    from pointnet2_amd.pointnet_util import PointnetSAModuleMSG
    mods = []
    for one in (False, True):
        torch.manual_seed(75)
        mod = PointnetSAModuleMSG(CFEAT, NPOINT, MSG_RADII, MSG_NSAMPLES, [WIDTHS] * 3).to(cuda)
        mod.ragged_one_launch = one
        mods.append(mod)
    return mods


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_geometry_is_the_default_routes(cuda, data):
    ref, one = _pair(cuda)
    g0 = ref.geometry(data["xyz_nan"], lengths=LENGTHS)
    g1 = one.geometry(data["xyz_nan"], lengths=LENGTHS)
    assert torch.equal(g1.fps_idx, g0.fps_idx) and _same_bits(g1.new_xyz, g0.new_xyz)
    assert len(g1.idx) == len(g0.idx) == len(MSG_RADII)
    for r, a, b in zip(MSG_RADII, g1.idx, g0.idx):
        assert a.dtype == torch.int32 and torch.equal(a, b), r
        assert bool((a < torch.tensor(LENGTHS, device=cuda)[:, None, None]).all()), r
    gp = one.geometry(data["xyz_nan"], plans=True, lengths=LENGTHS)           # with index plans: one per radius
    assert len(gp.plan) == len(MSG_RADII) and all(torch.equal(a, b) for a, b in zip(gp.idx, g0.idx))


def test_eval_forward_is_the_default_routes(cuda, data):
    ref, one = _pair(cuda)
    ref.eval(), one.eval()
    with torch.no_grad():
        a = one(data["xyz_nan"], data["feats"], lengths=LENGTHS)
        b = ref(data["xyz_nan"], data["feats"], lengths=LENGTHS)
    assert one.last_path == ref.last_path == "fused"
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and bool(torch.isfinite(a[1]).all())


def test_train_forward_and_backward_are_the_default_routes(cuda, data):
    from pointnet2_amd._tensors import set_deterministic
    ref, one = _pair(cuda)
    ref.train(), one.train()
    w = torch.randn(B, NPOINT, 3 * WIDTHS[-1], generator=torch.Generator().manual_seed(3)).to(cuda)
    set_deterministic(True)                                                   # the scatters in their reproducible mode: bits compare
    try:
        res = []
        for mod in (one, ref):
            feats = data["feats"].clone().requires_grad_(True)
            new_xyz, out = mod(data["xyz_finite"], feats, lengths=LENGTHS)    # the training node wants finite padding rows
            grads = torch.autograd.grad((out * w).sum(), [feats] + list(mod.parameters()), allow_unused=True)
            res.append((new_xyz, out, grads))
    finally:
        set_deterministic(False)
    assert one.last_path == ref.last_path
    (x1, o1, g1), (x0, o0, g0) = res
    assert _same_bits(x1, x0) and _same_bits(o1, o0) and bool(torch.isfinite(o1).all())
    assert g1[0] is not None and g1[1] is not None and len(g1) == len(g0)
    assert all((a is None and b is None) or _same_bits(a, b) for a, b in zip(g1, g0))


class _CountingLibrary:
    """Forwards every attribute of the loaded library; calls of its pn2_* entries are counted by name."""

    def __init__(self, lib, counts):
        self._lib, self._counts = lib, counts

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pn2_"):
            return fn

        def call(*args):
            self._counts[name] += 1
            return fn(*args)
        return call


def _census(monkeypatch, step):
    from pointnet2_amd import _C
    step()                                                                    # warm, uncounted
    counts = collections.Counter()
    proxy = _CountingLibrary(_C.lib(), counts)
    monkeypatch.setattr(_C, "lib", lambda: proxy)
    try:
        step()
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    return dict(counts)


def test_one_launch_replaces_the_per_radius_launches(cuda, data, monkeypatch):
    ref, one = _pair(cuda)
    ref.eval(), one.eval()

    def stepper(mod):
        def step():
            with torch.no_grad():
                mod(data["xyz_nan"], data["feats"], lengths=LENGTHS)
        return step
    got = _census(monkeypatch, stepper(one))
    assert got.get(ONE, 0) == 1 and got.get(PER_RADIUS, 0) == 0
    base = _census(monkeypatch, stepper(ref))
    assert base.get(ONE, 0) == 0 and base.get(PER_RADIUS, 0) == len(MSG_RADII)
    # nothing else differs between the two routes
    strip = lambda c: {k: v for k, v in c.items() if k not in (ONE, PER_RADIUS)}
    assert strip(got) == strip(base)


@pytest.mark.parametrize("case_id", ["msg_eval-lengths", "msg_train-lengths"])
def test_attribute_unset_keeps_the_golden_counts(cuda, monkeypatch, case_id):
    """tests/golden/module_call_census.json, the census module's own cases and shapes: with ragged_one_launch unset (the default)
    the recorded counts hold; set, the per-radius entry's calls become one call of the new entry and nothing else changes."""
    import test_module_call_census_gpu as C
    with open(GOLDEN) as f:
        want = json.load(f)[case_id]
    name, style = case_id.rsplit("-", 1)
    case = next(c for c in C.CASES if c[0] == name)
    got = C.census(case, style, cuda, monkeypatch)
    assert got == want and ONE not in got["calls"] and got["calls"][PER_RADIUS] == len(C.MSG_RADII)
    switched = (case[0], case[1], case[2], dict(case[3], ragged_one_launch=True)) + tuple(case[4:])
    got = C.census(switched, style, cuda, monkeypatch)
    expect = dict(want["calls"])
    del expect[PER_RADIUS]
    expect[ONE] = 1
    assert got["last_path"] == want["last_path"] and got["calls"] == expect
