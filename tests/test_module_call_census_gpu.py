"""Which C entries a module path calls, and how often.

The Python layer in front of libpn2ops.so decides which kernels a module runs; the library itself is tended elsewhere. So
what a change of that layer can change is exactly this: the set of C entries a forward (and, where gradients exist, a
backward) reaches, and the number of calls of each. Every case below replaces `_C.lib` by a proxy that forwards every call
and counts it by entry name, runs one warm step uncounted (weight packing, workspaces of a first call) and one counted
step, and compares name -> count and the module's `last_path` with tests/golden/module_call_census.json.

The golden file is written by scripts/record_module_call_census.py, which runs THIS module's case list; it was recorded on
the commit before the modules' routes were merged and is committed unchanged.

Counts are compared, never order (a level's index plan may be built before or after the centroids' re-gather). Only the
library's entries are counted: torch's own launches (cat, zeros, where, the layer-by-layer stacks) are not.

Shapes: b = 4 clouds of n = 256 points, npoint 64, nsample 32, 16 feature channels, stack (16, 16, 32); feature
propagation from 64 known to 256 unknown points, c2 = 32, c1 = 16, stack (32, 32). Rows are a multiple of 32 (the training
nodes' requirement) and b >= 4 keeps use_segmented_grad true at every channel count."""
import collections
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, NPOINT, RADIUS, NSAMPLE, CFEAT, STACK = 4, 256, 64, 0.3, 32, 16, (16, 16, 32)
LENGTHS = [256, 200, 131, 64]
MSG_RADII, MSG_NSAMPLES = [0.2, 0.4], [16, 32]
FP_N, FP_M, FP_C2, FP_C1, FP_STACK = 256, 64, 32, 16, (32, 32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "module_call_census.json")

ALL = ("plain", "geometry", "lengths")
# (name, module, constructor keywords, attributes set on the module, "train" | "frozen" | "eval", xyz requires a gradient,
#  call styles). "frozen": the module in eval() -- every batch norm on its running statistics -- with autograd on.
# fp_node: FP_NODE_MIN_SAVED = 0, so that the level trains as one node.
CASES = [
    ("sa_train", "sa", {}, {}, "train", False, ALL),
    ("sa_train_xyz_grad", "sa", {}, {"fused_xyz_grad": True}, "train", True, ALL),
    ("sa_train_index_plans", "sa", {}, {"index_plans": True}, "train", False, ALL),
    ("sa_frozen", "sa", {}, {"fused_frozen_bn": True}, "frozen", False, ALL),
    ("sa_eval_ball_max", "sa", {}, {}, "eval", False, ALL),
    ("sa_eval_knn", "sa", {"knn": True}, {}, "eval", False, ALL),
    ("sa_eval_avg", "sa", {"pooling": "avg"}, {}, "eval", False, ALL),
    ("sa_group_all_train", "sa", {"group_all": True}, {}, "train", False, ("plain",)),
    ("sa_group_all_eval", "sa", {"group_all": True}, {}, "eval", False, ("plain",)),
    ("sa_unfused_train", "sa", {}, {"fused_mlp": False}, "train", False, ALL),
    ("sa_unfused_eval", "sa", {}, {"fused_mlp": False}, "eval", False, ALL),
    ("msg_train", "msg", {}, {}, "train", False, ALL),
    ("msg_train_xyz_grad", "msg", {}, {"fused_xyz_grad": True}, "train", True, ALL),
    ("msg_frozen", "msg", {}, {"fused_frozen_bn": True}, "frozen", False, ALL),
    ("msg_eval", "msg", {}, {}, "eval", False, ALL),
    ("msg_unfused_train", "msg", {}, {"fused_mlp": False}, "train", False, ALL),
    ("msg_unfused_eval", "msg", {}, {"fused_mlp": False}, "eval", False, ALL),
    ("fp_eval", "fp", {}, {}, "eval", False, ALL),
    ("fp_train_node", "fp_node", {}, {}, "train", False, ("plain", "geometry")),
    ("fp_train_concat", "fp", {}, {}, "train", False, ALL),
    ("fp_train_ragged", "fp", {}, {"fused_ragged_train": True}, "train", False, ("lengths",)),
    ("fp_train_ragged_node", "fp_node", {}, {"fused_ragged_train": True, "fused_ragged_node": True}, "train", False, ("lengths",)),
    ("fp_frozen", "fp", {}, {"fused_frozen_bn": True}, "frozen", False, ("plain", "geometry")),
    ("fp_unfused_train", "fp", {}, {"fused_mlp": False}, "train", False, ("plain", "geometry")),
    ("fp_unfused_eval", "fp", {}, {"fused_mlp": False}, "eval", False, ("plain", "geometry")),
]
CASE_IDS = ["%s-%s" % (case[0], style) for case in CASES for style in case[6]]


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


def _module(kind, kw, attrs, mode, dev):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(0)
    if kind == "sa" and kw.get("group_all"):
        mod = U.PointnetSAModule(CFEAT, None, None, None, list(STACK), **kw)
    elif kind == "sa":
        mod = U.PointnetSAModule(CFEAT, NPOINT, RADIUS, NSAMPLE, list(STACK), **kw)
    elif kind == "msg":
        mod = U.PointnetSAModuleMSG(CFEAT, NPOINT, MSG_RADII, MSG_NSAMPLES, [list(STACK), list(STACK)], **kw)
    else:
        mod = U.PointnetFPModule(FP_C2 + FP_C1, list(FP_STACK), **kw)
    mod = mod.to(dev)
    for name, value in attrs.items():
        assert hasattr(mod, name)
        setattr(mod, name, value)
    return mod.train() if mode == "train" else mod.eval()


def make_step(case, style, dev):
    """-> step(): one forward (+ one backward unless the case is "eval") of the case in the given call style; returns the
    module's last_path. Inputs are fixed; every step starts from cleared gradients."""
    from pointnet2_amd.geometry import FPGeometry
    from pointnet2_amd.tf_interpolate import three_nn
    name, kind, kw, attrs, mode, xyz_grad, _ = case
    mod = _module(kind, kw, attrs, mode, dev)
    grad = mode != "eval"
    gen = torch.Generator().manual_seed(1)
    xyz = torch.rand(B, N, 3, generator=gen).to(dev)
    if kind in ("sa", "msg"):
        feats = torch.randn(B, N, CFEAT, generator=gen).to(dev)

        def forward(x, f):
            if style == "geometry":
                with torch.no_grad():
                    g = mod.geometry(x.detach(), plans=bool(attrs.get("index_plans")))
                return mod(x, f, geometry=g)[1]
            if style == "lengths":
                return mod(x, f, lengths=LENGTHS)[1]
            return mod(x, f)[1]
    else:
        known = xyz[:, :FP_M].contiguous()
        feats = torch.randn(B, FP_N, FP_C1, generator=gen).to(dev)
        feats2 = torch.randn(B, FP_M, FP_C2, generator=gen).to(dev)

        def forward(x, f):
            f2 = feats2.clone().requires_grad_(grad)
            if style == "geometry":
                return mod(x, known, f, f2, geometry=FPGeometry(*three_nn(x, known)))
            if style == "lengths":
                return mod(x, known, f, f2, lengths1=LENGTHS)
            return mod(x, known, f, f2)

    def step():
        mod.zero_grad(set_to_none=True)
        x = xyz.clone().requires_grad_(xyz_grad)
        f = feats.clone().requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            out = forward(x, f)
            if grad:
                out.sum().backward()
        return mod.last_path
    return step


def census(case, style, dev, monkeypatch):
    """-> {"last_path": ..., "calls": {entry name: count}} of one counted step behind one warm step."""
    from pointnet2_amd import _C, train_mlp
    if case[1] == "fp_node":
        monkeypatch.setattr(train_mlp, "FP_NODE_MIN_SAVED", 0)
    step = make_step(case, style, dev)
    step()
    counts = collections.Counter()
    proxy = _CountingLibrary(_C.lib(), counts)
    monkeypatch.setattr(_C, "lib", lambda: proxy)
    try:
        path = step()
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    return {"last_path": path, "calls": dict(sorted(counts.items()))}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_covers_exactly_the_case_list(golden):
    assert sorted(golden) == sorted(CASE_IDS)


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_module_path_calls_the_recorded_entries(cuda, monkeypatch, golden, case_id):
    name, style = case_id.rsplit("-", 1)
    case = next(c for c in CASES if c[0] == name)
    got = census(case, style, cuda, monkeypatch)
    want = golden[case_id]
    assert got["last_path"] == want["last_path"]
    assert got["calls"] == want["calls"]
