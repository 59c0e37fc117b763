"""Which C entry an operator call reaches, and with which arguments.

The module census (test_module_call_census_gpu.py) pins entry names and counts per module path. One level down nothing
did: an operator front that took the two-sided `_ragged_pair` entry with full counts where the one-sided `_ragged` entry
is meant -- or allocated where the caller's `out=` buffer should go -- passes every value test. Every case below calls one
public operator once warm and once with `_C.lib` replaced by a proxy that forwards every call of a pn2_* entry and records
it as [entry name, arguments], and compares the recording with tests/golden/operator_call_census.json EXACTLY, order
included (an operator's launches have a fixed order, unlike a module's).

An argument is recorded by the entry's declared argument type (_C._SIGNATURES): a host scalar keeps its value; a pointer
becomes None (NULL), "stream" (the launch's stream, always the last argument), the NAME of the caller's tensor whose
data_ptr() it equals (an input, or an out= tensor), or "fresh" (anything else: an allocation of the front's own, a view
into one). A host array (the multi-radius entry's radii, sample counts and output tables) becomes the list of its elements,
recorded the same way.

The golden file is written by scripts/record_operator_call_census.py, which runs THIS module's case list; it was recorded
on the commit before the operators' fronts were folded and is committed unchanged.

Shapes: the smallest at which every arm exists -- b = 2 clouds of n = 96 points (the cell-list kernel that
set_ball_query_kernel(2) forces needs n >= 64), m = 8 queries, nsample 4, k = 3; lengths1 = [96, 5], lengths2 = [8, 3]; the
packed form of that same batch, offsets [0, 96, 101] with max_points 96. Counts and offsets are int32 tensors on the
device, which the fronts hand on as they are (so they are recorded by name; full counts made by a front are "fresh")."""
import ctypes
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, M, NSAMPLE, K, RADIUS = 2, 96, 8, 4, 3, 0.3
LENGTHS1, LENGTHS2 = [96, 5], [8, 3]
OFFSETS, MAX_POINTS = [0, 96, 101], 96
MSG_RADII, MSG_NSAMPLES = [0.2, 0.4], [4, 6]
MSG_RADII5, MSG_NSAMPLES5 = [0.1, 0.2, 0.3, 0.4, 0.5], [2, 3, 4, 5, 6]        # beyond four radii: one launch per radius
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "operator_call_census.json")

BALL_LAYOUTS = ("dense", "dense_kernel2", "lengths1", "lengths2", "both", "packed", "packed_global")
RAGGED_LAYOUTS = ("dense", "lengths1", "lengths2", "both")


def _case_list():
    """[(case id, operator, layout, options)]"""
    cases = []
    for layout in BALL_LAYOUTS:
        for out in (False, True):
            cases.append(("query_ball_point-%s%s" % (layout, "-out" if out else ""), "query_ball_point", layout, {"out": out}))
        for want_idx in (True, False):
            for subtract in (True, False):
                cases.append(("query_ball_group_xyz-%s-%s-%s" % (layout, "idx" if want_idx else "noidx", "sub" if subtract else "nosub"),
                              "query_ball_group_xyz", layout, {"want_idx": want_idx, "subtract": subtract}))
    for layout in ("dense", "lengths1", "both"):
        cases.append(("query_ball_group_xyz_msg-%s" % layout, "query_ball_group_xyz_msg", layout, {"five": False}))
    for layout in ("dense", "both"):
        cases.append(("query_ball_group_xyz_msg-five_radii-%s" % layout, "query_ball_group_xyz_msg", layout, {"five": True}))
    for layout in RAGGED_LAYOUTS:
        cases.append(("knn_point-%s" % layout, "knn_point", layout, {"c": 3}))
    cases.append(("knn_point-dense-c2", "knn_point", "dense", {"c": 2}))
    for layout in RAGGED_LAYOUTS + ("packed", "packed_lengths2", "packed_global", "packed_global_lengths2"):
        for out in (False, True):
            cases.append(("three_nn-%s%s" % (layout, "-out" if out else ""), "three_nn", layout, {"out": out}))
    for layout in ("lengths", "npoints", "both"):
        cases.append(("sample_and_group_xyz-%s" % layout, "sample_and_group_xyz", layout, {}))
    return cases


CASES = _case_list()
CASE_IDS = [case[0] for case in CASES]


class _RecordingLibrary:
    """Forwards every attribute of the loaded library; calls of its pn2_* entries are recorded as [name, arguments]."""

    def __init__(self, lib, signatures, names, stream, calls):
        self._lib, self._signatures, self._names, self._stream, self._calls = lib, signatures, names, stream, calls

    def _pointer(self, value, last=False):
        if value is None:
            return None
        if last and value == self._stream:
            return "stream"
        return self._names.get(value, "fresh")

    def _argument(self, value, argtype, last):
        if isinstance(value, ctypes.Array):
            return [self._pointer(v) if value._type_ is ctypes.c_void_p else v for v in value]
        if argtype is ctypes.c_void_p:
            return self._pointer(value, last)
        return value

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pn2_"):
            return fn
        argtypes = self._signatures[name]

        def call(*args):
            assert len(args) == len(argtypes), name
            self._calls.append([name, [self._argument(a, t, i == len(args) - 1) for i, (a, t) in enumerate(zip(args, argtypes))]])
            return fn(*args)
        return call


def make_call(case, dev):
    """-> (call(): one call of the case's operator on fixed inputs, {name: the caller's tensor of that name})."""
    from pointnet2_amd import tf_grouping, tf_interpolate
    _, op, layout, opt = case
    gen = torch.Generator().manual_seed(0)
    cloud = torch.rand(B, N, opt.get("c", 3), generator=gen).to(dev)
    queries = cloud[:, :M].contiguous()
    flat = torch.cat([cloud[c, :k] for c, k in enumerate(LENGTHS1)]).contiguous()

    def counts(values):
        return torch.tensor(values, dtype=torch.int32, device=dev)

    packed = layout.startswith("packed")
    named, kw = {}, {}
    if op == "three_nn":                                  # xyz1 (b, n, 3) unknown, xyz2 (b, m, 3) known
        named["xyz1"], named["xyz2"] = (flat if packed else cloud), queries
        if layout in ("lengths1", "both"):
            kw["lengths1"] = named["lengths1"] = counts(LENGTHS1)
        if layout in ("lengths2", "both") or layout.endswith("lengths2"):
            kw["lengths2"] = named["lengths2"] = counts(LENGTHS2)
        if packed:
            kw["offsets1"] = named["offsets1"] = counts(OFFSETS)
            kw["max_points1"], kw["global_idx"] = MAX_POINTS, "global" in layout
        if opt["out"]:
            rows = (flat.shape[0],) if packed else (B, N)
            named["out[0]"] = torch.empty(rows + (3,), dtype=torch.float32, device=dev)
            named["out[1]"] = torch.empty(rows + (3,), dtype=torch.int32, device=dev)
            kw["out"] = (named["out[0]"], named["out[1]"])
        return (lambda: tf_interpolate.three_nn(named["xyz1"], named["xyz2"], **kw)), named
    if op == "sample_and_group_xyz":
        named["xyz"] = cloud
        if layout in ("lengths", "both"):
            kw["lengths"] = named["lengths"] = counts(LENGTHS1)
        if layout in ("npoints", "both"):
            kw["npoints"] = named["npoints"] = counts(LENGTHS2)
        return (lambda: tf_grouping.sample_and_group_xyz(M, RADIUS, NSAMPLE, cloud, **kw)), named
    named["xyz1"], named["xyz2"] = (flat if packed else cloud), queries
    if layout in ("lengths1", "both"):
        kw["lengths1"] = named["lengths1"] = counts(LENGTHS1)
    if layout in ("lengths2", "both"):
        kw["lengths2"] = named["lengths2"] = counts(LENGTHS2)
    if packed:
        kw["offsets"] = named["offsets"] = counts(OFFSETS)
        kw["max_points"], kw["global_idx"] = MAX_POINTS, "global" in layout
    if op == "knn_point":
        return (lambda: tf_grouping.knn_point(K, cloud, queries, **kw)), named
    if op == "query_ball_group_xyz_msg":
        radii, nsamples = (MSG_RADII5, MSG_NSAMPLES5) if opt["five"] else (MSG_RADII, MSG_NSAMPLES)
        return (lambda: tf_grouping.query_ball_group_xyz_msg(radii, nsamples, cloud, queries, **kw)), named
    if op == "query_ball_point":
        if opt["out"]:
            named["out[0]"] = torch.empty((B, M, NSAMPLE), dtype=torch.int32, device=dev)
            named["out[1]"] = torch.empty((B, M), dtype=torch.int32, device=dev)
            kw["out"] = (named["out[0]"], named["out[1]"])
        fn = lambda: tf_grouping.query_ball_point(RADIUS, NSAMPLE, named["xyz1"], queries, **kw)       # noqa: E731
    else:
        fn = lambda: tf_grouping.query_ball_group_xyz(RADIUS, NSAMPLE, named["xyz1"], queries, opt["subtract"],    # noqa: E731
                                                      opt["want_idx"], **kw)
    if layout != "dense_kernel2":
        return fn, named

    def forced():
        tf_grouping.set_ball_query_kernel(2)
        try:
            return fn()
        finally:
            tf_grouping.set_ball_query_kernel(0)
    return forced, named


def census(case, dev, monkeypatch):
    """-> [[entry name, [arguments]], ...] of one recorded call behind one warm call."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import stream_ptr
    call, named = make_call(case, dev)
    call()
    calls = []
    names = {t.data_ptr(): name for name, t in named.items()}
    assert len(names) == len(named)
    proxy = _RecordingLibrary(_C.lib(), _C._SIGNATURES, names, stream_ptr(dev), calls)
    monkeypatch.setattr(_C, "lib", lambda: proxy)
    try:
        kept = call()                                      # noqa: F841 -- results stay alive: no address is used twice
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    return calls


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_covers_exactly_the_case_list(golden):
    assert sorted(golden) == sorted(CASE_IDS)
    assert len(set(CASE_IDS)) == len(CASE_IDS)


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_operator_call_reaches_the_recorded_entries(cuda, monkeypatch, golden, case_id):
    case = next(c for c in CASES if c[0] == case_id)
    got = json.loads(json.dumps(census(case, cuda, monkeypatch)))
    assert got == golden[case_id]
