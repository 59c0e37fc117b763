"""Which masked kernels the ragged training nodes run at the cases of train_ragged_wide_cases.py -- asked of the library's own size
rules through pn2_mlp_train_ragged_plan / pn2_mlp_train_fp_ragged_plan (train_mlp.ragged_plan): host logic, no device.

(a) the union over the table reaches every tl_gemm_masked_kernel<NS, AMODE> (NS 1 / 2 / 4, A_PLAIN / A_RELU / A_DZ), each with
    resident and with streamed weights;
(b) ... and every (TPW, UPW) the weight-gradient rule can produce. The rule cuts at most 4 input and 8 output tiles into a slab:
    the test walks all 32 slab shapes through the entry. (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (4, 3) occur; the instantiated
    (2, 1), (4, 1) and (4, 2) cannot -- more than 8 output tiles need more than 4 tiles of operands;
(c) the ragged cases the suite had before reach NS 1 with resident weights and TPW 1 only.
`two` and the grid of a weight-gradient pass follow the device's CU count and are not asserted here."""
import ctypes

import pytest
import torch

import train_ragged_wide_cases as W

NS = (1, 2, 4)
AMODES = ("A_PLAIN", "A_RELU", "A_DZ")
TPW_UPW_INSTANTIATED = {(t, u) for t in (1, 2, 4) for u in (1, 2, 3)}
TPW_UPW_UNREACHABLE = {(2, 1), (4, 1), (4, 2)}

# what each new case must keep reaching (the GPU test relies on it: shrinking a case below a rule's threshold fails here)
EXPECT = {
    "W1": ({(4, "A_PLAIN", "streamed"), (4, "A_RELU", "streamed"), (2, "A_RELU", "resident"), (4, "A_DZ", "resident"), (4, "A_DZ", "streamed")},
           {(4, 3), (2, 2)}),
    "W3": ({(4, "A_PLAIN", "resident"), (4, "A_RELU", "resident"), (4, "A_DZ", "resident")}, {(2, 2)}),
    "W4": ({(4, "A_PLAIN", "resident"), (1, "A_RELU", "resident"), (4, "A_RELU", "resident"), (1, "A_DZ", "resident"), (4, "A_DZ", "resident")},
           {(1, 3), (1, 2), (2, 3), (1, 1)}),
    "W1_ns1": ({(1, m, "resident") for m in AMODES}, {(4, 3), (2, 2)}),
    "W1_ns2": ({(2, m, "resident") for m in AMODES}, {(4, 3), (2, 2)}),
    "W1_stream": ({(4, "A_PLAIN", "streamed"), (4, "A_RELU", "streamed"), (2, "A_RELU", "streamed"), (4, "A_DZ", "streamed")}, {(4, 3), (2, 2)}),
    "W1_ns1_stream": ({(1, m, "streamed") for m in AMODES}, {(4, 3), (2, 2)}),
    "W1_ns2_stream": ({(2, m, "streamed") for m in AMODES}, {(4, 3), (2, 2)}),
    "F1": ({(2, "A_RELU", "resident"), (4, "A_DZ", "resident"), (1, "A_PLAIN", "resident")}, {(2, 2), (2, 3)}),
    "F2": ({(2, "A_RELU", "resident"), (4, "A_DZ", "resident")}, {(2, 2)}),
    "F3": ({(2, "A_RELU", "resident"), (4, "A_DZ", "resident"), (1, "A_PLAIN", "resident")}, {(2, 2), (1, 3)}),
}
EXPECT["W2"] = EXPECT["W1"]
for _name in ("W1_nt", "W1_two_on", "W1_two_off"):
    EXPECT[_name] = EXPECT["W1"]
for _name in ("W4_two_on", "W4_two_off"):
    EXPECT[_name] = EXPECT["W4"]


def _all_cases():
    return dict(W.PLAIN, **W.FP)


def test_the_table_stays_small():
    for name, case in _all_cases().items():
        rows = case["b"] * case["n"]
        assert rows % 32 == 0 and rows <= 32768, name
        assert max([case.get("cin", 0), case.get("c2", 0) + case.get("c1", 0)] + case["mlp"]) <= 512, name
        assert len(case["lengths"]) == case["b"] and all(1 <= v <= case["n"] for v in case["lengths"]), name
    assert set(EXPECT) == set(_all_cases())


@pytest.mark.parametrize("name", sorted(_all_cases()))
def test_each_case_reaches_what_it_is_for(name):
    passes = W.plan_of(_all_cases()[name])
    gemms, wgrads = EXPECT[name]
    print(name, sorted(W.masked_gemms(passes)), sorted(W.masked_wgrads(passes)))
    assert W.masked_gemms(passes) == gemms
    assert W.masked_wgrads(passes) == wgrads


def test_plan_records():
    """the records of W1 and F1 in launch order: forward up, backward down, weight gradient before data gradient; the FP node's
    layer 1 as its two halves, the known-points half dense"""
    p = W.plan_of(W.PLAIN["W1"])
    assert [(q["kind"], q["backward"], q["layer"]) for q in p] == [("gemm", False, 1), ("gemm", False, 2), ("gemm", False, 3)] + \
        [(k, True, l) for l in (3, 2, 1) for k in ("wgrad", "gemm")]
    assert all(q["masked"] and q["rows"] == 16384 for q in p)
    assert [(q["K"], q["N"]) for q in p] == [(256, 256), (256, 256), (256, 128), (256, 128), (128, 256), (256, 256), (256, 256), (256, 256), (256, 256)]
    assert [q["amode"] for q in p if q["kind"] == "gemm"] == ["A_PLAIN", "A_RELU", "A_RELU", "A_DZ", "A_DZ", "A_DZ"]
    assert not any(q["nt"] for q in p if q["kind"] == "gemm")
    assert all(q["nt"] for q in W.plan_of(W.PLAIN["W1_nt"]) if q["kind"] == "gemm")
    f = W.plan_of(W.FP["F1"])
    mp = (8 * 257 + 31) // 32 * 32
    assert [(q["kind"], q["backward"], q["layer"], q["masked"], q["rows"], q["K"], q["N"]) for q in f] == [
        ("gemm", False, 1, False, mp, 256, 256), ("gemm", False, 1, False, 16384, 64, 256), ("gemm", False, 2, True, 16384, 256, 128),
        ("wgrad", True, 2, True, 16384, 256, 128), ("gemm", True, 2, True, 16384, 128, 256),
        ("wgrad", True, 1, False, mp, 256, 256), ("gemm", True, 1, False, mp, 256, 256),
        ("wgrad", True, 1, True, 16384, 64, 256), ("gemm", True, 1, True, 16384, 256, 64)]
    assert [q["masked"] for q in W.plan_of(W.FP["F2"]) if q["layer"] == 1] == [False, False, False]        # c1 = 0: no rows half
    f3 = [q for q in W.plan_of(W.FP["F3"]) if q["layer"] == 1 and q["masked"]]
    assert [(q["kind"], q["K"], q["N"]) for q in f3] == [("wgrad", 8, 256), ("gemm", 256, 6)]             # c1 6 read as 8 columns


def test_gemm_union_reaches_every_masked_instantiation():
    """(a)"""
    seen = set()
    for case in _all_cases().values():
        seen |= W.masked_gemms(W.plan_of(case))
    want = {(ns, m, r) for ns in NS for m in AMODES for r in ("resident", "streamed")}
    assert want - seen == set(), sorted(want - seen)
    assert seen - want == set()


def _slab_pairs():
    """(TPW, UPW) of every slab shape the rule can cut: tus <= 4 input tiles, tts <= 8 output tiles, through the entry (a one-layer
    stack of those widths at 32768 rows: nothing shrinks)"""
    from pointnet2_amd import train_mlp
    pairs = {}
    for tus in range(1, 5):
        for tts in range(1, 9):
            (w,) = [p for p in train_mlp.ragged_plan(16, 2048, [32 * tus, 32 * tts]) if p["kind"] == "wgrad"]
            assert (w["tus"], w["tts"], w["slabs"], w["masked"]) == (tus, tts, 1, True)
            pairs[(tus, tts)] = (w["tpw"], w["upw"])
    return pairs


def test_wgrad_union_reaches_every_reachable_pair():
    """(b)"""
    reachable = set(_slab_pairs().values())
    print("reachable (TPW, UPW):", sorted(reachable))
    assert reachable == TPW_UPW_INSTANTIATED - TPW_UPW_UNREACHABLE
    # wider layers are cut into slabs of at most 4 x 8 tiles: nothing new beyond the 32 shapes above
    from pointnet2_amd import train_mlp
    for widths in ([512, 512], [160, 288], [288, 160], [384, 96]):
        for p in train_mlp.ragged_plan(16, 2048, widths):
            if p["kind"] == "wgrad":
                assert p["tus"] <= 4 and p["tts"] <= 8 and (p["tpw"], p["upw"]) in reachable
    seen = set()
    for case in _all_cases().values():
        seen |= W.masked_wgrads(W.plan_of(case))
    assert seen == reachable, sorted(reachable - seen)


def test_the_old_cases_reach_one_organisation():
    """(c): the gap this table closes"""
    for name, case in sorted(W.OLD_PLAIN.items()) + sorted(W.OLD_FP.items()):
        passes = [p for p in W.plan_of(case) if p["masked"]]
        assert passes, name
        for p in passes:
            if p["kind"] == "gemm":
                assert (p["ns"], p["resident"]) == (1, True), (name, p)
            else:
                assert p["tpw"] == 1, (name, p)
            assert p["kind"] == "wgrad" or not p["nt"]


def test_ignored_options_do_not_change_the_plan():
    """ragged_opts: fuse_wgrad, pair_launch, side_stream and fold_finalize switched on change nothing a ragged call launches"""
    from pointnet2_amd import train_mlp
    for case in (W.PLAIN["W1"], W.PLAIN["W4"], W.FP["F1"]):
        with train_mlp.options(fuse_wgrad=True, pair_launch=True, side_stream=True, fold_finalize=True):
            assert W.plan_of(case) == W.plan_of(dict(case, opts={}))


def test_plan_entry_arguments():
    from pointnet2_amd import _C
    lib = _C.lib()
    widths = (ctypes.c_int * 3)(256, 256, 128)
    assert lib.pn2_mlp_train_ragged_plan(8, 2048, 2, None, None, None, 0) == -1
    assert lib.pn2_mlp_train_ragged_plan(8, 2047, 2, widths, None, None, 0) == -3          # b n % 32
    assert lib.pn2_mlp_train_ragged_plan(8, 2048, 2, widths, None, None, -1) == -3
    assert lib.pn2_mlp_train_ragged_plan(8, 2048, 2, widths, None, None, 0) == 6           # counting only
    buf = (ctypes.c_int * (2 * 14 + 1))(*([-7] * 29))
    assert lib.pn2_mlp_train_ragged_plan(8, 2048, 2, widths, None, buf, 2) == 6            # two records written, no more
    assert buf[0] == 0 and buf[14 + 2] == 2 and buf[28] == -7
    assert lib.pn2_mlp_train_fp_ragged_plan(8, 2047, 257, 256, 64, 2, widths, None, None, 0) == -3
    assert lib.pn2_mlp_train_fp_ragged_plan(8, 2048, 257, 256, 64, 2, None, None, None, 0) == -1
    fw = (ctypes.c_int * 3)(320, 256, 128)
    assert lib.pn2_mlp_train_fp_ragged_plan(8, 2048, 257, 256, 64, 2, fw, None, None, 0) == 9


def test_ragged_lengths_does_not_look_at_the_values():
    """lengths outside 1..n pass through untouched: the kernels clamp (tests/test_train_ragged_wide_gpu.py), check_lengths validates"""
    from pointnet2_amd._tensors import check_lengths, ragged_lengths
    bad = torch.tensor([0, -3, 2048 + 7, 5], dtype=torch.int64)
    got = ragged_lengths(bad, 4, torch.device("cpu"))
    assert got.dtype == torch.int32 and got.tolist() == [0, -3, 2055, 5]
    with pytest.raises(ValueError):
        check_lengths(bad, 2048)
