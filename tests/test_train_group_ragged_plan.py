"""Which masked kernels the cases of tests/test_train_group_ragged_gpu.py run, proved on the CPU from the library's own size rules
(train_mlp.group_ragged_plan -> pn2_mlp_train_group_ragged_plan: gemm_shape, wgrad_shape(gather) and prep_gemm under
ragged_group_opts). The node adds two families of matrix-core kernels to the plain rows' masked ones:

(a) tl_gemm_masked_kernel<NS, A_GATHER>, NS 1 / 2 / 4 -- the union over the table must reach every one, each with resident and
    with streamed weights;
(b) tl_wgrad_masked_gather_kernel<TPW, UPW> -- the union must reach every (TPW, UPW) pair that wgrad_shape(gather = true) can
    produce for a supported shape. The pairs are ENUMERATED from the rule here, over every tile count of both operands (the rule
    looks at tiles(cin), tiles(cout) and rows / 32 only) and row counts from 32 to 2^20, not listed by hand. Every pair the rule
    produces is reachable below 33 k rows, so none is excused. (TPW, UPW) does not depend on the device's CU count.

Neither needs a GPU: the plan entries are host logic."""
import pytest

from train_group_ragged_cases import CASES, dims

pytestmark = pytest.mark.filterwarnings("ignore")


def _plan(case):
    from pointnet2_amd import train_mlp
    b, n, m, ns, cfeat, has_idx, widths = dims(case)
    with train_mlp.options(**case.get("opts", {})):
        return train_mlp.group_ragged_plan(b, n, m, ns, cfeat, widths, has_idx)


def test_every_case_is_supported_and_runs_the_gathered_masked_passes():
    for name, case in CASES.items():
        plan = _plan(case)
        nl = len(case["widths"])
        fwd = [p for p in plan if not p["backward"]]
        assert [p["amode"] for p in fwd] == ["A_GATHER"] + ["A_RELU"] * (nl - 1), name
        assert all(p["masked"] for p in plan), name
        wg = [p for p in plan if p["kind"] == "wgrad"]
        assert [p["layer"] for p in wg] == list(range(nl, 0, -1)) and [p["gather"] for p in wg] == [False] * (nl - 1) + [True], name
        dg = [p for p in plan if p["kind"] == "gemm" and p["backward"]]
        assert all(p["amode"] == "A_DZ" for p in dg), name
        # layer 1's data gradient goes to the cfeat feature columns, and is absent without features
        assert [p["layer"] for p in dg] == list(range(nl, 1 if case["cfeat"] == 0 else 0, -1)), name
        if case["cfeat"]:
            assert dg[-1]["N"] == case["cfeat"], name


def test_union_reaches_every_gathered_masked_gemm():
    got = set()
    for case in CASES.values():
        p = _plan(case)[0]
        got.add((p["ns"], p["resident"]))
    assert got == {(ns, res) for ns in (1, 2, 4) for res in (True, False)}, sorted(got)


def _reachable_pairs(max_rows):
    """every (TPW, UPW) of the gathered weight gradient over supported one-layer levels of at most max_rows rows"""
    from pointnet2_amd import train_mlp
    pairs = {}
    for blocks in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 2048, 4096, 32768):
        rows = 32 * blocks
        if rows > max_rows:
            continue
        for tu in range(1, 21):                                    # tiles of the gathered input: cin = 3 + cfeat
            for tt in list(range(1, 18)) + [24, 32, 33, 64]:       # tiles of the output
                plan = train_mlp.group_ragged_plan(1, 64, blocks, 32, 32 * tu - 3, [32 * tu, 32 * tt])
                p = [q for q in plan if q["kind"] == "wgrad"][0]
                assert p["gather"]
                pairs.setdefault((p["tpw"], p["upw"]), (rows, tu, tt))
    return pairs


def test_union_reaches_every_gathered_weight_gradient_pair():
    everywhere = _reachable_pairs(1 << 20)
    small = _reachable_pairs(33 * 1024)
    assert set(everywhere) == set(small), "a pair only reachable above 33 k rows: %s" % (set(everywhere) - set(small),)
    assert all(tpw in (1, 2, 4) and upw in (1, 2, 3) for tpw, upw in everywhere)           # what is instantiated
    got = set()
    for case in CASES.values():
        p = [q for q in _plan(case) if q["kind"] == "wgrad" and q["gather"]][0]
        got.add((p["tpw"], p["upw"]))
    assert got == set(small), "cases reach %s, the rule produces %s" % (sorted(got), sorted(small))
