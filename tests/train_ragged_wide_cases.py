"""The ragged training nodes at the widths of the model's FP levels: one case table, shared by the host-only test of what each
case launches (test_train_ragged_wide_plan.py, through train_mlp.ragged_plan) and by the GPU test that runs them
(test_train_ragged_wide_gpu.py).

The widths select the kernels (csrc/train_mlp.hip: gemm_shape, pick_ns, wgrad_shape), the rows keep the few-rows loops from
shrinking them: every case has at least 16320 rows and at most 32768, layers of at most 256 channels (F1's input: 320). What each base case is for, with the
masked instantiations the plan test found for it (GEMM: NS, AMODE, weights; weight gradient: TPW, UPW):

PLAIN["W1"]  b 8, n 2048, 256 -> 256 -> 256 -> 128. Lengths: n itself, multiples of 32 (1024, 64), non-multiples (1500, 777, 1999)
             and 1 -- tiles fully valid, fully padding and mixed. NS 4 streamed (A_PLAIN, A_RELU, A_DZ at K = 256), NS 2
             resident (A_RELU into the 128-wide top), NS 4 resident (A_DZ at K = 128); weight gradients (4, 3) and (2, 2).
PLAIN["W2"]  the same with n 2040: b n is a multiple of 32, n is not -- a validity word spans two clouds. The same kernels.
PLAIN["W3"]  b 16, n 2048 (32768 rows), 128 -> 128 -> 128 -> 128 (sem_seg FP4's widths): NS 4 resident in all three modes; (2, 2).
PLAIN["W4"]  b 8, n 2048, 32 -> 256 -> 64 -> 256 -> 64 -> 64: the narrow layers of a wide level, for the weight-gradient shapes
             with ONE output tile per wave -- (1, 3), (1, 2), (1, 1), the only ones wgrad_two_per_cu acts on -- and (2, 3); the GEMMs
             into 64 columns run NS 1 (the few-rows loop of gemm_shape), those into 256 NS 4 resident.
W1 under options, a case each: max_ns 1 and 2 (NS 1 / NS 2 resident, all modes), force_stream (the streamed path at the rule's own
NS), both together (NS 1 / NS 2 streamed: at these widths no rule streams them unasked), nt on (non-temporal stores: the automatic
rule starts at 128 MB of output), wgrad_two_per_cu on / off (no pass of W1 qualifies: one output tile and two units per wave at
most -- so W4 takes the two as well).

FP["F1"]     sem_seg FP3-like: b 8, n 2048, m 257 (b m = 2056 known points: not a multiple of 32), c2 256, c1 64, 320 -> 256 ->
             128. The rows half of layer 1 is masked: weight gradient (2, 3) over (64, 256), grad_points1 by NS 1 A_PLAIN
             resident (K = 256, N = 64); layer 2: NS 2 A_RELU resident forward, (2, 2) and NS 4 A_DZ resident backward.
FP["F2"]     the same with c1 = 0: no rows half at all (layer 1 masked only in its two vector-unit passes).
FP["F3"]     the same with c1 = 6 (zero-padded to 8): rows half (1, 3) over (8, 256), grad_points1 by NS 1 A_PLAIN resident.

A case: the shape, `lengths`, and `opts` -- the keyword arguments of train_mlp.options() it runs under."""

_L2048 = (2048, 1500, 1024, 777, 1, 64, 2048, 1999)
_W1 = dict(b=8, n=2048, lengths=_L2048, cin=256, mlp=[256, 256, 128])
_W4 = dict(b=8, n=2048, lengths=_L2048, cin=32, mlp=[256, 64, 256, 64, 64])


def _with(base, **opts):
    return dict(base, opts=opts)


PLAIN = {
    "W1": _with(_W1),
    "W2": _with(dict(_W1, n=2040, lengths=(2040, 1500, 1024, 777, 1, 64, 2040, 1999))),
    "W3": _with(dict(b=16, n=2048, lengths=_L2048 + (33, 2047, 2048, 96, 1280, 5, 2016, 1111), cin=128, mlp=[128, 128, 128])),
    "W4": _with(_W4),
    "W1_ns1": _with(_W1, max_ns=1),
    "W1_ns2": _with(_W1, max_ns=2),
    "W1_stream": _with(_W1, force_stream=True),
    "W1_ns1_stream": _with(_W1, max_ns=1, force_stream=True),
    "W1_ns2_stream": _with(_W1, max_ns=2, force_stream=True),
    "W1_nt": _with(_W1, nt=True),
    "W1_two_on": _with(_W1, wgrad_two_per_cu=True),
    "W1_two_off": _with(_W1, wgrad_two_per_cu=False),
    "W4_two_on": _with(_W4, wgrad_two_per_cu=True),
    "W4_two_off": _with(_W4, wgrad_two_per_cu=False),
}

_F1 = dict(b=8, n=2048, m=257, lengths=_L2048, c2=256, c1=64, mlp=[256, 128])
FP = {
    "F1": _with(_F1),
    "F2": _with(dict(_F1, c1=0)),
    "F3": _with(dict(_F1, c1=6)),
}

# The cases the suite had before (tests/test_train_ragged_gpu.py, tests/test_fp_level_ragged_gpu.py: CASES there; the module
# test of tests/test_ragged_fp_fused_gpu.py runs the plain-rows node at 4 x 1024 rows, 38 -> 64 -> 32, case A's shape)
OLD_PLAIN = {
    "A": dict(b=4, n=1024, cin=38, mlp=[64, 32]),
    "B": dict(b=4, n=200, cin=32, mlp=[32, 32, 64]),
}
OLD_FP = {
    "A": dict(b=4, n=1024, m=256, c2=35, c1=6, mlp=[64, 32]),
    "B": dict(b=4, n=200, m=25, c2=32, c1=0, mlp=[32, 32, 64]),
    "C": dict(b=2, n=96, m=16, c2=16, c1=16, mlp=[32]),
}


def plan_of(case):
    """the passes of one forward + backward of the case (train_mlp.ragged_plan) under its options"""
    from pointnet2_amd import train_mlp
    with train_mlp.options(**case.get("opts", {})):
        if "c2" in case:
            return train_mlp.ragged_plan(case["b"], case["n"], [case["c2"] + case["c1"]] + case["mlp"], fp=(case["m"], case["c2"], case["c1"]))
        return train_mlp.ragged_plan(case["b"], case["n"], [(case["cin"] + 3) // 4 * 4] + case["mlp"])


def masked_gemms(passes):
    """{(NS, AMODE, "resident" | "streamed")} of the masked GEMMs"""
    return {(p["ns"], p["amode"], "resident" if p["resident"] else "streamed") for p in passes if p["kind"] == "gemm" and p["masked"]}


def masked_wgrads(passes):
    """{(TPW, UPW)} of the masked weight-gradient passes"""
    return {(p["tpw"], p["upw"]) for p in passes if p["kind"] == "wgrad" and p["masked"]}
