"""The ragged training nodes (pn2_mlp_train_*_ragged, pn2_mlp_train_*_fp_ragged) at the widths of the model's FP levels, where the
size rules pick the masked kernels the small ragged cases never reach: tl_gemm_masked_kernel<NS 1 / 2 / 4, A_PLAIN / A_RELU /
A_DZ> with resident and with streamed weights, tl_wgrad_masked_kernel<TPW, UPW> at all six reachable pairs, non-temporal stores,
the options that act on a ragged node and those that are ignored. The cases and what each is for: train_ragged_wide_cases.py;
that they reach those kernels: test_train_ragged_wide_plan.py (no GPU needed).

Helpers, seeds and references are those of tests/test_train_ragged_gpu.py (plain rows: seeds 91 / 92 / 93, 94 for the stack / the
inputs / the padding fills) and tests/test_fp_level_ragged_gpu.py (FP node: 101 / 102 / 103; geometry and three_nn(..., lengths1=)
as there). A case's runs -- padding rows of x / points1, grad_out and (FP) dist as zeros, finite random values and NaN -- and its
float64 reference are computed once per module; the FP node runs under set_deterministic(True) (that file's docstring says why).

Float64. Reference: the stack on the compacted valid rows in torch float64; its GRADIENTS take the kernels' own ReLU decisions
(relu(a z + c) > 0 from the saved z_l and (a, c)) under the cap of tests/test_fp_level_ragged_gpu.py -- at most 1e-5 N_valid
sum(widths) decisions differ, each with |y| <= 1e-5 of its layer's scale: a condition, asserted. Bound per tensor:
max(1e-5, 2 x the worst error of torch's own fp32 evaluation of the same formulas against float64's own results) of the tensor's
largest magnitude (tests/test_train_mlp_gpu.py's rule; the fp32 evaluation never sees the node, and its gradients take float64's
decisions -- rounding is what it measures, not a ReLU that one decision moves). It came to 1e-5 at every case: torch fp32's worst
error is 0.9e-6 .. 4.0e-6.
The seeds hold the cap where it can be checked without the node: a torch fp32 evaluation on the CPU against float64 on the compacted
rows (cpu_decision_counts below; FP geometry by torch.cdist) differs in
    W1 / W1_* 1 (margin 2.1e-8), W2 0, W3 0, W4 / W4_* 0, F1 1 (margin 9.7e-9), F2 0, F3 0 decisions
    against caps of 60.6, 60.4, 69.5, 66.6, 36.3, 36.3, 36.3 (9461 / 9445 / 18097 / 9461 valid rows).
Measured on an MI355X -- the worst error over a case's tensors, relative to the tensor's largest magnitude, against the bound of
1e-5, and the kernels' decisions that differ from float64's:
    W1 and its eight option cases  2.66e-6 (layer 1 grad_beta), 0 decisions      W2  1.99e-6 (layer 1 grad_beta), 0
    W3  2.94e-6 (layer 1 grad_beta), 1 (margin 1.8e-8)                          W4 and its two option cases  2.31e-6 (layer 2 grad_beta), 0
    F1  1.56e-6 (layer 1 grad_beta), 1 (3.3e-9)     F2  1.83e-6 (layer 1 grad_beta), 1 (3.0e-8)     F3  1.49e-6 (layer 1 grad_beta), 1 (3.4e-8)
The whole file takes 9 s; no case's test more than 2 s (the first, which loads the kernels)."""
import copy

import numpy as np
import pytest
import torch

import test_fp_level_ragged_gpu as F
import test_train_ragged_gpu as R
import train_ragged_wide_cases as W

pytestmark = pytest.mark.gpu

TOL = 1e-5                                                       # README, tests/test_train_mlp_gpu.py
FILLS = ("zero", "random", "nan")
IGNORED = dict(fuse_wgrad=True, pair_launch=True, side_stream=True, fold_finalize=True)
ALL = sorted(W.PLAIN) + sorted(W.FP)


def _case(name):
    return W.PLAIN[name] if name in W.PLAIN else W.FP[name]


def _options(case, extra=None):
    from pointnet2_amd import train_mlp
    return train_mlp.options(**dict(case.get("opts", {}), **(extra or {})))


# ---- the plain-rows node: tests/test_train_ragged_gpu.py's _run, which also keeps the saved z_l and (mean, invstd, a, c) ----
def _plain_call(net, x, gout, lens):
    """one forward + backward on a copy of `net`; lens: (b,) int32 on the device, or None for the dense node"""
    from pointnet2_amd import train_mlp
    net = copy.deepcopy(net)
    x = x.clone().requires_grad_(True)
    bns = [mod for mod in net if isinstance(mod, torch.nn.BatchNorm2d)]
    out = train_mlp.fp_mlp_train(net, x, **({} if lens is None else {"lengths": lens}))
    res = {}
    if lens is not None:
        saved = out.grad_fn.next_functions[0][0].saved_tensors
        saved, nl = saved[:len(saved) - 2], len(bns)                           # behind `out`: the mask and the lengths
        res["zs"] = [t.detach() for t in saved[-(2 * nl + 1):-(nl + 1)]]
        res["saves"] = [t.detach() for t in saved[-(nl + 1):-1]]
    out.backward(gout)
    res.update(out=out.detach(), grad_x=x.grad, param_grads=[p.grad for p in net.parameters()],
               running=[t.detach().clone() for mod in bns for t in (mod.running_mean, mod.running_var)])
    return res


def _plain_run(case, cuda, fill, lengths="case", extra=None):
    lens = case["lengths"] if lengths == "case" else lengths
    x, gout = R._inputs(case, cuda, fill, lens)
    with _options(case, extra):
        return _plain_call(R._net(case, cuda), x, gout, torch.tensor(lens, dtype=torch.int32, device=cuda) if lens is not None else None)


def _plain_reference(case, dev, zs=None, saves=None, dtype=torch.float64):
    """tests/test_train_ragged_gpu.py::_reference in `dtype` -- the stack on the compacted valid rows -- whose GRADIENTS take the
    kernels' ReLU decisions when zs / saves are given (as tests/test_fp_level_ragged_gpu.py::_reference) -> results, the number of
    decisions that differ from this evaluation's own, their largest |y| relative to the layer's scale"""
    net = R._net(case, dev)
    x, gout = R._inputs(case, dev, "zero")
    valid = R._valid(case, dev).reshape(-1)
    h = x.reshape(-1, case["cin"])[valid].to(dtype).requires_grad_(True)
    params, running, signs, cur, flips, margin, own = [], [], [], h, 0, 0.0, None
    mods = list(net)
    for l in range(len(mods) // 3):
        conv, bn = mods[3 * l], mods[3 * l + 1]
        w = conv.weight.detach().to(dtype).reshape(conv.out_channels, -1).requires_grad_(True)
        bias = conv.bias.detach().to(dtype).requires_grad_(True)
        gamma, beta = bn.weight.detach().to(dtype).requires_grad_(True), bn.bias.detach().to(dtype).requires_grad_(True)
        z = cur @ w.t() + bias
        cnt = z.shape[0]
        mean, var = z.mean(dim=0), z.var(dim=0, unbiased=False)
        y = (z - mean) / torch.sqrt(var + bn.eps) * gamma + beta
        params += [w, bias, gamma, beta]
        m = bn.momentum
        running += [(1 - m) * bn.running_mean.to(dtype) + m * mean.detach(),
                    (1 - m) * bn.running_var.to(dtype) + m * var.detach() * cnt / max(cnt - 1, 1)]
        own = torch.relu(y).detach()
        mask = y.detach() > 0
        signs.append(mask)
        if zs is not None:
            mask = (saves[l][2] * zs[l] + saves[l][3])[valid].to(y.device) > 0
            dis = (y.detach() > 0) != mask
            flips += int(dis.sum())
            if dis.any():
                margin = max(margin, float(y.detach()[dis].abs().max() / y.detach().abs().max()))
        cur = y * mask.to(dtype)
    grads = torch.autograd.grad(cur, [h] + params, gout.reshape(-1, gout.shape[2])[valid].to(dtype))
    return {"out": own, "grad_x": grads[0], "param_grads": list(grads[1:]), "running": running, "valid": valid, "signs": signs}, flips, margin


def _plain_flat(res):
    return [res["out"], res["grad_x"]] + list(res["param_grads"]) + list(res["running"])


# ---- the FP node: tests/test_fp_level_ragged_gpu.py's _run under the case's options ----
def _fp_run(case, cuda, fill, lengths="case", extra=None):
    with _options(case, extra):
        return F._run(case, cuda, fill, lengths=lengths)


def _run(name, cuda, fill, lengths="case", extra=None):
    case = _case(name)
    return (_plain_run if name in W.PLAIN else _fp_run)(case, cuda, fill, lengths, extra)


def _flat(name, res):
    return _plain_flat(res) if name in W.PLAIN else F._flat(res)


def _padding(name, cuda):
    return ~R._valid(_case(name), cuda)                                       # (b, n); both files clamp alike


@pytest.fixture(scope="module")
def results(cuda):
    """(case name, fill) -> the node's results; each computed once, on first use, never changed"""
    cache = {}

    def get(name, fill):
        if (name, fill) not in cache:
            cache[(name, fill)] = _run(name, cuda, fill)
        return cache[(name, fill)]
    return get


def _assert_same(name, a, b, what):
    fa, fb = _flat(name, a), _flat(name, b)
    assert len(fa) == len(fb)
    for i, (u, v) in enumerate(zip(fa, fb)):
        assert F._same_bits(u, v), (what, i)


@pytest.mark.parametrize("name", ALL)
def test_padding_invariance_bit_for_bit(cuda, results, name):
    """1: zeros, finite random values and NaN on the padding rows of x / points1, grad_out and (FP) dist: every output, gradient and
    running statistic the same bits, all finite"""
    base = results(name, "zero")
    flat = _flat(name, base)
    assert all(bool(torch.isfinite(t).all()) for t in flat)
    assert all(float(t.abs().sum()) > 0 for t in flat[:2])
    for fill in ("random", "nan"):
        _assert_same(name, base, results(name, fill), fill)


@pytest.mark.parametrize("name", ALL)
def test_padding_rows_are_exact_zeros(cuda, results, name):
    """2: out, grad_x / grad_points1 and (FP) weight: all-zero bits on the padding rows"""
    pad = _padding(name, cuda)
    assert int(pad.sum()) > 0
    whats = ("out", "grad_x") if name in W.PLAIN else ("out", "grad_p1", "weight")
    for fill in FILLS:
        res = results(name, fill)
        for what in whats:
            if res[what] is None:
                continue
            bits = res[what].reshape(pad.shape[0], pad.shape[1], -1)[pad].contiguous().view(torch.int32)
            assert int((bits != 0).sum()) == 0, (fill, what)


@pytest.mark.parametrize("name", ALL)
def test_saved_z_rows_are_zero_exactly_on_padding(cuda, results, name):
    """3: a row of every saved z_l is all-zero bits exactly where the row is padding -- a masked pass that took a neighbouring
    item's validity word would zero valid rows or fill padding rows"""
    pad = _padding(name, cuda).reshape(-1)
    for fill in FILLS:
        zs = results(name, fill)["zs"]
        assert len(zs) == len(_case(name)["mlp"])
        for l, z in enumerate(zs):
            zero_row = (z.reshape(pad.shape[0], -1).contiguous().view(torch.int32) == 0).all(dim=1)
            assert int((zero_row & ~pad).sum()) == 0, (fill, l, "a valid row was taken for padding")
            assert int((~zero_row & pad).sum()) == 0, (fill, l, "a padding row was let in")


@pytest.mark.parametrize("name", ALL)
def test_full_lengths_equal_the_dense_node(cuda, name):
    """4: lengths = (n, ..., n): the dense node's results under the same options, bit for bit"""
    case = _case(name)
    ragged = _run(name, cuda, "none", lengths=(case["n"],) * case["b"])
    dense = _run(name, cuda, "none", lengths=None)
    _assert_same(name, ragged, dense, "dense")


@pytest.mark.parametrize("name", ALL)
def test_run_to_run(cuda, results, name):
    """5"""
    _assert_same(name, results(name, "nan"), _run(name, cuda, "nan"), "again")


@pytest.mark.parametrize("name", ALL)
def test_ignored_options(cuda, results, name):
    """6: fuse_wgrad, pair_launch, side_stream and fold_finalize switched ON: the default call's bits"""
    _assert_same(name, results(name, "random"), _run(name, cuda, "random", extra=IGNORED), "ignored options")


def _compare(name, got, want, base32, cap_rows, flips, margin):
    """got (the node) against want (float64, the kernels' decisions); base32: (fp32, float64) pairs of torch's own evaluations"""
    case = _case(name)
    cap = 1e-5 * cap_rows * sum(case["mlp"])
    print("case %s: %d valid rows, %d ReLU decisions differ from float64's (cap %.1f), margin %.2e" % (name, cap_rows, flips, cap, margin))
    assert flips <= cap and margin <= 1e-5, (flips, margin)

    def rel(g, w):
        g, w = g.detach().double().cpu().reshape(w.shape).numpy(), w.detach().double().cpu().numpy()
        return float(np.abs(g - w).max()) / max(1e-30, float(np.abs(w).max()))

    baseline = max(rel(g, w) for g, w in base32)
    bound = max(TOL, 2.0 * baseline)
    print("case %s: torch fp32 against float64: worst %.3e -> bound %.3e of each tensor's largest magnitude" % (name, baseline, bound))
    errors, worst = [], (0.0, "")
    for label, g, w in _got_want_pairs(name, got, want):
        err = rel(g, w)
        print("case %s %s: error %.3e (bound %.3e)" % (name, label, err, bound))
        worst = max(worst, (err, label))
        if err > bound:
            errors.append((label, err))
    print("case %s WORST %.3e (%s), bound %.3e" % (name, worst[0], worst[1], bound))
    assert not errors, errors


def _got_want_pairs(name, got, want):
    """(label, the node's tensor on the valid rows, the reference's) of everything item 7 compares"""
    v = want["valid"]
    rows = lambda t: t.reshape(v.shape[0], -1).to(v.device)[v]               # noqa: E731
    pairs = [("out", rows(got["out"]), want["out"])]
    if name in W.PLAIN:
        pairs.append(("grad_x", rows(got["grad_x"]), want["grad_x"]))
    else:
        pairs.append(("grad_points2", got["grad_p2"], want["grad_p2"]))
        if want["grad_p1"] is not None:
            pairs.append(("grad_points1", rows(got["grad_p1"]), want["grad_p1"]))
    kinds = ("grad_weight", "grad_bias", "grad_gamma", "grad_beta")
    for i, (g, w) in enumerate(zip(got["param_grads"], want["param_grads"])):
        if i % 4 == 1:              # the conv bias under batch norm: its gradient is identically zero, float64 returns its own
            assert int((g != 0).sum()) == 0 and float(w.abs().max()) <= 1e-9 * float(want["param_grads"][i - 1].abs().max())   # rounding there
            continue
        pairs.append(("layer %d %s" % (i // 4 + 1, kinds[i % 4]), g, w))
    for i, (g, w) in enumerate(zip(got["running"], want["running"])):
        pairs.append(("layer %d %s" % (i // 2 + 1, ("running_mean", "running_var")[i % 2]), g, w))
    return pairs


def _references(name, dev, zs, saves, own_decisions=False):
    """-> float64 with the given ReLU decisions, the number of decisions that differ from its own, their margin; torch's own
    evaluations in fp32 (on float64's decisions, unless own_decisions) and in float64"""
    case = _case(name)
    if name in W.PLAIN:
        def ref(dtype, z=None, s=None):
            return _plain_reference(case, dev, z, s, dtype)
    else:
        p2, p1, idx, dist, gout = F._inputs(case, dev, "zero") if dev.type == "cuda" else _cpu_fp_inputs(case)
        valid = R._valid(case, dev)

        def ref(dtype, z=None, s=None):
            return F._reference(F._net(case, dev), p2, p1, idx, dist, gout, valid, z, s, dtype)
    want, flips, margin = ref(torch.float64, zs, saves)
    own64 = ref(torch.float64)[0]
    # torch's fp32 evaluation of the same formulas ON float64's LINEAR PIECE: with its own decisions one ReLU within rounding of zero
    # moves single gradient elements by their whole value (measured at W3 / F1: one such decision, 0.14 / 0.05 of grad_x's /
    # grad_points1's largest magnitude) and the bound made from it would check nothing
    own32 = ref(torch.float32)[0] if own_decisions else ref(torch.float32, *_as_saved(own64["signs"], R._valid(case, dev).reshape(-1)))[0]
    return want, flips, margin, own32, own64


def _as_saved(signs, valid):
    """ReLU decisions (N_valid, C_l) per layer -> (zs, saves) that a reference reads them back from: z := the decision, a := 1,
    c := -1/2"""
    zs, saves = [], []
    for sign in signs:
        c = sign.shape[1]
        z = torch.zeros(valid.shape[0], c, device=sign.device)
        z[valid.to(sign.device)] = sign.float()
        zs.append(z)
        saves.append(torch.stack([torch.zeros(c), torch.zeros(c), torch.ones(c), torch.full((c,), -0.5)]).to(sign.device))
    return zs, saves


def _own_pairs(name, a, b):
    """_got_want_pairs for two reference evaluations (both already on the valid rows)"""
    pairs = [(a["out"], b["out"])]
    if name in W.PLAIN:
        pairs.append((a["grad_x"], b["grad_x"]))
    else:
        pairs.append((a["grad_p2"], b["grad_p2"]))
        if b["grad_p1"] is not None:
            pairs.append((a["grad_p1"], b["grad_p1"]))
    pairs += [(g, w) for i, (g, w) in enumerate(zip(a["param_grads"], b["param_grads"])) if i % 4 != 1]
    return pairs + list(zip(a["running"], b["running"]))


@pytest.mark.parametrize("name", ALL)
def test_float64(cuda, results, name):
    """7: outputs on the valid rows, every parameter gradient, running_mean and running_var against torch float64 on the compacted
    valid rows"""
    got = results(name, "random")
    want, flips, margin, own32, own64 = _references(name, cuda, got["zs"], got["saves"])
    _compare(name, got, want, _own_pairs(name, own32, own64), int((~_padding(name, cuda)).sum()), flips, margin)


# ---- 8: lengths outside 1..n are clamped on the device ----
BAD, CLAMPED = (0, -5, 1024 + 7, 300), (1, 1, 1024, 300)                     # case A of both files: b 4, n 1024


def test_plain_lengths_outside_are_clamped(cuda):
    case = R.CASES["A"]
    x, gout = R._inputs(case, cuda, "nan", CLAMPED)
    net = R._net(case, cuda)
    bad = _plain_call(net, x, gout, torch.tensor(BAD, dtype=torch.int32, device=cuda))
    good = _plain_call(net, x, gout, torch.tensor(CLAMPED, dtype=torch.int32, device=cuda))
    assert all(bool(torch.isfinite(t).all()) for t in _plain_flat(bad))
    for i, (u, v) in enumerate(zip(_plain_flat(bad) + bad["zs"], _plain_flat(good) + good["zs"])):
        assert F._same_bits(u, v), i
    pad = ~R._valid(case, cuda, CLAMPED)
    assert int((bad["out"][pad].contiguous().view(torch.int32) != 0).sum()) == 0
    assert float(bad["out"][~pad].abs().sum()) > 0


def test_fp_lengths_outside_are_clamped(cuda):
    case = F.CASES["A"]
    tensors = F._inputs(case, cuda, "nan", CLAMPED)
    net = F._net(case, cuda)
    with F._deterministic():
        bad = F._call(copy.deepcopy(net), tensors, torch.tensor(BAD, dtype=torch.int32, device=cuda))
        good = F._call(copy.deepcopy(net), tensors, torch.tensor(CLAMPED, dtype=torch.int32, device=cuda))
    assert all(bool(torch.isfinite(t).all()) for t in F._flat(bad))
    for i, (u, v) in enumerate(zip(F._flat(bad) + bad["zs"], F._flat(good) + good["zs"])):
        assert F._same_bits(u, v), i
    pad = ~R._valid(case, cuda, CLAMPED)
    assert int((bad["out"][pad].contiguous().view(torch.int32) != 0).sum()) == 0


# ---- the seeds' condition without the node (on a CPU: python tests/test_train_ragged_wide_gpu.py) ----
def _cpu_fp_inputs(case):
    """F._inputs(case, cpu, "zero") with the three nearest known points by torch.cdist instead of three_nn"""
    xyz1, xyz2, p2, p1, gout = F._raw(case)
    d2 = torch.cdist(xyz1.double(), xyz2.double()) ** 2
    dist, idx = torch.topk(d2, 3, dim=2, largest=False)
    return p2, p1, idx.int(), dist.float(), gout


def cpu_decision_counts(names=("W1", "W2", "W3", "W4", "F1", "F2", "F3")):
    """per base case (the option cases share their base's tensors): how many ReLU decisions of a torch fp32 evaluation differ from
    float64's on the compacted rows and their margin -- the fp32 decisions handed to the float64 reference as if they were the
    kernels' (z := the decision, a := 1, c := -1/2) -- beside the cap"""
    dev = torch.device("cpu")
    for name in names:
        case = _case(name)
        valid = R._valid(case, dev).reshape(-1)
        own32 = _references(name, dev, None, None, own_decisions=True)[3]
        _, flips, margin, _, _ = _references(name, dev, *_as_saved(own32["signs"], valid))
        nv = int(valid.sum())
        print("%s: %d valid rows, cap %.1f, fp32 decisions differing from float64's: %d, margin %.2e" %
              (name, nv, 1e-5 * nv * sum(case["mlp"]), flips, margin))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    cpu_decision_counts()
