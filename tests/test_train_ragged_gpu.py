"""The fused training node on the plain rows of a ragged batch (train_mlp.fp_mlp_train(..., lengths=), pn2_mlp_train_*_ragged,
csrc/train_mlp_ragged.hip) on the GPU: batch statistics, running averages and every gradient over the valid rows only.

Case A: b 4, n 1024, lengths (1024, 700, 300, 64), stack 38 -> 64 -> 32 -- the odd width takes the zero-pad-to-40 path; 32-row
        tiles are fully valid, fully invalid, or mixed at a non-multiple of 32 (700, 300); one length is a multiple of 32.
Case B: b 4, n 200, lengths (200, 137, 1, 32), stack 32 -> 32 -> 32 -> 64 -- n % 32 != 0, so tiles hold parts of two clouds;
        one cloud has a single valid row; three layers.
The float64 reference of a case (the stack on the compacted valid rows, torch in float64) and the node's results per padding
fill are computed once per module and never changed."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {
    "A": dict(b=4, n=1024, lengths=(1024, 700, 300, 64), cin=38, mlp=[64, 32]),
    "B": dict(b=4, n=200, lengths=(200, 137, 1, 32), cin=32, mlp=[32, 32, 64]),
}
NAMES = ("out", "grad_x", "param_grads", "running")


def _net(case, cuda):
    """the case's stack with every parameter and running statistic away from its initial value"""
    from pointnet2_amd.pointnet_util import _SharedMLP
    torch.manual_seed(91)
    net = _SharedMLP(case["cin"], case["mlp"]).net
    with torch.no_grad():
        for mod in net:
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(-1.5, 1.5)                 # both signs
                mod.bias.uniform_(-0.5, 0.5)
                mod.running_mean.uniform_(-1.0, 1.0)
                mod.running_var.uniform_(0.5, 2.0)
    return net.to(cuda).train()


def _valid(case, cuda, lengths=None):
    lens = torch.tensor(lengths or case["lengths"], device=cuda).clamp(1, case["n"])
    return torch.arange(case["n"], device=cuda).unsqueeze(0) < lens.unsqueeze(1)          # (b, n)


def _inputs(case, cuda, fill, lengths=None):
    """x (b, n, cin) and grad_out (b, n, cout): the same valid rows for every fill; zeros, finite values or NaN on the others"""
    g = torch.Generator(device="cpu").manual_seed(92)
    x = torch.randn(case["b"], case["n"], case["cin"], generator=g).to(cuda)
    gout = torch.randn(case["b"], case["n"], case["mlp"][-1], generator=g).to(cuda)
    pad = ~_valid(case, cuda, lengths)
    for t, seed in ((x, 93), (gout, 94)):
        if fill == "zero":
            t[pad] = 0.0
        elif fill == "nan":
            t[pad] = float("nan")
        elif fill == "random":
            t[pad] = 3.0 * torch.randn(t[pad].shape, generator=torch.Generator(device="cpu").manual_seed(seed)).to(cuda)
    return x, gout


def _run(case, cuda, fill, lengths="case", net=None, **kw):
    """one forward + backward of the node on a fresh copy of the case's stack -> the four results (NAMES)"""
    from pointnet2_amd import train_mlp
    net = copy.deepcopy(net if net is not None else _net(case, cuda))
    lens = case["lengths"] if lengths == "case" else lengths
    x, gout = _inputs(case, cuda, fill, lens)
    x.requires_grad_(True)
    if lens is not None:
        kw["lengths"] = torch.tensor(lens, dtype=torch.int32, device=cuda)
    bns = [mod for mod in net if isinstance(mod, torch.nn.BatchNorm2d)]
    before = [int(mod.num_batches_tracked) for mod in bns]
    out = train_mlp.fp_mlp_train(net, x, **kw)
    out.backward(gout)
    running = [t.detach().clone() for mod in bns for t in (mod.running_mean, mod.running_var)]
    assert [int(mod.num_batches_tracked) for mod in bns] == [c + 1 for c in before]        # one batch counted
    return {"out": out.detach(), "grad_x": x.grad, "param_grads": [p.grad for p in net.parameters()], "running": running}


def _reference(case, cuda):
    """float64: the stack on the compacted valid rows (conv 1x1 + batch norm with batch statistics + ReLU, torch's conventions:
    the biased variance normalises, the unbiased one enters the running average)"""
    net = _net(case, cuda)
    x, gout = _inputs(case, cuda, "zero")
    valid = _valid(case, cuda).reshape(-1)
    h = x.reshape(-1, case["cin"])[valid].double().requires_grad_(True)
    params, running, cur = [], [], h
    mods = list(net)
    for i in range(0, len(mods), 3):
        conv, bn = mods[i], mods[i + 1]
        w = conv.weight.detach().double().reshape(conv.out_channels, -1).requires_grad_(True)
        bias = conv.bias.detach().double().requires_grad_(True)
        gamma, beta = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
        z = cur @ w.t() + bias
        cnt = z.shape[0]
        mean, var = z.mean(dim=0), z.var(dim=0, unbiased=False)
        cur = torch.relu((z - mean) / torch.sqrt(var + bn.eps) * gamma + beta)
        params += [w, bias, gamma, beta]
        m = bn.momentum
        running += [(1 - m) * bn.running_mean.double() + m * mean.detach(),
                    (1 - m) * bn.running_var.double() + m * var.detach() * cnt / max(cnt - 1, 1)]
    grads = torch.autograd.grad(cur, [h] + params, gout.reshape(-1, gout.shape[2])[valid].double())
    return {"out": cur.detach(), "grad_x": grads[0], "param_grads": list(grads[1:]), "running": running, "valid": valid}


@pytest.fixture(scope="module")
def results(cuda):
    """(case name, fill) -> the node's results, (case name, "ref") -> the float64 reference; each computed once, on first use"""
    cache = {}

    def get(name, what):
        if (name, what) not in cache:
            cache[(name, what)] = _reference(CASES[name], cuda) if what == "ref" else _run(CASES[name], cuda, what)
        return cache[(name, what)]
    return get


def _flat(res):
    return [res["out"], res["grad_x"]] + list(res["param_grads"]) + list(res["running"])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64(cuda, results, name):
    """out and grad_x on the valid rows, every parameter gradient, running_mean and running_var after one call: within 1e-5 of
    each tensor's scale of the float64 evaluation on the compacted rows"""
    got, want = results(name, "random"), results(name, "ref")
    valid = want["valid"]

    def close(g, w, what):
        g, w = g.detach().double().reshape(w.shape).cpu().numpy(), w.detach().cpu().numpy()
        err, bound = float(np.abs(g - w).max()), 1e-5 * max(1.0, float(np.abs(w).max()))
        print("case %s %s: max error %.3e (bound %.3e)" % (name, what, err, bound))
        assert err <= bound, what

    close(got["out"].reshape(valid.shape[0], -1)[valid], want["out"], "out")
    close(got["grad_x"].reshape(valid.shape[0], -1)[valid], want["grad_x"], "grad_x")
    kinds = ("grad_weight", "grad_bias", "grad_gamma", "grad_beta")
    for i, (g, w) in enumerate(zip(got["param_grads"], want["param_grads"])):
        close(g, w, "layer %d %s" % (i // 4 + 1, kinds[i % 4]))
    for i, (g, w) in enumerate(zip(got["running"], want["running"])):
        close(g, w, "layer %d %s" % (i // 2 + 1, ("running_mean", "running_var")[i % 2]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_padding_rows_are_exact_zeros(cuda, results, name):
    pad = ~_valid(CASES[name], cuda)
    assert int(pad.sum()) > 0
    for fill in ("zero", "random", "nan"):
        res = results(name, fill)
        for what in ("out", "grad_x"):
            bits = res[what][pad].contiguous().view(torch.int32)
            assert int((bits != 0).sum()) == 0, (fill, what)                 # all-zero bits: +0.0, not -0.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_padding_invariance_bit_for_bit(cuda, results, name):
    """the padding rows of x AND of grad_out as zeros, finite random values and NaN: every result the same bits, and finite"""
    base = _flat(results(name, "zero"))
    assert all(bool(torch.isfinite(t).all()) for t in base)
    assert float(base[0].abs().sum()) > 0 and float(base[1].abs().sum()) > 0
    for fill in ("random", "nan"):
        other = _flat(results(name, fill))
        assert len(other) == len(base)
        for i, (u, v) in enumerate(zip(base, other)):
            assert _same_bits(u, v), (fill, i)


@pytest.mark.parametrize("name", sorted(CASES))
def test_full_lengths_equal_the_dense_node(cuda, name):
    """lengths = (n, ..., n): every result is the dense node's, bit for bit"""
    case = CASES[name]
    net = _net(case, cuda)
    ragged = _flat(_run(case, cuda, "none", lengths=(case["n"],) * case["b"], net=net))
    dense = _flat(_run(case, cuda, "none", lengths=None, net=net))
    for i, (u, v) in enumerate(zip(ragged, dense)):
        assert _same_bits(u, v), i


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_to_run(cuda, results, name):
    again = _flat(_run(CASES[name], cuda, "nan"))
    for i, (u, v) in enumerate(zip(_flat(results(name, "nan")), again)):
        assert _same_bits(u, v), i


def test_no_host_read_of_lengths(cuda):
    """Case A: forward + backward captured once in a graph (one warm eager call first); lengths overwritten IN PLACE and the
    graph replayed: the results are an eager call's at the new lengths, bit for bit. No side stream: the graph is a chain."""
    from pointnet2_amd import train_mlp
    case = CASES["A"]
    new = (512, 1024, 33, 900)
    net = _net(case, cuda)
    params = list(net.parameters())
    x, gout = _inputs(case, cuda, "none")                                     # finite everywhere: valid rows under both lengths
    x.requires_grad_(True)
    lens = torch.tensor(case["lengths"], dtype=torch.int32, device=cuda)

    def step():
        out = train_mlp.fp_mlp_train(net, x, lengths=lens)
        return [out] + list(torch.autograd.grad(out, [x] + params, gout))

    step()                                                                    # warm
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    lens.copy_(torch.tensor(new, dtype=torch.int32, device=cuda))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in captured]
    want = step()
    old = _flat(_run(case, cuda, "none", net=net))[:2]
    assert not _same_bits(got[0], old[0])                                     # the replay did see the new lengths
    for i, (u, v) in enumerate(zip(got, want)):
        assert _same_bits(u, v), i
    pad = ~_valid(case, cuda, new)
    assert int((got[0][pad].contiguous().view(torch.int32) != 0).sum()) == 0
