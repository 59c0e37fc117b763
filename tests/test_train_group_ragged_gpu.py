"""The fused training node on the GROUPED rows of a ragged batch (train_mlp.sa_mlp_train(..., counts=),
pn2_mlp_train_*_group_ragged, csrc/train_mlp_ragged_group.hip): an SA level with per-cloud centroid counts and a group_all level
with per-cloud point counts -- batch statistics, running averages and every gradient over the valid rows only.

Cases: tests/train_group_ragged_cases.py (shared with the plan test, which proves which masked kernels they run).

Inputs. idx of a valid group names rows below its cloud's `lengths` (random, the second half of a group repeating its first
entry like the ball query's padding), idx of a padding group is 0 (what the two-sided ragged operators write). The padding --
rows of xyz and points beyond `lengths` (idx cases) or beyond `counts` (group_all), and the grad_out rows of padding groups -- is
zeros / finite random values / NaN.

The float64 reference follows tests/test_train_pool_gpu.py::_ref on the COMPACTED valid rows: the float64 stack evaluated with
the node's own ReLU decisions (from the saved z_l and (a, c)) and its own argsel; that the selected sample attains the group's
maximum over the valid rows is checked on its own (pool_gap). Tolerance: 1e-5 of each tensor's scale, the project's for every
masked and pooled node. All bitwise comparisons run in reproducible mode (set_deterministic(True)): the scatter of the per-row
feature gradient onto the points sums in a fixed order only there."""
import contextlib
import copy

import pytest
import torch

from train_group_ragged_cases import CAPTURE, CASES, NEW_COUNTS

pytestmark = pytest.mark.gpu

TOL = 1e-5
SEED = dict(net=211, inputs=212, fill=213)
FILLS = ("zero", "random", "nan")


@contextlib.contextmanager
def _deterministic(flag=True):
    from pointnet2_amd._tensors import set_deterministic
    set_deterministic(flag)
    try:
        yield
    finally:
        set_deterministic(False)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-30, float(b.abs().max())))


def _same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def _zero_bits(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _net(case, dev):
    """the case's stack with every parameter and running statistic away from its initial value"""
    from pointnet2_amd.pointnet_util import _SharedMLP
    torch.manual_seed(SEED["net"])
    net = _SharedMLP(3 + case["cfeat"], case["widths"]).net
    with torch.no_grad():
        for mod in net:
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(-0.4, 1.1)                 # both signs: the pool takes the min where gamma < 0
                mod.bias.uniform_(-0.5, 0.5)
                mod.running_mean.uniform_(-1.0, 1.0)
                mod.running_var.uniform_(0.5, 2.0)
    return net.to(dev).train()


def _valid_rows(case, dev, counts=None):
    """(b, m, ns) bool: the valid rows under counts (default: the case's)"""
    b, m, ns = case["b"], case["m"], case["ns"]
    cnt = torch.tensor(counts or case["counts"], device=dev)
    if case.get("group_all"):
        return (torch.arange(ns, device=dev).view(1, 1, ns) < cnt.clamp(1, ns).view(b, 1, 1)).expand(b, m, ns)
    return (torch.arange(m, device=dev).view(1, m, 1) < cnt.clamp(1, m).view(b, 1, 1)).expand(b, m, ns)


def _inputs(case, dev, fill, counts=None):
    """-> xyz, new_xyz, points, idx, grad_out on the GPU. fill "none": every row finite (the dense comparison)."""
    g = torch.Generator(device="cpu").manual_seed(SEED["inputs"])
    b, n, m, ns, cfeat = case["b"], case["n"], case["m"], case["ns"], case["cfeat"]
    group_all = case.get("group_all", False)
    xyz = torch.rand(b, n, 3, generator=g)
    points = torch.randn(b, n, cfeat, generator=g) if cfeat else None
    gout = torch.randn(b, m, case["widths"][-1], generator=g)
    new_xyz = idx = None
    valid = _valid_rows(case, "cpu", counts)
    if group_all:
        pad_pts = ~valid[:, 0, :]                                            # (b, n): points beyond counts
        pad_groups = torch.zeros(b, m, dtype=torch.bool)
    else:
        lens = torch.tensor(case["lengths"])
        sel = (torch.rand(b, m, generator=g) * lens.view(b, 1)).long().clamp(max=n - 1)
        new_xyz = torch.gather(xyz, 1, sel.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        idx = (torch.rand(b, m, ns, generator=g) * lens.view(b, 1, 1)).long().clamp(max=n - 1)
        idx[:, :, ns // 2:] = idx[:, :, :1]
        pad_groups = ~valid[:, :, 0]                                         # (b, m)
        if fill != "none":
            idx[pad_groups] = 0                                              # the ragged pair operators' fill
        idx = idx.int()
        pad_pts = torch.arange(n).view(1, n) >= lens.view(b, 1)
    if fill != "none":
        gf = torch.Generator(device="cpu").manual_seed(SEED["fill"])
        for t, pad in ((xyz, pad_pts), (points, pad_pts), (gout, pad_groups)):
            if t is None or not bool(pad.any()):
                continue
            if fill == "zero":
                t[pad] = 0.0
            elif fill == "nan":
                t[pad] = float("nan")
            else:
                t[pad] = 3.0 * torch.randn(t[pad].shape, generator=gf)
    return [t.to(dev) if t is not None else None for t in (xyz, new_xyz, points, idx, gout)]


def _saved(out, nl, has_x):
    """(z_l, save_l) of the fused node behind `out` (saved: x?, weights, biases, gammas, betas, z_l, save_l, out, ...)"""
    node = out.grad_fn
    while node is not None and type(node).__name__ != "_TrainMLPBackward":
        node = node.next_functions[0][0]
    sv = list(node.saved_tensors)
    off = (1 if has_x else 0) + 4 * nl
    return sv[off:off + nl], sv[off + nl:off + 2 * nl]


def _call(net, case, tensors, counts):
    """one forward + backward of the node -> dict of results (detached), with the saved z_l and (mean, invstd, a, c)"""
    from pointnet2_amd import train_mlp
    xyz, new_xyz, points, idx, gout = tensors
    pts = points.clone().requires_grad_(True) if points is not None else None
    kw = {} if counts is None else {"counts": counts}
    with train_mlp.options(**case.get("opts", {})):
        out, argsel = train_mlp.sa_mlp_train(net, xyz, new_xyz, pts, idx, case.get("xyz_first", True), **kw)
        pairs = train_mlp.conv_bn_pairs(net)
        zs, saves = _saved(out, len(pairs), pts is not None)                 # (before the backward frees them)
        params = [p for p in net.parameters()]
        grads = torch.autograd.grad(out, ([pts] if pts is not None else []) + params, gout, allow_unused=True)
    res = dict(out=out.detach(), argsel=argsel, gpts=grads[0] if pts is not None else None,
               gparams=list(grads[1 if pts is not None else 0:]), zs=[z.detach() for z in zs], saves=[s.detach() for s in saves],
               rm=[bn.running_mean.detach().clone() for _, bn in pairs], rv=[bn.running_var.detach().clone() for _, bn in pairs])
    return res


def _flat(res):
    """every result tensor of _call that must be the same bits from run to run"""
    ts = [res["out"], res["argsel"]] + ([res["gpts"]] if res["gpts"] is not None else [])
    return ts + [g for g in res["gparams"] if g is not None] + res["zs"] + res["rm"] + res["rv"]


_RESULTS = {}


def _results(name, cuda):
    """the case under the three fills, in reproducible mode, each from the same initial stack: computed once, never changed"""
    if name not in _RESULTS:
        case = CASES[name]
        base = _net(case, cuda)
        counts = torch.tensor(case["counts"], dtype=torch.int32, device=cuda)
        runs = {}
        with _deterministic():
            for fill in FILLS:
                net = copy.deepcopy(base)
                runs[fill] = (_call(net, case, _inputs(case, cuda, fill), counts), net)
        torch.cuda.synchronize()
        _RESULTS[name] = (base, runs)
    return _RESULTS[name]


def _reference(case, base, net_after, tensors, res, counts=None):
    """float64 on the compacted valid rows with the node's ReLU decisions and argsel -> dict of relative errors"""
    from pointnet2_amd import train_mlp
    xyz, new_xyz, points, idx, gout = tensors
    b, n, m, ns, cfeat = case["b"], case["n"], case["m"], case["ns"], case["cfeat"]
    valid = _valid_rows(case, "cpu", counts).reshape(-1)
    rows_v = valid.nonzero().squeeze(1)
    nv = int(rows_v.numel())
    x64 = xyz.double().cpu()
    p64 = points.double().cpu().requires_grad_(True) if cfeat else None
    if case.get("group_all"):
        gx, gp = x64.unsqueeze(1), (p64.unsqueeze(1) if cfeat else None)
    else:
        li, bi = idx.long().cpu(), torch.arange(b).view(b, 1, 1)
        gx = x64[bi, li] - new_xyz.double().cpu().unsqueeze(2)
        gp = p64[bi, li] if cfeat else None
    parts = [gx, gp] if case.get("xyz_first", True) else [gp, gx]
    rows64 = torch.cat([t for t in parts if t is not None], dim=-1).reshape(b * m * ns, 3 + cfeat)
    h = rows64.index_select(0, rows_v)                                       # the compacted rows: padding never enters
    pairs0, pairs1 = train_mlp.conv_bn_pairs(base), train_mlp.conv_bn_pairs(net_after)
    params64 = [tuple(t.detach().double().cpu().requires_grad_(True) for t in
                      (conv.weight.view(conv.out_channels, -1), conv.bias, bn.weight, bn.bias)) for conv, bn in pairs0]
    masks = [((z * s[2]) + s[3] > 0).cpu() for z, s in zip(res["zs"], res["saves"])]      # two roundings, as the kernels' fmul + fadd
    errs, flips, margin = {}, 0, 0.0
    for l, ((W, bias, gamma, beta), (conv, bn)) in enumerate(zip(params64, pairs0)):
        z = h @ W.t() + bias
        mean, var = z.mean(0), z.var(0, unbiased=False)
        y = (z - mean) / torch.sqrt(var + bn.eps) * gamma + beta
        mk = masks[l].index_select(0, rows_v)
        dis = (y.detach() > 0) != mk
        flips += int(dis.sum())
        if dis.any():
            margin = max(margin, float(y.detach()[dis].abs().max() / y.detach().abs().max()))
        h = y * mk.to(y.dtype)
        bn1 = pairs1[l][1]
        errs["rm%d" % (l + 1)] = _rel(bn1.running_mean, (1 - bn.momentum) * bn.running_mean.double().cpu() + bn.momentum * mean.detach())
        errs["rv%d" % (l + 1)] = _rel(bn1.running_var, (1 - bn.momentum) * bn.running_var.double().cpu() +
                                      bn.momentum * var.detach() * nv / max(nv - 1, 1))
    c = h.shape[1]
    hf = torch.zeros(b * m * ns, c, dtype=torch.float64).index_copy(0, rows_v, h).view(b * m, ns, c)
    sel = res["argsel"].reshape(b * m, c).long().cpu()
    want = hf.gather(1, sel.unsqueeze(1)).squeeze(1)                         # padding groups: row 0 of zeros
    top = torch.where(valid.view(b * m, ns, 1), hf.detach(), torch.full_like(hf, -1e300)).max(dim=1)[0]
    vg = valid.view(b * m, ns)[:, 0]
    errs["pool_gap"] = float((top[vg] - want.detach()[vg]).abs().max() / max(1e-30, float(top[vg].abs().max())))
    gw = torch.where(vg.view(-1, 1), gout.double().cpu().reshape(b * m, c), torch.zeros(1, dtype=torch.float64))
    (want * gw).sum().backward()
    errs["out"] = _rel(res["out"].reshape(b * m, c), want)
    if cfeat:
        errs["dpts"] = _rel(res["gpts"], p64.grad)
    gp_it = iter(res["gparams"])
    for l, p in enumerate(params64):
        gW, gbias, gg, gb = next(gp_it), next(gp_it), next(gp_it), next(gp_it)
        errs["dW%d" % (l + 1)] = _rel(gW.reshape(p[0].shape), p[0].grad)
        errs["dg%d" % (l + 1)] = _rel(gg, p[2].grad)
        errs["dbe%d" % (l + 1)] = _rel(gb, p[3].grad)
        assert float(gbias.abs().max()) == 0.0                               # batch norm removes the conv bias
    nmask = sum(int(mk.index_select(0, rows_v).numel()) for mk in masks)
    assert flips <= max(2, 1e-5 * nmask) and margin <= 1e-5, (flips, margin)
    return errs


@pytest.mark.parametrize("name", list(CASES))
def test_matches_float64_on_the_valid_rows(cuda, name):
    case = CASES[name]
    base, runs = _results(name, cuda)
    res, net = runs["nan"]
    errs = _reference(case, base, net, _inputs(case, cuda, "zero"), res)
    print(name, " ".join("%s=%.1e" % kv for kv in errs.items()), flush=True)
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("name", list(CASES))
def test_padding_is_exact_zero_bits(cuda, name):
    case = CASES[name]
    res, _ = _results(name, cuda)[1]["nan"]
    b, m, ns = case["b"], case["m"], case["ns"]
    valid = _valid_rows(case, cuda)
    pad_rows = ~valid.reshape(-1)
    for z in res["zs"]:
        assert _zero_bits(z[pad_rows])
    pad_groups = ~valid[:, :, 0]
    assert _zero_bits(res["out"][pad_groups]) and _zero_bits(res["argsel"][pad_groups])
    cnt = torch.tensor(case["counts"], device=cuda)
    limit = cnt.clamp(1, ns).view(b, 1, 1) if case.get("group_all") else torch.full((b, 1, 1), ns, device=cuda)
    sel_ok = (res["argsel"] >= 0) & (res["argsel"] < limit)
    assert bool(sel_ok[~pad_groups].all())
    if res["gpts"] is not None:
        lens = cnt.clamp(1, case["n"]) if case.get("group_all") else torch.tensor(case["lengths"], device=cuda)
        beyond = torch.arange(case["n"], device=cuda).view(1, -1) >= lens.view(b, 1)
        assert _zero_bits(res["gpts"][beyond])
        assert bool(torch.isfinite(res["gpts"]).all())


@pytest.mark.parametrize("name", list(CASES))
def test_results_do_not_depend_on_the_padding(cuda, name):
    runs = _results(name, cuda)[1]
    want = _flat(runs["zero"][0])
    for fill in ("random", "nan"):
        got = _flat(runs[fill][0])
        assert len(got) == len(want)
        for i, (u, v) in enumerate(zip(got, want)):
            assert _same_bits(u, v), (fill, i)
            assert bool(torch.isfinite(u.float()).all()), (fill, i)


@pytest.mark.parametrize("name", list(CASES))
def test_run_to_run_bits(cuda, name):
    case = CASES[name]
    base, runs = _results(name, cuda)
    counts = torch.tensor(case["counts"], dtype=torch.int32, device=cuda)
    with _deterministic():
        again = _call(copy.deepcopy(base), case, _inputs(case, cuda, "nan"), counts)
    for i, (u, v) in enumerate(zip(_flat(again), _flat(runs["nan"][0]))):
        assert _same_bits(u, v), i


@pytest.mark.parametrize("name", list(CASES))
def test_full_counts_agree_with_the_dense_node(cuda, name):
    """1e-5 of scale, not bits: the dense node pools in the GEMM's epilogue and sums the top gradient per group"""
    case = CASES[name]
    full = dict(case, counts=tuple([case["ns"] if case.get("group_all") else case["m"]] * case["b"]))
    base = _net(case, cuda)
    tensors = _inputs(full, cuda, "none")
    counts = torch.tensor(full["counts"], dtype=torch.int32, device=cuda)
    with _deterministic():
        net_r, net_d = copy.deepcopy(base), copy.deepcopy(base)
        rag = _call(net_r, full, tensors, counts)
        dense = _call(net_d, full, tensors, None)
    errs = {"out": _rel(rag["out"], dense["out"])}
    if rag["gpts"] is not None:
        errs["dpts"] = _rel(rag["gpts"], dense["gpts"])
    for i, (u, v) in enumerate(zip(rag["gparams"], dense["gparams"])):
        if i % 4 != 1:                                                       # (the conv bias gradient is exactly zero in both)
            errs["dparam%d" % i] = _rel(u, v)
    for l, (u, v) in enumerate(zip(rag["rm"] + rag["rv"], dense["rm"] + dense["rv"])):
        errs["stat%d" % l] = _rel(u, v)
    print(name, " ".join("%s=%.1e" % kv for kv in errs.items()), flush=True)
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("name", CAPTURE)
def test_capture_and_replay_sees_new_counts(cuda, name):
    case = CASES[name]
    new = NEW_COUNTS[name]
    base = _net(case, cuda)
    from pointnet2_amd import train_mlp
    pairs = train_mlp.conv_bn_pairs(base)
    stats0 = [(bn.running_mean.clone(), bn.running_var.clone()) for _, bn in pairs]
    # every row finite and every idx in range (fill "none"): both sets of counts run on the same tensors
    tensors = _inputs(case, cuda, "none")
    cnt = torch.tensor(case["counts"], dtype=torch.int32, device=cuda)

    def reset():
        with torch.no_grad():
            for (_, bn), (rm, rv) in zip(pairs, stats0):
                bn.running_mean.copy_(rm)
                bn.running_var.copy_(rv)

    def step():
        res = _call(base, case, tensors, cnt)
        return _flat(res)

    with _deterministic():
        side = torch.cuda.Stream()                                           # warm on a side stream, as a capture wants it
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            old = [t.detach().clone() for t in step()]
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step()
        reset()
        cnt.copy_(torch.tensor(new, dtype=torch.int32, device=cuda))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach().clone() for t in captured]
        del captured
        reset()
        want = step()
        torch.cuda.synchronize()
    assert not _same_bits(got[0], old[0])                                    # the replay did see the new counts
    for i, (u, v) in enumerate(zip(got, want)):
        assert _same_bits(u, v), i
