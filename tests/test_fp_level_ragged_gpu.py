"""The FP training node with a RAGGED unknown side (train_mlp.fp_level_train(..., lengths=), pn2_mlp_train_*_fp_ragged,
csrc/train_mlp_fp.hip) on the GPU: layer 1 once per known point with a row mask inside -- batch statistics, running
averages and every gradient over the valid rows only, the (b, n, c2 + c1) tensor never written.

Case A: b 4, n 1024, m 256, lengths (1024, 700, 300, 64), c2 35, c1 6, stack 64 -> 32: both zero-pad copies (35 -> 36, 6 -> 8);
        32-row tiles fully valid, fully padding or mixed at non-multiples of 32; the points1 W1b product is added to.
Case B: b 4, n 200, m 25, lengths (200, 137, 1, 32), c2 32, c1 0, stack 32 -> 32 -> 64: n % 32 != 0 (a validity word spans two
        clouds); b m = 100 known points enter padded to 128 rows; no skip features; a one-row cloud; three layers.
Case C: b 2, n 96, m 16, lengths (96, 50), c2 16, c1 16, stack 32: layer 1 is the top layer (the masked apply right behind it).

Geometry: xyz1 random with NaN on its padding rows, xyz2 random, three_nn(xyz1, xyz2, lengths1=). The padding rows of points1,
grad_out AND dist are zeros / finite random values / NaN; idx is left as three_nn wrote it there.

The float64 reference is utils/pointnet_util.py:211-226 in torch float64 on the COMPACTED valid rows. A ReLU whose argument is
within fp32 rounding of zero is decided by rounding, so the reference's gradients take the kernels' own decisions (from the saved
z_l and (a, c), as tests/test_fp_level_train_gpu.py::_masked64), under that file's cap: at most 1e-5 N_valid sum(widths) decisions
differ (2 at case A, NONE at B and C), each with |y| <= 1e-5 of its layer's scale. The cap is a condition. The seeds (SEED:
101 / 102 / 103 for the stack / the inputs / the padding fill) were chosen so that a torch fp32 evaluation of the same formulas on
the CPU (_reference(..., dtype=torch.float32) against float64, geometry by torch.cdist) stays within it: 0 differing decisions at
each of the three cases.

Bits. The interpolation gradient S (pn2_three_interpolate_grad_seg / _planned) sums its segments in an order that varies from run
to run unless its reproducible mode is on (set_deterministic(True); include/pn2ops.h says so of the dense node too): grad_points2
and layer 1's grad_weight come from S. The module-scoped results are therefore computed under set_deterministic(True), where
EVERY result is comparable bit for bit; test_run_to_run also runs the default mode, compares there what does not come from S bit
for bit, and holds what does to the float64 bound."""
import contextlib
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5                                                       # tests/test_fp_level_train_gpu.py's, README
SEED = dict(net=101, inputs=102, fill=103)
CASES = {
    "A": dict(b=4, n=1024, m=256, lengths=(1024, 700, 300, 64), c2=35, c1=6, mlp=[64, 32]),
    "B": dict(b=4, n=200, m=25, lengths=(200, 137, 1, 32), c2=32, c1=0, mlp=[32, 32, 64]),
    "C": dict(b=2, n=96, m=16, lengths=(96, 50), c2=16, c1=16, mlp=[32]),
}
FILLS = ("zero", "random", "nan")


@contextlib.contextmanager
def _deterministic(flag=True):
    from pointnet2_amd._tensors import set_deterministic
    set_deterministic(flag)
    try:
        yield
    finally:
        set_deterministic(False)


def _net(case, dev):
    """the case's stack with every parameter and running statistic away from its initial value"""
    from pointnet2_amd.pointnet_util import _SharedMLP
    torch.manual_seed(SEED["net"])
    net = _SharedMLP(case["c2"] + case["c1"], case["mlp"]).net
    with torch.no_grad():
        for mod in net:
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(-1.5, 1.5)                 # both signs
                mod.bias.uniform_(-0.5, 0.5)
                mod.running_mean.uniform_(-1.0, 1.0)
                mod.running_var.uniform_(0.5, 2.0)
    return net.to(dev).train()


def _valid(case, dev, lengths=None):
    lens = torch.tensor(lengths or case["lengths"], device=dev).clamp(1, case["n"])
    return torch.arange(case["n"], device=dev).unsqueeze(0) < lens.unsqueeze(1)          # (b, n)


def _raw(case):
    """the case's tensors on the CPU, the same for every fill: xyz1, xyz2, points2, points1 (or None), grad_out"""
    g = torch.Generator(device="cpu").manual_seed(SEED["inputs"])
    b, n, m = case["b"], case["n"], case["m"]
    xyz1, xyz2 = torch.rand(b, n, 3, generator=g), torch.rand(b, m, 3, generator=g)
    p2 = torch.randn(b, m, case["c2"], generator=g)
    p1 = torch.randn(b, n, case["c1"], generator=g) if case["c1"] else None
    gout = torch.randn(b, n, case["mlp"][-1], generator=g)
    return xyz1, xyz2, p2, p1, gout


def _inputs(case, cuda, fill, lengths=None):
    """-> points2, points1, idx, dist, grad_out on the GPU. fill "none": every row finite, the geometry of the dense three_nn (rows
    that are valid under any lengths); else NaN on xyz1's padding rows, the ragged three_nn, and the fill on the padding rows of
    points1, grad_out and dist."""
    from pointnet2_amd.tf_interpolate import three_nn
    xyz1, xyz2, p2, p1, gout = [t.to(cuda) if t is not None else None for t in _raw(case)]
    if fill == "none":
        dist, idx = three_nn(xyz1, xyz2)
        return p2, p1, idx, dist, gout
    pad = ~_valid(case, cuda, lengths)
    xyz1[pad] = float("nan")
    lens = torch.tensor(lengths or case["lengths"], dtype=torch.int32, device=cuda)
    dist, idx = three_nn(xyz1, xyz2, lengths1=lens)
    dist = dist.clone()
    for k, t in enumerate((p1, gout, dist)):
        if t is None:
            continue
        if fill == "zero":
            t[pad] = 0.0
        elif fill == "nan":
            t[pad] = float("nan")
        elif fill == "random":
            t[pad] = 3.0 * torch.randn(t[pad].shape, generator=torch.Generator(device="cpu").manual_seed(SEED["fill"] + k)).to(cuda)
    assert int(idx.min()) >= 0 and int(idx.max()) < case["m"]              # the contract for idx on padding rows
    return p2, p1, idx, dist, gout


def _call(net, tensors, lengths, plan=None):
    """one forward + backward of the node -> the results and, for the reference, the saved z_l and (mean, invstd, a, c)"""
    from pointnet2_amd import train_mlp
    p2, p1, idx, dist, gout = tensors
    p2 = p2.clone().requires_grad_(True)
    p1 = p1.clone().requires_grad_(True) if p1 is not None else None
    kw = {} if lengths is None else {"lengths": lengths}
    bns = [mod for mod in net if isinstance(mod, torch.nn.BatchNorm2d)]
    before = [int(mod.num_batches_tracked) for mod in bns]
    out, weight = train_mlp.fp_level_train(net, p2, p1, idx, dist, return_weight=True, plan=plan, **kw)
    params = list(net.parameters())
    inputs = [p2] + ([p1] if p1 is not None else [])
    grads = torch.autograd.grad(out, inputs + params, gout, retain_graph=True)
    assert [int(mod.num_batches_tracked) for mod in bns] == [c + 1 for c in before]        # one batch counted
    node = out.grad_fn.next_functions[0][0]
    nl, tail = len(bns), (2 if lengths is not None else 0)                  # saved behind `out`: the mask and the lengths
    saved = node.saved_tensors
    saved = saved[:len(saved) - tail]
    res = {"out": out.detach(), "weight": weight.detach(), "grad_p2": grads[0], "grad_p1": grads[1] if p1 is not None else None,
           "param_grads": list(grads[len(inputs):]),
           "running": [t.detach().clone() for mod in bns for t in (mod.running_mean, mod.running_var)],
           "zs": [t.detach() for t in saved[-(2 * nl + 1):-(nl + 1)]], "saves": [t.detach() for t in saved[-(nl + 1):-1]]}
    return res


def _run(case, cuda, fill, lengths="case", net=None, deterministic=True, plan=False):
    from pointnet2_amd.index_plan import index_plan
    net = copy.deepcopy(net if net is not None else _net(case, cuda))
    lens = case["lengths"] if lengths == "case" else lengths
    tensors = _inputs(case, cuda, fill, lens)
    dev_lens = torch.tensor(lens, dtype=torch.int32, device=cuda) if lens is not None else None
    with _deterministic(deterministic):
        return _call(net, tensors, dev_lens, index_plan(tensors[2], case["m"], "interpolate") if plan else None)


def _reference(net, p2, p1, idx, dist, gout, valid, zs=None, saves=None, dtype=torch.float64):
    """utils/pointnet_util.py:211-226 on the compacted valid rows, in `dtype` on the CPU: weights from clamp(dist, 1e-10),
    interpolation, concat, conv + batch-statistics batch norm + ReLU (the biased variance normalises, the unbiased one enters the
    running average with N_valid / max(N_valid - 1, 1)), grad_points2 by autograd through the gather. With zs / saves the ReLU
    decisions of the GRADIENTS are the kernels' (relu(a z + c) > 0 from the saved tensors); -> results, the number of decisions
    that differ from this evaluation's own, and their largest |y| relative to the layer's scale."""
    valid = valid.reshape(-1).cpu()
    b, m, _ = p2.shape
    n = idx.shape[1]
    cloud = (torch.arange(b * n) // n)[valid]
    ii = idx.reshape(-1, 3).cpu().long()[valid]
    d = dist.reshape(-1, 3).cpu().to(dtype)[valid]
    inv = 1.0 / torch.clamp(d, min=1e-10)
    w = inv / inv.sum(dim=1, keepdim=True)
    a2 = p2.detach().cpu().to(dtype).requires_grad_(True)
    a1 = p1.detach().cpu().to(dtype).reshape(b * n, -1)[valid].requires_grad_(True) if p1 is not None else None
    x = (a2[cloud[:, None], ii] * w[..., None]).sum(dim=1)                  # (N_valid, c2)
    h = torch.cat([x, a1], dim=1) if a1 is not None else x
    cnt = h.shape[0]
    params, running, signs, flips, margin, own = [], [], [], 0, 0.0, None
    mods = list(net)
    for l in range(len(mods) // 3):
        conv, bn = mods[3 * l], mods[3 * l + 1]
        W = conv.weight.detach().cpu().to(dtype).reshape(conv.out_channels, -1).requires_grad_(True)
        bias = conv.bias.detach().cpu().to(dtype).requires_grad_(True)
        gam, bet = bn.weight.detach().cpu().to(dtype).requires_grad_(True), bn.bias.detach().cpu().to(dtype).requires_grad_(True)
        params += [W, bias, gam, bet]
        z = h @ W.t() + bias
        mean, var = z.mean(dim=0), z.var(dim=0, unbiased=False)
        y = (z - mean) / torch.sqrt(var + bn.eps) * gam + bet
        mom = bn.momentum
        running += [(1 - mom) * bn.running_mean.cpu().to(dtype) + mom * mean.detach(),
                    (1 - mom) * bn.running_var.cpu().to(dtype) + mom * var.detach() * cnt / max(cnt - 1, 1)]
        own = torch.relu(y).detach()                                        # (the last layer's: `out`)
        mask = y.detach() > 0
        signs.append(mask)
        if zs is not None:
            mask = ((saves[l][2] * zs[l] + saves[l][3]).cpu()[valid] > 0)
            dis = (y.detach() > 0) != mask
            flips += int(dis.sum())
            if dis.any():
                margin = max(margin, float(y.detach()[dis].abs().max() / y.detach().abs().max()))
        h = y * mask.to(dtype)
    grads = torch.autograd.grad(h, [a2] + ([a1] if a1 is not None else []) + params, gout.reshape(b * n, -1).cpu().to(dtype)[valid])
    k = 2 if a1 is not None else 1
    return {"out": own, "grad_p2": grads[0], "grad_p1": grads[1] if a1 is not None else None, "param_grads": list(grads[k:]),
            "running": running, "valid": valid, "signs": signs}, flips, margin


@pytest.fixture(scope="module")
def results(cuda):
    """(case name, fill) -> the node's results under set_deterministic(True); each computed once, on first use, never changed"""
    cache = {}

    def get(name, fill):
        if (name, fill) not in cache:
            cache[(name, fill)] = _run(CASES[name], cuda, fill)
        return cache[(name, fill)]
    return get


def _flat(res):
    return [res["out"], res["weight"], res["grad_p2"]] + ([res["grad_p1"]] if res["grad_p1"] is not None else []) + \
        list(res["param_grads"]) + list(res["running"])


def _from_s(res):
    """positions in _flat of what comes from the interpolation gradient S: grad_points2 and layer 1's grad_weight"""
    return (2, 3 + (1 if res["grad_p1"] is not None else 0))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_float64(name, cuda, got, what="", only=None):
    """got against the float64 reference on the kernels' own linear piece: 1e-5 of each tensor's scale"""
    case = CASES[name]
    p2, p1, idx, dist, gout = _inputs(case, cuda, "zero")
    valid = _valid(case, cuda)
    want, flips, margin = _reference(_net(case, cuda), p2, p1, idx, dist, gout, valid, got["zs"], got["saves"])
    nv = int(valid.sum())
    print("case %s%s: %d valid rows, %d ReLU decisions differ from float64's (cap %.2f), margin %.2e" %
          (name, what, nv, flips, 1e-5 * nv * sum(case["mlp"]), margin))
    assert flips <= 1e-5 * nv * sum(case["mlp"]) and margin <= 1e-5, (flips, margin)
    v = want["valid"]
    errors = []

    def close(g, w, label):
        if only is not None and label not in only:
            return
        g, w = g.detach().double().cpu().reshape(w.shape).numpy(), w.detach().double().numpy()
        err, bound = float(np.abs(g - w).max()), TOL * max(1e-30, float(np.abs(w).max()))
        print("case %s%s %s: max error %.3e (bound %.3e)" % (name, what, label, err, bound))
        if err > bound:
            errors.append(label)

    close(got["out"].reshape(v.shape[0], -1).cpu()[v], want["out"], "out")
    close(got["grad_p2"], want["grad_p2"], "grad_points2")
    if case["c1"]:
        close(got["grad_p1"].reshape(v.shape[0], -1).cpu()[v], want["grad_p1"], "grad_points1")
    kinds = ("grad_weight", "grad_bias", "grad_gamma", "grad_beta")
    for i, (g, w) in enumerate(zip(got["param_grads"], want["param_grads"])):
        if i % 4 != 1:                                                       # (the conv bias: exactly zero under batch norm)
            close(g, w, "layer %d %s" % (i // 4 + 1, kinds[i % 4]))
        else:
            assert int((g != 0).sum()) == 0
    for i, (g, w) in enumerate(zip(got["running"], want["running"])):
        close(g, w, "layer %d %s" % (i // 2 + 1, ("running_mean", "running_var")[i % 2]))
    assert not errors, errors


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64(cuda, results, name):
    """out, grad_points2, grad_points1 (valid rows), every grad_weight / gamma / beta, running_mean and running_var after one
    call: within 1e-5 of each tensor's scale of the float64 evaluation on the compacted rows"""
    _check_float64(name, cuda, results(name, "random"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_padding_rows_are_exact_zeros(cuda, results, name):
    pad = ~_valid(CASES[name], cuda)
    assert int(pad.sum()) > 0
    for fill in FILLS:
        res = results(name, fill)
        for what in ("out", "grad_p1", "weight"):
            if res[what] is None:
                continue
            bits = res[what].reshape(pad.shape[0], pad.shape[1], -1)[pad].contiguous().view(torch.int32)
            assert int((bits != 0).sum()) == 0, (fill, what)                 # all-zero bits: +0.0, not -0.0
        for z in res["zs"]:
            assert int((z.reshape(pad.shape[0], pad.shape[1], -1)[pad].contiguous().view(torch.int32) != 0).sum()) == 0, fill


@pytest.mark.parametrize("name", sorted(CASES))
def test_padding_invariance_bit_for_bit(cuda, results, name):
    """the padding rows of points1, grad_out AND dist as zeros, finite random values and NaN: every result the same bits, finite"""
    base = _flat(results(name, "zero"))
    assert all(bool(torch.isfinite(t).all()) for t in base)
    assert all(float(t.abs().sum()) > 0 for t in base[:4])
    for fill in ("random", "nan"):
        other = _flat(results(name, fill))
        assert len(other) == len(base)
        for i, (u, v) in enumerate(zip(base, other)):
            assert _same_bits(u, v), (fill, i)


@pytest.mark.parametrize("name", sorted(CASES))
def test_full_lengths_equal_the_dense_node(cuda, name):
    """lengths = (n, ..., n): every result is fp_level_train(...) without lengths, bit for bit (the dense default folds no
    finalisation: fold_finalize is opt-in; both under set_deterministic(True), see the module's docstring)"""
    case = CASES[name]
    net = _net(case, cuda)
    ragged = _flat(_run(case, cuda, "none", lengths=(case["n"],) * case["b"], net=net))
    dense = _flat(_run(case, cuda, "none", lengths=None, net=net))
    assert len(ragged) == len(dense)
    for i, (u, v) in enumerate(zip(ragged, dense)):
        assert _same_bits(u, v), i


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_to_run(cuda, results, name):
    """the same bits twice: everything under set_deterministic(True); in the default mode everything that does not come from the
    interpolation gradient S -- and what does (grad_points2, layer 1's grad_weight) within the float64 bound"""
    first = results(name, "nan")
    for i, (u, v) in enumerate(zip(_flat(first), _flat(_run(CASES[name], cuda, "nan")))):
        assert _same_bits(u, v), i
    runs = [_run(CASES[name], cuda, "nan", deterministic=False) for _ in range(2)]
    skip = _from_s(first)
    for i, (u, v, w) in enumerate(zip(_flat(runs[0]), _flat(runs[1]), _flat(first))):
        if i not in skip:
            assert _same_bits(u, v) and _same_bits(u, w), i
    _check_float64(name, cuda, runs[1], " (default mode)", only=("grad_points2", "layer 1 grad_weight"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_index_plan(cuda, results, name):
    """plan=index_plan(idx, m, "interpolate"): the same `out` bits, the gradients within the float64 bound"""
    got = _run(CASES[name], cuda, "random", plan=True)
    assert _same_bits(got["out"], results(name, "random")["out"])
    _check_float64(name, cuda, got, " (index plan)")


def test_no_host_read_of_lengths(cuda):
    """Case A: forward + backward captured once in a graph (one warm eager call first); lengths overwritten IN PLACE and the
    graph replayed: the results are an eager call's at the new lengths, bit for bit, and not the old ones."""
    from pointnet2_amd import train_mlp
    case = CASES["A"]
    new = (512, 1024, 33, 900)
    net = _net(case, cuda)
    params = list(net.parameters())
    p2, p1, idx, dist, gout = _inputs(case, cuda, "none")                     # finite everywhere: valid rows under both lengths
    p2.requires_grad_(True)
    p1.requires_grad_(True)
    lens = torch.tensor(case["lengths"], dtype=torch.int32, device=cuda)

    def step():
        out, weight = train_mlp.fp_level_train(net, p2, p1, idx, dist, return_weight=True, lengths=lens)
        return [out, weight] + list(torch.autograd.grad(out, [p2, p1] + params, gout))

    with _deterministic():
        side = torch.cuda.Stream()                                            # warm on a side stream, as a capture wants it
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            # detached: a clone of `out` with its grad_fn would keep the warm call's autograd graph alive, and with it the leaves'
            # AccumulateGrad nodes on the warm call's stream -- the capture would then synchronise with that stream
            old = [t.detach().clone() for t in step()]
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = step()
        lens.copy_(torch.tensor(new, dtype=torch.int32, device=cuda))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach().clone() for t in captured]
        del captured                                                          # (and with it the capture's autograd graph)
        want = step()
    assert not _same_bits(got[0], old[0]) and not _same_bits(got[2], old[2])  # the replay did see the new lengths
    for i, (u, v) in enumerate(zip(got, want)):
        assert _same_bits(u, v), i
    pad = ~_valid(case, cuda, new)
    for t in (got[0], got[1], got[3]):
        assert int((t[pad].contiguous().view(torch.int32) != 0).sum()) == 0


def _module(case, cuda, node, patch_rule, monkeypatch):
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    if patch_rule:
        monkeypatch.setattr(train_mlp, "FP_NODE_MIN_SAVED", 0)
    mod = U.PointnetFPModule(case["c2"] + case["c1"], case["mlp"]).to(cuda).train()
    mod.mlp.net.load_state_dict(_net(case, cuda).state_dict())
    mod.fused_ragged_train = True
    mod.fused_ragged_node = node
    return mod


def test_module_takes_the_node_only_where_asked_and_preferred(cuda, monkeypatch):
    """PointnetFPModule on case A: fused_ragged_train + fused_ragged_node with the size rule patched to 0 -> the node, zero padding
    rows, the float64 bound; fused_ragged_node off -> "fused_train_ragged"; both on under the real size rule -> "fused_train_ragged"
    (the shape is below it)"""
    from pointnet2_amd.geometry import FPGeometry
    case = CASES["A"]
    xyz1, xyz2 = [t.to(cuda) for t in _raw(case)[:2]]
    pad = ~_valid(case, cuda)
    xyz1[pad] = float("nan")
    p2, p1, idx, dist, gout = _inputs(case, cuda, "nan")
    lens = torch.tensor(case["lengths"], dtype=torch.int32, device=cuda)
    for node, patch, path in ((True, True, "fused_train_ragged_node"), (False, True, "fused_train_ragged")):
        with monkeypatch.context() as mp:
            mod = _module(case, cuda, node, patch, mp)
            a2, a1 = p2.clone().requires_grad_(True), p1.clone().requires_grad_(True)
            # (the geometry handed in: dist with NaN on its padding rows; the fp_interp_concat route wants finite rows there)
            geo = FPGeometry(dist if node else torch.nan_to_num(dist), idx)
            out = mod(xyz1, xyz2, a1 if node else torch.nan_to_num(a1), a2, geometry=geo, lengths1=lens)
            assert mod.last_path == path
            assert int((out[pad].contiguous().view(torch.int32) != 0).sum()) == 0
            if not node:
                continue
            grads = torch.autograd.grad(out, [a2, a1] + list(mod.mlp.net.parameters()), gout, retain_graph=True)
            fn = out.grad_fn
            while type(fn).__name__ != "_TrainFPBackward":
                fn = fn.next_functions[0][0]
            saved = fn.saved_tensors[:-2]
            nl = len(case["mlp"])
            bns = [m_ for m_ in mod.mlp.net if isinstance(m_, torch.nn.BatchNorm2d)]
            got = {"out": out.detach(), "grad_p2": grads[0], "grad_p1": grads[1], "param_grads": list(grads[2:]),
                   "running": [t.detach().clone() for b_ in bns for t in (b_.running_mean, b_.running_var)],
                   "zs": [t.detach() for t in saved[-(2 * nl + 1):-(nl + 1)]], "saves": [t.detach() for t in saved[-(nl + 1):-1]]}
            assert int((grads[1][pad].contiguous().view(torch.int32) != 0).sum()) == 0
            _check_float64("A", cuda, got, " (module)")
    mod = _module(case, cuda, True, False, monkeypatch)                       # the real size rule
    mod(xyz1, xyz2, torch.nan_to_num(p1), p2, geometry=FPGeometry(torch.nan_to_num(dist), idx), lengths1=lens)
    assert mod.last_path == "fused_train_ragged"


def test_module_node_route_never_holds_the_concatenated_tensor(cuda, monkeypatch):
    """b 4, n 2048, m 64, c2 128, no skip features, stack [64] -- the (b, n, c2) tensor dominates: the peak memory of a forward
    + backward on the node route is below the "fused_train_ragged" route's by at least that tensor's bytes"""
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    from pointnet2_amd.geometry import FPGeometry
    from pointnet2_amd.tf_interpolate import three_nn
    monkeypatch.setattr(train_mlp, "FP_NODE_MIN_SAVED", 0)
    b, n, m, c2 = 4, 2048, 64, 128
    torch.manual_seed(SEED["inputs"])
    mod = U.PointnetFPModule(c2, [64]).to(cuda).train()
    mod.fused_ragged_train = True
    xyz1, xyz2 = torch.rand(b, n, 3, device=cuda), torch.rand(b, m, 3, device=cuda)
    p2 = torch.randn(b, m, c2, device=cuda, requires_grad=True)
    gout = torch.randn(b, n, 64, device=cuda)
    lens = torch.tensor((2048, 1500, 1024, 1999), dtype=torch.int32, device=cuda)
    geo = FPGeometry(*three_nn(xyz1, xyz2, lengths1=lens))

    def peak(node, path):
        mod.fused_ragged_node = node
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = mod(xyz1, xyz2, None, p2, geometry=geo, lengths1=lens)
        assert mod.last_path == path
        grads = torch.autograd.grad(out, [p2] + list(mod.parameters()), gout)
        torch.cuda.synchronize()
        del out, grads
        return torch.cuda.max_memory_allocated() - base
    peak(True, "fused_train_ragged_node")                                     # warm: both routes' kernels loaded
    peak(False, "fused_train_ragged")
    p_node, p_old = peak(True, "fused_train_ragged_node"), peak(False, "fused_train_ragged")
    print("peak memory: node route %d bytes, fused_train_ragged route %d bytes, the (b, n, c2) tensor %d bytes" %
          (p_node, p_old, b * n * c2 * 4))
    assert p_old - p_node >= b * n * c2 * 4, (p_node, p_old)
