"""The fused training node with FROZEN batch-norm statistics (train_mlp.sa_mlp_train / fp_mlp_train(..., frozen=True),
pn2_mlp_train_*_frozen, csrc/train_mlp_frozen.hip; modules: fused_frozen_bn, last_path "fused_frozen").

Kernel level: torch float64 autograd (on the device, as scripts/train_mlp_check.py: the configurations' own level shapes have up
to 2 M rows) over the layer-by-layer graph with the batch norms in eval() -- y = (h W^T + b -
running_mean) / sqrt(running_var + eps) * gamma + beta -- on the operators' indices, evaluated on the linear piece the kernels
chose (their ReLU decisions, their pooled sample; the scheme of tests/test_train_xyz_gpu.py). Checked: the output, the feature /
plain-input gradient, grad_xyz and grad_new_xyz, and dW, dgamma, dbeta and dbias of every layer. Bound: the project's rule
(tests/test_train_mlp_gpu.py): max(1e-5, 2 e32) of each tensor's scale, e32 = the worst error of torch's fp32 evaluation of the
same graph against the same float64 results. The running statistics are random and far from the batch's own (mean ~ N(0,1),
var ~ U(0.5,1.5)), some gammas are negative and one is exactly zero: a batch-statistics result misses the bound by orders of
magnitude, so the wrong node cannot pass.
Two deviations from a plain "float64 on the CPU against torch's own fp32 run": the float64 graph is evaluated by torch on the
device (independent kernels; a CPU evaluation of the 2 M-row levels takes minutes each), and e32 is torch's fp32 evaluation of the
SAME pinned linear piece, not torch's own layer-by-layer run with its own ReLU decisions (one flipped unit is an error of 1e-2 that
says nothing about fp32, tests/test_train_xyz_gpu.py) -- both make the bound tighter or leave it as it is, never wider.
Module level: the same module's layer-by-layer path (fused_mlp = False) on the same weights is the referee."""
import copy
from types import SimpleNamespace

import pytest
import torch

from test_train_pool_gpu import _net, _rel, _saved

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _pool(h, gx, mode, sel):
    """(groups, ns, C) -> pooled; the max on the kernels' sample `sel` (groups, C)."""
    if mode == "avg":
        return h.mean(dim=1)
    if mode == "weighted_avg":
        e = torch.exp(-gx.norm(dim=-1, keepdim=True) * 5)
        return (h * (e / e.sum(dim=1, keepdim=True))).sum(dim=1)
    top = h.gather(1, sel.long().unsqueeze(1)).squeeze(1)
    return top if mode == "max" else torch.cat([h.mean(dim=1), top], dim=-1)


def _ref(rows, gx, params, stats, eps, ns, mode, masks, sel):
    """The frozen graph on the pinned linear piece -> output, ReLU decisions that differ from the kernels', their margin."""
    h, flips, margin = rows, 0, 0.0
    for l, (W, bias, gamma, beta) in enumerate(params):
        mean, var = stats[l]
        y = (h @ W.t() + bias - mean) / torch.sqrt(var + eps[l]) * gamma + beta
        dis = (y.detach() > 0) != masks[l]
        flips += int(dis.sum())
        if dis.any():
            margin = max(margin, float(y.detach()[dis].abs().max() / y.detach().abs().max()))
        h = y * masks[l].to(y.dtype)
    if ns:
        h = _pool(h.view(-1, ns, h.shape[1]), gx, mode, sel)
    return h, flips, margin


def _rows(x, nx, p, idx, b, xyz_first):
    if idx is None:
        gx, gp = x.unsqueeze(1), (p.unsqueeze(1) if p is not None else None)
    else:
        li, bi = idx.long().to(x.device), torch.arange(b, device=x.device).view(b, 1, 1)
        gx = x[bi, li] - nx.unsqueeze(2)
        gp = p[bi, li] if p is not None else None
    parts = [gx, gp] if xyz_first else [gp, gx]
    full = torch.cat([t for t in parts if t is not None], dim=-1)
    return full.reshape(-1, full.shape[-1]), gx


def _frozen_net(cin, widths, g, dev):
    net = _net(cin, widths, g, dev)                                  # random gammas (some negative), betas, running statistics
    with torch.no_grad():
        for mod in net.net:
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight[1] = 0.0                                  # one scale exactly zero
    return net.eval()


def run_frozen_case(mode, b, n, m, ns, cfeat, widths, xyz_first=True, group_all=False, plain_cin=0, xyz_grad=False, seed=0, opts=None):
    """-> the kernels' worst relative error, torch fp32's own on the same graph, the errors by name, the gradients by name."""
    from pointnet2_amd import train_mlp
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(seed)
    torch.manual_seed(seed)
    cin = plain_cin or 3 + cfeat
    net = _frozen_net(cin, widths, g, dev)
    pairs = train_mlp.conv_bn_pairs(net.net)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    xyz = points = new_xyz = idx = x = None
    if plain_cin:
        x = torch.randn((b, n, cin), generator=g).to(dev).requires_grad_(True)
        nss = 0
    else:
        xyz = torch.rand((b, n, 3), generator=g).to(dev).requires_grad_(xyz_grad)
        points = torch.randn((b, n, cfeat), generator=g).to(dev).requires_grad_(True) if cfeat else None
        if group_all:
            mm, nss = 1, n
        else:
            sel = torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(b)]).to(dev)
            new_xyz = torch.gather(xyz.detach(), 1, sel.unsqueeze(-1).expand(-1, -1, 3)).contiguous().requires_grad_(xyz_grad)
            idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32)
            idx[:, :, ns // 2:] = idx[:, :, :1]                     # padded groups, like the ball query's
            idx = idx.to(dev)
            mm, nss = m, ns
    # The ReLU decisions are read back from the stored z_l. With top_stored = True (the default here) the node under test keeps
    # z_L itself; with top_stored = False / None (the z-free pooled top layer: what the size rule takes on the large levels) they
    # come from a TWIN forward of the same node on the same inputs that keeps z_L -- forward's arithmetic does not depend on it,
    # which the test asserts (same pooled output, same selected samples, bit for bit).
    opts = dict(opts or {})
    top_stored = opts.pop("top_stored", True)

    def forward():
        if plain_cin:
            return train_mlp.fp_mlp_train(net.net, x, frozen=True), None
        return train_mlp.sa_mlp_train(net.net, xyz, new_xyz, points, idx, xyz_first, pooling=mode, xyz_grad=xyz_grad, frozen=True)
    nl = len(pairs)
    with train_mlp.options(top_stored=True, **opts):
        twin, twin_sel = forward()
        zs, saves, _ = _saved(twin, nl, plain_cin or points is not None)
        masks = [((z * s[2]) + s[3] > 0) for z, s in zip(zs, saves)]     # two roundings, as the kernels' fmul + fadd
    with train_mlp.options(top_stored=top_stored, **opts):
        if top_stored is True:
            out, argsel = twin, twin_sel
        else:
            out, argsel = forward()
            assert torch.equal(out, twin) and torch.equal(argsel, twin_sel)
            if top_stored is False:
                node = out.grad_fn
                while type(node).__name__ != "_TrainMLPBackward":
                    node = node.next_functions[0][0]
                assert not node.nz[-1], "the node kept z_L although top_stored is off"
        params64 = [tuple(t.detach().double().requires_grad_(True) for t in
                          (conv.weight.view(conv.out_channels, -1), conv.bias, bn.weight, bn.bias)) for conv, bn in pairs]
        stats64 = [(bn.running_mean.double(), bn.running_var.double()) for _, bn in pairs]
        eps = [bn.eps for _, bn in pairs]
        sel = argsel.reshape(b * mm, -1) if argsel is not None else None

        def leaves(dt):
            if plain_cin:
                return [x.detach().to(dt).reshape(b * n, cin).requires_grad_(True)]
            return [xyz.detach().to(dt).requires_grad_(xyz_grad),
                    new_xyz.detach().to(dt).requires_grad_(xyz_grad) if new_xyz is not None else None,
                    points.detach().to(dt).requires_grad_(True) if cfeat else None]

        def graph(lv, params, stats):
            if plain_cin:
                return _ref(lv[0], None, params, stats, eps, 0, mode, masks, None)
            rows, gx = _rows(lv[0], lv[1], lv[2], idx, b, xyz_first)
            return _ref(rows, gx.reshape(b * mm, nss, 3), params, stats, eps, nss, mode, masks, sel)
        l64 = leaves(torch.float64)
        want, flips, margin = graph(l64, params64, stats64)
        gw = torch.randn(want.shape, generator=g, dtype=torch.float64).to(dev)
        (want * gw).sum().backward()
        (out.reshape(want.shape) * gw.float()).sum().backward()
        torch.cuda.synchronize()
    for k, v in net.state_dict().items():                            # running statistics and num_batches_tracked: never written
        assert torch.equal(v, before[k]), k
    # the yardstick: torch fp32 on the same graph, the same linear piece, against the same float64 results
    p32 = [tuple(t.detach().float().requires_grad_(True) for t in p) for p in params64]
    l32 = leaves(torch.float32)
    got32, _, _ = graph(l32, p32, [(a.float(), c.float()) for a, c in stats64])
    (got32 * gw.float()).sum().backward()
    errs, base, grads = {"out": _rel(out.reshape(want.shape), want)}, {"out": _rel(got32, want)}, {}
    mine = [x] if plain_cin else [xyz, new_xyz, points]
    for name, t, t32, t64 in zip(["dx"] if plain_cin else ["dxyz", "dnew_xyz", "dpts"], mine, l32, l64):
        if t is not None and t.requires_grad:
            errs[name], base[name] = _rel(t.grad.reshape(t64.shape), t64.grad), _rel(t32.grad, t64.grad)
            grads[name] = t.grad.detach().clone()
    for l, ((conv, bn), q32, q64) in enumerate(zip(pairs, p32, params64)):
        for name, t, k in (("dW", conv.weight, 0), ("db", conv.bias, 1), ("dg", bn.weight, 2), ("dbe", bn.bias, 3)):
            key = "%s%d" % (name, l + 1)
            errs[key], base[key] = _rel(t.grad.reshape(q64[k].shape), q64[k].grad), _rel(q32[k].grad, q64[k].grad)
            grads[key] = t.grad.detach().clone()
        assert float(conv.bias.grad.abs().max()) > 0.0              # NOT zero: the bias does not cancel under frozen statistics
    worst, e32 = max(errs.values()), max(base.values())
    print("%-12s worst %.2e (torch fp32 %.2e) flips %d margin %.1e  " % (mode, worst, e32, flips, margin) +
          " ".join("%s=%.1e" % kv for kv in errs.items()), flush=True)
    assert flips <= max(2, 1e-5 * sum(k.numel() for k in masks)) and margin <= 1e-5, (flips, margin)
    grads["out"] = out.detach().clone()
    return worst, e32, errs, grads


def _check(name, mode, worst, e32, errs):
    bound = max(TOL, 2.0 * e32)
    assert worst <= bound, "%s %s: worst %.2e (torch fp32 %.2e): %s" % (name, mode, worst, e32, errs)


# the SA and FP level shapes of reference configurations 2-5 (pointnet2_amd/reference_configs.py, scripts/config_shapes.py)
CONFIG_CASES = [
    ("cfg2 cls_ssg L1", dict(b=32, n=1024, m=512, ns=32, cfeat=0, widths=[64, 64, 128])),
    ("cfg2 cls_ssg L2", dict(b=32, n=512, m=128, ns=64, cfeat=128, widths=[128, 128, 256])),
    ("cfg2 cls_ssg L3 group_all", dict(b=32, n=128, m=1, ns=128, cfeat=256, widths=[256, 512, 1024], group_all=True)),
    ("cfg3 cls_msg L1 s1", dict(b=32, n=4096, m=512, ns=16, cfeat=3, widths=[32, 32, 64], xyz_first=False)),
    ("cfg3 cls_msg L1 s2", dict(b=32, n=4096, m=512, ns=32, cfeat=3, widths=[64, 64, 128], xyz_first=False)),
    ("cfg3 cls_msg L1 s3", dict(b=32, n=4096, m=512, ns=128, cfeat=3, widths=[64, 96, 128], xyz_first=False)),
    ("cfg3 cls_msg L2 s1", dict(b=32, n=512, m=128, ns=32, cfeat=320, widths=[64, 64, 128], xyz_first=False)),
    ("cfg3 cls_msg L2 s2", dict(b=32, n=512, m=128, ns=64, cfeat=320, widths=[128, 128, 256], xyz_first=False)),
    ("cfg3 cls_msg L2 s3", dict(b=32, n=512, m=128, ns=128, cfeat=320, widths=[128, 128, 256], xyz_first=False)),
    ("cfg3 cls_msg L3 group_all", dict(b=32, n=128, m=1, ns=128, cfeat=640, widths=[256, 512, 1024], group_all=True)),
    ("cfg4 part_seg SA1", dict(b=16, n=2048, m=512, ns=64, cfeat=3, widths=[64, 64, 128])),
    ("cfg4 part_seg SA2", dict(b=16, n=512, m=128, ns=64, cfeat=128, widths=[128, 128, 256])),
    ("cfg4 part_seg SA3 group_all", dict(b=16, n=128, m=1, ns=128, cfeat=256, widths=[256, 512, 1024], group_all=True)),
    ("cfg4 part_seg FP1", dict(b=16, n=128, m=0, ns=0, cfeat=0, widths=[256, 256], plain_cin=1280)),
    ("cfg4 part_seg FP2", dict(b=16, n=512, m=0, ns=0, cfeat=0, widths=[256, 128], plain_cin=384)),
    ("cfg4 part_seg FP3", dict(b=16, n=2048, m=0, ns=0, cfeat=0, widths=[128, 128, 128], plain_cin=134)),
    ("cfg5 sem_seg SA1", dict(b=8, n=8192, m=1024, ns=32, cfeat=0, widths=[32, 32, 64])),
    ("cfg5 sem_seg SA2", dict(b=8, n=1024, m=256, ns=32, cfeat=64, widths=[64, 64, 128])),
    ("cfg5 sem_seg SA3", dict(b=8, n=256, m=64, ns=32, cfeat=128, widths=[128, 128, 256])),
    ("cfg5 sem_seg SA4", dict(b=8, n=64, m=16, ns=32, cfeat=256, widths=[256, 256, 512])),
    ("cfg5 sem_seg FP1", dict(b=8, n=64, m=0, ns=0, cfeat=0, widths=[256, 256], plain_cin=768)),
    ("cfg5 sem_seg FP2", dict(b=8, n=256, m=0, ns=0, cfeat=0, widths=[256, 256], plain_cin=384)),
    ("cfg5 sem_seg FP3", dict(b=8, n=1024, m=0, ns=0, cfeat=0, widths=[256, 128], plain_cin=320)),
    ("cfg5 sem_seg FP4", dict(b=8, n=8192, m=0, ns=0, cfeat=0, widths=[128, 128, 128], plain_cin=128)),
]
SMALL_CASES = [
    ("ns16 msg order", dict(b=2, n=256, m=64, ns=16, cfeat=3, widths=[32, 32, 64], xyz_first=False)),
    ("group_all", dict(b=4, n=128, m=1, ns=128, cfeat=16, widths=[32, 64, 128], group_all=True)),
    ("msg order c32 ns64", dict(b=4, n=256, m=32, ns=64, cfeat=32, widths=[64, 64, 128], xyz_first=False)),
    ("one layer", dict(b=2, n=256, m=64, ns=32, cfeat=16, widths=[64])),
    ("xyz only", dict(b=2, n=256, m=64, ns=32, cfeat=0, widths=[32, 32, 64])),
    ("plain odd width 128 + 6", dict(b=2, n=2048, m=0, ns=0, cfeat=0, widths=[128, 128], plain_cin=134)),
    ("plain one layer", dict(b=2, n=512, m=0, ns=0, cfeat=0, widths=[64], plain_cin=32)),
]


# every level with the coordinates constant; the grouped ones with grad_xyz / grad_new_xyz as well (plain rows have no coordinates)
ALL_CASES = [(n_, kw_, False) for n_, kw_ in CONFIG_CASES + SMALL_CASES] + \
    [(n_, kw_, True) for n_, kw_ in CONFIG_CASES + SMALL_CASES if not kw_.get("plain_cin")]


@pytest.mark.parametrize("name,kw,xyz_grad", ALL_CASES, ids=["%s-%s" % (c[0], "xyz_grad" if c[2] else "xyz_const") for c in ALL_CASES])
def test_frozen_node_matches_float64(cuda, name, kw, xyz_grad):
    worst, e32, errs, _ = run_frozen_case("max", xyz_grad=xyz_grad, **kw)
    _check(name, "max", worst, e32, errs)


POOL_CASES = [c for c in CONFIG_CASES if c[0] in ("cfg2 cls_ssg L1", "cfg2 cls_ssg L2", "cfg5 sem_seg SA4")] + \
    [c for c in SMALL_CASES if not c[1].get("plain_cin")]


@pytest.mark.parametrize("xyz_grad", [False, True], ids=["xyz_const", "xyz_grad"])
@pytest.mark.parametrize("mode", ["avg", "weighted_avg", "max_and_avg"])
@pytest.mark.parametrize("name,kw", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_frozen_node_matches_float64_pooled(cuda, name, kw, mode, xyz_grad):
    if xyz_grad and mode == "weighted_avg":
        with pytest.raises(ValueError):                              # refused, as in the batch-statistics node
            run_frozen_case(mode, xyz_grad=True, **kw)
        return
    worst, e32, errs, _ = run_frozen_case(mode, xyz_grad=xyz_grad, **kw)
    _check(name, mode, worst, e32, errs)


# The pooled top layer WITHOUT its pre-norm tensor (top_stored off: what the size rule takes from 32 MB of z_L on, the metric shape
# and most configuration levels): tl_top_mats_kernel / tl_top_wgrad_fix_kernel / tl_top_s_kernel with the (a, 0, 0) coefficients,
# its routed part on the vector units or on the dense tiles, and the one-pass form (fuse_wgrad). The small shapes force it, as
# tests/test_train_mlp_gpu.py::test_routed_top_gradient_variants does for the batch-statistics node; the last case takes it by the
# size rule alone (top_stored = None: automatic).
ZTOP_SHAPES = [
    ("A xyz 32-32-64", dict(b=2, n=256, m=64, ns=32, cfeat=0, widths=[32, 32, 64])),
    ("B c64 64-64-128", dict(b=4, n=512, m=128, ns=32, cfeat=64, widths=[64, 64, 128])),
    ("C ns16 msg order", dict(b=2, n=256, m=64, ns=16, cfeat=3, widths=[32, 32, 64], xyz_first=False)),
    ("D c128 128-128-256 ns64", dict(b=4, n=512, m=64, ns=64, cfeat=128, widths=[128, 128, 256])),
    ("E group_all 256-512-1024", dict(b=4, n=128, m=1, ns=128, cfeat=256, widths=[256, 512, 1024], group_all=True)),
    ("H 64-96-128 ns128", dict(b=2, n=512, m=64, ns=128, cfeat=0, widths=[64, 96, 128])),
    ("two layers", dict(b=2, n=256, m=64, ns=32, cfeat=16, widths=[64, 128])),
]
ZTOP_OPTS = [dict(top_stored=False), dict(top_stored=False, top_sparse=True), dict(top_stored=False, top_sparse=False),
             dict(top_stored=False, fuse_wgrad=True), dict(top_stored=False, fuse_wgrad=False, pair_launch=False)]
_oid = lambda o: ",".join("%s=%s" % kv for kv in o.items())


@pytest.mark.parametrize("xyz_grad", [False, True], ids=["xyz_const", "xyz_grad"])
@pytest.mark.parametrize("opts", ZTOP_OPTS, ids=[_oid(o) for o in ZTOP_OPTS])
@pytest.mark.parametrize("name,kw", ZTOP_SHAPES, ids=[c[0] for c in ZTOP_SHAPES])
def test_frozen_node_without_the_top_tensor_matches_float64(cuda, name, kw, opts, xyz_grad):
    worst, e32, errs, _ = run_frozen_case("max", xyz_grad=xyz_grad, opts=opts, **kw)
    _check(name, _oid(opts), worst, e32, errs)


AUTO_ZTOP = [c for c in CONFIG_CASES if c[0] in ("cfg2 cls_ssg L1", "cfg2 cls_ssg L2", "cfg3 cls_msg L1 s2", "cfg5 sem_seg SA1")]


@pytest.mark.parametrize("xyz_grad", [False, True], ids=["xyz_const", "xyz_grad"])
@pytest.mark.parametrize("name,kw", AUTO_ZTOP, ids=[c[0] for c in AUTO_ZTOP])
def test_frozen_node_under_the_size_rules_matches_float64(cuda, name, kw, xyz_grad):
    """The organisation a user gets at the configurations' own sizes (top_stored automatic: z_L is not kept on these levels)."""
    import ctypes
    from pointnet2_amd import _C
    widths = [3 + kw["cfeat"]] + kw["widths"]
    rows = kw["b"] * kw["m"] * kw["ns"]
    assert not _C.lib().pn2_mlp_train_top_stored_ex(rows, len(widths) - 1, (ctypes.c_int * len(widths))(*widths), kw["ns"], None)
    worst, e32, errs, _ = run_frozen_case("max", xyz_grad=xyz_grad, opts=dict(top_stored=None), **kw)
    _check(name, "automatic", worst, e32, errs)


OPTS = [dict(top_stored=False), dict(top_stored=False, fuse_wgrad=True), dict(top_stored=False, top_sparse=True),
        dict(l1_per_point=True, l1_coords=False), dict(l1_per_point=False, l1_coords=False),
        dict(l1_coords=True), dict(fuse_wgrad=True), dict(fuse_wgrad=False), dict(pair_launch=True), dict(pair_launch=False),
        dict(max_ns=1), dict(max_ns=2)]


@pytest.mark.parametrize("opts", OPTS, ids=[_oid(o) for o in OPTS])
def test_organisation_overrides_change_no_result(cuda, opts):
    """Every pn2_train_opts override against the automatic organisation on the same inputs: within the bound of the float64
    comparison itself (the orders of the fp64 partial sums differ, include/pn2ops.h), and each one inside the float64 bound."""
    for name, kw in (("B", dict(b=4, n=512, m=128, ns=32, cfeat=64, widths=[64, 64, 128])),
                     ("A", dict(b=2, n=256, m=64, ns=32, cfeat=0, widths=[32, 32, 64])),
                     ("N", dict(b=2, n=256, m=64, ns=32, cfeat=3, widths=[32, 32, 64]))):
        for xyz_grad in (False, True):
            _, _, _, ref = run_frozen_case("max", xyz_grad=xyz_grad, **kw)
            worst, e32, errs, got = run_frozen_case("max", xyz_grad=xyz_grad, opts=opts, **kw)
            _check(name, str(opts), worst, e32, errs)
            for k in ref:
                assert _rel(got[k], ref[k]) <= TOL, (name, k)


# ---- module level --------------------------------------------------------------------------------------------------------------
def _freeze(mod, eval_module):
    """Random running statistics far from the batch's own; the module in eval(), or in train() with its batch norms in eval()."""
    mod.eval() if eval_module else mod.train()
    with torch.no_grad():
        for sub in mod.modules():
            if isinstance(sub, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                sub.eval()
                sub.running_mean.normal_()
                sub.running_var.uniform_(0.5, 1.5)
                sub.weight.uniform_(-0.4, 1.1)
    return mod


def _pair(mod, flag=True):
    ref = copy.deepcopy(mod)
    ref.fused_mlp = False
    mod.fused_frozen_bn = flag
    return mod, ref


def _l2(a, b):
    return float((a - b).norm() / max(1e-30, float(b.norm())))


def _run(mod, args, gw=None, **kw):
    """forward + backward of an SA / MSG module -> output, its gradient weights."""
    res = mod(*args, **kw)
    out = res[1]
    if gw is None:
        gw = torch.randn_like(out)
    (out * gw).sum().backward()
    return out, gw


def _compare(mod, ref, make_args, expect="fused_frozen", kw=None, kw_ref=None):
    """The module against its own layer-by-layer path: outputs tight, gradients in the L2 sense (two fp32 evaluations may sit on
    different linear pieces at a few elements), state_dict untouched, the conv-bias gradient non-zero."""
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    a, b_ = make_args(), make_args()
    oa, gw = _run(mod, a, **(kw or {}))
    ob, _ = _run(ref, b_, gw, **(kw_ref or kw or {}))
    assert mod.last_path == expect and ref.last_path == "unfused", (mod.last_path, ref.last_path)
    for k, v in mod.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert float((oa - ob).detach().abs().max()) <= 5e-5 * float(ob.detach().abs().max())
    for ta, tb in zip(a, b_):
        if ta is not None and ta.requires_grad:
            assert _l2(ta.grad, tb.grad) <= 5e-3
    for (na, pa), (_, pb) in zip(mod.named_parameters(), ref.named_parameters()):
        if pb.grad is None:
            assert pa.grad is None, na
            continue
        assert float(pb.grad.abs().max()) > 0 and _l2(pa.grad, pb.grad) <= 5e-3, na
    return a, b_


def test_modules_take_the_frozen_node(cuda):
    """SA (ball query, knn, group_all, mlp2, every pooling, a geometry computed ahead), MSG and FP; the module in eval() and in
    train() with its batch norms in eval(); feature, coordinate and parameter gradients."""
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd.geometry import GeometryAhead
    torch.manual_seed(0)
    xyz0 = torch.rand(4, 256, 3, device=cuda)
    f0 = torch.randn(4, 256, 16, device=cuda)

    def args(want_xyz=False):
        return lambda: (xyz0.clone().requires_grad_(want_xyz), f0.clone().requires_grad_(True))
    for eval_module in (True, False):
        for kw in (dict(), dict(knn=True), dict(group_all=True), dict(mlp2=[64, 32]), dict(pooling="avg"), dict(pooling="weighted_avg"),
                   dict(pooling="max_and_avg")):
            sa, ref = _pair(_freeze(U.PointnetSAModule(16, 64, 0.4, 32, [32, 32, 64], **kw).to(cuda), eval_module))
            _compare(sa, ref, args())
            if kw.get("pooling") != "weighted_avg":
                sa.fused_xyz_grad = True
                _compare(sa, ref, args(True))
        msg, ref = _pair(_freeze(U.PointnetSAModuleMSG(16, 64, [0.2, 0.4], [16, 32], [[32, 32, 64], [32, 48, 64]]).to(cuda), eval_module))
        _compare(msg, ref, args())
        msg.fused_xyz_grad = True
        _compare(msg, ref, args(True))
        sa, ref = _pair(_freeze(U.PointnetSAModule(16, 64, 0.4, 32, [32, 32, 64]).to(cuda), eval_module))
        sa.fused_xyz_grad = True
        geo = GeometryAhead([sa]).compute(xyz0).sa[0]
        _compare(sa, ref, args(True), kw=dict(geometry=geo))
        msg, ref = _pair(_freeze(U.PointnetSAModuleMSG(16, 64, [0.2, 0.4], [16, 32], [[32, 32, 64], [32, 48, 64]]).to(cuda), eval_module))
        msg.fused_xyz_grad = True
        geo = GeometryAhead([msg]).compute(xyz0).sa[0]
        _compare(msg, ref, args(True), kw=dict(geometry=geo))
        for c1, ahead in ((4, False), (6, False), (6, True)):        # (128 + 6: an odd width, zero-padded; ahead: three_nn computed ahead)
            fp, rfp = _pair(_freeze(U.PointnetFPModule(128 + c1, [64, 64]).to(cuda), eval_module))
            before = {k: v.clone() for k, v in fp.state_dict().items()}
            outs = []
            x2 = xyz0[:, :64].contiguous()
            for m_ in (fp, rfp):
                p1 = torch.randn(4, 256, c1, generator=torch.Generator().manual_seed(1)).to(cuda).requires_grad_(True)
                p2 = torch.randn(4, 64, 128, generator=torch.Generator().manual_seed(2)).to(cuda).requires_grad_(True)
                if ahead:
                    from pointnet2_amd.tf_interpolate import three_nn
                    dist, nidx = three_nn(xyz0, x2)
                    up = m_._forward_on(xyz0, p1, p2, SimpleNamespace(dist=dist, idx=nidx))     # three_nn's result computed ahead
                else:
                    up = m_(xyz0, x2, p1, p2)
                up.square().mean().backward()
                outs.append((up, p1.grad, p2.grad))
            assert fp.last_path == "fused_frozen" and rfp.last_path == "unfused"
            for k, v in fp.state_dict().items():
                assert torch.equal(v, before[k]), k
            assert float((outs[0][0] - outs[1][0]).abs().max()) <= 5e-5 * float(outs[1][0].abs().max())
            assert _l2(outs[0][1], outs[1][1]) <= 5e-3 and _l2(outs[0][2], outs[1][2]) <= 5e-3
            for (na, pa), (_, pb) in zip(fp.named_parameters(), rfp.named_parameters()):
                assert float(pb.grad.abs().max()) > 0 and _l2(pa.grad, pb.grad) <= 5e-3, na


def test_flag_off_is_the_layer_by_layer_path_bit_for_bit(cuda):
    """Flag off (the default): SA, MSG and FP in eval() and in train() with frozen batch norms report "unfused", and outputs and
    gradients are the BITS of the same module with fused_mlp = False (set_deterministic(True): the scatter gradients in their
    reproducible form; cudnn.deterministic: torch's own convolution gradients likewise)."""
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(1)
    xyz0 = torch.rand(4, 256, 3, device=cuda)
    f0 = torch.randn(4, 256, 16, device=cuda)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    P.set_deterministic(True)

    def same(mod, ref, a, b_, oa, ob):
        assert mod.last_path == "unfused" and ref.last_path == "unfused"
        assert torch.equal(oa, ob)
        for ta, tb in zip(a, b_):
            if ta is not None and ta.requires_grad:
                assert torch.equal(ta.grad, tb.grad)
        for (na, pa), (_, pb) in zip(mod.named_parameters(), ref.named_parameters()):
            assert torch.equal(pa.grad, pb.grad), na
    try:
        for eval_module in (True, False):
            for want_xyz in (False, True):
                mk = lambda: (xyz0.clone().requires_grad_(want_xyz), f0.clone().requires_grad_(True))
                for make in (lambda: U.PointnetSAModule(16, 64, 0.4, 32, [32, 32, 64]),
                             lambda: U.PointnetSAModule(16, 64, 0.4, 32, [32, 32, 64], pooling="max_and_avg", mlp2=[64]),
                             lambda: U.PointnetSAModuleMSG(16, 64, [0.2, 0.4], [16, 32], [[32, 32, 64], [32, 48, 64]])):
                    mod, ref = _pair(_freeze(make().to(cuda), eval_module), flag=False)
                    mod.fused_xyz_grad = True
                    a, b_ = mk(), mk()
                    oa, gw = _run(mod, a)
                    ob, _ = _run(ref, b_, gw)
                    same(mod, ref, a, b_, oa, ob)
            fp, rfp = _pair(_freeze(U.PointnetFPModule(128 + 6, [64, 64]).to(cuda), eval_module), flag=False)
            res = []
            for m_ in (fp, rfp):
                p1 = torch.randn(4, 256, 6, generator=torch.Generator().manual_seed(1)).to(cuda).requires_grad_(True)
                p2 = torch.randn(4, 64, 128, generator=torch.Generator().manual_seed(2)).to(cuda).requires_grad_(True)
                up = m_(xyz0, xyz0[:, :64].contiguous(), p1, p2)
                up.square().mean().backward()
                res.append(((p1, p2), up))
            same(fp, rfp, res[0][0], res[1][0], res[0][1], res[1][1])
    finally:
        P.set_deterministic(False)
        torch.backends.cudnn.deterministic = det


def test_what_the_training_node_refuses_stays_refused(cuda):
    import pointnet2_amd.pointnet_util as U
    xyz = torch.rand(2, 128, 3, device=cuda)
    f = torch.randn(2, 128, 8, device=cuda, requires_grad=True)

    def path(mod, x=xyz, feats=f):
        mod.fused_frozen_bn = True
        mod(x, feats)
        return mod.last_path
    assert path(_freeze(U.PointnetSAModule(8, 16, 0.4, 32, [32, 32, 64]).to(cuda), True)) == "fused_frozen"
    mixed = _freeze(U.PointnetSAModule(8, 16, 0.4, 32, [32, 32, 64]).to(cuda), False)
    mixed.mlp.net[1].train()                                         # one batch norm on batch statistics, two frozen
    assert path(mixed) == "unfused"
    assert path(U.PointnetSAModule(8, 16, 0.4, 32, [32, 32, 64], bn=False).to(cuda).eval()) == "unfused"
    assert path(_freeze(U.PointnetSAModule(8, 16, 0.4, 32, [32, 32, 64], use_xyz=False).to(cuda), True)) == "unfused"
    assert path(_freeze(U.PointnetSAModule(8, 16, 0.4, 24, [32, 32, 64]).to(cuda), True)) == "unfused"         # nsample 24
    wa = _freeze(U.PointnetSAModule(8, 16, 0.4, 32, [32, 32, 64], pooling="weighted_avg").to(cuda), True)
    wa.fused_xyz_grad = True
    assert path(wa, xyz.clone().requires_grad_(True)) == "unfused"
    nx = _freeze(U.PointnetSAModule(8, 16, 0.4, 32, [32, 32, 64]).to(cuda), True)                              # xyz wants a gradient, fused_xyz_grad off
    assert path(nx, xyz.clone().requires_grad_(True)) == "unfused"
    with torch.no_grad():                                            # eval() without autograd keeps the inference kernels
        assert path(_freeze(U.PointnetSAModule(8, 16, 0.4, 32, [32, 32, 64]).to(cuda), True)) == "fused"
    off = _freeze(U.PointnetSAModule(8, 16, 0.4, 32, [32, 32, 64]).to(cuda), True)
    off(xyz, f)
    assert off.last_path == "unfused"                                # the flag is off by default


def test_parameters_without_gradient_get_none_and_inputs_the_same_bits(cuda):
    """requires_grad = False on every parameter (saliency, a frozen backbone): no parameter gradient is produced, and the input
    gradients are those of the run with all gradients, bit for bit in reproducible mode. The library then runs no
    weight-gradient pass and sums nothing for these layers (pn2_mlp_train_backward_frozen: all four slots NULL); no kernel-name
    helper exists in the test suite, the rocprofv3 listing under profiles/frozen_bn/ shows the launches."""
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(2)
    xyz0 = torch.rand(4, 256, 3, device=cuda)
    f0 = torch.randn(4, 256, 16, device=cuda)
    from pointnet2_amd import train_mlp

    def case(kw, feats):
        sa = _freeze(U.PointnetSAModule(16 if feats else 0, 64, 0.4, 32, [32, 32, 64], **kw).to(cuda), True)
        sa.fused_frozen_bn = sa.fused_xyz_grad = True
        res = []
        for need in (True, False, "top"):
            for i, p in enumerate(sa.parameters()):
                p.requires_grad_(need is True or (need == "top" and i >= 8))     # "top": only the last layer's parameters
                p.grad = None
            x = xyz0.clone().requires_grad_(True)
            f = f0.clone().requires_grad_(True) if feats else None
            out = sa(x, f)[1]
            assert sa.last_path == "fused_frozen"
            (out * torch.ones_like(out)).sum().backward()
            for i, p in enumerate(sa.parameters()):
                assert (p.grad is not None) == p.requires_grad, i
            res.append((out.detach(), x.grad, f.grad if feats else None, [p.grad for p in sa.parameters()]))
        for other in res[1:]:
            assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
            assert not feats or torch.equal(res[0][2], other[2])
        for ga, gb in zip(res[0][3][8:], res[2][3][8:]):
            assert torch.equal(ga, gb)
    P.set_deterministic(True)
    try:
        # (top_stored = False: the same with the z-free pooled top layer, whose skipped form runs the data-gradient GEMM alone)
        for top_stored, shapes in ((None, (dict(), dict(group_all=True), dict(pooling="max_and_avg"))),
                                   (False, (dict(), dict(group_all=True)))):
            with train_mlp.options(top_stored=top_stored):
                for kw in shapes:
                    for feats in (True, False):
                        case(kw, feats)
        # a frozen backbone below a trained top layer, nothing wanted for the inputs: the chain stops at the top layer
        for top_stored in (None, False):
            with train_mlp.options(top_stored=top_stored):
                sa = _freeze(U.PointnetSAModule(16, 64, 0.4, 32, [32, 32, 64]).to(cuda), False)
                sa.fused_frozen_bn = True
                full = []
                for top_only in (False, True):
                    for i, p in enumerate(sa.parameters()):
                        p.requires_grad_(not top_only or i >= 8)
                        p.grad = None
                    out = sa(xyz0, f0)[1]
                    assert sa.last_path == "fused_frozen"
                    out.sum().backward()
                    full.append([p.grad for p in sa.parameters()])
                assert all(g is None for g in full[1][:8])
                for ga, gb in zip(full[0][8:], full[1][8:]):
                    assert torch.equal(ga, gb)
    finally:
        P.set_deterministic(False)


def test_deterministic_mode_gives_identical_bits(cuda):
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(3)
    xyz0 = torch.rand(4, 512, 3, device=cuda)
    f0 = torch.randn(4, 512, 64, device=cuda)
    sa = _freeze(U.PointnetSAModule(64, 128, 0.4, 32, [64, 64, 128]).to(cuda), True)
    sa.fused_frozen_bn = sa.fused_xyz_grad = True
    P.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            for p in sa.parameters():
                p.grad = None
            x, f = xyz0.clone().requires_grad_(True), f0.clone().requires_grad_(True)
            out = sa(x, f)[1]
            out.square().sum().backward()
            runs.append([out.detach(), x.grad, f.grad] + [p.grad for p in sa.parameters()])
        assert sa.last_path == "fused_frozen"
        for a, b_ in zip(*runs):
            assert torch.equal(a, b_)
    finally:
        P.set_deterministic(False)


def test_parameter_gradients_added_into_existing_grads_bias_included(cuda):
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    from pointnet2_amd.sharding import GradBucket
    torch.manual_seed(3)
    sa = _freeze(U.PointnetSAModule(64, 128, 0.4, 32, [64, 64, 128]).to(cuda), False)
    sa.fused_frozen_bn = True
    ref = copy.deepcopy(sa)
    xyz = torch.rand(4, 512, 3, device=cuda)
    feats = torch.randn(4, 512, 64, device=cuda)
    gw = torch.randn(4, 128, 128, device=cuda)
    bucket = GradBucket(sa.parameters())
    bucket.zero_()
    views = [p.grad.data_ptr() for p in sa.parameters()]
    with train_mlp.accumulate_into_grad():
        for _ in range(2):                                          # two micro-batches into the same bucket
            (sa(xyz, feats)[1] * gw).sum().backward()
    assert sa.last_path == "fused_frozen"
    assert [p.grad.data_ptr() for p in sa.parameters()] == views, "the .grad views were replaced"
    for _ in range(2):
        (ref(xyz, feats)[1] * gw).sum().backward()
    assert ref.last_path == "fused_frozen"
    for (name, p), q in zip(sa.named_parameters(), ref.parameters()):
        scale = float(q.grad.abs().max())
        assert scale > 0 and float((p.grad - q.grad).abs().max()) <= 1e-6 * scale, name


def test_frozen_step_is_graph_capturable(cuda):
    """forward + backward of a frozen SA level inside ONE HIP graph (the scheme of test_fused_training_step_is_graph_capturable):
    the replay on new data equals the eager evaluation of the same data."""
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(3)
    sa = _freeze(U.PointnetSAModule(16, 64, 0.4, 32, [32, 32, 64]).to(cuda), True)
    sa.fused_frozen_bn = True
    xyz = torch.rand(4, 256, 3, device=cuda)
    feats = torch.randn(4, 256, 16, device=cuda, requires_grad=True)
    w = torch.randn(4, 64, 64, device=cuda)
    params = list(sa.parameters())

    def step():
        _, out, _ = sa(xyz, feats)
        return out, torch.autograd.grad((out * w).sum(), params + [feats])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, grads_g = step()
    assert sa.last_path == "fused_frozen"
    xyz.copy_(torch.rand(4, 256, 3, device=cuda))
    with torch.no_grad():
        feats.copy_(torch.randn(4, 256, 16, device=cuda))
    g.replay()
    torch.cuda.synchronize()
    out_e, grads_e = step()
    assert torch.equal(out_g, out_e)
    for a, b_ in zip(grads_g, grads_e):
        assert float((a - b_).abs().max()) <= 1e-6 * max(1e-30, float(b_.abs().max()))
