"""The fused training node with the averaging pooling modes of pointnet_sa_module (utils/pointnet_util.py:128-142): avg,
weighted_avg and max_and_avg (csrc/train_mlp.hip: tl_pool_avg_kernel, tl_pool_top_grad_kernel; pn2_mlp_train_*_pool).

Kernel level: against torch float64 autograd on the CPU of the same graph -- grouped rows, conv / batch norm (batch
statistics) / ReLU, then the pooling formula of oracle/sa_module.py:pool. As in tests/test_train_mlp_gpu.py, a ReLU whose
argument is within fp32 rounding of zero is decided by rounding: the float64 graph is evaluated on the linear piece the
kernels chose (their ReLU decisions, and max_and_avg's pooled sample), and the decisions are checked on their own."""
import copy

import pytest
import torch

from test_train_mlp_gpu import CONFIG_CASES, KERNEL_CASES

pytestmark = pytest.mark.gpu

TOL = 1e-5
MODES = ["avg", "weighted_avg", "max_and_avg"]
CASES = [c for c in KERNEL_CASES if c[0][0] in "ABCDEHI"] + [c for c in CONFIG_CASES if c[0] in ("cfg2 cls_ssg L1", "cfg5 sem_seg SA2")]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-30, float(b.abs().max())))


def _net(cin, widths, g, dev):
    import pointnet2_amd.pointnet_util as U
    net = U._SharedMLP(cin, widths, bn=True).to(dev).train()
    with torch.no_grad():
        for mod in net.net:
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) * 1.5 - 0.4)       # some negative scales
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.3)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    return net


def _pool64(h, gx, mode, sel):
    """oracle/sa_module.py:pool on (groups, ns, C) rows; max_and_avg's max half on the kernels' sample `sel`."""
    if mode == "avg":
        return h.mean(dim=1)
    if mode == "weighted_avg":
        e = torch.exp(-gx.norm(dim=-1, keepdim=True) * 5)
        return (h * (e / e.sum(dim=1, keepdim=True))).sum(dim=1)
    top = h.max(dim=1)[0] if sel is None else h.gather(1, sel.long().unsqueeze(1)).squeeze(1)
    return torch.cat([h.mean(dim=1), top], dim=-1)


def _ref(rows, gx, params, eps, ns, mode, masks=None, sel=None):
    """The level's graph on the CPU: (groups ns, cin) rows -> pooled (groups, C or 2 C), the batch moments of every layer."""
    h, moments, flips, margin = rows, [], 0, 0.0
    for l, (W, bias, gamma, beta) in enumerate(params):
        z = h @ W.t() + bias
        mean, var = z.mean(0), z.var(0, unbiased=False)
        y = (z - mean) / torch.sqrt(var + eps[l]) * gamma + beta
        if masks is None:
            h = torch.relu(y)
        else:
            dis = (y.detach() > 0) != masks[l]
            flips += int(dis.sum())
            if dis.any():
                margin = max(margin, float(y.detach()[dis].abs().max() / y.detach().abs().max()))
            h = y * masks[l].to(y.dtype)
        moments.append((mean, var))
    c = h.shape[1]
    out = _pool64(h.view(-1, ns, c), gx, mode, sel)
    gap = 0.0
    if sel is not None:                     # the kernels' sample must attain the maximum
        top = torch.relu(h.detach()).view(-1, ns, c).max(dim=1)[0]
        gap = float((top - out.detach()[:, c:]).abs().max() / max(1e-30, float(top.abs().max())))
    return out, moments, flips, margin, gap


def _saved(out, nl, has_x):
    """(z_l, save_l, pool_w) of the fused node behind `out` (saved: x?, weights, biases, gammas, betas, z_l, save_l, out, argsel, ...)."""
    node = out.grad_fn
    while node is not None and type(node).__name__ != "_TrainMLPBackward":
        node = node.next_functions[0][0]
    sv = list(node.saved_tensors)
    off = (1 if has_x else 0) + 4 * nl
    zs, saves = sv[off:off + nl], sv[off + nl:off + 2 * nl]
    return zs, saves, sv[-1] if node.code == 2 else None


def run_pool_case(mode, b, n, m, ns, cfeat, widths, xyz_first=True, group_all=False, seed=0, idx=None, xyz=None, new_xyz=None):
    """-> worst relative error of every checked tensor, torch fp32's own worst error on the same graph."""
    from pointnet2_amd import train_mlp
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(seed)
    torch.manual_seed(seed)
    cin = 3 + cfeat
    net = _net(cin, widths, g, dev)
    pairs = train_mlp.conv_bn_pairs(net.net)
    rm0 = [bn.running_mean.clone() for _, bn in pairs]
    rv0 = [bn.running_var.clone() for _, bn in pairs]
    if xyz is None:
        xyz = torch.rand((b, n, 3), generator=g).to(dev)
    points = torch.randn((b, n, cfeat), generator=g).to(dev).requires_grad_(True) if cfeat else None
    if group_all:
        mm, nss = 1, n
    else:
        if new_xyz is None:
            sel = torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(b)]).to(dev)
            new_xyz = torch.gather(xyz, 1, sel.unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        if idx is None:
            idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(dev)
            idx[:, :, ns // 2:] = idx[:, :, :1]                 # padded groups, like the ball query's
        mm, nss = m, ns
    out, argsel = train_mlp.sa_mlp_train(net.net, xyz, None if group_all else new_xyz, points, None if group_all else idx,
                                         xyz_first, pooling=mode)
    nl = len(pairs)
    zs, saves, pool_w = _saved(out, nl, points is not None)
    masks = [((z * s[2]) + s[3] > 0).cpu() for z, s in zip(zs, saves)]     # two roundings, as the kernels' fmul + fadd
    # float64 rows on the CPU
    x64, p64 = xyz.double().cpu(), points.detach().double().cpu().requires_grad_(True) if cfeat else None
    if group_all:
        gx, gp = x64.unsqueeze(1), (p64.unsqueeze(1) if cfeat else None)
    else:
        li, bi = idx.long().cpu(), torch.arange(b).view(b, 1, 1)
        gx = x64[bi, li] - new_xyz.double().cpu().unsqueeze(2)
        gp = p64[bi, li] if cfeat else None
    parts = [gx, gp] if xyz_first else [gp, gx]
    rows64 = torch.cat([t for t in parts if t is not None], dim=-1).reshape(b * mm * nss, cin)
    if cfeat:
        rows64.retain_grad()
    params64 = [tuple(t.detach().double().cpu().requires_grad_(True) for t in
                      (conv.weight.view(conv.out_channels, -1), conv.bias, bn.weight, bn.bias)) for conv, bn in pairs]
    eps = [bn.eps for _, bn in pairs]
    gxr = gx.reshape(b * mm, nss, 3)
    sel = argsel.reshape(b * mm, -1).cpu() if argsel is not None else None
    want, moments, flips, margin, gap = _ref(rows64, gxr, params64, eps, nss, mode, masks, sel)
    gw = torch.randn(want.shape, generator=g, dtype=torch.float64)
    (want * gw).sum().backward()
    (out.reshape(want.shape) * gw.float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    errs = {"out": _rel(out.reshape(want.shape), want), "pool_gap": gap}
    if pool_w is not None:
        e = torch.exp(-gxr.norm(dim=-1) * 5)
        errs["pool_w"] = _rel(pool_w.view(b * mm, nss), e / e.sum(dim=1, keepdim=True))
    nrows = rows64.shape[0]
    for l, ((conv, bn), p) in enumerate(zip(pairs, params64)):
        errs["dW%d" % (l + 1)] = _rel(conv.weight.grad.view(conv.out_channels, -1), p[0].grad)
        errs["dg%d" % (l + 1)] = _rel(bn.weight.grad, p[2].grad)
        errs["dbe%d" % (l + 1)] = _rel(bn.bias.grad, p[3].grad)
        mean, var = moments[l]
        errs["rm%d" % (l + 1)] = _rel(bn.running_mean, (1 - bn.momentum) * rm0[l].double().cpu() + bn.momentum * mean.detach())
        errs["rv%d" % (l + 1)] = _rel(bn.running_var, (1 - bn.momentum) * rv0[l].double().cpu() +
                                      bn.momentum * var.detach() * nrows / (nrows - 1))
        assert float(conv.bias.grad.abs().max()) == 0.0
    if cfeat:
        errs["dpts"] = _rel(points.grad, p64.grad)
    # the scale: torch fp32 on the same graph (its own ReLU decisions and pool) against the same float64 results
    p32 = [tuple(t.detach().float().requires_grad_(True) for t in p) for p in params64]
    r32 = rows64.detach().float().requires_grad_(True)
    got32, _, _, _, _ = _ref(r32, gxr.float(), p32, eps, nss, mode)
    (got32 * gw.float()).sum().backward()
    base = [_rel(got32, want)]
    for q32, q64 in zip(p32, params64):
        base += [_rel(q32[0].grad, q64[0].grad), _rel(q32[2].grad, q64[2].grad), _rel(q32[3].grad, q64[3].grad)]
    if cfeat:
        base.append(_rel(r32.grad, rows64.grad))
    worst = max(errs.values())
    assert flips <= max(2, 1e-5 * sum(k.numel() for k in masks)) and margin <= 1e-5, (flips, margin)
    print("%-14s worst %.2e  " % (mode, worst) + " ".join("%s=%.1e" % kv for kv in errs.items()), flush=True)
    return worst, max(base), errs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_pooled_training_matches_float64(cuda, name, kw, mode):
    worst, base, errs = run_pool_case(mode, **kw)
    bound = max(TOL, 2.0 * base)
    assert worst <= bound, "%s %s: worst %.2e (torch fp32 %.2e): %s" % (name, mode, worst, base, errs)


@pytest.mark.parametrize("mode", ["avg", "weighted_avg"])
def test_sparse_balls_count_padded_duplicates(cuda, mode):
    """Clouds where most balls hold fewer points than nsample: the ball query pads with the first hit, and the average counts
    those duplicates (reduce_mean over nsample, :130-131; the weights of :132-138 likewise)."""
    from pointnet2_amd import synthetic as S
    from pointnet2_amd.tf_grouping import query_ball_point
    from pointnet2_amd.tf_sampling import farthest_point_sample, gather_point
    xyz = torch.from_numpy(S.sphere_clouds(4, 512, 11)).to(cuda)
    new_xyz = gather_point(xyz, farthest_point_sample(128, xyz))
    idx, cnt = query_ball_point(0.12, 32, xyz, new_xyz)
    assert float((cnt < 32).float().mean()) > 0.5 and float((cnt < 8).float().mean()) > 0.1
    for kw in (dict(cfeat=0, widths=[32, 32, 64]), dict(cfeat=16, widths=[64, 64, 128])):
        worst, base, errs = run_pool_case(mode, b=4, n=512, m=128, ns=32, idx=idx, xyz=xyz, new_xyz=new_xyz, **kw)
        assert worst <= max(TOL, 2.0 * base), errs


def _clone_pair(mod):
    ref = copy.deepcopy(mod)
    ref.fused_mlp = False
    return ref


def _compare_modules(sa, ref, xyz, f0, geometry=None):
    fa = f0.clone().requires_grad_(True) if f0 is not None else None
    fb = f0.clone().requires_grad_(True) if f0 is not None else None
    _, oa, ia = sa(xyz, fa, geometry) if geometry is not None else sa(xyz, fa)
    _, ob, ib = ref(xyz, fb)
    assert sa.last_path == "fused_train" and ref.last_path == "unfused"
    assert torch.equal(ia, ib)
    w = torch.randn_like(ob)
    (oa * w).sum().backward()
    (ob * w).sum().backward()
    scale = lambda t: max(1e-30, float(t.abs().max()))
    l2 = lambda a, b: float((a - b).norm() / b.norm())
    assert float((oa - ob).abs().max()) <= 2e-5 * scale(ob)
    if fa is not None:
        assert l2(fa.grad, fb.grad) <= 2e-3
    conv_biases = {id(mod.bias) for mod in sa.mlp.modules() if isinstance(mod, torch.nn.Conv2d)}
    # (mlp2 runs as torch modules on both sides: its conv biases under batch norm get rounding noise there, no gradient)
    post_biases = {id(mod.bias) for mod in (sa.mlp2.modules() if sa.mlp2 is not None else ()) if isinstance(mod, torch.nn.Conv2d)}
    for (na, pa), (nb, pb) in zip(sa.named_parameters(), ref.named_parameters()):
        if id(pa) in conv_biases:
            assert float(pa.grad.abs().max()) == 0.0           # exactly zero under batch norm (torch: rounding noise)
            continue
        if id(pa) in post_biases:
            continue
        assert l2(pa.grad, pb.grad) <= 2e-3, na
    for (na, ba), (nb, bb) in zip(sa.named_buffers(), ref.named_buffers()):
        assert float((ba.double() - bb.double()).abs().max()) <= 1e-5 * max(1.0, scale(bb.double())), na


LEVELS = {
    "plain": lambda pool: dict(args=(64, 128, 0.4, 32, [64, 64, 128]), kw=dict(pooling=pool)),
    "knn": lambda pool: dict(args=(16, 64, None, 32, [32, 32, 64]), kw=dict(pooling=pool, knn=True)),
    "group_all": lambda pool: dict(args=(64, None, None, None, [64, 64, 128]), kw=dict(pooling=pool, group_all=True)),
    "mlp2": lambda pool: dict(args=(16, 64, 0.4, 32, [32, 32, 64]), kw=dict(pooling=pool, mlp2=[64, 32])),
}


@pytest.mark.parametrize("level", list(LEVELS) + ["geometry_ahead"])
@pytest.mark.parametrize("mode", MODES)
def test_sa_module_takes_fused_train_and_matches_layer_by_layer(cuda, mode, level):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(0)
    spec = LEVELS["plain" if level == "geometry_ahead" else level](mode)
    sa = U.PointnetSAModule(*spec["args"], **spec["kw"]).to(cuda).train()
    ref = _clone_pair(sa)
    n = 128 if level == "group_all" else 512
    xyz = torch.rand(4, n, 3, device=cuda)
    f0 = torch.randn(4, n, spec["args"][0], device=cuda)
    geometry = None
    if level == "geometry_ahead":
        from pointnet2_amd.geometry import GeometryAhead
        geometry = GeometryAhead([sa]).compute(xyz).sa[0]
    _compare_modules(sa, ref, xyz, f0, geometry)


def test_pooling_zero_through_the_pool_entries_is_bit_identical(cuda, monkeypatch):
    """pn2_mlp_train_forward_pool / _backward_pool with pooling 0 against the _ex entries: every output bit, on a small level
    (z_L kept) and a large one (z-free top layer)."""
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import _C
    lib = _C.lib()
    for npoint, b in ((64, 4), (1024, 16)):
        torch.manual_seed(5)
        sa = U.PointnetSAModule(0, npoint, 0.3, 32, [64, 64, 128]).to(cuda).train()
        twin = copy.deepcopy(sa)
        xyz = torch.rand(b, 4 * npoint, 3, device=cuda)
        w = torch.randn(b, npoint, 128, device=cuda)
        results = []
        for mod, patched in ((sa, False), (twin, True)):
            with monkeypatch.context() as mp:
                if patched:
                    fwd, bwd = lib.pn2_mlp_train_forward_pool, lib.pn2_mlp_train_backward_pool
                    mp.setattr(lib, "pn2_mlp_train_forward_ex",
                               lambda rows, n, arr, grp, x, pr, out, argsel, zsel, ws, opts, st:
                               fwd(rows, n, arr, grp, pr, 0, out, argsel, zsel, None, ws, opts, st))
                    mp.setattr(lib, "pn2_mlp_train_backward_ex",
                               lambda rows, n, arr, grp, x, pr, out, argsel, zsel, gout, gx, grows, gpts, rep, ws, opts, st:
                               bwd(rows, n, arr, grp, pr, 0, out, argsel, zsel, None, gout, grows, gpts, rep, ws, opts, st))
                _, out, _ = mod(xyz, None)
                (out * w).sum().backward()
            assert mod.last_path == "fused_train"
            results.append([out.detach()] + [p.grad for p in mod.parameters()] + list(mod.buffers()))
        for a, c in zip(*results):
            assert torch.equal(a, c)


def test_max_half_of_max_and_avg_is_pooling_zero(cuda):
    from pointnet2_amd import train_mlp
    g = torch.Generator(device="cpu").manual_seed(9)
    for b, m in ((4, 64), (16, 1024)):
        torch.manual_seed(9)
        net = _net(3 + 16, [64, 64, 128], g, cuda)
        twin = copy.deepcopy(net)
        xyz = torch.rand((b, 4 * m, 3), generator=g).to(cuda)
        pts = torch.randn((b, 4 * m, 16), generator=g).to(cuda)
        new_xyz = xyz[:, :m].contiguous()
        idx = torch.randint(0, 4 * m, (b, m, 32), generator=g, dtype=torch.int32).to(cuda)
        with torch.no_grad():
            o0, a0 = train_mlp.sa_mlp_train(net.net, xyz, new_xyz, pts, idx, True)
            o3, a3 = train_mlp.sa_mlp_train(twin.net, xyz, new_xyz, pts, idx, True, pooling="max_and_avg")
        assert o3.shape[-1] == 2 * o0.shape[-1]
        assert torch.equal(o3[..., 128:], o0) and torch.equal(a3, a0)


@pytest.mark.parametrize("mode", MODES)
def test_reproducible_backward_is_bit_identical(cuda, mode):
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(4)
    sa = U.PointnetSAModule(32, 256, 0.3, 32, [64, 64, 128], pooling=mode).to(cuda).train()
    xyz = torch.rand(8, 1024, 3, device=cuda)
    feats = torch.randn(8, 1024, 32, device=cuda, requires_grad=True)
    old = P.is_deterministic()
    P.set_deterministic(True)
    try:
        _, out, _ = sa(xyz, feats)
        assert sa.last_path == "fused_train"
        w = torch.randn_like(out)
        params = list(sa.parameters()) + [feats]
        g1 = torch.autograd.grad((out * w).sum(), params, retain_graph=True)
        g2 = torch.autograd.grad((out * w).sum(), params)
    finally:
        P.set_deterministic(old)
    for a, c in zip(g1, g2):
        assert torch.equal(a, c)


def test_avg_and_weighted_levels_capture_in_one_graph(cuda):
    """forward + backward of an avg level and a weighted_avg level behind it in ONE HIP graph: each replay on new data is
    bit-identical to the eager evaluation of that data (two inputs in turn)."""
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(6)
    sa1 = U.PointnetSAModule(16, 128, 0.3, 32, [32, 32, 64], pooling="avg").to(cuda).train()
    sa2 = U.PointnetSAModule(64, 32, 0.5, 32, [64, 64, 128], pooling="weighted_avg").to(cuda).train()
    xyz = torch.rand(4, 512, 3, device=cuda)
    feats = torch.randn(4, 512, 16, device=cuda, requires_grad=True)
    w = torch.randn(4, 32, 128, device=cuda)
    params = list(sa1.parameters()) + list(sa2.parameters())

    def step():
        x1, f1, _ = sa1(xyz, feats)
        _, out, _ = sa2(x1, f1)
        return out, torch.autograd.grad((out * w).sum(), params + [feats])
    old = P.is_deterministic()
    P.set_deterministic(True)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out_g, grads_g = step()
        assert sa1.last_path == "fused_train" and sa2.last_path == "fused_train"
        inputs = [(torch.rand(4, 512, 3, device=cuda), torch.randn(4, 512, 16, device=cuda)) for _ in range(2)]
        for _ in range(2):
            for x_new, f_new in inputs:
                xyz.copy_(x_new)
                with torch.no_grad():
                    feats.copy_(f_new)
                graph.replay()
                torch.cuda.synchronize()
                out_e, grads_e = step()
                assert torch.equal(out_g, out_e)
                for a, c in zip(grads_g, grads_e):
                    assert torch.equal(a, c)
    finally:
        P.set_deterministic(old)


@pytest.mark.parametrize("mode", MODES)
def test_fallbacks_unchanged(cuda, mode):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(2)
    xyz = torch.rand(2, 256, 3, device=cuda)
    for sa, x in ((U.PointnetSAModule(0, 64, 0.3, 24, [32, 32, 64], pooling=mode), xyz),
                  (U.PointnetSAModule(0, 64, 0.3, 32, [32, 32, 64], pooling=mode, bn=False), xyz),
                  (U.PointnetSAModule(0, 64, 0.3, 32, [32, 32, 64], pooling=mode), xyz.clone().requires_grad_(True))):
        sa = sa.to(cuda).train()
        sa(x, None)
        assert sa.last_path == "unfused"
