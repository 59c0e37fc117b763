"""The coordinate gradients of the fused SA training node (train_mlp.sa_mlp_train(..., xyz_grad=True),
pn2_mlp_train_backward_xyz, csrc/train_mlp_xyz.hip): d / d xyz and d / d new_xyz through grouped_xyz - new_xyz
(utils/pointnet_util.py:44-46, :179-180).

Kernel level: the method of tests/test_train_pool_gpu.py::run_pool_case -- torch float64 autograd on the CPU over the
layer-by-layer graph, evaluated on the linear piece the kernels chose (their ReLU decisions, their pooled sample), with xyz and
new_xyz as float64 leaves; torch fp32 on the same graph is the yardstick. Bound: TOL = 1e-5 of each tensor's max-abs scale.
Module level: the same module's layer-by-layer path on the same weights is the referee."""
import copy

import pytest
import torch

from test_train_pool_gpu import _net, _rel, _saved

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _pool64(h, mode, sel):
    """(groups, ns, C) -> pooled; the max on the kernels' sample `sel` (groups, C) when given."""
    if mode == "avg":
        return h.mean(dim=1)
    top = h.max(dim=1)[0] if sel is None else h.gather(1, sel.long().unsqueeze(1)).squeeze(1)
    return top if mode == "max" else torch.cat([h.mean(dim=1), top], dim=-1)


def _ref(rows, params, eps, ns, mode, masks=None, sel=None):
    h, flips, margin = rows, 0, 0.0
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
    c = h.shape[1]
    out = _pool64(h.view(-1, ns, c), mode, sel)
    gap = 0.0
    if sel is not None:                     # the kernels' sample must attain the maximum
        top = torch.relu(h.detach()).view(-1, ns, c).max(dim=1)[0]
        gap = float((top - out.detach()[:, -c:]).abs().max() / max(1e-30, float(top.abs().max())))
    return out, flips, margin, gap


def _rows(x, nx, p, idx, b, xyz_first):
    """The grouped (rows, 3 + cfeat) input from the leaves x (b,n,3), nx (b,m,3) or None (group_all), p (b,n,c) or None."""
    if idx is None:
        gx, gp = x.unsqueeze(1), (p.unsqueeze(1) if p is not None else None)
    else:
        li, bi = idx.long().cpu(), torch.arange(b).view(b, 1, 1)
        gx = x[bi, li] - nx.unsqueeze(2)
        gp = p[bi, li] if p is not None else None
    parts = [gx, gp] if xyz_first else [gp, gx]
    full = torch.cat([t for t in parts if t is not None], dim=-1)
    return full.reshape(-1, full.shape[-1])


def run_xyz_case(mode, b, n, m, ns, cfeat, widths, xyz_first=True, group_all=False, seed=0, idx=None, points_grad=True, opts=None,
                 centroid_scale=None):
    """-> the kernels' worst relative error, torch fp32's own on the same graph, the errors by name, grad_xyz, grad_new_xyz."""
    from pointnet2_amd import train_mlp
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(seed)
    torch.manual_seed(seed)
    cin = 3 + cfeat
    net = _net(cin, widths, g, dev)
    pairs = train_mlp.conv_bn_pairs(net.net)
    xyz = torch.rand((b, n, 3), generator=g).to(dev).requires_grad_(True)
    points = torch.randn((b, n, cfeat), generator=g).to(dev).requires_grad_(points_grad) if cfeat else None
    new_xyz = None
    if group_all:
        mm, nss, idx = 1, n, None
    else:
        sel = torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(b)]).to(dev)
        new_xyz = torch.gather(xyz.detach(), 1, sel.unsqueeze(-1).expand(-1, -1, 3)).contiguous().requires_grad_(True)
        if idx is None:
            idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32)
            idx[:, :, ns // 2:] = idx[:, :, :1]                 # padded groups, like the ball query's
        idx = idx.to(dev)
        mm, nss = m, ns
    # (top_stored: the pooled top layer's z_L is kept, so that its ReLU decisions can be read back like the other layers')
    with train_mlp.options(top_stored=True, **(opts or {})):
        out, argsel = train_mlp.sa_mlp_train(net.net, xyz, new_xyz, points, idx, xyz_first, pooling=mode, xyz_grad=True)
        nl = len(pairs)
        zs, saves, _ = _saved(out, nl, points is not None)
        masks = [((z * s[2]) + s[3] > 0).cpu() for z, s in zip(zs, saves)]     # two roundings, as the kernels' fmul + fadd
        x64 = xyz.detach().double().cpu().requires_grad_(True)
        nx64 = new_xyz.detach().double().cpu().requires_grad_(True) if new_xyz is not None else None
        p64 = points.detach().double().cpu().requires_grad_(points_grad) if cfeat else None
        rows64 = _rows(x64, nx64, p64, idx, b, xyz_first)
        params64 = [tuple(t.detach().double().cpu().requires_grad_(True) for t in
                          (conv.weight.view(conv.out_channels, -1), conv.bias, bn.weight, bn.bias)) for conv, bn in pairs]
        eps = [bn.eps for _, bn in pairs]
        sel = argsel.reshape(b * mm, -1).cpu() if argsel is not None else None
        want, flips, margin, gap = _ref(rows64, params64, eps, nss, mode, masks, sel)
        gw = torch.randn(want.shape, generator=g, dtype=torch.float64)
        (want * gw).sum().backward()
        (out.reshape(want.shape) * gw.float().to(dev)).sum().backward()
        torch.cuda.synchronize()
    errs = {"out": _rel(out.reshape(want.shape), want), "pool_gap": gap, "dxyz": _rel(xyz.grad, x64.grad)}
    if new_xyz is not None and centroid_scale == "xyz":
        # ONE centroid in the whole batch: moving it shifts every row of z_1 by the same vector, which the batch statistics
        # remove -- the true gradient is zero, and the tensor has no scale of its own: grad_xyz's is used
        errs["dnew_xyz"] = float((new_xyz.grad.double().cpu() - nx64.grad).abs().max() / float(x64.grad.abs().max()))
    elif new_xyz is not None:
        errs["dnew_xyz"] = _rel(new_xyz.grad, nx64.grad)
    for l, ((conv, bn), p) in enumerate(zip(pairs, params64)):
        errs["dW%d" % (l + 1)] = _rel(conv.weight.grad.view(conv.out_channels, -1), p[0].grad)
        errs["dg%d" % (l + 1)] = _rel(bn.weight.grad, p[2].grad)
        errs["dbe%d" % (l + 1)] = _rel(bn.bias.grad, p[3].grad)
        assert float(conv.bias.grad.abs().max()) == 0.0
    if cfeat and points_grad:
        errs["dpts"] = _rel(points.grad, p64.grad)
    # the yardstick: torch fp32 on the same graph -- the same linear piece: the pinned ReLU decisions and pooled sample (with its own
    # decisions one flipped unit is an error of 1e-2, which says nothing about fp32) -- against the same float64 results
    x32 = x64.detach().float().requires_grad_(True)
    nx32 = nx64.detach().float().requires_grad_(True) if nx64 is not None else None
    q32 = p64.detach().float().requires_grad_(points_grad) if cfeat else None
    p32 = [tuple(t.detach().float().requires_grad_(True) for t in p) for p in params64]
    got32, _, _, _ = _ref(_rows(x32, nx32, q32, idx, b, xyz_first), p32, eps, nss, mode, masks, sel)
    (got32 * gw.float()).sum().backward()
    base = {"out": _rel(got32, want), "dxyz": _rel(x32.grad, x64.grad)}
    if nx32 is not None and centroid_scale == "xyz":
        base["dnew_xyz"] = float((nx32.grad.double() - nx64.grad).abs().max() / float(x64.grad.abs().max()))
    elif nx32 is not None:
        base["dnew_xyz"] = _rel(nx32.grad, nx64.grad)
    for l, (a32, a64) in enumerate(zip(p32, params64)):
        base["dW%d" % (l + 1)] = _rel(a32[0].grad, a64[0].grad)
        base["dg%d" % (l + 1)] = _rel(a32[2].grad, a64[2].grad)
        base["dbe%d" % (l + 1)] = _rel(a32[3].grad, a64[3].grad)
    if cfeat and points_grad:
        base["dpts"] = _rel(q32.grad, p64.grad)
    worst = max(errs.values())
    print("%-11s worst %.2e (torch fp32 %.2e) flips %d margin %.1e  " % (mode, worst, max(base.values()), flips, margin) +
          " ".join("%s=%.1e" % kv for kv in errs.items()), flush=True)
    assert flips <= max(2, 1e-5 * sum(k.numel() for k in masks)) and margin <= 1e-5, (flips, margin)
    return worst, max(base.values()), errs, xyz.grad.detach(), (new_xyz.grad.detach() if new_xyz is not None else None)


# The SA levels of reference_configs at a reduced batch, each layer-1 organisation forced (train_mlp.options), so that no
# branch is reached only by a size rule: (name, shape, options, points take a gradient)
COORDS = dict(l1_coords=True)
GATHER = dict(l1_coords=False, l1_per_point=False)
PER_POINT = dict(l1_coords=False, l1_per_point=True)
LEVEL_CASES = [
    ("cls_ssg SA1 coords-only", dict(b=4, n=1024, m=512, ns=32, cfeat=0, widths=[64, 64, 128]), COORDS, True),
    ("cls_ssg SA1 gathered", dict(b=4, n=1024, m=512, ns=32, cfeat=0, widths=[64, 64, 128]), GATHER, True),
    ("sem_seg SA1 coords-only", dict(b=2, n=8192, m=1024, ns=32, cfeat=0, widths=[32, 32, 64]), COORDS, True),
    ("part_seg SA1 normals cf<=5", dict(b=2, n=2048, m=512, ns=64, cfeat=3, widths=[64, 64, 128]), COORDS, False),
    ("cls_msg SA1 s1 normals msg order ns16", dict(b=4, n=4096, m=512, ns=16, cfeat=3, widths=[32, 32, 64], xyz_first=False), COORDS, False),
    ("cls_msg SA1 s3 normals msg order ns128", dict(b=2, n=4096, m=512, ns=128, cfeat=3, widths=[64, 96, 128], xyz_first=False), COORDS, False),
    ("cls_msg SA1 s2 gathered msg order", dict(b=2, n=4096, m=512, ns=32, cfeat=3, widths=[64, 64, 128], xyz_first=False), GATHER, True),
    ("cls_ssg SA2 per-point ns64", dict(b=4, n=512, m=128, ns=64, cfeat=128, widths=[128, 128, 256]), PER_POINT, True),
    ("cls_ssg SA2 gathered ns64", dict(b=4, n=512, m=128, ns=64, cfeat=128, widths=[128, 128, 256]), GATHER, True),
    ("sem_seg SA2 per-point", dict(b=8, n=1024, m=256, ns=32, cfeat=64, widths=[64, 64, 128]), PER_POINT, True),
    ("cls_msg SA2 s1 per-point msg order c320", dict(b=2, n=512, m=128, ns=32, cfeat=320, widths=[64, 64, 128], xyz_first=False), PER_POINT, True),
    ("cls_msg SA2 s3 gathered msg order ns128", dict(b=2, n=512, m=128, ns=128, cfeat=320, widths=[128, 128, 256], xyz_first=False), GATHER, True),
    ("sem_seg SA4 per-point", dict(b=8, n=64, m=16, ns=32, cfeat=256, widths=[256, 256, 512]), PER_POINT, True),
    ("cls_ssg SA3 group_all", dict(b=4, n=128, m=1, ns=128, cfeat=256, widths=[256, 512, 1024], group_all=True), {}, True),
]
POOL_CASES = [c for c in LEVEL_CASES if c[0] in ("cls_ssg SA1 coords-only", "cls_msg SA1 s1 normals msg order ns16", "cls_ssg SA2 per-point ns64",
                                                  "cls_ssg SA2 gathered ns64", "cls_ssg SA3 group_all")]


def _check(name, mode, worst, base, errs):
    """The bound is TOL alone. The yardstick (torch fp32 on the CPU, same linear piece) is printed beside, not asserted: it is
    inside TOL on the small shapes and at 1.0e-5 .. 2.2e-5 on the levels of 65k rows and more, whatever the seed -- its column
    sums run in fp32 where the kernels keep fp64 partial sums (measured: kernels 1.0e-6 .. 5.9e-6 on every case)."""
    assert worst <= TOL, "%s %s: worst %.2e (torch fp32 %.2e): %s" % (name, mode, worst, base, errs)


@pytest.mark.parametrize("name,kw,opts,pg", LEVEL_CASES, ids=[c[0] for c in LEVEL_CASES])
def test_coordinate_gradients_match_float64(cuda, name, kw, opts, pg):
    worst, base, errs, _, _ = run_xyz_case("max", points_grad=pg, opts=opts, **kw)
    _check(name, "max", worst, base, errs)


@pytest.mark.parametrize("mode", ["avg", "max_and_avg"])
@pytest.mark.parametrize("name,kw,opts,pg", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_coordinate_gradients_match_float64_pooled(cuda, name, kw, opts, pg, mode):
    worst, base, errs, _, _ = run_xyz_case(mode, points_grad=pg, opts=opts, **kw)
    _check(name, mode, worst, base, errs)


def test_organisations_are_the_ones_named(cuda):
    """The options above select what their names say (the library's own queries)."""
    import ctypes
    from pointnet2_amd import _C, train_mlp
    lib = _C.lib()
    for name, kw, opts, _ in LEVEL_CASES:
        widths = [3 + kw["cfeat"]] + kw["widths"]
        arr = (ctypes.c_int * len(widths))(*widths)
        gd = (ctypes.c_int * 6)(kw["b"], kw["n"], kw["m"], kw["ns"], kw["cfeat"], 0 if kw.get("group_all") else 1)
        with train_mlp.options(**opts):
            per_point = bool(lib.pn2_mlp_train_layer1_per_point_ex(len(widths) - 1, arr, gd, train_mlp._opts()))
        assert per_point == ("per-point" in name), name


# ---- index edge cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3, 4])
@pytest.mark.parametrize("org", ["coords", "gathered", "per_point"])
def test_index_edge_cases(cuda, b, org):
    """Padded groups (half a group repeating its first hit), points no group names (an exactly zero row), one point named more
    than 1,024 times in a cloud; b = 1 and 3 take the segmented reduction's inversion without LDS, b = 4 the one with."""
    n, m, ns = 1024, 128, 32
    g = torch.Generator(device="cpu").manual_seed(100 + b)
    idx = torch.randint(0, n // 2, (b, m, ns), generator=g, dtype=torch.int32)         # the upper half: never named
    idx[:, :, 0] = 7                                                                   # every group's first hit ...
    idx[:, :, ns // 2:] = idx[:, :, :1]                                                # ... and its padding: 128 * 17 = 2,176 references
    assert int((idx[0] == 7).sum()) > 1024
    kw = dict(coords=dict(cfeat=0, widths=[32, 32, 64], opts=COORDS), gathered=dict(cfeat=16, widths=[32, 32, 64], opts=GATHER),
              per_point=dict(cfeat=16, widths=[32, 32, 64], opts=PER_POINT))[org]
    worst, base, errs, gx, gn = run_xyz_case("max", b=b, n=n, m=m, ns=ns, idx=idx, seed=b, **kw)
    _check("edge b=%d %s" % (b, org), "max", worst, base, errs)
    assert float(gx[:, n // 2:].abs().max()) == 0.0                                    # exactly zero, not rounding noise
    assert float(gx[:, 7].abs().min()) > 0.0


@pytest.mark.parametrize("b", [1, 3])
def test_single_group_per_cloud(cuda, b):
    cs = "xyz" if b == 1 else None
    worst, base, errs, gx, gn = run_xyz_case("max", b=b, n=64, m=1, ns=32, cfeat=0, widths=[32, 32, 64], seed=b, centroid_scale=cs)
    _check("m=1 b=%d" % b, "max", worst, base, errs)
    worst, base, errs, gx, gn = run_xyz_case("avg", b=b, n=64, m=1, ns=32, cfeat=16, widths=[32, 32, 64], seed=b, opts=PER_POINT,
                                             centroid_scale=cs)
    _check("m=1 b=%d per-point" % b, "avg", worst, base, errs)


# ---- the sum rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,opts,pg", LEVEL_CASES[:1] + LEVEL_CASES[3:5] + LEVEL_CASES[7:9], ids=[c[0] for c in LEVEL_CASES[:1] + LEVEL_CASES[3:5] + LEVEL_CASES[7:9]])
@pytest.mark.parametrize("mode", ["max", "avg", "max_and_avg"])
def test_translation_sum_rule(cuda, name, kw, opts, pg, mode):
    """With idx fixed, translating every point and centroid of a cloud by one vector leaves every u_r unchanged:
    sum_p grad_xyz[i,p] + sum_j grad_new_xyz[i,j] = 0 per cloud, as the node returns them (before gather_point's backward)."""
    _, _, _, gx, gn = run_xyz_case(mode, points_grad=pg, opts=opts, **kw)
    total = gx.double().sum(dim=1) + gn.double().sum(dim=1)                            # (b, 3)
    scale = float(gx.abs().max())
    print("sum rule: |total| max %.3e, scale %.3e, ratio %.2e" % (float(total.abs().max()), scale, float(total.abs().max()) / scale))
    assert float(total.abs().max()) <= TOL * scale


# ---- nothing else moved -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["max", "avg", "max_and_avg"])
@pytest.mark.parametrize("org", ["coords", "gathered", "per_point"])
def test_everything_else_is_unchanged(cuda, org, mode):
    """out, argsel and the running statistics of a call with xyz_grad=True are the bits of the same call without; the parameter and
    points gradients agree within TOL -- bit for bit where the organisation is the same (a level without features replaces the
    moment form of layer 1's weight gradient by the pass over dy_1)."""
    import pointnet2_amd as P
    from pointnet2_amd import train_mlp
    cfeat, opts = dict(coords=(0, COORDS), gathered=(16, GATHER), per_point=(16, PER_POINT))[org]
    g = torch.Generator(device="cpu").manual_seed(21)
    torch.manual_seed(21)
    b, n, m, ns = 4, 512, 128, 32
    net = _net(3 + cfeat, [64, 64, 128], g, cuda)
    twin = copy.deepcopy(net)
    xyz = torch.rand((b, n, 3), generator=g).to(cuda)
    pts = torch.randn((b, n, cfeat), generator=g).to(cuda) if cfeat else None
    new_xyz = xyz[:, :m].contiguous()
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32).to(cuda)
    gw = None
    res = []
    old = P.is_deterministic()
    P.set_deterministic(True)
    try:
        for mod, flag in ((net, False), (twin, True)):
            x = xyz.clone().requires_grad_(flag)
            nx = new_xyz.clone().requires_grad_(flag)
            p = pts.clone().requires_grad_(True) if cfeat else None
            with train_mlp.options(**opts):
                out, argsel = train_mlp.sa_mlp_train(mod.net, x, nx, p, idx, True, pooling=mode, xyz_grad=flag)
                gw = torch.randn(out.shape, generator=g).to(cuda) if gw is None else gw
                (out * gw).sum().backward()
            assert (x.grad is not None) == flag and (nx.grad is not None) == flag
            res.append(([out.detach(), argsel] + list(mod.buffers()), [q.grad for q in mod.parameters()] + ([p.grad] if cfeat else [])))
    finally:
        P.set_deterministic(old)
    for a, c in zip(res[0][0], res[1][0]):
        assert (a is None and c is None) or torch.equal(a, c)
    for a, c in zip(res[0][1], res[1][1]):
        if org == "coords":
            assert float((a - c).abs().max()) <= TOL * max(1e-30, float(a.abs().max()))
        else:
            assert torch.equal(a, c)


def test_default_returns_no_coordinate_gradient(cuda):
    from pointnet2_amd import train_mlp
    g = torch.Generator(device="cpu").manual_seed(2)
    net = _net(3, [32, 32, 64], g, cuda)
    xyz = torch.rand((2, 256, 3), generator=g).to(cuda).requires_grad_(True)
    idx = torch.randint(0, 256, (2, 64, 32), generator=g, dtype=torch.int32).to(cuda)
    out, _ = train_mlp.sa_mlp_train(net.net, xyz, xyz[:, :64].detach().contiguous(), None, idx)
    out.sum().backward()
    assert xyz.grad is None
    with pytest.raises(ValueError):
        train_mlp.sa_mlp_train(net.net, xyz, xyz[:, :64].contiguous(), None, idx, pooling="weighted_avg", xyz_grad=True)


# ---- modules --------------------------------------------------------------------------------------------------------------------
def _module_pair(sa):
    sa.fused_xyz_grad = True
    ref = copy.deepcopy(sa)
    ref.fused_mlp = False
    return sa, ref


def _compare_xyz_grad(sa, ref, xyz0, f0, geometry=None):
    grads = []
    w = None
    for mod, geo in ((sa, geometry), (ref, None)):
        xyz = xyz0.clone().requires_grad_(True)
        f = f0.clone().requires_grad_(True) if f0 is not None else None
        res = mod(xyz, f, geo) if geo is not None else mod(xyz, f)
        new_xyz, out = res[0], res[1]
        w = torch.randn_like(out) if w is None else w
        wx = torch.linspace(-1.0, 1.0, new_xyz.numel(), device=new_xyz.device).view(new_xyz.shape)
        ((out * w).sum() + (new_xyz * wx).sum()).backward()       # new_xyz is an output too: GatherPoint's gradient
        grads.append((xyz.grad, out.detach()))
    assert sa.last_path == "fused_train" and ref.last_path == "unfused"
    (ga, oa), (gb, ob) = grads
    scale = float(gb.abs().max())
    err = float((ga - gb).abs().max()) / scale
    print("xyz.grad: fused node vs layer-by-layer %.2e of scale" % err, flush=True)
    assert float((oa - ob).abs().max()) <= 2e-5 * float(ob.abs().max())
    assert err <= 1e-5


SA_LEVELS = {
    "plain": dict(args=(16, 64, 0.4, 32, [32, 32, 64]), kw=dict()),
    "no features": dict(args=(0, 64, 0.4, 32, [32, 32, 64]), kw=dict()),
    "knn": dict(args=(16, 64, None, 32, [32, 32, 64]), kw=dict(knn=True)),
    "group_all": dict(args=(16, None, None, None, [32, 32, 64]), kw=dict(group_all=True)),
    "mlp2": dict(args=(16, 64, 0.4, 32, [32, 32, 64]), kw=dict(mlp2=[64, 32])),
    "avg": dict(args=(16, 64, 0.4, 32, [32, 32, 64]), kw=dict(pooling="avg")),
    "max_and_avg": dict(args=(16, 64, 0.4, 32, [32, 32, 64]), kw=dict(pooling="max_and_avg")),
}


@pytest.mark.parametrize("level", list(SA_LEVELS) + ["geometry_ahead"])
def test_sa_module_takes_the_node_and_matches_layer_by_layer(cuda, level):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(0)
    spec = SA_LEVELS["plain" if level == "geometry_ahead" else level]
    sa, ref = _module_pair(U.PointnetSAModule(*spec["args"], **spec["kw"]).to(cuda).train())
    n = 128 if level == "group_all" else 256
    xyz = torch.rand(2, n, 3, device=cuda)
    f0 = torch.randn(2, n, spec["args"][0], device=cuda) if spec["args"][0] else None
    geometry = None
    if level == "geometry_ahead":
        from pointnet2_amd.geometry import GeometryAhead
        geometry = GeometryAhead([sa]).compute(xyz).sa[0]
    _compare_xyz_grad(sa, ref, xyz, f0, geometry)


@pytest.mark.parametrize("ahead", [False, True])
def test_msg_module_takes_the_node_and_matches_layer_by_layer(cuda, ahead):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(1)
    msg, ref = _module_pair(U.PointnetSAModuleMSG(3, 64, [0.2, 0.4, 0.6], [16, 32, 64], [[32, 32, 64], [32, 48, 64], [32, 32, 64]]).to(cuda).train())
    xyz = torch.rand(2, 256, 3, device=cuda)
    nrm = torch.randn(2, 256, 3, device=cuda)
    geometry = None
    if ahead:
        from pointnet2_amd.geometry import GeometryAhead
        geometry = GeometryAhead([msg]).compute(xyz).sa[0]
    _compare_xyz_grad(msg, ref, xyz, nrm, geometry)


def test_default_and_weighted_avg_keep_the_layer_by_layer_path(cuda):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(2)
    xyz = torch.rand(2, 256, 3, device=cuda).requires_grad_(True)
    sa = U.PointnetSAModule(0, 64, 0.3, 32, [32, 32, 64]).to(cuda).train()
    assert sa.fused_xyz_grad is False
    sa(xyz, None)
    assert sa.last_path == "unfused"
    msg = U.PointnetSAModuleMSG(0, 64, [0.2, 0.4], [16, 32], [[32, 32, 64], [32, 48, 64]]).to(cuda).train()
    msg(xyz, None)
    assert msg.last_path == "unfused"
    wa = U.PointnetSAModule(0, 64, 0.3, 32, [32, 32, 64], pooling="weighted_avg").to(cuda).train()
    wa.fused_xyz_grad = True
    wa(xyz, None)
    assert wa.last_path == "unfused"
    nobn = U.PointnetSAModule(0, 64, 0.3, 32, [32, 32, 64], bn=False).to(cuda).train()
    nobn.fused_xyz_grad = True
    nobn(xyz, None)
    assert nobn.last_path == "unfused"
    ev = U.PointnetSAModule(0, 64, 0.3, 32, [32, 32, 64]).to(cuda).eval()
    ev.fused_xyz_grad = True
    ev(xyz, None)
    assert ev.last_path == "unfused"
    on = U.PointnetSAModule(0, 64, 0.3, 32, [32, 32, 64]).to(cuda).train()
    on.fused_xyz_grad = True
    on(xyz.detach(), None)                                      # no gradient wanted: the node as before
    assert on.last_path == "fused_train"
    on(xyz, None)
    assert on.last_path == "fused_train"


# ---- reproducible mode, graph capture, accumulation ---------------------------------------------------------------------
@pytest.mark.parametrize("cfeat,b", [(0, 8), (32, 8), (32, 2)])
def test_reproducible_backward_is_bit_identical(cuda, cfeat, b):
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(4)
    sa = U.PointnetSAModule(cfeat, 256, 0.3, 32, [64, 64, 128]).to(cuda).train()
    sa.fused_xyz_grad = True
    xyz = torch.rand(b, 1024, 3, device=cuda, requires_grad=True)
    feats = torch.randn(b, 1024, cfeat, device=cuda, requires_grad=True) if cfeat else None
    old = P.is_deterministic()
    P.set_deterministic(True)
    try:
        new_xyz, out, _ = sa(xyz, feats)
        assert sa.last_path == "fused_train"
        w = torch.randn_like(out)
        # the node's own two coordinate gradients: xyz through the rows only (new_xyz held as a leaf of this graph) and new_xyz
        wanted = [xyz, new_xyz] + list(sa.parameters())
        g1 = torch.autograd.grad((out * w).sum(), wanted, retain_graph=True)
        g2 = torch.autograd.grad((out * w).sum(), wanted)
    finally:
        P.set_deterministic(old)
    for a, c in zip(g1, g2):
        assert torch.equal(a, c)
    assert float(g1[0].abs().max()) > 0 and float(g1[1].abs().max()) > 0


@pytest.mark.parametrize("mode", ["max", "avg", "max_and_avg"])
def test_forward_and_backward_capture_in_one_graph(cuda, mode):
    """A captured forward + backward replayed on new input values equals the eager run bit for bit."""
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(6)
    sa1 = U.PointnetSAModule(16, 128, 0.3, 32, [32, 32, 64], pooling=mode).to(cuda).train()
    sa2 = U.PointnetSAModule(sa1.mlp.c_out * (2 if mode == "max_and_avg" else 1), 32, 0.5, 32, [64, 64, 128], pooling=mode).to(cuda).train()
    sa1.fused_xyz_grad = sa2.fused_xyz_grad = True
    xyz = torch.rand(4, 512, 3, device=cuda, requires_grad=True)
    feats = torch.randn(4, 512, 16, device=cuda, requires_grad=True)
    params = list(sa1.parameters()) + list(sa2.parameters())
    w = None

    def step():
        x1, f1, _ = sa1(xyz, feats)
        _, out, _ = sa2(x1, f1)
        return out, torch.autograd.grad((out * w).sum(), params + [feats, xyz])
    with torch.no_grad():
        w = torch.randn(4, 32, sa2.mlp.c_out * (2 if mode == "max_and_avg" else 1), device=cuda)
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
                with torch.no_grad():
                    xyz.copy_(x_new)
                    feats.copy_(f_new)
                graph.replay()
                torch.cuda.synchronize()
                out_e, grads_e = step()
                assert torch.equal(out_g, out_e)
                for a, c in zip(grads_g, grads_e):
                    assert torch.equal(a, c)
                assert float(grads_e[-1].abs().max()) > 0
    finally:
        P.set_deterministic(old)


def test_accumulation_into_grad_keeps_the_coordinate_gradient(cuda):
    """train_mlp.accumulate_into_grad: the parameter gradients land in .grad (added by the kernels), grad_xyz is returned to
    autograd, which accumulates it into xyz.grad."""
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    torch.manual_seed(3)
    sa = U.PointnetSAModule(64, 128, 0.4, 32, [64, 64, 128]).to(cuda).train()
    sa.fused_xyz_grad = True
    ref = copy.deepcopy(sa)
    xyz0 = torch.rand(4, 512, 3, device=cuda)
    feats = torch.randn(4, 512, 64, device=cuda)
    gw = torch.randn(4, 128, 128, device=cuda)
    old = P.is_deterministic()
    P.set_deterministic(True)
    try:
        xa = xyz0.clone().requires_grad_(True)
        for p in sa.parameters():
            p.grad = torch.zeros_like(p)
        slots = [p.grad.data_ptr() for p in sa.parameters()]
        with train_mlp.accumulate_into_grad():
            for _ in range(2):                                  # two micro-batches
                (sa(xa, feats)[1] * gw).sum().backward()
        assert sa.last_path == "fused_train"
        assert [p.grad.data_ptr() for p in sa.parameters()] == slots, "the .grad tensors were replaced"
        xb = xyz0.clone().requires_grad_(True)
        for _ in range(2):
            (ref(xb, feats)[1] * gw).sum().backward()
        assert ref.last_path == "fused_train"
    finally:
        P.set_deterministic(old)
    assert torch.equal(xa.grad, xb.grad) and float(xa.grad.abs().max()) > 0
    for (name, p), q in zip(sa.named_parameters(), ref.parameters()):
        scale = float(q.grad.abs().max())
        assert float((p.grad - q.grad).abs().max()) <= 1e-6 * max(scale, 1e-30), name
