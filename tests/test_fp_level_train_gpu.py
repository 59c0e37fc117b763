"""The FP-level training node (train_mlp.fp_level_train, pn2_mlp_train_*_fp, csrc/train_mlp_fp.hip): weights, interpolation,
concatenation and the layer stack of pointnet_fp_module (utils/pointnet_util.py:211-226) as ONE autograd node with layer 1 once
per known point. Against a float64 evaluation of :211-226 (interpolation and concat in float64, the stack through
oracle/train_stack, the scatter by index_add_), against the current path (fp_interp_concat + fp_mlp_train), and the node's
contracts: reproducible bits, accumulation into .grad, organisation overrides, graph capture, module routing and memory."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5
# name, b, n, m, c2, c1, widths: the seven FP levels of reference_configs.FP_LEVELS with their widths and skip channels, then
# the edge shapes
CASES = [
    ("part_seg FP1", 16, 128, 1, 1024, 256, [256, 256]),
    ("part_seg FP2", 16, 512, 128, 256, 128, [256, 128]),
    ("part_seg FP3", 16, 2048, 512, 128, 6, [128, 128, 128]),
    ("sem_seg FP1", 8, 64, 16, 512, 256, [256, 256]),
    ("sem_seg FP2", 8, 256, 64, 256, 128, [256, 256]),
    ("sem_seg FP3", 8, 1024, 256, 256, 64, [256, 128]),
    ("sem_seg FP4", 8, 8192, 1024, 128, 0, [128, 128, 128]),
    ("m = 1", 3, 64, 1, 32, 16, [64, 32]),
    ("m = 2", 3, 64, 2, 32, 16, [64, 32]),
    ("c1 = 0", 4, 256, 40, 64, 0, [64, 64]),
    ("c1 = 6", 4, 256, 40, 64, 6, [64, 64]),
    ("c2 = 29", 4, 256, 40, 29, 5, [32, 64]),
    ("one layer", 4, 256, 40, 64, 6, [64]),                      # layer 1 is the top layer
]


def _net(cin, widths, g, dev):
    import pointnet2_amd.pointnet_util as U
    net = U._SharedMLP(cin, widths, bn=True).to(dev).train()
    with torch.no_grad():
        for mod in net.net:
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) * 1.5 - 0.4)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.3)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    return net


def _inputs(b, n, m, c2, c1, g, dev):
    from pointnet2_amd.tf_interpolate import three_nn
    xyz1 = torch.rand((b, n, 3), generator=g).to(dev)
    xyz2 = xyz1[:, :m].contiguous() if m > 2 else torch.rand((b, m, 3), generator=g).to(dev)
    p2 = torch.randn((b, m, c2), generator=g).to(dev)
    p1 = torch.randn((b, n, c1), generator=g).to(dev) if c1 else None
    dist, idx = three_nn(xyz1, xyz2)
    return p2, p1, idx, dist


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def _float64(net, p2, p1, idx, dist, gout):
    """:211-226 in float64: weights, interpolation, concat, the stack (oracle/train_stack), the scatter onto points2."""
    from oracle import train_stack
    b, m, c2 = p2.shape
    n = idx.shape[1]
    d = dist.double().cpu().numpy()
    inv = 1.0 / np.maximum(d, 1e-10)
    w = inv / inv.sum(axis=2, keepdims=True)
    ii = idx.long().cpu().numpy()
    P2 = p2.double().cpu().numpy()
    rows = (P2[np.arange(b)[:, None, None], ii] * w[..., None]).sum(axis=2)               # (b, n, c2)
    if p1 is not None:
        rows = np.concatenate([rows, p1.double().cpu().numpy()], axis=2)
    layers = []
    for mod_c, mod_b in zip(net[0::3], net[1::3]):
        layers.append({"W": mod_c.weight.detach().double().cpu().numpy()[:, :, 0, 0].T, "b": mod_c.bias.detach().double().cpu().numpy(),
                       "gamma": mod_b.weight.detach().double().cpu().numpy(), "beta": mod_b.bias.detach().double().cpu().numpy(),
                       "running_mean": mod_b.running_mean.double().cpu().numpy(),
                       "running_var": mod_b.running_var.double().cpu().numpy()})
    out, cache = train_stack.forward(rows.reshape(b * n, -1), layers, 0, momentum=net[1].momentum, eps=net[1].eps)
    dh, grads = train_stack.backward(gout.double().cpu().numpy().reshape(b * n, -1), layers, cache)
    dh = torch.from_numpy(dh)
    g2 = torch.zeros((b * m, c2), dtype=torch.float64)
    tgt = (torch.arange(b)[:, None, None] * m + torch.from_numpy(ii)).reshape(-1)
    g2.index_add_(0, tgt, (dh[:, :c2].reshape(b, n, 1, c2) * torch.from_numpy(w)[..., None]).reshape(-1, c2))
    g1 = dh[:, c2:].numpy().reshape(b, n, -1) if p1 is not None else None
    return out, cache, grads, g2.numpy().reshape(b, m, c2), g1


def _masked64(net, p2, p1, idx, dist, gout, zs, saves):
    """The gradients of :211-226 in float64 on the kernels' OWN linear piece (tests/test_train_mlp_gpu.py): a ReLU whose argument
    is within fp32 rounding of zero is decided by rounding, so the float64 graph takes the kernels' decisions -- relu(a z + c)
    > 0 from the saved z_l and (a, c) -- and the decisions that differ from float64's are bounded on their own.
    -> gradients of points2, points1, every (W, gamma, beta); flips; their largest |y| relative to the layer's scale."""
    b, m, c2 = p2.shape
    d = dist.double().cpu()
    inv = 1.0 / torch.clamp(d, min=1e-10)
    w = inv / inv.sum(dim=2, keepdim=True)
    a2 = p2.double().cpu().requires_grad_(True)
    a1 = p1.double().cpu().requires_grad_(True) if p1 is not None else None
    ii = idx.long().cpu()
    x = (a2[torch.arange(b)[:, None, None], ii] * w[..., None]).sum(dim=2)
    h = (torch.cat([x, a1], dim=2) if a1 is not None else x).reshape(-1, x.shape[2] + (a1.shape[2] if a1 is not None else 0))
    params, flips, margin = [], 0, 0.0
    for l, (conv, bn) in enumerate(zip(net[0::3], net[1::3])):
        W = conv.weight.detach().double().cpu()[:, :, 0, 0].requires_grad_(True)
        gam = bn.weight.detach().double().cpu().requires_grad_(True)
        bet = bn.bias.detach().double().cpu().requires_grad_(True)
        params += [W, gam, bet]
        z = h @ W.t() + conv.bias.detach().double().cpu()
        mean, var = z.mean(0), z.var(0, unbiased=False)
        y = (z - mean) / torch.sqrt(var + bn.eps) * gam + bet
        mask = (saves[l][2] * zs[l] + saves[l][3]).cpu() > 0
        dis = (y.detach() > 0) != mask
        flips += int(dis.sum())
        if dis.any():
            margin = max(margin, float(y.detach()[dis].abs().max() / y.detach().abs().max()))
        h = y * mask.double()
    grads = torch.autograd.grad(h, [a2] + ([a1] if a1 is not None else []) + params, gout.double().cpu().reshape(h.shape))
    return grads, flips, margin


def _run(net, p2, p1, idx, dist, gout, return_weight=False):
    from pointnet2_amd import train_mlp
    p2 = p2.clone().requires_grad_(True)
    p1 = p1.clone().requires_grad_(True) if p1 is not None else None
    res = train_mlp.fp_level_train(net, p2, p1, idx, dist, return_weight=return_weight)
    out = res[0] if return_weight else res
    params = list(net.parameters())
    inputs = [p2] + ([p1] if p1 is not None else [])
    grads = torch.autograd.grad(out, inputs + params, gout, retain_graph=True)      # (the tests read the saved z_l)
    return res, grads[:len(inputs)], grads[len(inputs):]


@pytest.mark.parametrize("name,b,n,m,c2,c1,widths", CASES, ids=[c[0] for c in CASES])
def test_fp_level_against_float64(cuda, name, b, n, m, c2, c1, widths):
    g = torch.Generator(device="cpu").manual_seed(11)
    net = _net(c2 + c1, widths, g, cuda).net
    p2, p1, idx, dist = _inputs(b, n, m, c2, c1, g, cuda)
    gout = torch.randn((b, n, widths[-1]), generator=g).to(cuda)
    ref = copy.deepcopy(net)
    out64, cache, grads64, g2_64, g1_64 = _float64(ref, p2, p1, idx, dist, gout)
    res, in_grads, pgrads = _run(net, p2, p1, idx, dist, gout)
    node = res.grad_fn.next_functions[0][0]
    assert _rel(res.detach().cpu().numpy().reshape(b * n, -1), out64) <= TOL, "out"
    nl = len(widths)
    zs = node.saved_tensors[-(2 * nl + 1):-(nl + 1)]
    for l in range(nl):
        z64 = cache["layers"][l]["z"] - ref[3 * l].bias.detach().double().cpu().numpy()      # z is stored without the bias
        assert _rel(zs[l].cpu().numpy(), z64) <= TOL, "z_%d" % (l + 1)
    saves = node.saved_tensors[-(nl + 1):-1]
    mg, flips, margin = _masked64(ref, p2, p1, idx, dist, gout, zs, saves)
    if flips == 0:                                                 # the float64 graph's own decisions: oracle/train_stack's gradients
        want = [g2_64] + ([g1_64] if c1 else []) + sum(([g["dW"].T, g["dgamma"], g["dbeta"]] for g in grads64), [])
    else:                                                          # ReLU arguments within rounding of zero: the kernels' linear piece
        assert flips <= 1e-5 * b * n * sum(widths) and margin <= 1e-5, (flips, margin)
        want = [t.numpy() for t in mg]
    got = [in_grads[0]] + ([in_grads[1]] if c1 else []) + sum(([pgrads[4 * l][:, :, 0, 0], pgrads[4 * l + 2], pgrads[4 * l + 3]]
                                                               for l in range(nl)), [])
    for k, (a, e) in enumerate(zip(got, want)):
        assert _rel(a.cpu().numpy(), e) <= TOL, (k, _rel(a.cpu().numpy(), e), flips)
    for l in range(nl):
        bn = net[3 * l + 1]
        assert _rel(bn.running_mean.cpu().numpy(), cache["layers"][l]["running_mean"]) <= TOL
        assert _rel(bn.running_var.cpu().numpy(), cache["layers"][l]["running_var"]) <= TOL
        assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("name,b,n,m,c2,c1,widths", [CASES[i] for i in (0, 2, 6, 8, 11)], ids=[CASES[i][0] for i in (0, 2, 6, 8, 11)])
def test_fp_level_against_the_current_path(cuda, name, b, n, m, c2, c1, widths):
    """Against fp_interp_concat + fp_mlp_train: the weights bit for bit, outputs within 5e-6 of scale, gradients 5e-3 in L2."""
    from pointnet2_amd import train_mlp
    from pointnet2_amd.tf_interpolate import fp_interp_concat
    g = torch.Generator(device="cpu").manual_seed(5)
    net = _net(c2 + c1, widths, g, cuda).net
    ref = copy.deepcopy(net)
    p2, p1, idx, dist = _inputs(b, n, m, c2, c1, g, cuda)
    gout = torch.randn((b, n, widths[-1]), generator=g).to(cuda)
    (out, weight), in_grads, pgrads = _run(net, p2, p1, idx, dist, gout, return_weight=True)
    a2 = p2.clone().requires_grad_(True)
    a1 = p1.clone().requires_grad_(True) if p1 is not None else None
    x, w_ref = fp_interp_concat(a2, a1, idx, dist)
    out_ref = train_mlp.fp_mlp_train(ref, x, cin=c2 + c1)
    inputs = [a2] + ([a1] if a1 is not None else [])
    grads_ref = torch.autograd.grad(out_ref, inputs + list(ref.parameters()), gout)
    assert torch.equal(weight, w_ref)
    assert float((out - out_ref).abs().max()) <= 5e-6 * float(out_ref.abs().max())
    for a, r in zip(list(in_grads) + list(pgrads), grads_ref):
        if float(r.norm()) > 0:
            assert float((a - r).norm() / r.norm()) <= 5e-3


def test_fp_level_reproducible_and_accumulating(cuda):
    from pointnet2_amd import train_mlp
    from pointnet2_amd._tensors import set_deterministic
    g = torch.Generator(device="cpu").manual_seed(2)
    b, n, m, c2, c1, widths = 8, 1024, 256, 256, 64, [256, 128]
    net = _net(c2 + c1, widths, g, cuda).net
    p2, p1, idx, dist = _inputs(b, n, m, c2, c1, g, cuda)
    gout = torch.randn((b, n, widths[-1]), generator=g).to(cuda)
    set_deterministic(True)
    try:
        runs = [_run(net, p2, p1, idx, dist, gout) for _ in range(2)]
    finally:
        set_deterministic(False)
    for a, r in zip(list(runs[0][1]) + list(runs[0][2]), list(runs[1][1]) + list(runs[1][2])):
        assert torch.equal(a, r)
    params = list(net.parameters())
    base = [torch.randn(p.shape, generator=g).to(cuda) for p in params]
    for p, b0 in zip(params, base):
        p.grad = b0.clone()
    set_deterministic(True)
    try:
        with train_mlp.accumulate_into_grad():
            out = train_mlp.fp_level_train(net, p2, p1, idx, dist)
            (out * gout).sum().backward()
    finally:
        set_deterministic(False)
    for l in range(len(widths)):
        for k in (0, 2, 3):                                     # conv weight, bn weight, bn bias: added by the kernels
            i = 4 * l + k
            assert torch.equal(params[i].grad, base[i] + runs[0][2][i])


@pytest.mark.parametrize("opts", [dict(pair_launch=True), dict(pair_launch=False), dict(fuse_wgrad=True), dict(fuse_wgrad=False),
                                  dict(side_stream=True)], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_fp_level_options_change_nothing(cuda, opts):
    from pointnet2_amd import train_mlp
    g = torch.Generator(device="cpu").manual_seed(9)
    b, n, m, c2, c1, widths = 4, 2048, 512, 128, 6, [128, 128, 128]
    net = _net(c2 + c1, widths, g, cuda).net
    ref = copy.deepcopy(net)
    p2, p1, idx, dist = _inputs(b, n, m, c2, c1, g, cuda)
    gout = torch.randn((b, n, widths[-1]), generator=g).to(cuda)
    want = _run(ref, p2, p1, idx, dist, gout)
    with train_mlp.options(**opts):
        got = _run(net, p2, p1, idx, dist, gout)
    assert float((got[0] - want[0]).abs().max()) <= 5e-6 * float(want[0].abs().max())
    for a, r in zip(list(got[1]) + list(got[2]), list(want[1]) + list(want[2])):
        assert float((a - r).abs().max()) <= 5e-5 * max(1e-30, float(r.abs().max()))


def test_fp_level_graph_capture_replays_the_eager_bits(cuda):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(3)
    fp = U.PointnetFPModule(64 + 6, [64, 32]).to(cuda).train()
    xyz1 = torch.rand(4, 256, 3, device=cuda)
    xyz2 = xyz1[:, :40].contiguous()
    p1 = torch.randn(4, 256, 6, device=cuda, requires_grad=True)
    p2 = torch.randn(4, 40, 64, device=cuda, requires_grad=True)
    w = torch.randn(4, 256, 32, device=cuda)
    params = list(fp.parameters())

    from pointnet2_amd import train_mlp
    from pointnet2_amd.tf_interpolate import three_nn

    def step():                                                    # (a level this small: the module takes the two-step path)
        dist, idx = three_nn(xyz1, xyz2)
        out = train_mlp.fp_level_train(fp.mlp.net, p2, p1, idx, dist)
        return out, torch.autograd.grad((out * w).sum(), params + [p1, p2])
    from pointnet2_amd._tensors import set_deterministic
    set_deterministic(True)                                        # every scatter and reduction in its reproducible mode
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out_g, grads_g = step()
        with torch.no_grad():
            p2.copy_(torch.randn(4, 40, 64, device=cuda))
        g.replay()
        torch.cuda.synchronize()
        out_e, grads_e = step()
    finally:
        set_deterministic(False)
    assert torch.equal(out_g, out_e)
    for a, b in zip(grads_g, grads_e):
        assert torch.equal(a, b)


def test_fp_module_routes_to_the_node_and_saves_the_concatenated_input(cuda):
    """PointnetFPModule.train() takes the node with and without geometry=; at sem_seg FP4 the peak memory of forward + backward
    is at least b n pitch 4 bytes below the current path's, measured in the same process."""
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    from pointnet2_amd.tf_interpolate import three_nn
    b, n, m, c2 = 8, 8192, 1024, 128
    torch.manual_seed(1)
    fp = U.PointnetFPModule(c2, [128, 128, 128]).to(cuda).train()
    xyz1 = torch.rand(b, n, 3, device=cuda)
    xyz2 = xyz1[:, :m].contiguous()
    p2 = torch.randn(b, m, c2, device=cuda, requires_grad=True)
    gout = torch.randn(b, n, 128, device=cuda)

    class _G:                                                      # a geometry computed ahead: three_nn's (dist, idx)
        def __init__(self):
            self.dist, self.idx = three_nn(xyz1, xyz2)

        def wait(self):
            return self
    calls = []
    real = train_mlp.fp_level_train

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    train_mlp.fp_level_train = spy
    try:
        for geo in (None, _G()):
            out = fp(xyz1, xyz2, None, p2, geometry=geo)
            (out * gout).sum().backward()
            assert fp.last_path == "fused_train"
    finally:
        train_mlp.fp_level_train = real
    assert len(calls) == 2
    small = U.PointnetFPModule(c2, [128, 128]).to(cuda).train()           # sem_seg FP1's size: the node is slower there
    s1 = torch.rand(8, 64, 3, device=cuda)
    train_mlp.fp_level_train = spy
    try:
        small(s1, s1[:, :16].contiguous(), None, torch.randn(8, 16, c2, device=cuda)).sum()
    finally:
        train_mlp.fp_level_train = real
    assert len(calls) == 2 and small.last_path == "fused_train"
    assert train_mlp.fp_level_supported(small.mlp.net, 8, 64, 16, c2, 0) and not train_mlp.fp_level_preferred(8, 64, 16, c2)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        (out * gout).sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    dist, idx = three_nn(xyz1, xyz2)

    def old():
        from pointnet2_amd.tf_interpolate import fp_interp_concat
        x, _ = fp_interp_concat(p2, None, idx, dist)
        return train_mlp.fp_mlp_train(fp.mlp.net, x, cin=c2)
    new = lambda: train_mlp.fp_level_train(fp.mlp.net, p2, None, idx, dist)
    p_new, p_old = peak(new), peak(old)
    assert p_old - p_new >= b * n * c2 * 4, (p_new, p_old)


def test_unsupported_fp_level_keeps_the_current_path(cuda):
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    torch.manual_seed(6)
    fp = U.PointnetFPModule(32 + 8, [32, 32]).to(cuda).train()
    xyz1 = torch.rand(3, 70, 3, device=cuda)                       # b n = 210: no multiple of 32
    xyz2 = xyz1[:, :20].contiguous()
    p2 = torch.randn(3, 20, 32, device=cuda, requires_grad=True)
    p1 = torch.randn(3, 70, 8, device=cuda, requires_grad=True)
    assert not train_mlp.fp_level_supported(fp.mlp.net, 3, 70, 20, 32, 8)
    out = fp(xyz1, xyz2, p1, p2)
    out.sum().backward()
    assert out.shape == (3, 70, 32) and p2.grad is not None and fp.last_path == "unfused"


def test_fp_level_the_node_does_not_cover_trains_on_the_two_step_path(cuda):
    """fp_level_supported says no (layer 1 of width 96: no whole rows per workgroup of its vector pass) where the stack itself
    runs: the module keeps fp_interp_concat + fp_mlp_train, and the node is not called."""
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    torch.manual_seed(8)
    fp = U.PointnetFPModule(64 + 8, [96, 32]).to(cuda).train()
    ref = copy.deepcopy(fp)
    ref.fused_mlp = False
    xyz1 = torch.rand(4, 256, 3, device=cuda)
    xyz2 = xyz1[:, :64].contiguous()
    assert train_mlp.stack_supported(fp.mlp.net, 4 * 256, 0, False)
    assert not train_mlp.fp_level_supported(fp.mlp.net, 4, 256, 64, 64, 8)
    calls = []
    real = train_mlp.fp_level_train

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    train_mlp.fp_level_train = spy
    outs = []
    try:
        for mod in (fp, ref):
            p2 = torch.randn(4, 64, 64, device=cuda, generator=None).requires_grad_(True) if not outs else outs[0][1]
            p1 = torch.randn(4, 256, 8, device=cuda).requires_grad_(True) if not outs else outs[0][2]
            a2, a1 = p2.detach().clone().requires_grad_(True), p1.detach().clone().requires_grad_(True)
            out = mod(xyz1, xyz2, a1, a2)
            out.square().mean().backward()
            outs.append((out, p2, p1, a2.grad, a1.grad))
    finally:
        train_mlp.fp_level_train = real
    assert calls == [] and fp.last_path == "fused_train" and ref.last_path == "unfused"
    (oa, _, _, ga2, ga1), (ob, _, _, gb2, gb1) = outs
    assert float((oa - ob).abs().max()) <= 5e-5 * float(ob.abs().max())
    assert float((ga2 - gb2).norm() / gb2.norm()) <= 5e-3 and float((ga1 - gb1).norm() / gb1.norm()) <= 5e-3
