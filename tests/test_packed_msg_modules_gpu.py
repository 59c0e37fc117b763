"""PointnetSAModuleMSG on PACKED batches (packed_batches; offsets= / max_points=) on the GPU, on the batch of
test_packed_modules_gpu.py: b = 3, counts (96, 33, 64), npoint 16, 6 feature channels; radii (0.3, 0.5), stacks
(32, 32, 64) / (32, 48, 64).

  geometry   new_xyz and every radius' idx equal the padded lengths= forward's exactly (idx up to the global offset), every
             group inside its own slab.
  inference  where both routes take the same fused-kernel family the outputs are equal bit for bit; where they run layer by
             layer they are two evaluations of the same stacks, within the bound test_packed_modules_gpu.py uses for such a
             pair: 2e-5 of the output's scale.
  training   forward output, every parameter gradient and running statistic of both stacks and points.grad against the float64
             restatement in oracle/train_stack.py (channel order features first) on the flat view, within 1e-5 of each tensor's
             scale, the project's bound for these nodes.
  chain      the packed MSG level, then PointnetFPModule(offsets1=) back onto the packed points, against the padded forward.
  refusals   what is not offered with offsets raises ValueError."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NPOINT, CFEAT = 16, 6
COUNTS = (96, 33, 64)                                        # total 193: slabs start at rows 96 and 129
RADII, STACKS = [0.3, 0.5], [[32, 32, 64], [32, 48, 64]]


def _batch(cuda, counts=COUNTS, seed=5):
    """-> flat xyz (total, 3) in the unit cube, flat features (total, CFEAT), offsets, the padded twins and lengths"""
    import pointnet2_amd as P
    g = torch.Generator().manual_seed(seed)
    total, n = sum(counts), max(counts)
    xyz = torch.rand((total, 3), generator=g).to(cuda)
    feats = torch.randn((total, CFEAT), generator=g).to(cuda)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=cuda)
    xp, lens = P.unpack_batch(xyz, offs, n=n)
    fp, _ = P.unpack_batch(feats, offs, n=n)
    return xyz, feats, offs, xp, fp, lens.to(cuda)


def _stir(mod, train=False):
    with torch.no_grad():
        for bn in [x for x in mod.modules() if isinstance(x, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d))]:
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(-1.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
    return mod.train() if train else mod.eval()


def _msg(cuda, nsamples, train=False):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(3)
    mod = _stir(U.PointnetSAModuleMSG(CFEAT, NPOINT, RADII, nsamples, STACKS).to(cuda), train)
    mod.packed_batches = True
    return mod


def _bits(t):
    return t.contiguous().view(torch.int32)


def _valid_rows(padded, counts):
    return torch.cat([padded[c, :n] for c, n in enumerate(counts)])


def _same_or_close(got, want, same_family):
    if same_family:
        assert torch.equal(_bits(got), _bits(want))
    else:
        assert (got - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())


# ------------------------------------------------------------------------------------------------ geometry and inference
@pytest.mark.parametrize("nsamples", [[16, 32], [8, 16]], ids=["fused", "layer_by_layer"])   # nsample 8: no fused SA kernel
def test_level_equals_the_padded_forward(cuda, nsamples):
    from pointnet2_amd import sa_mlp
    mod = _msg(cuda, nsamples)
    xyz, feats, offs, xp, fpad, lens = _batch(cuda)
    n, b = max(COUNTS), len(COUNTS)
    with torch.no_grad():
        new_xyz, out = mod(xyz, feats, offsets=offs, max_points=n)
        path = mod.last_path
        g = mod.packed_geometry(xyz, offs, n)
        wxyz, wout = mod(xp, fpad, lengths=lens)
        padded_path = mod.last_path
        wg = mod.geometry(xp, lengths=lens)
    # geometry: exact
    assert new_xyz.shape == (b, NPOINT, 3) and out.shape == (b, NPOINT, 128)
    assert torch.equal(_bits(new_xyz), _bits(wxyz)) and torch.equal(_bits(g.new_xyz.view(b, NPOINT, 3)), _bits(wxyz))
    assert torch.equal(g.fps_idx.view(b, NPOINT), wg.fps_idx + offs[:-1, None])
    assert len(g.idx) == len(wg.idx) == 2
    for idx, widx, ns in zip(g.idx, wg.idx, nsamples):
        assert idx.shape == (1, b * NPOINT, ns)
        idx = idx.view(b, NPOINT, ns)
        assert torch.equal(idx, widx + offs[:-1, None, None])                # global rows of the flat array
        assert bool((idx >= offs[:-1, None, None]).all()) and bool((idx < offs[1:, None, None]).all())   # inside its own slab
    # features
    fused = all(sa_mlp.supported(3 + CFEAT, tuple(w), ns) for w, ns in zip(STACKS, nsamples))
    assert fused == (nsamples == [16, 32])
    assert path == ("packed_fused" if fused else "packed_unfused") and padded_path == ("fused" if fused else "unfused")
    _same_or_close(out, wout, fused)                                         # one family per stack, chosen from (cin, widths, nsample) alone


def test_two_level_chain_equals_the_padded_forward(cuda):
    """the packed MSG level, then the FP level back onto the packed points"""
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import sa_mlp
    mod = _msg(cuda, [16, 32])
    fp = _stir(U.PointnetFPModule(128 + CFEAT, [64, 32]).to(cuda))
    xyz, feats, offs, xp, fpad, lens = _batch(cuda)
    total, n = sum(COUNTS), max(COUNTS)
    with torch.no_grad():
        new_xyz, l1 = mod(xyz, feats, offsets=offs, max_points=n)
        out = fp(xyz, new_xyz, feats, l1, offsets1=offs, max_points1=n)
        fp_path = fp.last_path
        wxyz, wl1 = mod(xp, fpad, lengths=lens)
        wout = fp(xp, wxyz, fpad, wl1, lengths1=lens)
        fp_padded_path = fp.last_path
    assert mod.last_path == "fused" and torch.equal(_bits(l1), _bits(wl1))
    assert out.shape == (total, 32)
    kinds = sa_mlp.fp_kind(total, 128, CFEAT, (64, 32)), sa_mlp.fp_kind(3 * n, 128, CFEAT, (64, 32))
    assert kinds[0] is not None and fp_path == "packed_fused" and fp_padded_path == "fused"
    _same_or_close(out, _valid_rows(wout, COUNTS), kinds[0] == kinds[1])


# ---------------------------------------------------------------------------------------------------------------- training
def _layers_of(net):
    """the stack's parameters and running statistics as oracle/train_stack.py takes them (float64 numpy), in layer order"""
    out, mods = [], list(net)
    for i in range(0, len(mods), 3):
        conv, bn = mods[i], mods[i + 1]
        out.append(dict(W=conv.weight.detach().reshape(conv.out_channels, -1).t().double().cpu().numpy(),
                        b=conv.bias.detach().double().cpu().numpy(), gamma=bn.weight.detach().double().cpu().numpy(),
                        beta=bn.bias.detach().double().cpu().numpy(), running_mean=bn.running_mean.detach().double().cpu().numpy(),
                        running_var=bn.running_var.detach().double().cpu().numpy(), conv=conv, bn=bn))
    return out


def _close(got, want, what):
    got, want = got.detach().double().cpu().numpy().reshape(want.shape), np.asarray(want)
    err, bound = float(np.abs(got - want).max()), 1e-5 * max(1.0, float(np.abs(want).max()))
    print("%s: max error %.3e (bound %.3e)" % (what, err, bound))
    assert err <= bound, what


def _check_stack(layers, grads, cache, what):
    for i, (L, G, C) in enumerate(zip(layers, grads, cache["layers"])):
        conv, bn = L["conv"], L["bn"]
        _close(conv.weight.grad.reshape(conv.out_channels, -1).t(), G["dW"], "%s layer %d grad_weight" % (what, i + 1))
        _close(conv.bias.grad, G["db"], "%s layer %d grad_bias" % (what, i + 1))
        _close(bn.weight.grad, G["dgamma"], "%s layer %d grad_gamma" % (what, i + 1))
        _close(bn.bias.grad, G["dbeta"], "%s layer %d grad_beta" % (what, i + 1))
        _close(bn.running_mean, C["running_mean"], "%s layer %d running_mean" % (what, i + 1))
        _close(bn.running_var, C["running_var"], "%s layer %d running_var" % (what, i + 1))


@pytest.mark.parametrize("index_plans", [False, True], ids=["no_plans", "index_plans"])
def test_level_trains_on_the_fused_nodes(cuda, index_plans):
    """train(): one fused node per radius on the flat view (B npoint groups of one cloud of `total` points), no mask"""
    from oracle import train_stack as T
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import train_mlp
    nsamples = [16, 32]
    mod = _msg(cuda, nsamples, train=True)
    mod.index_plans = index_plans
    xyz, feats, offs, _, _, _ = _batch(cuda)
    total, b = sum(COUNTS), len(COUNTS)
    layers = [_layers_of(mlp.net) for mlp in mod.mlps]                      # (before the call: the running statistics move)
    masks, plans = [], []
    keep, keep_plan = train_mlp._ragged_mask, U.index_plan
    train_mlp._ragged_mask = lambda *a: masks.append(a) or keep(*a)
    U.index_plan = lambda idx, n, kind: plans.append(n) or keep_plan(idx, n, kind)
    try:
        feats.requires_grad_(True)
        new_xyz, out = mod(xyz, feats, offsets=offs, max_points=max(COUNTS))
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(cuda)
        out.backward(gout)
    finally:
        train_mlp._ragged_mask, U.index_plan = keep, keep_plan
    assert mod.last_path == "packed_fused_train" and not masks
    assert plans == ([total, total] if index_plans else [])                 # one plan per radius, on `total` rows
    assert new_xyz.shape == (b, NPOINT, 3) and out.shape == (b, NPOINT, 128) and feats.grad.shape == (total, CFEAT)
    g = mod.packed_geometry(xyz, offs, max(COUNTS))                          # the geometry the forward used: same launches, same bits
    assert torch.equal(_bits(g.new_xyz.view(b, NPOINT, 3)), _bits(new_xyz))
    xh, fh, qh = xyz.cpu().numpy()[None], feats.detach().cpu().numpy()[None], new_xyz.reshape(1, -1, 3).cpu().numpy()
    grad_points, col = np.zeros((total, CFEAT)), 0
    for si, (ns, L) in enumerate(zip(nsamples, layers)):
        idx = g.idx[si].cpu().numpy()
        rows = T.group_rows(xh, qh, fh, idx, xyz_first=False)
        want, cache = T.forward(rows, L, pool=ns)
        width = want.shape[1]
        go = gout.reshape(-1, out.shape[2])[:, col:col + width].double().cpu().numpy()
        grad_rows, grads = T.backward(go, L, cache)
        _close(out.reshape(-1, out.shape[2])[:, col:col + width], want, "scale %d out" % si)
        _check_stack(L, grads, cache, "scale %d" % si)
        grad_points += T.scatter_feature_grad(grad_rows, idx, total, CFEAT, xyz_first=False)[0]
        col += width
    assert col == out.shape[2]
    _close(feats.grad, grad_points, "grad_points")


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_with_the_flag_on(cuda):
    import pointnet2_amd.pointnet_util as U
    mod = _msg(cuda, [16, 32])
    xyz, feats, offs, xp, fpad, lens = _batch(cuda)
    n = max(COUNTS)
    kw = dict(offsets=offs, max_points=n)
    ahead = mod.geometry(xp, lengths=lens)
    xyz_grad = _msg(cuda, [16, 32], train=True)
    xyz_grad.fused_xyz_grad = True
    wants_grad = xyz.clone().requires_grad_(True)
    trainer = _msg(cuda, [16, 32], train=True)
    with torch.no_grad():
        calls = [lambda: mod(xyz, feats, lengths=list(COUNTS), **kw), lambda: mod(xyz, feats, npoints=[16, 8, 16], **kw),
                 lambda: mod(xyz, feats, geometry=ahead, **kw), lambda: xyz_grad(xyz, feats, **kw), lambda: mod(xyz, feats, offsets=offs)]
        for call in calls:
            with pytest.raises(ValueError, match="offsets|max_points"):
                call()
    with pytest.raises(ValueError, match="offsets"):
        trainer(wants_grad, feats, **kw)
    off = U.PointnetSAModuleMSG(CFEAT, NPOINT, RADII, [16, 32], STACKS).to(cuda).eval()
    with torch.no_grad(), pytest.raises(ValueError, match="offsets"):      # the default module refuses as it always has
        off(xyz, feats, **kw)
