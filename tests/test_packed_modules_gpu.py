"""PointnetSAModule / PointnetFPModule on PACKED batches (offsets= / max_points=, offsets1= / max_points1=) on
the GPU, on the first set-abstraction level and the last feature-propagation level of a small two-level network: b = 3, counts
(96, 33, 64), npoint 16.

  geometry   the packed forward's new_xyz / idx equal the padded lengths= forward's exactly (idx up to the global offset).
  inference  where both routes take the same fused-kernel family (asserted with pn2_sa_mlp3_config / fp_kind) the outputs are
             equal bit for bit on the rows of valid points; where they run layer by layer they are two evaluations of the same
             stack, within the bound tests/test_ragged_infer_modules_gpu.py uses for such a pair: 2e-5 of the output's scale.
  training   forward outputs and every parameter / input gradient against the float64 restatement of the level in
             oracle/train_stack.py on the compacted rows, within 1e-5 of each tensor's scale (tests/test_train_ragged_gpu.py's
             tolerance); the FP level once with total a multiple of 32 (the dense node: no mask buffer is requested) and once
             with total = 193 (the masked node with b = 1, the tail the only masked word).
  refusals   the options not offered with offsets raise ValueError."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NPOINT, RADIUS, CFEAT = 16, 0.4, 6
COUNTS = (96, 33, 64)                                        # total 193: slabs start at rows 96 and 129
COUNTS_32 = (96, 32, 64)                                     # total 192


def _batch(cuda, counts, seed=5):
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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _valid_rows(padded, counts):
    return torch.cat([padded[c, :n] for c, n in enumerate(counts)])


def _levels(cuda, nsample, train=False):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(3)
    sa = _stir(U.PointnetSAModule(CFEAT, NPOINT, RADIUS, nsample, [32, 32, 64]).to(cuda), train)
    fp = _stir(U.PointnetFPModule(64 + CFEAT, [64, 32]).to(cuda), train)
    return sa, fp


# ------------------------------------------------------------------------------------------------ geometry and inference
@pytest.mark.parametrize("nsample", [8, 16])                               # 8: no fused SA kernel, layer by layer; 16: the resident kernel
def test_two_level_network_equals_the_padded_forward(cuda, nsample):
    from pointnet2_amd import sa_mlp
    sa, fp = _levels(cuda, nsample)
    xyz, feats, offs, xp, fpad, lens = _batch(cuda, COUNTS)
    total, n = sum(COUNTS), max(COUNTS)
    with torch.no_grad():
        new_xyz, l1, idx = sa(xyz, feats, offsets=offs, max_points=n)
        sa_path = sa.last_path
        wxyz, wl1, widx = sa(xp, fpad, lengths=lens)
        sa_padded_path = sa.last_path
        out = fp(xyz, new_xyz, feats, l1, offsets1=offs, max_points1=n)
        fp_path = fp.last_path
        wout = fp(xp, wxyz, fpad, wl1, lengths1=lens)
        fp_padded_path = fp.last_path
    # geometry: exact
    assert new_xyz.shape == (3, NPOINT, 3) and idx.shape == (3, NPOINT, nsample) and l1.shape == (3, NPOINT, 64)
    assert torch.equal(_bits(new_xyz), _bits(wxyz))
    assert torch.equal(idx, widx + offs[:-1, None, None])                    # global rows of the flat array
    assert int(idx.min()) >= 0 and bool((idx < offs[1:, None, None]).all())  # every group inside its own slab
    # SA features
    fused = sa_mlp.supported(3 + CFEAT, (32, 32, 64), nsample)
    assert fused == (nsample == 16)
    assert sa_path == ("packed_fused" if fused else "packed_unfused") and sa_padded_path == ("fused" if fused else "unfused")
    if fused:                                                                # one family, chosen from (cin, widths, nsample) alone
        assert sa_mlp.kind(3 + CFEAT, (32, 32, 64), nsample) == "resident"
        assert torch.equal(_bits(l1), _bits(wl1))
    else:
        assert (l1 - wl1).abs().max().item() <= 2e-5 * max(1.0, wl1.abs().max().item())
    # FP level: (total, C) against the valid rows of the padded (b, n, C)
    assert out.shape == (total, 32)
    want = _valid_rows(wout, COUNTS)
    kinds = sa_mlp.fp_kind(total, 64, CFEAT, (64, 32)), sa_mlp.fp_kind(3 * n, 64, CFEAT, (64, 32))
    assert kinds[0] is not None and fp_path == "packed_fused" and fp_padded_path == "fused"
    if fused and kinds[0] == kinds[1]:                                       # same inputs, same family: the same bits
        assert torch.equal(_bits(out), _bits(want))
    else:
        assert (out - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())


def test_fp_level_alone_same_inputs_same_bits(cuda):
    """the FP level fed with identical known features: the packed call and the padded call take the same kernel family and give
    the same bits on the rows of valid points"""
    from pointnet2_amd import sa_mlp
    _, fp = _levels(cuda, 16)
    xyz, feats, offs, xp, fpad, lens = _batch(cuda, COUNTS)
    g = torch.Generator().manual_seed(6)
    known_xyz = torch.rand((3, NPOINT, 3), generator=g).to(cuda)
    known = torch.randn((3, NPOINT, 64), generator=g).to(cuda)
    with torch.no_grad():
        out = fp(xyz, known_xyz, feats, known, offsets1=offs, max_points1=max(COUNTS))
        assert fp.last_path == "packed_fused"
        wout = fp(xp, known_xyz, fpad, known, lengths1=lens)
        assert fp.last_path == "fused"
    assert sa_mlp.fp_kind(sum(COUNTS), 64, CFEAT, (64, 32)) == sa_mlp.fp_kind(3 * max(COUNTS), 64, CFEAT, (64, 32))
    assert torch.equal(_bits(out), _bits(_valid_rows(wout, COUNTS)))


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


def test_sa_level_trains_on_the_fused_node(cuda):
    """the first SA level in train(): the fused node on the flat view (B npoint groups of one cloud of `total` points), no mask"""
    from oracle import train_stack as T
    from pointnet2_amd import train_mlp
    sa, _ = _levels(cuda, 16, train=True)
    xyz, feats, offs, _, _, _ = _batch(cuda, COUNTS)
    total = sum(COUNTS)
    layers = _layers_of(sa.mlp.net)                                          # (before the call: the running statistics move)
    masks = []
    keep = train_mlp._ragged_mask
    train_mlp._ragged_mask = lambda *a: masks.append(a) or keep(*a)
    try:
        feats.requires_grad_(True)
        new_xyz, out, idx = sa(xyz, feats, offsets=offs, max_points=max(COUNTS))
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(cuda)
        out.backward(gout)
    finally:
        train_mlp._ragged_mask = keep
    assert sa.last_path == "packed_fused_train" and not masks
    rows = T.group_rows(xyz.cpu().numpy()[None], new_xyz.reshape(1, -1, 3).cpu().numpy(), feats.detach().cpu().numpy()[None],
                        idx.reshape(1, 3 * NPOINT, 16).cpu().numpy())
    want, cache = T.forward(rows, layers, pool=16)
    grad_rows, grads = T.backward(gout.reshape(-1, out.shape[2]).double().cpu().numpy(), layers, cache)
    _close(out, want, "SA out")
    _check_stack(layers, grads, cache, "SA")
    _close(feats.grad, T.scatter_feature_grad(grad_rows, idx.reshape(1, 3 * NPOINT, 16).cpu().numpy(), total, CFEAT)[0], "SA grad_points")


@pytest.mark.parametrize("counts,path,masked", [(COUNTS_32, "packed_fused_train", False), (COUNTS, "packed_fused_train_ragged", True)],
                         ids=["total_192_dense_node", "total_193_masked_tail"])
def test_fp_level_trains(cuda, oracle, counts, path, masked):
    from oracle import train_stack as T
    from pointnet2_amd import train_mlp
    _, fp = _levels(cuda, 16, train=True)
    xyz, feats, offs, _, _, _ = _batch(cuda, counts)
    total, m, c2 = sum(counts), NPOINT, 64
    g = torch.Generator().manual_seed(8)
    known_xyz = torch.rand((3, m, 3), generator=g).to(cuda)
    known = torch.randn((3, m, c2), generator=g).to(cuda).requires_grad_(True)
    feats.requires_grad_(True)
    layers = _layers_of(fp.mlp.net)
    masks = []
    keep = train_mlp._ragged_mask
    train_mlp._ragged_mask = lambda *a: masks.append(a) or keep(*a)
    try:
        out = fp(xyz, known_xyz, feats, known, offsets1=offs, max_points1=max(counts))
        gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(cuda)
        out.backward(gout)
    finally:
        train_mlp._ragged_mask = keep
    assert fp.last_path == path, fp.last_path
    assert bool(masks) == masked                                             # total % 32 == 0: no mask buffer at all
    assert out.shape == (total, 32) and feats.grad.shape == (total, CFEAT) and known.grad.shape == (3, m, c2)
    # float64 restatement on the compacted rows: three_nn per slice (CPU oracle), weights, interpolation, concat, the stack
    xh, kh = xyz.cpu().numpy(), known_xyz.cpu().numpy()
    oh = offs.cpu().numpy()
    dist = np.concatenate([oracle.three_nn(xh[None, oh[c]:oh[c + 1]], kh[c:c + 1])[0][0] for c in range(3)]).astype(np.float64)
    nidx = np.concatenate([oracle.three_nn(xh[None, oh[c]:oh[c + 1]], kh[c:c + 1])[1][0] + c * m for c in range(3)])   # rows of (b m, c2)
    inv = 1.0 / np.maximum(dist, 1e-10)
    w = inv / inv.sum(axis=1, keepdims=True)
    p2 = known.detach().double().cpu().numpy().reshape(3 * m, c2)
    rows = np.concatenate([(p2[nidx] * w[:, :, None]).sum(axis=1), feats.detach().double().cpu().numpy()], axis=1)
    want, cache = T.forward(rows, layers, pool=0)
    grad_rows, grads = T.backward(gout.double().cpu().numpy(), layers, cache)
    _close(out, want, "FP out")
    _check_stack(layers, grads, cache, "FP")
    _close(feats.grad, grad_rows[:, c2:], "FP grad_points1")
    g2 = np.zeros((3 * m, c2))
    for k in range(3):
        np.add.at(g2, nidx[:, k], grad_rows[:, :c2] * w[:, k:k + 1])
    _close(known.grad, g2.reshape(3, m, c2), "FP grad_points2")


# --------------------------------------------------------------------------------------------------------------- refusals
def test_options_not_offered_with_offsets(cuda):
    import pointnet2_amd.pointnet_util as U
    xyz, feats, offs, _, _, _ = _batch(cuda, COUNTS)
    n = max(COUNTS)
    kw = dict(offsets=offs, max_points=n)
    msg = U.PointnetSAModuleMSG(CFEAT, NPOINT, [0.3, 0.5], [16, 32], [[32, 32, 64], [32, 48, 64]]).to(cuda).eval()
    everything = U.PointnetSAModule(CFEAT, None, None, None, [32, 32, 64], group_all=True).to(cuda).eval()
    knn = U.PointnetSAModule(CFEAT, NPOINT, RADIUS, 16, [32, 32, 64], knn=True).to(cuda).eval()
    plain = U.PointnetSAModule(CFEAT, NPOINT, RADIUS, 16, [32, 32, 64]).to(cuda).eval()
    xyz_grad = U.PointnetSAModule(CFEAT, NPOINT, RADIUS, 16, [32, 32, 64]).to(cuda).train()
    xyz_grad.fused_xyz_grad = True
    fp = U.PointnetFPModule(64 + CFEAT, [64, 32]).to(cuda).eval()
    known_xyz, known = torch.rand(3, NPOINT, 3, device=cuda), torch.rand(3, NPOINT, 64, device=cuda)
    calls = [lambda: msg(xyz, feats, **kw), lambda: everything(xyz, feats, **kw), lambda: knn(xyz, feats, **kw),
             lambda: plain(xyz, feats, npoints=[16, 8, 16], **kw), lambda: plain(xyz, feats, lengths=list(COUNTS), **kw),
             lambda: xyz_grad(xyz, feats, **kw), lambda: plain(xyz, feats, offsets=offs),
             lambda: fp(xyz, known_xyz, feats, known, offsets1=offs, max_points1=n, lengths1=list(COUNTS)),
             lambda: fp(xyz, known_xyz, feats, known, offsets1=offs)]
    with torch.no_grad():
        for call in calls:
            with pytest.raises(ValueError, match="offsets|max_points"):
                call()
