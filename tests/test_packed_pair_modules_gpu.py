"""PointnetSAModule / PointnetFPModule on packed batches with the second side (set_packed_pairs(True); DESIGN.md 4.12 "the second
side, packed") on the GPU, on the small two-level network of tests/test_packed_modules_gpu.py: b = 3, counts (96, 33, 64),
npoint 16, stacks [32, 32, 64].

  knn        a knn module on packed input: eval() bit-identical to the module's own _forward_on on a flat-view geometry built by
             hand from the dense operators on each slice; train() against the float64 restatement of oracle/train_stack.py on
             the oracle's geometry per slice, within 1e-5 of each tensor's scale (that file's tolerance).
  npoints    eval(): rows below npoints[c] are the packed forward's without npoints (the chain is prefix-consistent), rows from
             npoints[c] on exact zeros. train(): the compacting path, last_path "packed_unfused_ragged", against the padded
             module with lengths= / npoints= -- two layer-by-layer evaluations of one stack: the output, the feature gradient
             and every parameter gradient within 2e-5 of each tensor's scale.
  two levels new_xyz, the features and lengths=npoints feed a second, padded level: equal to the all-padded forward.
  FP         lengths2 with offsets1: full counts change nothing; short counts keep every neighbour below c m + m_c."""
import numpy as np
import pytest
import torch

import test_packed_modules_gpu as PMOD
from test_packed_modules_gpu import CFEAT, COUNTS, NPOINT, RADIUS, _batch, _bits, _check_stack, _close, _layers_of, _stir

pytestmark = pytest.mark.gpu

NPOINTS = (16, 5, 9)                                         # m_c = m, short, short


@pytest.fixture(autouse=True)
def pairs_on():
    import pointnet2_amd as P
    from pointnet2_amd import _tensors
    before = _tensors.packed_pairs()
    P.set_packed_pairs(True)
    try:
        yield
    finally:
        P.set_packed_pairs(before)


def _sa(cuda, nsample, train=False, knn=False, seed=3):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(seed)
    return _stir(U.PointnetSAModule(CFEAT, NPOINT, RADIUS, nsample, [32, 32, 64], knn=knn).to(cuda), train)


def _near(got, want, what):
    err, bound = (got - want).abs().max().item(), 2e-5 * max(1.0, want.abs().max().item())
    print("%s: max difference %.3e (bound %.3e)" % (what, err, bound))
    assert err <= bound, what


# ------------------------------------------------------------------------------------------------------------------ kNN
@pytest.mark.parametrize("nsample", [8, 16])                               # 8: layer by layer; 16: the resident inference kernel
def test_knn_module_on_packed_input_is_forward_on_of_the_hand_built_geometry(cuda, nsample):
    import pointnet2_amd as P
    from pointnet2_amd.geometry import SAGeometry
    sa = _sa(cuda, nsample, knn=True)
    xyz, feats, offs, _, _, _ = _batch(cuda, COUNTS)
    total, b = sum(COUNTS), len(COUNTS)
    with torch.no_grad():
        new_xyz, out, idx = sa(xyz, feats, offsets=offs, max_points=max(COUNTS))
        path = sa.last_path
        assert path == ("packed_fused" if nsample == 16 else "packed_unfused")
        parts = []
        for c in range(b):                                                   # the dense operators on each slice alone
            lo, hi = int(offs[c]), int(offs[c + 1])
            sl = xyz[lo:hi].unsqueeze(0).contiguous()
            fi, nx = P.farthest_point_sample_gather(NPOINT, sl)
            _, ki = P.knn_point(nsample, sl, nx)
            parts.append((nx, ki + lo, fi + lo))
        g = SAGeometry(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), torch.cat([p[2] for p in parts], 1))
        wxyz, wout, widx = sa._forward_on(xyz.view(1, total, 3), feats.view(1, total, CFEAT), g, path[len("packed_"):])
    assert torch.equal(_bits(new_xyz), _bits(wxyz.view(b, NPOINT, 3))) and torch.equal(idx, widx.view(b, NPOINT, nsample))
    assert int(idx.min()) >= 0 and bool((idx >= offs[:-1, None, None]).all()) and bool((idx < offs[1:, None, None]).all())
    assert torch.equal(_bits(out), _bits(wout.view(b, NPOINT, 64)))


def _oracle_knn_geometry(oracle, xyz, offs, nsample):
    """FPS and kNN of the CPU oracle per slice -> new_xyz (b, m, 3), idx (b, m, nsample) global"""
    xh, oh = xyz.cpu().numpy(), offs.cpu().numpy()
    nx, gi = [], []
    for c in range(len(oh) - 1):
        sl = np.ascontiguousarray(xh[None, oh[c]:oh[c + 1]])
        q = oracle.gather_point(sl, oracle.farthest_point_sample(NPOINT, sl))
        dx = sl[:, None, :, 0] - q[0][None, :, None, 0]
        dy = sl[:, None, :, 1] - q[0][None, :, None, 1]
        dz = sl[:, None, :, 2] - q[0][None, :, None, 2]
        oi, _ = oracle.select_top_k(nsample, ((dx * dx + dy * dy) + dz * dz).astype(np.float32))
        nx.append(q[0])
        gi.append(oi[0, :, :nsample] + oh[c])
    return np.stack(nx), np.stack(gi).astype(np.int32)


def test_knn_module_on_packed_input_trains(cuda, oracle):
    from oracle import train_stack as T
    sa = _sa(cuda, 16, train=True, knn=True)
    xyz, feats, offs, _, _, _ = _batch(cuda, COUNTS)
    total = sum(COUNTS)
    layers = _layers_of(sa.mlp.net)                                          # (before the call: the running statistics move)
    feats.requires_grad_(True)
    new_xyz, out, idx = sa(xyz, feats, offsets=offs, max_points=max(COUNTS))
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(cuda)
    out.backward(gout)
    assert sa.last_path == "packed_fused_train"
    wxyz, widx = _oracle_knn_geometry(oracle, xyz, offs, 16)
    assert np.array_equal(new_xyz.cpu().numpy(), wxyz) and np.array_equal(idx.cpu().numpy(), widx)
    flat_idx = widx.reshape(1, 3 * NPOINT, 16)
    rows = T.group_rows(xyz.cpu().numpy()[None], wxyz.reshape(1, -1, 3), feats.detach().cpu().numpy()[None], flat_idx)
    want, cache = T.forward(rows, layers, pool=16)
    grad_rows, grads = T.backward(gout.reshape(-1, out.shape[2]).double().cpu().numpy(), layers, cache)
    _close(out, want, "kNN SA out")
    _check_stack(layers, grads, cache, "kNN SA")
    _close(feats.grad, T.scatter_feature_grad(grad_rows, flat_idx, total, CFEAT)[0], "kNN SA grad_points")


# -------------------------------------------------------------------------------------------------------------- npoints
@pytest.mark.parametrize("knn", [False, True])
@pytest.mark.parametrize("nsample", [8, 16])
def test_npoints_with_offsets_eval(cuda, nsample, knn):
    sa = _sa(cuda, nsample, knn=knn)
    xyz, feats, offs, _, _, _ = _batch(cuda, COUNTS)
    cnts = torch.tensor(NPOINTS, dtype=torch.int32, device=cuda)
    with torch.no_grad():
        new_xyz, out, idx = sa(xyz, feats, offsets=offs, max_points=max(COUNTS), npoints=cnts)
        path = sa.last_path
        wxyz, wout, widx = sa(xyz, feats, offsets=offs, max_points=max(COUNTS))
        assert path == sa.last_path == ("packed_fused" if nsample == 16 else "packed_unfused")
    for c, mc in enumerate(NPOINTS):
        assert torch.equal(_bits(new_xyz[c, :mc]), _bits(wxyz[c, :mc])) and torch.equal(idx[c, :mc], widx[c, :mc])
        assert torch.equal(new_xyz[c, mc:], xyz[int(offs[c])].expand(NPOINT - mc, 3))              # sample 0 repeated
        assert bool((idx[c, mc:] == offs[c]).all())                                                # the cloud's own first row
        assert not _bits(out[c, mc:]).any().item()                                                 # exact zeros
        # equal bit for bit: in eval() a row depends on its own group alone, and the two calls run the same route (the resident
        # kernel, or the same layers on tensors of the same shapes)
        assert torch.equal(_bits(out[c, :mc]), _bits(wout[c, :mc]))
    assert bool((idx >= offs[:-1, None, None]).all()) and bool((idx < offs[1:, None, None]).all())


@pytest.mark.parametrize("knn", [False, True])
def test_npoints_with_offsets_train_takes_the_compacting_path(cuda, knn):
    sa = _sa(cuda, 16, train=True, knn=knn)
    xyz, feats, offs, xp, fpad, lens = _batch(cuda, COUNTS)
    cnts = torch.tensor(NPOINTS, dtype=torch.int32, device=cuda)
    feats.requires_grad_(True)
    fpad.requires_grad_(True)
    params = list(sa.parameters())
    gout = torch.randn((3, NPOINT, 64), generator=torch.Generator().manual_seed(7)).to(cuda)
    new_xyz, out, idx = sa(xyz, feats, offsets=offs, max_points=max(COUNTS), npoints=cnts)
    assert sa.last_path == "packed_unfused_ragged"
    grads = torch.autograd.grad(out, [feats] + params, gout)
    wxyz, wout, widx = sa(xp, fpad, lengths=lens, npoints=cnts)
    assert sa.last_path == "unfused_ragged"
    wgrads = torch.autograd.grad(wout, [fpad] + params, gout)
    assert torch.equal(_bits(new_xyz), _bits(wxyz)) and torch.equal(idx, widx + offs[:-1, None, None])
    for c, mc in enumerate(NPOINTS):
        _near(out[c, :mc].detach(), wout[c, :mc].detach(), "cloud %d" % c)
        assert not _bits(out[c, mc:].detach()).any().item() and not _bits(wout[c, mc:].detach()).any().item()
    # the same gradients: the fill rows' output gradient reaches nothing, the valid groups are the padded call's
    _near(grads[0], PMOD._valid_rows(wgrads[0], COUNTS), "grad_points")
    assert not _bits(torch.cat([wgrads[0][c, n:] for c, n in enumerate(COUNTS)])).any().item()   # padding rows: exactly zero
    for (name, _), g, w in zip(sa.named_parameters(), grads[1:], wgrads[1:]):
        _near(g, w, "grad " + name)


def test_two_levels_packed_then_padded(cuda):
    """level 1 on the packed batch with npoints, level 2 padded with lengths = npoints: the all-padded forward's results"""
    import pointnet2_amd.pointnet_util as U
    sa1 = _sa(cuda, 16)
    torch.manual_seed(4)
    sa2 = _stir(U.PointnetSAModule(64, 4, 0.8, 8, [32, 32, 64]).to(cuda))
    xyz, feats, offs, xp, fpad, lens = _batch(cuda, COUNTS)
    cnts = torch.tensor(NPOINTS, dtype=torch.int32, device=cuda)
    with torch.no_grad():
        x1, f1, _ = sa1(xyz, feats, offsets=offs, max_points=max(COUNTS), npoints=cnts)
        x2, f2, i2 = sa2(x1, f1, lengths=cnts)
        wx1, wf1, _ = sa1(xp, fpad, lengths=lens, npoints=cnts)
        wx2, wf2, wi2 = sa2(wx1, wf1, lengths=cnts)
    assert torch.equal(_bits(x1), _bits(wx1)) and torch.equal(_bits(x2), _bits(wx2)) and torch.equal(i2, wi2)
    _near(f1, wf1, "level 1")
    _near(f2, wf2, "level 2")
    assert x2.shape == (3, 4, 3) and f2.shape == (3, 4, 64) and torch.isfinite(f2).all()


# ------------------------------------------------------------------------------------------------------------------- FP
def test_fp_module_lengths2_with_offsets1(cuda, monkeypatch):
    import pointnet2_amd.pointnet_util as U
    _, fp = PMOD._levels(cuda, 16)
    xyz, feats, offs, _, _, _ = _batch(cuda, COUNTS)
    g = torch.Generator().manual_seed(6)
    known_xyz = torch.rand((3, NPOINT, 3), generator=g).to(cuda)
    known = torch.randn((3, NPOINT, 64), generator=g).to(cuda)
    seen = []
    real = U.three_nn

    def spy(*a, **kw):
        dist, idx = real(*a, **kw)
        seen.append(kw["out"][1] if kw.get("out") is not None else idx)
        return dist, idx
    monkeypatch.setattr(U, "three_nn", spy)
    kw = dict(offsets1=offs, max_points1=max(COUNTS))
    with torch.no_grad():
        plain = fp(xyz, known_xyz, feats, known, **kw)
        full = fp(xyz, known_xyz, feats, known, lengths2=[NPOINT] * 3, **kw)
        assert fp.last_path == "packed_fused"
        known_xyz[1, 5:] = float("nan")                                      # beyond the counts: never read
        known_xyz[2, 9:] = float("nan")
        short = fp(xyz, known_xyz, feats, known, lengths2=torch.tensor(NPOINTS, dtype=torch.int32, device=cuda), **kw)
    assert torch.equal(_bits(plain), _bits(full)) and torch.equal(seen[0], seen[1])
    assert short.shape == (sum(COUNTS), 32) and torch.isfinite(short).all()
    idx = seen[2].reshape(-1, 3)
    for c, mc in enumerate(NPOINTS):
        rows = idx[int(offs[c]):int(offs[c + 1])]
        assert bool((rows >= c * NPOINT).all()) and bool((rows < c * NPOINT + mc).all()), c
