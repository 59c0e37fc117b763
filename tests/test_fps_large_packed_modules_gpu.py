"""PointnetSAModule / PointnetFPModule on a PACKED batch whose max_points lies beyond the register tiers of farthest point
sampling (counts 17000 and 9000, under set_fps_ragged_large(True)): the level's sampling goes through
pn2_farthest_point_sample_large_packed_ex, everything behind it through the code the packed levels already have. Compared with the
same modules' padded lengths= forward as tests/test_packed_modules_gpu.py compares its levels: geometry exactly, features bit for
bit where both routes take the same fused-kernel family (asserted)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NPOINT, RADIUS, NSAMPLE, CFEAT = 64, 0.2, 16, 6
COUNTS = (17000, 9000)                                       # total 26000: the second slab starts at row 17000
WIDTHS, FP_WIDTHS = [32, 32, 64], [64, 32]


@pytest.fixture()
def ragged_large():
    from pointnet2_amd import tf_sampling as T
    before = T._FPS_RAGGED_LARGE[0]
    T.set_fps_ragged_large(True)
    try:
        yield
    finally:
        T.set_fps_ragged_large(before)


def _stir(mod):
    with torch.no_grad():
        for bn in [x for x in mod.modules() if isinstance(x, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d))]:
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(-1.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
    return mod.eval()


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_sa_and_fp_level_equal_the_padded_forward(cuda, ragged_large):
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import sa_mlp
    from pointnet2_amd import synthetic as S
    total, n, b = sum(COUNTS), max(COUNTS), len(COUNTS)
    clouds = S.sphere_clouds(b, n, 1381)
    xyz = torch.from_numpy(np.concatenate([clouds[i, :c] for i, c in enumerate(COUNTS)])).to(cuda)
    feats = torch.randn((total, CFEAT), generator=torch.Generator().manual_seed(5)).to(cuda)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(COUNTS)]), dtype=torch.int32, device=cuda)
    xp, lens = P.unpack_batch(xyz, offs, n=n)
    fpad, _ = P.unpack_batch(feats, offs, n=n)
    lens = lens.to(cuda)
    torch.manual_seed(3)
    sa = _stir(U.PointnetSAModule(CFEAT, NPOINT, RADIUS, NSAMPLE, WIDTHS).to(cuda))
    fp = _stir(U.PointnetFPModule(64 + CFEAT, FP_WIDTHS).to(cuda))
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
    assert new_xyz.shape == (b, NPOINT, 3) and idx.shape == (b, NPOINT, NSAMPLE) and l1.shape == (b, NPOINT, 64)
    assert torch.equal(_bits(new_xyz), _bits(wxyz))
    assert torch.equal(idx, widx + offs[:-1, None, None])                    # global rows of the flat array
    assert int(idx.min()) >= 0 and bool((idx < offs[1:, None, None]).all())  # every group inside its own slab
    # SA features: one fused family, chosen from (cin, widths, nsample) alone
    assert sa_mlp.supported(3 + CFEAT, tuple(WIDTHS), NSAMPLE)
    assert sa_path.startswith("packed_") and sa_path == "packed_fused" and sa_padded_path == "fused"
    assert torch.equal(_bits(l1), _bits(wl1))
    # FP level back onto the 26000 packed rows: against the valid rows of the padded (b, n, C)
    assert out.shape == (total, FP_WIDTHS[-1])
    kinds = sa_mlp.fp_kind(total, 64, CFEAT, tuple(FP_WIDTHS)), sa_mlp.fp_kind(b * n, 64, CFEAT, tuple(FP_WIDTHS))
    assert kinds[0] is not None and kinds[0] == kinds[1]                      # same inputs, same family: the same bits
    assert fp_path.startswith("packed_") and fp_path == "packed_fused" and fp_padded_path == "fused"
    want = torch.cat([wout[c, :k] for c, k in enumerate(COUNTS)])
    assert torch.equal(_bits(out), _bits(want))
