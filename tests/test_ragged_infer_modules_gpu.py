"""fused_ragged_eval (opt-in) on the three module classes: eval() with lengths= / npoints= / lengths1= through the fused
inference kernels with the counts inside (last_path "fused_ragged") gives exactly what the default routes give -- the dense
kernels on every row and a torch.where -- because the valid rows are the same kernel arithmetic and the padding rows are +0.0
either way. With NaN in the padding rows of the features the flag-on result equals the flag-off result on zero-filled padding.
The ragged group_all level is compared with today's layer-by-layer route ("unfused": another evaluation order) within the
fused-vs-layer-by-layer bound of tests/test_sa_mlp_gpu.py for the cooperative kernel, 2e-5 of the output scale."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, M = 3, 96, 9
LENGTHS, NPOINTS = [96, 50, 7], [9, 4, 1]


def _stir(mod):
    for bn in [x for x in mod.modules() if isinstance(x, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d))]:
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
    return mod.eval()


def _clouds(cuda, c, n=N):
    g = torch.Generator().manual_seed(11 + c)
    return torch.rand((B, n, 3), generator=g).to(cuda), torch.randn((B, n, c), generator=g).to(cuda)


def _counts(cuda):
    return (torch.tensor(LENGTHS, dtype=torch.int32, device=cuda), torch.tensor(NPOINTS, dtype=torch.int32, device=cuda))


def _with_padding(points, lengths, value):
    out = points.clone()
    for c, L in enumerate(lengths):
        out[c, L:] = value
    return out


def _on_off(mod, call, off_path):
    """call(mod) with the flag off and on -> (off, on) outputs; the paths are asserted."""
    with torch.no_grad():
        mod.fused_ragged_eval = False
        off = call(mod)
        assert mod.last_path == off_path, mod.last_path
        mod.fused_ragged_eval = True
        on = call(mod)
        assert mod.last_path == "fused_ragged", mod.last_path
        mod.fused_ragged_eval = False
    return off, on


SA_CASES = ["level", "geometry", "knn", "mlp2", "lengths_only", "npoints_only"]


@pytest.mark.parametrize("case", SA_CASES)
def test_sa_module(cuda, case):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(0)
    mod = _stir(U.PointnetSAModule(6, M, 0.4, 16, [32, 32, 64], mlp2=[48] if case == "mlp2" else None, knn=case == "knn").to(cuda))
    assert mod.fused_ragged_eval is False
    xyz, points = _clouds(cuda, 6)
    lengths, npoints = _counts(cuda)
    kw = dict(lengths=lengths, npoints=npoints)
    if case == "lengths_only":
        kw = dict(lengths=lengths)
    if case == "npoints_only":
        kw = dict(npoints=npoints)
    if case == "geometry":
        call = lambda m: m(xyz, points, geometry=m.geometry(xyz, **kw), **kw)
    else:
        call = lambda m: m(xyz, points, **kw)
    off, on = _on_off(mod, call, "fused")
    for a, w in zip(on, off):                              # new_xyz, new_points, idx
        assert torch.equal(a, w)
    if "npoints" in kw:
        assert torch.equal(on[1][1, NPOINTS[1]:].view(torch.int32), torch.zeros_like(on[1][1, NPOINTS[1]:]).view(torch.int32))
    if "lengths" in kw:
        # NaN in the padding rows of the features: flag on == flag off on zero-filled padding
        nan_call = lambda m: (m(xyz, _with_padding(points, LENGTHS, float("nan")), geometry=m.geometry(xyz, **kw), **kw) if case == "geometry"
                              else m(xyz, _with_padding(points, LENGTHS, float("nan")), **kw))
        zero_points = _with_padding(points, LENGTHS, 0.0)
        with torch.no_grad():
            mod.fused_ragged_eval = True
            on_nan = nan_call(mod)
            assert mod.last_path == "fused_ragged"
            mod.fused_ragged_eval = False
            off_zero = mod(xyz, zero_points, geometry=mod.geometry(xyz, **kw), **kw) if case == "geometry" else mod(xyz, zero_points, **kw)
        assert torch.equal(on_nan[1], off_zero[1])


def test_sa_module_ragged_group_all(cuda):
    import pointnet2_amd.pointnet_util as U
    from pointnet2_amd import sa_mlp
    torch.manual_seed(1)
    mod = _stir(U.PointnetSAModule(6, None, None, None, [256, 256, 512], group_all=True).to(cuda))
    mod.ragged_group_all = True
    assert sa_mlp.kind(9, (256, 256, 512), N) == "cooperative"
    xyz, points = _clouds(cuda, 6)
    lengths, _ = _counts(cuda)
    (_, ref, _), (nx, out, _) = _on_off(mod, lambda m: m(xyz, points, lengths=lengths), "unfused")
    assert out.shape == (B, 1, 512) and torch.all(nx == 0)
    # two different evaluations: the bound of test_sa_mlp_gpu.py::test_group_all_module_takes_the_fused_kernel
    assert (out - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    with torch.no_grad():
        mod.fused_ragged_eval = True
        _, on_nan, _ = mod(_with_padding(xyz, LENGTHS, float("nan")), _with_padding(points, LENGTHS, float("nan")), lengths=lengths)
        assert mod.last_path == "fused_ragged"
    assert torch.equal(on_nan, out)                        # nothing beyond a length is looked at


def test_msg_module(cuda):
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(2)
    mod = _stir(U.PointnetSAModuleMSG(6, M, [0.3, 0.5], [16, 32], [[32, 32, 64], [32, 48, 64]]).to(cuda))
    assert mod.fused_ragged_eval is False
    xyz, points = _clouds(cuda, 6)
    lengths, npoints = _counts(cuda)
    off, on = _on_off(mod, lambda m: m(xyz, points, lengths=lengths, npoints=npoints), "fused")
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert torch.equal(on[1][2, NPOINTS[2]:].view(torch.int32), torch.zeros_like(on[1][2, NPOINTS[2]:]).view(torch.int32))
    with torch.no_grad():
        mod.fused_ragged_eval = True
        on_nan = mod(xyz, _with_padding(points, LENGTHS, float("nan")), lengths=lengths, npoints=npoints)
        assert mod.last_path == "fused_ragged"
        mod.fused_ragged_eval = False
        off_zero = mod(xyz, _with_padding(points, LENGTHS, 0.0), lengths=lengths, npoints=npoints)
    assert torch.equal(on_nan[1], off_zero[1])


@pytest.mark.parametrize("geometry", [False, True], ids=["level", "geometry"])
@pytest.mark.parametrize("c1", [6, 0])
def test_fp_module(cuda, geometry, c1):
    import pointnet2_amd as P
    import pointnet2_amd.pointnet_util as U
    torch.manual_seed(3)
    c2 = 32
    mod = _stir(U.PointnetFPModule(c2 + c1, [64, 64]).to(cuda))
    assert mod.fused_ragged_eval is False
    xyz1, points1 = _clouds(cuda, max(c1, 1))
    points1 = points1 if c1 else None
    xyz2, points2 = _clouds(cuda, c2, n=M)
    lengths1, lengths2 = _counts(cuda)

    def call(m, p1=points1, p2=points2):
        g = None
        if geometry:
            dist, idx = P.three_nn(xyz1, xyz2, lengths1=lengths1, lengths2=lengths2)
            g = U.FPGeometry(dist, idx, None)
        return m(xyz1, xyz2, p1, p2, geometry=g, lengths1=lengths1, lengths2=lengths2)

    off, on = _on_off(mod, call, "fused")
    assert torch.equal(on, off)
    assert torch.equal(on[1, LENGTHS[1]:].view(torch.int32), torch.zeros_like(on[1, LENGTHS[1]:]).view(torch.int32))
    nan1 = None if points1 is None else _with_padding(points1, LENGTHS, float("nan"))
    zero1 = None if points1 is None else _with_padding(points1, LENGTHS, 0.0)
    with torch.no_grad():
        mod.fused_ragged_eval = True
        on_nan = call(mod, nan1, _with_padding(points2, NPOINTS, float("nan")))
        assert mod.last_path == "fused_ragged"
        mod.fused_ragged_eval = False
        off_zero = call(mod, zero1, _with_padding(points2, NPOINTS, 0.0))
    assert torch.equal(on_nan, off_zero)
