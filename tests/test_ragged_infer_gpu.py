"""The fused inference MLPs with count arrays and the one-call ragged levels (include/pn2ops.h "ragged inference") on the GPU.
The oracle is the existing dense entry on each cloud's slices (itself pinned by test_sa_mlp_gpu.py / test_fp_mlp_gpu.py and the
exact-arithmetic probes): every row of the fused stacks is an independent fixed-order sum and the max pool is order-independent,
so every comparison is exact -- as int32 views, so that -0.0 on a padding row fails. All padding is poisoned: NaN in the rows of
xyz / points / points1 / points2 beyond a length and of new_xyz / dist beyond a count, and idx rows beyond a count name the
cloud's own padding rows (in bounds: a kernel that followed them would show NaN, not fault). Every case asserts the kernel
family it means to exercise."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _layers(rng, dims):
    return [((rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32),
             (0.1 * rng.standard_normal(dims[i + 1])).astype(np.float32)) for i in range(len(dims) - 1)]


def _clamp(counts, hi):
    return [min(max(int(c), 1), hi) for c in counts]


# ---- grouped set abstraction rows with npoints ------------------------------------------------------------------------------
def _grouped_inputs(cuda, seed, b, n, m, ns, cfeat, lengths, counts):
    """Random clouds with every padding row / entry poisoned for the (clamped) counts."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand((b, n, 3), generator=g)
    points = torch.randn((b, n, cfeat), generator=g) if cfeat else None
    new_xyz = torch.rand((b, m, 3), generator=g)
    idx = torch.zeros((b, m, ns), dtype=torch.int32)
    for c in range(b):
        L, k = lengths[c], counts[c]
        idx[c] = torch.randint(0, L, (m, ns), generator=g, dtype=torch.int32)
        xyz[c, L:] = NAN
        if points is not None:
            points[c, L:] = NAN
        new_xyz[c, k:] = NAN
        idx[c, k:] = torch.randint(L, n, (m - k, ns), generator=g, dtype=torch.int32) if L < n else n - 1
    dev = lambda t: None if t is None else t.to(cuda)
    return dev(xyz), dev(points), dev(new_xyz), dev(idx)


COUNT_SETS = ([9, 4, 1], [9, 9, 9], [0, 12, 5])           # the last one clamps to 1, 9, 5
BASE = dict(b=3, n=96, m=9, lengths=[96, 50, 7])

GROUPED = [  # family, cfeat, widths, nsample, resident variants
    ("resident", 0, (64, 64, 128), 16, (0, 1, 2)),
    ("resident", 0, (64, 64, 128), 32, (0, 1, 2)),
    ("resident", 0, (64, 64, 128), 64, (0,)),
    ("resident", 6, (64, 64, 128), 32, (0, 2)),
    ("streamed", 64, (128, 128, 256), 32, (0,)),
    ("streamed", 64, (128, 128, 256), 64, (0,)),
    ("cooperative", 64, (256, 256, 512), 32, (0,)),
    ("cooperative", 64, (256, 256, 512), 24, (0,)),
    ("cooperative", 64, (256, 256, 512), 64, (0,)),       # two parts and < 256 rows: the split route with padding units
]


def _check_grouped(cuda, family, cfeat, widths, ns, variants, b, n, m, lengths, count_sets):
    from pointnet2_amd import sa_mlp
    rng = np.random.default_rng(cfeat + ns)
    assert sa_mlp.kind(3 + cfeat, widths, ns) == family
    packed = sa_mlp.PackedMLP3(_layers(rng, (3 + cfeat,) + tuple(widths)), cuda, ns)
    assert packed.kind == family
    for raw in count_sets:
        counts = _clamp(raw, m)
        xyz, points, new_xyz, idx = _grouped_inputs(cuda, 7 + ns, b, n, m, ns, cfeat, lengths, counts)
        npoints = torch.tensor(raw, dtype=torch.int32, device=cuda)
        want = torch.zeros((b, m, widths[2]), dtype=torch.float32, device=cuda)
        for c in range(b):                                 # the dense entry on the cloud's slices alone
            L, k = lengths[c], counts[c]
            want[c, :k] = sa_mlp.sa_mlp_maxpool(xyz[c:c + 1, :L], new_xyz[c:c + 1, :k], None if points is None else points[c:c + 1, :L],
                                                idx[c:c + 1, :k], packed)[0]
        assert not torch.isnan(want).any()
        try:
            for variant in variants:
                sa_mlp.set_resident_variant(variant)
                for lens in (None, torch.tensor(lengths, dtype=torch.int32, device=cuda)):
                    got = sa_mlp.sa_mlp_maxpool(xyz, new_xyz, points, idx, packed, npoints=npoints, lengths=lens)
                    assert torch.equal(_bits(got), _bits(want)), (family, ns, raw, variant)
                if counts == [m] * b:                      # full counts: the dense entry on the whole batch
                    assert torch.equal(_bits(got), _bits(sa_mlp.sa_mlp_maxpool(xyz, new_xyz, points, idx, packed)))
        finally:
            sa_mlp.set_resident_variant(0)


@pytest.mark.parametrize("family,cfeat,widths,ns,variants", GROUPED, ids=["%s-c%d-ns%d" % (g[0], g[1], g[3]) for g in GROUPED])
def test_grouped_rows_with_npoints(cuda, family, cfeat, widths, ns, variants):
    """m = 9 is odd: at nsample 16 an item of the resident kernels straddles two clouds and a count boundary."""
    _check_grouped(cuda, family, cfeat, widths, ns, variants, count_sets=COUNT_SETS, **BASE)


MANY = [("resident", 0, (64, 64, 128), 32, (0, 1, 2)), ("resident", 0, (64, 64, 128), 16, (0, 1, 2)),
        ("streamed", 64, (128, 128, 256), 32, (0,)), ("cooperative", 64, (256, 256, 512), 32, (0,)),
        ("cooperative", 64, (256, 256, 512), 64, (0,))]


@pytest.mark.parametrize("family,cfeat,widths,ns,variants", MANY, ids=["%s-ns%d" % (g[0], g[3]) for g in MANY])
def test_grouped_rows_with_items_of_padding_only(cuda, family, cfeat, widths, ns, variants):
    """300 rows: the cooperative kernel's non-split route; most work items of clouds 1 and 2 are padding only."""
    _check_grouped(cuda, family, cfeat, widths, ns, variants, b=3, n=96, m=100, lengths=[96, 50, 7], count_sets=([100, 37, 1],))


# ---- group_all with lengths ----------------------------------------------------------------------------------------------------
def _group_all_case(cuda, widths, b, n, lengths, check):
    from pointnet2_amd import sa_mlp
    cfeat = 5
    rng = np.random.default_rng(widths[2] + b)
    g = torch.Generator().manual_seed(b + n)
    xyz, points = torch.rand((b, n, 3), generator=g), torch.randn((b, n, cfeat), generator=g)
    for c in range(b):
        xyz[c, lengths[c]:] = NAN
        points[c, lengths[c]:] = NAN
    xyz, points = xyz.to(cuda), points.to(cuda)
    assert sa_mlp.kind(3 + cfeat, widths, n) == "cooperative"
    packed = sa_mlp.PackedMLP3(_layers(rng, (3 + cfeat,) + tuple(widths)), cuda, n)
    got = sa_mlp.sa_mlp_maxpool(xyz, None, points, None, packed, lengths=torch.tensor(lengths, dtype=torch.int32, device=cuda))
    assert got.shape == (b, 1, widths[2]) and not torch.isnan(got).any()
    for c in check:
        L = lengths[c]
        assert sa_mlp.kind(3 + cfeat, widths, L) == "cooperative"          # one PackedMLP3 serves every slice (_same_kernel)
        want = sa_mlp.sa_mlp_maxpool(xyz[c:c + 1, :L], None, points[c:c + 1, :L], None, packed)
        assert torch.equal(_bits(got[c:c + 1]), _bits(want)), (widths, c, L)


@pytest.mark.parametrize("widths", [(256, 256, 512), (256, 512, 1024)], ids=["fused", "gemm_last"])
@pytest.mark.parametrize("lengths", [[200, 1, 31, 33, 64], [32, 20, 129, 160, 199]], ids=["a", "b"])
def test_group_all_with_lengths(cuda, widths, lengths):
    """b 5, n 200 (seven parts, split): a tail, a whole part, a part boundary +- 1, and a cloud whose valid parts end more than one
    GEMM chunk of four before the padded seven."""
    _group_all_case(cuda, widths, 5, 200, lengths, range(5))


def test_group_all_with_lengths_non_split_route(cuda):
    rng = np.random.default_rng(40)
    lengths = [int(v) for v in rng.integers(1, 41, 256)]
    lengths[0], lengths[1], lengths[255] = 1, 40, 33
    _group_all_case(cuda, (256, 256, 512), 256, 40, lengths, [0, 1, 2, 3, 100, 200, 254, 255])


# ---- feature propagation rows with lengths1 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1], ids=["streamed", "cooperative"])
@pytest.mark.parametrize("widths", [[256, 128], [128, 128, 128]], ids=["2layers", "3layers"])
@pytest.mark.parametrize("c1", [0, 6, 64])
def test_fp_rows_with_lengths1(cuda, kind, widths, c1):
    import pointnet2_amd as P
    from pointnet2_amd import _C, sa_mlp
    b, n, m, c2 = 4, 70, 20, 64
    lengths1, lengths2 = [70, 1, 32, 33], [20, 3, 7, 20]
    rng = np.random.default_rng(c1 + len(widths))
    arr = (ctypes.c_int * len(widths))(*widths)
    assert _C.lib().pn2_fp_mlp_config(c2, c1, len(widths), arr, kind, None, None, None) == 0
    packed = sa_mlp.PackedFPMLP(_layers(rng, [c2 + c1] + widths), c2, c1, cuda, kind)
    assert packed.kind == kind
    g = torch.Generator().manual_seed(c1)
    xyz1, xyz2 = torch.rand((b, n, 3), generator=g), torch.rand((b, m, 3), generator=g)
    points2 = torch.randn((b, m, c2), generator=g)
    points1 = torch.randn((b, n, c1), generator=g) if c1 else None
    for c in range(b):
        xyz1[c, lengths1[c]:] = NAN
        xyz2[c, lengths2[c]:] = NAN
        points2[c, lengths2[c]:] = NAN
        if points1 is not None:
            points1[c, lengths1[c]:] = NAN
    dev = lambda t: None if t is None else t.to(cuda)
    xyz1, xyz2, points1, points2 = dev(xyz1), dev(xyz2), dev(points1), dev(points2)
    l1 = torch.tensor(lengths1, dtype=torch.int32, device=cuda)
    l2 = torch.tensor(lengths2, dtype=torch.int32, device=cuda)
    dist, idx = P.three_nn(xyz1, xyz2, lengths1=l1, lengths2=l2)
    dist, idx = dist.clone(), idx.clone()
    for c in range(b):                                     # poison what the operator wrote on the padding rows
        dist[c, lengths1[c]:] = NAN
        idx[c, lengths1[c]:] = lengths2[c] if lengths2[c] < m else m - 1
    got = sa_mlp.fp_mlp(points2, points1, idx, dist, packed, lengths1=l1)
    want = torch.zeros_like(got)
    for c in range(b):
        L1, L2 = lengths1[c], lengths2[c]
        want[c, :L1] = sa_mlp.fp_mlp(points2[c:c + 1, :L2], None if points1 is None else points1[c:c + 1, :L1], idx[c:c + 1, :L1],
                                     dist[c:c + 1, :L1], packed)[0]
    assert not torch.isnan(want).any()
    assert torch.equal(_bits(got), _bits(want))


# ---- one call per ragged level -------------------------------------------------------------------------------------------------
LB, LN, LM, LNS, LR = 3, 300, 64, 32, 0.3


def _level_clouds(cuda):
    g = torch.Generator().manual_seed(5)
    return torch.rand((LB, LN, 3), generator=g).to(cuda), torch.randn((LB, LN, 6), generator=g).to(cuda)


def _sa_by_operators(xyz, points, packed, lengths, npoints):
    import pointnet2_amd as P
    from pointnet2_amd import sa_mlp
    fps_idx, new_xyz = P.farthest_point_sample_gather(LM, xyz, lengths=lengths, npoints=npoints)
    idx, cnt, grouped = P.query_ball_group_xyz(LR, LNS, xyz, new_xyz, True, lengths1=lengths, lengths2=npoints)
    out = sa_mlp.sa_mlp_maxpool(xyz, new_xyz, points, idx, packed, npoints=npoints, lengths=lengths)
    return new_xyz, out, idx, fps_idx, cnt, grouped


def test_sa_level_ragged_is_the_three_operators(cuda):
    from pointnet2_amd import sa_mlp
    xyz, points = _level_clouds(cuda)
    packed = sa_mlp.PackedMLP3(_layers(np.random.default_rng(1), (9, 64, 64, 128)), cuda, LNS)
    buffers = sa_mlp.LevelBuffers()
    for lens, cnts in (([300, 120, 33], [64, 20, 1]), ([64, 300, 299], [7, 64, 63])):      # the second call reuses the buffers
        lengths = torch.tensor(lens, dtype=torch.int32, device=cuda)
        npoints = torch.tensor(cnts, dtype=torch.int32, device=cuda)
        got = sa_mlp.sa_level_ragged(LM, LR, LNS, xyz, points, packed, lengths, npoints, buffers)
        want = _sa_by_operators(xyz, points, packed, lengths, npoints)
        assert len(got) == 6
        for a, w in zip(got, want):
            assert torch.equal(a, w)
    # a dense side is full counts
    got = sa_mlp.sa_level_ragged(LM, LR, LNS, xyz, points, packed, lengths, None)
    want = _sa_by_operators(xyz, points, packed, lengths, torch.full((LB,), LM, dtype=torch.int32, device=cuda))
    assert all(torch.equal(a, w) for a, w in zip(got, want))


def _fp_level_inputs(cuda):
    g = torch.Generator().manual_seed(6)
    xyz1, xyz2 = torch.rand((LB, LN, 3), generator=g).to(cuda), torch.rand((LB, LM, 3), generator=g).to(cuda)
    return xyz1, xyz2, torch.randn((LB, LN, 6), generator=g).to(cuda), torch.randn((LB, LM, 64), generator=g).to(cuda)


@pytest.mark.parametrize("kind", [0, 1], ids=["streamed", "cooperative"])
def test_fp_level_ragged_is_the_two_operators(cuda, kind):
    import pointnet2_amd as P
    from pointnet2_amd import sa_mlp
    xyz1, xyz2, points1, points2 = _fp_level_inputs(cuda)
    packed = sa_mlp.PackedFPMLP(_layers(np.random.default_rng(2), [70, 128, 128]), 64, 6, cuda, kind)
    buffers = sa_mlp.LevelBuffers()
    for lens1, lens2 in (([300, 120, 33], [64, 20, 3]), ([64, 300, 299], [7, 64, 63])):
        l1 = torch.tensor(lens1, dtype=torch.int32, device=cuda)
        l2 = torch.tensor(lens2, dtype=torch.int32, device=cuda)
        got = sa_mlp.fp_level_ragged(xyz1, xyz2, points1, points2, packed, l1, l2, buffers)
        dist, idx = P.three_nn(xyz1, xyz2, lengths1=l1, lengths2=l2)
        assert torch.equal(got, sa_mlp.fp_mlp(points2, points1, idx, dist, packed, lengths1=l1))
        assert torch.equal(got[1, lens1[1]:], torch.zeros_like(got[1, lens1[1]:]))
    got = sa_mlp.fp_level_ragged(xyz1, xyz2, points1, points2, packed, l1)                # a dense known side
    dist, idx = P.three_nn(xyz1, xyz2, lengths1=l1)
    assert torch.equal(got, sa_mlp.fp_mlp(points2, points1, idx, dist, packed, lengths1=l1))


def test_ragged_levels_in_a_captured_graph(cuda):
    """Packed first; one SA and one FP level captured on one stream; the counts are overwritten in place and the graph replayed."""
    from pointnet2_amd import sa_mlp
    xyz, points = _level_clouds(cuda)
    xyz1, xyz2, points1, points2 = _fp_level_inputs(cuda)
    sa_packed = sa_mlp.PackedMLP3(_layers(np.random.default_rng(1), (9, 64, 64, 128)), cuda, LNS)
    fp_packed = sa_mlp.PackedFPMLP(_layers(np.random.default_rng(2), [70, 128, 128]), 64, 6, cuda, 1)
    lengths = torch.tensor([300, 120, 33], dtype=torch.int32, device=cuda)
    npoints = torch.tensor([64, 20, 1], dtype=torch.int32, device=cuda)
    l1 = torch.tensor([300, 120, 33], dtype=torch.int32, device=cuda)
    l2 = torch.tensor([64, 20, 3], dtype=torch.int32, device=cuda)
    run = lambda: (sa_mlp.sa_level_ragged(LM, LR, LNS, xyz, points, sa_packed, lengths, npoints),
                   sa_mlp.fp_level_ragged(xyz1, xyz2, points1, points2, fp_packed, l1, l2))
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        run()                                              # eager warm-up on the capture stream
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sa_out, fp_out = run()
    lengths.copy_(torch.tensor([64, 300, 299], dtype=torch.int32))
    npoints.copy_(torch.tensor([7, 64, 63], dtype=torch.int32))
    l1.copy_(torch.tensor([10, 300, 150], dtype=torch.int32))
    l2.copy_(torch.tensor([64, 5, 40], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize(cuda)
    sa_want, fp_want = run()
    for a, w in zip(sa_out, sa_want):
        assert torch.equal(a, w)
    assert torch.equal(fp_out, fp_want)
