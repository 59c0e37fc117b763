"""Ragged farthest-point sampling on every tier (pn2_farthest_point_sample_ragged_variant; set_fps_variant with lengths= /
npoints=): the batched and pruned tiers run their dense bodies on each cloud's slice inside the template of the PADDED n, so a
cloud may be one point in 8192 rank slots (DESIGN.md 4.11 "padding slots"; tests/test_fps_batch_padding_model.py is the CPU
model).

THE SLICE RULE, whatever the tier: cloud i's result is the oracle's on xyz[i:i+1, :lengths[i]] (truncated to npoints[i] where
counts are given; the rows from there on are index 0 and xyz[i, 0]). Expectations are computed once per case and shared by the
paddings and the variants. Each case runs under the two paddings of tests/test_ragged_gpu.py -- NaN, and the cloud's own points
offset by 1e3 (picked at once if read) --, once per variant that covers the padded n, through farthest_point_sample_gather and
farthest_point_sample."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

PADDINGS = ["nan", "adversarial"]
AUTO, FULL, PRUNED, BATCH = 0, 1, 2, 3
NAMES = {AUTO: "auto", FULL: "full", PRUNED: "pruned", BATCH: "batch"}


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def lens_t(v, cuda):
    return torch.tensor(v, dtype=torch.int32, device=cuda)


def padded(xyz, lengths, padding):
    out = xyz.copy()
    n = xyz.shape[1]
    for i, ni in enumerate(lengths):
        if ni < n:
            out[i, ni:] = np.nan if padding == "nan" else xyz[i, ni:] + np.float32(1e3)
    return out


def covering(n):
    """the variants whose rank-slot envelope holds the padded n (ranks = 512 ceil(n / 512))"""
    ranks = 512 * ((n + 511) // 512)
    return [FULL, AUTO] + ([BATCH] if 512 < ranks <= 8192 else []) + ([PRUNED] if 2048 < ranks <= 8192 else [])


@contextlib.contextmanager
def forced(variant):
    from pointnet2_amd import tf_sampling
    before = tf_sampling._FPS_VARIANT[0]
    tf_sampling.set_fps_variant(variant)
    try:
        yield
    finally:
        tf_sampling.set_fps_variant(before)


def nonfinite_clouds(b, n, seed):
    """Six uniform clouds with non-finite coordinates placed against the lengths of the "nonfinite" case below (a non-finite point
    keeps its start distance for ever and, once picked, is picked in every later round; tests/fps_cases.py): four kinds inside
    cloud 0; the ONLY one of cloud 1 just below its length and that of cloud 2 just beyond (cloud 2 is a finite cloud: the point
    is padding); cloud 3 starts on a NaN point (every sample 0); in cloud 4 it is the one point of the second rank; cloud 5 is
    exhausted (m > n_c) with the chain locked on its last point."""
    assert b == 6 and n == 4096
    nan, inf = float("nan"), float("inf")
    c = S.uniform_clouds(b, n, seed)
    for cloud_no, k, axis, value in [(0, 700, 0, nan), (0, 1030, 2, inf), (0, 3000, 1, -inf), (0, 518, 0, inf), (1, 2999, 1, nan),
                                     (2, 2049, 0, nan), (3, 0, 0, nan), (4, 512, 1, inf), (5, 36, 0, -inf)]:
        c[cloud_no, k, axis] = value
    return c


# name: (generator, padded n, lengths, m, npoints or None)
CASES = {
    # one case per batched-tier template; m = 300: AUTO takes the batched tier, m > n_c occurs
    "template_1024": (S.uniform_clouds, 1024, [1024, 700, 513, 512, 300, 64, 2, 1], 300, None),
    "template_2048": (S.uniform_clouds, 2048, [2048, 1537, 1025, 1024, 513, 100, 1], 300, None),
    "template_4096": (S.uniform_clouds, 4096, [4096, 3000, 2049, 2048, 1000, 513, 37, 1], 300, None),
    "template_8192": (S.uniform_clouds, 8192, [8192, 4097, 4096, 2048, 600, 1], 300, None),
    # ties and exhausted clouds under a large template
    "lattice": (S.lattice_clouds, 4096, [4096, 1500, 700], 900, None),
    "duplicated": (S.duplicated_clouds, 4096, [4096, 1500, 700], 500, None),
    "identical": (S.identical_clouds, 4096, [3000, 600, 1], 260, None),
    # per-cloud sample counts around PN2_BT_EARLY = 48
    "counts_early": (S.sphere_clouds, 4096, [4096, 37, 4096, 600, 2049, 100, 3000, 513], 320, [1, 2, 47, 48, 49, 255, 256, 320]),
    # the pruned tier: AUTO takes it at 8192 rank slots with 128 <= m < 256; forced at 4096
    "pruned_8192": (S.uniform_clouds, 8192, [8192, 5000, 4097, 4096, 1000, 1], 200, None),
    "pruned_4096": (S.sphere_clouds, 4096, [4096, 2049, 2048, 100], 130, None),
    "pruned_4096_counts": (S.sphere_clouds, 4096, [4096, 2049, 2048, 100], 130, [130, 1, 64, 129]),
    # non-finite points INSIDE the valid lengths, on all four variants (m = 300: AUTO takes the batched tier)
    "nonfinite": (nonfinite_clouds, 4096, [4096, 3000, 2049, 700, 513, 37], 300, None),
}
RUNS = [(name, v) for name in CASES for v in covering(CASES[name][1])]


@functools.lru_cache(maxsize=None)
def case(name):
    import oracle as O
    gen, n, lengths, m, npoints = CASES[name]
    xyz = gen(len(lengths), n, 31)
    want = np.zeros((len(lengths), m), dtype=np.int32)
    for i, ni in enumerate(lengths):
        mi = m if npoints is None else npoints[i]
        want[i, :mi] = O.farthest_point_sample(m, xyz[i:i + 1, :ni])[0][:mi]          # rows from m_i on: index 0
    want.setflags(write=False)
    xyz.setflags(write=False)
    return xyz, want


@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("name,variant", RUNS, ids=["%s-%s" % (n, NAMES[v]) for n, v in RUNS])
def test_every_tier_obeys_the_slice_rule(cuda, oracle, name, variant, padding):
    import pointnet2_amd as P
    _, n, lengths, m, npoints = CASES[name]
    xyz, want = case(name)
    x = dev(padded(xyz, lengths, padding), cuda)
    lens = lens_t(lengths, cuda)
    cnts = lens_t(npoints, cuda) if npoints is not None else None
    with forced(variant):
        idx, new_xyz = P.farthest_point_sample_gather(m, x, lengths=lens, npoints=cnts)
        idx2 = P.farthest_point_sample(m, x, lengths=lens, npoints=cnts)
    got = host(idx)
    assert (got >= 0).all() and (got < np.asarray(lengths)[:, None]).all()              # every index is < n_c
    assert np.array_equal(got, want), "first mismatch at %s" % np.argwhere(got != want)[:3].tolist()
    gathered = np.stack([xyz[i][want[i]] for i in range(len(lengths))])
    assert np.array_equal(bits(host(new_xyz)), bits(gathered))                           # the gathered slice, bit for bit
    assert np.array_equal(host(idx2), want)
    if npoints is not None:
        for i, mi in enumerate(npoints):                                                 # fill rows: index 0 and xyz[c, 0]
            assert (got[i, mi:] == 0).all()
            assert np.array_equal(bits(host(new_xyz)[i, mi:]), bits(np.broadcast_to(xyz[i, 0], (m - mi, 3))))


@pytest.mark.parametrize("n,m", [(1024, 300), (4096, 300), (8192, 200)])
def test_full_lengths_is_the_dense_operator_at_the_same_variant(cuda, n, m):
    import pointnet2_amd as P
    x = dev(S.sphere_clouds(3, n, 12), cuda)
    for variant in covering(n):
        with forced(variant):
            didx, dxyz = P.farthest_point_sample_gather(m, x)
            idx, new_xyz = P.farthest_point_sample_gather(m, x, lengths=[n] * 3)
            cidx, cxyz = P.farthest_point_sample_gather(m, x, lengths=[n] * 3, npoints=[m] * 3)
        assert torch.equal(idx, didx) and torch.equal(new_xyz, dxyz), NAMES[variant]
        assert torch.equal(cidx, didx) and torch.equal(cxyz, dxyz), NAMES[variant]


def test_a_forced_tier_outside_its_envelope_is_refused(cuda):
    import pointnet2_amd as P
    x = torch.zeros(2, 512, 3, device=cuda)
    for variant in (PRUNED, BATCH):
        with forced(variant), pytest.raises(ValueError):
            P.farthest_point_sample(4, x, lengths=[512, 3])


def test_capture_and_replay_with_new_counts(cuda):
    """one ragged AUTO call (the batched tier: 4096 rank slots, m = 320) captured once; lengths and npoints are rewritten in place;
    the replay equals the eager call on the new counts (the host never read them). Rows beyond the LARGER length hold NaN."""
    import pointnet2_amd as P
    first, second = ([4096, 700, 2049, 64], [320, 40, 7, 1]), ([900, 4096, 1, 2500], [3, 320, 64, 256])
    xyz = S.sphere_clouds(4, 4096, 53)
    x = dev(padded(xyz, [max(a, b) for a, b in zip(first[0], second[0])], "nan"), cuda)
    lens, cnts = lens_t(first[0], cuda), lens_t(first[1], cuda)

    def step():
        return P.farthest_point_sample_gather(320, x, lengths=lens, npoints=cnts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        old = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    lens.copy_(lens_t(second[0], cuda))
    cnts.copy_(lens_t(second[1], cuda))
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in captured]
    want = step()
    assert not all(torch.equal(g, o) for g, o in zip(got, old))                  # the replay did see the new counts
    assert torch.equal(got[0], want[0])
    assert np.array_equal(bits(host(got[1])), bits(host(want[1]))) and torch.isfinite(got[1]).all()


def test_sa_module_inherits_the_tier(cuda):
    """PointnetSAModule in eval() with lengths= and npoints=: forced FULL against AUTO (the batched tier at 1024 rank slots,
    npoint = 256), identical outputs -- the modules reach the tiers through _fps_ragged, no module code knows about them"""
    from pointnet2_amd.pointnet_util import PointnetSAModule
    torch.manual_seed(3)
    mod = PointnetSAModule(0, 256, 0.2, 16, [16, 16, 32]).to(cuda).eval()
    lengths, npoints = [1024, 700, 64], [256, 100, 30]
    x = dev(padded(S.sphere_clouds(3, 1024, 7), lengths, "adversarial"), cuda)
    outs = {}
    for variant in (FULL, AUTO):
        with forced(variant), torch.no_grad():
            outs[variant] = mod(x, None, lengths=lens_t(lengths, cuda), npoints=lens_t(npoints, cuda))
    assert len(outs[FULL]) == len(outs[AUTO])
    for a, b in zip(outs[FULL], outs[AUTO]):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b)


def _event_us(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in evs:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return float(np.median([s.elapsed_time(e) for s, e in evs])) * 1e3


def test_ragged_auto_is_the_batched_tier_at_the_metric_shape(cuda):
    """Tripwire for a silent fall-back to the register tier: the metric shape (32 x 4096 -> 1024) with every length = n, HIP-event
    medians of 10 runs as tests/test_perf_smoke_gpu.py takes them. Ragged PN2_FPS_FULL launches the register-tier kernel that was
    the only ragged kernel before the tiers were offered; the project's record (profiles/ragged/README.md: dense 196.9 us against
    ragged 398 us) puts AUTO / FULL at 0.49-0.54, a fall-back gives 1.0; 0.75 sits between the two with room for box-to-box spread."""
    import pointnet2_amd as P
    x = dev(S.sphere_clouds(32, 4096, 1000), cuda)
    lens = lens_t([4096] * 32, cuda)
    with forced(FULL):
        t_full = _event_us(lambda: P.farthest_point_sample_gather(1024, x, lengths=lens))
    with forced(AUTO):
        t_auto = _event_us(lambda: P.farthest_point_sample_gather(1024, x, lengths=lens))
    print("ragged FPS 32 x 4096 -> 1024, every length = n: AUTO %.1f us, FULL %.1f us, ratio %.3f" % (t_auto, t_full, t_auto / t_full))
    assert t_auto <= 0.75 * t_full, "ragged AUTO %.1f us against ragged FULL %.1f us" % (t_auto, t_full)
