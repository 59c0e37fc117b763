"""Device tests of ragged farthest-point sampling beyond 16384 padded points (pn2_farthest_point_sample_large_ragged(_ex),
csrc/fps_large.hip and the global-memory kernel of csrc/fps.hip with counts; DESIGN.md 4.1e "with lengths").

THE SLICE RULE (tests/test_ragged_fps_tiers_gpu.py): cloud i's rows equal the oracle's on xyz[i:i+1, :lengths[i]], truncated to
npoints[i]; the rows from there on are index 0 and xyz[i, 0]. Expectations are computed once per case
(tests/fps_large_ragged_cases.py) and shared by the two paddings -- NaN, and the cloud's own points offset by 1e3 (picked at once
if read) --, the two kernels and the three group lengths. The short slices are those the CPU model has reproduced the oracle on
(tests/test_fps_large_ragged_model.py). Then: full lengths against the dense entries bit for bit, the Python operators under
set_fps_ragged_large, sample_and_group_xyz on a padded batch, a captured graph replayed over rewritten clouds and counts, and a
relative tripwire against the global-memory kernel."""
import contextlib

import numpy as np
import pytest
import torch

from fps_large_ragged_cases import CASES, TABLE_CASES, cloud, expected, lengths_of, slice_rule
from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

PADDINGS = ["nan", "adversarial"]
GENERIC, TIER = 1, 2
KERNELS = [(GENERIC, 256), (TIER, 64), (TIER, 128), (TIER, 256)]      # (kernel, group_len)


def dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)       # a copy: the shared clouds are read-only


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


def run(kernel, group_len, x, lens, cnts, m, want_xyz=True):
    """pn2_farthest_point_sample_large_ragged_ex (kernel None: the plain entry) into buffers no row of which may survive."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    b, n, _ = x.shape
    ws = torch.empty((lib.pn2_fps_large_ws_bytes(b, n),), dtype=torch.uint8, device=x.device)
    out = torch.full((b, m), -7, dtype=torch.int32, device=x.device)
    oxyz = torch.full((b, m, 3), float("nan"), dtype=torch.float32, device=x.device) if want_xyz else None
    if kernel is None:
        rc = lib.pn2_farthest_point_sample_large_ragged(b, n, m, ptr(x), ptr(lens), ptr(cnts), ptr(ws), ptr(out), ptr(oxyz), stream_ptr(x.device))
    else:
        rc = lib.pn2_farthest_point_sample_large_ragged_ex(kernel, group_len, b, n, m, ptr(x), ptr(lens), ptr(cnts), ptr(ws), ptr(out),
                                                           ptr(oxyz), stream_ptr(x.device))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, oxyz


def check_slice_rule(got, got_xyz, xyz, want, lengths, m, npoints):
    assert (got >= 0).all() and (got < np.asarray(lengths)[:, None]).all()               # every index is < n_c
    assert np.array_equal(got, want), "first mismatch at %s" % np.argwhere(got != want)[:3].tolist()
    if got_xyz is not None:
        gathered = np.stack([xyz[i][want[i]] for i in range(len(lengths))])
        assert np.array_equal(bits(got_xyz), bits(gathered))                             # the gathered slice, bit for bit
    if npoints is not None:
        for i, mi in enumerate(npoints):                                                 # fill rows: index 0 and xyz[c, 0]
            assert (got[i, mi:] == 0).all()
            if got_xyz is not None:
                assert np.array_equal(bits(got_xyz[i, mi:]), bits(np.broadcast_to(xyz[i, 0], (m - mi, 3))))


# a case without lengths has no padding rows: one padding is enough
RUNS = [(name, pad) for name in CASES for pad in (PADDINGS if CASES[name][3] is not None else PADDINGS[:1])]


@pytest.mark.parametrize("kernel,group_len", KERNELS, ids=["generic", "tier64", "tier128", "tier256"])
@pytest.mark.parametrize("name,padding", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_every_kernel_obeys_the_slice_rule(cuda, oracle, name, padding, kernel, group_len):
    _, _, n, given, m, npoints = CASES[name]
    lengths = lengths_of(name)
    xyz, want = cloud(name), expected(name)
    x = dev(padded(xyz, lengths, padding), cuda)
    cnts = lens_t(npoints, cuda) if npoints is not None else None
    out, oxyz = run(kernel, group_len, x, lens_t(lengths, cuda), cnts, m)
    check_slice_rule(host(out), host(oxyz), xyz, want, lengths, m, npoints)


@pytest.mark.parametrize("kernel,group_len", [(GENERIC, 256), (TIER, 64)], ids=["generic", "tier64"])
@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_the_whole_group_table_beside_shorter_slices(cuda, oracle, name, kernel, group_len):
    """4096 groups in one workgroup, 2049, 1094 and 1 in its neighbours (tests/fps_large_ragged_cases.py, TABLE_CASES)."""
    _, _, n, lengths, m, npoints = TABLE_CASES[name]
    xyz, want = cloud(name), expected(name)
    x = dev(padded(xyz, lengths, "nan"), cuda)
    out, oxyz = run(kernel, group_len, x, lens_t(lengths, cuda), None, m)
    check_slice_rule(host(out), host(oxyz), xyz, want, lengths, m, npoints)


def test_the_plain_entry_and_a_null_out_xyz(cuda, oracle):
    """_ex(0, 256, ...): the size rule on the padded extents -- the global-memory kernel at (20000, 128), the tier at (17000, 300)."""
    from pointnet2_amd import _C
    assert _C.lib().pn2_fps_large_pays(20000, 128) == 0 and _C.lib().pn2_fps_large_pays(17000, 300) == 1
    for name in ("counts", "lattice"):
        _, _, n, _, m, npoints = CASES[name]
        lengths = lengths_of(name)
        x = dev(padded(cloud(name), lengths, "nan"), cuda)
        cnts = lens_t(npoints, cuda) if npoints is not None else None
        for want_xyz in (True, False):
            out, oxyz = run(None, None, x, lens_t(lengths, cuda), cnts, m, want_xyz)
            assert (oxyz is None) == (not want_xyz)
            check_slice_rule(host(out), host(oxyz) if want_xyz else None, cloud(name), expected(name), lengths, m, npoints)


def test_full_lengths_is_the_dense_entry_bit_for_bit(cuda):
    """kernel 2 against pn2_farthest_point_sample_large, kernel 1 against pn2_farthest_point_sample_gather; with and without a
    full npoints."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    b, n, m = 3, 17000, 96
    x = dev(S.sphere_clouds(b, n, 1311), cuda)
    st = stream_ptr(cuda)
    ws = torch.empty((lib.pn2_fps_large_ws_bytes(b, n),), dtype=torch.uint8, device=cuda)
    temp = torch.empty((lib.pn2_fps_temp_floats(b, n),), dtype=torch.float32, device=cuda)
    dense = {}
    for kernel in (GENERIC, TIER):
        out = torch.full((b, m), -7, dtype=torch.int32, device=cuda)
        oxyz = torch.full((b, m, 3), float("nan"), dtype=torch.float32, device=cuda)
        if kernel == TIER:
            assert lib.pn2_farthest_point_sample_large(b, n, m, ptr(x), ptr(ws), ptr(out), ptr(oxyz), st) == 0
        else:
            assert lib.pn2_farthest_point_sample_gather(b, n, m, ptr(x), ptr(temp), ptr(out), ptr(oxyz), st) == 0
        torch.cuda.synchronize()
        dense[kernel] = (out, oxyz)
    assert torch.equal(dense[GENERIC][0], dense[TIER][0])
    full_n, full_m = lens_t([n] * b, cuda), lens_t([m] * b, cuda)
    for kernel in (GENERIC, TIER):
        for cnts in (None, full_m):
            out, oxyz = run(kernel, 256, x, full_n, cnts, m)
            assert torch.equal(out, dense[kernel][0]), kernel
            assert np.array_equal(bits(host(oxyz)), bits(host(dense[kernel][1]))), kernel


@contextlib.contextmanager
def switches(ragged_large, large=None, variant=0):
    from pointnet2_amd import tf_sampling as T
    before = (T._FPS_RAGGED_LARGE[0], T._FPS_LARGE[0], T._FPS_VARIANT[0])
    T.set_fps_ragged_large(ragged_large)
    T.set_fps_large(large)
    T.set_fps_variant(variant)
    try:
        yield
    finally:
        T.set_fps_ragged_large(before[0])
        T.set_fps_large(before[1])
        T.set_fps_variant(before[2])


def test_the_python_operators_under_the_switch(cuda, oracle):
    import pointnet2_amd as P
    name = "counts"
    _, _, n, _, m, npoints = CASES[name]
    lengths = lengths_of(name)
    xyz, want = cloud(name), expected(name)
    x = dev(padded(xyz, lengths, "adversarial"), cuda)
    lens, cnts = lens_t(lengths, cuda), lens_t(npoints, cuda)
    want_lengths_only = slice_rule(oracle, xyz, lengths, m)
    want_counts_only = expected("counts_full")
    got = {}
    for mode in (None, True, False):
        with switches(True, mode):
            idx = P.farthest_point_sample(m, x, lengths=lens, npoints=cnts)
            pre = torch.full((len(lengths), m), -1, dtype=torch.int32, device=cuda)
            ret = P.farthest_point_sample(m, x, out=pre, lengths=lens, npoints=cnts)
            assert ret is pre or ret.data_ptr() == pre.data_ptr()                         # out= honoured
            gidx, gxyz = P.farthest_point_sample_gather(m, x, lengths=lens, npoints=cnts)
            assert not getattr(gxyz, "_pn2_fps_ordered", False)                           # fill rows break the farthest-point order
            lidx, lxyz = P.farthest_point_sample_gather(m, x, lengths=lens)
            assert getattr(lxyz, "_pn2_fps_ordered", False)                               # the hint, as on the existing ragged route
            cidx = P.farthest_point_sample(m, dev(xyz, cuda), npoints=cnts)               # npoints alone: full counts stand in
            got[mode] = (idx, pre, gidx, gxyz, lidx, lxyz, cidx)
    for mode, (idx, pre, gidx, gxyz, lidx, lxyz, cidx) in got.items():
        check_slice_rule(host(gidx), host(gxyz), xyz, want, lengths, m, npoints)
        check_slice_rule(host(lidx), host(lxyz), xyz, want_lengths_only, lengths, m, None)
        assert torch.equal(idx, gidx) and torch.equal(pre, gidx), mode
        assert np.array_equal(host(cidx), want_counts_only), mode
        for a, b in zip(got[mode], got[False]):                                           # all modes give the same tensors
            assert np.array_equal(bits(host(a)) if a.dtype == torch.float32 else host(a),
                                  bits(host(b)) if b.dtype == torch.float32 else host(b)), mode
    # the switch off: today's refusal, for every form of the call
    with switches(False):
        for kw in (dict(lengths=lens), dict(npoints=cnts), dict(lengths=lens, npoints=cnts)):
            with pytest.raises(ValueError, match="at most 16384"):
                P.farthest_point_sample(m, x, **kw)
            with pytest.raises(ValueError, match="at most 16384"):
                P.farthest_point_sample_gather(m, x, **kw)
    # a forced tier keeps the limit with the switch on
    for variant in (1, 2, 3):
        with switches(True, None, variant), pytest.raises(ValueError, match="at most 16384"):
            P.farthest_point_sample(m, x, lengths=lens)
    # beyond the new envelope: refused by name, before any launch
    big = torch.empty((1, 1048577, 3), dtype=torch.float32, device=cuda)
    with switches(True), pytest.raises(ValueError, match="at most 1048576"):
        P.farthest_point_sample(4, big, lengths=[5])


def test_sample_and_group_xyz_on_a_padded_batch(cuda):
    """Two clouds padded to 17000 points through sample_and_group_xyz(..., lengths=, npoints=): cloud by cloud the dense
    operators on the slice pair, the documented fills beyond (sample 0 repeated; idx 0, pts_cnt 0, grouped_xyz +0.0)."""
    import pointnet2_amd as P
    n, lengths, m, npoints, radius, ns = 17000, [17000, 9000], 64, [64, 40], 0.2, 16
    xyz = S.sphere_clouds(2, n, 1312)
    x = dev(padded(xyz, lengths, "nan"), cuda)
    with switches(True):
        fps_idx, new_xyz, idx, cnt, grouped = P.sample_and_group_xyz(m, radius, ns, x, lengths=lens_t(lengths, cuda),
                                                                     npoints=lens_t(npoints, cuda))
    for i, (ni, mi) in enumerate(zip(lengths, npoints)):
        xi = dev(xyz[i:i + 1, :ni], cuda)
        didx, dxyz = P.farthest_point_sample_gather(mi, xi)
        qidx, qcnt, qgrouped = P.query_ball_group_xyz(radius, ns, xi, dxyz, True)
        assert torch.equal(fps_idx[i, :mi], didx[0])
        assert np.array_equal(bits(host(new_xyz[i, :mi])), bits(host(dxyz[0])))
        assert torch.equal(idx[i, :mi], qidx[0]) and torch.equal(cnt[i, :mi], qcnt[0])
        assert np.array_equal(bits(host(grouped[i, :mi])), bits(host(qgrouped[0])))
        assert (host(fps_idx[i, mi:]) == 0).all() and (host(idx[i, mi:]) == 0).all() and (host(cnt[i, mi:]) == 0).all()
        assert np.array_equal(bits(host(new_xyz[i, mi:])), bits(np.broadcast_to(xyz[i, 0], (m - mi, 3))))
        assert (bits(host(grouped[i, mi:])) == 0).all()


@pytest.mark.parametrize("kernel", [GENERIC, TIER], ids=["generic", "tier"])
def test_one_kernel_node_replayed_over_rewritten_clouds_and_counts(cuda, oracle, kernel):
    """The entry inside a captured graph: no memset node, no host read, nothing kept between launches beyond the caller's
    workspace. Replayed three times with the cloud, lengths and npoints rewritten on the device in between; each replay equals
    the oracle on the new slices."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    b, n, m = 3, 18000, 96
    rounds = [(1321, [18000, 300, 16385], [96, 96, 1]), (1322, [64, 18000, 9000], [50, 2, 96]), (1323, [16641, 1, 18000], [96, 7, 33])]
    x = torch.zeros((b, n, 3), dtype=torch.float32, device=cuda)
    lens = lens_t([n] * b, cuda)
    cnts = lens_t([m] * b, cuda)
    ws = torch.empty((lib.pn2_fps_large_ws_bytes(b, n),), dtype=torch.uint8, device=cuda)
    out = torch.zeros((b, m), dtype=torch.int32, device=cuda)
    oxyz = torch.zeros((b, m, 3), dtype=torch.float32, device=cuda)

    def call():
        assert lib.pn2_farthest_point_sample_large_ragged_ex(kernel, 256, b, n, m, ptr(x), ptr(lens), ptr(cnts), ptr(ws), ptr(out),
                                                             ptr(oxyz), stream_ptr(cuda)) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for seed, lengths, npoints in rounds:
        xyz = S.uniform_clouds(b, n, seed)
        x.copy_(dev(padded(xyz, lengths, "nan"), cuda))
        lens.copy_(lens_t(lengths, cuda))
        cnts.copy_(lens_t(npoints, cuda))
        out.fill_(-1)
        oxyz.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        check_slice_rule(host(out), host(oxyz), xyz, slice_rule(oracle, xyz, lengths, m, npoints), lengths, m, npoints)


def test_not_slower_than_the_global_memory_kernel(cuda):
    """Relative tripwire at b = 2, uniform 131072 -> 512, lengths [131072, 70000]: the median of five alternating timings of
    kernel 2 is not above kernel 1's in the same process (the dense ratio at this shape is 2.5-3.5 x: the margin is the tier's
    own advantage)."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    b, n, m = 2, 131072, 512
    lengths = [131072, 70000]
    x = dev(padded(S.uniform_clouds(b, n, 1331), lengths, "nan"), cuda)
    lens = lens_t(lengths, cuda)
    ws = [torch.empty((lib.pn2_fps_large_ws_bytes(b, n),), dtype=torch.uint8, device=cuda) for _ in range(2)]
    out = [torch.zeros((b, m), dtype=torch.int32, device=cuda) for _ in range(2)]
    oxyz = [torch.zeros((b, m, 3), dtype=torch.float32, device=cuda) for _ in range(2)]
    st = stream_ptr(cuda)

    def generic():
        assert lib.pn2_farthest_point_sample_large_ragged_ex(GENERIC, 256, b, n, m, ptr(x), ptr(lens), None, ptr(ws[0]), ptr(out[0]),
                                                             ptr(oxyz[0]), st) == 0

    def tier():
        assert lib.pn2_farthest_point_sample_large_ragged_ex(TIER, 256, b, n, m, ptr(x), ptr(lens), None, ptr(ws[1]), ptr(out[1]),
                                                             ptr(oxyz[1]), st) == 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    generic(); tier()
    torch.cuda.synchronize()
    tg, tt = [], []
    for _ in range(5):
        tg.append(timed(generic))
        tt.append(timed(tier))
    assert torch.equal(out[0], out[1]) and np.array_equal(bits(host(oxyz[0])), bits(host(oxyz[1])))
    assert (host(out[1])[1] < lengths[1]).all()
    print("kernel 1 %.3f ms, kernel 2 %.3f ms (medians of 5)" % (np.median(tg), np.median(tt)))
    assert np.median(tt) <= np.median(tg)
