"""Device tests of packed farthest-point sampling beyond 16384 points per cloud (pn2_farthest_point_sample_large_packed(_ex):
csrc/fps_large.hip's packed kernel with its short-cloud body, and the global-memory kernel of csrc/fps.hip in the packed mode;
DESIGN.md 4.1e "packed").

THE SLICE RULE: cloud c's rows equal the oracle's on its slice of the flat array (plus offsets[c] with global_idx), out_xyz is the
gathered slice bit for bit. The batches are those of tests/fps_large_ragged_cases.py laid back to back -- all clouds lie in one
unit cube, so a read across a slab boundary changes a result, and the lengths put slabs at odd rows; the cases with npoints are
used with their lengths only. Then: the short body's boundaries, a workspace sentinel that shows which body ran, the padded entry
bit for bit, a captured graph replayed over rewritten offsets, the Python operators, and a relative tripwire for the short body."""
import contextlib

import numpy as np
import pytest
import torch

from fps_large_ragged_cases import CASES, cloud, expected, lengths_of, slice_rule
from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

GENERIC, TIER = 1, 2
CHOICES = [(GENERIC, 256, 0), (TIER, 64, 0), (TIER, 128, 0), (TIER, 256, 0), (TIER, 256, 8192)]     # (kernel, group_len, short_max)
CHOICE_IDS = ["generic", "tier64", "tier128", "tier256", "tier256_short8192"]
SHORT_LENGTHS = [8193, 8192, 8191, 4097, 2049, 1025, 1024, 1023, 65, 1, 17000]                     # around every slot count of the short body
SHORT_M = 96


def dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pack(xyz, lengths):
    """-> flat (total, 3) float32 and offsets (b + 1,) int32: cloud i is xyz[i, :lengths[i]]"""
    flat = np.concatenate([xyz[i, :ni] for i, ni in enumerate(lengths)]).astype(np.float32)
    return flat, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def run(choice, flat, offs, nmax, m, global_idx=0, want_xyz=True, ws=None):
    """pn2_farthest_point_sample_large_packed_ex (choice None: the plain entry) into buffers no row of which may survive."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    b, total = offs.shape[0] - 1, flat.shape[0]
    if ws is None:
        ws = torch.empty((lib.pn2_fps_large_packed_ws_bytes(total),), dtype=torch.uint8, device=flat.device)
    out = torch.full((b, m), -7, dtype=torch.int32, device=flat.device)
    oxyz = torch.full((b, m, 3), float("nan"), dtype=torch.float32, device=flat.device) if want_xyz else None
    tail = (b, total, nmax, m, ptr(flat), ptr(offs), global_idx, ptr(ws), ptr(out), ptr(oxyz), stream_ptr(flat.device))
    rc = lib.pn2_farthest_point_sample_large_packed(*tail) if choice is None else lib.pn2_farthest_point_sample_large_packed_ex(*choice, *tail)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, oxyz


def check(got, got_xyz, xyz, want, lengths, offsets=None):
    """xyz: (b, n, 3); offsets: the bases the indices carry (global_idx) or None"""
    local = got - (np.asarray(offsets[:-1])[:, None] if offsets is not None else 0)
    assert (local >= 0).all() and (local < np.asarray(lengths)[:, None]).all()           # every index inside its own slab
    assert np.array_equal(local, want), "first mismatch at %s" % np.argwhere(local != want)[:3].tolist()
    if got_xyz is not None:
        gathered = np.stack([xyz[i][want[i]] for i in range(len(lengths))])
        assert np.array_equal(bits(got_xyz), bits(gathered))                             # the gathered slice, bit for bit


_NO_COUNTS = {}


def expected_for_lengths(oracle, name):
    """the case's expectation; a case with npoints is used with its lengths only: every cloud yields m samples"""
    if CASES[name][5] is None:
        return expected(name)
    if name not in _NO_COUNTS:
        _NO_COUNTS[name] = slice_rule(oracle, cloud(name), lengths_of(name), CASES[name][4])
    return _NO_COUNTS[name]


@pytest.mark.parametrize("global_idx", [0, 1])
@pytest.mark.parametrize("choice", CHOICES, ids=CHOICE_IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_kernel_obeys_the_slice_rule(cuda, oracle, name, choice, global_idx):
    _, _, n, _, m, _ = CASES[name]
    lengths = lengths_of(name)
    xyz, want = cloud(name), expected_for_lengths(oracle, name)
    flat, offs = pack(xyz, lengths)
    x, o = dev(flat, cuda), dev(offs, cuda)
    out, oxyz = run(choice, x, o, n, m, global_idx)
    check(host(out), host(oxyz), xyz, want, lengths, offs if global_idx else None)
    out2, none = run(choice, x, o, n, m, global_idx, want_xyz=False)                      # a NULL out_xyz: the same indices
    assert none is None and torch.equal(out, out2)


_SHORT = {}


def short_batch(oracle):
    """uniform clouds of SHORT_LENGTHS points in one unit cube and their oracle samples: computed once"""
    if not _SHORT:
        xyz = S.uniform_clouds(len(SHORT_LENGTHS), max(SHORT_LENGTHS), 1341)
        _SHORT["xyz"] = xyz
        _SHORT["want"] = slice_rule(oracle, xyz, SHORT_LENGTHS, SHORT_M)
        _SHORT["flat"], _SHORT["offs"] = pack(xyz, SHORT_LENGTHS)
    return _SHORT["xyz"], _SHORT["want"], _SHORT["flat"], _SHORT["offs"]


@pytest.mark.parametrize("global_idx", [0, 1])
@pytest.mark.parametrize("short_max", [0, 1024, 8192])
def test_short_body_boundaries(cuda, oracle, short_max, global_idx):
    """clouds of 8193 / 8192 / 8191 points (the capacity), around every multiple of 1024 the body's slot loop stops at, 65, 1, and
    a long one: with the threshold at 0 (all by the cell-sorted body), 1024 and 8192"""
    xyz, want, flat, offs = short_batch(oracle)
    out, oxyz = run((TIER, 256, short_max), dev(flat, cuda), dev(offs, cuda), 17000, SHORT_M, global_idx)
    check(host(out), host(oxyz), xyz, want, SHORT_LENGTHS, offs if global_idx else None)


def test_the_plain_entry(cuda, oracle):
    """_ex(0, 256, -1, ...): the size rule on nmax and m, the library's short-cloud rule"""
    xyz, want, flat, offs = short_batch(oracle)
    for global_idx in (0, 1):
        out, oxyz = run(None, dev(flat, cuda), dev(offs, cuda), 17000, SHORT_M, global_idx)
        check(host(out), host(oxyz), xyz, want, SHORT_LENGTHS, offs if global_idx else None)


def test_the_short_body_ran_and_touches_no_workspace(cuda, oracle):
    """The workspace is filled with a sentinel byte first. short_max = 8192: the record rows AND the distance rows of every cloud
    of at most 8192 points still hold it afterwards; short_max = 0: every record row of such a cloud was written. Rows of the
    longer clouds are written in both runs."""
    from pointnet2_amd import _C
    xyz, want, flat, offs = short_batch(oracle)
    total = flat.shape[0]
    assert _C.lib().pn2_fps_large_packed_ws_bytes(total) == 20 * total
    x, o = dev(flat, cuda), dev(offs, cuda)
    for short_max in (8192, 0):
        ws = torch.full((20 * total,), 0xA5, dtype=torch.uint8, device=cuda)
        out, _ = run((TIER, 256, short_max), x, o, 17000, SHORT_M, ws=ws)
        check(host(out), None, xyz, want, SHORT_LENGTHS)
        w = host(ws)
        recs, md = w[:16 * total].reshape(total, 16), w[16 * total:].reshape(total, 4)
        for c, nc in enumerate(SHORT_LENGTHS):
            r, d = recs[offs[c]:offs[c + 1]], md[offs[c]:offs[c + 1]]
            if nc <= 8192 and short_max == 8192:
                assert (r == 0xA5).all() and (d == 0xA5).all(), (short_max, nc)
            else:                                              # a record is {x, y, z, k}: k < 17000 never has the sentinel's bytes
                assert (r != 0xA5).any(axis=1).all(), (short_max, nc)
                assert (d != 0xA5).any(axis=1).all(), (short_max, nc)


@pytest.mark.parametrize("kernel", [GENERIC, TIER], ids=["generic", "tier"])
def test_equals_the_padded_entry_bit_for_bit(cuda, kernel):
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    name = "boundaries"
    _, _, n, _, m, _ = CASES[name]
    lengths = lengths_of(name)
    xyz = cloud(name)
    b = len(lengths)
    pad = xyz.copy()
    for i, ni in enumerate(lengths):
        pad[i, ni:] = np.nan
    xp, lens = dev(pad, cuda), torch.tensor(lengths, dtype=torch.int32, device=cuda)
    ws = torch.empty((lib.pn2_fps_large_ws_bytes(b, n),), dtype=torch.uint8, device=cuda)
    wout = torch.full((b, m), -7, dtype=torch.int32, device=cuda)
    wxyz = torch.full((b, m, 3), float("nan"), dtype=torch.float32, device=cuda)
    assert lib.pn2_farthest_point_sample_large_ragged_ex(kernel, 256, b, n, m, ptr(xp), ptr(lens), None, ptr(ws), ptr(wout), ptr(wxyz),
                                                         stream_ptr(cuda)) == 0
    torch.cuda.synchronize()
    flat, offs = pack(xyz, lengths)
    for short_max in ((0, 8192) if kernel == TIER else (0,)):
        out, oxyz = run((kernel, 256, short_max), dev(flat, cuda), dev(offs, cuda), n, m)
        assert torch.equal(out, wout)
        assert np.array_equal(bits(host(oxyz)), bits(host(wxyz)))


@pytest.mark.parametrize("choice", [(GENERIC, 256, 0), (TIER, 256, 8192)], ids=["generic", "tier_short8192"])
def test_one_kernel_node_replayed_over_rewritten_offsets(cuda, oracle, choice):
    """The entry inside a captured graph: no memset node, no host read of offsets. Replayed three times with the flat array and
    offsets rewritten in place (total fixed); cloud 0 goes from the cell-sorted body to the short body (18000 -> 9000 -> 1 points),
    cloud 1 the other way (300 -> 7685 -> 16684). Each replay equals the oracle on the new slices."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    b, nmax, m, total = 3, 18000, 96, 34685
    rounds = [(1351, [18000, 300, 16385]), (1352, [9000, 7685, 18000]), (1353, [1, 16684, 18000])]
    assert all(sum(c) == total for _, c in rounds)
    flat = torch.zeros((total, 3), dtype=torch.float32, device=cuda)
    offs = dev(np.array([0, 12000, 24000, total], dtype=np.int32), cuda)
    ws = torch.empty((lib.pn2_fps_large_packed_ws_bytes(total),), dtype=torch.uint8, device=cuda)
    out = torch.zeros((b, m), dtype=torch.int32, device=cuda)
    oxyz = torch.zeros((b, m, 3), dtype=torch.float32, device=cuda)

    def call():
        assert lib.pn2_farthest_point_sample_large_packed_ex(*choice, b, total, nmax, m, ptr(flat), ptr(offs), 1, ptr(ws), ptr(out),
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
    for seed, counts in rounds:
        xyz = S.uniform_clouds(b, nmax, seed)
        f, o = pack(xyz, counts)
        flat.copy_(dev(f, cuda))
        offs.copy_(dev(o, cuda))
        out.fill_(-1)
        oxyz.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        check(host(out), host(oxyz), xyz, slice_rule(oracle, xyz, counts, m), counts, o)


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
    name = "lattice"                                                                      # ties: every route must break them alike
    _, _, n, _, m, _ = CASES[name]
    lengths = lengths_of(name)
    xyz, want = cloud(name), expected(name)
    f, o = pack(xyz, lengths)
    flat, offs = dev(f, cuda), dev(o, cuda)
    got = {}
    for mode in (None, True, False):
        with switches(True, mode):
            idx = P.farthest_point_sample(m, flat, offsets=offs, max_points=n)
            pre = torch.full((len(lengths), m), -1, dtype=torch.int32, device=cuda)
            ret = P.farthest_point_sample(m, flat, out=pre, offsets=offs, max_points=n)
            assert ret is pre or ret.data_ptr() == pre.data_ptr()                         # out= honoured
            gidx, gxyz = P.farthest_point_sample_gather(m, flat, offsets=offs, max_points=n)
            assert getattr(gxyz, "_pn2_fps_ordered", False)                               # the ordered hint is set
            glob = P.farthest_point_sample(m, flat, offsets=offs, max_points=n, global_idx=True)
            got[mode] = (idx, pre, gidx, gxyz, glob)
    for mode, (idx, pre, gidx, gxyz, glob) in got.items():
        check(host(gidx), host(gxyz), xyz, want, lengths)
        check(host(glob), None, xyz, want, lengths, o)
        assert torch.equal(idx, gidx) and torch.equal(pre, gidx), mode
        for a, b in zip(got[mode], got[False]):                                           # all modes give the same tensors
            assert np.array_equal(bits(host(a)) if a.dtype == torch.float32 else host(a),
                                  bits(host(b)) if b.dtype == torch.float32 else host(b)), mode
    with switches(False), pytest.raises(ValueError, match="at most 16384 points per cloud"):
        P.farthest_point_sample(m, flat, offsets=offs, max_points=n)
    for variant in (1, 2, 3):
        with switches(True, None, variant), pytest.raises(ValueError, match="at most 16384 points per cloud"):
            P.farthest_point_sample(m, flat, offsets=offs, max_points=n)
    with switches(True), pytest.raises(ValueError, match="at most 1048576 points per cloud"):
        P.farthest_point_sample(m, flat, offsets=offs, max_points=1048577)


def test_sample_and_group_on_a_packed_batch(cuda):
    """Two clouds of 17000 and 9000 points through sample_and_group(..., offsets=, max_points=17000): cloud by cloud the dense
    operators on the slice (idx carries the slab's first row)."""
    import pointnet2_amd as P
    from pointnet2_amd.pointnet_util import sample_and_group
    counts, m, radius, ns = [17000, 9000], 64, 0.2, 16
    xyz = S.sphere_clouds(2, 17000, 1361)
    f, o = pack(xyz, counts)
    flat, offs = dev(f, cuda), dev(o, cuda)
    feats = torch.rand((flat.shape[0], 5), generator=torch.Generator().manual_seed(4)).to(cuda)
    with switches(True):
        new_xyz, new_points, idx, grouped = sample_and_group(m, radius, ns, flat, feats, offsets=offs, max_points=17000)
    for i, ni in enumerate(counts):
        xi = dev(xyz[i:i + 1, :ni], cuda)
        didx, dxyz = P.farthest_point_sample_gather(m, xi)
        qidx, qcnt, qgrouped = P.query_ball_group_xyz(radius, ns, xi, dxyz, True)
        assert np.array_equal(bits(host(new_xyz[i])), bits(host(dxyz[0])))
        assert torch.equal(idx[i], qidx[0] + int(o[i]))
        assert np.array_equal(bits(host(grouped[i])), bits(host(qgrouped[0])))
        fi = feats[int(o[i]):int(o[i + 1])]
        want_points = torch.cat([qgrouped[0], fi[qidx[0].long()]], dim=-1)                # xyz first, then the features
        assert np.array_equal(bits(host(new_points[i])), bits(host(want_points)))


def test_the_short_body_is_not_slower_than_the_cell_sorted_body(cuda):
    """Relative tripwire at b = 2 clouds of 2048 points, nmax = 20000, m = 256: the median of five alternating timings with
    short_max = 8192 is not above that with short_max = 0 in the same process (the measured ratio at this shape is in
    profiles/fps_large_packed/README.md: the margin is the body's own advantage)."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    b, nc, nmax, m = 2, 2048, 20000, 256
    xyz = S.uniform_clouds(b, nc, 1371)
    f, o = pack(xyz, [nc] * b)
    flat, offs = dev(f, cuda), dev(o, cuda)
    total = flat.shape[0]
    ws = [torch.empty((lib.pn2_fps_large_packed_ws_bytes(total),), dtype=torch.uint8, device=cuda) for _ in range(2)]
    out = [torch.zeros((b, m), dtype=torch.int32, device=cuda) for _ in range(2)]
    oxyz = [torch.zeros((b, m, 3), dtype=torch.float32, device=cuda) for _ in range(2)]
    st = stream_ptr(cuda)

    def go(which, short_max):
        assert lib.pn2_farthest_point_sample_large_packed_ex(TIER, 256, short_max, b, total, nmax, m, ptr(flat), ptr(offs), 0, ptr(ws[which]),
                                                             ptr(out[which]), ptr(oxyz[which]), st) == 0

    def timed(which, short_max):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        go(which, short_max)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    go(0, 0); go(1, 8192)
    torch.cuda.synchronize()
    t_sorted, t_short = [], []
    for _ in range(5):
        t_sorted.append(timed(0, 0))
        t_short.append(timed(1, 8192))
    assert torch.equal(out[0], out[1]) and np.array_equal(bits(host(oxyz[0])), bits(host(oxyz[1])))
    print("short_max 0: %.3f ms, short_max 8192: %.3f ms (medians of 5)" % (np.median(t_sorted), np.median(t_short)))
    assert np.median(t_short) <= np.median(t_sorted)
