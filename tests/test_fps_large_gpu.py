"""Device tests of the large-cloud FPS tier (csrc/fps_large.hip; 16384 < n <= 1048576): index-exact against the
CPU oracle through pn2_farthest_point_sample_large_ex at every group length, on the clouds its CPU model has reproduced the oracle
on (tests/fps_large_cases.py) and on the sizes where the grouping takes another shape (a one-record last group, a whole number
of groups and one record either side of it, several clouds, more samples than points, one sample, degenerate boxes, a coarse fp32
grid, non-finite coordinates) and, at the group lengths that can hold them, on the clouds that fill all 4096 box slots of the
kernel (1048576 points at L = 256); out_xyz is the gather of the indices bit for bit; the Python operators give the same tensors whichever kernel runs; the
entry is one kernel node in a captured graph; and it is not slower than the global-memory kernel where the size rule sends it."""
import numpy as np
import pytest
import torch

from fps_large_cases import FULL_TABLE_CASES, LARGE_CASES
from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

GROUP_LENS = (64, 128, 256)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


EXTRA_CASES = [
    ("n16639", lambda: S.uniform_clouds(1, 16384 + 255, 1221), 64),              # one record short of a whole number of 256-groups
    ("n16640", lambda: S.uniform_clouds(1, 16384 + 256, 1222), 64),              # whole groups at every group length
    ("n16641", lambda: S.uniform_clouds(1, 16384 + 257, 1223), 64),              # a one-record last group at every group length
    ("three_clouds", lambda: np.concatenate([S.uniform_clouds(1, 17000, 1224), S.sphere_clouds(1, 17000, 1225),
                                             S.quantized_clouds(1, 17000, 1226)]), 100),
    ("m_gt_n", lambda: S.duplicated_clouds(1, 16500, 1227), 16600),              # every distance 0 long before the end
    ("m1", lambda: S.uniform_clouds(2, 16500, 1228), 1),
    ("flat", lambda: _f32(S.sphere_clouds(1, 20000, 1229) * np.array([1.0, 1.0, 0.0], np.float32)), 200),
    ("line", lambda: _f32(S.sphere_clouds(1, 20000, 1230) * np.array([1.0, 0.0, 0.0], np.float32)), 200),
    ("far_offset", lambda: _f32(S.sphere_clouds(1, 20000, 1231) * np.float32(1e-3) + np.float32(100.0)), 200),   # coarse fp32 grid
]
CASES = [(c[0], c[1], c[2]) for c in LARGE_CASES] + EXTRA_CASES
# the whole group table: a case at its own group length and every larger one (fewer groups: a smaller L is PN2_E_TOO_LARGE)
FULL_TABLE_RUNS = [(c[0], L) for c in FULL_TABLE_CASES for L in GROUP_LENS if L >= c[3]]
_WANT = {}


def _case(oracle, name):
    """(cloud, oracle indices), computed once per case and shared by the group lengths."""
    if name not in _WANT:
        table = CASES + [(c[0], c[1], c[2]) for c in FULL_TABLE_CASES]
        _, make, m = table[[c[0] for c in table].index(name)]
        x = _f32(make())
        _WANT[name] = (x, oracle.farthest_point_sample(m, x))
    return _WANT[name]


def _large(x, m, group_len=None, want_xyz=True):
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    b, n, _ = x.shape
    dev = x.device
    ws = torch.empty((lib.pn2_fps_large_ws_bytes(b, n),), dtype=torch.uint8, device=dev)
    out = torch.full((b, m), -7, dtype=torch.int32, device=dev)
    oxyz = torch.full((b, m, 3), float("nan"), dtype=torch.float32, device=dev) if want_xyz else None
    if group_len is None:
        rc = lib.pn2_farthest_point_sample_large(b, n, m, ptr(x), ptr(ws), ptr(out), ptr(oxyz), stream_ptr(dev))
    else:
        rc = lib.pn2_farthest_point_sample_large_ex(group_len, b, n, m, ptr(x), ptr(ws), ptr(out), ptr(oxyz), stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, oxyz


@pytest.mark.parametrize("group_len", GROUP_LENS)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_index_exact_against_the_oracle(cuda, oracle, name, group_len):
    _check_against_the_oracle(cuda, oracle, name, group_len)


def _check_against_the_oracle(cuda, oracle, name, group_len):
    xyz, want = _case(oracle, name)
    x = torch.from_numpy(xyz).to(cuda)
    out, oxyz = _large(x, want.shape[1], group_len)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), "%s L=%d: first difference at %s" % (name, group_len, np.argwhere(got != want)[:3].ravel())
    gathered = np.take_along_axis(xyz, want[:, :, None].astype(np.int64).repeat(3, axis=2), axis=1)
    assert np.array_equal(oxyz.cpu().numpy().view(np.uint32), gathered.view(np.uint32)), "out_xyz is not gather_point(inp, idx) bit for bit"


@pytest.mark.parametrize("name,group_len", FULL_TABLE_RUNS, ids=["%s-L%d" % r for r in FULL_TABLE_RUNS])
def test_the_whole_group_table(cuda, oracle, name, group_len):
    """4096 groups, all four box slots of every lane (and 2049: a one-record group alone in slot 2), on the clouds whose winners
    the CPU model has found in all four quarters of the table, every quarter both updated and skipped
    (tests/test_fps_large_model.py)."""
    _check_against_the_oracle(cuda, oracle, name, group_len)


def test_the_python_operator_at_the_top_of_the_envelope(cuda, oracle):
    """1048576 points, the largest cloud the tier takes: the size rule (None), the tier (True) and the global-memory kernel
    (False) return the oracle's indices."""
    import pointnet2_amd as P
    xyz, want = _case(oracle, "full_table_256")
    x = torch.from_numpy(xyz).to(cuda)
    try:
        for mode in (True, False, None):
            P.set_fps_large(mode)
            assert np.array_equal(P.farthest_point_sample(want.shape[1], x).cpu().numpy(), want), mode
    finally:
        P.set_fps_large(None)


def test_the_plain_entry_and_a_null_out_xyz(cuda, oracle):
    xyz, want = _case(oracle, "uniform20000")
    x = torch.from_numpy(xyz).to(cuda)
    out, oxyz = _large(x, want.shape[1], None, want_xyz=False)
    assert oxyz is None and np.array_equal(out.cpu().numpy(), want)
    out, oxyz = _large(x, want.shape[1], None)
    import pointnet2_amd as P
    assert np.array_equal(out.cpu().numpy(), want) and torch.equal(oxyz, P.gather_point(x, out))


def test_the_python_operators_whichever_kernel_runs(cuda, oracle):
    import pointnet2_amd as P
    xyz, want = _case(oracle, "three_clouds")
    x = torch.from_numpy(xyz).to(cuda)
    m = want.shape[1]
    got = {}
    try:
        for mode in (True, False, None):
            P.set_fps_large(mode)
            idx = P.farthest_point_sample(m, x)
            pre = torch.full((x.shape[0], m), -1, dtype=torch.int32, device=cuda)
            ret = P.farthest_point_sample(m, x, out=pre)
            assert ret is pre or ret.data_ptr() == pre.data_ptr()                 # out= honoured
            gidx, gxyz = P.farthest_point_sample_gather(m, x)
            assert getattr(gxyz, "_pn2_fps_ordered", False)                       # the hint of a sampling's output
            got[mode] = (idx, pre, gidx, gxyz)
    finally:
        P.set_fps_large(None)
    for mode, (idx, pre, gidx, gxyz) in got.items():
        assert np.array_equal(idx.cpu().numpy(), want), mode
        assert torch.equal(pre, idx) and torch.equal(gidx, idx), mode
        assert torch.equal(gxyz, got[False][3]), mode


def test_one_kernel_node_replayed_over_rotated_inputs(cuda, oracle):
    """The entry inside a captured graph: no memset node, no host synchronisation, nothing kept between launches but the
    caller's workspace. Replayed over three rotations of a 20000-point cloud, each replay equal to the oracle."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    base = S.uniform_clouds(1, 20000, 1232)[0] - np.float32(0.5)
    m = 96
    clouds = []
    for a in (0.0, 0.7, 2.1):
        rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], np.float32)
        clouds.append(_f32((base @ rot.T)[None]))
    x = torch.from_numpy(clouds[0]).to(cuda)
    ws = torch.empty((lib.pn2_fps_large_ws_bytes(1, 20000),), dtype=torch.uint8, device=cuda)
    out = torch.zeros((1, m), dtype=torch.int32, device=cuda)
    oxyz = torch.zeros((1, m, 3), dtype=torch.float32, device=cuda)

    def call():
        assert lib.pn2_farthest_point_sample_large(1, 20000, m, ptr(x), ptr(ws), ptr(out), ptr(oxyz), stream_ptr(cuda)) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for c in clouds:
        x.copy_(torch.from_numpy(c))
        out.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want = oracle.farthest_point_sample(m, c)
        assert np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(oxyz.cpu().numpy()[0], c[0][want[0]])


def test_not_slower_than_the_global_memory_kernel(cuda):
    """Relative tripwire at b = 2, uniform 131072 -> 512: the median of five alternating timings of the new entry is not above
    the global-memory kernel's (pn2_farthest_point_sample_gather, unchanged) in the same process."""
    from pointnet2_amd import _C
    from pointnet2_amd._tensors import ptr, stream_ptr
    lib = _C.lib()
    b, n, m = 2, 131072, 512
    x = torch.from_numpy(S.uniform_clouds(b, n, 1233)).to(cuda)
    ws = torch.empty((lib.pn2_fps_large_ws_bytes(b, n),), dtype=torch.uint8, device=cuda)
    temp = torch.empty((lib.pn2_fps_temp_floats(b, n),), dtype=torch.float32, device=cuda)
    out = [torch.zeros((b, m), dtype=torch.int32, device=cuda) for _ in range(2)]
    oxyz = [torch.zeros((b, m, 3), dtype=torch.float32, device=cuda) for _ in range(2)]
    st = stream_ptr(cuda)

    def generic():
        assert lib.pn2_farthest_point_sample_gather(b, n, m, ptr(x), ptr(temp), ptr(out[0]), ptr(oxyz[0]), st) == 0

    def large():
        assert lib.pn2_farthest_point_sample_large(b, n, m, ptr(x), ptr(ws), ptr(out[1]), ptr(oxyz[1]), st) == 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    generic(); large()
    torch.cuda.synchronize()
    tg, tl = [], []
    for _ in range(5):
        tg.append(timed(generic))
        tl.append(timed(large))
    assert torch.equal(out[0], out[1]) and torch.equal(oxyz[0], oxyz[1])
    print("generic %.3f ms, large %.3f ms (medians of 5)" % (np.median(tg), np.median(tl)))
    assert np.median(tl) <= np.median(tg)
