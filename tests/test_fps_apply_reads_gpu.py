"""APPLY's LDS reads in the batched FPS tier (csrc/fps_batch_body.h): an updater wave reads the count word and
its lane's ring row back to back and waits once, and a sample reaches the packed subtract as a scalar register pair. The row's
address hangs on `done` and the lane, so a lane may read a row at or beyond the count -- stale from an earlier batch, half
written, or past the ring's 64 rows if the index were not clamped -- and leaves by the np mask. The cases aim at what that can
break: a chunk that starts so late in the ring that the clamp acts, rows of a long batch left behind short ones, output rows
that end inside a batch, clouds that run out of distinct points (the fill flag travels with the end flag), slow batches
(single != 0 travels with the end flag; runs of one-per-exchange rounds, which take the sample from vector registers, sit between
batches, which take it from scalar ones), the dense path and a wave that a whole batch leaves untouched. (Reading single / theta /
vlast early, behind the count word, was measured and dropped -- profiles/fps_apply/README.md; the cases that aimed at it stay.)

Every case: B = 4 clouds, the batched tier forced against the full tier and the CPU oracle with a guard row behind the output,
and once through pn2_sample_and_group_xyz_ex; indices are equal, no tolerance. Sizes are the smallest at which each instance of
the body exists: 1024 rank slots (64 samples per chunk), 2048 (32), 4096 (16), 8192 (16 slots per thread), n = 700 / 2500 for
padding items. Where a case's property belongs to the data it is asserted first on the numpy model's trace of cloud 0
(tests/test_fps_list_handoff_gpu.py's `_trace`, tests/test_fps_updater_gpu.py's `_pairs` for what APPLY's box test sees), at
the sizes that dealing covers.

The clamp. At 16 samples per chunk lane l reads row done + l % 16, so the index passes 63 only in a chunk that starts at
done >= 49: the batch then holds at least 50 samples (a chunk starts below the count). The cloud is built like the 52-sample
one of tests/test_fps_picker_loop_gpu.py (64 places, a ladder of points on each) at 4096 points; seeds 0..119 were searched with
the model. How many samples a chunk holds is the kernel's clock's decision: a wave that polls late enough takes samples 49..
in a chunk of its own only if it had consumed 49 before -- with eight waves, 50+ samples at one per ~270 cycles and a chunk per
~700 the late start is the common case, not a certainty. At 2048 and 1024 rank slots (32 / 64 samples per chunk) the clamp acts
in every chunk that starts at done >= 33 / 1: the long-batch cases there exercise it too."""
import functools

import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

FPS_FULL, FPS_BATCH = 1, 3      # include/pn2ops.h
B = 4


def _handoff():
    import test_fps_list_handoff_gpu as H
    return H


def _updater():
    import test_fps_updater_gpu as U
    return U


def _picker_gen(name):
    import test_fps_picker_loop_gpu as L
    return getattr(L, name)


# ---- clouds
CLAMP = dict(n=4096, sites=64, per=20, seed=81, m=700)       # the model: a batch of 56 samples (seeds 0..119 searched)


def _ladders(n, sites, per, seed):
    return np.stack([_picker_gen("_site_ladders")(n, sites, per, seed + i) for i in range(B)])


def _spot(n, seed, ratio):
    """that part of the points on one spot (the cloud's point 0), the rest a sphere"""
    return S.dropout_clouds(B, n, seed, ratio=ratio)


def _quantised(n, seed, q):
    return (np.round(S.uniform_clouds(B, n, seed) * q) / q).astype(np.float32)


def _tiny(n, seed):
    """a cube of extent 1e-3 around (0.5, 0.5, 0.5): every sample reaches most groups"""
    return (np.float32(0.5) + S.uniform_clouds(B, n, seed) * np.float32(1e-3)).astype(np.float32)


# ---- what a case's name promises, as a predicate on (records, pairs) of its cloud 0
def _clamp(recs, pairs):
    return max(r["a"] for r in recs) >= 50       # (the issue's figure is 49; a chunk that starts at done >= 49 needs 50)


def _stale(recs, pairs):
    """a long batch, then one of at most a third of its length: the ring holds the long one's rows beyond the short one's count"""
    a = [r["a"] for r in recs]
    return any(x >= 12 and 3 * y <= x for x, y in zip(a, a[1:]))


def _row_ends_inside(recs, pairs):
    return recs[-1]["ended"] == "row" and recs[-1]["a"] >= 2


def _fill(recs, pairs):
    return recs[-1]["ended"] == "zero"


def _slow(recs, pairs):
    """at least half of the batches yield a sample or two (the bound is strict and the values at the top are equal): what the
    picker's clock answers with runs of one-per-exchange rounds"""
    a = [r["a"] for r in recs]
    return len(a) >= 20 and 2 * sum(1 for v in a if v <= 2) >= len(a)


def _dense(recs, pairs):
    return _updater()._dense(recs, pairs)


def _one_group_untouched(recs, pairs):
    return _updater()._sparse_one_group(recs, pairs)


CASES = [
    # name, clouds, m, property on the trace of cloud 0 (None: a size the model's dealing does not cover), needs `pairs`
    ("clamp_ladders_4096", lambda: _ladders(CLAMP["n"], CLAMP["sites"], CLAMP["per"], CLAMP["seed"]), CLAMP["m"], _clamp, False),
    ("stale_rows_ladders_2048", lambda: _ladders(2048, 64, 12, 72), 600, _stale, False),
    ("stale_rows_ladders_1024", lambda: _ladders(1024, 64, 12, 72), 600, _stale, False),
    ("row300_cube_2048", lambda: S.uniform_clouds(B, 2048, 602), 300, _row_ends_inside, False),
    ("row300_sphere_4096", lambda: S.sphere_clouds(B, 4096, 603), 300, _row_ends_inside, False),
    ("m_gt_n_1024", lambda: S.uniform_clouds(B, 1024, 604), 1100, None, False),
    ("fill_doubled_1024", lambda: _picker_gen("_doubled")(B, 1024, 605), 600, _fill, False),
    ("fill_spot_2048", lambda: _spot(2048, 606, 0.9), 300, _fill, False),
    ("slow_lattice16_2048", lambda: _picker_gen("_lattice16")(B, 2048, 607), 300, _slow, False),
    ("ties_quantised64_4096", lambda: _quantised(4096, 608, 64.0), 300, None, False),
    ("dense_spot_2048", lambda: _spot(2048, 609, 0.9), 256, _dense, True),
    ("dense_tiny_1024", lambda: _tiny(1024, 610), 256, _dense, True),
    ("one_group_sphere_1024", lambda: S.sphere_clouds(B, 1024, 611), 256, _one_group_untouched, True),
    ("cube_8192", lambda: S.uniform_clouds(B, 8192, 612), 256, None, False),
    ("spot_8192", lambda: _spot(8192, 613, 0.9), 300, None, False),
    ("padded_sphere_700", lambda: S.sphere_clouds(B, 700, 614), 256, None, False),
    ("padded_cube_2500", lambda: S.uniform_clouds(B, 2500, 615), 300, None, False),
]


@functools.lru_cache(maxsize=None)
def _case(name):
    for c in CASES:
        if c[0] == name:
            xyz = np.ascontiguousarray(c[1](), dtype=np.float32)
            assert xyz.shape[0] == B
            if c[3] is None:
                return xyz, c[2], None, None, None, None
            idx, recs = _handoff()._trace(xyz[0], c[2])
            pairs = _updater()._pairs(xyz[0], idx, recs) if c[4] else None
            return xyz, c[2], idx, recs, pairs, c[3]
    raise KeyError(name)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_apply_reads_index_exact(cuda, oracle, name):
    from pointnet2_amd import _C
    xyz, m, model_idx, recs, pairs, prop = _case(name)
    b, n, _ = xyz.shape
    want = oracle.farthest_point_sample(m, xyz)
    if prop is not None:
        print("%s: batches %s" % (name, [r["a"] for r in recs][:60]))
        assert prop(recs, pairs), "%s: the model's chain does not do what the case's name says" % name
        assert np.array_equal(model_idx, want[0]), name
    x = torch.from_numpy(xyz).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    lib = _C.lib()

    def run(tier):
        buf = torch.full((b + 1, m), -1, dtype=torch.int32, device=cuda)    # one guard row behind the output
        rc = lib.pn2_farthest_point_sample_variant(tier, b, n, m, x.data_ptr(), None, buf.data_ptr(), None, st)
        assert rc == 0, rc
        got = buf.cpu().numpy()
        assert (got[-1] == -1).all(), "%s tier %d: wrote past the end of the output" % (name, tier)
        return got[:-1]

    full = run(FPS_FULL)
    assert np.array_equal(full, want), "%s full tier: first mismatch at %s" % (name, np.argwhere(full != want)[:3])
    for rep in range(2):
        got = run(FPS_BATCH)
        assert np.array_equal(got, want), "%s batched tier rep %d: first mismatch at %s" % (name, rep, np.argwhere(got != want)[:3])
    # the overlapped launch with the batched tier as its producer
    ns, r = 16, 0.2
    ws = torch.zeros((lib.pn2_sample_and_group_ws_bytes(b, m),), dtype=torch.uint8, device=cuda)
    fps = torch.full((b + 1, m), -1, dtype=torch.int32, device=cuda)
    new_xyz = torch.empty((b, m, 3), device=cuda)
    idx = torch.empty((b, m, ns), dtype=torch.int32, device=cuda)
    cnt = torch.empty((b, m), dtype=torch.int32, device=cuda)
    grouped = torch.empty((b, m, ns, 3), device=cuda)
    rc = lib.pn2_sample_and_group_xyz_ex(b, n, m, r, ns, x.data_ptr(), ws.data_ptr(), 0, FPS_BATCH, 2, fps.data_ptr(), new_xyz.data_ptr(),
                                         idx.data_ptr(), cnt.data_ptr(), grouped.data_ptr(), 1, st)
    assert rc == 0, rc
    got = fps.cpu().numpy()
    assert (got[-1] == -1).all() and np.array_equal(got[:-1], want), name
    assert np.array_equal(new_xyz.cpu().numpy(), oracle.gather_point(xyz, want)), name
    off = lib.pn2_sample_and_group_status_offset(b, m)
    assert int(ws[off:off + 4].view(torch.int32)) == 0, name
