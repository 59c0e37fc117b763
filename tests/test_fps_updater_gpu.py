"""The updater waves of the batched FPS tier (csrc/fps_batch_body.h): APPLY -- a wave tests the picker's new
samples against its groups' boxes, 64 (sample, group) pairs at a time, and updates the touched groups either sample by sample in
straight-line code (the dense path: at least half of a chunk's pairs touched) or group by group through the bits of the
touched mask (the sparse path) -- and COLLECT -- second-best value of a lane's slots, the straight way to the list write for
0 < candidates <= 8, bisection and the exact fallback beside it. Every case runs the batched tier forced against the full tier
and the CPU oracle with a guard row behind the output, and once through pn2_sample_and_group_xyz_ex; indices are bit-exact.

Sizes are the smallest at which each instance of the body exists: 1024 rank slots (2 slots per thread, one group per wave, 64
samples per chunk), 2048 (two groups per wave), 4096 (four), 8192 (16 slots, four per group), and n = 700 / 2500 for padding
items. Where a case's property belongs to the data it is asserted first on a trace of the numpy model
(tests/test_fps_list_handoff_gpu.py's `_trace` with that file's dealing of points to lanes) -- at 1024 / 2048 / 4096 points, the
sizes that dealing covers; the 8192 / 700 / 2500 cases carry the same kind of cloud without a trace. `_pairs` below adds what
APPLY sees: the groups' boxes and, per batch and wave, which (sample, group) pairs pass the box test with the kernel's v*.

What the test does not observe: how many samples a chunk really holds (a wave takes what the picker has published when it
polls) and whether a slow-batch run starts are decided by the kernel's clock. The dense / sparse properties are therefore
stated per BATCH and wave: if at least half of a batch's pairs are touched, so are at least half of some chunk's, however the
batch is cut; a group touched by two samples of a batch that are next to each other in it runs the mask iteration twice
whenever the two arrive in one chunk (up to 16 samples at 4096 rank slots, one every ~270 cycles against ~700 per chunk)."""
import functools

import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

FPS_FULL, FPS_BATCH = 1, 3      # include/pn2ops.h


def _handoff():
    import test_fps_list_handoff_gpu as H
    return H


def _leaves(x):
    """point -> (wave, group of the wave) under the dealing of test_fps_list_handoff_gpu._lanes: leaf -> wave as there, the leaves
    of one wave numbered in leaf order"""
    import test_fps_batch_model as M
    n = x.shape[0]
    k0, k1, k2 = {4096: (4, 4, 2), 2048: (4, 2, 2), 1024: (2, 2, 2)}[n]
    ext = x.max(axis=0) - x.min(axis=0)
    a0, a1, a2 = np.argsort(-ext, kind="stable")
    wave = np.zeros(n, dtype=np.int64)
    leaf = np.zeros(n, dtype=np.int64)
    for a, p0 in enumerate(np.array_split(np.argsort(x[:, a0], kind="stable"), k0)):
        for i1, p1 in enumerate(np.array_split(p0[np.argsort(x[p0, a1], kind="stable")], k1)):
            for i2, p2 in enumerate(np.array_split(p1[np.argsort(x[p1, a2], kind="stable")], k2)):
                r = i1 * k2 + i2
                wave[p2] = (r + a) % M.WAVES if n == 4096 else ((a * k1 + i1) * k2 + i2) % M.WAVES
                leaf[p2] = (a * k1 + i1) * k2 + i2
    return wave, leaf


def _pairs(x, idx, recs):
    """per batch of the trace: for every wave, the matrix [sample of the batch, group of the wave] of pairs that pass APPLY's box
    test -- squared distance from the sample to the group's box < v* = fl(1.00001 * value of the previous batch's last sample)
    (the first batch: of the last early round's sample), the kernel's arithmetic"""
    from test_fps_batch_model import F, WAVES, _sqdist
    x = x.astype(F)
    wave, leaf = _leaves(x)
    boxes = {}
    for lf in np.unique(leaf):
        p = x[leaf == lf]
        boxes[lf] = (int(wave[leaf == lf][0]), p.min(axis=0), p.max(axis=0))
    td = np.full(x.shape[0], 1e38, dtype=F)
    val = np.zeros(len(idx), dtype=F)
    for i, k in enumerate(idx):
        val[i] = td[k] if i else F(1e38)
        td = np.minimum(td, _sqdist(x, x[k]))
    out = []
    for r in recs:
        j, a = r["j"], r["a"]
        thr = F(F(val[j - 1] * F(1.00001)) + F(1e-30))
        s = x[idx[j:j + a]]
        per_wave = []
        for w in range(WAVES):
            cols = []
            for lf in sorted(b for b in boxes if boxes[b][0] == w):
                _, lo, hi = boxes[lf]
                d = (s - np.clip(s, lo, hi)).astype(F)
                bd = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F) + (d[:, 2] * d[:, 2]).astype(F)
                cols.append(~(bd >= thr))
            per_wave.append(np.stack(cols, axis=1))
        out.append(per_wave)
    return out


# ---- what a case's name promises, as a predicate on (records, pairs) of its cloud 0
def _dense(recs, pairs):
    """some wave sees at least half of a batch's (sample, group) pairs touched: so does some chunk of it (the dense path)"""
    return any(2 * t.sum() >= t.size and t.shape[0] >= 1 for pw in pairs for t in pw)


def _sparse_twice(recs, pairs):
    """in a batch of which a wave sees under half of the pairs touched, one of its groups is touched by two samples that are next
    to each other in the batch: the mask iteration of the sparse path runs more than once (more than one group per wave: with one
    the dense rule takes every touched chunk)"""
    for pw in pairs:
        for t in pw:
            if t.shape[1] > 1 and 2 * t.sum() < t.size and (t[1:] & t[:-1]).any():
                return True
    return False


def _sparse_one_group(recs, pairs):
    """one group per wave: batches in which a wave is not touched at all (the chunk is skipped) and ones in which it is"""
    return any(not t.any() for pw in pairs for t in pw) and any(t.any() for pw in pairs for t in pw)


def _long_batches(recs, pairs):
    return max(r["a"] for r in recs) >= 33       # more than two chunks' worth at 4096 rank slots


def _fill(recs, pairs):
    return recs[-1]["ended"] == "zero"


def _bisects_or_ties(recs, pairs):
    return any(max(r["bis"]) > 0 for r in recs)


def _exact_fallback(recs, pairs):
    return any(any(r["exact"]) for r in recs) and any(max(r["bis"]) > 0 for r in recs)


def _first_batch_has_an_empty_wave(recs, pairs):
    """nobody of some wave reaches theta in the first batch: that wave sends its exact best lane (no bisection ran)"""
    r = recs[0]
    return any(e and b == 0 and c == 1 for e, b, c in zip(r["exact"], r["bis"], r["cnt"])) and any(c > 1 for c in r["cnt"])


def _spot(b, n, seed, ratio):
    """that part of the points on one spot (the cloud's point 0), the rest a sphere"""
    return S.dropout_clouds(b, n, seed, ratio=ratio)


def _tiny(b, n, seed):
    """a cube of extent 1e-3 around (0.5, 0.5, 0.5): differences of nearby fp32 numbers, distances ~1e-7"""
    return (np.float32(0.5) + S.uniform_clouds(b, n, seed) * np.float32(1e-3)).astype(np.float32)


def _picker_gen(name):
    import test_fps_picker_loop_gpu as L
    return getattr(L, name)


def _ladders4096(b, n, seed):
    """40 places, 20 rungs each: the model takes batches of 39, one sample per place, from sample ~150 on"""
    return np.stack([_picker_gen("_site_ladders")(n, 40, 20, seed + i) for i in range(b)])


CASES = [
    # ---- the dense path
    # (90 % on one spot: in the model dense at 2048 points, at 4096 only 21 % of a batch's pairs at the most; 95 % there)
    ("dense_spot_2048", lambda: _spot(3, 2048, 501, 0.9), 256, _dense),
    ("dense_spot_4096", lambda: _spot(2, 4096, 501, 0.95), 256, _dense),
    ("dense_tiny_1024", lambda: _tiny(3, 1024, 502), 256, _dense),
    ("dense_tiny_8192", lambda: _tiny(2, 8192, 503), 256, None),
    # ---- the sparse path
    ("sparse_sphere_4096", lambda: S.sphere_clouds(2, 4096, 504), 300, _sparse_twice),
    ("sparse_cube_2048", lambda: S.uniform_clouds(3, 2048, 505), 300, _sparse_twice),
    ("sparse_sphere_1024", lambda: S.sphere_clouds(4, 1024, 506), 256, _sparse_one_group),
    ("sparse_cube_8192", lambda: S.uniform_clouds(2, 8192, 507), 256, None),
    # ---- padding items
    ("padded_sphere_700", lambda: S.sphere_clouds(4, 700, 508), 256, None),
    ("padded_cube_2500", lambda: S.uniform_clouds(2, 2500, 509), 300, None),
    # ---- batches of more than two chunks
    ("long_batches_4096", lambda: _ladders4096(2, 4096, 72), 300, _long_batches),
    # ---- a cloud that runs out of distinct points
    ("fill_2048", lambda: _spot(3, 2048, 510, 0.9), 300, _fill),
    # ---- COLLECT's branches
    ("lattice_2048", lambda: _picker_gen("_lattice16")(2, 2048, 511), 300, _exact_fallback),
    ("doubled_4096", lambda: _picker_gen("_doubled")(2, 4096, 512), 256, _bisects_or_ties),
    ("empty_wave_first_batch_2048", lambda: S.sphere_clouds(2, 2048, 513), 256, _first_batch_has_an_empty_wave),
]


@functools.lru_cache(maxsize=None)
def _case(name):
    for c in CASES:
        if c[0] == name:
            xyz = np.ascontiguousarray(c[1](), dtype=np.float32)
            if c[3] is None:
                return xyz, c[2], None, None, None, None
            idx, recs = _handoff()._trace(xyz[0], c[2])
            return xyz, c[2], idx, recs, _pairs(xyz[0], idx, recs), c[3]
    raise KeyError(name)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_updater_index_exact(cuda, oracle, name):
    from pointnet2_amd import _C
    xyz, m, model_idx, recs, pairs, prop = _case(name)
    b, n, _ = xyz.shape
    want = oracle.farthest_point_sample(m, xyz)
    if prop is not None:
        print("%s: batches %s" % (name, [r["a"] for r in recs][:40]))
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
