"""The picker's sample loop of the batched FPS tier (csrc/fps_batch_body.h) has no sample counter: a list
ends by the bound exit alone, the winner's coordinates leave through v_readfirstlane under exec = its lane, and the batches that
can reach the end of the output row run the compiler's counted form of the loop. The cases aim at what that can break: a batch
that takes (nearly) a whole list, rows that end inside a list -- from the first batch on, and with more samples than points --,
ties at most samples, a chain that ends at value 0 from inside the loop, degenerate and huge coordinates. Every case: the batched
tier forced against the full tier and the CPU oracle, indices bit-exact, a guard row behind the output, and once through the
overlapped sample-and-group launch.

The large-yield cloud was searched with the numpy model of the tier (tests/test_fps_batch_model.py, seeds 0..119 of
_site_ladders at n = 1024 and 2048 with 64 and 65 sites): the largest batch found with the shipped list targets (36 / 20) yields
52 samples of a list of 8 candidate lanes per wave; no seed gave a batch of 64 (a list with total = 64 needs all eight updater
waves to stop their bisection at exactly eight lanes), so 52 is what is covered."""
import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

FPS_FULL, FPS_BATCH = 1, 3      # include/pn2ops.h


def _site_ladders(n, sites, per, seed, q=1.0 / 3, s=0.05, jit=2e-3):
    """`sites` places about 1 apart, each a geometric ladder of `per` points on a line (ratio q): the chain visits the places,
    then takes one point per place and rung -- `sites` candidates of nearly equal value at a time, everything else q * q below."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(sites ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:sites].astype(np.float64)
    c = g * 1.0 + rng.random((sites, 3)) * 0.3
    d = rng.standard_normal((sites, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sc = s * (1 + jit * rng.random(sites))
    pts = [c] + [c + d * (sc * q ** k)[:, None] for k in range(per - 1)]
    p = np.stack(pts, 1).reshape(-1, 3)
    p = p[rng.permutation(len(p))]
    return np.concatenate([p, np.repeat(p[:1], n - len(p), axis=0)]).astype(np.float32)


def _lattice16(b, n, seed):
    """n distinct points of the 16 x 16 x 16 lattice: equal distances at the top at most samples"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(1.0 / 16)
    return np.stack([g[rng.permutation(4096)[:n]] for _ in range(b)])


def _doubled(b, n, seed):
    """every point twice: the speculative maximum is held by two lanes until one of the pair is taken"""
    c = S.sphere_clouds(b, n // 2, seed)
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([x, x])[rng.permutation(n)] for x in c])


def _islands(c, shift):
    c = np.array(c, dtype=np.float32)
    c[:, c.shape[1] // 2:, 0] += np.float32(shift)
    return c


LADDER = dict(n=2048, sites=64, per=12, seed=72, m=600)      # the model: a batch of 52 samples ends at sample 512, 88 before the end of the row


def _ladder_clouds():
    return np.stack([_site_ladders(LADDER["n"], LADDER["sites"], LADDER["per"], LADDER["seed"] + i) for i in range(2)])


CASES = [
    # ---- a batch that takes most of a list (asserted on the CPU model below)
    ("ladders2048", _ladder_clouds, LADDER["m"]),
    # ---- the row ends inside a list: P = 2, 4, 8 slots per thread
    ("row257_n1024", lambda: S.sphere_clouds(3, 1024, 301), 257),
    ("row300_n2048", lambda: S.uniform_clouds(2, 2048, 302), 300),
    ("row511_n4096", lambda: S.sphere_clouds(2, 4096, 303), 511),
    ("row1000_n4096", lambda: S.uniform_clouds(2, 4096, 304), 1000),
    ("row1000_n1024", lambda: S.sphere_clouds(2, 1024, 305), 1000),
    ("row52_n1024", lambda: S.sphere_clouds(4, 1024, 306), 52),          # fewer than 64 samples left from the first batch on
    ("row60_n4096", lambda: S.uniform_clouds(2, 4096, 307), 60),
    ("m_gt_n_1024", lambda: S.uniform_clouds(2, 1024, 308), 1100),
    # ---- ties, the exact arg-max path
    ("lattice16_2048", lambda: _lattice16(2, 2048, 309), 600),
    ("doubled2048", lambda: _doubled(2, 2048, 310), 700),
    # ---- value 0 ends the chain from inside the loop: 90 % of the points on one spot
    ("spot2048", lambda: S.dropout_clouds(3, 2048, 311, ratio=0.9), 512),
    # ---- degenerate and huge coordinates
    ("line2048", lambda: S.sphere_clouds(2, 2048, 312) * np.array([1.0, 0.0, 0.0], np.float32), 300),
    ("islands_1e19", lambda: _islands(S.sphere_clouds(2, 4096, 313), 3e19), 300),
]


def test_the_model_sees_a_batch_that_takes_most_of_a_list():
    """CPU part of the ladders case (runs with the GPU cases: it is their premise)"""
    from test_fps_batch_model import _batched_fps
    _, batches = _batched_fps(_ladder_clouds()[0], LADDER["m"])
    print("ladders2048: batch sizes of the model:", batches)
    assert max(batches) >= 48, "the largest batch of the model yields %d samples" % max(batches)


@pytest.mark.parametrize("name,make,m", CASES, ids=[c[0] for c in CASES])
def test_picker_loop_index_exact(cuda, oracle, name, make, m):
    from pointnet2_amd import _C
    import pointnet2_amd as P
    xyz = np.ascontiguousarray(make(), dtype=np.float32)
    b, n, _ = xyz.shape
    want = oracle.farthest_point_sample(m, xyz)
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
    fps_idx, new_xyz = P.sample_and_group_xyz(m, 0.2, 32, x)[:2]              # the overlapped launch's producers
    assert np.array_equal(fps_idx.cpu().numpy(), want), name
    assert np.array_equal(new_xyz.cpu().numpy(), oracle.gather_point(xyz, want)), name
