"""CPU model of the large-cloud FPS tier (csrc/fps_large.hip): the cloud is sorted into the cells of a 32 x 32 x 32
grid in Morton order, the sorted order is cut into groups of L consecutive records with tight bounding boxes, and in a round a
group whose box lies farther from the new sample than the value v* that just won the arg-max is NOT updated (the pruned
tier's rule, tests/test_fps_pruned_model.py); the arg-max runs over CACHED group keys, the generic kernel's 64-bit
(value bits << 32) | (0xFFFFFFFF - tie key). Restated in numpy with the kernel's fp32 formulas and run as a whole chain against
the oracle's sequential sampling. The assertion inside the loop is the exactness claim itself -- skipping a group changes no
running distance -- checked in EVERY round for EVERY skipped group. No GPU (the device tier is tested against the same oracle on
the same clouds in tests/test_fps_large_gpu.py)."""
import numpy as np
import pytest

from fps_large_cases import FULL_TABLE_CASES, FULL_TABLE_NAMES, LARGE_CASES, LARGE_NAMES
from pointnet2_amd import synthetic as S

F = np.float32
REF_THREADS = 512
AXIS_CELLS = 32


def _sqdist(p, s):
    dx, dy, dz = (p[:, 0] - s[0]).astype(F), (p[:, 1] - s[1]).astype(F), (p[:, 2] - s[2]).astype(F)
    return ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)


def _spread5(v):
    return (v & 1) | ((v & 2) << 2) | ((v & 4) << 4) | ((v & 8) << 6) | ((v & 16) << 8)


def _cell_order(x):
    """The kernel's prologue: bounding box, 32 bins per axis (a degenerate axis: bin 0), Morton cell number, cell order. The
    order inside a cell is timing dependent on the device and irrelevant; here it is the input order."""
    with np.errstate(all="ignore"):
        lo, hi = np.fmin.reduce(x, axis=0).astype(F), np.fmax.reduce(x, axis=0).astype(F)     # fminf / fmaxf: NaNs drop out
        e = (hi - lo).astype(F)
        ok = (e > 0) & np.isfinite(e)
        scale = np.where(ok, F(AXIS_CELLS) / np.where(ok, e, F(1)), F(0)).astype(F)
        scale = np.where(np.isfinite(scale), scale, F(0)).astype(F)
        lo = np.where(ok, lo, F(0)).astype(F)
        f = ((x - lo[None, :]).astype(F) * scale[None, :]).astype(F)
        bins = np.fmin(np.fmax(f, F(0)), F(AXIS_CELLS - 1)).astype(np.int64)            # fmaxf(NaN, 0) = 0
    cell = (_spread5(bins[:, 0]) << 2) | (_spread5(bins[:, 1]) << 1) | _spread5(bins[:, 2])
    return np.argsort(cell, kind="stable")


def _med3(s, lo, hi):
    """v_med3_f32, the kernel's clamp: the median of three. A box axis without a finite-or-infinite member (all NaN) is
    lo = inf, hi = -inf, whose median with s is s; a NaN sample gives NaN - something = NaN below whatever comes back here."""
    return np.fmax(np.fmin(s, lo), np.fmin(np.fmax(s, lo), hi))


def _large_fps(x, m, L, check=True, stats=None):
    """-> (indices, updated share of (group, round) pairs). stats: a dict that receives "group_of" (point -> its group) and
    "updates" (per group, the rounds it was updated in)."""
    x = np.ascontiguousarray(x, dtype=F)
    n = x.shape[0]
    order = _cell_order(x)                                   # record i of the sorted copy = point order[i]
    rec = x[order]
    G = (n + L - 1) // L
    pad = G * L - n
    k = order.astype(np.int64)
    tiekey = ((k & (REF_THREADS - 1)) << 22) | (k >> 9)      # smaller wins a tie
    low = np.concatenate([np.uint64(0xFFFFFFFF) - tiekey.astype(np.uint64), np.zeros(pad, np.uint64)])
    real = np.concatenate([np.ones(n, bool), np.zeros(pad, bool)])
    recp = np.concatenate([rec, np.repeat(rec[-1:], pad, axis=0)]) if pad else rec
    with np.errstate(all="ignore"):
        # tight boxes by fminf / fmaxf, as lg_group_finish builds them: a NaN coordinate drops out of its box
        lo = np.fmin.reduce(np.where(real[:, None], recp, F(np.inf)).reshape(G, L, 3), axis=1).astype(F)
        hi = np.fmax.reduce(np.where(real[:, None], recp, F(-np.inf)).reshape(G, L, 3), axis=1).astype(F)
    mind = np.full(G * L, 1e38, dtype=F)
    updates = np.zeros(G, dtype=np.int64)

    def keys_of(rows):                                       # the generic kernel's key; a missing record: 0
        v = mind.reshape(G, L)[rows].view(np.uint32).astype(np.uint64)
        return np.where(real.reshape(G, L)[rows], (v << np.uint64(32)) | low.reshape(G, L)[rows], np.uint64(0))

    gkey = keys_of(np.arange(G)).max(axis=1)                  # cached group keys: the keys of the START distances
    out = np.zeros(m, dtype=np.int32)
    vstar = F(1e38)
    s = x[0]
    updated = 0
    for j in range(1, m):
        with np.errstate(all="ignore"):
            thr = F(F(vstar * F(1.00001)) + F(1e-30))
            a = (s[None, :] - _med3(s[None, :], lo, hi)).astype(F)                         # sample - clamp(sample, lo, hi)
            bd = ((a[:, 0] * a[:, 0]).astype(F) + (a[:, 1] * a[:, 1]).astype(F)).astype(F) + (a[:, 2] * a[:, 2]).astype(F)
            far = bd >= thr                                                                # NaN -> not far -> updated
            if check:
                d = _sqdist(recp, s)
                skipped = np.repeat(far, L) & real
                # THE CLAIM: skipping these groups changes nothing (fminf: a NaN distance lowers nothing either)
                assert (np.fmin(d[skipped], mind[skipped]) == mind[skipped]).all(), \
                    "round %d: a skipped group holds a point the sample would have lowered" % j
            rows = np.nonzero(~far)[0]
            view = mind.reshape(G, L)
            view[rows] = np.fmin(_sqdist(recp.reshape(G, L, 3)[rows].reshape(-1, 3), s).reshape(-1, L), view[rows])
        gkey[rows] = keys_of(rows).max(axis=1)                # touched groups refresh their key, the others keep theirs
        updated += len(rows)
        updates[rows] += 1
        best = gkey.max()                                   # the arg-max runs over cached keys only
        tk = np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))
        cur = int(((tk & np.uint64(0x3FFFFF)) << np.uint64(9)) | (tk >> np.uint64(22)))
        vstar = np.array([best >> np.uint64(32)], dtype=np.uint64).astype(np.uint32).view(F)[0]
        s = x[cur]
        out[j] = cur
    if stats is not None:
        stats["group_of"] = np.empty(n, dtype=np.int64)
        stats["group_of"][order] = np.arange(n) // L
        stats["updates"] = updates
    return out, updated / max(G * (m - 1), 1)


@pytest.mark.parametrize("name,make,m,L", LARGE_CASES, ids=LARGE_NAMES)
def test_cached_group_keys_and_the_skip_rule_give_the_oracles_samples(oracle, name, make, m, L):
    clouds = make()
    want = oracle.farthest_point_sample(m, clouds)
    for b in range(clouds.shape[0]):
        got, share = _large_fps(clouds[b], m, L)
        assert np.array_equal(got, want[b]), "%s cloud %d: first difference at %s" % (name, b, np.argwhere(got != want[b])[:3].ravel())
        if name.startswith("identical"):
            assert share == 1.0, "every box of an identical cloud holds every sample: nothing can be pruned (%.3f)" % share


SLOT_GROUPS = 1024                                           # groups per box slot: 16 waves x 64 lanes


@pytest.mark.parametrize("name,make,m,L,groups", FULL_TABLE_CASES, ids=FULL_TABLE_NAMES)
def test_the_whole_group_table(oracle, name, make, m, L, groups):
    """The clouds that fill the kernel's four box slots per lane (slot i = groups 1024 i .. 1024 i + 1023). Besides the oracle's
    samples, CONDITIONS ON THE CASE, so that the device test of the same cloud does run what it is there for: the winners come
    from groups of all four quarters of the table (publishing from best[] at every slot), and in every quarter some (group,
    round) pairs were updated and some skipped (both branches of every slot's ballot)."""
    clouds = make()
    n = clouds.shape[1]
    assert (n + L - 1) // L == groups
    want = oracle.farthest_point_sample(m, clouds)
    for b in range(clouds.shape[0]):
        stats = {}
        got, share = _large_fps(clouds[b], m, L, stats=stats)
        assert np.array_equal(got, want[b]), "%s cloud %d: first difference at %s" % (name, b, np.argwhere(got != want[b])[:3].ravel())
        slots = (groups + SLOT_GROUPS - 1) // SLOT_GROUPS
        winners = np.bincount(stats["group_of"][want[b][1:]] // SLOT_GROUPS, minlength=slots)
        per_slot = [stats["updates"][q * SLOT_GROUPS:(q + 1) * SLOT_GROUPS] for q in range(slots)]
        shares = [float(u.sum()) / (len(u) * (m - 1)) for u in per_slot]
        print("%s cloud %d: winners per quarter %s, updated share per quarter %s" % (name, b, winners.tolist(), ["%.3f" % v for v in shares]))
        if groups == 4096:
            assert slots == 4 and (winners > 0).all(), winners
            assert all(0.0 < v < 1.0 for v in shares), shares
        else:                                                # slot2_first_group: one group in slot 2, one record in it
            assert slots == 3 and len(per_slot[2]) == 1 and n - (groups - 1) * L == 1
            assert 0 < per_slot[2][0] < m - 1, "the one-record group is both updated and skipped"


SHARE_CASES = [("uniform131072", lambda: S.uniform_clouds(1, 131072, 1211), 1024, 256),
               ("sphere65536", lambda: S.sphere_clouds(1, 65536, 1212), 1024, 256)]


@pytest.mark.parametrize("name,make,m,L", SHARE_CASES, ids=[c[0] for c in SHARE_CASES])
def test_the_rule_prunes_on_large_clouds(oracle, name, make, m, L):
    """Work count of the model: the share of (group, round) pairs that had to be updated. An x-major grid gives 0.094 / 0.072 on
    these two shapes; the Morton grid must stay below a quarter as well."""
    clouds = make()
    got, share = _large_fps(clouds[0], m, L, check=False)
    print("%s: updated share %.4f" % (name, share))
    assert np.array_equal(got, oracle.farthest_point_sample(m, clouds)[0])
    assert share < 0.25, "updated share %.3f" % share
