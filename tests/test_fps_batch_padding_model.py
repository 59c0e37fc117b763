"""CPU model of the batched FPS tier on clouds that are MOSTLY PADDING SLOTS (csrc/fps_batch_body.h run by the ragged wrappers
of csrc/fps.hip; DESIGN.md 4.11 "padding slots"). It is the model of tests/test_fps_batch_model.py restated with the padding
slots PRESENT: a template of NS rank slots (1024: 2 per updater thread, 8 leaves; 8192: 16 per thread, 32 leaves), of which only
n_c hold points. The other NS - n_c items sit at point 0's position with value bits 0 and key low word 0, and all NS items are
dealt to (wave, lane, slot) as fps_pruned_prologue deals them: 64 bins per axis over the bounding box, three counting passes,
tickets inside a bin (arbitrary on the device: a seeded shuffle here). A ragged cloud can be one point in 8192 slots, so whole
lanes, whole updater waves and whole leaves hold nothing but padding; such a wave finds no lane at theta, falls back to its
"exact best lane" -- the lowest lane among equal (0 : 0) keys -- and puts a padding candidate of value 0 on the list.

The chain is the kernel's: EARLY rounds on the 64-bit keys of ALL slots; COLLECT per lane (best key, second-best value of its
P slots) and per wave (theta, bisection, exact fallback, the bound word); the picker's sample loop in its UNCOUNTED form
(PN2_BT_NOCTR: no sample counter, it must leave by the bound exit) unless fewer than 64 output rows are left; the value-0 tail.
Asserted inside the loops: every accepted pick is the arg-max over the REAL points, no padding slot is picked before the tail
(nor in it: the tail is point 0), every batch accepts at least one sample, the bound is >= 1 so that the uncounted loop ends, and
a batch never takes more than the ring's 64 rows. The chains are then compared with the oracle on the slice. No GPU."""
import functools

import numpy as np
import pytest

from pointnet2_amd import synthetic as S

F = np.float32
REF_THREADS = 512
WAVES, CAP, LIST_HI, LIST_LO, G0, EARLY, BINS = 8, 8, 36, 20, F(0.10), 48, 64   # fps_batch_body.h / fps_pruned_body.h
TEMPLATES = {1024: (2, 2, (2, 2, 2)), 8192: (16, 4, (4, 4, 2))}                   # NS: slots per thread, slots per group, parts per pass


def _bits(v):
    return np.asarray(v, dtype=F).view(np.uint32).astype(np.int64)


def _float(b):
    return np.array([b], dtype=np.uint32).view(F)[0]


def _sqdist(p, s):
    dx, dy, dz = (p[:, 0] - s[0]).astype(F), (p[:, 1] - s[1]).astype(F), (p[:, 2] - s[2]).astype(F)
    return ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)


def _deal(pos, ns, seed):
    """fps_pruned_prologue on 512 updater threads: item -> (thread, slot). Returns tab[thread, slot] = item."""
    P, GS, K = TEMPLATES[ns]
    G = K[0] * K[1] * K[2]
    rng = np.random.default_rng(seed)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    e = (hi - lo).astype(F)
    ok = (e > 0) & np.isfinite(e)
    lo3, ex = np.where(ok, lo, F(0)).astype(F), np.where(ok, e, F(0)).astype(F)
    a0, a1, a2 = 0, 1, 2                                                           # axes by extent, ties keep x, y, z order
    if ex[a1] > ex[a0]:
        a0, a1 = a1, a0
    if ex[a2] > ex[a0]:
        a0, a2 = a2, a0
    if ex[a2] > ex[a1]:
        a1, a2 = a2, a1
    seg = np.zeros(ns, dtype=np.int64)
    rank = np.zeros(ns, dtype=np.int64)
    child = ns
    for lev, ax in enumerate((a0, a1, a2)):
        sc = F(BINS) / ex[ax] if ex[ax] > 0 else F(0)
        q = np.clip(((pos[:, ax] - lo3[ax]).astype(F) * sc).astype(F).astype(np.int64), 0, BINS - 1)
        counter = seg * BINS + q
        order = rng.permutation(ns)                                                # the order in which the tickets are drawn
        order = order[np.argsort(counter[order], kind="stable")]
        sc_sorted = counter[order]
        first = np.searchsorted(sc_sorted, sc_sorted, side="left")                 # start of the item's (segment, bin) run
        seg_first = np.searchsorted(sc_sorted // BINS, sc_sorted // BINS, side="left")
        r = np.empty(ns, dtype=np.int64)
        r[order] = np.arange(ns) - seg_first                                       # exclusive prefix of the bin + the ticket
        assert (first >= seg_first).all()
        child //= K[lev]
        seg = (counter >> 6) * K[lev] + r // child
        rank = r & (child - 1)
    assert child == 64 * GS and (np.bincount(seg, minlength=G) == child).all(), "a leaf = GS slots of all 64 lanes of one wave"
    R = K[1] * K[2]
    a, r = seg // R, seg % R
    wave, group = (((r + a) & (WAVES - 1)), a) if G == 32 else ((seg & (WAVES - 1)), seg // WAVES)
    thread, slot = wave * 64 + (rank & 63), group * GS + (rank >> 6)
    tab = np.full((64 * WAVES, P), -1, dtype=np.int64)
    tab[thread, slot] = np.arange(ns)
    assert (tab >= 0).all()
    return tab


def _padded_batched_fps(x, m, ns, seed=0, early=EARLY, runs=None):
    x = x.astype(F)
    n = x.shape[0]
    P = TEMPLATES[ns][0]
    assert 1 <= n <= ns and m >= 1
    q = (n + REF_THREADS - 1) // REF_THREADS
    k = np.arange(ns)
    real = k < n
    tie = (k % REF_THREADS) * q + k // REF_THREADS
    low = np.where(real, ns - 1 - tie, 0).astype(np.int64)                          # padding: key low word 0
    assert n == ns or (low[real] > 0).all()
    pos = np.where(real[:, None], x[np.minimum(k, n - 1)], x[0]).astype(F)           # padding items at point 0's position
    tab = _deal(pos, ns, seed)
    td = np.where(real, F(1e38), F(0)).astype(F)                                    # padding: value bits 0
    td = np.minimum(td, _sqdist(pos, x[0]))
    out = [0]
    stats = dict(batches=[], padding_candidates=0, padding_waves=int((~real[tab]).reshape(WAVES, -1).all(axis=1).sum()))

    def keys():
        return (_bits(td) << 32) | low

    def argmax_real():
        best = td[:n].max()
        c = np.nonzero(td[:n] == best)[0]
        return int(c[np.argmin(tie[c])]), best

    def accept(item, value, what):
        assert real[item], "%s: padding slot %d picked at sample %d" % (what, item, len(out))
        pa, va = argmax_real()
        assert item == pa and value == va, "%s, sample %d: pick %d is not the arg-max %d over the real points" % (what, len(out), item, pa)
        out.append(int(item))

    def single_round():
        kk = keys()
        w = int(np.argmax(kk))                                                      # real keys are distinct; padding (0 : 0) is below point 0's (0 : NS - 1)
        v = td[w]
        accept(w, v, "one-per-exchange round")
        np.minimum(td, _sqdist(pos, pos[w]), out=td)
        return v

    vlast = F(1e38)
    while len(out) < min(early, m):
        vlast = single_round()
    g = G0
    theta_b = int(_bits(F(vlast * F(F(1.0) - G0)))) if len(out) > 1 else int(_bits(F(1e38)))
    vlast_b = int(_bits(vlast))
    lanes = np.arange(64)
    while len(out) < m:
        # COLLECT
        kk = keys()[tab]                                                            # [thread, slot]
        kl = kk.max(axis=1)
        vb = kl >> 32
        sec = np.sort(_bits(td)[tab], axis=1)[:, -2]                                # the second largest value of the lane, as a multiset
        cand, bound, total = [], 0, 0
        for w in range(WAVES):
            us = w * 64 + lanes
            thb = theta_b
            sel = us[vb[us] >= thb]
            exact = False
            had = len(sel)
            if had > CAP:
                lob, hib = theta_b, vlast_b + 1
                for _ in range(16):
                    mid = lob + ((hib - lob) >> 1)
                    if mid == lob:
                        break
                    s2 = us[vb[us] >= mid]
                    if len(s2) > CAP:
                        lob = mid
                    elif len(s2) == 0:
                        hib = mid
                    else:
                        sel, thb = s2, mid
                        break
                exact = len(sel) > CAP
            elif had == 0:
                exact = True
            if exact:
                best = kl[us].max()
                eq = us[kl[us] == best]
                if len(eq) > 1:                                                     # THE EQUAL-KEYS RULE: only among padding
                    assert best == 0 and not real[tab[eq]].any(), "equal lane keys among real slots"
                sel = eq[:1]                                                        # mk &= 0 - mk: the lowest lane
                if had != 0:
                    thb = int(vb[sel[0]]) + 1
            bound = max(bound, thb, int((sec[sel] + 1).max()))
            cand += list(sel)
            total += len(sel)
        cand = np.array(cand, dtype=np.int64)
        assert 1 <= len(cand) <= 64 and bound >= 1, "the uncounted loop ends by the bound exit only if the bound is >= 1"
        ckey = kl[cand]
        cbits, clo = ckey >> 32, ckey & 0xFFFFFFFF
        stats["padding_candidates"] += int((clo == 0).sum()) if n < ns else 0
        # mirror row of a candidate: the real point with that low word; row 0 (padding) holds whatever the staging left there --
        # modelled as point 0's position, its value is 0 and stays 0 whatever the coordinates are
        item_of_low = np.zeros(ns, dtype=np.int64)
        item_of_low[low[real]] = k[real]
        citem = np.where((clo > 0) | (n == ns), item_of_low[clo], -1)
        cpos = np.where((citem >= 0)[:, None], pos[np.maximum(citem, 0)], x[0]).astype(F)
        cval = np.array([_float(b) for b in cbits], dtype=F)
        taken = np.zeros(len(cand), dtype=bool)

        def cur_bits():
            return np.where(taken, -1, _bits(cval))                                 # a taken lane holds -1.0f: negative as an integer

        def exact_argmax():
            b = cur_bits()
            bh = int(b.max())
            eq = np.nonzero(b == bh)[0]
            if len(eq) > 1:
                ml = clo[eq].max()
                eq = eq[clo[eq] == ml][:1]                                          # equal keys exist only among padding slots
            return int(eq[0]), bh

        amax = min(m - len(out), 64)
        counted = amax < 64                                                         # PN2_BT_NOCTR: only a batch that could pass the end of the row counts
        c, bh = exact_argmax()                                                      # the batch's first sample: always accepted
        a = 0
        for guard in range(65):
            assert guard < 64, "the sample loop did not end: more samples than the ring has rows"
            assert citem[c] >= 0, "padding candidate picked at sample %d" % len(out)
            accept(int(citem[c]), cval[c], "batch")
            a += 1
            vlast_b = bh
            taken[c] = True
            if counted and a >= amax:
                break
            ms = max(int(cur_bits().max()) if not taken.all() else 0, 0)            # lanes without a DPP source read 0
            d = _sqdist(pos, pos[citem[c]])
            np.minimum(td, d, out=td)
            cval = np.minimum(cval, _sqdist(cpos, pos[citem[c]]))
            if ms < bound:
                break
            eq = np.nonzero(cur_bits() == ms)[0]
            if len(eq) == 1:
                c, bh = int(eq[0]), ms
            else:
                c, bh = exact_argmax()
                if bh < bound:
                    break
        assert 1 <= a <= 64, "every batch accepts at least one sample and never more than the ring holds"
        stats["batches"].append(a)
        if vlast_b == 0:                                                            # THE VALUE-0 TAIL: the rest is the winner's index
            assert a == 1 and out[-1] == 0, "the tail's sample is point 0 and the first of its batch"
            while len(out) < m:
                out.append(out[-1])
            break
        if total > LIST_HI:
            g = max(F(g * F(0.8)), F(1.0 / 128.0))
        elif total < LIST_LO:
            g = min(F(g * F(1.25)), F(0.5))
        theta_b = int(_bits(F(_float(vlast_b) * F(F(1.0) - g))))
        single = min(runs(len(stats["batches"])) if runs else 0, m - len(out))
        if single:
            for _ in range(single):
                vlast = single_round()
            vlast_b = int(_bits(vlast))
            theta_b = int(_bits(F(vlast * F(F(1.0) - G0))))
    assert len(out) == m
    return np.array(out, dtype=np.int32), stats


LENGTHS = [1, 2, 37, 512, 513, 600]
SLOTS = [1024, 8192]
SAMPLES = [1, 2, 47, 48, 49, 300]


@functools.lru_cache(maxsize=None)
def _cloud(n):
    return S.uniform_clouds(1, n, 100 + n)


@functools.lru_cache(maxsize=None)
def _want(n, m):
    import oracle as O
    return O.farthest_point_sample(m, _cloud(n))[0]


@pytest.mark.parametrize("m", SAMPLES)
@pytest.mark.parametrize("ns", SLOTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_a_mostly_padding_cloud_gives_the_oracles_chain(oracle, n, ns, m):
    got, stats = _padded_batched_fps(_cloud(n)[0], m, ns, seed=n + m)
    assert np.array_equal(got, _want(n, m)), "first mismatch at %s" % np.argwhere(got != _want(n, m))[:3].ravel()
    assert (got < n).all()
    if m > EARLY:
        assert len(stats["batches"]) >= 1 and min(stats["batches"]) >= 1
        if ns == 8192 and n <= 37:
            assert stats["padding_waves"] >= 1 and stats["padding_candidates"] >= 1, "the case is meant to hold all-padding waves"


@pytest.mark.parametrize("ns", SLOTS)
@pytest.mark.parametrize("n", [1, 37, 600])
def test_the_tail_inside_a_batch_and_without_the_early_rounds(oracle, n, ns):
    """early = 1: the first list is collected right behind sample 0 (theta = 1e38: every wave sends its exact best lane, the
    all-padding waves a padding lane), so the value-0 tail of a small cloud is reached inside the batches"""
    import oracle as O
    m = 2 * n + 3
    want = O.farthest_point_sample(m, _cloud(n))[0]
    got, stats = _padded_batched_fps(_cloud(n)[0], m, ns, seed=7, early=1)
    assert np.array_equal(got, want)
    assert (got[n:] == 0).all()


@pytest.mark.parametrize("make", [S.lattice_clouds, S.duplicated_clouds, S.identical_clouds], ids=["lattice", "duplicated", "identical"])
def test_ties_and_exhausted_clouds_under_a_large_template(oracle, make):
    import oracle as O
    clouds = make(1, 600, 17)
    want = O.farthest_point_sample(300, clouds)[0]
    for runs in (None, lambda b: 16 if b % 3 == 2 else 0):
        got, _ = _padded_batched_fps(clouds[0], 300, 8192, seed=3, runs=runs)
        assert np.array_equal(got, want), "first mismatch at %s" % np.argwhere(got != want)[:3].ravel()


def test_the_dealing_is_irrelevant(oracle):
    """which padding item lands on which side of a cut is timing dependent on the device (tickets): any draw gives the chain"""
    for seed in range(4):
        got, _ = _padded_batched_fps(_cloud(37)[0], 60, 8192, seed=seed)
        assert np.array_equal(got, _want(37, 60))
