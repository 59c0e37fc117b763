"""The hand-over between two candidate lists of the batched FPS tier (csrc/fps_batch_body.h): the places of a
list that no wave filled hold an invalid key the picker wrote a batch earlier (no count per wave), every updater wave raises ONE
bound word and adds to ONE total, one store of the picker clears the other parity's bound, total and count, and the sample loop
counts by an LDS add. The cases aim at what that can break; every case runs three ways -- the batched
tier forced against the full tier and the CPU oracle with a guard row behind the output, and once through
pn2_sample_and_group_xyz_ex -- and indices are bit-exact.

A case must do what its name says: `_trace` below restates tests/test_fps_batch_model.py's chain with its helpers and records,
per batch, what every wave contributed (lanes, bisection steps, exact fallback), who decided the bound, how the batch ended. The
property of each case is asserted on that trace before the GPU runs. `_lanes` below deals points to lanes as the kernel does at
each size: 32 groups at 4096 rank slots (the model file's dealing, the one P = 8 case), 16 at 2048, 8 at 1024
(fps_pruned_prologue: pr_k0 / pr_k1 / pr_k2 cuts, leaf id -> wave id % 8). Neither dealing is the kernel's to the point: the
kernel cuts by 64 bins per axis and orders the items of one bin by an LDS ticket, which is timing dependent, so no model has the
GPU's very lists; the trace shows that the cloud makes lists of the named kind under the kernel's grouping. The slow-batch run
itself is the kernel's clock's decision and is not observed here: the model asserts that the cloud's batches yield under two
samples each, which is what makes the kernel leave them (SLOW BATCHES in the header)."""
import functools

import numpy as np
import pytest
import torch

from pointnet2_amd import synthetic as S

pytestmark = pytest.mark.gpu

FPS_FULL, FPS_BATCH = 1, 3      # include/pn2ops.h


def _lanes(x):
    """point -> wave * 64 + lane at the kernel's grouping of this size. 4096 rank slots: the model file's 32 leaves. 2048 / 1024:
    16 = 4 x 2 x 2 / 8 = 2 x 2 x 2 leaves of equal size along the axes sorted by extent, leaf id = (a * K1 + i1) * K2 + i2 -> wave
    id % 8, position p of the leaf -> lane p % 64 (fps_pruned_prologue, the branch for fewer than 32 groups)."""
    import test_fps_batch_model as M
    n = x.shape[0]
    assert n in (1024, 2048, 4096), "no padding items in these cases: the rank slots are the points"
    if n == 4096:
        return M._lanes(x, 16)
    k0, k1, k2 = (4, 2, 2) if n == 2048 else (2, 2, 2)
    ext = x.max(axis=0) - x.min(axis=0)
    a0, a1, a2 = np.argsort(-ext, kind="stable")
    unit = np.zeros(n, dtype=np.int64)
    for a, p0 in enumerate(np.array_split(np.argsort(x[:, a0], kind="stable"), k0)):
        for i1, p1 in enumerate(np.array_split(p0[np.argsort(x[p0, a1], kind="stable")], k1)):
            for i2, p2 in enumerate(np.array_split(p1[np.argsort(x[p1, a2], kind="stable")], k2)):
                leaf = (a * k1 + i1) * k2 + i2
                unit[p2] = (leaf % M.WAVES) * 64 + np.arange(len(p2)) % 64
    return unit


def _trace(x, m, lanes=_lanes):
    """test_fps_batch_model._batched_fps with the COLLECT vectorised, the dealing of `lanes` and a record per batch. Returns
    (indices, records)."""
    from test_fps_batch_model import CAP, EARLY, F, G0, LIST_HI, LIST_LO, REF_THREADS, WAVES, _bits, _bits_to_float, _sqdist
    x = x.astype(F)
    n = x.shape[0]
    q = (n + REF_THREADS - 1) // REF_THREADS
    rank = (np.arange(n) % REF_THREADS) * q + np.arange(n) // REF_THREADS
    unit = lanes(x)
    td = np.minimum(np.full(n, 1e38, dtype=F), _sqdist(x, x[0]))
    out = [0]

    def argmax_all():
        c = np.nonzero(td == td.max())[0]
        return int(c[np.argmin(rank[c])])

    vlast = F(1e38)
    while len(out) < min(EARLY, m):
        p = argmax_all()
        vlast = td[p]
        out.append(p)
        td = np.minimum(td, _sqdist(x, x[p]))
    g = G0
    theta_b = int(_bits(F(vlast * F(F(1.0) - g)))) if len(out) > 1 else int(_bits(F(1e38)))
    vlast_b = int(_bits(vlast))
    recs = []
    while len(out) < m:
        # per lane: best point (value, then rank) and second-best value
        o = np.lexsort((rank, -_bits(td), unit))
        first = np.r_[True, unit[o][1:] != unit[o][:-1]]
        heads = np.nonzero(first)[0]
        us_all = unit[o][heads]
        best = o[heads]
        nxt = np.minimum(heads + 1, n - 1)
        has2 = (heads + 1 < n) & (unit[o][nxt] == us_all)
        vb = _bits(td[best])
        sb = np.where(has2, _bits(td[o[nxt]]), 0)
        rec = dict(j=len(out), cnt=[], bis=[], exact=[], theta=theta_b)
        cand, src = [], ("theta", -1, theta_b)
        for w in range(WAVES):
            iw = np.nonzero(us_all // 64 == w)[0]
            thb, steps = theta_b, 0
            sel = iw[vb[iw] >= thb]
            exact = False
            if len(sel) > CAP:
                lob, hib = theta_b, vlast_b + 1
                for _ in range(16):
                    mid = lob + ((hib - lob) >> 1)
                    if mid == lob:
                        break
                    steps += 1
                    s2 = iw[vb[iw] >= mid]
                    if len(s2) > CAP:
                        lob = mid
                    elif len(s2) == 0:
                        hib = mid
                    else:
                        sel, thb = s2, mid
                        break
                exact = len(sel) > CAP
            elif len(sel) == 0:
                exact = True
            if exact:
                had = len(sel)
                oo = np.lexsort((rank[best[iw]], -vb[iw]))
                sel = iw[oo[:1]]
                if had != 0:
                    thb = int(vb[sel[0]]) + 1
            sec = int((sb[sel] + 1).max())
            # who decides the bound: a wave's own raised threshold (bisection, equal values), a candidate lane's second-best
            # value, or theta itself (every wave's threshold alike)
            for kind, v in (("thr", thb if thb > theta_b else -1), ("sec", sec)):
                if v > src[2]:
                    src = (kind, w, v)
            rec["cnt"].append(len(sel)); rec["bis"].append(steps); rec["exact"].append(exact)
            cand += list(sel)
        bound = src[2]
        rec["src"] = src
        cand = np.array(cand, dtype=np.int64)
        cp = best[cand]
        cv = td[cp].copy()
        alive = np.ones(len(cp), dtype=bool)
        a, ended = 0, "list"
        while True:
            if len(out) >= m:
                ended = "row"
                break
            live = np.nonzero(alive)[0]
            if len(live) == 0 or a >= 64:
                break
            oo = np.lexsort((rank[cp[live]], -_bits(cv[live])))
            c = live[oo[0]]
            bh = int(_bits(cv[c]))
            if a > 0 and bh < bound:
                ended = "bound"
                break
            p = int(cp[c])
            out.append(p)
            a += 1
            vlast_b = bh
            alive[c] = False
            d = _sqdist(x, x[p])
            td = np.minimum(td, d)
            cv = np.minimum(cv, d[cp])
            if bh == 0:
                ended = "zero"
                break
        rec.update(a=a, total=len(cand), ended=ended)
        recs.append(rec)
        if ended == "zero":
            out += [out[-1]] * (m - len(out))
            break
        if len(cand) > LIST_HI:
            g = max(F(g * F(0.8)), F(1.0 / 128.0))
        elif len(cand) < LIST_LO:
            g = min(F(g * F(1.25)), F(0.5))
        theta_b = int(_bits(F(_bits_to_float(vlast_b) * F(F(1.0) - g))))
    return np.array(out, dtype=np.int32), recs


# ---- what a case's name promises, as a predicate on the trace of its cloud 0
def _mixed(recs):
    from test_fps_batch_model import CAP
    return any(min(r["cnt"]) == 1 and max(r["cnt"]) == CAP for r in recs)


def _all_exact(recs):
    from test_fps_batch_model import WAVES
    return any(all(r["exact"]) and r["total"] == WAVES for r in recs)


def _one_list(recs):
    return len(recs) == 1


def _bound_moves(recs):
    """a candidate lane's second-best value decides one batch, ANOTHER wave's raised threshold the next: both parities' word"""
    return any(a["src"][0] == "sec" and b["src"][0] == "thr" and a["src"][1] != b["src"][1] for a, b in zip(recs, recs[1:]))


def _bisects(recs):
    return any(max(r["bis"]) > 0 and not r["exact"][int(np.argmax(r["bis"]))] for r in recs)


def _bisects_or_ties(recs):
    return any(max(r["bis"]) > 0 for r in recs)


def _ends_at_zero(recs):
    """the chain runs out of distinct points while it takes lists (not in the early rounds): the sample of value 0 is the first of
    its list -- no later one can be, the bound is >= 1 as an integer -- and the fill flag travels with that batch's end flag"""
    return recs[-1]["ended"] == "zero" and len(recs) >= 3


def _odd_and_even(recs):
    return any(r["a"] % 2 == 1 and r["a"] > 2 for r in recs) and any(r["a"] % 2 == 0 and r["a"] > 2 for r in recs)


def _big_batch(recs):
    return max(r["a"] for r in recs) >= 48


def _row_ends_inside(recs):
    return recs[-1]["ended"] == "row" and recs[-1]["a"] >= 2


def _slow(recs):
    return len(recs) >= 20 and np.mean([r["a"] for r in recs]) < 2.0


def _quantised(b, n, seed, q):
    return (np.round(S.uniform_clouds(b, n, seed) * q) / q).astype(np.float32)


def _picker_gen(name):
    import test_fps_picker_loop_gpu as L
    return getattr(L, name)


def _model_lanes(x):
    from test_fps_batch_model import _lanes as model_lanes
    return model_lanes(x, 16)


def _ladders():
    L = _picker_gen("LADDER")
    return _picker_gen("_ladder_clouds")(), L["m"]


CASES = [
    # ---- invalid lanes
    ("mixed_lists_4096", lambda: S.sphere_clouds(2, 4096, 401), 512, _mixed),           # the P = 8 code the benchmark runs
    ("mixed_lists_2048", lambda: S.uniform_clouds(3, 2048, 402), 400, _mixed),
    ("all_exact_lattice", lambda: _picker_gen("_lattice16")(2, 2048, 403), 300, _all_exact),
    ("first_list_is_last", lambda: S.sphere_clouds(4, 1024, 404), 49, _one_list),
    # ---- the shared bound word
    ("bound_moves_2048", lambda: S.duplicated_clouds(2, 2048, 405), 500, _bound_moves),
    # ---- bisection
    ("bisect_sphere2048", lambda: S.sphere_clouds(2, 2048, 406), 600, _bisects),
    ("bisect_lattice16", lambda: _picker_gen("_lattice16")(2, 2048, 309), 600, _bisects_or_ties),
    ("bisect_doubled", lambda: _picker_gen("_doubled")(2, 2048, 310), 700, _bisects_or_ties),
    # ---- a chain that ends at value 0 inside a list, with fill
    ("zero_inside_list", lambda: S.dropout_clouds(3, 2048, 407, ratio=0.9), 512, _ends_at_zero),
    # ---- more samples than points
    ("m_gt_n_1024", lambda: S.uniform_clouds(2, 1024, 408), 1100, _ends_at_zero),
    # ---- count by add
    ("odd_even_batches", lambda: S.sphere_clouds(2, 1024, 409), 400, _odd_and_even),
    # (the 52-sample batch is the one tests/test_fps_picker_loop_gpu.py found, with the model file's dealing: asserted with that
    # one; under the 16-group dealing this cloud's largest batch is 31 of a list of 47)
    ("ladders2048", lambda: _ladders()[0], None, _big_batch, _model_lanes),
    ("row_ends_inside_list", lambda: S.uniform_clouds(2, 2048, 410), 301, _row_ends_inside),
    # ---- a run of one-per-exchange rounds between two lists: the preset list waits through the picker's barrier-only stretch
    ("slow_quantised", lambda: _quantised(2, 2048, 411, 16.0), 600, _slow),
]


@functools.lru_cache(maxsize=None)
def _case(name):
    for c in CASES:
        if c[0] == name:
            xyz = np.ascontiguousarray(c[1](), dtype=np.float32)
            m = c[2] if c[2] is not None else _ladders()[1]
            idx, recs = _trace(xyz[0], m, c[4] if len(c) > 4 else _lanes)
            return xyz, m, idx, recs, c[3]
    raise KeyError(name)


def test_the_trace_is_the_model():
    """the instrumented chain, with the model file's dealing, takes the batches of tests/test_fps_batch_model.py's"""
    from test_fps_batch_model import _batched_fps
    x = S.sphere_clouds(1, 2048, 499)[0]
    want, batches = _batched_fps(x, 300)
    got, recs = _trace(x, 300, _model_lanes)
    assert np.array_equal(got, want) and [r["a"] for r in recs] == batches


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_list_handoff_index_exact(cuda, oracle, name):
    from pointnet2_amd import _C
    xyz, m, model_idx, recs, prop = _case(name)
    b, n, _ = xyz.shape
    print("%s: batches %s, list sizes %s" % (name, [r["a"] for r in recs][:40], [r["total"] for r in recs][:40]))
    assert prop(recs), "%s: the model's chain does not do what the case's name says" % name
    want = oracle.farthest_point_sample(m, xyz)
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
