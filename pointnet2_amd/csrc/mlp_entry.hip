// mlp_entry.hip -- the C entry points of the fused inference MLPs (include/pn2ops.h: pn2_sa_mlp3_*, pn2_fp_mlp*): validate,
// build the stack's PLAN, switch on the plan's family (each family's _pick / _pack / _launch: sa_mlp_common.h). A plan is a
// plain value built per call from the stack's shape alone: nothing is cached and nothing is allocated.
#include "sa_mlp_common.h"

#include <limits.h>
#include <stdlib.h>

namespace pn2 {

// ---- set abstraction ------------------------------------------------------------------------------------------------
// Which kernel runs a stack: the resident one when the input is narrow and the weights fit in LDS, the streamed one up
// to widths (128,128,256), else the cooperative one (wide stacks such as (256,256,512) and the group_all level's
// (256,512,1024); any nsample, masked). The family numbers are pn2_sa_mlp3_config's info4[0].
enum { kSaResident = 0, kSaStreamed = 1, kSaCooperative = 2 };

struct SaPlan {
    int family, nsample;
    union {                                   // the family's configuration
        MlpResidentConfig rc;
        MlpStreamConfig sc;
        MlpCoopConfig cc;
    };
    int tiles[3];                             // 32-channel output tiles of the three layers, as reported
    size_t w_floats, b_floats;                // packed sizes
    // scratch of a call: the streamed kernel's per-point layer 1, the input of the cooperative family's last-layer GEMM
    size_t ws_bytes(long long b, long long n, long long m) const
    {
        if (family == kSaStreamed) return mlp_stream_ws_bytes(sc, b * n);
        if (family == kSaCooperative) return mlp_coop_ws_bytes(cc, 0, b * m, nsample);
        return 0;
    }
};

static bool sa_plan(int cin, int c1, int c2, int c3, int nsample, SaPlan &p)
{
    auto chosen = [&p](int family, int t1, int t2, int t3, size_t w_floats, size_t b_floats) {
        p.family = family;
        p.tiles[0] = t1; p.tiles[1] = t2; p.tiles[2] = t3;
        p.w_floats = w_floats; p.b_floats = b_floats;
        return true;
    };
    const bool whole = nsample == 16 || (nsample > 0 && nsample % 32 == 0);
    const int widths[3] = {c1, c2, c3};
    p.nsample = nsample;
    if (whole && mlp_resident_pick(cin, c1, c2, c3, p.rc))
        return chosen(kSaResident, p.rc.t1, p.rc.t2, p.rc.t3, mlp_resident_w_floats(p.rc), mlp_resident_b_floats(p.rc));
    if (whole && nsample != 16 && mlp_stream_pick(cin, c1, c2, c3, p.sc))
        return chosen(kSaStreamed, p.sc.t1, p.sc.t2, p.sc.t3, mlp_stream_w_floats(p.sc), mlp_stream_b_floats(p.sc));
    if (nsample > 0 && mlp_coop_pick(cin, 3, widths, p.cc) && mlp_coop_has_kernel(p.cc, 0))
        return chosen(kSaCooperative, 4 * p.cc.q1, 4 * p.cc.q2, 4 * p.cc.q3, mlp_coop_w_floats(p.cc), mlp_coop_b_floats(p.cc));
    return false;
}

// pn2_sa_mlp3_maxpool_ex, pn2_sa_mlp3_pool and pn2_sa_mlp3_maxpool_ragged behind their own range checks. ragged: the counts
// form (max pooling) -- grouped rows take npoints, the group_all form takes lengths; the plan and every launch dimension come
// from the padded extents as in the dense call, the kernels are the families' ragged twins.
static int sa_mlp3_run(int b, int n, int m, int nsample, int cfeat, const float *xyz, const float *new_xyz, const float *points,
                       const int *idx, int c1, int c2, int c3, const float *wpacked, const float *bpacked, float *out, void *ws,
                       int variant, int pooling, void *stream, bool ragged = false, const int *lengths = nullptr,
                       const int *npoints = nullptr)
{
    if (b < 0 || n <= 0 || m < 0 || cfeat < 0) return PN2_E_SHAPE;
    if (nsample <= 0) return PN2_E_ARG;
    if (b == 0 || m == 0) return PN2_OK;
    // idx == NULL and new_xyz == NULL together (max pooling only): the group_all level (sample_and_group_all,
    // pointnet_util.py:59-84): m = 1, the group is the whole cloud in index order (nsample = n), no centroid subtraction
    const bool group_all = pooling == 0 && !idx && !new_xyz;
    if (group_all && (m != 1 || nsample != n)) return PN2_E_ARG;
    if (!xyz || (!group_all && (!new_xyz || !idx)) || !wpacked || !bpacked || !out || (cfeat > 0 && !points)) return PN2_E_NULL;
    if (ragged && group_all && npoints) return PN2_E_ARG;
    if (ragged && !(group_all ? lengths : npoints)) return PN2_E_NULL;
    const int *counts = !ragged ? nullptr : group_all ? lengths : npoints;      // (grouped rows: lengths is not needed, idx stays below it)
    SaPlan p;
    if (!sa_plan(3 + cfeat, c1, c2, c3, nsample, p)) return PN2_E_TOO_LARGE;
    // only the cooperative kernel gathers without idx, and only the other two pool by anything but the maximum
    if (p.family == kSaCooperative ? pooling != 0 : group_all) return PN2_E_TOO_LARGE;
    hipStream_t st = as_stream(stream);
    const float *pts = cfeat > 0 ? points : nullptr;
    switch (p.family) {
    case kSaResident:
        return mlp_resident_launch(p.rc, b, n, m, nsample, cfeat, c3, xyz, new_xyz, pts, idx, wpacked, bpacked, out, st, variant, pooling, counts);
    case kSaStreamed:
        return mlp_stream_launch(p.sc, b, n, m, nsample, cfeat, c3, xyz, new_xyz, pts ? pts : xyz, idx, wpacked, bpacked, out, ws, st, pooling, counts);
    default: {
        CoopParams cp = {n, m, nsample, cfeat, 0, c3, p.cc.ti, (long long)b * m, xyz, new_xyz, pts, nullptr, idx, nullptr,
                         wpacked, bpacked, out, 0, counts};
        return mlp_coop_launch(p.cc, 0, cp, st, ws);
    }
    }
}

// ---- feature propagation ----------------------------------------------------------------------------------------------
// family = the caller's `kind` (fp_mlp.hip / coop_mlp.hip: same results, different packing). Packed weights: [the family's
// own stream][per-point kernel: known-feature rows of layer 1]; packed bias: [the family's own][kFpZeroBias zeros: the
// per-point kernel adds no bias, the interpolation weights multiply Q only].
constexpr int kFpZeroBias = 128;
enum { kFpStreamed = 0, kFpCooperative = 1 };

struct FpPlan {
    int family;
    union {
        FpConfig fc;
        MlpCoopConfig cc;
    };
    int tiles[4];                             // tiles of skip channels, of layers 1, 2, 3, as reported
    int tif;                                  // tiles of known features (c2)
    size_t wpoint, zeros;                     // where the per-point stream / the zero bias start = the family's own sizes
    size_t w_floats, b_floats;
    size_t ws_bytes(long long b, long long m) const { return sizeof(float) * (size_t)(b * m) * 32 * tiles[1]; }
};

static bool fp_plan(int c2, int c1, int nlayers, const int *widths, int kind, FpPlan &p)
{
    auto chosen = [&p, c2](int ti, int t1, int t2, int t3, size_t w_own, size_t b_own) {
        p.tiles[0] = ti; p.tiles[1] = t1; p.tiles[2] = t2; p.tiles[3] = t3;
        p.tif = (c2 + 31) / 32;
        p.wpoint = w_own; p.zeros = b_own;
        p.w_floats = w_own + (size_t)p.tif * t1 * kPairWords;          // (t1 is 4 or 8: whole stages)
        p.b_floats = b_own + kFpZeroBias;
        return true;
    };
    p.family = kind;
    if (kind == kFpCooperative) {
        if (!mlp_coop_pick(c1, nlayers, widths, p.cc) || !mlp_coop_has_kernel(p.cc, 1)) return false;
        return chosen(p.cc.ti, 4 * p.cc.q1, 4 * p.cc.q2, 4 * p.cc.q3, mlp_coop_w_floats(p.cc), mlp_coop_b_floats(p.cc));
    }
    if (!fp_stream_pick(c2, c1, nlayers, widths, p.fc)) return false;
    return chosen(p.fc.ti, p.fc.t1, p.fc.t2, p.fc.t3, fp_stream_w_floats(p.fc), fp_stream_b_floats(p.fc));
}

// Q = points2 . W1a: few known points (most FP levels) -> one workgroup per (item, output tile), no staging;
// many -> the streamed per-point kernel, 128 output channels per launch
static int fp_point_layer(int t1, long long known_rows, int c2, int tif, const float *points2, const float *wpoint,
                          const float *zero_bias, float *pre, hipStream_t st)
{
    if (point_layer_prefers_few_rows(known_rows, t1, tif)) return point_layer_few_rows_launch(t1, c2, known_rows, tif, points2, wpoint, nullptr, pre, st);
    for (int half = 0; half < t1 / 4; ++half)
        if (int rc = point_layer_launch(4, c2, known_rows, tif, points2, wpoint + (size_t)half * tif * 4 * kPairWords, zero_bias,
                                        pre, 32 * t1, 128 * half, st)) return rc;
    return PN2_OK;
}

}  // namespace pn2

extern "C" int pn2_sa_mlp3_config(int cin, int c1, int c2, int c3, int nsample, int *info4, long long *w_floats,
                                  long long *b_floats)
{
    using namespace pn2;
    if (cin < 3 || c1 <= 0 || c2 <= 0 || c3 <= 0 || nsample <= 0) return PN2_E_ARG;
    SaPlan p;
    if (!sa_plan(cin, c1, c2, c3, nsample, p)) return PN2_E_TOO_LARGE;
    if (info4) { info4[0] = p.family; info4[1] = p.tiles[0]; info4[2] = p.tiles[1]; info4[3] = p.tiles[2]; }
    if (w_floats) *w_floats = (long long)p.w_floats;
    if (b_floats) *b_floats = (long long)p.b_floats;
    return PN2_OK;
}

extern "C" int pn2_sa_mlp3_pack(int cin, int c1, int c2, int c3, int nsample, int xyz_first, const float *w1,
                                const float *bias1, const float *w2, const float *bias2, const float *w3,
                                const float *bias3, float *wpacked, float *bpacked)
{
    using namespace pn2;
    SaPlan p;
    if (cin < 3 || c1 <= 0 || c2 <= 0 || c3 <= 0 || !sa_plan(cin, c1, c2, c3, nsample, p)) return PN2_E_TOO_LARGE;
    if (!w1 || !w2 || !w3 || !bias1 || !bias2 || !bias3 || !wpacked || !bpacked) return PN2_E_NULL;
    const float *ws[3] = {w1, w2, w3}, *bs[3] = {bias1, bias2, bias3};
    switch (p.family) {
    case kSaResident:
        mlp_resident_pack(p.rc, cin, c1, c2, c3, xyz_first, ws, bs, wpacked, bpacked);
        break;
    case kSaStreamed:
        mlp_stream_pack(p.sc, cin, c1, c2, c3, xyz_first, ws, bs, wpacked, bpacked);
        break;
    default: {
        // kernel channel order of layer 1: [features, xyz]; caller's weight rows: [xyz, features] when xyz_first
        const int cf = cin - 3, widths[3] = {c1, c2, c3};
        int *krow = (int *)malloc(sizeof(int) * (size_t)cin);
        for (int k = 0; k < cin; ++k) krow[k] = xyz_first ? (k < cf ? 3 + k : k - cf) : k;
        mlp_coop_pack(p.cc, cin, 3, widths, krow, ws, bs, wpacked, bpacked, true);
        free(krow);
    }
    }
    return PN2_OK;
}

extern "C" long long pn2_sa_mlp3_ws_bytes(int b, int n, int m, int cin, int c1, int c2, int c3, int nsample)
{
    using namespace pn2;
    SaPlan p;
    if (b <= 0 || n <= 0 || m <= 0 || cin < 3 || c1 <= 0 || c2 <= 0 || c3 <= 0 || nsample <= 0) return 0;
    if (!sa_plan(cin, c1, c2, c3, nsample, p)) return 0;
    return (long long)p.ws_bytes(b, n, m);
}

extern "C" int pn2_sa_mlp3_maxpool(int b, int n, int m, int nsample, int cfeat, const float *xyz, const float *new_xyz,
                                   const float *points, const int *idx, int c1, int c2, int c3, const float *wpacked,
                                   const float *bpacked, float *out, void *ws, void *stream)
{
    return pn2::sa_mlp3_run(b, n, m, nsample, cfeat, xyz, new_xyz, points, idx, c1, c2, c3, wpacked, bpacked, out, ws, 0, 0, stream);
}

extern "C" int pn2_sa_mlp3_maxpool_ex(int b, int n, int m, int nsample, int cfeat, const float *xyz, const float *new_xyz,
                                      const float *points, const int *idx, int c1, int c2, int c3, const float *wpacked,
                                      const float *bpacked, float *out, void *ws, int variant, void *stream)
{
    if (variant < 0 || variant > 3) return PN2_E_ARG;
    return pn2::sa_mlp3_run(b, n, m, nsample, cfeat, xyz, new_xyz, points, idx, c1, c2, c3, wpacked, bpacked, out, ws, variant, 0, stream);
}

extern "C" int pn2_sa_mlp3_maxpool_ragged(int b, int n, int m, int nsample, int cfeat, const float *xyz, const int *lengths,
                                          const float *new_xyz, const int *npoints, const float *points, const int *idx, int c1,
                                          int c2, int c3, const float *wpacked, const float *bpacked, float *out, void *ws,
                                          int variant, void *stream)
{
    if (variant < 0 || variant > 3) return PN2_E_ARG;
    return pn2::sa_mlp3_run(b, n, m, nsample, cfeat, xyz, new_xyz, points, idx, c1, c2, c3, wpacked, bpacked, out, ws, variant, 0, stream,
                            true, lengths, npoints);
}

extern "C" int pn2_sa_mlp3_pool_supported(int cin, int c1, int c2, int c3, int nsample, int pooling)
{
    using namespace pn2;
    if (pooling < 0 || pooling > 3 || cin < 3 || c1 <= 0 || c2 <= 0 || c3 <= 0 || nsample <= 0) return 0;
    SaPlan p;
    if (!sa_plan(cin, c1, c2, c3, nsample, p)) return 0;
    return pooling == 0 || p.family != kSaCooperative;
}

// pooling: 0 max, 1 avg, 2 weighted_avg, 3 max_and_avg (out is (b, m, 2 c3): [avg, max]); modes 1-3 only on the resident
// and the streamed family's stacks (pn2_sa_mlp3_pool_supported), else PN2_E_TOO_LARGE: the caller goes layer by layer
extern "C" int pn2_sa_mlp3_pool(int b, int n, int m, int nsample, int cfeat, const float *xyz, const float *new_xyz,
                                const float *points, const int *idx, int c1, int c2, int c3, const float *wpacked,
                                const float *bpacked, int pooling, float *out, void *ws, void *stream)
{
    if (pooling < 0 || pooling > 3) return PN2_E_ARG;
    return pn2::sa_mlp3_run(b, n, m, nsample, cfeat, xyz, new_xyz, points, idx, c1, c2, c3, wpacked, bpacked, out, ws, 0, pooling, stream);
}

// tiles4 = {tiles of skip channels, tiles of layer 1, 2, 3}.
extern "C" int pn2_fp_mlp_config(int c2, int c1, int nlayers, const int *widths, int kind, int *tiles4, long long *w_floats,
                                 long long *b_floats)
{
    using namespace pn2;
    if (c2 <= 0 || c1 < 0 || !widths || (kind != 0 && kind != 1)) return PN2_E_ARG;
    FpPlan p;
    if (!fp_plan(c2, c1, nlayers, widths, kind, p)) return PN2_E_TOO_LARGE;
    if (tiles4) { tiles4[0] = p.tiles[0]; tiles4[1] = p.tiles[1]; tiles4[2] = p.tiles[2]; tiles4[3] = p.tiles[3]; }
    if (w_floats) *w_floats = (long long)p.w_floats;
    if (b_floats) *b_floats = (long long)p.b_floats;
    return PN2_OK;
}

// Scratch of a pn2_fp_mlp call: Q = points2 . W1a, one row of the padded first width per known point.
extern "C" long long pn2_fp_mlp_ws_bytes(int b, int m, int c2, int c1, int nlayers, const int *widths, int kind)
{
    using namespace pn2;
    if (b <= 0 || m <= 0 || c2 <= 0 || c1 < 0 || !widths || (kind != 0 && kind != 1)) return 0;
    FpPlan p;
    if (!fp_plan(c2, c1, nlayers, widths, kind, p)) return 0;
    return (long long)p.ws_bytes(b, m);
}

// Host code: permute (cin_i, cout_i) row-major weights (rows of layer 1 in the reference's concat order
// [interpolated, points1]) into the tile-pair streams the chosen kernel and the per-point kernel consume.
extern "C" int pn2_fp_mlp_pack(int c2, int c1, int nlayers, const int *widths, int kind, const float *const *w,
                               const float *const *bias, float *wpacked, float *bpacked)
{
    using namespace pn2;
    if (c2 <= 0 || c1 < 0 || !widths || !w || !bias || !wpacked || !bpacked) return PN2_E_NULL;
    if (kind != 0 && kind != 1) return PN2_E_ARG;
    FpPlan p;
    if (!fp_plan(c2, c1, nlayers, widths, kind, p)) return PN2_E_TOO_LARGE;
    int *skip_row = (int *)malloc(sizeof(int) * (size_t)(c1 > 0 ? c1 : 1));
    for (int k = 0; k < c1; ++k) skip_row[k] = c2 + k;              // rows of w[0] behind the interpolated channels
    if (p.family == kFpCooperative) mlp_coop_pack(p.cc, c1, nlayers, widths, skip_row, w, bias, wpacked, bpacked, false);
    else fp_stream_pack(p.fc, c1, nlayers, widths, skip_row, w, bias, wpacked, bpacked);
    free(skip_row);
    // the per-point kernel's streams: known-feature rows of layer 1, 128 output channels (4 tiles) per stream, feature
    // tiles outermost
    float *wp = wpacked + p.wpoint;
    for (int half = 0; half < p.tiles[1] / 4; ++half)
        for (int u = 0; u < p.tif; ++u)
            for (int t = 4 * half; t < 4 * half + 4; ++t) wp = mlp_pack_pair_x6(wp, w[0], c2, widths[0], t, u, nullptr);
    for (int i = 0; i < kFpZeroBias; ++i) bpacked[p.zeros + i] = 0.0f;
    return PN2_OK;
}

namespace pn2 {
static int fp_mlp_run(int b, int n, int m, int c2, int c1, const float *points2, const float *points1, const int *idx,
                      const float *dist, int nlayers, const int *widths, int kind, const float *wpacked, const float *bpacked,
                      float *out, void *ws, void *stream, bool ragged, const int *lengths1);
}

extern "C" int pn2_fp_mlp(int b, int n, int m, int c2, int c1, const float *points2, const float *points1, const int *idx,
                          const float *dist, int nlayers, const int *widths, int kind, const float *wpacked,
                          const float *bpacked, float *out, void *ws, void *stream)
{
    return pn2::fp_mlp_run(b, n, m, c2, c1, points2, points1, idx, dist, nlayers, widths, kind, wpacked, bpacked, out, ws, stream, false,
                           nullptr);
}

extern "C" int pn2_fp_mlp_ragged(int b, int n, int m, int c2, int c1, const float *points2, const float *points1, const int *lengths1,
                                 const int *idx, const float *dist, int nlayers, const int *widths, int kind, const float *wpacked,
                                 const float *bpacked, float *out, void *ws, void *stream)
{
    return pn2::fp_mlp_run(b, n, m, c2, c1, points2, points1, idx, dist, nlayers, widths, kind, wpacked, bpacked, out, ws, stream, true,
                           lengths1);
}

// pn2_fp_mlp (ragged == false) and pn2_fp_mlp_ragged (lengths1 required): Q = points2 . W1a for every known row either way
// (rows of points2 beyond a cloud's known count are multiplied and never gathered), then the family's dense kernel or its twin
int pn2::fp_mlp_run(int b, int n, int m, int c2, int c1, const float *points2, const float *points1, const int *idx,
                           const float *dist, int nlayers, const int *widths, int kind, const float *wpacked, const float *bpacked,
                           float *out, void *ws, void *stream, bool ragged, const int *lengths1)
{
    using namespace pn2;
    if (b < 0 || n < 0 || m <= 0 || c2 <= 0 || c1 < 0) return PN2_E_SHAPE;
    if (!widths) return PN2_E_NULL;
    if (kind != 0 && kind != 1) return PN2_E_ARG;
    FpPlan p;
    if (!fp_plan(c2, c1, nlayers, widths, kind, p)) return PN2_E_TOO_LARGE;
    const long long rows = (long long)b * n;
    if (rows == 0) return PN2_OK;
    if (!points2 || (c1 > 0 && !points1) || !idx || !dist || !wpacked || !bpacked || !out || !ws) return PN2_E_NULL;
    if (ragged && !lengths1) return PN2_E_NULL;
    if ((long long)m * c2 > INT_MAX) return PN2_E_TOO_LARGE;
    const int cout = widths[nlayers - 1];
    hipStream_t st = as_stream(stream);
    float *pre = (float *)ws;
    if (int rc = fp_point_layer(p.tiles[1], (long long)b * m, c2, p.tif, points2, wpacked + p.wpoint, bpacked + p.zeros, pre, st)) return rc;
    if (p.family == kFpCooperative) {
        CoopParams cp = {n, m, 0, c2, c1, cout, p.cc.ti, rows, nullptr, nullptr, pre, c1 > 0 ? points1 : nullptr, idx, dist,
                         wpacked, bpacked, out, 0, ragged ? lengths1 : nullptr};
        return mlp_coop_launch(p.cc, 1, cp, st, nullptr);
    }
    return fp_stream_launch(p.fc, rows, n, m, c1, cout, pre, points1, idx, dist, wpacked, bpacked, out, st, ragged ? lengths1 : nullptr);
}
