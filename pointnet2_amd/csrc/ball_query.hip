// ball_query.hip -- query_ball_point (+ optional fused group of xyz) for gfx950.
//
// Replaces query_ball_point_gpu / queryBallPointLauncher (reference
// tf_ops/grouping/tf_grouping_g.cu:3-36, :125-128; CPU twin
// tf_ops/grouping/test/query_ball_point.cpp:19-47). Index-exact:
//   * the reference predicate max(sqrtf(s),1e-20f) < radius is evaluated as
//     s < s*, with s* the smallest fp32 whose predicate is false, found on the
//     host by bisection with the host's correctly rounded sqrtf
//     (pn2_ball_threshold). sqrtf is monotone, so the two are identical for
//     every s, and no device sqrt (whatever its rounding) is involved;
//   * s itself is the fp32 value ((dx*dx)+(dy*dy))+(dz*dz), no FMA.
//
// Design (DESIGN.md "ball query"). The reference walks the cloud with ONE
// thread per query. Here one 64-lane wave owns a query and sweeps the cloud 64
// candidates at a time in ascending index order: the cloud is staged once per
// workgroup in LDS as float4 (one ds_read_b128 per lane per step), the hit
// mask is a v_cmp (ballot), v_mbcnt gives each hit its ordered output slot,
// and the sweep stops (wave-uniformly) as soon as nsample hits are in. A wave
// sweeps TWO queries at once over 128 candidates per trip, so every LDS read
// feeds two distance chains and four independent chains are in flight per lane
// (the one-query, one-chunk first version was latency bound: 123 us at the
// metric shape). The result row is assembled in an LDS row buffer and leaves the CU as ONE
// coalesced store per query (the reference scatters 4-byte stores). With
// FUSE the same epilogue also emits xyz1[idx]-centroid straight from the LDS
// copy of the cloud (pointnet_util.py:44-46 needs three ops and two extra
// passes over idx for this).
//
// Two kernels share the exact predicate and the output stage. The SWEEP kernel above is O(m*n) with
// an early exit; the CELL-LIST kernel (ball_query_cells_kernel, device code in the second half of
// ball_query_body.h) bins the cloud per workgroup and visits ~27 cells per query: 57 -> 24 us at the
// metric shape. bq_use_cells() picks by shape; the cell-list kernel falls back to the sweep body by
// itself when the data make the grid useless (coarse grid, crowded cells).
#include "ball_query_body.h"

#include <limits.h>
#include <math.h>
#include <string.h>

namespace pn2 {

// One kernel, three modes (pn2_device.h: Counts). No count array: the dense kernel, the cloud index addresses the tensors.
// One (pn2_query_ball_group_xyz_ragged): cloud c holds lengths1[c] <= n points in its padded (n, 3) slab. The workgroup hands
// the body its own slabs as cloud 0 with n = n_c: staging, the +inf pad and the sweep bounds are those of the dense kernel on
// the slice, rows at or beyond n_c are never addressed. The LDS is sized on the host for the padded n (both layouts grow with n).
// Two (pn2_query_ball_group_xyz_ragged_pair): cloud c also holds only m_c = lengths2[c] valid queries. The workgroup sweeps
// [q0, min(q0 + qpb, m_c)) -- the body never reads a query row at or beyond its q1 --, fills its rows from m_c on (bq_fill_rows)
// and, when it holds nothing else, leaves before the staging (block-uniform).
// Packed (pn2_query_ball_group_xyz_packed; pn2_device.h: Packed): the one-array mode with the cloud's slab taken from the
// offsets -- xyz1 is the flat (total, 3) array, n is nmax, the queries and the outputs stay dense (b, m, ...). With global_idx
// the stored indices are rows of the flat array; the grouped rows are gathered with the local index as before.
// Packed with one count array (pn2_query_ball_group_xyz_packed_pair): the two combined -- the slab from the offsets, m_c from
// lengths2; the fill rows store the cloud's own first row (offsets[c] under global_idx, else 0) as their index.
template <bool LDS_CLOUD, bool FUSE, class... Cnt>
__global__ __launch_bounds__(kBqThreads) void ball_query_kernel(int n, int m, int nsample, float thr, int qpb,
                                                                const float *__restrict__ xyz1,
                                                                const float *__restrict__ xyz2, int *__restrict__ idx,
                                                                int *__restrict__ pts_cnt,
                                                                float *__restrict__ grouped, int subtract, CountArg<Cnt>... cnt)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Counts<Cnt...> counts(cnt...);
    if constexpr (sizeof...(Cnt) == 0) {
        const int q0 = blockIdx.x * qpb;
        bq_block_body<LDS_CLOUD, FUSE, false>(n, m, nsample, thr, blockIdx.y, q0, min(q0 + qpb, m), xyz1, xyz2, nullptr,
                                              nullptr, idx, pts_cnt, grouped, subtract, smem);
    } else if constexpr (Counts<Cnt...>::packed) {
        const int c = blockIdx.y;
        const int start = cloud_start(counts.pk, c);
        const int nc = cloud_count(counts.pk, c, start, n);
        const int q0 = blockIdx.x * qpb;
        const size_t rows = (size_t)c * m;
        int mc = m;
        if constexpr (sizeof...(Cnt) == 2) {
            mc = cloud_count(counts.side[1], c, m);
            bq_fill_rows<kBqThreads>(max(q0, mc), min(q0 + qpb, m), nsample, idx ? idx + rows * nsample : nullptr,
                                     pts_cnt ? pts_cnt + rows : nullptr, grouped ? grouped + rows * nsample * 3 : nullptr,
                                     counts.pk.global_idx ? start : 0);
            if (q0 >= mc) return;
        }
        bq_block_body<LDS_CLOUD, FUSE, false>(nc, m, nsample, thr, 0, q0, min(q0 + qpb, mc), xyz1 + (size_t)start * 3, xyz2 + rows * 3,
                                              nullptr, nullptr, idx ? idx + rows * nsample : nullptr, pts_cnt ? pts_cnt + rows : nullptr,
                                              grouped ? grouped + rows * nsample * 3 : nullptr, subtract, smem, 1u, 0, nullptr,
                                              counts.pk.global_idx ? start : 0);
    } else {
        const int c = blockIdx.y;
        const int nc = cloud_count(counts.side[0], c, n);
        int mc = m;
        if constexpr (sizeof...(Cnt) == 2) mc = cloud_count(counts.side[1], c, m);
        const int q0 = blockIdx.x * qpb;
        const size_t rows = (size_t)c * m;
        int *__restrict__ oi = idx ? idx + rows * nsample : nullptr;
        int *__restrict__ oc = pts_cnt ? pts_cnt + rows : nullptr;
        float *__restrict__ og = grouped ? grouped + rows * nsample * 3 : nullptr;
        if constexpr (sizeof...(Cnt) == 2) {
            bq_fill_rows<kBqThreads>(max(q0, mc), min(q0 + qpb, m), nsample, oi, oc, og);
            if (q0 >= mc) return;
        }
        bq_block_body<LDS_CLOUD, FUSE, false>(nc, m, nsample, thr, 0, q0, min(q0 + qpb, mc), xyz1 + (size_t)c * n * 3, xyz2 + rows * 3,
                                              nullptr, nullptr, oi, oc, og, subtract, smem);
    }
}

template <bool LDS_CLOUD, bool FUSE>
static int launch_bq(int b, int n, int m, float thr, int nsample, const float *xyz1, const int *lengths, const float *xyz2, int *idx,
                     int *pts_cnt, float *grouped, int subtract, hipStream_t st, const int *lengths2 = nullptr, const Packed *pk = nullptr)
{
    // aim at ~2 workgroups per CU over the whole launch; each stages the cloud once
    constexpr int kGran = kBqWaves * kBqQpw;
    long long total = (long long)b * m;
    int qpb = (int)((total + 511) / 512);
    qpb = ((qpb + kGran - 1) / kGran) * kGran;
    if (qpb < kGran) qpb = kGran;
    if (qpb > m) qpb = ((m + kGran - 1) / kGran) * kGran;
    const int gx = (m + qpb - 1) / qpb;
    const size_t lds = (LDS_CLOUD ? sizeof(float4) * (size_t)((n + 127) & ~127) : 0) + sizeof(int) * (size_t)nsample * kGran;
    if (lds > 160 * 1024) return PN2_E_TOO_LARGE;
    if (pk)
        return launch_counts_packed<true>([](auto... c) { return ball_query_kernel<LDS_CLOUD, FUSE, decltype(c)...>; }, *pk, lengths2,
                                           dim3(gx, b), dim3(kBqThreads), lds, st, n, m, nsample, thr, qpb, xyz1, xyz2, idx, pts_cnt, grouped,
                                           subtract);
    return launch_counts([](auto... c) { return ball_query_kernel<LDS_CLOUD, FUSE, decltype(c)...>; }, lengths, lengths2, dim3(gx, b),
                         dim3(kBqThreads), lds, st, n, m, nsample, thr, qpb, xyz1, xyz2, idx, pts_cnt, grouped, subtract);
}

// Cell-list kernel (ball_query_body.h, second half): the grid is built per workgroup, so a workgroup
// takes a larger share of the queries than in the sweep kernel to amortise the binning pass.
// With counts (as in ball_query_kernel; a workgroup of fill rows alone leaves before the binning): a cloud below 64 points takes
// the sweep body at once (block-uniform; the host keeps such clouds off the cell list in the dense dispatch too, bq_use_cells);
// larger ones bin their own n_c points, and the body's own fallback (coarse grid, crowded cells) uses the sweep layout inside
// the same LDS, sized for the padded n.
template <int NT, int LPQ, bool FUSE, class... Cnt>
__global__ __launch_bounds__(NT, NT / 256) void ball_query_cells_kernel(int b, int n, int m, int nsample, float thr,
                                                                      float radius, int qpb, int parts,
                                                                      const float *__restrict__ xyz1,
                                                                      const float *__restrict__ xyz2,
                                                                      int *__restrict__ idx,
                                                                      int *__restrict__ pts_cnt,
                                                                      float *__restrict__ grouped, int subtract, CountArg<Cnt>... cnt)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Counts<Cnt...> counts(cnt...);
    int cloud, part;
    decode_cloud_block(blockIdx.x, parts, b, cloud, part);
    if constexpr (sizeof...(Cnt) == 0) {
        const int q0 = part * qpb;
        bq_cells_block_body<NT, LPQ, FUSE, false, true>(n, m, nsample, thr, radius, cloud, q0, min(q0 + qpb, m), xyz1, xyz2,   // BLK: crowded balls walk the first half of the indices first (ball_query_body.h)
                                         nullptr, nullptr, idx, pts_cnt, grouped, subtract, smem);
    } else if constexpr (Counts<Cnt...>::packed) {          // as in ball_query_kernel; a cloud below 64 points as in the count modes
        const int start = cloud_start(counts.pk, cloud);
        const int nc = cloud_count(counts.pk, cloud, start, n);
        const int ibase = counts.pk.global_idx ? start : 0;
        int mc = m;
        if constexpr (sizeof...(Cnt) == 2) mc = cloud_count(counts.side[1], cloud, m);
        const int q0 = part * qpb, q1 = min(q0 + qpb, mc);
        const size_t rows = (size_t)cloud * m;
        const float *__restrict__ x1 = xyz1 + (size_t)start * 3;
        const float *__restrict__ x2 = xyz2 + rows * 3;
        int *__restrict__ oi = idx ? idx + rows * nsample : nullptr;
        int *__restrict__ oc = pts_cnt ? pts_cnt + rows : nullptr;
        float *__restrict__ og = grouped ? grouped + rows * nsample * 3 : nullptr;
        if constexpr (sizeof...(Cnt) == 2) {
            bq_fill_rows<NT>(max(q0, mc), min(q0 + qpb, m), nsample, oi, oc, og, ibase);
            if (q0 >= mc) return;
        }
        if (nc < 64)
            bq_block_body<true, FUSE, false, NT>(nc, m, nsample, thr, 0, q0, q1, x1, x2, nullptr, nullptr, oi, oc, og, subtract, smem, 1u, 0,
                                                 nullptr, ibase);
        else
            bq_cells_block_body<NT, LPQ, FUSE, false, true>(nc, m, nsample, thr, radius, 0, q0, q1, x1, x2, nullptr, nullptr, oi, oc, og,
                                                            subtract, smem, 1u, nullptr, 0, ibase);
    } else {
        const int nc = cloud_count(counts.side[0], cloud, n);
        int mc = m;
        if constexpr (sizeof...(Cnt) == 2) mc = cloud_count(counts.side[1], cloud, m);
        const int q0 = part * qpb, q1 = min(q0 + qpb, mc);
        const size_t rows = (size_t)cloud * m;
        const float *__restrict__ x1 = xyz1 + (size_t)cloud * n * 3;
        const float *__restrict__ x2 = xyz2 + rows * 3;
        int *__restrict__ oi = idx ? idx + rows * nsample : nullptr;
        int *__restrict__ oc = pts_cnt ? pts_cnt + rows : nullptr;
        float *__restrict__ og = grouped ? grouped + rows * nsample * 3 : nullptr;
        if constexpr (sizeof...(Cnt) == 2) {
            bq_fill_rows<NT>(max(q0, mc), min(q0 + qpb, m), nsample, oi, oc, og);
            if (q0 >= mc) return;
        }
        if (nc < 64)
            bq_block_body<true, FUSE, false, NT>(nc, m, nsample, thr, 0, q0, q1, x1, x2, nullptr, nullptr, oi, oc, og, subtract, smem);
        else
            bq_cells_block_body<NT, LPQ, FUSE, false, true>(nc, m, nsample, thr, radius, 0, q0, q1, x1, x2, nullptr, nullptr, oi, oc, og,
                                                            subtract, smem);
    }
}

static size_t bq_sweep_lds_bytes(int n, int nsample, int nthreads = kBqThreads)
{
    return sizeof(float4) * (size_t)((n + 127) & ~127) + sizeof(int) * (size_t)nsample * (nthreads / 64) * kBqQpw;
}

// Per-call dispatch options (pn2_query_ball_group_xyz_ex; the reference-shaped entry points pass {0, 0}):
// kernel 0 = automatic, 1 = sweep kernel only, 2 = cell-list kernel whenever it fits, 3 = same with
// 512-thread workgroups only; qpb = queries per workgroup of the cell-list kernel, 0 = automatic.
struct BqOpts { int kernel, qpb; };

// Geometry of the cell-list kernel: workgroup size and lanes per query. The query loop is branchy,
// LDS-latency-bound code that wants 16 waves on a CU: two 512-thread workgroups when two fit in the
// LDS (small clouds), one 1024-thread workgroup otherwise; and a wave should carry as many queries
// as the LDS holds bitmaps for. Returns false when nothing fits (the sweep kernel is used).
struct BqCellsGeom { int nthreads, lpq; };
static bool bq_cells_pick(int n, int nsample, int kernel, BqCellsGeom &g)
{
    static const BqCellsGeom order[] = {{512, 8}, {512, 16}, {1024, 8}, {1024, 16}, {512, 8}, {512, 16}, {512, 32}};
    for (int i = 0; i < 7; ++i) {
        const BqCellsGeom &c = order[i];
        if (kernel == 3 && c.nthreads != 512) continue;
        const size_t cap = (i < 2 && kernel != 3) ? 80 * 1024 : 160 * 1024;   // first two: only if two workgroups fit
        if (bq_cells_lds_bytes(n, nsample, c.lpq, c.nthreads) <= cap &&
            bq_sweep_lds_bytes(n, nsample, c.nthreads) <= cap) { g = c; return true; }
    }
    return false;
}

// The cell-list kernel pays a binning pass per workgroup and only prunes when the grid is fine; measured
// on MI355X (scripts/bq_probe.py) it wins from about 2048 points per cloud and a launch that fills the GPU.
static bool bq_use_cells(int b, int n, int m, int kernel)
{
    if (n > kBqCellsMaxPoints || n < 64 || kernel == 1) return false;
    if (kernel >= 2) return true;
    return n >= 2048 && (long long)b * m >= 8192;
}

template <int NT, int LPQ, bool FUSE>
static int launch_bq_cells(int b, int n, int m, float thr, float radius, int nsample, const float *xyz1, const int *lengths,
                           const float *xyz2, int *idx, int *pts_cnt, float *grouped, int subtract, int opt_qpb,
                           hipStream_t st, const int *lengths2 = nullptr, const Packed *pk = nullptr)
{
    constexpr int kGran = (NT / 64) * (64 / LPQ);               // queries per workgroup trip
    long long total = (long long)b * m;
    int qpb = opt_qpb > 0 ? opt_qpb : (int)((total + 255) / 256);
    qpb = ((qpb + kGran - 1) / kGran) * kGran;
    if (qpb < kGran) qpb = kGran;
    if (qpb > m) qpb = ((m + kGran - 1) / kGran) * kGran;
    const int gx = (m + qpb - 1) / qpb;
    const size_t a = bq_cells_lds_bytes(n, nsample, LPQ, NT), s = bq_sweep_lds_bytes(n, nsample, NT);
    const size_t lds = a > s ? a : s;                       // the fallback inside the kernel uses the sweep layout
    if (pk)
        return launch_counts_packed<true>([](auto... c) { return ball_query_cells_kernel<NT, LPQ, FUSE, decltype(c)...>; }, *pk, lengths2,
                                           dim3((unsigned)gx * b), dim3(NT), lds, st, b, n, m, nsample, thr, radius, qpb, gx, xyz1, xyz2, idx,
                                           pts_cnt, grouped, subtract);
    return launch_counts([](auto... c) { return ball_query_cells_kernel<NT, LPQ, FUSE, decltype(c)...>; }, lengths, lengths2,
                         dim3((unsigned)gx * b), dim3(NT), lds, st, b, n, m, nsample, thr, radius, qpb, gx, xyz1, xyz2, idx, pts_cnt,
                         grouped, subtract);
}

template <bool FUSE>
static int dispatch_bq_cells(BqCellsGeom g, int b, int n, int m, float thr, float radius, int nsample,
                             const float *xyz1, const int *lengths, const float *xyz2, int *idx, int *pts_cnt, float *grouped,
                             int subtract, int qpb, hipStream_t st, const int *lengths2 = nullptr, const Packed *pk = nullptr)
{
#define PN2_BQ_CASE(NT, LPQ) \
    if (g.nthreads == NT && g.lpq == LPQ) \
        return launch_bq_cells<NT, LPQ, FUSE>(b, n, m, thr, radius, nsample, xyz1, lengths, xyz2, idx, pts_cnt, grouped, subtract, qpb, st, lengths2, pk)
    PN2_BQ_CASE(1024, 8);
    PN2_BQ_CASE(1024, 16);
    PN2_BQ_CASE(512, 8);
    PN2_BQ_CASE(512, 16);
    PN2_BQ_CASE(512, 32);
#undef PN2_BQ_CASE
    return PN2_E_TOO_LARGE;
}

// lengths: NULL = every cloud holds n points; else the points per cloud. lengths2 (with lengths only): the valid queries per
// cloud (the count modes of the two kernels). pk: the packed mode -- n is nmax, xyz1 holds pk->total rows.
static int ball_query_common(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                             int subtract, int *idx, int *pts_cnt, float *grouped, bool fuse, BqOpts opt, void *stream,
                             const int *lengths = nullptr, const int *lengths2 = nullptr, const Packed *pk = nullptr)
{
    if (opt.kernel < 0 || opt.kernel > 3 || opt.qpb < 0) return PN2_E_ARG;
    if (!(radius > 0.0f) || nsample <= 0) return PN2_E_ARG;   // tf_grouping.cpp:71,74
    if (b < 0 || n <= 0 || m < 0) return PN2_E_SHAPE;
    if (b == 0 || m == 0) return PN2_OK;
    if (!xyz1 || !xyz2) return PN2_E_NULL;
    if (fuse ? !grouped : !idx) return PN2_E_NULL;
    if ((pk ? (long long)pk->total : (long long)b * n) * 3 > INT_MAX || (long long)b * m * nsample * 3 > (1ll << 40)) return PN2_E_TOO_LARGE;
    if (b > 65535) return PN2_E_TOO_LARGE;
    const float thr = pn2_ball_threshold(radius);
    hipStream_t st = as_stream(stream);
    const bool lds = n <= kBqMaxLdsPoints &&
                     sizeof(float4) * (size_t)((n + 127) & ~127) + sizeof(int) * (size_t)nsample * kBqWaves * kBqQpw <= 160 * 1024;
    BqCellsGeom geom;
    if (bq_use_cells(b, n, m, opt.kernel) && bq_cells_pick(n, nsample, opt.kernel, geom))
        return fuse ? dispatch_bq_cells<true>(geom, b, n, m, thr, radius, nsample, xyz1, lengths, xyz2, idx, pts_cnt, grouped, subtract, opt.qpb, st, lengths2, pk)
                    : dispatch_bq_cells<false>(geom, b, n, m, thr, radius, nsample, xyz1, lengths, xyz2, idx, pts_cnt, nullptr, 0, opt.qpb, st, lengths2, pk);
    if (fuse)
        return lds ? launch_bq<true, true>(b, n, m, thr, nsample, xyz1, lengths, xyz2, idx, pts_cnt, grouped, subtract, st, lengths2, pk)
                   : launch_bq<false, true>(b, n, m, thr, nsample, xyz1, lengths, xyz2, idx, pts_cnt, grouped, subtract, st, lengths2, pk);
    return lds ? launch_bq<true, false>(b, n, m, thr, nsample, xyz1, lengths, xyz2, idx, pts_cnt, nullptr, 0, st, lengths2, pk)
               : launch_bq<false, false>(b, n, m, thr, nsample, xyz1, lengths, xyz2, idx, pts_cnt, nullptr, 0, st, lengths2, pk);
}

}  // namespace pn2

// Smallest fp32 s* for which max(sqrtf(s*),1e-20f) < radius is FALSE.
// The predicate is monotone non-increasing in s >= 0 (sqrtf is correctly rounded,
// hence monotone), so  in-ball <=> s < s*.  Bisection over the fp32 bit patterns.
extern "C" float pn2_ball_threshold(float radius)
{
    if (!(radius > 0.0f) || !(1e-20f < radius)) return 0.0f;   // nothing is ever inside
    uint32_t lo = 0u;           // s=+0: predicate true
    uint32_t hi = 0x7f800000u;  // s=+inf: predicate false
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        float s;
        memcpy(&s, &mid, sizeof s);
        const float r = sqrtf(s);
        const float d = (r < 1e-20f) ? 1e-20f : r;
        if (d < radius) lo = mid; else hi = mid;
    }
    float out;
    memcpy(&out, &hi, sizeof out);
    return out;
}

extern "C" int pn2_query_ball_point(int b, int n, int m, float radius, int nsample, const float *xyz1,
                                    const float *xyz2, int *idx, int *pts_cnt, void *stream)
{
    return pn2::ball_query_common(b, n, m, radius, nsample, xyz1, xyz2, 0, idx, pts_cnt, nullptr, false, {0, 0}, stream);
}

extern "C" int pn2_query_ball_group_xyz(int b, int n, int m, float radius, int nsample, const float *xyz1,
                                        const float *xyz2, int subtract_centroid, int *idx, int *pts_cnt,
                                        float *grouped_xyz, void *stream)
{
    return pn2::ball_query_common(b, n, m, radius, nsample, xyz1, xyz2, subtract_centroid, idx, pts_cnt,
                                  grouped_xyz, true, {0, 0}, stream);
}

// The same operator with the kernel choice as per-call arguments (tests force every kernel at every shape,
// scripts/bq_probe.py tunes the dispatch): kernel 0 automatic, 1 sweep, 2 cell list, 3 cell list with
// 512-thread workgroups; cells_qpb = queries per workgroup of the cell-list kernel (0 automatic).
// grouped_xyz == NULL: plain query_ball_point. Stateless like everything else in the library.
extern "C" int pn2_query_ball_group_xyz_ex(int b, int n, int m, float radius, int nsample, const float *xyz1,
                                           const float *xyz2, int subtract_centroid, int *idx, int *pts_cnt,
                                           float *grouped_xyz, int kernel, int cells_qpb, void *stream)
{
    return pn2::ball_query_common(b, n, m, radius, nsample, xyz1, xyz2, grouped_xyz ? subtract_centroid : 0, idx, pts_cnt,
                                  grouped_xyz, grouped_xyz != nullptr, {kernel, cells_qpb}, stream);
}

// The ragged entries' prologue: the dense entry's attribute and extent checks, then nothing to do, and only then the `sides`
// count arrays the entry requires (lengths2 with sides == 2).
static int ball_query_ragged(int sides, int b, int n, int m, float radius, int nsample, const float *xyz1, const int *lengths1,
                             const float *xyz2, const int *lengths2, int subtract_centroid, int *idx, int *pts_cnt, float *grouped_xyz,
                             int kernel, int cells_qpb, void *stream)
{
    if (kernel < 0 || kernel > 3 || cells_qpb < 0) return PN2_E_ARG;
    if (!(radius > 0.0f) || nsample <= 0) return PN2_E_ARG;
    if (b < 0 || n <= 0 || m < 0) return PN2_E_SHAPE;
    if (b == 0 || m == 0) return PN2_OK;
    if (!lengths1 || (sides == 2 && !lengths2)) return PN2_E_NULL;
    return pn2::ball_query_common(b, n, m, radius, nsample, xyz1, xyz2, grouped_xyz ? subtract_centroid : 0, idx, pts_cnt,
                                  grouped_xyz, grouped_xyz != nullptr, {kernel, cells_qpb}, stream, lengths1, lengths2);
}

// Ragged batch: cloud c of xyz1 is xyz1[c, :lengths1[c]] of a padded (b, n, 3) tensor, lengths1 (b) int32 on the device, never
// read by the host; the queries xyz2 (b, m, 3) are dense. Result per cloud = pn2_query_ball_group_xyz_ex on the slice, for
// every `kernel`. grouped_xyz == NULL: plain query_ball_point.
extern "C" int pn2_query_ball_group_xyz_ragged(int b, int n, int m, float radius, int nsample, const float *xyz1, const int *lengths1,
                                               const float *xyz2, int subtract_centroid, int *idx, int *pts_cnt, float *grouped_xyz,
                                               int kernel, int cells_qpb, void *stream)
{
    return ball_query_ragged(1, b, n, m, radius, nsample, xyz1, lengths1, xyz2, nullptr, subtract_centroid, idx, pts_cnt, grouped_xyz,
                             kernel, cells_qpb, stream);
}

// Ragged on both sides: cloud c additionally holds only lengths2[c] valid rows of xyz2 (b int32 on the device, clamped into
// 1..m, never read by the host). Rows below lengths2[c] = pn2_query_ball_group_xyz_ex on (xyz1[c, :lengths1[c]],
// xyz2[c, :lengths2[c]]) for every `kernel`; the rows from lengths2[c] on are written as idx 0, pts_cnt 0, grouped_xyz +0.0 and
// their queries are never read. Codes in the order of pn2_query_ball_group_xyz_ragged; both count arrays are required.
extern "C" int pn2_query_ball_group_xyz_ragged_pair(int b, int n, int m, float radius, int nsample, const float *xyz1,
                                                    const int *lengths1, const float *xyz2, const int *lengths2, int subtract_centroid,
                                                    int *idx, int *pts_cnt, float *grouped_xyz, int kernel, int cells_qpb, void *stream)
{
    return ball_query_ragged(2, b, n, m, radius, nsample, xyz1, lengths1, xyz2, lengths2, subtract_centroid, idx, pts_cnt, grouped_xyz,
                             kernel, cells_qpb, stream);
}

// Packed batch: cloud c of xyz1 is xyz1[offsets1[c] : offsets1[c + 1]] of a flat (total, 3) array, offsets1 (b + 1) int32 on the
// device, never read by the host; nmax bounds every cloud's count and takes the padded n's place in the kernel choice, the grid
// and the LDS size. The queries xyz2 (b, m, 3) and the outputs are dense. Result per cloud = pn2_query_ball_group_xyz_ex on the
// slice for every `kernel`; global_idx 1 writes idx as offsets1[c] + k. grouped_xyz == NULL: plain query_ball_point. Codes in
// the order of pn2_query_ball_group_xyz_ragged (PN2_E_TOO_LARGE for total 3 > INT_MAX).
// The packed entries' prologue and launch; sides == 2 requires lengths2.
static int ball_query_packed(int sides, int b, int total, int nmax, int m, float radius, int nsample, const float *xyz1,
                             const int *offsets1, const float *xyz2, const int *lengths2, int subtract_centroid, int global_idx, int *idx,
                             int *pts_cnt, float *grouped_xyz, int kernel, int cells_qpb, void *stream)
{
    if (kernel < 0 || kernel > 3 || cells_qpb < 0) return PN2_E_ARG;
    if (!(radius > 0.0f) || nsample <= 0) return PN2_E_ARG;
    if (b < 0 || nmax <= 0 || m < 0) return PN2_E_SHAPE;
    if (b == 0 || m == 0) return PN2_OK;
    if (total <= 0) return PN2_E_SHAPE;
    if (!offsets1 || (sides == 2 && !lengths2)) return PN2_E_NULL;
    const pn2::Packed pk = {offsets1, total, global_idx ? 1 : 0};
    return pn2::ball_query_common(b, nmax, m, radius, nsample, xyz1, xyz2, grouped_xyz ? subtract_centroid : 0, idx, pts_cnt, grouped_xyz,
                                  grouped_xyz != nullptr, {kernel, cells_qpb}, stream, nullptr, lengths2, &pk);
}

extern "C" int pn2_query_ball_group_xyz_packed(int b, int total, int nmax, int m, float radius, int nsample, const float *xyz1,
                                               const int *offsets1, const float *xyz2, int subtract_centroid, int global_idx, int *idx,
                                               int *pts_cnt, float *grouped_xyz, int kernel, int cells_qpb, void *stream)
{
    return ball_query_packed(1, b, total, nmax, m, radius, nsample, xyz1, offsets1, xyz2, nullptr, subtract_centroid, global_idx, idx,
                             pts_cnt, grouped_xyz, kernel, cells_qpb, stream);
}

// Packed on the first side, ragged on the second: cloud c additionally holds only lengths2[c] valid rows of xyz2 ((b) int32 on
// the device, clamped into 1..m, never read by the host). Rows below lengths2[c] = pn2_query_ball_group_xyz_ex on the slice
// pair = pn2_query_ball_group_xyz_ragged_pair on the padded copy; the rows from lengths2[c] on are written as pts_cnt 0,
// grouped_xyz +0.0 and idx 0 -- offsets1[c] under global_idx, the cloud's own first row -- and their queries are never read.
// Codes in the order of pn2_query_ball_group_xyz_packed; lengths2 is required (PN2_E_NULL where offsets1 is).
extern "C" int pn2_query_ball_group_xyz_packed_pair(int b, int total, int nmax, int m, float radius, int nsample, const float *xyz1,
                                                    const int *offsets1, const float *xyz2, const int *lengths2, int subtract_centroid,
                                                    int global_idx, int *idx, int *pts_cnt, float *grouped_xyz, int kernel,
                                                    int cells_qpb, void *stream)
{
    return ball_query_packed(2, b, total, nmax, m, radius, nsample, xyz1, offsets1, xyz2, lengths2, subtract_centroid, global_idx, idx,
                             pts_cnt, grouped_xyz, kernel, cells_qpb, stream);
}
