// ball_query_msg.hip -- multi-radius ball query + grouping of xyz: ONE staging / binning of the cloud
// serves every radius of a multi-scale-grouping level.
//
// Reference: pointnet_sa_module_msg, utils/pointnet_util.py:175-186 -- for every radius of the level the
// loop calls query_ball_point(radius, nsample, xyz, new_xyz) and group_point(xyz, idx) and subtracts the
// centroid, i.e. it rescans the cloud once per radius (three launches of query_ball_point_gpu,
// tf_grouping_g.cu:3-36, over the same xyz / new_xyz). pointnet2_cls_msg.py:27 runs radii
// (0.1, 0.2, 0.4) x nsample (16, 32, 128) over 4096-point clouds.
//
// Here a workgroup owns (cloud, query range) for ALL radii. It bins the cloud once into the cell list
// of ball_query_body.h -- cells sized for the SMALLEST radius -- and then runs the query loop once per
// radius against the same LDS-resident, cell-sorted array: a larger radius simply visits a larger block
// of cells (the "wide" runs of bq_cells_query_loop). When the cell list does not apply (small clouds,
// coarse grid, crowded cells) the cloud is staged once in index order and swept per radius. Both paths
// use the device bodies of the single-radius kernels, so every output is bit-identical to separate
// pn2_query_ball_point / pn2_query_ball_group_xyz calls (tests/test_configs_gpu.py).
#include "ball_query_body.h"

#include <limits.h>
#include <math.h>

namespace pn2 {

constexpr int kBqMaxScales = 4;

struct BqScale {
    float thr, radius;
    int nsample, lpq;                     // lanes per query of this radius' pass (as many queries per wave as the LDS holds)
    int *idx, *cnt;
    float *grouped;
};
struct BqScales {
    int count;
    float bin_radius;                     // the cell list is built for this radius (see pn2_query_ball_group_xyz_msg)
    BqScale s[kBqMaxScales];
};

// One workgroup's share of a cloud -- queries [q0, q1) of cloud `cloud`, every radius -- shared by the dense and the ragged
// kernel below. n: the points of the cloud (the LDS layout and every loop bound follow it); xyz1 / xyz2: bases such that the
// cloud's slab is xyz1 + cloud n 3 and its queries xyz2 + cloud m 3; out_rows: rows of m-major output in front of row
// cloud m + j (0 when the scales' pointers are the tensors' bases and `cloud` does the addressing). Block-uniform throughout.
// ibase: added to every index where it is stored, for every radius, by the list passes and the sweep alike (the packed mode's
// global_idx; an empty ball stores ibase + 0); grouped rows are gathered with the local index. Every other caller passes a
// literal 0, which folds away.
template <int NT>
__device__ __forceinline__ void bq_msg_block_body(int n, int m, int cloud, int q0, int q1, int use_cells, int max_ns,
                                                  int wave_stride_b, const BqScales &sc, const float *__restrict__ xyz1,
                                                  const float *__restrict__ xyz2, int subtract, size_t out_rows, char *smem,
                                                  int ibase)
{
    const float *__restrict__ data = xyz1 + (size_t)cloud * n * 3;

    // cell-list layout (ball_query_body.h), wave areas sized for the largest nsample of the level
    float4 *sorted = reinterpret_cast<float4 *>(smem);
    int *tab = reinterpret_cast<int *>(smem + sizeof(float4) * (size_t)n);
    char *wave_area = reinterpret_cast<char *>(tab + kBqTabInts);
    const size_t wave_stride = (size_t)wave_stride_b;             // largest per-wave area over the radii
    float *misc = reinterpret_cast<float *>(wave_area + (size_t)(NT / 64) * wave_stride);

    bool cells = false;
    BqGrid g;
    if (use_cells) {                                             // block-uniform
        if (threadIdx.x == 0) tab[0] = 0;
        cells = bq_build_grid<NT>(n, sc.bin_radius * 1.001f, data, sorted, tab + 1, misc, g);
    }
    // Radii still to be served by the index-ordered sweep: all of them without a cell list; with one, the radii whose block of
    // visited cells covers half of the grid or more (round 6). There the list prunes nothing -- on a uniform cube binned at 0.2
    // a ball of radius 0.4 reaches 5 of the 5 cells of every axis, 4096 candidates per query -- while the sweep stops at the
    // nsample-th hit (crowded balls: ~500 candidates for 128 hits); on the sphere-surface clouds of pointnet2_cls_msg.py:27 the
    // same radius reaches 5 of 10 cells per axis and stays on the list. uniform-cube level (0.1, 0.2, 0.4): 108 us -> see
    // profiles/r06/bq_msg_wide.txt. The cloud is restaged in index order once, behind the list passes.
    unsigned todo = (1u << sc.count) - 1u;
    if (cells) {
        for (int i = 0; i < sc.count; ++i) {
            const BqScale &s = sc.s[i];
            int *const s_idx = s.idx ? s.idx + out_rows * (size_t)s.nsample : nullptr;
            int *const s_cnt = s.cnt ? s.cnt + out_rows : nullptr;
            float *const s_grouped = s.grouped ? s.grouped + out_rows * (size_t)s.nsample * 3 : nullptr;
            const float reach = s.radius * 1.001f;
            const float fx = fminf(1.0f, (2.0f * reach * g.ix + 1.0f) / (float)g.gx);
            const float fy = fminf(1.0f, (2.0f * reach * g.iy + 1.0f) / (float)g.gy);
            const float fz = fminf(1.0f, (2.0f * reach * g.iz + 1.0f) / (float)g.gz);
            if (__builtin_amdgcn_readfirstlane((int)(fx * fy * fz >= 0.5f))) continue;   // block-uniform: the grid is the workgroup's
#define PN2_MSG_LOOP(LPQ)                                                                                           \
    bq_cells_query_loop<NT, LPQ, true, false>(n, m, s.nsample, s.thr, s.radius, s.radius * 1.001f, cloud, q0, q1, g, data, \
                                              xyz2, nullptr, nullptr, s_idx, s_cnt, s_grouped, subtract, sorted, tab, \
                                              wave_area, wave_stride, 1u, nullptr, nullptr, ibase)
            if (s.lpq == 8) PN2_MSG_LOOP(8);                      // block-uniform
            else if (s.lpq == 16) PN2_MSG_LOOP(16);
            else PN2_MSG_LOOP(32);
#undef PN2_MSG_LOOP
            todo &= ~(1u << i);
        }
        if (!todo) return;
    }
    // index-ordered LDS copy, padded to a multiple of 128 with points at +inf (never hit), swept per radius
    __syncthreads();                                             // the binning / list passes may still be reading
    float4 *cloud_lds = reinterpret_cast<float4 *>(smem);
    const int npad = (n + 127) & ~127;
    for (int k = threadIdx.x; k < npad; k += NT) {
        if (k < n) {
            const float *p = data + (size_t)k * 3;
            cloud_lds[k] = make_float4(p[0], p[1], p[2], 0.0f);
        } else {
            cloud_lds[k] = make_float4(INFINITY, INFINITY, INFINITY, 0.0f);
        }
    }
    __syncthreads();
    for (int i = 0; i < sc.count; ++i) {
        if (!((todo >> i) & 1u)) continue;
        const BqScale &s = sc.s[i];
        bq_block_body<true, true, false, NT, true>(n, m, s.nsample, s.thr, cloud, q0, q1, xyz1, xyz2, nullptr, nullptr,
                                                   s.idx ? s.idx + out_rows * (size_t)s.nsample : nullptr,
                                                   s.cnt ? s.cnt + out_rows : nullptr,
                                                   s.grouped ? s.grouped + out_rows * (size_t)s.nsample * 3 : nullptr, subtract,
                                                   smem, 1u, max_ns, nullptr, ibase);
    }
}

// One kernel, three modes (pn2_device.h: Counts). No count array: the dense kernel. With counts
// (pn2_query_ball_group_xyz_msg_ragged / _ragged_pair): cloud c holds nc = lengths1[c] <= n points in its padded (n, 3) slab. The
// workgroup hands the body n = nc, cloud 0 and the cloud's own slabs of the padded tensors, the outputs moved by the cloud's
// c m rows: layout, staging, binning, the +inf pad and every loop bound are those of the dense kernel on the slice, and rows
// at or beyond nc are never addressed. Everything the HOST decided -- geometry, lanes per query, wave_stride, LDS bytes -- was
// sized for the padded n (msg_plan), and what fits n fits nc: the sorted array (16 nc bytes), the sweep copy's npad = nc
// rounded up to 128 and bq_cells_wave_bytes(nc, ., lpq) (windows of 4096 points) are all non-decreasing in the point count,
// and wave_stride is passed in, never re-derived from nc. Per cloud, block-uniform: below 64 points the binning is skipped and
// the cloud is swept (the rule of ball_query_cells_kernel); larger clouds bin their own nc points, so bq_build_grid's
// give-up rules and the half-of-the-grid rule of the body apply to that cloud's grid. No global atomics, no memset, nothing
// that waits on another workgroup.
// Counts on both sides: cloud c also holds only m_c = lengths2[c] valid queries. The body gets the query range cut at m_c; the
// workgroup's rows from m_c on are filled for EVERY radius (idx 0, pts_cnt 0, grouped +0.0), and a workgroup of such rows alone
// leaves before any staging or binning (block-uniform).
// Packed (pn2_query_ball_group_xyz_msg_packed; pn2_device.h: Packed): the one-sided count mode with the cloud's slab taken from
// the offsets -- xyz1 is the flat (total, 3) array, n is nmax, the queries and the outputs stay dense (b, m, ...). The body gets
// exactly the one-sided call: n = nc, cloud 0, xyz1 + start 3, the cloud's m query rows, out_rows = cloud m, and the same
// per-cloud rule use_cells && nc >= 64. The host decided from nmax (msg_plan(b, nmax, m, ...)) as the ragged entry decides from
// the padded n, and the argument above carries over word for word: what fits nmax fits nc. A slab may start at ANY row of the
// flat array -- no alignment is asked of offsets -- because the body reads coordinates as scalars (staging, binning and the
// FUSE gather all go through data[k * 3 + {0, 1, 2}]). With global_idx the stored indices are rows of the flat array.
// Packed with one count array (pn2_query_ball_group_xyz_msg_packed_pair): m_c = lengths2[c] as in the two-array mode; the fill
// rows of every radius store the cloud's own first row (offsets[c] under global_idx, else 0) as their index.
template <int NT, class... Cnt>
__global__ __launch_bounds__(NT, NT / 256) void ball_query_msg_kernel(int b, int n, int m, int qpb, int parts,
                                                                    int use_cells, int max_ns, int wave_stride_b, BqScales sc,
                                                                    const float *__restrict__ xyz1,
                                                                    const float *__restrict__ xyz2, int subtract, CountArg<Cnt>... cnt)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Counts<Cnt...> counts(cnt...);
    int cloud, part;
    decode_cloud_block(blockIdx.x, parts, b, cloud, part);
    if constexpr (sizeof...(Cnt) == 0) {
        const int q0 = part * qpb;
        bq_msg_block_body<NT>(n, m, cloud, q0, min(q0 + qpb, m), use_cells, max_ns, wave_stride_b, sc, xyz1, xyz2, subtract, 0, smem, 0);
    } else if constexpr (Counts<Cnt...>::packed) {
        const int start = cloud_start(counts.pk, cloud);
        const int nc = cloud_count(counts.pk, cloud, start, n);
        const int q0 = part * qpb;
        const size_t rows = (size_t)cloud * m;
        int mc = m;
        if constexpr (sizeof...(Cnt) == 2) {                         // the second side's counts, as in the two-array mode below
            mc = cloud_count(counts.side[1], cloud, m);
            const int f0 = max(q0, mc), f1 = min(q0 + qpb, m);
            if (f0 < f1) {                                           // block-uniform
                for (int i = 0; i < sc.count; ++i) {
                    const BqScale &s = sc.s[i];
                    bq_fill_rows<NT>(f0, f1, s.nsample, s.idx ? s.idx + rows * (size_t)s.nsample : nullptr, s.cnt ? s.cnt + rows : nullptr,
                                     s.grouped ? s.grouped + rows * (size_t)s.nsample * 3 : nullptr, counts.pk.global_idx ? start : 0);
                }
            }
            if (q0 >= mc) return;
        }
        bq_msg_block_body<NT>(nc, m, 0, q0, min(q0 + qpb, mc), (use_cells && nc >= 64) ? 1 : 0, max_ns, wave_stride_b, sc,
                              xyz1 + (size_t)start * 3, xyz2 + rows * 3, subtract, rows, smem, counts.pk.global_idx ? start : 0);
    } else {
        const int nc = cloud_count(counts.side[0], cloud, n);
        int mc = m;
        if constexpr (sizeof...(Cnt) == 2) mc = cloud_count(counts.side[1], cloud, m);
        const int q0 = part * qpb;
        const size_t rows = (size_t)cloud * m;
        if constexpr (sizeof...(Cnt) == 2) {
            const int f0 = max(q0, mc), f1 = min(q0 + qpb, m);
            if (f0 < f1) {                                           // block-uniform
                for (int i = 0; i < sc.count; ++i) {
                    const BqScale &s = sc.s[i];
                    bq_fill_rows<NT>(f0, f1, s.nsample, s.idx ? s.idx + rows * (size_t)s.nsample : nullptr, s.cnt ? s.cnt + rows : nullptr,
                                     s.grouped ? s.grouped + rows * (size_t)s.nsample * 3 : nullptr);
                }
            }
            if (q0 >= mc) return;
        }
        bq_msg_block_body<NT>(nc, m, 0, q0, min(q0 + qpb, mc), (use_cells && nc >= 64) ? 1 : 0, max_ns, wave_stride_b, sc,
                              xyz1 + (size_t)cloud * n * 3, xyz2 + rows * 3, subtract, rows, smem, 0);
    }
}

static size_t msg_sweep_bytes(int n, int max_ns, int nthreads)
{
    return sizeof(float4) * (size_t)((n + 127) & ~127) + sizeof(int) * (size_t)max_ns * (nthreads / 64) * kBqQpw;
}

// Queries per workgroup: about one workgroup per CU when the cloud is binned (the binning pass is per
// workgroup), two for the sweep; a multiple of the smallest trip (two queries per wave).
static int msg_qpb(int b, int m, int nthreads, int use_cells)
{
    const int gran = (nthreads / 64) * kBqQpw;
    const long long total = (long long)b * m;
    int qpb = (int)((total + (use_cells ? 255 : 511)) / (use_cells ? 256 : 512));
    qpb = ((qpb + gran - 1) / gran) * gran;
    if (qpb > m) qpb = ((m + gran - 1) / gran) * gran;
    return qpb;
}

// Lanes per query for every radius: the smallest of {8, 16, 32} (most queries per wave) that (1) fits the LDS
// left beside the sorted cloud and the cell table, (2) does not carry more queries per workgroup trip than the
// workgroup owns (waves * 64 / lpq <= qpb: otherwise waves idle), and (3) is at least 16 for a radius beyond
// the binning radius (long "wide" runs). Returns the per-wave stride, 0 if nothing fits.
static size_t msg_pick_lpq(int n, int nthreads, size_t cap, int qpb, BqScales &sc)
{
    const size_t fixed = sizeof(float4) * (size_t)n + sizeof(int) * (size_t)kBqTabInts + kBqMiscBytes;
    if (fixed >= cap) return 0;
    const size_t budget = (cap - fixed) / (size_t)(nthreads / 64);
    size_t stride = 0;
    for (int i = 0; i < sc.count; ++i) {
        int lpq_min = sc.s[i].radius > sc.bin_radius * 1.01f ? 16 : 8;
        while (lpq_min < 32 && (nthreads / 64) * (64 / lpq_min) > qpb) lpq_min *= 2;
        int lpq = 0;
        for (int cand : {8, 16, 32})
            if (cand >= lpq_min && bq_cells_wave_bytes(n, sc.s[i].nsample, cand) <= budget) { lpq = cand; break; }
        if (!lpq) return 0;
        sc.s[i].lpq = lpq;
        const size_t bytes = bq_cells_wave_bytes(n, sc.s[i].nsample, lpq);
        stride = bytes > stride ? bytes : stride;
    }
    return stride;
}

// Everything the host decides about one call, taken ONCE: the launcher and pn2_query_ball_group_xyz_msg_plan both read it from
// msg_plan below, so what the plan entry reports is what is launched.
struct MsgPlan {
    int nt;                               // threads per workgroup; 0: nothing to launch (b == 0 or m == 0)
    size_t cap, lds, wave_stride;         // LDS cap of the geometry, dynamic LDS requested, bytes between two waves' areas
    int use_cells, qpb, parts, max_ns;
    BqScales sc;                          // thr, radius, nsample, lpq per scale and bin_radius; the output pointers are the launcher's
};

// The checks of the arguments that need no pointer but radii / nsamples (the launcher looks at its output pointers next).
static int msg_check_args(int b, int n, int m, int nscales, const float *radii, const int *nsamples)
{
    if (nscales <= 0 || nscales > kBqMaxScales || !radii || !nsamples) return PN2_E_ARG;
    if (b < 0 || n <= 0 || m < 0) return PN2_E_SHAPE;
    for (int i = 0; i < nscales; ++i)
        if (!(radii[i] > 0.0f) || nsamples[i] <= 0) return PN2_E_ARG;   // tf_grouping.cpp:71,74
    return PN2_OK;
}

static int msg_plan(int b, int n, int m, int nscales, const float *radii, const int *nsamples, MsgPlan &p)
{
    if (int rc = msg_check_args(b, n, m, nscales, radii, nsamples)) return rc;
    p.nt = 0;
    p.cap = p.lds = p.wave_stride = 0;
    p.use_cells = p.qpb = p.parts = p.max_ns = 0;
    BqScales &sc = p.sc;
    sc.count = nscales;
    for (int i = 0; i < nscales; ++i) {
        sc.s[i] = {pn2_ball_threshold(radii[i]), radii[i], nsamples[i], 8, nullptr, nullptr, nullptr};
        p.max_ns = nsamples[i] > p.max_ns ? nsamples[i] : p.max_ns;
    }
    // Cell size: the SECOND smallest radius when there are three or more (else the smallest). Cells sized for
    // the smallest radius make every larger radius walk "wide" runs (whole y-ranges of a z-slab, every x): at
    // pointnet2_cls_msg.py:27's (0.1, 0.2, 0.4) binning at 0.2 keeps the 0.1 and 0.2 passes on <= 3 x 3 short
    // runs and only the 0.4 pass wide (measured: 91 us binned at 0.1 with 8 lanes per query, 56 at 0.1 with 16).
    {
        float r1 = radii[0], r2 = INFINITY;                      // smallest, second smallest
        for (int i = 1; i < nscales; ++i) {
            if (radii[i] < r1) { r2 = r1; r1 = radii[i]; }
            else if (radii[i] < r2) r2 = radii[i];
        }
        sc.bin_radius = (nscales >= 3) ? r2 : r1;
    }
    for (int i = 0; i < nscales; ++i)
        if ((long long)b * m * nsamples[i] * 3 > (1ll << 40)) return PN2_E_TOO_LARGE;
    if (b == 0 || m == 0) return PN2_OK;
    if ((long long)b * n * 3 > INT_MAX) return PN2_E_TOO_LARGE;
    if (n > kBqCellsMaxPoints) return PN2_E_TOO_LARGE;          // callers launch the single-radius operator per scale
    // the binning pass is amortised over every radius of the level: worth it from mid-sized clouds on
    p.use_cells = n >= 1024 && (long long)b * m * nscales >= 8192;
    // geometry: two 512-thread workgroups per CU when everything fits in half the LDS, else one of 1024, else one of 512
    struct Geom { int nt; size_t cap; };
    static const Geom order[] = {{512, 80 * 1024}, {1024, 160 * 1024}, {512, 160 * 1024}};
    for (const Geom &g : order) {
        if (msg_sweep_bytes(n, p.max_ns, g.nt) > g.cap) continue;
        const int qpb = msg_qpb(b, m, g.nt, p.use_cells);
        const size_t stride = msg_pick_lpq(n, g.nt, g.cap, qpb, sc);
        if (!stride) continue;
        const size_t cells = sizeof(float4) * (size_t)n + sizeof(int) * (size_t)kBqTabInts + (size_t)(g.nt / 64) * stride + kBqMiscBytes;
        const size_t sweep = msg_sweep_bytes(n, p.max_ns, g.nt);
        p.nt = g.nt;
        p.cap = g.cap;
        p.lds = cells > sweep ? cells : sweep;
        p.wave_stride = stride;
        p.qpb = qpb;
        p.parts = (m + qpb - 1) / qpb;
        return PN2_OK;
    }
    return PN2_E_TOO_LARGE;
}

template <int NT>
static int launch_msg(int b, int n, int m, const MsgPlan &p, const float *xyz1, const int *lengths1, const float *xyz2, int subtract,
                      hipStream_t st, const int *lengths2 = nullptr, const Packed *pk = nullptr)
{
    // with counts the same plan: every host decision is taken from the padded n (packed: from nmax)
    if (pk)
        return launch_counts_packed<true>([](auto... c) { return ball_query_msg_kernel<NT, decltype(c)...>; }, *pk, lengths2,
                                           dim3((unsigned)p.parts * b), dim3(NT), p.lds, st, b, n, m, p.qpb, p.parts, p.use_cells,
                                           p.max_ns, (int)p.wave_stride, p.sc, xyz1, xyz2, subtract);
    return launch_counts([](auto... c) { return ball_query_msg_kernel<NT, decltype(c)...>; }, lengths1, lengths2,
                         dim3((unsigned)p.parts * b), dim3(NT), p.lds, st, b, n, m, p.qpb, p.parts, p.use_cells, p.max_ns,
                         (int)p.wave_stride, p.sc, xyz1, xyz2, subtract);
}

}  // namespace pn2

extern "C" int pn2_query_ball_group_xyz_msg_plan(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                                                 int *info, float *bin_radius)
{
    using namespace pn2;
    MsgPlan p;
    const int rc = msg_plan(b, n, m, nscales, radii, nsamples, p);
    if (rc == PN2_E_ARG || rc == PN2_E_SHAPE) return rc;         // nothing to report about such arguments
    if (bin_radius) *bin_radius = p.sc.bin_radius;
    if (info) {
        const bool chosen = rc == PN2_OK && p.nt > 0;
        const int head[6] = {p.nt, (int)p.cap, (int)p.lds, p.use_cells, p.qpb, p.parts};
        for (int i = 0; i < 6; ++i) info[i] = head[i];
        for (int i = 0; i < kBqMaxScales; ++i) info[6 + i] = (chosen && i < nscales) ? p.sc.s[i].lpq : 0;
    }
    return rc;
}

// lengths1: NULL = every cloud holds n points; else the points per cloud; lengths2 (with lengths1 only): the valid queries per
// cloud (the kernel's count modes). pk: the packed mode -- n is nmax, xyz1 holds pk->total rows.
static int msg_run(int b, int n, int m, int nscales, const float *radii, const int *nsamples, const float *xyz1, const int *lengths1,
                   const float *xyz2, int subtract_centroid, int *const *idx, int *const *pts_cnt, float *const *grouped_xyz,
                   void *stream, const int *lengths2 = nullptr, const pn2::Packed *pk = nullptr)
{
    using namespace pn2;
    if (int rc = msg_check_args(b, n, m, nscales, radii, nsamples)) return rc;
    for (int i = 0; i < nscales; ++i)
        if (!(idx && idx[i]) && !(grouped_xyz && grouped_xyz[i])) return PN2_E_NULL;
    MsgPlan p;
    if (int rc = msg_plan(b, n, m, nscales, radii, nsamples, p)) return rc;
    if (p.nt == 0) return PN2_OK;                                // b == 0 or m == 0
    if (pk && (long long)pk->total * 3 > INT_MAX) return PN2_E_TOO_LARGE;
    if (!xyz1 || !xyz2) return PN2_E_NULL;
    for (int i = 0; i < nscales; ++i) {
        p.sc.s[i].idx = idx ? idx[i] : nullptr;
        p.sc.s[i].cnt = pts_cnt ? pts_cnt[i] : nullptr;
        p.sc.s[i].grouped = grouped_xyz ? grouped_xyz[i] : nullptr;
    }
    hipStream_t st = as_stream(stream);
    if (p.nt == 1024) return launch_msg<1024>(b, n, m, p, xyz1, lengths1, xyz2, subtract_centroid, st, lengths2, pk);
    return launch_msg<512>(b, n, m, p, xyz1, lengths1, xyz2, subtract_centroid, st, lengths2, pk);
}

extern "C" int pn2_query_ball_group_xyz_msg(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                                            const float *xyz1, const float *xyz2, int subtract_centroid, int *const *idx,
                                            int *const *pts_cnt, float *const *grouped_xyz, void *stream)
{
    return msg_run(b, n, m, nscales, radii, nsamples, xyz1, nullptr, xyz2, subtract_centroid, idx, pts_cnt, grouped_xyz, stream);
}

// The ragged entries' prologue, codes in the order of the single-radius ragged entries: attributes and extents, then nothing to
// do, then the `sides` count arrays the entry requires, then the dense entry's remaining checks.
static int msg_run_ragged(int sides, int b, int n, int m, int nscales, const float *radii, const int *nsamples, const float *xyz1,
                          const int *lengths1, const float *xyz2, const int *lengths2, int subtract_centroid, int *const *idx,
                          int *const *pts_cnt, float *const *grouped_xyz, void *stream)
{
    if (int rc = pn2::msg_check_args(b, n, m, nscales, radii, nsamples)) return rc;
    if (b == 0 || m == 0) return PN2_OK;
    if (!lengths1 || (sides == 2 && !lengths2)) return PN2_E_NULL;
    return msg_run(b, n, m, nscales, radii, nsamples, xyz1, lengths1, xyz2, subtract_centroid, idx, pts_cnt, grouped_xyz, stream,
                   lengths2);
}

// Ragged batch: cloud c of xyz1 is xyz1[c, :lengths1[c]] of a padded (b, n, 3) tensor, lengths1 (b) int32 on the device, never
// read by the host; the queries xyz2 (b, m, 3) are dense. Result per cloud and radius = pn2_query_ball_group_xyz_msg on the
// slice = pn2_query_ball_group_xyz_ragged per radius.
extern "C" int pn2_query_ball_group_xyz_msg_ragged(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                                                   const float *xyz1, const int *lengths1, const float *xyz2,
                                                   int subtract_centroid, int *const *idx, int *const *pts_cnt,
                                                   float *const *grouped_xyz, void *stream)
{
    return msg_run_ragged(1, b, n, m, nscales, radii, nsamples, xyz1, lengths1, xyz2, nullptr, subtract_centroid, idx, pts_cnt,
                          grouped_xyz, stream);
}

// Ragged on both sides: cloud c additionally holds only lengths2[c] valid rows of xyz2 (clamped into 1..m on the device). Rows
// below lengths2[c] = pn2_query_ball_group_xyz_msg on the slice pair = pn2_query_ball_group_xyz_ragged_pair per radius; the rows
// from lengths2[c] on are written, for every radius, as idx 0, pts_cnt 0, grouped_xyz +0.0. Codes in the order of
// pn2_query_ball_group_xyz_msg_ragged; both count arrays are required.
extern "C" int pn2_query_ball_group_xyz_msg_ragged_pair(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                                                        const float *xyz1, const int *lengths1, const float *xyz2,
                                                        const int *lengths2, int subtract_centroid, int *const *idx,
                                                        int *const *pts_cnt, float *const *grouped_xyz, void *stream)
{
    return msg_run_ragged(2, b, n, m, nscales, radii, nsamples, xyz1, lengths1, xyz2, lengths2, subtract_centroid, idx, pts_cnt,
                          grouped_xyz, stream);
}

// Packed batch: cloud c of xyz1 is xyz1[offsets1[c] : offsets1[c + 1]] of a flat (total, 3) array, offsets1 (b + 1) int32 on the
// device, never read by the host; nmax bounds every cloud's count and takes the padded n's place in every host decision --
// pn2_query_ball_group_xyz_msg_plan(b, nmax, m, ...) reports what is launched. The queries xyz2 (b, m, 3) and the outputs are
// dense. Result per cloud and radius = pn2_query_ball_group_xyz_msg on the slice = pn2_query_ball_group_xyz_packed per radius =
// pn2_query_ball_group_xyz_msg_ragged on the padded copy; global_idx 1 writes idx as offsets1[c] + k. Codes in the order of
// pn2_query_ball_group_xyz_msg_ragged with offsets1 where lengths1 stood; total <= 0 or nmax > total is PN2_E_SHAPE, total 3 >
// INT_MAX PN2_E_TOO_LARGE.
static int msg_run_packed(int sides, int b, int total, int nmax, int m, int nscales, const float *radii, const int *nsamples,
                          const float *xyz1, const int *offsets1, const float *xyz2, const int *lengths2, int subtract_centroid,
                          int global_idx, int *const *idx, int *const *pts_cnt, float *const *grouped_xyz, void *stream)
{
    if (int rc = pn2::msg_check_args(b, nmax, m, nscales, radii, nsamples)) return rc;
    if (b == 0 || m == 0) return PN2_OK;
    if (total <= 0 || nmax > total) return PN2_E_SHAPE;
    if (!offsets1 || (sides == 2 && !lengths2)) return PN2_E_NULL;
    const pn2::Packed pk = {offsets1, total, global_idx ? 1 : 0};
    return msg_run(b, nmax, m, nscales, radii, nsamples, xyz1, nullptr, xyz2, subtract_centroid, idx, pts_cnt, grouped_xyz, stream,
                   lengths2, &pk);
}

extern "C" int pn2_query_ball_group_xyz_msg_packed(int b, int total, int nmax, int m, int nscales, const float *radii,
                                                   const int *nsamples, const float *xyz1, const int *offsets1, const float *xyz2,
                                                   int subtract_centroid, int global_idx, int *const *idx, int *const *pts_cnt,
                                                   float *const *grouped_xyz, void *stream)
{
    return msg_run_packed(1, b, total, nmax, m, nscales, radii, nsamples, xyz1, offsets1, xyz2, nullptr, subtract_centroid, global_idx,
                          idx, pts_cnt, grouped_xyz, stream);
}

// Packed on the first side, ragged on the second: rows below lengths2[c] = pn2_query_ball_group_xyz_msg on the slice pair =
// pn2_query_ball_group_xyz_packed_pair per radius = pn2_query_ball_group_xyz_msg_ragged_pair on the padded copy; the rows from
// lengths2[c] on are written, for every radius, as pts_cnt 0, grouped_xyz +0.0 and idx 0 (offsets1[c] under global_idx). Codes
// in the order of pn2_query_ball_group_xyz_msg_packed; lengths2 is required.
extern "C" int pn2_query_ball_group_xyz_msg_packed_pair(int b, int total, int nmax, int m, int nscales, const float *radii,
                                                        const int *nsamples, const float *xyz1, const int *offsets1,
                                                        const float *xyz2, const int *lengths2, int subtract_centroid, int global_idx,
                                                        int *const *idx, int *const *pts_cnt, float *const *grouped_xyz, void *stream)
{
    return msg_run_packed(2, b, total, nmax, m, nscales, radii, nsamples, xyz1, offsets1, xyz2, lengths2, subtract_centroid, global_idx,
                          idx, pts_cnt, grouped_xyz, stream);
}
