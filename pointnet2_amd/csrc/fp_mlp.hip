// fp_mlp.hip -- a whole feature-propagation layer behind three_nn in ONE kernel, on the matrix cores.
//
// Reference: pointnet_fp_module, utils/pointnet_util.py:199-229 --
//     dist, idx = three_nn(xyz1, xyz2)                                   (:211, stays pn2_three_nn)
//     dist = max(dist, 1e-10); norm = sum(1/dist); weight = (1/dist)/norm (:212-215)
//     interpolated = three_interpolate(points2, idx, weight)             (:216)
//     new_points1 = concat([interpolated, points1], axis=2)              (:219, interpolated FIRST)
//     for each width: conv2d 1x1 + batch_norm + ReLU                     (:223-226)
// i.e. five to ten launches with every intermediate -- weights, the (b,n,c2) interpolated tensor, the
// concatenation, every layer's activations -- in HBM. Here a wave owns 32 unknown points: each lane
// computes its point's three inverse-distance weights from `dist`, gathers the three known rows a
// 32-channel tile at a time straight into the layer-1 MFMA operand registers (weighted sum in the
// reference's order (p1*w1 + p2*w2) + p3*w3, skip-link channels appended), and runs the layer stack with
// the machinery of the streamed-weights SA kernel (sa_mlp_stream.hip: activations chained in accumulator
// registers between layers in their three-level bf16 operand form, weight tile pairs streamed through a
// double-buffered LDS stage shared by the four waves,
// the LAST layer with swapped MFMA operands so that a lane holds 16 points of one output channel). The
// epilogue is a plain store of bias + ReLU instead of a max-pool: 128 contiguous bytes per half wave.
// Batch norm is folded into the weights by the caller (inference), like pn2_sa_mlp3_maxpool.
//
// The first layer is linear in its input and the interpolation is linear in the known features:
//     W1^T [interp(points2), points1] = interp(points2 . W1a) + W1b^T points1.
// point_layer_kernel (sa_mlp_stream.hip) therefore evaluates Q = points2 . W1a ONCE PER KNOWN POINT (m rows, a
// quarter or less of the n unknown ones at every level of the reference models) into caller scratch; the kernels
// here interpolate rows of Q (the first width's channels instead of c2) into the layer-1 accumulators and only the
// skip-link part of layer 1 is left as MFMA work per unknown point (none at all when there is no skip link: sem_seg's
// last level). A reassociation of the sum inside fp32 rounding; the weights w1 + w2 + w3 = 1 multiply Q, not the bias.
//
// Stacks: two or three layers, widths up to 256 with (tiles of layer 1) + (tiles of layer 2) <= 16 --
// every FP stack of the reference models: [256,256], [256,128], [128,128,128]
// (pointnet2_part_seg.py:31-33, pointnet2_sem_seg.py:34-37) -- and any number of input channels.
#include "sa_mlp_common.h"

namespace pn2 {

__device__ __forceinline__ float fp_interp3(float p1, float p2, float p3, float w1, float w2, float w3)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(p1, w1), __fmul_rn(p2, w2)), __fmul_rn(p3, w3));   // tf_interpolate.cpp:122
}

// T3 == 0: two layers (layer 2 is the last one). TL = tiles of the last layer.
// RAGGED (lengths1 (b) in device memory, include/pn2ops.h "ragged inference"): lockstep like the streamed SA kernel, so by
// redirect and select -- a lane whose point is at or beyond its cloud's length gathers through row 0 of its own cloud (idx,
// dist and points1 of the padding row are not read) and the row is stored as +0.0. The dense instantiations have none of it.
template <int T1, int T2, int T3, bool RAGGED = false>
__global__ __launch_bounds__(kMlpThreads) void fp_mlp_stream_kernel(int n, int m, int c1, int cout, long long rows,
                                                                    int ti, const float *__restrict__ pre,
                                                                    const float *__restrict__ points1,
                                                                    const int *__restrict__ idx,
                                                                    const float *__restrict__ dist,
                                                                    const float *__restrict__ wstream,
                                                                    const float *__restrict__ bpacked,
                                                                    float *__restrict__ out,
                                                                    const int *__restrict__ lengths1)
{
    constexpr int TB = T1 + T2 + T3;
    __shared__ __attribute__((aligned(16))) u32x4 wbuf[2][kStageVec];
    __shared__ float bias_s[TB * 32];
    const float *b1 = bias_s, *b2 = b1 + T1 * 32, *b3 = b2 + T2 * 32;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, s = lane & 31;
    for (int i = tid; i < TB * 32; i += kMlpThreads) bias_s[i] = bpacked[i];

    const int l1_pairs = pad_to_stage(ti * T1);
    const int stages_per_item = (l1_pairs + T2 * T1 + T3 * T2) / kS;
    int stage = 0;
    u32x4 stg0, stg1, stg2, stg3, stg4, stg5;
    static_assert(kStageVec == 6 * kMlpThreads, "the staging registers are spelled out for six vectors per thread");
    static_assert((T2 * T1) % kS == 0 && (T3 * T2) % kS == 0, "layers must start on stage boundaries");
#define PN2_STREAM_ISSUE(st)                                                                                           \
    do {                                                                                                               \
        const u32x4 *src_ = reinterpret_cast<const u32x4 *>(wstream) + (size_t)((st) % stages_per_item) * kStageVec + tid; \
        stg0 = src_[0]; stg1 = src_[256]; stg2 = src_[512]; stg3 = src_[768]; stg4 = src_[1024]; stg5 = src_[1280];   \
    } while (0)
#define PN2_STREAM_COMMIT(st)                                                                                          \
    do {                                                                                                               \
        u32x4 *dst_ = wbuf[(st) & 1] + tid;                                                                            \
        dst_[0] = stg0; dst_[256] = stg1; dst_[512] = stg2; dst_[768] = stg3; dst_[1024] = stg4; dst_[1280] = stg5;   \
    } while (0)
#define PN2_NEXT_STAGE()                                                                                               \
    do {                                                                                                               \
        PN2_STREAM_COMMIT(stage + 1);                                                                                  \
        __syncthreads();                                                                                               \
        ++stage;                                                                                                       \
        PN2_STREAM_ISSUE(stage + 1);                                                                                   \
    } while (0)
    PN2_STREAM_ISSUE(0);
    PN2_STREAM_COMMIT(0);
    __syncthreads();
    PN2_STREAM_ISSUE(1);

    const long long groups = (rows + 31) / 32;                              // work item = 32 consecutive unknown points
    const long long wave = (long long)blockIdx.x * (kMlpThreads / 64) + (tid >> 6);
    const long long nwaves = (long long)gridDim.x * (kMlpThreads / 64);
    const long long trips = (groups + nwaves - 1) / nwaves;                 // lockstep: every wave runs all trips
    const bool vec1 = (c1 & 3) == 0;

    for (long long trip = 0; trip < trips; ++trip) {
        const long long g = wave + trip * nwaves;
        const long long row0 = (g < groups ? g : groups - 1) * 32;
        const bool item_ok = g < groups;
        const long long row_own = min(row0 + s, rows - 1);                   // this lane's point (clamped: loads stay valid)
        const long long cloud = row_own / n;
        bool ok = true;
        if (RAGGED) ok = (int)(row_own - cloud * n) < min(max(lengths1[cloud], 1), n);
        const long long row = ok ? row_own : cloud * n;
        const unsigned long long valid_rows = RAGGED ? __ballot(ok) : ~0ull;  // bit i: point row0 + i is a valid row
        // inverse-distance weights, pointnet_util.py:212-215
        const int *ip = idx + row * 3;
        const float *dp = dist + row * 3;
        const int i1 = ip[0], i2 = ip[1], i3 = ip[2];
        const float r1 = __fdiv_rn(1.0f, fmaxf(dp[0], 1e-10f)), r2 = __fdiv_rn(1.0f, fmaxf(dp[1], 1e-10f)),
                    r3 = __fdiv_rn(1.0f, fmaxf(dp[2], 1e-10f));
        const float norm = __fadd_rn(__fadd_rn(r1, r2), r3);
        const float w1 = __fdiv_rn(r1, norm), w2 = __fdiv_rn(r2, norm), w3 = __fdiv_rn(r3, norm);
        // rows of Q = points2 . W1a of the three neighbours (32 * T1 floats each), this lane's channels 4h .. 4h + 3 of a quartet
        const float *qbase = pre + (size_t)cloud * m * (32 * T1) + 4 * h;
        const float *qa = qbase + (size_t)i1 * (32 * T1), *qb = qbase + (size_t)i2 * (32 * T1), *qc = qbase + (size_t)i3 * (32 * T1);
        const float *p1 = points1 ? points1 + (size_t)row * c1 : nullptr;

        // one 32-channel tile of the skip features: register v <- channel 32u + mlp_chan(v, h) of points1
        auto gather = [&](int u) __attribute__((always_inline)) -> f32x16 {
            f32x16 x;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k0 = 32 * u + 8 * q + 4 * h;
                if (vec1 && k0 + 3 < c1) {
                    const float4 f = *reinterpret_cast<const float4 *>(p1 + k0);
                    x[4 * q] = f.x; x[4 * q + 1] = f.y; x[4 * q + 2] = f.z; x[4 * q + 3] = f.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[4 * q + r] = k0 + r < c1 ? p1[k0 + r] : 0.0f;
                }
            }
            return x;
        };

        // layer 1: bias + the interpolated rows of Q (tf_interpolate.cpp:122's order per channel) + the skip part on
        // the matrix pipe, input tiles outermost (one gathered tile alive, all T1 accumulators alive)
        f32x16 h1[T1];
#pragma unroll
        for (int t = 0; t < T1; ++t) {
            h1[t] = mlp_bias(b1, t, h);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 a = *reinterpret_cast<const float4 *>(qa + 32 * t + 8 * q), bq = *reinterpret_cast<const float4 *>(qb + 32 * t + 8 * q),
                             c = *reinterpret_cast<const float4 *>(qc + 32 * t + 8 * q);
                h1[t][4 * q] = __fadd_rn(h1[t][4 * q], fp_interp3(a.x, bq.x, c.x, w1, w2, w3));
                h1[t][4 * q + 1] = __fadd_rn(h1[t][4 * q + 1], fp_interp3(a.y, bq.y, c.y, w1, w2, w3));
                h1[t][4 * q + 2] = __fadd_rn(h1[t][4 * q + 2], fp_interp3(a.z, bq.z, c.z, w1, w2, w3));
                h1[t][4 * q + 3] = __fadd_rn(h1[t][4 * q + 3], fp_interp3(a.w, bq.w, c.w, w1, w2, w3));
            }
        }
        if (ti > 0) {
            f32x16 x = gather(0);
            int slot = 0;
            for (int u = 0; u < ti; ++u) {
                f32x16 xn = x;
                if (u + 1 < ti) xn = gather(u + 1);
                const ActSplit xs = split_act(x);
#pragma unroll
                for (int t = 0; t < T1; ++t) {
                    h1[t] = stream_pair<false>(wbuf[stage & 1], slot, lane, xs, h1[t]);
                    if (++slot == kS) { slot = 0; PN2_NEXT_STAGE(); }
                }
                x = xn;
            }
            if (slot != 0) PN2_NEXT_STAGE();
        }
        ActSplit s1[T1];
#pragma unroll
        for (int t = 0; t < T1; ++t) s1[t] = split_act(mlp_relu(h1[t]));

        // the last layer: operands swapped -> register v of lane (c, hh) holds point mlp_chan(v, hh) of the
        // item, channel 32t + c; bias + ReLU and a plain store (128 contiguous bytes per half wave)
        auto store_tile = [&](int t, const f32x16 &acc, const float *blast) __attribute__((always_inline)) {
            const int ch = 32 * t + s;
            const float bias = b3_at(blast, ch);
            if (item_ok && ch < cout) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const long long r = row0 + mlp_chan(v, h);
                    const float val = fmaxf(__fadd_rn(acc[v], bias), 0.0f);
                    if (r < rows) out[r * cout + ch] = (!RAGGED || ((valid_rows >> mlp_chan(v, h)) & 1ull)) ? val : 0.0f;
                }
            }
        };
        if (T3 == 0) {
#pragma unroll
            for (int t = 0; t < T2; ++t) {
                f32x16 acc;
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
#pragma unroll
                for (int u = 0; u < T1; ++u) {
                    acc = stream_pair<true>(wbuf[stage & 1], (t * T1 + u) % kS, lane, s1[u], acc);
                    if ((t * T1 + u) % kS == kS - 1) PN2_NEXT_STAGE();
                }
                store_tile(t, acc, b2);
            }
        } else {
            ActSplit s2[T2];
#pragma unroll
            for (int t = 0; t < T2; ++t) {
                f32x16 acc = mlp_bias(b2, t, h);
#pragma unroll
                for (int u = 0; u < T1; ++u) {
                    acc = stream_pair<false>(wbuf[stage & 1], (t * T1 + u) % kS, lane, s1[u], acc);
                    if ((t * T1 + u) % kS == kS - 1) PN2_NEXT_STAGE();
                }
                s2[t] = split_act(mlp_relu(acc));
            }
#pragma unroll
            for (int t = 0; t < (T3 ? T3 : 1); ++t) {
                f32x16 acc;
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
#pragma unroll
                for (int u = 0; u < T2; ++u) {
                    acc = stream_pair<true>(wbuf[stage & 1], (t * T2 + u) % kS, lane, s2[u], acc);
                    if ((t * T2 + u) % kS == kS - 1) PN2_NEXT_STAGE();
                }
                store_tile(t, acc, b3);
            }
        }
    }
#undef PN2_STREAM_ISSUE
#undef PN2_STREAM_COMMIT
#undef PN2_NEXT_STAGE
}

// the instantiated tile shapes, smallest first within two and within three layers: X(t1, t2, t3), t3 == 0: two layers
#define PN2_FP_SHAPES(X) X(4, 4, 0) X(8, 4, 0) X(8, 8, 0) X(4, 4, 4) X(8, 4, 4) X(8, 8, 4) X(8, 8, 8)

// widths are padded up to a shape's with zero weights
bool fp_stream_pick(int c2, int c1, int nlayers, const int *widths, FpConfig &cfg)
{
    if (c2 < 1 || c1 < 0 || (nlayers != 2 && nlayers != 3)) return false;
    for (int i = 0; i < nlayers; ++i)
        if (widths[i] < 1 || widths[i] > 256) return false;
#define PN2_FP_FITS(A, B, C)                                                                                           \
    if ((C != 0) == (nlayers == 3) && widths[0] <= 32 * A && widths[1] <= 32 * B && (nlayers == 2 || widths[2] <= 32 * C)) { \
        cfg = {(c1 + 31) / 32, (c2 + 31) / 32, A, B, C};                                                               \
        return true;                                                                                                   \
    }
    PN2_FP_SHAPES(PN2_FP_FITS)
#undef PN2_FP_FITS
    return false;
}

// this kernel's stream: skip rows of layer 1 (padded to a stage), layer 2, layer 3; biases [layer 1][layer 2][layer 3]
static long long fp_main_pairs(const FpConfig &c) { return (long long)pad_to_stage(c.ti * c.t1) + c.t2 * c.t1 + c.t3 * c.t2; }
size_t fp_stream_w_floats(const FpConfig &c) { return (size_t)fp_main_pairs(c) * kPairWords; }
size_t fp_stream_b_floats(const FpConfig &c) { return (size_t)(c.t1 + c.t2 + c.t3) * 32; }

// skip_row: row of ws[0] of skip channel k (the rows behind the interpolated channels)
void fp_stream_pack(const FpConfig &c, int c1, int nlayers, const int *widths, const int *skip_row, const float *const *ws,
                    const float *const *bs, float *wpacked, float *bpacked)
{
    float *wp = wpacked, *bp = bpacked;
    for (int u = 0; u < c.ti; ++u)
        for (int t = 0; t < c.t1; ++t) wp = mlp_pack_pair_x6(wp, ws[0], c1, widths[0], t, u, skip_row);
    wp = mlp_pack_stage_padding(wp, c.ti * c.t1);
    for (int t = 0; t < c.t2; ++t)
        for (int u = 0; u < c.t1; ++u) wp = mlp_pack_pair_x6(wp, ws[1], widths[0], widths[1], t, u, nullptr);
    for (int t = 0; t < c.t3; ++t)
        for (int u = 0; u < c.t2; ++u) wp = mlp_pack_pair_x6(wp, ws[2], widths[1], widths[2], t, u, nullptr);
    const int tout[3] = {c.t1, c.t2, c.t3};
    for (int L = 0; L < nlayers; ++L) bp = mlp_pack_bias(bp, bs[L], widths[L], tout[L]);
}

int fp_stream_launch(const FpConfig &c, long long rows, int n, int m, int c1, int cout, const float *pre, const float *points1,
                     const int *idx, const float *dist, const float *wp, const float *bp, float *out, hipStream_t st,
                     const int *lengths1)
{
    decltype(&fp_mlp_stream_kernel<4, 4, 0>) kern = nullptr;
#define PN2_FP_KERNEL(A, B, C) \
    if (c.t1 == A && c.t2 == B && c.t3 == C) kern = lengths1 ? fp_mlp_stream_kernel<A, B, C, true> : fp_mlp_stream_kernel<A, B, C>;
    PN2_FP_SHAPES(PN2_FP_KERNEL)
#undef PN2_FP_KERNEL
    if (!kern) return PN2_E_TOO_LARGE;
    const long long blocks = ((rows + 31) / 32 + 3) / 4;          // four 32-point items per workgroup
    // persistent, at most one workgroup per CU: every workgroup streams the weights
    return launch(kern, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(kMlpThreads), 0, st, n, m, c1, cout, rows, c.ti, pre,
                  points1, idx, dist, wp, bp, out, lengths1);
}

}  // namespace pn2
