// train_mlp_top.hip -- the pooled top layer of the training node WITHOUT its pre-norm tensor: the matrices that rewrite its
// passes in terms of the layer's input, the routed part of its weight gradient on the vector units, and their launches. gfx950.
#include "train_mlp_device.h"

namespace pn2 {

// ---- pooled top layer WITHOUT its pre-norm tensor ------------------------------------------------------------------------
// z_L (rows, C_L) is the largest tensor of an SA level and is only ever needed in dz_L = s dy_L - c0 - c1 z_L. With
// z_L = h W + b (h = the layer's input) both products that consume dz_L split into a part through the ROUTED gradient
// (one entry per group and channel) and a part through h:
//     dz_L W^T   = (s dy_L) W^T - h M - 1 r^T           M = W diag(c1) W^T  (K x K),   r = W (c0 + b c1)
//     h^T dz_L   = h^T (s dy_L) - (h^T h) W diag(c1) - (h^T 1) (c0 + b c1)^T
// so backward reads h (K channels) where it would read z_L (C_L = 2K channels in the reference stacks), forward never
// writes z_L, and the extra matrix work is K / C_L of the layer's -- the passes are memory-bound, it is free.
// tl_top_mats_kernel: the stacked fp32 weight of the data-gradient GEMM, rows [0, NFp) = W^T (c -> k), rows [NFp, NFp + K)
// = -M, and its constant row -r. One thread per element, fp64 accumulation.
__global__ __launch_bounds__(256) void tl_top_mats_kernel(const float *__restrict__ w, long long sk, long long sn, int K, int NF,
                                                          int NFp, const float *__restrict__ coef, const float *__restrict__ bias,
                                                          float *__restrict__ wp, float *__restrict__ rowc)
{
    // (W staged in LDS -- 64 x 128 at the metric shape -- was measured in the last session of round 6: 13.2 -> 24.5 us; the walk
    // over a row's columns hits the same cache lines trip after trip, the staging loop does not. Not kept.)
    auto W = [&](int n, int c) __attribute__((always_inline)) -> float { return w[n * sk + c * sn]; };
    const long long total = (long long)(NFp + K + 1) * K;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / K), n = (int)(i - (long long)r * K);
        if (r < NFp) {
            wp[i] = r < NF ? W(n, r) : 0.0f;
        } else if (r < NFp + K) {
            const int j = r - NFp;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};                  // four chains: the loop is load latency, not arithmetic
            int c = 0;
            for (; c + 4 <= NF; c += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    acc[u] += (double)W(j, c + u) * (double)coef[2 * NF + c + u] * (double)W(n, c + u);
            }
            for (; c < NF; ++c) acc[0] += (double)W(j, c) * (double)coef[2 * NF + c] * (double)W(n, c);
            wp[i] = (float)(-((acc[0] + acc[1]) + (acc[2] + acc[3])));
        } else {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            int c = 0;
            for (; c + 4 <= NF; c += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    acc[u] += ((double)coef[NF + c + u] + (bias ? (double)bias[c + u] : 0.0) * (double)coef[2 * NF + c + u]) *
                              (double)W(n, c + u);
            }
            for (; c < NF; ++c)
                acc[0] += ((double)coef[NF + c] + (bias ? (double)bias[c] : 0.0) * (double)coef[2 * NF + c]) * (double)W(n, c);
            rowc[n] = (float)(-((acc[0] + acc[1]) + (acc[2] + acc[3])));
        }
    }
}

// dW[k][n] = S[k][n] - c1[n] sum_j G[k][j] W[j][n] - sumh[k] (c0[n] + b[n] c1[n]); sf = [S | G | sumh ..] (K, ld) fp64
__global__ __launch_bounds__(256) void tl_top_wgrad_fix_kernel(const double *__restrict__ sf, int ld, int K, int NF, int goff, int hoff,
                                                               const float *__restrict__ w, long long sk, long long sn,
                                                               const float *__restrict__ coef, const float *__restrict__ bias,
                                                               float *__restrict__ gw, const double *__restrict__ S, int accumulate)
{
    const long long total = (long long)K * NF;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int k = (int)(i / NF), n = (int)(i - (long long)k * NF);
        const double *row = sf + (size_t)k * ld;
        double a4[4] = {0.0, 0.0, 0.0, 0.0};
        int j = 0;
        for (; j + 4 <= K; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) a4[u] += row[goff + j + u] * (double)w[(j + u) * sk + n * sn];
        }
        for (; j < K; ++j) a4[0] += row[goff + j] * (double)w[j * sk + n * sn];
        const double acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
        const double c0 = coef[NF + n], c1 = coef[2 * NF + n], b = bias ? (double)bias[n] : 0.0;
        const float gv = (float)((S ? S[i] : row[n]) - c1 * acc - row[hoff] * (c0 + b * c1));
        gw[k * sk + n * sn] = accumulate ? __fadd_rn(gw[k * sk + n * sn], gv) : gv;      // S: (K, NF) of tl_top_s_kernel
    }
}

// ---- the ROUTED part of that weight gradient on the vector units ----------------------------------------------------------
// S = h^T (s dy_L), and dy_L has one non-zero per group and channel (the pooled sample):
//     S[k][c] = sum over the groups g of   h[row(g, argsel[g][c])][k] * s_c gq[g][c]
// -- C_L K multiply-adds per GROUP instead of per row. As tiles of the dense kernel (tl_wgrad_kernel, K_FILL units) the
// routed gradient was 2/3 of its operand tiles and matrix-core work (312 us at the metric shape, instruction-bound).
// A workgroup of eight waves stages the h rows of GB groups in LDS (relu(a z + c) applied on the way in; the next
// batch's rows are in flight in registers meanwhile); a wave owns 64 channels x KC inputs of S in registers, a lane = a
// channel: it reads the KC values of ITS pooled sample's row (ds_read_b128) and scales them. One (K, C_L) partial per
// workgroup, summed in fp64 afterwards (tl_wgrad_reduce_a_kernel + tl_top_s_reduce_kernel).
template <int KC, int NLD>
__global__ __launch_bounds__(kTopSThreads, (KC <= 16 && NLD <= 4) ? 4 : 2) void tl_top_s_kernel(const TlTopS p)
{
    extern __shared__ __attribute__((aligned(16))) float tops_lds[];
    float *coefs = tops_lds, *tile = tops_lds + 2 * p.K;            // [pa | pc], then GB x ns rows of ld floats
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kchunks = p.K / KC, nitems = ((p.NF + 63) / 64) * kchunks, item = blockIdx.y * 8 + wave;
    const bool work = item < nitems;
    const int cc = work ? item / kchunks : 0, kc = work ? item - cc * kchunks : 0, c = cc * 64 + lane;
    const bool cok = work && c < p.NF;
    const float sc = cok ? p.coef[c] : 0.0f;
    for (int i = threadIdx.x; i < p.K; i += kTopSThreads) { coefs[i] = p.pa[i]; coefs[p.K + i] = p.pc[i]; }
    float acc[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) acc[k] = 0.0f;
    const int k4row = p.K / 4;
    const long long nb = (p.groups + p.GB - 1) / p.GB;
    float4 raw[NLD];
    int an[kTopSGroups];
    float vn[kTopSGroups];
    auto fetch = [&](long long batch) {                          // rows of a batch are one contiguous range of z
        const long long g0 = batch * p.GB;
        const int ng = batch < nb ? (int)(p.groups - g0 < p.GB ? p.groups - g0 : p.GB) : 0;
        const int total4 = ng * p.ns * k4row;
        const float *src = p.z + (size_t)g0 * p.ns * p.K;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = threadIdx.x + i * kTopSThreads;
            raw[i] = e < total4 ? ld4(src + (size_t)e * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int gi = 0; gi < kTopSGroups; ++gi) {
            const bool ok = cok && gi < ng;
            const size_t o = (size_t)(g0 + gi) * p.NF + c;
            an[gi] = ok ? p.argsel[o] : 0;
            vn[gi] = ok ? __fmul_rn(sc, p.gq[o]) : 0.0f;
        }
    };
    fetch(blockIdx.x);
    __syncthreads();                                               // coefs
    for (long long batch = blockIdx.x; batch < nb; batch += gridDim.x) {
        const int total4 = p.GB * p.ns * k4row;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = threadIdx.x + i * kTopSThreads;
            if (e < total4) {
                const int row = e / k4row, k = (e - row * k4row) * 4;
                const float4 a = *reinterpret_cast<const float4 *>(coefs + k), b = *reinterpret_cast<const float4 *>(coefs + p.K + k);
                float4 h;
                h.x = vmax(__fadd_rn(__fmul_rn(a.x, raw[i].x), b.x), 0.0f);
                h.y = vmax(__fadd_rn(__fmul_rn(a.y, raw[i].y), b.y), 0.0f);
                h.z = vmax(__fadd_rn(__fmul_rn(a.z, raw[i].z), b.z), 0.0f);
                h.w = vmax(__fadd_rn(__fmul_rn(a.w, raw[i].w), b.w), 0.0f);
                *reinterpret_cast<float4 *>(tile + (size_t)row * p.ld + k) = h;
            }
        }
        int ac[kTopSGroups];
        float vc[kTopSGroups];
#pragma unroll
        for (int gi = 0; gi < kTopSGroups; ++gi) { ac[gi] = an[gi]; vc[gi] = vn[gi]; }
        __syncthreads();
        fetch(batch + gridDim.x);                                  // in flight under the multiply-adds
        if (work) {
#pragma unroll
            for (int gi = 0; gi < kTopSGroups; ++gi) {
                if (gi < p.GB) {
                    const float *hr = tile + (size_t)(gi * p.ns + ac[gi]) * p.ld + kc * KC;
#pragma unroll
                    for (int k4 = 0; k4 < KC / 4; ++k4) {
                        const float4 h = *reinterpret_cast<const float4 *>(hr + 4 * k4);
                        acc[4 * k4] = fmaf(vc[gi], h.x, acc[4 * k4]);
                        acc[4 * k4 + 1] = fmaf(vc[gi], h.y, acc[4 * k4 + 1]);
                        acc[4 * k4 + 2] = fmaf(vc[gi], h.z, acc[4 * k4 + 2]);
                        acc[4 * k4 + 3] = fmaf(vc[gi], h.w, acc[4 * k4 + 3]);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (cok) {
        float *dst = p.partial + ((size_t)blockIdx.x * p.K + (size_t)kc * KC) * p.NF + c;
#pragma unroll
        for (int k = 0; k < KC; ++k) dst[(size_t)k * p.NF] = acc[k];
    }
}

// S (K, NF) fp64 = sum of `nparts` fp32 partials
__global__ __launch_bounds__(256) void tl_top_s_reduce_kernel(const float *__restrict__ in, int nparts, long long total,
                                                              double *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        int q = 0;
        for (; q + 4 <= nparts; q += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] += (double)in[(size_t)(q + u) * total + i];
        }
        for (; q < nparts; ++q) a[0] += (double)in[(size_t)q * total + i];
        out[i] = (a[0] + a[1]) + (a[2] + a[3]);
    }
}

template <int KC>
static int launch_top_s_kc(const TlTopS &p, const TopSShape &t, hipStream_t st)
{
    const dim3 grid((unsigned)t.gridx, (unsigned)t.gridy);
#define PN2_TS_CASE(N)                                                              \
    if (t.NLD == N) {                                                               \
        auto kern = tl_top_s_kernel<KC, N>;                                         \
        if (int rc = allow_dynamic_lds(kern, t.lds)) return rc;                     \
        return launch(kern, grid, dim3(kTopSThreads), t.lds, st, p);                \
    }
    PN2_TS_CASE(1) PN2_TS_CASE(2) PN2_TS_CASE(4) PN2_TS_CASE(8)
#undef PN2_TS_CASE
    return PN2_E_ARG;
}

// S (K, NF) fp64 = h^T (s dy_L) through the pooled samples (tl_top_s_kernel + the two reduction stages)
int launch_top_s(TlTopS &p, const TopSShape &t, float *part2, double *s64, hipStream_t st)
{
    p.GB = t.GB; p.ld = t.ld;
    int rc = t.KC == 64 ? launch_top_s_kc<64>(p, t, st) : t.KC == 32 ? launch_top_s_kc<32>(p, t, st)
           : t.KC == 16 ? launch_top_s_kc<16>(p, t, st) : t.KC == 8 ? launch_top_s_kc<8>(p, t, st) : launch_top_s_kc<4>(p, t, st);
    if (rc) return rc;
    const long long total = (long long)p.K * p.NF;
    const float *src = p.partial;
    int nparts = t.gridx;
    if (t.nchunks) {
        const long long e4 = total / 4;
        rc = launch_wgrad_reduce_a(reinterpret_cast<const float4 *>(p.partial), reinterpret_cast<float4 *>(part2), (long long)t.gridx, 32,
                                   (long long)t.nchunks, e4, st);
        if (rc) return rc;
        src = part2;
        nparts = t.nchunks;
    }
    long long blocks = (total + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    return launch(tl_top_s_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, nparts, total, s64);
}

int launch_top_mats(const float *w, long long sk, long long sn, int K, int NF, int NFp, const float *coef, const float *bias, float *wp,
                    float *rowc, hipStream_t st)
{
    long long blocks = ((long long)(NFp + K + 1) * K + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    return launch(tl_top_mats_kernel, dim3((unsigned)blocks), dim3(256), 0, st, w, sk, sn, K, NF, NFp, coef, bias, wp, rowc);
}

int launch_top_wgrad_fix(const double *sf, int ld, int K, int NF, int goff, int hoff, const float *w, long long sk, long long sn,
                         const float *coef, const float *bias, float *gw, const double *S, int accumulate, hipStream_t st)
{
    long long blocks = ((long long)K * NF + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    return launch(tl_top_wgrad_fix_kernel, dim3((unsigned)blocks), dim3(256), 0, st, sf, ld, K, NF, goff, hoff, w, sk, sn, coef, bias, gw,
                  S, accumulate);
}

}  // namespace pn2
