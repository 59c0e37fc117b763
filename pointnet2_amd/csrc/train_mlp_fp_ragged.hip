// train_mlp_fp_ragged.hip -- the two vector-unit passes of the FP training node (train_mlp_fp.hip) on a RAGGED unknown side:
// masked twins of tl_fp_l1_forward_kernel and tl_fp_l1_dz_kernel, kernels of their own (the dense ones are not touched). gfx950.
//
// Row r of the b n unknown points is valid iff bit r & 31 of validity word r >> 5 is set (the mask buffer of
// pn2_mlp_train_*_ragged, written by tl_ragged_mask_kernel from `lengths`; train_mlp_ragged.hip). The two values DESIGN.md
// section 4.11 names are taken as zero on a padding row, by SELECTS (points1, dist, grad_out may hold NaN there):
//   z_1   where it is formed: nothing of idx, dist, Q or of what the points1 W1b GEMM left in the row is used; the row is
//         written as +0.0, its weights as (0, 0, 0), and it adds nothing to the partial moments;
//   dz_1  where it is formed: s dy_1 - c0 - c1 z_1 would be -c0; the row is written as +0.0.
// Everything behind them (layers 2..L, the weight gradients, the interpolation gradient) then meets zero rows.
// With every row valid the forward kernel runs the dense kernel's operations on the dense kernel's rows in the dense kernel's
// order (same thread <-> (row lane, 4 columns) mapping, chunking, kFpU, partial-moment layout): the same bits.
//
// idx on padding rows. The interpolation gradient behind the dz pass (pn2_three_interpolate_grad_seg / _planned) reads idx and
// weight on EVERY row, so padding rows must hold indices in [0, m): ragged three_nn writes (0, 0, 0) there, and with the zero
// weights written here those rows add 0 * 0 to known point 0 of their cloud -- one long segment per short cloud, which the
// segmented kernels handle, and the same as on the fp_interp_concat route. That cost is not addressed here.
#include "train_mlp_internal.h"

namespace pn2 {

constexpr int kFprThreads = 512, kFprU = 4;           // tl_fp_l1_forward_kernel's (train_mlp_fp.hip: kFpThreads, kFpU)

__device__ __forceinline__ float4 fpr_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

__device__ __forceinline__ float fpr_interp3(float p1, float p2, float p3, float w1, float w2, float w3)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(p1, w1), __fmul_rn(p2, w2)), __fmul_rn(p3, w3));   // tf_interpolate.cpp:122
}

// tl_fp_l1_forward_kernel with the row mask. A lane whose row is padding (or past the end) redirects its loads of idx, dist
// and Q to row c n of its cloud (row 0 past the end), which is valid by the clamp of the lengths to 1..n -- the dense kernel's
// `base` may itself be padding -- and does not read z at all; what it computes from there is dropped by the selects below.
__global__ __launch_bounds__(kFprThreads) void tl_fp_l1_forward_masked_kernel(long long rows, int n, int m, int C,
                                                                              const int *__restrict__ idx, const float *__restrict__ dist,
                                                                              float *__restrict__ weight, const float *__restrict__ Q,
                                                                              float *z, int add, const unsigned *__restrict__ mask,
                                                                              double *__restrict__ stats)
{
    const int qpr = C / 4, q = threadIdx.x % qpr, rl = threadIdx.x / qpr, rpb = kFprThreads / qpr, col = 4 * q;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    const long long stride = rpb, span = (long long)kFprU * stride;
    const long long chunk = (rows + (long long)gridDim.x * span - 1) / ((long long)gridDim.x * span) * span;
    const long long first = (long long)blockIdx.x * chunk, stop = first + chunk < rows ? first + chunk : rows;
    for (long long base = first + rl; base < stop; base += span) {
        long long row[kFprU], src[kFprU];
        bool inb[kFprU], ok[kFprU];
        float w[kFprU][3];
        const float *qa[kFprU][3];
#pragma unroll
        for (int u = 0; u < kFprU; ++u) {
            const long long rr = base + u * stride;
            inb[u] = rr < rows;
            row[u] = inb[u] ? rr : 0;
            ok[u] = inb[u] && ((mask[row[u] >> 5] >> (unsigned)(row[u] & 31)) & 1u);
            src[u] = ok[u] ? rr : row[u] / n * n;                 // the cloud's first row: always valid
        }
#pragma unroll
        for (int u = 0; u < kFprU; ++u) {
            const long long r = src[u];
            const float *dp = dist + r * 3;
            const int *ip = idx + r * 3;
            // the weights exactly as pn2_fp_interp_concat forms them (csrc/interpolate.hip, pointnet_util.py:212-215)
            const float r1 = __fdiv_rn(1.0f, fmaxf(dp[0], 1e-10f)), r2 = __fdiv_rn(1.0f, fmaxf(dp[1], 1e-10f)),
                        r3 = __fdiv_rn(1.0f, fmaxf(dp[2], 1e-10f));
            const float norm = __fadd_rn(__fadd_rn(r1, r2), r3);
            w[u][0] = __fdiv_rn(r1, norm); w[u][1] = __fdiv_rn(r2, norm); w[u][2] = __fdiv_rn(r3, norm);
            if (q == 0 && inb[u] && weight) {
                float *wp = weight + row[u] * 3;
                wp[0] = ok[u] ? w[u][0] : 0.0f; wp[1] = ok[u] ? w[u][1] : 0.0f; wp[2] = ok[u] ? w[u][2] : 0.0f;
            }
            const float *qb = Q + (r / n) * (long long)m * C + col;
            qa[u][0] = qb + (long long)ip[0] * C; qa[u][1] = qb + (long long)ip[1] * C; qa[u][2] = qb + (long long)ip[2] * C;
        }
        float4 a[kFprU][3], zo[kFprU];
#pragma unroll
        for (int u = 0; u < kFprU; ++u) {
            a[u][0] = fpr_ld4(qa[u][0]); a[u][1] = fpr_ld4(qa[u][1]); a[u][2] = fpr_ld4(qa[u][2]);
            zo[u] = (add && ok[u]) ? fpr_ld4(z + row[u] * C + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < kFprU; ++u) {
            float v[4] = {fpr_interp3(a[u][0].x, a[u][1].x, a[u][2].x, w[u][0], w[u][1], w[u][2]),
                          fpr_interp3(a[u][0].y, a[u][1].y, a[u][2].y, w[u][0], w[u][1], w[u][2]),
                          fpr_interp3(a[u][0].z, a[u][1].z, a[u][2].z, w[u][0], w[u][1], w[u][2]),
                          fpr_interp3(a[u][0].w, a[u][1].w, a[u][2].w, w[u][0], w[u][1], w[u][2])};
            if (add) { v[0] = __fadd_rn(v[0], zo[u].x); v[1] = __fadd_rn(v[1], zo[u].y); v[2] = __fadd_rn(v[2], zo[u].z); v[3] = __fadd_rn(v[3], zo[u].w); }
            if (ok[u]) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { s1[i] += (double)v[i]; s2[i] += (double)v[i] * (double)v[i]; }
                *reinterpret_cast<float4 *>(z + row[u] * C + col) = make_float4(v[0], v[1], v[2], v[3]);
            } else if (inb[u]) {
                *reinterpret_cast<float4 *>(z + row[u] * C + col) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    __shared__ double red[2][kFprThreads][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { red[0][threadIdx.x][i] = s1[i]; red[1][threadIdx.x][i] = s2[i]; }
    __syncthreads();
    if (rl == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double x = 0.0, y = 0.0;
            for (int k = 0; k < rpb; ++k) { x += red[0][k * qpr + q][i]; y += red[1][k * qpr + q][i]; }
            stats[((size_t)blockIdx.x * 2) * C + col + i] = x;
            stats[((size_t)blockIdx.x * 2 + 1) * C + col + i] = y;
        }
    }
}

// tl_fp_l1_dz_kernel with the row mask: dz_1 = valid ? s dy_1 - c0 - c1 z_1 : +0.0, in place over dy_1
__global__ __launch_bounds__(256) void tl_fp_l1_dz_masked_kernel(long long total4, int C, const float *__restrict__ z, float *g,
                                                                 const float *__restrict__ coef, const unsigned *__restrict__ mask)
{
    const int q4 = C / 4;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long long)gridDim.x * 256) {
        const long long row = e / q4;
        const int col = (int)(e - row * q4) * 4;
        const bool rv = (mask[row >> 5] >> (unsigned)(row & 31)) & 1u;
        const float4 dy = reinterpret_cast<const float4 *>(g)[e], zz = reinterpret_cast<const float4 *>(z)[e];
        const float4 s = fpr_ld4(coef + col), c0 = fpr_ld4(coef + C + col), c1 = fpr_ld4(coef + 2 * C + col);
        float4 o;
        o.x = rv ? __fsub_rn(__fsub_rn(__fmul_rn(s.x, dy.x), c0.x), __fmul_rn(c1.x, zz.x)) : 0.0f;
        o.y = rv ? __fsub_rn(__fsub_rn(__fmul_rn(s.y, dy.y), c0.y), __fmul_rn(c1.y, zz.y)) : 0.0f;
        o.z = rv ? __fsub_rn(__fsub_rn(__fmul_rn(s.z, dy.z), c0.z), __fmul_rn(c1.z, zz.z)) : 0.0f;
        o.w = rv ? __fsub_rn(__fsub_rn(__fmul_rn(s.w, dy.w), c0.w), __fmul_rn(c1.w, zz.w)) : 0.0f;
        reinterpret_cast<float4 *>(g)[e] = o;
    }
}

// ---- launches for train_mlp.hip: fp_launch_l1_forward / fp_launch_l1_dz with the validity words ----
int fp_launch_l1_forward_masked(long long rows, int n, int m, int C, const int *idx, const float *dist, float *weight, const float *Q,
                                float *z, bool add, const unsigned *mask, double *stats, int max_parts, hipStream_t st, int *nparts)
{
    const int rpb = kFprThreads / (C / 4);
    long long blocks = (rows + (long long)rpb * kFprU - 1) / ((long long)rpb * kFprU);
    if (blocks > max_parts) blocks = max_parts;
    *nparts = (int)blocks;
    return launch(tl_fp_l1_forward_masked_kernel, dim3((unsigned)blocks), dim3(kFprThreads), 0, st, rows, n, m, C, idx, dist, weight, Q, z,
                  add ? 1 : 0, mask, stats);
}

int fp_launch_l1_dz_masked(long long rows, int C, const float *z, float *g, const float *coef, const unsigned *mask, hipStream_t st)
{
    const long long total4 = rows * C / 4;
    long long blocks = (total4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    return launch(tl_fp_l1_dz_masked_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(256), 0, st, total4, C, z, g, coef, mask);
}

}  // namespace pn2
