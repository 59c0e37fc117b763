// train_mlp_fp.hip -- the training node of a feature-propagation level (pointnet_fp_module, utils/pointnet_util.py:211-226)
// with layer 1 evaluated once per KNOWN point: the entry points, their argument checks and the kernels only this level type
// needs. The passes themselves are train_mlp.hip's (tl_train_forward / tl_train_backward with TlCall::fp). gfx950.
//
// Layer 1 and the interpolation are both linear, so
//     z_1 = [interp(points2), points1] W_1 = interp(points2 W1a) + points1 W1b
// (W1a: the first c2 input rows of W_1, W1b: the last c1 -- the reference's concat order, :219; the inference kernel uses the
// same identity, csrc/fp_mlp.hip). Forward:
//     Q    = points2 W1a                      GEMM over the b m known points (E_STORE, no moments)
//     z_1  = points1 W1b                      GEMM over the b n rows (c1 > 0)
//     z_1 += (Q[i1] w1 + Q[i2] w2) + Q[i3] w3 tl_fp_l1_forward_kernel: the weights from dist, partial rows of sum z, sum z^2
// then layers 2..L as on every other level. Backward, after the passes of layers L..2:
//     dz_1 = s dy_1 - c0 - c1 z_1             in place (tl_fp_l1_dz_kernel)
//     S    = three_interpolate_grad(dz_1)     onto (b m, C_1): pn2_three_interpolate_grad_seg
//     dW1a = points2^T S,   grad_points2 = S W1a^T       over the b m known points
//     dW1b = points1^T dz_1, grad_points1 = dz_1 W1b^T   over the b n rows
// each pair in one launch where the shapes have a pair kernel. The concatenated (b, n, c2 + c1) input and its gradient are
// never written. Widths that are no multiple of 4 enter as zero-padded copies of points2 / points1 alone, and b m known
// points as a copy of points2 padded to a multiple of 32 rows.
//
// A RAGGED unknown side (pn2_mlp_train_*_fp_ragged). The two vector-unit passes have masked twins, kernels of their own beside
// the dense ones. Row r of the b n unknown points is valid iff bit r & 31 of validity word r >> 5 is set (the mask buffer of
// pn2_mlp_train_*_ragged, written by tl_ragged_mask_kernel from `lengths`; train_mlp_ragged.hip). The two values DESIGN.md
// section 4.11 names are taken as zero on a padding row, by SELECTS (points1, dist, grad_out may hold NaN there):
//   z_1   where it is formed: nothing of idx, dist, Q or of what the points1 W1b GEMM left in the row is used; the row is
//         written as +0.0, its weights as (0, 0, 0), and it adds nothing to the partial moments;
//   dz_1  where it is formed: s dy_1 - c0 - c1 z_1 would be -c0; the row is written as +0.0.
// Everything behind them (layers 2..L, the weight gradients, the interpolation gradient) then meets zero rows.
// With every row valid the masked forward kernel runs the dense kernel's operations on the dense kernel's rows in the dense
// kernel's order (same thread <-> (row lane, 4 columns) mapping, chunking, kFpU, partial-moment layout): the same bits.
//
// idx on padding rows. The interpolation gradient behind the dz pass (pn2_three_interpolate_grad_seg / _planned) reads idx and
// weight on EVERY row, so padding rows must hold indices in [0, m): ragged three_nn writes (0, 0, 0) there, and with the zero
// weights written here those rows add 0 * 0 to known point 0 of their cloud -- one long segment per short cloud, which the
// segmented kernels handle, and the same as on the fp_interp_concat route. That cost is not addressed here.
//
// The dense and the masked kernel of a pass stay TWINS: one `template <bool MASKED>` body inlined into both changes the
// generated code of all four (e % q4 against e / q4, the fallback row `base` against 0, ...), so merging the bodies is a change
// of its own with a GPU timing, not a tidying.
#include "train_mlp_internal.h"

namespace pn2 {

constexpr int kFpThreads = 512, kFpU = 4;

// layer 1's width on the vector-unit pass: thread <-> 4 columns of a row, whole rows per 512-thread workgroup
static bool fp_width_ok(int C)
{
    return C > 0 && C % 4 == 0 && C / 4 <= kFpThreads && kFpThreads % (C / 4) == 0;
}

__device__ __forceinline__ float4 fp_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

__device__ __forceinline__ float fp_interp3(float p1, float p2, float p3, float w1, float w2, float w3)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(p1, w1), __fmul_rn(p2, w2)), __fmul_rn(p3, w3));   // tf_interpolate.cpp:122
}

__global__ __launch_bounds__(256) void tl_fp_pad_kernel(long long rows_in, int c, long long total, int cp,
                                                        const float *__restrict__ src, float *__restrict__ dst)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / cp;
        const int k = (int)(e - r * cp);
        dst[e] = (r < rows_in && k < c) ? src[r * c + k] : 0.0f;
    }
}

// thread <-> (row lane, 4 columns) as tl_l1_forward_kernel; a workgroup walks one contiguous range of rows, kFpU rows in
// flight per thread (index -> weights -> three rows of Q is a chain of dependent loads)
__global__ __launch_bounds__(kFpThreads) void tl_fp_l1_forward_kernel(long long rows, int n, int m, int C, const int *__restrict__ idx,
                                                                      const float *__restrict__ dist, float *__restrict__ weight,
                                                                      const float *__restrict__ Q, float *z, int add,
                                                                      double *__restrict__ stats)
{
    const int qpr = C / 4, q = threadIdx.x % qpr, rl = threadIdx.x / qpr, rpb = kFpThreads / qpr, col = 4 * q;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    const long long stride = rpb, span = (long long)kFpU * stride;
    const long long chunk = (rows + (long long)gridDim.x * span - 1) / ((long long)gridDim.x * span) * span;
    const long long first = (long long)blockIdx.x * chunk, stop = first + chunk < rows ? first + chunk : rows;
    for (long long base = first + rl; base < stop; base += span) {
        long long row[kFpU];
        bool ok[kFpU];
        float w[kFpU][3];
        const float *qa[kFpU][3];
#pragma unroll
        for (int u = 0; u < kFpU; ++u) {
            const long long rr = base + u * stride;
            ok[u] = rr < rows;
            row[u] = ok[u] ? rr : base;
        }
#pragma unroll
        for (int u = 0; u < kFpU; ++u) {
            const long long r = row[u];
            const float *dp = dist + r * 3;
            const int *ip = idx + r * 3;
            // the weights exactly as pn2_fp_interp_concat forms them (csrc/interpolate.hip, pointnet_util.py:212-215)
            const float r1 = __fdiv_rn(1.0f, fmaxf(dp[0], 1e-10f)), r2 = __fdiv_rn(1.0f, fmaxf(dp[1], 1e-10f)),
                        r3 = __fdiv_rn(1.0f, fmaxf(dp[2], 1e-10f));
            const float norm = __fadd_rn(__fadd_rn(r1, r2), r3);
            w[u][0] = __fdiv_rn(r1, norm); w[u][1] = __fdiv_rn(r2, norm); w[u][2] = __fdiv_rn(r3, norm);
            if (q == 0 && ok[u] && weight) { weight[r * 3] = w[u][0]; weight[r * 3 + 1] = w[u][1]; weight[r * 3 + 2] = w[u][2]; }
            const float *qb = Q + (r / n) * (long long)m * C + col;
            qa[u][0] = qb + (long long)ip[0] * C; qa[u][1] = qb + (long long)ip[1] * C; qa[u][2] = qb + (long long)ip[2] * C;
        }
        float4 a[kFpU][3], zo[kFpU];
#pragma unroll
        for (int u = 0; u < kFpU; ++u) {
            a[u][0] = fp_ld4(qa[u][0]); a[u][1] = fp_ld4(qa[u][1]); a[u][2] = fp_ld4(qa[u][2]);
            zo[u] = add ? fp_ld4(z + row[u] * C + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < kFpU; ++u) {
            float v[4] = {fp_interp3(a[u][0].x, a[u][1].x, a[u][2].x, w[u][0], w[u][1], w[u][2]),
                          fp_interp3(a[u][0].y, a[u][1].y, a[u][2].y, w[u][0], w[u][1], w[u][2]),
                          fp_interp3(a[u][0].z, a[u][1].z, a[u][2].z, w[u][0], w[u][1], w[u][2]),
                          fp_interp3(a[u][0].w, a[u][1].w, a[u][2].w, w[u][0], w[u][1], w[u][2])};
            if (add) { v[0] = __fadd_rn(v[0], zo[u].x); v[1] = __fadd_rn(v[1], zo[u].y); v[2] = __fadd_rn(v[2], zo[u].z); v[3] = __fadd_rn(v[3], zo[u].w); }
            if (ok[u]) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { s1[i] += (double)v[i]; s2[i] += (double)v[i] * (double)v[i]; }
                *reinterpret_cast<float4 *>(z + row[u] * C + col) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
    __shared__ double red[2][kFpThreads][4];
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

// tl_fp_l1_forward_kernel with the row mask. A lane whose row is padding (or past the end) redirects its loads of idx, dist
// and Q to row c n of its cloud (row 0 past the end), which is valid by the clamp of the lengths to 1..n -- the dense kernel's
// `base` may itself be padding -- and does not read z at all; what it computes from there is dropped by the selects below.
__global__ __launch_bounds__(kFpThreads) void tl_fp_l1_forward_masked_kernel(long long rows, int n, int m, int C,
                                                                              const int *__restrict__ idx, const float *__restrict__ dist,
                                                                              float *__restrict__ weight, const float *__restrict__ Q,
                                                                              float *z, int add, const unsigned *__restrict__ mask,
                                                                              double *__restrict__ stats)
{
    const int qpr = C / 4, q = threadIdx.x % qpr, rl = threadIdx.x / qpr, rpb = kFpThreads / qpr, col = 4 * q;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    const long long stride = rpb, span = (long long)kFpU * stride;
    const long long chunk = (rows + (long long)gridDim.x * span - 1) / ((long long)gridDim.x * span) * span;
    const long long first = (long long)blockIdx.x * chunk, stop = first + chunk < rows ? first + chunk : rows;
    for (long long base = first + rl; base < stop; base += span) {
        long long row[kFpU], src[kFpU];
        bool inb[kFpU], ok[kFpU];
        float w[kFpU][3];
        const float *qa[kFpU][3];
#pragma unroll
        for (int u = 0; u < kFpU; ++u) {
            const long long rr = base + u * stride;
            inb[u] = rr < rows;
            row[u] = inb[u] ? rr : 0;
            ok[u] = inb[u] && ((mask[row[u] >> 5] >> (unsigned)(row[u] & 31)) & 1u);
            src[u] = ok[u] ? rr : row[u] / n * n;                 // the cloud's first row: always valid
        }
#pragma unroll
        for (int u = 0; u < kFpU; ++u) {
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
        float4 a[kFpU][3], zo[kFpU];
#pragma unroll
        for (int u = 0; u < kFpU; ++u) {
            a[u][0] = fp_ld4(qa[u][0]); a[u][1] = fp_ld4(qa[u][1]); a[u][2] = fp_ld4(qa[u][2]);
            zo[u] = (add && ok[u]) ? fp_ld4(z + row[u] * C + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < kFpU; ++u) {
            float v[4] = {fp_interp3(a[u][0].x, a[u][1].x, a[u][2].x, w[u][0], w[u][1], w[u][2]),
                          fp_interp3(a[u][0].y, a[u][1].y, a[u][2].y, w[u][0], w[u][1], w[u][2]),
                          fp_interp3(a[u][0].z, a[u][1].z, a[u][2].z, w[u][0], w[u][1], w[u][2]),
                          fp_interp3(a[u][0].w, a[u][1].w, a[u][2].w, w[u][0], w[u][1], w[u][2])};
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
    __shared__ double red[2][kFpThreads][4];
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

// dz_1 = s dy_1 - c0 - c1 z_1, the operations of the GEMMs' A_DZ prologue (train_mlp_device.h, tl_finish), in place over dy_1
__global__ __launch_bounds__(256) void tl_fp_l1_dz_kernel(long long total4, int C, const float *__restrict__ z, float *g,
                                                          const float *__restrict__ coef)
{
    const int q4 = C / 4;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long long)gridDim.x * 256) {
        const int col = (int)(e % q4) * 4;
        const float4 dy = reinterpret_cast<const float4 *>(g)[e], zz = reinterpret_cast<const float4 *>(z)[e];
        const float4 s = fp_ld4(coef + col), c0 = fp_ld4(coef + C + col), c1 = fp_ld4(coef + 2 * C + col);
        float4 o;
        o.x = __fsub_rn(__fsub_rn(__fmul_rn(s.x, dy.x), c0.x), __fmul_rn(c1.x, zz.x));
        o.y = __fsub_rn(__fsub_rn(__fmul_rn(s.y, dy.y), c0.y), __fmul_rn(c1.y, zz.y));
        o.z = __fsub_rn(__fsub_rn(__fmul_rn(s.z, dy.z), c0.z), __fmul_rn(c1.z, zz.z));
        o.w = __fsub_rn(__fsub_rn(__fmul_rn(s.w, dy.w), c0.w), __fmul_rn(c1.w, zz.w));
        reinterpret_cast<float4 *>(g)[e] = o;
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
        const float4 s = fp_ld4(coef + col), c0 = fp_ld4(coef + C + col), c1 = fp_ld4(coef + 2 * C + col);
        float4 o;
        o.x = rv ? __fsub_rn(__fsub_rn(__fmul_rn(s.x, dy.x), c0.x), __fmul_rn(c1.x, zz.x)) : 0.0f;
        o.y = rv ? __fsub_rn(__fsub_rn(__fmul_rn(s.y, dy.y), c0.y), __fmul_rn(c1.y, zz.y)) : 0.0f;
        o.z = rv ? __fsub_rn(__fsub_rn(__fmul_rn(s.z, dy.z), c0.z), __fmul_rn(c1.z, zz.z)) : 0.0f;
        o.w = rv ? __fsub_rn(__fsub_rn(__fmul_rn(s.w, dy.w), c0.w), __fmul_rn(c1.w, zz.w)) : 0.0f;
        reinterpret_cast<float4 *>(g)[e] = o;
    }
}

static unsigned grid_of(long long work, long long cap)
{
    long long blocks = (work + 255) / 256;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

// ---- launches for train_mlp.hip ----
// dst (rows_out, cp) = src (rows_in, c) zero-padded (rows_out >= rows_in, cp >= c); a plain copy when the shapes agree
int fp_launch_pad(const float *src, long long rows_in, int c, long long rows_out, int cp, float *dst, hipStream_t st)
{
    const long long total = rows_out * cp;
    return launch(tl_fp_pad_kernel, dim3(grid_of(total, 4096)), dim3(256), 0, st, rows_in, c, total, cp, src, dst);
}

// z_1 (rows, C) = interp(Q) [+ z_1 when `add`]; the weights to `weight`; (nparts, 2, C) fp64 partial moments.
// mask: the validity words of a ragged unknown side (the masked twin runs), or nullptr: every row is valid
int fp_launch_l1_forward(long long rows, int n, int m, int C, const int *idx, const float *dist, float *weight, const float *Q,
                         float *z, bool add, const unsigned *mask, double *stats, int max_parts, hipStream_t st, int *nparts)
{
    const int rpb = kFpThreads / (C / 4);
    long long blocks = (rows + (long long)rpb * kFpU - 1) / ((long long)rpb * kFpU);
    if (blocks > max_parts) blocks = max_parts;
    *nparts = (int)blocks;
    const dim3 grid((unsigned)blocks), block(kFpThreads);
    if (mask) return launch(tl_fp_l1_forward_masked_kernel, grid, block, 0, st, rows, n, m, C, idx, dist, weight, Q, z, add ? 1 : 0, mask, stats);
    return launch(tl_fp_l1_forward_kernel, grid, block, 0, st, rows, n, m, C, idx, dist, weight, Q, z, add ? 1 : 0, stats);
}

// dz_1 = s dy_1 - c0 - c1 z_1 in place over dy_1 (coef: (3, C)); mask as above: +0.0 on a padding row
int fp_launch_l1_dz(long long rows, int C, const float *z, float *g, const float *coef, const unsigned *mask, hipStream_t st)
{
    const long long total4 = rows * C / 4;
    const dim3 grid(grid_of(total4, 8192));
    if (mask) return launch(tl_fp_l1_dz_masked_kernel, grid, dim3(256), 0, st, total4, C, z, g, coef, mask);
    return launch(tl_fp_l1_dz_kernel, grid, dim3(256), 0, st, total4, C, z, g, coef);
}

// ---- argument checks ----
static int fp_dims(const pn2_fp_src *s)
{
    if (s->b <= 0 || s->n <= 0 || s->m <= 0 || s->c2 <= 0 || s->c1 < 0) return PN2_E_ARG;
    const long long rows = (long long)s->b * s->n, bm = (long long)s->b * s->m;
    if (rows % 32 || rows >= (1ll << 31) || bm >= (1ll << 31) - 32) return PN2_E_ARG;
    return PN2_OK;
}

// widths (cin_1 = c2 + c1, cout_1 .. cout_L) this node runs: at most 7 layers (the forward pack launch takes one job per layer
// plus W1b), widths multiples of 4, layer 1's on the vector-unit pass
static bool fp_widths_ok(int nlayers, const int *widths, const pn2_fp_src *s)
{
    if (!widths || nlayers < 1 || nlayers > 7 || widths[0] != s->c2 + s->c1 || !fp_width_ok(widths[1])) return false;
    for (int l = 1; l <= nlayers; ++l)
        if (widths[l] <= 0 || widths[l] % 4) return false;
    return true;
}

static int fp_layer_widths(int nlayers, const pn2_bn_layer *layers, int *widths)
{
    if (!layers || nlayers < 1 || nlayers > 7) return PN2_E_ARG;
    widths[0] = layers[0].cin;
    for (int l = 0; l < nlayers; ++l) {
        if (l > 0 && layers[l].cin != layers[l - 1].cout) return PN2_E_ARG;
        widths[l + 1] = layers[l].cout;
    }
    return PN2_OK;
}

// the checks both directions make first, in this order
static int fp_level_args(int nlayers, const pn2_bn_layer *layers, const pn2_fp_src *src)
{
    if (!src) return PN2_E_NULL;
    int widths[9];
    if (int rc = fp_dims(src)) return rc;
    if (int rc = fp_layer_widths(nlayers, layers, widths)) return rc;
    return fp_widths_ok(nlayers, widths, src) ? PN2_OK : PN2_E_ARG;
}

static TlCall fp_call(int nlayers, const pn2_bn_layer *layers, const FpL1 &f, const float *out, void *ws, const pn2_train_opts *opts,
                      void *stream)
{
    TlCall c{};
    c.rows = f.rows; c.nlayers = nlayers; c.layers = layers;
    c.has_fp = true; c.fp = f;
    c.out = out;
    c.ws = ws; c.opts = opts; c.stream = stream;
    return c;
}

}  // namespace pn2

extern "C" int pn2_mlp_train_fp_supported(int b, int n, int m, int c2, int c1, int nlayers, const int *widths)
{
    using namespace pn2;
    const pn2_fp_src s = {b, n, m, c2, c1, nullptr, nullptr, nullptr, nullptr};
    if (fp_dims(&s) || !fp_widths_ok(nlayers, widths, &s)) return 0;
    return tl_fp_ws_bytes(&s, nlayers, widths, 0, nullptr) > 0 && tl_fp_ws_bytes(&s, nlayers, widths, 1, nullptr) > 0 ? 1 : 0;
}

extern "C" long long pn2_mlp_train_ws_bytes_fp(int b, int n, int m, int c2, int c1, int nlayers, const int *widths, int backward,
                                               const pn2_train_opts *opts)
{
    using namespace pn2;
    const pn2_fp_src s = {b, n, m, c2, c1, nullptr, nullptr, nullptr, nullptr};
    if (fp_dims(&s) || !fp_widths_ok(nlayers, widths, &s)) return -1;
    return tl_fp_ws_bytes(&s, nlayers, widths, backward, opts);
}

extern "C" int pn2_mlp_train_forward_fp(int nlayers, const pn2_bn_layer *layers, const pn2_fp_src *src, float *out, float *weight,
                                        void *ws, const pn2_train_opts *opts, void *stream)
{
    using namespace pn2;
    if (int rc = fp_level_args(nlayers, layers, src)) return rc;
    if (src->c1 == 0 && src->points1) return PN2_E_ARG;
    if (!src->points2 || !src->idx || !src->dist || (src->c1 > 0 && !src->points1) || !out || !weight || !ws) return PN2_E_NULL;
    FpL1 f = fp_l1(src);
    f.weight_out = weight;
    return tl_train_forward(fp_call(nlayers, layers, f, out, ws, opts, stream));
}

extern "C" int pn2_mlp_train_backward_fp(int nlayers, const pn2_bn_layer *layers, const pn2_fp_src *src, const float *weight,
                                         const float *out, const float *grad_out, float *grad_points2, float *grad_points1,
                                         int reproducible, void *ws, const pn2_train_opts *opts, void *stream)
{
    using namespace pn2;
    if (int rc = fp_level_args(nlayers, layers, src)) return rc;
    if (src->c1 == 0 && (src->points1 || grad_points1)) return PN2_E_ARG;
    if (!src->points2 || !src->idx || (src->c1 > 0 && !src->points1) || !weight || !out || !grad_out || !ws) return PN2_E_NULL;
    FpL1 f = fp_l1(src);
    f.weight = weight;
    f.grad_points2 = grad_points2;
    f.grad_points1 = grad_points1;
    TlCall c = fp_call(nlayers, layers, f, out, ws, opts, stream);
    c.grad_out = grad_out;
    c.reproducible = reproducible;
    return tl_train_backward(c);
}

// ---- the same node with a RAGGED unknown side (pn2_mlp_train_*_fp_ragged, include/pn2ops.h): TlCall::mask beside TlCall::fp.
// The masked layer-1 passes are the twins above, everything else the masked passes of the plain-rows ragged node
// (train_mlp_ragged.hip) under its one organisation (ragged_opts, train_mlp.hip). pn2_fp_src is the dense entries'.
extern "C" int pn2_mlp_train_fp_ragged_supported(int b, int n, int m, int c2, int c1, int nlayers, const int *widths)
{
    using namespace pn2;
    if (!pn2_mlp_train_fp_supported(b, n, m, c2, c1, nlayers, widths)) return 0;
    const long long rows = (long long)b * n;
    if (rows <= 0 || rows % 32) return 0;
    const pn2_fp_src s = {b, n, m, c2, c1, nullptr, nullptr, nullptr, nullptr};
    return tl_fp_ws_bytes(&s, nlayers, widths, 0, nullptr, true) > 0 && tl_fp_ws_bytes(&s, nlayers, widths, 1, nullptr, true) > 0 ? 1 : 0;
}

extern "C" long long pn2_mlp_train_ws_bytes_fp_ragged(int b, int n, int m, int c2, int c1, int nlayers, const int *widths, int backward,
                                                      const pn2_train_opts *opts)
{
    using namespace pn2;
    const pn2_fp_src s = {b, n, m, c2, c1, nullptr, nullptr, nullptr, nullptr};
    if (fp_dims(&s) || !fp_widths_ok(nlayers, widths, &s)) return -1;
    return tl_fp_ws_bytes(&s, nlayers, widths, backward, opts, true);
}

extern "C" int pn2_mlp_train_forward_fp_ragged(int nlayers, const pn2_bn_layer *layers, const pn2_fp_src *src, const int *lengths,
                                               float *out, float *weight, void *mask, void *ws, const pn2_train_opts *opts, void *stream)
{
    using namespace pn2;
    if (!lengths || !mask) return PN2_E_NULL;
    if (int rc = fp_level_args(nlayers, layers, src)) return rc;
    if (src->c1 == 0 && src->points1) return PN2_E_ARG;
    if (!src->points2 || !src->idx || !src->dist || (src->c1 > 0 && !src->points1) || !out || !weight || !ws) return PN2_E_NULL;
    FpL1 f = fp_l1(src);
    f.weight_out = weight;
    TlCall c = fp_call(nlayers, layers, f, out, ws, opts, stream);
    c.mask = mask; c.lengths = lengths; c.rg_b = src->b; c.rg_n = src->n;
    return tl_train_forward(c);
}

extern "C" int pn2_mlp_train_backward_fp_ragged(int nlayers, const pn2_bn_layer *layers, const pn2_fp_src *src, const int *lengths,
                                                const float *weight, const float *out, const float *grad_out, float *grad_points2,
                                                float *grad_points1, int reproducible, const void *mask, void *ws,
                                                const pn2_train_opts *opts, void *stream)
{
    using namespace pn2;
    (void)lengths;                                                 // taken for symmetry: backward reads the mask forward wrote
    if (!mask) return PN2_E_NULL;
    if (int rc = fp_level_args(nlayers, layers, src)) return rc;
    if (src->c1 == 0 && (src->points1 || grad_points1)) return PN2_E_ARG;
    if (!src->points2 || !src->idx || (src->c1 > 0 && !src->points1) || !weight || !out || !grad_out || !ws) return PN2_E_NULL;
    FpL1 f = fp_l1(src);
    f.weight = weight;
    f.grad_points2 = grad_points2;
    f.grad_points1 = grad_points1;
    TlCall c = fp_call(nlayers, layers, f, out, ws, opts, stream);
    c.mask = const_cast<void *>(mask); c.rg_b = src->b; c.rg_n = src->n;
    c.grad_out = grad_out;
    c.reproducible = reproducible;
    return tl_train_backward(c);
}
