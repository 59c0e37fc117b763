// train_mlp_small.hip -- the small kernels between the passes of the training node: the per-channel finalisations, the top
// of the stack in both directions, the pooling modes. One launch function each. gfx950.
#include "train_mlp_device.h"

namespace pn2 {

// ---- per-channel finalisation kernels (one thread per channel) -----------------------------------------------------------
// batch moments -> (mean, invstd, a, c), running statistics (torch.nn.BatchNorm semantics: unbiased variance in the average)
// the per-channel sums arrive as `nparts` partial rows; a block of 256 threads owns 8 channels and adds the rows 32 at a time
__device__ __forceinline__ void tl_sum_parts(const double *__restrict__ stats, int nparts, int N, double &s1, double &s2)
{
    __shared__ double sh[2][32][8];
    const int g = threadIdx.x >> 3, cl = threadIdx.x & 7, c = blockIdx.x * 8 + cl;
    double a = 0.0, b = 0.0;
    if (c < N)
        for (int q = g; q < nparts; q += 32) { a += stats[((size_t)q * 2) * N + c]; b += stats[((size_t)q * 2 + 1) * N + c]; }
    sh[0][g][cl] = a;
    sh[1][g][cl] = b;
    __syncthreads();
    s1 = 0.0; s2 = 0.0;
    if (g == 0) {
#pragma unroll
        for (int i = 0; i < 32; ++i) { s1 += sh[0][i][cl]; s2 += sh[1][i][cl]; }
    }
}

__global__ __launch_bounds__(256) void tl_bn_finalize_kernel(const double *__restrict__ stats, int nparts, int N, double count,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             float *running_mean, float *running_var, float momentum, float eps,
                                                             float *__restrict__ save, const float *__restrict__ bias, int var_biased)
{
    double s1, s2;
    tl_sum_parts(stats, nparts, N, s1, s2);
    const int c = blockIdx.x * 8 + (threadIdx.x & 7);
    if (threadIdx.x >= 8 || c >= N) return;
    tl_bn_finalize_channel(c, N, s1, s2, count, gamma, beta, running_mean, running_var, momentum, eps, save, bias, var_biased);
}

// (sum dy, sum dy z) -> grad_gamma, grad_beta and the coefficients of dz = s dy - c0 - c1 z
__global__ __launch_bounds__(256) void tl_bn_backward_finalize_kernel(const double *__restrict__ stats, int nparts, int N,
                                                                      double count, const float *__restrict__ gamma,
                                                                      const float *__restrict__ save, float *__restrict__ grad_gamma,
                                                                      float *__restrict__ grad_beta, float *__restrict__ coef, int accumulate)
{
    double s1, s2;
    tl_sum_parts(stats, nparts, N, s1, s2);
    const int c = blockIdx.x * 8 + (threadIdx.x & 7);
    if (threadIdx.x >= 8 || c >= N) return;
    tl_bn_backward_finalize_channel(c, N, s1, s2, count, gamma, save, grad_gamma, grad_beta, coef, accumulate);
}

// ... the same two with the row count read from device memory: the plain rows of a ragged batch (train_mlp_ragged.hip), whose
// count is the number of valid rows -- a sum of clamped lengths the host never sees
__global__ __launch_bounds__(256) void tl_bn_finalize_counted_kernel(const double *__restrict__ stats, int nparts, int N,
                                                                     const double *__restrict__ count, const float *__restrict__ gamma,
                                                                     const float *__restrict__ beta, float *running_mean,
                                                                     float *running_var, float momentum, float eps,
                                                                     float *__restrict__ save, const float *__restrict__ bias,
                                                                     int var_biased)
{
    double s1, s2;
    tl_sum_parts(stats, nparts, N, s1, s2);
    const int c = blockIdx.x * 8 + (threadIdx.x & 7);
    if (threadIdx.x >= 8 || c >= N) return;
    tl_bn_finalize_channel(c, N, s1, s2, *count, gamma, beta, running_mean, running_var, momentum, eps, save, bias, var_biased);
}

__global__ __launch_bounds__(256) void tl_bn_backward_finalize_counted_kernel(const double *__restrict__ stats, int nparts, int N,
                                                                              const double *__restrict__ count,
                                                                              const float *__restrict__ gamma,
                                                                              const float *__restrict__ save,
                                                                              float *__restrict__ grad_gamma,
                                                                              float *__restrict__ grad_beta, float *__restrict__ coef,
                                                                              int accumulate)
{
    double s1, s2;
    tl_sum_parts(stats, nparts, N, s1, s2);
    const int c = blockIdx.x * 8 + (threadIdx.x & 7);
    if (threadIdx.x >= 8 || c >= N) return;
    tl_bn_backward_finalize_channel(c, N, s1, s2, *count, gamma, save, grad_gamma, grad_beta, coef, accumulate);
}

// pool: partial extrema of z (the max where gamma >= 0, else the min) -> out = relu(a zsel + c), the sample the gradient flows to, zsel
__global__ void tl_pool_finalize_kernel(long long groups, int N, int parts, int prow, const float *__restrict__ pmax,
                                        const int *__restrict__ pamax, const float *__restrict__ gamma,
                                        const float *__restrict__ save,
                                        float *__restrict__ out, int *__restrict__ argsel, float *__restrict__ zsel)
{
    const long long total = groups * N;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long g = i / N;
        const int c = (int)(i - g * N);
        const float a = save[2 * N + c], cc = save[3 * N + c];
        const bool up = gamma[c] >= 0.0f;                          // the rule of the GEMM epilogue that wrote the partials
        float best = 0.0f;
        int arg = 0;
        for (int q = 0; q < parts; ++q) {
            const size_t o = (size_t)(g * parts + q) * N + c;
            const float v = pmax[o];
            const int r = pamax[o] + q * prow;
            if (q == 0 || (up ? v > best : v < best)) { best = v; arg = r; }
        }
        out[i] = vmax(__fadd_rn(__fmul_rn(a, best), cc), 0.0f);
        argsel[i] = arg;
        zsel[i] = best;
    }
}

// ... on the grouped rows of a ragged batch (train_mlp_ragged_group.hip): the pool as a pass of its own over the STORED z_L,
// behind its finalisation. Per group and channel the extremum of z over the VALID rows (the dense rule: the max where
// gamma >= 0, else the min; the first occurrence), then out = relu(a z_sel + c). The valid rows of a group are a prefix of it,
// so a group whose first row is a padding row is a padding group: out = +0.0, argsel = 0. A thread owns four channels of a group.
__global__ __launch_bounds__(256) void tl_pool_masked_kernel(long long groups, int ns, int N, const float *__restrict__ z,
                                                             const float *__restrict__ gamma, const float *__restrict__ save,
                                                             const unsigned *__restrict__ mask, float *__restrict__ out,
                                                             int *__restrict__ argsel)
{
    const int n4 = N / 4;
    const long long total = groups * n4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long g = i / n4;
        const int c = (int)(i - g * n4) * 4;
        const float4 a = ld4(save + 2 * N + c), cc = ld4(save + 3 * N + c);
        const bool up[4] = {gamma[c] >= 0.0f, gamma[c + 1] >= 0.0f, gamma[c + 2] >= 0.0f, gamma[c + 3] >= 0.0f};
        const long long row0 = g * ns;
        const float *zr = z + (size_t)row0 * N + c;
        const bool any = (mask[row0 >> 5] >> (unsigned)(row0 & 31)) & 1u;
        const float4 first = ld4(zr);
        float best[4] = {first.x, first.y, first.z, first.w};
        int arg[4] = {0, 0, 0, 0};
#pragma unroll 4
        for (int k = 1; k < ns; ++k) {
            const long long r = row0 + k;
            const bool rv = (mask[r >> 5] >> (unsigned)(r & 31)) & 1u;
            const float4 t = ld4(zr + (size_t)k * N);
            const float v[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool take = rv && (up[j] ? v[j] > best[j] : v[j] < best[j]);
                best[j] = take ? v[j] : best[j];
                arg[j] = take ? k : arg[j];
            }
        }
        float4 o;
        o.x = any ? vmax(__fadd_rn(__fmul_rn(a.x, best[0]), cc.x), 0.0f) : 0.0f;
        o.y = any ? vmax(__fadd_rn(__fmul_rn(a.y, best[1]), cc.y), 0.0f) : 0.0f;
        o.z = any ? vmax(__fadd_rn(__fmul_rn(a.z, best[2]), cc.z), 0.0f) : 0.0f;
        o.w = any ? vmax(__fadd_rn(__fmul_rn(a.w, best[3]), cc.w), 0.0f) : 0.0f;
        *reinterpret_cast<float4 *>(out + g * N + c) = o;
        *reinterpret_cast<int4 *>(argsel + g * N + c) = make_int4(any ? arg[0] : 0, any ? arg[1] : 0, any ? arg[2] : 0, any ? arg[3] : 0);
    }
}

// pooled top layer: gq = grad_out . [out > 0]; sums of dy and dy z over all rows = over the selected entries
__global__ __launch_bounds__(256) void tl_pool_grad_kernel(long long groups, int N, const float *__restrict__ out,
                                                           const float *__restrict__ gout, const float *__restrict__ zsel,
                                                           float *__restrict__ gq, double *__restrict__ stats)
{
    // thread (x = column within a 64-column strip, y = row lane): column sums over a strided set of groups
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int ry = threadIdx.x >> 6;
    double s1 = 0.0, s2 = 0.0;
    if (c < N) {
        // four groups per trip: the three loads of each are independent of the sums, and one group at a time left the loop a
        // chain of memory latencies (36 us for 64 MB at the metric shape)
        const long long gstep = (long long)gridDim.y * 4;
        long long g = (long long)blockIdx.y * 4 + ry;
        for (; g + 3 * gstep < groups; g += 4 * gstep) {
            float o4[4], g4[4], z4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t o = (size_t)(g + u * gstep) * N + c;
                o4[u] = out[o]; g4[u] = gout[o]; z4[u] = zsel[o];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float q = o4[u] > 0.0f ? g4[u] : 0.0f;
                gq[(size_t)(g + u * gstep) * N + c] = q;
                s1 += (double)q;
                s2 += (double)q * (double)z4[u];
            }
        }
        for (; g < groups; g += gstep) {
            const size_t o = (size_t)g * N + c;
            const float q = out[o] > 0.0f ? gout[o] : 0.0f;
            gq[o] = q;
            s1 += (double)q;
            s2 += (double)q * (double)zsel[o];
        }
    }
    __shared__ double sh[2][4][64];
    sh[0][ry][threadIdx.x & 63] = s1;
    sh[1][ry][threadIdx.x & 63] = s2;
    __syncthreads();
    if (stats && ry == 0 && c < N) {                 // (stats == nullptr: a top layer that wants no parameter gradient, frozen statistics)
        const int x = threadIdx.x & 63;
        stats[((size_t)blockIdx.y * 2) * N + c] = sh[0][0][x] + sh[0][1][x] + sh[0][2][x] + sh[0][3][x];
        stats[((size_t)blockIdx.y * 2 + 1) * N + c] = sh[1][0][x] + sh[1][1][x] + sh[1][2][x] + sh[1][3][x];
    }
}

// unpooled top layer (FP levels): out = relu(a z + c)
__global__ __launch_bounds__(256) void tl_apply_kernel(long long total4, int N, const float *__restrict__ z,
                                                       const float *__restrict__ save, float *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int c = (int)((i * 4) % N);
        const float4 zz = ld4(z + i * 4), a = ld4(save + 2 * N + c), cc = ld4(save + 3 * N + c);
        float4 o;
        o.x = vmax(__fadd_rn(__fmul_rn(a.x, zz.x), cc.x), 0.0f);
        o.y = vmax(__fadd_rn(__fmul_rn(a.y, zz.y), cc.y), 0.0f);
        o.z = vmax(__fadd_rn(__fmul_rn(a.z, zz.z), cc.z), 0.0f);
        o.w = vmax(__fadd_rn(__fmul_rn(a.w, zz.w), cc.w), 0.0f);
        *reinterpret_cast<float4 *>(out + i * 4) = o;
    }
}

// ... on the rows of a ragged batch (train_mlp_ragged.hip): out = relu(a z + c) on the valid rows, exactly 0 on the others
__global__ __launch_bounds__(256) void tl_apply_masked_kernel(long long total4, int N, const float *__restrict__ z,
                                                              const float *__restrict__ save, const unsigned *__restrict__ mask,
                                                              float *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const long long row = (i * 4) / N;
        const int c = (int)(i * 4 - row * N);
        const bool rv = (mask[row >> 5] >> (unsigned)(row & 31)) & 1u;
        const float4 zz = ld4(z + i * 4), a = ld4(save + 2 * N + c), cc = ld4(save + 3 * N + c);
        float4 o;
        o.x = rv ? vmax(__fadd_rn(__fmul_rn(a.x, zz.x), cc.x), 0.0f) : 0.0f;
        o.y = rv ? vmax(__fadd_rn(__fmul_rn(a.y, zz.y), cc.y), 0.0f) : 0.0f;
        o.z = rv ? vmax(__fadd_rn(__fmul_rn(a.z, zz.z), cc.z), 0.0f) : 0.0f;
        o.w = rv ? vmax(__fadd_rn(__fmul_rn(a.w, zz.w), cc.w), 0.0f) : 0.0f;
        *reinterpret_cast<float4 *>(out + i * 4) = o;
    }
}

// unpooled top layer backward: dy = grad_out . [out > 0] (rows, N) + its two column sums
__global__ __launch_bounds__(256) void tl_top_grad_kernel(long long rows, int N, const float *__restrict__ out,
                                                          const float *__restrict__ gout, const float *__restrict__ z,
                                                          float *__restrict__ dy, double *__restrict__ stats)
{
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int ry = threadIdx.x >> 6;
    double s1 = 0.0, s2 = 0.0;
    if (c < N) {
        // four rows per trip (independent loads in flight; one row at a time was a chain of memory latencies, as in
        // tl_pool_grad_kernel): the sums keep their order
        const long long rstep = (long long)gridDim.y * 4;
        long long r = (long long)blockIdx.y * 4 + ry;
        for (; r + 3 * rstep < rows; r += 4 * rstep) {
            float o4[4], g4[4], z4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t o = (size_t)(r + u * rstep) * N + c;
                o4[u] = out[o]; g4[u] = gout[o]; z4[u] = z[o];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float q = o4[u] > 0.0f ? g4[u] : 0.0f;
                dy[(size_t)(r + u * rstep) * N + c] = q;
                s1 += (double)q;
                s2 += (double)q * (double)z4[u];
            }
        }
        for (; r < rows; r += rstep) {
            const size_t o = (size_t)r * N + c;
            const float q = out[o] > 0.0f ? gout[o] : 0.0f;
            dy[o] = q;
            s1 += (double)q;
            s2 += (double)q * (double)z[o];
        }
    }
    __shared__ double sh[2][4][64];
    sh[0][ry][threadIdx.x & 63] = s1;
    sh[1][ry][threadIdx.x & 63] = s2;
    __syncthreads();
    if (stats && ry == 0 && c < N) {                 // (stats == nullptr: a top layer that wants no parameter gradient, frozen statistics)
        const int x = threadIdx.x & 63;
        stats[((size_t)blockIdx.y * 2) * N + c] = sh[0][0][x] + sh[0][1][x] + sh[0][2][x] + sh[0][3][x];
        stats[((size_t)blockIdx.y * 2 + 1) * N + c] = sh[1][0][x] + sh[1][1][x] + sh[1][2][x] + sh[1][3][x];
    }
}

// ---- pooled averages (pooling 1 avg, 2 weighted_avg, 3 max_and_avg; utils/pointnet_util.py:128-142) ----------------------
// A mean does not commute with batch norm + ReLU the way a max does, so these modes keep z_L (the unpooled top layer of the FP
// levels) and reduce each group after the layer's moments are final: out[g, c] = sum_k w_gk relu(a_c z_L[g ns + k, c] + c_c).
// Padded ball-query slots (duplicates of the first hit) count, as in the reference's reduce_mean over nsample.

// weighted_avg weights, one wave per group: w = exp(-5 |xyz[idx] - new_xyz|) / (sum over the group) (:132-138; the fp32 formula
// of sa_mlp.hip); group_all (new_xyz NULL): |xyz|. The wave's butterfly sum has a fixed order and gives every lane the same bits.
__global__ __launch_bounds__(256) void tl_pool_weights_kernel(long long groups, int ns, int n, int m, const float *__restrict__ xyz,
                                                              const float *__restrict__ new_xyz, const int *__restrict__ idx,
                                                              float *__restrict__ w)
{
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= groups) return;
    const long long cloud = g / m;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (new_xyz) { cx = new_xyz[g * 3]; cy = new_xyz[g * 3 + 1]; cz = new_xyz[g * 3 + 2]; }
    float s = 0.0f;
    for (int k = lane; k < ns; k += 64) {
        const long long r = g * ns + k;
        const int pt = idx ? idx[r] : k;
        const float *p = xyz + (cloud * n + pt) * 3;
        const float dx = __fsub_rn(p[0], cx), dy = __fsub_rn(p[1], cy), dz = __fsub_rn(p[2], cz);
        const float e = expf(-5.0f * sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz))));
        w[r] = e;
        s = __fadd_rn(s, e);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o));
    for (int k = lane; k < ns; k += 64) w[g * ns + k] = w[g * ns + k] / s;
}

// out[g, c] (pitch N, or 2 N with the max half `maxv` behind it: max_and_avg) = sum_k w relu(a z + c); w = pool_w, or 1 / ns
__global__ __launch_bounds__(256) void tl_pool_avg_kernel(long long groups, int ns, int N, const float *__restrict__ z,
                                                          const float *__restrict__ save, const float *__restrict__ pool_w,
                                                          const float *__restrict__ maxv, float *__restrict__ out)
{
    const int n4 = N / 4, opitch = maxv ? 2 * N : N;
    const long long total = groups * n4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long g = i / n4;
        const int c = (int)(i - g * n4) * 4;
        const float4 a = ld4(save + 2 * N + c), cc = ld4(save + 3 * N + c);
        const float *zr = z + (size_t)g * ns * N + c;
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 4
        for (int k = 0; k < ns; ++k) {
            const float4 v = ld4(zr + (size_t)k * N);
            float4 h;
            h.x = vmax(__fadd_rn(__fmul_rn(a.x, v.x), cc.x), 0.0f);
            h.y = vmax(__fadd_rn(__fmul_rn(a.y, v.y), cc.y), 0.0f);
            h.z = vmax(__fadd_rn(__fmul_rn(a.z, v.z), cc.z), 0.0f);
            h.w = vmax(__fadd_rn(__fmul_rn(a.w, v.w), cc.w), 0.0f);
            if (pool_w) {
                const float wk = pool_w[g * ns + k];
                h.x = __fmul_rn(wk, h.x); h.y = __fmul_rn(wk, h.y); h.z = __fmul_rn(wk, h.z); h.w = __fmul_rn(wk, h.w);
            }
            s.x = __fadd_rn(s.x, h.x); s.y = __fadd_rn(s.y, h.y); s.z = __fadd_rn(s.z, h.z); s.w = __fadd_rn(s.w, h.w);
        }
        if (!pool_w) {
            const float fn = (float)ns;
            s.x = s.x / fn; s.y = s.y / fn; s.z = s.z / fn; s.w = s.w / fn;
        }
        *reinterpret_cast<float4 *>(out + g * opitch + c) = s;
        if (maxv) *reinterpret_cast<float4 *>(out + g * opitch + N + c) = ld4(maxv + g * N + c);
    }
}

// the averaged top layer's dense gradient (the pooled counterpart of tl_top_grad_kernel, same grid, same `stats` layout):
// dy[row, c] = [a z + c > 0] (w_row g_avg[g, c] + [k == argsel[g, c]] g_max[g, c]); g_max / argsel only with max_and_avg.
// A thread owns four channels (16-byte accesses) and a block 16 rows at a time: with tl_top_grad_kernel's 64 x 4 shape the
// pass kept too few bytes in flight (576 us for 2 x 512 MB at the metric shape).
__device__ __forceinline__ float4 tl_pool_dy4(long long r, int c, int ns, int N, float inv_ns, const float *gout, float4 zz,
                                              float4 a, float4 cc, const float *pool_w, const int *argsel)
{
    const unsigned g = (unsigned)r / (unsigned)ns, k = (unsigned)r - g * (unsigned)ns;
    const size_t go = (size_t)g * (argsel ? 2 * N : N) + c;
    const float w = pool_w ? pool_w[r] : inv_ns;
    const float4 ga = ld4(gout + go);
    float4 q = make_float4(__fmul_rn(w, ga.x), __fmul_rn(w, ga.y), __fmul_rn(w, ga.z), __fmul_rn(w, ga.w));
    if (argsel) {
        const int4 s = *reinterpret_cast<const int4 *>(argsel + (size_t)g * N + c);
        const float4 gm = ld4(gout + go + N);
        if ((unsigned)s.x == k) q.x = __fadd_rn(q.x, gm.x);
        if ((unsigned)s.y == k) q.y = __fadd_rn(q.y, gm.y);
        if ((unsigned)s.z == k) q.z = __fadd_rn(q.z, gm.z);
        if ((unsigned)s.w == k) q.w = __fadd_rn(q.w, gm.w);
    }
    q.x = __fadd_rn(__fmul_rn(a.x, zz.x), cc.x) > 0.0f ? q.x : 0.0f;
    q.y = __fadd_rn(__fmul_rn(a.y, zz.y), cc.y) > 0.0f ? q.y : 0.0f;
    q.z = __fadd_rn(__fmul_rn(a.z, zz.z), cc.z) > 0.0f ? q.z : 0.0f;
    q.w = __fadd_rn(__fmul_rn(a.w, zz.w), cc.w) > 0.0f ? q.w : 0.0f;
    return q;
}

__device__ __forceinline__ void tl_pool_acc(double *s1, double *s2, float4 q, float4 z)
{
    s1[0] += (double)q.x; s1[1] += (double)q.y; s1[2] += (double)q.z; s1[3] += (double)q.w;
    s2[0] += (double)q.x * (double)z.x; s2[1] += (double)q.y * (double)z.y;
    s2[2] += (double)q.z * (double)z.z; s2[3] += (double)q.w * (double)z.w;
}

// block (16 four-channel lanes x 16 row lanes) = 64 channels; grid (N / 64 rounded up, row parts <= kMaxParts)
__global__ __launch_bounds__(256) void tl_pool_top_grad_kernel(long long rows, int ns, int N, const float *__restrict__ gout,
                                                               const float *__restrict__ z, const float *__restrict__ save,
                                                               const float *__restrict__ pool_w, const int *__restrict__ argsel,
                                                               float *__restrict__ dy, double *__restrict__ stats)
{
    const int c = (blockIdx.x * 16 + (threadIdx.x & 15)) * 4;
    const int ry = threadIdx.x >> 4;
    const float inv_ns = 1.0f / (float)ns;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (c < N) {
        const float4 a = ld4(save + 2 * N + c), cc = ld4(save + 3 * N + c);
        const long long rstep = (long long)gridDim.y * 16;
        long long r = (long long)blockIdx.y * 16 + ry;
        for (; r + 3 * rstep < rows; r += 4 * rstep) {               // four rows per trip, the sums in row order
            float4 z4[4], q4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) z4[u] = ld4(z + (size_t)(r + u * rstep) * N + c);
#pragma unroll
            for (int u = 0; u < 4; ++u) q4[u] = tl_pool_dy4(r + u * rstep, c, ns, N, inv_ns, gout, z4[u], a, cc, pool_w, argsel);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                *reinterpret_cast<float4 *>(dy + (size_t)(r + u * rstep) * N + c) = q4[u];
                tl_pool_acc(s1, s2, q4[u], z4[u]);
            }
        }
        for (; r < rows; r += rstep) {
            const float4 zz = ld4(z + (size_t)r * N + c);
            const float4 q = tl_pool_dy4(r, c, ns, N, inv_ns, gout, zz, a, cc, pool_w, argsel);
            *reinterpret_cast<float4 *>(dy + (size_t)r * N + c) = q;
            tl_pool_acc(s1, s2, q, zz);
        }
    }
    __shared__ double sh[2][16][64];
    const int x0 = (threadIdx.x & 15) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) { sh[0][ry][x0 + j] = s1[j]; sh[1][ry][x0 + j] = s2[j]; }
    __syncthreads();
    const int x = threadIdx.x, col = blockIdx.x * 64 + x;
    if (stats && x < 64 && col < N) {
        double t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) { t1 += sh[0][i][x]; t2 += sh[1][i][x]; }
        stats[((size_t)blockIdx.y * 2) * N + col] = t1;
        stats[((size_t)blockIdx.y * 2 + 1) * N + col] = t2;
    }
}

// ... of the max pool over the valid rows of a ragged batch's grouped rows (tl_pool_masked_kernel; same grid, same `stats`
// layout): the DENSE dy_L[row, c] = (row valid && k == argsel[g, c] && out[g, c] > 0) ? grad_out[g, c] : +0.0 -- selects: the
// grad_out rows of padding groups may hold anything -- and its two column sums. From here on the stack is an unpooled one.
__global__ __launch_bounds__(256) void tl_pool_top_grad_masked_kernel(long long rows, int ns, int N, const float *__restrict__ out,
                                                                      const float *__restrict__ gout, const int *__restrict__ argsel,
                                                                      const unsigned *__restrict__ mask, const float *__restrict__ z,
                                                                      float *__restrict__ dy, double *__restrict__ stats)
{
    const int c = (blockIdx.x * 16 + (threadIdx.x & 15)) * 4;
    const int ry = threadIdx.x >> 4;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (c < N) {
        const long long rstep = (long long)gridDim.y * 16;
#pragma unroll 2
        for (long long r = (long long)blockIdx.y * 16 + ry; r < rows; r += rstep) {
            const unsigned g = (unsigned)r / (unsigned)ns, k = (unsigned)r - g * (unsigned)ns;
            const bool rv = (mask[r >> 5] >> (unsigned)(r & 31)) & 1u;
            const size_t go = (size_t)g * N + c;
            const float4 o = ld4(out + go), ga = ld4(gout + go), zz = ld4(z + (size_t)r * N + c);
            const int4 s = *reinterpret_cast<const int4 *>(argsel + go);
            const bool on[4] = {rv && (unsigned)s.x == k && o.x > 0.0f, rv && (unsigned)s.y == k && o.y > 0.0f,
                                rv && (unsigned)s.z == k && o.z > 0.0f, rv && (unsigned)s.w == k && o.w > 0.0f};
            const float4 q = make_float4(on[0] ? ga.x : 0.0f, on[1] ? ga.y : 0.0f, on[2] ? ga.z : 0.0f, on[3] ? ga.w : 0.0f);
            *reinterpret_cast<float4 *>(dy + (size_t)r * N + c) = q;
            const float zv[4] = {zz.x, zz.y, zz.z, zz.w}, qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s1[j] += (double)qv[j];
                s2[j] += on[j] ? (double)qv[j] * (double)zv[j] : 0.0;
            }
        }
    }
    __shared__ double sh[2][16][64];
    const int x0 = (threadIdx.x & 15) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) { sh[0][ry][x0 + j] = s1[j]; sh[1][ry][x0 + j] = s2[j]; }
    __syncthreads();
    const int x = threadIdx.x, col = blockIdx.x * 64 + x;
    if (stats && x < 64 && col < N) {
        double t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) { t1 += sh[0][i][x]; t2 += sh[1][i][x]; }
        stats[((size_t)blockIdx.y * 2) * N + col] = t1;
        stats[((size_t)blockIdx.y * 2 + 1) * N + col] = t2;
    }
}

__global__ void tl_identity_coef_kernel(int C, float *__restrict__ coef)       // dz = 1 * g - 0 - 0 * z
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * C) coef[i] = i < C ? 1.0f : 0.0f;
}

// ---- launches (parts: rows of the kernel's partial-sum array = gridDim.y, the caller's choice) ----
// count: the row count on the device (ragged rows: the number of valid rows), or nullptr: `rows`
int launch_bn_finalize(const double *stats, int nparts, int N, double rows, const double *count, const float *gamma, const float *beta,
                       float *running_mean, float *running_var, float momentum, float eps, float *save, const float *bias,
                       int var_biased, hipStream_t st)
{
    const dim3 grid((unsigned)((N + 7) / 8));
    if (count)
        return launch(tl_bn_finalize_counted_kernel, grid, dim3(256), 0, st, stats, nparts, N, count, gamma, beta, running_mean,
                      running_var, momentum, eps, save, bias, var_biased);
    return launch(tl_bn_finalize_kernel, grid, dim3(256), 0, st, stats, nparts, N, rows, gamma, beta, running_mean, running_var,
                  momentum, eps, save, bias, var_biased);
}

int launch_bn_backward_finalize(const double *stats, int nparts, int N, double rows, const double *count, const float *gamma,
                                const float *save, float *grad_gamma, float *grad_beta, float *coef, int accumulate, hipStream_t st)
{
    const dim3 grid((unsigned)((N + 7) / 8));
    if (count)
        return launch(tl_bn_backward_finalize_counted_kernel, grid, dim3(256), 0, st, stats, nparts, N, count, gamma, save, grad_gamma,
                      grad_beta, coef, accumulate);
    return launch(tl_bn_backward_finalize_kernel, grid, dim3(256), 0, st, stats, nparts, N, rows, gamma, save, grad_gamma, grad_beta,
                  coef, accumulate);
}

int launch_pool_finalize(long long groups, int N, int parts, int prow, const float *pmax, const int *pamax, const float *gamma,
                         const float *save, float *out, int *argsel, float *zsel, hipStream_t st)
{
    long long blocks = (groups * N + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    return launch(tl_pool_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, st, groups, N, parts, prow, pmax, pamax, gamma, save, out,
                  argsel, zsel);
}

int launch_pool_grad(long long groups, int N, const float *out, const float *gout, const float *zsel, float *gq, double *stats,
                     int parts, hipStream_t st)
{
    return launch(tl_pool_grad_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)parts), dim3(256), 0, st, groups, N, out, gout, zsel, gq,
                  stats);
}

// mask: the validity words of ragged rows, or nullptr: every row is valid
int launch_apply(long long total4, int N, const float *z, const float *save, const unsigned *mask, float *out, hipStream_t st)
{
    long long blocks = (total4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (mask) return launch(tl_apply_masked_kernel, dim3((unsigned)blocks), dim3(256), 0, st, total4, N, z, save, mask, out);
    return launch(tl_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, st, total4, N, z, save, out);
}

int launch_top_grad(long long rows, int N, const float *out, const float *gout, const float *z, float *dy, double *stats, int parts,
                    hipStream_t st)
{
    return launch(tl_top_grad_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)parts), dim3(256), 0, st, rows, N, out, gout, z, dy, stats);
}

int launch_pool_weights(long long groups, int ns, int n, int m, const float *xyz, const float *new_xyz, const int *idx, float *w,
                        hipStream_t st)
{
    return launch(tl_pool_weights_kernel, dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, st, groups, ns, n, m, xyz, new_xyz, idx, w);
}

int launch_pool_avg(long long groups, int ns, int N, const float *z, const float *save, const float *pool_w, const float *maxv,
                    float *out, hipStream_t st)
{
    long long blocks = (groups * (N / 4) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    return launch(tl_pool_avg_kernel, dim3((unsigned)blocks), dim3(256), 0, st, groups, ns, N, z, save, pool_w, maxv, out);
}

int launch_pool_top_grad(long long rows, int ns, int N, const float *gout, const float *z, const float *save, const float *pool_w,
                         const int *argsel, float *dy, double *stats, int parts, hipStream_t st)
{
    return launch(tl_pool_top_grad_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)parts), dim3(256), 0, st, rows, ns, N, gout, z, save,
                  pool_w, argsel, dy, stats);
}

int launch_pool_masked(long long groups, int ns, int N, const float *z, const float *gamma, const float *save, const unsigned *mask,
                       float *out, int *argsel, hipStream_t st)
{
    long long blocks = (groups * (N / 4) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    return launch(tl_pool_masked_kernel, dim3((unsigned)blocks), dim3(256), 0, st, groups, ns, N, z, gamma, save, mask, out, argsel);
}

int launch_pool_top_grad_masked(long long rows, int ns, int N, const float *out, const float *gout, const int *argsel,
                                const unsigned *mask, const float *z, float *dy, double *stats, int parts, hipStream_t st)
{
    return launch(tl_pool_top_grad_masked_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)parts), dim3(256), 0, st, rows, ns, N, out,
                  gout, argsel, mask, z, dy, stats);
}

int launch_identity_coef(int C, float *coef, hipStream_t st)
{
    return launch(tl_identity_coef_kernel, dim3((unsigned)((3 * C + 127) / 128)), dim3(128), 0, st, C, coef);
}

}  // namespace pn2
