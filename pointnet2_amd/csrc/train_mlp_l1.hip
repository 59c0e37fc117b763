// train_mlp_l1.hip -- layer 1 of a grouped level of the training node on the vector units: once per point, or from the three
// centred coordinates alone; the kernels and their launches. gfx950.
#include "train_mlp_device.h"

#include <string.h>

namespace pn2 {

// ---- layer 1 of a grouped level ONCE PER POINT -----------------------------------------------------------------------------
// Layer 1 reads [xyz_j - c, f_j] (utils/pointnet_util.py:44-50): z_1 = W1f^T f_j + W1x^T (xyz_j - c) + b. The feature term
// depends on the POINT only, and a point is a sample of nsample m / n (16-64) groups: P = points . W1f is one GEMM over the
// b n points (the generic kernel, plain rows), and the pass over the b m nsample rows only gathers a row of P (cout_1 floats
// where the features were up to 320) and adds the three coordinate terms -- no matrix pipe needed for K = 3. Backward:
//     dW1x = (xyz - c)^T dz_1 and dz_1 itself      one pass over the rows (tl_l1_dz_kernel; dz_1 overwrites dy_1)
//     S    = scatter-add of dz_1 onto the points   pn2_group_point_grad_seg (the level's ordinary segmented reduction)
//     dW1f = points^T S,   dPoints = S W1f^T       two GEMMs over the b n points
// instead of a weight-gradient and a data-gradient GEMM over all rows with the gathered 131-323 channel input, and a
// segmented reduction of a (rows, cfeat) tensor. (The inference kernels do the same: csrc/sa_mlp_stream.hip.)
// (the arguments: TlL1, train_mlp_kernels.h)

// thread <-> (row lane, 4 columns): a block of kL1Threads covers kL1Threads / (C / 4) rows at a time, columns fixed per
// thread, and every thread keeps kL1U rows in flight (all loads of a batch are issued before the first is used: the
// point number -> coordinates / row of P chain is two dependent latencies, one row at a time ran at 1-2 TB/s).
// P == nullptr: a level WITHOUT features (the first level of every network): z_1 = b + (xyz - c) W1 on the vector units,
// three multiply-adds per output -- the generic gathered GEMM spent a matrix-core pass on a contraction of three.
// (kL1Threads = 512, kL1U = 4: train_mlp_kernels.h)

struct L1Rows {                                   // the batch's rows: number, point, group (clamped to a valid row when !ok)
    unsigned row[kL1U];
    size_t pt[kL1U];                              // cloud * n + point
    unsigned grp[kL1U];
    bool ok[kL1U];
};

__device__ __forceinline__ L1Rows l1_rows(const TlL1 &p, unsigned base, unsigned stride, unsigned rows)
{
    L1Rows r;
#pragma unroll
    for (int u = 0; u < kL1U; ++u) {
        const unsigned rr = base + (unsigned)u * stride;
        r.ok[u] = rr < rows;
        r.row[u] = r.ok[u] ? rr : base;
        r.grp[u] = r.row[u] / (unsigned)p.nsample;
    }
#pragma unroll
    for (int u = 0; u < kL1U; ++u) r.pt[u] = (size_t)(r.grp[u] / (unsigned)p.m) * p.n + p.idx[r.row[u]];
    return r;
}

__device__ __forceinline__ void l1_coords(const TlL1 &p, const L1Rows &r, float (&x)[kL1U][3])
{
#pragma unroll
    for (int u = 0; u < kL1U; ++u) {
        const float *px = p.xyz + r.pt[u] * 3;
        x[u][0] = px[0]; x[u][1] = px[1]; x[u][2] = px[2];
    }
    if (p.new_xyz) {
#pragma unroll
        for (int u = 0; u < kL1U; ++u) {
            const float *pc = p.new_xyz + (size_t)r.grp[u] * 3;
            const float c0 = pc[0], c1 = pc[1], c2 = pc[2];
            x[u][0] = __fsub_rn(x[u][0], c0); x[u][1] = __fsub_rn(x[u][1], c1); x[u][2] = __fsub_rn(x[u][2], c2);   // pointnet_util.py:46
        }
    }
}

__global__ __launch_bounds__(kL1Threads) void tl_l1_forward_kernel(const TlL1 p)
{
    const int qpr = p.C / 4, q = threadIdx.x % qpr, rl = threadIdx.x / qpr, rpb = kL1Threads / qpr, col = 4 * q;
    float a0[4], a1[4], a2[4], b4[4] = {0.f, 0.f, 0.f, 0.f};
    {
        const float *w = p.wx + (size_t)col * p.sn;
#pragma unroll
        for (int i = 0; i < 4; ++i) { a0[i] = w[i * p.sn]; a1[i] = w[p.skx + i * p.sn]; a2[i] = w[2 * p.skx + i * p.sn]; }
        if (p.bias) { const float4 b = ld4(p.bias + col); b4[0] = b.x; b4[1] = b.y; b4[2] = b.z; b4[3] = b.w; }
    }
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    // a workgroup walks ONE contiguous range of rows, a batch = kL1U consecutive slices of rpb rows (whole 32 KB runs of z)
    const unsigned rows = (unsigned)p.rows, stride = (unsigned)rpb, span = kL1U * stride;
    const unsigned chunk = (rows + gridDim.x * span - 1) / (gridDim.x * span) * span;
    const unsigned first = blockIdx.x * chunk, stop = first + chunk < rows ? first + chunk : rows;
    for (unsigned base = first + rl; base < stop; base += span) {
        const L1Rows r = l1_rows(p, base, stride, rows);
        float x[kL1U][3];
        float4 pp[kL1U];
        l1_coords(p, r, x);
#pragma unroll
        for (int u = 0; u < kL1U; ++u) pp[u] = p.P ? ld4(p.P + r.pt[u] * p.C + col) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < kL1U; ++u) {
            float z[4] = {pp[u].x + b4[0], pp[u].y + b4[1], pp[u].z + b4[2], pp[u].w + b4[3]};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                z[i] = fmaf(x[u][0], a0[i], z[i]);
                z[i] = fmaf(x[u][1], a1[i], z[i]);
                z[i] = fmaf(x[u][2], a2[i], z[i]);
            }

            if (r.ok[u]) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { s1[i] += z[i]; s2[i] = fmaf(z[i], z[i], s2[i]); }
                typedef float v4f __attribute__((ext_vector_type(4)));
                const v4f zo = {z[0], z[1], z[2], z[3]};
                __builtin_nontemporal_store(zo, reinterpret_cast<v4f *>(p.z + (size_t)r.row[u] * p.C + col));
            }
        }
    }
    if (!p.stats) return;                       // frozen statistics (train_mlp_frozen.hip): nobody reads the batch moments
    __shared__ double red[2][kL1Threads][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { red[0][threadIdx.x][i] = (double)s1[i]; red[1][threadIdx.x][i] = (double)s2[i]; }
    __syncthreads();
    if (rl == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double a = 0.0, b = 0.0;
            for (int k = 0; k < rpb; ++k) { a += red[0][k * qpr + q][i]; b += red[1][k * qpr + q][i]; }
            p.stats[((size_t)blockIdx.x * 2) * p.C + col + i] = a;
            p.stats[((size_t)blockIdx.x * 2 + 1) * p.C + col + i] = b;
        }
    }
}

// dz_1 = s dy_1 - c0 - c1 z_1 and the coordinate rows of the weight gradient, dW1x = (xyz - c)^T dz_1, in one pass over the
// rows. STORE: dz_1 overwrites dy_1 (the per-point path scatters it onto the points next); a level without features needs
// only dW1x = its whole first-layer weight gradient.
template <bool STORE, bool FEAT>
__global__ __launch_bounds__(kL1Threads) void tl_l1_dz_kernel(const TlL1 p)
{
    constexpr int NIN = FEAT ? 3 + kL1MaxFeat : 3;               // rows of the weight gradient a thread accumulates
    const int qpr = p.C / 4, q = threadIdx.x % qpr, rl = threadIdx.x / qpr, rpb = kL1Threads / qpr, col = 4 * q;
    const int nin = FEAT ? 3 + p.cf : 3;
    const float4 s4 = ld4(p.coef + col), c04 = ld4(p.coef + p.C + col), c14 = ld4(p.coef + 2 * p.C + col);
    const float s[4] = {s4.x, s4.y, s4.z, s4.w}, c0[4] = {c04.x, c04.y, c04.z, c04.w}, c1[4] = {c14.x, c14.y, c14.z, c14.w};
    float acc[NIN][4];
#pragma unroll
    for (int k = 0; k < NIN; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[k][i] = 0.0f;
    // a workgroup walks ONE contiguous range of rows, a batch = kL1U consecutive slices of rpb rows (whole 32 KB runs of z)
    const unsigned rows = (unsigned)p.rows, stride = (unsigned)rpb, span = kL1U * stride;
    const unsigned chunk = (rows + gridDim.x * span - 1) / (gridDim.x * span) * span;
    const unsigned first = blockIdx.x * chunk, stop = first + chunk < rows ? first + chunk : rows;
    for (unsigned base = first + rl; base < stop; base += span) {
        const L1Rows r = l1_rows(p, base, stride, rows);
        float x[kL1U][NIN];
        float4 g4[kL1U], z4[kL1U];
#pragma unroll
        for (int u = 0; u < kL1U; ++u) {
            const size_t o = (size_t)r.row[u] * p.C + col;
            g4[u] = ld4(p.g + o);
            z4[u] = ld4(p.z + o);
        }
        {
            float xc[kL1U][3];
            l1_coords(p, r, xc);
#pragma unroll
            for (int u = 0; u < kL1U; ++u) {
                x[u][0] = xc[u][0]; x[u][1] = xc[u][1]; x[u][2] = xc[u][2];
                if (FEAT) {
#pragma unroll
                    for (int k = 0; k < kL1MaxFeat; ++k) x[u][3 + k] = k < p.cf ? p.points[r.pt[u] * p.cf + k] : 0.0f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kL1U; ++u) {
            const float gg[4] = {g4[u].x, g4[u].y, g4[u].z, g4[u].w}, zz[4] = {z4[u].x, z4[u].y, z4[u].z, z4[u].w};
            float dz[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dz[i] = __fsub_rn(__fsub_rn(__fmul_rn(s[i], gg[i]), c0[i]), __fmul_rn(c1[i], zz[i]));      // s dy - c0 - c1 z
                const float dv = r.ok[u] ? dz[i] : 0.0f;
#pragma unroll
                for (int k = 0; k < NIN; ++k) acc[k][i] = fmaf(x[u][k], dv, acc[k][i]);
            }
            if (STORE && r.ok[u])
                *reinterpret_cast<float4 *>(p.g + (size_t)r.row[u] * p.C + col) = make_float4(dz[0], dz[1], dz[2], dz[3]);
        }
    }
    __shared__ float red[3][kL1Threads][4];
#pragma unroll
    for (int k0 = 0; k0 < NIN; k0 += 3) {                          // three gradient rows per trip through the 24 KB buffer
        if (k0) __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) red[k][threadIdx.x][i] = k0 + k < NIN ? acc[k0 + k < NIN ? k0 + k : 0][i] : 0.0f;
        __syncthreads();
        if (rl == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (k0 + k < nin) {
                        double a = 0.0;
                        for (int j = 0; j < rpb; ++j) a += (double)red[k][j * qpr + q][i];
                        p.part[((size_t)blockIdx.x * nin + k0 + k) * p.C + col + i] = (float)a;
                    }
                }
        }
    }
}

// dW1x[k][col] = sum over the workgroups' partials (fp64), written to rows [xyz_off, xyz_off + 3) of grad_weight.
// A block of 256 threads owns 8 of the 3 C sums and adds the partial rows 32 at a time (a thread per sum walking all
// 256 rows was 60 us of dependent L2 latencies).
// (nin = 3 + cf rows: the coordinate rows go to gw, the feature rows to gwf -- the two blocks of the layer's weight gradient)
__global__ __launch_bounds__(256) void tl_l1_wx_reduce_kernel(const float *__restrict__ part, int nparts, int C, int nin,
                                                              float *__restrict__ gw, float *__restrict__ gwf,
                                                              long long sk, long long sn, int accumulate)
{
    __shared__ double sh[32][8];
    const int g = threadIdx.x >> 3, cl = threadIdx.x & 7, i = blockIdx.x * 8 + cl;
    double a = 0.0;
    if (i < nin * C)
        for (int q = g; q < nparts; q += 32) a += (double)part[(size_t)q * nin * C + i];
    sh[g][cl] = a;
    __syncthreads();
    if (g != 0 || i >= nin * C) return;
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < 32; ++r) sum += sh[r][cl];
    const int k = i / C, col = i - k * C;
    float *dst = k < 3 ? gw + k * sk + col * sn : gwf + (k - 3) * sk + col * sn;
    *dst = accumulate ? __fadd_rn(*dst, (float)sum) : (float)sum;
}

// ---- layer 1 of a level without features, weight gradient from moments (TlWgrad::l1x) ----------------------------------------
// the centred coordinates of every row as (x, y, z, 0) -- the layer above's one-pass backward reads them 16 bytes per row
// instead of gathering through idx -- and the nine moments sum x, sum x x^T of this workgroup's rows (fp64)
constexpr int kL1XrowsThreads = 1024;
__global__ __launch_bounds__(kL1XrowsThreads) void tl_l1_xrows_kernel(const TlL1 p, float4 *__restrict__ xg, double *__restrict__ mom)
{
    // (last session of round 6. The launch is at most 256 workgroups -- one partial row of moments each, summed in fp64 by the
    // consumer; with 256 threads a thread walked 16 rows one at a time, a chain of idx -> coordinates round trips, and nine
    // threads then added 256 LDS values each, serially: 20.8 us at the metric shape. Now 1024 threads, four rows in flight per
    // thread -- one trip at the metric shape -- and the workgroup's sums meet through a shuffle tree + one sum per wave, a fixed order.)
    double s[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i] = 0.0;
    const unsigned rows = (unsigned)p.rows, stride = gridDim.x * (unsigned)kL1XrowsThreads;
    auto row_in = [&](unsigned r, float (&x)[3], float (&c)[3]) __attribute__((always_inline)) {
        const unsigned grp = r / (unsigned)p.nsample;
        const size_t pt = (size_t)(grp / (unsigned)p.m) * p.n + p.idx[r];
        const float *px = p.xyz + pt * 3;
        x[0] = px[0]; x[1] = px[1]; x[2] = px[2];
        c[0] = c[1] = c[2] = 0.0f;
        if (p.new_xyz) {
            const float *pc = p.new_xyz + (size_t)grp * 3;
            c[0] = pc[0]; c[1] = pc[1]; c[2] = pc[2];
        }
    };
    auto row_out = [&](unsigned r, const float (&x)[3], const float (&c)[3]) __attribute__((always_inline)) {
        float x0 = x[0], x1 = x[1], x2 = x[2];
        if (p.new_xyz) { x0 = __fsub_rn(x0, c[0]); x1 = __fsub_rn(x1, c[1]); x2 = __fsub_rn(x2, c[2]); }      // pointnet_util.py:46
        xg[r] = make_float4(x0, x1, x2, 0.0f);
        const double d0 = x0, d1 = x1, d2 = x2;
        s[0] += d0; s[1] += d1; s[2] += d2;
        s[3] += d0 * d0; s[4] += d0 * d1; s[5] += d0 * d2; s[6] += d1 * d1; s[7] += d1 * d2; s[8] += d2 * d2;
    };
    unsigned r = blockIdx.x * (unsigned)kL1XrowsThreads + threadIdx.x;
    for (; (unsigned long long)r + 3ull * stride < rows; r += 4u * stride) {
        float x[4][3], c[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) row_in(r + u * stride, x[u], c[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) row_out(r + u * stride, x[u], c[u]);
    }
    for (; r < rows; r += stride) {
        float x[3], c[3];
        row_in(r, x, c);
        row_out(r, x, c);
    }
    __shared__ double red[kL1XrowsThreads / 64][9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        double v = s[i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < kL1XrowsThreads / 64; ++w) a += red[w][threadIdx.x];
        mom[(size_t)blockIdx.x * 9 + threadIdx.x] = a;
    }
}

// dW_1[k][c] = s_c A[k][c] - c0_c (sum x_k) - c1_c ((sum x x^T) W_1)[k][c] in fp64. A block of 256 threads owns 8 of the 3 C
// entries and adds the partial rows 32 at a time, in a fixed order (a thread per entry walking 256 rows was 160 us of
// dependent L2 latencies); every block sums the nine moments itself the same way.
__global__ __launch_bounds__(256) void tl_l1_wx_combine_kernel(const double *__restrict__ mom, int nmom, const double *__restrict__ l1a,
                                                               int nparts, int C, int pitch, const float *__restrict__ coef,
                                                               const float *__restrict__ wx, long long skx, long long sn,
                                                               float *__restrict__ gw, int accumulate)
{
    __shared__ double sh[32][9];
    __shared__ double m9[9];
    const int g = threadIdx.x >> 3, cl = threadIdx.x & 7;
    // moments: thread (g, j) for j < 9 (cl + 8 * (g & 1) covers 0..15) -- simpler: 32 groups x 9 values via two passes
    for (int j = cl; j < 9; j += 8) {
        double a = 0.0;
        for (int q = g; q < nmom; q += 32) a += mom[(size_t)q * 9 + j];
        sh[g][j] = a;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        double a = 0.0;
#pragma unroll
        for (int r = 0; r < 32; ++r) a += sh[r][threadIdx.x];
        m9[threadIdx.x] = a;
    }
    __syncthreads();
    const int i = blockIdx.x * 8 + cl;                             // entry k * C + c
    const bool ok = i < 3 * C;
    const int k = ok ? i / C : 0, c = ok ? i - k * C : 0;
    double a = 0.0;
    if (ok)
        for (int q = g; q < nparts; q += 32) a += l1a[((size_t)q * 3 + k) * pitch + c];
    __syncthreads();
    sh[g][cl] = a;
    __syncthreads();
    if (g != 0 || !ok) return;
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < 32; ++r) sum += sh[r][cl];
    const double xx[3][3] = {{m9[3], m9[4], m9[5]}, {m9[4], m9[6], m9[7]}, {m9[5], m9[7], m9[8]}};
    double mw = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) mw += xx[k][j] * (double)wx[j * skx + c * sn];
    const double gr = (double)coef[c] * sum - (double)coef[C + c] * m9[k] - (double)coef[2 * C + c] * mw;
    gw[k * skx + c * sn] = accumulate ? __fadd_rn(gw[k * skx + c * sn], (float)gr) : (float)gr;
}

// layer 1 on the vector units: the pass over the rows (P: the per-point products, or nullptr for a level without features)
int launch_l1_forward(long long rows, const GroupDims &gd, const pn2_group_src *group, const pn2_bn_layer &L, const float *P,
                             double *stats, hipStream_t st, int *nparts)
{
    const TlGather gt = make_gather(group);
    TlL1 q;
    memset(&q, 0, sizeof(q));
    q.rows = rows; q.n = gd.n; q.m = gd.m; q.nsample = gd.nsample; q.C = L.cout;
    q.xyz = group->xyz; q.new_xyz = group->new_xyz; q.idx = group->idx; q.P = P;
    q.wx = L.weight + gt.xyz_off * L.w_stride_k; q.skx = L.w_stride_k; q.sn = L.w_stride_n;

    q.bias = nullptr; q.z = L.z;                  // no conv bias in the stored tensor (pn2_mlp_train_forward)
    q.stats = stats;
    const int rpb = kL1Threads / (L.cout / 4);
    long long blocks = (rows + (long long)rpb * kL1U - 1) / ((long long)rpb * kL1U);
    if (blocks > kMaxParts) blocks = kMaxParts;
    *nparts = (int)blocks;
    return launch(tl_l1_forward_kernel, dim3((unsigned)blocks), dim3(kL1Threads), 0, st, q);
}

// dz_1 (in place when `store`) and dW1x -> rows [xyz_off, xyz_off + 3) of the layer's weight gradient
int launch_l1_dz(long long rows, const GroupDims &gd, const pn2_group_src *group, const pn2_bn_layer &L, float *dy,
                        const float *coef, float *part, bool store, hipStream_t st, bool wgrad)
{
    const TlGather gt = make_gather(group);
    TlL1 q;
    memset(&q, 0, sizeof(q));
    q.rows = rows; q.n = gd.n; q.m = gd.m; q.nsample = gd.nsample; q.C = L.cout;
    q.xyz = group->xyz; q.new_xyz = group->new_xyz; q.idx = group->idx;
    q.z = L.z; q.g = dy; q.coef = coef; q.part = part;
    const bool feat = !store && gt.cfeat > 0;                     // (store = the per-point path: its features went through P)
    if (feat) { q.points = group->points; q.cf = gt.cfeat; }
    const int nin = 3 + q.cf;
    const int rpb = kL1Threads / (L.cout / 4);
    long long blocks = (rows + (long long)rpb * kL1U - 1) / ((long long)rpb * kL1U);
    if (blocks > kMaxParts) blocks = kMaxParts;
    if (int rc = store ? launch(tl_l1_dz_kernel<true, false>, dim3((unsigned)blocks), dim3(kL1Threads), 0, st, q)
                 : feat ? launch(tl_l1_dz_kernel<false, true>, dim3((unsigned)blocks), dim3(kL1Threads), 0, st, q)
                        : launch(tl_l1_dz_kernel<false, false>, dim3((unsigned)blocks), dim3(kL1Threads), 0, st, q)) return rc;
    if (!wgrad) return PN2_OK;                                    // dz_1 alone (frozen statistics, no parameter gradient wanted)
    return launch(tl_l1_wx_reduce_kernel, dim3((unsigned)((nin * L.cout + 7) / 8)), dim3(256), 0, st, (const float *)part, (int)blocks,
                  L.cout, nin, L.grad_weight + gt.xyz_off * L.w_stride_k, L.grad_weight + gt.feat_off * L.w_stride_k, L.w_stride_k,
                  L.w_stride_n, L.grad_accumulate);
}

int launch_l1_xrows(const TlL1 &q, float4 *xg, double *mom, hipStream_t st, int *nparts)
{
    long long xb = (q.rows + kL1XrowsThreads - 1) / kL1XrowsThreads;
    if (xb > kMaxParts) xb = kMaxParts;
    *nparts = (int)xb;
    return launch(tl_l1_xrows_kernel, dim3((unsigned)xb), dim3(kL1XrowsThreads), 0, st, q, xg, mom);
}

int launch_l1_wx_combine(const double *mom, int nmom, const double *l1a, int nparts, int C, int pitch, const float *coef,
                         const float *wx, long long skx, long long sn, float *gw, int accumulate, hipStream_t st)
{
    return launch(tl_l1_wx_combine_kernel, dim3((unsigned)((3 * C + 7) / 8)), dim3(256), 0, st, mom, nmom, l1a, nparts, C, pitch, coef, wx,
                  skx, sn, gw, accumulate);
}

}  // namespace pn2
