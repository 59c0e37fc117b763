// train_mlp_xyz.hip -- the coordinate gradients of the SA training node (pn2_mlp_train_backward_xyz): the entry points, their
// argument checks and the two kernels only this gradient needs. The passes themselves are train_mlp.hip's
// (tl_train_backward with TlCall::grad_xyz). gfx950.
//
// The reference differentiates a set-abstraction level with respect to the coordinates: GroupPoint and GatherPoint register
// gradients, and d loss / d xyz flows through grouped_xyz - new_xyz (utils/pointnet_util.py:44-46, :179-180) into layer 1.
// Row r = (cloud i, group j, sample k) with p = idx[i,j,k] reads u_r = xyz[i,p] - new_xyz[i,j]; with W1x the three coordinate
// rows of layer 1's weight and dz_1 the gradient at layer 1's pre-norm output (backward forms it anyway),
//     g_r               = dz_1[r,:] . W1x^T                     tl_xyz_rows_kernel: one pass over (dy_1, z_1), 3 floats per row
//     grad_new_xyz[i,j] = - sum_k g_(i,j,k)                     tl_xyz_centroid_kernel: a group's rows are contiguous
//     grad_xyz[i,p]     = sum over the rows r that name p of g_r  pn2_group_point_grad_seg at 3 channels (no float atomics;
//                                                               `reproducible` = its sorted-segment mode)
// group_all has neither centroid nor idx: grad_xyz[i,k] = g_r, written by the first kernel. Where layer 1 runs once per point
// (tl_l1_forward_kernel) backward has already scattered dz_1 onto the points as S (b n, cout_1), and grad_xyz = S . W1x^T is
// the same kernel over the b n points: no second scatter. weighted_avg pooling is refused: its weights exp(-5 |grouped xyz|)
// depend on xyz, and the norm has no derivative at the centroid, which is a member of its own ball.
#include "train_mlp_internal.h"

#include <limits.h>

namespace pn2 {

struct TlXyz {
    long long rows;
    int C;                      // cout_1
    const float *G;             // (rows, C): dy_1 -- or dz_1 itself when coef == nullptr; argsel != nullptr: gq (groups, C)
    const float *Z;             // (rows, C): z_1 (coef != nullptr)
    const float *coef;          // (3, C): s, c0, c1 of dz_1 = s dy_1 - c0 - c1 z_1, or nullptr
    const int *argsel;          // a pooled single-layer stack: (groups, C), the max routes dy to ONE sample of the group
    int group_rows;             // ... rows per group
    const float *wx;            // W1x: wx[k * sk + col * sn], k = 0..2
    long long sk, sn;
    float *out;                 // (rows, 3)
};

constexpr int kXyzThreads = 256, kXyzU = 4;

struct XyzCols { float w[3][4], s[4], c0[4], c1[4]; };

__device__ __forceinline__ float4 xyz_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

__device__ __forceinline__ XyzCols xyz_cols(const TlXyz &p, int col)
{
    XyzCols c;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) c.w[k][i] = p.wx[k * p.sk + (col + i) * p.sn];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c.s[i] = p.coef ? p.coef[col + i] : 1.0f;
        c.c0[i] = p.coef ? p.coef[p.C + col + i] : 0.0f;
        c.c1[i] = p.coef ? p.coef[2 * p.C + col + i] : 0.0f;
    }
    return c;
}

// g_r = dz_1[r,:] . W1x^T. LPR lanes share a row, 4 columns each per trip (SINGLE: C / 4 <= LPR, one trip, the columns'
// weights and coefficients stay in registers); a workgroup takes batches of kXyzU slices of 256 / LPR rows, all loads of a
// batch issued before the first is used; the lanes of a row meet through a shuffle tree (a fixed order: same bits every run).
template <int LPR, bool SINGLE>
__global__ __launch_bounds__(kXyzThreads) void tl_xyz_rows_kernel(const TlXyz p)
{
    constexpr int RPB = kXyzThreads / LPR;
    const int gl = threadIdx.x % LPR, rl = threadIdx.x / LPR, nq = p.C / 4;
    XyzCols ch;
    if (SINGLE) ch = xyz_cols(p, 4 * (gl < nq ? gl : 0));
    const long long span = (long long)RPB * kXyzU, nb = (p.rows + span - 1) / span;
    for (long long bt = blockIdx.x; bt < nb; bt += gridDim.x) {
        long long row[kXyzU];
        bool ok[kXyzU];
        float acc[kXyzU][3];
#pragma unroll
        for (int u = 0; u < kXyzU; ++u) {
            const long long r = bt * span + (long long)u * RPB + rl;
            ok[u] = r < p.rows;
            row[u] = ok[u] ? r : p.rows - 1;
            acc[u][0] = acc[u][1] = acc[u][2] = 0.0f;
        }
        for (int q = gl; q < nq; q += LPR) {
            const int col = 4 * q;
            if (!SINGLE) ch = xyz_cols(p, col);
            float4 g4[kXyzU], z4[kXyzU];
            int4 s4[kXyzU];
            int sample[kXyzU];
#pragma unroll
            for (int u = 0; u < kXyzU; ++u) {
                if (p.argsel) {
                    const long long grp = row[u] / p.group_rows;
                    sample[u] = (int)(row[u] - grp * p.group_rows);
                    g4[u] = xyz_ld4(p.G + (size_t)grp * p.C + col);
                    s4[u] = *reinterpret_cast<const int4 *>(p.argsel + (size_t)grp * p.C + col);
                } else {
                    sample[u] = 0;
                    s4[u] = make_int4(0, 0, 0, 0);
                    g4[u] = xyz_ld4(p.G + (size_t)row[u] * p.C + col);
                }
                z4[u] = p.coef ? xyz_ld4(p.Z + (size_t)row[u] * p.C + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < kXyzU; ++u) {
                const float gg[4] = {g4[u].x, g4[u].y, g4[u].z, g4[u].w}, zz[4] = {z4[u].x, z4[u].y, z4[u].z, z4[u].w};
                const int sl[4] = {s4[u].x, s4[u].y, s4[u].z, s4[u].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float dy = gg[i];
                    if (p.argsel) dy = sl[i] == sample[u] ? dy : 0.0f;
                    const float dz = p.coef ? __fsub_rn(__fsub_rn(__fmul_rn(ch.s[i], dy), ch.c0[i]), __fmul_rn(ch.c1[i], zz[i])) : dy;
#pragma unroll
                    for (int k = 0; k < 3; ++k) acc[u][k] = fmaf(dz, ch.w[k][i], acc[u][k]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kXyzU; ++u) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float v = acc[u][k];
#pragma unroll
                for (int o = LPR / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
                acc[u][k] = v;
            }
            if (gl == 0 && ok[u]) {
                float *o = p.out + (size_t)row[u] * 3;
                o[0] = acc[u][0]; o[1] = acc[u][1]; o[2] = acc[u][2];
            }
        }
    }
}

// grad_new_xyz[group] = - sum of the group's ns rows of g (16 lanes a group, a fixed order)
__global__ __launch_bounds__(256) void tl_xyz_centroid_kernel(long long groups, int ns, const float *__restrict__ g,
                                                              float *__restrict__ out)
{
    const int l16 = threadIdx.x & 15;
    const long long per = (long long)gridDim.x * 16, trips = (groups + per - 1) / per;
    for (long long t = 0; t < trips; ++t) {                          // wave-uniform: the shuffles need all lanes
        const long long gi = t * per + (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
        const bool ok = gi < groups;
        const float *src = g + (size_t)(ok ? gi : groups - 1) * ns * 3;
        float a[3] = {0.f, 0.f, 0.f};
        for (int k = l16; k < ns; k += 16) {
            a[0] = __fadd_rn(a[0], src[(size_t)k * 3]);
            a[1] = __fadd_rn(a[1], src[(size_t)k * 3 + 1]);
            a[2] = __fadd_rn(a[2], src[(size_t)k * 3 + 2]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) a[k] += __shfl_xor(a[k], o);
        if (ok && l16 == 0) {
            out[gi * 3] = -a[0]; out[gi * 3 + 1] = -a[1]; out[gi * 3 + 2] = -a[2];
        }
    }
}

// ---- called by tl_train_backward (train_mlp.hip) ----
int xyz_launch_rows(long long rows, int C, const float *G, const float *Z, const float *coef, const int *argsel, int group_rows,
                    const float *wx, long long sk, long long sn, float *out, hipStream_t st)
{
    TlXyz p;
    memset(&p, 0, sizeof(p));
    p.rows = rows; p.C = C; p.G = G; p.Z = Z; p.coef = coef; p.argsel = argsel; p.group_rows = group_rows;
    p.wx = wx; p.sk = sk; p.sn = sn; p.out = out;
    const int nq = C / 4;
    int lpr = 1;
    while (lpr < nq && lpr < 64) lpr <<= 1;
    const long long span = (long long)(kXyzThreads / lpr) * kXyzU;
    long long blocks = (rows + span - 1) / span;
    if (blocks > 2048) blocks = 2048;
    const dim3 grid((unsigned)blocks), block(kXyzThreads);
    switch (lpr) {
    case 1: return launch(tl_xyz_rows_kernel<1, true>, grid, block, 0, st, p);
    case 2: return launch(tl_xyz_rows_kernel<2, true>, grid, block, 0, st, p);
    case 4: return launch(tl_xyz_rows_kernel<4, true>, grid, block, 0, st, p);
    case 8: return launch(tl_xyz_rows_kernel<8, true>, grid, block, 0, st, p);
    case 16: return launch(tl_xyz_rows_kernel<16, true>, grid, block, 0, st, p);
    case 32: return launch(tl_xyz_rows_kernel<32, true>, grid, block, 0, st, p);
    default: break;
    }
    return nq <= 64 ? launch(tl_xyz_rows_kernel<64, true>, grid, block, 0, st, p) : launch(tl_xyz_rows_kernel<64, false>, grid, block, 0, st, p);
}

int xyz_launch_centroids(long long groups, int ns, const float *g, float *out, hipStream_t st)
{
    long long blocks = (groups + 15) / 16;
    if (blocks > 2048) blocks = 2048;
    return launch(tl_xyz_centroid_kernel, dim3((unsigned)blocks), dim3(256), 0, st, groups, ns, g, out);
}

}  // namespace pn2

extern "C" int pn2_mlp_train_xyz_supported(long long rows, int nlayers, const int *widths, int pool_rows, int pooling,
                                           const int *group_dims)
{
    if (pooling == 2 || !pn2_mlp_train_pool_supported(rows, nlayers, widths, pool_rows, pooling)) return 0;
    if (pool_rows <= 0) return 0;                                    // grouped levels only
    if (!group_dims) return 1;                                       // (the shape alone)
    const long long b = group_dims[0], n = group_dims[1], m = group_dims[2], ns = group_dims[3];
    if (b <= 0 || n <= 0 || m <= 0 || ns != pool_rows || b * m * ns != rows || group_dims[4] < 0) return 0;
    if (widths[0] != 3 + group_dims[4]) return 0;
    if (!group_dims[5] && (m != 1 || ns != n)) return 0;             // group_all: one group holding the cloud
    if (m * ns > INT_MAX || b * n > INT_MAX) return 0;               // the segmented reduction's index range
    return pn2::tl_xyz_ws_bytes(rows, nlayers, widths, pool_rows, pooling, group_dims, nullptr) >= 0 ? 1 : 0;
}

extern "C" long long pn2_mlp_train_ws_bytes_xyz(long long rows, int nlayers, const int *widths, int pool_rows, int pooling,
                                                const int *group_dims, const pn2_train_opts *opts)
{
    if (!widths || !group_dims || pooling < 0 || pooling > 3 || pooling == 2 || pool_rows <= 0) return -1;
    return pn2::tl_xyz_ws_bytes(rows, nlayers, widths, pool_rows, pooling, group_dims, opts);
}

extern "C" int pn2_mlp_train_backward_xyz(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                          int pool_rows, int pooling, const float *out, const int *argsel, const float *zsel,
                                          const float *pool_w, const float *grad_out, float *grad_feat_rows, float *grad_points,
                                          float *grad_xyz, float *grad_new_xyz, int reproducible, void *ws,
                                          const pn2_train_opts *opts, void *stream)
{
    if (!grad_xyz && !grad_new_xyz)
        return pn2_mlp_train_backward_pool(rows, nlayers, layers, group, pool_rows, pooling, out, argsel, zsel, pool_w, grad_out,
                                           grad_feat_rows, grad_points, reproducible, ws, opts, stream);
    if (pooling < 0 || pooling > 3 || pooling == 2 || pool_rows <= 0) return PN2_E_ARG;
    if (!group || !grad_xyz) return PN2_E_NULL;
    if (group->new_xyz && !grad_new_xyz) return PN2_E_NULL;
    if (!group->new_xyz && grad_new_xyz) return PN2_E_ARG;
    if (group->m <= 0 || group->nsample <= 0 || (long long)group->m * group->nsample > INT_MAX ||
        (long long)group->b * group->n > INT_MAX) return PN2_E_ARG;
    if (int rc = pn2::tl_pool_args(pool_rows, pooling, true)) return rc;
    pn2::TlCall c{};
    c.rows = rows; c.nlayers = nlayers; c.layers = layers;
    c.group = group;
    c.pool_rows = pool_rows; c.pooling = pooling;
    c.out = out; c.argsel = argsel; c.zsel = zsel;                  // (pool_w: weighted_avg was refused above)
    c.grad_out = grad_out;
    c.grad_feat_rows = grad_feat_rows; c.grad_points = grad_points;
    c.grad_xyz = grad_xyz; c.grad_new_xyz = grad_new_xyz;
    c.reproducible = reproducible;
    c.ws = ws; c.opts = opts; c.stream = stream;
    return pn2::tl_train_backward(c);
}
