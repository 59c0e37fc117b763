// train_mlp_device.h -- device code that more than one kernel family of the training node uses: the per-channel
// finalisations and the last-ticket tail that folds them into a pass (TlFin), the A-operand loaders and prologues of the GEMM
// body (tl_gemm_body.inc), the operand units of the weight-gradient body (tl_wgrad_body.inc). Included by the translation
// units that hold kernels (train_mlp_gemm / _wgrad / _pair / _top / _l1 / _small.hip); no host logic.
#pragma once
#include "train_mlp_kernels.h"

namespace pn2 {

// ---- per-channel finalisations (tl_bn_*finalize_kernel, and folded into the producing launch: TlFin) ----
// batch moments of one channel -> (mean, invstd, a, c), running statistics (torch.nn.BatchNorm semantics: unbiased variance in
// the average unless var_biased -- tf.contrib.layers.batch_norm, tf_util.py:512-531, averages the biased one)
__device__ __forceinline__ void tl_bn_finalize_channel(int c, int N, double s1, double s2, double count, const float *gamma,
                                                       const float *beta, float *running_mean, float *running_var, float momentum,
                                                       float eps, float *save, const float *bias, int var_biased)
{
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const double invstd = 1.0 / sqrt(var + (double)eps);
    const double a = (double)gamma[c] * invstd;
    save[c] = (float)mean;
    save[N + c] = (float)invstd;
    save[2 * N + c] = (float)a;
    save[3 * N + c] = (float)((double)beta[c] - a * mean);
    // the stored pre-norm tensor is h W WITHOUT the conv bias (see pn2_mlp_train_forward): the layer's batch mean is mean + b
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * (mean + (bias ? (double)bias[c] : 0.0)));
    if (running_var) {
        const double bv = (var_biased || count <= 1.0) ? var : var * count / (count - 1.0);
        running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * bv);
    }
}

// (sum dy, sum dy z) of one channel -> grad_gamma, grad_beta and the coefficients of dz = s dy - c0 - c1 z
__device__ __forceinline__ void tl_bn_backward_finalize_channel(int c, int N, double s1, double s2, double count, const float *gamma,
                                                                const float *save, float *grad_gamma, float *grad_beta, float *coef,
                                                                int accumulate)
{
    const double mean = save[c], invstd = save[N + c];
    const double dbeta = s1, dgamma = (s2 - mean * s1) * invstd;
    const double s = (double)gamma[c] * invstd;
    const double c1 = s * dgamma * invstd / count;
    const double c0 = s * dbeta / count - c1 * mean;
    if (grad_gamma) grad_gamma[c] = accumulate ? __fadd_rn(grad_gamma[c], (float)dgamma) : (float)dgamma;
    if (grad_beta) grad_beta[c] = accumulate ? __fadd_rn(grad_beta[c], (float)dbeta) : (float)dbeta;
    coef[c] = (float)s;
    coef[N + c] = (float)c0;
    coef[2 * N + c] = (float)c1;
}

// Device-scope traffic of the hand-off WITHOUT cache-wide fences. A release fence at agent scope is a write-back of the whole
// L2 of the XCD (buffer_wbl2) and an acquire fence invalidates it: with one such pair per workgroup the folded form measured
// 20-35 us SLOWER per pass than the separate launch (the passes' own outputs are tens of megabytes of dirty lines, and the
// invalidate costs the workgroups still running their weights). Instead the partial rows are written with write-through
// stores (agent-scope relaxed atomic stores: sc1), the storing threads wait for the write acknowledgements (s_waitcnt
// vmcnt(0)) before the workgroup takes its ticket (agent-scope relaxed atomic add, performed at the memory side), and the last
// workgroup reads the rows with agent-scope relaxed atomic loads, which bypass the non-coherent copies of its own L2 -- the
// hand-off form of sa_fused.hip's sample granules, with the ticket in place of the tag.
typedef unsigned long long __attribute__((address_space(1))) tl_gu64;
typedef unsigned __attribute__((address_space(1))) tl_gu32;

__device__ __forceinline__ void tl_fin_store(double *p, double v)     // a partial sum another workgroup of this launch will read
{
    __hip_atomic_store((tl_gu64 *)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double tl_fin_load(const double *p)
{
    return __longlong_as_double((long long)__hip_atomic_load((const tl_gu64 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// The tail of a producing workgroup of NT threads (every thread of every workgroup of the launch calls it, after its
// tl_fin_store()s of the partial row). `lds`: >= 16 NT + 16 bytes of the workgroup's LDS that nobody uses any more.
template <int NT>
__device__ __forceinline__ void tl_fin_tail(const TlFin &f, char *lds)
{
    const int tid = threadIdx.x;
    unsigned *flag = reinterpret_cast<unsigned *>(lds);
    double *sh = reinterpret_cast<double *>(lds + 16);              // [2][NT]
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // this thread's write-through stores are acknowledged ...
    __syncthreads();                                                // ... and so are every other thread's of this workgroup
    if (tid == 0)
        *flag = (__hip_atomic_fetch_add((tl_gu32 *)f.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == f.total - 1u) ? 1u : 0u;
    __syncthreads();
    if (*flag == 0u) return;                                        // workgroup-uniform
    int cb = 32;                                                    // channels per sweep (a power of two), J = NT / cb threads each
    while (cb < f.N && cb < NT) cb <<= 1;
    const int J = NT / cb, c = tid & (cb - 1), j = tid / cb;
    const int chunk = (f.nparts + J - 1) / J;
    const int N = f.N;
    const double *st = f.stats;
    for (int c0 = 0; c0 < N; c0 += cb) {
        const int ch = c0 + c;
        double s1 = 0.0, s2 = 0.0;
        if (ch < N) {
            int q = j * chunk;
            const int q1 = min(f.nparts, q + chunk);
            const double *src = st + (size_t)q * 2 * N + ch;
            for (; q + 8 <= q1; q += 8, src += (size_t)16 * N) {    // sixteen independent loads in flight, the sums in order
                double a[8], b[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { a[u] = tl_fin_load(src + (size_t)(2 * u) * N); b[u] = tl_fin_load(src + (size_t)(2 * u + 1) * N); }
#pragma unroll
                for (int u = 0; u < 8; ++u) { s1 += a[u]; s2 += b[u]; }
            }
            for (; q < q1; ++q, src += (size_t)2 * N) { s1 += tl_fin_load(src); s2 += tl_fin_load(src + N); }
        }
        sh[tid] = s1;
        sh[NT + tid] = s2;
        __syncthreads();
        if (j == 0 && ch < N) {
            double t1 = sh[c], t2 = sh[NT + c];
            for (int jj = 1; jj < J; ++jj) { t1 += sh[jj * cb + c]; t2 += sh[NT + jj * cb + c]; }
            if (f.mode == 1)
                tl_bn_finalize_channel(ch, N, t1, t2, f.count, f.gamma, f.beta, f.running_mean, f.running_var, f.momentum, f.eps, f.save,
                                       f.bias, f.var_biased);
            else
                tl_bn_backward_finalize_channel(ch, N, t1, t2, f.count, f.gamma, f.save, f.grad_gamma, f.grad_beta, f.coef, f.accumulate);
        }
        __syncthreads();
    }
}

// ---- A operand: load + prologue. Register v = 8e + j of lane (row s, half hl) <-> channel 32u + 16e + 8hl + j ------------
struct ARaw { f32x16 a, g; int4 sel[4]; };
struct RowCtx { long long grp; int sample, pt; long long cloud; };      // of the lane's row (gather / pooled passes)

template <int AMODE>
__device__ __forceinline__ RowCtx tl_row_ctx(const TlGemm &p, long long row, bool active)
{
    RowCtx c = {0, 0, 0, 0};
    if (!active) return c;
    if (AMODE == A_GATHER) {
        c.grp = row / p.g.nsample;
        c.sample = (int)(row - c.grp * p.g.nsample);
        c.cloud = c.grp / p.g.m;
        c.pt = p.g.idx ? p.g.idx[row] : c.sample;
    } else if (AMODE == A_DZ_POOL || AMODE == A_FILL) {
        c.grp = row / p.group_rows;
        c.sample = (int)(row - c.grp * p.group_rows);
    }
    return c;
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// Buffer addressing (SRSRC): a wave-uniform 128-bit descriptor in SGPRs + ONE per-lane byte offset in a VGPR + a uniform
// byte offset in an SGPR per instruction. A lane's eight row loads then share one address register (flat addressing
// needs a 64-bit VGPR pair per load in flight: 100+ registers of addresses in the kernels below).
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void *base, unsigned bytes)
{
    // The descriptor's inputs go through readfirstlane: they ARE wave-uniform (kernel arguments, block and wave numbers),
    // but hipcc cannot always prove it -- anything that met a value derived from threadIdx in a select or a phi is
    // "divergent" to it -- and an unproven descriptor gets a waterfall loop (4 x v_readfirstlane, compare, saveexec,
    // branch) around EVERY buffer instruction: 487 readfirstlanes per two blocks in the weight-gradient kernel.
    const unsigned long long a = (unsigned long long)(uintptr_t)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const unsigned nb = __builtin_amdgcn_readfirstlane(bytes);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>((uintptr_t)(((unsigned long long)hi << 32) | lo)), 0, (int)nb,
                                             0x00020000);
}
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }       // a value known to be wave-uniform
__device__ __forceinline__ float bload(rsrc_t r, int voff, int soff)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ float4 bload4(rsrc_t r, int voff, int soff)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}
__device__ __forceinline__ int4 bload4i(rsrc_t r, int voff, int soff)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_int4((int)v[0], (int)v[1], (int)v[2], (int)v[3]);
}
template <bool NT>
__device__ __forceinline__ void bstore(float x, rsrc_t r, int voff, int soff)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x), r, voff, soff, NT ? 2 : 0);     // aux bit 1 = nt (streaming store)
}

template <int AMODE>
__device__ __forceinline__ void tl_load_raw(const TlGemm &p, long long row0, long long row, const RowCtx &rc, int u, int hl,
                                            bool active, ARaw &r)
{
#pragma unroll
    for (int v = 0; v < 16; ++v) { r.a[v] = 0.0f; r.g[v] = 0.0f; }
    if (!active) return;
    if (AMODE == A_GATHER) {
        const TlGather &g = p.g;
        const float *px = g.xyz + ((size_t)rc.cloud * g.n + rc.pt) * 3;
        const float *pf = g.points ? g.points + ((size_t)rc.cloud * g.n + rc.pt) * g.cfeat : nullptr;
        const float *pc = g.new_xyz ? g.new_xyz + rc.grp * 3 : nullptr;
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 32 * u + 16 * e + 8 * hl + j;
                float val = 0.0f;
                const int kx = k - g.xyz_off, kf = k - g.feat_off;
                if (kx >= 0 && kx < 3) val = pc ? __fsub_rn(px[kx], pc[kx]) : px[kx];      // pointnet_util.py:46
                else if (kf >= 0 && kf < g.cfeat) val = pf[kf];
                r.a[8 * e + j] = val;
            }
        return;
    }
    const int s = (int)(row - row0);
    if (AMODE == A_FILL) {
        if (u < p.tk0) {                                           // (groups, K0) routed gradient + its sample numbers
            const float *pg = p.G + (size_t)rc.grp * p.K0;
            const int *ps = p.argsel + (size_t)rc.grp * p.K0;
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int k = 32 * u + 16 * e + 8 * hl + 4 * q;
                    int4 s4 = {-1, -1, -1, -1};
                    if (k < p.K0) {
                        const float4 t = ld4(pg + k);
                        r.a[8 * e + 4 * q] = t.x; r.a[8 * e + 4 * q + 1] = t.y; r.a[8 * e + 4 * q + 2] = t.z; r.a[8 * e + 4 * q + 3] = t.w;
                        s4 = *reinterpret_cast<const int4 *>(ps + k);
                    }
                    r.sel[2 * e + q] = s4;
                }
        } else {                                                   // rows of the layer below
            const rsrc_t r2 = make_rsrc(p.A2 + (size_t)row0 * p.K1, 32u * (unsigned)p.K1 * 4u);
            const int voff2 = (s * p.K1 + 8 * hl) * 4, soff2 = (u - p.tk0) * 128;
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int k = 32 * (u - p.tk0) + 16 * e + 8 * hl + 4 * q;
                    if (k < p.K1) {
                        const float4 t = bload4(r2, voff2 + (16 * e + 4 * q) * 4, soff2);
                        r.a[8 * e + 4 * q] = t.x; r.a[8 * e + 4 * q + 1] = t.y; r.a[8 * e + 4 * q + 2] = t.z; r.a[8 * e + 4 * q + 3] = t.w;
                    }
                }
        }
        return;
    }
    // rows of the item: descriptor at the item's first row, lane offset = its row and half, uniform offset = the k tile
    const rsrc_t ra = make_rsrc(p.A + (size_t)row0 * p.K, 32u * (unsigned)p.K * 4u);
    const int voff = (s * p.K + 8 * hl) * 4, soff = u * 128;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = 32 * u + 16 * e + 8 * hl + 4 * q;
            if (k < p.K) {
                const float4 t = bload4(ra, voff + (16 * e + 4 * q) * 4, soff);
                r.a[8 * e + 4 * q] = t.x; r.a[8 * e + 4 * q + 1] = t.y; r.a[8 * e + 4 * q + 2] = t.z; r.a[8 * e + 4 * q + 3] = t.w;
            }
        }
    if (AMODE == A_DZ) {
        const rsrc_t rg = make_rsrc(p.G + (size_t)row0 * p.K, 32u * (unsigned)p.K * 4u);
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int k = 32 * u + 16 * e + 8 * hl + 4 * q;
                if (k < p.K) {
                    const float4 t = bload4(rg, voff + (16 * e + 4 * q) * 4, soff);
                    r.g[8 * e + 4 * q] = t.x; r.g[8 * e + 4 * q + 1] = t.y; r.g[8 * e + 4 * q + 2] = t.z; r.g[8 * e + 4 * q + 3] = t.w;
                }
            }
    }
    if (AMODE == A_DZ_POOL) {
        const float *pg = p.G + (size_t)rc.grp * p.K;
        const int *ps = p.argsel + (size_t)rc.grp * p.K;
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int k = 32 * u + 16 * e + 8 * hl + 4 * q;
                int4 s4 = {-1, -1, -1, -1};
                if (k < p.K) {
                    const float4 t = ld4(pg + k);
                    r.g[8 * e + 4 * q] = t.x; r.g[8 * e + 4 * q + 1] = t.y; r.g[8 * e + 4 * q + 2] = t.z; r.g[8 * e + 4 * q + 3] = t.w;
                    s4 = *reinterpret_cast<const int4 *>(ps + k);
                }
                r.sel[2 * e + q] = s4;
            }
    }
}

// the pass's prologue on the 16 values of one k tile; lp*: the per-channel parameters in LDS (zero beyond K)
template <int AMODE>
__device__ __forceinline__ f32x16 tl_finish(const ARaw &r, const RowCtx &rc, int u, int tk0, int hl, const float *lp0,
                                            const float *lp1, const float *lp2)
{
    if (AMODE == A_PLAIN || AMODE == A_GATHER) return r.a;
    f32x16 x;
    const int sample = rc.sample;
    if (AMODE == A_FILL) {                                         // lp0: s (fill tiles) / a (rows of the layer below); lp1: c
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int k = 32 * u + 16 * e + 8 * hl + 4 * q;
                const float4 c0 = ld4(lp0 + k), c1 = ld4(lp1 + k);
                const float a0[4] = {c0.x, c0.y, c0.z, c0.w}, a1[4] = {c1.x, c1.y, c1.z, c1.w};
                const int4 s4 = r.sel[2 * e + q];
                const int sl[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int v = 8 * e + 4 * q + i;
                    if (u < tk0) x[v] = sl[i] == sample ? __fmul_rn(a0[i], r.a[v]) : 0.0f;        // the pool routes dy to ONE sample
                    else x[v] = vmax(__fadd_rn(__fmul_rn(a0[i], r.a[v]), a1[i]), 0.0f);
                }
            }
        return x;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int k = 32 * u + 16 * e + 8 * hl + 4 * q;
            const float4 c0 = ld4(lp0 + k), c1 = ld4(lp1 + k);
            const float a0[4] = {c0.x, c0.y, c0.z, c0.w}, a1[4] = {c1.x, c1.y, c1.z, c1.w};
            if (AMODE == A_RELU) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int v = 8 * e + 4 * q + i;
                    x[v] = vmax(__fadd_rn(__fmul_rn(a0[i], r.a[v]), a1[i]), 0.0f);        // h = relu(a z + c)
                }
            } else {
                const float4 c2 = ld4(lp2 + k);
                const float a2[4] = {c2.x, c2.y, c2.z, c2.w};
                int sl[4] = {0, 0, 0, 0};
                if (AMODE == A_DZ_POOL) {
                    const int4 s4 = r.sel[2 * e + q];
                    sl[0] = s4.x; sl[1] = s4.y; sl[2] = s4.z; sl[3] = s4.w;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int v = 8 * e + 4 * q + i;
                    float dy = r.g[v];
                    if (AMODE == A_DZ_POOL) dy = sl[i] == sample ? dy : 0.0f;             // the pool routes dy to ONE sample
                    x[v] = __fsub_rn(__fsub_rn(__fmul_rn(a0[i], dy), a1[i]), __fmul_rn(a2[i], r.a[v]));   // s dy - c0 - c1 z
                }
            }
        }
    return x;
}

// ---- weight gradient: the operand units of tl_wgrad_body.inc ----
// One UNIT of operand data = what one wave holds as the MFMA fragment of K16 step e of a 32-channel tile: lane (c, hl)
// <-> channel 32 tile + c, rows 16e + 8hl + j (j = 0..7) of the 32-row block. A wave loads a unit with dword loads whose
// 32 lanes cover 128 contiguous bytes of a row, applies the pass's prologue, splits into the three bf16 levels and writes
// three 16-byte fragments into the block's LDS image, from where EVERY wave of the workgroup reads the fragments of the
// output tiles it owns: operands cross the vector memory path once per workgroup.
//
// Two rules shaped this code (both measured):
//  * BRANCH-FREE loads. The units of a workgroup differ in kind (rows of h, rows of z and dy, routed gradient, nothing),
//    and a wait shared by paths with different numbers of loads in flight can only be vmcnt(0) -- with branches around the
//    loads the two-block prefetch drained at every block. Every unit of every wave therefore issues the same sequence of
//    buffer loads, and what a unit does not need points at an empty descriptor (out-of-range: returns 0, no memory access).
//  * Everything that does not depend on the block is computed ONCE per unit (WgUnit, before the block loop): these
//    kernels issue ~2500 instructions per 32-row block and wave, and were bound by that, not by memory.
enum { K_NONE = 0, K_H = 1, K_HGATHER = 2, K_DZ = 3, K_DZPOOL = 4, K_FILL = 5, K_ONES = 6 };
enum { D_DZ = 0, D_DZPOOL = 1, D_TOP = 2 };                       // second-operand class of the launch (template parameter)

struct WgRaw { float z[8], g[8]; float gq; int sel, off; };      // off: first row of the unit inside its group
struct WgUnit {
    int kind;                   // uniform
    int relu;                   // uniform: K_H rows go through relu(p0 z + p1) (else taken as they are)
    int e, tile;                // uniform: K16 step, tile of the block image
    const float *b1, *b2;       // uniform: row streams (nullptr: none)
    int pitch1;                 // uniform: floats per row of the row streams
    int voff;                   // lane: byte offset of its first row inside the block's rows (kWgOob: no such channel)
    const float *bq;            // uniform: per-group values (routed gradient / centroid)
    const int *bs;              // uniform: per-group sample numbers
    int nq, chq;                // uniform pitch / lane channel (-1: none) of the per-group streams
    // gather (layer 1 of an SA level): a lane's channel is a coordinate (kx) or a feature (kf) of the row's point; the two
    // tensors are read through two UNIFORM descriptors, the lane that needs neither / only one reads out of range there
    // (a per-lane descriptor would put a waterfall loop around every load)
    const float *bgx, *bgf;     // uniform: xyz, points
    int kx, kf, pitchf;         // lane: coordinate / feature number (-1: none); uniform: feature channels per point
    float p0, p1, p2;           // lane: per-channel parameters of the prologue
};
constexpr int kWgOob = (int)0xfffffff0u;                         // beyond every descriptor's num_records (<= 0x7fffffff)

__device__ __forceinline__ int bloadi(rsrc_t r, int voff, int soff)
{
    return (int)__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
}

__device__ __forceinline__ WgUnit wg_plan_unit(const TlWgrad &p, int unit, int nunits, int us, int ts, int lane)
{
    WgUnit w;
    const int hl = lane >> 5, c = lane & 31;
    w.kind = K_NONE; w.relu = 0; w.e = unit & 1; w.tile = unit >> 1;
    w.b1 = nullptr; w.b2 = nullptr; w.bq = nullptr; w.bs = nullptr; w.bgx = nullptr; w.bgf = nullptr;
    w.pitch1 = 0; w.voff = kWgOob; w.nq = 0; w.chq = -1; w.kx = -1; w.kf = -1; w.pitchf = 0;
    w.p0 = 1.0f; w.p1 = 0.0f; w.p2 = 0.0f;
    if (unit >= nunits) return w;
    const int rin = 16 * w.e + 8 * hl, tx = (p.KI + 31) / 32;
    if (w.tile < p.tus) {                                          // the layer's input h
        const int ch = (us * p.tus + w.tile) * 32 + c;
        if (p.amode == A_GATHER) {
            const TlGather &g = p.g;
            const int kx = ch - g.xyz_off, kf = ch - g.feat_off;
            w.kind = K_HGATHER;
            w.bgx = g.xyz; w.bgf = g.points; w.pitchf = g.cfeat; w.bq = g.new_xyz; w.nq = 3;     // pointers: uniform choices only
            if (ch < p.KI && kx >= 0 && kx < 3) { w.kx = kx; w.chq = g.new_xyz ? kx : -1; }
            else if (ch < p.KI && kf >= 0 && kf < g.cfeat) w.kf = kf;
        } else {
            w.kind = K_H; w.b1 = p.A; w.pitch1 = p.KI; w.relu = p.amode == A_RELU;
            if (ch < p.KI) {
                w.voff = (rin * p.KI + ch) * 4;
                if (p.amode == A_RELU) { w.p0 = p.pa[ch]; w.p1 = p.pc[ch]; }
            }
        }
        return w;
    }
    const int tg = ts * p.tts + w.tile - p.tus;                    // tile of the second operand
    if (p.dmode == A_FILL) {                                       // [s dy routed to the pooled samples | h itself | ones]
        if (tg < p.tf) {
            const int ch = tg * 32 + c;
            w.kind = K_FILL; w.bq = p.G; w.bs = p.argsel; w.nq = p.NF;
            if (ch < p.NF) { w.chq = ch; w.p0 = p.coef[ch]; }
        } else if (tg < p.tf + tx) {
            if (!p.xshare) {
                const int ch = (tg - p.tf) * 32 + c;
                w.kind = K_H; w.b1 = p.A; w.pitch1 = p.KI; w.relu = 1;
                if (ch < p.KI) { w.voff = (rin * p.KI + ch) * 4; w.p0 = p.pa[ch]; w.p1 = p.pc[ch]; }
            }
        } else if (tg == p.tf + tx) {
            w.kind = K_ONES;
        }
        return w;
    }
    const int ch = tg * 32 + c;                                    // dz = s dy - c0 - c1 z
    w.kind = p.dmode == A_DZ_POOL ? K_DZPOOL : K_DZ;
    w.b1 = p.Z; w.pitch1 = p.NO;
    if (p.dmode == A_DZ_POOL) { w.bq = p.G; w.bs = p.argsel; w.nq = p.NO; } else w.b2 = p.G;
    if (ch < p.NO) {
        w.voff = (rin * p.NO + ch) * 4;
        if (p.dmode == A_DZ_POOL) w.chq = ch;
        w.p0 = p.coef[ch]; w.p1 = p.coef[p.NO + ch]; w.p2 = p.coef[2 * p.NO + ch];
    }
    return w;
}

// the loads of one unit for the block whose first row is row0 (live = false: no such block -- everything out of range).
// grp_u / off_u: group of the block and its first row inside it when a group is a multiple of 32 rows (uniform).
template <bool GATHER, int DCLS>
__device__ __forceinline__ void wg_load_unit(const TlWgrad &p, const WgUnit &w, long long row0, int grp_u, int off_u, int lane,
                                             bool live, WgRaw &r)
{
    const int hl = lane >> 5, rin = 16 * w.e + 8 * hl, step = uni(w.pitch1 * 4);
    const unsigned bytes1 = live ? 32u * (unsigned)w.pitch1 * 4u : 0u;
    rsrc_t r1 = make_rsrc(w.b1 ? w.b1 + (size_t)row0 * w.pitch1 : nullptr, w.b1 ? bytes1 : 0u);
    // per-group values: groups are 16 rows or a multiple of 32 (one group per block, uniform)
    const bool g16 = p.group_rows == 16;
    const int grp = g16 ? (((int)row0 + rin) >> 4) : grp_u;
    r.off = g16 ? ((rin & 8)) : off_u + rin;
    rsrc_t rq = make_rsrc(w.bq, (w.bq && live) ? 0x7fffffffu : 0u);
    const rsrc_t rs = make_rsrc(w.bs, (w.bs && live) ? 0x7fffffffu : 0u);
    int voffq = w.chq >= 0 ? (grp * w.nq + w.chq) * 4 : kWgOob;
    if (GATHER) {
        // rows of the grouped input: the point numbers of the step's 16 rows come through wave-uniform (scalar) loads --
        // counted by lgkmcnt, they do not disturb the vector loads in flight -- and each lane then picks its half
        const TlGather &g = p.g;
        const bool gat = w.kind == K_HGATHER;
        const int ggrp = (int)((unsigned)((int)row0 + rin) / (unsigned)g.nsample);      // group sizes are multiples of 8
        const int s0 = (int)row0 + rin - ggrp * g.nsample, cloud = ggrp / g.m;
        int pts[16];
        const int *ip = (g.idx && live) ? g.idx + row0 + 16 * w.e : nullptr;
#pragma unroll
        for (int j = 0; j < 16; ++j) pts[j] = ip ? ip[j] : 0;
        const rsrc_t r2 = make_rsrc(w.b2 ? w.b2 + (size_t)row0 * w.pitch1 : nullptr, w.b2 ? bytes1 : 0u);
        const rsrc_t rx = make_rsrc(w.bgx, (w.bgx && live) ? 0x7fffffffu : 0u), rf = make_rsrc(w.bgf, (w.bgf && live) ? 0x7fffffffu : 0u);
        if (gat) voffq = w.chq >= 0 ? (ggrp * 3 + w.chq) * 4 : kWgOob;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int pt = g.idx ? (hl ? pts[8 + j] : pts[j]) : s0 + j;
            const int vx = w.kx >= 0 ? ((cloud * g.n + pt) * 3 + w.kx) * 4 : kWgOob;
            const int vf = w.kf >= 0 ? ((cloud * g.n + pt) * w.pitchf + w.kf) * 4 : kWgOob;
            const int vr = w.voff == kWgOob ? kWgOob : w.voff + j * step;
            r.z[j] = bload(gat ? rx : r1, gat ? vx : vr, 0);         // uniform choice of the descriptor
            r.g[j] = bload(gat ? rf : r2, gat ? vf : vr, 0);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) r.z[j] = bload(r1, w.voff, j * step);
        if (DCLS == D_DZ) {
            const rsrc_t r2 = make_rsrc(w.b2 ? w.b2 + (size_t)row0 * w.pitch1 : nullptr, w.b2 ? bytes1 : 0u);
#pragma unroll
            for (int j = 0; j < 8; ++j) r.g[j] = bload(r2, w.voff, j * step);
        }
    }
    if (DCLS != D_DZ || GATHER) {
        r.gq = bload(rq, voffq, 0);
        r.sel = bloadi(rs, voffq, 0);
    }
}

// Position of lane's 16-byte fragment inside a (tile, level, e) row of the block image. Plain lane order serves the weight
// gradient (every reader takes lane's own fragment); the data gradient fused into the pass reads the image TRANSPOSED --
// lane = row, eight 2-byte reads from eight channels' fragments -- and in plain order the 64 lanes of such a read hit
// four banks (rows 8 apart are 128-byte multiples apart). The XOR spreads the eight (e, row half, channel half) classes
// over the eight 16-byte bank groups; it permutes fragments inside aligned groups of eight, so the 16-byte accesses
// stay conflict-free.
__device__ __forceinline__ int wg_swz(int lane, int e) { return lane ^ (((lane >> 3) & 1) | (((lane >> 5) & 1) << 1) | (e << 2)); }

// prologue + split of a loaded unit -> its three fragments in the block image ([tile][level][e][lane] 16-byte vectors)
// zr != nullptr (data gradient in the same pass): the RAW rows of the first operand (the pre-norm tensor of the layer below)
// also go to LDS as fp32 [row][channel], pitch zpitch floats -- the data gradient's epilogue needs them for the ReLU mask
// and the batch-norm backward sums, and a global load there, however close in L2, could only return after every older
// prefetch load (in-order return counting): it cost the two-block prefetch
//
// imgA != nullptr: a dense second-operand unit (dz) also leaves its three levels in the layout the DATA gradient's MFMA reads
// as its A operand -- lane = row, eight consecutive channels per 16-byte fragment: [tile][level][K16 step q][row + 32 g] --
// as 2-byte stores (each lane holds ONE channel of eight rows; the transposition has to happen somewhere, and here it is
// spread over the eight producer waves instead of eight 2-byte reads per fragment in the two consumer waves). The 16-byte
// slot index is XOR-ed with (g | hl << 1 | q << 2): without it the 64 lanes of one store hit four banks.
//
// MASKED (ragged rows, train_mlp_ragged.hip): mw is the validity word of the block; the unit's eight rows 16 e + 8 hl + j whose
// bit is clear enter BOTH operands as zero (selects behind the prologues): h^T dz gets nothing from a padding row, whatever it holds.
template <int DCLS, bool MASKED = false>
__device__ __forceinline__ void wg_store_unit(const WgUnit &w, const WgRaw &r, int lane, u32x4 *img, float *zr = nullptr, int zpitch = 0,
                                              u32x4 *imgA = nullptr, int tus = 0, unsigned mw = 0xffffffffu)
{
    if (w.kind == K_NONE || w.kind == K_ONES) return;             // nothing / written once before the loop
    if (zr && w.kind == K_H && w.relu && w.tile * 32 + 32 <= zpitch) {
        float *zo = zr + (16 * w.e + 8 * (lane >> 5)) * zpitch + w.tile * 32 + (lane & 31);
#pragma unroll
        for (int j = 0; j < 8; ++j) zo[j * zpitch] = r.z[j];
    }
    u32x4 *o = img + ((size_t)w.tile * 3 * 2 + w.e) * 64 + wg_swz(lane, w.e);
    if (DCLS == D_TOP && w.kind == K_FILL) {
        // one non-zero per lane (the pool routes dy to ONE row): split it once and drop its three bf16 levels into slot rel
        const int rel = r.sel - r.off;                             // the pooled sample's row inside this unit, if it is here
        const float v = (rel >= 0 && rel < 8 && w.chq >= 0) ? __fmul_rn(w.p0, r.gq) : 0.0f;
        const unsigned b1 = pack_bf16(v, 0.0f) & 0xffffu;
        const float r1 = __fsub_rn(v, __uint_as_float(b1 << 16));
        const unsigned b2 = pack_bf16(r1, 0.0f) & 0xffffu;
        const float r2 = __fsub_rn(r1, __uint_as_float(b2 << 16));
        const unsigned b3 = pack_bf16(r2, 0.0f) & 0xffffu;
        const int d = rel >> 1, sh = (rel & 1) * 16;
        u32x4 l1, l2, l3;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            l1[q] = d == q ? b1 << sh : 0u;
            l2[q] = d == q ? b2 << sh : 0u;
            l3[q] = d == q ? b3 << sh : 0u;
        }
        o[0] = l1; o[128] = l2; o[256] = l3;
        return;
    }
    f32x16 x;
#pragma unroll
    for (int v = 0; v < 16; ++v) x[v] = 0.0f;
    if (w.kind == K_H) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float y = vmax(__fadd_rn(__fmul_rn(w.p0, r.z[j]), w.p1), 0.0f);
            x[j] = w.voff == kWgOob ? 0.0f : w.relu ? y : r.z[j];
        }
    } else if (w.kind == K_HGATHER) {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = __fadd_rn(__fsub_rn(r.z[j], r.gq), r.g[j]);   // pointnet_util.py:46: coordinate - centroid (z, gq) or feature (g); the other stream read 0
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float dy = DCLS == D_DZPOOL ? (r.sel - r.off == j ? r.gq : 0.0f) : r.g[j];
            x[j] = w.voff == kWgOob ? 0.0f : __fsub_rn(__fsub_rn(__fmul_rn(w.p0, dy), w.p1), __fmul_rn(w.p2, r.z[j]));
        }
    }
    if (MASKED) {
        const unsigned mb = mw >> (16 * w.e + 8 * (lane >> 5));
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = ((mb >> j) & 1u) ? x[j] : 0.0f;
    }
    const ActSplit sp = split_act(x);                             // registers 0..7 -> p[0][level]
    o[0] = sp.p[0][0];
    o[128] = sp.p[0][1];
    o[256] = sp.p[0][2];
    if (imgA && (w.kind == K_DZ || w.kind == K_DZPOOL)) {
        const int c = lane & 31, hl = lane >> 5, q = c >> 4, g = (c >> 3) & 1, sg = g | (hl << 1) | (q << 2);
        char *ba = reinterpret_cast<char *>(imgA) + ((size_t)(w.tile - tus) * 6 + q) * 1024 + (16 * w.e + 8 * hl + 32 * g) * 16 + (c & 7) * 2;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                char *pa = ba + (((2 * d + half) ^ sg) << 4);
#pragma unroll
                for (int lv = 0; lv < 3; ++lv)
                    *reinterpret_cast<unsigned short *>(pa + lv * 2048) = (unsigned short)(half ? sp.p[0][lv][d] >> 16 : sp.p[0][lv][d] & 0xffffu);
            }
    }
}

}  // namespace pn2
