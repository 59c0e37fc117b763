// fps.hip -- farthest point sampling for gfx950 (MI355X).
//
// Replaces farthestpointsamplingKernel/Launcher (reference
// tf_ops/sampling/tf_sampling_g.cu:105-170, :203-205). Results are index-exact
// with that kernel run in CPU arithmetic (oracle/pn2_oracle.c), including its
// tie rule: among equal running-min distances the point with the smallest
// (k mod 512, k) wins (512 = the reference's blockDim).
//
// Design (DESIGN.md "FPS"). FPS is a chain of m-1 dependent block-wide
// arg-max steps; it is latency bound, not HBM bound. One workgroup owns one
// cloud for the whole chain:
//   * every point's x,y,z and running min-distance live in VGPRs for all m
//     rounds (no per-round memory traffic at all; the reference round-trips
//     `temp` through global memory every round);
//   * points are dealt to threads in TIE-RANK order: thread t holds ranks
//     t*P .. t*P+P-1 where rank(k) = (k mod 512)*ceil(n/512) + k/512, so the
//     reference's tie rule becomes "smaller rank wins";
//   * a candidate is the 64-bit key (value bits : T*P - 1 - rank). Read as
//     an fp64 number that pattern is positive, finite and ordered exactly like
//     (larger value, then smaller rank), so EVERY level of the arg-max is a
//     plain v_max_f64: P-1 per lane, six DPP steps per wave (two v_mov_b32_dpp
//     + one v_max_f64 each, no scalar unit), W-1 per wave after the barrier;
//   * one s_barrier per round: lane 63 of each wave publishes the wave key in
//     a parity double-buffered LDS slot array, every wave max-reduces the W
//     keys from broadcast reads and broadcast-reads the winner's (x,y,z,k) from
//     an LDS mirror of the cloud kept in rank order: two dependent LDS trips.
// Round time on MI355X at B=32, N=4096 (512 threads x 8 points), scripts/fps_prod_lab.hip:
//   650 ns  first version (int compares + v_cndmask, DPP + v_readlane + ballot, 3 LDS trips)
//   557 ns  asm DPP ladder, broadcast select, -fno-slp-vectorize (hipcc's v_pk_* packing cost 11 %)
//   506 ns  64-bit rank keys (2 LDS trips), key low word formed in VALU
//   425 ns  v_max_f64 on the keys at all three levels
// Rejected after measurement: ds_max_u64 LDS atomics (~30 cycles per same-address op);
// scalar-unit resolution of lane/slot (SALU ops cost a 4-cycle issue slot); box-pruned
// updates over Morton-sorted 64-point regions (exact, but 784 ns: the per-slot scalar
// branches and a non-rank-ordered lane arg-max cost more than the skipped distances).
// The tiers that prune (fps_pruned_body.h, fps_batch_body.h), the rule that picks one and its geometry, and the step from that
// choice to a kernel are fps_tier.h's. Clouds too large for the register tiers fall back to a global-memory tier that keeps the
// running distances in the caller's `temp` buffer (or go to fps_large.hip).
#include "fps_tier.h"

#include <limits.h>

namespace pn2 {

template <int T, int P, bool LDSXYZ>
__global__ __launch_bounds__(T) void fps_reg_kernel(int n, int m, int Q, const float *__restrict__ xyz,
                                                    int *__restrict__ out, float *__restrict__ out_xyz)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fps_reg_body<T, P, LDSXYZ, false>(n, m, Q, blockIdx.x, xyz, out, out_xyz, nullptr, smem);
}

// the pruned and the batched tier (PrunedTier, BatchTier: fps_tier.h) on dense input
template <int P, int GS>
__global__ __launch_bounds__(kPrT) void fps_pruned_kernel(int n, int m, int Q, const float *__restrict__ xyz,
                                                          int *__restrict__ out, float *__restrict__ out_xyz)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fps_pruned_body<P, GS, false>(n, m, Q, blockIdx.x, xyz, out, out_xyz, nullptr, smem);
}

template <int P, int GS>
__global__ __launch_bounds__(kBtT) void fps_batch_kernel(int n, int m, int Q, const float *__restrict__ xyz,
                                                         int *__restrict__ out, float *__restrict__ out_xyz)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fps_batch_body<P, GS, false>(n, m, Q, blockIdx.x, xyz, out, out_xyz, nullptr, smem);
}

// Ragged batch on every tier (pn2_farthest_point_sample_ragged_variant; Pk = Packed: pn2_farthest_point_sample_packed). Cloud c
// holds n_c = lengths[c] <= n points in its padded (n, 3) slab -- or its rows of the flat array (FpsSlab, fps_body.h). The
// workgroup hands the tier's body its own slab as cloud 0 with n = n_c and Q = ceil(n_c / 512): every body takes (n, m, Q, cloud,
// xyz, ...) alike, so the tie ranks, the dealing and the padding slots are exactly those of the dense kernel on the slice, and
// rows at or beyond n_c are never addressed (fps_body.h: valid = ... && k < n; fps_pruned_prologue: k = i < n ? i : 0). The tier's
// template, thread count and LDS bytes come from the padded n (fps_choose): threads * P >= 512 ceil(n / 512) >= 512 Q_c, so every
// tie rank of the slice has a slot; the pruned and batched tiers deal the items i >= n_c as padding items at point 0's position
// (value 0, key low word 0). There a cloud may be ONE point in 8192 slots, where dense input fills at least half of a template:
// DESIGN.md 4.11 goes through the prologue, COLLECT, the picker's uncounted loop, the equal-keys rule, the value-0 tail, the
// slow-batch clock and the pruned tier's skipped reduction on such clouds, and through the termination of every wait inside the
// workgroup (tests/test_fps_batch_padding_model.py is the CPU model). n_c, m_c and Q_c are block-uniform scalars, so every wave
// of the workgroup -- the batched tier's picker included -- executes the barriers of the same chain.
// COUNTS, a sample count per cloud (pn2_farthest_point_sample_ragged_counts): cloud c yields m_c = npoints[c] samples. The body
// runs with m = m_c on the cloud's slab, so rows below m_c are the first m_c samples of the dense operator on the slice (the chain
// is prefix-consistent: round j depends on rounds < j alone). Rows m_c .. m-1 repeat sample 0, the way a ball query pads with its
// first hit; sample 0 is point 0 by the reference's rule (tf_sampling_g.cu:114-116), so the fill is index 0 and xyz[c, 0] and
// reads nothing back (fps_ragged_fill, fps_body.h). The fill rows are disjoint from the body's, so no barrier stands between the
// two. Without COUNTS npoints is never read. COUNTS on packed input (pn2_farthest_point_sample_packed_counts) composes the two: the
// slab from the offsets, m_c from npoints; under global_idx the fill index is the cloud's own first row, offsets[c].
template <class Tier, bool COUNTS, class... Pk>
__global__ __launch_bounds__(Tier::threads) void fps_ragged_kernel(int n, int m, const float *__restrict__ xyz, const int *__restrict__ lengths,
                                                                   const int *__restrict__ npoints, int *__restrict__ out,
                                                                   float *__restrict__ out_xyz, Pk... pk)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const FpsSlab s = fps_slab<COUNTS>(blockIdx.x, n, m, xyz, lengths, npoints, out, out_xyz, pk...);
    Tier::body(s.nc, s.mc, (s.nc + kRefThreads - 1) / kRefThreads, s.src, s.dst, s.dxyz, smem);
    if constexpr (sizeof...(Pk) != 0) fps_global_rows<Tier::threads>(s.mc, s.base, s.dst);
    if (COUNTS) fps_ragged_fill<Tier::threads>(s.mc, m, s.src, s.dst, s.dxyz, sizeof...(Pk) != 0 ? s.base : 0);
}

// ---------------------------------------------------------------------------
// Input that is ALREADY in farthest-point order (round 5; pn2_farthest_point_sample_ordered).
// The second and later levels of every network sample from the previous level's samples
// (pointnet2_sem_seg.py:28-31: l2 = sa(l1_xyz, ...)): the first m of them, in the order level 1 picked them, are a
// farthest-point order of the subset with the same fp32 running distances, so farthest_point_sample(m, new_xyz_1) is
// 0, 1, ..., m-1 -- unless the reference's tie rule (smallest (k mod 512, k), tf_sampling_g.cu:146,153-163), applied to the
// RENUMBERED points, breaks an exact tie the other way, or the cloud has run out of distinct points (every further sample
// is index 0). Whether it is the identity is decidable without the chain: sample i is selected at step i iff no other
// point j beats it there, i.e. iff for every j != i the running distance r_i(j) = min_{s<i} d(j, s) and the selection
// value v_i = r_i(i) satisfy (r_i(j), tie key j) < (v_i, tie key i). All r and v are prefix minima of the n x m distance
// matrix: n independent rows, no reduction. fps_verify_kernel evaluates them (parts x b workgroups) and flags a cloud on
// the first violation; the chain kernel behind it writes 0..m-1 for unflagged clouds and runs the real chain for
// flagged ones, so the result never depends on the guess.
// ---------------------------------------------------------------------------
constexpr int kVerT = 1024;
// a < b ? x : y as a bit select on a mask the compiler cannot see through (it turned the plain select into an exec-mask
// branch around the computation of x: one exposed LDS latency per step; a volatile barrier on x serialised the reads)
__device__ __forceinline__ float pick_lt(int a, int b, float x, float y)
{
    unsigned sel = (unsigned)((a - b) >> 31);                  // all ones when a < b (|a - b| < 2^31 here)
    asm("" : "+v"(sel));
    return __uint_as_float((__float_as_uint(x) & sel) | (__float_as_uint(y) & ~sel));
}
// Work decomposition: n x (m - 1) prefix-minimum entries per cloud would be m - 1 DEPENDENT steps per thread if a thread
// owned a row (60 us at m = 256: one LDS read + ten dependent vector instructions per step and nothing to overlap them with).
// A row is therefore cut into C chunks of L source samples (C a power of two <= 16, L ~ 32): chunk minima first, an exclusive
// minimum over the earlier chunks as the carry, then the chunk's own steps against the selection values -- 2 L dependent
// steps. A workgroup is C waves = C chunks x 64 points (sample reads are LDS broadcasts; small workgroups, because the work of
// a cloud is vector-issue bound on the CUs it lands on: 1024-thread workgroups measured 10.8 us at m = 128).
// The selection values v_i = r_i(i) are rows of the same matrix; every workgroup first rebuilds them for its cloud
// (triangular, the same chunks, LDS atomic minimum of the fp32 bit patterns: the values are >= 0) -- m^2 / 2 distance tests
// next to the workgroup's own 64 x 2 m, cheaper than a launch boundary.
__global__ __launch_bounds__(kVerT) void fps_verify_kernel(int n, int m, int C, int L, const float *__restrict__ xyz, int *__restrict__ flags)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *sm = reinterpret_cast<float4 *>(smem);             // [m]: x, y, z of sample e and the value sample e + 1 was selected with
    float *part = reinterpret_cast<float *>(sm + m);           // [C][64] chunk minima
    const int cloud = blockIdx.y, t = threadIdx.x;
    const float *__restrict__ src = xyz + (size_t)cloud * n * 3;
    const int T = C * 64;                                      // one wave per chunk, 64 points per workgroup
    for (int i = t; i < m; i += T)
        sm[i] = make_float4(src[(size_t)i * 3 + 0], src[(size_t)i * 3 + 1], src[(size_t)i * 3 + 2], 1e38f);   // 1e38: tf_sampling_g.cu:118
    __syncthreads();
    const int E = m - 1;                                       // source samples 0 .. m - 2 (the last sample updates nothing)
    // selection values: v_i = min_{e < i} d(i, e), i = 1 .. m - 1 (tf_sampling_g.cu:144)
    const int mpad = (m + 63) & ~63;
    for (int item = t; item < mpad * C; item += T) {
        // c is wave-uniform (mpad and the wave's first item are multiples of 64); the compiler is told so, the loops below are
        // scalar-controlled and hand-blocked by 8 (a runtime-bound loop is not unrolled for this target: one LDS read and ten
        // dependent instructions per step otherwise)
        const int c = __builtin_amdgcn_readfirstlane(item / mpad), i = item - c * mpad;
        const int e0 = c * L;
        const int eend = min(min(e0 + L, E), __builtin_amdgcn_readfirstlane(i | 63));   // no lane of the wave has a source at or beyond it
        if (e0 >= eend) continue;
        const float4 p = sm[min(i, m - 1)];
        float r = 1e38f;
        int eb = e0;
        for (; eb + 8 <= eend; eb += 8) {                        // whole blocks: eight independent LDS reads in flight
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float4 q = sm[eb + u];
                r = vmin_f32(pick_lt(eb + u, i, sqdist(p.x, p.y, p.z, q.x, q.y, q.z), 1e38f), r);
            }
        }
        for (; eb < eend; ++eb) {
            const float4 q = sm[eb];
            r = vmin_f32(pick_lt(eb, i, sqdist(p.x, p.y, p.z, q.x, q.y, q.z), 1e38f), r);
        }
        if (i >= 1 && i < m) atomicMin(reinterpret_cast<unsigned *>(&sm[i - 1].w), __float_as_uint(r));
    }
    __syncthreads();
    // every point against every step
    constexpr int JB = 64;
    const int c = __builtin_amdgcn_readfirstlane(t / JB), jl = t - c * JB;
    const int j = blockIdx.x * JB + jl;
    const bool live = j < n;
    const int jc = live ? j : 0;
    const float px = src[(size_t)jc * 3 + 0], py = src[(size_t)jc * 3 + 1], pz = src[(size_t)jc * 3 + 2];
    const int e0 = c * L, e1 = min(e0 + L, E);
    float r = 1e38f;
    if (C > 1) {                                               // kernel-uniform
        float a = 1e38f;
        int eb = e0;
        for (; eb + 8 <= e1; eb += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float4 q = sm[eb + u];
                a = vmin_f32(sqdist(px, py, pz, q.x, q.y, q.z), a);
            }
        }
        for (; eb < e1; ++eb) {
            const float4 q = sm[eb];
            a = vmin_f32(sqdist(px, py, pz, q.x, q.y, q.z), a);
        }
        part[c * JB + jl] = a;
        __syncthreads();
        for (int c2 = 0; c2 < c; ++c2) r = vmin_f32(part[c2 * JB + jl], r);
    }
    const unsigned tkj = ((unsigned)(j & (kRefThreads - 1)) << 22) | (unsigned)(j >> 9);
    // a coordinate that is not a finite number: v_min drops NaNs where the chain's arg-max sees them -- leave it to the chain
    int bad = !(__builtin_fabsf(px) <= 3.402823466e38f && __builtin_fabsf(py) <= 3.402823466e38f && __builtin_fabsf(pz) <= 3.402823466e38f);
    auto step = [&](int e) {
        const float4 q = sm[e];                                     // sample e and the value sample e + 1 was selected with
        r = vmin_f32(sqdist(px, py, pz, q.x, q.y, q.z), r);         // r_i(j), i = e + 1
        const int i = e + 1;
        const unsigned tki = ((unsigned)(i & (kRefThreads - 1)) << 22) | (unsigned)(i >> 9);
        bad |= (int)(j != i) & ~((int)(r < q.w) | ((int)(r == q.w) & (int)(tkj >= tki)));   // (value, key) order of tf_sampling_g.cu:146,153-163
    };
    int eb = e0;
    for (; eb + 8 <= e1; eb += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) step(eb + u);
    }
    for (; eb < e1; ++eb) step(eb);
    if (live && (bad & 1)) flags[cloud] = 1;
}

// chunks of ~32 source samples, at most 16 of them
static void fps_verify_shape(int m, int &C, int &L)
{
    const int E = m - 1;
    C = 1;
    while (C < 16 && C * 32 < E) C <<= 1;
    L = (E + C - 1) / C;
}

static int launch_verify(int b, int n, int m, const float *inp, int *flags, hipStream_t st)
{
    int C, L;
    fps_verify_shape(m, C, L);
    return launch(fps_verify_kernel, dim3((n + 63) / 64, b), dim3(C * 64), sizeof(float4) * (size_t)m + sizeof(float) * C * 64, st, n, m, C,
                  L, inp, flags);
}

// the chain behind the verifier: identity for unflagged clouds, the real chain (and a cleared flag) for the others
template <int P>
__global__ __launch_bounds__(256) void fps_reg_cond_kernel(int n, int m, int Q, const float *__restrict__ xyz, int *__restrict__ out,
                                                           float *__restrict__ out_xyz, int *__restrict__ flags)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int cloud = blockIdx.x, t = threadIdx.x;
    if (flags[cloud] == 0) {                                     // block-uniform
        int *__restrict__ dst = out + (size_t)cloud * m;
        for (int j = t; j < m; j += 256) dst[j] = j;
        if (out_xyz) {
            const float *__restrict__ src = xyz + (size_t)cloud * n * 3;
            float *__restrict__ d = out_xyz + (size_t)cloud * m * 3;
            for (int e = t; e < m * 3; e += 256) d[e] = src[e];
        }
        return;
    }
    fps_reg_body<256, P, true, false>(n, m, Q, cloud, xyz, out, out_xyz, nullptr, smem);
    if (t == 0) flags[cloud] = 0;                                // the workspace is left as it was found
}

// ---------------------------------------------------------------------------
// Generic tier: any n. Running distances in global `temp` (b*n floats), cloud
// re-read from global/L2 each round, 64-bit (value, tie-key) reduction.
// Slow path for clouds beyond the register tiers (n > 16384).
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m)
{
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// One cloud by one 1024-thread workgroup: n points at src, n running distances at mind, m samples to dst (and dxyz). n and m are
// workgroup-uniform (the dense kernel: the launch's; fps_generic_ragged_kernel: the cloud's own).
__device__ __forceinline__ void fps_generic_body(int n, int m, const float *__restrict__ src, float *__restrict__ mind,
                                                 int *__restrict__ dst, float *__restrict__ dxyz)
{
    constexpr int T = 1024, W = T / PN2_WAVE;
    __shared__ unsigned long long part[2][W];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int k = t; k < n; k += T) mind[k] = 1e38f;
    int cur = 0;
    if (t == 0) {
        dst[0] = 0;
        if (dxyz) { dxyz[0] = src[0]; dxyz[1] = src[1]; dxyz[2] = src[2]; }
    }
    // each thread only ever touches its own mind[k] (k = t mod T): no barrier needed for temp
    for (int j = 1; j < m; ++j) {
        const float sx = src[(size_t)cur * 3 + 0], sy = src[(size_t)cur * 3 + 1], sz = src[(size_t)cur * 3 + 2];
        unsigned long long best = 0ull;  // (value bits << 32) | ~tiekey ; real candidates are > 0
        for (int k = t; k < n; k += T) {
            const float d = sqdist(src[(size_t)k * 3 + 0], src[(size_t)k * 3 + 1], src[(size_t)k * 3 + 2], sx, sy, sz);
            const float d2 = __builtin_fminf(d, mind[k]);
            mind[k] = d2;
            const unsigned tiekey = ((unsigned)(k & (kRefThreads - 1)) << 22) | (unsigned)(k >> 9);
            const unsigned long long key =
                ((unsigned long long)(unsigned)__float_as_int(d2) << 32) | (unsigned long long)(0xFFFFFFFFu - tiekey);
            best = key > best ? key : best;
        }
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned long long o = shfl_xor_u64(best, s);
            best = o > best ? o : best;
        }
        if (lane == 0) part[j & 1][w] = best;
        __syncthreads();
        unsigned long long v = (lane < W) ? part[j & 1][lane] : 0ull;
#pragma unroll
        for (int s = 1; s < W; s <<= 1) {
            const unsigned long long o = shfl_xor_u64(v, s);
            v = o > v ? o : v;
        }
        const unsigned tiekey = 0xFFFFFFFFu - (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
        cur = (int)(((tiekey & 0x3FFFFFu) << 9) | (tiekey >> 22));
        if (t == 0) {
            dst[j] = cur;
            if (dxyz) {
                dxyz[j * 3 + 0] = src[(size_t)cur * 3 + 0];
                dxyz[j * 3 + 1] = src[(size_t)cur * 3 + 1];
                dxyz[j * 3 + 2] = src[(size_t)cur * 3 + 2];
            }
        }
    }
}

__global__ __launch_bounds__(1024) void fps_generic_kernel(int n, int m, const float *__restrict__ xyz,
                                                           float *__restrict__ temp, int *__restrict__ out,
                                                           float *__restrict__ out_xyz)
{
    const int cloud = blockIdx.x;
    fps_generic_body(n, m, xyz + (size_t)cloud * n * 3, temp + (size_t)cloud * n, out + (size_t)cloud * m,
                     out_xyz ? out_xyz + (size_t)cloud * m * 3 : nullptr);
}

// Ragged batch beyond the register tiers (pn2_farthest_point_sample_large_ragged, kernel 1): the slice rule of
// fps_ragged_kernel on the global-memory body. Slabs addressed with the padded n and m, the body run with n_c and m_c: every
// loop over the cloud is k < n_c (rows at or beyond n_c of the cloud and of temp are never addressed), a thread without a point
// contributes key 0, below every real key, and the one barrier per round sits in the loop j < m_c of workgroup-uniform bound.
// COUNTS: rows m_c .. m-1 are fps_ragged_fill's.
// Pk = Packed (pn2_farthest_point_sample_large_packed, kernel 1): the slab is the cloud's rows of the flat array and its running
// distances are the same rows of temp (total floats), so nothing is sized by b n; global_idx as in fps_ragged_kernel.
__device__ __forceinline__ float *fps_generic_temp(float *__restrict__ temp, int c, int n) { return temp + (size_t)c * n; }
__device__ __forceinline__ float *fps_generic_temp(float *__restrict__ temp, int c, int, Packed pk) { return temp + cloud_start(pk, c); }

template <bool COUNTS, class... Pk>
__global__ __launch_bounds__(1024) void fps_generic_ragged_kernel(int n, int m, const float *__restrict__ xyz, const int *__restrict__ lengths,
                                                                  const int *__restrict__ npoints, float *__restrict__ temp,
                                                                  int *__restrict__ out, float *__restrict__ out_xyz, Pk... pk)
{
    const int c = blockIdx.x;
    const FpsSlab s = fps_slab<COUNTS>(c, n, m, xyz, lengths, npoints, out, out_xyz, pk...);
    fps_generic_body(s.nc, s.mc, s.src, fps_generic_temp(temp, c, n, pk...), s.dst, s.dxyz);
    if constexpr (sizeof...(Pk) != 0) fps_global_rows<1024>(s.mc, s.base, s.dst);
    if (COUNTS) fps_ragged_fill<1024>(s.mc, m, s.src, s.dst, s.dxyz);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// the dense kernel of a tier
template <int T, int P, bool LDSXYZ>
static auto fps_dense_kernel(RegTier<T, P, LDSXYZ>) { return fps_reg_kernel<T, P, LDSXYZ>; }
template <int P, int GS>
static auto fps_dense_kernel(PrunedTier<P, GS>) { return fps_pruned_kernel<P, GS>; }
template <int P, int GS>
static auto fps_dense_kernel(BatchTier<P, GS>) { return fps_batch_kernel<P, GS>; }

// The three launches, each a function of the tier's tag (fps_with_tier). Dense: one workgroup per cloud of n points.
static auto fps_dense_launch(int b, int n, int m, int Q, const float *inp, int *out, float *oxyz, hipStream_t st)
{
    return [=](auto tier) { return launch_lds(fps_dense_kernel(tier), dim3(b), dim3(tier.threads), tier.lds, st, n, m, Q, inp, out, oxyz); };
}

// Ragged: npoints NULL = m samples from every cloud; else the per-cloud sample counts (COUNTS)
static auto fps_ragged_launch(int b, int n, int m, const float *inp, const int *lengths, const int *npoints, int *out, float *oxyz,
                              hipStream_t st)
{
    return [=](auto tier) {
        using Tier = decltype(tier);
        return launch_lds(npoints ? fps_ragged_kernel<Tier, true> : fps_ragged_kernel<Tier, false>, dim3(b), dim3(tier.threads), tier.lds, st,
                          n, m, inp, lengths, npoints, out, oxyz);
    };
}

// Packed: n is nmax; lengths is NULL and never read; npoints NULL = m samples from every cloud, else the per-cloud counts (COUNTS)
static auto fps_packed_launch(int b, int n, int m, const float *inp, Packed pk, const int *npoints, int *out, float *oxyz, hipStream_t st)
{
    return [=](auto tier) {
        using Tier = decltype(tier);
        return launch_lds(npoints ? fps_ragged_kernel<Tier, true, Packed> : fps_ragged_kernel<Tier, false, Packed>, dim3(b),
                          dim3(tier.threads), tier.lds, st, n, m, inp, nullptr, npoints, out, oxyz, pk);
    };
}

// the global-memory kernel with counts, for the ragged entry of fps_large.hip (declared there). npoints: NULL = m samples from
// every cloud; temp: (b, n) floats
int fps_launch_generic_ragged(int b, int n, int m, const float *inp, const int *lengths, const int *npoints, float *temp, int *out,
                              float *oxyz, hipStream_t st)
{
    return launch(npoints ? fps_generic_ragged_kernel<true> : fps_generic_ragged_kernel<false>, dim3(b), dim3(1024), 0, st, n, m, inp,
                  lengths, npoints, temp, out, oxyz);
}

// the same kernel in the packed mode, for the packed entry of fps_large.hip: n is nmax, temp pk.total floats
int fps_launch_generic_packed(int b, int n, int m, const float *inp, Packed pk, float *temp, int *out, float *oxyz, hipStream_t st)
{
    return launch(fps_generic_ragged_kernel<false, Packed>, dim3(b), dim3(1024), 0, st, n, m, inp, nullptr, nullptr, temp, out, oxyz, pk);
}

// Every (T, P) of the register tier, for the tuning harness (bench.py --fps-sweep; pn2_farthest_point_sample_ex): fps_choose
// names six of them.
template <int T, bool LDSXYZ, class F>
static int with_reg_p(int P, F f)
{
    switch (P) {
    case 1: return f(RegTier<T, 1, LDSXYZ>{});
    case 2: return f(RegTier<T, 2, LDSXYZ>{});
    case 4: return f(RegTier<T, 4, LDSXYZ>{});
    case 8: return f(RegTier<T, 8, LDSXYZ>{});
    case 16: return f(RegTier<T, 16, LDSXYZ>{});
    case 32:
        if constexpr (T <= 512) return f(RegTier<T, 32, LDSXYZ>{});
        break;
    default: break;
    }
    return PN2_E_ARG;
}

static int fps_launch_config(int T, int P, int b, int n, int m, const float *inp, int *out, float *oxyz,
                             hipStream_t st)
{
    const int Q = (n + kRefThreads - 1) / kRefThreads;
    if ((long long)T * P < (long long)kRefThreads * Q) return PN2_E_ARG;
    const bool lds = (long long)T * P <= kMaxLdsSlots;
    const auto go = fps_dense_launch(b, n, m, Q, inp, out, oxyz, st);
    switch (T) {
    case 256: return lds ? with_reg_p<256, true>(P, go) : with_reg_p<256, false>(P, go);
    case 512: return lds ? with_reg_p<512, true>(P, go) : with_reg_p<512, false>(P, go);
    case 1024: return lds ? with_reg_p<1024, true>(P, go) : with_reg_p<1024, false>(P, go);
    default: return PN2_E_ARG;
    }
}

template <int P>
static int launch_cond(int b, int n, int m, int Q, const float *inp, int *out, float *oxyz, int *flags, hipStream_t st)
{
    return launch_lds(fps_reg_cond_kernel<P>, dim3(b), dim3(256), RegTier<256, P, true>::lds, st, n, m, Q, inp, out, oxyz, flags);
}

}  // namespace pn2

extern "C" long long pn2_fps_temp_floats(int b, int n)
{
    if (b <= 0 || n <= 0) return 0;
    return n > pn2::kMaxRegPoints ? (long long)b * n : 0;
}

static int fps_entry(int b, int n, int m, const float *inp, float *temp, int *out, float *out_xyz, void *stream,
                     int variant = PN2_FPS_AUTO)
{
    using namespace pn2;
    if (m <= 0 || b == 0) return PN2_OK;          // tf_sampling_g.cu:106
    if (b < 0 || n <= 0) return PN2_E_SHAPE;
    if (!inp || !out) return PN2_E_NULL;
    if ((long long)b * n * 3 > INT_MAX || (long long)b * m * 3 > INT_MAX) return PN2_E_TOO_LARGE;
    hipStream_t st = as_stream(stream);
    if (n > kMaxRegPoints) {
        if (!temp) return PN2_E_NULL;
        if (int rc = launch(fps_generic_kernel, dim3(b), dim3(1024), 0, st, n, m, inp, temp, out, out_xyz)) return rc;
        return PN2_OK;
    }
    FpsChoice c;
    if (int rc = fps_choose(variant, n, m, c)) return rc;
    return fps_with_tier(c, fps_dense_launch(b, n, m, c.Q, inp, out, out_xyz, st));
}

extern "C" int pn2_farthest_point_sample(int b, int n, int m, const float *inp, float *temp, int *out, void *stream)
{
    return fps_entry(b, n, m, inp, temp, out, nullptr, stream);
}

extern "C" int pn2_farthest_point_sample_gather(int b, int n, int m, const float *inp, float *temp, int *out,
                                                float *out_xyz, void *stream)
{
    if (m > 0 && b > 0 && !out_xyz) return PN2_E_NULL;
    return fps_entry(b, n, m, inp, temp, out, out_xyz, stream);
}

// Same operator with the tier chosen by the caller (tests, A/B timing; results never depend on it): PN2_FPS_AUTO = the
// size rule of pn2_farthest_point_sample, PN2_FPS_FULL = every point updated every round (fps_reg_body), PN2_FPS_PRUNED =
// the kd-grouped tier (PN2_E_ARG outside 2049..8192 rank slots). out_xyz may be NULL.
extern "C" int pn2_farthest_point_sample_variant(int variant, int b, int n, int m, const float *inp, float *temp, int *out,
                                                 float *out_xyz, void *stream)
{
    if (variant < PN2_FPS_AUTO || variant > PN2_FPS_BATCH) return PN2_E_ARG;
    return fps_entry(b, n, m, inp, temp, out, out_xyz, stream, variant);
}

// Ragged batch: cloud c is inp[c, :lengths[c]] of a padded (b, n, 3) tensor, lengths (b) int32 on the device, never read by
// the host. Result per cloud = pn2_farthest_point_sample_gather on the slice, tie rule included, whatever the tier. The tier is
// fps_choose's at the PADDED n and m, as for dense input. PN2_E_TOO_LARGE beyond 16384 points. out_xyz may be NULL.
// pk: the packed mode (pn2_farthest_point_sample_packed): n is nmax, the flat array's extent is pk->total, lengths / npoints NULL.
static int fps_ragged_entry(int b, int n, int m, const float *inp, const int *lengths, const int *npoints, bool counts, int *out,
                            float *out_xyz, void *stream, int variant = PN2_FPS_AUTO, const pn2::Packed *pk = nullptr)
{
    using namespace pn2;
    if (m <= 0 || b == 0) return PN2_OK;
    if (b < 0 || n <= 0 || (pk && pk->total <= 0)) return PN2_E_SHAPE;
    if (!inp || !out || !(pk ? pk->offsets : lengths) || (counts && !npoints)) return PN2_E_NULL;
    if (n > kMaxRegPoints) return PN2_E_TOO_LARGE;
    if ((pk ? (long long)pk->total : (long long)b * n) * 3 > INT_MAX || (long long)b * m * 3 > INT_MAX) return PN2_E_TOO_LARGE;
    hipStream_t st = as_stream(stream);
    FpsChoice c;
    if (int rc = fps_choose(variant, n, m, c)) return rc;
    if (pk) return fps_with_tier(c, fps_packed_launch(b, n, m, inp, *pk, npoints, out, out_xyz, st));
    return fps_with_tier(c, fps_ragged_launch(b, n, m, inp, lengths, npoints, out, out_xyz, st));
}

extern "C" int pn2_farthest_point_sample_ragged(int b, int n, int m, const float *inp, const int *lengths, int *out, float *out_xyz,
                                                void *stream)
{
    return fps_ragged_entry(b, n, m, inp, lengths, nullptr, false, out, out_xyz, stream);
}

// The same with a sample count per cloud: cloud c yields m_c = npoints[c] samples (b int32 on the device, clamped into 1..m,
// never read by the host). Rows below m_c = the first m_c samples of pn2_farthest_point_sample_gather on the slice; rows
// m_c .. m-1 repeat sample 0 (index 0, the cloud's first point). Codes and envelope of pn2_farthest_point_sample_ragged.
extern "C" int pn2_farthest_point_sample_ragged_counts(int b, int n, int m, const float *inp, const int *lengths, const int *npoints,
                                                       int *out, float *out_xyz, void *stream)
{
    return fps_ragged_entry(b, n, m, inp, lengths, npoints, true, out, out_xyz, stream);
}

// Both ragged entries with the tier chosen by the caller (tests, A/B timing; results never depend on it): variant as in
// pn2_farthest_point_sample_variant, the size rule on the padded n and m; npoints NULL = m samples from every cloud. The two
// entries above are its PN2_FPS_AUTO case.
extern "C" int pn2_farthest_point_sample_ragged_variant(int variant, int b, int n, int m, const float *inp, const int *lengths,
                                                        const int *npoints, int *out, float *out_xyz, void *stream)
{
    if (variant < PN2_FPS_AUTO || variant > PN2_FPS_BATCH) return PN2_E_ARG;
    return fps_ragged_entry(b, n, m, inp, lengths, npoints, false, out, out_xyz, stream, variant);
}

// Packed batch: cloud c is inp[offsets[c] : offsets[c + 1]] of a flat (total, 3) array, offsets (b + 1) int32 on the device, never
// read by the host; nmax bounds every cloud's count and takes the padded n's place in the tier rule, the template and the LDS
// size. Result per cloud = pn2_farthest_point_sample_gather on the slice, whatever the tier; global_idx 1 adds offsets[c] to the
// cloud's indices. out (b, m) and out_xyz (b, m, 3, may be NULL) are dense. variant, codes and envelope as
// pn2_farthest_point_sample_ragged_variant (PN2_E_TOO_LARGE for nmax > 16384 or total 3 > INT_MAX).
extern "C" int pn2_farthest_point_sample_packed(int variant, int b, int total, int nmax, int m, const float *inp, const int *offsets,
                                                int global_idx, int *out, float *out_xyz, void *stream)
{
    if (variant < PN2_FPS_AUTO || variant > PN2_FPS_BATCH) return PN2_E_ARG;
    const pn2::Packed pk = {offsets, total, global_idx ? 1 : 0};
    return fps_ragged_entry(b, nmax, m, inp, nullptr, nullptr, false, out, out_xyz, stream, variant, &pk);
}

// The same with a sample count per cloud, as pn2_farthest_point_sample_ragged_counts: cloud c yields m_c = npoints[c] samples
// ((b) int32 on the device, clamped into 1..m, never read by the host). Rows below m_c = the first m_c samples of
// pn2_farthest_point_sample_gather on the slice = pn2_farthest_point_sample_ragged_counts on the padded copy; rows m_c .. m-1
// repeat sample 0: index 0 (offsets[c] under global_idx) and the cloud's first point. npoints is required; codes and envelope of
// pn2_farthest_point_sample_packed (PN2_E_TOO_LARGE for nmax > 16384).
extern "C" int pn2_farthest_point_sample_packed_counts(int variant, int b, int total, int nmax, int m, const float *inp,
                                                       const int *offsets, const int *npoints, int global_idx, int *out, float *out_xyz,
                                                       void *stream)
{
    if (variant < PN2_FPS_AUTO || variant > PN2_FPS_BATCH) return PN2_E_ARG;
    const pn2::Packed pk = {offsets, total, global_idx ? 1 : 0};
    return fps_ragged_entry(b, nmax, m, inp, nullptr, npoints, true, out, out_xyz, stream, variant, &pk);
}

// farthest_point_sample for input the caller BELIEVES to be in farthest-point order already (the previous level's samples:
// pointnet2_sem_seg.py:28-31, pointnet2_cls_ssg.py:27-29): verified in parallel, the chain runs only for clouds where the
// belief is wrong -- the result is pn2_farthest_point_sample's whatever the input is. ws: pn2_fps_ordered_ws_bytes(b) bytes,
// zeroed by the caller ONCE (every call leaves it zeroed). Outside 2 <= m <= min(n, 1024), n <= 2048 there is nothing to
// gain and the call is pn2_farthest_point_sample_gather / pn2_farthest_point_sample (PN2_E_TOO_LARGE beyond the register
// tiers, where that operator needs its temp buffer). out_xyz may be NULL.
extern "C" long long pn2_fps_ordered_ws_bytes(int b) { return b > 0 ? (long long)b * 4 : 0; }

extern "C" int pn2_farthest_point_sample_ordered(int b, int n, int m, const float *inp, int *out, float *out_xyz, void *ws,
                                                 void *stream)
{
    using namespace pn2;
    if (m <= 0 || b == 0) return PN2_OK;
    if (b < 0 || n <= 0) return PN2_E_SHAPE;
    if (!inp || !out) return PN2_E_NULL;
    if (n > kMaxRegPoints) return PN2_E_TOO_LARGE;
    if (m < 2 || m > n || m > 1024 || n > 2048) return fps_entry(b, n, m, inp, nullptr, out, out_xyz, stream);
    if (b > 65535) return fps_entry(b, n, m, inp, nullptr, out, out_xyz, stream);   // beyond the check launch's grid.y: the plain operator (same result)
    if (!ws) return PN2_E_NULL;
    hipStream_t st = as_stream(stream);
    int *flags = static_cast<int *>(ws);
    if (int rc = launch_verify(b, n, m, inp, flags, st)) return rc;
    FpsChoice c;                                           // the register tier's geometry at n <= 2048: 256 threads
    if (int rc = fps_choose(PN2_FPS_FULL, n, m, c)) return rc;
    switch (c.T == 256 ? c.P : 0) {
    case 2: return launch_cond<2>(b, n, m, c.Q, inp, out, out_xyz, flags, st);
    case 4: return launch_cond<4>(b, n, m, c.Q, inp, out, out_xyz, flags, st);
    case 8: return launch_cond<8>(b, n, m, c.Q, inp, out, out_xyz, flags, st);
    default: return PN2_E_ARG;
    }
}

// test hook: the verifier of pn2_farthest_point_sample_ordered alone. flags (b ints, zeroed by the caller) comes back 1 for the
// clouds whose farthest-point sampling is NOT 0 .. m-1 (exactly those: the first violated step is where the chain leaves the
// identity). Same envelope as the short cut: 2 <= m <= min(n, 1024), n <= 2048.
extern "C" int pn2_fps_ordered_check(int b, int n, int m, const float *inp, int *flags, void *stream)
{
    using namespace pn2;
    if (b <= 0 || !inp || !flags) return PN2_E_ARG;
    if (m < 2 || m > n || m > 1024 || n > 2048 || b > 65535) return PN2_E_ARG;
    return launch_verify(b, n, m, inp, flags, as_stream(stream));
}

// tuning / test hook: run the register tier with an explicit geometry
extern "C" int pn2_farthest_point_sample_ex(int T, int P, int b, int n, int m, const float *inp, int *out, void *stream)
{
    if (m <= 0 || b <= 0 || n <= 0 || !inp || !out) return PN2_E_ARG;
    if (n > pn2::kMaxRegPoints) return PN2_E_TOO_LARGE;
    return pn2::fps_launch_config(T, P, b, n, m, inp, out, nullptr, pn2::as_stream(stream));
}
