// fps_large.hip -- farthest point sampling for clouds of 16385 .. 1048576 points: exact spatial pruning over a cell-sorted copy
// of the cloud.
//
// Same results as fps_generic_kernel (fps.hip) / the reference kernel (tf_sampling_g.cu:105-170), index for index, tie rule
// included (smallest (k mod 512, k) among equal running distances). What changes is how much of a round is done. The generic
// kernel updates the running distance of EVERY point against the new sample: n distance tests, n running distances read and
// written in global memory, per round. But a new sample can only lower running distances inside the ball of radius
// sqrt(v*) around it (v* = the value that just won the arg-max; fps_pruned_body.h), and on a large cloud that ball holds a
// few per cent of the points after a few dozen samples.
//
// Organisation. One 1024-thread workgroup per cloud, one launch, nothing waits on another workgroup.
//   Prologue (passes over the cloud): bounding box; an LDS histogram over a 32 x 32 x 32 cell grid in Morton order; exclusive
//   prefix sums; a scatter with returning LDS atomics that writes the cloud into the workspace in cell order as 16-byte
//   records {x, y, z, original index k}. The sorted order is cut into GROUPS of L consecutive records (L = 64, 128 or 256); a
//   Morton run of cells is a compact blob whatever the local density, so a group's tight bounding box is small. The order of
//   the records inside a cell is the order of the atomics, i.e. timing dependent -- and irrelevant: any partition gives the
//   same samples (fps_pruned_body.h), a compact one gives more skips.
//   Ownership. Group g belongs to wave g mod 16; lane l of that wave owns the records g L + l + 64 r (r < L / 64), so every
//   running distance is only ever read and written by ONE thread (as in the generic kernel) and no barrier or fence guards the
//   distance array. Lane l of wave w also holds, in registers, the box and the cached key of the wave's groups number l,
//   l + 64, l + 128, l + 192 (at most 4096 groups = 256 per wave).
//   Chain, per round: every lane tests its (up to four) boxes against the new sample -- the pruned tier's rule, bd >= v* *
//   1.00001f + 1e-30f means "cannot change" --, a ballot per box slot gives the wave its touched groups, and the wave walks them:
//   L / 64 records per lane, sqdist, __builtin_fminf, the generic kernel's 64-bit key (value bits : 0xFFFFFFFF - tie key), a
//   wave-wide maximum = the group's new key, cached by the owning lane. The coordinates of a group's best record go to an LDS
//   table only its own wave touches. The wave key is the maximum of the cached group keys (recomputed only when a group
//   changed); the lane that owns the winning group publishes (key, x, y, z) in the wave's LDS slot. One __syncthreads() per
//   round; behind it every thread reads the 16 wave keys and the winner's coordinates from LDS: the winner never costs a
//   dependent global-memory load. Slots are double buffered by the round's parity, as in the generic kernel.
// Exactness: the skip rule and its proof are those of fps_pruned_body.h (header comment there); groups that are not skipped
// compute exactly the generic kernel's values, and the arg-max over cached keys is the arg-max over all records because an
// untouched group's records -- hence its key -- did not change.
// Ragged batches (lengths / npoints on the device): the chain is a body that takes one cloud's extents; fps_large_ragged_kernel
// runs it on each cloud's slice (pn2_farthest_point_sample_large_ragged).
// Packed batches (offsets on the device): fps_large_packed_kernel runs the same body on the cloud's rows of the flat array and
// of the workspace, and a short-cloud body (fps_large_short_body) on clouds of at most 8192 points
// (pn2_farthest_point_sample_large_packed).
#include "fps_body.h"

#include <limits.h>
#include <math.h>

namespace pn2 {

constexpr int kLgT = 1024;                       // threads: 16 waves, the chain stays inside one CU
constexpr int kLgW = kLgT / PN2_WAVE;
constexpr int kLgMinPoints = 16384;              // exclusive: up to here the register tiers
constexpr int kLgMaxPoints = 1 << 20;
constexpr int kLgMaxGroups = 4096;               // box + key slots: four per lane
constexpr int kLgNB = kLgMaxGroups / kLgW / PN2_WAVE;
constexpr int kLgAxisCells = 32;                 // cells per axis
constexpr int kLgCells = kLgAxisCells * kLgAxisCells * kLgAxisCells;
constexpr int kLgCellsPerThread = kLgCells / kLgT;
// LDS (bytes): [0, 128 Ki) the cell histogram of the prologue, afterwards its first 64 KiB = best-record coordinates per group |
// wave keys [2][16] u64 | wave coordinates [2][16] float4 | bounding-box partials [16][8] f32 | scan totals [16] i32
constexpr size_t kLgHistBytes = (size_t)kLgCells * 4;
constexpr size_t kLgKeyOff = kLgHistBytes, kLgXyzOff = kLgKeyOff + 256, kLgRedOff = kLgXyzOff + 512, kLgTotOff = kLgRedOff + 512;
constexpr size_t kLgLdsBytes = kLgTotOff + 64;
static_assert((size_t)kLgMaxGroups * 16 <= kLgHistBytes && kLgLdsBytes <= 160 * 1024, "LDS layout");
static_assert(kLgNB == 4, "four box slots per lane");

__device__ __forceinline__ unsigned long long lg_shfl_xor_u64(unsigned long long v, int m)
{
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// wave-wide maximum, in every lane
__device__ __forceinline__ unsigned long long lg_wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long o = lg_shfl_xor_u64(v, s);
        v = o > v ? o : v;
    }
    return v;
}

template <bool MAX>
__device__ __forceinline__ float lg_wave_minmax(float v)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const float o = __shfl_xor(v, s, 64);
        v = MAX ? fmaxf(v, o) : fminf(v, o);
    }
    return v;
}

// bin of a coordinate along one axis: 0 .. 31, NaN and everything out of range included (fmaxf(NaN, 0) = 0)
__device__ __forceinline__ unsigned lg_axis_bin(float c, float lo, float scale)
{
    const float f = fminf(fmaxf(__fmul_rn(__fsub_rn(c, lo), scale), 0.0f), (float)(kLgAxisCells - 1));
    return (unsigned)(int)f;
}

// five bits to every third bit
__device__ __forceinline__ unsigned lg_spread5(unsigned v)
{
    return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6) | ((v & 16u) << 8);
}

struct LgGrid {
    float lx, ly, lz, sx, sy, sz;
};

__device__ __forceinline__ int lg_cell(const LgGrid &gr, float x, float y, float z)
{
    return (int)((lg_spread5(lg_axis_bin(x, gr.lx, gr.sx)) << 2) | (lg_spread5(lg_axis_bin(y, gr.ly, gr.sy)) << 1) |
                 lg_spread5(lg_axis_bin(z, gr.lz, gr.sz)));
}

struct LgBox {
    float lx, ly, lz, hx, hy, hz;
};

// The records of one group as its wave holds them: lane l has records base + l + 64 r (those below n exist).
template <int R>
struct LgRecs {
    float4 p[R];
    float d0[R];
};

// every load in flight before the first use; a missing record re-reads the cloud's last one (never used)
template <int R, bool INIT>
__device__ __forceinline__ void lg_group_load(int n, int g, int lane, const float4 *recs, const float *md, LgRecs<R> &q)
{
    const int base = g * (R * 64) + lane;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = min(base + r * 64, n - 1);
        q.p[r] = recs[i];
        q.d0[r] = INIT ? 1e38f : md[i];
    }
}

// One pass of a wave over ONE group, behind lg_group_load: returns the group's key in every lane and leaves the coordinates of
// the record that holds it in best[g]. INIT: the running distances are set to the reference's start value 1e38
// (tf_sampling_g.cu:118) and the group's tight box is computed; else they are lowered against the sample (sx, sy, sz).
template <int R, bool INIT>
__device__ __forceinline__ unsigned long long lg_group_finish(int n, int g, int lane, const LgRecs<R> &q, float *md, float sx,
                                                              float sy, float sz, float4 *best, LgBox &box)
{
    const int base = g * (R * 64) + lane;
    unsigned long long lk = 0ull;
    float bx = 0.0f, by = 0.0f, bz = 0.0f, bw = 0.0f;
    if (INIT) {
        box.lx = box.ly = box.lz = INFINITY;
        box.hx = box.hy = box.hz = -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = base + r * 64;
        const bool real = i < n;
        const float4 p = q.p[r];
        float d2;
        if (INIT) {
            d2 = 1e38f;
            if (real) {
                box.lx = fminf(box.lx, p.x); box.ly = fminf(box.ly, p.y); box.lz = fminf(box.lz, p.z);
                box.hx = fmaxf(box.hx, p.x); box.hy = fmaxf(box.hy, p.y); box.hz = fmaxf(box.hz, p.z);
            }
        } else {
            d2 = __builtin_fminf(sqdist(p.x, p.y, p.z, sx, sy, sz), q.d0[r]);              // min(d, td), tf_sampling_g.cu:144
        }
        if (real) md[i] = d2;
        const unsigned k = (unsigned)__float_as_int(p.w);
        const unsigned tiekey = ((k & (unsigned)(kRefThreads - 1)) << 22) | (k >> 9);
        const unsigned long long key = real ? ((unsigned long long)(unsigned)__float_as_int(d2) << 32) | (unsigned long long)(0xFFFFFFFFu - tiekey)
                                            : 0ull;
        if (key > lk) { lk = key; bx = p.x; by = p.y; bz = p.z; bw = p.w; }
    }
    const unsigned long long gkey = lg_wave_max_u64(lk);
    if (lk == gkey && gkey != 0ull) best[g] = make_float4(bx, by, bz, bw);                 // keys are unique: one lane
    if (INIT) {
        box.lx = lg_wave_minmax<false>(box.lx); box.ly = lg_wave_minmax<false>(box.ly); box.lz = lg_wave_minmax<false>(box.lz);
        box.hx = lg_wave_minmax<true>(box.hx); box.hy = lg_wave_minmax<true>(box.hy); box.hz = lg_wave_minmax<true>(box.hz);
    }
    return gkey;
}

// The whole chain of ONE cloud by one workgroup: n points at src, their records and running distances at recs / md (n entries
// each), m samples to dst (and dxyz). n and m are workgroup-uniform; nothing else about them is assumed, so the dense kernel
// passes the launch's extents and the ragged kernel a cloud's own (fps_large_ragged_kernel below goes through what that needs).
template <int L, bool SHORT>
__device__ __forceinline__ void fps_large_body(int n, int m, const float *__restrict__ src, float4 *__restrict__ recs,
                                               float *__restrict__ md, int *__restrict__ dst, float *__restrict__ dxyz, char *smem)
{
    constexpr int T = kLgT, W = kLgW, NB = kLgNB, R = L / 64;
    static_assert(L == 64 || L == 128 || L == 256, "records per group");
    int *hist = reinterpret_cast<int *>(smem);
    float4 *best = reinterpret_cast<float4 *>(smem);                                       // [groups], after the prologue
    unsigned long long *skey = reinterpret_cast<unsigned long long *>(smem + kLgKeyOff);   // [2][W]
    float4 *sxyz = reinterpret_cast<float4 *>(smem + kLgXyzOff);                            // [2][W]
    float *red = reinterpret_cast<float *>(smem + kLgRedOff);                               // [W][8]
    int *wtot = reinterpret_cast<int *>(smem + kLgTotOff);                                  // [W]

    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);

    float sx = src[0], sy = src[1], sz = src[2];           // the first sample is point 0 (tf_sampling_g.cu:114-116)
    if (t == 0) {
        dst[0] = 0;
        if (dxyz) { dxyz[0] = sx; dxyz[1] = sy; dxyz[2] = sz; }
    }
    if (m == 1) return;                                    // workgroup-uniform, before any barrier

    // ---- prologue 1: bounding box -------------------------------------------------------------------------------------------
    LgGrid gr;
    {
        float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
        for (int k = t; k < n; k += T) {
            const float x = src[(size_t)k * 3 + 0], y = src[(size_t)k * 3 + 1], z = src[(size_t)k * 3 + 2];
            lx = fminf(lx, x); ly = fminf(ly, y); lz = fminf(lz, z);
            hx = fmaxf(hx, x); hy = fmaxf(hy, y); hz = fmaxf(hz, z);
        }
        lx = lg_wave_minmax<false>(lx); ly = lg_wave_minmax<false>(ly); lz = lg_wave_minmax<false>(lz);
        hx = lg_wave_minmax<true>(hx); hy = lg_wave_minmax<true>(hy); hz = lg_wave_minmax<true>(hz);
        if (lane == 0) {
            red[w * 8 + 0] = lx; red[w * 8 + 1] = ly; red[w * 8 + 2] = lz;
            red[w * 8 + 4] = hx; red[w * 8 + 5] = hy; red[w * 8 + 6] = hz;
        }
        for (int c = t; c < kLgCells; c += T) hist[c] = 0;
        // SHORT (clouds that may have fewer than 16 groups: a ragged batch; dense input has 65 or more): a wave without a group
        // never publishes, and every thread reads all 16 slots of a round -- such a slot holds 0, below every real key, throughout.
        if (SHORT && t < 2 * W) skey[t] = 0ull;
        __syncthreads();
        float lo[3], sc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float l = red[a], h = red[4 + a];
#pragma unroll
            for (int ww = 1; ww < W; ++ww) { l = fminf(l, red[ww * 8 + a]); h = fmaxf(h, red[ww * 8 + 4 + a]); }
            const float e = __fsub_rn(h, l);
            const bool ok = e > 0.0f && e < INFINITY;       // degenerate / non-finite axis: every point in bin 0
            const float s = ok ? (float)kLgAxisCells / e : 0.0f;
            lo[a] = ok ? l : 0.0f;
            sc[a] = s < INFINITY ? s : 0.0f;                // an extent so small that the scale overflows: bin 0 as well
        }
        gr.lx = lo[0]; gr.ly = lo[1]; gr.lz = lo[2];
        gr.sx = sc[0]; gr.sy = sc[1]; gr.sz = sc[2];
    }

    // ---- prologue 2: histogram over the cells, exclusive prefix sums --------------------------------------------------------
    for (int k = t; k < n; k += T)
        atomicAdd(&hist[lg_cell(gr, src[(size_t)k * 3 + 0], src[(size_t)k * 3 + 1], src[(size_t)k * 3 + 2])], 1);
    __syncthreads();
    {
        int *mine = hist + t * kLgCellsPerThread;           // thread t scans cells 32 t .. 32 t + 31
        int sum = 0;
#pragma unroll 8
        for (int c = 0; c < kLgCellsPerThread; ++c) sum += mine[c];
        int incl = sum;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int o = __shfl_up(incl, s, 64);
            if (lane >= s) incl += o;
        }
        if (lane == 63) wtot[w] = incl;
        __syncthreads();
        int run = incl - sum;
        for (int ww = 0; ww < w; ++ww) run += wtot[ww];
#pragma unroll 8
        for (int c = 0; c < kLgCellsPerThread; ++c) {
            const int h = mine[c];
            mine[c] = run;
            run += h;
        }
    }
    __syncthreads();

    // ---- prologue 3: scatter into cell order (a returning atomic hands out the places of a cell) ----------------------------
    for (int k = t; k < n; k += T) {
        const float x = src[(size_t)k * 3 + 0], y = src[(size_t)k * 3 + 1], z = src[(size_t)k * 3 + 2];
        const int at = atomicAdd(&hist[lg_cell(gr, x, y, z)], 1);
        if ((unsigned)at < (unsigned)n) recs[at] = make_float4(x, y, z, __int_as_float(k));   // always: same cells as the histogram pass
    }
    __syncthreads();                                        // the records are visible to the workgroup; the histogram is dead

    // ---- prologue 4: boxes, start distances and start keys of this wave's groups --------------------------------------------
    const int G = (n + L - 1) / L;
    unsigned long long gk[NB];                              // lane l, slot i: group w + 16 (l + 64 i); 0 = no such group
    LgBox gb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        gk[i] = 0ull;
        gb[i].lx = gb[i].ly = gb[i].lz = gb[i].hx = gb[i].hy = gb[i].hz = 0.0f;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        for (int bit = 0; bit < 64; ++bit) {
            const int g = w + W * (i * 64 + bit);
            if (g >= G) break;                              // wave-uniform
            LgBox bx;
            LgRecs<R> q;
            lg_group_load<R, true>(n, g, lane, recs, md, q);
            const unsigned long long k = lg_group_finish<R, true>(n, g, lane, q, md, 0.0f, 0.0f, 0.0f, best, bx);
            if (lane == bit) { gk[i] = k; gb[i] = bx; }
        }
    }
    unsigned long long wave_key;
    {
        unsigned long long lk = gk[0];
#pragma unroll
        for (int i = 1; i < NB; ++i) lk = gk[i] > lk ? gk[i] : lk;
        wave_key = lg_wave_max_u64(lk);
    }

    // ---- the chain ----------------------------------------------------------------------------------------------------------
    float vstar = 1e38f;                                    // every running distance is <= vstar
    for (int j = 1; j < m; ++j) {
        const int par = j & 1;
        const float thr = __fadd_rn(__fmul_rn(vstar, 1.00001f), 1e-30f);
        bool touched = false;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (w + W * (i * 64) >= G) break;               // wave-uniform: no group in this slot or the later ones
            // distance from the sample to the box = sample - clamp(sample, lo, hi) per axis (v_med3_f32 is the clamp)
            const float ax = __fsub_rn(sx, __builtin_amdgcn_fmed3f(sx, gb[i].lx, gb[i].hx));
            const float ay = __fsub_rn(sy, __builtin_amdgcn_fmed3f(sy, gb[i].ly, gb[i].hy));
            const float az = __fsub_rn(sz, __builtin_amdgcn_fmed3f(sz, gb[i].lz, gb[i].hz));
            const float bd = __fadd_rn(__fadd_rn(__fmul_rn(ax, ax), __fmul_rn(ay, ay)), __fmul_rn(az, az));
            unsigned long long todo = __ballot(!(bd >= thr) && gk[i] != 0ull);             // NaN -> not far -> updated
            if (todo != 0ull) {                             // wave-uniform
                // scalar loop over the touched groups; the next group's records are requested before this one's are used
                touched = true;
                int bit = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                LgRecs<R> q;
                lg_group_load<R, false>(n, w + W * (i * 64 + bit), lane, recs, md, q);
                for (;;) {
                    const bool more = todo != 0ull;
                    int nbit = 0;
                    LgRecs<R> qn;
                    if (more) {
                        nbit = __builtin_ctzll(todo);
                        todo &= todo - 1ull;
                        lg_group_load<R, false>(n, w + W * (i * 64 + nbit), lane, recs, md, qn);
                    }
                    LgBox unused;
                    const unsigned long long k = lg_group_finish<R, false>(n, w + W * (i * 64 + bit), lane, q, md, sx, sy, sz, best, unused);
                    if (lane == bit) gk[i] = k;
                    if (!more) break;
                    q = qn;
                    bit = nbit;
                }
            }
        }
        if (touched) {                                      // wave-uniform; else the cached wave key stands
            unsigned long long lk = gk[0];
#pragma unroll
            for (int i = 1; i < NB; ++i) lk = gk[i] > lk ? gk[i] : lk;
            wave_key = lg_wave_max_u64(lk);
        }
        // the lane that owns the wave's best group publishes (key, coordinates of its best record)
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (gk[i] == wave_key && wave_key != 0ull) {
                skey[par * W + w] = wave_key;
                sxyz[par * W + w] = best[w + W * (i * 64 + lane)];
            }
        }
        __syncthreads();
        unsigned long long bk = skey[par * W];
        int bwv = 0;
#pragma unroll
        for (int ww = 1; ww < W; ++ww) {
            const unsigned long long k = skey[par * W + ww];
            if (k > bk) { bk = k; bwv = ww; }
        }
        const float4 s = sxyz[par * W + bwv];               // same address in every lane: LDS broadcast
        sx = s.x; sy = s.y; sz = s.z;
        vstar = __int_as_float((int)(unsigned)(bk >> 32));
        if (t == 0) {
            dst[j] = __float_as_int(s.w);
            if (dxyz) { dxyz[j * 3 + 0] = s.x; dxyz[j * 3 + 1] = s.y; dxyz[j * 3 + 2] = s.z; }
        }
    }
}

// A cloud of at most kLgShortCap points inside a launch of this tier (a packed batch whose nmax is large: fps_large_packed_kernel):
// no cell sort, no records, no running distances in global memory -- recs / md are not even arguments. The cloud lies in the
// 128 KiB the histogram would have used, as float4 {x, y, z, .} at its own index (8192 x 16 B = kLgHistBytes: the capacity), and
// thread t owns the points t + 1024 r, r < 8: coordinates and running distances in registers for the whole chain. A round is
// fps_generic_body's round (fps.hip) on those registers: the sample's coordinates from one broadcast LDS read, sqdist,
// __builtin_fminf, the same 64-bit key, wave maximum, one slot per wave in the key array (parity double-buffered), one
// __syncthreads(), 16 keys, decode. The arithmetic per point is the generic kernel's, hence its samples, ties, non-finite points
// and m > n (value 0: point 0 wins) included. Slots r with 1024 r >= n are skipped by a workgroup-uniform branch; a thread without
// a point in a slot that runs contributes key 0, below every real key.
constexpr int kLgShortCap = (int)(kLgHistBytes / 16);
constexpr int kLgShortP = kLgShortCap / kLgT;
static_assert(kLgShortCap == 8192 && kLgShortP == 8, "short clouds: eight points per thread, the histogram's LDS");

__device__ __forceinline__ void fps_large_short_body(int n, int m, const float *__restrict__ src, int *__restrict__ dst,
                                                     float *__restrict__ dxyz, char *smem)
{
    constexpr int T = kLgT, W = kLgW, P = kLgShortP;
    float4 *pts = reinterpret_cast<float4 *>(smem);                                        // [n]
    unsigned long long *part = reinterpret_cast<unsigned long long *>(smem + kLgKeyOff);   // [2][W]
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);

    if (t == 0) {
        dst[0] = 0;                                         // the first sample is point 0 (tf_sampling_g.cu:114-116)
        if (dxyz) { dxyz[0] = src[0]; dxyz[1] = src[1]; dxyz[2] = src[2]; }
    }
    if (m == 1) return;                                     // workgroup-uniform, before any barrier

    float px[P], py[P], pz[P], md[P];
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int k = t + T * r;
        const int kk = k < n ? k : 0;                       // no such point: point 0's coordinates, key 0 below
        px[r] = src[(size_t)kk * 3 + 0]; py[r] = src[(size_t)kk * 3 + 1]; pz[r] = src[(size_t)kk * 3 + 2];
        md[r] = 1e38f;                                      // tf_sampling_g.cu:118
        if (k < n) pts[k] = make_float4(px[r], py[r], pz[r], 0.0f);
    }
    __syncthreads();

    int cur = 0;
    for (int j = 1; j < m; ++j) {
        const float4 s = pts[cur];                          // same address in every lane: LDS broadcast
        unsigned long long best = 0ull;                     // (value bits << 32) | ~tiekey; real candidates are > 0
#pragma unroll
        for (int r = 0; r < P; ++r) {
            if (T * r >= n) break;                          // workgroup-uniform
            const int k = t + T * r;
            const float d2 = __builtin_fminf(sqdist(px[r], py[r], pz[r], s.x, s.y, s.z), md[r]);   // min(d, td), tf_sampling_g.cu:144
            md[r] = d2;
            const unsigned tiekey = ((unsigned)(k & (kRefThreads - 1)) << 22) | (unsigned)(k >> 9);
            const unsigned long long key =
                k < n ? ((unsigned long long)(unsigned)__float_as_int(d2) << 32) | (unsigned long long)(0xFFFFFFFFu - tiekey) : 0ull;
            best = key > best ? key : best;
        }
        best = lg_wave_max_u64(best);
        if (lane == 0) part[(j & 1) * W + w] = best;
        __syncthreads();
        unsigned long long v = (lane < W) ? part[(j & 1) * W + lane] : 0ull;
#pragma unroll
        for (int sh = 1; sh < W; sh <<= 1) {
            const unsigned long long o = lg_shfl_xor_u64(v, sh);
            v = o > v ? o : v;
        }
        const unsigned tiekey = 0xFFFFFFFFu - (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
        cur = (int)(((tiekey & 0x3FFFFFu) << 9) | (tiekey >> 22));
        if (t == 0) {
            dst[j] = cur;
            if (dxyz) {
                const float4 q = pts[cur];
                dxyz[j * 3 + 0] = q.x; dxyz[j * 3 + 1] = q.y; dxyz[j * 3 + 2] = q.z;
            }
        }
    }
}

template <int L>
__global__ __launch_bounds__(kLgT) void fps_large_kernel(int n, int m, const float *__restrict__ xyz, float4 *__restrict__ recs_all,
                                                         float *__restrict__ md_all, int *__restrict__ out, float *__restrict__ out_xyz)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int cloud = blockIdx.x;
    fps_large_body<L, false>(n, m, xyz + (size_t)cloud * n * 3, recs_all + (size_t)cloud * n, md_all + (size_t)cloud * n,
                      out + (size_t)cloud * m, out_xyz ? out_xyz + (size_t)cloud * m * 3 : nullptr, smem);
}

// Ragged batch (pn2_farthest_point_sample_large_ragged): cloud c holds n_c = lengths[c] <= n points in its padded (n, 3) slab and
// -- with COUNTS -- yields m_c = npoints[c] <= m samples (both counts: cloud_count, pn2_device.h). The workgroup hands the body its
// own slabs, all addressed with the PADDED n and m, and runs it with n = n_c, m = m_c: the cloud is computed exactly as if it were
// alone (the slice rule of fps_ragged_kernel, fps.hip; the chain is prefix-consistent, so m_c samples are the first m_c of m).
// The prologue is fps_slab's (fps_body.h) written out: through that function the compiler orders this kernel's scalar address
// arithmetic differently (profiles/fps_one_ladder/README.md), and the kernels' instruction text is kept as it was.
// Rows m_c .. m-1 are fps_ragged_fill's: index 0 and xyz[c, 0], disjoint from the body's rows, so no barrier stands in between.
// What the body assumed of kernel-uniform extents, per workgroup:
//   * the return at m_c == 1 is a return from the body before its first barrier; the fill follows it;
//   * every __syncthreads() sits at the top level of the body or of the chain's loop over j < m_c, and n_c, m_c are read through
//     readfirstlane: all 1024 threads of the workgroup run the same barriers, whatever the other workgroups' counts are;
//   * the passes over the cloud (box, histogram, scatter) run k < n_c, and the histogram then sums to n_c, so the scatter's
//     places are 0 .. n_c-1: rows at or beyond n_c of the cloud, of the records and of the distances are never addressed;
//   * G = ceil(n_c / L) may be as small as 1, with a single real record: lg_group_load's min(i, n_c - 1) keeps the reads of the
//     missing records inside the slice, lg_group_finish gives them key 0 and stores nothing for them;
//   * with G < 16 some waves own no group: their group keys and wave key stay 0, they never publish, and their key slots were
//     zeroed in the prologue (SHORT; a dense cloud has at least 65 groups and compiles without the store);
//   * a one-point or otherwise degenerate cloud has a box of extent 0: every point in cell 0, as for dense input;
//   * m_c > n_c runs on at value 0, where the smallest tie key -- point 0 -- wins, as the dense operator with npoint > n.
template <int L, bool COUNTS>
__global__ __launch_bounds__(kLgT) void fps_large_ragged_kernel(int n, int m, const float *__restrict__ xyz, const int *__restrict__ lengths,
                                                                const int *__restrict__ npoints, float4 *__restrict__ recs_all,
                                                                float *__restrict__ md_all, int *__restrict__ out,
                                                                float *__restrict__ out_xyz)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int c = blockIdx.x;
    const int nc = cloud_count(lengths, c, n);
    const int mc = COUNTS ? cloud_count(npoints, c, m) : m;
    const float *__restrict__ src = xyz + (size_t)c * n * 3;
    int *__restrict__ dst = out + (size_t)c * m;
    float *__restrict__ dxyz = out_xyz ? out_xyz + (size_t)c * m * 3 : nullptr;
    fps_large_body<L, true>(nc, mc, src, recs_all + (size_t)c * n, md_all + (size_t)c * n, dst, dxyz, smem);
    if (COUNTS) fps_ragged_fill<kLgT>(mc, m, src, dst, dxyz);
}

// Packed batch (pn2_farthest_point_sample_large_packed): cloud c is rows offsets[c] .. offsets[c + 1] - 1 of the flat (total, 3)
// array, at most n = nmax of them (cloud_start / cloud_count, pn2_device.h: clamped, block-uniform scalars). The records and the
// running distances of the cloud are the same rows of the workspace's two arrays (total entries each: recs_all + start stays
// 16-byte aligned, coordinates are read as scalars), and the body runs on them with n = n_c exactly as in
// fps_large_ragged_kernel: the list above that kernel holds word for word with n_c taken from offsets (there are no counts and no
// fill here). A cloud of at most short_max <= kLgShortCap points takes fps_large_short_body instead: one block-uniform branch
// behind the slab prologue, every barrier of either body inside its own side, and neither recs nor md touched. global_idx:
// fps_global_rows (fps_body.h) behind the body -- both bodies return at m == 1 workgroup-uniformly and before any barrier, so its
// barrier is reached by all threads.
template <int L>
__global__ __launch_bounds__(kLgT) void fps_large_packed_kernel(int n, int m, int short_max, const float *__restrict__ xyz,
                                                                float4 *__restrict__ recs_all, float *__restrict__ md_all,
                                                                int *__restrict__ out, float *__restrict__ out_xyz, Packed pk)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int c = blockIdx.x;
    const int start = cloud_start(pk, c);
    const int nc = cloud_count(pk, c, start, n);
    const float *__restrict__ src = xyz + (size_t)start * 3;
    int *__restrict__ dst = out + (size_t)c * m;
    float *__restrict__ dxyz = out_xyz ? out_xyz + (size_t)c * m * 3 : nullptr;
    if (nc <= min(__builtin_amdgcn_readfirstlane(short_max), kLgShortCap))
        fps_large_short_body(nc, m, src, dst, dxyz, smem);
    else
        fps_large_body<L, true>(nc, m, src, recs_all + start, md_all + start, dst, dxyz, smem);
    fps_global_rows<kLgT>(m, pk.global_idx ? start : 0, dst);
}

template <int L>
static int launch_large(int b, int n, int m, const float *inp, void *ws, int *out, float *oxyz, hipStream_t st)
{
    float4 *recs = static_cast<float4 *>(ws);
    float *md = reinterpret_cast<float *>(recs + (size_t)b * n);
    return launch_lds(fps_large_kernel<L>, dim3(b), dim3(kLgT), kLgLdsBytes, st, n, m, inp, recs, md, out, oxyz);
}

// npoints: NULL = m samples from every cloud
template <int L>
static int launch_large_ragged(int b, int n, int m, const float *inp, const int *lengths, const int *npoints, void *ws, int *out,
                               float *oxyz, hipStream_t st)
{
    float4 *recs = static_cast<float4 *>(ws);
    float *md = reinterpret_cast<float *>(recs + (size_t)b * n);
    return launch_lds(npoints ? fps_large_ragged_kernel<L, true> : fps_large_ragged_kernel<L, false>, dim3(b), dim3(kLgT), kLgLdsBytes, st,
                      n, m, inp, lengths, npoints, recs, md, out, oxyz);
}

// fps.hip: the global-memory kernel with counts (running distances in temp, (b, n) floats)
int fps_launch_generic_ragged(int b, int n, int m, const float *inp, const int *lengths, const int *npoints, float *temp, int *out,
                              float *oxyz, hipStream_t st);

// ... and in the packed mode (temp: pk.total floats)
int fps_launch_generic_packed(int b, int n, int m, const float *inp, Packed pk, float *temp, int *out, float *oxyz, hipStream_t st);

// packed: the workspace is pk.total records, then pk.total running distances
template <int L>
static int launch_large_packed(int b, int n, int m, int short_max, const float *inp, Packed pk, void *ws, int *out, float *oxyz,
                               hipStream_t st)
{
    float4 *recs = static_cast<float4 *>(ws);
    float *md = reinterpret_cast<float *>(recs + (size_t)pk.total);
    return launch_lds(fps_large_packed_kernel<L>, dim3(b), dim3(kLgT), kLgLdsBytes, st, n, m, short_max, inp, recs, md, out, oxyz, pk);
}

static bool large_covers(int n) { return n > kLgMinPoints && n <= kLgMaxPoints; }

}  // namespace pn2

extern "C" int pn2_fps_large_supported(int n, int m) { return (pn2::large_covers(n) && m > 0) ? 1 : 0; }

// 16 bytes of record and 4 of running distance per point: (b, n) records first, then (b, n) distances
extern "C" long long pn2_fps_large_ws_bytes(int b, int n)
{
    if (b <= 0 || !pn2::large_covers(n)) return 0;
    return (long long)b * n * 20;
}

// Where the tier pays (measured, profiles/fps_large/README.md: medians of 20, two runs of every figure within 0.2 % of each
// other). Against the global-memory kernel on uniform-cube / sphere-surface clouds, generic time over this tier's:
//   n = 20000: 0.82 / 0.95 at m = 64, 1.20 / 1.38 at 256, 1.49 / 1.70 at 1024;   32768: 0.88 / 1.05, 1.39 / 1.70, 1.88 / 2.24;
//   65536: 1.05 / 1.32 at m = 64, 1.88 / 2.42 at 256;   131072: 1.28 / 1.67, 2.50 / 3.46;   1048576: 2.57 / 3.39, 6.73 / 9.71.
// The prologue (sort + boxes) is what a short chain cannot earn back: 1 only from the smallest measured m at which BOTH kinds
// were ahead, and nowhere below the smallest m of the sweep.
extern "C" int pn2_fps_large_pays(int n, int m)
{
    if (!pn2_fps_large_supported(n, m)) return 0;
    return m >= (n >= 65536 ? 64 : 256) ? 1 : 0;
}

extern "C" int pn2_farthest_point_sample_large_ex(int group_len, int b, int n, int m, const float *inp, void *ws, int *out,
                                                  float *out_xyz, void *stream)
{
    using namespace pn2;
    if (m <= 0 || b == 0) return PN2_OK;                   // the dense entry's order (fps_entry, fps.hip)
    if (b < 0 || n <= 0) return PN2_E_SHAPE;
    if (!inp || !out || !ws) return PN2_E_NULL;
    if (!large_covers(n)) return PN2_E_TOO_LARGE;
    if ((long long)b * n * 3 > INT_MAX || (long long)b * m * 3 > INT_MAX) return PN2_E_TOO_LARGE;
    if (group_len != 64 && group_len != 128 && group_len != 256) return PN2_E_ARG;
    if (((long long)n + group_len - 1) / group_len > kLgMaxGroups) return PN2_E_TOO_LARGE;   // four box slots per lane
    if (reinterpret_cast<uintptr_t>(ws) & 15) return PN2_E_ARG;                               // 16-byte records
    hipStream_t st = as_stream(stream);
    switch (group_len) {
    case 64: return launch_large<64>(b, n, m, inp, ws, out, out_xyz, st);
    case 128: return launch_large<128>(b, n, m, inp, ws, out, out_xyz, st);
    default: return launch_large<256>(b, n, m, inp, ws, out, out_xyz, st);
    }
}

extern "C" int pn2_farthest_point_sample_large(int b, int n, int m, const float *inp, void *ws, int *out, float *out_xyz, void *stream)
{
    return pn2_farthest_point_sample_large_ex(256, b, n, m, inp, ws, out, out_xyz, stream);
}

// Ragged batch of large clouds: cloud c is inp[c, :lengths[c]] of a padded (b, n, 3) tensor, 16384 < n <= 1048576, and yields
// npoints[c] samples (NULL: m). Both count arrays live on the device and are never read by the host, so every host decision is
// taken on the padded extents: ws is pn2_fps_large_ws_bytes(b, n) bytes, and kernel 0 follows pn2_fps_large_pays(n, m). kernel 1
// is the global-memory kernel with counts (its running distances in the workspace's distance array), kernel 2 the cell-sorted
// tier. Result per cloud = the dense operator on the slice, whichever kernel runs.
extern "C" int pn2_farthest_point_sample_large_ragged_ex(int kernel, int group_len, int b, int n, int m, const float *inp,
                                                         const int *lengths, const int *npoints, void *ws, int *out, float *out_xyz,
                                                         void *stream)
{
    using namespace pn2;
    if (m <= 0 || b == 0) return PN2_OK;
    if (b < 0 || n <= 0) return PN2_E_SHAPE;
    if (!inp || !out || !ws || !lengths) return PN2_E_NULL;
    if (!large_covers(n)) return PN2_E_TOO_LARGE;
    if ((long long)b * n * 3 > INT_MAX || (long long)b * m * 3 > INT_MAX) return PN2_E_TOO_LARGE;
    if (kernel < 0 || kernel > 2) return PN2_E_ARG;
    if (group_len != 64 && group_len != 128 && group_len != 256) return PN2_E_ARG;
    const bool tier = kernel == 2 || (kernel == 0 && pn2_fps_large_pays(n, m));
    if (tier && ((long long)n + group_len - 1) / group_len > kLgMaxGroups) return PN2_E_TOO_LARGE;   // four box slots per lane
    if (reinterpret_cast<uintptr_t>(ws) & 15) return PN2_E_ARG;                                       // 16-byte records
    hipStream_t st = as_stream(stream);
    if (!tier) {
        float *md = reinterpret_cast<float *>(static_cast<float4 *>(ws) + (size_t)b * n);
        return fps_launch_generic_ragged(b, n, m, inp, lengths, npoints, md, out, out_xyz, st);
    }
    switch (group_len) {
    case 64: return launch_large_ragged<64>(b, n, m, inp, lengths, npoints, ws, out, out_xyz, st);
    case 128: return launch_large_ragged<128>(b, n, m, inp, lengths, npoints, ws, out, out_xyz, st);
    default: return launch_large_ragged<256>(b, n, m, inp, lengths, npoints, ws, out, out_xyz, st);
    }
}

extern "C" int pn2_farthest_point_sample_large_ragged(int b, int n, int m, const float *inp, const int *lengths, const int *npoints,
                                                      void *ws, int *out, float *out_xyz, void *stream)
{
    return pn2_farthest_point_sample_large_ragged_ex(0, 256, b, n, m, inp, lengths, npoints, ws, out, out_xyz, stream);
}

// Packed batch of large clouds: cloud c is inp[offsets[c] : offsets[c + 1]] of a flat (total, 3) array, offsets (b + 1) int32 on
// the device and never read by the host; 16384 < nmax <= 1048576 bounds every cloud's count and takes the padded n's place in every
// host decision. The workspace follows the flat array: total records, then total running distances.
extern "C" long long pn2_fps_large_packed_ws_bytes(int total) { return total > 0 ? (long long)total * 20 : 0; }

// short_max = -1, the library's rule (measured, profiles/fps_large_packed/README.md: medians of 20, b = 8 clouds of n_c points,
// the tier's cell-sorted body over the short body, uniform-cube / sphere-surface clouds; nmax = 20000 and 131072 agree to 2 %):
//   n_c = 1024: 1.67 / 1.67 at m = 256, 1.62 / 1.62 at m = 1024;   2048: 1.75 / 1.73, 1.68 / 1.66;
//   4096: 1.93 / 1.85, 1.81 / 1.74;                                  8192: 2.05 / 1.91, 1.78 / 1.67.
// The largest measured n_c at which the short body was ahead for both kinds and both m -- its capacity.
constexpr int kLgShortRule = 8192;
static_assert(kLgShortRule <= pn2::kLgShortCap, "the rule stays inside the short body's capacity");

extern "C" int pn2_farthest_point_sample_large_packed_ex(int kernel, int group_len, int short_max, int b, int total, int nmax, int m,
                                                         const float *inp, const int *offsets, int global_idx, void *ws, int *out,
                                                         float *out_xyz, void *stream)
{
    using namespace pn2;
    if (m <= 0 || b == 0) return PN2_OK;
    if (b < 0 || nmax <= 0 || total <= 0) return PN2_E_SHAPE;
    if (!inp || !offsets || !out || !ws) return PN2_E_NULL;
    if (!large_covers(nmax)) return PN2_E_TOO_LARGE;
    if ((long long)total * 3 > INT_MAX || (long long)b * m * 3 > INT_MAX) return PN2_E_TOO_LARGE;
    if (kernel < 0 || kernel > 2) return PN2_E_ARG;
    if (group_len != 64 && group_len != 128 && group_len != 256) return PN2_E_ARG;
    if (short_max < -1 || short_max > kLgShortCap) return PN2_E_ARG;
    const bool tier = kernel == 2 || (kernel == 0 && pn2_fps_large_pays(nmax, m));
    if (tier && ((long long)nmax + group_len - 1) / group_len > kLgMaxGroups) return PN2_E_TOO_LARGE;   // four box slots per lane
    if (reinterpret_cast<uintptr_t>(ws) & 15) return PN2_E_ARG;                                          // 16-byte records
    hipStream_t st = as_stream(stream);
    const Packed pk = {offsets, total, global_idx ? 1 : 0};
    if (!tier) {
        float *md = reinterpret_cast<float *>(static_cast<float4 *>(ws) + (size_t)total);
        return fps_launch_generic_packed(b, nmax, m, inp, pk, md, out, out_xyz, st);
    }
    const int sm = short_max < 0 ? kLgShortRule : short_max;
    switch (group_len) {
    case 64: return launch_large_packed<64>(b, nmax, m, sm, inp, pk, ws, out, out_xyz, st);
    case 128: return launch_large_packed<128>(b, nmax, m, sm, inp, pk, ws, out, out_xyz, st);
    default: return launch_large_packed<256>(b, nmax, m, sm, inp, pk, ws, out, out_xyz, st);
    }
}

extern "C" int pn2_farthest_point_sample_large_packed(int b, int total, int nmax, int m, const float *inp, const int *offsets,
                                                      int global_idx, void *ws, int *out, float *out_xyz, void *stream)
{
    return pn2_farthest_point_sample_large_packed_ex(0, 256, -1, b, total, nmax, m, inp, offsets, global_idx, ws, out, out_xyz, stream);
}
