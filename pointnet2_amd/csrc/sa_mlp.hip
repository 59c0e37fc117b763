// sa_mlp.hip -- the grouped local MLP of a set-abstraction layer fused with its max-pool, on the
// matrix cores. gfx950.
//
// Replaces, for inference, reference utils/pointnet_util.py:44-50 + :117-127:
//     grouped_xyz = group_point(xyz, idx) - new_xyz ; new_points = concat(grouped_xyz, group_point(points, idx))
//     3 x [ tf_util.conv2d 1x1 + batch_norm (eps 1e-3) + ReLU ]  (tf_util.py:88-150, :512-531)
//     new_points = reduce_max(new_points, axis=[2])
// i.e. per centroid an (nsample x Cin) matrix through three dense layers and a column max. The
// reference (and a plain PyTorch port) materialises the (b, m, nsample, C) tensor of every layer in
// HBM: 128-640 MB per SA level in the segmentation configs. Here NOTHING between the idx tensor and
// the (b, m, C3) result leaves the CU: rows are gathered straight into MFMA operand registers, the
// activations of all three layers stay in registers, the max runs over lanes.
// Batch norm is folded into the weights by the caller (inference statistics): W' = W*s, b' = (b-mu)*s+beta.
//
// Arithmetic: fp32 results on the bf16 matrix pipe. Every fp32 operand is the exact sum of three bf16 values
// (nearest-even residuals: 8 + 8 + 8 significant bits), a product a.b is evaluated as the six bf16 x bf16 terms
// a1b1, a1b2, a2b1, a1b3, a2b2, a3b1 (each exact in the fp32 accumulator; the three dropped terms are below 2^-24
// relative), i.e. six v_mfma_f32_32x32x16_bf16 per 16 contraction indices where the fp32-input
// v_mfma_f32_32x32x2_f32 needs eight at twice the cycles each: 2.7x fewer matrix-pipe cycles for the same
// accuracy (measured against an fp64 evaluation: the same error as an fp32 fma chain, tests/test_sa_mlp_gpu.py).
// The weights are split on the host when they are packed (three levels stored side by side, 6 bytes per weight);
// the activations are split in registers right after each layer's ReLU: 5.5 VALU operations per value
// (v_cvt_pk_bf16_f32, shift/mask back to fp32, subtract, twice) -- once per value and layer, amortised over the
// layer's output width.
//
// Formulation. One wave owns 32 samples (one centroid at nsample = 32) and computes the TRANSPOSED
// layer  H^T (channels x samples) = W^T (Cout x Cin) . X^T (Cin x samples):
//   MFMA "A" operand = a 32x16 block of W^T: lane l supplies W[k][n = 32t + (l & 31)] for eight k (slots j = 0..7
//                      of lane half l >> 5), chosen below;
//   MFMA "B" operand = a 16x32 block of X^T: lane l supplies X[sample = l & 31][k], the same eight k;
//   C/D: lane l, register v holds H^T[channel 8(v>>2) + 4(l>>5) + (v&3)][sample l & 31].
// The contraction index k may be visited in ANY order as long as A and B agree. Giving slot j of K16 step e
// (e = 0, 1) of input tile u the index k = 32u + 8((8e + j) >> 2) + 4(l >> 5) + (j & 3) makes the B operand of step e
// EXACTLY accumulator registers 8e .. 8e + 7 of the previous layer's tile u (after the split into levels): the
// activations never move between layers -- no LDS round trip, no shuffles. The weights are stored pre-permuted to
// match (mlp_resident_pack), in LDS, one ds_read_b128 per lane, level and K16 step.
// The LAST layer swaps the two MFMA operands (their lane maps are the same: index l & 31, slots by l >> 5),
// which yields the untransposed H (samples x channels): a lane then holds 16 SAMPLES of one
// channel, so the max-pool is 15 lane-local v_max plus one exchange with lane l ^ 32, and bias + ReLU
// are applied once to the pooled value (x -> relu(x + b) is monotone, so max and it commute exactly).
// Pooling across lanes instead (the first version) cost 5 cross-lane steps for each of 64 registers.
// Eight waves (two per SIMD) share one copy of the weights in LDS.
#include "sa_mlp_common.h"

namespace pn2 {

// One dense layer on the wave's 32 samples: out[t] = relu(bias + sum_u W^T[t][u] . in[u]), 12 bf16 MFMAs per
// (t, u) pair (two K16 steps of six). The weights of step i + 1 are read from LDS while the MFMAs of step i
// run (the compiler fence keeps the prefetch where it is written; left alone, hipcc hoists EVERY weight read
// of the layer to its top and runs out of registers). `ksteps` = K16 steps of an input tile that can be
// non-zero (2, except for a narrow first layer). LAST: operands swapped (see the header): out[t] holds raw
// sums H[sample][channel l & 31], no bias, no ReLU, max-accumulated over the centroid's 32-sample groups
// unless `first`.
template <int TOUT, int TIN, bool LAST>
__device__ __forceinline__ void mlp_layer(const float *wp, const float *bp, const ActSplit (&in)[TIN], f32x16 (&out)[TOUT],
                                          int lane, int h, int ksteps, bool first)
{
    const u32x4 *w4 = reinterpret_cast<const u32x4 *>(wp) + lane;
    u32x4 cur[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) cur[l] = w4[l * 64];
    f32x16 acc;
    constexpr int kSteps = TOUT * TIN * 2;
#pragma unroll
    for (int i = 0; i < kSteps; ++i) {
        const int pair = i >> 1, e = i & 1, t = pair / TIN, u = pair % TIN;
        u32x4 nxt[3];
        if (i + 1 < kSteps) {
#pragma unroll
            for (int l = 0; l < 3; ++l) nxt[l] = w4[((i + 1) * 3 + l) * 64];
        }
        if (u == 0 && e == 0) {
            if (LAST) {
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
            } else {
                acc = mlp_bias(bp, t, h);
            }
        }
        asm volatile("" ::: "memory");
        if (e < ksteps) acc = mma_x6<LAST>(cur, in[u].p[e], acc);
        if (u == TIN - 1 && e == 1) {
            if (!LAST) {
                out[t] = mlp_relu(acc);
            } else if (first) {
                out[t] = acc;
            } else {
#pragma unroll
                for (int v = 0; v < 16; ++v) out[t][v] = vmax(out[t][v], acc[v]);
            }
        }
        if (i + 1 < kSteps) {
#pragma unroll
            for (int l = 0; l < 3; ++l) cur[l] = nxt[l];
        }
    }
}

// T1, T2, T3: output tiles (32 channels each) of the three layers; the input is one tile (Cin <= 32).
// SPAN: samples per centroid inside one 32-sample group (32, or 16 when nsample = 16).
// POOL: the reference's pooling modes (utils/pointnet_util.py:128-140): 0 max (the text above), 1 avg, 2 weighted_avg
// (weights exp(-5 |grouped_xyz|) normalised over the group), 3 max_and_avg (out = [avg (c3), max (c3)] per centroid). An average
// does not commute with bias + ReLU, so modes 1-3 apply them to every sample's raw sum and accumulate per lane: a lane holds 16
// samples of one channel, the sums of registers 0-7 and 8-15 are kept apart (SPAN = 16: two centroids), one exchange with
// lane l ^ 32 at the end. The weights of mode 2 come from the layer-1 operand (lanes 0-31 hold their sample's centred
// coordinates) through one ds_bpermute per register and 32-sample part.
// RAGGED (max pooling only; npoints (b) in device memory, include/pn2ops.h "ragged inference"): centroid row j of cloud c is
// padding when j >= clamp(npoints[c], 1, m). A lane whose row is padding gathers through row 0 of its own cloud (always valid:
// finite arithmetic, nothing of the padding row is dereferenced) and its pooled result is stored as +0.0; at SPAN = 16 the two
// rows of an item are judged apart (with an odd m they belong to different clouds). An item that is padding only is left
// before its gather and its MFMAs. The dense instantiations have none of it.
template <int T1, int T2, int T3, int SPAN, int NT, int POOL = 0, bool RAGGED = false>
__global__ __launch_bounds__(NT) void sa_mlp3_kernel(int n, int m, int nsample, int cfeat, int c3, long long rows,
                                                              const float *__restrict__ xyz,
                                                              const float *__restrict__ new_xyz,
                                                              const float *__restrict__ points,
                                                              const int *__restrict__ idx,
                                                              const float *__restrict__ wpacked,
                                                              const float *__restrict__ bpacked, float *__restrict__ out,
                                                              const int *__restrict__ npoints)
{
    static_assert(!RAGGED || POOL == 0, "counts: max pooling only");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *w1 = reinterpret_cast<float *>(smem);
    float *w2 = w1 + mlp_w_floats(T1, 1);
    float *w3 = w2 + mlp_w_floats(T2, T1);
    float *b1 = w3 + mlp_w_floats(T3, T2);
    float *b2 = b1 + mlp_b_floats(T1);
    float *b3 = b2 + mlp_b_floats(T2);
    {
        const size_t wf = mlp_w_floats(T1, 1) + mlp_w_floats(T2, T1) + mlp_w_floats(T3, T2);
        const size_t bf = mlp_b_floats(T1) + mlp_b_floats(T2) + mlp_b_floats(T3);
        const float4 *src = reinterpret_cast<const float4 *>(wpacked);
        float4 *dst = reinterpret_cast<float4 *>(w1);
        for (size_t i = threadIdx.x; i < wf / 4; i += NT) dst[i] = src[i];
        for (size_t i = threadIdx.x; i < bf; i += NT) b1[i] = bpacked[i];
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int h = lane >> 5, s = lane & 31;
    const int cin = 3 + cfeat;
    const int quartets1 = (cin + 7) / 8;                 // register quartet q covers channels 8q .. 8q+7
    const int ksteps1 = cin > 16 ? 2 : 1;                // K16 step e covers channels 16e .. 16e+15
    const int parts = SPAN == 32 ? nsample / 32 : 1;     // 32-sample groups per centroid
    const long long wave = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * (NT / 64);
    const long long groups = SPAN == 32 ? rows : (rows + 1) / 2;

    // The gather is software-pipelined over the work items (a 32-sample group of a centroid): the index
    // of item i + 1 is fetched when item i starts, its coordinates/features after item i's second layer
    // (the index has arrived by then), so both dependent global round trips hide under MFMA work.
    auto item_row = [&](long long g) -> long long {
        const long long r = SPAN == 32 ? g : g * 2 + (s >> 4);
        return r < rows ? r : rows - 1;                          // an odd tail at nsample = 16 recomputes the last row
    };
    // RAGGED: is row r (< rows) below its cloud's count, and the row a lane gathers through
    auto row_valid = [&](long long r) -> bool {
        const long long cloud = r / m;
        return (int)(r - cloud * m) < min(max(npoints[cloud], 1), m);
    };
    auto gather_row = [&](long long g) -> long long {
        const long long r = item_row(g);
        if (!RAGGED) return r;
        return row_valid(r) ? r : r / m * m;
    };
    auto item_padding = [&](long long g) -> bool {              // wave-uniform: every row of the item is padding
        if (SPAN == 32) return !row_valid(g);
        return !row_valid(2 * g) && (2 * g + 1 >= rows || !row_valid(2 * g + 1));
    };
    auto store_zeros = [&](long long g) {
#pragma unroll
        for (int t = 0; t < T3; ++t) {
            const int ch = 32 * t + s;
            if (h == 0 && ch < c3) {
                if (SPAN == 32) out[g * c3 + ch] = 0.0f;
                else {
                    out[(2 * g) * c3 + ch] = 0.0f;
                    if (2 * g + 1 < rows) out[(2 * g + 1) * c3 + ch] = 0.0f;
                }
            }
        }
    };
    auto load_index = [&](long long g, int part) -> int {
        const int sample = SPAN == 32 ? part * 32 + s : (s & 15);
        return idx[gather_row(g) * nsample + sample];
    };
    // layer-1 operand: register v <- input channel mlp_chan(v, h) of this lane's sample. The loads only
    // (raw coordinates; `cen` = the centroid coordinate to subtract, 0 for feature channels): the
    // subtraction is done when the operand is consumed, one item later, so no wait sits in the MFMA stream
    auto load_x0 = [&](long long g, int p, f32x16 &cen) -> f32x16 {
        const long long row = gather_row(g), cloud = row / m;
        const float *px = xyz + ((size_t)cloud * n + p) * 3;
        const float *pf = points ? points + ((size_t)cloud * n + p) * cfeat : nullptr;
        const float *c = new_xyz + row * 3;
        f32x16 x0;
        if (!points) {                                   // xyz only (every first SA level): three loads, no per-register tests
#pragma unroll
            for (int v = 0; v < 16; ++v) { x0[v] = 0.0f; cen[v] = 0.0f; }
            if (h == 0) {
                x0[0] = px[0]; x0[1] = px[1]; x0[2] = px[2];
                cen[0] = c[0]; cen[1] = c[1]; cen[2] = c[2];
            }
            return x0;
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int k = mlp_chan(v, h);
            float val = 0.0f, sub = 0.0f;
            if ((v >> 2) < quartets1) {
                if (k < 3) { val = px[k]; sub = c[k]; }
                else if (k < cin) val = pf[k - 3];
            }
            x0[v] = val;
            cen[v] = sub;
        }
        return x0;
    };

    long long g = wave;
    int part = 0;
    f32x16 x0, cen;
    if (RAGGED) {
        while (g < groups && item_padding(g)) { store_zeros(g); g += nwaves; }
    }
    if (g < groups) x0 = load_x0(g, load_index(g, 0), cen);
    f32x16 best[T3];
    float sa[T3], sb[T3], ma[T3], mb[T3], ea = 0.0f, eb = 0.0f;      // POOL != 0: sums / maxima of registers 0-7 and 8-15, weight sums
    while (g < groups) {
        // the item after this one
        const bool last_part = part + 1 == parts;
        long long gn = last_part ? g + nwaves : g;
        if (RAGGED && last_part) {                               // items of padding only: their zeros, no gather, no MFMAs
            while (gn < groups && item_padding(gn)) { store_zeros(gn); gn += nwaves; }
        }
        const int partn = last_part ? 0 : part + 1;
        const bool more = gn < groups;
        int pn = 0;
        if (more) pn = load_index(gn, partn);
        ActSplit s0[1], s1[T1], s2[T2];
        float e_lane = 0.0f;
        {
            f32x16 in0;
#pragma unroll
            for (int v = 0; v < 4; ++v) in0[v] = __fsub_rn(x0[v], cen[v]);      // channels 0-2 live in registers 0-2 of lanes 0-31
#pragma unroll
            for (int v = 4; v < 16; ++v) in0[v] = x0[v];
            s0[0] = split_act(in0);
            if (POOL == 2)                                       // :133-134, tf.norm + exp(-5 d); lanes 0-31 hold the coordinates
                e_lane = expf(-5.0f * sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(in0[0], in0[0]), __fmul_rn(in0[1], in0[1])), __fmul_rn(in0[2], in0[2]))));
        }
        {
            f32x16 h1[T1];
            mlp_layer<T1, 1, false>(w1, b1, s0, h1, lane, h, ksteps1, true);
#pragma unroll
            for (int t = 0; t < T1; ++t) s1[t] = split_act(h1[t]);
        }
        {
            f32x16 h2[T2];
            mlp_layer<T2, T1, false>(w2, b2, s1, h2, lane, h, 2, true);
#pragma unroll
            for (int t = 0; t < T2; ++t) s2[t] = split_act(h2[t]);
        }
        if (more) x0 = load_x0(gn, pn, cen);
        mlp_layer<T3, T2, true>(w3, b3, s2, best, lane, h, 2, POOL != 0 || part == 0);
        if (POOL != 0) {
            // this part's 16 samples per lane: bias + ReLU per sample, then the (weighted) sums; max_and_avg keeps the raw maxima too
            float wv[16];
            if (POOL == 2) {
#pragma unroll
                for (int v = 0; v < 16; ++v) wv[v] = __shfl(e_lane, 8 * (v >> 2) + 4 * h + (v & 3));
            }
            if (part == 0) {
                ea = eb = 0.0f;
#pragma unroll
                for (int t = 0; t < T3; ++t) { sa[t] = sb[t] = 0.0f; ma[t] = mb[t] = -3.0e38f; }
            }
            if (POOL == 2) {
#pragma unroll
                for (int v = 0; v < 8; ++v) { ea += wv[v]; eb += wv[8 + v]; }
            }
#pragma unroll
            for (int t = 0; t < T3; ++t) {
                const float bias = b3_at(b3, 32 * t + s);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    float r = fmaxf(__fadd_rn(best[t][v], bias), 0.0f);
                    if (POOL == 2) r *= wv[v];
                    if (v < 8) sa[t] += r; else sb[t] += r;
                    if (POOL == 3) { if (v < 8) ma[t] = fmaxf(ma[t], best[t][v]); else mb[t] = fmaxf(mb[t], best[t][v]); }
                }
            }
            if (!last_part) { part = partn; continue; }
            const long long row = item_row(g);
            const int oc = POOL == 3 ? 2 * c3 : c3;                 // floats per output row
            float d0 = (float)nsample, d1 = (float)nsample;
            if (POOL == 2) {
                if (SPAN == 32) { d0 = ea + eb; d0 += __shfl_xor(d0, 32); }
                else { d0 = ea + __shfl_xor(ea, 32); d1 = eb + __shfl_xor(eb, 32); }
            }
#pragma unroll
            for (int t = 0; t < T3; ++t) {
                const int ch = 32 * t + s;
                const float bias = b3_at(b3, ch);
                if (SPAN == 32) {
                    float sum = sa[t] + sb[t], mx = fmaxf(ma[t], mb[t]);
                    sum += __shfl_xor(sum, 32);
                    mx = fmaxf(mx, __shfl_xor(mx, 32));
                    if (h == 0 && ch < c3) {
                        out[row * oc + ch] = sum / d0;
                        if (POOL == 3) out[row * oc + c3 + ch] = fmaxf(__fadd_rn(mx, bias), 0.0f);
                    }
                } else {
                    const float s0_ = sa[t] + __shfl_xor(sa[t], 32), s1_ = sb[t] + __shfl_xor(sb[t], 32);
                    const float m0 = fmaxf(ma[t], __shfl_xor(ma[t], 32)), m1 = fmaxf(mb[t], __shfl_xor(mb[t], 32));
                    if (h == 0 && ch < c3) {
                        out[(2 * g) * oc + ch] = s0_ / d0;
                        if (POOL == 3) out[(2 * g) * oc + c3 + ch] = fmaxf(__fadd_rn(m0, bias), 0.0f);
                        if (2 * g + 1 < rows) {
                            out[(2 * g + 1) * oc + ch] = s1_ / d1;
                            if (POOL == 3) out[(2 * g + 1) * oc + c3 + ch] = fmaxf(__fadd_rn(m1, bias), 0.0f);
                        }
                    }
                }
            }
            g = gn;
            part = 0;
            continue;
        }
        if (!last_part) { part = partn; continue; }
        const long long row = item_row(g);
        // Pool: lane l holds channel 32t + (l & 31) for the samples 8(v >> 2) + 4(l >> 5) + (v & 3), v = 0..15
        // (SPAN = 16: registers 0-7 are the first centroid's 16 samples, 8-15 the second's); bias and ReLU
        // on the pooled value; one coalesced 128-byte store per tile and centroid.
#pragma unroll
        for (int t = 0; t < T3; ++t) {
            const int ch = 32 * t + s;
            const float bias = b3_at(b3, ch);
            if (SPAN == 32) {
                float mx = best[t][0];
#pragma unroll
                for (int v = 1; v < 16; ++v) mx = fmaxf(mx, best[t][v]);
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                if (h == 0 && ch < c3) out[row * c3 + ch] = fmaxf(__fadd_rn(mx, bias), 0.0f);      // (RAGGED: the item is a valid row)
            } else {
                float m0 = best[t][0], m1 = best[t][8];
#pragma unroll
                for (int v = 1; v < 8; ++v) { m0 = fmaxf(m0, best[t][v]); m1 = fmaxf(m1, best[t][8 + v]); }
                m0 = fmaxf(m0, __shfl_xor(m0, 32));
                m1 = fmaxf(m1, __shfl_xor(m1, 32));
                if (h == 0 && ch < c3) {
                    const float v0 = fmaxf(__fadd_rn(m0, bias), 0.0f), v1 = fmaxf(__fadd_rn(m1, bias), 0.0f);
                    out[(2 * g) * c3 + ch] = (!RAGGED || row_valid(2 * g)) ? v0 : 0.0f;
                    if (2 * g + 1 < rows) out[(2 * g + 1) * c3 + ch] = (!RAGGED || row_valid(2 * g + 1)) ? v1 : 0.0f;
                }
            }
        }
        g = gn;
        part = 0;
    }
}

// ---- two items per wave -------------------------------------------------------------------------------------------
// What the kernel above leaves on the table (profiles/r04/ubench_mfma_valu.txt): on gfx950 a wave's vector instructions
// hide completely under its OWN queued MFMAs (four per v_mfma_f32_32x32x16_bf16 cost nothing) as long as they do not
// depend on them, while the vector work of the OTHER wave of the SIMD hides only by half. Within one 32-sample item the
// level split of a layer's output depends on the layer's last MFMAs and feeds the next layer's first ones, so with one
// item per wave the kernel runs at MFMA time + vector time (81 + 54 us at the metric shape). Here a wave carries TWO
// items, A and B, half a phase apart: every layer of one item ("host": its weight reads and MFMAs, step by step) is
// followed, step by step, by pieces of the other item's vector work ("guest": ReLU + level split of the previous layer's
// accumulators, the input subtraction, the pooling tail),
//     L1(A) | input split B      L1(B) | split h1 A      L2(A) | split h1 B
//     L2(B) | split h2 A         L3(A) | split h2 B      L3(B) | pool A, input split of A's next item
// so the guest's instructions are independent of the MFMAs in flight. One wave per SIMD (256 threads, up to 512 registers
// with the accumulation registers as overflow) carries the state of both items. A sched_barrier after every step keeps
// hipcc from regrouping the two streams. Arithmetic and results are bit-identical to the kernel above. Levels of one
// 32-sample group per centroid (nsample 32 or 16) and at most 16 input channels; the rest keeps one item per wave.
template <bool RELU>
__device__ __forceinline__ void split_piece(const f32x16 &x, int e, int d, ActSplit &s)
{
    float a = x[8 * e + 2 * d], b = x[8 * e + 2 * d + 1];
    // a piece belongs to the step of the host layer it is written in: the empty volatile statement is ordered with the steps'
    // sched_barriers, and the piece's arithmetic depends on it (left alone, instruction selection emits a guest's whole split
    // in front of the host layer, and the barriers then keep it there)
    asm volatile("" : "+v"(a), "+v"(b));
    if (RELU) { a = vmax(a, 0.0f); b = vmax(b, 0.0f); }
    const unsigned int p1 = pack_bf16(a, b);
    const float ra = __fsub_rn(a, __uint_as_float(p1 << 16)), rb = __fsub_rn(b, __uint_as_float(p1 & 0xffff0000u));
    const unsigned int p2 = pack_bf16(ra, rb);
    const float sa = __fsub_rn(ra, __uint_as_float(p2 << 16)), sb = __fsub_rn(rb, __uint_as_float(p2 & 0xffff0000u));
    unsigned int q1 = p1, q2 = p2, q3 = pack_bf16(sa, sb);
    asm volatile("" : "+v"(q1), "+v"(q2), "+v"(q3));      // ... and its results exist when the step ends (nothing sinks to the consumer)
    s.p[e][0][d] = q1;
    s.p[e][1][d] = q2;
    s.p[e][2][d] = q3;
}

// pieces [lo, hi) of "ReLU + level split of the T tiles x" (eight pieces per tile); lo, hi are literals after unrolling
template <int T>
__device__ __forceinline__ void split_pieces(const f32x16 (&x)[T], ActSplit (&s)[T], int lo, int hi)
{
#pragma unroll
    for (int c = 0; c < T * 8; ++c)
        if (c >= lo && c < hi) split_piece<true>(x[c >> 3], (c >> 2) & 1, c & 3, s[c >> 3]);
}

// mlp_layer with a guest: hook(i) runs after the MFMAs of step i (i = 2 (t TIN + u) + e), and nothing is scheduled across
// the end of a step. The ReLU of a hidden layer is left to the consumer's split (out[t] = bias + sums).
template <int TOUT, int TIN, bool LAST, int KSTEPS, typename Hook>
__device__ __forceinline__ void mlp_layer_host(const float *wp, const float *bp, const ActSplit (&in)[TIN], f32x16 (&out)[TOUT],
                                               int lane, int h, Hook hook)
{
    const u32x4 *w4 = reinterpret_cast<const u32x4 *>(wp) + lane;
    // the weights of a step are read from LDS PN2_PAIR_PREFETCH steps ahead (three buffers in rotation)
#ifndef PN2_PAIR_PREFETCH
#define PN2_PAIR_PREFETCH 1
#endif
    constexpr int PF = PN2_PAIR_PREFETCH;
    u32x4 wb[PF + 1][3];
    constexpr int kSteps = TOUT * TIN * 2;
#pragma unroll
    for (int j = 0; j < PF; ++j)
        if (j < kSteps) {
#pragma unroll
            for (int l = 0; l < 3; ++l) wb[j][l] = w4[(j * 3 + l) * 64];
        }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < kSteps; ++i) {
        const int pair = i >> 1, e = i & 1, t = pair / TIN, u = pair % TIN;
        if (i + PF < kSteps) {
#pragma unroll
            for (int l = 0; l < 3; ++l) wb[(i + PF) % (PF + 1)][l] = w4[((i + PF) * 3 + l) * 64];
        }
        if (u == 0 && e == 0) {
            if (LAST) {
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
            } else {
                acc = mlp_bias(bp, t, h);
            }
        }
        if (e < KSTEPS) acc = mma_x6<LAST>(wb[i % (PF + 1)], in[u].p[e], acc);
        if (u == TIN - 1 && e == 1) out[t] = acc;
        hook(i);
#ifndef PN2_PAIR_NOBARRIER                 /* lab switch (scripts/build_mlp_labs.sh): what the step barriers are worth */
        __builtin_amdgcn_sched_barrier(0);
#endif
    }
}

// RAGGED: as in sa_mlp3_kernel, by redirect and select only -- the two items of a wave advance together through one
// schedule of hosts and guests, so an item of padding only runs on row 0 of its cloud and stores +0.0.
template <int T1, int T2, int T3, int SPAN, int NT, bool RAGGED = false>
__global__ __launch_bounds__(NT) void sa_mlp3_pair_kernel(int n, int m, int nsample, int cfeat, int c3, long long rows,
                                                           const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                           const float *__restrict__ points, const int *__restrict__ idx,
                                                           const float *__restrict__ wpacked, const float *__restrict__ bpacked,
                                                           float *__restrict__ out, const int *__restrict__ npoints)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *w1 = reinterpret_cast<float *>(smem);
    float *w2 = w1 + mlp_w_floats(T1, 1);
    float *w3 = w2 + mlp_w_floats(T2, T1);
    float *b1 = w3 + mlp_w_floats(T3, T2);
    float *b2 = b1 + mlp_b_floats(T1);
    float *b3 = b2 + mlp_b_floats(T2);
    {
        const size_t wf = mlp_w_floats(T1, 1) + mlp_w_floats(T2, T1) + mlp_w_floats(T3, T2);
        const size_t bf = mlp_b_floats(T1) + mlp_b_floats(T2) + mlp_b_floats(T3);
        const float4 *src = reinterpret_cast<const float4 *>(wpacked);
        float4 *dst = reinterpret_cast<float4 *>(w1);
        for (size_t i = threadIdx.x; i < wf / 4; i += NT) dst[i] = src[i];
        for (size_t i = threadIdx.x; i < bf; i += NT) b1[i] = bpacked[i];
    }
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int h = lane >> 5, s = lane & 31;
    const int cin = 3 + cfeat;                           // <= 16: one K16 step in layer 1, input registers 0 .. 7
    const long long wave = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * (NT / 64);
    const long long groups = SPAN == 32 ? rows : (rows + 1) / 2;

    auto item_row = [&](long long g) __attribute__((always_inline)) -> long long {
        const long long r = SPAN == 32 ? g : g * 2 + (s >> 4);
        return r < rows ? r : rows - 1;
    };
    auto row_valid = [&](long long r) __attribute__((always_inline)) -> bool {
        const long long cloud = r / m;
        return (int)(r - cloud * m) < min(max(npoints[cloud], 1), m);
    };
    auto gather_row = [&](long long g) __attribute__((always_inline)) -> long long {
        const long long r = item_row(g);
        if (!RAGGED) return r;
        return row_valid(r) ? r : r / m * m;
    };
    auto load_index = [&](long long g) __attribute__((always_inline)) -> int {
        const int sample = SPAN == 32 ? s : (s & 15);
        return idx[gather_row(g) * nsample + sample];
    };
    // layer-1 operand registers 0 .. 7 of this lane's sample (channels mlp_chan(v, h)) and what to subtract from them
    auto load_x0 = [&](long long g, int p, float (&x0)[8], float (&cen)[8]) __attribute__((always_inline)) {
        const long long row = gather_row(g), cloud = row / m;
        const float *px = xyz + ((size_t)cloud * n + p) * 3;
        const float *c = new_xyz + row * 3;
        if (!points) {                                   // xyz only: channels 0-2 live in registers 0-2 of lanes 0-31
            const float keep = h == 0 ? 1.0f : 0.0f;
#pragma unroll
            for (int v = 0; v < 8; ++v) { x0[v] = 0.0f; cen[v] = 0.0f; }
#pragma unroll
            for (int v = 0; v < 3; ++v) { x0[v] = px[v] * keep; cen[v] = c[v] * keep; }
            return;
        }
        const float *pf = points + ((size_t)cloud * n + p) * cfeat;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int k = mlp_chan(v, h);
            float val = 0.0f, sub = 0.0f;
            if (k < 3) { val = px[k]; sub = c[k]; }
            else if (k < cin) val = pf[k - 3];
            x0[v] = val;
            cen[v] = sub;
        }
    };
    // the input split: (x0 - centroid) -> the three levels of K16 step 0
    auto input_split = [&](const float (&x0)[8], const float (&cen)[8], ActSplit &s0) __attribute__((always_inline)) {
        f32x16 in0;
#pragma unroll
        for (int v = 0; v < 4; ++v) in0[v] = __fsub_rn(x0[v], cen[v]);
#pragma unroll
        for (int v = 4; v < 8; ++v) in0[v] = x0[v];
#pragma unroll
        for (int v = 8; v < 16; ++v) in0[v] = 0.0f;
#pragma unroll
        for (int d = 0; d < 4; ++d) split_piece<false>(in0, 0, d, s0);
#pragma unroll
        for (int l = 0; l < 3; ++l) s0.p[1][l] = u32x4{0u, 0u, 0u, 0u};
    };
    // pool + bias + ReLU + store of output tile t of item g (see sa_mlp3_kernel)
    auto pool_tile = [&](const f32x16 (&best)[T3], int t, long long g) __attribute__((always_inline)) {
        const long long row = item_row(g);
        const int ch = 32 * t + s;
        const float bias = b3_at(b3, ch);
        const bool live = g < groups && h == 0 && ch < c3;
        if (SPAN == 32) {
            float mx = best[t][0];
            asm volatile("" : "+v"(mx));                 // (pinned to its step, see split_piece)
#pragma unroll
            for (int v = 1; v < 16; ++v) mx = fmaxf(mx, best[t][v]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            if (live) {
                const float val = fmaxf(__fadd_rn(mx, bias), 0.0f);
                out[row * c3 + ch] = (!RAGGED || row_valid(row)) ? val : 0.0f;
            }
        } else {
            float m0 = best[t][0], m1 = best[t][8];
            asm volatile("" : "+v"(m0), "+v"(m1));
#pragma unroll
            for (int v = 1; v < 8; ++v) { m0 = fmaxf(m0, best[t][v]); m1 = fmaxf(m1, best[t][8 + v]); }
            m0 = fmaxf(m0, __shfl_xor(m0, 32));
            m1 = fmaxf(m1, __shfl_xor(m1, 32));
            if (live) {
                const float v0 = fmaxf(__fadd_rn(m0, bias), 0.0f), v1 = fmaxf(__fadd_rn(m1, bias), 0.0f);
                out[(2 * g) * c3 + ch] = (!RAGGED || row_valid(2 * g)) ? v0 : 0.0f;
                if (2 * g + 1 < rows) out[(2 * g + 1) * c3 + ch] = (!RAGGED || row_valid(2 * g + 1)) ? v1 : 0.0f;
            }
        }
    };
    auto clampg = [&](long long g) __attribute__((always_inline)) -> long long { return g < groups ? g : groups - 1; };

    // stream A: items wave, wave + 2 nwaves, ...; stream B: wave + nwaves, wave + 3 nwaves, ... (an item beyond the end
    // recomputes the last one and stores nothing)
    long long gA = wave, gB = wave + nwaves;
    if (gA >= groups) return;
    float xA[8], cA[8], xB[8], cB[8];
    load_x0(clampg(gA), load_index(clampg(gA)), xA, cA);
    load_x0(clampg(gB), load_index(clampg(gB)), xB, cB);
    ActSplit s0A[1], s0B[1];
    input_split(xA, cA, s0A[0]);
    while (gA < groups) {
        const long long gAn = clampg(gA + 2 * nwaves), gBn = clampg(gB + 2 * nwaves);
        const int pnA = load_index(gAn);                 // x, c of A are consumed: its next item's index first, the row later
        f32x16 h1A[T1], h1B[T1], h2A[T2], h2B[T2], accA[T3], accB[T3];
        ActSplit s1A[T1], s1B[T1], s2A[T2], s2B[T2];
        // L1(A) | input split of B
        mlp_layer_host<T1, 1, false, 1>(w1, b1, s0A, h1A, lane, h, [&](int i) __attribute__((always_inline)) {
            if (i == 0) input_split(xB, cB, s0B[0]);
        });
        const int pnB = load_index(gBn);
        // L1(B) | ReLU + split of A's first layer
        mlp_layer_host<T1, 1, false, 1>(w1, b1, s0B, h1B, lane, h, [&](int i) __attribute__((always_inline)) {
            constexpr int NP = T1 * 8, NS = T1 * 2;
            split_pieces<T1>(h1A, s1A, i * NP / NS, (i + 1) * NP / NS);
        });
        // L2(A) | ReLU + split of B's first layer
        mlp_layer_host<T2, T1, false, 2>(w2, b2, s1A, h2A, lane, h, [&](int i) __attribute__((always_inline)) {
            constexpr int NP = T1 * 8, NS = T2 * T1 * 2;
            split_pieces<T1>(h1B, s1B, i * NP / NS, (i + 1) * NP / NS);
        });
        load_x0(gAn, pnA, xA, cA);                       // in flight under the next layers
        // L2(B) | ReLU + split of A's second layer
        mlp_layer_host<T2, T1, false, 2>(w2, b2, s1B, h2B, lane, h, [&](int i) __attribute__((always_inline)) {
            constexpr int NP = T2 * 8, NS = T2 * T1 * 2;
            split_pieces<T2>(h2A, s2A, i * NP / NS, (i + 1) * NP / NS);
        });
        load_x0(gBn, pnB, xB, cB);
        // L3(A) | ReLU + split of B's second layer
        mlp_layer_host<T3, T2, true, 2>(w3, b3, s2A, accA, lane, h, [&](int i) __attribute__((always_inline)) {
            constexpr int NP = T2 * 8, NS = T3 * T2 * 2;
            split_pieces<T2>(h2B, s2B, i * NP / NS, (i + 1) * NP / NS);
        });
        // L3(B) | pool of A (its MFMAs were queued before this layer's), then the input split of A's next item
        mlp_layer_host<T3, T2, true, 2>(w3, b3, s2B, accB, lane, h, [&](int i) __attribute__((always_inline)) {
            constexpr int NS = T3 * T2 * 2, first = NS / 4;          // leave the first steps to A's last MFMAs
#pragma unroll
            for (int t = 0; t < T3; ++t)
                if (i == first + t * ((NS - first - 1) / T3)) pool_tile(accA, t, gA);
            if (i == NS - 1) input_split(xA, cA, s0A[0]);
        });
        // pool of B: nothing left to hide it under
#pragma unroll
        for (int t = 0; t < T3; ++t) pool_tile(accB, t, gB);
        gA += 2 * nwaves;
        gB += 2 * nwaves;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------
// the instantiated tile configurations, smallest first: X(t1, t2, t3)
#define PN2_RESIDENT_SHAPES(X) X(1, 1, 2) X(2, 2, 4) X(2, 3, 4)

size_t mlp_resident_w_floats(const MlpResidentConfig &c) { return mlp_w_floats(c.t1, 1) + mlp_w_floats(c.t2, c.t1) + mlp_w_floats(c.t3, c.t2); }
size_t mlp_resident_b_floats(const MlpResidentConfig &c) { return mlp_b_floats(c.t1) + mlp_b_floats(c.t2) + mlp_b_floats(c.t3); }
static size_t resident_lds_bytes(const MlpResidentConfig &c) { return sizeof(float) * (mlp_resident_w_floats(c) + mlp_resident_b_floats(c)); }

// smallest instantiated tile configuration that covers (c1, c2, c3) with a one-tile input, if its weights fit in LDS;
// padded channels carry zero weights and zero bias, cost MFMA time and never reach memory
bool mlp_resident_pick(int cin, int c1, int c2, int c3, MlpResidentConfig &cfg)
{
    if (cin > 32) return false;
#define PN2_RESIDENT_FITS(A, B, C)                                                \
    if (c1 <= 32 * A && c2 <= 32 * B && c3 <= 32 * C) {                           \
        cfg = {A, B, C};                                                          \
        return resident_lds_bytes(cfg) <= (size_t)kMlpMaxLds;                     \
    }
    PN2_RESIDENT_SHAPES(PN2_RESIDENT_FITS)
#undef PN2_RESIDENT_FITS
    return false;
}

// xyz_first: see pn2_sa_mlp3_pack (include/pn2ops.h); the kernel's channel order of layer 1 is [xyz, features]
void mlp_resident_pack(const MlpResidentConfig &c, int cin, int c1, int c2, int c3, int xyz_first, const float *const *ws,
                       const float *const *bs, float *wpacked, float *bpacked)
{
    const int cfeat = cin - 3;
    const int kin[3] = {cin, c1, c2}, nout[3] = {c1, c2, c3};
    const int tin[3] = {1, c.t1, c.t2}, tout[3] = {c.t1, c.t2, c.t3};
    int krow[32];
    for (int k = 0; k < 32; ++k) krow[k] = (!xyz_first && k < cin) ? (k < 3 ? cfeat + k : k - 3) : k;
    float *wp = wpacked, *bp = bpacked;
    for (int L = 0; L < 3; ++L) {
        for (int t = 0; t < tout[L]; ++t)
            for (int u = 0; u < tin[L]; ++u) wp = mlp_pack_pair_x6(wp, ws[L], kin[L], nout[L], t, u, L == 0 ? krow : nullptr);
        bp = mlp_pack_bias(bp, bs[L], nout[L], tout[L]);
    }
}

template <int T1, int T2, int T3>
static int launch_mlp(int b, int n, int m, int nsample, int cfeat, int c3, const float *xyz, const float *new_xyz,
                      const float *points, const int *idx, const float *wp, const float *bp, float *out, hipStream_t st, int variant,
                      int pooling, const int *npoints)
{
    const size_t lds = resident_lds_bytes({T1, T2, T3});
    if (lds > (size_t)kMlpMaxLds) return PN2_E_TOO_LARGE;
    const long long rows = (long long)b * m;
    const bool half = nsample == 16;
    const long long groups = half ? (rows + 1) / 2 : rows;
    // two items per wave (sa_mlp3_pair_kernel): one 32-sample group per centroid, at most 16 input channels
    // (variant: 0 by the size rule below, 1 never, 2 / 3 wherever the kernel covers the shape: four / eight waves per workgroup)
    const bool pair_ok = (nsample == 32 || nsample == 16) && 3 + cfeat <= 16 && T2 <= 2;      // (T2 = 3: two items' state spills)
    // size rule (measured, profiles/r04/mlp_two_items.txt): eight waves x two items is 6-8 % faster than eight waves x one from
    // ~8k items (metric shape 139 -> 131 us, cls_ssg SA1 36 -> 33), neutral below; four waves x two items is no faster than
    // one item per wave (142 us): kept for tests / A-B only
    if (variant == 0 && pair_ok && groups >= 8192) variant = 3;
    // persistent (at most 256 workgroups): every workgroup stages the weights once, its waves share that copy
    auto run = [&](auto kern, int threads, int items_per_wave) -> int {
        const int per_block = threads / 64 * items_per_wave;
        const long long blocks = (groups + per_block - 1) / per_block;
        if (int rc = allow_dynamic_lds(kern, lds)) return rc;
        return launch(kern, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(threads), lds, st, n, m, nsample, cfeat, c3, rows, xyz,
                      new_xyz, points, idx, wp, bp, out, npoints);
    };
    if (npoints) {
        // the ragged twins: the dense choice above (from the padded extents), max pooling only
        if (pooling != 0) return PN2_E_ARG;
        if (pair_ok && variant >= 2) {
            if constexpr (T2 <= 2) {
                if (variant == 2)
                    return run(half ? sa_mlp3_pair_kernel<T1, T2, T3, 16, 256, true> : sa_mlp3_pair_kernel<T1, T2, T3, 32, 256, true>, 256, 2);
                return run(half ? sa_mlp3_pair_kernel<T1, T2, T3, 16, 512, true> : sa_mlp3_pair_kernel<T1, T2, T3, 32, 512, true>, 512, 2);
            }
        }
        return run(half ? sa_mlp3_kernel<T1, T2, T3, 16, 512, 0, true> : sa_mlp3_kernel<T1, T2, T3, 32, 512, 0, true>, 512, 1);
    }
    if (pooling != 0) {
        // avg / weighted_avg / max_and_avg (pointnet_util.py:130-140): one item per wave, eight waves (sa_mlp3_kernel<.., POOL>)
#define PN2_POOL_CASE(P) \
        if (pooling == P) return run(half ? sa_mlp3_kernel<T1, T2, T3, 16, 512, P> : sa_mlp3_kernel<T1, T2, T3, 32, 512, P>, 512, 1);
        PN2_POOL_CASE(1) PN2_POOL_CASE(2) PN2_POOL_CASE(3)
#undef PN2_POOL_CASE
        return PN2_E_ARG;
    }
    if (pair_ok && variant >= 2) {
        if constexpr (T2 <= 2) {
            if (variant == 2)                                         // four waves x two items
                return run(half ? sa_mlp3_pair_kernel<T1, T2, T3, 16, 256> : sa_mlp3_pair_kernel<T1, T2, T3, 32, 256>, 256, 2);
            // eight waves x two items (fits 256 registers)
            return run(half ? sa_mlp3_pair_kernel<T1, T2, T3, 16, 512> : sa_mlp3_pair_kernel<T1, T2, T3, 32, 512>, 512, 2);
        }
    }
    // eight waves x one item (two waves per SIMD: one wave's operand splitting overlaps the other's MFMAs) when a wave fits
    // in 256 registers
    return run(half ? sa_mlp3_kernel<T1, T2, T3, 16, 512> : sa_mlp3_kernel<T1, T2, T3, 32, 512>, 512, 1);
}

int mlp_resident_launch(const MlpResidentConfig &c, int b, int n, int m, int nsample, int cfeat, int c3, const float *xyz,
                        const float *new_xyz, const float *points, const int *idx, const float *wp, const float *bp,
                        float *out, hipStream_t st, int variant, int pooling, const int *npoints)
{
#define PN2_RESIDENT_LAUNCH(A, B, C)                 \
    if (c.t1 == A && c.t2 == B && c.t3 == C)         \
        return launch_mlp<A, B, C>(b, n, m, nsample, cfeat, c3, xyz, new_xyz, points, idx, wp, bp, out, st, variant, pooling, npoints);
    PN2_RESIDENT_SHAPES(PN2_RESIDENT_LAUNCH)
#undef PN2_RESIDENT_LAUNCH
    return PN2_E_TOO_LARGE;
}

}  // namespace pn2
