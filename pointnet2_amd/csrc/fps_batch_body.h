// fps_batch_body.h -- farthest point sampling with SEVERAL samples per arg-max exchange and a wave of its own for the
// arg-max chain (round 6).
//
// Same results as fps_pruned_body / fps_reg_body / the reference kernel (tf_sampling_g.cu:105-170), bit for bit. What changes is
// the shape of the chain. In every other tier a sample costs one workgroup-wide arg-max: a six-step wave ladder, an LDS write, a
// barrier, an LDS read, a tournament, a mirror read -- ~700 dependent cycles of which the distance update is ~120. Here the
// workgroup exchanges a short LIST of candidates once per BATCH; one more wave, the PICKER, then works through the list on its
// own -- one wave ladder and nine vector instructions per sample, no barrier, no LDS trip on its path -- for as many samples as
// the list provably determines (~20 on the bench clouds once the chain is past its first quarter), while the UPDATER waves
// apply the samples to the slots as they appear. Measured (profiles/r06/fps_batch.txt): 4096 -> 1024 220 us against the pruned
// tier's 366, 8192 -> 1024 247 against 416.
//
// Why a list determines several samples. Let td[] be the running distances after j samples, ordered by the reference's key
// (value, then smaller tie rank). Fix a threshold theta below the current maximum. A point whose value is below theta can never
// become a sample while the sample values stay >= theta, because running distances only fall. So as long as the next sample's
// value is >= theta, the next sample is the best of the points that are >= theta NOW, after lowering their values by the samples
// taken since -- and those are few: the points near the covering radius. The batch ends when the best listed candidate falls
// below the bound; everything taken until then is exactly the reference's sequence (scripts/fps_batch_sim.py checks the rule
// against the oracle; tests/test_fps_batch_model.py is the CPU model of this file's arithmetic).
//
// Organisation. 576 threads: waves 0..7 are the updaters -- they hold the slots as the pruned tier deals them (fps_pruned_prologue
// on 512 threads: 32 spatial groups, four per wave, rank-ordered LDS mirror, group boxes) --, wave 8 is the picker. EIGHT updater
// waves, two per SIMD, because a lone wave issues one instruction per ~5-8 cycles whatever its kind (vector, scalar, branch) and
// the apply loop is half scalar work: two waves share a SIMD's vector and scalar issue (four updater waves of twice the slots:
// +14 % on the whole chain).
//   * EARLY. The first PN2_BT_EARLY samples are taken one per exchange (the full tier's round on the updaters; the picker sits
//     them out at the barriers): while the farthest-point distance still halves every few samples a list yields three or four.
//   * COLLECT (updaters, once per batch). Every lane computes the best key and the second-best VALUE of its P slots. Lanes whose
//     best value is >= theta are candidate lanes: at most 64 / W per wave -- a wave with more raises its own threshold by
//     bisection on the value bits, a wave with none (or with too many equal values) falls back to its exact best lane (one
//     64-bit wave ladder). A candidate lane writes its best key to the wave's part of the list; the BOUND -- the smallest
//     value bits a sample must have for the list to be complete -- is the maximum over the waves of their thresholds and of
//     (second-best value + 1 ulp) of their candidate lanes: ONE word of the batch that every wave raises (an LDS atomic maximum
//     on the fp32 bit patterns: the values are >= 0; issued as a plain ds_max_u32 -- hipcc turns atomicMax into a readlane loop
//     over the active lanes; same-address atomics of several waves serialise in the LDS unit in a few cycles each). The waves'
//     candidate counts go into one total the same way (ds_add_u32). One barrier, the only one of the batch.
//     The second-best value comes from triples of slots (v_max3 / v_med3: 9 instructions at eight slots for 16,
//     PN2_BT_SEC3). The common outcome -- between 1 and 64 / W lanes reach theta -- is decided on the scalar popcount of the
//     ballot and goes straight to the list write with exec set from the ballot mask; bisection and the exact fallback stand
//     beside that way with a copy of the write (PN2_BT_CTAIL): 43 instructions from the first v_max_f64 to the barrier for 77
//     (profiles/fps_updaters/README.md).
//   * READ (picker, behind the barrier). Lane i takes place i of the list: the key's high word is the value, its low word the
//     mirror row (x, y, z, k). The places no wave filled hold the invalid key (a negative word | row 0) that the picker wrote there a
//     batch earlier, in its idle time, so there is no count per wave to load and compare; bound and total come with one 8-byte
//     load, and one 16-byte store clears the other parity's bound, total and count (profiles/fps_turnaround/README.md).
//   * PICK (picker). Per sample, hand-scheduled (the
//     asm block below: 32 instructions, no pad; 33 measured ~273 cycles at 4096 rank slots against 291 for the 40 before --
//     profiles/fps_picker/README.md): the winner lane alone (exec = one lane) stores its (x, y, z, k) row and then adds 1 to the
//     count in LDS, hands its coordinates to scalar registers (three v_readfirstlane inside that window) and leaves the contest; the
//     reference's distance (tf_sampling_g.cu:141-144) from the
//     sample to the other candidates, nine vector instructions; and, interleaved with those, the 32-bit wave ladder
//     (v_max_i32 with the DPP operand folded in) over the values as they were BEFORE the update -- values only fall, so a lane
//     that still holds that maximum afterwards is the arg-max if it is the only one (99 % of the samples); otherwise the exact
//     arg-max (value ladder, 64-bit keys among equal values, the pruned tier's ladder). A sample is accepted while its value
//     bits are >= the bound; the first sample of a batch always is: the list holds every updater wave's best lane, so its
//     maximum is the global one. The loop counts nothing: a list has at most 64 valid lanes, so it ends by the bound exit; only a
//     batch that could pass the end of the output row (fewer than 64 samples left) runs the compiler's counted form.
//   * APPLY (updaters, behind the picker). A wave polls the count and reads, in the same LDS round trip, its lanes' ring rows
//     (row done + the lane's sample, clamped to the ring: PN2_BT_RING1) -- two reads back to back, one wait: LDS serves a wave's
//     operations in order and the picker stores a row before it adds to the count, so what lies below the count read is
//     complete and the lanes beyond it leave by the np mask. It takes up to CH = 64 / GW new samples at a time -- lane l tests
//     sample l % CH against the box of the wave's group l / CH: one distance-to-box computation for 64 (sample, group) pairs --
//     and updates the touched groups, group by group (packed fp32, as in the pruned tier; no key work: keys are only needed at
//     COLLECT). A group's bits of the touched mask are one field of a scalar word and a bit's number is the lane that holds
//     the sample (PN2_BT_GBITS): an untouched group costs a field extract and a branch, a sample s_ff1, s_bitset0 and the
//     loop's compare. The skip test uses the value of the previous batch's LAST sample as v* (no running distance is above it).
//   * theta = (1 - g) * (value of the last sample); g adapts so that the list stays about half full. The picker decides
//     and publishes theta with the end-of-batch flag (behind the last pick, where the updaters are still applying: moved
//     ahead of the sample loop the adaptation sits on the chain and cost the metric 3 % -- profiles/fps_turnaround/README.md).
//
// Once a sample's value is 0 every running distance is 0 and the reference keeps selecting point 0 (its tie rule): the rest of
// the output is filled directly. A cloud on which a point still stands at the start value 1e38 at the end of the early rounds --
// every cloud with a NaN or infinite coordinate -- gets no lists at all (the updaters' branch, "NO LISTS").
//
// Exactness of the acceptance rule in fp32 bit patterns: values are non-negative floats, so integer comparison of the bits is
// the value order; "value > second-best" is "bits >= second-best bits + 1". A sample with value bits >= the maximum of the waves'
// bounds beats (by value alone, no tie rule needed) every point that is not a listed candidate's best point; among the listed
// ones the 64-bit keys decide, ties included. Degenerate clouds with many EQUAL values at the top (lattices) make short batches
// (the bound is strict), never different samples.
//
// Hand-offs inside the workgroup: LDS only. The picker's row store and count store come from the same lane (LDS executes a
// wave's operations in order), counts are release stores / acquire loads at workgroup scope. Double-buffered by batch parity:
// list, bound, total and the header; the sample ring is single (a batch's samples are consumed before the next barrier).
// Chains of different clouds now differ in length (the lists are the data's): 248-261 us over the 32 clouds of a bench batch.
#pragma once
#include "fps_pruned_body.h"

namespace pn2 {

constexpr int kBtCand = PN2_WAVE;              // 64 candidates = the picker's lanes: 64 / W candidate lanes per updater wave
constexpr int kBtMaxW = 8;                     // updater waves: 4 (one per SIMD) or 8 (two per SIMD)
#ifndef PN2_BT_UT
#define PN2_BT_UT 512                          // updater threads of the product
#endif
constexpr int kBtUT = PN2_BT_UT;
constexpr int kBtT = kBtUT + PN2_WAVE;         // + the picker
constexpr unsigned kBtEnd = 0x100u, kBtFill = 0x200u, kBtCountMask = 0xffu;

struct BtXchg {
    double list[kBtCand];                      // wave w's candidates from w * cap on, cap = 64 / W; the other places hold the invalid key
    unsigned cnt[kBtMaxW];                     // lab only (PN2_BT_READ1 = 0): one count and one bound word per updater wave
    unsigned bound[kBtMaxW];
    // one 16-byte row that the picker clears in one store and reads (bmax, total) in one 8-byte load
    unsigned bmax;                             // the batch's bound: LDS maximum over every wave's threshold and candidate lanes
    unsigned total;                            // candidate lanes of the batch, all waves (LDS add): only the adaptation of g reads it
    unsigned count;                            // samples of this batch published so far | kBtEnd | kBtFill
    unsigned spare0;
    unsigned single;                           // after this batch: that many samples one per exchange (SLOW BATCHES below)
    unsigned theta, vlast;                     // for the NEXT collect: threshold bits, value bits of the batch's last sample
    unsigned spare1;
};
static_assert(sizeof(BtXchg) == 8 * kBtCand + 8 * kBtMaxW + 32, "the size the LDS budget of every geometry was measured with");
static_assert(sizeof(BtXchg) % 16 == 0 && offsetof(BtXchg, bmax) % 16 == 0, "16-byte rows");

// P = slots per updater thread, UT = updater threads
__host__ __device__ constexpr size_t fps_batch_xchg_offset(int P, int UT = kBtUT) { return (fps_pruned_lds_bytes(P, UT) + 15) & ~(size_t)15; }
__host__ __device__ constexpr size_t fps_batch_lds_bytes(int P, int UT = kBtUT) { return fps_batch_xchg_offset(P, UT) + 2 * sizeof(BtXchg) + 16 * kBtCand; }

__device__ __forceinline__ float vmax_f32(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmed3_f32(float a, float b, float c)
{
    float r;
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ float vmax3_f32(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// The second largest (as a multiset) of P running distances. Leaves are TRIPLES of slots -- (v_max3, v_med3) are the two largest
// of three --, two left over make a pair (v_max, v_min), one left over joins at the end; three (largest, second) pairs merge into
// max3 of the largest and max(med3 of the largest, max3 of the seconds): a second that does not belong to the overall largest is
// below its own largest, which is at most the median. The last merge needs no largest. 1 / 3 / 9 / 19 instructions at 2 / 4 / 8 /
// 16 slots against 2 / 6 / 16 / 36 for the network of pairs. Running distances are never NaN (v_min_f32 keeps the non-NaN
// operand and they start at 1e38) and never -0, so every form returns the same bits.
template <int P>
__device__ __forceinline__ float bt_second_best(const float (&v)[P])
{
    static_assert(P == 2 || P == 4 || P == 8 || P == 16, "slots per updater thread");
    constexpr int NT = P / 3, REM = P % 3, K = NT + (REM == 2 ? 1 : 0), KF = K >= 3 ? 3 : K;   // pairs, pairs at the last merge
    float h[K > 0 ? K : 1], l[K > 0 ? K : 1];
#pragma unroll
    for (int i = 0; i < NT; ++i) { h[i] = vmax3_f32(v[3 * i], v[3 * i + 1], v[3 * i + 2]); l[i] = vmed3_f32(v[3 * i], v[3 * i + 1], v[3 * i + 2]); }
    if constexpr (REM == 2) { h[NT] = vmax_f32(v[P - 2], v[P - 1]); l[NT] = vmin_f32(v[P - 2], v[P - 1]); }
    int k = K;
#pragma unroll
    while (k > 3) {                                 // (16 slots: five pairs) the last three into one
        const float hm = vmed3_f32(h[k - 3], h[k - 2], h[k - 1]), lm = vmax3_f32(l[k - 3], l[k - 2], l[k - 1]);
        h[k - 3] = vmax3_f32(h[k - 3], h[k - 2], h[k - 1]);
        l[k - 3] = vmax_f32(hm, lm);
        k -= 2;
    }
    if constexpr (REM == 1) {                       // one slot left over: merge all the way, then the median of (largest, second, slot)
        if constexpr (KF == 3) {
            const float hm = vmed3_f32(h[0], h[1], h[2]), lm = vmax3_f32(l[0], l[1], l[2]);
            h[0] = vmax3_f32(h[0], h[1], h[2]);
            l[0] = vmax_f32(hm, lm);
        }
        return vmed3_f32(h[0], l[0], v[P - 1]);
    } else {
        if constexpr (KF == 3) return vmax_f32(vmed3_f32(h[0], h[1], h[2]), vmax3_f32(l[0], l[1], l[2]));
        else return l[0];
    }
}

// wave-wide signed maximum, result in lane 63: the DPP operand rides on the v_max itself (VOP2), one instruction per step.
// Lanes without a source (bound_ctrl:0 reads 0) combine with 0 -- harmless for a maximum of values of which at least one is >= 0.
__device__ __forceinline__ int bt_wave_max_i32_lane63(int v)
{
    // written with the builtin so that the compiler folds the v_mov_dpp into the v_max (GCNDPPCombine), keeps track of the DPP
    // hazards itself and schedules independent work into the wait states
#define PN2_BT_STEP(ctrl) v = max(v, __builtin_amdgcn_update_dpp(0, v, ctrl, 0xf, 0xf, true))
    PN2_BT_STEP(0xB1);    // quad_perm:[1,0,3,2]
    PN2_BT_STEP(0x4E);    // quad_perm:[2,3,0,1]
    PN2_BT_STEP(0x141);   // row_half_mirror
    PN2_BT_STEP(0x140);   // row_mirror
    PN2_BT_STEP(0x142);   // row_bcast:15
    PN2_BT_STEP(0x143);   // row_bcast:31
#undef PN2_BT_STEP
    return v;
}

// The key of a list place that no wave filled: the DOUBLE -1.0, high word 0xBFF00000, low word 0. As a candidate value the high
// word is the float -1.875: negative, so below every value as an integer like the -1.0f (0xBF800000) a taken lane holds, and kept
// by v_min_f32 against any distance; the low word is mirror row 0. The word 0xBF800000 itself would do the same and was measured
// 0.002 ms per step slower on the benchmark (-1.0 is an inline constant of the 64-bit move; the other pattern takes two literal
// moves and a register pair that lives across the batch loop): profiles/fps_turnaround/README.md.
__device__ __forceinline__ double kBtInvalidKey() { return -1.0; }

// NO LISTS (the updaters' branch of the body): did the last sample but one of the early rounds still have the start value 1e38?
// Read behind the last early round's barrier by every wave, the picker included; written once, in front of that barrier. Fewer
// than two early rounds (a lab build, or a row of one or two samples, which has no lists anyway) leave the rule off.
__device__ __forceinline__ bool bt_stands_at_start(const BtXchg *xch, int jE)
{
    return jE >= 3 && __builtin_amdgcn_readfirstlane((int)xch[0].spare1) == __float_as_int(1e38f);
}

// LDS atomic maximum without the compiler's wave-level pre-reduction (a readlane loop over the active lanes: ~50 cycles per
// lane on a lone wave; the LDS unit serialises same-address atomics in a few cycles each)
__device__ __forceinline__ void lds_max_u32(unsigned *p, unsigned v)
{
    asm volatile("ds_max_u32 %0, %1" :: "v"((unsigned)(size_t)p), "v"(v) : "memory");
}

// LDS add without a return value: same-address adds of several waves serialise in the LDS unit like the maxima above
__device__ __forceinline__ void lds_add_u32(unsigned *p, unsigned v)
{
    asm volatile("ds_add_u32 %0, %1" :: "v"((unsigned)(size_t)p), "v"(v) : "memory");
}

// Where the batched tier exists and pays (measured, profiles/r06/fps_batch.txt): 513..8192 rank slots (1024 / 2048: 8 / 16 groups,
// 4096 / 8192: 32). Its grouping prologue costs 2-10 us more than the full tier's staging, its first PN2_BT_EARLY samples cost the
// full tier's round, from ~200 samples on a sample is 160-175 ns against 250-390. npoint = 256: 61 us against 67 (full) at 1024
// rank slots, 68 / 81 at 2048, 84 / 102 at 4096, 109 / 134 (pruned) at 8192; npoint = 128: no gain anywhere.
inline bool fps_batch_covers(int ranks) { return ranks > 512 && ranks <= 8192; }
#ifdef PN2_BT_LAB_NEVER_AUTO      // A/B library: the size rule never chooses this tier (scripts/: what did the tier change in a model?)
inline bool fps_batch_pays(int, int) { return false; }
#else
inline bool fps_batch_pays(int ranks, int m) { return fps_batch_covers(ranks) && m >= 256; }
#endif

#ifdef PN2_BT_STATS
// lab: [0] batches, [1] samples, [2] exact fallbacks, [3] bisection steps, [4] sum of list sizes, [5] (group, sample) updates,
// [6] picker cycles in READ, [7] picker cycles in PICK, [8] picker cycles waiting at the barrier, [9] updater 0 cycles in COLLECT,
// [10] updater 0 cycles from the barrier to the end flag, [11] tie resolutions, [12] speculation misses, [13] samples taken one per
// exchange after slow batches, [14] such runs; updater 0: [15] cycles from seeing the end flag to arriving at the next list barrier
// (epilogue + COLLECT), [16] chunks, [17] polls that found nothing, [18] (group, sample) updates taken on the dense path, [19] cycles
// around the poll's wait (count word; with PN2_BT_RING1 the ring row too), [20] from there to the ring row's arrival (readfirstlane,
// compare, branch, the chunk counter's atomic and, without PN2_BT_RING1, the row's own round trip), [21] two clock reads back to back,
// all three per chunk and only with PN2_BT_STATS_CHUNK (default 1: the three clock reads and atomics per chunk make updater 0 later
// than it is -- the per-wave figures that follow are taken with 0); every updater wave w:
// [24 + w] cycles behind the first arriver at the list barrier, [32 + w] times it was the last to arrive
__device__ unsigned long long g_bt_stats[40];
#ifndef PN2_BT_STATS_FROM
#define PN2_BT_STATS_FROM 0
#endif
#ifndef PN2_BT_STATS_CHUNK
#define PN2_BT_STATS_CHUNK 1
#endif
#define PN2_BT_STAT(i, v) do { if (lane == 0 && cloud == 0 && j >= PN2_BT_STATS_FROM) atomicAdd(&g_bt_stats[i], (unsigned long long)(v)); } while (0)
#define PN2_BT_CLOCK() __builtin_readcyclecounter()
#else
#define PN2_BT_STAT(i, v) do { } while (0)
#define PN2_BT_CLOCK() 0ll
#pragma clang diagnostic ignored "-Wunused-variable"
#endif

#ifndef PN2_BT_LIST_HI
#define PN2_BT_LIST_HI 36      // measured: 44 / 28 +1.7 %, 54 / 40 +6 %, 28 / 14 +2 %, 20 / 10 +7 % (profiles/r06/fps_batch.txt)
#define PN2_BT_LIST_LO 20
#endif
#ifndef PN2_BT_EARLY
#define PN2_BT_EARLY 48            // the first samples of a cloud are taken one per exchange (below; 32 / 64 / 96 measured: 255.7 / 255.5 / 261.9 us, none: 280.4)
#endif
#ifndef PN2_BT_ASM_LOOP
#define PN2_BT_ASM_LOOP 1
#endif
// lab switches of the hand-scheduled sample loop (each cut measured alone: profiles/fps_picker/README.md)
#ifndef PN2_BT_RFL
#define PN2_BT_RFL 1                 // the winner's coordinates by v_readfirstlane while exec is its lane (0: s_ff1 + three v_readlane)
#endif
#ifndef PN2_BT_NOCTR
#define PN2_BT_NOCTR 1               // no sample counter in the loop: the bound exit ends a list (0: s_add / s_cmp / s_cbranch per sample)
#endif
#ifndef PN2_BT_FILL
#define PN2_BT_FILL 1                // the add of na in the ladder's last wait state, the two pads no rule asks for dropped (0: three s_nop)
#endif
// lab switches of the hand-over between two lists (each cut measured alone: profiles/fps_turnaround/README.md)
#ifndef PN2_BT_READ1
#define PN2_BT_READ1 1               // READ: one bound word and one total for the batch, unused list places preset to the invalid key (0: a count and a bound word per wave, reduced by the picker)
#endif
#ifndef PN2_BT_CADD
#define PN2_BT_CADD 1                // sample loop: the count word by ds_add_u32, bh = ms in the wait state the add of na filled (0: ds_write_b32 of na, v_add_u32 na, s_mov on the back edge)
#endif
// lab switches of the updater waves' cuts (each measured alone: profiles/fps_updaters/README.md)
#ifndef PN2_BT_SEC3
#define PN2_BT_SEC3 1                // COLLECT: the second-best value over triples of slots, v_max3 / v_med3 (0: pairs, v_max / v_min / v_med3 per node)
#endif
#ifndef PN2_BT_CTAIL
#define PN2_BT_CTAIL 1               // COLLECT: 0 < cnt <= CAP goes straight to the list write, exec set from the ballot mask (0: one tail behind bisection and fallback, (mask >> lane) & 1 in vector registers)
#endif
#ifndef PN2_BT_GBITS
#define PN2_BT_GBITS 1               // APPLY: lane l tests sample l % CH against group l / CH, so a group's bits of the touched mask are one 32-bit field whose bit numbers are lane numbers (0: sample l / GW, group l % GW, strided 64-bit masks)
#endif
// lab switches of the APPLY chunk's LDS reads (each measured alone: profiles/fps_apply/README.md)
#ifndef PN2_BT_RING1
#define PN2_BT_RING1 1               // APPLY: the lane's ring row read behind the count word, one wait for both (0: the row read waits for the count, two dependent LDS round trips per chunk)
#endif
#ifndef PN2_BT_SSRC
#define PN2_BT_SSRC 1                // APPLY: the sample as an SGPR pair of the packed subtract, op_sel_hi:[1,0] (0: v_readlane + v_mov into the low half of a register pair)
#endif
#ifndef PN2_BT_G0
#define PN2_BT_G0 0.10f               // initial 1 - theta / (last sample value)
#endif
// SLOW BATCHES. A batch costs a COLLECT + a barrier + a list read whatever it yields (~0.6 us), and a sample whose arg-max needs
// the 64-bit keys costs three times the speculative one; the classic round is 0.39 us at 4096 rank slots. Clouds with many EQUAL
// values at the top (lattices, coordinates quantised to a coarse grid, duplicated points) end most batches after a sample or two
// -- the bound is strict -- or resolve ties at every sample, and the tier then costs 1.2-2 x the full tier's chain
// (profiles/r06/fps_tier_by_cloud.txt: 493 / 694 / 778 us against 395 at 4096 -> 1024). The picker therefore CLOCKS both forms:
// the EARLY rounds give the cost of a one-per-exchange round on this cloud and this device, the interval between two list
// barriers the cost of a batch. When the batches of a run (decayed sums) cost more per sample than the round -- 1.5 x the round
// while fewer than PN2_BT_SLOW_MIN batches have been clocked --, the workgroup takes the next R samples one per exchange (the
// EARLY round), then tries batches again; R doubles (16 .. 512) while the batches stay slow and starts over after eight batches
// in a row that pay. Same samples either way -- both
// forms are the reference's arg-max; only the schedule depends on the clock.
#ifndef PN2_BT_PACKED_FROM
#define PN2_BT_PACKED_FROM 16       // the one-per-exchange round on register PAIRS from this many slots per thread (all sizes packed: 1024 -> 1024 182 -> 190 us)
#endif
#ifndef PN2_BT_SLOW_MIN
#define PN2_BT_SLOW_MIN 3
#define PN2_BT_QUICK 1
#define PN2_BT_SINGLE0 16
#define PN2_BT_SINGLE1 512
#endif

template <int P, int GS, bool PUBLISH, int UT = kBtUT>
__device__ __forceinline__ void fps_batch_body(int n, int m, int Q, int cloud, const float *__restrict__ xyz,
                                               int *__restrict__ out, float *__restrict__ out_xyz,
                                               unsigned long long *__restrict__ tagged, char *smem, unsigned tag = 1u)
{
    constexpr int W = UT / PN2_WAVE, NS = UT * P;      // updater waves, rank slots
    constexpr int GW = P / GS;                         // groups per updater wave
    constexpr int CAP = kBtCand / W;                   // candidate lanes per updater wave
    constexpr int BT = UT + PN2_WAVE;                  // threads of the workgroup
    constexpr int CH = PN2_WAVE / GW;                  // samples per APPLY chunk: one lane per (sample, group) pair
    constexpr bool GB = PN2_BT_GBITS && GW > 1;        // lane l: sample l % CH, group l / CH (else sample l / GW, group l % GW; one group: the same)
    static_assert((W * GW == 32 && (W == 4 || W == 8)) || (W == 8 && (GW == 2 || GW == 1)),
                  "32 groups on four or eight updater waves; 16 / 8 groups (2048 / 1024 rank slots) on eight");
    float4 *lds_rank = reinterpret_cast<float4 *>(smem + 256);
    BtXchg *xch = reinterpret_cast<BtXchg *>(smem + fps_batch_xchg_offset(P, UT));
    float4 *ring = reinterpret_cast<float4 *>(smem + fps_batch_xchg_offset(P, UT) + 2 * sizeof(BtXchg));   // [kBtCand] samples of the batch: x, y, z, k

    const float *__restrict__ src = xyz + (size_t)cloud * n * 3;
    int *__restrict__ dst = out + (size_t)cloud * m;
    float *__restrict__ dxyz = out_xyz ? out_xyz + (size_t)cloud * m * 3 : nullptr;
    pn2_gu64 *gtag = PUBLISH ? (pn2_gu64 *)(tagged + (size_t)cloud * m) : nullptr;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);

    int j = 1;                                   // samples written so far (wave-uniform, the same in every wave)
    const int jE = min(PN2_BT_EARLY, m);         // samples 1 .. jE - 1 are taken one per exchange
    int fill_k = -1;                             // >= 0: the cloud ran out of distinct points at sample j, the rest is this index

    if (w == W) {
        // ================================================ the picker ===========================================================
#ifndef PN2_NO_SETPRIO
        __builtin_amdgcn_s_setprio(3);           // it shares SIMD 0 with updater wave 0 and is the chain
#endif
        for (int i = lane; i < (int)(2 * sizeof(BtXchg) / 4); i += PN2_WAVE) reinterpret_cast<unsigned *>(xch)[i] = 0u;   // counts, bounds, flags
#if PN2_BT_READ1
        xch[0].list[lane] = kBtInvalidKey();     // (below); behind the zeroes: a wave's LDS writes execute in order
        xch[1].list[lane] = kBtInvalidKey();
#endif
        for (int i = 0; i < kPrPrologueBarriers; ++i) __syncthreads();
        long long e0 = 0;
        for (; j < jE; ++j) {                    // the updaters' early rounds: one barrier each
            if (j == 8) e0 = (long long)__builtin_readcyclecounter();
            __syncthreads();
        }
        if (bt_stands_at_start(xch, jE))         // NO LISTS (the updaters' branch): their rounds to the end of the row
            for (; j < m; ++j) __syncthreads();
        // SLOW BATCHES: cycles of a one-per-exchange round (none measured: batches always pay), decayed cycles / samples of the
        // batches since the last such run, batches counted, length of the next run, clock at the previous idle point
        const float round_cyc = jE >= 24 ? (float)((long long)__builtin_readcyclecounter() - e0) / (float)(jE - 8) : 1e30f;
        // The bookkeeping runs in the picker's idle time ahead of a list barrier (the updaters are collecting), not between the last
        // pick and the end flag: a decision is published with the end flag of the batch that follows it.
        float bt_cyc = 0.f, bt_smp = 0.f;
        int bt_n = 0, bt_paid = 0, run = PN2_BT_SINGLE0, a_prev = 0, single_next = 0;
        long long qb = 0;
        float g = PN2_BT_G0;
        int par = 0;
        if (j < m)
        for (;;) {
            const long long q0 = PN2_BT_CLOCK();
#if PN2_BT_READ1
            // The NEXT batch's list, every place to the invalid key: high word negative -- below every value as an integer and kept by
            // v_min_f32 --, low word 0 -- mirror row 0. The updaters then write their candidates over it and the picker needs no
            // count per wave to tell a candidate from an empty place. Nobody else touches that buffer now: the picker took its keys
            // into registers a whole batch ago (behind the previous barrier), this batch's COLLECT writes the other parity, the
            // one-per-exchange rounds exchange through the pruned layout's wave keys, and the updaters write it again only in
            // the COLLECT that follows this batch's end flag -- a store of this wave behind this one (LDS executes a wave's
            // operations in order), which they acquire first.
            xch[par ^ 1].list[lane] = kBtInvalidKey();
#endif
            // SLOW BATCHES, in the idle time (the clock's latency too: s_memtime shares the LDS counter, behind the barrier it sat
            // on the list read): the batch that just ended into the decayed sums, then the decision
            {
                const long long qn = (long long)__builtin_readcyclecounter();
                if (bt_n > 0) {
                    bt_cyc = 0.75f * bt_cyc + (float)(qn - qb); bt_smp = 0.75f * bt_smp + (float)a_prev;
                    if (bt_n > PN2_BT_QUICK) {       // at least two whole batches of this run have been clocked
                        if (bt_cyc > bt_smp * round_cyc * (bt_n > PN2_BT_SLOW_MIN ? 1.0f : 1.5f)) {
                            single_next = run;
                            run = min(2 * run, PN2_BT_SINGLE1);
                            bt_n = -1; bt_paid = 0; bt_cyc = 0.f; bt_smp = 0.f;   // the next interval holds the run: not folded
                        } else if (++bt_paid >= 8) {
                            run = PN2_BT_SINGLE0;
                        }
                    }
                }
                qb = qn;
                ++bt_n;
            }
            __syncthreads();                     // the list of this batch is complete
            const long long q1 = PN2_BT_CLOCK();
            BtXchg &X = xch[par];
            typedef float bt_f4 __attribute__((ext_vector_type(4)));
#if PN2_BT_READ1
            // The other parity's bound, total and count, one store: everybody is past the batch that used them, and the updaters
            // raise them again only behind this batch's end flag (a later store of this wave, which they acquire first) -- written
            // behind the barrier, read by nobody before the next one, like the per-wave words this row replaces.
            if (lane == 0) *reinterpret_cast<uint4 *>(&xch[par ^ 1].bmax) = make_uint4(0u, 0u, 0u, 0u);
            const uint2 bt2 = *reinterpret_cast<const uint2 *>(&X.bmax);            // same address in every lane: LDS broadcast
            const double key = X.list[lane];
            const unsigned lowc = (unsigned)__double2loint(key);                    // an empty place: row 0
            const bt_f4 cand = *reinterpret_cast<const bt_f4 *>(&lds_rank[lowc]);   // x, y, z, bits of k
            const int boundb = __builtin_amdgcn_readfirstlane((int)bt2.x);
            const int total = __builtin_amdgcn_readfirstlane((int)bt2.y);
            int cval = __double2hiint(key);                                         // an empty place: 0xBFF00000, negative
#else
            if (lane == 0) __hip_atomic_store(&xch[par ^ 1].count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // everybody is past the batch that used it
            const uint4 c4 = *reinterpret_cast<const uint4 *>(X.cnt), c5 = *reinterpret_cast<const uint4 *>(X.cnt + 4);      // waves beyond W: 0
            const uint4 b4 = *reinterpret_cast<const uint4 *>(X.bound), b5 = *reinterpret_cast<const uint4 *>(X.bound + 4);
            const double key = X.list[lane];
            const unsigned cw = X.cnt[lane / CAP];
            const bool valid = (unsigned)(lane & (CAP - 1)) < cw;
            const unsigned lowc = valid ? (unsigned)__double2loint(key) : 0u;
            const bt_f4 cand = *reinterpret_cast<const bt_f4 *>(&lds_rank[lowc]);   // x, y, z, bits of k
            const int boundb = __builtin_amdgcn_readfirstlane((int)max(max(max(b4.x, b4.y), max(b4.z, b4.w)), max(max(b5.x, b5.y), max(b5.z, b5.w))));
            const int total = __builtin_amdgcn_readfirstlane((int)(c4.x + c4.y + c4.z + c4.w + c5.x + c5.y + c5.z + c5.w));
            int cval = valid ? __double2hiint(key) : (int)0xBF800000;             // -1.0f: below every value as an integer, kept by v_min_f32
#endif
            const int clo = (int)lowc;
            int a = 0;
            int vlastb = 0;
            bool fill = false;
            const unsigned ring_base = (unsigned)(size_t)ring, count_addr = (unsigned)(size_t)&X.count;   // LDS byte addresses
            const long long q2 = PN2_BT_CLOCK();
            int bh;
            unsigned long long eq;                                               // one bit: the winner's lane
            // the exact arg-max of the current values: value ladder, then the 64-bit keys among equal values
            auto argmax = [&]() __attribute__((always_inline)) {
                bh = __builtin_amdgcn_readlane(bt_wave_max_i32_lane63(cval), 63);
                eq = __ballot(cval == bh);
                if (__popcll(eq) != 1) {
                    PN2_BT_STAT(11, 1);
                    const double kq = cval == bh ? __hiloint2double(cval, clo) : -1.0;
                    const double km = wave_max_f64_lane63(kq);
                    const int ml = __builtin_amdgcn_readlane(__double2loint(km), 63);
                    eq = __ballot(cval == bh && clo == ml);
                    eq &= 0ull - eq;                                             // equal keys exist only among padding slots
                }
            };
            argmax();                                                            // the batch's first sample: always (the global arg-max)
            const int amax = min(m - j, kBtCand);
            unsigned raddr = ring_base, na = 1u;
            // The compiler's form of the sample loop. It is the whole loop where PN2_BT_ASM_LOOP is 0, and the loop of the batches
            // that can reach the end of the output row (PN2_BT_NOCTR below): the only form that counts its samples.
            auto pick_counted = [&]() __attribute__((always_inline)) {
                for (;;) {
                    // the winner lane alone stores its row and then the new count: two LDS writes of one wave execute in order, so a
                    // reader that sees the count sees the row (no wait in between, none behind). It also leaves the contest (-1.0f).
                    asm volatile("s_mov_b64 exec, %1\n\t"
                                 "ds_write_b128 %2, %3\n\t"
                                 "ds_write_b32 %4, %5\n\t"
                                 "v_mov_b32 %0, 0xbf800000\n\t"
                                 "s_mov_b64 exec, -1"
                                 : "+v"(cval) : "s"(eq), "v"(raddr), "v"(cand), "v"(count_addr), "v"(na) : "memory");
                    const int wl = (int)__builtin_ctzll(eq);
                    raddr += 16u; na += 1u;
                    a = __builtin_amdgcn_readfirstlane(a + 1);                   // scalar loop control
                    vlastb = bh;
                    if (a >= amax) break;
                    // SPECULATION: the maximum of the values as they are BEFORE this sample's update is computed in the shadow of the
                    // update. Values only fall: a lane that still holds that maximum afterwards is the arg-max -- if it is the only one.
                    // (A sample of value 0 ends the batch by itself: nothing is above the bound afterwards.)
                    const int ms = __builtin_amdgcn_readlane(bt_wave_max_i32_lane63(cval), 63);
                    const float sx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand.x), wl));
                    const float sy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand.y), wl));
                    const float sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand.z), wl));
                    const float d = sqdist(cand.x, cand.y, cand.z, sx, sy, sz);  // tf_sampling_g.cu:141-143
                    cval = __float_as_int(vmin_f32(d, __int_as_float(cval)));    // :144
                    if (ms < boundb) break;                                      // nothing above the bound is left, whatever the update did
                    eq = __ballot(cval == ms);
                    bh = ms;
                    if (__popcll(eq) != 1) {
                        PN2_BT_STAT(12, 1);
                        argmax();
                        if (bh < boundb) break;
                    }
                }
            };
#if PN2_BT_ASM_LOOP
            // The sample loop, hand-scheduled (the compiler's version of the same loop -- pick_counted above -- takes three taken
            // branches and six more scalar moves per sample; on a lone wave every instruction is an issue slot of ~8 cycles):
            //   publish: the winner lane alone (exec = eq) stores its row and then the new count -- two LDS writes of one wave
            //     execute in order, so a reader that sees the count sees the row; no wait in between, none behind --, hands its
            //     coordinates to the scalar registers (PN2_BT_RFL: v_readfirstlane reads the one active lane; no lane number, no
            //     v_readlane that waits for one) and leaves the contest (-1.0f);
            //   SPECULATION: the maximum of the values as they are BEFORE this sample's update is computed in the shadow of the
            //     update (the DPP steps need two independent instructions between them anyway). Values only fall: a lane that
            //     still holds that maximum afterwards is the arg-max -- if it is the only one. A sample of value 0 ends the batch by
            //     itself: nothing is above the bound afterwards.
            //   NO SAMPLE COUNTER (PN2_BT_NOCTR): a list has at most 64 valid lanes, every taken lane is -1.0f and every empty place negative too, so after the last
            //     of them the ladder's maximum is 0 (lanes without a DPP source read 0) or negative -- below the bound, which is >= 1
            //     as an integer (second-best bits + 1) -- and the loop leaves by the bound exit. The count is read back from na
            //     behind the loop. Only the end of the output row needs a count inside the loop: a batch with fewer than 64
            //     samples left to write (the last one or two of a cloud) runs pick_counted instead.
            // Wait states (inline asm gets none from the compiler; the rules are the ones hipcc pads its own code for on gfx950):
            //   a VALU write of a VGPR -> a DPP read of it: 2 (between two ladder steps: two instructions of the distance, in
            //     front of the last step the add of raddr and bh = ms, a scalar move: any instruction is a wait state --
            //     PN2_BT_FILL, PN2_BT_CADD; the winner's -1.0f is written four ahead);
            //   a VALU write of a VGPR -> v_readlane / v_readfirstlane of it: 1 (v_min_f32 stands between the ladder and ms);
            //   v_readlane / v_readfirstlane writes an SGPR -> a VALU reads it: 2 (s_cmp + s_cbranch between ms and the v_cmp;
            //     the sample's coordinates are read four or more instructions after they are written); a scalar read needs none
            //     (bh = ms reads the ms of the pass before, a whole pass after the v_readlane that wrote it);
            //   exec is written by scalar moves only (a VALU write of exec would cost the DPP steps 5).
            // reason: 0 = the batch is full / the cloud is done, 1 = nothing above the bound is left, 2 = the speculative maximum
            // is gone or not unique (the exact arg-max below decides, then the loop resumes).
#if PN2_BT_RFL
#define PN2_BT_A_WINNER_IN  "v_readfirstlane_b32 %[sx], %[cx]\n\tv_readfirstlane_b32 %[sy], %[cy]\n\tv_readfirstlane_b32 %[sz], %[cz]\n\t"
#define PN2_BT_A_LANE       ""
#define PN2_BT_A_SXY        ""
#define PN2_BT_A_SZ         ""
#else
#define PN2_BT_A_WINNER_IN  ""
#define PN2_BT_A_LANE       "s_ff1_i32_b64 %[wl], %[eq]\n\t"
#define PN2_BT_A_SXY        "v_readlane_b32 %[sx], %[cx], %[wl]\n\tv_readlane_b32 %[sy], %[cy], %[wl]\n\t"
#define PN2_BT_A_SZ         "v_readlane_b32 %[sz], %[cz], %[wl]\n\t"
#endif
#if PN2_BT_NOCTR
#define PN2_BT_A_COUNT      ""
#define PN2_BT_A_FULL       ""
#else
#define PN2_BT_A_COUNT      "s_add_i32 %[a], %[a], 1\n\t"
#define PN2_BT_A_FULL       "s_cmp_ge_i32 %[a], %[amax]\n\ts_cbranch_scc1 2f\n\t"
#endif
            // COUNT BY ADD (PN2_BT_CADD): the winner lane adds 1 to the count word (ds_add_u32, no return) instead of storing na, so
            // na and its v_add_u32 leave the loop. The word is 0 when a batch starts (the picker cleared it behind the previous
            // barrier) and holds the count alone until the end flag's store; the row store and the add come from one lane, in order,
            // like the two stores before. The wait state the add of na filled takes the back edge's s_mov (bh = ms: the value of
            // the sample just published; ms enters the block equal to bh, so the first pass changes nothing), which leaves the
            // loop's head. The count is read back from the ring address behind the loop.
#if PN2_BT_CADD
#define PN2_BT_A_PUBCOUNT   "ds_add_u32 %[caddr], %[one]\n\t"
#define PN2_BT_A_NA         ""
#else
#define PN2_BT_A_PUBCOUNT   "ds_write_b32 %[caddr], %[na]\n\t"
#define PN2_BT_A_NA         "v_add_u32 %[na], 1, %[na]\n\t"
#endif
#if PN2_BT_CADD && PN2_BT_FILL
#define PN2_BT_A_HEAD       "0:\n\t"
#define PN2_BT_A_BH         "s_mov_b32 %[bh], %[ms]\n\t"
#define PN2_BT_A_MS         "+s"
#else
#define PN2_BT_A_HEAD       "s_branch 1f\n\t0:\n\ts_mov_b32 %[bh], %[ms]\n\t1:\n\t"   /* the speculative maximum stood: it is the next sample's value */
#define PN2_BT_A_BH         ""
#define PN2_BT_A_MS         "=&s"
#endif
#if PN2_BT_FILL
#define PN2_BT_A_ADDS_EARLY ""
#define PN2_BT_A_PAD_DPP    "v_add_u32 %[raddr], 16, %[raddr]\n\t" PN2_BT_A_NA PN2_BT_A_BH   /* the two wait states in front of the last ladder step */
#define PN2_BT_A_PAD        ""
#else
#define PN2_BT_A_ADDS_EARLY "v_add_u32 %[raddr], 16, %[raddr]\n\t" PN2_BT_A_NA
#define PN2_BT_A_PAD_DPP    "s_nop 1\n\t"
#define PN2_BT_A_PAD        "s_nop 0\n\t"
#endif
            const float cx = cand.x, cy = cand.y, cz = cand.z;
#if PN2_BT_NOCTR
            if (amax < kBtCand) pick_counted();
            else
#endif
            for (;;) {
                int reason, t_wl, t_sx, t_sy, t_sz, t_cnt;
                int t_ms = bh;                                                   // (PN2_BT_CADD: read by the block, see above)
                int v_t;
                float v_dx, v_dy, v_dz;
                asm volatile(
                    PN2_BT_A_HEAD
                    "s_mov_b64 exec, %[eq]\n\t"
                    "ds_write_b128 %[raddr], %[cand]\n\t"
                    PN2_BT_A_PUBCOUNT
                    "v_mov_b32 %[cval], 0xbf800000\n\t"           // four instructions ahead of the ladder's first step
                    PN2_BT_A_WINNER_IN
                    "s_mov_b64 exec, -1\n\t"
                    PN2_BT_A_LANE
                    PN2_BT_A_COUNT
                    PN2_BT_A_ADDS_EARLY
                    PN2_BT_A_FULL
                    PN2_BT_A_SXY
                    "v_max_i32_dpp %[t], %[cval], %[cval] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                    PN2_BT_A_SZ
                    "v_subrev_f32 %[dx], %[sx], %[cx]\n\t"
                    "v_subrev_f32 %[dy], %[sy], %[cy]\n\t"
                    "v_max_i32_dpp %[t], %[t], %[t] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                    "v_subrev_f32 %[dz], %[sz], %[cz]\n\t"
                    "v_mul_f32 %[dx], %[dx], %[dx]\n\t"
                    "v_max_i32_dpp %[t], %[t], %[t] row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                    "v_mul_f32 %[dy], %[dy], %[dy]\n\t"
                    "v_mul_f32 %[dz], %[dz], %[dz]\n\t"
                    "v_max_i32_dpp %[t], %[t], %[t] row_mirror row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                    "v_add_f32 %[dx], %[dx], %[dy]\n\t"
                    "v_add_f32 %[dx], %[dx], %[dz]\n\t"
                    "v_max_i32_dpp %[t], %[t], %[t] row_bcast:15 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                    PN2_BT_A_PAD_DPP
                    "v_max_i32_dpp %[t], %[t], %[t] row_bcast:31 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                    "v_min_f32 %[cval], %[dx], %[cval]\n\t"       // the wait state between the ladder's last step and the v_readlane
                    PN2_BT_A_PAD
                    "v_readlane_b32 %[ms], %[t], 63\n\t"
                    PN2_BT_A_PAD
                    "s_cmp_lt_i32 %[ms], %[bound]\n\t"
                    "s_cbranch_scc1 3f\n\t"
                    "v_cmp_eq_u32_e64 %[eq], %[ms], %[cval]\n\t"
                    "s_bcnt1_i32_b64 %[cnt], %[eq]\n\t"
                    "s_cmp_eq_u32 %[cnt], 1\n\t"
                    "s_cbranch_scc1 0b\n\t"
                    "s_mov_b32 %[reason], 2\n\t"
                    "s_branch 4f\n\t"
#if !PN2_BT_NOCTR
                    "2:\n\t"
                    "s_mov_b32 %[reason], 0\n\t"
                    "s_branch 4f\n\t"
#endif
                    "3:\n\t"
                    "s_mov_b32 %[reason], 1\n\t"
                    "4:"
                    : [cval] "+v"(cval), [raddr] "+v"(raddr), [na] "+v"(na), [eq] "+s"(eq), [bh] "+s"(bh),
#if !PN2_BT_NOCTR
                      [a] "+s"(a),
#endif
                      [reason] "=&s"(reason), [wl] "=&s"(t_wl), [sx] "=&s"(t_sx), [sy] "=&s"(t_sy), [sz] "=&s"(t_sz), [ms] PN2_BT_A_MS(t_ms), [cnt] "=&s"(t_cnt),
                      [t] "=&v"(v_t), [dx] "=&v"(v_dx), [dy] "=&v"(v_dy), [dz] "=&v"(v_dz)
                    : [cand] "v"(cand), [caddr] "v"(count_addr), [cx] "v"(cx), [cy] "v"(cy), [cz] "v"(cz), [amax] "s"(amax), [bound] "s"(boundb), [one] "v"(1u)
                    : "memory", "scc");
                vlastb = bh;                                                     // the value of the sample published last
                if (reason != 2) break;
                PN2_BT_STAT(12, 1);
                argmax();
                if (bh < boundb) break;
            }
#if PN2_BT_NOCTR
#if PN2_BT_CADD
            a = (int)((unsigned)__builtin_amdgcn_readfirstlane((int)raddr) - ring_base) >> 4;   // one ring row per sample (pick_counted moves it too)
#else
            a = __builtin_amdgcn_readfirstlane((int)na) - 1;                     // na is the count the next sample would publish
#endif
#endif
#undef PN2_BT_A_WINNER_IN
#undef PN2_BT_A_LANE
#undef PN2_BT_A_SXY
#undef PN2_BT_A_SZ
#undef PN2_BT_A_COUNT
#undef PN2_BT_A_FULL
#undef PN2_BT_A_PUBCOUNT
#undef PN2_BT_A_NA
#undef PN2_BT_A_HEAD
#undef PN2_BT_A_BH
#undef PN2_BT_A_MS
#undef PN2_BT_A_ADDS_EARLY
#undef PN2_BT_A_PAD_DPP
#undef PN2_BT_A_PAD
#else
            pick_counted();
#endif
            if (vlastb == 0) { fill = true; fill_k = __builtin_amdgcn_readlane(__float_as_int(cand.w), (int)__builtin_ctzll(eq)); }   // every running distance is 0 from here on
            const long long q3 = PN2_BT_CLOCK();
            // the list about half full
            if (total > PN2_BT_LIST_HI) g = fmaxf(g * 0.8f, 1.0f / 128.0f);
            else if (total < PN2_BT_LIST_LO) g = fminf(g * 1.25f, 0.5f);
            X.theta = __float_as_uint(__fmul_rn(__int_as_float(vlastb), 1.0f - g));
            X.vlast = (unsigned)vlastb;
            a_prev = a;
            int single = min(single_next, m - (j + a));
            if (single_next) { PN2_BT_STAT(13, single); PN2_BT_STAT(14, 1); }
            single_next = 0;
            single = __builtin_amdgcn_readfirstlane(single);
            X.single = (unsigned)single;
            if (lane == 0)
                __hip_atomic_store(&X.count, (unsigned)a | kBtEnd | (fill ? kBtFill : 0u), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            PN2_BT_STAT(0, 1); PN2_BT_STAT(1, a); PN2_BT_STAT(4, total); PN2_BT_STAT(6, q2 - q1); PN2_BT_STAT(7, q3 - q2); PN2_BT_STAT(8, q1 - q0);
            j = __builtin_amdgcn_readfirstlane(j + a);
            if (fill || j >= m) break;
            for (int i = 0; i < single; ++i) __syncthreads();     // the updaters' one-per-exchange rounds: one barrier each
            j += single;
            if (j >= m) break;
            par ^= 1;
        }
    } else {
        // ================================================ the updaters =========================================================
        PrSlots<P> S;
        fps_pruned_prologue<P, GS, UT>(n, Q, src, smem, S);
        pn2_f2 (&xx)[P / 2] = S.xx;
        pn2_f2 (&yy)[P / 2] = S.yy;
        pn2_f2 (&zz)[P / 2] = S.zz;
        float (&md)[P] = S.md;
        unsigned (&low)[P] = S.low;
        // (the picker has zeroed the exchange area before the prologue's barriers and clears a parity's bound, total and count behind
        // the barrier of the batch in between)
        // lane l tests samples against the box of THIS wave's group l / CH (PN2_BT_GBITS; l % GW without)
        float blx, bly, blz, bhx, bhy, bhz;
        {
            const float *gbox = reinterpret_cast<const float *>(smem + 256 + (size_t)16 * NS + (size_t)kPrHistRows * kPrBins * 4);
            const float *o = gbox + (w * GW + (GB ? lane / CH : (lane & (GW - 1)))) * 8;
            blx = o[0]; bly = o[1]; blz = o[2]; bhx = o[4]; bhy = o[5]; bhz = o[6];
        }
        pn2_f2 sxy = {0.f, 0.f}, syy = {0.f, 0.f}, szk = {0.f, 0.f};   // the sample in the LOW halves (fps_body.h: the high-half broadcast form is not safe)
        // PN2_BT_SSRC: APPLY's samples come out of v_readlane, that is in scalar registers. v_pk_add_f32 takes an SGPR pair as a
        // source and op_sel_hi:[1,0] makes both halves read the pair's LOW word, like the low-half broadcast of a register pair:
        // the three v_mov into the low halves go away (21 instructions per sparse update for 24). The pairs' high words are set
        // once per kernel and never read. scripts/pk_hazard_lab.hip: the form returns the bits of the register-pair form and of
        // __fsub_rn in both halves, normal and denormal operands, alone, beside a VALU kernel and beside an MFMA kernel, with 0, 1,
        // 2 and 5 wait states behind the v_readlane that writes the pair (the compiler puts none there).
        typedef unsigned bt_u2 __attribute__((ext_vector_type(2)));
        bt_u2 ssx = {0u, 0u}, ssy = {0u, 0u}, ssz = {0u, 0u};
        auto pk_sub_bcast_s = [](pn2_f2 a, bt_u2 sp) __attribute__((always_inline)) {
            pn2_f2 r;
            asm volatile("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "s"(sp));
            return r;
        };
        auto update_group = [&](auto gic, auto scalar_sample) __attribute__((always_inline)) {
            constexpr int gi = decltype(gic)::value;
            constexpr bool SS = decltype(scalar_sample)::value;                  // the sample is in ssx / ssy / ssz (else sxy / syy / szk)
            constexpr int H = GS / 2;
            pn2_f2 dx[H], dy[H], dz[H];
#pragma unroll
            for (int h = 0; h < H; ++h) dx[h] = SS ? pk_sub_bcast_s(xx[gi * H + h], ssx) : pk_sub_bcast_lo(xx[gi * H + h], sxy);
#pragma unroll
            for (int h = 0; h < H; ++h) dy[h] = SS ? pk_sub_bcast_s(yy[gi * H + h], ssy) : pk_sub_bcast_lo(yy[gi * H + h], syy);
#pragma unroll
            for (int h = 0; h < H; ++h) dz[h] = SS ? pk_sub_bcast_s(zz[gi * H + h], ssz) : pk_sub_bcast_lo(zz[gi * H + h], szk);
#pragma unroll
            for (int h = 0; h < H; ++h) dx[h] = pk_mul(dx[h], dx[h]);
#pragma unroll
            for (int h = 0; h < H; ++h) dy[h] = pk_mul(dy[h], dy[h]);
#pragma unroll
            for (int h = 0; h < H; ++h) dz[h] = pk_mul(dz[h], dz[h]);
#pragma unroll
            for (int h = 0; h < H; ++h) dx[h] = pk_add(dx[h], dy[h]);
#pragma unroll
            for (int h = 0; h < H; ++h) dx[h] = pk_add(dx[h], dz[h]);
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const int p0 = gi * GS + 2 * h;
                md[p0] = vmin_f32(dx[h].x, md[p0]);              // min(d,td), tf_sampling_g.cu:144
                md[p0 + 1] = vmin_f32(dx[h].y, md[p0 + 1]);
            }
        };
        auto update_all = [&](auto ss) __attribute__((always_inline)) {
            update_group(std::integral_constant<int, 0>(), ss);
            if constexpr (GW >= 2) update_group(std::integral_constant<int, 1>(), ss);
            if constexpr (GW >= 4) { update_group(std::integral_constant<int, 2>(), ss); update_group(std::integral_constant<int, 3>(), ss); }
            if constexpr (GW == 8) {
                update_group(std::integral_constant<int, 4>(), ss); update_group(std::integral_constant<int, 5>(), ss);
                update_group(std::integral_constant<int, 6>(), ss); update_group(std::integral_constant<int, 7>(), ss);
            }
        };
        // sample 0 is point 0 (tf_sampling_g.cu:114-116): every slot against it
        {
            const float4 s = lds_rank[NS - 1];
            sxy.x = s.x; syy.x = s.y; szk.x = s.z;
            update_all(std::false_type());
        }
        if (t == 0) {
            dst[0] = 0;
            if (PUBLISH) __hip_atomic_store(gtag, (unsigned long long)tag << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        unsigned vlastb = __float_as_uint(1e38f);    // value bits of the last sample: no running distance is above it
        unsigned thetab = __float_as_uint(1e38f);    // first batch: nobody reaches it, every wave sends its exact best lane
        // ---- EARLY: the first samples, one per exchange (the full tier's round, fps_body.h) --------------------------------------
        // While the farthest-point distance still halves every few samples a list determines three or four samples and every
        // sample reaches most groups: a batch then costs more than the classic round (measured: the first 64 samples 44 us in
        // batches, 25 us like this; the whole chain at 4096 -> 1024 280 -> 255 us). The picker and its barriers: one per round, see its branch.
        // The update works on single registers, not pairs, as the full tier does at 512 threads (fps_body.h: two waves per SIMD, 411
        // against 438 ns per round there; 395 against 440 here). The index is stored at once: behind the next round's key reads
        // (the full tier's place for it) the overlapped launch lost 6 us. Also what the workgroup falls back to when batches do not
        // pay (SLOW BATCHES above).
        auto single_rounds = [&](const int jend) __attribute__((always_inline)) {
            double *partial = reinterpret_cast<double *>(smem);                  // [2][W]: the pruned layout's wave keys
            for (; j < jend; ++j) {
                double kd[P];
#pragma unroll
                for (int p = 0; p < P; ++p) kd[p] = __hiloint2double(__float_as_int(md[p]), (int)low[p]);
#pragma unroll
                for (int st = 1; st < P; st <<= 1)
#pragma unroll
                    for (int i = 0; i + st < P; i += 2 * st)
                        asm("v_max_f64 %0, %1, %2" : "=v"(kd[i]) : "v"(kd[i]), "v"(kd[i + st]));
                const double wd = wave_max_f64_lane63(kd[0]);
                double *slot = partial + (j & 1) * W;
                if (lane == 63) {
                    slot[w] = wd;
                    if (w == 0 && j == jE - 1) xch[0].spare1 = vlastb;           // NO LISTS (below): the previous sample's value, written once
                }
                __syncthreads();
                double key[W];
#pragma unroll
                for (int i = 0; i < W; ++i) key[i] = slot[i];
#pragma unroll
                for (int st = 1; st < W; st <<= 1)
#pragma unroll
                    for (int i = 0; i + st < W; i += 2 * st)
                        asm("v_max_f64 %0, %1, %2" : "=v"(key[i]) : "v"(key[i]), "v"(key[i + st]));
                vlastb = (unsigned)__double2hiint(key[0]);
                const float4 s = lds_rank[(unsigned)__double2loint(key[0])];    // same address in every lane: LDS broadcast
                if (t == 0) {
                    const int k = __float_as_int(s.w);
                    dst[j] = k;
                    if (PUBLISH)
                        __hip_atomic_store(gtag + j, ((unsigned long long)tag << 32) | (unsigned long long)(unsigned)k, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                }
                if constexpr (P >= PN2_BT_PACKED_FROM) {                         // (16 slots on single registers: spills at 576 threads)
                    sxy.x = s.x; syy.x = s.y; szk.x = s.z;
                    update_all(std::false_type());
                } else {
#pragma unroll
                    for (int p = 0; p < P; ++p) {
                        const float d = p & 1 ? sqdist(xx[p / 2].y, yy[p / 2].y, zz[p / 2].y, s.x, s.y, s.z)
                                              : sqdist(xx[p / 2].x, yy[p / 2].x, zz[p / 2].x, s.x, s.y, s.z);   // tf_sampling_g.cu:141-143
                        md[p] = vmin_f32(d, md[p]);                              // :144
                    }
                }
            }
            thetab = __float_as_uint(__fmul_rn(__uint_as_float(vlastb), 1.0f - PN2_BT_G0));
        };
        // NO LISTS while a point stands at the start value 1e38. A list is exact because a picked candidate leaves it: its distance
        // to itself is 0. A point with a NaN or infinite coordinate is at distance NaN (or inf) from everything, itself included;
        // min() leaves it at 1e38 for ever, and once the reference has picked it, it picks it in every later round (values only
        // fall, and it had the best tie rank at 1e38 already) -- whatever else still stands at 1e38, which is what a list would
        // go on to. While such a point exists every sample's value is 1e38, so: if the last sample but one of the early rounds
        // (the word wave 0 left in front of the last round's barrier: the picker reads the same word behind it) still had that
        // value, the rest of the row is taken one per exchange as well. Exact whatever the cause; a cloud of finite points that
        // is still at 1e38 after 46 samples (46 clusters ~1e19 apart) merely runs at the full tier's pace.
        for (int jend = jE; j < jend;) {
            single_rounds(jend);
            if (bt_stands_at_start(xch, jE)) jend = m;
        }
        int par = 0;
        long long uend = 0;                          // lab: the clock when the previous batch's end flag was seen
        if (j < m)
        for (;;) {
            BtXchg &X = xch[par];
            const long long u0 = PN2_BT_CLOCK();
            // ---- COLLECT ----------------------------------------------------------------------------------------------------------
            double kl;
            float sec;
            {
                // best key and the two largest values of the lane's P slots (straight-line: 2 P - 1 tournament nodes)
                double kd[P];
#pragma unroll
                for (int p = 0; p < P; ++p) kd[p] = __hiloint2double(__float_as_int(md[p]), (int)low[p]);
#if PN2_BT_SEC3
#pragma unroll
                for (int st = 1; st < P; st <<= 1)
#pragma unroll
                    for (int i = 0; i + st < P; i += 2 * st)
                        asm("v_max_f64 %0, %1, %2" : "=v"(kd[i]) : "v"(kd[i]), "v"(kd[i + st]));
                kl = kd[0];
                sec = bt_second_best<P>(md);
#else
                float hv[P / 2], lv[P / 2];
#pragma unroll
                for (int i = 0; i < P / 2; ++i) { hv[i] = vmax_f32(md[2 * i], md[2 * i + 1]); lv[i] = vmin_f32(md[2 * i], md[2 * i + 1]); }
#pragma unroll
                for (int st = 1; st < P; st <<= 1)
#pragma unroll
                    for (int i = 0; i + st < P; i += 2 * st)
                        asm("v_max_f64 %0, %1, %2" : "=v"(kd[i]) : "v"(kd[i]), "v"(kd[i + st]));
#pragma unroll
                for (int st = 1; st < P / 2; st <<= 1)
#pragma unroll
                    for (int i = 0; i + st < P / 2; i += 2 * st) {
                        const float ll = vmax_f32(lv[i], lv[i + st]);
                        lv[i] = vmed3_f32(hv[i], hv[i + st], ll);     // second largest of (h1 >= l1, h2 >= l2)
                        hv[i] = vmax_f32(hv[i], hv[i + st]);
                    }
                kl = kd[0];
                sec = lv[0];
#endif
            }
            const unsigned vb = (unsigned)__double2hiint(kl);
            unsigned long long mask = __ballot(vb >= thetab);
            int cnt = __popcll(mask);
            unsigned thb = thetab;                   // this wave's threshold: its points outside the list are below it
#if PN2_BT_CTAIL && PN2_BT_READ1
            // The list write, the same code at the end of both ways below so that the common one carries no copies for the other:
            // exec = the candidate lanes (the ballot mask as it is: every lane of an updater wave is active here), their keys to the
            // wave's places and their second-best values + 1 ulp into the bound; then lane 0 alone, the wave's count into the total
            // and its threshold into the bound. Scalar writes of exec need no wait state in front of the LDS operations (the
            // picker's publish does the same).
            static_assert(offsetof(BtXchg, total) == offsetof(BtXchg, bmax) + 4, "one address register for both words");
            auto list_write = [&](const unsigned long long mk, const int c, const unsigned th) __attribute__((always_inline)) {
                const unsigned pos = __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
                asm volatile("s_mov_b64 exec, %[mk]\n\t"
                             "ds_write_b64 %[la], %[kl]\n\t"
                             "ds_max_u32 %[ba], %[sec1]\n\t"
                             "s_mov_b64 exec, 1\n\t"
                             "ds_add_u32 %[ba], %[c] offset:4\n\t"
                             "ds_max_u32 %[ba], %[th]\n\t"
                             "s_mov_b64 exec, -1"
                             :: [mk] "s"(mk), [la] "v"((unsigned)(size_t)&X.list[w * CAP] + 8u * pos), [kl] "v"(kl),
                                [ba] "v"((unsigned)(size_t)&X.bmax), [sec1] "v"(__float_as_uint(sec) + 1u), [c] "v"((unsigned)c), [th] "v"(th)
                             : "memory");
            };
            if ((unsigned)(cnt - 1) < (unsigned)CAP) {
                list_write(mask, cnt, thb);          // 0 < cnt <= CAP: theta stands, no fallback
            } else {
#endif
            bool exact = false;
            if (cnt > CAP) {
                unsigned lob = thetab, hib = vlastb + 1u;       // more than CAP lanes at lob, none at hib
                for (int it = 0; it < 16; ++it) {
                    const unsigned mid = lob + ((hib - lob) >> 1);
                    if (mid == lob) break;
                    const unsigned long long mk = __ballot(vb >= mid);
                    const int c = __popcll(mk);
                    PN2_BT_STAT(3, 1);
                    if (c > CAP) lob = mid;
                    else if (c == 0) hib = mid;
                    else { mask = mk; cnt = c; thb = mid; break; }
                }
                exact = cnt > CAP;
            } else if (cnt == 0) {
                exact = true;
            }
            if (exact) {                              // the wave's best lane alone
                PN2_BT_STAT(2, 1);
                const double wk = wave_max_f64_lane63(kl);
                const int bh = __builtin_amdgcn_readlane(__double2hiint(wk), 63), bl = __builtin_amdgcn_readlane(__double2loint(wk), 63);
                unsigned long long mk = __ballot(__double2hiint(kl) == bh && __double2loint(kl) == bl);
                mk &= 0ull - mk;                      // equal keys exist only among padding slots
                if (cnt != 0) thb = (unsigned)bh + 1u;   // too many equal values: everything else of the wave is <= this lane's value, with a lower key
                mask = mk;
                cnt = 1;
            }
#if PN2_BT_CTAIL && PN2_BT_READ1
                // (the compiler carries this way's mask through the bisection's loop in vector registers: back to a scalar pair)
                list_write(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(mask >> 32)) << 32) |
                               (unsigned)__builtin_amdgcn_readfirstlane((int)mask), cnt, thb);
            }
#else
            if ((mask >> lane) & 1ull) {
                const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                X.list[w * CAP + pos] = kl;
#if PN2_BT_READ1
                lds_max_u32(&X.bmax, __float_as_uint(sec) + 1u);
#else
                lds_max_u32(&X.bound[w], __float_as_uint(sec) + 1u);
#endif
            }
            if (lane == 0) {
#if PN2_BT_READ1
                lds_add_u32(&X.total, (unsigned)cnt);     // every wave into the batch's two words: the picker reads them as they are
                lds_max_u32(&X.bmax, thb);
#else
                X.cnt[w] = (unsigned)cnt;
                lds_max_u32(&X.bound[w], thb);
#endif
            }
#endif
            const long long u1 = PN2_BT_CLOCK();
            if (w == 0 && uend) PN2_BT_STAT(15, u1 - uend);
#if defined(PN2_BT_STATS) && PN2_BT_READ1
            if (lane == 0) X.cnt[w] = (unsigned)u1;              // lab: this wave's arrival (the per-wave count words are free with PN2_BT_READ1)
#endif
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the asm LDS operations above are invisible to the compiler's counters
            __syncthreads();
            const long long u2 = PN2_BT_CLOCK();
#if defined(PN2_BT_STATS) && PN2_BT_READ1
            // lab: how far behind the first arriver this wave reached the list barrier, and whether it was the last. Nobody writes
            // this parity's words again before the barrier after next.
            {
                int first = 0, last = 0;
                for (int i = 0; i < W; ++i) {
                    const int d = (int)(X.cnt[i] - (unsigned)u1);
                    first = min(first, d); last = max(last, d);
                }
                PN2_BT_STAT(24 + w, -first);
                PN2_BT_STAT(32 + w, last == 0);
            }
#endif
#if !PN2_BT_READ1
            if (lane == 0) xch[par ^ 1].bound[w] = 0u;            // next batch's word of this wave (nobody reads it before the next barrier)
#endif
            // ---- APPLY: the picker's samples as they appear ----------------------------------------------------------------------------
            int done = 0;
            unsigned c;
            // v* of the skip test: the previous batch's last sample value bounds every running distance (fps_pruned_body: the exact skip)
            const float thr = __fadd_rn(__fmul_rn(__uint_as_float(vlastb), 1.00001f), 1e-30f);
            const int pi = GB ? (lane & (CH - 1)) : lane / GW;                   // this lane's sample of a chunk
            typedef std::integral_constant<bool, PN2_BT_SSRC != 0> bt_ss;
            auto sample_in = [&](const float4 &s4, const int sl) __attribute__((always_inline)) {   // sample <- lane sl of the chunk's ring read
#if PN2_BT_SSRC
                ssx.x = (unsigned)__builtin_amdgcn_readlane(__float_as_int(s4.x), sl);
                ssy.x = (unsigned)__builtin_amdgcn_readlane(__float_as_int(s4.y), sl);
                ssz.x = (unsigned)__builtin_amdgcn_readlane(__float_as_int(s4.z), sl);
#else
                sxy.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s4.x), sl));
                syy.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s4.y), sl));
                szk.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s4.z), sl));
#endif
            };
#if PN2_BT_RING1
            // ONE LDS ROUND TRIP PER CHUNK (PN2_BT_RING1). The count word and this lane's ring row are read back to back and waited
            // for once: the row's address hangs on `done` and the lane, not on the count. LDS serves a wave's operations in order,
            // so the row's read is served behind the count's; the picker's winner lane stores a row and then adds to the count, in
            // order too. So every row below the count just read is complete. Rows at or beyond it may be stale or half written:
            // their lanes leave by the np mask below as before (without the cut they re-read row `done`). The row index is clamped
            // to the ring's 64 rows (done + the lane's sample reaches 78 at 16 samples per chunk, 126 at 64). The compiler puts a
            // wait behind an acquire load, so the two reads and their single wait are one asm statement (list_write above does
            // the same); the wait is the acquire. A poll that finds nothing wastes the row's read and nothing else.
            typedef float bt_f3 __attribute__((ext_vector_type(3)));
            unsigned poll_addr = (unsigned)(size_t)&X.count;
            unsigned row0_addr = (unsigned)(size_t)ring + 16u * (unsigned)pi, row_last_addr = (unsigned)(size_t)ring + 16u * (kBtCand - 1);
            asm("" : "+v"(poll_addr), "+v"(row0_addr), "+v"(row_last_addr));   // three registers of the batch: not worked out again in every poll
#endif
            for (;;) {
#ifdef PN2_BT_STATS
                const long long w0 = PN2_BT_CLOCK();
#endif
#if PN2_BT_RING1
                bt_f3 srow;
                asm volatile("ds_read_b32 %[c], %[ca]\n\t"
                             "ds_read_b96 %[s], %[ra]\n\t"
                             "s_waitcnt lgkmcnt(0)"
                             : [c] "=&v"(c), [s] "=&v"(srow)
                             : [ca] "v"(poll_addr), [ra] "v"(min(row0_addr + 16u * (unsigned)done, row_last_addr))
                             : "memory");
#else
                c = __hip_atomic_load(&X.count, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
#ifdef PN2_BT_STATS
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // lab: the count's wait inside [19]
#endif
#endif
#ifdef PN2_BT_STATS
                const long long w1 = PN2_BT_CLOCK();
#endif
                c = (unsigned)__builtin_amdgcn_readfirstlane((int)c);
                const int avail = (int)(c & kBtCountMask);
                if (avail == done) {
                    if (c & kBtEnd) break;
                    if (w == 0) PN2_BT_STAT(17, 1);
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                if (w == 0) PN2_BT_STAT(16, 1);
                constexpr unsigned long long kStride = GW == 8 ? 0x0101010101010101ull : GW == 4 ? 0x1111111111111111ull
                                                       : GW == 2 ? 0x5555555555555555ull : ~0ull;   // one bit per sample
                const int np = min(avail - done, CH);
#if PN2_BT_RING1
                const float4 s = make_float4(srow.x, srow.y, srow.z, 0.f);      // (w, the point's index, is not used here)
#else
                const float4 s = ring[done + (pi < np ? pi : 0)];
#endif
#ifdef PN2_BT_STATS
                // lab: updater 0's cycles inside the chunk's two waits -- [19] around the count's (the poll's) wait, [20] around the
                // ring row's (PN2_BT_RING1: nothing is left to wait for), [21] two clock reads with nothing in between, the cost
                // each of the two figures carries
                if (PN2_BT_STATS_CHUNK && w == 0) {
#if !PN2_BT_RING1
                    asm volatile("s_waitcnt lgkmcnt(0)" :: "v"(s.x), "v"(s.y), "v"(s.z) : "memory");
#endif
                    const long long w2 = PN2_BT_CLOCK();
                    const long long w3 = PN2_BT_CLOCK();
                    PN2_BT_STAT(19, w1 - w0); PN2_BT_STAT(20, w2 - w1); PN2_BT_STAT(21, w3 - w2);
                }
#endif
                const float ax = __fsub_rn(s.x, __builtin_amdgcn_fmed3f(s.x, blx, bhx));
                const float ay = __fsub_rn(s.y, __builtin_amdgcn_fmed3f(s.y, bly, bhy));
                const float az = __fsub_rn(s.z, __builtin_amdgcn_fmed3f(s.z, blz, bhz));
                const float bd = __fadd_rn(__fadd_rn(__fmul_rn(ax, ax), __fmul_rn(ay, ay)), __fmul_rn(az, az));
                unsigned long long touched = ~__ballot(bd >= thr);               // NaN -> not far -> updated
                if constexpr (GB) {
                    // the lanes of samples np .. CH - 1 leave: the same np bits of every group's field (CH <= 32: both words alike)
                    constexpr unsigned kRep = CH == 32 ? 1u : CH == 16 ? 0x00010001u : 0x01010101u;
                    if (np < CH) { const unsigned vm = ((1u << np) - 1u) * kRep; touched &= ((unsigned long long)vm << 32) | vm; }
                } else {
                    if (np * GW < 64) touched &= (1ull << (np * GW)) - 1ull;
                }
                // group by group (static): the samples that reach group g, straight into that group's update -- no dispatch on a
                // group number (three compare-and-branch pairs per (group, sample) otherwise)
                if (touched) {
                    // the first samples of a cloud reach most groups: then every sample of the chunk updates all of the wave's
                    // groups in straight-line code (an update of an untouched group changes nothing)
                    if (2 * __popcll(touched) >= GW * np) {
                        if (w == 0) PN2_BT_STAT(18, GW * np);
                        for (int p = 0; p < np; ++p) {
                            const int sl = GB ? p : p * GW;                      // a lane that holds sample p
                            sample_in(s, sl);
                            update_all(bt_ss());
                        }
                    } else {
                        auto one_group = [&](auto gic) __attribute__((always_inline)) {
                            constexpr int g8 = decltype(gic)::value;
                            if constexpr (GB) {
                                // the group's field of the mask, one scalar word: bit p = sample p = lane p of the chunk's ring read.
                                // An untouched group costs the field extract and a branch; a sample costs s_ff1, one s_bitset0
                                // and the loop's compare.
                                unsigned mg = (unsigned)(touched >> (g8 * CH));
                                if constexpr (CH < 32) mg &= (1u << CH) - 1u;
                                while (mg) {
                                    const int sl = (int)__builtin_ctz(mg);
                                    asm("s_bitset0_b32 %0, %1" : "+s"(mg) : "s"(sl));
                                    sample_in(s, sl);
                                    PN2_BT_STAT(5, 1);
                                    update_group(gic, bt_ss());
                                }
                            } else {
                                unsigned long long mg = touched & (kStride << g8);
                                while (mg) {
                                    const int sl = (int)__builtin_ctzll(mg) & ~(GW - 1);
                                    mg &= mg - 1ull;
                                    sample_in(s, sl);
                                    PN2_BT_STAT(5, 1);
                                    update_group(gic, bt_ss());
                                }
                            }
                        };
                        one_group(std::integral_constant<int, 0>());
                        if constexpr (GW >= 2) one_group(std::integral_constant<int, 1>());
                        if constexpr (GW >= 4) { one_group(std::integral_constant<int, 2>()); one_group(std::integral_constant<int, 3>()); }
                        if constexpr (GW == 8) {
                            one_group(std::integral_constant<int, 4>()); one_group(std::integral_constant<int, 5>());
                            one_group(std::integral_constant<int, 6>()); one_group(std::integral_constant<int, 7>());
                        }
                    }
                }
                done += np;
            }
            const long long u3 = PN2_BT_CLOCK();
            uend = u3;
            if (w == 0) { PN2_BT_STAT(9, u1 - u0); PN2_BT_STAT(10, u3 - u2); }
            const int a = (int)(c & kBtCountMask);
            // ---- the batch's samples leave in one store ------------------------------------------------------------------------------
            if (w == 0 && lane < a) {
                const int k = __float_as_int(ring[lane].w);
                dst[j + lane] = k;
                if (PUBLISH)
                    __hip_atomic_store(gtag + (j + lane), ((unsigned long long)tag << 32) | (unsigned long long)(unsigned)k, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
            if (c & kBtFill) fill_k = __float_as_int(ring[a - 1].w);
            j += a;
            if ((c & kBtFill) || j >= m) break;
            thetab = X.theta;
            vlastb = X.vlast;
            const int single = __builtin_amdgcn_readfirstlane((int)X.single);    // SLOW BATCHES (the picker's decision, published ahead of the end flag)
            if (single) {
                single_rounds(min(j + single, m));                               // (the picker has clipped it already: a run never passes the output row)
                if (j >= m) break;
            }
            par ^= 1;
        }
    }
    if (fill_k >= 0) {
        for (int i = j + t; i < m; i += BT) {
            dst[i] = fill_k;
            if (PUBLISH)
                __hip_atomic_store(gtag + i, ((unsigned long long)tag << 32) | (unsigned long long)(unsigned)fill_k, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    fps_gather_epilogue<BT>(m, src, dst, dxyz);
}

}  // namespace pn2
