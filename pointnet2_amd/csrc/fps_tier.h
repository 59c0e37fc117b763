// fps_tier.h -- which farthest-point-sampling kernel a launch runs: the tiers as compile-time tags, the ONE size rule that picks
// a tier and its geometry (fps_choose), and the ONE step from that runtime choice to a tag (fps_with_tier). Shared by fps.hip
// (dense, ragged and packed launches) and sa_fused.hip (the producers of the overlapped launch).
#pragma once
#include "fps_body.h"
#include "fps_pruned_body.h"
#include "fps_batch_body.h"

namespace pn2 {

enum { kFpsReg = 0, kFpsPruned = 1, kFpsBatch = 2 };   // the values of sa_fused_kernel's TIER

// What fps_choose decides. T threads (the batched tier: kBtT, its updaters and the picker), P rank slots per (updater) thread,
// GS slots per kd group (0 on the register tier), Q = ceil(n / 512), the quotient of the tie ranks (fps_body.h).
struct FpsChoice {
    int tier, T, P, GS, Q;
};

constexpr int kMaxLdsSlots = 8192;     // 256 B + 16 B per rank slot <= 160 KiB: up to here the register tier mirrors the cloud in LDS
constexpr int kMaxRegPoints = 16384;

// ---- the tiers as tags ----------------------------------------------------------------------------------------------------------
// threads and lds are the launch's; body runs the tier's chain on ONE cloud handed over as cloud 0 (n points at src, m samples to
// dst and -- unless NULL -- dxyz), which is how the ragged kernel calls every tier; matches: is this the template c names?
template <int T, int P, bool LDSXYZ>
struct RegTier {
    static constexpr int threads = T;
    static constexpr size_t lds = 256 + (LDSXYZ ? sizeof(float4) : sizeof(int)) * (size_t)T * P;
    static bool matches(const FpsChoice &c) { return c.tier == kFpsReg && c.T == T && c.P == P; }
    __device__ __forceinline__ static void body(int n, int m, int Q, const float *__restrict__ src, int *__restrict__ dst,
                                                float *__restrict__ dxyz, char *smem)
    {
        fps_reg_body<T, P, LDSXYZ, false>(n, m, Q, 0, src, dst, dxyz, nullptr, smem);
    }
};
template <int T, int P>
using RegTierAt = RegTier<T, P, ((long long)T * P <= kMaxLdsSlots)>;

// Pruned tier (fps_pruned_body.h): kd-grouped slots, per-round box tests, only the groups the new sample can reach are
// updated. 2049..8192 rank slots, chains long enough to pay for the kd build.
template <int P, int GS>
struct PrunedTier {
    static constexpr int threads = kPrT;
    static constexpr size_t lds = fps_pruned_lds_bytes(P);
    static bool matches(const FpsChoice &c) { return c.tier == kFpsPruned && c.P == P; }
    __device__ __forceinline__ static void body(int n, int m, int Q, const float *__restrict__ src, int *__restrict__ dst,
                                                float *__restrict__ dxyz, char *smem)
    {
        fps_pruned_body<P, GS, false>(n, m, Q, 0, src, dst, dxyz, nullptr, smem);
    }
};

// Batched tier (fps_batch_body.h): the pruned tier's slots and boxes, several samples per arg-max exchange.
// P = slots per updater thread (kBtUT of them), GS slots per group
template <int P, int GS>
struct BatchTier {
    static constexpr int threads = kBtT;
    static constexpr size_t lds = fps_batch_lds_bytes(P);
    static bool matches(const FpsChoice &c) { return c.tier == kFpsBatch && c.P == P; }
    __device__ __forceinline__ static void body(int n, int m, int Q, const float *__restrict__ src, int *__restrict__ dst,
                                                float *__restrict__ dxyz, char *smem)
    {
        fps_batch_body<P, GS, false>(n, m, Q, 0, src, dst, dxyz, nullptr, smem);
    }
};

// The batched tier's template at 1024 / 2048 / 4096 / 8192 rank slots: 8 / 16 groups of 2 slots below 4096 (512 updater threads
// only), 32 groups from there on -- at 512 updater threads 8 slots per thread in groups of 2 or 16 in groups of 4.
constexpr int fps_batch_p(int slots) { return slots / kBtUT; }
constexpr int fps_batch_gs(int slots) { return slots <= 2048 ? 2 : slots / kBtUT / (32 / (kBtUT / 64)); }

// ---- the size rule ----------------------------------------------------------------------------------------------------------------
inline int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

inline bool fps_pruned_covers(int ranks) { return ranks > 2048 && ranks <= 8192; }

// The kernel of a cloud of n <= 16384 points (a ragged batch: the padded n; a packed one: nmax -- the host knows no other) and m
// samples. variant: PN2_FPS_AUTO = the batched tier where it pays, else the pruned tier where it pays, else the register tier;
// _FULL / _PRUNED / _BATCH force one. PN2_E_ARG: a forced tier outside its rank-slot envelope. Results never depend on the choice.
inline int fps_choose(int variant, int n, int m, FpsChoice &c)
{
    c.Q = (n + kRefThreads - 1) / kRefThreads;
    const int ranks = kRefThreads * c.Q;
    if (variant == PN2_FPS_BATCH || (variant == PN2_FPS_AUTO && fps_batch_pays(ranks, m))) {
        if (!fps_batch_covers(ranks) || (ranks <= 2048 && kBtUT != 512)) return PN2_E_ARG;
        const int slots = ranks <= 1024 ? 1024 : ranks <= 2048 ? 2048 : ranks <= 4096 ? 4096 : 8192;
        c = {kFpsBatch, kBtT, fps_batch_p(slots), fps_batch_gs(slots), c.Q};
        return PN2_OK;
    }
    if (variant == PN2_FPS_PRUNED || (variant == PN2_FPS_AUTO && fps_pruned_pays(ranks, m))) {
        if (!fps_pruned_covers(ranks)) return PN2_E_ARG;
        // 32 groups either way: 16 slots per thread in groups of 2, 32 in groups of 4
        c = {kFpsPruned, kPrT, ranks <= 4096 ? 16 : 32, ranks <= 4096 ? 2 : 4, c.Q};
        return PN2_OK;
    }
    // register tier (measured, scripts/fps_prod_lab.hip, ns per round at n = 1024/2048/4096/8192):
    // 256 threads with the packed distance update 273/312/402/585, 512 threads (scalar) 288/326/393/552
    const int T = ranks <= 2048 ? 256 : 512;
    c = {kFpsReg, T, next_pow2((ranks + T - 1) / T), 0, c.Q};
    return PN2_OK;
}

// ---- from the choice to a tag -----------------------------------------------------------------------------------------------------
// f(tag) of the first tag that matches c; PN2_E_ARG if none does
template <class F, class... Tier>
inline int fps_first_match(const FpsChoice &c, F f, Tier... tier)
{
    int rc = PN2_E_ARG;
    (void)((Tier::matches(c) && ((rc = f(tier)), true)) || ...);
    return rc;
}

// Calls f with the tag of c's kernel -- a generic lambda that names the kernel it launches for the tag -- and returns what f
// returns. The lists below are every template fps_choose can name, hence every instantiation of a kernel launched this way.
template <class F>
inline int fps_with_tier(const FpsChoice &c, F f)
{
    if (c.tier == kFpsReg)
        return fps_first_match(c, f, RegTierAt<256, 2>{}, RegTierAt<256, 4>{}, RegTierAt<256, 8>{}, RegTierAt<512, 8>{}, RegTierAt<512, 16>{},
                               RegTierAt<512, 32>{});
    if (c.tier == kFpsPruned) return fps_first_match(c, f, PrunedTier<16, 2>{}, PrunedTier<32, 4>{});
    if constexpr (kBtUT == 512)
        return fps_first_match(c, f, BatchTier<fps_batch_p(1024), fps_batch_gs(1024)>{}, BatchTier<fps_batch_p(2048), fps_batch_gs(2048)>{},
                               BatchTier<fps_batch_p(4096), fps_batch_gs(4096)>{}, BatchTier<fps_batch_p(8192), fps_batch_gs(8192)>{});
    else
        return fps_first_match(c, f, BatchTier<fps_batch_p(4096), fps_batch_gs(4096)>{}, BatchTier<fps_batch_p(8192), fps_batch_gs(8192)>{});
}

}  // namespace pn2
