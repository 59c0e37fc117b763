// train_mlp_pair.hip -- a layer's data-gradient GEMM and its weight-gradient pass as two ranges of workgroups of ONE launch
// (tl_pair_kernel: both bodies, tl_gemm_body.inc and tl_wgrad_body.inc), and the table of shape pairs it is built for. gfx950.
#include "train_mlp_device.h"

#include <stdio.h>
#include <type_traits>

namespace pn2 {

// ---- a layer's data gradient AND its weight gradient in one launch, side by side (small levels) ---------------------------------
// dy_{l-1} = dz_l W_l^T (tl_gemm_body) and dW_l = h_{l-1}^T dz_l (tl_wgrad_body) read the same tensors and write disjoint ones. On
// a level of a few thousand rows each is a launch of 10-50 us that occupies a fraction of the chip for a few dependent
// round trips to memory, and one after the other they were half of such a level's backward time (profiles/r04: sem_seg SA4
// 25 + 29 and 40 + 30 us for its two upper layers). Two streams cost more than they gave (~10 us per cross-queue
// dependency, SideStream in train_mlp.hip). Here the two passes are two RANGES OF WORKGROUPS of one grid -- blocks [0, ga * gsl) run the
// GEMM on a (ga, gsl) grid, the rest the weight gradient on a (gw, slabs) grid -- like the producers and consumers of
// sa_fused_kernel, but with nothing to exchange. Registers and LDS are the larger of the two bodies'. One instantiation per
// shape pair that occurs at the reference networks' levels (launch_pair's table); any other pair takes the two launches.
template <int NS, int AMODE, int TPW, int UPW, int DCLS, bool GATHER = false>
__global__ __launch_bounds__(kTlThreads) void tl_pair_kernel(const TlGemm pg, const TlWgrad pw, const unsigned ga, const unsigned gsl,
                                                             const unsigned gw)
{
    const unsigned na = ga * gsl;
    if (blockIdx.x < na) {
        const unsigned sbx = blockIdx.x % ga, sby = blockIdx.x / ga;
        const TlGemm &p = pg;
#define PN2_BX sbx
#define PN2_BY sby
#define PN2_GX ga
#define PN2_STATS true                  // (the pair keeps the sums as a run-time choice: p.stats may be NULL under frozen statistics)
#define PN2_MASKED false
#include "tl_gemm_body.inc"
#undef PN2_STATS
#undef PN2_MASKED
#undef PN2_BX
#undef PN2_BY
#undef PN2_GX
    } else {
        const unsigned sb = blockIdx.x - na, sbx = sb % gw, sby = sb / gw;
        constexpr bool DY = false, L1X = false;
        const TlWgrad &p = pw;
#define PN2_BX sbx
#define PN2_BY sby
#define PN2_GX gw
#define PN2_MASKED false
#include "tl_wgrad_body.inc"
#undef PN2_MASKED
#undef PN2_BX
#undef PN2_BY
#undef PN2_GX
    }
}

// One launch for a layer's data-gradient GEMM (its workgroups first) and its weight-gradient pass (tl_pair_kernel), then the
// weight gradient's reduction. kNoPair: no kernel for this pair of shapes -- the caller launches the two passes one after the
// other. The table = the pairs the size rules produce at the levels of the four reference networks below 0.5 M rows
// (scripts/train_pairs.py lists them); a level of other widths simply takes the two launches.
int launch_pair(int amode, TlGemm &pg, const GemmShape &g, TlWgrad &pw, const WgradShape &w, const pn2_bn_layer &L, hipStream_t st,
                       const Opts &o, int *nparts, double *plain)
{
    if (pw.dy_w) return kNoPair;
    if (pw.partial_cap && w.partial_bytes > pw.partial_cap) return PN2_E_ARG;   // never write past the planned buffer
    const bool gather = pw.amode == A_GATHER;
    const int dcls = pw.dmode == A_FILL ? D_TOP : pw.dmode == A_DZ_POOL ? D_DZPOOL : D_DZ;
    size_t lds = g.lds > w.lds ? g.lds : w.lds;
    if (pg.fin.ticket && lds < kFinLds) lds = kFinLds;
#define PN2_PAIR(AM, NS_, DC, TP, UP) PN2_PAIR_G(AM, NS_, DC, TP, UP, false)
#define PN2_PAIR_G(AM, NS_, DC, TP, UP, GA)                                                                              \
    if (amode == AM && g.ns == NS_ && dcls == DC && w.tpw == TP && w.upw == UP && gather == GA) {                        \
        auto kern = tl_pair_kernel<NS_, AM, TP, UP, DC, GA>;                                                             \
        const dim3 ga = prep_gemm(pg, g, o);                                                                             \
        if (pg.fin.ticket) { pg.fin.total = ga.x * ga.y; pg.fin.nparts = (int)ga.x; }                                    \
        pw.tus = w.tus; pw.tts = w.tts; pw.tslabs = w.tslabs;                                                            \
        if (int rc = allow_dynamic_lds(kern, lds)) return rc;                                                            \
        const unsigned total = ga.x * ga.y + (unsigned)w.gridx * (unsigned)(w.uslabs * w.tslabs);                        \
        if (int rc = launch(kern, dim3(total), dim3(kTlThreads), lds, st, pg, pw, ga.x, ga.y, (unsigned)w.gridx)) return rc; \
        if (nparts) *nparts = (int)ga.x;                                                                                 \
        return launch_wgrad_reduce(pw, w, L, st, plain);                                                                 \
    }
    PN2_PAIR(A_DZ, 1, D_DZ, 1, 1)
    PN2_PAIR(A_DZ, 1, D_DZ, 1, 2)
    PN2_PAIR(A_DZ, 1, D_DZ, 2, 2)
    PN2_PAIR(A_DZ, 1, D_DZ, 4, 3)
    PN2_PAIR(A_DZ, 2, D_DZ, 1, 1)
    PN2_PAIR(A_DZ, 2, D_DZ, 2, 2)
    PN2_PAIR(A_DZ, 2, D_DZ, 4, 3)
    PN2_PAIR(A_DZ, 4, D_DZ, 2, 2)
    PN2_PAIR(A_DZ_POOL, 1, D_DZPOOL, 4, 3)
    PN2_PAIR(A_DZ_POOL, 2, D_DZPOOL, 4, 3)
    PN2_PAIR(A_FILL, 1, D_TOP, 1, 2)
    PN2_PAIR(A_FILL, 2, D_TOP, 2, 3)
    PN2_PAIR(A_FILL, 4, D_TOP, 4, 3)
    PN2_PAIR(A_PLAIN, 1, D_DZ, 1, 1)                               // layer 1 per point: dPoints = S W1f^T beside dW1f = points^T S
    PN2_PAIR(A_PLAIN, 1, D_DZ, 2, 2)
    PN2_PAIR(A_PLAIN, 2, D_DZ, 2, 2)
    PN2_PAIR(A_PLAIN, 4, D_DZ, 1, 2)
    PN2_PAIR(A_PLAIN, 4, D_DZ, 2, 2)
    PN2_PAIR_G(A_DZ, 1, D_DZ, 4, 3, true)                          // layer 1 of a group_all level (gathered input) with a feature gradient
    PN2_PAIR_G(A_DZ, 1, D_DZ, 2, 2, true)
    PN2_PAIR_G(A_DZ, 2, D_DZ, 4, 3, true)
#undef PN2_PAIR
#undef PN2_PAIR_G
#ifdef PN2_PAIR_TRACE              /* lab build (scripts/build_mlp_labs.sh train_mlp_pair pairtrace:-DPN2_PAIR_TRACE): which pairs a run asks for that the table does not hold */
    fprintf(stderr, "no pair kernel: amode %d ns %d dcls %d tpw %d upw %d gather %d (rows %lld)\n", amode, g.ns, dcls, w.tpw, w.upw, (int)gather, pg.rows);
#endif
    return kNoPair;
}

}  // namespace pn2
