// train_mlp_wgrad_tpw.h -- tl_wgrad_kernel and its dispatch over the launch shapes, for ONE value of TPW (output tiles per wave)
// per translation unit: train_mlp_wgrad_tpw1 / 2 / 4.hip instantiate launch_wgrad_tpw<TPW>, train_mlp_wgrad.hip calls them. Every
// instantiation of the kernel is made in exactly one of the three (27, 27 and 15 kernels).
#pragma once
#include "train_mlp_device.h"

#include <type_traits>

namespace pn2 {

// Every wave keeps the rows of the NEXT TWO blocks in flight in registers (two raw sets, the block loop is unrolled by
// two), the block image in LDS is double buffered, one s_barrier per block.
// TPW: output tiles per wave; UPW: operand units a wave loads per 32-row block
//
// One pass per layer (DY): the weight gradient dW_l = h^T dz and the data gradient dy_{l-1} = (dz W_l^T) . [h > 0] consume
// the SAME two tiles of a row block -- dz_l from (dy_l, z_l) and h_{l-1} from z_{l-1} -- so as two kernels the layer's
// activations crossed HBM twice per direction. With DY the block image serves both: the waves that own no (or the fewest)
// dW tiles take one 32-column tile of dy_{l-1} each. Its A operand is the image read TRANSPOSED (lane = row: eight
// ds_read_u16 per 16-byte fragment instead of one ds_read_b128, no vector instruction but four packs -- the operand was
// formed, split and stored once, by the unit loads), its B operand the packed W^T, LDS-resident for the whole launch;
// the epilogue is the data-gradient GEMM's (mask of the layer below from its pre-norm tensor, the batch-norm backward
// sums, 128-byte row stores). The dy waves run their own copy of the block loop (template ROLE): vector-memory returns
// are counted in order, and a wait shared with waves that issue no mask loads / stores between two prefetches could
// only be the smaller count, i.e. the dy waves would wait for half of the prefetch they just issued.
template <int TPW, int UPW, bool GATHER, int DCLS, bool DY, bool L1X = false>
__global__ __launch_bounds__(kTlThreads) void tl_wgrad_kernel(const TlWgrad p)
{
#define PN2_BX blockIdx.x
#define PN2_BY blockIdx.y
#define PN2_GX gridDim.x
#define PN2_MASKED false
#include "tl_wgrad_body.inc"
#undef PN2_MASKED
#undef PN2_BX
#undef PN2_BY
#undef PN2_GX
}

template <int TPW, bool GATHER, int DCLS, bool DY = false, bool L1X = false>
static int launch_wgrad_kern(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st)
{
    const size_t lds = DY ? w.lds_dy : w.lds;
#define PN2_WG_CASE(U)                                                          \
    if (w.upw == U) {                                                           \
        auto kern = tl_wgrad_kernel<TPW, U, GATHER, DCLS, DY, L1X>;             \
        if (int rc = allow_dynamic_lds(kern, lds)) return rc;                   \
        return launch(kern, grid, dim3(kTlThreads), lds, st, p);                \
    }
    PN2_WG_CASE(1) PN2_WG_CASE(2) PN2_WG_CASE(3)
#undef PN2_WG_CASE
    return PN2_E_ARG;
}

template <int TPW>
int launch_wgrad_tpw(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st)
{
    if (p.dy_w) {                                                  // the data gradient in the same pass (fuse_shape: TPW <= 2, no gather)
        if constexpr (TPW > 2) return PN2_E_ARG;                   // (no such kernel, and none instantiated in this TPW's file)
        else {
            if (p.amode == A_GATHER) return PN2_E_ARG;
            if (p.dmode == A_FILL) return launch_wgrad_kern<TPW, false, D_TOP, true>(p, w, grid, st);
            if (p.l1x) return p.dmode == A_DZ ? launch_wgrad_kern<TPW, false, D_DZ, true, true>(p, w, grid, st) : PN2_E_ARG;
            return p.dmode == A_DZ_POOL ? launch_wgrad_kern<TPW, false, D_DZPOOL, true>(p, w, grid, st)
                                        : launch_wgrad_kern<TPW, false, D_DZ, true>(p, w, grid, st);
        }
    }
    if (p.dmode == A_FILL) return launch_wgrad_kern<TPW, false, D_TOP>(p, w, grid, st);
    if (p.amode == A_GATHER)
        return p.dmode == A_DZ_POOL ? launch_wgrad_kern<TPW, true, D_DZPOOL>(p, w, grid, st)
                                    : launch_wgrad_kern<TPW, true, D_DZ>(p, w, grid, st);
    return p.dmode == A_DZ_POOL ? launch_wgrad_kern<TPW, false, D_DZPOOL>(p, w, grid, st)
                                : launch_wgrad_kern<TPW, false, D_DZ>(p, w, grid, st);
}

}  // namespace pn2
