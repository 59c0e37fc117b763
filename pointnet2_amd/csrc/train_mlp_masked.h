// train_mlp_masked.h -- the GEMM pass with a row mask as a kernel template (tl_gemm_body.inc, PN2_MASKED), for the translation
// units that instantiate it: train_mlp_ragged.hip (A_PLAIN / A_RELU / A_DZ: the plain rows of a ragged batch and the layers
// above layer 1 of a grouped one) and train_mlp_ragged_group.hip (A_GATHER: layer 1 of a grouped level). Every instantiation is
// made in exactly one of the two.
#pragma once
#include "train_mlp_device.h"

namespace pn2 {

template <int NS, int AMODE>
__global__ __launch_bounds__(kTlThreads) void tl_gemm_masked_kernel(const TlGemm p)
{
#define PN2_BX blockIdx.x
#define PN2_BY blockIdx.y
#define PN2_GX gridDim.x
#define PN2_STATS true
#define PN2_MASKED true
#include "tl_gemm_body.inc"
#undef PN2_BX
#undef PN2_BY
#undef PN2_GX
#undef PN2_STATS
#undef PN2_MASKED
}

}  // namespace pn2
