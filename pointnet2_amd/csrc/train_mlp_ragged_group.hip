// train_mlp_ragged_group.hip -- the training node on the GROUPED rows of a ragged batch (pn2_mlp_train_*_group_ragged,
// include/pn2ops.h): an SA level whose clouds hold counts[c] <= m valid centroids each, or a group_all level whose clouds hold
// counts[c] <= n valid points; max pooling, batch statistics. The batch moments, every gradient and the running averages are
// those of the valid rows alone, and the host never reads `counts`. gfx950.
//
// The invariant. In the flat row order r = (c m + j) nsample + k a row is valid iff j < counts[c]
// (whole groups) or, in a group_all level (m = 1, nsample = n), iff k < counts[c]: either way a PREFIX of the cloud's m nsample
// rows, the shape of mask the plain rows carry (train_mlp_ragged.hip: one validity word per 32 rows, N_valid on the device;
// tl_ragged_mask_kernel with a unit and a cap). Two selects make a padding row absent, as there:
//   h_0      the gathered row (A_GATHER in the GEMM's prologue, the K_HGATHER units of the weight gradient) is taken as zero:
//            whatever xyz / points hold beyond a cloud's points never enters a product, and z_1 .. z_L of the row are 0;
//   dz_l     as on plain rows. dy_L is formed dense by tl_pool_top_grad_masked_kernel, +0.0 on padding rows.
// The pool is a pass of its own over the stored z_L (tl_pool_masked_kernel, train_mlp_small.hip): the extremum over the valid
// rows of a group. A gathered row needs its index in range whether it is valid or not: idx of a padding group holds indices in
// [0, n) (the ragged pair operators write 0), a group_all row is its own point.
//
// What is here: the masked instantiations the plain rows do not have -- tl_gemm_masked_kernel<NS, A_GATHER> and the gathered
// weight-gradient pass tl_wgrad_masked_gather_kernel<TPW, UPW> -- behind launch_masked_gemm / launch_masked_wgrad, and the entry
// points. The host side is train_mlp.hip's under one fixed organisation (ragged_group_opts there): layer 1 is the gathered GEMM,
// z_L is kept, a data-gradient GEMM and a weight-gradient pass per layer.
#include "train_mlp_masked.h"

#include <type_traits>

namespace pn2 {

int launch_masked_gather_gemm(const TlGemm &p, const GemmShape &g, dim3 grid, hipStream_t st)
{
#define PN2_TL_CASE(NS)                                                      \
    if (g.ns == NS) {                                                        \
        auto kern = tl_gemm_masked_kernel<NS, A_GATHER>;                     \
        if (int rc = allow_dynamic_lds(kern, g.lds)) return rc;              \
        return launch(kern, grid, dim3(kTlThreads), g.lds, st, p);           \
    }
    PN2_TL_CASE(4) PN2_TL_CASE(2) PN2_TL_CASE(1)
#undef PN2_TL_CASE
    return PN2_E_ARG;
}

// ---- the weight-gradient pass with the row mask and a GATHERED first operand (tl_wgrad_body.inc, PN2_MASKED): dz from (dy, z) ----
template <int TPW, int UPW>
__global__ __launch_bounds__(kTlThreads) void tl_wgrad_masked_gather_kernel(const TlWgrad p)
{
    constexpr bool GATHER = true, DY = false, L1X = false;
    constexpr int DCLS = D_DZ;
#define PN2_BX blockIdx.x
#define PN2_BY blockIdx.y
#define PN2_GX gridDim.x
#define PN2_MASKED true
#include "tl_wgrad_body.inc"
#undef PN2_BX
#undef PN2_BY
#undef PN2_GX
#undef PN2_MASKED
}

template <int TPW>
static int launch_masked_gather_wgrad_tpw(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st)
{
#define PN2_WG_CASE(U)                                                          \
    if (w.upw == U) {                                                           \
        auto kern = tl_wgrad_masked_gather_kernel<TPW, U>;                      \
        if (int rc = allow_dynamic_lds(kern, w.lds)) return rc;                 \
        return launch(kern, grid, dim3(kTlThreads), w.lds, st, p);              \
    }
    PN2_WG_CASE(1) PN2_WG_CASE(2) PN2_WG_CASE(3)
#undef PN2_WG_CASE
    return PN2_E_ARG;
}

int launch_masked_gather_wgrad(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st)
{
    if (!p.mask || p.dy_w || p.dmode != A_DZ || p.amode != A_GATHER) return PN2_E_ARG;
    return w.tpw == 1 ? launch_masked_gather_wgrad_tpw<1>(p, w, grid, st) : w.tpw == 2 ? launch_masked_gather_wgrad_tpw<2>(p, w, grid, st)
                                                                                         : launch_masked_gather_wgrad_tpw<4>(p, w, grid, st);
}

// 0 ok, else the PN2_E_* code both entries return before anything is launched
static int group_ragged_args(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group, int pool_rows,
                             const int *counts, const void *mask)
{
    if (!counts || !mask || !group || !layers) return PN2_E_NULL;
    if (nlayers < 1 || nlayers > 8) return PN2_E_ARG;
    int widths[9];
    for (int l = 0; l < nlayers; ++l) { widths[l] = layers[l].cin; widths[l + 1] = layers[l].cout; }
    const int gd[6] = {group->b, group->n, group->m, group->nsample, group->points ? group->cfeat : 0, group->idx ? 1 : 0};
    return tl_group_ragged_supported(rows, nlayers, widths, pool_rows, gd) ? PN2_OK : PN2_E_ARG;
}

static TlCall group_ragged_call(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group, int pool_rows,
                                const float *out, const int *argsel, void *mask, void *ws, const pn2_train_opts *opts, void *stream)
{
    TlCall c{};
    c.rows = rows; c.nlayers = nlayers; c.layers = layers;
    c.group = group;
    c.pool_rows = pool_rows;
    c.out = out; c.argsel = argsel;
    c.mask = mask; c.rg_b = group->b;
    c.rg_n = group->m * group->nsample;                            // (below 2^31: rows is)
    c.rg_unit = group->idx ? group->nsample : 1;                   // whole groups / the points of the one group
    c.rg_cap = group->idx ? group->m : group->n;
    c.ws = ws; c.opts = opts; c.stream = stream;
    return c;
}

}  // namespace pn2

extern "C" int pn2_mlp_train_group_ragged_supported(long long rows, int nlayers, const int *widths, int pool_rows, const int *group_dims)
{
    return pn2::tl_group_ragged_supported(rows, nlayers, widths, pool_rows, group_dims) ? 1 : 0;
}

extern "C" long long pn2_mlp_train_ws_bytes_group_ragged(long long rows, int nlayers, const int *widths, int pool_rows, int backward,
                                                         const int *group_dims, const pn2_train_opts *opts)
{
    return pn2::tl_group_ragged_ws_bytes(rows, nlayers, widths, pool_rows, backward, group_dims, opts);
}

extern "C" int pn2_mlp_train_forward_group_ragged(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                                  int pool_rows, const int *counts, float *out, int *argsel, void *mask, void *ws,
                                                  const pn2_train_opts *opts, void *stream)
{
    if (int rc = pn2::group_ragged_args(rows, nlayers, layers, group, pool_rows, counts, mask)) return rc;
    pn2::TlCall c = pn2::group_ragged_call(rows, nlayers, layers, group, pool_rows, out, argsel, mask, ws, opts, stream);
    c.lengths = counts;
    return pn2::tl_train_forward(c);
}

extern "C" int pn2_mlp_train_backward_group_ragged(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                                   int pool_rows, const int *counts, const float *out, const int *argsel,
                                                   const float *grad_out, float *grad_feat_rows, int reproducible, const void *mask,
                                                   void *ws, const pn2_train_opts *opts, void *stream)
{
    if (int rc = pn2::group_ragged_args(rows, nlayers, layers, group, pool_rows, counts, mask)) return rc;
    pn2::TlCall c = pn2::group_ragged_call(rows, nlayers, layers, group, pool_rows, out, argsel, const_cast<void *>(mask), ws, opts, stream);
    c.grad_out = grad_out;
    c.grad_feat_rows = grad_feat_rows;
    c.reproducible = reproducible;
    return pn2::tl_train_backward(c);
}

extern "C" int pn2_mlp_train_group_ragged_plan(long long rows, int nlayers, const int *widths, int pool_rows, const int *group_dims,
                                               const pn2_train_opts *opts, int *passes, int cap)
{
    if (!widths || !group_dims) return PN2_E_NULL;
    if (cap < 0 || !pn2::tl_group_ragged_supported(rows, nlayers, widths, pool_rows, group_dims)) return PN2_E_ARG;
    return pn2::tl_group_ragged_plan(rows, nlayers, widths, group_dims, opts, passes, cap);
}
