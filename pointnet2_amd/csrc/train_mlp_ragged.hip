// train_mlp_ragged.hip -- the training node on the plain rows of a RAGGED batch (pn2_mlp_train_*_ragged, include/pn2ops.h): b
// clouds padded to n rows each, cloud c holding clamp(lengths[c], 1, n) valid rows; the batch statistics, every gradient and the
// running averages are those of the valid rows alone, and the host never reads `lengths`. gfx950.
//
// The invariant. The node keeps z_l = h_{l-1} W_l WITHOUT the bias, so a padding row is absent from
// every pass once two values are taken as zero there, by SELECTS (the padding rows of x and of grad_out may hold anything):
//   h_{l-1}  where it is formed: x (A_PLAIN) and relu(a z + c) (A_RELU) in the GEMM's prologue, the K_H units of the weight
//            gradient, and `out` (tl_apply_masked_kernel). Then z_l of the row is exactly 0 at every layer: nothing enters
//            sum z or sum z^2, h^T dz gets nothing, `out` is 0, so tl_top_grad_kernel's out > 0 is false and dy_L is 0;
//   dz_l     where it is formed (s dy - c0 - c1 z would be -c0): A_DZ in the GEMM's prologue, the K_DZ units. Then the data
//            gradient's row is 0 (E_MASK selects between 0 + 0 and 0), nothing enters sum dy or sum dy z, and grad_x is 0.
// The row count of the two finalisations is the number of valid rows, read from device memory (tl_bn_*finalize_counted_kernel).
//
// What is here: the kernel that turns `lengths` into one validity word per 32 rows and the count; the MASKED instantiations of
// the GEMM body (A_PLAIN / A_RELU / A_DZ; the kernel template: train_mlp_masked.h) and of the weight-gradient body (dense rows,
// D_DZ) -- kernels of their own, the dense ones are not touched, launch_gemm / launch_wgrad come here when the call has a mask
// (and go on to train_mlp_ragged_group.hip for the gathered layer 1 of a grouped level); the entry points. The small masked and
// counted kernels stand beside their dense twins (train_mlp_small.hip: the apply, the finalisations; train_mlp_fp.hip: the FP
// node's layer-1 passes) behind ONE launch function per pair. The host side is train_mlp.hip's, under one fixed organisation
// (ragged_opts there): a data-gradient GEMM and a weight-gradient pass per layer, finalisations as launches of their own.
#include "train_mlp_masked.h"

#include <type_traits>

namespace pn2 {

__device__ __forceinline__ int rg_clamp(int len, int n) { return len < 1 ? 1 : len > n ? n : len; }

// one thread per validity word (32 rows, which may hold the tail of one cloud, its padding and the head of the next);
// block 0 also sums the clamped lengths -- integers: the count does not depend on the order.
// A cloud is n rows of which the first unit * clamp(lengths[c], 1, cap) are valid: unit 1 and cap n on plain rows and in a
// group_all level (lengths = points per cloud), unit nsample and cap m on the n = m nsample grouped rows of a cloud (lengths =
// centroids per cloud; train_mlp_ragged_group.hip)
__global__ __launch_bounds__(256) void tl_ragged_mask_kernel(int b, int n, int unit, int cap, const int *__restrict__ lengths,
                                                             double *__restrict__ count, unsigned *__restrict__ words, long long nwords)
{
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < nwords; w += (long long)gridDim.x * 256) {
        const long long r0 = w * 32;
        int c = (int)(r0 / n), i = (int)(r0 - (long long)c * n);
        int len = unit * rg_clamp(lengths[c], cap);
        unsigned m = 0u;
        for (int j = 0; j < 32; ++j) {
            if (i >= n) {
                i = 0;
                ++c;
                len = c < b ? unit * rg_clamp(lengths[c], cap) : 0;
            }
            m |= (i < len ? 1u : 0u) << j;
            ++i;
        }
        words[w] = m;
    }
    if (blockIdx.x != 0) return;
    __shared__ long long sh[256];
    long long s = 0;
    for (int c = threadIdx.x; c < b; c += 256) s += (long long)unit * rg_clamp(lengths[c], cap);
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = (double)sh[0];
}

int launch_ragged_mask(int b, int n, const int *lengths, void *mask, hipStream_t st, int unit, int cap)
{
    if (unit <= 0 || cap <= 0) { unit = 1; cap = n; }              // plain rows
    const long long nwords = (long long)b * n / 32;
    long long blocks = (nwords + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    return launch(tl_ragged_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, st, b, n, unit, cap, lengths,
                  const_cast<double *>(ragged_count(mask)),
                  const_cast<unsigned *>(ragged_words(mask)), nwords);
}

// ---- the GEMM pass with the row mask (tl_gemm_masked_kernel: train_mlp_masked.h) ----
template <int NS>
static int launch_masked_gemm_ns(int amode, const TlGemm &p, const GemmShape &g, dim3 grid, hipStream_t st)
{
#define PN2_TL_CASE(M)                                                       \
    case M: {                                                                \
        auto kern = tl_gemm_masked_kernel<NS, M>;                            \
        if (int rc = allow_dynamic_lds(kern, g.lds)) return rc;              \
        return launch(kern, grid, dim3(kTlThreads), g.lds, st, p);           \
    }
    switch (amode) {
        PN2_TL_CASE(A_PLAIN)
        PN2_TL_CASE(A_RELU)
        PN2_TL_CASE(A_DZ)
    }
#undef PN2_TL_CASE
    return PN2_E_ARG;
}

int launch_masked_gemm(int amode, const TlGemm &p, const GemmShape &g, dim3 grid, hipStream_t st)
{
    if (!p.mask || p.nostats || p.fin.ticket) return PN2_E_ARG;    // (no frozen form, no folded finalisation: its count is a value)
    if (amode == A_GATHER) return launch_masked_gather_gemm(p, g, grid, st);       // layer 1 of a grouped level (train_mlp_ragged_group.hip)
    if (g.ns == 4) return launch_masked_gemm_ns<4>(amode, p, g, grid, st);
    if (g.ns == 2) return launch_masked_gemm_ns<2>(amode, p, g, grid, st);
    return launch_masked_gemm_ns<1>(amode, p, g, grid, st);
}

// ---- the weight-gradient pass with the row mask (tl_wgrad_body.inc, PN2_MASKED): dense rows, dz from (dy, z) ----
template <int TPW, int UPW>
__global__ __launch_bounds__(kTlThreads) void tl_wgrad_masked_kernel(const TlWgrad p)
{
    constexpr bool GATHER = false, DY = false, L1X = false;
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
static int launch_masked_wgrad_tpw(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st)
{
#define PN2_WG_CASE(U)                                                          \
    if (w.upw == U) {                                                           \
        auto kern = tl_wgrad_masked_kernel<TPW, U>;                             \
        if (int rc = allow_dynamic_lds(kern, w.lds)) return rc;                 \
        return launch(kern, grid, dim3(kTlThreads), w.lds, st, p);              \
    }
    PN2_WG_CASE(1) PN2_WG_CASE(2) PN2_WG_CASE(3)
#undef PN2_WG_CASE
    return PN2_E_ARG;
}

int launch_masked_wgrad(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st)
{
    if (!p.mask || p.dy_w || p.dmode != A_DZ) return PN2_E_ARG;
    if (p.amode == A_GATHER) return launch_masked_gather_wgrad(p, w, grid, st);     // layer 1 of a grouped level (train_mlp_ragged_group.hip)
    if (p.amode != A_PLAIN && p.amode != A_RELU) return PN2_E_ARG;
    return w.tpw == 1 ? launch_masked_wgrad_tpw<1>(p, w, grid, st) : w.tpw == 2 ? launch_masked_wgrad_tpw<2>(p, w, grid, st)
                                                                                 : launch_masked_wgrad_tpw<4>(p, w, grid, st);
}

// b clouds of n rows -> the row count the node runs on, or 0: not a positive multiple of 32 below 2^31
static long long ragged_rows(int b, int n)
{
    if (b <= 0 || n <= 0) return 0;
    const long long rows = (long long)b * n;
    return (rows % 32 || rows >= (1ll << 31)) ? 0 : rows;
}

static bool ragged_widths_ok(int nlayers, const int *widths)
{
    return widths && nlayers >= 1 && nlayers <= 8 && widths[0] > 0 && widths[0] % 4 == 0;      // plain rows are read 16 bytes at a time
}

// 0 ok, else the PN2_E_* code both entries return before anything is launched
static int ragged_args(int b, int n, const int *lengths, const void *mask)
{
    if (!lengths || !mask) return PN2_E_NULL;
    return ragged_rows(b, n) ? PN2_OK : PN2_E_ARG;
}

static TlCall ragged_call(int b, int n, int nlayers, const pn2_bn_layer *layers, const float *x, const float *out, void *mask, void *ws,
                          const pn2_train_opts *opts, void *stream)
{
    TlCall c{};
    c.rows = ragged_rows(b, n); c.nlayers = nlayers; c.layers = layers;
    c.x = x;
    c.out = out;
    c.mask = mask; c.rg_b = b; c.rg_n = n;
    c.ws = ws; c.opts = opts; c.stream = stream;
    return c;
}

}  // namespace pn2

extern "C" int pn2_mlp_train_ragged_supported(int b, int n, int nlayers, const int *widths)
{
    const long long rows = pn2::ragged_rows(b, n);
    if (!rows || !pn2::ragged_widths_ok(nlayers, widths)) return 0;
    return (pn2::tl_ragged_ws_bytes(rows, nlayers, widths, 0, nullptr) >= 0 && pn2::tl_ragged_ws_bytes(rows, nlayers, widths, 1, nullptr) >= 0) ? 1 : 0;
}

extern "C" long long pn2_mlp_train_ws_bytes_ragged(int b, int n, int nlayers, const int *widths, int backward, const pn2_train_opts *opts)
{
    const long long rows = pn2::ragged_rows(b, n);
    if (!rows || !pn2::ragged_widths_ok(nlayers, widths)) return -1;
    return pn2::tl_ragged_ws_bytes(rows, nlayers, widths, backward, opts);
}

extern "C" int pn2_mlp_train_forward_ragged(int b, int n, const int *lengths, int nlayers, const pn2_bn_layer *layers, const float *x,
                                            float *out, void *mask, void *ws, const pn2_train_opts *opts, void *stream)
{
    if (int rc = pn2::ragged_args(b, n, lengths, mask)) return rc;
    pn2::TlCall c = pn2::ragged_call(b, n, nlayers, layers, x, out, mask, ws, opts, stream);
    c.lengths = lengths;
    return pn2::tl_train_forward(c);
}

extern "C" int pn2_mlp_train_backward_ragged(int b, int n, const int *lengths, int nlayers, const pn2_bn_layer *layers, const float *x,
                                             const float *out, const float *grad_out, float *grad_x, const void *mask, void *ws,
                                             const pn2_train_opts *opts, void *stream)
{
    if (int rc = pn2::ragged_args(b, n, lengths, mask)) return rc;
    pn2::TlCall c = pn2::ragged_call(b, n, nlayers, layers, x, out, const_cast<void *>(mask), ws, opts, stream);
    c.grad_out = grad_out;
    c.grad_x = grad_x;
    return pn2::tl_train_backward(c);
}
