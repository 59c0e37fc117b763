// train_mlp_wgrad.hip -- the weight-gradient pass of the training node (see train_mlp.hip for the formulation): the launch of
// tl_wgrad_kernel (train_mlp_wgrad_tpw.h: the kernel, with or without the layer's data gradient in the same pass, and its
// instantiations, one translation unit per TPW) and the reductions of the workgroups' partial sums. gfx950.
#include "train_mlp_device.h"

#include <stdio.h>

namespace pn2 {

// The sum of the workgroups' slabs ([slab][workgroup][E floats]) -> the caller's weight gradient, ONE launch: a block owns 32
// consecutive floats of the slab layout ([tile][v >> 2][lane][v & 3]: what the workgroups dumped, so every partial is read as
// contiguous 128-byte pieces) and its eight groups of 32 threads each add an eighth of the workgroups, in order, in fp64;
// the eight sums meet in LDS and are added in order. A fixed order whatever the timing; two stages in two launches (fp32
// sums of 32 workgroups, then fp64) were 17-20 us per weight gradient on levels whose whole backward is 200 us, one thread
// per OUTPUT element read 4 of every 16 bytes it touched.
// (tl_wgrad_reduce_a_kernel below still serves tl_top_s_kernel's partials, train_mlp_top.hip.)
__global__ __launch_bounds__(256) void tl_wgrad_reduce_kernel(const float *__restrict__ in, long long nw, int TU, int TT, int tslabs,
                                                              int KI, int NO, float *__restrict__ gw, long long sk, long long sn,
                                                              double *__restrict__ plain, int accumulate)
{
    __shared__ double sh[8][32];
    const int ox = threadIdx.x & 31, ck = threadIdx.x >> 5;
    const int tu = (KI + 31) / 32, tt = (NO + 31) / 32, uslabs = (tu + TU - 1) / TU;
    const long long e = (long long)TU * TT * 1024, total = (long long)uslabs * tslabs * e;
    const long long chunk = (nw + 7) / 8;
    for (long long base = (long long)blockIdx.x * 32; base < total; base += (long long)gridDim.x * 32) {      // uniform trip count
        const long long i = base + ox, slab = i / e;
        const int r = (int)(i - slab * e), tile = r >> 10, q = r & 1023;
        const int v = ((q >> 8) << 2) | (q & 3), lane = (q >> 2) & 63;
        const int us = (int)(slab / tslabs), ts = (int)(slab - (long long)us * tslabs), ul = tile / TT, tl = tile - ul * TT;
        const int k = (us * TU + ul) * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3), n = (ts * TT + tl) * 32 + (lane & 31);
        const bool live = us * TU + ul < tu && ts * TT + tl < tt && k < KI && n < NO;
        double sum = 0.0;
        if (live) {
            const long long w0 = ck * chunk, w1 = w0 + chunk < nw ? w0 + chunk : nw;
            const float *src = in + (size_t)(slab * nw + w0) * e + r;
#pragma unroll 8
            for (long long w = w0; w < w1; ++w, src += e) sum += (double)*src;
        }
        sh[ck][ox] = sum;
        __syncthreads();
        if (ck == 0 && live) {
            double d = sh[0][ox];
#pragma unroll
            for (int c = 1; c < 8; ++c) d += sh[c][ox];
            if (plain) plain[(size_t)k * NO + n] = d;              // (KI, NO) row-major fp64, for the pooled top layer's fix-up
            else gw[k * sk + n * sn] = accumulate ? __fadd_rn(gw[k * sk + n * sn], (float)d) : (float)d;
        }
        __syncthreads();
    }
}

// sums of `chunk` consecutive workgroups' partials (layout unchanged): in [slab][nw][E] -> out [slab][nchunks][E]
__global__ __launch_bounds__(256) void tl_wgrad_reduce_a_kernel(const float4 *__restrict__ in, float4 *__restrict__ out,
                                                                long long nw, int chunk, long long nchunks, long long e4)
{
    const long long slab = blockIdx.z, ck = blockIdx.y;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < e4; i += (long long)gridDim.x * 256) {
        float4 sum = {0.0f, 0.0f, 0.0f, 0.0f};
        const long long w0 = ck * chunk, w1 = w0 + chunk < nw ? w0 + chunk : nw;
        for (long long w = w0; w < w1; ++w) {
            const float4 v = in[(slab * nw + w) * e4 + i];
            sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
        }
        out[(slab * nchunks + ck) * e4 + i] = sum;
    }
}

// tl_wgrad_kernel for the launch's shape: one translation unit per TPW (train_mlp_wgrad_tpw.h)
template <int TPW>
int launch_wgrad_tpw(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st);

// the sum of the workgroups' slabs -> the caller's weight gradient (or `plain`, fp64, for the pooled top layer's fix-up)
int launch_wgrad_reduce(const TlWgrad &p, const WgradShape &w, const pn2_bn_layer &L, hipStream_t st, double *plain)
{
    const long long total = (long long)w.uslabs * w.tslabs * (long long)w.e;     // floats of the slab layout
    long long blocks = (total + 31) / 32;
    if (blocks > 4096) blocks = 4096;
    return launch(tl_wgrad_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float *)p.partial, w.nw, w.tus, w.tts, w.tslabs,
                  p.kout > 0 ? p.kout : p.KI, p.NO, L.grad_weight, L.w_stride_k, L.w_stride_n, plain, L.grad_accumulate);
}

int launch_wgrad(TlWgrad &p, const WgradShape &w, const pn2_bn_layer &L, hipStream_t st, double *plain)
{
    if (p.partial_cap && w.partial_bytes > p.partial_cap) return PN2_E_ARG;   // never write past the planned buffer
    p.tus = w.tus; p.tts = w.tts; p.tslabs = w.tslabs;
    const dim3 grid((unsigned)w.gridx, (unsigned)(w.uslabs * w.tslabs));
    // lab build: cycles per phase and wave of workgroup 0, printed per launch. The switch is read here and in the kernel body
    // (tl_wgrad_body.inc, compiled in train_mlp_wgrad_tpw1 / 2 / 4.hip), so all four sources take it:
    //   scripts/build_mlp_labs.sh train_mlp_wgrad,train_mlp_wgrad_tpw1,train_mlp_wgrad_tpw2,train_mlp_wgrad_tpw4 wgtime:-DPN2_WG_TIMING
#ifdef PN2_WG_TIMING
    static unsigned long long *tbuf = nullptr;
    if (!tbuf) (void)hipMalloc(&tbuf, 48 * sizeof(unsigned long long));
    (void)clear_async(tbuf, 48 * sizeof(unsigned long long), st);
    p.timing = tbuf;
#endif
    int rc = p.mask ? launch_masked_wgrad(p, w, grid, st)          // ragged rows: kernels of their own (train_mlp_ragged.hip)
           : w.tpw == 1 ? launch_wgrad_tpw<1>(p, w, grid, st) : w.tpw == 2 ? launch_wgrad_tpw<2>(p, w, grid, st)
                                                                             : launch_wgrad_tpw<4>(p, w, grid, st);
    if (rc) return rc;
#ifdef PN2_WG_TIMING
    {
        unsigned long long h[48];
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h, tbuf, sizeof(h), hipMemcpyDeviceToHost);
        const double nb = (double)((p.rows / 32 + w.gridx - 1) / w.gridx);
        fprintf(stderr, "wgtime KI %d NO %d dy %d tus %d tts %d blocks/wg %.0f (cycles per block: units | barrier | loads+dW | dy mfma | dy epilogue | loop)\n",
                p.KI, p.NO, p.dy_w ? 1 : 0, w.tus, w.tts, nb);
        for (int wv = 0; wv < 8; ++wv)
            fprintf(stderr, "  wave %d: %7.0f %7.0f %7.0f %7.0f %7.0f %7.0f\n", wv, h[wv * 6] / nb, h[wv * 6 + 1] / nb, h[wv * 6 + 2] / nb,
                    h[wv * 6 + 3] / nb, h[wv * 6 + 4] / nb, h[wv * 6 + 5] / nb);
    }
#endif
    return launch_wgrad_reduce(p, w, L, st, plain);
}

// sums of 32 consecutive partials each, ahead of an fp64 stage (tl_top_s_kernel's partials: launch_top_s, train_mlp_top.hip)
int launch_wgrad_reduce_a(const float4 *in, float4 *out, long long nw, int chunk, long long nchunks, long long e4, hipStream_t st)
{
    long long bx = (e4 + 255) / 256;
    if (bx > 64) bx = 64;
    return launch(tl_wgrad_reduce_a_kernel, dim3((unsigned)bx, (unsigned)nchunks, 1u), dim3(256), 0, st, in, out, nw, chunk, nchunks, e4);
}

}  // namespace pn2
