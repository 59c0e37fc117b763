// train_mlp_gemm.hip -- the GEMM pass of the training node (see train_mlp.hip for the formulation): tl_gemm_kernel, the
// weight packing tl_pack_kernel, and their launches. gfx950.
#include "train_mlp_device.h"

#include <stdlib.h>
#include <string.h>

namespace pn2 {

// STATS = false: the pass sums nothing (TlGemm::nostats: frozen batch-norm statistics, train_mlp_frozen.hip)
template <int NS, int AMODE, bool STATS = true>
__global__ __launch_bounds__(kTlThreads) void tl_gemm_kernel(const TlGemm p)
{
#define PN2_BX blockIdx.x
#define PN2_BY blockIdx.y
#define PN2_GX gridDim.x
#define PN2_STATS STATS
#define PN2_MASKED false
#include "tl_gemm_body.inc"
#undef PN2_BX
#undef PN2_BY
#undef PN2_GX
#undef PN2_STATS
#undef PN2_MASKED
}

// ---- weights -> three-level bf16 operand tiles, on the device ---------------------------------------------------------
// value for K16 step e, level, lane l, slot j of pair (slab, u, t) = level of W[32u + 16e + 8(l >> 5) + j][32(slab NS + t) + (l & 31)]
__global__ __launch_bounds__(256) void tl_pack_kernel(const TlPackJobs jobs)
{
    if (jobs.ident && blockIdx.x == 0 && blockIdx.y == 0)         // dz = 1 * g - 0 - 0 * z (layer 1 per point: S enters as it is)
        for (int i = threadIdx.x; i < 3 * jobs.ident_c; i += 256) jobs.ident[i] = i < jobs.ident_c ? 1.0f : 0.0f;
    if (jobs.tickets && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < kFinTickets) jobs.tickets[threadIdx.x] = 0u;
    const TlPackJob &q = jobs.j[blockIdx.y];
    const long long total = (long long)q.slabs * q.tk * q.ns * 128;     // one thread per (pair, e, lane)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int lane = (int)(i & 63), e = (int)((i >> 6) & 1);
        const long long pair = i >> 7;
        const int t = (int)(pair % q.ns), u = (int)((pair / q.ns) % q.tk), slab = (int)(pair / ((long long)q.ns * q.tk));
        const int n = (slab * q.ns + t) * 32 + (lane & 31);
        f32x16 x;
#pragma unroll
        for (int v = 0; v < 16; ++v) x[v] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 32 * u + 16 * e + 8 * (lane >> 5) + j;
            x[j] = (k < q.K && n < q.N) ? q.w[k * q.sk + n * q.sn] : 0.0f;
        }
        const ActSplit sp = split_act(x);
        u32x4 *o = q.out + pair * kPairVec + (size_t)e * 192 + lane;
        o[0] = sp.p[0][0];
        o[64] = sp.p[0][1];
        o[128] = sp.p[0][2];
    }
}

// (Measured and not kept, round 4: a workgroup splitting its own resident slab from the fp32 weight instead of copying the
// packed tiles -- one launch of 7-9 us fewer per direction, but +5-7 us in EVERY GEMM of the level (4-6 trips of eight strided
// loads and a split per thread ahead of the first MFMA; with all loads issued up front the 48 live registers cost more than
// the latency they hid: sem_seg SA4 backward 245 -> 269 us, the metric level's data gradient 266 -> 292 us).
void add_pack_job(TlPackJobs &jobs, int &n, const float *w, long long sk, long long sn, const GemmShape &g, void *out)
{
    TlPackJob &q = jobs.j[n++];
    q.w = w; q.sk = sk; q.sn = sn; q.K = g.K; q.N = g.N; q.tk = g.tk; q.ns = g.ns; q.slabs = g.slabs;
    q.out = reinterpret_cast<u32x4 *>(out);
}

int launch_pack_jobs(const TlPackJobs &jobs, int n, hipStream_t st)
{
    if (n == 0) return PN2_OK;
    long long most = 0;
    for (int i = 0; i < n; ++i) {
        const long long total = (long long)jobs.j[i].slabs * jobs.j[i].tk * jobs.j[i].ns * 128;
        if (total > most) most = total;
    }
    long long blocks = (most + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    return launch(tl_pack_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, st, jobs);
}

int launch_pack(const float *w, long long sk, long long sn, const GemmShape &g, void *out, hipStream_t st)
{
    TlPackJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    int n = 0;
    add_pack_job(jobs, n, w, sk, sn, g, out);
    return launch_pack_jobs(jobs, n, st);
}

template <int NS>
static int launch_gemm_ns(int amode, const TlGemm &p, const GemmShape &g, dim3 grid, hipStream_t st)
{
#define PN2_TL_CASE(M)                                                                   \
    case M: {                                                                            \
        auto kern = p.nostats ? tl_gemm_kernel<NS, M, false> : tl_gemm_kernel<NS, M, true>; \
        if (int rc = allow_dynamic_lds(kern, lds)) return rc;                            \
        return launch(kern, grid, dim3(kTlThreads), lds, st, p);                         \
    }
    const size_t lds = (p.fin.ticket && g.lds < kFinLds) ? kFinLds : g.lds;             // the folded finalisation's scratch (tl_fin_tail)
    switch (amode) {
        PN2_TL_CASE(A_PLAIN)
        PN2_TL_CASE(A_GATHER)
        PN2_TL_CASE(A_RELU)
        PN2_TL_CASE(A_DZ)
        PN2_TL_CASE(A_DZ_POOL)
        PN2_TL_CASE(A_FILL)
    }
#undef PN2_TL_CASE
    return PN2_E_ARG;
}

dim3 prep_gemm(TlGemm &p, const GemmShape &g, const Opts &o)
{
    p.K = g.K; p.N = g.N; p.tk = g.tk; p.resident = g.resident;
    {
        const size_t obytes = (size_t)p.rows * g.N * sizeof(float);
        p.nt = o.nt == PN2_OPT_OFF ? 0 : o.nt == PN2_OPT_ON ? 1 : obytes >= ((size_t)128 << 20);
#ifdef PN2_TL_LAB_BUILD            /* timing-study builds only (scripts/build_mlp_labs.sh train_mlp_gemm): 1 = no stores, 2 = no statistics */
        p.lab = getenv("PN2_TL_LAB") ? atoi(getenv("PN2_TL_LAB")) : 0;
#else
        p.lab = 0;
#endif
    }
    const long long rounds = (p.rows / 32 + kTlWaves - 1) / kTlWaves;
    long long gx = kMaxParts / g.slabs;                        // persistent: one 8-wave workgroup per CU over all slabs
    if (gx < 1) gx = 1;
    if (gx > rounds) gx = rounds;
    return dim3((unsigned)gx, (unsigned)g.slabs);
}

int launch_gemm(int amode, TlGemm &p, const GemmShape &g, hipStream_t st, const Opts &o, int *nparts)
{
    const dim3 grid = prep_gemm(p, g, o);
    if (nparts) *nparts = (int)grid.x;
    if (p.fin.ticket) { p.fin.total = grid.x * grid.y; p.fin.nparts = (int)grid.x; }
    if (p.mask) return launch_masked_gemm(amode, p, g, grid, st);      // ragged rows: kernels of their own (train_mlp_ragged.hip)
    if (g.ns == 4) return launch_gemm_ns<4>(amode, p, g, grid, st);
    if (g.ns == 2) return launch_gemm_ns<2>(amode, p, g, grid, st);
    return launch_gemm_ns<1>(amode, p, g, grid, st);
}

}  // namespace pn2
