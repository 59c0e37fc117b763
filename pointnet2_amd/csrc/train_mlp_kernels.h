// train_mlp_kernels.h -- the kernels of the training node as its host code (train_mlp.hip) sees them: the parameter structs
// that tl_train_forward / tl_train_backward fill, the constants the size rules share with the kernels, and the launch
// functions of every kernel family, one translation unit each. It defines no device code of its own (the node's is
// train_mlp_device.h) and no host logic; sa_mlp_common.h, included for u32x4 and kPairWords, brings its device helpers and
// pn2_device.h's static pn2_clear_kernel along, so every file that includes this one is built with the Makefile's MLPFLAGS.
#pragma once
#include "sa_mlp_common.h"        // u32x4, kPairWords
#include "train_mlp_internal.h"   // the shape structs, GroupDims, Opts

namespace pn2 {

constexpr int kTlThreads = 512;          // GEMM workgroup: 8 waves, one 32-row item each per round
constexpr int kTlWaves = kTlThreads / 64;
constexpr int kPairVec = kPairWords / 4; // 16-byte vectors of one 32x32 weight tile pair
constexpr int kMaxParts = 256;           // rows of a per-channel partial-sum array (one per row workgroup)

enum { A_PLAIN = 0, A_GATHER = 1, A_RELU = 2, A_DZ = 3, A_DZ_POOL = 4, A_FILL = 5 };
enum { E_STORE = 0, E_POOL = 1, E_MASK = 2, E_PLAIN = 3 };

// ---- per-channel finalisations, folded into the launch that produces their partial sums --------------------------------------
// Between two passes of a level stands a reduction over ALL rows: the workgroups of a pass leave one partial row each, and a
// 5 us launch (tl_bn_finalize_kernel / tl_bn_backward_finalize_kernel) turns the rows into the next pass's coefficients. A
// level of a few thousand rows is ~25 launches of which a third are such 5 us finalisations (profiles/r04: sem_seg SA4 forward
// 89 us in 9 launches, 24 of them in pack / finalise launches). TlFin folds the finalisation into the producer: every workgroup
// publishes its partial row (device-scope release), takes a ticket, and the workgroup that draws the LAST ticket -- all rows
// are then visible to it (device-scope acquire) -- does the finalisation before it exits. No workgroup ever waits for another:
// nothing can hang. The sums are added in a fixed order (J contiguous chunks of the partial rows, each in ascending order, the
// chunk sums in ascending order), so results do not depend on which workgroup comes last. Tickets live in the caller's workspace
// and are zeroed by the direction's first launch (tl_pack_kernel).
struct TlFin {
    unsigned *ticket;           // nullptr: not folded (the caller launches the finalisation kernel)
    unsigned total;             // workgroups that publish a partial row (all of them take a ticket)
    int mode;                   // 1: batch moments -> (mean, invstd, a, c) + running statistics; 2: (sum dy, sum dy z) -> grad_gamma, grad_beta, dz coefficients
    int nparts, N;
    const double *stats;        // (nparts, 2, N) partial rows -- written by THIS launch, read after the ticket
    double count;
    const float *gamma, *beta, *bias;
    float *running_mean, *running_var;
    float momentum, eps;
    int var_biased;
    float *save;                // mode 1: written (4, N); mode 2: read
    float *grad_gamma, *grad_beta, *coef;
    int accumulate;
};

constexpr size_t kFinLds = 16 * 512 + 64;          // LDS the tail needs at 512 threads: two doubles per thread + the flag
constexpr int kFinTickets = 16;                    // one counter per layer of a direction

struct TlGather {
    int n, m, nsample, cfeat, xyz_off, feat_off;
    const float *xyz, *new_xyz, *points;
    const int *idx;
};

struct TlGemm {
    long long rows;
    int K, N;                   // contraction width = pitch of A; output width = pitch of out / zprev
    int tk;                     // 32-wide k tiles
    int resident;               // every k tile's weights stay in LDS
    // A operand
    const float *A;             // A_PLAIN: x; A_RELU: z of the layer below; A_DZ / A_DZ_POOL: z of this layer
    const float *G;             // A_DZ: dy (rows, K); A_DZ_POOL: gq (groups, K)
    const int *argsel;          // A_DZ_POOL: (groups, K)
    const float *p0, *p1, *p2;  // A_RELU: a, c; A_DZ*: s, c0, c1   (K floats each)
    int group_rows;             // A_DZ_POOL, A_FILL
    // A_FILL (pooled top layer without its pre-norm tensor, see pn2_mlp_train_backward): k tiles [0, tk0) are the routed
    // gradient s dy -- (argsel == sample) ? p0[k] * G[group][k] : 0, K0 channels -- and k tiles [tk0, tk) are
    // h = relu(q0 * A2 + q1) of the layer below (K1 channels, pitch K1)
    int tk0, K0, K1;
    const float *A2, *q0, *q1;
    TlGather g;                 // A_GATHER
    const u32x4 *wpacked;       // [slab][k tile][NS] tile pairs
    const float *bias;          // (N) or nullptr
    // epilogue
    int emode;
    float *out;                 // E_STORE / E_POOL: z (rows, N); E_MASK: dy of the layer below (rows, N); E_PLAIN: see col0
    int out_pitch, col0, col1;  // E_PLAIN: columns [col0, col1) go to out[row * out_pitch + col - col0]
    double *stats;              // (2, N): E_STORE / E_POOL: sum z, sum z^2; E_MASK: sum dy, sum dy * zprev
    const float *zprev, *ea, *ec;   // E_MASK: pre-norm tensor of the layer below (rows, N) and its (a, c)
    float *pmax;                // E_POOL partials (rows / prow, N): the extremum the pool will select -- the max of z where
    int *pamax;                 // gamma >= 0, the min where gamma < 0 (batch norm + ReLU are monotone per channel) -- and its row
    const float *pool_gamma;    // E_POOL: (N) batch-norm scale of this layer (its sign picks max or min)
    int prow;                   // 32 or 16
    int nt;                     // streaming (non-temporal) stores: outputs that do not fit the 256 MB Infinity Cache anyway
    int lab;                    // lab builds of the timing study only (PN2_TL_LAB, prep_gemm): 1 = no stores, 2 = no statistics; 0 in production
    int nostats;                // 1: the kernel's compile-time "no statistics" variant (frozen batch-norm statistics); stats is NULL then
    TlFin fin;                  // the per-channel finalisation of `stats`, by the workgroup that finishes last (fin.ticket != nullptr)
    const unsigned *mask;       // ragged rows (train_mlp_ragged.hip): bit r & 31 of word r / 32 = row r is valid; nullptr: every row is
};

// ---- weights -> three-level bf16 operand tiles, on the device (tl_pack_kernel, train_mlp_gemm.hip) ----
struct TlPackJob { const float *w; long long sk, sn; int K, N, tk, ns, slabs; u32x4 *out; };
struct TlPackJobs {                                               // one launch packs every layer of a level (blockIdx.y = layer)
    TlPackJob j[8];
    float *ident; int ident_c;                                    // ... and writes the identity coefficients (1, 0, 0) x ident_c, if wanted
    unsigned *tickets;                                            // ... and zeroes the tickets of the direction's folded finalisations (TlFin)
};

// ---- weight gradient: dW (KI x NO) = h^T dz, contraction over the rows -----------------------------------------------------
struct TlWgrad {
    long long rows;
    int amode;                  // A_PLAIN / A_GATHER / A_RELU: how h (rows, KI) is formed
    int KI;
    const float *A, *pa, *pc;
    TlGather g;
    int dmode;                  // A_DZ / A_DZ_POOL / A_FILL
    int NO;                     // A_FILL: tf * 32 + tx * 32 + 32 columns: [routed gradient (NF) | h again (KI) | ones] (wg_plan_unit)
    int tf, NF;                 // A_FILL: tiles / channels of the routed-gradient block
    int xshare;                 // A_FILL: every tile of h is in the slab's image, the "h again" tiles are read from there
    const float *Z, *G;
    const int *argsel;
    const float *coef;          // (3, NO): s, c0, c1
    int group_rows;
    float *partial;             // [slab][workgroup][tus * tts tiles][1024]
    size_t partial_cap;         // host side: bytes planned for `partial` (0 = unchecked); a launch whose slabs need more is refused
    int kout;                   // host side: rows of dW the reduction writes (0 = KI; a zero-padded input: its true width)
    int tus, tts, tslabs;       // tiles of h / of dz per slab; slabs along dz
    // ---- the layer's DATA gradient in the same pass (template flag DY; one slab only): dy_{l-1} = (second operand) . Wt,
    // contraction over the k tiles the block image already holds, see "One pass per layer" in train_mlp_wgrad.hip
    const u32x4 *dy_w;          // packed operand tiles [k tile][dy_nt] of Wt (tl_pack_kernel, ns = dy_nt, one slab)
    int dy_tk, dy_nt;           // k tiles (32 channels) of the contraction / 32-column tiles of the output
    int dy_tf;                  // D_TOP with shared h tiles: k tiles >= dy_tf are image tiles (u - dy_tf), the others tus + u
    int dy_cols, dy_pitch;      // output columns / floats per row of dy_out and dy_zprev
    float *dy_out;              // (rows, dy_pitch)
    const float *dy_zprev, *dy_ea, *dy_ec;   // ReLU mask of the layer below: its pre-norm tensor and (a, c); nullptr: plain store
    const float *dy_bias;       // constant row added to every output row (D_TOP: -r) or nullptr
    double *dy_stats;           // (gridDim.x, 2, dy_pitch): sum dy, sum dy * zprev of this workgroup's rows, or nullptr
    int dy_nt_store;            // streaming stores
    int single;                 // ONE block image in LDS (two barriers per block) instead of two
    int dy_acopy;               // the dense second-operand units also write their fragments in the data gradient's own layout
    // Layer 1 of a level WITHOUT features below this layer (its input is the three centred coordinates x of a row): the
    // data gradient produced here is dy_1, and all that is wanted from it is dW_1 = x^T dz_1. With dz_1 = s dy_1 - c0 - c1 z_1
    // and z_1 = x W_1:   dW_1 = s (x^T dy_1) - c0 (x^T 1) - c1 ((x^T x) W_1)   -- the last two from nine moments of x, the
    // first accumulated HERE from the epilogue's registers. dy_1 is then never written and the pass over (dy_1, z_1) that
    // formed dW_1 (tl_l1_dz_kernel) disappears.
    const float4 *l1x;          // (rows) centred coordinates of every row, w = 0 (tl_l1_xrows_kernel) or nullptr
    double *l1a;                // (gridDim.x, 3, dy_pitch): sum over this workgroup's rows of x[k] * dy[.][col]
    int xr_off;                 // byte offset of the coordinate rows in LDS
    unsigned long long *timing; // lab builds (PN2_WG_TIMING, launch_wgrad): per-wave cycle counts of the block loop's phases, workgroup 0
    const unsigned *mask;       // ragged rows (train_mlp_ragged.hip): the validity word of every 32-row block, or nullptr
};

// ---- the ROUTED part of the pooled top layer's weight gradient on the vector units (tl_top_s_kernel, train_mlp_top.hip) ----
struct TlTopS {
    long long groups;
    int ns, K, NF, GB, ld;                  // rows per group, input / output channels, groups per batch, LDS row pitch (floats)
    const float *z, *pa, *pc;               // z_{L-1} (rows, K) and the coefficients of h = relu(pa z + pc)
    const float *gq;                        // (groups, NF) routed gradient
    const int *argsel;                      // (groups, NF) pooled sample of the group
    const float *coef;                      // s (NF)
    float *partial;                         // (gridDim.x, K, NF)
};
constexpr int kTopSThreads = 512, kTopSGroups = 8;

// ---- layer 1 of a grouped level on the vector units, once per point or from the coordinates alone (train_mlp_l1.hip) ----
struct TlL1 {
    long long rows;
    int n, m, nsample, C;                   // points per cloud, groups per cloud, rows per group, cout_1
    const float *xyz, *new_xyz;             // (b,n,3), (b,m,3) or nullptr
    const int *idx;                         // (rows)
    const float *P;                         // forward: (b n, C)
    const float *wx;                        // forward: W1x, 3 rows of the weight: wx[k * skx + col * sn]
    long long skx, sn;
    const float *bias;                      // forward: (C) or nullptr
    float *z;                               // forward: out (rows, C);  backward: z_1 (rows, C)
    double *stats;                          // forward: (workgroups, 2, C) partial sums
    float *g;                               // backward: dy_1 in, dz_1 out (rows, C)
    const float *coef;                      // backward: (3, C): s, c0, c1
    float *part;                            // backward: (workgroups, 3 + cf, C) partial dW1 rows: coordinates, then features
    // backward, a FEW feature channels beside the coordinates whose gradient nobody wants (the input normals of cls_msg /
    // part_seg level 1): gathered per row and handled like three more coordinates -- the weight gradient of a layer of six
    // inputs is no more a matrix-core job than one of three (forward keeps the gathered GEMM: measured faster there)
    const float *points;                    // (b n, cf) or nullptr
    int cf;                                 // 0..kL1MaxFeat
};
constexpr int kL1MaxFeat = 5;               // 3 + 5 = 8 inputs at most on the vector units
constexpr int kL1Threads = 512, kL1U = 4;         // (the thread layout: train_mlp_l1.hip)

// ---- train_mlp.hip ----
TlGather make_gather(const pn2_group_src *g);

// ---- train_mlp_gemm.hip: tl_gemm_kernel, tl_pack_kernel ----
void add_pack_job(TlPackJobs &jobs, int &n, const float *w, long long sk, long long sn, const GemmShape &g, void *out);
int launch_pack_jobs(const TlPackJobs &jobs, int n, hipStream_t st);
int launch_pack(const float *w, long long sk, long long sn, const GemmShape &g, void *out, hipStream_t st);
dim3 prep_gemm(TlGemm &p, const GemmShape &g, const Opts &o);
int launch_gemm(int amode, TlGemm &p, const GemmShape &g, hipStream_t st, const Opts &o, int *nparts = nullptr);

// ---- train_mlp_wgrad.hip: tl_wgrad_kernel and the reductions of the workgroups' partial sums ----
int launch_wgrad(TlWgrad &p, const WgradShape &w, const pn2_bn_layer &L, hipStream_t st, double *plain = nullptr);
int launch_wgrad_reduce(const TlWgrad &p, const WgradShape &w, const pn2_bn_layer &L, hipStream_t st, double *plain);
int launch_wgrad_reduce_a(const float4 *in, float4 *out, long long nw, int chunk, long long nchunks, long long e4, hipStream_t st);

// ---- train_mlp_pair.hip: tl_pair_kernel ----
constexpr int kNoPair = -12345;     // launch_pair: no kernel for this pair of shapes, the caller launches the two passes
int launch_pair(int amode, TlGemm &pg, const GemmShape &g, TlWgrad &pw, const WgradShape &w, const pn2_bn_layer &L, hipStream_t st,
                const Opts &o, int *nparts, double *plain = nullptr);

// ---- train_mlp_top.hip: the pooled top layer without its pre-norm tensor ----
int launch_top_mats(const float *w, long long sk, long long sn, int K, int NF, int NFp, const float *coef, const float *bias, float *wp,
                    float *rowc, hipStream_t st);
int launch_top_wgrad_fix(const double *sf, int ld, int K, int NF, int goff, int hoff, const float *w, long long sk, long long sn,
                         const float *coef, const float *bias, float *gw, const double *S, int accumulate, hipStream_t st);
int launch_top_s(TlTopS &p, const TopSShape &t, float *part2, double *s64, hipStream_t st);

// ---- train_mlp_l1.hip ----
int launch_l1_forward(long long rows, const GroupDims &gd, const pn2_group_src *group, const pn2_bn_layer &L, const float *P,
                      double *stats, hipStream_t st, int *nparts);
int launch_l1_dz(long long rows, const GroupDims &gd, const pn2_group_src *group, const pn2_bn_layer &L, float *dy, const float *coef,
                 float *part, bool store, hipStream_t st, bool wgrad = true);
int launch_l1_xrows(const TlL1 &q, float4 *xg, double *mom, hipStream_t st, int *nparts);
int launch_l1_wx_combine(const double *mom, int nmom, const double *l1a, int nparts, int C, int pitch, const float *coef,
                         const float *wx, long long skx, long long sn, float *gw, int accumulate, hipStream_t st);

// ---- train_mlp_small.hip: the per-channel and pooling kernels, one launch each (parts: rows of the partial-sum array) ----
// (count: the row count read from device memory -- ragged rows: the number of valid rows -- or nullptr: `rows`)
int launch_bn_finalize(const double *stats, int nparts, int N, double rows, const double *count, const float *gamma, const float *beta,
                       float *running_mean, float *running_var, float momentum, float eps, float *save, const float *bias,
                       int var_biased, hipStream_t st);
int launch_bn_backward_finalize(const double *stats, int nparts, int N, double rows, const double *count, const float *gamma,
                                const float *save, float *grad_gamma, float *grad_beta, float *coef, int accumulate, hipStream_t st);
int launch_pool_finalize(long long groups, int N, int parts, int prow, const float *pmax, const int *pamax, const float *gamma,
                         const float *save, float *out, int *argsel, float *zsel, hipStream_t st);
int launch_pool_grad(long long groups, int N, const float *out, const float *gout, const float *zsel, float *gq, double *stats,
                     int parts, hipStream_t st);
int launch_apply(long long total4, int N, const float *z, const float *save, const unsigned *mask, float *out, hipStream_t st);
int launch_top_grad(long long rows, int N, const float *out, const float *gout, const float *z, float *dy, double *stats, int parts,
                    hipStream_t st);
int launch_pool_weights(long long groups, int ns, int n, int m, const float *xyz, const float *new_xyz, const int *idx, float *w,
                        hipStream_t st);
int launch_pool_avg(long long groups, int ns, int N, const float *z, const float *save, const float *pool_w, const float *maxv,
                    float *out, hipStream_t st);
int launch_pool_top_grad(long long rows, int ns, int N, const float *gout, const float *z, const float *save, const float *pool_w,
                         const int *argsel, float *dy, double *stats, int parts, hipStream_t st);
int launch_identity_coef(int C, float *coef, hipStream_t st);
// (the grouped rows of a ragged batch: the max pool over the valid rows of the stored z_L, and the dense dy_L it routes back)
int launch_pool_masked(long long groups, int ns, int N, const float *z, const float *gamma, const float *save, const unsigned *mask,
                       float *out, int *argsel, hipStream_t st);
int launch_pool_top_grad_masked(long long rows, int ns, int N, const float *out, const float *gout, const int *argsel,
                                const unsigned *mask, const float *z, float *dy, double *stats, int parts, hipStream_t st);

// ---- train_mlp_ragged.hip: plain rows of a ragged batch (pn2_mlp_train_*_ragged) ----
// The caller's mask buffer: the number of valid rows as a double, then one validity word per 32 rows
constexpr size_t kRaggedWordsOff = 16;
inline const double *ragged_count(const void *mask) { return static_cast<const double *>(mask); }
inline const unsigned *ragged_words(const void *mask)
{
    return reinterpret_cast<const unsigned *>(static_cast<const char *>(mask) + kRaggedWordsOff);
}
// (b clouds of n rows, the first unit * clamp(lengths[c], 1, cap) of each valid; unit = 0: plain rows, unit 1 and cap n)
int launch_ragged_mask(int b, int n, const int *lengths, void *mask, hipStream_t st, int unit = 0, int cap = 0);
int launch_masked_gemm(int amode, const TlGemm &p, const GemmShape &g, dim3 grid, hipStream_t st);
int launch_masked_wgrad(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st);

// ---- train_mlp_ragged_group.hip: the grouped rows of a ragged batch (pn2_mlp_train_*_group_ragged): layer 1's gathered passes ----
int launch_masked_gather_gemm(const TlGemm &p, const GemmShape &g, dim3 grid, hipStream_t st);
int launch_masked_gather_wgrad(const TlWgrad &p, const WgradShape &w, dim3 grid, hipStream_t st);

}  // namespace pn2
