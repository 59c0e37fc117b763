// train_mlp_internal.h -- what the files of the training node share. train_mlp.hip is its host side (the size rules, the plan,
// the passes of both directions); train_mlp_gemm / _wgrad / _pair / _top / _l1 / _small.hip hold one kernel family each with its
// launch functions (train_mlp_kernels.h); train_mlp_fp.hip / train_mlp_xyz.hip / train_mlp_frozen.hip the entry points, argument
// checks and kernels of one node type each (train_mlp_ragged.hip: the plain rows of a ragged batch, and the masked GEMM and
// weight-gradient kernels). A kernel that takes a row mask stands beside its dense twin, and the launch function of the pair
// chooses between them. Every extern "C" entry checks its arguments, fills a TlCall and hands it to tl_train_forward /
// tl_train_backward.
#pragma once
#include "pn2_device.h"

#include <string.h>

namespace pn2 {

// group dims as the C ABI passes them to the workspace queries: b, n, m, nsample, cfeat, has_idx
struct GroupDims { int b, n, m, nsample, cfeat, has_idx; };
inline GroupDims group_dims_of(const int *d) { return {d[0], d[1], d[2], d[3], d[4], d[5]}; }

// An FP level whose layer 1 runs once per KNOWN point (pn2_mlp_train_*_fp; its kernels and entry points: train_mlp_fp.hip)
struct FpL1 {
    int b, n, m, c2, c1;
    int c2p, c1p;                    // the widths rounded up to a multiple of 4 (the GEMMs read rows 16 bytes at a time)
    long long rows, bm, mp;          // b n unknown points; b m known points, and that rounded up to a multiple of 32
    const float *points2, *points1;
    const int *idx;
    const void *idx_plan;            // pn2_three_interpolate_plan of idx, or NULL: backward inverts idx itself
    const float *dist;
    float *weight_out;               // forward: the interpolation weights (b,n,3)
    const float *weight;             // backward: the same
    float *grad_points2, *grad_points1;
    bool pad2() const { return mp != bm || c2p != c2; }     // points2 enters as a zero-padded copy (mp, c2p)
    bool pad1() const { return c1 > 0 && c1p != c1; }       // points1 as a zero-padded copy (rows, c1p)
    bool gstage2() const { return mp != bm; }               // grad_points2 is written to the workspace (mp rows), then copied
};

inline FpL1 fp_l1(const pn2_fp_src *s)
{
    FpL1 f;
    memset(&f, 0, sizeof(f));
    f.b = s->b; f.n = s->n; f.m = s->m; f.c2 = s->c2; f.c1 = s->c1;
    f.c2p = (s->c2 + 3) / 4 * 4; f.c1p = (s->c1 + 3) / 4 * 4;
    f.rows = (long long)s->b * s->n; f.bm = (long long)s->b * s->m; f.mp = (f.bm + 31) / 32 * 32;
    f.points2 = s->points2; f.points1 = s->points1; f.idx = s->idx; f.idx_plan = s->idx_plan; f.dist = s->dist;
    return f;
}

// One call of the training node, either direction. An entry value-initialises it (TlCall c{}) and names what it has.
struct TlCall {
    long long rows;
    int nlayers;
    const pn2_bn_layer *layers;
    // the input: a grouped level, plain rows x (rows, cin_1), or an FP level with layer 1 per known point
    const pn2_group_src *group;
    const float *x;
    bool has_fp;
    FpL1 fp;
    int pool_rows;
    int pooling;                     // 0 max, 1 avg, 2 weighted_avg, 3 max_and_avg (the pn2_mlp_train_*_pool entries check it)
    // Normalisation with the RUNNING statistics (train_mlp_frozen.hip): no reduction over the rows stands between two layers
    // in either direction. Forward's (m', invstd, a, c) and backward's (a, 0, 0) of EVERY layer come from one launch each
    // before the first pass, the per-channel sums of backward feed only grad_gamma / grad_beta / grad_bias (one launch for
    // all layers behind the last pass), and a layer that wants no parameter gradient runs no weight-gradient pass at all.
    bool frozen;
    // Plain rows of a RAGGED batch (train_mlp_ragged.hip), or an FP level whose unknown side is ragged (has_fp; rg_b = fp.b,
    // rg_n = fp.n; train_mlp_fp.hip): row c n + i is valid iff i < clamp(lengths[c], 1, n). `mask` is the
    // caller's buffer (the valid-row count, one validity word per 32 rows): forward writes it from `lengths` before its first
    // pass, backward reads it. nullptr: every row is valid.
    // The GROUPED rows of a ragged batch (`group` with a mask; train_mlp_ragged_group.hip): rg_n = m nsample rows per cloud of
    // which the first rg_unit * clamp(lengths[c], 1, rg_cap) are valid -- whole groups (rg_unit = nsample, rg_cap = m: lengths
    // counts centroids), or the points of a group_all level (rg_unit = 1, rg_cap = n). rg_unit = 0: plain rows.
    void *mask;
    const int *lengths;              // forward only
    int rg_b, rg_n;
    int rg_unit, rg_cap;
    // forward writes these, backward reads them. Whichever of argsel / zsel / pool_w the pooling mode does not use is
    // ignored, whatever the caller passed (tl_pool_buffers)
    const float *out;
    const int *argsel;
    const float *zsel, *pool_w;
    // backward only
    const float *grad_out;
    float *grad_x, *grad_feat_rows, *grad_points;
    float *grad_xyz, *grad_new_xyz;  // the coordinate gradients (train_mlp_xyz.hip), or NULL
    float *const *grad_bias;         // frozen: per layer (cout) or NULL -- the conv bias takes a gradient there (a sum dy)
    int reproducible;
    void *ws;
    const pn2_train_opts *opts;
    void *stream;
};

// The organisation overrides of a call (include/pn2ops.h: pn2_train_opts; NULL = every rule automatic). They travel as an
// argument through every rule and launch: the library reads no environment variable and keeps no mode.
typedef pn2_train_opts Opts;

// ---- launch shapes: made by the size rules of train_mlp.hip (gemm_shape, wgrad_shape, fuse_shape, top_s_shape), read by its
// plan and by the launch functions of the kernel families ----
struct GemmShape { int K, N, tk, tn, ns, slabs, resident; size_t lds, pack_bytes; };
struct WgradShape { int tus, tts, uslabs, tslabs, tpw, upw, two; long long gridx, nw, nchunks; size_t e, lds, lds_dy, partial_bytes; };
// the layer's data gradient inside its weight-gradient pass (tl_wgrad_kernel<.., DY>; ok = false: two passes)
struct FuseShape { bool ok; int tk, nt, single, acopy, upw; size_t lds, xr_off, pack_bytes; };
// launch shape of tl_top_s_kernel (ok = false: the dense kernel takes the routed gradient as operand tiles)
struct TopSShape { bool ok; int GB, KC, NLD, ld, gridx, gridy, nchunks; size_t lds, part_bytes, part2_bytes; };

// ---- train_mlp.hip: the passes (arguments checked by the entries first) and the workspace queries that need the plan ----
int tl_train_forward(const TlCall &call);
int tl_train_backward(const TlCall &call);
int tl_pool_args(int pool_rows, int pooling, bool grouped);     // 0, or the PN2_E_* code of a bad (pool_rows, pooling)
long long tl_xyz_ws_bytes(long long rows, int nlayers, const int *widths, int pool_rows, int pooling, const int *group_dims,
                          const pn2_train_opts *opts);
long long tl_fp_ws_bytes(const pn2_fp_src *s, int nlayers, const int *widths, int backward, const pn2_train_opts *opts,
                         bool ragged = false);
long long tl_ragged_ws_bytes(long long rows, int nlayers, const int *widths, int backward, const pn2_train_opts *opts);
// the grouped rows of a ragged batch (pn2_mlp_train_*_group_ragged, train_mlp_ragged_group.hip), under ragged_group_opts
bool tl_group_ragged_supported(long long rows, int nlayers, const int *widths, int pool_rows, const int *group_dims);
long long tl_group_ragged_ws_bytes(long long rows, int nlayers, const int *widths, int pool_rows, int backward, const int *group_dims,
                                   const pn2_train_opts *opts);
int tl_group_ragged_plan(long long rows, int nlayers, const int *widths, const int *group_dims, const pn2_train_opts *opts, int *passes,
                         int cap);

// ---- train_mlp_fp.hip ----
int fp_launch_pad(const float *src, long long rows_in, int c, long long rows_out, int cp, float *dst, hipStream_t st);
// (mask: the validity words of a ragged unknown side, or nullptr: every row is valid)
int fp_launch_l1_forward(long long rows, int n, int m, int C, const int *idx, const float *dist, float *weight, const float *Q,
                         float *z, bool add, const unsigned *mask, double *stats, int max_parts, hipStream_t st, int *nparts);
int fp_launch_l1_dz(long long rows, int C, const float *z, float *g, const float *coef, const unsigned *mask, hipStream_t st);

// ---- train_mlp_xyz.hip: the coordinate gradients (pn2_mlp_train_backward_xyz) ----
int xyz_launch_rows(long long rows, int C, const float *G, const float *Z, const float *coef, const int *argsel, int group_rows,
                    const float *wx, long long sk, long long sn, float *out, hipStream_t st);
int xyz_launch_centroids(long long groups, int ns, const float *g, float *out, hipStream_t st);

// ---- train_mlp_frozen.hip: one launch for all layers each ----
struct FrozenSums { const double *stats; int nparts; bool skip; };     // a layer's partial rows (sum dy, sum dy z); skip: wants nothing
int frozen_launch_save(int nlayers, const pn2_bn_layer *layers, hipStream_t st);
int frozen_launch_coef(int nlayers, const pn2_bn_layer *layers, float *const *coef, hipStream_t st);
int frozen_launch_grads(int nlayers, const pn2_bn_layer *layers, const FrozenSums *sums, float *const *grad_bias, hipStream_t st);

}  // namespace pn2
