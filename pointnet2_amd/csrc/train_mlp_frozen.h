// train_mlp_frozen.h -- what train_mlp.hip and train_mlp_frozen.hip share for the frozen-statistics training node.
#pragma once
#include "pn2_device.h"

namespace pn2 {
// Normalisation with the RUNNING statistics: no reduction over the rows stands between two layers in either direction.
// Forward's (m', invstd, a, c) and backward's (a, 0, 0) of EVERY layer come from one launch each before the first pass, the
// per-channel sums of backward feed only grad_gamma / grad_beta / grad_bias (one launch for all layers behind the last
// pass), and a layer that wants no parameter gradient runs no weight-gradient pass at all.
struct TlFrozen {
    float *const *grad_bias;    // backward: per layer (cout) or NULL -- the conv bias takes a gradient here (a sum dy)
};
struct FrozenSums { const double *stats; int nparts; bool skip; };     // a layer's partial rows (sum dy, sum dy z); skip: wants nothing

// ---- train_mlp_frozen.hip: one launch for all layers each ----
int frozen_launch_save(int nlayers, const pn2_bn_layer *layers, hipStream_t st);
int frozen_launch_coef(int nlayers, const pn2_bn_layer *layers, float *const *coef, hipStream_t st);
int frozen_launch_grads(int nlayers, const pn2_bn_layer *layers, const FrozenSums *sums, float *const *grad_bias, hipStream_t st);

// ---- train_mlp.hip: the passes (arguments checked by the entries in train_mlp_frozen.hip) ----
int tl_frozen_forward(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group, const float *x,
                      int pool_rows, int pooling, float *out, int *argsel, float *zsel, float *pool_w, void *ws,
                      const pn2_train_opts *opts, void *stream);
int tl_frozen_backward(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group, const float *x,
                       int pool_rows, int pooling, const float *out, const int *argsel, const float *zsel, const float *pool_w,
                       const float *grad_out, float *grad_x, float *grad_feat_rows, float *grad_points, float *grad_xyz,
                       float *grad_new_xyz, float *const *grad_bias, int reproducible, void *ws, const pn2_train_opts *opts,
                       void *stream);
}  // namespace pn2
