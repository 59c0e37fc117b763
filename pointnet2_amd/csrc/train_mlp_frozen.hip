// train_mlp_frozen.hip -- the training node with FROZEN batch-norm statistics (pn2_mlp_train_*_frozen): the entry points,
// their argument checks and the three per-channel kernels only this mode needs. The passes themselves are train_mlp.hip's
// (tl_train_forward / tl_train_backward with TlCall::frozen). gfx950.
//
// A batch norm in eval() normalises with its running statistics (torch.nn.BatchNorm, training = False): gradients through a
// model in eval() (saliency, adversarial points, test-time optimisation) and fine-tuning with frozen batch norms. Per layer,
// with the stored pre-norm tensor z = h W (without the conv bias, as in the batch-statistics node):
//     invstd = 1 / sqrt(running_var + eps)      a = gamma invstd      m' = running_mean - bias      c = beta - a m'
//     y  = relu(a z + c)                        dz = a dy             (no mean / variance correction: s, c0, c1 = a, 0, 0)
//     dbeta = sum dy     dgamma = (sum dy z - m' dbeta) invstd        dbias = a dbeta   (NOT zero: the bias no longer cancels)
// No statistic over the rows stands between two layers, so:
//     forward   tl_frozen_save_kernel fills every layer's save (m', invstd, a, c) in ONE launch; the layer GEMMs sum no moments
//               (no partial rows, no tl_bn_finalize_kernel, no ticket); the pool / apply / average epilogues are the node's own
//     backward  tl_frozen_coef_kernel writes (a, 0, 0) of every layer in ONE launch before the first pass; the sums (sum dy,
//               sum dy z) remain as inputs of the three per-channel gradients and are turned into them by ONE launch behind the
//               last pass (tl_frozen_grads_kernel); a layer whose gradient slots are all NULL runs no weight-gradient pass and
//               sums nothing, and the chain stops at the lowest layer that still needs something
// Running statistics are read, never written.
#include "train_mlp_internal.h"

#include <limits.h>

namespace pn2 {

constexpr int kFrozenMaxLayers = 8;

struct FrozenSaveJob { int C; float eps; const float *gamma, *beta, *bias, *mean, *var; float *save; };
struct FrozenSaveJobs { FrozenSaveJob l[kFrozenMaxLayers]; };

// blockIdx.y = layer, one thread per channel: save = (m', invstd, a, c)
__global__ __launch_bounds__(256) void tl_frozen_save_kernel(const FrozenSaveJobs jobs)
{
    const FrozenSaveJob &j = jobs.l[blockIdx.y];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= j.C) return;
    const double invstd = 1.0 / sqrt((double)j.var[c] + (double)j.eps);
    const double a = (double)j.gamma[c] * invstd;
    const double m = (double)j.mean[c] - (j.bias ? (double)j.bias[c] : 0.0);
    j.save[c] = (float)m;
    j.save[j.C + c] = (float)invstd;
    j.save[2 * j.C + c] = (float)a;
    j.save[3 * j.C + c] = (float)((double)j.beta[c] - a * m);
}

struct FrozenCoefJob { int C; const float *save; float *coef; };
struct FrozenCoefJobs { FrozenCoefJob l[kFrozenMaxLayers]; };

// blockIdx.y = layer: the coefficients of dz = s dy - c0 - c1 z are (a, 0, 0)
__global__ __launch_bounds__(256) void tl_frozen_coef_kernel(const FrozenCoefJobs jobs)
{
    const FrozenCoefJob &j = jobs.l[blockIdx.y];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= j.C) return;
    j.coef[c] = j.save[2 * j.C + c];
    j.coef[j.C + c] = 0.0f;
    j.coef[2 * j.C + c] = 0.0f;
}

struct FrozenGradJob {
    int C, nparts, accumulate;
    const double *stats;        // (nparts, 2, C) partial rows: sum dy, sum dy z; nullptr: the layer wants nothing
    const float *save;
    float *grad_gamma, *grad_beta, *grad_bias;
};
struct FrozenGradJobs { FrozenGradJob l[kFrozenMaxLayers]; };

// blockIdx.y = layer; a block of 256 threads owns 8 channels and adds the partial rows 32 at a time, in a fixed order
// (as tl_bn_backward_finalize_kernel): the same bits every run
__global__ __launch_bounds__(256) void tl_frozen_grads_kernel(const FrozenGradJobs jobs)
{
    const FrozenGradJob &j = jobs.l[blockIdx.y];
    if (!j.stats || blockIdx.x * 8 >= j.C) return;                 // (uniform per block)
    __shared__ double sh[2][32][8];
    const int g = threadIdx.x >> 3, cl = threadIdx.x & 7, c = blockIdx.x * 8 + cl;
    double a = 0.0, b = 0.0;
    if (c < j.C)
        for (int q = g; q < j.nparts; q += 32) { a += j.stats[((size_t)q * 2) * j.C + c]; b += j.stats[((size_t)q * 2 + 1) * j.C + c]; }
    sh[0][g][cl] = a;
    sh[1][g][cl] = b;
    __syncthreads();
    if (g != 0 || c >= j.C) return;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 32; ++i) { s1 += sh[0][i][cl]; s2 += sh[1][i][cl]; }
    const double m = j.save[c], invstd = j.save[j.C + c], sc = j.save[2 * j.C + c];
    const float dbeta = (float)s1, dgamma = (float)((s2 - m * s1) * invstd), dbias = (float)(sc * s1);
    if (j.grad_gamma) j.grad_gamma[c] = j.accumulate ? __fadd_rn(j.grad_gamma[c], dgamma) : dgamma;
    if (j.grad_beta) j.grad_beta[c] = j.accumulate ? __fadd_rn(j.grad_beta[c], dbeta) : dbeta;
    if (j.grad_bias) j.grad_bias[c] = j.accumulate ? __fadd_rn(j.grad_bias[c], dbias) : dbias;
}

// ---- called by tl_train_forward / tl_train_backward (train_mlp.hip) ----
int frozen_launch_save(int nlayers, const pn2_bn_layer *layers, hipStream_t st)
{
    FrozenSaveJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    int cmax = 0;
    for (int l = 0; l < nlayers; ++l) {
        const pn2_bn_layer &L = layers[l];
        if (!L.running_mean || !L.running_var) return PN2_E_NULL;
        jobs.l[l] = {L.cout, L.eps, L.gamma, L.beta, L.bias, L.running_mean, L.running_var, L.save};
        if (L.cout > cmax) cmax = L.cout;
    }
    return launch(tl_frozen_save_kernel, dim3((unsigned)((cmax + 255) / 256), (unsigned)nlayers), dim3(256), 0, st, jobs);
}

int frozen_launch_coef(int nlayers, const pn2_bn_layer *layers, float *const *coef, hipStream_t st)
{
    FrozenCoefJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    int cmax = 0;
    for (int l = 0; l < nlayers; ++l) {
        jobs.l[l] = {layers[l].cout, layers[l].save, coef[l]};
        if (layers[l].cout > cmax) cmax = layers[l].cout;
    }
    return launch(tl_frozen_coef_kernel, dim3((unsigned)((cmax + 255) / 256), (unsigned)nlayers), dim3(256), 0, st, jobs);
}

int frozen_launch_grads(int nlayers, const pn2_bn_layer *layers, const FrozenSums *sums, float *const *grad_bias, hipStream_t st)
{
    FrozenGradJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    int cmax = 0;
    for (int l = 0; l < nlayers; ++l) {
        const pn2_bn_layer &L = layers[l];
        if (sums[l].skip) continue;                                // (stats stays nullptr: the layer's blocks return at once)
        jobs.l[l] = {L.cout, sums[l].nparts, L.grad_accumulate, sums[l].stats, L.save, L.grad_gamma, L.grad_beta,
                     grad_bias ? grad_bias[l] : nullptr};
        if (L.cout > cmax) cmax = L.cout;
    }
    if (cmax == 0) return PN2_OK;
    return launch(tl_frozen_grads_kernel, dim3((unsigned)((cmax + 7) / 8), (unsigned)nlayers), dim3(256), 0, st, jobs);
}

// 0 ok, else the PN2_E_* code the entries return before anything is launched
static int frozen_args(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group, const float *x,
                       int pool_rows, int pooling)
{
    if (pooling < 0 || pooling > 3 || rows <= 0 || rows % 32 || nlayers < 1 || nlayers > kFrozenMaxLayers) return PN2_E_ARG;
    if (!layers || (!group && !x)) return PN2_E_NULL;
    if (group && x) return PN2_E_ARG;
    if (pooling != 0 && !group) return PN2_E_NULL;
    if (group ? pool_rows <= 0 : pool_rows != 0) return PN2_E_ARG;
    for (int l = 0; l < nlayers; ++l)
        if (!layers[l].running_mean || !layers[l].running_var) return PN2_E_NULL;
    return PN2_OK;
}

static TlCall frozen_call(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group, const float *x,
                          int pool_rows, int pooling, const float *out, const int *argsel, const float *zsel, const float *pool_w,
                          void *ws, const pn2_train_opts *opts, void *stream)
{
    TlCall c{};
    c.rows = rows; c.nlayers = nlayers; c.layers = layers;
    c.group = group; c.x = x;
    c.pool_rows = pool_rows; c.pooling = pooling;
    c.frozen = true;
    c.out = out; c.argsel = argsel; c.zsel = zsel; c.pool_w = pool_w;
    c.ws = ws; c.opts = opts; c.stream = stream;
    return c;
}

}  // namespace pn2

extern "C" int pn2_mlp_train_frozen_supported(long long rows, int nlayers, const int *widths, int pool_rows, int pooling,
                                              const int *group_dims, int want_xyz)
{
    if (!widths || rows <= 0 || rows % 32) return 0;
    if (want_xyz) return pn2_mlp_train_xyz_supported(rows, nlayers, widths, pool_rows, pooling, group_dims);
    return pn2_mlp_train_pool_supported(rows, nlayers, widths, pool_rows, pooling);
}

extern "C" long long pn2_mlp_train_ws_bytes_frozen(long long rows, int nlayers, const int *widths, int pool_rows, int pooling,
                                                   int backward, const int *group_dims, int want_xyz, const pn2_train_opts *opts)
{
    if (!widths || pooling < 0 || pooling > 3) return -1;
    if (backward && want_xyz) return pn2_mlp_train_ws_bytes_xyz(rows, nlayers, widths, pool_rows, pooling, group_dims, opts);
    return pn2_mlp_train_ws_bytes_pool(rows, nlayers, widths, pool_rows, pooling, backward, group_dims, opts);
}

extern "C" int pn2_mlp_train_forward_frozen(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                            const float *x, int pool_rows, int pooling, float *out, int *argsel, float *zsel,
                                            float *pool_w, void *ws, const pn2_train_opts *opts, void *stream)
{
    if (int rc = pn2::frozen_args(rows, nlayers, layers, group, x, pool_rows, pooling)) return rc;
    return pn2::tl_train_forward(pn2::frozen_call(rows, nlayers, layers, group, x, pool_rows, pooling, out, argsel, zsel, pool_w, ws,
                                                  opts, stream));
}

extern "C" int pn2_mlp_train_backward_frozen(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                             const float *x, int pool_rows, int pooling, const float *out, const int *argsel,
                                             const float *zsel, const float *pool_w, const float *grad_out, float *grad_x,
                                             float *grad_feat_rows, float *grad_points, float *grad_xyz, float *grad_new_xyz,
                                             float *const *grad_bias, int reproducible, void *ws, const pn2_train_opts *opts,
                                             void *stream)
{
    if (int rc = pn2::frozen_args(rows, nlayers, layers, group, x, pool_rows, pooling)) return rc;
    if (grad_xyz || grad_new_xyz) {                                  // the checks of pn2_mlp_train_backward_xyz
        if (pooling == 2) return PN2_E_ARG;                          // weighted_avg: its weights depend on xyz
        if (!group || !grad_xyz) return PN2_E_NULL;
        if (group->new_xyz && !grad_new_xyz) return PN2_E_NULL;
        if (!group->new_xyz && grad_new_xyz) return PN2_E_ARG;
        if (group->m <= 0 || group->nsample <= 0 || (long long)group->m * group->nsample > INT_MAX ||
            (long long)group->b * group->n > INT_MAX) return PN2_E_ARG;
    }
    pn2::TlCall c = pn2::frozen_call(rows, nlayers, layers, group, x, pool_rows, pooling, out, argsel, zsel, pool_w, ws, opts, stream);
    c.grad_out = grad_out;
    c.grad_x = grad_x; c.grad_feat_rows = grad_feat_rows; c.grad_points = grad_points;
    c.grad_xyz = grad_xyz; c.grad_new_xyz = grad_new_xyz;
    c.grad_bias = grad_bias;
    c.reproducible = reproducible;
    return pn2::tl_train_backward(c);
}
