/*
 * pn2ops.h -- C ABI of libpn2ops.so: the PointNet++ set-abstraction /
 * feature-propagation operator kernels, hand-written for AMD MI355X (gfx950).
 *
 * Drop-in seam. The reference's TensorFlow op classes call free C++
 * "Launcher" functions that are declared in the op .cpp and defined in the
 * .cu. Every entry point below replaces exactly one
 * of them and keeps its argument list (same order, same meaning, same
 * row-major fp32/int32 layouts), plus
 *     - a trailing `void *stream` (a hipStream_t; NULL = the null stream), and
 *     - an `int` return: 0 ok, <0 invalid argument (PN2_E_*), >0 a hipError_t
 *       raised by the launch (the reference launchers return void and never
 *       check; validation lived in OpKernel::Compute as OP_REQUIRES).
 *
 * Ownership: the caller allocates every buffer (inputs, outputs, scratch);
 * the library holds no state and no memory, never synchronises, and only
 * enqueues work on `stream`. All pointers are DEVICE pointers. Entry points
 * are re-entrant and thread-safe.
 *
 * Gradient entry points ZERO their output themselves (the reference made the
 * caller do it: cudaMemset in tf_sampling.cpp:174, tf_grouping.cpp:204,
 * memset in tf_interpolate.cpp:258) -- a documented, deliberate difference:
 * the zero-fill is enqueued on the same stream right before the scatter.
 */
#ifndef PN2OPS_H
#define PN2OPS_H

#ifdef __cplusplus
extern "C" {
#endif

#define PN2_OK 0
#define PN2_E_NULL (-1)     /* a required pointer is NULL */
#define PN2_E_SHAPE (-2)    /* negative / zero extent where the reference requires positive */
#define PN2_E_ARG (-3)      /* attribute out of range (radius<=0, nsample<=0, npoint<=0, k<=0 ...) */
#define PN2_E_TOO_LARGE (-4)/* extent beyond what the kernels index with int32 */

/* library identification: returns "pn2ops <version> gfx950" */
const char *pn2_version(void);

/* ---- tf_ops/sampling ------------------------------------------------- */

/* replaces farthestpointsamplingLauncher(int b,int n,int m,const float*inp,float*temp,int*out)
 *   declared tf_ops/sampling/tf_sampling.cpp:94, defined tf_sampling_g.cu:203-205.
 * inp (b,n,3) f32 -> out (b,m) i32.  temp: scratch of pn2_fps_temp_floats(b,n)
 * floats (the reference allocates 32*n, tf_sampling.cpp:115); may be NULL when
 * pn2_fps_temp_floats(b,n)==0 (the register-resident tiers need no scratch).
 * Selection order and tie rule are the reference kernel's (ties -> smallest
 * (k mod 512, k)). m<=0 is a no-op like tf_sampling_g.cu:106. */
int pn2_farthest_point_sample(int b, int n, int m, const float *inp, float *temp, int *out, void *stream);
long long pn2_fps_temp_floats(int b, int n);

/* replaces gatherpointLauncher(b,n,m,inp,idx,out)  tf_sampling.cpp:125, tf_sampling_g.cu:206-208
 * inp (b,n,3), idx (b,m) -> out (b,m,3) */
int pn2_gather_point(int b, int n, int m, const float *inp, const int *idx, float *out, void *stream);

/* replaces scatteraddpointLauncher(b,n,m,out_g,idx,inp_g)  tf_sampling.cpp:150, tf_sampling_g.cu:209-211
 * out_g (b,m,3), idx (b,m) -> inp_g (b,n,3), zero-filled here then accumulated */
int pn2_gather_point_grad(int b, int n, int m, const float *out_g, const int *idx, float *inp_g, void *stream);

/* replaces probsampleLauncher(b,n,m,inp_p,inp_r,temp,out)  tf_sampling.cpp:65, tf_sampling_g.cu:198-201
 * inp_p (b,n) weights, inp_r (b,m) uniforms in [0,1) -> out (b,m); temp: b*n floats */
int pn2_prob_sample(int b, int n, int m, const float *inp_p, const float *inp_r, float *temp, int *out, void *stream);

/* ---- tf_ops/grouping -------------------------------------------------- */

/* replaces queryBallPointLauncher(b,n,m,radius,nsample,xyz1,xyz2,idx,pts_cnt)
 *   tf_ops/grouping/tf_grouping.cpp:66, tf_grouping_g.cu:125-128 (CPU twin test/query_ball_point.cpp:19-47)
 * xyz1 (b,n,3) dataset, xyz2 (b,m,3) queries -> idx (b,m,nsample), pts_cnt (b,m).
 * Rows with no point in the ball are written as zeros (the reference leaves them
 * uninitialised; its harness pre-zeroes, query_ball_point.cpp:94). */
int pn2_query_ball_point(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                         int *idx, int *pts_cnt, void *stream);

/* replaces selectionSortLauncher(b,n,m,k,dist,outi,out)  tf_grouping.cpp:108, tf_grouping_g.cu:129-132
 * dist (b,m,n) -> outi (b,m,n) i32, out (b,m,n) f32; the first k of each row are the k smallest, ascending.
 * NaN of either sign follows the reference's `<` comparisons at every row length: one in the unsorted tail is never
 * selected, and a round whose own slot holds one swaps nothing (it stays there). */
int pn2_selection_sort(int b, int n, int m, int k, const float *dist, int *outi, float *out, void *stream);

/* knn_point (tf_grouping.py:48-73) in one kernel, without the (b,m,n) distance/index tensors: the distance
 * row ((dx*dx)+(dy*dy))+(dz*dz) of a query is built in LDS, the same k swap rounds as selectionSortLauncher
 * run on it, and only the first k (value, index) pairs are written -- identical to slicing the reference's
 * outputs, ties included. Rows with NaN distances are outside that claim: a NaN sorts last here, where the reference's
 * rounds leave one found at a slot below k in place. xyz1 (b,n,3), xyz2 (b,m,3) -> val (b,m,k) f32, idx (b,m,k) i32.
 * PN2_E_TOO_LARGE for n > 14336 or k > n (callers keep the matrix + pn2_selection_sort path). */
int pn2_knn_point(int b, int n, int m, int k, const float *xyz1, const float *xyz2, float *val, int *idx,
                  void *stream);

/* replaces groupPointLauncher(b,n,c,m,nsample,points,idx,out)  tf_grouping.cpp:142, tf_grouping_g.cu:133-136
 * points (b,n,c), idx (b,m,nsample) -> out (b,m,nsample,c) */
int pn2_group_point(int b, int n, int c, int m, int nsample, const float *points, const int *idx, float *out,
                    void *stream);

/* replaces groupPointGradLauncher(b,n,c,m,nsample,grad_out,idx,grad_points)  tf_grouping.cpp:173, tf_grouping_g.cu:137-141
 * grad_out (b,m,nsample,c), idx -> grad_points (b,n,c), zero-filled here then accumulated */
int pn2_group_point_grad(int b, int n, int c, int m, int nsample, const float *grad_out, const int *idx,
                         float *grad_points, void *stream);

/* ---- tf_ops/3d_interpolation ------------------------------------------ */

/* replaces threenn_cpu(b,n,m,xyz1,xyz2,dist,idx)  tf_ops/3d_interpolation/tf_interpolate.cpp:60-103
 * xyz1 (b,n,3) unknown, xyz2 (b,m,3) known -> dist (b,n,3) SQUARED distances ascending, idx (b,n,3) */
int pn2_three_nn(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist, int *idx, void *stream);

/* replaces threeinterpolate_cpu(b,m,c,n,points,idx,weight,out)  tf_interpolate.cpp:107-127
 * points (b,m,c), idx/weight (b,n,3) -> out (b,n,c) */
int pn2_three_interpolate(int b, int m, int c, int n, const float *points, const int *idx, const float *weight,
                          float *out, void *stream);

/* replaces threeinterpolate_grad_cpu(b,n,c,m,grad_out,idx,weight,grad_points)  tf_interpolate.cpp:131-153
 * grad_out (b,n,c), idx/weight (b,n,3) -> grad_points (b,m,c), zero-filled here then accumulated */
int pn2_three_interpolate_grad(int b, int n, int c, int m, const float *grad_out, const int *idx,
                               const float *weight, float *grad_points, void *stream);

/* ---- run-to-run reproducible gradients (no reference counterpart) -------------
 * Same contracts as pn2_gather_point_grad / pn2_group_point_grad / pn2_three_interpolate_grad above
 * (tf_sampling_g.cu:182-190, tf_grouping_g.cu:60-78, tf_interpolate.cpp:131-153), but the scatter-add
 * accumulates 64-bit fixed-point integers, so the result does not depend on the order in which the
 * atomics land: two calls on the same inputs return identical bits. `ws` is device scratch of
 * pn2_det_grad_ws_bytes(b, rows, c) bytes (rows = n for gather/group, m for three_interpolate; c = 3 for
 * gather); it needs no initialisation. Non-finite gradients fall back to the fp32-atomic accumulation. */
long long pn2_det_grad_ws_bytes(int b, int rows, int c);
int pn2_gather_point_grad_det(int b, int n, int m, const float *out_g, const int *idx, float *inp_g, void *ws,
                              void *stream);
int pn2_group_point_grad_det(int b, int n, int c, int m, int nsample, const float *grad_out, const int *idx,
                             float *grad_points, void *ws, void *stream);
int pn2_three_interpolate_grad_det(int b, int n, int c, int m, const float *grad_out, const int *idx,
                                   const float *weight, float *grad_points, void *ws, void *stream);

/* ---- the same gradients as a segmented reduction (no reference counterpart) ----------------------
 * idx is inverted first (counting sort by target row), then one lane group sums the grad_out rows of
 * every output row: no float atomics, no zero-fill, ~3x the throughput of the atomic scatter from 16
 * channels up. deterministic != 0: identical bits on every run. A target row is summed in fp32 in ascending entry order --
 * bit-identical to the reference's CPU loops -- when b >= 4, rows <= 24576, rows + entries <= 36864 (counters and list in
 * 144 KiB of LDS) and the row has at most 1024 entries; every other row is a 64-bit fixed-point sum with one scale per
 * element from the largest |addend| of the row (INTEGRATION.md C'').
 * ws: pn2_seg_grad_ws_bytes(b, rows, entries) bytes of uninitialised device scratch
 * (group_point: rows = n, entries = m * nsample; three_interpolate: rows = m, entries = 3 * n). */
long long pn2_seg_grad_ws_bytes(int b, int rows, long long entries);
/* Host logic, no device work (tests, maintainers): how the default mode of pn2_*_grad_seg lays out the long-row part of its
 * reduction for out_rows = b * rows target rows of c channels with `entries` references per cloud. long_from: rows with that
 * many references or more are summed by a whole workgroup each (twice the average row, between 32 and 64); long_blocks: the
 * number of such workgroups = the stride of the rows one of them looks at (rows w, w + long_blocks, ...): coprime with `rows`,
 * residue at its golden section, so that the low point numbers of every cloud -- where a ball query's padding piles the
 * references up, tf_grouping_g.cu:24-31 -- spread evenly over the workgroups. */
int pn2_seg_grad_plan(int rows, long long entries, int c, long long out_rows, int *long_from, int *long_blocks);
int pn2_group_point_grad_seg(int b, int n, int c, int m, int nsample, const float *grad_out, const int *idx,
                             float *grad_points, void *ws, int deterministic, void *stream);
int pn2_three_interpolate_grad_seg(int b, int n, int c, int m, const float *grad_out, const int *idx,
                                   const float *weight, float *grad_points, void *ws, int deterministic, void *stream);

/* ---- index plans: the inversion of an index tensor as a call of its own ----
 * The inversion above depends on idx alone -- not on the gradient, the channel count or the mode's arithmetic. A PLAN is the
 * inverse of one index tensor in caller-owned device memory of pn2_seg_plan_bytes(b, rows, entries) bytes (uninitialised; 4-byte
 * aligned; rows / entries as for pn2_seg_grad_ws_bytes). One build call writes it -- the same kernels, chosen by the same rules,
 * as inside pn2_*_grad_seg; kernels only, so the call can be captured --, and any number of pn2_*_grad_planned calls then READ it
 * and never write it: at any channel count, in both modes, from several streams at once (behind the build in stream order).
 *   sorted != 0 selects the sorting inversion wherever `deterministic` of pn2_*_grad_seg does. A plan built with sorted = 1
 *   serves both modes: deterministic = 1 on it returns the bits of pn2_*_grad_seg(deterministic = 1), deterministic = 0 the
 *   default mode's sums. deterministic = 1 on a plan built with sorted = 0 is still identical from run to run, but sums EVERY
 *   row in fixed point (all its sorted flags are 0).
 *   A plan is valid for exactly the idx contents it was built from; keeping the two together is the caller's contract, as with
 *   every pointer pair of this ABI.
 * Beside the workspace layout of pn2_*_grad_seg a plan holds a TABLE of each cloud's long rows (long_count[b], long_rows[b][cap],
 * cap = entries / 32 + 1; rows of at least long_from references, in no particular order), written by the build while it has the
 * counts. The table walk of the default mode's long-row part deals the table's entries to its workgroups round-robin, so it is
 * balanced wherever the long rows are (the walk of pn2_seg_grad_plan relies on them sitting at the low point numbers of every cloud).
 * pn2_seg_plan_layout (host only; tests, maintainers): byte offsets inside a plan of start int[b][rows + 1], sorted int[b][rows],
 * list int[b][entries], long_count, long_rows; the long-row threshold; the table's capacity per cloud.
 * The planned gradient calls take the arguments of pn2_*_grad_seg with `plan` in place of idx and ws. Argument errors return
 * PN2_E_* before anything is launched (a NULL plan: PN2_E_NULL), b == 0 returns PN2_OK, entries == 0 zero-fills grad_points
 * without reading the plan (building a plan of such a shape is a no-op). *_ex: variant of the default mode's long-row part,
 * 0 = the library's choice (today the stride walk: the faster one on ball-query lists), 1 = the stride walk of
 * pn2_*_grad_seg, 2 = the table walk (the one to ask for when the long rows are not at the low point numbers: kNN lists,
 * lists of the caller's own; more than 2048 clouds take the stride walk all the same); other values PN2_E_ARG. The variants
 * return identical bits. */
long long pn2_seg_plan_bytes(int b, int rows, long long entries);
int pn2_seg_plan_layout(int b, int rows, long long entries, long long *offsets5, int *long_from, long long *long_cap);
int pn2_group_point_plan(int b, int n, int m, int nsample, const int *idx, int sorted, void *plan, void *stream);
int pn2_three_interpolate_plan(int b, int n, int m, const int *idx, int sorted, void *plan, void *stream);
int pn2_group_point_grad_planned(int b, int n, int c, int m, int nsample, const float *grad_out, const void *plan,
                                 float *grad_points, int deterministic, void *stream);
int pn2_three_interpolate_grad_planned(int b, int n, int c, int m, const float *grad_out, const void *plan,
                                       const float *weight, float *grad_points, int deterministic, void *stream);
int pn2_group_point_grad_planned_ex(int b, int n, int c, int m, int nsample, const float *grad_out, const void *plan,
                                    float *grad_points, int deterministic, int variant, void *stream);
int pn2_three_interpolate_grad_planned_ex(int b, int n, int c, int m, const float *grad_out, const void *plan,
                                          const float *weight, float *grad_points, int deterministic, int variant, void *stream);

/* ---- grouped local MLP + max-pool of a set-abstraction layer, fused, on the matrix cores ---------
 * (no reference kernel; replaces for INFERENCE the TF graph of utils/pointnet_util.py:44-50 + :117-127:
 *  group_point(xyz)-new_xyz ++ group_point(points) -> 3 x [conv2d 1x1 + batch_norm + ReLU] -> reduce_max
 *  over nsample). fp32 in, fp32 out, fp32 accuracy: every product is evaluated as six
 *  bf16 MFMA terms on three-level bf16 operands (error of an fp32 evaluation; csrc/sa_mlp.hip).
 *   xyz (b,n,3), new_xyz (b,m,3), points (b,n,cfeat) or NULL when cfeat == 0, idx (b,m,nsample) i32
 *   -> out (b,m,c3).  Input channel order is the reference's: [relative xyz (3), features (cfeat)].
 * Three kernels behind one entry: weights resident in LDS (3 + cfeat <= 32, widths within (64,96,128);
 * nsample 16 or a multiple of 32), streamed through LDS (up to 384 input channels, widths within
 * (128,128,256); nsample a multiple of 32), or the cooperative kernel for wide stacks -- (256,256,512) and the
 * group_all level's (256,512,1024), any number of input channels, any nsample (the tail of the group is
 * masked). idx == NULL together with new_xyz == NULL selects the group_all form (sample_and_group_all,
 * pointnet_util.py:59-84: m = 1, nsample = n, the group is the whole cloud, no centroid subtraction).
 * PN2_E_TOO_LARGE outside: callers keep the unfused path.
 * Weights: w_i (cin_i, cout_i) row-major = the reference's conv kernel [1,1,cin,cout] (tf_util.py:113-117)
 * with batch norm folded in by the caller; xyz_first says whether the rows of w1 are [xyz, features]
 * (pointnet_util.py:50) or [features, xyz] (:184, MSG). pn2_sa_mlp3_pack (host code) permutes them into the
 * order the kernel consumes and splits every weight into its three bf16 levels: wpacked / bpacked of the sizes
 * pn2_sa_mlp3_config reports in 4-byte words (info4 = {kind: 0 resident / 1 streamed / 2 cooperative, output
 * tiles of the three layers}; 6 bytes per padded weight), uploaded by the caller. */
int pn2_sa_mlp3_config(int cin, int c1, int c2, int c3, int nsample, int *info4, long long *w_floats,
                       long long *b_floats);
int pn2_sa_mlp3_pack(int cin, int c1, int c2, int c3, int nsample, int xyz_first, const float *w1, const float *bias1,
                     const float *w2, const float *bias2, const float *w3, const float *bias3, float *wpacked,
                     float *bpacked);
/* ws: scratch of pn2_sa_mlp3_ws_bytes(b, n, m, 3 + cfeat, c1, c2, c3, nsample) bytes (0 for the resident kernel and most
 * cooperative shapes: NULL is fine then). The streamed kernel evaluates the FEATURE part of layer 1 once per point into
 * it (W1^T [f_j, xyz_j - c] = W1f^T f_j + W1x^T (xyz_j - c): the first term does not depend on the centroid, and a point
 * belongs to nsample * m / n groups) and starts every sample from its point's row. Stacks whose last layer is wider than
 * 512 (the group_all level's 256-512-1024) keep the second layer's output there for the GEMM that runs the last layer. */
long long pn2_sa_mlp3_ws_bytes(int b, int n, int m, int cin, int c1, int c2, int c3, int nsample);
int pn2_sa_mlp3_maxpool(int b, int n, int m, int nsample, int cfeat, const float *xyz, const float *new_xyz,
                        const float *points, const int *idx, int c1, int c2, int c3, const float *wpacked,
                        const float *bpacked, float *out, void *ws, void *stream);
/* The same with the organisation of the resident kernel chosen by the caller: variant 0 = by the size rule, 1 = one 32-sample
 * item per wave (two waves per SIMD), 2 / 3 = two items per wave, half a layer apart (csrc/sa_mlp.hip: sa_mlp3_pair_kernel), one /
 * two waves per SIMD; nsample 32 or 16, at most 16 input channels and widths up to (64, 64, 128), else ignored. Results are
 * bit-identical. */
int pn2_sa_mlp3_maxpool_ex(int b, int n, int m, int nsample, int cfeat, const float *xyz, const float *new_xyz,
                           const float *points, const int *idx, int c1, int c2, int c3, const float *wpacked,
                           const float *bpacked, float *out, void *ws, int variant, void *stream);
/* The reference's other pooling modes behind the same stack (utils/pointnet_util.py:128-140): pooling 0 max
 * (= pn2_sa_mlp3_maxpool), 1 avg (tf.reduce_mean over the group), 2 weighted_avg (weights exp(-5 |grouped_xyz|) normalised
 * over the group, :132-138), 3 max_and_avg (out (b, m, 2 c3) = concat([avg, max]), :139-142). Same operands, same packed
 * weights, same scratch (pn2_sa_mlp3_ws_bytes). Modes 1-3 are served for the stacks the resident and the streamed kernel
 * cover (pn2_sa_mlp3_config kind 0 / 1: widths up to (128, 128, 256), nsample 16 or a multiple of 32);
 * pn2_sa_mlp3_pool_supported says 1 / 0, the cooperative kernel's shapes return PN2_E_TOO_LARGE and the caller evaluates
 * the level layer by layer. idx / new_xyz NULL (group_all) only with pooling 0. */
int pn2_sa_mlp3_pool_supported(int cin, int c1, int c2, int c3, int nsample, int pooling);
int pn2_sa_mlp3_pool(int b, int n, int m, int nsample, int cfeat, const float *xyz, const float *new_xyz,
                     const float *points, const int *idx, int c1, int c2, int c3, const float *wpacked,
                     const float *bpacked, int pooling, float *out, void *ws, void *stream);

/* ---- a feature-propagation layer behind three_nn, fused, on the matrix cores --------------------------
 * (no reference kernel; replaces for INFERENCE the TF graph of utils/pointnet_util.py:212-226: the
 *  inverse-distance weights, three_interpolate, concat([interpolated, points1]) and 2-3 x [conv2d 1x1 +
 *  batch_norm + ReLU]). fp32 in, fp32 out, fp32 accuracy (the arithmetic of pn2_sa_mlp3_maxpool).
 *   points2 (b,m,c2) known features, points1 (b,n,c1) skip features or NULL when c1 == 0,
 *   idx (b,n,3) i32 and dist (b,n,3) squared distances as pn2_three_nn writes them -> out (b,n,widths[nlayers-1]).
 * nlayers 2 or 3, widths <= 256 (padded to the instantiated tile shapes; PN2_E_TOO_LARGE outside: callers keep
 * the unfused path). w[i] (cin_i, cout_i) row-major with batch norm folded in by the caller, rows of w[0] in
 * the reference's concat order [interpolated, points1]; pn2_fp_mlp_pack (host code) permutes them into the
 * streams the kernels consume (sizes from pn2_fp_mlp_config; tiles4 = skip-link / layer tile counts).
 * The first layer is linear and so is the interpolation: W1^T [interp(points2), points1] = interp(points2 . W1a) +
 * W1b^T points1. Q = points2 . W1a is evaluated once per KNOWN point into `ws` (pn2_fp_mlp_ws_bytes bytes, caller's),
 * rows of Q are interpolated instead of rows of points2, and only the skip-link part of layer 1 is matrix work per
 * unknown point. */
int pn2_fp_mlp_config(int c2, int c1, int nlayers, const int *widths, int kind, int *tiles4, long long *w_floats,
                      long long *b_floats);
int pn2_fp_mlp_pack(int c2, int c1, int nlayers, const int *widths, int kind, const float *const *w,
                    const float *const *bias, float *wpacked, float *bpacked);
long long pn2_fp_mlp_ws_bytes(int b, int m, int c2, int c1, int nlayers, const int *widths, int kind);
int pn2_fp_mlp(int b, int n, int m, int c2, int c1, const float *points2, const float *points1, const int *idx,
               const float *dist, int nlayers, const int *widths, int kind, const float *wpacked, const float *bpacked,
               float *out, void *ws, void *stream);
/* kind selects the kernel (and with it the packed layout): 0 = one wave per 32 points, weights streamed
 * through LDS (many points: sem_seg FP4, 65536 points, 88 TFLOP/s); 1 = four waves share 32 points and split
 * each layer's output tiles (few points, wide layers: a 512-point level is otherwise 16 serial MFMA chains).
 * Same results either way; pack with the kind you launch with. */

/* ---- fused entry points (no reference counterpart) ---- */

/* farthest_point_sample + gather_point(inp, out) in one launch: what
 * pointnet_util.py:40 computes with two ops. out (b,m) i32 as pn2_farthest_point_sample,
 * out_xyz (b,m,3) f32 = inp[out] (bit-exact copies). temp as pn2_farthest_point_sample. */
int pn2_farthest_point_sample_gather(int b, int n, int m, const float *inp, float *temp, int *out, float *out_xyz,
                                     void *stream);

/* farthest_point_sample (+ gather_point when out_xyz is not NULL) for input the caller BELIEVES to be in farthest-point
 * order already -- the second and later levels of every network sample from the previous level's samples
 * (models/pointnet2_sem_seg.py:28-31, pointnet2_cls_ssg.py:27-29), whose first m points are, up to exact ties under the
 * renumbered tie rule (tf_sampling_g.cu:146,153-163) and clouds that ran out of distinct points, selected as 0, 1, ..., m-1.
 * The belief is CHECKED in parallel (n independent prefix-minimum rows, no dependent rounds) and the chain runs only for
 * the clouds where it fails: the result is pn2_farthest_point_sample's for any input. ws: pn2_fps_ordered_ws_bytes(b)
 * bytes, zeroed ONCE by the caller (every call leaves it zeroed). Outside 2 <= m <= min(n, 1024), n <= 2048 the call is
 * the plain operator (PN2_E_TOO_LARGE beyond 16384 points, where that one needs its temp buffer). */
long long pn2_fps_ordered_ws_bytes(int b);
int pn2_farthest_point_sample_ordered(int b, int n, int m, const float *inp, int *out, float *out_xyz, void *ws, void *stream);
/* test hook: the check alone. flags (b ints, zeroed by the caller) comes back 1 exactly for the clouds whose sampling is not
 * 0 .. m-1. PN2_E_ARG outside the short cut's envelope. */
int pn2_fps_ordered_check(int b, int n, int m, const float *inp, int *flags, void *stream);

/* query_ball_point + group_point(xyz1, idx) - centroid in one pass over the
 * LDS-resident cloud: what pointnet_util.py:44-46 computes with three ops.
 * grouped_xyz (b,m,nsample,3) = xyz1[idx] - xyz2[:, :, None] when subtract_centroid!=0,
 * else the plain group. idx / pts_cnt as pn2_query_ball_point (either may be NULL). */
int pn2_query_ball_group_xyz(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                             int subtract_centroid, int *idx, int *pts_cnt, float *grouped_xyz, void *stream);

/* pn2_query_ball_group_xyz with the kernel choice as PER-CALL arguments (no process state): kernel 0 =
 * automatic, 1 = sweep kernel, 2 = cell-list kernel whenever it fits, 3 = cell-list kernel with 512-thread
 * workgroups; cells_qpb = queries per workgroup of the cell-list kernel (0 = automatic). grouped_xyz may be
 * NULL (plain query_ball_point). Used by the parity tests to force every kernel at every shape and by
 * scripts/bq_probe.py; results are identical whatever the choice. */
int pn2_query_ball_group_xyz_ex(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                                int subtract_centroid, int *idx, int *pts_cnt, float *grouped_xyz, int kernel,
                                int cells_qpb, void *stream);

/* Multi-radius form for multi-scale grouping (pointnet_sa_module_msg, utils/pointnet_util.py:175-186: one
 * query_ball_point + group_point + centroid subtraction PER RADIUS over the same xyz / new_xyz): the cloud is
 * staged and binned ONCE per workgroup (cells sized for the bin radius, see the plan entry below) and queried once per radius.
 * radii / nsamples: HOST arrays of nscales (<= 4) entries; idx / pts_cnt / grouped_xyz: HOST arrays of nscales
 * DEVICE pointers, scale i shaped (b,m,nsamples[i]) / (b,m) / (b,m,nsamples[i],3); the arrays themselves or
 * single entries of pts_cnt and of one of idx / grouped_xyz may be NULL. Every output is bit-identical to
 * pn2_query_ball_group_xyz called per radius. PN2_E_TOO_LARGE -- before anything is launched -- for n > 8192 and
 * whenever no LDS geometry fits the combination (e.g. n = 8192 with nsample >= 127 on a later radius, n = 8000 with
 * nsample 256): call the single-radius operator per radius then, as the Python operator does. */
int pn2_query_ball_group_xyz_msg(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                                 const float *xyz1, const float *xyz2, int subtract_centroid, int *const *idx,
                                 int *const *pts_cnt, float *const *grouped_xyz, void *stream);

/* What pn2_query_ball_group_xyz_msg launches for these shapes: host only, no device, and the launcher takes its decision through
 * the same function. It describes pn2_query_ball_group_xyz_msg_ragged (below, "ragged batches") as well: that launch takes every
 * host decision from the padded n, so threads, LDS, use_cells, qpb, parts and lanes per query are the same; and
 * pn2_query_ball_group_xyz_msg_packed ("packed batches") with n = nmax, for the same reason. Returns the launcher's code for the shapes (PN2_E_ARG / PN2_E_SHAPE as there, with nothing written;
 * PN2_E_TOO_LARGE: no LDS geometry fits, info[0] = 0). info (PN2_BQ_MSG_PLAN_FIELDS ints, may be NULL):
 *   [0] threads per workgroup (0: nothing is launched -- b = 0, m = 0 or an error)   [1] LDS cap of the chosen geometry, bytes
 *   [2] dynamic LDS requested, bytes   [3] use_cells: 1 = the workgroups try to bin their cloud, 0 = staged and swept
 *   [4] qpb, queries per workgroup (a multiple of the workgroup's granule: may exceed m)   [5] parts, workgroups per cloud
 *   [6 + i] lanes per query (8, 16 or 32) of scale i's pass over the cell list, 0 from nscales on
 * bin_radius (may be NULL): the radius the cells are sized for -- the second smallest of three or more radii, else the smallest. */
#define PN2_BQ_MSG_PLAN_FIELDS 10
int pn2_query_ball_group_xyz_msg_plan(int b, int n, int m, int nscales, const float *radii, const int *nsamples, int *info,
                                      float *bin_radius);

/* pn2_three_nn with the kernel chosen by the caller (results never depend on it; tests force each, scripts time them):
 * 0 = the library's choice, 1 = the sweep of every known point (round 1), 2 = the cell list (round 6: the known points binned
 * once per workgroup, 3 x 3 x 3 cells visited per unknown point, an exactness test on the third-best distance and a sweep for
 * the points that fail it; PN2_E_ARG below 64 or above 8192 known points). */
int pn2_three_nn_ex(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist, int *idx, int variant, void *stream);
/* ---- ragged batches: per-cloud point counts (DESIGN.md "Ragged batches") ----------------------------------------------------
 * Layout: a padded tensor (b, n, 3) plus `lengths` (b) int32 in DEVICE memory, 1 <= lengths[c] <= n; cloud c is rows
 * 0 .. lengths[c]-1 of its slab. THE SLICE RULE: for every entry below the result for cloud c is bit- and index-identical to
 * the dense entry applied to that slice alone (b = 1, n = lengths[c]), FPS tie rule included (rank (k mod 512) Q_c + k / 512,
 * Q_c = ceil(lengths[c] / 512)). Rows at or beyond lengths[c] are never read: they may hold NaN, Inf or anything else.
 * The host never reads `lengths` (no synchronisation; stream-ordered and capturable like the dense twins); the kernels clamp
 * a length into 1..n for memory safety only -- validating is the caller's business (Python: pointnet2_amd.check_lengths).
 * A NULL lengths is PN2_E_NULL; the other argument checks and codes are the dense entries'.
 *
 * pn2_farthest_point_sample_ragged: one workgroup per cloud; the tier is chosen by the size rule of pn2_farthest_point_sample
 *   applied to the PADDED n and m (the PN2_FPS_AUTO case of pn2_farthest_point_sample_ragged_variant below: batched, pruned or
 *   register tier), template, threads and LDS from the padded n. Every tier obeys the slice rule, so the choice shows in time
 *   alone. PN2_E_TOO_LARGE for n > 16384. out_xyz (b,m,3) may be NULL. m > lengths[c] behaves as the dense operator with
 *   npoint > n.
 * pn2_query_ball_group_xyz_ragged: xyz1 ragged (lengths1), the queries xyz2 (b,m,3) dense; kernel / cells_qpb as
 *   pn2_query_ball_group_xyz_ex (a cloud below 64 points takes the sweep inside the cell-list kernel); grouped_xyz NULL =
 *   plain query_ball_point.
 * pn2_query_ball_group_xyz_msg_ragged: pn2_query_ball_group_xyz_msg with xyz1 ragged (lengths1), the queries xyz2 (b,m,3) dense:
 *   ONE launch, one staging / binning of each cloud's own lengths1[c] points for every radius. Per cloud and radius the outputs
 *   are pn2_query_ball_group_xyz_msg's on the slice, hence pn2_query_ball_group_xyz_ragged's called per radius, bit for bit;
 *   every output entry is written. Geometry, LDS, qpb and lanes per query come from the padded n
 *   (pn2_query_ball_group_xyz_msg_plan describes this launch too); on the device a cloud below 64 points is swept without
 *   binning, a larger one bins its own points and the give-up rules apply to its own grid. Codes as the dense entry
 *   (PN2_E_TOO_LARGE for n > 8192 or when no LDS geometry fits: call pn2_query_ball_group_xyz_ragged per radius then);
 *   b = 0 or m = 0 is PN2_OK before lengths1 is looked at.
 * pn2_knn_point_ragged: the envelope of pn2_knn_point (n <= 14336, k <= n); where k > lengths1[c] the entries from
 *   lengths1[c] on repeat entry 0 of their row (val and idx), so every row is fully written.
 * pn2_three_nn_ragged: the UNKNOWN side xyz1 is ragged, the known side xyz2 (b,m,3) dense; variant as pn2_three_nn_ex.
 *   Rows at or beyond lengths1[c] are written as idx (0,0,0), dist (0,0,0). */
int pn2_farthest_point_sample_ragged(int b, int n, int m, const float *inp, const int *lengths, int *out, float *out_xyz,
                                     void *stream);
int pn2_query_ball_group_xyz_ragged(int b, int n, int m, float radius, int nsample, const float *xyz1, const int *lengths1,
                                    const float *xyz2, int subtract_centroid, int *idx, int *pts_cnt, float *grouped_xyz,
                                    int kernel, int cells_qpb, void *stream);
int pn2_query_ball_group_xyz_msg_ragged(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                                        const float *xyz1, const int *lengths1, const float *xyz2, int subtract_centroid,
                                        int *const *idx, int *const *pts_cnt, float *const *grouped_xyz, void *stream);
int pn2_knn_point_ragged(int b, int n, int m, int k, const float *xyz1, const int *lengths1, const float *xyz2, float *val, int *idx,
                         void *stream);
int pn2_three_nn_ragged(int b, int n, int m, const float *xyz1, const int *lengths1, const float *xyz2, float *dist, int *idx,
                        int variant, void *stream);

/* ---- ragged batches, the second side: per-cloud sample counts and a ragged query / known side ---------------------------------
 * A second count array (b) int32 in DEVICE memory joins `lengths`: for FPS `npoints` -- cloud c yields m_c = npoints[c] samples --,
 * for the pair operators `lengths2` -- cloud c has m_c = lengths2[c] valid rows of xyz2 (b,m,3). Never read by the host, clamped
 * on the device into 1..m for memory safety only. THE PAIR SLICE RULE: for cloud c and rows j < m_c the result is bit- and
 * index-identical to the dense entry on (xyz1[c, :lengths1[c]], xyz2[c, :m_c]) alone; for FPS that is the first m_c samples of
 * the slice (the chain is prefix-consistent, sample 0 is point 0), and m_c > lengths[c] behaves as the dense operator with
 * npoint > n. Rows of xyz1 at or beyond lengths1[c] and rows of xyz2 at or beyond m_c are never read. Output rows j >= m_c are
 * fully written with fixed values:
 *   pn2_farthest_point_sample_ragged_counts     out[c, j] = out[c, 0] = 0, out_xyz[c, j] = out_xyz[c, 0] (sample 0 repeated)
 *   pn2_query_ball_group_xyz_ragged_pair        idx row all 0, pts_cnt 0, grouped_xyz all +0.0 (with or without subtract_centroid)
 *   pn2_query_ball_group_xyz_msg_ragged_pair    the same for every radius
 *   pn2_knn_point_ragged_pair                   idx row all 0, val row all +0.0
 *   pn2_three_nn_ragged_pair                    the ragged side is the KNOWN side: no new output rows; rows beyond lengths1[c]
 *                                               stay (0,0,0) / (0,0,0); m_c < 3 gives the dense operator's +inf / index 0 entries,
 *                                               and every index is below m_c
 * A workgroup or wave that holds such rows only writes them and leaves before any staging, binning or barrier. BOTH count
 * arrays are required (NULL: PN2_E_NULL; a caller with one dense side passes an array of full counts); validation order, codes
 * and envelopes are those of the one-sided twin above, and every host decision (geometry, queries per workgroup, LDS bytes, the
 * multi-radius plan) is taken from the padded n and m. Stream-ordered, no memset, nothing read on the host: capturable. */
int pn2_farthest_point_sample_ragged_counts(int b, int n, int m, const float *inp, const int *lengths, const int *npoints,
                                            int *out, float *out_xyz, void *stream);
int pn2_query_ball_group_xyz_ragged_pair(int b, int n, int m, float radius, int nsample, const float *xyz1, const int *lengths1,
                                         const float *xyz2, const int *lengths2, int subtract_centroid, int *idx, int *pts_cnt,
                                         float *grouped_xyz, int kernel, int cells_qpb, void *stream);
int pn2_query_ball_group_xyz_msg_ragged_pair(int b, int n, int m, int nscales, const float *radii, const int *nsamples,
                                             const float *xyz1, const int *lengths1, const float *xyz2, const int *lengths2,
                                             int subtract_centroid, int *const *idx, int *const *pts_cnt,
                                             float *const *grouped_xyz, void *stream);
int pn2_knn_point_ragged_pair(int b, int n, int m, int k, const float *xyz1, const int *lengths1, const float *xyz2,
                              const int *lengths2, float *val, int *idx, void *stream);
int pn2_three_nn_ragged_pair(int b, int n, int m, const float *xyz1, const int *lengths1, const float *xyz2, const int *lengths2,
                             float *dist, int *idx, int variant, void *stream);

/* ---- ragged inference: counts in the fused MLPs, one call per ragged level ------------------------------------------------------
 * The fused inference kernels with count arrays (b) int32 in DEVICE memory, never read by the host; a count is clamped into
 * 1..extent on the device, for memory safety only. THE SLICE RULE FOR THE FUSED MLPS: for cloud c the output rows below its count
 * are bit-identical to the dense entry applied to the cloud's slices alone (b = 1); output rows at or beyond the count are fully
 * written with all-zero bits (+0.0). Every row of the fused stacks is an independent fixed-order sum and the max pool is
 * order-independent, so the rule holds exactly. No host synchronisation and no memset beyond the dense entry's own clear of a
 * split group_all output; everything is stream-ordered and capturable.
 * Rows of xyz / points / points1 / points2 at or beyond a length may hold anything, NaN included, and influence nothing -- a
 * per-point pre-pass (the streamed SA kernel's layer 1, the FP kernels' Q = points2 . W1a) may still multiply them: those results
 * are never gathered. Rows of new_xyz, idx, dist at or beyond a count are never dereferenced (a padding row gathers through valid
 * row 0 of its own cloud, or is skipped). All host decisions (kernel family, grid, LDS, workspace bytes) come from the padded
 * extents: pn2_sa_mlp3_ws_bytes and pn2_fp_mlp_ws_bytes serve these entries unchanged, and so do the packed weights.
 *
 * pn2_sa_mlp3_maxpool_ragged: pn2_sa_mlp3_maxpool_ex (max pooling) with `lengths` behind xyz and `npoints` behind new_xyz.
 *   Grouped form: npoints is required (NULL: PN2_E_NULL) -- centroid row j of cloud c is valid for j < npoints[c]; lengths may be
 *   NULL (idx of a valid row stays below its cloud's length; it would only let a per-point pre-pass skip rows, which none does).
 *   group_all form (idx == NULL && new_xyz == NULL, m = 1, nsample = n): lengths is required (NULL: PN2_E_NULL) -- cloud c's group
 *   is its first lengths[c] rows; a non-NULL npoints is PN2_E_ARG. Otherwise the validation order and codes are the dense
 *   entry's: b == 0 / m == 0 is PN2_OK before any count pointer is looked at, a stack only the other pooling modes cover is
 *   PN2_E_TOO_LARGE.
 * pn2_fp_mlp_ragged: pn2_fp_mlp with `lengths1` (required) behind points1: rows of the unknown side at or beyond lengths1[c].
 * pn2_sa_level_ragged: pn2_farthest_point_sample_ragged_counts, pn2_query_ball_group_xyz_ragged_pair (kernel 0, cells_qpb 0,
 *   centroid subtracted), pn2_sa_mlp3_maxpool_ragged enqueued by one call; both count arrays are required (a caller with a dense
 *   side passes full counts). No overlapped launch: no sample workspace, no generation, no FPS temp. The first failing part's
 *   code is returned.
 * pn2_fp_level_ragged: pn2_three_nn_ragged_pair (variant 0) + pn2_fp_mlp_ragged. */
int pn2_sa_mlp3_maxpool_ragged(int b, int n, int m, int nsample, int cfeat, const float *xyz, const int *lengths,
                               const float *new_xyz, const int *npoints, const float *points, const int *idx, int c1, int c2,
                               int c3, const float *wpacked, const float *bpacked, float *out, void *ws, int variant,
                               void *stream);
int pn2_fp_mlp_ragged(int b, int n, int m, int c2, int c1, const float *points2, const float *points1, const int *lengths1,
                      const int *idx, const float *dist, int nlayers, const int *widths, int kind, const float *wpacked,
                      const float *bpacked, float *out, void *ws, void *stream);
int pn2_sa_level_ragged(int b, int n, int m, float radius, int nsample, int cfeat, const float *xyz, const int *lengths,
                        const int *npoints, const float *points, int c1, int c2, int c3, const float *wpacked,
                        const float *bpacked, int *fps_idx, float *new_xyz, int *idx, int *pts_cnt, float *grouped_xyz,
                        float *out, void *ws_mlp, void *stream);
int pn2_fp_level_ragged(int b, int n, int m, int c2, int c1, const float *xyz1, const int *lengths1, const float *xyz2,
                        const int *lengths2, const float *points2, const float *points1, int nlayers, const int *widths,
                        int kind, const float *wpacked, const float *bpacked, float *dist, int *idx, float *out, void *ws,
                        void *stream);

/* pn2_group_point / pn2_three_interpolate with the kernel choice per call (parity tests force every kernel,
 * scripts/bw_probe.py times them). group: 0 automatic, 1 flat first-generation kernels, 2 row kernels,
 * 3 row kernels with non-temporal stores; three_interpolate: 0 automatic, 1 flat, 2 row kernel, 3 row kernel with
 * non-temporal stores. */
int pn2_group_point_ex(int b, int n, int c, int m, int nsample, const float *points, const int *idx, float *out,
                       int variant, void *stream);
int pn2_three_interpolate_ex(int b, int m, int c, int n, const float *points, const int *idx, const float *weight,
                             float *out, int variant, void *stream);

/* farthest_point_sample (register-resident tier, n <= 16384) with an explicit workgroup geometry: T threads
 * in {256, 512, 1024}, P points per thread (a power of two, T * P >= 512 * ceil(n / 512)). Every geometry
 * returns the same indices; tests cover all of them, scripts/ time them. Stateless. */
int pn2_farthest_point_sample_ex(int T, int P, int b, int n, int m, const float *inp, int *out, void *stream);

/* farthest_point_sample [+ gather_point when out_xyz != NULL] with the TIER chosen by the caller. Every tier returns the
 * reference's indices (tf_sampling_g.cu:105-170); tests force each one, scripts time them.
 *   PN2_FPS_AUTO    what pn2_farthest_point_sample does: the batched tier at 513..8192 rank slots (= 512 * ceil(n / 512)) with
 *                   npoint >= 256, the pruned tier at 4097..8192 with 128 <= npoint < 256, the full tier otherwise;
 *   PN2_FPS_FULL    every point's running distance is updated against every new sample (csrc/fps_body.h);
 *   PN2_FPS_PRUNED  points dealt to the threads by a kd-tree built in LDS; per round only the groups whose bounding box
 *                   lies within the current farthest-point distance of the new sample are updated -- exactly the points
 *                   the reference's min() can change (csrc/fps_pruned_body.h). PN2_E_ARG outside 2049..8192 rank slots;
 *   PN2_FPS_BATCH   (round 6) the pruned tier's groups, several samples per arg-max exchange: a candidate list per batch, a wave of
 *                   its own for the arg-max chain, eight updater waves behind it (csrc/fps_batch_body.h). PN2_E_ARG outside
 *                   513..8192 rank slots. */
#define PN2_FPS_AUTO 0
#define PN2_FPS_FULL 1
#define PN2_FPS_PRUNED 2
#define PN2_FPS_BATCH 3
int pn2_farthest_point_sample_variant(int variant, int b, int n, int m, const float *inp, float *temp, int *out,
                                      float *out_xyz, void *stream);
/* The ragged entries (pn2_farthest_point_sample_ragged, and with npoints != NULL pn2_farthest_point_sample_ragged_counts) with
 * the tier chosen by the caller; those two are this entry with PN2_FPS_AUTO. variant as above, the size rule applied to the
 * padded n and m; PN2_FPS_FULL is the register tier in the geometry chosen from the padded n. The pruned and batched tiers run
 * their dense bodies on each cloud's slice with (lengths[c], npoints[c], ceil(lengths[c] / 512)) in the template of the padded
 * n: the slots beyond a cloud's points are the padding slots dense input has too (value 0, lowest key), up to all but one of
 * them (DESIGN.md 4.11 "padding slots"). Results are the slice rule's whatever the tier; the fill rows of the counts form are
 * index 0 and xyz[c, 0]. Neither count array is read by the host, no memset, capturable.
 * Codes: a variant out of range is PN2_E_ARG, checked first; then the order and codes of pn2_farthest_point_sample_ragged
 * (b = 0 or m <= 0 PN2_OK, extents PN2_E_SHAPE, inp / lengths / out NULL PN2_E_NULL, n > 16384 PN2_E_TOO_LARGE); a forced
 * PN2_FPS_PRUNED / PN2_FPS_BATCH outside its rank-slot envelope (of the padded n) is PN2_E_ARG. */
int pn2_farthest_point_sample_ragged_variant(int variant, int b, int n, int m, const float *inp, const int *lengths,
                                             const int *npoints /* NULL: m samples from every cloud */,
                                             int *out, float *out_xyz /* may be NULL */, void *stream);

/* ---- packed batches: clouds back to back with offsets, no padding ---------------------------------------------
 * Layout: the first side's coordinates are ONE flat array (total, 3) plus `offsets` (b + 1) int32 in DEVICE memory,
 * 0 = offsets[0] < offsets[1] < ... < offsets[b] = total; cloud c is rows offsets[c] .. offsets[c + 1] - 1. `nmax` is a HOST
 * bound on every cloud's count, offsets[c + 1] - offsets[c] <= nmax: kernel choice, FPS tier, grid and LDS bytes come from it
 * exactly as the _ragged entries take them from the padded n. The second side (the queries of the ball query, the known points
 * of three_nn) and the sampling outputs stay dense (b, m, ...). THE SLICE RULE, PACKED: for every cloud c the result is bit-
 * and index-identical to the dense entry applied to flat[offsets[c] : offsets[c + 1]] alone (b = 1) -- hence to the _ragged
 * entry on the same clouds padded --, and no cloud reads a row of its neighbours. A slab may start at any row (coordinates are
 * read as scalars).
 * global_idx: 0 = indices are cloud-local, as the reference's; 1 = a point index of the packed side is written as
 *   offsets[c] + k, a row of the flat array, and a known-point index of pn2_three_nn_packed as c m + j, a row of xyz2 viewed as
 *   (b m, 3) -- what the index-driven operators (group_point, three_interpolate, the fused stacks) take on the flat views
 *   (1, total, c) / (1, b m, c). One wave-uniform add where the index is stored; everything else is the local result.
 * The host never reads `offsets` (no synchronisation, no memset, stream-ordered: capturable, and a replay follows offsets changed
 * in place); the kernels clamp a cloud's start into 0..total-1 and its count into 1..min(nmax, total - start) for memory safety
 * only -- validating is the caller's business (Python: pointnet2_amd.check_offsets).
 * Codes, in this order (the _ragged entries'): attributes out of range PN2_E_ARG; b < 0, nmax <= 0, m < 0 PN2_E_SHAPE; b = 0 or
 * m = 0 (three_nn: b = 0) PN2_OK before any pointer is looked at; total <= 0 PN2_E_SHAPE; a missing array PN2_E_NULL;
 * total 3 > INT_MAX PN2_E_TOO_LARGE.
 *
 * pn2_farthest_point_sample_packed: variant as pn2_farthest_point_sample_ragged_variant, the size rule on nmax and m; tie rank
 *   per cloud, Q_c = ceil(n_c / 512). out (b,m), out_xyz (b,m,3) or NULL (always the cloud's own points, whatever global_idx).
 *   m > n_c behaves as the dense operator with npoint > n. PN2_E_TOO_LARGE for nmax > 16384.
 * pn2_query_ball_group_xyz_packed: xyz1 (total,3) packed, the queries xyz2 (b,m,3) dense; kernel / cells_qpb as
 *   pn2_query_ball_group_xyz_ragged; idx (b,m,nsample), pts_cnt (b,m), grouped_xyz (b,m,nsample,3) or NULL.
 * pn2_three_nn_packed: the UNKNOWN side xyz1 (total,3) packed, the known side xyz2 (b,m,3) dense or -- lengths2 != NULL -- with
 *   lengths2[c] valid rows as in pn2_three_nn_ragged_pair; variant as pn2_three_nn_ex. dist, idx (total,3): row offsets1[c] + i
 *   belongs to point i of cloud c; there are no padding rows.
 * pn2_query_ball_group_xyz_msg_packed: pn2_query_ball_group_xyz_msg with xyz1 (total,3) packed, the queries xyz2 (b,m,3) dense:
 *   ONE launch, one staging / binning of every cloud for all radii. Per cloud and radius the result equals
 *   pn2_query_ball_group_xyz_msg on flat[offsets1[c] : offsets1[c + 1]] alone, hence pn2_query_ball_group_xyz_packed per radius
 *   and pn2_query_ball_group_xyz_msg_ragged on the padded copy. idx[i] (b,m,nsamples[i]), pts_cnt[i] (b,m), grouped_xyz[i]
 *   (b,m,nsamples[i],3); pts_cnt, as a whole or per scale, and idx[i] beside a grouped_xyz[i] may be NULL as in the other
 *   multi-radius entries. Every host decision comes from nmax: pn2_query_ball_group_xyz_msg_plan(b, nmax, m, ...) reports what
 *   is launched. Codes in the order of pn2_query_ball_group_xyz_msg_ragged with offsets1 where lengths1 stood: PN2_E_ARG
 *   (nscales, radii, nsamples), PN2_E_SHAPE (b < 0, nmax <= 0, m < 0), PN2_OK for b = 0 or m = 0, PN2_E_SHAPE for total <= 0
 *   or nmax > total, PN2_E_NULL for offsets1, then for a scale with neither idx nor grouped_xyz, PN2_E_TOO_LARGE for nmax above
 *   the cell kernels' point limit (8192), a shape no LDS geometry fits, or total 3 > INT_MAX -- nothing is launched, call
 *   pn2_query_ball_group_xyz_packed per radius then, as the Python operator does --, PN2_E_NULL for xyz1 / xyz2. */
int pn2_farthest_point_sample_packed(int variant, int b, int total, int nmax, int m, const float *inp, const int *offsets,
                                     int global_idx, int *out, float *out_xyz /* may be NULL */, void *stream);
int pn2_query_ball_group_xyz_packed(int b, int total, int nmax, int m, float radius, int nsample, const float *xyz1,
                                    const int *offsets1, const float *xyz2, int subtract_centroid, int global_idx, int *idx,
                                    int *pts_cnt, float *grouped_xyz, int kernel, int cells_qpb, void *stream);
int pn2_three_nn_packed(int b, int total, int nmax, int m, const float *xyz1, const int *offsets1, const float *xyz2,
                        const int *lengths2 /* may be NULL */, int global_idx, float *dist, int *idx, int variant, void *stream);
int pn2_query_ball_group_xyz_msg_packed(int b, int total, int nmax, int m, int nscales, const float *radii, const int *nsamples,
                                        const float *xyz1, const int *offsets1, const float *xyz2, int subtract_centroid,
                                        int global_idx, int *const *idx, int *const *pts_cnt, float *const *grouped_xyz, void *stream);

/* The second side, packed: a count per cloud behind the offsets -- the sample counts of FPS, the valid rows of the dense query
 * side (b,m,3) of the ball queries and of kNN. THE PAIR SLICE RULE ("ragged batches, the second side") COMBINED WITH THE SLICE
 * RULE, PACKED: for cloud c with n_c = offsets[c + 1] - offsets[c] points and m_c valid rows on the second side, the rows
 * j < m_c are bit- and index-identical to the dense entry on (flat[offsets[c] : offsets[c + 1]], xyz2[c, :m_c]) alone and to the
 * _ragged_counts / _ragged_pair entry on the same clouds padded. No cloud reads a row of its neighbours; no query row at or
 * beyond m_c is read. The rows j >= m_c are fully written with the padded twin's fixed values, except that under
 * global_idx = 1 every index fill is offsets[c], the cloud's own first row, where the local form writes 0 -- the rule an empty
 * ball already follows --, so idx - offsets[c] equals the padded twin everywhere and every stored index names a row of its own
 * cloud. Counts are (b) int32 on the device, never read by the host, clamped on the device into 1..m for memory safety only.
 * Every host decision (FPS tier, grid, LDS bytes, queries per workgroup, the multi-radius plan) comes from nmax and m as in the
 * one-sided entries; no memset, no synchronisation, capturable, and a replay follows offsets and counts changed in place.
 * Codes: those of the one-sided packed entry of the same family, in its order; npoints / lengths2 are required in the _counts
 * / _pair entries (PN2_E_NULL where the offsets are checked).
 *
 * pn2_farthest_point_sample_packed_counts: cloud c yields npoints[c] samples; rows from there on repeat sample 0 -- index 0
 *   (offsets[c] under global_idx) and the cloud's first point. PN2_E_TOO_LARGE for nmax > 16384.
 * pn2_query_ball_group_xyz_packed_pair: fill rows idx 0 (offsets1[c]), pts_cnt 0, grouped_xyz +0.0.
 * pn2_query_ball_group_xyz_msg_packed_pair: the same for every radius of the one launch; the plan is
 *   pn2_query_ball_group_xyz_msg_plan(b, nmax, m, ...).
 * pn2_knn_point_packed: pn2_knn_point with xyz1 (total,3) packed, xyz2 (b,m,3), val / idx (b,m,k). The first min(k, n_c) entries
 *   of a row are pn2_knn_point's on the slice, the rest repeat entry 0 (pn2_knn_point_ragged). lengths2 NULL: every query row is
 *   valid; else fill rows are val +0.0, idx 0 (offsets1[c]). Codes of pn2_knn_point_ragged with nmax where n stood: k <= 0
 *   PN2_E_ARG; b < 0, nmax <= 0, m < 0 PN2_E_SHAPE; b m = 0 PN2_OK; total <= 0 PN2_E_SHAPE; a missing array PN2_E_NULL; k > nmax,
 *   nmax > 14336 or total 3 > INT_MAX PN2_E_TOO_LARGE. */
int pn2_farthest_point_sample_packed_counts(int variant, int b, int total, int nmax, int m, const float *inp, const int *offsets,
                                            const int *npoints, int global_idx, int *out, float *out_xyz /* may be NULL */,
                                            void *stream);
int pn2_query_ball_group_xyz_packed_pair(int b, int total, int nmax, int m, float radius, int nsample, const float *xyz1,
                                         const int *offsets1, const float *xyz2, const int *lengths2, int subtract_centroid,
                                         int global_idx, int *idx, int *pts_cnt, float *grouped_xyz, int kernel, int cells_qpb,
                                         void *stream);
int pn2_query_ball_group_xyz_msg_packed_pair(int b, int total, int nmax, int m, int nscales, const float *radii, const int *nsamples,
                                             const float *xyz1, const int *offsets1, const float *xyz2, const int *lengths2,
                                             int subtract_centroid, int global_idx, int *const *idx, int *const *pts_cnt,
                                             float *const *grouped_xyz, void *stream);
int pn2_knn_point_packed(int b, int total, int nmax, int m, int k, const float *xyz1, const int *offsets1, const float *xyz2,
                         const int *lengths2 /* may be NULL */, int global_idx, float *val, int *idx, void *stream);

/* farthest_point_sample [+ gather_point when out_xyz != NULL] for LARGE dense clouds, 16384 < n <= 1048576: the tier of
 * csrc/fps_large.hip. Same indices as pn2_farthest_point_sample, tie rule (smallest (k mod 512, k)), inf
 * distances clamped to the 1e38 start value, duplicates and m > n included; out_xyz == gather_point(inp, out) bit for bit, written
 * as the samples are chosen. One launch of one workgroup per cloud: the cloud is sorted into the cells of a grid (records
 * {x, y, z, k} in ws), cut into groups of group_len consecutive records with tight boxes, and a round updates only the groups the
 * new sample can reach (the pruned tier's exact rule). No memset, no host synchronisation, capturable.
 *   pn2_fps_large_supported(n, m)  1 inside the envelope (16384 < n <= 1048576, m >= 1), else 0;
 *   pn2_fps_large_pays(n, m)       1 where the tier measured faster than the global-memory kernel of pn2_farthest_point_sample on
 *                                  uniform AND sphere-surface clouds by more than the spread of the measurement
 *                                  (profiles/fps_large/README.md); the Python operators follow it;
 *   pn2_fps_large_ws_bytes(b, n)   size of ws: 20 bytes per point ((b, n) 16-byte records, then (b, n) running distances); 0
 *                                  outside the envelope. ws needs no initialisation and must be 16-byte aligned (PN2_E_ARG).
 *   group_len                      64, 128 or 256 records per group (the plain entry: 256). At most 4096 groups per cloud: 64 covers
 *                                  n <= 262144, 128 n <= 524288, 256 the whole envelope (PN2_E_TOO_LARGE beyond).
 * Codes, in this order, all before anything is launched: m <= 0 or b == 0 PN2_OK; b < 0 or n <= 0 PN2_E_SHAPE; inp, out or ws
 * NULL PN2_E_NULL; n outside the envelope, or b n 3 / b m 3 beyond int32, PN2_E_TOO_LARGE; group_len not one of the three
 * PN2_E_ARG. Ragged batches: the _large_ragged entries below (the _ragged entries stop at 16384 points). */
long long pn2_fps_large_ws_bytes(int b, int n);
int pn2_fps_large_supported(int n, int m);
int pn2_fps_large_pays(int n, int m);
int pn2_farthest_point_sample_large(int b, int n, int m, const float *inp, void *ws, int *out, float *out_xyz /* may be NULL */,
                                    void *stream);
int pn2_farthest_point_sample_large_ex(int group_len, int b, int n, int m, const float *inp, void *ws, int *out,
                                       float *out_xyz /* may be NULL */, void *stream);

/* Ragged batches of LARGE clouds, padded n of 16385 .. 1048576: `lengths` (b) and `npoints` (b, or NULL: m samples from every
 * cloud) int32 in DEVICE memory, clamped on the device into 1..n / 1..m, never read by the host. THE SLICE RULE of the ragged
 * entries above: cloud c's rows below npoints[c] are the first npoints[c] samples of the dense operator on inp[c, :lengths[c]]
 * alone, tie rule included (m > lengths[c] behaves as the dense operator with npoint > n); rows from npoints[c] on are index 0 and
 * inp[c, 0]; rows of inp at or beyond lengths[c] are never read. One launch of one workgroup per cloud, no memset, no host
 * synchronisation, capturable; nothing is kept between launches beyond ws.
 *   ws         pn2_fps_large_ws_bytes(b, n) bytes on the PADDED n, 16-byte aligned, no initialisation;
 *   kernel     0 = the library's rule, pn2_fps_large_pays(n, m) on the padded extents (the host knows no others);
 *              1 = the global-memory kernel of pn2_farthest_point_sample with counts (its running distances in ws);
 *              2 = the cell-sorted tier of pn2_farthest_point_sample_large (csrc/fps_large.hip);
 *   group_len  64, 128 or 256, as pn2_farthest_point_sample_large_ex (kernel 1 ignores a valid value).
 * The plain entry is _ex(0, 256, ...). Results never depend on kernel or group_len.
 * Codes, in this order, all before anything is launched: m <= 0 or b == 0 PN2_OK; b < 0 or n <= 0 PN2_E_SHAPE; inp, out, ws or
 * lengths NULL PN2_E_NULL; n outside the envelope, or b n 3 / b m 3 beyond int32, PN2_E_TOO_LARGE; kernel not 0..2 or group_len
 * not one of the three PN2_E_ARG; more than 4096 groups of group_len records in n points where the tier would run
 * PN2_E_TOO_LARGE; a misaligned ws PN2_E_ARG. */
int pn2_farthest_point_sample_large_ragged(int b, int n, int m, const float *inp, const int *lengths,
                                           const int *npoints /* NULL: m samples from every cloud */, void *ws, int *out,
                                           float *out_xyz /* may be NULL */, void *stream);
int pn2_farthest_point_sample_large_ragged_ex(int kernel, int group_len, int b, int n, int m, const float *inp, const int *lengths,
                                              const int *npoints /* NULL: m samples from every cloud */, void *ws, int *out,
                                              float *out_xyz /* may be NULL */, void *stream);

/* Packed batches of LARGE clouds (the packed layout of pn2_farthest_point_sample_packed, which stops at nmax = 16384): cloud c is
 * inp[offsets[c] : offsets[c + 1]] of a flat (total, 3) array, offsets (b + 1) int32 in DEVICE memory, clamped on the device and
 * never read by the host; 16384 < nmax <= 1048576 bounds every cloud's count and stands for the padded n in every host decision.
 * Result per cloud = the dense operator on the slice, tie rule included; global_idx 1 adds offsets[c] to the cloud's indices; out
 * (b, m) and out_xyz (b, m, 3) are dense. One launch of one workgroup per cloud, no memset, no global atomics, no host
 * synchronisation: capturable, and a replay follows offsets rewritten in place.
 *   ws         pn2_fps_large_packed_ws_bytes(total) = 20 total bytes: total 16-byte records, then total floats (0 for total <= 0);
 *              16-byte aligned, no initialisation. Cloud c uses the rows offsets[c] .. of both arrays;
 *   kernel     0 = pn2_fps_large_pays(nmax, m), 1 = the global-memory kernel, 2 = the cell-sorted tier;
 *   group_len  64, 128 or 256 (kernel 1 ignores a valid value);
 *   short_max  the tier only (kernel 1 ignores a valid value): a cloud of at most short_max points is sampled by a body that
 *              keeps it in LDS and registers -- no cell sort, ws untouched for that cloud. -1 = the library's measured rule
 *              (profiles/fps_large_packed/README.md), 0 = never, 1 .. 8192 = that threshold.
 * The plain entry is _ex(0, 256, -1, ...). Results never depend on kernel, group_len or short_max.
 * Codes, in this order, all before anything is launched: m <= 0 or b == 0 PN2_OK; b < 0, nmax <= 0 or total <= 0 PN2_E_SHAPE; inp,
 * offsets, out or ws NULL PN2_E_NULL; nmax outside the envelope, or total 3 / b m 3 beyond int32, PN2_E_TOO_LARGE; kernel not
 * 0..2, group_len not one of the three or short_max not -1..8192 PN2_E_ARG; more than 4096 groups of group_len records in nmax
 * points where the tier would run PN2_E_TOO_LARGE; a misaligned ws PN2_E_ARG. */
long long pn2_fps_large_packed_ws_bytes(int total);
int pn2_farthest_point_sample_large_packed(int b, int total, int nmax, int m, const float *inp, const int *offsets, int global_idx,
                                           void *ws, int *out, float *out_xyz /* may be NULL */, void *stream);
int pn2_farthest_point_sample_large_packed_ex(int kernel, int group_len, int short_max, int b, int total, int nmax, int m,
                                              const float *inp, const int *offsets, int global_idx, void *ws, int *out,
                                              float *out_xyz /* may be NULL */, void *stream);

/* The whole xyz half of sample_and_group (pointnet_util.py:40-46) in ONE launch, with the ball
 * queries overlapped under the farthest-point-sampling chain: producer workgroups (one per cloud)
 * publish each sample as they select it, consumer workgroups on the other CUs run query j as soon as
 * sample j exists. Outputs are bit-identical to the separate operators:
 *   fps_idx (b,m) i32, new_xyz (b,m,3) f32, idx (b,m,nsample) i32, pts_cnt (b,m) i32,
 *   grouped_xyz (b,m,nsample,3) f32 (minus the centroid when subtract_centroid != 0).
 * ws: device scratch of pn2_sample_and_group_ws_bytes(b,m) bytes (zeroed here on `stream`): the sample
 * granules and a status word.
 * Returns PN2_E_TOO_LARGE for shapes outside the overlapped launch's envelope (b > 256, n > 8192,
 * n < 64, nsample > 256) and when the device cannot hold all b producer workgroups at once
 * (occupancy query at launch): use pn2_farthest_point_sample_gather + pn2_query_ball_group_xyz then.
 * Clouds too large for a cell list beside their sorted copy in LDS (n > ~7000) are served by exactly those two launches from
 * inside this call (their consumers would have to sweep the whole cloud per query and no longer hide under the chain:
 * 478 us against 459 at b = 8, 8192 -> 1024); same outputs, ws untouched.
 * Inside a captured HIP graph (hipStreamIsCapturing on `stream`) this call enqueues exactly those two launches as well: a
 * replayed overlapped launch would carry the same tag as the replay before it and depend on the clear alone, and round 5's
 * soak of a serving loop saw such launches accept granules that were not theirs (profiles/r06/stale_granules.md). The
 * overlapped launch INSIDE a graph is pn2_sample_and_group_xyz_gen(generation = PN2_GENERATION_DEVICE). */
int pn2_sample_and_group_xyz(int b, int n, int m, float radius, int nsample, const float *xyz, void *ws,
                             int *fps_idx, float *new_xyz, int *idx, int *pts_cnt, float *grouped_xyz,
                             int subtract_centroid, void *stream);
long long pn2_sample_and_group_ws_bytes(int b, int m);
/* The same launch without the per-call clear of ws: the caller manages generations. Zero ws ONCE when it is
 * allocated, then pass a generation that no earlier launch on this workspace used (1, 2, 3, ... 0xfffffffe: what an
 * earlier generation left behind can never be mistaken for a published sample). One ws per stream;
 * generation 0 is PN2_E_ARG; re-zero ws before wrapping around. Saves a memset launch (~5 us) per call.
 * generation = PN2_GENERATION_DEVICE (round 6): the launch numbers ITSELF -- every workgroup of a cloud arrives at a counter
 * word of ws with one returning atomic add, which gives the cloud's producer and consumers the same launch ordinal and
 * consecutive launches different tags, with no clear and no number from the host. This is the form for captured graphs
 * (frozen arguments): zero ws ONCE when it is allocated (outside the graph), give every captured call site a workspace of
 * its own, never use a workspace in two forms or from two launches at the same time. Costs the chain one atomic round trip
 * (~2 us) per launch. */
#define PN2_GENERATION_DEVICE 0xffffffffu
int pn2_sample_and_group_xyz_gen(int b, int n, int m, float radius, int nsample, const float *xyz, void *ws,
                                 unsigned generation, int *fps_idx, float *new_xyz, int *idx, int *pts_cnt,
                                 float *grouped_xyz, int subtract_centroid, void *stream);
/* Byte offset inside ws of the launch status word (u32): 0 ok, 1 = a consumer stopped waiting for its producer
 * after ~10 s (cannot happen while the device makes progress; the launch's outputs are then incomplete). The
 * library never synchronises, so a caller that wants to assert forward progress reads the word after
 * synchronising the stream. */
long long pn2_sample_and_group_status_offset(int b, int m);
/* pn2_sample_and_group_xyz[_gen] with the organisation of the launch chosen by the caller (outputs never depend on it):
 * fps_variant = FPS tier of the producer workgroups (PN2_FPS_AUTO / PN2_FPS_FULL / PN2_FPS_PRUNED / PN2_FPS_BATCH as in
 * pn2_farthest_point_sample_variant); consumers = persistent consumer workgroups per cloud (0 = the library's choice, which
 * includes the two launches for clouds beyond ~7000 points; > 0 = always the overlapped launch; each
 * stages its cloud once and walks the 64-query ranges c, c + consumers, ... in publish order; the grid is
 * b * (1 + consumers) workgroups, consumers <= 16). generation 0 = clear `ws` first (eager; the two launches inside a capture),
 * PN2_GENERATION_DEVICE as in pn2_sample_and_group_xyz_gen. */
int pn2_sample_and_group_xyz_ex(int b, int n, int m, float radius, int nsample, const float *xyz, void *ws, unsigned generation,
                                int fps_variant, int consumers, int *fps_idx, float *new_xyz, int *idx, int *pts_cnt,
                                float *grouped_xyz, int subtract_centroid, void *stream);


/* ---- one call per level (inference) ---------------------------------------------------------------------
 * pn2_sa_level = pointnet_sa_module (utils/pointnet_util.py:87-154) for max pooling and three layers: the overlapped
 * sample-and-group launch (or, outside its envelope, pn2_farthest_point_sample_gather + pn2_query_ball_group_xyz) followed
 * by pn2_sa_mlp3_maxpool, enqueued by ONE call. ws_sample: pn2_sample_and_group_ws_bytes(b, m) bytes, handled as in
 * pn2_sample_and_group_xyz_gen (generation > 0: zeroed once by the caller, a fresh generation per call, or
 * PN2_GENERATION_DEVICE for captured graphs) or cleared here (generation = 0; the two launches inside a capture); NULL: never the overlapped launch, always the two-launch path; fps_temp: pn2_fps_temp_floats(b, n) floats or NULL when that is 0; ws_mlp: pn2_sa_mlp3_ws_bytes(...)
 * bytes or NULL when that is 0; wpacked / bpacked from pn2_sa_mlp3_pack. Outputs as the two operators' (all required).
 * pn2_fp_level = pointnet_fp_module (:199-229): pn2_three_nn followed by pn2_fp_mlp (dist / idx are outputs too). */
int pn2_sa_level(int b, int n, int m, float radius, int nsample, int cfeat, const float *xyz, const float *points,
                 void *ws_sample, unsigned generation, float *fps_temp, int c1, int c2, int c3, const float *wpacked,
                 const float *bpacked, int *fps_idx, float *new_xyz, int *idx, int *pts_cnt, float *grouped_xyz, float *out,
                 void *ws_mlp, void *stream);
int pn2_fp_level(int b, int n, int m, int c2, int c1, const float *xyz1, const float *xyz2, const float *points2,
                 const float *points1, int nlayers, const int *widths, int kind, const float *wpacked, const float *bpacked,
                 float *dist, int *idx, float *out, void *ws, void *stream);
/* pn2_sa_level for a level whose xyz is believed to be in farthest-point order (the previous level's new_xyz):
 * pn2_farthest_point_sample_ordered (ws_ordered: its workspace) + pn2_query_ball_group_xyz + pn2_sa_mlp3_maxpool. Same
 * outputs as pn2_sa_level for any input. */
int pn2_sa_level_ordered(int b, int n, int m, float radius, int nsample, int cfeat, const float *xyz, const float *points,
                         void *ws_ordered, int c1, int c2, int c3, const float *wpacked, const float *bpacked, int *fps_idx,
                         float *new_xyz, int *idx, int *pts_cnt, float *grouped_xyz, float *out, void *ws_mlp, void *stream);

/* ---- training mode of the shared MLPs (second half) ---------------------------
 *
 * The reference builds every SA / FP level with is_training = True (train.py:188): each of the level's
 * tf_util.conv2d 1x1 layers is followed by batch normalisation over ALL rows of the level
 * (tf_util.py:512-531: batch moments, eps 1e-3, moving averages updated with bn_decay, train.py:96-104) and a
 * ReLU; SA levels end in reduce_max over nsample (utils/pointnet_util.py:113-127), FP levels do not (:222-226).
 * pn2_mlp_train_forward / _backward run such a stack in training mode on the matrix cores:
 *   forward, per layer l:   z_l = h_{l-1} W_l + b_l         one MFMA GEMM launch; its prologue forms
 *                                                           h_{l-1} = relu(a_{l-1} z_{l-1} + c_{l-1}) from the stored
 *                                                           pre-norm tensor (layer 1: gathers the grouped rows from
 *                                                           xyz / points / idx -- the (b,m,nsample,C) tensor never
 *                                                           exists); its epilogue accumulates sum z, sum z^2 per
 *                                                           channel (and, last SA layer, the per-group max / min of z
 *                                                           with their sample numbers: BN + ReLU are monotone per
 *                                                           channel, so the pool commutes with them)
 *                           (a_l, c_l) from the batch moments, running statistics updated in place
 *   backward, per layer:    dz_l = s_l dy_l - c0_l - c1_l z_l   (batch-norm backward written per channel)
 *                           dW_l = h_{l-1}^T dz_l           MFMA, contraction over the rows
 *                           dy_{l-1} = (dz_l W_l^T) . [h_{l-1} > 0]    MFMA GEMM; epilogue accumulates the two
 *                                                           per-channel sums batch-norm backward needs one layer down
 * fp32 in, fp32 out; products on the bf16 matrix pipe as six bf16 terms (see pn2_sa_mlp3_maxpool).
 * Everything is enqueued on `stream` from ONE call per direction; no host synchronisation; all buffers the
 * caller's. rows must be a multiple of 32; widths multiples of 4 (layer 1's input width is free when grouped).
 */
typedef struct pn2_group_src {     /* the rows of a grouped tensor (pointnet_util.py:44-50, :59-84): row = (cloud*m + j)*nsample + k */
    int b, n, m, nsample;
    int cfeat;                     /* channels of `points` (0: xyz only) */
    int xyz_first;                 /* channel order [xyz, features] (:50, single-scale) or [features, xyz] (:184, MSG) */
    const float *xyz;              /* (b,n,3) */
    const float *new_xyz;          /* (b,m,3), subtracted from the grouped xyz; NULL: no centroid (group_all) */
    const float *points;           /* (b,n,cfeat) or NULL */
    const int *idx;                /* (b,m,nsample); NULL: sample k of the group is point k (group_all: m = 1, nsample = n) */
    const void *idx_plan;          /* pn2_group_point_plan(b, n, m, nsample, idx, ...) of THIS idx, or NULL. With a plan the
                                      backward calls reduce from it (pn2_group_point_grad_planned) and invert nothing; NULL =
                                      they invert idx themselves, as before. The struct gained this trailing field with the
                                      index plans (56 -> 64 bytes): callers MUST zero-initialise pn2_group_src (memset / = {0})
                                      before filling it. */
} pn2_group_src;

typedef struct pn2_bn_layer {
    int cin, cout;
    const float *weight;           /* W[k][n] = weight[k*w_stride_k + n*w_stride_n]; a torch conv kernel (cout,cin,1,1): 1, cin */
    long long w_stride_k, w_stride_n;
    const float *bias;             /* (cout) or NULL */
    const float *gamma, *beta;     /* batch-norm scale / offset (cout) */
    float *running_mean, *running_var;   /* (cout), updated in place with `momentum`; NULL: not tracked */
    float momentum, eps;           /* torch convention: new = (1-momentum)*old + momentum*batch; momentum = 1 - bn_decay */
    float *z;                      /* (rows, cout) pre-norm tensor h W (WITHOUT the bias, which batch norm cancels), written by forward, read by backward */
    float *save;                   /* (4, cout): batch mean of z (= the layer's batch mean - bias), 1/sqrt(var+eps), a = gamma*invstd, c = beta - a*mean */
    float *grad_weight;            /* backward: same strides as weight */
    float *grad_gamma, *grad_beta; /* backward: (cout) */
    int grad_accumulate;           /* backward: 0 = the three gradients are written, 1 = ADDED to what the buffers hold (one fp32
                                      add per element, as a framework's own accumulation into .grad would do) */
    int running_var_biased;        /* which batch variance enters running_var: 0 = the UNBIASED one, var * N / (N - 1)
                                      (torch.nn.BatchNorm; also tf.contrib.layers.batch_norm, the reference's live path
                                      tf_util.py:526-531, wherever it takes the fused kernel); 1 = the biased one, var
                                      (tf.nn.moments: contrib's non-fused path, the default of the TF 1.2 the reference
                                      was tested on). The struct gained this trailing field in library version 0.2.0:
                                      callers MUST zero-initialise pn2_bn_layer (memset / = {0}) before filling it. */
} pn2_bn_layer;

/* pool_rows: 0 = no pooling, out is (rows, cout_L) = relu(bn(z_L)); else the group size (nsample: 16 or a multiple of
 * 32), out (rows/pool_rows, cout_L) = max over the group; argsel (same shape, i32) receives the sample number the
 * gradient flows to and zsel the selected pre-norm value (both needed by backward).
 * group != NULL: layer 1 reads the grouped rows; else x is the (rows, cin_1) input. */
/* Organisation of the passes (csrc/train_mlp.hip) is chosen by size rules -- results never depend on it. The *_ex entry
 * points take the rules' overrides as a per-call argument (A/B timing, and the tests that force every variant); the
 * library reads no environment variable and keeps no mode. A zeroed struct (or opts == NULL) = every rule automatic. */
enum { PN2_OPT_AUTO = 0, PN2_OPT_OFF = 1, PN2_OPT_ON = 2 };
typedef struct pn2_train_opts {
    int top_stored;                /* keep the pooled top layer's pre-norm tensor z_L (AUTO: kept below 32 MB) */
    int top_sparse;                /* routed part of that layer's weight gradient on the vector units (AUTO: from 2^24 row x inputs) */
    int l1_per_point;              /* layer 1 of a grouped level with features once per point (OFF: never) */
    int l1_coords;                 /* layer 1 of a feature-less level on the vector units (OFF: never) */
    int force_stream;              /* ON: weights streamed through LDS even where they would stay resident */
    int max_ns;                    /* cap on 32-column output tiles per wave: 0 (= 4), 1, 2, 4 */
    int nt;                        /* non-temporal stores: AUTO by size (outputs >= 128 MB), OFF never, ON always */
    int fuse_wgrad;                /* a layer's data gradient inside its weight-gradient pass (one pass over the layer's activations
                                      instead of two; AUTO: from 0.5 M rows where the layer's tiles fit one slab; ON: wherever
                                      they fit, the z-free pooled top layer included), OFF: never */
    int wgrad_two_per_cu;          /* two weight-gradient workgroups per CU where registers and LDS allow (AUTO / ON), OFF: one */
    int side_stream;               /* backward: the weight-gradient launches on a helper stream beside the data-gradient chain
                                      (fork / join by events on the caller's stream): ON only -- measured slower on all but the
                                      group_all level, so AUTO = OFF */
    int pair_launch;               /* backward: a layer's data-gradient GEMM and its weight-gradient pass as two ranges of workgroups
                                      of ONE launch (independent passes over the same tensors; AUTO: below 0.5 M rows, where each is a
                                      latency-bound launch over part of the chip; ON: wherever the shape pair has a kernel), OFF: never */
    int fold_finalize;             /* the per-channel finalisation of a pass's sums (batch moments -> coefficients, running statistics;
                                      backward: grad_gamma, grad_beta, dz coefficients) by the LAST workgroup of the pass that produced
                                      them (ticket; write-through partial rows) instead of a launch of its own: ON only -- measured
                                      1-8 us SLOWER per pass than the 5 us launch it saves (the XCDs' L2s are not coherent: the hand-off
                                      is four trips to memory), so AUTO = OFF. The sums are added in a fixed order either way; the two
                                      orders differ, so results agree to the fp64 rounding of the sums, not bit for bit */
} pn2_train_opts;
long long pn2_mlp_train_ws_bytes(long long rows, int nlayers, const int *widths /* cin_1, cout_1 .. cout_L */,
                                 int pool_rows, int backward,
                                 const int *group_dims /* grouped input: {b, n, m, nsample, cfeat, idx != NULL}; else NULL */);
/* 1: layer 1 of this grouped level is evaluated once per POINT -- z_1 = (points W1f)[idx] + (xyz - c) W1x + b, the
 * feature term being a GEMM over the b n points instead of the b m nsample rows (csrc/train_mlp.hip, tl_l1_forward_kernel)
 * -- and backward then produces the gradient of `points` itself (grad_points) instead of the per-row grad_feat_rows. */
int pn2_mlp_train_layer1_per_point(int nlayers, const int *widths, const int *group_dims);
/* 1: layers[L-1].z (the top layer's pre-norm tensor) is written by forward and read by backward; 0: it is neither --
 * pooled stacks of >= 2 layers on large levels run the passes that would read z_L on the layer's INPUT instead
 * (z_L = h W + b; csrc/train_mlp.hip, tl_top_mats_kernel), and layers[L-1].z may be NULL. */
int pn2_mlp_train_top_stored(long long rows, int nlayers, const int *widths, int pool_rows);
int pn2_mlp_train_forward(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                          const float *x, int pool_rows, float *out, int *argsel, float *zsel, void *ws, void *stream);
/* grad_out: shape of out. grad_x: (rows, cin_1) or NULL (plain input). Grouped input: grad_feat_rows (rows, cfeat) -- the
 * gradient of the grouped FEATURE rows, to be scattered with pn2_group_point_grad_seg -- or, when
 * pn2_mlp_train_layer1_per_point() says so, grad_points (b, n, cfeat), the gradient of `points` itself (the scatter runs
 * inside, `reproducible` selects its sorted-segment mode); NULL: not wanted. The bias gradient of a layer under batch
 * normalisation is identically zero and is not produced. */
int pn2_mlp_train_backward(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                           const float *x, int pool_rows, const float *out, const int *argsel, const float *zsel,
                           const float *grad_out, float *grad_x, float *grad_feat_rows, float *grad_points, int reproducible,
                           void *ws, void *stream);
/* the same five entry points with the organisation overrides (the plain ones pass NULL) */
long long pn2_mlp_train_ws_bytes_ex(long long rows, int nlayers, const int *widths, int pool_rows, int backward,
                                    const int *group_dims, const pn2_train_opts *opts);
int pn2_mlp_train_layer1_per_point_ex(int nlayers, const int *widths, const int *group_dims, const pn2_train_opts *opts);
int pn2_mlp_train_top_stored_ex(long long rows, int nlayers, const int *widths, int pool_rows, const pn2_train_opts *opts);
int pn2_mlp_train_forward_ex(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                             const float *x, int pool_rows, float *out, int *argsel, float *zsel, void *ws,
                             const pn2_train_opts *opts, void *stream);
int pn2_mlp_train_backward_ex(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                              const float *x, int pool_rows, const float *out, const int *argsel, const float *zsel,
                              const float *grad_out, float *grad_x, float *grad_feat_rows, float *grad_points,
                              int reproducible, void *ws, const pn2_train_opts *opts, void *stream);
/* The pooling modes of pointnet_sa_module (utils/pointnet_util.py:128-142) in training mode, grouped input only (the entries
 * above pool by max). pooling: 0 max (the _ex entries' path, bit for bit), 1 avg (out (groups, cout_L) = the mean over the
 * group, padded ball-query slots included, :130-131), 2 weighted_avg (w = exp(-5 |grouped xyz|) normalised over the group,
 * :132-138; group_all: |xyz|), 3 max_and_avg (out (groups, 2 cout_L) = concat([avg, max]), :139-142; the max half is
 * pooling 0's output bit for bit). Modes 1-3 keep the top layer's pre-norm tensor (layers[L-1].z is always written and
 * read: opts.top_stored does not apply) and reduce each group after the layer's batch moments; their backward forms the
 * dense top gradient and runs the layers below as pooling 0 does. argsel / zsel (groups, cout_L): modes 0 and 3 only;
 * pool_w (rows) f32: mode 2 only -- the normalised weights, written by forward, read by backward. Returns PN2_E_ARG for a
 * pooling outside 0..3, PN2_E_NULL for modes 1-3 without `group`, before anything is launched.
 * pn2_mlp_train_pool_supported: 1 where both directions run (rows and widths as for pn2_mlp_train_ws_bytes, pool_rows
 * 16 or a multiple of 32), else 0. Workspaces: pn2_mlp_train_ws_bytes_pool (group_dims as for pn2_mlp_train_ws_bytes). */
int pn2_mlp_train_pool_supported(long long rows, int nlayers, const int *widths, int pool_rows, int pooling);
long long pn2_mlp_train_ws_bytes_pool(long long rows, int nlayers, const int *widths, int pool_rows, int pooling, int backward,
                                      const int *group_dims, const pn2_train_opts *opts);
int pn2_mlp_train_forward_pool(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                               int pool_rows, int pooling, float *out, int *argsel, float *zsel, float *pool_w, void *ws,
                               const pn2_train_opts *opts, void *stream);
int pn2_mlp_train_backward_pool(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                int pool_rows, int pooling, const float *out, const int *argsel, const float *zsel,
                                const float *pool_w, const float *grad_out, float *grad_feat_rows, float *grad_points,
                                int reproducible, void *ws, const pn2_train_opts *opts, void *stream);

/* The coordinate gradients of the SA training node: what GroupPoint's and GatherPoint's registered gradients carry through
 * grouped_xyz - new_xyz (utils/pointnet_util.py:44-46, :179-180). pn2_mlp_train_backward_xyz takes the arguments of
 * pn2_mlp_train_backward_pool plus grad_xyz (b,n,3) and grad_new_xyz (b,m,3), both WRITTEN (not accumulated): with W1x the
 * three coordinate rows of layers[0]'s weight and dz_1 the gradient at layer 1's pre-norm output,
 *     g_r = dz_1[r,:] . W1x^T,   grad_xyz[i,p] = sum of g_r over the rows that name point p,   grad_new_xyz[i,j] = - sum_k g_(i,j,k)
 * (group_all: grad_xyz[i,k] = g_r). grad_new_xyz is d / d new_xyz alone: the centroids' own dependence on xyz (GatherPoint)
 * is the caller's. Every other result is pn2_mlp_train_backward_pool's; forward is pn2_mlp_train_forward_pool. Passes
 * (csrc/train_mlp_xyz.hip): one over (dy_1, z_1) for the rows g, one over g for the centroids, the 3-channel segmented
 * reduction pn2_group_point_grad_seg for the points (`reproducible` = its sorted-segment mode) -- or, where layer 1 runs once
 * per point, grad_xyz = S . W1x^T from the scattered dz_1 backward holds anyway. A level without features keeps dy_1 and
 * tl_l1_dz_kernel's pass (its moment form never writes dy_1). Both new pointers NULL: pn2_mlp_train_backward_pool exactly.
 * Otherwise, before anything is launched: PN2_E_ARG for pooling 2 (weighted_avg: its weights depend on xyz, and |grouped xyz|
 * has no derivative at the centroid, a member of its own ball) or grad_new_xyz without group->new_xyz; PN2_E_NULL without
 * `group`, without grad_xyz, or with group->new_xyz but no grad_new_xyz. ws: pn2_mlp_train_ws_bytes_xyz bytes (>= the _pool
 * backward workspace; -1 where unsupported). pn2_mlp_train_xyz_supported: 1 where pn2_mlp_train_pool_supported says 1, the
 * pooling is 0, 1 or 3 and group_dims (b, n, m, nsample, cfeat, idx != NULL; NULL = judge the shape alone) fit rows and
 * widths[0] = 3 + cfeat; else 0. */
int pn2_mlp_train_xyz_supported(long long rows, int nlayers, const int *widths, int pool_rows, int pooling, const int *group_dims);
long long pn2_mlp_train_ws_bytes_xyz(long long rows, int nlayers, const int *widths, int pool_rows, int pooling,
                                     const int *group_dims, const pn2_train_opts *opts);
int pn2_mlp_train_backward_xyz(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                               int pool_rows, int pooling, const float *out, const int *argsel, const float *zsel,
                               const float *pool_w, const float *grad_out, float *grad_feat_rows, float *grad_points,
                               float *grad_xyz, float *grad_new_xyz, int reproducible, void *ws, const pn2_train_opts *opts,
                               void *stream);

/* The training node of a feature-propagation level (pointnet_fp_module, utils/pointnet_util.py:211-226) with the interpolation
 * INSIDE it. Layer 1 and three_interpolate are both linear, so
 *     z_1 = [interp(points2), points1] W_1 = interp(points2 W1a) + points1 W1b
 * (W1a: the first c2 input rows of layers[0]'s weight, W1b: the last c1 -- the reference's concat order, :219). Passes
 * (csrc/train_mlp_fp.hip): forward Q = points2 W1a over the b m KNOWN points, z_1 = points1 W1b + (Q[i1] w1 + Q[i2] w2) + Q[i3] w3
 * over the b n rows with its batch moments, layers 2..L as pn2_mlp_train_forward; backward layers L..2 as
 * pn2_mlp_train_backward, then dz_1, S = three_interpolate_grad(dz_1) onto (b m, cout_1) (pn2_three_interpolate_grad_seg;
 * `reproducible` = its sorted-segment mode), dW1a = points2^T S and grad_points2 = S W1a^T over the b m known points,
 * dW1b = points1^T dz_1 and grad_points1 = dz_1 W1b^T over the b n rows. The (b, n, c2 + c1) input and its gradient are never
 * written. weight (b, n, 3): the interpolation weights from dist, bit-identical to pn2_fp_interp_concat's, written by forward
 * and read by backward. layers[0].cin = c2 + c1 (neither needs to be a multiple of 4), weights and grad_weight in the conv
 * layout; b n a multiple of 32; at most 7 layers; pn2_mlp_train_fp_supported says which widths run. grad_points2 /
 * grad_points1: NULL = not wanted. Argument errors return PN2_E_ARG / PN2_E_NULL before anything is launched. */
typedef struct pn2_fp_src {
    int b, n, m, c2, c1;
    const float *points2;          /* (b,m,c2) features of the known points */
    const float *points1;          /* (b,n,c1) skip features; NULL iff c1 == 0 */
    const int *idx;                /* (b,n,3) three_nn's indices */
    const float *dist;             /* (b,n,3) three_nn's squared distances (forward) */
    const void *idx_plan;          /* pn2_three_interpolate_plan(b, n, m, idx, ...) of THIS idx, or NULL: backward reduces from
                                      it (pn2_three_interpolate_grad_planned) instead of inverting idx. The struct gained this
                                      trailing field with the index plans (56 -> 64 bytes): callers MUST zero-initialise
                                      pn2_fp_src (memset / = {0}) before filling it. */
} pn2_fp_src;
int pn2_mlp_train_fp_supported(int b, int n, int m, int c2, int c1, int nlayers, const int *widths /* c2 + c1, cout_1 .. cout_L */);
long long pn2_mlp_train_ws_bytes_fp(int b, int n, int m, int c2, int c1, int nlayers, const int *widths, int backward,
                                    const pn2_train_opts *opts);
int pn2_mlp_train_forward_fp(int nlayers, const pn2_bn_layer *layers, const pn2_fp_src *src, float *out, float *weight, void *ws,
                             const pn2_train_opts *opts, void *stream);
int pn2_mlp_train_backward_fp(int nlayers, const pn2_bn_layer *layers, const pn2_fp_src *src, const float *weight, const float *out,
                              const float *grad_out, float *grad_points2, float *grad_points1, int reproducible, void *ws,
                              const pn2_train_opts *opts, void *stream);

/* The training node with FROZEN batch-norm statistics (csrc/train_mlp_frozen.hip): every layer normalises with its RUNNING
 * statistics (torch.nn.BatchNorm in eval()) -- gradients through a model in eval(), fine-tuning with frozen batch norms.
 * layers[l].running_mean / running_var are REQUIRED (PN2_E_NULL without them) and only read; momentum is ignored. With the
 * stored z = h W (without the conv bias): invstd = 1 / sqrt(running_var + eps), a = gamma invstd, m' = running_mean - bias,
 * c = beta - a m' -- `save` keeps its layout (m', invstd, a, c) -- y = relu(a z + c), dz = a dy, grad_beta = sum dy,
 * grad_gamma = (sum dy z - m' grad_beta) invstd, grad_bias = a grad_beta (NOT zero here: the bias no longer cancels).
 * One entry pair serves grouped rows (group != NULL, x NULL, pool_rows = nsample, pooling 0..3 as
 * pn2_mlp_train_forward_pool) and plain rows (group NULL, x (rows, cin_1), pool_rows 0, pooling 0); the arguments are those
 * of pn2_mlp_train_forward_pool / pn2_mlp_train_backward_xyz plus x / grad_x and
 *   grad_bias: NULL, or nlayers pointers (cout_l each, or NULL) that receive the conv-bias gradients; layers[l].grad_accumulate
 *              applies to them as to the other three.
 * grad_xyz / grad_new_xyz: both NULL or as pn2_mlp_train_backward_xyz (weighted_avg refused with PN2_E_ARG).
 * A layer whose grad_weight, grad_gamma, grad_beta and grad_bias slot are ALL NULL wants no parameter gradient: it runs no
 * weight-gradient pass and sums nothing, and the chain stops at the lowest layer that still needs something (a parameter
 * gradient, or layer 1's input / coordinate gradient). Otherwise grad_weight, grad_gamma and grad_beta must all be given
 * (PN2_E_NULL). Workspaces: pn2_mlp_train_ws_bytes_frozen (want_xyz: backward with the coordinate gradients); where it runs:
 * pn2_mlp_train_frozen_supported (= the _pool / _xyz queries). pn2_train_opts as in the other entries (fold_finalize has
 * nothing to fold and is ignored); `reproducible` likewise. Argument errors return PN2_E_ARG / PN2_E_NULL before anything is
 * launched: pooling outside 0..3, rows not a multiple of 32, group and x both or neither, missing running statistics. */
int pn2_mlp_train_frozen_supported(long long rows, int nlayers, const int *widths, int pool_rows, int pooling,
                                   const int *group_dims, int want_xyz);
long long pn2_mlp_train_ws_bytes_frozen(long long rows, int nlayers, const int *widths, int pool_rows, int pooling, int backward,
                                        const int *group_dims, int want_xyz, const pn2_train_opts *opts);
int pn2_mlp_train_forward_frozen(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                 const float *x, int pool_rows, int pooling, float *out, int *argsel, float *zsel, float *pool_w,
                                 void *ws, const pn2_train_opts *opts, void *stream);
int pn2_mlp_train_backward_frozen(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                  const float *x, int pool_rows, int pooling, const float *out, const int *argsel,
                                  const float *zsel, const float *pool_w, const float *grad_out, float *grad_x,
                                  float *grad_feat_rows, float *grad_points, float *grad_xyz, float *grad_new_xyz,
                                  float *const *grad_bias, int reproducible, void *ws, const pn2_train_opts *opts, void *stream);

/* The training node on the plain rows of a RAGGED batch (csrc/train_mlp_ragged.hip): b clouds padded to n rows each, x and out
 * (b n, C) as in pn2_mlp_train_forward_ex / _backward_ex with group == NULL and pool_rows == 0, and lengths (b) i32 ON THE
 * DEVICE: row c n + i is VALID iff i < clamp(lengths[c], 1, n) (the clamp of the ragged operators above). The batch moments,
 * the running statistics and every gradient are those of the valid rows alone -- what the dense entries compute on the
 * compacted rows. A padding row of x and of grad_out may hold anything, NaN and Inf included: it is never used (selects, not
 * products); out and grad_x are exactly zero (all-zero bits) there, and so is layers[l].z. The host never reads lengths: the
 * calls are stream-ordered, make no host synchronisation and no memset, and can be captured in a graph whose replays see
 * whatever lengths holds then. The row count of the statistics is N_valid = sum of the clamped lengths; the unbiased running
 * variance takes N_valid / max(N_valid - 1, 1). A batch with fewer than 2 valid rows has no variance to speak of (the batch
 * variance is 0, every output is relu(beta)): that is the caller's business, as it is with a dense batch of one row.
 * mask: the caller's buffer of 16 + 4 (b n / 32) bytes, 8-byte aligned, that FORWARD writes (N_valid as a double, then one
 * 32-bit validity word per 32 rows -- a word may hold the tail of one cloud, its padding and the head of the next) and
 * BACKWARD reads: keep it with layers[l].z and save between the two calls. backward takes lengths for symmetry and does not
 * read it.
 * Organisation: the masked passes run one fixed organisation (a data-gradient GEMM and a weight-gradient pass per layer, the
 * finalisations as launches of their own); the pn2_train_opts fields fuse_wgrad, pair_launch, side_stream and fold_finalize
 * are IGNORED, and those that apply to grouped or pooled levels have nothing to act on; the others (force_stream, max_ns, nt,
 * wgrad_two_per_cu) act as in the dense entries. grad_accumulate and running_var_biased likewise. Results are reproducible
 * run to run (fixed summation orders), and with every length equal to n they are the dense entries' results bit for bit
 * (fold_finalize aside, whose sums take another fixed order).
 * _supported: 1 where b n is a positive multiple of 32 below 2^31 and the dense plain-rows node takes the widths (cin_1 and
 * every cout a multiple of 4, 1..8 layers); _ws_bytes_ragged: -1 where it is 0. Before anything is launched: PN2_E_NULL
 * for a NULL lengths or mask (and the dense entries' NULL checks), PN2_E_ARG for b n not a positive multiple of 32 (and the
 * dense entries' argument checks). */
int pn2_mlp_train_ragged_supported(int b, int n, int nlayers, const int *widths);
long long pn2_mlp_train_ws_bytes_ragged(int b, int n, int nlayers, const int *widths, int backward, const pn2_train_opts *opts);
int pn2_mlp_train_forward_ragged(int b, int n, const int *lengths, int nlayers, const pn2_bn_layer *layers, const float *x,
                                 float *out, void *mask, void *ws, const pn2_train_opts *opts, void *stream);
int pn2_mlp_train_backward_ragged(int b, int n, const int *lengths, int nlayers, const pn2_bn_layer *layers, const float *x,
                                  const float *out, const float *grad_out, float *grad_x, const void *mask, void *ws,
                                  const pn2_train_opts *opts, void *stream);

/* The feature-propagation node pn2_mlp_train_*_fp (layer 1 once per KNOWN point, the (b, n, c2 + c1) input never written) with
 * a RAGGED unknown side (csrc/train_mlp_fp.hip): the b n unknown points are b clouds padded to n rows, lengths (b) i32 ON
 * THE DEVICE, row c n + i VALID iff i < clamp(lengths[c], 1, n); the b m known points are dense (a previous level's output).
 * src, out, weight, grad_points2 / grad_points1 and `reproducible` as in pn2_mlp_train_forward_fp / _backward_fp (pn2_fp_src is
 * unchanged); lengths and mask as in pn2_mlp_train_forward_ragged / _backward_ragged: the same buffer of 16 + 4 (b n / 32) bytes,
 * 8-byte aligned, written by forward (N_valid, one validity word per 32 rows), read by backward, to be kept with layers[l].z.
 * The batch moments, the running statistics and every gradient are those of the valid rows alone -- what the dense entries
 * compute on the compacted rows. Two selects beyond the plain-rows ragged node's make a padding row absent: where z_1 is formed
 * (nothing of idx, dist, Q or of the points1 W1b product is used there; z_1 = +0.0, weight = (0, 0, 0), nothing enters the
 * moments) and where dz_1 is formed (+0.0 instead of -c0). A padding row of points1, dist and grad_out may hold anything, NaN
 * and Inf included; out, grad_points1, weight and layers[l].z are all-zero bits there. The known-points half (Q = points2 W1a,
 * dW1a, grad_points2) runs dense; the rows half (dW1b, grad_points1) runs the masked weight-gradient kernel and the masked GEMM.
 * idx ON PADDING ROWS MUST HOLD INDICES IN [0, m): the interpolation gradient reads idx on every row (pn2_three_nn_ragged
 * writes (0, 0, 0) there); with the zero weights those rows add 0 * 0 to known point 0 of their cloud.
 * The host never reads lengths: stream-ordered, no host synchronisation, no memset, capturable in a graph whose replays see
 * whatever lengths holds then. Organisation, pn2_train_opts, grad_accumulate, running_var_biased, reproducibility: as the
 * plain-rows ragged entries; with every length equal to n the results are pn2_mlp_train_*_fp's bit for bit (fold_finalize aside).
 * _supported: 1 where pn2_mlp_train_fp_supported is 1 and b n is a positive multiple of 32; _ws_bytes_fp_ragged: -1 where the
 * dense query is. Before anything is launched: PN2_E_NULL for a NULL lengths (forward) or mask and the dense _fp entries' NULL
 * checks, PN2_E_ARG as the dense _fp entries. backward takes lengths for symmetry and does not read it. */
int pn2_mlp_train_fp_ragged_supported(int b, int n, int m, int c2, int c1, int nlayers, const int *widths);
long long pn2_mlp_train_ws_bytes_fp_ragged(int b, int n, int m, int c2, int c1, int nlayers, const int *widths, int backward,
                                           const pn2_train_opts *opts);
int pn2_mlp_train_forward_fp_ragged(int nlayers, const pn2_bn_layer *layers, const pn2_fp_src *src, const int *lengths, float *out,
                                    float *weight, void *mask, void *ws, const pn2_train_opts *opts, void *stream);
int pn2_mlp_train_backward_fp_ragged(int nlayers, const pn2_bn_layer *layers, const pn2_fp_src *src, const int *lengths,
                                     const float *weight, const float *out, const float *grad_out, float *grad_points2,
                                     float *grad_points1, int reproducible, const void *mask, void *ws, const pn2_train_opts *opts,
                                     void *stream);

/* The training node on the GROUPED rows of a RAGGED batch (csrc/train_mlp_ragged_group.hip): pn2_mlp_train_forward_ex /
 * _backward_ex with a group and the max pool (pool_rows == group->nsample), batch statistics, and counts (b) i32 ON THE DEVICE:
 *   group->idx != NULL   counts[c] = valid centroids of cloud c, clamped into 1..m (the clamp of the _ragged_pair operators): row
 *                        (c, j, k) of the flat order r = (c m + j) nsample + k is VALID iff j < counts[c];
 *   group->idx == NULL   (group_all: m == 1, nsample == n) counts[c] = valid points of cloud c, clamped into 1..n: row (c, 0, k)
 *                        is VALID iff k < counts[c].
 * N_valid = unit * sum of the clamped counts, unit = nsample in the first case, 1 in the second. mask: the buffer of
 * pn2_mlp_train_forward_ragged, 16 + 4 (rows / 32) bytes, 8-byte aligned: forward writes it, backward reads it.
 * The contract is the plain-rows ragged node's: the batch moments, the running statistics and every gradient are those of the
 * valid rows alone, by selects, never by products. Rows of xyz / points beyond a cloud's own points, the rows of a group_all level
 * beyond counts[c] and the grad_out rows of padding groups may hold anything, NaN and Inf included. idx ON PADDING GROUPS MUST HOLD
 * INDICES IN [0, n) (the _ragged_pair operators write 0 there). layers[l].z is all-zero bits on padding rows; out rows of padding
 * groups are all-zero bits and their argsel is 0; grad_feat_rows ((rows, cfeat), the caller scatters it as the dense node's; for
 * group_all it IS the gradient of points) is all-zero bits on padding rows; argsel of a valid group names a valid row of it. There
 * is no zsel. No host synchronisation, no memset; capturable, a replay sees whatever counts holds then; reproducible run to run.
 * Organisation: ONE fixed one (csrc/train_mlp.hip: ragged_group_opts): the plain-rows ragged node's, and of the grouped node's
 * alternative forms none -- layer 1 is the gathered GEMM (tl_gemm_masked_kernel<NS, A_GATHER>) with the gathered masked
 * weight-gradient pass (tl_wgrad_masked_gather_kernel<TPW, UPW>), z_L is always stored (the caller allocates every layers[l].z)
 * and pooled over its valid rows by a vector-unit pass of its own, and backward forms the dense dy_L and runs an unpooled stack. The
 * pn2_train_opts fields top_stored, top_sparse, l1_per_point, l1_coords, fuse_wgrad, pair_launch, side_stream and fold_finalize
 * are IGNORED; force_stream, max_ns, nt and wgrad_two_per_cu act as in the dense entries. With full counts the results agree with
 * the dense node's to rounding, not bit for bit (the dense node pools in the GEMM's epilogue and sums the top gradient per group).
 * Not offered: frozen statistics, coordinate gradients, the pooling modes other than max.
 * _supported: 1 where group_dims {b, n, m, nsample, cfeat, idx != NULL} describe the rows (b m nsample == rows, pool_rows ==
 * nsample, widths[0] == 3 + cfeat, group_all: m == 1 and nsample == n) and pn2_mlp_train_ws_bytes_ex accepts the shape under that
 * organisation in both directions (rows a positive multiple of 32 below 2^31, groups of 16 or a multiple of 32 rows, every cout
 * a multiple of 4, 1..8 layers); _ws_bytes_group_ragged: -1 where it is 0. Before anything is launched: PN2_E_NULL without counts,
 * mask, group or layers (and the dense entries' NULL checks: out, argsel, ws, layers[l].z ...), PN2_E_ARG where _supported says 0
 * (and the dense entries' argument checks). backward takes counts for symmetry and does not read it. */
int pn2_mlp_train_group_ragged_supported(long long rows, int nlayers, const int *widths, int pool_rows, const int *group_dims);
long long pn2_mlp_train_ws_bytes_group_ragged(long long rows, int nlayers, const int *widths, int pool_rows, int backward,
                                              const int *group_dims, const pn2_train_opts *opts);
int pn2_mlp_train_forward_group_ragged(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                       int pool_rows, const int *counts, float *out, int *argsel, void *mask, void *ws,
                                       const pn2_train_opts *opts, void *stream);
int pn2_mlp_train_backward_group_ragged(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                        int pool_rows, const int *counts, const float *out, const int *argsel,
                                        const float *grad_out, float *grad_feat_rows, int reproducible, const void *mask,
                                        void *ws, const pn2_train_opts *opts, void *stream);
/* ... and what one such call launches on the matrix cores, as pn2_mlp_train_ragged_plan below (records of
 * PN2_RAGGED_PLAN_FIELDS ints): forward layer 1 is the masked gathered GEMM ([8] AMODE 1 = A_GATHER), backward layer 1 the gathered
 * masked weight-gradient pass ([3] = 2: tl_wgrad_masked_gather_kernel<TPW, UPW>; shaped by wgrad_shape with gather) and, with
 * cfeat > 0, the masked A_DZ GEMM onto the cfeat feature columns. The pool and its gradient are vector-unit passes, not listed. */
int pn2_mlp_train_group_ragged_plan(long long rows, int nlayers, const int *widths, int pool_rows, const int *group_dims,
                                    const pn2_train_opts *opts, int *passes, int cap);

/* What a ragged training call launches on the matrix cores: host logic, no device work (tests, maintainers). The two entries
 * take the arguments of pn2_mlp_train_ws_bytes_ragged / _ws_bytes_fp_ragged without `backward` and describe BOTH directions of
 * one call that wants every gradient (grad_x; grad_points2 and grad_points1), in launch order: forward layers 1..L, then
 * backward layers L..1, per layer the weight-gradient pass before the data-gradient GEMM. They evaluate the size rules the
 * launches evaluate (csrc/train_mlp.hip: ragged_opts, gemm_shape, wgrad_shape, the GEMM's grid and nt rule), so a record names
 * the kernel instantiation that pass runs. passes: cap records of PN2_RAGGED_PLAN_FIELDS ints each, or NULL to count; returns
 * the number of passes (records beyond cap are not written), or PN2_E_ARG where the _supported query says 0, PN2_E_NULL
 * without widths. A record:
 *   [0] kind: 0 = GEMM (tl_gemm_masked_kernel<NS, AMODE> when masked, else tl_gemm_kernel), 1 = weight-gradient pass
 *       (tl_wgrad_masked_kernel<TPW, UPW> when masked, else tl_wgrad_kernel)
 *   [1] 0 forward, 1 backward   [2] layer, 1-based   [3] 1: the masked kernel, 0: the dense one (2: the gathered masked
 *       weight-gradient pass, pn2_mlp_train_group_ragged_plan only)   [4] rows
 *   [5] K, [6] N: GEMM: contraction and output channels as the shape rule gets them; weight gradient: input and output channels
 *   GEMM:            [7] NS  [8] AMODE (0 A_PLAIN, 1 A_GATHER, 2 A_RELU, 3 A_DZ)  [9] 1 resident weights, 0 streamed  [10] column slabs
 *                    [11] 1: non-temporal stores (opts.nt, else from 128 MB of output)  [12] grid x  [13] 0
 *   weight gradient: [7] TPW [8] UPW  [9] `two` (two workgroups per CU)  [10] slabs (input slabs x output slabs)
 *                    [11] input tiles per slab  [12] grid x  [13] output tiles per slab
 * The FP node's vector-unit passes (z_1 and dz_1 with the mask, the interpolation gradient) and the per-channel finalisations are
 * not listed; its layer 1 appears as its two halves: the known-points half (forward Q = points2 W1a; backward dW1a and
 * grad_points2, b m rows rounded up to 32) with [3] = 0, the rows half (forward points1 W1b, a dense store GEMM, [3] = 0;
 * backward dW1b and grad_points1, [3] = 1) -- absent with c1 = 0.
 * NS, AMODE, residency, slabs, nt, TPW and UPW depend on the shape and opts alone. `two` and grid x of a weight-gradient pass
 * depend on the CU count of the current device, which is taken as 256 where there is no device: do not rely on them there. */
#define PN2_RAGGED_PLAN_FIELDS 14
int pn2_mlp_train_ragged_plan(int b, int n, int nlayers, const int *widths, const pn2_train_opts *opts, int *passes, int cap);
int pn2_mlp_train_fp_ragged_plan(int b, int n, int m, int c2, int c1, int nlayers, const int *widths, const pn2_train_opts *opts,
                                 int *passes, int cap);

/* The input rows of a feature-propagation level's layer stack in ONE launch (pointnet_fp_module, utils/pointnet_util.py:211-219):
 * inverse-distance weights from three_nn's `dist`, three_interpolate of points2 (b,m,c2), concatenation with the skip features
 * points1 (b,n,c1; NULL with c1 = 0), zero columns up to `pitch` (a multiple of 4 >= c2 + c1: the training entry points read
 * rows 16 bytes at a time) -> out (b,n,pitch); weight (b,n,3) receives the weights (needed by the gradient) unless NULL.
 * The operators' formulas in IEEE fp32 (agreement with the composition of torch elementwise kernels + pn2_three_interpolate:
 * 2e-6 of the tensor's scale, tests/test_fp_train_gpu.py). The gradient call splits the stack's input
 * gradient grad_x (b,n,pitch) into grad_points1 (b,n,c1; may be NULL) and the interpolated part (scratch, (b,n,c2) floats),
 * which pn2_three_interpolate_grad_seg scatters onto grad_points2 (b,m,c2) (ws_seg: pn2_seg_grad_ws_bytes(b, m, 3 n)). */
int pn2_fp_interp_concat(int b, int n, int m, int c2, int c1, int pitch, const float *points2, const float *points1,
                         const int *idx, const float *dist, float *out, float *weight, void *stream);
int pn2_fp_interp_concat_grad(int b, int n, int m, int c2, int c1, int pitch, const float *grad_x, const int *idx,
                              const float *weight, float *grad_points2, float *grad_points1, float *scratch, void *ws_seg,
                              int deterministic, void *stream);
/* the same from an index plan of idx (pn2_three_interpolate_plan(b, n, m, idx, ...)) in place of idx and ws_seg */
int pn2_fp_interp_concat_grad_planned(int b, int n, int m, int c2, int c1, int pitch, const float *grad_x, const void *plan,
                                      const float *weight, float *grad_points2, float *grad_points1, float *scratch,
                                      int deterministic, void *stream);

/* diagnostics: byte offsets inside the BACKWARD workspace of the two dy buffers ((rows, max width) each; after a
 * backward of L layers they hold dy_{L-1}, dy_{L-2}, ... alternately, starting with gb when pooled) and of the
 * per-layer (2, cout) fp64 sums / (3, cout) fp32 coefficients */
int pn2_mlp_train_ws_layout(long long rows, int nlayers, const int *widths, int pool_rows, long long *ga, long long *gb,
                            long long *stats, long long *coef);

/* ---- host helpers ------------------------------------------------------- */

/* The exact fp32 threshold s* with  max(sqrtf(s),1e-20f) < radius  <=>  s < s*
 * (host computation, monotonicity of correctly-rounded sqrtf). Exposed for tests. */
float pn2_ball_threshold(float radius);

#ifdef __cplusplus
}
#endif
#endif /* PN2OPS_H */
