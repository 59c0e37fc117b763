// train_mlp.hip -- TRAINING mode of the shared MLPs of a set-abstraction / feature-propagation level on the matrix
// cores (second half). gfx950.
//
// Reference: utils/pointnet_util.py:113-127 (SA: 3 x [conv2d 1x1 + batch_norm + ReLU], reduce_max over nsample),
// :222-226 (FP: the same stack without the pool), tf_util.py:512-531 (batch moments, eps 1e-3, moving averages),
// train.py:96-104 (bn_decay), train.py:188 (is_training = True: the reference's main mode).
//
// Why this is not the inference kernel with one more flag. Batch statistics couple ALL rows of a level: layer l's
// normalisation needs the moments of z_l over every row before layer l+1 can start, and the backward pass has the
// same coupling in the other direction (dz = s dy - c0 - c1 z with c0, c1 from two per-channel sums over all rows).
// So a level is a SEQUENCE of passes with a per-channel reduction between them, and each pass is one GEMM over
// the rows with everything elementwise folded into its prologue and epilogue. The pre-norm tensors z_l are the only
// activations kept in HBM (plain row-major (rows, C) fp32, the caller's buffers); h_l = relu(a z + c), the
// grouped input, dz, the ReLU masks and the normalised tensors never exist in memory.
//
// One GEMM core serves every pass (tl_gemm_kernel): a wave owns 32 rows and NS 32-column output tiles,
//     D (32 rows x 32 cols) += A (32 rows x 16 k) . B (16 k x 32 cols)      v_mfma_f32_32x32x16_bf16
//   A operand = the wave's rows: lane l supplies row l & 31, contraction indices 32u + 16e + 8(l >> 5) + j, j = 0..7,
//               i.e. 32 contiguous bytes of a row-major row -- read straight from HBM (two dwordx4), transformed by
//               the pass's prologue, split into three bf16 levels (sa_mlp_common.h: fp32 products as six bf16 terms);
//   B operand = weights, packed ON THE DEVICE each step (they change with every optimiser step) into the same
//               three-level operand layout, staged through LDS (all k tiles resident when they fit, else a
//               double-buffered stream of one k tile per stage, one s_barrier per stage);
//   C/D: lane l holds column l & 31 for the 16 rows 8(v >> 2) + 4(l >> 5) + (v & 3): per-channel work of the epilogue
//        (bias, batch moments, max / min pool, ReLU mask of the layer below, batch-norm backward sums) is lane-local,
//        and a row's 32 columns leave as one 128-byte store.
// The weight gradient contracts over ROWS (tl_wgrad_kernel): both operands are read with lane = channel, slots = rows
// (coalesced 128-byte row segments), each wave accumulates its share of the rows into a register-resident dW slab,
// and a two-stage reduction sums the waves' slabs (fp64 in the last stage) in a fixed order: the result does not
// depend on timing.
//
// Where things are. This file is the HOST side of the node: the size rules and the plan of a level's workspace, the two
// directions (Fwd, Bwd) as sequences of launches, and the C entry points. The kernels live one family per translation unit,
// each with its launch function(s), declared in train_mlp_kernels.h together with the parameter structs filled here:
//     train_mlp_gemm.hip   tl_gemm_kernel (body: tl_gemm_body.inc), tl_pack_kernel
//     train_mlp_wgrad.hip  tl_wgrad_kernel (body: tl_wgrad_body.inc), the reductions of its partial sums
//     train_mlp_pair.hip   tl_pair_kernel: both bodies in one launch
//     train_mlp_top.hip    the pooled top layer without its pre-norm tensor (tl_top_*)
//     train_mlp_l1.hip     layer 1 of a grouped level on the vector units (tl_l1_*)
//     train_mlp_small.hip  per-channel finalisations, the top of the stack, the pooling modes
// train_mlp_device.h is the device code they share; train_mlp_fp / _xyz / _frozen.hip hold the entry points and kernels of
// one node type each (train_mlp_internal.h); train_mlp_ragged.hip the plain rows of a ragged batch, train_mlp_ragged_group.hip
// its grouped rows (the masked gathered passes of layer 1; the pool over the valid rows is train_mlp_small.hip's). A kernel that takes a row mask
// stands beside its dense twin; here c.mask only selects an ARGUMENT (mask_words(), row_count()), the launch function the kernel.
#include "train_mlp_kernels.h"    // the parameter structs and launches of the kernels; TlCall, the shape structs (train_mlp_internal.h)

#include <string.h>

namespace pn2 {

// ---- the size rules and the plan ----------------------------------------------------------------------------------------------
static inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
static inline int tiles(int c) { return (c + 31) / 32; }
static inline Opts opts_of(const pn2_train_opts *o)
{
    Opts d;
    memset(&d, 0, sizeof(d));
    return o ? *o : d;
}
// The rows of a ragged batch (TlCall::mask, train_mlp_ragged.hip) run ONE organisation: a data-gradient GEMM and a weight-gradient
// pass per layer, every finalisation a launch of its own -- the masked kernels exist for those passes only. The other fields
// keep the caller's values.
static inline Opts ragged_opts(const pn2_train_opts *o)
{
    Opts d = opts_of(o);
    d.fuse_wgrad = PN2_OPT_OFF; d.pair_launch = PN2_OPT_OFF; d.side_stream = PN2_OPT_OFF; d.fold_finalize = PN2_OPT_OFF;
    return d;
}
// The GROUPED rows of a ragged batch (TlCall::mask with a group, train_mlp_ragged_group.hip): ragged_opts, and of the grouped
// node's alternative forms none -- z_L is always kept and pooled by a pass of its own, layer 1 is always the gathered GEMM with
// the gathered weight-gradient pass: the only forms that have a masked kernel.
static inline Opts ragged_group_opts(const pn2_train_opts *o)
{
    Opts d = ragged_opts(o);
    d.top_stored = PN2_OPT_ON; d.top_sparse = PN2_OPT_OFF; d.l1_per_point = PN2_OPT_OFF; d.l1_coords = PN2_OPT_OFF;
    return d;
}
static inline int pick_ns(int tn, const Opts &o)
{
    const int cap = (o.max_ns == 1 || o.max_ns == 2) ? o.max_ns : 4;      // results never depend on it
    const int ns = tn >= 3 ? 4 : tn == 2 ? 2 : 1;
    return ns > cap ? cap : ns;
}
// CUs of the current device (partition modes expose fewer than 256); 256 when there is no device (host-side queries)
static inline int device_cus()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0) {
        (void)hipGetLastError();
        return 256;
    }
    return cus > 256 ? 256 : cus;
}

static GemmShape gemm_shape(long long rows, int K, int N, const Opts &o)
{
    GemmShape g;
    g.K = K; g.N = N;
    g.tk = tiles(K); g.tn = tiles(N);
    g.ns = pick_ns(g.tn, o);
    g.slabs = (g.tn + g.ns - 1) / g.ns;
    // few rows (group_all, the deep levels of the segmentation nets): a workgroup covers 256 rows of one column slab, so
    // narrower slabs are what spreads the pass over the chip -- the rows are re-read per slab, which is nothing here
    const long long rounds = (rows / 32 + kTlWaves - 1) / kTlWaves;
    while (g.ns > 1 && rounds * g.slabs < 128) {
        g.ns /= 2;
        g.slabs = (g.tn + g.ns - 1) / g.ns;
    }
    const size_t params = (size_t)3 * g.tk * 32 * sizeof(float), stage = (size_t)g.ns * kPairWords * 4;
    g.resident = params + stage * g.tk <= (size_t)144 * 1024 && o.force_stream != PN2_OPT_ON;
    g.lds = params + stage * (g.resident ? g.tk : 2);
    g.pack_bytes = (size_t)g.slabs * g.tk * g.ns * kPairWords * 4;
    return g;
}

static WgradShape wgrad_shape(long long rows, int KI, int NO, bool gather = false, int cus = 256, int two_opt = PN2_OPT_AUTO)
{
    WgradShape w;
    const int tu = tiles(KI), tt = tiles(NO);
    w.tus = tu < 4 ? tu : 4;
    w.tts = tt < 8 ? tt : 8;
    if (gather && tu > 4 && tu <= 6) {
        // layer 1 of an SA level with features (131 / 134 input channels = five tiles): the grouped input is gathered from
        // an L2-resident tensor and cheap to read again, dz is not -- so ALL input tiles sit in one slab and dz is cut into
        // slabs of two tiles, each read once (with the 4 + 8 shape dz crossed HBM twice). Two units and two tiles per wave.
        w.tus = tu;
        w.tts = tt < 2 ? tt : 2;
    }
    // few rows: more, smaller slabs spread the pass over the chip (each slab re-reads the rows, which is nothing here)
    while ((long long)((tu + w.tus - 1) / w.tus) * ((tt + w.tts - 1) / w.tts) * ((rows / 32 + 3) / 4) < 64 && (w.tus > 1 || w.tts > 1)) {
        if (w.tts >= w.tus && w.tts > 1) w.tts = (w.tts + 1) / 2; else w.tus = (w.tus + 1) / 2;
    }
    w.uslabs = (tu + w.tus - 1) / w.tus;
    w.tslabs = (tt + w.tts - 1) / w.tts;
    const int nout = w.tus * w.tts, per = (nout + 7) / 8;
    w.tpw = per <= 1 ? 1 : per <= 2 ? 2 : 4;
    w.upw = (2 * (w.tus + w.tts) + 7) / 8;
    const size_t slabs = (size_t)w.uslabs * w.tslabs;
    const long long blocks = rows / 32;
    long long gx = cus / (long long)slabs;                         // one workgroup per CU over all slabs ...
    // ... or TWO where a second one fits beside the first (<= 128 registers: one output tile and at most two units per wave,
    // no gather; half the LDS): these passes run one barrier per 32-row block with little work behind it, and a second
    // workgroup fills the waits of the first
    // (measured, scripts/lab_ab.sh wgrad_two_per_cu: Gram pass 173 -> 124 us, layer-2 weight gradient 171 -> 140 us at the metric
    // shape; nothing to gain below ~16 row blocks per workgroup, where the passes are a few microseconds of launch latency)
    w.two = two_opt != PN2_OPT_OFF && w.tpw == 1 && w.upw <= 2 && !gather && (size_t)2 * (w.tus + w.tts) * 6144 <= (size_t)76 * 1024 &&
            (two_opt == PN2_OPT_ON || blocks >= 16ll * cus);
    if (w.two) gx *= 2;
    if (gx < 1) gx = 1;
    if (gx > (blocks + 3) / 4) gx = (blocks + 3) / 4;               // at least four row blocks per workgroup
    w.gridx = gx;
    w.nw = gx;
    w.e = (size_t)nout * 1024;
    w.lds = (size_t)2 * (w.tus + w.tts) * 6144;
    w.lds_dy = 0;
    w.nchunks = w.nw > 32 ? (w.nw + 31) / 32 : 0;
    w.partial_bytes = slabs * w.nw * w.e * sizeof(float);
    return w;
}

// Can the layer's data gradient ride in its weight-gradient pass (tl_wgrad_kernel<.., DY>)? One slab (every tile of both
// operands in the block image), at most four output tiles and two dW tiles per wave, and image(s) + resident W^T within the
// CU's LDS -- with ONE image and two barriers per block when two do not fit. kc: channels of the contraction (= the second
// operand's tiles that enter the product), ki: output columns.
static FuseShape fuse_shape(long long rows, const WgradShape &w, int kc, int ki, const Opts &o, bool dense = true)
{
    FuseShape f;
    memset(&f, 0, sizeof(f));
    if (o.fuse_wgrad == PN2_OPT_OFF || w.uslabs != 1 || w.tslabs != 1 || w.tpw > 2) return f;
    // measured (scripts/lab_ab.sh fuse_wgrad): -7 % of a level's backward at 1 M rows (-25 % of the layer's two passes), -4 % at
    // 0.5 M, nothing below -- there the passes are latency-bound and the resident W^T costs its load per workgroup
    if (o.fuse_wgrad == PN2_OPT_AUTO && rows < (1ll << 19)) return f;
    f.tk = tiles(kc); f.nt = tiles(ki);
    if (f.nt > 4 || f.tk > 8) return f;
    f.upw = w.upw;
    f.acopy = dense ? 1 : 0;                                       // dense second operand: its fragments also in the data gradient's layout
    const size_t img = (size_t)(w.tus + w.tts + (f.acopy ? f.tk : 0)) * 6144 + (size_t)32 * (w.tus * 32 + 2) * 4;      // operand fragments + the raw rows of the layer below
    const size_t wb = (size_t)f.tk * f.nt * kPairWords * 4;
    const size_t cap = (size_t)156 * 1024;
    if (2 * img + wb <= cap) f.single = 0;
    else if (img + wb <= cap) f.single = 1;
    else return f;
    f.xr_off = (f.single ? img : 2 * img) + wb;                   // 2 x 32 coordinate rows behind everything else
    f.lds = f.xr_off + 1024;
    f.pack_bytes = wb;
    f.ok = true;
    return f;
}

struct TlPlan {
    size_t pack[8];             // forward: W_l; backward: W_l^T
    size_t stats[8];            // (2, cout_l) doubles
    size_t coef[8];             // backward: (3, cout_l) floats
    size_t pool;                // forward: pmax, pamax (2 arrays of parts_total x cout_L)
    size_t gq;                  // backward, pooled: (groups, cout_L)
    size_t ga, gb;              // backward: dy ping-pong (rows, max width)
    size_t partial;             // backward: weight-gradient partial sums
    size_t partial_cap;         // ... and the bytes planned for them (launch_wgrad / launch_pair refuse a larger shape)
    size_t topw, topsf;         // backward, pooled top layer without z_L: stacked fp32 weight + constant row; [S | G | sumh] fp64
    size_t tops_part, tops_part2, tops64;   // ... its routed part on the vector units: partials (two stages), S (K, C_L) fp64
    size_t l1p;                 // layer 1 per point: forward P (b n, cout_1); backward S (b n, cout_1)
    size_t l1seg, l1part, l1coef;   // backward: scratch of the segmented reduction, dW1x partials (256, 3, cout_1), identity coefficients
    size_t l1xg, l1mom, l1a;        // backward, level without features: centred coordinates of every row, their moments, x^T dy_1 partials
    size_t fpw, fp2, fp1, fpg2;     // FP level (FpL1): W1b's operand tiles, zero-padded points2 / points1, grad_points2 staged
    size_t tickets;             // kFinTickets counters of the folded finalisations (TlFin), zeroed by the direction's pack launch
    size_t total;
};

// Is the pooled top layer's pre-norm tensor z_L kept (small levels), or are the passes that would read it rewritten in
// terms of the layer's input (tl_top_mats_kernel)? One rule for forward, backward and the caller's allocation.
static bool top_stored(long long rows, int nlayers, const int *widths, int pool_rows, const Opts &o)
{
    if (!pool_rows || nlayers < 2) return true;
    if (o.top_stored != PN2_OPT_AUTO) return o.top_stored == PN2_OPT_ON;
    return (size_t)rows * widths[nlayers] * sizeof(float) < ((size_t)32 << 20);
}
static inline int top_cols(int kin, int cl) { return tiles(cl) * 32 + tiles(kin) * 32 + 32; }

// the workspace behind TlPlan::total when the coordinate gradients are wanted: g (rows, 3) of a level with idx, then the scratch
// of its segmented reduction (not where layer 1 runs per point: grad_xyz comes from S there)
struct XyzPlan { size_t g, seg, total; };

// Is layer 1 of this grouped level evaluated once per POINT (tl_l1_forward_kernel)? One rule for forward, backward, the
// workspace sizes and the caller's allocation of the feature gradient.
static bool l1_per_point(int nlayers, const int *widths, const GroupDims *g, const Opts &o)
{
    if (!g || !g->has_idx || nlayers < 2 || o.l1_per_point == PN2_OPT_OFF) return false;
    const int c1 = widths[1];
    if (g->cfeat < 8 || g->cfeat % 4 || ((long long)g->b * g->n) % 32 || c1 % 4 || c1 / 4 > 256 || 256 % (c1 / 4)) return false;
    return widths[0] == 3 + g->cfeat;
}

static TopSShape top_s_shape(long long rows, int pool_rows, int K, int NF, const Opts &o)
{
    TopSShape t;
    memset(&t, 0, sizeof(t));
    if (!pool_rows || K % 4) return t;
    {
        // measured (scripts/lab_ab.sh PN2_TL_TOP_SPARSE): 3-12 % of a level's backward from 0.26 M rows x 128 inputs up,
        // nothing or a few microseconds lost below (sem_seg's levels) -- there the extra launches cost what the tiles saved
        if (o.top_sparse == PN2_OPT_OFF || (o.top_sparse == PN2_OPT_AUTO && rows * K < (1ll << 24))) return t;
    }
    const long long per_group = (long long)pool_rows * K;           // floats of one group's input rows
    if (per_group > 16384) return t;                               // eight 16-byte loads per thread at most
    t.ld = K + 4;                                                  // rows 16 bytes apart in the banks
    const size_t group_lds = (size_t)pool_rows * t.ld * 4;
    int gb = (int)(8192 / per_group);                              // four loads per thread when a group allows (registers: two
    if (gb < 1) gb = 1;                                            // workgroups per CU), eight for the largest groups
    if (gb > kTopSGroups) gb = kTopSGroups;
    while (gb > 1 && (size_t)gb * group_lds > ((size_t)64 << 10)) --gb;
    t.GB = gb;
    t.lds = (size_t)2 * K * 4 + (size_t)gb * group_lds;
    if (t.lds > ((size_t)144 << 10)) return t;
    const int per_thread = (int)((gb * per_group / 4 + kTopSThreads - 1) / kTopSThreads);
    t.NLD = per_thread <= 1 ? 1 : per_thread <= 2 ? 2 : per_thread <= 4 ? 4 : 8;
    const int nchunk = (NF + 63) / 64;
    t.KC = 4;
    for (int kc = 64; kc >= 4; kc /= 2)                            // the widest strip of inputs that still gives eight waves work
        if (K % kc == 0 && nchunk * (K / kc) >= 6) { t.KC = kc; break; }
    const int items = nchunk * (K / t.KC);
    t.gridy = (items + 7) / 8;
    const long long groups = rows / pool_rows, nb = (groups + gb - 1) / gb;
    long long gx = ((long long)32 << 20) / ((long long)K * NF * 4);  // at most 32 MB of partial sums ...
    if (gx < 128) gx = 128;                                        // ... but half the chip at least
    if (gx > 512) gx = 512;
    if (gx > nb) gx = nb;
    t.gridx = (int)gx;
    t.nchunks = gx > 32 ? (int)((gx + 31) / 32) : 0;
    t.part_bytes = (size_t)gx * K * NF * 4;
    t.part2_bytes = (size_t)t.nchunks * K * NF * 4;
    t.ok = true;
    return t;
}

// Is this a grouped level WITHOUT features whose first layer (a contraction of the three coordinates) runs on the vector
// units (tl_l1_forward_kernel with P == nullptr, tl_l1_dz_kernel<false>)? The first level of every reference network.
static bool l1_coords_only(int nlayers, const int *widths, const GroupDims *g, const Opts &o)
{
    // (round 4: also with up to kL1MaxFeat feature channels beside the coordinates -- normals -- gathered per row)
    if (!g || !g->has_idx || g->cfeat > kL1MaxFeat || widths[0] != 3 + g->cfeat || nlayers < 2 || o.l1_coords == PN2_OPT_OFF) return false;
    const int c1 = widths[1];
    return c1 % 4 == 0 && c1 / 4 <= kL1Threads && kL1Threads % (c1 / 4) == 0;
}

// The weight-gradient launch's slab shape AS PLANNED: the launches call wgrad_shape with the device's CU count (<= 256,
// device_cus) and the caller's wgrad_two_per_cu, both of which can only make the grid -- hence the `partial` buffers --
// SMALLER than 256 CUs with two workgroups per CU wherever the shape allows them (planned with the
// defaults, an opted-in second workgroup or a 129..255-CU device wrote its slabs past the planned buffer).
static WgradShape wgrad_plan_shape(long long rows, int KI, int NO, bool gather, const Opts &o)
{
    return wgrad_shape(rows, KI, NO, gather, 256, o.wgrad_two_per_cu == PN2_OPT_OFF ? PN2_OPT_OFF : PN2_OPT_ON);
}

static bool tl_plan(long long rows, int nlayers, const int *widths, int pool_rows, int backward, TlPlan &pl,
                    const GroupDims *gd, const Opts &o, const FpL1 *fp = nullptr)
{
    if (rows <= 0 || rows % 32 || rows >= (1ll << 31) || nlayers < 1 || nlayers > 8) return false;
    if (pool_rows && pool_rows != 16 && pool_rows % 32) return false;
    memset(&pl, 0, sizeof(pl));
    size_t off = 0;
    int maxw = 0;
    for (int l = 0; l < nlayers; ++l) {
        const int cin = widths[l], cout = widths[l + 1];
        if (cin <= 0 || cout <= 0 || cout % 4) return false;
        const bool ztop = backward && l == nlayers - 1 && !top_stored(rows, nlayers, widths, pool_rows, o);
        const GemmShape g = ztop ? gemm_shape(rows, tiles(cout) * 32 + cin, cin, o) : backward ? gemm_shape(rows, cout, cin, o) : gemm_shape(rows, cin, cout, o);
        size_t pb = g.pack_bytes;
        if (l == 0 && l1_per_point(nlayers, widths, gd, o)) {           // the per-point GEMMs' operand tiles instead
            const long long bn = (long long)gd->b * gd->n;
            const GemmShape gp = backward ? gemm_shape(bn, cout, gd->cfeat, o) : gemm_shape(bn, gd->cfeat, cout, o);
            if (gp.pack_bytes > pb) pb = gp.pack_bytes;
        }
        if (l == 0 && fp) {                                          // W1a's tiles for the GEMMs over the known points
            const GemmShape ga = backward ? gemm_shape(fp->mp, cout, fp->c2, o) : gemm_shape(fp->mp, fp->c2p, cout, o);
            if (ga.pack_bytes > pb) pb = ga.pack_bytes;
        }
        pl.pack[l] = off; off = align_up(off + pb);
        pl.stats[l] = off; off = align_up(off + sizeof(double) * 2 * cout * kMaxParts);
        if (backward) { pl.coef[l] = off; off = align_up(off + sizeof(float) * 3 * cout); }
        if (cout > maxw) maxw = cout;
    }
    const int cl = widths[nlayers];
    if (!backward) {
        if (pool_rows) {
            const long long parts = rows / (pool_rows == 16 ? 16 : 32);
            pl.pool = off; off = align_up(off + (size_t)2 * parts * cl * 4);
        }
    } else {
        if (pool_rows) { pl.gq = off; off = align_up(off + (size_t)(rows / pool_rows) * cl * 4); }
        pl.ga = off; off = align_up(off + (size_t)rows * maxw * 4);
        pl.gb = off; off = align_up(off + (size_t)rows * maxw * 4);
        size_t p1 = 0;
        const bool ztop = !top_stored(rows, nlayers, widths, pool_rows, o);
        for (int l = 0; l < nlayers; ++l) {
            const bool zt = ztop && l == nlayers - 1;
            for (int gat = 0; gat < (l == 0 ? 2 : 1); ++gat) {      // layer 1 may be a gathered input (other slab shape)
                const WgradShape w = wgrad_plan_shape(rows, widths[l], zt ? top_cols(widths[l], widths[l + 1]) : widths[l + 1], gat != 0, o);
                if (w.partial_bytes > p1) p1 = w.partial_bytes;
            }
            if (zt) {                                              // without the routed tiles (tl_top_s_kernel takes them)
                const WgradShape w = wgrad_plan_shape(rows, widths[l], top_cols(widths[l], 0), false, o);
                if (w.partial_bytes > p1) p1 = w.partial_bytes;
            }
        }
        if (l1_per_point(nlayers, widths, gd, o)) {                  // dW1f = points^T S over the b n points
            const WgradShape w = wgrad_plan_shape((long long)gd->b * gd->n, gd->cfeat, widths[1], false, o);
            if (w.partial_bytes > p1) p1 = w.partial_bytes;
        }
        if (fp) {                                                    // dW1a over the known points, dW1b over the rows
            for (int h = 0; h < 2; ++h) {
                if (h == 1 && fp->c1 == 0) break;
                const WgradShape w = h == 0 ? wgrad_plan_shape(fp->mp, fp->c2p, widths[1], false, o)
                                            : wgrad_plan_shape(rows, fp->c1p, widths[1], false, o);
                if (w.partial_bytes > p1) p1 = w.partial_bytes;
            }
        }
        pl.partial = off; off = align_up(off + p1);
        pl.partial_cap = p1;
        if (ztop) {
            const int kin = widths[nlayers - 1];
            pl.topw = off; off = align_up(off + sizeof(float) * (size_t)(tiles(cl) * 32 + kin + 1) * kin);
            pl.topsf = off; off = align_up(off + sizeof(double) * (size_t)kin * top_cols(kin, cl));
            const TopSShape ts = top_s_shape(rows, pool_rows, kin, cl, o);
            if (ts.ok) {
                pl.tops_part = off; off = align_up(off + ts.part_bytes);
                pl.tops_part2 = off; off = align_up(off + ts.part2_bytes);
                pl.tops64 = off; off = align_up(off + sizeof(double) * (size_t)kin * cl);
            }
        }
    }
    if (l1_per_point(nlayers, widths, gd, o)) {
        const long long bn = (long long)gd->b * gd->n;
        pl.l1p = off; off = align_up(off + (size_t)bn * widths[1] * 4);
        if (backward) {
            pl.l1seg = off; off = align_up(off + (size_t)pn2_seg_grad_ws_bytes(gd->b, gd->n, (long long)gd->m * gd->nsample));
            pl.l1part = off; off = align_up(off + (size_t)kMaxParts * 3 * widths[1] * 4);
            pl.l1coef = off; off = align_up(off + (size_t)3 * widths[1] * 4);
        }
    } else if (backward && l1_coords_only(nlayers, widths, gd, o)) {
        pl.l1part = off; off = align_up(off + (size_t)kMaxParts * (3 + kL1MaxFeat) * widths[1] * 4);
        pl.l1xg = off; off = align_up(off + (size_t)rows * 16);
        pl.l1mom = off; off = align_up(off + (size_t)kMaxParts * 9 * sizeof(double));
        pl.l1a = off; off = align_up(off + (size_t)kMaxParts * 3 * widths[1] * sizeof(double));
    }
    if (fp) {
        const int C1 = widths[1];
        pl.l1p = off; off = align_up(off + (size_t)fp->mp * C1 * 4);              // forward Q, backward S: (mp, C1)
        if (fp->c1 > 0) {
            const size_t wb = backward ? gemm_shape(rows, C1, fp->c1, o).pack_bytes : gemm_shape(rows, fp->c1p, C1, o).pack_bytes;
            pl.fpw = off; off = align_up(off + wb);
        }
        if (fp->pad2()) { pl.fp2 = off; off = align_up(off + (size_t)fp->mp * fp->c2p * 4); }
        if (fp->pad1()) { pl.fp1 = off; off = align_up(off + (size_t)rows * fp->c1p * 4); }
        if (backward) {
            const long long sb = pn2_seg_grad_ws_bytes(fp->b, fp->m, 3ll * fp->n);
            if (sb < 0) return false;
            pl.l1seg = off; off = align_up(off + (size_t)sb);
            pl.l1coef = off; off = align_up(off + (size_t)3 * C1 * 4);
            if (fp->gstage2()) { pl.fpg2 = off; off = align_up(off + (size_t)fp->mp * fp->c2 * 4); }
        }
    }
    pl.tickets = off; off = align_up(off + sizeof(unsigned) * kFinTickets);
    pl.total = off;
    return true;
}

static bool xyz_plan(const TlPlan &pl, long long rows, int nlayers, const int *widths, const GroupDims &gd, const Opts &o, XyzPlan &x)
{
    size_t off = pl.total;
    x.g = x.seg = off;
    if (gd.has_idx) {
        off = align_up(off + (size_t)rows * 3 * sizeof(float));
        x.seg = off;
        if (!l1_per_point(nlayers, widths, &gd, o)) {
            const long long sb = pn2_seg_grad_ws_bytes(gd.b, gd.n, (long long)gd.m * gd.nsample);
            if (sb < 0) return false;
            off = align_up(off + (size_t)sb);
        }
    }
    x.total = off;
    return true;
}

static GroupDims group_dims(const pn2_group_src *g)
{
    GroupDims d = {g->b, g->n, g->m, g->nsample, g->points ? g->cfeat : 0, g->idx ? 1 : 0};
    return d;
}

TlGather make_gather(const pn2_group_src *g)
{
    TlGather t;
    t.n = g->n; t.m = g->m; t.nsample = g->nsample; t.cfeat = g->points ? g->cfeat : 0;
    t.xyz_off = g->xyz_first ? 0 : t.cfeat;
    t.feat_off = g->xyz_first ? 3 : 0;
    t.xyz = g->xyz; t.new_xyz = g->new_xyz; t.points = g->points; t.idx = g->idx;
    return t;
}

// Is the pair launch wanted for this layer? (pn2_train_opts.pair_launch; the helper stream, when asked for, keeps the two launches)
static inline bool pair_wanted(long long rows, const Opts &o)
{
    if (o.pair_launch == PN2_OPT_OFF || o.side_stream == PN2_OPT_ON) return false;
    return o.pair_launch == PN2_OPT_ON || rows < (1ll << 19);
}

// ---- a helper stream for the backward pass of SMALL levels --------------------------------------------------------------------
// A layer's weight gradient and its data gradient both start from (dy_l, z_l, z_{l-1}) and neither needs the other. On levels
// of a few thousand rows each is a launch of 10-50 us that covers a fraction of the chip (the deep levels of the segmentation
// networks: ~25 such launches per level, one after the other on the caller's stream, were 260 us per level whatever its
// size). With a helper stream the weight-gradient launches (and their reductions / fix-ups) CAN run beside the data-gradient
// chain (opt-in, pn2_train_opts.side_stream -- the measurement at its use site says why it is not the default): fork after the layer's batch-norm coefficients exist, join before the next layer's data gradient overwrites the
// dy buffer the helper reads. One helper stream and two events per (device, caller stream), created on first use and kept
// (with allow_dynamic_lds's table the library's only process state); event record / wait are legal under HIP graph capture
// (the helper joins the capture at the fork and returns at the join), so a captured training step keeps working.
struct SideKey { int dev; hipStream_t main; bool operator==(const SideKey &o) const { return dev == o.dev && main == o.main; } };
struct SideKeyHash { size_t operator()(const SideKey &k) const { return std::hash<unsigned long long>()((unsigned long long)(uintptr_t)k.main * 31ull + (unsigned long long)k.dev); } };
struct SideRes { hipStream_t side; hipEvent_t fork_ev, join_ev; };

struct SideStream {
    hipStream_t main = nullptr, side = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    bool forked = false;
    int init(hipStream_t st, bool enable)
    {
        main = st;
        if (!enable) return PN2_OK;
        static std::mutex mu;
        static std::unordered_map<SideKey, SideRes, SideKeyHash> table;
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return (int)e;
        std::lock_guard<std::mutex> lock(mu);
        const SideKey key = {dev, st};
        auto it = table.find(key);
        if (it == table.end()) {
            SideRes r = {nullptr, nullptr, nullptr};
            if ((e = hipStreamCreateWithFlags(&r.side, hipStreamNonBlocking)) == hipSuccess &&
                (e = hipEventCreateWithFlags(&r.fork_ev, hipEventDisableTiming)) == hipSuccess)
                e = hipEventCreateWithFlags(&r.join_ev, hipEventDisableTiming);
            if (e != hipSuccess) {                                 // nothing half-built stays behind
                if (r.join_ev) (void)hipEventDestroy(r.join_ev);
                if (r.fork_ev) (void)hipEventDestroy(r.fork_ev);
                if (r.side) (void)hipStreamDestroy(r.side);
                return (int)e;
            }
            it = table.emplace(key, r).first;
        }
        side = it->second.side; fork_ev = it->second.fork_ev; join_ev = it->second.join_ev;
        return PN2_OK;
    }
    // Scope guard: an error return between fork() and join() must not leave the helper stream forked -- under HIP graph
    // capture that would be an unjoined capture, which invalidates it. join() is idempotent.
    ~SideStream() { (void)join(); }
    SideStream() = default;
    SideStream(const SideStream &) = delete;
    SideStream &operator=(const SideStream &) = delete;
    hipStream_t get() const { return side ? side : main; }      // where the forked work goes
    int fork()                                                   // the helper continues from here
    {
        if (!side || forked) return PN2_OK;
        hipError_t e = hipEventRecord(fork_ev, main);
        if (e == hipSuccess) e = hipStreamWaitEvent(side, fork_ev, 0);
        forked = e == hipSuccess;
        return (int)e;
    }
    int join()                                                   // the caller's stream waits for everything forked so far
    {
        if (!side || !forked) return PN2_OK;
        hipError_t e = hipEventRecord(join_ev, side);
        if (e == hipSuccess) e = hipStreamWaitEvent(main, join_ev, 0);
        forked = false;
        return (int)e;
    }
};

static bool layers_ok(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group, int *widths,
                      const FpL1 *fp = nullptr)
{
    if (!layers || nlayers < 1 || nlayers > 8) return false;
    for (int l = 0; l < nlayers; ++l) {
        const pn2_bn_layer &L = layers[l];
        if (L.cin <= 0 || L.cout <= 0 || L.cout % 4) return false;
        if (l > 0 && L.cin != layers[l - 1].cout) return false;
        if (!L.weight || !L.gamma || !L.beta || !L.save) return false;
        widths[l] = L.cin;
        widths[l + 1] = L.cout;
    }
    if (group) {
        if (group->b <= 0 || group->n <= 0 || group->m <= 0 || group->nsample <= 0 || !group->xyz) return false;
        if ((long long)group->b * group->m * group->nsample != rows) return false;
        if (layers[0].cin != 3 + (group->points ? group->cfeat : 0)) return false;
        if (!group->idx && group->nsample != group->n) return false;
    } else if (fp) {
        if (layers[0].cin != fp->c2 + fp->c1 || fp->rows != rows) return false;
    } else if (layers[0].cin % 4) {
        return false;
    }
    return true;
}

}  // namespace pn2

extern "C" long long pn2_mlp_train_ws_bytes_ex(long long rows, int nlayers, const int *widths, int pool_rows, int backward,
                                               const int *group_dims, const pn2_train_opts *opts)
{
    pn2::TlPlan pl;
    pn2::GroupDims gd;
    if (group_dims) gd = pn2::group_dims_of(group_dims);
    if (!widths || !pn2::tl_plan(rows, nlayers, widths, pool_rows, backward, pl, group_dims ? &gd : nullptr, pn2::opts_of(opts))) return -1;
    return (long long)pl.total;
}
extern "C" long long pn2_mlp_train_ws_bytes(long long rows, int nlayers, const int *widths, int pool_rows, int backward,
                                            const int *group_dims)
{
    return pn2_mlp_train_ws_bytes_ex(rows, nlayers, widths, pool_rows, backward, group_dims, nullptr);
}

// 1: layer 1 of this grouped level runs once per point; backward then writes the gradient of `points` itself
// (grad_points (b, n, cfeat)) instead of the per-row gradient grad_feat_rows
extern "C" int pn2_mlp_train_layer1_per_point_ex(int nlayers, const int *widths, const int *group_dims, const pn2_train_opts *opts)
{
    if (!widths || !group_dims || nlayers < 1 || nlayers > 8) return 0;
    const pn2::GroupDims gd = pn2::group_dims_of(group_dims);
    return pn2::l1_per_point(nlayers, widths, &gd, pn2::opts_of(opts)) ? 1 : 0;
}
extern "C" int pn2_mlp_train_layer1_per_point(int nlayers, const int *widths, const int *group_dims)
{
    return pn2_mlp_train_layer1_per_point_ex(nlayers, widths, group_dims, nullptr);
}

// 1: the top layer's pre-norm tensor z_L is written by forward and read by backward (the caller allocates layers[L-1].z);
// 0: it is not (pooled stacks of two or more layers on large levels: layers[L-1].z may be NULL)
extern "C" int pn2_mlp_train_top_stored_ex(long long rows, int nlayers, const int *widths, int pool_rows, const pn2_train_opts *opts)
{
    if (!widths || nlayers < 1 || nlayers > 8) return 1;
    return pn2::top_stored(rows, nlayers, widths, pool_rows, pn2::opts_of(opts)) ? 1 : 0;
}
extern "C" int pn2_mlp_train_top_stored(long long rows, int nlayers, const int *widths, int pool_rows)
{
    return pn2_mlp_train_top_stored_ex(rows, nlayers, widths, pool_rows, nullptr);
}

// byte offsets of the backward workspace's dy ping-pong buffers and per-layer sums (diagnostics: scripts/train_mlp_check.py)
extern "C" int pn2_mlp_train_ws_layout(long long rows, int nlayers, const int *widths, int pool_rows, long long *ga, long long *gb,
                                       long long *stats, long long *coef)
{
    pn2::TlPlan pl;
    if (!widths || !pn2::tl_plan(rows, nlayers, widths, pool_rows, 1, pl, nullptr, pn2::opts_of(nullptr))) return PN2_E_ARG;
    if (ga) *ga = (long long)pl.ga;
    if (gb) *gb = (long long)pl.gb;
    for (int l = 0; l < nlayers; ++l) {
        if (stats) stats[l] = (long long)pl.stats[l];
        if (coef) coef[l] = (long long)pl.coef[l];
    }
    return PN2_OK;
}

namespace pn2 {
// Per-channel finalisations inside the launches that produce their sums (TlFin): OPT-IN. Measured (rocprofv3 per-dispatch
// traces, profiles/r04/fold_finalize_experiment.txt): the folded pass is 5-7 us longer on a level of 4,096 rows (sem_seg SA4:
// 17.1 / 25.8 / 31.6 against 15.2 / 18.6 / 26.2 us) and 13 us longer with 256 partial rows of 128 channels (sem_seg FP4), for a
// finalisation launch of 4.5-6 us saved -- the write-through stores, the ticket and the last workgroup's reads are four or
// more dependent trips to memory, because the L2s of the eight XCDs are not coherent with each other. With release / acquire
// fences instead (a write-back and an invalidate of the whole L2 per workgroup) it was 20-35 us longer.
static inline bool fold_wanted(const Opts &o) { return o.fold_finalize == PN2_OPT_ON; }

static TlFin fin_forward(const pn2_bn_layer &L, long long rows, double *stats, unsigned *ticket)
{
    TlFin f;
    memset(&f, 0, sizeof(f));
    f.ticket = ticket; f.mode = 1; f.N = L.cout; f.stats = stats; f.count = (double)rows;
    f.gamma = L.gamma; f.beta = L.beta; f.bias = L.bias; f.running_mean = L.running_mean; f.running_var = L.running_var;
    f.momentum = L.momentum; f.eps = L.eps; f.var_biased = L.running_var_biased; f.save = L.save;
    return f;
}

static TlFin fin_backward(const pn2_bn_layer &L, long long rows, double *stats, float *coef, unsigned *ticket)
{
    TlFin f;
    memset(&f, 0, sizeof(f));
    f.ticket = ticket; f.mode = 2; f.N = L.cout; f.stats = stats; f.count = (double)rows;
    f.gamma = L.gamma; f.save = L.save; f.grad_gamma = L.grad_gamma; f.grad_beta = L.grad_beta; f.coef = coef;
    f.accumulate = L.grad_accumulate;
    return f;
}

// 0 ok, else the PN2_E_* code the pooling entries return before anything is launched
int tl_pool_args(int pool_rows, int pooling, bool grouped)
{
    if (pooling < 0 || pooling > 3) return PN2_E_ARG;
    if (pooling == 0) return PN2_OK;
    if (!grouped) return PN2_E_NULL;
    return pool_rows > 0 ? PN2_OK : PN2_E_ARG;
}

// Which of argsel / zsel / pool_w a pooling mode uses: the max's selection for max and max_and_avg (the extrema of the GEMM
// epilogue, E_POOL), the weights for weighted_avg. The others never reach a check or a kernel, whatever the caller passed.
static TlCall tl_pool_buffers(TlCall c)
{
    if (c.pooling != 0 && c.pooling != 3) { c.argsel = nullptr; c.zsel = nullptr; }
    if (c.pooling != 2) c.pool_w = nullptr;
    return c;
}

// a GEMM over the dense rows A against the operand tiles at `wpacked`
static TlGemm dense_gemm(long long rows, const float *A, const void *wpacked)
{
    TlGemm p;
    memset(&p, 0, sizeof(p));
    p.rows = rows;
    p.A = A;
    p.wpacked = reinterpret_cast<const u32x4 *>(wpacked);
    return p;
}

// ... that stores its product and sums no moments (forward: the per-point products of layer 1)
static TlGemm store_gemm(long long rows, const float *A, const void *wpacked, float *out)
{
    TlGemm p = dense_gemm(rows, A, wpacked);
    p.emode = E_STORE;
    p.out = out;
    return p;
}

// the epilogue of a data gradient that leaves the stack: `cols` plain columns, no mask, no sums
static void plain_out(TlGemm &p, float *out, int cols)
{
    p.emode = E_PLAIN;
    p.out = out; p.out_pitch = cols; p.col0 = 0; p.col1 = cols;
}

// What both directions of a call work from: the call (its pooling buffers normalised), the rules' overrides, the workspace
struct TlRun {
    const TlCall c;
    const Opts o;
    const FpL1 *const fp;            // the FP level with layer 1 per known point, or nullptr
    char *const base;
    const hipStream_t st;
    int widths[9];
    TlPlan pl;
    GroupDims gd;
    bool fold = false;               // a layer's per-channel finalisation inside the pass that sums for it (TlFin)

    explicit TlRun(const TlCall &call)
        : c(tl_pool_buffers(call)), o(!call.mask ? opts_of(call.opts) : call.group ? ragged_group_opts(call.opts) : ragged_opts(call.opts)),
          fp(c.has_fp ? &c.fp : nullptr), base(static_cast<char *>(call.ws)),
          st(as_stream(call.stream)) {}
    TlRun(const TlRun &) = delete;
    TlRun &operator=(const TlRun &) = delete;

    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
    unsigned *tickets() const { return at<unsigned>(pl.tickets); }
    double *stats(int l) const { return at<double>(pl.stats[l]); }
    bool want_max() const { return c.pooling == 0 || c.pooling == 3; }
    const unsigned *mask_words() const { return c.mask ? ragged_words(c.mask) : nullptr; }     // ragged rows, or nullptr
    const double *row_count() const { return c.mask ? ragged_count(c.mask) : nullptr; }        // ... their valid rows, on the device

    // the checks both directions make first, in this order
    int check_inputs()
    {
        if (!layers_ok(c.rows, c.nlayers, c.layers, c.group, widths, fp)) return PN2_E_ARG;
        if (c.frozen && fp) return PN2_E_ARG;                     // (the FP node with layer 1 per known point has no frozen form)
        // the row mask: batch statistics; plain rows or the FP node unpooled, a grouped level with the max pool and no
        // coordinate gradients (train_mlp_ragged_group.hip)
        if (c.mask && (c.frozen || (c.group ? (c.pooling != 0 || c.pool_rows <= 0 || c.grad_xyz || c.grad_new_xyz) : c.pool_rows != 0)))
            return PN2_E_ARG;
        return PN2_OK;
    }
    bool masked_group() const { return c.mask && c.group; }        // the grouped rows of a ragged batch
    bool pool_buffers_missing(int pool_rows) const
    {
        // (the masked pool pass reads z_L itself: no zsel)
        return (pool_rows && want_max() && (!c.argsel || (!c.zsel && !c.mask))) || (c.pooling == 2 && !c.pool_w);
    }
    bool plan(int pool_rows, int backward)
    {
        if (c.group) gd = group_dims(c.group);
        return tl_plan(c.rows, c.nlayers, widths, pool_rows, backward, pl, c.group ? &gd : nullptr, o, fp);
    }

    // The FP node's inputs as the GEMMs read them: zero-padded copies of points2 / points1 where their shapes need one
    int fp_padded_inputs(const float *&p2, const float *&p1) const
    {
        p2 = fp->points2; p1 = fp->points1;
        if (fp->pad2()) {
            float *d = at<float>(pl.fp2);
            if (int rc = fp_launch_pad(fp->points2, fp->bm, fp->c2, fp->mp, fp->c2p, d, st)) return rc;
            p2 = d;
        }
        if (fp->pad1()) {
            float *d = at<float>(pl.fp1);
            if (int rc = fp_launch_pad(fp->points1, c.rows, fp->c1, c.rows, fp->c1p, d, st)) return rc;
            p1 = d;
        }
        return PN2_OK;
    }
};

// ---- forward ----------------------------------------------------------------------------------------------------------------
struct Fwd : TlRun {
    using TlRun::TlRun;
    bool per_point = false, coords_only = false, keep_top = true;

    float *out() const { return const_cast<float *>(c.out); }     // (TlCall: forward writes these)

    // every layer's weights -> operand tiles, one launch
    int pack_weights()
    {
        TlPackJobs jobs;
        memset(&jobs, 0, sizeof(jobs));
        int nj = 0;
        for (int l = 0; l < c.nlayers; ++l) {
            const pn2_bn_layer &L = c.layers[l];
            if (l == 0 && coords_only) continue;                 // no matrix-core pass at all
            if (l == 0 && fp) {                                   // W1a for the known points' GEMM, W1b for the one over the rows
                add_pack_job(jobs, nj, L.weight, L.w_stride_k, L.w_stride_n, gemm_shape(fp->mp, fp->c2, L.cout, o), base + pl.pack[l]);
                if (fp->c1 > 0)
                    add_pack_job(jobs, nj, L.weight + (long long)fp->c2 * L.w_stride_k, L.w_stride_k, L.w_stride_n,
                                 gemm_shape(c.rows, fp->c1, L.cout, o), base + pl.fpw);
                continue;
            }
            if (l == 0 && per_point) {                           // only the feature rows of W_1: P = points . W1f
                const TlGather gt = make_gather(c.group);
                add_pack_job(jobs, nj, L.weight + gt.feat_off * L.w_stride_k, L.w_stride_k, L.w_stride_n,
                             gemm_shape((long long)gd.b * gd.n, gt.cfeat, L.cout, o), base + pl.pack[l]);
            } else {
                add_pack_job(jobs, nj, L.weight, L.w_stride_k, L.w_stride_n, gemm_shape(c.rows, L.cin, L.cout, o), base + pl.pack[l]);
            }
        }
        fold = fold_wanted(o) && nj > 0 && !c.frozen;             // (the pack launch zeroes the tickets; frozen: nothing to fold)
        if (fold) jobs.tickets = tickets();
        return launch_pack_jobs(jobs, nj, st);
    }

    // a layer's batch moments: summed by its pass, or not at all under frozen statistics
    double *moments(int l) const { return c.frozen ? nullptr : stats(l); }

    // the np partial rows of layer l's moments -> its (mean, invstd, a, c) and running statistics; nothing under frozen ones
    int finalize_moments(int l, int np) const
    {
        if (c.frozen) return PN2_OK;
        const pn2_bn_layer &L = c.layers[l];
        return launch_bn_finalize(stats(l), np, L.cout, (double)c.rows, row_count(), L.gamma, L.beta, L.running_mean, L.running_var,
                                  L.momentum, L.eps, L.save, L.bias, L.running_var_biased, st);
    }

    // an unpooled top layer: out = relu(a z_L + c)
    int apply(const pn2_bn_layer &L) const
    {
        return launch_apply(c.rows * L.cout / 4, L.cout, L.z, L.save, mask_words(), out(), st);
    }

    // layer 1 of an FP level once per KNOWN point (train_mlp_fp.hip): Q = points2 W1a over the b m known points,
    // z_1 = points1 W1b over the rows, then one pass adds the interpolated rows of Q and sums the batch moments.
    // Ragged rows (c.mask): the known points are a previous level's dense output, so Q stays dense; points1 W1b stays the dense
    // store GEMM too -- rows are independent, a NaN padding row of points1 stays in its row of z_1 -- and the masked layer-1 pass
    // (tl_fp_l1_forward_masked_kernel) never reads that row and overwrites it with zeros.
    int layer1_fp()
    {
        const pn2_bn_layer &L = c.layers[0];
        float *Q = at<float>(pl.l1p);
        const float *p2, *p1;
        if (int rc = fp_padded_inputs(p2, p1)) return rc;
        TlGemm q = store_gemm(fp->mp, p2, base + pl.pack[0], Q);  // no moments: Q is not z_1
        if (int rc = launch_gemm(A_PLAIN, q, gemm_shape(fp->mp, fp->c2p, L.cout, o), st, o)) return rc;
        if (fp->c1 > 0) {
            TlGemm q1 = store_gemm(c.rows, p1, base + pl.fpw, L.z);
            if (int rc = launch_gemm(A_PLAIN, q1, gemm_shape(c.rows, fp->c1p, L.cout, o), st, o)) return rc;
        }
        int np = 0;
        if (int rc = fp_launch_l1_forward(c.rows, fp->n, fp->m, L.cout, fp->idx, fp->dist, fp->weight_out, Q, L.z, fp->c1 > 0, mask_words(),
                                          stats(0), kMaxParts, st, &np)) return rc;
        if (int rc = finalize_moments(0, np)) return rc;
        return c.nlayers == 1 ? apply(L) : PN2_OK;
    }

    // layer 1 once per point (tl_l1_forward_kernel): P = points . W1f over the b n points, then one pass over the rows
    int layer1_per_point()
    {
        const pn2_bn_layer &L = c.layers[0];
        const TlGather gt = make_gather(c.group);
        const long long bn = (long long)gd.b * gd.n;
        float *P = at<float>(pl.l1p);
        TlGemm q = store_gemm(bn, c.group->points, base + pl.pack[0], P);
        if (int rc = launch_gemm(A_PLAIN, q, gemm_shape(bn, gt.cfeat, L.cout, o), st, o)) return rc;
        int np = 0;
        if (int rc = launch_l1_forward(c.rows, gd, c.group, L, P, moments(0), st, &np)) return rc;
        return finalize_moments(0, np);
    }

    // a level without features: z_1 = b + (xyz - c) W1 in one pass on the vector units (tl_l1_forward_kernel, no P)
    int layer1_coords_only()
    {
        int np = 0;
        if (int rc = launch_l1_forward(c.rows, gd, c.group, c.layers[0], nullptr, moments(0), st, &np)) return rc;
        return finalize_moments(0, np);
    }

    // a layer as one GEMM over the rows, with the pooling of the top layer behind it
    int generic_layer(int l)
    {
        const pn2_bn_layer &L = c.layers[l];
        const long long rows = c.rows;
        const int pool_rows = c.pool_rows, pooling = c.pooling;
        const GemmShape g = gemm_shape(rows, L.cin, L.cout, o);
        const bool last = l == c.nlayers - 1;
        TlGemm p;
        memset(&p, 0, sizeof(p));
        p.rows = rows;
        int amode;
        if (l == 0 && c.group) { amode = A_GATHER; p.g = make_gather(c.group); }
        else if (l == 0) { amode = A_PLAIN; p.A = c.x; }
        else { const pn2_bn_layer &D = c.layers[l - 1]; amode = A_RELU; p.A = D.z; p.p0 = D.save + 2 * D.cout; p.p1 = D.save + 3 * D.cout; }
        p.wpacked = at<const u32x4>(pl.pack[l]);
        p.bias = nullptr;                                        // see the comment above the layer loop
        p.emode = (last && pool_rows && want_max() && !c.mask) ? E_POOL : E_STORE;    // (ragged rows: the pool is a pass of its own)
        p.out = (last && !keep_top) ? nullptr : L.z;              // the pooled top layer of a large level is never written
        p.stats = moments(l);
        p.nostats = c.frozen ? 1 : 0;                             // the GEMM's compile-time "no statistics" variant
        p.mask = mask_words();
        if (p.emode == E_POOL) {
            const long long parts = rows / (pool_rows == 16 ? 16 : 32);
            float *pp = at<float>(pl.pool);
            p.pmax = pp;
            p.pamax = reinterpret_cast<int *>(pp + parts * L.cout);
            p.pool_gamma = L.gamma;
            p.prow = pool_rows == 16 ? 16 : 32;
        }
        int nparts = 0;
        if (fold) p.fin = fin_forward(L, rows, p.stats, tickets() + l);
        if (int rc = launch_gemm(amode, p, g, st, o, &nparts)) return rc;
        if (!fold)
            if (int rc = finalize_moments(l, nparts)) return rc;
        if (last && pool_rows && c.mask)                          // the grouped rows of a ragged batch: the max over the valid rows of z_L
            return launch_pool_masked(rows / pool_rows, pool_rows, L.cout, L.z, L.gamma, L.save, mask_words(), out(),
                                      const_cast<int *>(c.argsel), st);
        // max_and_avg: the max half as pooling 0 computes it, into the workspace behind the plan; the average kernel places it
        float *maxv = pooling == 3 ? at<float>(pl.total) : nullptr;
        if (last && pool_rows && want_max()) {
            const long long groups = rows / pool_rows;
            const int prow = pool_rows == 16 ? 16 : 32;
            if (int rc = launch_pool_finalize(groups, L.cout, pool_rows / prow, prow, p.pmax, p.pamax, L.gamma, L.save, maxv ? maxv : out(),
                                              const_cast<int *>(c.argsel), const_cast<float *>(c.zsel), st)) return rc;
        }
        if (last && pool_rows && pooling != 0) {
            const long long groups = rows / pool_rows;
            if (pooling == 2) {
                if (int rc = launch_pool_weights(groups, pool_rows, c.group->n, c.group->m, c.group->xyz, c.group->new_xyz, c.group->idx,
                                                 const_cast<float *>(c.pool_w), st)) return rc;
            }
            return launch_pool_avg(groups, pool_rows, L.cout, L.z, L.save, c.pool_w, maxv, out(), st);
        }
        return (last && !pool_rows) ? apply(L) : PN2_OK;
    }

    int run()
    {
        if (int rc = check_inputs()) return rc;
        if ((!c.group && !c.x && !fp) || !c.out || !c.ws || pool_buffers_missing(c.pool_rows)) return PN2_E_NULL;
        if (c.mask && !c.lengths) return PN2_E_NULL;
        if (c.pool_rows && (c.rows % c.pool_rows || (c.group && c.pool_rows != c.group->nsample))) return PN2_E_ARG;
        if (!plan(c.mask ? 0 : c.pool_rows, 0)) return PN2_E_ARG;  // (ragged rows: no partial extrema, tl_group_ragged_ws_bytes)
        per_point = c.group && l1_per_point(c.nlayers, widths, &gd, o);
        // forward: layer 1 on the vector units only WITHOUT features (with the input normals gathered per row the vector kernel
        // measured slower than the gathered GEMM: cls_msg forward 2.51 -> 2.57 ms; its backward counterpart is the one that pays)
        coords_only = c.group && gd.cfeat == 0 && l1_coords_only(c.nlayers, widths, &gd, o);
        keep_top = c.pooling != 0 || c.mask || top_stored(c.rows, c.nlayers, widths, c.pool_rows, o);    // a mean needs z_L itself, the masked pool too
        for (int l = 0; l < c.nlayers; ++l)
            if (!c.layers[l].z && (keep_top || l < c.nlayers - 1)) return PN2_E_NULL;
        if (c.mask)                                               // ragged rows: lengths -> the validity words and the count
            if (int rc = launch_ragged_mask(c.rg_b, c.rg_n, c.lengths, c.mask, st, c.rg_unit, c.rg_cap)) return rc;
        if (int rc = pack_weights()) return rc;
        if (c.frozen)                                             // every layer's (m', invstd, a, c) from the running statistics
            if (int rc = frozen_launch_save(c.nlayers, c.layers, st)) return rc;
        // The conv bias is NOT added to the pre-norm tensors: batch normalisation removes any per-channel constant, so
        // z_l := h W_l gives the same output, the same gradients (the bias gradient is zero) and the same batch variance; only
        // the batch MEAN that enters the running average is mean(z_l) + b_l (tl_bn_finalize_kernel). It is more than a saved
        // add: the folded form a z + c loses accuracy with |mean| / std of a channel, and a bias is pure mean.
        for (int l = 0; l < c.nlayers; ++l) {
            const int rc = l > 0 ? generic_layer(l) : fp ? layer1_fp() : per_point ? layer1_per_point()
                         : coords_only ? layer1_coords_only() : generic_layer(0);
            if (rc) return rc;
        }
        return PN2_OK;
    }
};

// pooling: 0 max, 1 avg, 2 weighted_avg, 3 max_and_avg (pn2_mlp_train_forward_pool checks it)
int tl_train_forward(const TlCall &call) { return Fwd(call).run(); }

// ---- backward ---------------------------------------------------------------------------------------------------------------
// pooling 1-3 (pn2_mlp_train_backward_pool): the averaged top layer is an UNPOOLED one from here on -- its dense gradient
// (tl_pool_top_grad_kernel) enters the passes of the FP levels' top layer, and everything below runs unchanged
struct Bwd : TlRun {
    using TlRun::TlRun;
    const int cus = device_cus();
    long long rows = 0;
    int nlayers = 0;
    const pn2_bn_layer *layers = nullptr;
    XyzPlan xp;
    // decided once
    int pool_rows = 0, avg_rows = 0;                    // the max's group size; > 0: the group size of the averaged top layer
    int mask_rows = 0;                                  // > 0: the group size of the max over the valid rows (ragged grouped rows)
    bool want_xyz = false, want_dx = false, per_point = false, coords_only = false;
    bool ztop = false;                                  // pooled top layer without z_L (tl_top_mats_kernel)
    bool skip[8] = {false, false, false, false, false, false, false, false};
    int lo = 0;
    FuseShape fz[8];
    WgradShape wz[8];
    // running
    bool ident_written = false;
    bool folded[8] = {false, false, false, false, false, false, false, false};     // layers whose backward finalisation ran inside the pass above
    int nparts[8];                                      // rows of each layer's partial-sum array
    float *gq = nullptr;                                // the pooled gradient (groups, cout_L)
    float *gcur = nullptr, *gnext = nullptr;            // dy of the current layer (dense case) / of the layer below
    int l1_moment_parts = 0;                            // > 0: layer 1's weight gradient comes from moments (TlWgrad::l1x)
    // weight-gradient launches on a helper stream beside the data-gradient chain (SideStream above): OPT-IN. Measured
    // (scripts/lab_ab.sh side_stream, profiles/r04/README.md): every fork / join is a cross-queue dependency of ~10 us on this
    // runtime, three pairs per level -- sem_seg SA2 280 -> 330 us, SA4 250 -> 305, FP4 335 -> 380; only the group_all level
    // (three wide layers over 4,096 rows) gains, 431 -> 379 us. The size rule therefore never switches it on.
    SideStream sd;

    float *coef(int l) const { return at<float>(pl.coef[l]); }
    bool below(int l) const { return l > lo || (l == 0 && want_dx); }
    double *sums_of(int l) const { return skip[l] ? nullptr : stats(l); }
    bool pooled_top(int l) const { return pool_rows && l == nlayers - 1; }

    // the arguments, the plan, and everything that is decided once
    int prepare()
    {
        rows = c.rows; nlayers = c.nlayers; layers = c.layers;
        if (int rc = check_inputs()) return rc;
        want_xyz = c.group && c.grad_xyz;               // the coordinate gradients (pn2_mlp_train_backward_xyz, train_mlp_xyz.hip)
        if ((!c.group && !c.x && !fp) || !c.out || !c.grad_out || !c.ws || pool_buffers_missing(c.pool_rows)) return PN2_E_NULL;
        avg_rows = c.pooling ? c.pool_rows : 0;
        if (c.pooling && (!c.group || avg_rows <= 0 || rows % avg_rows || avg_rows != c.group->nsample)) return PN2_E_ARG;
        // the grouped rows of a ragged batch: the pooled top layer is an UNPOOLED one too -- its dense gradient comes from
        // tl_pool_top_grad_masked_kernel and the masked passes of the plain rows run below it
        mask_rows = masked_group() ? c.pool_rows : 0;
        if (mask_rows && (rows % mask_rows || mask_rows != c.group->nsample)) return PN2_E_ARG;
        pool_rows = (c.pooling || mask_rows) ? 0 : c.pool_rows;
        // frozen statistics: a layer whose four gradient slots are all NULL wants no parameter gradient -- no weight-gradient pass,
        // no per-channel sums (batch statistics cannot allow that: dz itself needs the sums)
        for (int l = 0; l < nlayers; ++l) {
            const bool all3 = layers[l].grad_weight && layers[l].grad_gamma && layers[l].grad_beta;
            const bool any = layers[l].grad_weight || layers[l].grad_gamma || layers[l].grad_beta ||
                             (c.frozen && c.grad_bias && c.grad_bias[l]);
            if (c.frozen && !any) { skip[l] = true; continue; }
            if (!all3) return PN2_E_NULL;
        }
        if (!plan(pool_rows, 1)) return PN2_E_ARG;
        memset(&xp, 0, sizeof(xp));
        if (want_xyz && !xyz_plan(pl, rows, nlayers, widths, gd, o, xp)) return PN2_E_ARG;
        per_point = c.group && l1_per_point(nlayers, widths, &gd, o);
        coords_only = c.group && l1_coords_only(nlayers, widths, &gd, o);
        want_dx = fp ? (fp->grad_points2 || fp->grad_points1)
                : c.group ? ((per_point ? c.grad_points : c.grad_feat_rows) && c.group->points && c.group->cfeat > 0) : c.grad_x != nullptr;
        ztop = !top_stored(rows, nlayers, widths, pool_rows, o);
        for (int l = 0; l < nlayers; ++l)
            if (!layers[l].z && !(ztop && l == nlayers - 1)) return PN2_E_NULL;
        // frozen statistics: the chain stops at the lowest layer that still needs something (lo; 0 otherwise), and a layer takes
        // a data gradient from above only where something below it is wanted
        if (c.frozen)
            while (lo < nlayers - 1 && skip[lo] && !(lo == 0 && (want_dx || want_xyz))) ++lo;
        // Which layers run their data gradient inside the weight-gradient pass (one pass over the layer's activations instead of
        // two, tl_wgrad_kernel<.., DY>): decided here, once, for the packing below and the launches
        memset(fz, 0, sizeof(fz));
        for (int l = lo; l < nlayers; ++l) {
            const pn2_bn_layer &L = layers[l];
            if (skip[l] || (l > 0 && !below(l))) continue;              // no weight-gradient pass to fuse into / no data gradient to fuse
            if (ztop && l == nlayers - 1) {
                // (the z-free pooled top layer in one pass is correct and tested, but not yet faster than its three kernels -- 690 vs
                // 590 us at the metric shape: two waves carry the whole data gradient, 72 MFMAs on transposed reads each -- so the
                // size rule leaves it off; fuse_wgrad = PN2_OPT_ON forces it)
                wz[l] = wgrad_shape(rows, L.cin, top_cols(L.cin, L.cout), false, cus, PN2_OPT_OFF);
                if (o.fuse_wgrad == PN2_OPT_ON) fz[l] = fuse_shape(rows, wz[l], tiles(L.cout) * 32 + L.cin, L.cin, o, false);
            } else if (!(l == 0 && (c.group || fp || !want_dx))) {
                wz[l] = wgrad_shape(rows, L.cin, L.cout, false, cus, PN2_OPT_OFF);
                fz[l] = fuse_shape(rows, wz[l], L.cout, L.cin, o);
            }
            if (fz[l].ok) { wz[l].lds_dy = fz[l].lds; wz[l].upw = fz[l].upw; }
        }
        gq = at<float>(pl.gq);
        gcur = at<float>(pl.ga); gnext = at<float>(pl.gb);
        return PN2_OK;
    }

    // W_l^T of every data-gradient GEMM, one launch
    int pack_weights()
    {
        TlPackJobs jobs;
        memset(&jobs, 0, sizeof(jobs));
        int nj = 0;
        for (int l = lo; l < nlayers; ++l) {
            const pn2_bn_layer &L = layers[l];
            if (below(l) && !(ztop && l == nlayers - 1)) {               // dy_{l-1} = dz_l . W_l^T
                if (fz[l].ok) {                                   // every output tile in ONE slab (the fused pass keeps W^T resident)
                    add_pack_job(jobs, nj, L.weight, L.w_stride_n, L.w_stride_k, one_slab(L.cout, L.cin, fz[l]), base + pl.pack[l]);
                } else if (l == 0 && fp) {                        // W1a^T, W1b^T: the data gradients of points2 / points1
                    if (fp->grad_points2)
                        add_pack_job(jobs, nj, L.weight, L.w_stride_n, L.w_stride_k, gemm_shape(fp->mp, L.cout, fp->c2, o), base + pl.pack[l]);
                    if (fp->grad_points1 && fp->c1 > 0)
                        add_pack_job(jobs, nj, L.weight + (long long)fp->c2 * L.w_stride_k, L.w_stride_n, L.w_stride_k,
                                     gemm_shape(rows, L.cout, fp->c1, o), base + pl.fpw);
                } else if (l == 0 && c.group) {
                    // layer 1 of a grouped level: only the FEATURE rows of W_1 (the grouped xyz takes no gradient here);
                    // per point: the same tiles, for the GEMM over the b n points
                    const TlGather gt = make_gather(c.group);
                    add_pack_job(jobs, nj, L.weight + gt.feat_off * L.w_stride_k, L.w_stride_n, L.w_stride_k,
                                 gemm_shape(per_point ? (long long)gd.b * gd.n : rows, L.cout, gt.cfeat, o), base + pl.pack[l]);
                } else {
                    add_pack_job(jobs, nj, L.weight, L.w_stride_n, L.w_stride_k, gemm_shape(rows, L.cout, L.cin, o), base + pl.pack[l]);
                }
            }
        }
        if ((per_point || fp) && nj > 0) {                        // the identity coefficients of layer 1's per-point weight gradient
            jobs.ident = at<float>(pl.l1coef);
            jobs.ident_c = layers[0].cout;
        }
        ident_written = jobs.ident != nullptr;
        fold = fold_wanted(o) && nj > 0 && !c.frozen;             // (the pack launch zeroes the tickets)
        if (fold) jobs.tickets = tickets();
        return launch_pack_jobs(jobs, nj, st);
    }

    // the operand tiles of a data gradient that rides in the weight-gradient pass: every output tile in one slab
    static GemmShape one_slab(int K, int N, const FuseShape &f)
    {
        GemmShape gg;
        memset(&gg, 0, sizeof(gg));
        gg.K = K; gg.N = N; gg.tk = f.tk; gg.tn = f.nt; gg.ns = f.nt; gg.slabs = 1;
        return gg;
    }

    // frozen statistics: dz = a dy for every layer, known before the first pass
    int frozen_coefficients() const
    {
        float *cf[8];
        for (int l = 0; l < nlayers; ++l) cf[l] = coef(l);
        return frozen_launch_coef(nlayers, layers, cf, st);
    }

    // top of the stack: dy_L and its two column sums
    int top_gradient()
    {
        const pn2_bn_layer &T = layers[nlayers - 1];
        const long long groups = pool_rows ? rows / pool_rows : 0;
        long long gy = pool_rows ? (groups + 63) / 64 : (rows + 255) / 256;
        if (gy > kMaxParts) gy = kMaxParts;
        const int parts = (int)gy;                          // rows of the partial sums = the kernels' gridDim.y
        nparts[nlayers - 1] = parts;
        double *sums = sums_of(nlayers - 1);
        if (mask_rows)
            return launch_pool_top_grad_masked(rows, mask_rows, T.cout, c.out, c.grad_out, c.argsel, mask_words(), T.z, gcur, sums, parts, st);
        if (avg_rows)
            return launch_pool_top_grad(rows, avg_rows, T.cout, c.grad_out, T.z, T.save, c.pool_w, c.pooling == 3 ? c.argsel : nullptr, gcur,
                                        sums, parts, st);
        if (pool_rows) return launch_pool_grad(groups, T.cout, c.out, c.grad_out, c.zsel, gq, sums, parts, st);
        return launch_top_grad(rows, T.cout, c.out, c.grad_out, T.z, gcur, sums, parts, st);
    }

    // The coordinate gradients, from layer 1's dz_1 = s G - c0 - c1 Z (cf == nullptr: G is dz_1 itself; sel: the pooled
    // single-layer stack, G = gq): g_r = dz_1[r] . W1x^T per row, grad_new_xyz = minus the group sums, grad_xyz = the rows
    // scattered onto the points -- or, where backward has dz_1 on the points already (S, layer 1 per point), S . W1x^T
    int xyz_pass(const float *G, const float *Z, const float *cf, const int *sel, const float *S) const
    {
        const pn2_bn_layer &L1 = layers[0];
        const pn2_group_src *group = c.group;
        const float *wx = L1.weight + make_gather(group).xyz_off * L1.w_stride_k;
        if (!group->idx)                                  // group_all: row k of cloud i IS point k, no centroid
            return xyz_launch_rows(rows, L1.cout, G, Z, cf, sel, gd.nsample, wx, L1.w_stride_k, L1.w_stride_n, c.grad_xyz, st);
        float *g3 = at<float>(xp.g);
        if (c.grad_new_xyz || !S) {
            if (int rc = xyz_launch_rows(rows, L1.cout, G, Z, cf, sel, gd.nsample, wx, L1.w_stride_k, L1.w_stride_n, g3, st)) return rc;
            if (c.grad_new_xyz)
                if (int rc = xyz_launch_centroids(rows / gd.nsample, gd.nsample, g3, c.grad_new_xyz, st)) return rc;
        }
        if (S)
            return xyz_launch_rows((long long)gd.b * gd.n, L1.cout, S, nullptr, nullptr, nullptr, 1, wx, L1.w_stride_k, L1.w_stride_n,
                                   c.grad_xyz, st);
        if (group->idx_plan)                              // the level's index plan: nothing is inverted here
            return pn2_group_point_grad_planned(gd.b, gd.n, 3, gd.m, gd.nsample, g3, group->idx_plan, c.grad_xyz, c.reproducible, c.stream);
        return pn2_group_point_grad_seg(gd.b, gd.n, 3, gd.m, gd.nsample, g3, group->idx, c.grad_xyz, base + xp.seg, c.reproducible, c.stream);
    }

    // a weight-gradient pass into the planned partial sums
    TlWgrad wgrad_into_partial(long long wrows, int KI) const
    {
        TlWgrad w;
        memset(&w, 0, sizeof(w));
        w.rows = wrows;
        w.KI = KI;
        w.partial = at<float>(pl.partial); w.partial_cap = pl.partial_cap;
        return w;
    }

    // the first operand of a layer's passes: h_{l-1} = relu(a z_{l-1} + c) of the layer below
    static void relu_input(TlWgrad &w, const pn2_bn_layer &D)
    {
        w.amode = A_RELU; w.A = D.z; w.pa = D.save + 2 * D.cout; w.pc = D.save + 3 * D.cout;
    }

    // the data gradient's epilogue into the layer below: dy_{l-1} masked by that layer's ReLU, its (dy, dy z) summed -- and,
    // folded, the sums turned into that layer's gradients and coefficients by the same launch
    void into_below(TlGemm &p, int l)
    {
        const pn2_bn_layer &D = layers[l - 1];
        p.emode = E_MASK;
        p.out = gnext;
        p.zprev = D.z; p.ea = D.save + 2 * D.cout; p.ec = D.save + 3 * D.cout;
        p.stats = sums_of(l - 1);
        p.nostats = (c.frozen && !p.stats) ? 1 : 0;
        if (!fold) return;
        p.fin = fin_backward(D, rows, p.stats, coef(l - 1), tickets() + (l - 1));
        folded[l - 1] = true;
    }

    // ... the same epilogue where the data gradient rides in the weight-gradient pass
    void dy_into_below(TlWgrad &w, int l) const
    {
        const pn2_bn_layer &D = layers[l - 1];
        w.dy_out = gnext;
        w.dy_zprev = D.z; w.dy_ea = D.save + 2 * D.cout; w.dy_ec = D.save + 3 * D.cout;
        w.dy_stats = sums_of(l - 1);
    }

    void dy_in_wgrad(TlWgrad &w, int l, int cols) const
    {
        w.dy_w = at<const u32x4>(pl.pack[l]);
        w.xr_off = (int)fz[l].xr_off;
        w.dy_tk = fz[l].tk; w.dy_nt = fz[l].nt; w.single = fz[l].single;
        w.dy_cols = cols; w.dy_pitch = cols;
        w.dy_nt_store = o.nt == PN2_OPT_OFF ? 0 : o.nt == PN2_OPT_ON ? 1 : (size_t)rows * cols * sizeof(float) >= ((size_t)128 << 20);
    }

    // A data gradient beside the weight gradient of the same layer, independent passes over the same activations: ONE launch
    // for both where the pair has a kernel (tl_pair_kernel), else the weight gradient first (on the helper stream when that
    // is asked for), then the GEMM. pair_rows: the row count the pair rule looks at.
    int beside(int amode, TlGemm &p, const GemmShape &g, TlWgrad &w, const WgradShape &ws, const pn2_bn_layer &L, long long pair_rows,
               int *np, double *plain = nullptr)
    {
        int rc = kNoPair;
        if (pair_wanted(pair_rows, o)) rc = launch_pair(amode, p, g, w, ws, L, st, o, np, plain);
        if (rc == kNoPair) {
            if ((rc = sd.fork())) return rc;
            if ((rc = launch_wgrad(w, ws, L, sd.get(), plain))) return rc;
            rc = launch_gemm(amode, p, g, st, o, np);
        }
        return rc;
    }

    int identity_coefficients(int C) const
    {
        if (ident_written) return PN2_OK;
        return launch_identity_coef(C, at<float>(pl.l1coef), st);
    }

    // layer l's per-channel sums -> grad_gamma, grad_beta and the coefficients of dz_l (unless the pass above did it, or the
    // statistics are frozen); then the helper stream's reads of the dy buffer this layer's data gradient overwrites
    int begin_layer(int l)
    {
        const pn2_bn_layer &L = layers[l];
        if (!folded[l] && !c.frozen)
            if (int rc = launch_bn_backward_finalize(stats(l), nparts[l], L.cout, (double)rows, row_count(), L.gamma, L.save, L.grad_gamma,
                                                     L.grad_beta, coef(l), L.grad_accumulate, st)) return rc;
        return sd.join();
    }

    // ---- the pooled top layer in terms of its input h = relu(a z_{l-1} + c): see tl_top_mats_kernel
    int pooled_top_without_z(int l)
    {
        const pn2_bn_layer &L = layers[l], &D = layers[l - 1];
        const int K = L.cin, NF = L.cout, tf = tiles(NF), NFp = tf * 32, ld = top_cols(K, NF);
        float *wp = at<float>(pl.topw), *rowc = wp + (size_t)(NFp + K) * K;
        double *sf = at<double>(pl.topsf);
        if (int rc = launch_top_mats(L.weight, L.w_stride_k, L.w_stride_n, K, NF, NFp, coef(l), nullptr, wp, rowc, st)) return rc;    // z_L = h W: no bias term
        // both variants: the routed gradient and h as the dense kernel's second operand, tl_top_wgrad_fix_kernel behind it
        TlWgrad w = wgrad_into_partial(rows, K);
        relu_input(w, D);
        w.dmode = A_FILL;
        w.G = gq; w.argsel = c.argsel; w.coef = coef(l); w.group_rows = pool_rows;
        auto fix = [&](int ldw, int tfw, const double *s64, hipStream_t s) {
            return launch_top_wgrad_fix(sf, ldw, K, NF, tfw * 32, tfw * 32 + tiles(K) * 32, L.weight, L.w_stride_k, L.w_stride_n, coef(l),
                                        nullptr, L.grad_weight, s64, L.grad_accumulate, s);
        };
        if (fz[l].ok) {
            // ---- ONE pass over z_{l-1}: the routed gradient and h as operand tiles of the block image serve the weight
            // gradient (S, Gram matrix, column sums: tl_top_wgrad_fix_kernel combines them) AND the data gradient
            // dy_{l-1} = [s dy routed | h] . [W^T ; -M] - r, masked by the layer below (as separate kernels z_{l-1} crossed
            // HBM in the data-gradient GEMM, in tl_top_s_kernel and in the Gram pass)
            if (int rc = launch_pack(wp, K, 1, one_slab(NFp + K, K, fz[l]), base + pl.pack[l], st)) return rc;
            w.NO = ld; w.tf = tf; w.NF = NF;
            w.xshare = 1;                                     // one slab: the "h again" tiles are the first operand's
            dy_in_wgrad(w, l, K);
            w.dy_tf = tf;
            dy_into_below(w, l);
            w.dy_bias = rowc;
            if (int rc = launch_wgrad(w, wz[l], L, st, sf)) return rc;
            nparts[l - 1] = (int)wz[l].gridx;
            return fix(ld, tf, nullptr, st);
        }
        // weight gradient: the routed part S on the vector units (tl_top_s_kernel) when its shape allows, the Gram
        // matrix h^T h and the column sums of h from the dense kernel, combined by tl_top_wgrad_fix_kernel;
        // data gradient: the GEMM over [routed gradient | h]. The dense kernel and the GEMM are independent passes over
        // z_{l-1}: one launch for both where the pair has a kernel (tl_pair_kernel)
        const TopSShape ts = top_s_shape(rows, pool_rows, K, NF, o);
        double *s64 = ts.ok ? at<double>(pl.tops64) : nullptr;
        const bool wg = !skip[l];                          // (frozen statistics: a layer without parameter gradients)
        if (int rc = sd.fork()) return rc;                 // the weight gradient's kernels beside the data gradient below
        if (ts.ok && wg) {
            TlTopS q;
            memset(&q, 0, sizeof(q));
            q.groups = rows / pool_rows; q.ns = pool_rows; q.K = K; q.NF = NF;
            q.z = D.z; q.pa = D.save + 2 * D.cout; q.pc = D.save + 3 * D.cout;
            q.gq = gq; q.argsel = c.argsel; q.coef = coef(l);
            q.partial = at<float>(pl.tops_part);
            if (int rc = launch_top_s(q, ts, at<float>(pl.tops_part2), s64, sd.get())) return rc;
        }
        const int tfw = ts.ok ? 0 : tf, ldw = ts.ok ? top_cols(K, 0) : ld;       // operand tiles of the dense kernel
        w.NO = ldw; w.tf = tfw; w.NF = ts.ok ? 0 : NF;
        const WgradShape ws_ = wgrad_shape(rows, K, ldw, false, cus, o.wgrad_two_per_cu);
        w.xshare = ws_.uslabs == 1;
        const GemmShape g = gemm_shape(rows, NFp + K, K, o);
        if (int rc = launch_pack(wp, K, 1, g, base + pl.pack[l], st)) return rc;
        TlGemm p;
        memset(&p, 0, sizeof(p));
        p.rows = rows;
        p.tk0 = tf; p.K0 = NF; p.K1 = K;
        p.G = gq; p.argsel = c.argsel; p.p0 = coef(l); p.group_rows = pool_rows;
        p.A2 = D.z; p.q0 = D.save + 2 * D.cout; p.q1 = D.save + 3 * D.cout;
        p.wpacked = at<const u32x4>(pl.pack[l]);
        p.bias = rowc;
        into_below(p, l);
        int np = 0;
        if (int rc = wg ? beside(A_FILL, p, g, w, ws_, L, rows, &np, sf) : launch_gemm(A_FILL, p, g, st, o, &np)) return rc;
        nparts[l - 1] = np;
        return wg ? fix(ldw, tfw, s64, sd.get()) : PN2_OK;
    }

    // ---- a level without features (or with a few whose gradient nobody wants -- the network's input normals): the
    // first layer's weight gradient on the vector units
    int layer1_coords_only()
    {
        const pn2_bn_layer &L = layers[0];
        if (l1_moment_parts) {                                // ... from x^T dy_1 of the pass above and the moments of x
            const TlGather gt = make_gather(c.group);
            return launch_l1_wx_combine(at<double>(pl.l1mom), l1_moment_parts, at<double>(pl.l1a), nparts[0], L.cout, L.cout, coef(0),
                                        L.weight + gt.xyz_off * L.w_stride_k, L.w_stride_k, L.w_stride_n,
                                        L.grad_weight + gt.xyz_off * L.w_stride_k, L.grad_accumulate, st);
        }
        // ... in one pass over dy_1 and z_1
        if (!skip[0])
            if (int rc = launch_l1_dz(rows, gd, c.group, L, gcur, coef(0), at<float>(pl.l1part), false, st)) return rc;
        return want_xyz ? xyz_pass(gcur, L.z, coef(0), nullptr, nullptr) : PN2_OK;
    }

    // Layer 1 per point / per known point, one half of W_1: dW_half = A^T D over hr rows (rows kc of the weight gradient from
    // row koff; kp: A's width as read) and, when gout is wanted, gout = D W_half^T beside it. D is dz_1 itself: the weight
    // gradient's pass takes the identity coefficients, which the caller has made sure of (identity_coefficients).
    // mask: the hr rows are the level's ragged rows (the FP node's points1 half). Both launches are then the MASKED kernels
    // (train_mlp_ragged.hip), which select zero for a padding row of A (points1 may hold NaN there) and of D: nothing of it enters
    // dW_half, and its row of gout is 0 + 0 products = all-zero bits. (D's padding rows are zeros in memory already, so the dense
    // GEMM would give the same; the masked one does not depend on that.) ragged_opts has no pair launch: two launches.
    int l1_half(long long hr, int kp, int kc, const float *A, const float *D, size_t pack, float *gout, int koff, long long pair_rows,
                const unsigned *mask = nullptr)
    {
        const pn2_bn_layer &L = layers[0];
        TlWgrad w = wgrad_into_partial(hr, kp);
        w.kout = kc; w.amode = A_PLAIN; w.A = A;
        w.dmode = A_DZ; w.NO = L.cout; w.Z = D; w.G = D; w.coef = at<float>(pl.l1coef);
        w.mask = mask;
        pn2_bn_layer Lh = L;
        Lh.grad_weight = L.grad_weight + (long long)koff * L.w_stride_k;
        const WgradShape ws_ = wgrad_shape(hr, kp, L.cout, false, cus, o.wgrad_two_per_cu);
        if (!gout) return launch_wgrad(w, ws_, Lh, st);
        TlGemm p = dense_gemm(hr, D, base + pack);
        p.mask = mask;
        plain_out(p, gout, kc);
        return beside(A_PLAIN, p, gemm_shape(hr, L.cout, kc, o), w, ws_, Lh, pair_rows, nullptr);
    }

    // ---- layer 1 of an FP level per KNOWN point (train_mlp_fp.hip): dz_1 in place, its interpolation gradient S onto
    // the known points, then each half of W_1 -- a weight gradient and a data gradient over its own rows. Ragged rows (c.mask):
    // dz_1 by the masked pass (zero on padding rows, where the interpolation weights are zero too: S gets 0 * 0 from them), the
    // known-points half dense, the rows half masked (l1_half)
    int layer1_fp()
    {
        const pn2_bn_layer &L = layers[0];
        float *S = at<float>(pl.l1p);
        if (int rc = fp_launch_l1_dz(rows, L.cout, L.z, gcur, coef(0), mask_words(), st)) return rc;
        if (int rc = fp->idx_plan ? pn2_three_interpolate_grad_planned(fp->b, fp->n, L.cout, fp->m, gcur, fp->idx_plan, fp->weight, S,
                                                                       c.reproducible, c.stream)
                                  : pn2_three_interpolate_grad_seg(fp->b, fp->n, L.cout, fp->m, gcur, fp->idx, fp->weight, S,
                                                                   base + pl.l1seg, c.reproducible, c.stream)) return rc;
        if (fp->mp > fp->bm)                                  // the padding rows of S meet the zero rows of points2's copy
            if (int rc = clear_async(S + fp->bm * L.cout, sizeof(float) * (size_t)(fp->mp - fp->bm) * L.cout, st)) return rc;
        if (int rc = identity_coefficients(L.cout)) return rc;
        const float *p2, *p1;
        if (int rc = fp_padded_inputs(p2, p1)) return rc;
        float *g2 = (fp->grad_points2 && fp->gstage2()) ? at<float>(pl.fpg2) : fp->grad_points2;
        if (int rc = l1_half(fp->mp, fp->c2p, fp->c2, p2, S, pl.pack[0], g2, 0, fp->mp)) return rc;
        if (g2 && g2 != fp->grad_points2)
            if (int rc = fp_launch_pad(g2, fp->bm, fp->c2, fp->bm, fp->c2, fp->grad_points2, st)) return rc;
        if (fp->c1 > 0) return l1_half(rows, fp->c1p, fp->c1, p1, gcur, pl.fpw, fp->grad_points1, fp->c2, rows, mask_words());
        return PN2_OK;
    }

    // ---- layer 1 once per point (see tl_l1_forward_kernel): dz_1 and dW1x in one pass over the rows, the scatter of
    // dz_1 onto the points, then two GEMMs over the b n points
    int layer1_per_point()
    {
        const pn2_bn_layer &L = layers[0];
        const TlGather gt = make_gather(c.group);
        const long long bn = (long long)gd.b * gd.n;
        float *S = at<float>(pl.l1p);
        if (int rc = launch_l1_dz(rows, gd, c.group, L, gcur, coef(0), at<float>(pl.l1part), true, st, !skip[0])) return rc;
        if (int rc = c.group->idx_plan ? pn2_group_point_grad_planned(gd.b, gd.n, L.cout, gd.m, gd.nsample, gcur, c.group->idx_plan, S,
                                                                      c.reproducible, c.stream)
                                       : pn2_group_point_grad_seg(gd.b, gd.n, L.cout, gd.m, gd.nsample, gcur, c.group->idx, S,
                                                                  base + pl.l1seg, c.reproducible, c.stream)) return rc;
        if (want_xyz)                                         // (gcur holds dz_1 now)
            if (int rc = xyz_pass(gcur, nullptr, nullptr, nullptr, S)) return rc;
        if (skip[0]) {                                        // frozen statistics, no dW_1 wanted: the data gradient alone
            if (!want_dx) return PN2_OK;
            TlGemm p = dense_gemm(bn, S, base + pl.pack[0]);
            plain_out(p, c.grad_points, gt.cfeat);
            return launch_gemm(A_PLAIN, p, gemm_shape(bn, L.cout, gt.cfeat, o), st, o);
        }
        if (int rc = identity_coefficients(L.cout)) return rc;
        // dW1f = points^T S; dPoints = S W1f^T: beside it, in one launch where the pair has a kernel
        // (the pair rule looks at the level's rows here, not at the b n points)
        return l1_half(bn, gt.cfeat, gt.cfeat, c.group->points, S, pl.pack[0], want_dx ? c.grad_points : nullptr, gt.feat_off, rows);
    }

    // ---- every other layer: the weight gradient from (dy_l, z_l, the layer's input), the data gradient into the layer below
    int generic_layer(int l)
    {
        const pn2_bn_layer &L = layers[l];
        const bool ptop = pooled_top(l);
        if (l == 0 && want_xyz)                                     // the generic gathered layer 1: from (dy_1, z_1), which nothing below overwrites
            if (int rc = xyz_pass(ptop ? gq : gcur, L.z, coef(0), ptop ? c.argsel : nullptr, nullptr)) return rc;
        // weight gradient
        TlWgrad w = wgrad_into_partial(rows, L.cin);
        if (l == 0 && c.group) { w.amode = A_GATHER; w.g = make_gather(c.group); }
        else if (l == 0) { w.amode = A_PLAIN; w.A = c.x; }
        else relu_input(w, layers[l - 1]);
        w.dmode = ptop ? A_DZ_POOL : A_DZ;
        w.NO = L.cout;
        w.Z = L.z;
        w.G = ptop ? gq : gcur;
        w.argsel = c.argsel;
        w.coef = coef(l);
        w.group_rows = pool_rows;
        w.mask = mask_words();
        if (fz[l].ok) {
            // ... and the data gradient in the same pass over (dy_l, z_l, z_{l-1}), see tl_wgrad_kernel
            dy_in_wgrad(w, l, L.cin);
            w.dy_tf = 0; w.dy_acopy = fz[l].acopy;
            if (l > 0) dy_into_below(w, l);
            else w.dy_out = c.grad_x;
            // (not with the coordinate gradients: g_r needs dy_1 row by row, so it is written and tl_l1_dz_kernel's pass runs)
            if (l == 1 && coords_only && gd.cfeat == 0 && !ptop && !want_xyz && !skip[0]) {            // (a pooled two-layer stack keeps the pass over dy_1: its dz comes from the routed gradient)
                // the layer below takes the three centred coordinates: dy_1 is wanted only as x^T dy_1 (TlWgrad::l1x) -- never
                // written, and tl_l1_dz_kernel's pass over (dy_1, z_1) is replaced by nine moments of x
                const pn2_bn_layer &D = layers[0];
                TlL1 q;
                memset(&q, 0, sizeof(q));
                q.rows = rows; q.n = gd.n; q.m = gd.m; q.nsample = gd.nsample; q.C = D.cout;
                q.xyz = c.group->xyz; q.new_xyz = c.group->new_xyz; q.idx = c.group->idx;
                if (int rc = launch_l1_xrows(q, at<float4>(pl.l1xg), at<double>(pl.l1mom), st, &l1_moment_parts)) return rc;
                w.l1x = at<const float4>(pl.l1xg);
                w.l1a = at<double>(pl.l1a);
                w.dy_out = nullptr;
            }
            if (int rc = launch_wgrad(w, wz[l], L, st)) return rc;
            if (l > 0) nparts[l - 1] = (int)wz[l].gridx;
            return PN2_OK;
        }
        const WgradShape ws_ = wgrad_shape(rows, L.cin, L.cout, w.amode == A_GATHER, cus, o.wgrad_two_per_cu);
        if (!below(l))                                         // no data gradient below this layer
            return skip[l] ? PN2_OK : launch_wgrad(w, ws_, L, st);
        // data gradient: independent of the weight gradient -- ONE launch for both where the pair has a kernel
        // (tl_pair_kernel), else the weight gradient first (on the helper stream when that is asked for)
        const int cfeat = (l == 0 && c.group) ? make_gather(c.group).cfeat : 0;
        const GemmShape g = (l == 0 && c.group) ? gemm_shape(rows, L.cout, cfeat, o) : gemm_shape(rows, L.cout, L.cin, o);
        TlGemm p = dense_gemm(rows, L.z, base + pl.pack[l]);
        p.G = ptop ? gq : gcur;
        p.argsel = c.argsel;
        p.p0 = coef(l); p.p1 = coef(l) + L.cout; p.p2 = coef(l) + 2 * L.cout;
        p.group_rows = pool_rows;
        p.mask = mask_words();
        if (l > 0) into_below(p, l);
        else if (c.group) plain_out(p, c.grad_feat_rows, cfeat);
        else plain_out(p, c.grad_x, L.cin);
        const int amode = ptop ? A_DZ_POOL : A_DZ;
        int np = 0;
        // (frozen statistics, no parameter gradient: the data gradient alone)
        if (int rc = skip[l] ? launch_gemm(amode, p, g, st, o, &np) : beside(amode, p, g, w, ws_, L, rows, &np)) return rc;
        if (l > 0) nparts[l - 1] = np;
        return PN2_OK;
    }

    // frozen statistics: the per-channel sums of every layer -> grad_gamma, grad_beta, grad_bias: one launch, behind the last
    // pass (nothing waits for it)
    int frozen_gradients() const
    {
        FrozenSums fs[8];
        for (int l = 0; l < nlayers; ++l) {
            fs[l].skip = skip[l];
            fs[l].stats = skip[l] ? nullptr : stats(l);
            fs[l].nparts = skip[l] ? 0 : nparts[l];
        }
        return frozen_launch_grads(nlayers, layers, fs, c.grad_bias, st);
    }

    int run()
    {
        if (int rc = prepare()) return rc;
        if (int rc = pack_weights()) return rc;
        if (c.frozen)
            if (int rc = frozen_coefficients()) return rc;
        if (int rc = top_gradient()) return rc;
        if (int rc = sd.init(st, o.side_stream == PN2_OPT_ON)) return rc;
        // top down; a layer-1 form is the last stage of its call, so nothing reads gcur / gnext behind it
        for (int l = nlayers - 1; l >= lo; --l) {
            if (int rc = begin_layer(l)) return rc;
            const int rc = (pooled_top(l) && ztop) ? pooled_top_without_z(l)
                         : l > 0 ? generic_layer(l)
                         : (coords_only && !(gd.cfeat > 0 && want_dx)) ? layer1_coords_only()
                         : fp ? layer1_fp()
                         : per_point ? layer1_per_point()
                         : generic_layer(0);
            if (rc) return rc;
            float *tmp = gcur; gcur = gnext; gnext = tmp;
        }
        if (c.frozen)
            if (int rc = frozen_gradients()) return rc;
        return sd.join();                                          // everything of this call is ordered before what the caller enqueues next
    }
};

int tl_train_backward(const TlCall &call) { return Bwd(call).run(); }

// a grouped level or plain rows, the max pool when pool_rows > 0 (the entries without a pooling argument)
static TlCall max_call(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group, const float *x, int pool_rows,
                       const float *out, const int *argsel, const float *zsel, void *ws, const pn2_train_opts *opts, void *stream)
{
    TlCall c{};
    c.rows = rows; c.nlayers = nlayers; c.layers = layers;
    c.group = group; c.x = x;
    c.pool_rows = pool_rows;
    c.out = out; c.argsel = argsel; c.zsel = zsel;
    c.ws = ws; c.opts = opts; c.stream = stream;
    return c;
}

// the workspace of the coordinate gradients behind the node's own (pn2_mlp_train_ws_bytes_xyz, train_mlp_xyz.hip)
long long tl_xyz_ws_bytes(long long rows, int nlayers, const int *widths, int pool_rows, int pooling, const int *group_dims,
                          const pn2_train_opts *opts)
{
    if (!widths || !group_dims || nlayers < 1 || nlayers > 8) return -1;
    const GroupDims gd = group_dims_of(group_dims);
    const Opts o = opts_of(opts);
    TlPlan pl;
    if (!tl_plan(rows, nlayers, widths, pooling ? 0 : pool_rows, 1, pl, &gd, o)) return -1;      // as pn2_mlp_train_ws_bytes_pool
    XyzPlan xp;
    if (!xyz_plan(pl, rows, nlayers, widths, gd, o, xp)) return -1;
    return (long long)xp.total;
}

// the workspace of the plain rows of a ragged batch (pn2_mlp_train_ws_bytes_ragged, train_mlp_ragged.hip): under ragged_opts
long long tl_ragged_ws_bytes(long long rows, int nlayers, const int *widths, int backward, const pn2_train_opts *opts)
{
    TlPlan pl;
    if (!tl_plan(rows, nlayers, widths, 0, backward, pl, nullptr, ragged_opts(opts))) return -1;
    return (long long)pl.total;
}

// The grouped rows of a ragged batch (pn2_mlp_train_*_group_ragged, train_mlp_ragged_group.hip). Supported: the dims describe the
// rows, and the dense node's plan takes the shape in both directions under ragged_group_opts (hence rows a positive multiple of
// 32 and groups of 16 or a multiple of 32 rows). The workspace is planned WITHOUT the pool, as both directions run: forward keeps
// no partial extrema, backward's top layer is an unpooled one.
bool tl_group_ragged_supported(long long rows, int nlayers, const int *widths, int pool_rows, const int *group_dims)
{
    if (!widths || !group_dims || nlayers < 1 || nlayers > 8 || pool_rows <= 0) return false;
    const GroupDims gd = group_dims_of(group_dims);
    if (gd.b <= 0 || gd.n <= 0 || gd.m <= 0 || gd.nsample <= 0 || gd.cfeat < 0) return false;
    if ((long long)gd.b * gd.m * gd.nsample != rows || pool_rows != gd.nsample || widths[0] != 3 + gd.cfeat) return false;
    if (!gd.has_idx && (gd.m != 1 || gd.nsample != gd.n)) return false;
    const Opts o = ragged_group_opts(nullptr);
    TlPlan pl;
    return tl_plan(rows, nlayers, widths, pool_rows, 0, pl, &gd, o) && tl_plan(rows, nlayers, widths, pool_rows, 1, pl, &gd, o);
}

long long tl_group_ragged_ws_bytes(long long rows, int nlayers, const int *widths, int pool_rows, int backward, const int *group_dims,
                                   const pn2_train_opts *opts)
{
    if (!tl_group_ragged_supported(rows, nlayers, widths, pool_rows, group_dims)) return -1;
    const GroupDims gd = group_dims_of(group_dims);
    TlPlan pl;
    if (!tl_plan(rows, nlayers, widths, 0, backward, pl, &gd, ragged_group_opts(opts))) return -1;
    return (long long)pl.total;
}

// the workspace of the FP level with layer 1 per known point (pn2_mlp_train_ws_bytes_fp, train_mlp_fp.hip); ragged: of its
// form with a row mask (pn2_mlp_train_ws_bytes_fp_ragged), planned under ragged_opts as its passes run
long long tl_fp_ws_bytes(const pn2_fp_src *s, int nlayers, const int *widths, int backward, const pn2_train_opts *opts, bool ragged)
{
    const FpL1 f = fp_l1(s);
    TlPlan pl;
    if (!tl_plan(f.rows, nlayers, widths, 0, backward, pl, nullptr, ragged ? ragged_opts(opts) : opts_of(opts), &f)) return -1;
    return (long long)pl.total;
}

// ---- what a ragged call launches on the matrix cores (pn2_mlp_train_ragged_plan / _fp_ragged_plan, include/pn2ops.h): host
// logic for tests and maintainers. It walks the layers as Fwd::run / Bwd::run do under a row mask -- ragged_opts: no fused data
// gradient, no pair launch, so generic_layer is launch_wgrad then launch_gemm, and l1_half the same -- and asks the rules the
// launches ask: gemm_shape, wgrad_shape with the device's CU count and the caller's wgrad_two_per_cu, prep_gemm for grid and nt.
struct RaggedPlanOut {
    int *rec;
    int cap, n;
    const Opts o;
    const int cus;
    int *next()
    {
        int *r = (rec && n < cap) ? rec + (size_t)n * PN2_RAGGED_PLAN_FIELDS : nullptr;
        ++n;
        if (r) memset(r, 0, sizeof(int) * PN2_RAGGED_PLAN_FIELDS);
        return r;
    }
    void head(int *r, int kind, int backward, int layer, bool masked, long long rows, int K, int N) const
    {
        r[0] = kind; r[1] = backward; r[2] = layer + 1; r[3] = masked ? 1 : 0; r[4] = (int)rows; r[5] = K; r[6] = N;
    }
    // a GEMM over `rows` rows, K -> N channels, as launch_gemm(amode, p, gemm_shape(rows, K, N, o), st, o) shapes it
    void gemm(int backward, int layer, bool masked, long long rows, int amode, int K, int N)
    {
        const GemmShape g = gemm_shape(rows, K, N, o);
        TlGemm p;
        memset(&p, 0, sizeof(p));
        p.rows = rows;
        const dim3 grid = prep_gemm(p, g, o);
        int *r = next();
        if (!r) return;
        head(r, 0, backward, layer, masked, rows, K, N);
        r[7] = g.ns; r[8] = amode; r[9] = g.resident ? 1 : 0; r[10] = g.slabs; r[11] = p.nt; r[12] = (int)grid.x;
    }
    // a weight-gradient pass over `rows` rows, KI input and NO output channels, as launch_wgrad(w, wgrad_shape(...), L, st) shapes it
    // (gather: layer 1 of a grouped level, tl_wgrad_masked_gather_kernel -- field [3] is 2 then)
    void wgrad(int layer, bool masked, long long rows, int KI, int NO, bool gather = false)
    {
        const WgradShape w = wgrad_shape(rows, KI, NO, gather, cus, o.wgrad_two_per_cu);
        int *r = next();
        if (!r) return;
        head(r, 1, 1, layer, masked, rows, KI, NO);
        if (gather) r[3] = 2;
        r[7] = w.tpw; r[8] = w.upw; r[9] = w.two ? 1 : 0; r[10] = w.uslabs * w.tslabs; r[11] = w.tus; r[12] = (int)w.gridx; r[13] = w.tts;
    }
    // layers lo..L-1 of a direction where they are Fwd / Bwd::generic_layer with the mask (plain rows: from layer 0; FP: from 1)
    void generic_forward(long long rows, int nlayers, const int *widths, int lo)
    {
        for (int l = lo; l < nlayers; ++l) gemm(0, l, true, rows, l == 0 ? A_PLAIN : A_RELU, widths[l], widths[l + 1]);
    }
    void generic_backward(long long rows, int nlayers, const int *widths, int lo)
    {
        for (int l = nlayers - 1; l >= lo; --l) {
            wgrad(l, true, rows, widths[l], widths[l + 1]);
            gemm(1, l, true, rows, A_DZ, widths[l + 1], widths[l]);    // (below(l): l > 0, or grad_x wanted)
        }
    }
};

int tl_ragged_plan(long long rows, int nlayers, const int *widths, const pn2_train_opts *opts, int *passes, int cap)
{
    RaggedPlanOut po = {passes, cap, 0, ragged_opts(opts), device_cus()};
    po.generic_forward(rows, nlayers, widths, 0);
    po.generic_backward(rows, nlayers, widths, 0);
    return po.n;
}

// the grouped rows of a ragged batch, under ragged_group_opts: Fwd::generic_layer(0) is the masked gathered GEMM, the layers above
// it the plain rows' masked passes; Bwd::generic_layer(0) the masked gathered weight-gradient pass and -- with features -- the
// masked A_DZ GEMM onto their cfeat columns. The pool and its gradient are vector-unit passes and not listed.
int tl_group_ragged_plan(long long rows, int nlayers, const int *widths, const int *group_dims, const pn2_train_opts *opts, int *passes,
                         int cap)
{
    const GroupDims gd = group_dims_of(group_dims);
    RaggedPlanOut po = {passes, cap, 0, ragged_group_opts(opts), device_cus()};
    po.gemm(0, 0, true, rows, A_GATHER, widths[0], widths[1]);
    po.generic_forward(rows, nlayers, widths, 1);
    po.generic_backward(rows, nlayers, widths, 1);
    po.wgrad(0, true, rows, widths[0], widths[1], true);
    if (gd.cfeat > 0) po.gemm(1, 0, true, rows, A_DZ, widths[1], gd.cfeat);
    return po.n;
}

int tl_fp_ragged_plan(const pn2_fp_src *s, int nlayers, const int *widths, const pn2_train_opts *opts, int *passes, int cap)
{
    const FpL1 f = fp_l1(s);
    const int C1 = widths[1];
    RaggedPlanOut po = {passes, cap, 0, ragged_opts(opts), device_cus()};
    // Fwd::layer1_fp: Q over the known points and points1 W1b over the rows, both dense store GEMMs
    po.gemm(0, 0, false, f.mp, A_PLAIN, f.c2p, C1);
    if (f.c1 > 0) po.gemm(0, 0, false, f.rows, A_PLAIN, f.c1p, C1);
    po.generic_forward(f.rows, nlayers, widths, 1);
    po.generic_backward(f.rows, nlayers, widths, 1);
    // Bwd::layer1_fp -> l1_half: the known-points half dense, the rows half masked
    po.wgrad(0, false, f.mp, f.c2p, C1);
    po.gemm(1, 0, false, f.mp, A_PLAIN, C1, f.c2);
    if (f.c1 > 0) {
        po.wgrad(0, true, f.rows, f.c1p, C1);
        po.gemm(1, 0, true, f.rows, A_PLAIN, C1, f.c1);
    }
    return po.n;
}
}  // namespace pn2

extern "C" int pn2_mlp_train_ragged_plan(int b, int n, int nlayers, const int *widths, const pn2_train_opts *opts, int *passes, int cap)
{
    if (!widths) return PN2_E_NULL;
    if (cap < 0 || !pn2_mlp_train_ragged_supported(b, n, nlayers, widths)) return PN2_E_ARG;
    return pn2::tl_ragged_plan((long long)b * n, nlayers, widths, opts, passes, cap);
}

extern "C" int pn2_mlp_train_fp_ragged_plan(int b, int n, int m, int c2, int c1, int nlayers, const int *widths,
                                            const pn2_train_opts *opts, int *passes, int cap)
{
    if (!widths) return PN2_E_NULL;
    if (cap < 0 || !pn2_mlp_train_fp_ragged_supported(b, n, m, c2, c1, nlayers, widths)) return PN2_E_ARG;
    pn2_fp_src s;
    memset(&s, 0, sizeof(s));
    s.b = b; s.n = n; s.m = m; s.c2 = c2; s.c1 = c1;
    return pn2::tl_fp_ragged_plan(&s, nlayers, widths, opts, passes, cap);
}

extern "C" int pn2_mlp_train_forward(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                     const float *x, int pool_rows, float *out, int *argsel, float *zsel, void *ws, void *stream)
{
    return pn2_mlp_train_forward_ex(rows, nlayers, layers, group, x, pool_rows, out, argsel, zsel, ws, nullptr, stream);
}

extern "C" int pn2_mlp_train_forward_ex(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                        const float *x, int pool_rows, float *out, int *argsel, float *zsel, void *ws,
                                        const pn2_train_opts *opts, void *stream)
{
    return pn2::tl_train_forward(pn2::max_call(rows, nlayers, layers, group, x, pool_rows, out, argsel, zsel, ws, opts, stream));
}

extern "C" int pn2_mlp_train_backward(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                      const float *x, int pool_rows, const float *out, const int *argsel, const float *zsel,
                                      const float *grad_out, float *grad_x, float *grad_feat_rows, float *grad_points,
                                      int reproducible, void *ws, void *stream)
{
    return pn2_mlp_train_backward_ex(rows, nlayers, layers, group, x, pool_rows, out, argsel, zsel, grad_out, grad_x, grad_feat_rows,
                                     grad_points, reproducible, ws, nullptr, stream);
}

extern "C" int pn2_mlp_train_backward_ex(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                         const float *x, int pool_rows, const float *out, const int *argsel, const float *zsel,
                                         const float *grad_out, float *grad_x, float *grad_feat_rows, float *grad_points,
                                         int reproducible, void *ws, const pn2_train_opts *opts, void *stream)
{
    pn2::TlCall c = pn2::max_call(rows, nlayers, layers, group, x, pool_rows, out, argsel, zsel, ws, opts, stream);
    c.grad_out = grad_out;
    c.grad_x = grad_x; c.grad_feat_rows = grad_feat_rows; c.grad_points = grad_points;
    c.reproducible = reproducible;
    return pn2::tl_train_backward(c);
}

// ---- the pooling modes of the training node (pn2_mlp_train_*_pool, include/pn2ops.h) -------------------------------------
extern "C" int pn2_mlp_train_pool_supported(long long rows, int nlayers, const int *widths, int pool_rows, int pooling)
{
    pn2::TlPlan pl;
    if (!widths || nlayers < 1 || nlayers > 8 || pooling < 0 || pooling > 3 || (pooling && pool_rows <= 0)) return 0;
    if (pool_rows && rows % pool_rows) return 0;
    const pn2::Opts o = pn2::opts_of(nullptr);
    if (!pn2::tl_plan(rows, nlayers, widths, pool_rows, 0, pl, nullptr, o)) return 0;
    return pn2::tl_plan(rows, nlayers, widths, pooling ? 0 : pool_rows, 1, pl, nullptr, o) ? 1 : 0;
}

extern "C" long long pn2_mlp_train_ws_bytes_pool(long long rows, int nlayers, const int *widths, int pool_rows, int pooling,
                                                 int backward, const int *group_dims, const pn2_train_opts *opts)
{
    if (pooling == 0) return pn2_mlp_train_ws_bytes_ex(rows, nlayers, widths, pool_rows, backward, group_dims, opts);
    if (pooling < 0 || pooling > 3 || pool_rows <= 0 || !widths || nlayers < 1 || nlayers > 8) return -1;
    const long long b = pn2_mlp_train_ws_bytes_ex(rows, nlayers, widths, backward ? 0 : pool_rows, backward, group_dims, opts);
    if (b < 0 || backward || pooling != 3 || rows % pool_rows) return b;
    return b + (long long)pn2::align_up((size_t)(rows / pool_rows) * widths[nlayers] * sizeof(float));   // the max half (forward)
}

extern "C" int pn2_mlp_train_forward_pool(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                          int pool_rows, int pooling, float *out, int *argsel, float *zsel, float *pool_w, void *ws,
                                          const pn2_train_opts *opts, void *stream)
{
    if (int rc = pn2::tl_pool_args(pool_rows, pooling, group != nullptr)) return rc;
    pn2::TlCall c = pn2::max_call(rows, nlayers, layers, group, nullptr, pool_rows, out, argsel, zsel, ws, opts, stream);
    c.pooling = pooling; c.pool_w = pool_w;
    return pn2::tl_train_forward(c);
}

extern "C" int pn2_mlp_train_backward_pool(long long rows, int nlayers, const pn2_bn_layer *layers, const pn2_group_src *group,
                                           int pool_rows, int pooling, const float *out, const int *argsel, const float *zsel,
                                           const float *pool_w, const float *grad_out, float *grad_feat_rows, float *grad_points,
                                           int reproducible, void *ws, const pn2_train_opts *opts, void *stream)
{
    if (int rc = pn2::tl_pool_args(pool_rows, pooling, group != nullptr)) return rc;
    pn2::TlCall c = pn2::max_call(rows, nlayers, layers, group, nullptr, pool_rows, out, argsel, zsel, ws, opts, stream);
    c.pooling = pooling; c.pool_w = pool_w;
    c.grad_out = grad_out;
    c.grad_feat_rows = grad_feat_rows; c.grad_points = grad_points;
    c.reproducible = reproducible;
    return pn2::tl_train_backward(c);
}
