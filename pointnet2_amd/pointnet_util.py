"""PointNet++ layer library on the MI355X operators -- the consumer side of the
drop-in boundary (reference utils/pointnet_util.py: sample_and_group :22,
sample_and_group_all :59, pointnet_sa_module :87, pointnet_sa_module_msg :156,
pointnet_fp_module :199).

The geometric part (sampling, grouping, interpolation) calls the HIP operators;
the learned part (1x1 conv + BN + ReLU stacks, the reference's tf_util.conv2d)
is plain torch.nn -- it is outside the hot path this package accelerates.
TF builds its variables inside `tf.variable_scope`; in torch the equivalent
state lives in nn.Module objects, so each reference *function* with learned
weights has a Module twin here (PointnetSAModule, PointnetSAModuleMSG,
PointnetFPModule) whose forward() follows the reference function line by line
in behaviour (concat order, pooling modes, weight formula).
"""
import torch
import torch.nn as nn

from .tf_sampling import farthest_point_sample, farthest_point_sample_gather, gather_point, mark_fps_ordered
from .tf_grouping import (query_ball_point, group_point, knn_point, query_ball_group_xyz,
                          query_ball_group_xyz_msg, sample_and_group_xyz)
from .tf_interpolate import three_nn, three_interpolate, fp_interp_concat
from ._tensors import lengths_for, packed_args, packed_pairs, ragged_lengths, require, use_segmented_grad
from . import sa_mlp
from . import train_mlp
from .geometry import FPGeometry, SAGeometry
from .index_plan import index_plan


def _grouped_input(xyz, points, idx, new_xyz, use_xyz, xyz_first, plan=None, grouped_xyz=None):
    """The input of a level's layer stack behind idx (:45-50; the MSG module's :179-184): group xyz and subtract the centroid,
    group the features, concatenate in the level's channel order -- xyz_first: [xyz, features], the single-scale module's (:50);
    False: features FIRST, the MSG module's (:184). grouped_xyz: a fused launch has grouped and centred xyz already (xyz and
    new_xyz are not looked at). plan: the index plan of idx for both gathers' backward.
    -> new_points (b, m, nsample, C), grouped_xyz (b, m, nsample, 3)"""
    if grouped_xyz is None:
        grouped_xyz = group_point(xyz, idx, plan=plan) - new_xyz.unsqueeze(2)
    if points is None:
        return grouped_xyz, grouped_xyz
    grouped_points = group_point(points, idx, plan=plan)
    if use_xyz:
        grouped_points = torch.cat([grouped_xyz, grouped_points] if xyz_first else [grouped_points, grouped_xyz], dim=-1)
    return grouped_points, grouped_xyz


def _valid_row_list(valid):
    """The valid rows of a (b, m) mask as the (total,) row list of index_select / _scatter_rows. nonzero() SYNCHRONISES (the host
    reads how many there are): only the compacting "unfused_ragged" paths come here."""
    return valid.reshape(-1).nonzero().squeeze(1)


def _sample_and_group_packed(npoint, radius, nsample, xyz, points, use_xyz, offsets, max_points, knn=False, npoints=None):
    """sample_and_group on a packed batch: packed FPS + gather and packed ball query + group (two launches, no host
    synchronisation, capturable), indices GLOBAL -- rows of the flat array --, so the features are group_point on the flat view
    (1, total, c). xyz carries no gradient here (the packed operators are not differentiable).
    knn / npoints (set_packed_pairs(True)): packed kNN in the ball query's place -- grouped_xyz is then the gathered rows minus
    the centroid, as on the padded kNN route -- and per-cloud sample counts, which are the query side's lengths2; a fill row's
    group is nsample times the cloud's own first row."""
    offs, b, total, nmax = packed_args(offsets, max_points, None, xyz, "sample_and_group")
    m, ns = int(npoint), int(nsample)
    if npoints is None and not knn:
        _, new_xyz = farthest_point_sample_gather(m, xyz, offsets=offs, max_points=nmax)
        idx, _, grouped_xyz = query_ball_group_xyz(radius, ns, xyz, new_xyz, True, offsets=offs, max_points=nmax, global_idx=True)
    else:
        _, new_xyz = farthest_point_sample_gather(m, xyz, npoints=npoints, offsets=offs, max_points=nmax)
        if knn:
            _, idx = knn_point(ns, xyz, new_xyz, lengths2=npoints, offsets=offs, max_points=nmax, global_idx=True)
            grouped_xyz = group_point(xyz.reshape(1, total, 3), idx.view(1, b * m, ns)).view(b, m, ns, 3) - new_xyz.unsqueeze(2)
        else:
            idx, _, grouped_xyz = query_ball_group_xyz(radius, ns, xyz, new_xyz, True, lengths2=npoints, offsets=offs, max_points=nmax,
                                                       global_idx=True)
    if points is not None:
        require(points.dim() == 2 and points.shape[0] == total, "sample_and_group: with offsets, points is (total, channel)")
        points = points.reshape(1, total, points.shape[1])
    new_points, _ = _grouped_input(None, points, idx.view(1, b * m, ns), None, use_xyz, True, grouped_xyz=grouped_xyz.view(1, b * m, ns, 3))
    return new_xyz, new_points.view(b, m, ns, new_points.shape[3]), idx, grouped_xyz


def sample_and_group(npoint, radius, nsample, xyz, points, knn=False, use_xyz=True, fused=None, lengths=None, npoints=None, offsets=None,
                     max_points=None):
    """reference: pointnet_util.py:22-56.

    xyz (b, ndataset, 3), points (b, ndataset, channel) or None
    -> new_xyz (b, npoint, 3), new_points (b, npoint, nsample, 3+channel),
       idx (b, npoint, nsample), grouped_xyz (b, npoint, nsample, 3)

    fused: use the fused kernels for the xyz branch (bit-identical values): the single overlapped
    launch of csrc/sa_fused.hip (or, with knn, FPS+gather in one launch). Default: whenever xyz
    needs no gradient.
    lengths: (b,) per-cloud point counts of a ragged batch (cloud i is xyz[i, :lengths[i]], points[i, :lengths[i]]): sampling
    and grouping see each cloud's own points only (the ragged operators; FPS + gather and ball query + group as two
    launches), idx names valid rows only, so the padding rows are never gathered.
    npoints: (b,) per-cloud sample counts (cloud i yields npoints[i] <= npoint centroids): centroid rows from npoints[i] on
    repeat sample 0 and their groups are idx 0 (point 0: valid, so the padding rows of xyz / points are still never
    gathered); on the fused ball-query route their grouped_xyz is +0.0, elsewhere point 0 minus the centroid (= +0.0 as well).
    offsets / max_points: a PACKED batch -- xyz (total, 3) and points (total, channel) hold the clouds back to back, cloud i is
    rows offsets[i] .. offsets[i + 1] - 1 (offsets (b + 1,) on the device, max_points a host int bounding every cloud's count).
    new_xyz, new_points and grouped_xyz come back dense (b, npoint, ...) and are each cloud's dense results; idx holds GLOBAL
    rows of the flat arrays. Not with lengths / npoints / knn, and xyz gets no gradient (ValueError where it wants one).
    Under set_packed_pairs(True) knn and npoints are offered with offsets too (_sample_and_group_packed): the results are the
    padded call's with lengths= / npoints= on the padded copy, idx shifted by offsets[i].
    """
    if offsets is not None:
        pairs = packed_pairs()
        require(lengths is None and (npoints is None or pairs), "sample_and_group: offsets and lengths / npoints are two layouts; give one")
        require(not knn or pairs, "sample_and_group: knn is not offered with offsets")
        require(not (torch.is_grad_enabled() and isinstance(xyz, torch.Tensor) and xyz.requires_grad),
                "sample_and_group: with offsets xyz gets no gradient; detach it")
        return _sample_and_group_packed(npoint, radius, nsample, xyz, points, use_xyz, offsets, max_points, knn, npoints)
    if fused is None:
        fused = not (torch.is_grad_enabled() and xyz.requires_grad)
    if lengths is not None:
        lengths = lengths_for(lengths, xyz)
    if npoints is not None:
        npoints = lengths_for(npoints, xyz, "npoints")
    grouped_xyz = None
    if fused and not knn:
        _, new_xyz, idx, _, grouped_xyz = sample_and_group_xyz(npoint, radius, nsample, xyz, True, lengths=lengths,
                                                               npoints=npoints)   # :40-46
    else:
        if fused:
            _, new_xyz = farthest_point_sample_gather(npoint, xyz, lengths=lengths, npoints=npoints)   # :40 in one launch
        else:
            fps_idx = farthest_point_sample(npoint, xyz, lengths=lengths, npoints=npoints)
            new_xyz = gather_point(xyz, fps_idx)                              # :40
            if npoints is None:
                new_xyz = mark_fps_ordered(new_xyz)
        if knn:
            _, idx = knn_point(nsample, xyz, new_xyz, lengths1=lengths, lengths2=npoints)           # :42
        else:
            idx, _ = query_ball_point(radius, nsample, xyz, new_xyz, lengths1=lengths, lengths2=npoints)   # :44
    # :45-50 (translation normalisation, xyz FIRST); the fused launch has done :45-46
    new_points, grouped_xyz = _grouped_input(xyz, points, idx, new_xyz, use_xyz, True, grouped_xyz=grouped_xyz)
    return new_xyz, new_points, idx, grouped_xyz


def _all_in_one_group(xyz):
    """The geometry of a group_all level (:72-74): one centroid at the origin, one group naming every point."""
    b, n, _ = xyz.shape
    new_xyz = torch.zeros((b, 1, 3), dtype=torch.float32, device=xyz.device)
    idx = torch.arange(n, dtype=torch.int32, device=xyz.device).reshape(1, 1, n).repeat(b, 1, 1)
    return new_xyz, idx


def sample_and_group_all(xyz, points, use_xyz=True):
    """reference: pointnet_util.py:59-84 (one group holding every point, centroid (0,0,0))."""
    new_xyz, idx = _all_in_one_group(xyz)
    grouped_xyz = xyz.reshape(xyz.shape[0], 1, xyz.shape[1], 3)
    if points is not None:
        new_points = torch.cat([xyz, points], dim=2) if use_xyz else points
        new_points = new_points.unsqueeze(1)
    else:
        new_points = grouped_xyz
    return new_xyz, new_points, idx, grouped_xyz


def _inverse_distance_weights(dist):
    """three_nn's squared distances -> the interpolation weights of pointnet_fp_module (pointnet_util.py:212-215)."""
    inv = 1.0 / torch.clamp(dist, min=1e-10)                                  # :212
    return inv / inv.sum(dim=2, keepdim=True)                                 # :213-215


def three_nn_weights(xyz1, xyz2, lengths1=None, lengths2=None):
    """Inverse-squared-distance weights of pointnet_fp_module (pointnet_util.py:211-215).
    lengths1: (b,) per-cloud counts of a ragged unknown side (three_nn): rows beyond the length get idx (0,0,0) and the
    finite weights (1/3, 1/3, 1/3).
    lengths2: (b,) per-cloud counts of a ragged known side (three_nn): a cloud with fewer than three known points has +inf
    distances on the missing neighbours, hence weight 0 there -- the weights stay finite."""
    dist, idx = three_nn(xyz1, xyz2, lengths1=lengths1, lengths2=lengths2)
    return idx, _inverse_distance_weights(dist)


def use_tf_moving_variance(model, flag=True):
    """Make every batch norm of `model` feed the BIASED batch variance (tf.nn.moments: 1 / N) to its running variance in the
    fused training path instead of torch's unbiased one (var * N / (N - 1); a relative difference of 1 / N, 2.4e-4 on a
    4,096-row level). pn2_bn_layer.running_var_biased. WHICH convention the reference has depends on the TensorFlow it runs
    on: its live path is tf.contrib.layers.batch_norm (tf_util.py:526-531; the tf.nn.moments code at :487-510 is
    batch_norm_template_unused). With `fused` off -- the default of the TF 1.2 the README names -- contrib's moving
    variance receives tf.nn.moments' biased variance (flag=True reproduces that); where contrib takes the fused kernel
    (the default of later TF 1.x for rank-2/4 inputs) the moving average receives the Bessel-corrected variance, which is
    torch's convention (leave the flag off). Not a parity claim by itself: pick the convention of the checkpoint you load.
    The layer-by-layer torch path always keeps torch's convention."""
    for mod in model.modules():
        if isinstance(mod, (nn.BatchNorm1d, nn.BatchNorm2d)):
            mod.running_var_biased = bool(flag)
    return model


def _no_packing_under_capture():
    """Packing folds the batch norms on the host (.cpu()) and uploads pageable memory: both are illegal
    while a HIP graph is being captured. Fail with an instruction instead of corrupting the capture."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("the fused MLP weights are not packed yet (or changed): call module.prepare_fused(device) -- "
                           "or run one eager eval forward -- before capturing a graph")


def _train_fused_ok(mod, stacks, pooling, group_all, xyz, points, m=None):
    """Training (batch-statistics batch norm, autograd) of a set-abstraction module on stacks pn2_mlp_train_forward covers: conv
    1x1 + BN + ReLU triples, rows a multiple of 32, nsample 16 or a multiple of 32 (train_mlp.py); avg / weighted_avg /
    max_and_avg where pn2_mlp_train_pool_supported says so. stacks: [(net, nsample)] -- the module's one stack, or one per
    radius of an MSG module (which asks with pooling "max"); every one of them must be covered.
    m: the centroid rows per cloud of xyz when that is not mod.npoint (the flat view of a packed batch: one cloud of
    B npoint centroids)."""
    if not mod.fused_mlp or not mod.training or not xyz.is_cuda:
        return False
    want_xyz = torch.is_grad_enabled() and xyz.requires_grad
    if (want_xyz and not mod.fused_xyz_grad) or (points is not None and not mod.use_xyz):
        return False
    b, n, _ = xyz.shape
    m = 1 if group_all else (mod.npoint if m is None else m)
    if want_xyz:                                   # (never weighted_avg: its weights depend on xyz)
        cfeat = points.shape[2] if points is not None else 0
        return all(train_mlp.xyz_grad_supported(net, b * m * ns, ns, pooling, b, n, m, cfeat, not group_all) for net, ns in stacks)
    if pooling != "max":
        return all(train_mlp.pool_supported(net, b * m * ns, ns, pooling) for net, ns in stacks)
    return all(train_mlp.stack_supported(net, b * m * ns, ns, True) for net, ns in stacks)


def _frozen_ok(mod, stacks, pooling, group_all, xyz, points, m=None):
    """Autograd through stacks whose batch norms all normalise with their running statistics (fused_frozen_bn): something
    must want a gradient -- an input (xyz only with fused_xyz_grad, as in training) or a parameter of a stack -- and
    pn2_mlp_train_frozen_supported must cover every stack. What the batch-statistics node refuses is refused here too."""
    if not mod.fused_frozen_bn or not mod.fused_mlp or not torch.is_grad_enabled() or not xyz.is_cuda:
        return False
    want_xyz = xyz.requires_grad
    if (want_xyz and not mod.fused_xyz_grad) or (points is not None and not mod.use_xyz):
        return False
    if not (want_xyz or (points is not None and points.requires_grad) or
            any(p.requires_grad for net, _ in stacks for p in net.parameters())):
        return False
    b, n, _ = xyz.shape
    m = 1 if group_all else (mod.npoint if m is None else m)
    dims = (b, n, m, points.shape[2] if points is not None else 0, not group_all) if want_xyz else None
    return all(train_mlp.frozen_supported(net, b * m * ns, ns, True, pooling, dims) for net, ns in stacks)


def _train_mode(mod, stacks, pooling, group_all, xyz, points, m=None):
    """"fused_train" (batch statistics), "fused_frozen" (running statistics, opt-in) or None: which fused autograd node."""
    if _train_fused_ok(mod, stacks, pooling, group_all, xyz, points, m):
        return "fused_train"
    return "fused_frozen" if _frozen_ok(mod, stacks, pooling, group_all, xyz, points, m) else None


def _ragged_train_ok(mod, stacks, group_all, xyz, points):
    """fused_ragged_train (opt-in): can the masked fused training node (train_mlp.sa_mlp_train(..., counts=)) run this module's
    stacks on the grouped rows of a ragged batch? Max pooling without mlp2 is the caller's to check; xyz must need no gradient
    (the node has no coordinate gradients). stacks: [(net, nsample)], as _train_fused_ok."""
    if not mod.fused_ragged_train or not mod.fused_mlp or not mod.training or not xyz.is_cuda:
        return False
    if (torch.is_grad_enabled() and xyz.requires_grad) or (points is not None and not mod.use_xyz):
        return False
    b, n, _ = xyz.shape
    m = 1 if group_all else mod.npoint
    cfeat = points.shape[2] if points is not None else 0
    return all(train_mlp.group_ragged_supported(net, b, n, m, ns, cfeat, not group_all) for net, ns in stacks)


def _masked_pool(x, valid, dists, pooling):
    """pointnet_sa_module's pooling (:128-142) of x (b, C, m, k) over the VALID entries of its last axis: valid (b, k) bool,
    dists (b, m, k, 1) the grouped points' distances from the centroid (weighted_avg). Selects, not products: an entry that is
    not valid may hold anything. No host synchronisation."""
    b, k = valid.shape
    v = valid.view(b, 1, 1, k)
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    cnt = valid.sum(dim=1).clamp(min=1).to(x.dtype).view(b, 1, 1, 1)
    if pooling == "max":
        return torch.where(v, x, torch.full((), float("-inf"), dtype=x.dtype, device=x.device)).max(dim=3, keepdim=True)[0]
    if pooling == "avg":
        return torch.where(v, x, zero).sum(dim=3, keepdim=True) / cnt
    if pooling == "weighted_avg":                                     # :130-136
        w = torch.where(valid.view(b, 1, k, 1), torch.exp(-dists * 5), zero)
        w = (w / w.sum(dim=2, keepdim=True)).permute(0, 3, 1, 2)
        return (torch.where(v, x, zero) * w).sum(dim=3, keepdim=True)
    if pooling == "max_and_avg":                                      # :137-140: concat([avg, max])
        return torch.cat([_masked_pool(x, valid, dists, "avg"), _masked_pool(x, valid, dists, "max")], dim=1)
    raise ValueError("unknown pooling %r" % (pooling,))


def _valid_rows(counts, b, m, dev, name="npoints"):
    """(b, m) bool: row j of cloud c is below counts[c] (clamped into 1..m, as the kernels clamp it). No host synchronisation."""
    cnts = ragged_lengths(counts, b, dev, name).clamp(1, max(m, 1))
    return torch.arange(m, device=dev, dtype=torch.int32).unsqueeze(0) < cnts.unsqueeze(1)


def _zero_padding_rows(out, valid):
    """Exact zeros on the rows that belong to no valid centroid / point (a torch.where: NaN-proof, no host synchronisation)."""
    return torch.where(valid.unsqueeze(2), out, torch.zeros((), dtype=out.dtype, device=out.device))


def _scatter_rows(yv, rows, total_rows):
    """(len(rows), C) -> (total_rows, C) with yv on `rows` and exact zeros elsewhere (differentiable)."""
    return torch.zeros((total_rows, yv.shape[1]), dtype=yv.dtype, device=yv.device).index_copy(0, rows, yv)


class _SharedMLP(nn.Module):
    """Stack of tf_util.conv2d([1,1]) + BN + ReLU (tf_util.py conv2d; BN eps 1e-3 is
    tf.contrib.layers.batch_norm's default). Operates on (b, C, h, w)."""

    def __init__(self, c_in, widths, bn=True):
        super().__init__()
        layers = []
        for w in widths:
            layers.append(nn.Conv2d(c_in, w, kernel_size=1, bias=True))
            if bn:
                layers.append(nn.BatchNorm2d(w, eps=1e-3))
            layers.append(nn.ReLU(inplace=True))
            c_in = w
        self.net = nn.Sequential(*layers)
        self.c_out = c_in
        self.widths = tuple(widths)

    def folded_layers(self, zero_xyz_rows=None):
        """[(W (cin, cout), b (cout))] with eval-mode batch norm folded in (sa_mlp.fold_batch_norm).
        zero_xyz_rows: "first" / "last" -- three ZERO rows added to the first layer's weight where the fused kernels feed the
        grouped coordinates (use_xyz=False levels, pointnet_util.py:49-52: the coordinates then contribute exact zeros to
        every sum, which is the layer stack on the features alone)."""
        out, mods = [], list(self.net)
        for i, mod in enumerate(mods):
            if isinstance(mod, nn.Conv2d):
                bn = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d) else None
                out.append(sa_mlp.fold_batch_norm(mod.weight, mod.bias, bn))
        if zero_xyz_rows is not None:
            import numpy as np
            w, b = out[0]
            z = np.zeros((3, w.shape[1]), dtype=w.dtype)
            out[0] = (np.concatenate([z, w] if zero_xyz_rows == "first" else [w, z], axis=0), b)
        return out

    def forward(self, x):
        return self.net(x)


class PointnetSAModule(nn.Module):
    """reference: pointnet_sa_module, pointnet_util.py:87-154."""

    def __init__(self, c_in, npoint, radius, nsample, mlp, mlp2=None, group_all=False, bn=True, pooling="max",
                 knn=False, use_xyz=True, use_nchw=False):
        super().__init__()
        # use_nchw (:87, :101): the reference's conv2d data-format switch -- "usually faster than NHWC" on its backend, the
        # same numbers either way. Accepted for signature parity and ignored: the layouts here are the kernels' own.
        if pooling not in ("max", "avg", "weighted_avg", "max_and_avg"):
            raise ValueError("unknown pooling %r" % (pooling,))
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        self.group_all, self.pooling, self.knn, self.use_xyz = group_all, pooling, knn, use_xyz
        self.c_in = c_in
        feat = 3 if c_in == 0 else (c_in + 3 if use_xyz else c_in)
        self.mlp = _SharedMLP(feat, mlp, bn)
        c = self.mlp.c_out * (2 if pooling == "max_and_avg" else 1)
        self.mlp2 = _SharedMLP(c, mlp2, bn) if mlp2 else None
        self.fused_mlp = True          # eval-mode forward may use the fused MFMA kernel (sa_mlp.py)
        # training with an xyz that requires a gradient: take the fused node with its coordinate gradients
        # (train_mlp.sa_mlp_train(..., xyz_grad=True)) instead of the layer-by-layer path. Opt-in.
        self.fused_xyz_grad = False
        # training without a geometry: build the level's index plan where idx is born (index_plan.py), so that the backward
        # inverts idx nowhere -- and the two scatters of an xyz_grad backward share one inversion. A geometry's own plans
        # (GeometryAhead(..., plans=True)) are used whatever this says. Opt-in.
        self.index_plans = False
        # gradients through a stack whose batch norms are all in eval() (the module in eval(), or in train() with its batch norms
        # frozen): take the fused node with frozen statistics (train_mlp.sa_mlp_train(..., frozen=True)) instead of the
        # layer-by-layer path; last_path "fused_frozen". Opt-in.
        self.fused_frozen_bn = False
        # training with npoints= (per-cloud sample counts; _forward_counts) -- and, on a group_all level with ragged_group_all,
        # with lengths=: take the fused node with a row mask (train_mlp.sa_mlp_train(..., counts=)) instead of compacting the
        # valid rows and running the stack layer by layer: no nonzero(), no host synchronisation; last_path
        # "fused_train_ragged". Max pooling without mlp2, an xyz that needs no gradient, a stack group_ragged_supported
        # covers; anything else keeps the compacting path. Opt-in (the name is the FP module's).
        self.fused_ragged_train = False
        # a group_all level accepts lengths= (per-cloud point counts; _forward_all_ragged): the group is the cloud's VALID rows.
        # Without it group_all refuses lengths. Opt-in.
        self.ragged_group_all = False
        # eval() with lengths= / npoints= (/ lengths1=): the fused inference kernels with the counts inside
        # (pn2_*_ragged, include/pn2ops.h "ragged inference") instead of the dense kernels on every row and a torch.where behind
        # them: padding rows are neither gathered nor computed where a kernel can skip them, a level without a geometry is ONE
        # C call; last_path "fused_ragged". Where the dense fused route would run (_fused_ok / _fused_kind), max pooling. Opt-in.
        self.fused_ragged_eval = False
        self.reuse_buffers = False     # eval: keep the level's result / scratch tensors and overwrite them on the next call
        self.last_path = None
        self._pack_cache = None
        self._lvl_buffers = None

    def _train_mode(self, xyz, points, m=None):
        """The module-level _train_mode on this module's one stack (a group_all level's group is the whole cloud)."""
        return _train_mode(self, [(self.mlp.net, xyz.shape[1] if self.group_all else self.nsample)], self.pooling, self.group_all,
                           xyz, points, m)

    def _level_buffers(self):
        if not self.reuse_buffers:
            return None
        if self._lvl_buffers is None:
            self._lvl_buffers = sa_mlp.LevelBuffers()
        return self._lvl_buffers

    def _fused_ok(self, xyz, points):
        """Inference on a layer stack pn2_sa_mlp3_maxpool / pn2_sa_mlp3_pool covers (see sa_mlp.py)."""
        if not self.fused_mlp or self.training or torch.is_grad_enabled():
            return False
        if not xyz.is_cuda:
            return False
        if self.pooling != "max":                  # avg / weighted_avg / max_and_avg (:130-140): the resident kernel's stacks
            cin = 3 + (points.shape[2] if points is not None else 0)
            return not self.group_all and sa_mlp.pool_supported(cin, self.mlp.widths, self.nsample, self.pooling)
        # (mlp2, :142-150, runs on the POOLED (b, npoint, C) rows behind the fused stack: _post)
        # (use_xyz=False: the kernels still gather the coordinates, against three zero rows of weight -- _packed)
        cin = 3 + (points.shape[2] if points is not None else 0)
        if self.group_all:                         # only the cooperative kernel gathers a whole cloud without idx
            return sa_mlp.supported(cin, self.mlp.widths, xyz.shape[1]) and sa_mlp.kind(cin, self.mlp.widths, xyz.shape[1]) == "cooperative"
        return sa_mlp.supported(cin, self.mlp.widths, self.nsample)

    def _packed(self, device, nsample=None):
        """Folded + packed weights, rebuilt when a parameter or a running statistic changed."""
        stamp = tuple((t.data_ptr(), t._version) for t in list(self.mlp.parameters()) + list(self.mlp.buffers()))
        nsample = nsample or self.nsample
        if self._pack_cache is None or self._pack_cache[0] != (stamp, device):
            self._pack_cache = ((stamp, device), {})            # one entry per nsample / cloud size, dropped when a weight changes
        hit = self._pack_cache[1].get(nsample)
        if hit is None:
            _no_packing_under_capture()
            if len(self._pack_cache[1]) >= 8:
                self._pack_cache[1].clear()
            no_xyz = not self.use_xyz and self.c_in > 0                 # features only (pointnet_util.py:49-52)
            hit = sa_mlp.PackedMLP3(self.mlp.folded_layers("first" if no_xyz else None), device, nsample, True)
            self._pack_cache[1][nsample] = hit
        return hit

    def prepare_fused(self, device, n=None):
        """Fold the batch norms and pack the weights for the fused kernel NOW (a host-side step with a
        device-to-host copy and an upload): call it once after loading weights / before capturing a HIP
        graph, so that forward() finds the cache warm. group_all levels pack per cloud size: pass n (the number of
        points this level will see)."""
        cin = self.mlp.net[0].in_channels + (3 if not self.use_xyz and self.c_in > 0 else 0)
        if self.group_all:
            if n and sa_mlp.supported(cin, self.mlp.widths, n) and sa_mlp.kind(cin, self.mlp.widths, n) == "cooperative":
                self._packed(device, n)
        elif sa_mlp.supported(cin, self.mlp.widths, self.nsample or 0):
            self._packed(device)
        return self

    def geometry(self, xyz, plans=False, lengths=None, npoints=None):
        """This level's sampling and grouping alone (:40-46; what forward() launches before its layer stack) -> SAGeometry, or
        None for a group_all level (no sampling, the group is the cloud). geometry.GeometryAhead calls it on its own stream.
        plans: with the index plan of idx, built right behind the launch that wrote it.
        lengths: (b,) per-cloud point counts of a ragged batch: the ragged operators (each cloud's geometry is the dense
        geometry of its slice; idx and fps_idx name valid rows only). ValueError for a group_all level.
        npoints: (b,) per-cloud sample counts (cloud c yields npoints[c] <= npoint centroids): rows below the count are the
        slice's geometry, rows from it on hold the operators' fills -- sample 0 as the centroid, a group of nsample times
        point 0. The caller hands npoints to the next level as its lengths."""
        if self.group_all:
            if npoints is not None or (lengths is not None and not self.ragged_group_all):
                raise ValueError("group_all with lengths: the group would contain the padding rows")
            return None
        if lengths is not None:
            lengths = ragged_lengths(lengths, xyz.shape[0], xyz.device)
        if npoints is not None:
            npoints = ragged_lengths(npoints, xyz.shape[0], xyz.device, "npoints")
        if self.knn:
            fps_idx, new_xyz = farthest_point_sample_gather(self.npoint, xyz, lengths=lengths, npoints=npoints)
            _, idx = knn_point(self.nsample, xyz, new_xyz, lengths1=lengths, lengths2=npoints)
        else:
            fps_idx, new_xyz, idx, _, _ = sample_and_group_xyz(self.npoint, self.radius, self.nsample, xyz, True, lengths=lengths,
                                                               npoints=npoints)
        return SAGeometry(new_xyz, idx, fps_idx, index_plan(idx, xyz.shape[1], "group") if plans else None)

    def _forward_on(self, xyz, points, g, path=None):
        """The layer stack on a geometry -- forward()'s own or one computed ahead (geometry.py): same paths, same results, and
        the same gradients: with xyz.requires_grad the centroids are re-gathered differentiably (SAGeometry.new_xyz_for; the
        fused training node is taken then only with fused_xyz_grad, the inference kernels never). The only place where
        sa_mlp_train and sa_mlp_pool are called with an idx. path: the last_path forward() has already decided on."""
        if path is None:
            path = self._train_mode(xyz, points) or ("fused" if self._fused_ok(xyz, points) else "unfused")
        self.last_path = path
        new_xyz, idx, plan = g.new_xyz_for(xyz), g.idx, getattr(g, "plan", None)
        if path in ("fused_train", "fused_frozen"):
            # ONE autograd node for gather + layer stack (batch-statistics batch norm -- or, "fused_frozen", the running
            # statistics) + pooling, forward and backward on the matrix cores (train_mlp.py)
            if plan is None and self.index_plans and torch.is_grad_enabled():
                plan = index_plan(idx, xyz.shape[1], "group")
            out, _ = train_mlp.sa_mlp_train(self.mlp.net, xyz, new_xyz, points, idx, True, self.pooling,
                                            xyz_grad=torch.is_grad_enabled() and xyz.requires_grad, frozen=path == "fused_frozen",
                                            plan=plan)
            return new_xyz, self._post(out), idx
        if path == "fused":
            return new_xyz, self._post(sa_mlp.sa_mlp_pool(xyz, new_xyz, points, idx, self._packed(xyz.device), self.pooling)), idx
        new_points, grouped_xyz = _grouped_input(xyz, points, idx, new_xyz, self.use_xyz, True, plan)   # :45-50
        return self._stack_and_pool(new_xyz, new_points, idx, grouped_xyz)

    def _forward_all(self, xyz, points, mode):
        """A group_all level on the fused kernels: sample_and_group_all (:59-84) + the layer stack + pooling as the training node
        (mode) or as the cooperative inference kernel; new_xyz = origin, the group is the whole cloud, channels [xyz, features]."""
        new_xyz, idx = _all_in_one_group(xyz)
        if mode is not None:
            self.last_path = mode
            out, _ = train_mlp.sa_mlp_train(self.mlp.net, xyz, None, points, None, True, self.pooling,
                                            xyz_grad=torch.is_grad_enabled() and xyz.requires_grad, frozen=mode == "fused_frozen")
        else:
            self.last_path = "fused"
            out = sa_mlp.sa_mlp_maxpool(xyz, None, points, None, self._packed(xyz.device, xyz.shape[1]))
        return new_xyz, self._post(out), idx

    def _forward_all_ragged(self, xyz, points, lengths):
        """A group_all level with per-cloud point counts (ragged_group_all): the group of cloud c is its lengths[c] valid rows;
        the output rows (b, 1, C) are all valid. Rows beyond a length may hold anything.
        eval(): the layer stack on every row -- eval batch norm is row-wise -- and the pooling over the valid rows only
        (_masked_pool); no host synchronisation, last_path "unfused".
        train(): with fused_ragged_train and support (_ragged_train_ok; max pooling, no mlp2) the fused node with a row mask,
        counts = lengths: no synchronisation, last_path "fused_train_ragged". Otherwise the valid rows of all clouds are compacted
        to (1, C, total, 1), the stack runs on them in train mode (batch statistics over the valid rows) and each cloud's slice
        is pooled (every pooling mode); plain PyTorch, synchronises, last_path "unfused_ragged"."""
        b, n, _ = xyz.shape
        lengths = ragged_lengths(lengths, b, xyz.device)
        valid = _valid_rows(lengths, b, n, xyz.device, "lengths")               # (b, n)
        new_xyz, idx = _all_in_one_group(xyz)
        if self.fused_ragged_eval and self.pooling == "max" and self._train_mode(xyz, points) is None and self._fused_ok(xyz, points):
            # the cooperative kernel on each cloud's first lengths[c] rows (the padded n chooses the kernel): one launch
            self.last_path = "fused_ragged"
            out = sa_mlp.sa_mlp_maxpool(xyz, None, points, None, self._packed(xyz.device, n), lengths=lengths)
            return new_xyz, self._post(out), idx
        if self.training and self.pooling == "max" and self.mlp2 is None and \
                _ragged_train_ok(self, [(self.mlp.net, n)], True, xyz, points):
            self.last_path = "fused_train_ragged"
            out, _ = train_mlp.sa_mlp_train(self.mlp.net, xyz, None, points, None, True, counts=lengths)
            return new_xyz, out, idx
        _, new_points, _, grouped_xyz = sample_and_group_all(xyz, points, self.use_xyz)    # (b, 1, n, C), (b, 1, n, 3)
        # (zeros on the padding rows before anything is computed from them: a NaN there would otherwise reach the weights'
        # gradients as NaN times a zero output gradient)
        keep = valid.view(b, 1, n, 1)
        zero = torch.zeros((), dtype=xyz.dtype, device=xyz.device)
        new_points, grouped_xyz = torch.where(keep, new_points, zero), torch.where(keep, grouped_xyz, zero)
        dists = grouped_xyz.norm(dim=-1, keepdim=True)
        if not self.training:
            self.last_path = "unfused"
            x = _masked_pool(self.mlp(new_points.permute(0, 3, 1, 2)), valid, dists, self.pooling)
        else:
            self.last_path = "unfused_ragged"
            rows = _valid_row_list(valid)
            c = new_points.shape[3]
            pv = new_points.reshape(b * n, c).index_select(0, rows)             # (total, C)
            y = self.mlp(pv.t().reshape(1, c, -1, 1))                            # statistics over the valid rows of all clouds
            dv = dists.reshape(b * n, 1).index_select(0, rows)
            outs, start = [], 0
            for k in lengths.clamp(1, n).tolist():                              # each cloud's slice of the compacted rows
                every = torch.ones((1, k), dtype=torch.bool, device=xyz.device)
                outs.append(_masked_pool(y[:, :, start:start + k, 0].unsqueeze(2), every, dv[start:start + k].view(1, 1, k, 1), self.pooling))
                start += k
            x = torch.cat(outs, dim=0)                                          # (b, C', 1, 1)
        if self.mlp2 is not None:
            x = self.mlp2(x)
        return new_xyz, x.squeeze(3).permute(0, 2, 1).contiguous(), idx

    def _forward_counts(self, xyz, points, g, npoints):
        """forward() with per-cloud sample counts on the geometry g (geometry(npoints=)): cloud c has npoints[c] valid
        centroids; output rows from the count on are exact zeros. eval(): the existing stack paths on all npoint rows -- the
        padding centroids' groups are nsample copies of point 0, so everything is finite -- then a torch.where; no host
        synchronisation. train(): the batch statistics must cover the valid groups only, so the valid centroids' grouped rows
        are compacted to (1, total, nsample, C) and the stack, the pooling and mlp2 run layer by layer on them (every pooling
        mode); plain PyTorch, synchronises, last_path "unfused_ragged". Nothing of a padding centroid reaches a statistic or
        a gradient; the padding rows of xyz / points are never gathered, so their gradients are exactly zero."""
        b, m = xyz.shape[0], self.npoint
        valid = _valid_rows(npoints, b, m, xyz.device)
        if not self.training:
            mode = self._train_mode(xyz, points)
            fused = mode is None and self._fused_ok(xyz, points)
            if fused and self.fused_ragged_eval and self.pooling == "max":
                # the counts inside the kernel: padding centroids are not gathered and come back as +0.0 (mlp2 maps a zero row to
                # its bias, so the zeroing stays behind _post)
                self.last_path = "fused_ragged"
                new_xyz, idx = g.new_xyz_for(xyz), g.idx
                out = sa_mlp.sa_mlp_maxpool(xyz, new_xyz, points, idx, self._packed(xyz.device), npoints=npoints)
                return new_xyz, (out if self.mlp2 is None else _zero_padding_rows(self._post(out), valid)), idx
            new_xyz, out, idx = self._forward_on(xyz, points, g, mode or ("fused" if fused else "unfused"))
            return new_xyz, _zero_padding_rows(out, valid), idx
        if self.pooling == "max" and self.mlp2 is None and _ragged_train_ok(self, [(self.mlp.net, g.idx.shape[2])], False, xyz, points):
            # fused_ragged_train: ONE autograd node on the geometry as it stands -- the padding centroids' groups stay where they
            # are (nsample copies of point 0) and a row mask keeps them out of every statistic and gradient
            self.last_path = "fused_train_ragged"
            new_xyz = g.new_xyz_for(xyz)
            out, _ = train_mlp.sa_mlp_train(self.mlp.net, xyz, new_xyz, points, g.idx, True, plan=getattr(g, "plan", None),
                                            counts=npoints)
            return new_xyz, out, g.idx
        return self._forward_compacted(xyz, points, g, valid)

    def _forward_compacted(self, xyz, points, g, valid):
        """The compacting training path of _forward_counts: valid marks the centroid rows of g, in their order, that take part
        (any shape; a packed level's (B, npoint) mask over the flat view's one cloud of B npoint centroids)."""
        self.last_path = "unfused_ragged"
        new_xyz, idx, plan = g.new_xyz_for(xyz), g.idx, getattr(g, "plan", None)
        new_points, grouped_xyz = _grouped_input(xyz, points, idx, new_xyz, self.use_xyz, True, plan)   # :45-50
        rows = _valid_row_list(valid)
        ns, every = idx.shape[2], valid.numel()
        pv = new_points.reshape(every, ns, new_points.shape[3]).index_select(0, rows).unsqueeze(0)    # (1, total, nsample, C)
        gv = grouped_xyz.reshape(every, ns, 3).index_select(0, rows).unsqueeze(0)
        _, yv, _ = self._stack_and_pool(None, pv, None, gv)                     # (1, total, C'): statistics over the valid groups
        return new_xyz, _scatter_rows(yv[0], rows, every).reshape(idx.shape[0], idx.shape[1], yv.shape[2]), idx

    def _forward_packed(self, xyz, points, offsets, max_points, npoints=None):
        """forward() on a PACKED batch: xyz (total, 3), points (total, c) or None, cloud i = rows
        offsets[i] .. offsets[i + 1] - 1. The geometry is built in the FLAT VIEW -- packed FPS + gather and packed ball query
        with global indices give SAGeometry(new_xyz (1, B npoint, 3), idx (1, B npoint, nsample), fps_idx) on xyz (1, total, 3)
        -- and handed to _forward_on: every route behind a geometry is index-driven, so the training nodes, the inference
        kernels and the layer-by-layer path run unchanged on one cloud of `total` points and B npoint centroids. No padding
        row exists, so nothing is masked. The route predicates get the true centroid count (m = B npoint). last_path is the
        route's with "packed_" in front; where no fused route takes the flat view it is "packed_unfused", layer by layer.
        Under set_packed_pairs(True): a knn module takes packed kNN where the ball query stands, nothing behind the geometry
        changes. npoints (per-cloud sample counts, the next level's lengths=): the geometry carries the operators' fills on the
        rows from npoints[c] on -- sample 0 as the centroid, a group of nsample times the cloud's own first row. eval(): the same
        routes on every row, then exact zeros on those rows (_zero_padding_rows); no synchronisation. train(): the compacting
        layer-by-layer path of _forward_counts on the flat view (_forward_compacted: the batch statistics cover the valid
        groups only; synchronises), last_path "packed_unfused_ragged" -- the masked fused node wants (b, m) rows over b source
        clouds and has no flat-view form.
        -> new_xyz (B, npoint, 3), features (B, npoint, C), idx (B, npoint, nsample) global."""
        offs, b, total, nmax = packed_args(offsets, max_points, None, xyz, "PointnetSAModule")
        if points is not None:
            require(points.dim() == 2 and points.shape[0] == total, "PointnetSAModule: with offsets, points is (total, channel)")
        m, ns = self.npoint, self.nsample
        flat = xyz.detach()
        if npoints is None and not self.knn:
            fps_idx, new_xyz = farthest_point_sample_gather(m, flat, offsets=offs, max_points=nmax, global_idx=True)
            idx, _ = query_ball_point(self.radius, ns, flat, new_xyz, offsets=offs, max_points=nmax, global_idx=True)
        else:
            if npoints is not None:
                npoints = ragged_lengths(npoints, b, flat.device, "npoints")
            fps_idx, new_xyz = farthest_point_sample_gather(m, flat, npoints=npoints, offsets=offs, max_points=nmax, global_idx=True)
            if self.knn:
                _, idx = knn_point(ns, flat, new_xyz, lengths2=npoints, offsets=offs, max_points=nmax, global_idx=True)
            else:
                idx, _ = query_ball_point(self.radius, ns, flat, new_xyz, lengths2=npoints, offsets=offs, max_points=nmax, global_idx=True)
        g = SAGeometry(new_xyz.view(1, b * m, 3), idx.view(1, b * m, ns), fps_idx.view(1, b * m))
        xf = xyz.reshape(1, total, 3)
        pf = points.reshape(1, total, points.shape[1]) if points is not None else None
        if npoints is not None:
            valid = _valid_rows(npoints, b, m, flat.device)
            if self.training:
                new_xyz_f, out, _ = self._forward_compacted(xf, pf, g, valid)
                self.last_path = "packed_unfused_ragged"
                return new_xyz_f.view(b, m, 3), out.view(b, m, out.shape[2]), idx
            path = self._train_mode(xf, pf, b * m) or ("fused" if self._fused_ok(xf, pf) else "unfused")
            new_xyz_f, out, _ = self._forward_on(xf, pf, g, path)
            self.last_path = "packed_" + path
            return new_xyz_f.view(b, m, 3), _zero_padding_rows(out.view(b, m, out.shape[2]), valid), idx
        path = self._train_mode(xf, pf, b * m) or ("fused" if self._fused_ok(xf, pf) else "unfused")
        new_xyz_f, out, _ = self._forward_on(xf, pf, g, path)
        self.last_path = "packed_" + path
        return new_xyz_f.view(b, m, 3), out.view(b, m, out.shape[2]), idx

    def forward(self, xyz, points, geometry=None, lengths=None, npoints=None, offsets=None, max_points=None):
        """Resolve the level's geometry, then run the layer stack on it (_forward_on): a geometry computed ahead
        (geometry=), the ragged operators' (lengths=), or this call's own (geometry()) for the training nodes and for the
        inference kernel behind kNN or a pooling other than max. Three routes are not "geometry, then stack" and stay apart:
        a group_all level (no sampling; _forward_all), the single C call sa_mlp.sa_level (eval, ball query, max pooling: it
        owns the level's buffers) and the layer-by-layer path without a geometry (sample_and_group's own launches, or the
        differentiable operator sequence when xyz needs a gradient).

        lengths: (b,) per-cloud point counts of a ragged batch (cloud i is xyz[i, :lengths[i]], points[i, :lengths[i]]): idx
        names valid rows only, so rows beyond a length are never gathered -- they must be finite (coordinates too when the
        module trains: a training node may run its first layer once per point, padding rows included, and a NaN times a zero
        gradient is a NaN), they influence no output and no gradient, and their own gradients are exactly zero. Not for group_all
        levels (ValueError) unless ragged_group_all is set (_forward_all_ragged: the group is the cloud's valid rows, which
        may then hold anything beyond a length).
        npoints: (b,) per-cloud sample counts, with or without lengths (_forward_counts; a geometry= must come from
        geometry(npoints=)): new_points rows from npoints[c] on are exact zeros; hand npoints to the next level as its lengths.
        offsets / max_points: a packed batch, xyz (total, 3) and points (total, c), see _forward_packed. Single scale, ball
        query; ValueError with group_all, knn, lengths / npoints, a geometry= or fused_xyz_grad. Under set_packed_pairs(True) a knn
        module and npoints= are offered with offsets as well (_forward_packed)."""
        if offsets is not None:
            pairs = packed_pairs()
            require(lengths is None and (npoints is None or pairs), "PointnetSAModule: offsets and lengths / npoints are two layouts; give one")
            require(not self.group_all, "PointnetSAModule: group_all is not offered with offsets")
            require(not self.knn or pairs, "PointnetSAModule: knn is not offered with offsets")
            require(geometry is None, "PointnetSAModule: a geometry computed ahead is not offered with offsets")
            require(not self.fused_xyz_grad, "PointnetSAModule: fused_xyz_grad is not offered with offsets")
            return self._forward_packed(xyz, points, offsets, max_points, npoints)
        if (lengths is not None or npoints is not None) and self.group_all:
            if npoints is not None or not self.ragged_group_all:
                raise ValueError("group_all with lengths: the group would contain the padding rows")
            return self._forward_all_ragged(xyz, points, lengths)
        if (lengths is not None or npoints is not None) and geometry is None and self.fused_ragged_eval and not self.knn and \
                self.pooling == "max" and self._train_mode(xyz, points) is None and self._fused_ok(xyz, points):
            # ONE C call (csrc/levels.hip: pn2_sa_level_ragged), full counts for a dense side
            self.last_path = "fused_ragged"
            new_xyz, out, idx, _, _, _ = sa_mlp.sa_level_ragged(self.npoint, self.radius, self.nsample, xyz, points,
                                                                 self._packed(xyz.device), lengths, npoints, self._level_buffers())
            if self.mlp2 is not None:
                out = self._post(out)
                if npoints is not None:
                    out = _zero_padding_rows(out, _valid_rows(npoints, xyz.shape[0], self.npoint, xyz.device))
            return new_xyz, out, idx
        if npoints is not None:
            g = geometry.wait() if geometry is not None else self.geometry(xyz, lengths=lengths, npoints=npoints)
            return self._forward_counts(xyz, points, g, npoints)
        mode = self._train_mode(xyz, points)
        if self.group_all and (mode is not None or self._fused_ok(xyz, points)):
            return self._forward_all(xyz, points, mode)
        fused = mode is None and self._fused_ok(xyz, points)      # (a group_all level that got here says no once more)
        if self.group_all:
            g = None
        elif geometry is not None:
            g = geometry.wait()
        elif lengths is not None:
            g = self.geometry(xyz, lengths=lengths)
        elif mode is not None or (fused and (self.knn or self.pooling != "max")):
            g = self.geometry(xyz, plans=mode is not None and self.index_plans and torch.is_grad_enabled())
        else:
            g = None
        if g is not None:
            return self._forward_on(xyz, points, g, mode or ("fused" if fused else "unfused"))
        if fused:
            # ONE C call (csrc/levels.hip): FPS + ball query in the overlapped launch, then one kernel from idx to the
            # pooled features: the (b, npoint, nsample, C) tensors of pointnet_util.py:44-50 and :117-127 never exist
            self.last_path = "fused"
            new_xyz, out, idx, _, _, _ = sa_mlp.sa_level(self.npoint, self.radius, self.nsample, xyz, points,
                                                          self._packed(xyz.device), self._level_buffers())
            return new_xyz, self._post(out), idx
        self.last_path = "unfused"
        if self.group_all:
            new_xyz, new_points, idx, grouped_xyz = sample_and_group_all(xyz, points, self.use_xyz)
        else:
            new_xyz, new_points, idx, grouped_xyz = sample_and_group(self.npoint, self.radius, self.nsample, xyz,
                                                                     points, self.knn, self.use_xyz)
        return self._stack_and_pool(new_xyz, new_points, idx, grouped_xyz)

    def _post(self, pooled):
        """mlp2 (:142-150: conv 1x1 + BN + ReLU on the pooled features) behind a fused stack + pool: (b, npoint, C) rows through
        the same modules the layer-by-layer path applies to its (b, C, npoint, 1) tensor; differentiable (training: behind
        the fused autograd node)."""
        if self.mlp2 is None:
            return pooled
        x = self.mlp2(pooled.permute(0, 2, 1).unsqueeze(3))
        return x.squeeze(3).permute(0, 2, 1).contiguous()

    def _stack_and_pool(self, new_xyz, new_points, idx, grouped_xyz):
        """The layer stack, the pooling and mlp2 of the layer-by-layer path (:117-152)."""
        x = self.mlp(new_points.permute(0, 3, 1, 2))                 # (b, C, npoint, nsample)
        if self.pooling == "max":
            x = x.max(dim=3, keepdim=True)[0]
        elif self.pooling == "avg":
            x = x.mean(dim=3, keepdim=True)
        elif self.pooling == "weighted_avg":                          # :130-136
            dists = grouped_xyz.norm(dim=-1, keepdim=True)
            w = torch.exp(-dists * 5)
            w = (w / w.sum(dim=2, keepdim=True)).permute(0, 3, 1, 2)
            x = (x * w).sum(dim=3, keepdim=True)
        elif self.pooling == "max_and_avg":                           # :137-140: concat([avg, max])
            x = torch.cat([x.mean(dim=3, keepdim=True), x.max(dim=3, keepdim=True)[0]], dim=1)
        else:
            raise ValueError("unknown pooling %r" % (self.pooling,))
        if self.mlp2 is not None:
            x = self.mlp2(x)
        return new_xyz, x.squeeze(3).permute(0, 2, 1).contiguous(), idx


class PointnetSAModuleMSG(nn.Module):
    """reference: pointnet_sa_module_msg, pointnet_util.py:156-196 (one FPS, several radii;
    concat order features FIRST, :184 -- the opposite of the single-scale module)."""

    def __init__(self, c_in, npoint, radius_list, nsample_list, mlp_list, bn=True, use_xyz=True, use_nchw=False):
        super().__init__()                                # (use_nchw, :156: accepted and ignored, see PointnetSAModule)
        self.npoint, self.radius_list, self.nsample_list, self.use_xyz = npoint, radius_list, nsample_list, use_xyz
        self.c_in = c_in
        feat = 3 if c_in == 0 else (c_in + 3 if use_xyz else c_in)
        self.mlps = nn.ModuleList([_SharedMLP(feat, widths, bn) for widths in mlp_list])
        self.fused_mlp = True          # eval-mode forward may use the fused MFMA kernel (sa_mlp.py)
        self.fused_xyz_grad = False    # see PointnetSAModule: the fused training node for an xyz that requires a gradient (opt-in)
        self.fused_frozen_bn = False   # see PointnetSAModule: the fused node with frozen batch-norm statistics (opt-in)
        self.index_plans = False       # see PointnetSAModule: one index plan per radius, built where its idx is born (opt-in)
        # geometry(lengths=): every radius of a ragged level in ONE multi-radius launch (query_ball_group_xyz_msg(..., lengths1=):
        # each cloud staged and binned once) instead of one ragged ball query per radius -- same bits. Opt-in; measured in
        # profiles/ragged_msg/README.md.
        self.ragged_one_launch = False
        # training with npoints=: one fused node with a row mask per scale instead of the compacting layer-by-layer path; see
        # PointnetSAModule.fused_ragged_train. last_path "fused_train_ragged". Opt-in.
        self.fused_ragged_train = False
        self.fused_ragged_eval = False  # see PointnetSAModule: eval() with counts on the fused inference kernels (opt-in)
        # forward(offsets=, max_points=): a packed batch -- packed FPS + gather, then every radius in ONE packed
        # multi-radius launch, the stacks on the flat view (_forward_packed). Opt-in: with it off the module refuses offsets as
        # it always has (ValueError), which callers may rely on to learn that a level is not packed.
        self.packed_batches = False
        self.last_path = None
        self._pack_cache = {}

    def _fused_ok(self, xyz, points):
        if not self.fused_mlp or self.training or torch.is_grad_enabled() or not xyz.is_cuda:
            return False
        cin = 3 + (points.shape[2] if points is not None else 0)       # (use_xyz=False: three zero rows of weight, _packed)
        return all(sa_mlp.supported(cin, mlp.widths, ns) for mlp, ns in zip(self.mlps, self.nsample_list))

    def _packed(self, si, device):
        mlp = self.mlps[si]
        stamp = (tuple((t.data_ptr(), t._version) for t in list(mlp.parameters()) + list(mlp.buffers())), device)
        hit = self._pack_cache.get(si)
        if hit is None or hit[0] != stamp:
            _no_packing_under_capture()
            # the MSG module concatenates features FIRST (:184): xyz_first=False
            no_xyz = not self.use_xyz and self.c_in > 0                 # features only (:182-184 without the concat)
            hit = (stamp, sa_mlp.PackedMLP3(mlp.folded_layers("last" if no_xyz else None), device, self.nsample_list[si],
                                            xyz_first=False))
            self._pack_cache[si] = hit
        return hit[1]

    def prepare_fused(self, device):
        """See PointnetSAModule.prepare_fused."""
        cin = self.mlps[0].net[0].in_channels + (3 if not self.use_xyz and self.c_in > 0 else 0)
        if all(sa_mlp.supported(cin, mlp.widths, ns) for mlp, ns in zip(self.mlps, self.nsample_list)):
            for si in range(len(self.mlps)):
                self._packed(si, device)
        return self

    def _group_scales(self, xyz, want_idx, with_fps=False):
        """FPS + every radius of the level: the single overlapped launch covers FPS and the first radius
        (:173-180), ONE multi-radius launch (one staging / binning of the cloud) the remaining radii --
        the reference rescans the cloud once per radius (:175-186).
        -> new_xyz, [(idx or None, grouped_xyz) per scale] (with_fps: and the samples' indices)"""
        fps_idx, new_xyz, idx0, _, gx0 = sample_and_group_xyz(self.npoint, self.radius_list[0], self.nsample_list[0], xyz, True)
        scales = [(idx0, gx0)]
        if len(self.radius_list) > 1:
            rest = query_ball_group_xyz_msg(self.radius_list[1:], self.nsample_list[1:], xyz, new_xyz, True, want_idx=want_idx)
            scales += [(i, g) for i, _, g in rest]
        return (new_xyz, scales, fps_idx) if with_fps else (new_xyz, scales)

    def geometry(self, xyz, plans=False, lengths=None, npoints=None):
        """This level's sampling and every radius' grouping alone (:173-180) -> SAGeometry with one idx per radius (plans: and
        one index plan per radius). lengths: (b,) per-cloud point counts of a ragged batch: ragged FPS + gather, then one
        ragged ball query per radius -- or, with ragged_one_launch, ONE ragged multi-radius launch for all radii (the first
        included: there is no overlapped launch with lengths to serve it); the results are the same bit for bit.
        npoints: (b,) per-cloud sample counts (see PointnetSAModule.geometry), with or without lengths: the two-sided ragged
        operators, one launch per radius or -- ragged_one_launch -- one for all; same bits."""
        if npoints is not None:
            npoints = ragged_lengths(npoints, xyz.shape[0], xyz.device, "npoints")
        if lengths is not None:
            lengths = ragged_lengths(lengths, xyz.shape[0], xyz.device)
        if lengths is None and npoints is None:
            new_xyz, scales, fps_idx = self._group_scales(xyz, True, with_fps=True)
        else:
            fps_idx, new_xyz = farthest_point_sample_gather(self.npoint, xyz, lengths=lengths, npoints=npoints)
            if self.ragged_one_launch:
                scales = [(i, g) for i, _, g in query_ball_group_xyz_msg(self.radius_list, self.nsample_list, xyz, new_xyz, True,
                                                                         lengths1=lengths, lengths2=npoints)]
            else:
                scales = [query_ball_group_xyz(r, k, xyz, new_xyz, True, lengths1=lengths, lengths2=npoints)[0::2]
                          for r, k in zip(self.radius_list, self.nsample_list)]
        return SAGeometry(new_xyz, [idx for idx, _ in scales], fps_idx,
                          [index_plan(idx, xyz.shape[1], "group") for idx, _ in scales] if plans else None)

    def _forward_fused(self, xyz, points, g):
        """Inference: the grouping launches of _group_scales (g None; no geometry object on the eager path, which is bound by
        the host) or a geometry, then one fused MLP + max-pool kernel per scale; no grouped tensor is ever materialised."""
        if g is None:
            new_xyz, scales = self._group_scales(xyz, True)
            idxs = [idx for idx, _ in scales]
        else:
            new_xyz, idxs = g.new_xyz, g.idx
        outs = [sa_mlp.sa_mlp_maxpool(xyz, new_xyz, points, idx, self._packed(si, xyz.device)) for si, idx in enumerate(idxs)]
        return new_xyz, torch.cat(outs, dim=2)

    def _forward_train(self, xyz, points, g, mode):
        """Training on a geometry: one autograd node per scale (train_mlp.py); channel order features FIRST (:184).
        "fused_frozen": the same with the running statistics (fused_frozen_bn). With xyz.requires_grad (fused_xyz_grad) the
        centroids are re-gathered differentiably and autograd adds the scales' coordinate gradients."""
        new_xyz = g.new_xyz_for(xyz)
        plans = getattr(g, "plan", None)
        if plans is None and self.index_plans and torch.is_grad_enabled():
            plans = [index_plan(idx, xyz.shape[1], "group") for idx in g.idx]
        want_xyz = torch.is_grad_enabled() and xyz.requires_grad
        outs = [train_mlp.sa_mlp_train(mlp.net, xyz, new_xyz, points, idx, False, xyz_grad=want_xyz, frozen=mode == "fused_frozen",
                                       plan=plan)[0]
                for mlp, idx, plan in zip(self.mlps, g.idx, plans or [None] * len(g.idx))]
        return new_xyz, torch.cat(outs, dim=2)

    def _forward_layers(self, xyz, points, g):
        """Layer by layer (:173-195). g None: this call's own launches -- _group_scales' grouped_xyz, or the differentiable
        operator sequence when xyz needs a gradient."""
        fused = g is not None or not (torch.is_grad_enabled() and xyz.requires_grad)
        scales = None
        if g is not None:
            new_xyz = g.new_xyz_for(xyz)               # (re-gathered differentiably when xyz needs a gradient: tf_sampling.py:43-47)
            scales = [(idx, None) for idx in g.idx]
        elif fused:
            new_xyz, scales = self._group_scales(xyz, points is not None)
        else:
            new_xyz = mark_fps_ordered(gather_point(xyz, farthest_point_sample(self.npoint, xyz)))   # :173
        outs = []
        for si, (radius, nsample, mlp) in enumerate(zip(self.radius_list, self.nsample_list, self.mlps)):
            idx, grouped_xyz = scales[si] if fused else (query_ball_point(radius, nsample, xyz, new_xyz)[0], None)   # :178
            grouped, _ = _grouped_input(xyz, points, idx, new_xyz, self.use_xyz, False, grouped_xyz=grouped_xyz)   # :179-184
            x = mlp(grouped.permute(0, 3, 1, 2))
            outs.append(x.max(dim=3)[0])                                        # :193
        return new_xyz, torch.cat(outs, dim=1).permute(0, 2, 1).contiguous()    # :195

    def _forward_counts(self, xyz, points, g, npoints):
        """forward() with per-cloud sample counts, see PointnetSAModule._forward_counts: eval() runs the existing paths on all
        rows and zeroes the padding rows; train() compacts the valid centroids' groups per radius and runs each stack layer by
        layer on (1, C, total, nsample) -- last_path "unfused_ragged", synchronises."""
        b, m = xyz.shape[0], self.npoint
        valid = _valid_rows(npoints, b, m, xyz.device)
        if not self.training:
            if self.fused_ragged_eval and self._fused_ok(xyz, points):
                # one fused kernel with the counts inside per scale: padding centroids are skipped and stored as +0.0
                self.last_path = "fused_ragged"
                outs = [sa_mlp.sa_mlp_maxpool(xyz, g.new_xyz, points, idx, self._packed(si, xyz.device), npoints=npoints)
                        for si, idx in enumerate(g.idx)]
                return g.new_xyz, torch.cat(outs, dim=2)
            new_xyz, out = self._forward_on_geometry(xyz, points, g)
            return new_xyz, _zero_padding_rows(out, valid)
        if _ragged_train_ok(self, [(mlp.net, idx.shape[2]) for mlp, idx in zip(self.mlps, g.idx)], False, xyz, points):
            # fused_ragged_train: one masked node per scale on the geometry as it stands; channel order features FIRST (:184)
            self.last_path = "fused_train_ragged"
            new_xyz = g.new_xyz_for(xyz)
            plans = getattr(g, "plan", None) or [None] * len(g.idx)
            outs = [train_mlp.sa_mlp_train(mlp.net, xyz, new_xyz, points, idx, False, plan=plan, counts=npoints)[0]
                    for mlp, idx, plan in zip(self.mlps, g.idx, plans)]
            return new_xyz, torch.cat(outs, dim=2)
        self.last_path = "unfused_ragged"
        new_xyz = g.new_xyz_for(xyz)
        rows = _valid_row_list(valid)
        outs = []
        for idx, mlp in zip(g.idx, self.mlps):
            grouped, _ = _grouped_input(xyz, points, idx, new_xyz, self.use_xyz, False)       # :179-184
            gv = grouped.reshape(b * m, idx.shape[2], grouped.shape[3]).index_select(0, rows)          # (total, nsample, C)
            outs.append(mlp(gv.permute(2, 0, 1).unsqueeze(0)).max(dim=3)[0][0].t())                # (total, C')  :193
        yv = torch.cat(outs, dim=1)                                             # :195
        return new_xyz, _scatter_rows(yv, rows, b * m).reshape(b, m, yv.shape[1])

    def _forward_on_geometry(self, xyz, points, g, m=None):
        """One function per path on a geometry (g None: the inference kernels and the layer-by-layer path keep their own
        launches, the training nodes take this call's own geometry()). m: the centroid rows per cloud of xyz when that is not
        npoint (the flat view of a packed batch)."""
        if self._fused_ok(xyz, points):
            self.last_path = "fused"
            return self._forward_fused(xyz, points, g)
        mode = _train_mode(self, [(mlp.net, ns) for mlp, ns in zip(self.mlps, self.nsample_list)], "max", False, xyz, points, m)
        if mode is not None:
            self.last_path = mode
            return self._forward_train(xyz, points, g or self.geometry(xyz, plans=self.index_plans and torch.is_grad_enabled()), mode)
        self.last_path = "unfused"
        return self._forward_layers(xyz, points, g)

    def packed_geometry(self, xyz, offsets, max_points, plans=False):
        """geometry() of a PACKED batch (packed_batches), in the FLAT VIEW: packed FPS + gather, then every radius
        in ONE packed multi-radius launch (each cloud's slab staged and binned once), both with global indices.
        -> SAGeometry(new_xyz (1, B npoint, 3), [idx_i (1, B npoint, nsample_i)], fps_idx (1, B npoint)) on xyz (1, total, 3):
        idx_i holds rows of the flat array (plans: one index plan per radius on `total` rows)."""
        require(self.packed_batches, "PointnetSAModuleMSG: packed batches (offsets=) are not offered for MSG levels")
        offs, b, total, nmax = packed_args(offsets, max_points, None, xyz, "PointnetSAModuleMSG")
        m = self.npoint
        flat = xyz.detach()
        fps_idx, new_xyz = farthest_point_sample_gather(m, flat, offsets=offs, max_points=nmax, global_idx=True)
        scales = query_ball_group_xyz_msg(self.radius_list, self.nsample_list, flat, new_xyz, True, offsets=offs, max_points=nmax,
                                          global_idx=True)
        idxs = [i.view(1, b * m, i.shape[2]) for i, _, _ in scales]
        return SAGeometry(new_xyz.view(1, b * m, 3), idxs, fps_idx.view(1, b * m),
                          [index_plan(i, total, "group") for i in idxs] if plans else None)

    def _forward_packed(self, xyz, points, offsets, max_points):
        """forward() on a PACKED batch: xyz (total, 3), points (total, c) or None, cloud i = rows offsets[i] .. offsets[i + 1] - 1.
        The geometry is built in the flat view (packed_geometry) and handed to the existing function of each path
        (_forward_on_geometry): every route behind a geometry is index-driven, so the training nodes, the inference kernels and
        the layer-by-layer path run unchanged on one cloud of `total` points and B npoint centroids, and nothing is masked. The
        route predicates get the true centroid count (m = B npoint). last_path is the route's with "packed_" in front.
        -> new_xyz (B, npoint, 3), features (B, npoint, sum C_i); the per-scale global idx: packed_geometry()."""
        require(not (torch.is_grad_enabled() and isinstance(xyz, torch.Tensor) and xyz.requires_grad),
                "PointnetSAModuleMSG: with offsets xyz cannot require a gradient (detach it)")
        offs, b, total, nmax = packed_args(offsets, max_points, None, xyz, "PointnetSAModuleMSG")
        if points is not None:
            require(points.dim() == 2 and points.shape[0] == total, "PointnetSAModuleMSG: with offsets, points is (total, channel)")
        m = self.npoint
        xf = xyz.reshape(1, total, 3)
        pf = points.reshape(1, total, points.shape[1]) if points is not None else None
        g = self.packed_geometry(xyz, offs, nmax)                  # (index_plans: _forward_train builds them, on `total` rows)
        new_xyz_f, out = self._forward_on_geometry(xf, pf, g, b * m)
        self.last_path = "packed_" + self.last_path
        return new_xyz_f.view(b, m, 3), out.view(b, m, out.shape[2])

    def forward(self, xyz, points, geometry=None, lengths=None, npoints=None, offsets=None, max_points=None):
        """Resolve the level's geometry -- computed ahead (geometry=), the ragged operators' (lengths=, see
        PointnetSAModule.forward) or, for the training nodes, this call's own (geometry()) -- then one function per path on it.
        Without a geometry the inference kernels and the layer-by-layer path keep their own launches (_group_scales).
        npoints: (b,) per-cloud sample counts, with or without lengths (_forward_counts).
        offsets / max_points: a packed batch, xyz (total, 3) and points (total, c), see _forward_packed -- with packed_batches
        set; ValueError without it, and with lengths / npoints, a geometry=, fused_xyz_grad or an xyz that needs a gradient."""
        if self.packed_batches and offsets is not None:
            require(lengths is None and npoints is None, "PointnetSAModuleMSG: offsets and lengths / npoints are two layouts; give one")
            require(geometry is None, "PointnetSAModuleMSG: a geometry computed ahead is not offered with offsets")
            require(not self.fused_xyz_grad, "PointnetSAModuleMSG: fused_xyz_grad is not offered with offsets")
            return self._forward_packed(xyz, points, offsets, max_points)
        require(offsets is None and max_points is None, "PointnetSAModuleMSG: packed batches (offsets=) are not offered for MSG levels")
        if npoints is not None:
            g = geometry.wait() if geometry is not None else self.geometry(xyz, lengths=lengths, npoints=npoints)
            return self._forward_counts(xyz, points, g, npoints)
        if geometry is None and lengths is not None:
            geometry = self.geometry(xyz, lengths=lengths)
        return self._forward_on_geometry(xyz, points, None if geometry is None else geometry.wait())


class PointnetFPModule(nn.Module):
    """reference: pointnet_fp_module, pointnet_util.py:199-229."""

    def __init__(self, c_in, mlp, bn=True):
        super().__init__()
        self.mlp = _SharedMLP(c_in, mlp, bn)
        self.fused_mlp = True          # eval-mode forward may use the fused kernel (csrc/fp_mlp.hip)
        self.fused_frozen_bn = False   # see PointnetSAModule: the fused node with frozen batch-norm statistics (opt-in)
        self.index_plans = False       # see PointnetSAModule: the index plan of three_nn's idx, built behind three_nn (opt-in)
        # train() with a ragged unknown side (lengths1=): fp_interp_concat + the fused node with a row mask
        # (train_mlp.fp_mlp_train(..., lengths=)) instead of the compacting layer-by-layer path: no host synchronisation, nothing
        # compacted, capturable; last_path "fused_train_ragged". Opt-in, like fused_frozen_bn (_forward_ragged).
        self.fused_ragged_train = False
        # ... and, with fused_ragged_train on, the ONE-NODE form with a row mask (train_mlp.fp_level_train(..., lengths=)) where
        # the dense route would take the one-node form (fp_level_preferred) and train_mlp.fp_level_ragged_supported: layer 1 once
        # per known point, the (b, n, c2 + c1) tensor and its gradient never written; last_path "fused_train_ragged_node".
        # Opt-in of its own. Measured (profiles/ragged_fp_node/README.md, warm forward + backward): sem_seg FP4 0.66-0.67 ->
        # 0.64 ms and 288 -> 231 MB peak; part_seg FP3 0.525-0.530 -> 0.521-0.524 ms, which is within the spread of the medians
        # -- NOT faster there -- and 158 -> 132 MB peak. Folding it into the size rule is a later change.
        self.fused_ragged_node = False
        self.fused_ragged_eval = False  # see PointnetSAModule: eval() with counts on the fused inference kernels (opt-in)
        self.reuse_buffers = False     # eval: keep the level's result / scratch tensors and overwrite them on the next call
        self.last_path = None
        self._pack_cache = None
        self._lvl_buffers = None

    _level_buffers = PointnetSAModule._level_buffers

    def _plan_of(self, idx, m, plan=None):
        """The level's index plan: the geometry's, or (index_plans) one built here, behind the launch that wrote idx."""
        if plan is None and self.index_plans and torch.is_grad_enabled():
            plan = index_plan(idx, m, "interpolate")
        return plan

    def _frozen_ok(self, x1, x2, rows):
        """Autograd through the stack with every batch norm in eval() (fused_frozen_bn): an input (x1 / x2: the tensors the
        stack's input is made of) or a parameter wants a gradient, and the frozen node covers `rows` plain rows. The level then
        runs fp_interp_concat + fp_mlp_train(frozen=True) whatever fp_level_preferred says (the one-node form has no frozen mode)."""
        if not self.fused_frozen_bn or not self.fused_mlp or not torch.is_grad_enabled() or not x2.is_cuda:
            return False
        if not (x2.requires_grad or (x1 is not None and x1.requires_grad) or any(p.requires_grad for p in self.mlp.net.parameters())):
            return False
        return train_mlp.frozen_supported(self.mlp.net, rows, 0, False)

    def _fused_kind(self, points1, points2, npoints):
        """The fused kernel for this call (sa_mlp.fp_kind: cooperative below 16384 unknown points, streamed
        above), or None: training, autograd, CPU tensors, or a stack no kernel covers."""
        if not self.fused_mlp or self.training or torch.is_grad_enabled() or not points2.is_cuda:
            return None
        c1 = points1.shape[2] if points1 is not None else 0
        return sa_mlp.fp_kind(npoints, points2.shape[2], c1, self.mlp.widths)

    def _packed(self, c2, c1, kind, device):
        stamp = (tuple((t.data_ptr(), t._version) for t in list(self.mlp.parameters()) + list(self.mlp.buffers())), device)
        if self._pack_cache is None or self._pack_cache[0] != stamp:
            self._pack_cache = (stamp, {})                      # one entry per (c2, c1, kernel kind)
        hit = self._pack_cache[1].get((c2, c1, kind))
        if hit is None:
            _no_packing_under_capture()
            hit = sa_mlp.PackedFPMLP(self.mlp.folded_layers(), c2, c1, device, kind)
            self._pack_cache[1][(c2, c1, kind)] = hit
        return hit

    def prepare_fused(self, c2, c1, npoints, device):
        """See PointnetSAModule.prepare_fused (c2 / c1 = channels of points2 / points1, npoints = b * n unknown points)."""
        kind = sa_mlp.fp_kind(npoints, c2, c1, self.mlp.widths)
        if kind is not None:
            self._packed(c2, c1, kind, device)
        return self

    def _train_mode(self, points1, points2, rows):
        """"fused_train" / "fused_frozen" / None: which fused autograd node runs the stack behind ONE launch for weights +
        interpolation + concatenation. Only where that launch's gradient is the segmented scatter (use_segmented_grad)."""
        if not use_segmented_grad(points2.shape[0], points2.shape[1], points2.shape[2]):
            return None
        if self.fused_mlp and self.training and points2.is_cuda and train_mlp.stack_supported(self.mlp.net, rows, 0, False):
            return "fused_train"
        return "fused_frozen" if self._frozen_ok(points1, points2, rows) else None

    def _forward_on(self, xyz1, points1, points2, g):
        """forward() on three_nn's result computed ahead (geometry.py): everything after :211, same paths, same results."""
        kind = self._fused_kind(points1, points2, xyz1.shape[0] * xyz1.shape[1])
        if kind is not None:
            self.last_path = "fused"
            c1 = points1.shape[2] if points1 is not None else 0
            return sa_mlp.fp_mlp(points2, points1, g.idx, g.dist, self._packed(points2.shape[2], c1, kind, points2.device))
        return self._stack_on(xyz1, points1, points2, g)

    def _stack_on(self, xyz1, points1, points2, g, lengths=None, node_ok=train_mlp.fp_level_supported, paths=None):
        """Everything after :211 but the inference kernels, on three_nn's result g (dist, idx and perhaps a plan).
        lengths: _forward_ragged's fused case -- it has found the mode to be "fused_train" and gives its own condition for the
        one-node form (node_ok) and its last_path values (paths: of concat + stack, of the node)."""
        dist, idx, plan = g.dist, g.idx, getattr(g, "plan", None)
        b, n = xyz1.shape[0], xyz1.shape[1]
        m, c2 = points2.shape[1], points2.shape[2]
        c1 = points1.shape[2] if points1 is not None else 0
        mode = self._train_mode(points1, points2, b * n) if lengths is None else "fused_train"
        if mode is None:                                                        # layer by layer
            return self._after_weights(points1, points2, idx, _inverse_distance_weights(dist), plan)
        # ONE launch for weights + interpolation + concatenation (+ the zero pad of an odd width), then the layer stack as one
        # autograd node (train_mlp.py) with batch-statistics batch norm -- or, "fused_frozen", the running statistics; backward:
        # the stack's kernels, one split + the segmented scatter of three_interpolate's gradient
        plan = self._plan_of(idx, m, plan)
        node = mode == "fused_train" and train_mlp.fp_level_preferred(b, n, m, c2) and node_ok(self.mlp.net, b, n, m, c2, c1)
        self.last_path = paths[node] if paths else mode
        if node:
            # weights, interpolation, concatenation and the stack as ONE node, layer 1 once per known point (train_mlp_fp.hip)
            return train_mlp.fp_level_train(self.mlp.net, points2, points1, idx, dist, plan=plan, lengths=lengths)     # :212-226
        x, _ = fp_interp_concat(points2, points1, idx, dist, plan=plan)         # :212-219, on every row
        return train_mlp.fp_mlp_train(self.mlp.net, x, cin=c2 + c1, frozen=mode == "fused_frozen", lengths=lengths)

    def _forward_ragged(self, xyz1, xyz2, points1, points2, lengths1, geometry=None, lengths2=None):
        """forward() with a ragged unknown side: cloud i's unknown points are xyz1[i, :lengths1[i]] (points1 likewise; the
        known side is a previous level's dense output). three_nn never reads the padding rows; output rows beyond a length
        are exactly zero. eval(): the existing paths on all rows (the padding rows of points1 must be finite), then a
        torch.where. train(): the batch statistics must cover the valid rows only, so the valid rows of interpolate + concat
        are compacted to (1, total, C), the layer stack runs layer by layer on them and the result is scattered back --
        plain PyTorch, last_path "unfused_ragged", synchronises (the row list is built on the host's schedule).
        With fused_ragged_train (opt-in), CUDA tensors and a stack the masked node covers (_train_mode says "fused_train" and
        train_mlp.ragged_supported): ONE launch for weights + interpolation + concatenation on all rows, then the stack as one
        autograd node whose passes skip the padding rows (fp_mlp_train(..., lengths=)); last_path "fused_train_ragged". The
        host reads nothing, the index plan is _stack_on's. With fused_ragged_node as well (opt-in), where the dense route would
        take the one-node form (fp_level_preferred) and train_mlp.fp_level_ragged_supported says yes: weights, interpolation,
        concatenation and the stack as ONE node with the row mask inside, layer 1 once per known point
        (fp_level_train(..., lengths=)); last_path "fused_train_ragged_node". Without that attribute the two-launch route is
        taken even where fp_level_preferred would choose the node.
        lengths2: a ragged KNOWN side as well (cloud i's known points are xyz2[i, :lengths2[i]], points2 likewise): only
        three_nn changes -- idx stays below lengths2[i] on the valid rows, so the padding rows of points2 are never gathered
        and their gradient is exactly zero; they must be finite (the one-node form multiplies every known row by W1a)."""
        b, n = xyz1.shape[0], xyz1.shape[1]
        dev = xyz1.device
        lens = ragged_lengths(lengths1, b, dev, "lengths1")
        if self.fused_ragged_eval and not self.training:
            kind = self._fused_kind(points1, points2, b * n)
            if kind is not None:
                # the level's kernel with lengths1 inside (padding rows gather nothing and come back as +0.0; points1 may hold
                # anything there): ONE C call behind the two-sided three_nn, or the kernel alone on a geometry
                self.last_path = "fused_ragged"
                packed = self._packed(points2.shape[2], points1.shape[2] if points1 is not None else 0, kind, points2.device)
                if geometry is not None:
                    g = geometry.wait()
                    return sa_mlp.fp_mlp(points2, points1, g.idx, g.dist, packed, lengths1=lens)
                return sa_mlp.fp_level_ragged(xyz1, xyz2, points1, points2, packed, lens, lengths2, self._level_buffers())
        valid = torch.arange(n, device=dev, dtype=torch.int32).unsqueeze(0) < lens.unsqueeze(1)      # (b, n), no host sync
        if geometry is not None:
            g = geometry.wait()
        else:
            dist, idx = three_nn(xyz1, xyz2, lengths1=lens, lengths2=lengths2)   # :211
            g = FPGeometry(dist, idx, self._plan_of(idx, xyz2.shape[1]))
        if not self.training:
            out = self._forward_on(xyz1, points1, points2, g)
            return torch.where(valid.unsqueeze(2), out, torch.zeros((), dtype=out.dtype, device=dev))
        if self.fused_ragged_train and xyz1.is_cuda and self._train_mode(points1, points2, b * n) == "fused_train" and \
                train_mlp.ragged_supported(self.mlp.net, b, n):
            return self._stack_on(xyz1, points1, points2, g, lens, paths=("fused_train_ragged", "fused_train_ragged_node"),
                                  node_ok=lambda *level: self.fused_ragged_node and train_mlp.fp_level_ragged_supported(*level))
        self.last_path = "unfused_ragged"
        interpolated = three_interpolate(points2, g.idx, _inverse_distance_weights(g.dist), plan=getattr(g, "plan", None))   # :212-216
        x = torch.cat([interpolated, points1], dim=2) if points1 is not None else interpolated   # :219
        rows = _valid_row_list(valid)
        xv = x.reshape(b * n, x.shape[2]).index_select(0, rows)                 # the valid rows of all clouds, (total, C)
        y = self.mlp(xv.t().unsqueeze(0).unsqueeze(3))                          # (1, C, total, 1): statistics over the valid rows
        yv = y[0, :, :, 0].t()
        return _scatter_rows(yv, rows, b * n).reshape(b, n, yv.shape[1])

    def _forward_packed(self, xyz1, xyz2, points1, points2, offsets1, max_points1, lengths2=None):
        """forward() with a PACKED unknown side: xyz1 (total, 3), points1 (total, c1) or None, cloud i = rows
        offsets1[i] .. offsets1[i + 1] - 1; the known side xyz2 (B, m, 3), points2 (B, m, c2) is a previous level's dense
        output. Packed three_nn with global indices gives FPGeometry(dist, idx (1, total, 3)) in the FLAT VIEW, idx naming rows
        of points2 viewed as (1, B m, c2); the inference kernel and _stack_on run unchanged on it. -> (total, C).
        eval(): the fused kernel where _fused_kind has one for `total` rows. train(): `total` a multiple of 32 -- the dense
        routes of _stack_on, no mask anywhere. Otherwise the stack's rows are extended to the next multiple of 32 (idx 0 /
        dist 0 / points1 0 on the <= 31 tail rows) and the masked plain-rows node runs with b = 1 and lengths =
        offsets1[B : B + 1] = total, already on the device: the tail is the only masked word, nothing synchronises; where the
        masked node does not cover the stack, layer by layer on the `total` rows. last_path: the route's with "packed_" in front.
        lengths2 (set_packed_pairs(True)): a previous level's npoints -- handed to the packed three_nn, so every idx names one of
        its cloud's first lengths2[i] known rows; nothing else changes."""
        dev = xyz1.device
        b, m, c2 = points2.shape
        offs, b, total, nmax = packed_args(offsets1, max_points1, None, xyz1, "PointnetFPModule", "offsets1", "max_points1", b=b)
        c1 = 0
        if points1 is not None:
            require(points1.dim() == 2 and points1.shape[0] == total, "PointnetFPModule: with offsets1, points1 is (total, channel)")
            c1 = points1.shape[1]
        p2 = points2.reshape(1, b * m, c2)
        kind = self._fused_kind(points1.view(1, total, c1) if points1 is not None else None, p2, total)
        n32 = (total + 31) // 32 * 32
        tail = kind is None and n32 != total and self.training and xyz1.is_cuda and self.fused_mlp and \
            train_mlp.ragged_supported(self.mlp.net, 1, n32) and self._train_mode(None, p2, n32) == "fused_train"
        rows = n32 if tail else total
        # three_nn writes the first `total` rows of buffers that already have the stack's row count
        dist = torch.zeros((rows, 3), dtype=torch.float32, device=dev) if tail else torch.empty((rows, 3), dtype=torch.float32, device=dev)
        idx = torch.zeros((rows, 3), dtype=torch.int32, device=dev) if tail else torch.empty((rows, 3), dtype=torch.int32, device=dev)
        three_nn(xyz1.detach(), xyz2.detach(), out=(dist[:total], idx[:total]), lengths2=lengths2, offsets1=offs, max_points1=nmax,
                 global_idx=True)                                               # :211
        g = FPGeometry(dist.view(1, rows, 3), idx.view(1, rows, 3), self._plan_of(idx.view(1, rows, 3), b * m))
        if tail:
            p1 = torch.nn.functional.pad(points1, (0, 0, 0, rows - total)).view(1, rows, c1) if points1 is not None else None
            x1 = xyz1.new_empty((1, rows, 0))                                   # (_stack_on reads the row count off it, nothing else)
            out = self._stack_on(x1, p1, p2, g, offs[b:b + 1], paths=("fused_train_ragged", "fused_train_ragged_node"),
                                 node_ok=lambda *level: self.fused_ragged_node and train_mlp.fp_level_ragged_supported(*level))
            self.last_path = "packed_" + self.last_path
            return out[0, :total]
        x1 = xyz1.reshape(1, total, 3)
        p1 = points1.reshape(1, total, c1) if points1 is not None else None
        if kind is not None:
            self.last_path = "packed_fused"
            return sa_mlp.fp_mlp(p2, p1, g.idx, g.dist, self._packed(c2, c1, kind, dev))[0]
        out = self._stack_on(x1, p1, p2, g)
        self.last_path = "packed_" + self.last_path
        return out[0]

    def forward(self, xyz1, xyz2, points1, points2, geometry=None, lengths1=None, lengths2=None, offsets1=None, max_points1=None):
        """three_nn -- computed ahead (geometry=) or here -- then the stack on its result (_stack_on). One route stays apart:
        inference without a geometry is ONE C call (sa_mlp.fp_level: three_nn and the level's kernel; it owns the level's
        buffers). lengths1: a ragged unknown side, see _forward_ragged. lengths2: a ragged known side (a previous level's
        npoints); without lengths1 the unknown side is dense and the result is that of the dense routes on the two-sided
        three_nn's result. offsets1 / max_points1: a packed unknown side, xyz1 (total, 3) and points1 (total, c1), see
        _forward_packed; ValueError with lengths1 / lengths2 or a geometry= (lengths2 is offered under set_packed_pairs(True))."""
        if offsets1 is not None:
            require(lengths1 is None and (lengths2 is None or packed_pairs()),
                    "PointnetFPModule: offsets1 and lengths1 / lengths2 are two layouts; give one")
            require(geometry is None, "PointnetFPModule: a geometry computed ahead is not offered with offsets1")
            return self._forward_packed(xyz1, xyz2, points1, points2, offsets1, max_points1, lengths2)
        if lengths1 is not None:
            return self._forward_ragged(xyz1, xyz2, points1, points2, lengths1, geometry, lengths2)
        if geometry is None and lengths2 is not None:
            dist, idx = three_nn(xyz1, xyz2, lengths2=lengths2)                  # :211
            return self._forward_on(xyz1, points1, points2, FPGeometry(dist, idx, self._plan_of(idx, xyz2.shape[1])))
        if geometry is not None:
            return self._forward_on(xyz1, points1, points2, geometry.wait())
        kind = self._fused_kind(points1, points2, xyz1.shape[0] * xyz1.shape[1])
        if kind is not None:
            # ONE C call (csrc/levels.hip): three_nn, then one kernel for weights, interpolation, concatenation and the
            # layer stack (:211-226)
            self.last_path = "fused"
            c1 = points1.shape[2] if points1 is not None else 0
            return sa_mlp.fp_level(xyz1, xyz2, points1, points2, self._packed(points2.shape[2], c1, kind, points2.device),
                                   self._level_buffers())
        return self._stack_on(xyz1, points1, points2, FPGeometry(*three_nn(xyz1, xyz2)))                  # :211

    def _after_weights(self, points1, points2, idx, weight, plan=None):
        """:216-226 of the layer-by-layer path."""
        interpolated = three_interpolate(points2, idx, weight, plan=plan)       # :216
        x = torch.cat([interpolated, points1], dim=2) if points1 is not None else interpolated   # :219
        if self.fused_mlp and self.training and x.is_cuda and \
                train_mlp.stack_supported(self.mlp.net, x.shape[0] * x.shape[1], 0, False):
            # training: the layer stack with batch-statistics batch norm as one autograd node (train_mlp.py)
            self.last_path = "fused_train"
            return train_mlp.fp_mlp_train(self.mlp.net, x)
        if self._frozen_ok(None, x, x.shape[0] * x.shape[1]):
            self.last_path = "fused_frozen"
            return train_mlp.fp_mlp_train(self.mlp.net, x, frozen=True)
        self.last_path = "unfused"
        x = self.mlp(x.permute(0, 2, 1).unsqueeze(2))                           # (b, C, 1, n)
        return x.squeeze(2).permute(0, 2, 1).contiguous()
