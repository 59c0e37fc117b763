"""Training mode of the shared MLPs (conv 1x1 + batch norm with BATCH statistics + ReLU stacks, SA levels with
their max-pool) on the matrix cores: forward and backward, one C call per direction.

Reference: utils/pointnet_util.py:113-127 (SA), :222-226 (FP), tf_util.py:512-531 (batch moments, moving
averages), train.py:96-104 (bn_decay schedule), train.py:188 (is_training = True). Kernels and the pass structure:
csrc/train_mlp.hip, include/pn2ops.h (pn2_mlp_train_forward / _backward); SURVEY.md section 8 row f2.

What autograd sees is ONE node per level: inputs = the grouped features (or the plain rows of an FP level) and
the level's parameters; saved for backward = the pre-norm tensors z_l (rows, C_l) and a few per-channel vectors.
The grouped (b, m, nsample, C) tensors, the normalised / rectified activations and the ReLU masks never exist.
"""
import contextlib
import ctypes

import torch
import torch.nn as nn

from . import _C
from ._tensors import f32, i32, is_deterministic, on_device, ptr, ragged_lengths, require, same_device, scatter_grad, stream_ptr

_vp, _i, _ll, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float


class GroupSrc(ctypes.Structure):          # pn2_group_src
    _fields_ = [("b", _i), ("n", _i), ("m", _i), ("nsample", _i), ("cfeat", _i), ("xyz_first", _i),
                ("xyz", _vp), ("new_xyz", _vp), ("points", _vp), ("idx", _vp), ("idx_plan", _vp)]


class BnLayer(ctypes.Structure):           # pn2_bn_layer
    _fields_ = [("cin", _i), ("cout", _i), ("weight", _vp), ("w_stride_k", _ll), ("w_stride_n", _ll), ("bias", _vp),
                ("gamma", _vp), ("beta", _vp), ("running_mean", _vp), ("running_var", _vp), ("momentum", _f), ("eps", _f),
                ("z", _vp), ("save", _vp), ("grad_weight", _vp), ("grad_gamma", _vp), ("grad_beta", _vp), ("grad_accumulate", _i),
                ("running_var_biased", _i)]


class FpSrc(ctypes.Structure):             # pn2_fp_src
    _fields_ = [("b", _i), ("n", _i), ("m", _i), ("c2", _i), ("c1", _i), ("points2", _vp), ("points1", _vp), ("idx", _vp),
                ("dist", _vp), ("idx_plan", _vp)]


class TrainOpts(ctypes.Structure):         # pn2_train_opts: 0 = automatic, 1 = off, 2 = on
    _fields_ = [("top_stored", _i), ("top_sparse", _i), ("l1_per_point", _i), ("l1_coords", _i), ("force_stream", _i),
                ("max_ns", _i), ("nt", _i), ("fuse_wgrad", _i), ("wgrad_two_per_cu", _i), ("side_stream", _i),
                ("pair_launch", _i), ("fold_finalize", _i)]


_OPT_NAMES = tuple(name for name, _ in TrainOpts._fields_)
_OPTS = {}                         # overrides in force (empty: every rule automatic -> the library gets NULL)


def _opts_from(saved):
    """A dict of overrides -> the `const pn2_train_opts *` argument (a ctypes reference that keeps its struct alive), or None."""
    if not saved:
        return None
    o = TrainOpts()
    for k, v in saved.items():
        setattr(o, k, (v or 0) if k == "max_ns" else (0 if v is None else 2 if v else 1))
    return ctypes.byref(o)


def _opts():
    """The overrides in force. The SAME ones must reach the workspace query, the organisation queries, forward and backward
    of one node: backward re-reads what forward ran under (ctx.opts)."""
    return _opts_from(_OPTS)


def parse_options(text):
    """'top_stored=0,fuse_wgrad=1,max_ns=2' -> the keyword arguments of options() (the A/B scripts take such a string from
    their command line / PN2_TRAIN_OPTS; the package itself never reads the environment)."""
    kw = {}
    for item in (text or "").replace(" ", "").split(","):
        if not item:
            continue
        k, _, v = item.partition("=")
        require(k in _OPT_NAMES and v.lstrip("-").isdigit(), "bad training option %r" % item)
        kw[k] = int(v) if k == "max_ns" else (None if int(v) < 0 else bool(int(v)))
    return kw


@contextlib.contextmanager
def options(**kw):
    """Force the organisation of the training passes inside the block (tests that cover every variant, A/B timing):
    top_stored / top_sparse / l1_per_point / l1_coords / force_stream / nt / fuse_wgrad / wgrad_two_per_cu / side_stream / pair_launch / fold_finalize = True | False | None (automatic),
    max_ns = 1 | 2 | 4. Results never depend on them. They travel to the library as a per-call argument
    (pn2_mlp_train_*_ex); the library itself reads no environment variable. A node's backward runs under the options its
    forward ran under."""
    for k in kw:
        require(k in _OPT_NAMES, "unknown training option %r (known: %s)" % (k, ", ".join(_OPT_NAMES)))
    old = dict(_OPTS)
    _OPTS.update(kw)
    try:
        yield
    finally:
        _OPTS.clear()
        _OPTS.update(old)


def _widths_array(widths):
    return (ctypes.c_int * len(widths))(*widths)


def conv_bn_pairs(net):
    """[(conv, bn)] of an nn.Sequential of Conv (1x1) + BatchNorm + ReLU triples, or None if it is anything else."""
    mods, out = list(net), []
    if not mods or len(mods) % 3:
        return None
    for i in range(0, len(mods), 3):
        conv, bn, relu = mods[i], mods[i + 1], mods[i + 2]
        if not isinstance(conv, (nn.Conv2d, nn.Conv1d)) or not isinstance(bn, (nn.BatchNorm2d, nn.BatchNorm1d)) or \
                not isinstance(relu, nn.ReLU):
            return None
        if any(k != 1 for k in conv.kernel_size) or conv.groups != 1:
            return None
        out.append((conv, bn))
    return out


def _stack_widths(pairs, padded=False):
    """cin_1, cout_1 .. cout_L as the library's queries take them; padded: plain rows, whose input width fp_mlp_train
    zero-pads to a multiple of 4."""
    cin = pairs[0][0].in_channels
    return [(cin + 3) // 4 * 4 if padded else cin] + [c.out_channels for c, _ in pairs]


def stack_supported(net, rows, pool_rows=0, grouped=True):
    """Can pn2_mlp_train_forward run this stack on `rows` rows? (host-side check)"""
    pairs = conv_bn_pairs(net)
    if not pairs or len(pairs) > 8 or rows <= 0 or rows % 32 or rows >= 2 ** 31:
        return False
    if pool_rows and pool_rows != 16 and pool_rows % 32:
        return False
    for conv, bn in pairs:
        if conv.out_channels % 4 or bn.momentum is None or not bn.affine:
            return False
        # a batch norm frozen with bn.eval() inside a model in train() (fine-tuning) normalises with its RUNNING statistics
        # and must not update them: that is not this path (batch statistics), the layer-by-layer path handles it
        if not bn.training or not conv.training:
            return False
        if any(t is not None and t.dtype != torch.float32 for t in (conv.weight, conv.bias, bn.weight, bn.bias)):
            return False
    return True                    # plain rows of a width that is no multiple of 4 are zero-padded by fp_mlp_train


class _Level:
    """Non-tensor description of one call (what the autograd node needs besides its differentiable inputs)."""
    __slots__ = ("pairs", "rows", "pool_rows", "xyz", "new_xyz", "idx", "b", "n", "m", "nsample", "xyz_first", "grouped", "pooling",
                 "xyz_grad", "frozen", "plan")


# pointnet_sa_module's pooling modes (utils/pointnet_util.py:128-142) -> the library's codes (pn2_mlp_train_forward_pool)
POOLING = {"max": 0, "avg": 1, "weighted_avg": 2, "max_and_avg": 3}


def pool_supported(net, rows, ns, pooling):
    """Can the fused training node run this stack with this pooling on `rows` grouped rows in groups of `ns`?"""
    code = POOLING.get(pooling)
    if code is None or not stack_supported(net, rows, ns, True):
        return False
    widths = _stack_widths(conv_bn_pairs(net))
    return bool(_C.lib().pn2_mlp_train_pool_supported(rows, len(widths) - 1, _widths_array(widths), ns, code))


def xyz_grad_supported(net, rows, ns, pooling, b, n, m, cfeat, has_idx=True):
    """Can the fused training node also return the gradients with respect to xyz and new_xyz (sa_mlp_train(..., xyz_grad=True))
    for this stack on `rows` = b m ns grouped rows of b clouds of n points with cfeat feature channels? Mirrors
    pn2_mlp_train_xyz_supported: every pooling but weighted_avg, wherever pool_supported says yes. has_idx=False: group_all."""
    code = POOLING.get(pooling)
    if code is None or code == 2 or not stack_supported(net, rows, ns, True):
        return False
    widths = _stack_widths(conv_bn_pairs(net))
    gdims = (ctypes.c_int * 6)(b, n, m, ns, cfeat, 1 if has_idx else 0)
    return bool(_C.lib().pn2_mlp_train_xyz_supported(rows, len(widths) - 1, _widths_array(widths), ns, code, gdims))


def frozen_supported(net, rows, pool_rows=0, grouped=True, pooling="max", xyz_dims=None):
    """The mirror of stack_supported for a stack whose batch norms ALL normalise with their running statistics (`not
    bn.training`, with track_running_stats): can the frozen-statistics node (pn2_mlp_train_*_frozen; sa_mlp_train /
    fp_mlp_train with frozen=True) run it on `rows` rows? A mixed stack (some batch norms frozen, some not) is not supported.
    xyz_dims = (b, n, m, cfeat, has_idx): with the coordinate gradients as well (xyz_grad=True)."""
    pairs = conv_bn_pairs(net)
    code = POOLING.get(pooling)
    if not pairs or len(pairs) > 8 or code is None or rows <= 0 or rows % 32 or rows >= 2 ** 31:
        return False
    if grouped and (pool_rows <= 0 or (pool_rows != 16 and pool_rows % 32)):
        return False
    if not grouped and (pool_rows or code):
        return False
    for conv, bn in pairs:
        if conv.out_channels % 4 or not bn.affine or bn.training:
            return False
        if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
            return False
        if any(t is not None and t.dtype != torch.float32 for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean,
                                                                      bn.running_var)):
            return False
    if code == 0 and xyz_dims is None:
        return True                # as stack_supported: the max path needs no query of the library (the entries check their plan)
    widths = _stack_widths(pairs, padded=not grouped)
    gdims = None
    if xyz_dims is not None:
        if not grouped or code == 2:
            return False
        b, n, m, cfeat, has_idx = xyz_dims
        gdims = (ctypes.c_int * 6)(b, n, m, pool_rows, cfeat, 1 if has_idx else 0)
    return bool(_C.lib().pn2_mlp_train_frozen_supported(rows, len(widths) - 1, _widths_array(widths), pool_rows, code, gdims,
                                                        1 if xyz_dims is not None else 0))


def group_ragged_supported(net, b, n, m, nsample, cfeat, has_idx=True):
    """Can the fused training node run this stack on the GROUPED rows of a ragged batch -- sa_mlp_train(..., counts=): b clouds
    of n points, m groups of nsample rows (has_idx=False: the group_all level, m = 1 and nsample = n), cfeat feature channels,
    max pooling, batch statistics over the valid rows only? Mirrors pn2_mlp_train_group_ragged_supported."""
    if min(b, n, m, nsample) <= 0 or cfeat < 0 or not stack_supported(net, b * m * nsample, nsample, True):
        return False
    widths = _stack_widths(conv_bn_pairs(net))
    gdims = (ctypes.c_int * 6)(b, n, m, nsample, cfeat, 1 if has_idx else 0)
    return bool(_C.lib().pn2_mlp_train_group_ragged_supported(b * m * nsample, len(widths) - 1, _widths_array(widths), nsample, gdims))


def ragged_supported(net, b, n):
    """Can the fused training node run this stack on the plain rows of a RAGGED batch -- b clouds padded to n rows, batch
    statistics over the valid rows only (fp_mlp_train(..., lengths=), pn2_mlp_train_*_ragged)? Mirrors
    pn2_mlp_train_ragged_supported: b n a positive multiple of 32, and a stack stack_supported takes as plain rows."""
    if b <= 0 or n <= 0 or not stack_supported(net, b * n, 0, False):
        return False
    widths = _stack_widths(conv_bn_pairs(net), padded=True)
    return bool(_C.lib().pn2_mlp_train_ragged_supported(b, n, len(widths) - 1, _widths_array(widths)))


_PLAN_FIELDS = 14                    # PN2_RAGGED_PLAN_FIELDS
_PLAN_AMODES = {0: "A_PLAIN", 1: "A_GATHER", 2: "A_RELU", 3: "A_DZ"}


def ragged_plan(b, n, widths, fp=None):
    """What one ragged forward + backward launches on the matrix cores under the options in force (options(...)), from the
    library's own size rules (pn2_mlp_train_ragged_plan; fp=(m, c2, c1): pn2_mlp_train_fp_ragged_plan): host logic, no device
    work (tests, maintainers). widths: cin_1 (a multiple of 4; FP: c2 + c1), cout_1 .. cout_L. -> one dict per pass in launch
    order: kind "gemm" (ns, amode, resident, slabs, nt, grid) or "wgrad" (tpw, upw, two, slabs, tus, tts, grid), backward,
    layer (1-based), masked, rows, K, N. `two` and a weight gradient's grid follow the device's CU count (256 without one)."""
    warr, opts = _widths_array(widths), _opts()
    head = (b, n) + (tuple(fp) if fp is not None else ()) + (len(widths) - 1, warr, opts)
    fn = _C.lib().pn2_mlp_train_fp_ragged_plan if fp is not None else _C.lib().pn2_mlp_train_ragged_plan
    return _plan_passes(fn, head)


def group_ragged_plan(b, n, m, nsample, cfeat, widths, has_idx=True):
    """ragged_plan for the GROUPED rows of a ragged batch (sa_mlp_train(..., counts=), pn2_mlp_train_group_ragged_plan): b clouds
    of n points, m groups of nsample rows each (has_idx=False: group_all, m = 1 and nsample = n), cfeat feature channels;
    widths: 3 + cfeat, cout_1 .. cout_L. The same dicts; forward layer 1 has amode "A_GATHER", backward layer 1's weight
    gradient `gather` True (on every other weight gradient it is False). The pool and its gradient are not listed."""
    gdims = (ctypes.c_int * 6)(b, n, m, nsample, cfeat, 1 if has_idx else 0)
    head = (b * m * nsample, len(widths) - 1, _widths_array(widths), nsample, gdims, _opts())
    return _plan_passes(_C.lib().pn2_mlp_train_group_ragged_plan, head)


def _plan_passes(fn, head):
    """The records of a plan entry fn(*head, passes, cap) as dicts."""
    count = fn(*head, None, 0)
    require(count >= 0, "ragged_plan: unsupported shape (%s)" % _C.PN2_ERRORS.get(count, count))
    buf = (ctypes.c_int * (count * _PLAN_FIELDS))()
    require(fn(*head, buf, count) == count, "ragged_plan: the pass count changed between two queries")
    passes = []
    for i in range(count):
        r = buf[i * _PLAN_FIELDS:(i + 1) * _PLAN_FIELDS]
        p = dict(kind="wgrad" if r[0] else "gemm", backward=bool(r[1]), layer=r[2], masked=bool(r[3]), rows=r[4], K=r[5], N=r[6])
        if r[0]:
            p.update(tpw=r[7], upw=r[8], two=bool(r[9]), slabs=r[10], tus=r[11], grid=r[12], tts=r[13], gather=r[3] == 2)
        else:
            p.update(ns=r[7], amode=_PLAN_AMODES[r[8]], resident=bool(r[9]), slabs=r[10], nt=bool(r[11]), grid=r[12])
        passes.append(p)
    return passes


def _layer_array(level, weights, biases, gammas, betas, zs, saves, grads=None, update_running=True):
    n = len(level.pairs)
    arr = (BnLayer * n)()
    for l, (conv, bn) in enumerate(level.pairs):
        L = arr[l]
        cin = weights[l].shape[1]                                  # conv.in_channels, or its zero-padded width (fp_mlp_train)
        L.cin, L.cout = cin, conv.out_channels
        L.weight = ptr(weights[l])
        L.w_stride_k, L.w_stride_n = 1, cin                        # conv kernel (cout, cin, 1[, 1]): W[k][n] = weight[n][k]
        L.bias = ptr(biases[l])
        L.gamma, L.beta = ptr(gammas[l]), ptr(betas[l])
        track = update_running and bn.track_running_stats and bn.running_mean is not None
        L.running_mean = ptr(bn.running_mean) if track else None
        L.running_var = ptr(bn.running_var) if track else None
        L.momentum, L.eps = float(bn.momentum), float(bn.eps)
        L.z, L.save = ptr(zs[l]), ptr(saves[l])
        # tf.contrib.layers.batch_norm feeds the BIASED batch variance to the moving variance (tf_util.py:512-531), torch the
        # unbiased one: a batch-norm module marked with `running_var_biased = True` (pointnet_util.use_tf_moving_variance)
        # follows the reference
        L.running_var_biased = 1 if getattr(bn, "running_var_biased", False) else 0
        if grads is not None:
            L.grad_weight, L.grad_gamma, L.grad_beta = ptr(grads[l][0]), ptr(grads[l][1]), ptr(grads[l][2])
    return arr


def _group_struct(level, points):
    g = GroupSrc()
    g.b, g.n, g.m, g.nsample = level.b, level.n, level.m, level.nsample
    g.cfeat = points.shape[2] if points is not None else 0
    g.xyz_first = 1 if level.xyz_first else 0
    g.xyz, g.new_xyz, g.points, g.idx = ptr(level.xyz), ptr(level.new_xyz), ptr(points), ptr(level.idx)
    if level.plan is not None:                 # backward's scatters onto the points reduce from it and invert nothing
        g.idx_plan = ptr(level.plan.buffer)
    return g


def _group_dims(level, points):
    """{b, n, m, nsample, cfeat, idx != NULL} of a grouped level for the workspace / per-point queries, or None."""
    if not level.grouped:
        return None
    return (ctypes.c_int * 6)(level.b, level.n, level.m, level.nsample, points.shape[2] if points is not None else 0,
                              1 if level.idx is not None else 0)


def _workspace(query_name, dev, error_text, *args):
    """The scratch buffer of one call, sized by the library's query `query_name(*args)`."""
    nbytes = getattr(_C.lib(), query_name)(*args)
    require(nbytes >= 0, error_text)
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)


def _level_workspace(level, widths, code, backward, dev, gdims, opts, want_xyz=False, ragged=False):
    """... of an SA / plain-rows node: the query that belongs to the level's mode."""
    if ragged and level.grouped:
        return _workspace("pn2_mlp_train_ws_bytes_group_ragged", dev, "pn2_mlp_train_group_ragged: unsupported level",
                          level.rows, len(widths) - 1, _widths_array(widths), level.pool_rows, backward, gdims, opts)
    if ragged:
        return _workspace("pn2_mlp_train_ws_bytes_ragged", dev, "pn2_mlp_train_ragged: unsupported stack (b n % 32, widths % 4)",
                          level.b, level.n, len(widths) - 1, _widths_array(widths), backward, opts)
    head = (level.rows, len(widths) - 1, _widths_array(widths), level.pool_rows)
    if level.frozen:
        return _workspace("pn2_mlp_train_ws_bytes_frozen", dev,
                          "pn2_mlp_train: unsupported stack or pooling for frozen batch-norm statistics",
                          *head, code, backward, gdims, 1 if want_xyz else 0, opts)
    if want_xyz:
        return _workspace("pn2_mlp_train_ws_bytes_xyz", dev, "pn2_mlp_train: unsupported stack or pooling for the coordinate gradients",
                          *head, code, gdims, opts)
    if code:
        return _workspace("pn2_mlp_train_ws_bytes_pool", dev, "pn2_mlp_train: unsupported stack or pooling", *head, code, backward, gdims,
                          opts)
    return _workspace("pn2_mlp_train_ws_bytes_ex", dev,
                      "pn2_mlp_train: unsupported stack (rows %% 32, widths %% 4, pool group 16 or a multiple of 32)",
                      *head, backward, gdims, opts)


_KEEP_WS = [False, None]          # diagnostics (scripts/train_mlp_check.py): keep the last backward's workspace
_ACCUMULATE = [False]


def set_accumulate_into_grad(flag):
    """Opt in: when a layer's parameters already HAVE `.grad` tensors (a flat gradient bucket's views, sharding.GradBucket,
    or a second micro-batch), the backward kernels add their results into them (pn2_bn_layer.grad_accumulate) and the
    autograd node returns no gradient for those parameters -- instead of autograd launching one `grad += new` per
    parameter afterwards (46 launches = 0.2 ms of a pointnet2_cls_ssg step). Same arithmetic: one fp32 add per element.
    Off by default because parameter hooks (DistributedDataParallel's) do not see gradients that bypass autograd.
    Only for `loss.backward()`: under `torch.autograd.grad(...)` `.grad` must not be touched, and a node cannot tell the
    two apart -- so do not call autograd.grad on these levels while the mode is on (it would receive None for the
    parameters and find them added to `.grad`). Prefer the scoped form, `with accumulate_into_grad(): loss.backward()`."""
    _ACCUMULATE[0] = bool(flag)


@contextlib.contextmanager
def accumulate_into_grad(flag=True):
    """set_accumulate_into_grad for the duration of a block (around `loss.backward()`)."""
    old = _ACCUMULATE[0]
    _ACCUMULATE[0] = bool(flag)
    try:
        yield
    finally:
        _ACCUMULATE[0] = old


def _grad_slot(param, like):
    """param.grad if the kernels may add into it: the saved tensor IS the parameter (not a padded copy), fp32, dense."""
    g = param.grad
    if g is None or not param.requires_grad or like.data_ptr() != param.data_ptr() or like.shape != param.shape:
        return None
    if g.dtype != torch.float32 or g.device != param.device or not g.is_contiguous() or g.shape != param.shape:
        return None
    return g


def _unpack_params(params, n):
    """A node's *params -> weights, biases (entries may be None), gammas, betas of its n layers."""
    return ([f32(params[4 * l], "weight") for l in range(n)], [params[4 * l + 1] for l in range(n)],
            [params[4 * l + 2] for l in range(n)], [params[4 * l + 3] for l in range(n)])


def _count_batch(pairs):
    nbt = [bn.num_batches_tracked for _, bn in pairs if bn.track_running_stats and bn.num_batches_tracked is not None]
    if nbt:
        torch._foreach_add_(nbt, 1)                            # one launch for the level's counters


def _batch_stat_grads(pairs, weights, gammas, betas):
    """Batch statistics: per layer the (weight, gamma, beta) gradients the kernels write -- the parameters' own .grad where the
    kernels may add into it (`direct`, set_accumulate_into_grad), else fresh tensors."""
    grads, direct = [], []
    for l, (conv, bn) in enumerate(pairs):
        slots = (_grad_slot(conv.weight, weights[l]), _grad_slot(bn.weight, gammas[l]), _grad_slot(bn.bias, betas[l])) \
            if _ACCUMULATE[0] else (None, None, None)
        direct.append(all(t is not None for t in slots))
        grads.append(slots if direct[-1] else
                     (torch.empty_like(weights[l]), torch.empty_like(gammas[l]), torch.empty_like(betas[l])))
    return grads, direct


def _batch_stat_results(grads, direct, biases, widths, dev):
    """... and what the node returns for them, four per layer. The conv bias gradients are exactly zero under batch norm (one
    zero buffer, one fill launch, a view per layer)."""
    result, zero, off = [], None, 0
    for l in range(len(grads)):
        if direct[l]:                                          # added into .grad by the kernels (zero for the bias: nothing to add)
            result += [None, None, None, None]
        else:
            if zero is None and biases[l] is not None:
                zero = torch.zeros((sum(widths[1:]),), dtype=torch.float32, device=dev)
            gb = zero[off:off + widths[l + 1]] if biases[l] is not None else None
            result += [grads[l][0], gb, grads[l][1], grads[l][2]]
        off += widths[l + 1]
    return result


def _frozen_stat_grads(pairs, weights, biases, gammas, betas, widths, needs, dev):
    """Frozen statistics: per layer the (weight, gamma, beta) gradients the kernels write and the conv bias gradient (real
    under frozen statistics) -> grads, direct, gbias. needs[l]: which of the layer's (weight, bias, gamma, beta) want a gradient.
    NULL slots for a layer none of whose parameters wants one: the library then runs no weight-gradient pass for it. Otherwise
    the three tensors the kernels write are all given (scratch for an unwanted one)."""
    grads, direct, gbias = [], [], [None] * len(pairs)
    small, soff = None, 0                  # ONE buffer for the per-channel gradients (gamma, beta, bias) of every layer
    for l, (conv, bn) in enumerate(pairs):
        need = needs[l]
        if not any(need):
            direct.append(False)
            grads.append((None, None, None))
            continue
        srcs = ((conv.weight, weights[l]), (conv.bias, biases[l]), (bn.weight, gammas[l]), (bn.bias, betas[l]))
        slots = [_grad_slot(p, like) if (_ACCUMULATE[0] and nd) else None for (p, like), nd in zip(srcs, need)]
        d = _ACCUMULATE[0] and all(s is not None for s, nd in zip(slots, need) if nd)     # direct: every WANTED slot exists
        direct.append(d)
        if small is None:                  # (a level is bound by the host's enqueue rate: one allocation, not three per layer)
            small = torch.empty((3 * sum(widths[1:]),), dtype=torch.float32, device=dev)
        w = widths[l + 1]
        vec = [small[soff + k * w:soff + (k + 1) * w] for k in range(3)]
        soff += 3 * w
        # (a direct layer's UNWANTED slot is scratch the kernels add into and nobody reads: never returned)
        grads.append((slots[0] if (d and need[0]) else torch.empty_like(weights[l]),
                      slots[2] if (d and need[2]) else vec[0], slots[3] if (d and need[3]) else vec[1]))
        if need[1]:
            gbias[l] = slots[1] if d else vec[2]
    return grads, direct, gbias


def _frozen_stat_results(grads, direct, gbias, needs):
    """... and what the node returns for them, four per layer: only what was wanted, nothing for a direct layer."""
    result = []
    for l, nd in enumerate(needs):
        if direct[l] or not any(nd):
            result += [None, None, None, None]
        else:
            result += [grads[l][0] if nd[0] else None, gbias[l], grads[l][1] if nd[2] else None, grads[l][2] if nd[3] else None]
    return result


def _forward_stack(level, params, keep_top=None):
    """What every node's forward begins with -> n, dev, widths, the options in force, the layer array and `layers` for
    _save_layers: the parameters unpacked, the pre-norm tensors z_l -- the only activations kept -- and the per-channel
    statistics. keep_top(n, widths array, opts) false: the top layer's z is not even written (a pooled top layer on a large level)."""
    n = len(level.pairs)
    weights, biases, gammas, betas = _unpack_params(params, n)
    dev = weights[0].device
    widths = [weights[0].shape[1]] + [c.out_channels for c, _ in level.pairs]
    opts = _opts()
    top = keep_top is None or keep_top(n, _widths_array(widths), opts)
    zs = [torch.empty((level.rows, w), dtype=torch.float32, device=dev) if (top or l < n - 1) else None
          for l, w in enumerate(widths[1:])]
    saves = [torch.empty((4, w), dtype=torch.float32, device=dev) for w in widths[1:]]
    return n, dev, widths, opts, _layer_array(level, weights, biases, gammas, betas, zs, saves), (weights, biases, gammas, betas, zs, saves)


def _backward_stack(ctx, needs=None):
    """What every node's backward begins with -> the node's own saved tensors (head, out, tail), dev, the options forward ran
    under, the layer array with the parameters' gradient slots, and `pgrads` for _param_grads. needs: frozen statistics -- per
    layer which of (weight, bias, gamma, beta) want a gradient; None: batch statistics."""
    level, widths = ctx.level, ctx.widths
    n = len(level.pairs)
    head, weights, biases, gammas, betas, zs, saves, out, tail = _saved_layers(ctx, n)
    dev = out.device
    gbias = None
    if needs is not None:
        grads, direct, gbias = _frozen_stat_grads(level.pairs, weights, biases, gammas, betas, widths, needs, dev)
    else:
        grads, direct = _batch_stat_grads(level.pairs, weights, gammas, betas)
    # (frozen: the library wants the running statistics named in both directions; it only ever reads them)
    arr = _layer_array(level, weights, biases, gammas, betas, zs, saves, grads, update_running=needs is not None)
    for l in range(n):
        arr[l].grad_accumulate = 1 if direct[l] else 0
    return head, out, tail, dev, _opts_from(ctx.opts), arr, (needs, grads, direct, gbias, biases, widths, dev)


def _param_grads(pgrads):
    """... and what the node returns for the parameters, four per layer."""
    needs, grads, direct, gbias, biases, widths, dev = pgrads
    if needs is not None:                                      # (the conv bias takes a real gradient under frozen statistics)
        return _frozen_stat_results(grads, direct, gbias, needs)
    return _batch_stat_results(grads, direct, biases, widths, dev)


def _ragged_mask(rows, dev):
    """The buffer a node owns on ragged rows: forward writes it (the valid-row count, one validity word per 32 rows), backward
    reads it. 16 + 4 (rows / 32) bytes, 8-byte aligned."""
    return torch.empty((2 + (rows // 32 + 1) // 2,), dtype=torch.int64, device=dev)


def _save_layers(ctx, level, widths, layers, head, out, tail=()):
    """save_for_backward of a training node: its own leading tensors, then per layer the weights, the biases and pre-norm tensors
    that exist, gammas, betas and statistics, the output, its own trailing tensors. _saved_layers is the inverse."""
    weights, biases, gammas, betas, zs, saves = layers
    ctx.level, ctx.widths = level, widths
    ctx.opts = dict(_OPTS)                                  # backward must see the organisation forward ran under
    ctx.nhead = len(head)
    ctx.nbias = [b is not None for b in biases]
    ctx.nz = [z is not None for z in zs]
    ctx.save_for_backward(*head, *weights, *[b for b in biases if b is not None], *gammas, *betas, *[z for z in zs if z is not None],
                          *saves, out, *tail)


def _saved_layers(ctx, n):
    """-> head, weights, biases, gammas, betas, zs, saves, out, tail as _save_layers was given them (None where nothing was)."""
    sv = list(ctx.saved_tensors)
    head = [sv.pop(0) for _ in range(ctx.nhead)]
    weights = [sv.pop(0) for _ in range(n)]
    biases = [sv.pop(0) if has else None for has in ctx.nbias]
    gammas = [sv.pop(0) for _ in range(n)]
    betas = [sv.pop(0) for _ in range(n)]
    zs = [sv.pop(0) if has else None for has in ctx.nz]
    saves = [sv.pop(0) for _ in range(n)]
    return head, weights, biases, gammas, betas, zs, saves, sv.pop(0), sv


class _TrainMLP(torch.autograd.Function):
    """inputs: level, x (points (b,n,c) when grouped -- may be None -- else the (rows, cin) input), xyz and new_xyz (the
    level's own tensors when their gradients are wanted, level.xyz_grad; else None: the coordinates are constants of the node),
    lengths ((b,) i32 on the device: the plain rows of a RAGGED batch, pn2_mlp_train_*_ragged -- or, on a grouped level, its
    per-cloud centroid counts / a group_all level's point counts, pn2_mlp_train_*_group_ragged; else None), then per layer
    conv.weight, conv.bias (or None), bn.weight, bn.bias. On ragged rows the node owns the validity mask: forward writes it, it
    is saved behind everything else with lengths, and the host never reads lengths -- no synchronisation in either direction."""

    @staticmethod
    def forward(ctx, level, x, xyz_in, new_xyz_in, lengths, *params):
        rows = level.rows
        code = level.pooling if level.pool_rows else 0
        ragged = lengths is not None
        # (the averaging modes always keep z_L: a mean does not commute with batch norm + ReLU; ragged rows are never pooled)
        n, dev, widths, opts, arr, layers = _forward_stack(level, params, lambda n, warr, opts: code != 0 or ragged or bool(
            _C.lib().pn2_mlp_train_top_stored_ex(rows, n, warr, level.pool_rows, opts)))
        cl = widths[-1]
        pool_w = None
        if level.pool_rows:
            groups = rows // level.pool_rows
            out = torch.empty((groups, 2 * cl if code == 3 else cl), dtype=torch.float32, device=dev)
            # argsel / zsel: the max's selection (max, max_and_avg); an empty placeholder for the averages
            argsel = torch.empty((groups, cl) if code in (0, 3) else (0,), dtype=torch.int32, device=dev)
            # (ragged grouped rows: the pool is a pass over z_L itself, there is no zsel)
            zsel = torch.empty((groups, cl), dtype=torch.float32, device=dev) if code in (0, 3) and not ragged else None
            if code == 2:
                pool_w = torch.empty((rows,), dtype=torch.float32, device=dev)
        else:
            out = torch.empty((rows, cl), dtype=torch.float32, device=dev)
            argsel = zsel = None
        mask = _ragged_mask(rows, dev) if ragged else None
        grp = _group_struct(level, x) if level.grouped else None
        ws = _level_workspace(level, widths, code, 0, dev, _group_dims(level, x), opts, ragged=ragged)
        gptr, xptr = (ctypes.byref(grp), None) if level.grouped else (None, ptr(x))
        with on_device(dev):
            if ragged and level.grouped:
                _C.check(_C.lib().pn2_mlp_train_forward_group_ragged(rows, n, arr, gptr, level.pool_rows, ptr(lengths), ptr(out),
                                                                     ptr(argsel), ptr(mask), ptr(ws), opts, stream_ptr(dev)),
                         "mlp_train_forward_group_ragged")
            elif ragged:
                _C.check(_C.lib().pn2_mlp_train_forward_ragged(level.b, level.n, ptr(lengths), n, arr, xptr, ptr(out), ptr(mask),
                                                               ptr(ws), opts, stream_ptr(dev)), "mlp_train_forward_ragged")
            elif level.frozen:      # running statistics (bn.eval()): read, never written -- no counter either
                _C.check(_C.lib().pn2_mlp_train_forward_frozen(rows, n, arr, gptr, xptr, level.pool_rows, code, ptr(out),
                                                               ptr(argsel) if code in (0, 3) else None, ptr(zsel), ptr(pool_w),
                                                               ptr(ws), opts, stream_ptr(dev)), "mlp_train_forward_frozen")
            elif code:              # avg / weighted_avg / max_and_avg (grouped levels only)
                _C.check(_C.lib().pn2_mlp_train_forward_pool(rows, n, arr, gptr, level.pool_rows, code, ptr(out),
                                                             ptr(argsel) if code == 3 else None, ptr(zsel), ptr(pool_w), ptr(ws),
                                                             opts, stream_ptr(dev)), "mlp_train_forward_pool")
            else:
                _C.check(_C.lib().pn2_mlp_train_forward_ex(rows, n, arr, gptr, xptr, level.pool_rows, ptr(out), ptr(argsel),
                                                           ptr(zsel), ptr(ws), opts, stream_ptr(dev)), "mlp_train_forward")
        if not level.frozen:
            _count_batch(level.pairs)
        ctx.code, ctx.ragged = code, ragged
        if not level.pool_rows:
            _save_layers(ctx, level, widths, layers, [x], out, [mask, lengths] if ragged else ())
            return out
        ctx.mark_non_differentiable(argsel)
        _save_layers(ctx, level, widths, layers, [x] if x is not None else [], out,
                     [argsel] + [t for t in (zsel, pool_w) if t is not None] + ([mask, lengths] if ragged else []))
        return out, argsel

    @staticmethod
    def backward(ctx, grad_out, *unused):
        level, widths, code = ctx.level, ctx.widths, ctx.code
        n = len(level.pairs)
        frozen = level.frozen
        # (the parameters stand behind level, x, xyz, new_xyz and lengths)
        head, out, tail, dev, opts, arr, pgrads = _backward_stack(
            ctx, [[bool(ctx.needs_input_grad[5 + 4 * l + k]) for k in range(4)] for l in range(n)] if frozen else None)
        x = head[0] if head else None
        argsel = tail.pop(0) if level.pool_rows else None
        ragged = ctx.ragged                                     # (what forward ran)
        zsel = tail.pop(0) if level.pool_rows and code in (0, 3) and not ragged else None
        pool_w = tail.pop(0) if code == 2 else None
        mask, lengths = tail if tail else (None, None)         # ragged rows: what forward saved last
        rows = level.rows
        grad_out = f32(grad_out, "grad_out")
        need_x = ctx.needs_input_grad[1] and x is not None
        # the coordinate gradients (sa_mlp_train(..., xyz_grad=True)): written by the library, both or neither
        want_xyz = level.xyz_grad and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
        grad_xyz = grad_new_xyz = None
        grad_x = grad_rows = grad_pts = None
        gdims = _group_dims(level, x)
        # (ragged grouped rows: one organisation, the gathered layer 1 -- the library writes the per-row gradient)
        per_point = level.grouped and mask is None and bool(_C.lib().pn2_mlp_train_layer1_per_point_ex(n, _widths_array(widths), gdims, opts))
        if need_x and level.grouped and per_point:
            grad_pts = torch.empty(tuple(x.shape), dtype=torch.float32, device=dev)      # written by the library itself
        elif need_x and level.grouped:
            grad_rows = torch.empty((rows, x.shape[2]), dtype=torch.float32, device=dev)
        elif need_x:
            grad_x = torch.empty((rows, widths[0]), dtype=torch.float32, device=dev)
        if want_xyz:
            grad_xyz = torch.empty((level.b, level.n, 3), dtype=torch.float32, device=dev)
            if level.new_xyz is not None:
                grad_new_xyz = torch.empty((level.b, level.m, 3), dtype=torch.float32, device=dev)
        ws = _level_workspace(level, widths, code, 1, dev, gdims, opts, want_xyz, ragged=mask is not None)
        if _KEEP_WS[0]:
            _KEEP_WS[1] = (ws, rows, widths, level.pool_rows)
        grp = _group_struct(level, x) if level.grouped else None
        with on_device(dev):
            if mask is not None and level.grouped:
                _C.check(_C.lib().pn2_mlp_train_backward_group_ragged(rows, n, arr, ctypes.byref(grp), level.pool_rows, ptr(lengths),
                                                                      ptr(out), ptr(argsel), ptr(grad_out), ptr(grad_rows),
                                                                      1 if is_deterministic() else 0, ptr(mask), ptr(ws), opts,
                                                                      stream_ptr(dev)), "mlp_train_backward_group_ragged")
            elif mask is not None:
                _C.check(_C.lib().pn2_mlp_train_backward_ragged(level.b, level.n, ptr(lengths), n, arr, ptr(x), ptr(out), ptr(grad_out),
                                                                ptr(grad_x), ptr(mask), ptr(ws), opts, stream_ptr(dev)),
                         "mlp_train_backward_ragged")
            elif frozen:
                gb_arr = (ctypes.c_void_p * n)(*[ptr(t) for t in pgrads[3]])
                _C.check(_C.lib().pn2_mlp_train_backward_frozen(rows, n, arr, ctypes.byref(grp) if grp is not None else None,
                                                                None if level.grouped else ptr(x), level.pool_rows, code, ptr(out),
                                                                ptr(argsel) if code in (0, 3) else None, ptr(zsel), ptr(pool_w),
                                                                ptr(grad_out), ptr(grad_x), ptr(grad_rows), ptr(grad_pts),
                                                                ptr(grad_xyz), ptr(grad_new_xyz), gb_arr,
                                                                1 if is_deterministic() else 0, ptr(ws), opts, stream_ptr(dev)),
                         "mlp_train_backward_frozen")
            elif want_xyz:
                _C.check(_C.lib().pn2_mlp_train_backward_xyz(rows, n, arr, ctypes.byref(grp), level.pool_rows, code, ptr(out),
                                                             ptr(argsel) if code in (0, 3) else None, ptr(zsel), None,
                                                             ptr(grad_out), ptr(grad_rows), ptr(grad_pts), ptr(grad_xyz),
                                                             ptr(grad_new_xyz), 1 if is_deterministic() else 0, ptr(ws), opts,
                                                             stream_ptr(dev)), "mlp_train_backward_xyz")
            elif code:
                _C.check(_C.lib().pn2_mlp_train_backward_pool(rows, n, arr, ctypes.byref(grp), level.pool_rows, code, ptr(out),
                                                              ptr(argsel) if code == 3 else None, ptr(zsel), ptr(pool_w),
                                                              ptr(grad_out), ptr(grad_rows), ptr(grad_pts),
                                                              1 if is_deterministic() else 0, ptr(ws), opts, stream_ptr(dev)),
                         "mlp_train_backward_pool")
            else:
                _C.check(_C.lib().pn2_mlp_train_backward_ex(rows, n, arr, ctypes.byref(grp) if grp is not None else None,
                                                            None if level.grouped else ptr(x), level.pool_rows, ptr(out), ptr(argsel),
                                                            ptr(zsel), ptr(grad_out), ptr(grad_x), ptr(grad_rows), ptr(grad_pts),
                                                            1 if is_deterministic() else 0, ptr(ws), opts, stream_ptr(dev)),
                         "mlp_train_backward")
            if grad_pts is not None:
                grad_x = grad_pts
            if grad_rows is not None:
                # the grouped feature rows' gradient back onto the points: group_point's backward (_tensors.scatter_grad)
                b, npts, c = x.shape
                m, ns = level.m, level.nsample
                if level.idx is None:                      # group_all: row k of cloud i IS point k
                    grad_x = grad_rows.view(b, npts, c)
                else:
                    grad_x = torch.empty((b, npts, c), dtype=torch.float32, device=dev)
                    _C.check(scatter_grad(_C.lib(), "group_point", (b, npts, c, m, ns, ptr(grad_rows)), level.idx, level.plan,
                                          (ptr(grad_x),), b, npts, c, m * ns, dev), "group_point_grad")
        result = [None, grad_x if need_x else None, grad_xyz if ctx.needs_input_grad[2] else None,
                  grad_new_xyz if ctx.needs_input_grad[3] else None, None]
        return tuple(result + _param_grads(pgrads))


def _params(pairs):
    out = []
    for conv, bn in pairs:
        out += [conv.weight, conv.bias, bn.weight, bn.bias]
    return out


def sa_mlp_train(net, xyz, new_xyz, points, idx, xyz_first=True, pooling="max", xyz_grad=False, frozen=False, plan=None, counts=None):
    """Training-mode shared MLP + pooling of one SA level / one MSG scale.
    net: nn.Sequential of (Conv2d 1x1, BatchNorm2d, ReLU) triples; xyz (b,n,3); new_xyz (b,m,3) or None and idx
    (b,m,nsample) i32 or None (both None: the group_all level); points (b,n,c) or None.
    pooling: "max" (default), "avg", "weighted_avg" or "max_and_avg" (utils/pointnet_util.py:128-142; the last gives
    (b, m, 2 cout) = concat([avg, max])).
    xyz_grad: xyz and new_xyz are differentiable inputs of the node too (GroupPoint's and GatherPoint's gradients through
    grouped_xyz - new_xyz, :44-46; pn2_mlp_train_backward_xyz) -- every pooling but weighted_avg. The gradient of new_xyz is
    returned for new_xyz itself: pass new_xyz = gather_point(xyz, fps_idx) and autograd adds the centroids' path back to xyz.
    Default False: the coordinates are constants of the node (no gradient flows to them), outputs and saved tensors the same bits.
    frozen: the stack's batch norms are all in eval() and normalise with their RUNNING statistics (pn2_mlp_train_*_frozen,
    frozen_supported): the statistics and num_batches_tracked are not touched, the conv biases take a real gradient, and
    parameters that need no gradient get none (a layer none of whose parameters needs one runs no weight-gradient pass).
    plan: an IndexPlan of idx (index_plan(idx, n, "group")): the backward's scatters onto the points -- the features' and, with
    xyz_grad, the coordinates' -- reduce from it, and idx is inverted nowhere in the backward.
    counts: (b,) per-cloud counts of a RAGGED batch (an int32 / int64 tensor or a sequence, ragged_lengths): with idx the number
    of valid CENTROIDS of each cloud (group j of cloud c is valid iff j < counts[c]; what geometry(npoints=) produced -- idx of a
    padding group must hold indices in [0, n), the two-sided ragged operators write 0), for the group_all form the number of valid
    POINTS (row k of cloud c is valid iff k < counts[c]). The batch statistics, the running averages and every gradient are
    those of the valid rows alone (group_ragged_supported; pn2_mlp_train_*_group_ragged). Rows of xyz / points beyond a cloud's
    own points and the output gradient of padding groups may hold anything, NaN included; the output and argsel of a padding group
    and the gradient of points on rows no valid group names are exactly zero. The host never reads the counts (no
    synchronisation; a count outside its range is clamped). Only with pooling="max", and not with xyz_grad or frozen
    (ValueError).
    -> (b, m, cout) pooled features (differentiable w.r.t. points and the parameters), argsel (b, m, cout) i32 -- the max's
    selection; None for avg and weighted_avg."""
    require(pooling in POOLING, "unknown pooling %r" % (pooling,))
    if counts is not None:
        bad = [t for t, on in (("pooling=%r" % (pooling,), pooling != "max"), ("xyz_grad=True", xyz_grad), ("frozen=True", frozen)) if on]
        require(not bad, "sa_mlp_train: counts= is not offered with %s" % " and ".join(bad))
    pairs = conv_bn_pairs(net)
    require(pairs is not None, "sa_mlp_train expects Conv 1x1 + BatchNorm + ReLU triples")
    xyz = f32(xyz, "xyz")
    require(xyz.dim() == 3 and xyz.shape[2] == 3, "xyz must be (b, n, 3), got %s" % (tuple(xyz.shape),))
    b, n, _ = xyz.shape
    lv = _Level()
    lv.pairs, lv.grouped, lv.xyz_first = pairs, True, bool(xyz_first)
    lv.xyz = xyz
    if idx is None:
        require(new_xyz is None, "group_all takes neither idx nor new_xyz")
        lv.new_xyz, lv.idx, lv.m, lv.nsample = None, None, 1, n
    else:
        # the kernels index xyz / points through idx and new_xyz through the group number: a mismatch reads out of bounds
        require(new_xyz is not None, "idx without new_xyz")
        lv.new_xyz, lv.idx = f32(new_xyz, "new_xyz"), i32(idx, "idx")
        require(idx.dim() == 3 and idx.shape[0] == b, "idx must be (b, m, nsample) with b = %d, got %s" % (b, tuple(idx.shape)))
        require(tuple(new_xyz.shape) == (b, idx.shape[1], 3),
                "new_xyz must be (b, m, 3) = %s, got %s" % ((b, idx.shape[1], 3), tuple(new_xyz.shape)))
        same_device(xyz, lv.new_xyz, lv.idx)
        lv.m, lv.nsample = idx.shape[1], idx.shape[2]
    lv.plan = None
    if plan is not None:
        require(idx is not None, "a group_all level has no idx and takes no plan")
        lv.plan = plan.check("group", b, n, lv.m * lv.nsample, xyz.device)
    lv.b, lv.n = b, n
    lv.rows = b * lv.m * lv.nsample
    lv.pool_rows = lv.nsample
    lv.pooling = POOLING[pooling]
    if points is not None:
        points = f32(points, "points")
        require(points.dim() == 3 and tuple(points.shape[:2]) == (b, n),
                "points must be (b, n, c) with (b, n) = %s, got %s" % ((b, n), tuple(points.shape)))
        same_device(xyz, points)
    cin = 3 + (points.shape[2] if points is not None else 0)
    require(pairs[0][0].in_channels == cin, "the first layer expects %d channels, got %d" % (pairs[0][0].in_channels, cin))
    lv.frozen = bool(frozen)
    if lv.frozen:
        require(frozen_supported(net, lv.rows, lv.pool_rows, True, pooling,
                                 (b, n, lv.m, points.shape[2] if points is not None else 0, idx is not None) if xyz_grad else None),
                "unsupported stack for the fused training path with frozen batch-norm statistics (pooling %r)" % (pooling,))
    else:
        require(stack_supported(net, lv.rows, lv.pool_rows, True), "unsupported stack for the fused training path")
        require(lv.pooling == 0 or pool_supported(net, lv.rows, lv.pool_rows, pooling),
                "unsupported stack for the fused training path with pooling %r" % (pooling,))
    same_device(xyz, pairs[0][0].weight)
    lv.xyz_grad = bool(xyz_grad)
    if counts is not None:
        counts = ragged_lengths(counts, b, xyz.device, "counts")
        require(group_ragged_supported(net, b, n, lv.m, lv.nsample, points.shape[2] if points is not None else 0, idx is not None),
                "unsupported level for the fused training path on ragged grouped rows")
        out, argsel = _TrainMLP.apply(lv, points, None, None, counts, *_params(pairs))
    elif lv.xyz_grad:
        require(lv.frozen or xyz_grad_supported(net, lv.rows, lv.pool_rows, pooling, b, n, lv.m, points.shape[2] if points is not None else 0,
                                   idx is not None),
                "the fused training path has no coordinate gradients for this level (pooling %r)" % (pooling,))
        out, argsel = _TrainMLP.apply(lv, points, lv.xyz, lv.new_xyz, None, *_params(pairs))
    else:
        out, argsel = _TrainMLP.apply(lv, points, None, None, None, *_params(pairs))
    if lv.pooling in (1, 2):
        return out.view(b, lv.m, -1), None
    return out.view(b, lv.m, -1), argsel.view(b, lv.m, -1)


def fp_mlp_train(net, x, cin=None, frozen=False, lengths=None):
    """Training-mode shared MLP of one FP level on plain rows: x (b, n, cin) -> (b, n, cout).
    cin: the first layer's input width when x already carries zero columns up to a multiple of 4 behind it
    (tf_interpolate.fp_interp_concat writes them); default: x's own width (padded here if odd).
    frozen: the batch norms normalise with their running statistics (see sa_mlp_train).
    lengths: (b,) per-cloud row counts of a ragged batch (cloud i is x[i, :lengths[i]]; an int32 / int64 tensor or a sequence,
    ragged_lengths): the batch statistics, the running averages and every gradient are those of the valid rows alone, as if the
    stack had run on the compacted rows (ragged_supported; pn2_mlp_train_*_ragged). The padding rows of x and of the output's
    gradient may hold anything, NaN included; the output and the gradient of x are exactly zero there. Nothing is compacted and
    the host never reads the lengths (no synchronisation; a length outside 1..n is clamped, check_lengths is where values are
    looked at). A batch with fewer than two valid rows has no variance: the caller's business. Not with frozen=True
    (ValueError: eval() + a torch.where already differentiates correctly there)."""
    pairs = conv_bn_pairs(net)
    require(pairs is not None, "fp_mlp_train expects Conv 1x1 + BatchNorm + ReLU triples")
    x = f32(x, "x")
    require(x.dim() == 3, "x must be (b, n, cin), got %s" % (tuple(x.shape),))
    b, n, c = x.shape
    if lengths is not None:
        require(not frozen, "fp_mlp_train: lengths= is not offered with frozen=True")
        lengths = ragged_lengths(lengths, b, x.device)
    if cin is not None and cin != c:
        require(cin < c and c % 4 == 0 and c - cin < 4, "x must be cin columns zero-padded to a multiple of 4")
        prepadded, c = True, cin
    else:
        prepadded = False
    same_device(x, pairs[0][0].weight)
    lv = _Level()
    lv.pairs, lv.grouped, lv.xyz_first = pairs, False, True
    lv.xyz = lv.new_xyz = lv.idx = lv.plan = None
    lv.b, lv.n, lv.m, lv.nsample = b, n, 0, 0
    lv.rows, lv.pool_rows, lv.pooling = b * n, 0, 0
    lv.frozen = bool(frozen)
    require(frozen_supported(net, lv.rows, 0, False) if lv.frozen else stack_supported(net, lv.rows, 0, False),
            "unsupported stack for the fused training path")
    require(lengths is None or ragged_supported(net, b, n), "unsupported stack for the fused training path on ragged rows")
    require(pairs[0][0].in_channels == c, "the first layer expects %d channels, got %d" % (pairs[0][0].in_channels, c))
    params = _params(pairs)
    x = x.reshape(b * n, x.shape[2])
    if c % 4:
        # the kernels read rows 16 bytes at a time: zero columns up to a multiple of 4 on the input and on the first
        # layer's weight (autograd slices both gradients back); part_seg's last level has 128 + 6 channels
        pad = 4 - c % 4
        if not prepadded:
            x = torch.nn.functional.pad(x, (0, pad))
        w = params[0]
        params[0] = torch.nn.functional.pad(w, (0, 0) * (w.dim() - 2) + (0, pad))
    lv.xyz_grad = False
    return _TrainMLP.apply(lv, x, None, None, lengths, *params).view(b, n, -1)


# ---- a feature-propagation level as ONE node with the interpolation inside (pn2_mlp_train_*_fp, csrc/train_mlp_fp.hip) ----
class _FpLevel:
    __slots__ = ("pairs", "rows", "b", "n", "m", "c2", "c1", "idx", "dist", "plan")


def fp_level_supported(net, b, n, m, c2, c1):
    """Can the FP training node (layer 1 per known point, pn2_mlp_train_*_fp) run this stack on b clouds of n unknown and m
    known points with c2 interpolated and c1 skip channels?"""
    pairs = conv_bn_pairs(net)
    if not pairs or len(pairs) > 7 or pairs[0][0].in_channels != c2 + c1 or not stack_supported(net, b * n, 0, False):
        return False
    return bool(_C.lib().pn2_mlp_train_fp_supported(b, n, m, c2, c1, len(pairs), _widths_array(_stack_widths(pairs))))


def fp_level_ragged_supported(net, b, n, m, c2, c1):
    """... and with a RAGGED unknown side (fp_level_train(..., lengths=), pn2_mlp_train_*_fp_ragged): where fp_level_supported
    holds and b n is a positive multiple of 32. Mirrors pn2_mlp_train_fp_ragged_supported."""
    if b <= 0 or n <= 0 or (b * n) % 32 or not fp_level_supported(net, b, n, m, c2, c1):
        return False
    widths = _stack_widths(conv_bn_pairs(net))
    return bool(_C.lib().pn2_mlp_train_fp_ragged_supported(b, n, m, c2, c1, len(widths) - 1, _widths_array(widths)))


# Where the modules take the node. It no longer forms the interpolated part of layer 1's input on the b (n - m) rows that are
# not known points, and pays for it with a few more latency-bound passes (two layer-1 GEMMs instead of one, the dz / scatter
# launches). Summed kernel time of one warm forward + backward (profiles/fp_train/README.md), node vs current path, and the
# saved elements b (n - m) c2: sem_seg FP4 391 vs 463 us (7.3 M), part_seg FP3 317 vs 338 (3.1 M), part_seg FP1 287 vs 375
# (2.1 M) -- and the other way round at part_seg FP2 219 vs 214 (1.6 M), sem_seg FP3 213 vs 208 (1.6 M), FP2 200 vs 172
# (0.4 M), FP1 199 vs 192 (0.2 M).
FP_NODE_MIN_SAVED = 1_800_000


def fp_level_preferred(b, n, m, c2):
    """Is the FP node faster than fp_interp_concat + fp_mlp_train at this size (FP_NODE_MIN_SAVED)? Results do not depend on it."""
    return b * (n - m) * c2 >= FP_NODE_MIN_SAVED


def _fp_src(level, points2, points1):
    s = FpSrc()
    s.b, s.n, s.m, s.c2, s.c1 = level.b, level.n, level.m, level.c2, level.c1
    s.points2, s.points1, s.idx, s.dist = ptr(points2), ptr(points1), ptr(level.idx), ptr(level.dist)
    if level.plan is not None:                 # backward's interpolation gradient reduces from it and inverts nothing
        s.idx_plan = ptr(level.plan.buffer)
    return s


def _ws_fp(level, widths, backward, dev, opts, ragged=False):
    query = "pn2_mlp_train_ws_bytes_fp_ragged" if ragged else "pn2_mlp_train_ws_bytes_fp"
    return _workspace(query, dev, query + ": unsupported level", level.b, level.n, level.m,
                      level.c2, level.c1, len(widths) - 1, _widths_array(widths), backward, opts)


class _TrainFP(torch.autograd.Function):
    """inputs: level, points2 (b,m,c2), points1 (b,n,c1) or None, lengths ((b,) i32 on the device: a ragged unknown side,
    pn2_mlp_train_*_fp_ragged; else None), then per layer conv.weight, conv.bias (or None), bn.weight, bn.bias. Saved: the inputs,
    the interpolation weights, the parameters, the pre-norm tensors z_l -- and, as on _TrainMLP's ragged rows, the validity mask
    the node owns and lengths, last."""

    @staticmethod
    def forward(ctx, level, points2, points1, lengths, *params):
        n, dev, widths, opts, arr, layers = _forward_stack(level, params)
        ragged = lengths is not None
        out = torch.empty((level.rows, widths[-1]), dtype=torch.float32, device=dev)
        weight = torch.empty((level.b, level.n, 3), dtype=torch.float32, device=dev)
        mask = _ragged_mask(level.rows, dev) if ragged else None
        src = _fp_src(level, points2, points1)
        ws = _ws_fp(level, widths, 0, dev, opts, ragged)
        with on_device(dev):
            if ragged:
                _C.check(_C.lib().pn2_mlp_train_forward_fp_ragged(n, arr, ctypes.byref(src), ptr(lengths), ptr(out), ptr(weight),
                                                                  ptr(mask), ptr(ws), opts, stream_ptr(dev)),
                         "mlp_train_forward_fp_ragged")
            else:
                _C.check(_C.lib().pn2_mlp_train_forward_fp(n, arr, ctypes.byref(src), ptr(out), ptr(weight), ptr(ws), opts,
                                                           stream_ptr(dev)), "mlp_train_forward_fp")
        _count_batch(level.pairs)
        ctx.mark_non_differentiable(weight)
        _save_layers(ctx, level, widths, layers, [points2] + ([points1] if points1 is not None else []) + [weight], out,
                     [mask, lengths] if ragged else ())
        return out, weight

    @staticmethod
    def backward(ctx, grad_out, _unused):
        level, widths = ctx.level, ctx.widths
        n = len(level.pairs)
        head, out, tail, dev, opts, arr, pgrads = _backward_stack(ctx)
        points2, points1, weight = head[0], (head[1] if len(head) == 3 else None), head[-1]
        mask, lengths = tail if tail else (None, None)
        grad_out = f32(grad_out, "grad_out")
        g2 = torch.empty_like(points2) if ctx.needs_input_grad[1] else None
        g1 = torch.empty_like(points1) if points1 is not None and ctx.needs_input_grad[2] else None
        ws = _ws_fp(level, widths, 1, dev, opts, mask is not None)
        src = _fp_src(level, points2, points1)
        det = 1 if is_deterministic() else 0
        with on_device(dev):
            if mask is not None:
                _C.check(_C.lib().pn2_mlp_train_backward_fp_ragged(n, arr, ctypes.byref(src), ptr(lengths), ptr(weight), ptr(out),
                                                                   ptr(grad_out), ptr(g2), ptr(g1), det, ptr(mask), ptr(ws), opts,
                                                                   stream_ptr(dev)), "mlp_train_backward_fp_ragged")
            else:
                _C.check(_C.lib().pn2_mlp_train_backward_fp(n, arr, ctypes.byref(src), ptr(weight), ptr(out), ptr(grad_out), ptr(g2),
                                                            ptr(g1), det, ptr(ws), opts, stream_ptr(dev)), "mlp_train_backward_fp")
        return tuple([None, g2, g1, None] + _param_grads(pgrads))


def fp_level_train(net, points2, points1, idx, dist, return_weight=False, plan=None, lengths=None):
    """Training-mode feature-propagation level with the interpolation inside ONE autograd node (pointnet_fp_module,
    utils/pointnet_util.py:211-226): inverse-distance weights from three_nn's squared distances `dist` (b,n,3) and `idx`
    (b,n,3) i32, three_interpolate of points2 (b,m,c2), concatenation with the skip features points1 (b,n,c1) or None, and the
    layer stack `net` (Conv 1x1 + BatchNorm + ReLU triples, batch statistics). Layer 1 runs once per KNOWN point
    (z_1 = interp(points2 W1a) + points1 W1b); the (b,n,c2+c1) input never exists. -> (b,n,cout), differentiable w.r.t.
    points2, points1 and every parameter (and the weights (b,n,3) with return_weight).
    plan: an IndexPlan of idx (index_plan(idx, m, "interpolate")): the backward inverts nothing.
    lengths: (b,) per-cloud counts of a ragged UNKNOWN side (cloud i's unknown points are rows [0, lengths[i]) of points1 / idx /
    dist; an int32 / int64 tensor or a sequence, ragged_lengths; the known side points2 is dense): the batch statistics, the
    running averages and every gradient are those of the valid rows alone, as on the compacted rows (fp_level_ragged_supported;
    pn2_mlp_train_*_fp_ragged). The padding rows of points1, dist and the output's gradient may hold anything, NaN included; the
    output, the gradient of points1 and the returned weights are exactly zero there. idx must hold indices in [0, m) on the
    padding rows too (three_nn(..., lengths1=) writes (0, 0, 0)). The host never reads the lengths (no synchronisation; a length
    outside 1..n is clamped)."""
    pairs = conv_bn_pairs(net)
    require(pairs is not None, "fp_level_train expects Conv 1x1 + BatchNorm + ReLU triples")
    points2, idx, dist = f32(points2, "points2"), i32(idx, "idx"), f32(dist, "dist")
    require(points2.dim() == 3, "points2 must be (b, m, c2), got %s" % (tuple(points2.shape),))
    b, m, c2 = points2.shape
    require(idx.dim() == 3 and idx.shape[0] == b and idx.shape[2] == 3, "idx must be (b, n, 3), got %s" % (tuple(idx.shape),))
    require(tuple(dist.shape) == tuple(idx.shape), "dist must have idx's shape %s" % (tuple(idx.shape),))
    n = idx.shape[1]
    c1 = 0
    if points1 is not None:
        points1 = f32(points1, "points1")
        require(points1.dim() == 3 and tuple(points1.shape[:2]) == (b, n),
                "points1 must be (b, n, c1) with (b, n) = %s, got %s" % ((b, n), tuple(points1.shape)))
        c1 = points1.shape[2]
        same_device(points2, points1, idx, dist, pairs[0][0].weight)
    else:
        same_device(points2, idx, dist, pairs[0][0].weight)
    require(pairs[0][0].in_channels == c2 + c1, "the first layer expects %d channels, got %d" % (pairs[0][0].in_channels, c2 + c1))
    require(fp_level_supported(net, b, n, m, c2, c1), "unsupported level for the FP training node")
    if lengths is not None:
        lengths = ragged_lengths(lengths, b, points2.device)
        require(fp_level_ragged_supported(net, b, n, m, c2, c1), "unsupported level for the FP training node on ragged rows")
    lv = _FpLevel()
    lv.pairs, lv.rows, lv.b, lv.n, lv.m, lv.c2, lv.c1, lv.idx, lv.dist = pairs, b * n, b, n, m, c2, c1, idx, dist
    lv.plan = None if plan is None else plan.check("interpolate", b, m, 3 * n, points2.device)
    out, weight = _TrainFP.apply(lv, points2, points1, lengths, *_params(pairs))
    out = out.view(b, n, -1)
    return (out, weight) if return_weight else out
