"""Sampling ops -- the Python surface of the reference's tf_ops/sampling/tf_sampling.py
(prob_sample :13, gather_point :29, farthest_point_sample :48), on torch tensors
resident on an MI355X, backed by the HIP kernels in csrc/fps.hip, group.hip and
prob_sample.hip through the C ABI (include/pn2ops.h).

Same names, argument order (hyper-parameters first, tensors last) and return
arity as the reference; differentiability as registered there: GatherPoint has a
gradient w.r.t. its first input (tf_sampling.py:43-47), FarthestPointSample and
ProbSample are NoGradient (:22, :57).
"""
import torch

from . import _C, _tensors
from ._tensors import (det_workspace, f32, i32, is_deterministic, lengths_for, on_device, out_or_empty, packed_args, pair_counts, ptr,
                       ragged_lengths, require, same_device, stream_ptr)


def prob_sample(inp, inpr):
    """inp (b, ncategory) f32 weights, inpr (b, npoints) f32 uniforms -> (b, npoints) i32.

    reference: tf_sampling.py:13-21, op ProbSample tf_sampling.cpp:66-92.
    """
    inp = f32(inp, "inp")
    inpr = f32(inpr, "inpr")
    require(inp.dim() == 2, "ProbSample expects (batch_size,num_choices) inp shape")
    b, n = inp.shape
    require(inpr.dim() == 2 and inpr.shape[0] == b, "ProbSample expects (batch_size,num_points) inpr shape")
    m = inpr.shape[1]
    dev = same_device(inp, inpr)
    out = torch.empty((b, m), dtype=torch.int32, device=dev)
    temp = torch.empty((b, n), dtype=torch.float32, device=dev)   # allocate_temp, tf_sampling.cpp:87
    with on_device(dev):
        _C.check(_C.lib().pn2_prob_sample(b, n, m, ptr(inp), ptr(inpr), ptr(temp), ptr(out), stream_ptr(dev)),
                 "prob_sample")
    return out


def _gather_point_launch(inp, idx, out=None):
    b, n, _ = inp.shape
    m = idx.shape[1]
    dev = inp.device
    out = out_or_empty(out, (b, m, 3), torch.float32, dev)
    with on_device(dev):
        _C.check(_C.lib().pn2_gather_point(b, n, m, ptr(inp), ptr(idx), ptr(out), stream_ptr(dev)),
                 "gather_point")
    return out


class _GatherPoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, idx):
        out = _gather_point_launch(inp, idx)
        ctx.save_for_backward(idx)
        ctx.n = inp.shape[1]
        return out

    @staticmethod
    def backward(ctx, out_g):
        (idx,) = ctx.saved_tensors
        out_g = out_g.contiguous()
        b, m = idx.shape
        dev = out_g.device
        inp_g = torch.empty((b, ctx.n, 3), dtype=torch.float32, device=dev)   # zero-filled by the library
        with on_device(dev):
            if is_deterministic():
                ws = det_workspace(_C.lib(), b, ctx.n, 3, dev)
                _C.check(_C.lib().pn2_gather_point_grad_det(b, ctx.n, m, ptr(out_g), ptr(idx), ptr(inp_g), ptr(ws),
                                                            stream_ptr(dev)), "gather_point_grad")
            else:
                _C.check(_C.lib().pn2_gather_point_grad(b, ctx.n, m, ptr(out_g), ptr(idx), ptr(inp_g),
                                                        stream_ptr(dev)), "gather_point_grad")
        return inp_g, None


def gather_point(inp, idx, out=None):
    """inp (b, ndataset, 3) f32, idx (b, npoints) i32 -> (b, npoints, 3) f32.

    reference: tf_sampling.py:29-37, op GatherPoint tf_sampling.cpp:126-148.
    out: optional preallocated result (inference: no autograd node is built for it).
    """
    inp = f32(inp, "inp")
    idx = i32(idx, "idx")
    require(inp.dim() == 3 and inp.shape[2] == 3, "GatherPoint expects (batch_size,num_points,3) inp shape")
    require(idx.dim() == 2 and idx.shape[0] == inp.shape[0], "GatherPoint expects (batch_size,num_result) idx shape")
    same_device(inp, idx)
    if out is not None:
        require(not (inp.requires_grad and torch.is_grad_enabled()), "out= is for inference: inp requires grad")
        return _gather_point_launch(inp, idx, out)
    return _GatherPoint.apply(inp, idx)


# Tier of the farthest-point-sampling kernels, passed with every call (pn2_farthest_point_sample_variant): 0 = the
# library's size rule, 1 = every point updated every round (csrc/fps_body.h), 2 = kd-grouped slots with exact box pruning
# (csrc/fps_pruned_body.h; 2049..8192 rank slots only), 3 = the same slots with several samples per arg-max exchange
# (csrc/fps_batch_body.h, round 6; same sizes). Results never depend on it: the tests force every tier.
FPS_AUTO, FPS_FULL, FPS_PRUNED, FPS_BATCH = 0, 1, 2, 3
_FPS_VARIANT = [FPS_AUTO]


def set_fps_variant(variant=FPS_AUTO):
    """Applies to calls with `lengths=` / `npoints=` (ragged batches) too: every tier runs on each cloud's slice and gives the
    slice rule's result. With FPS_AUTO those calls go through pn2_farthest_point_sample_ragged / _ragged_counts, which apply
    the library's size rule to the padded n and npoint; a forced tier goes through pn2_farthest_point_sample_ragged_variant
    (ValueError where the padded n is outside the tier's rank-slot envelope, as for dense input). One preparation of the
    counts serves all three (_fps_ragged)."""
    require(int(variant) in (FPS_AUTO, FPS_FULL, FPS_PRUNED, FPS_BATCH), "fps variant must be 0 (auto), 1 (full), 2 (pruned) or 3 (batched)")
    _FPS_VARIANT[0] = int(variant)


# Large dense clouds (16384 < n <= 1048576): the cell-sorted, box-pruned tier of csrc/fps_large.hip instead of the global-memory
# kernel. None = where the library's measured size rule says it pays (pn2_fps_large_pays), True = wherever it is supported,
# False = never. Dense input (no lengths / npoints) -- ragged batches of this size only under set_fps_ragged_large(True) below,
# where the same three modes choose the kernel --, and only while no tier is forced with set_fps_variant. Results never depend on it.
_FPS_LARGE = [None]
FPS_REG_MAX_POINTS = 16384              # up to here the register-resident tiers (pn2_fps_temp_floats is 0)


def set_fps_large(mode=None):
    require(mode is None or isinstance(mode, bool), "fps large mode must be None (the size rule), True or False")
    _FPS_LARGE[0] = mode


def _fps_large_takes(lib, b, n, m):
    if _FPS_VARIANT[0] or _FPS_LARGE[0] is False or b <= 0 or n <= FPS_REG_MAX_POINTS:   # the register tiers: not even a query
        return False
    return bool(lib.pn2_fps_large_supported(n, m) if _FPS_LARGE[0] else lib.pn2_fps_large_pays(n, m))


def _fps_large(lib, b, n, m, inp, out, new_xyz, op):
    dev = inp.device
    ws = torch.empty((lib.pn2_fps_large_ws_bytes(b, n),), dtype=torch.uint8, device=dev)    # per call, as temp is
    with on_device(dev):
        _C.check(lib.pn2_farthest_point_sample_large(b, n, m, ptr(inp), ptr(ws), ptr(out), ptr(new_xyz), stream_ptr(dev)), op)


# ---- input that is already in farthest-point order ------------------------------------------------------------------------
# The second and later levels of every network sample from the previous level's samples (pointnet2_sem_seg.py:28-31): the
# first m of them are, up to exact ties and exhausted clouds, selected as 0 .. m-1. new_xyz tensors that come out of a
# farthest-point sampling here carry a HINT (a Python attribute); an operator that receives a hinted tensor calls
# pn2_farthest_point_sample_ordered, which checks the belief on the device and runs the chain only where it fails -- the
# hint can cost time, never a result (tests/test_fps_ordered_gpu.py feeds it wrong hints). set_ordered_hints(False) ignores
# the hints.
_ORDERED = [True]
_ORDERED_WS = {}


def set_ordered_hints(flag=True):
    _ORDERED[0] = bool(flag)


def mark_fps_ordered(t):
    """Tag a (b, m, 3) tensor as being in farthest-point order (the output of a farthest-point sampling)."""
    try:
        t._pn2_fps_ordered = True
    except Exception:        # noqa: BLE001 -- a tensor subclass without attributes: no hint, nothing lost
        pass
    return t


def ordered_worthwhile(t, m):
    """Is the ordered entry point worth calling for m samples out of `t`? (a chain long enough to pay for the check + one more
    launch: 128 <= m <= min(n, 1024), n <= 2048)"""
    return _ORDERED[0] and t.dim() == 3 and 128 <= int(m) <= min(t.shape[1], 1024) and t.shape[1] <= 2048 and t.shape[0] > 0


def ordered_hint(t, m):
    """Does `t` carry the farthest-point-order tag (an attribute of the tensor OBJECT a sampling operator returned: read it
    before any dtype / layout conversion or detach(), which make new objects), and is the short cut worthwhile for m samples?"""
    return bool(getattr(t, "_pn2_fps_ordered", False)) and ordered_worthwhile(t, m)


def ordered_workspace(lib, dev, stream, b):
    """Flag words of pn2_farthest_point_sample_ordered, one buffer per (device, stream, batch): zeroed once, every call leaves
    it zeroed. Under graph capture a fresh zeroed buffer belongs to the graph."""
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros((b,), dtype=torch.int32, device=dev)
    key = (dev.index, stream, b)
    ws = _ORDERED_WS.get(key)
    if ws is None:
        if len(_ORDERED_WS) > 64:
            _ORDERED_WS.clear()              # buffers still referenced by enqueued launches stay alive with their tensors' storage
        ws = torch.zeros((max(1, lib.pn2_fps_ordered_ws_bytes(b) // 4),), dtype=torch.int32, device=dev)
        _ORDERED_WS[key] = ws
    return ws


FPS_RAGGED_MAX_POINTS = 16384           # the register tiers' envelope (pn2_farthest_point_sample_ragged)
FPS_RAGGED_LARGE_MAX_POINTS = 1048576   # the large-cloud entry's (pn2_farthest_point_sample_large_ragged)

# Ragged batches beyond 16384 padded points: opt-in. Off (the default), `lengths=` / `npoints=` stop at FPS_RAGGED_MAX_POINTS with
# the ValueError below. On, a padded n of 16385 .. 1048576 goes through pn2_farthest_point_sample_large_ragged_ex with a workspace
# allocated per call; set_fps_large chooses its kernel (None = pn2_fps_large_pays on the padded n and npoint, True = the
# cell-sorted tier, False = the global-memory kernel with counts). A tier forced with set_fps_variant keeps the 16384 limit.
# The switch covers BOTH variable-size layouts: with `offsets=`, max_points of 16385 .. 1048576 goes through
# pn2_farthest_point_sample_large_packed_ex (_fps_packed below) with the same three kernel modes and the library's short-cloud rule.
_FPS_RAGGED_LARGE = [False]


def set_fps_ragged_large(flag=False):
    """Variable-size batches beyond 16384 points per cloud, in both layouts: padded (`lengths=` / `npoints=`, the padded n) and
    packed (`offsets=` / `max_points=`). Off, both stop at 16384 with a ValueError; on, both reach 1048576."""
    require(isinstance(flag, bool), "fps ragged large flag must be True or False")
    _FPS_RAGGED_LARGE[0] = flag


def _fps_ragged(m, inp, lengths, out, new_xyz, op, npoints=None):
    """Both ragged forms, the counts prepared once: without lengths every cloud holds all n points (an array of full counts made on
    the device), without npoints every cloud yields m samples (NULL). A tier forced with set_fps_variant applies up to 16384
    padded points."""
    b, n, _ = inp.shape
    large = _FPS_RAGGED_LARGE[0] and not _FPS_VARIANT[0] and n > FPS_RAGGED_MAX_POINTS
    limit = FPS_RAGGED_LARGE_MAX_POINTS if large else FPS_RAGGED_MAX_POINTS
    require(n <= limit, "%s with lengths supports at most %d points per (padded) cloud, got %d" % (op, limit, n))
    dev = inp.device
    _, lens, cnts, _, _ = pair_counts(lengths, npoints, b, n, m, dev, ("lengths", "npoints"))
    lib = _C.lib()
    if not large:
        with on_device(dev):
            tail = (ptr(out), ptr(new_xyz), stream_ptr(dev))
            if _FPS_VARIANT[0]:             # a forced tier: one entry for both forms
                rc = lib.pn2_farthest_point_sample_ragged_variant(_FPS_VARIANT[0], b, n, m, ptr(inp), ptr(lens), ptr(cnts), *tail)
            elif cnts is None:              # the two entries that are its PN2_FPS_AUTO case (the modules' call census pins them)
                rc = lib.pn2_farthest_point_sample_ragged(b, n, m, ptr(inp), ptr(lens), *tail)
            else:
                rc = lib.pn2_farthest_point_sample_ragged_counts(b, n, m, ptr(inp), ptr(lens), ptr(cnts), *tail)
            _C.check(rc, op)
        return
    kernel = {None: 0, True: 2, False: 1}[_FPS_LARGE[0]]
    ws = torch.empty((lib.pn2_fps_large_ws_bytes(b, n),), dtype=torch.uint8, device=dev)    # per call, on the padded n
    with on_device(dev):
        _C.check(lib.pn2_farthest_point_sample_large_ragged_ex(kernel, 256, b, n, m, ptr(inp), ptr(lens), ptr(cnts), ptr(ws), ptr(out),
                                                               ptr(new_xyz), stream_ptr(dev)), op)


def _fps_packed(npoint, inp, offsets, max_points, lengths, npoints, global_idx, out, want_xyz, op):
    """The packed form of both sampling operators (pn2_farthest_point_sample_packed; with npoints, under set_packed_pairs(True),
    pn2_farthest_point_sample_packed_counts): inp (total, 3), offsets (b + 1,) on the
    device, max_points a host int. -> idx (b, npoint), new_xyz (b, npoint, 3) or None. A tier forced with set_fps_variant
    applies; nothing synchronises. max_points of 16385 .. 1048576 under set_fps_ragged_large(True):
    pn2_farthest_point_sample_large_packed_ex with a workspace of 20 bytes per row of the flat array, allocated per call."""
    require(npoints is None or _tensors.packed_pairs(), "%s: per-cloud sample counts (npoints=) are not offered with offsets" % op)
    offs, b, total, nmax = packed_args(offsets, max_points, lengths, inp, op)           # (before anything else, like lengths_for)
    cnts = None
    if npoints is not None:                                # set_packed_pairs(True): pn2_farthest_point_sample_packed_counts
        cnts = ragged_lengths(npoints, b, inp.device, "npoints")               # (shape and dtype complaints before the device's)
        require(nmax <= FPS_RAGGED_MAX_POINTS, "%s: npoints with offsets supports at most %d points per cloud, got max_points = %d"
                % (op, FPS_RAGGED_MAX_POINTS, nmax))
    large = _FPS_RAGGED_LARGE[0] and not _FPS_VARIANT[0] and nmax > FPS_RAGGED_MAX_POINTS
    limit = FPS_RAGGED_LARGE_MAX_POINTS if large else FPS_RAGGED_MAX_POINTS
    require(nmax <= limit, "%s with offsets supports at most %d points per cloud, got max_points = %d" % (op, limit, nmax))
    inp = f32(inp.detach(), "inp")
    m = int(npoint)
    dev = inp.device
    out = out_or_empty(out, (b, m), torch.int32, dev)
    new_xyz = torch.empty((b, m, 3), dtype=torch.float32, device=dev) if want_xyz else None
    if large:
        lib = _C.lib()
        kernel = {None: 0, True: 2, False: 1}[_FPS_LARGE[0]]
        ws = torch.empty((lib.pn2_fps_large_packed_ws_bytes(total),), dtype=torch.uint8, device=dev)    # per call, on the flat array
        with on_device(dev):
            _C.check(lib.pn2_farthest_point_sample_large_packed_ex(kernel, 256, -1, b, total, nmax, m, ptr(inp), ptr(offs),
                                                                   1 if global_idx else 0, ptr(ws), ptr(out), ptr(new_xyz),
                                                                   stream_ptr(dev)), op)
        return out, new_xyz
    if cnts is not None:
        with on_device(dev):
            _C.check(_C.lib().pn2_farthest_point_sample_packed_counts(_FPS_VARIANT[0], b, total, nmax, m, ptr(inp), ptr(offs), ptr(cnts),
                                                                      1 if global_idx else 0, ptr(out), ptr(new_xyz), stream_ptr(dev)), op)
        return out, new_xyz
    with on_device(dev):
        _C.check(_C.lib().pn2_farthest_point_sample_packed(_FPS_VARIANT[0], b, total, nmax, m, ptr(inp), ptr(offs), 1 if global_idx else 0,
                                                           ptr(out), ptr(new_xyz), stream_ptr(dev)), op)
    return out, new_xyz


def _fps(npoint, inp, op, want_xyz, out=None, ordered=None, lengths=None, npoints=None, offsets=None, max_points=None, global_idx=False):
    """The one body of farthest_point_sample and farthest_point_sample_gather -> idx (b, npoint), new_xyz (b, npoint, 3) or None.
    op: the operator's name in messages; want_xyz: gather the samples too; out: optional preallocated idx; ordered: None = follow
    inp's hint, True / False = force / forbid the checked short cut."""
    require(int(npoint) > 0, "FarthestPointSample expects positive npoint")
    if offsets is not None:
        out, new_xyz = _fps_packed(npoint, inp, offsets, max_points, lengths, npoints, global_idx, out, want_xyz, op)
        return out, (mark_fps_ordered(new_xyz) if want_xyz and npoints is None else new_xyz)   # fill rows break the farthest-point order
    if lengths is not None:
        lengths = lengths_for(lengths, inp)
    if npoints is not None:
        npoints = lengths_for(npoints, inp, "npoints")
    if ordered is None:                                    # (before detach(): the hint is an attribute of the caller's tensor object)
        ordered = isinstance(inp, torch.Tensor) and ordered_hint(inp, npoint)      # the previous level's samples: checked short cut
    inp = f32(inp.detach() if isinstance(inp, torch.Tensor) else inp, "inp")
    require(inp.dim() == 3 and inp.shape[2] == 3, "FarthestPointSample expects (batch_size,num_points,3) inp shape")
    b, n, _ = inp.shape
    require(n > 0 or b == 0, "FarthestPointSample expects at least one point per cloud")
    m = int(npoint)
    dev = inp.device
    out = out_or_empty(out, (b, m), torch.int32, dev)
    new_xyz = torch.empty((b, m, 3), dtype=torch.float32, device=dev) if want_xyz else None
    if lengths is not None or npoints is not None:
        _fps_ragged(m, inp, lengths, out, new_xyz, op, npoints)
        return out, (mark_fps_ordered(new_xyz) if want_xyz and npoints is None else new_xyz)   # fill rows break the farthest-point order
    lib = _C.lib()
    if _fps_large_takes(lib, b, n, m):
        _fps_large(lib, b, n, m, inp, out, new_xyz, op)
        return out, (mark_fps_ordered(new_xyz) if want_xyz else None)
    tf = lib.pn2_fps_temp_floats(b, n)
    temp = torch.empty((tf,), dtype=torch.float32, device=dev) if tf > 0 else None   # allocate_temp, tf_sampling.cpp:115
    with on_device(dev):
        if ordered and b > 0 and n <= 16384:
            st = stream_ptr(dev)
            ws = ordered_workspace(lib, dev, st, b)
            _C.check(lib.pn2_farthest_point_sample_ordered(b, n, m, ptr(inp), ptr(out), ptr(new_xyz), ptr(ws), st),
                     "farthest_point_sample_ordered")
        elif _FPS_VARIANT[0]:
            _C.check(lib.pn2_farthest_point_sample_variant(_FPS_VARIANT[0], b, n, m, ptr(inp), ptr(temp), ptr(out), ptr(new_xyz),
                                                           stream_ptr(dev)), op)
        elif want_xyz:
            _C.check(lib.pn2_farthest_point_sample_gather(b, n, m, ptr(inp), ptr(temp), ptr(out), ptr(new_xyz), stream_ptr(dev)), op)
        else:
            _C.check(lib.pn2_farthest_point_sample(b, n, m, ptr(inp), ptr(temp), ptr(out), stream_ptr(dev)), op)
    return out, (mark_fps_ordered(new_xyz) if want_xyz else None)


def farthest_point_sample_gather(npoint, inp, ordered=None, lengths=None, npoints=None, offsets=None, max_points=None, global_idx=False):
    """Fused farthest_point_sample + gather_point (pointnet_util.py:40 in one launch).
    offsets / max_points: a PACKED batch -- inp is one flat (total, 3) array, cloud i is inp[offsets[i] : offsets[i + 1]]
    (offsets (b + 1,) on the device), max_points a host int that bounds every cloud's count (it takes the padded n's place in
    the tier rule; required, so nothing synchronises). Each cloud's result is the dense operator's on its slice; idx and new_xyz
    stay dense (b, npoint[, 3]). global_idx: indices are rows of the flat array (offsets[i] + k) instead of cloud-local.
    Not to be mixed with lengths (ValueError). npoints with offsets is offered under set_packed_pairs(True), up to 16384 points per
    cloud (pn2_farthest_point_sample_packed_counts): rows from npoints[i] on repeat sample 0, idx 0 -- offsets[i] under global_idx.
    lengths: (b,) per-cloud point counts of a ragged batch (cloud i is inp[i, :lengths[i]]): each cloud's result is the
    dense operator's on its slice, rows beyond the length are never read. None = every cloud holds all n points.
    npoints: (b,) per-cloud sample counts (cloud i yields m_i = npoints[i] <= npoint samples; clamped into 1..npoint on the
    device, check_lengths(npoints, npoint) validates): rows below m_i are the first m_i samples of the slice, rows from m_i on
    repeat sample 0 (idx 0, the cloud's first point). Without lengths every cloud holds all n points.

    npoint int, inp (b, ndataset, 3) f32 -> idx (b, npoint) i32, new_xyz (b, npoint, 3) f32
    with new_xyz == gather_point(inp, idx) bit for bit. No reference counterpart
    (SURVEY.md 8f1); not differentiable -- use gather_point when inp needs a gradient.
    ordered: None = follow inp's hint (above), True / False = force / forbid the checked short cut for input in
    farthest-point order (same results either way).
    """
    return _fps(npoint, inp, "farthest_point_sample_gather", True, None, ordered, lengths, npoints, offsets, max_points, global_idx)


def farthest_point_sample(npoint, inp, out=None, lengths=None, npoints=None, offsets=None, max_points=None, global_idx=False):
    """npoint int, inp (b, ndataset, 3) f32 -> (b, npoint) i32, first index 0.
    lengths: (b,) per-cloud point counts of a ragged batch, see farthest_point_sample_gather.
    npoints: (b,) per-cloud sample counts, see farthest_point_sample_gather.
    offsets / max_points / global_idx: a packed batch, inp (total, 3), see farthest_point_sample_gather.

    reference: tf_sampling.py:48-56, op FarthestPointSample tf_sampling.cpp:95-123,
    kernel tf_sampling_g.cu:105-170 (tie rule: smallest (k mod 512, k)).
    out: optional preallocated (b, npoint) i32 result.
    """
    return _fps(npoint, inp, "farthest_point_sample", False, out, None, lengths, npoints, offsets, max_points, global_idx)[0]
