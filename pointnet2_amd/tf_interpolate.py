"""Interpolation ops -- the Python surface of the reference's
tf_ops/3d_interpolation/tf_interpolate.py (three_nn :8, three_interpolate :19) on
torch tensors resident on an MI355X, backed by csrc/interpolate.hip through the
C ABI (include/pn2ops.h). The reference runs these ops on the CPU only
(tf_interpolate.cpp:187,222,262).

Differentiability as registered in the reference: ThreeInterpolate has a
gradient w.r.t. `points` only (tf_interpolate.py:29-34); ThreeNN is NoGradient (:18).
"""
import torch

from . import _C
from ._tensors import (out_or_empty, f32, i32, is_deterministic, lengths_for, on_device, packed_args, pair_counts, ptr, ragged_lengths, require,
                       same_device, scatter_grad, seg_workspace, stream_ptr)


# three_nn kernel choice of the packed calls (pn2_three_nn_packed's variant): 0 the library's, 1 the sweep, 2 the cell list.
# Results never depend on it; the tests force both.
_NN_PACKED_VARIANT = [0]


def three_nn(xyz1, xyz2, out=None, lengths1=None, lengths2=None, offsets1=None, max_points1=None, global_idx=False):
    """xyz1 (b, n, 3) unknown, xyz2 (b, m, 3) known -> dist (b, n, 3) f32 SQUARED
    distances ascending, idx (b, n, 3) i32. out: optional preallocated (dist, idx).
    lengths1: (b,) per-cloud counts of a ragged UNKNOWN side (cloud i is xyz1[i, :lengths1[i]]; the known side is dense):
    valid rows are the dense operator's, rows beyond the length are never read and come back as idx (0,0,0), dist (0,0,0).
    lengths2: (b,) per-cloud counts of a ragged KNOWN side (cloud i's known points are xyz2[i, :lengths2[i]]; rows beyond are
    never read): every row is the dense operator's on the slice pair, so idx < lengths2[i], and fewer than three known points
    leave the dense operator's +inf / index 0 entries. With one of lengths1 / lengths2 given the other side is dense.
    offsets1 / max_points1: a PACKED unknown side -- xyz1 is one flat (total, 3) array, cloud i is
    xyz1[offsets1[i] : offsets1[i + 1]] (offsets1 (b + 1,) on the device; max_points1 a host int bounding every cloud's count,
    required); xyz2 (b, m, 3) stays dense (lengths2 allowed). dist, idx are (total, 3), row offsets1[i] + j = point j of cloud i,
    the dense operator's on the slice; no padding rows. global_idx: a known-point index is written as i m + k, a row of
    xyz2.view(b m, 3). Not to be mixed with lengths1 (ValueError).

    reference: tf_interpolate.py:8-17, op ThreeNN tf_interpolate.cpp:157-187,
    loop threenn_cpu :60-103.
    """
    packed = offsets1 is not None
    if packed:
        require(isinstance(xyz2, torch.Tensor) and xyz2.dim() == 3 and xyz2.shape[2] == 3, "ThreeNN expects (b,m,3) xyz2 shape")
        b, m, _ = xyz2.shape
        offs, b, total, nmax = packed_args(offsets1, max_points1, lengths1, xyz1, "three_nn", "offsets1", "max_points1", b=b)
    else:
        if lengths1 is not None:
            lengths1 = lengths_for(lengths1, xyz1, "lengths1")
        if lengths2 is not None:
            lengths2 = lengths_for(lengths2, xyz1, "lengths2")
    xyz1 = f32(xyz1, "xyz1")
    xyz2 = f32(xyz2, "xyz2")
    if packed:
        dev = same_device(xyz1, xyz2)
        lens2 = ragged_lengths(lengths_for(lengths2, xyz2, "lengths2"), b, dev, "lengths2") if lengths2 is not None else None
        entry, behind1, behind2 = "_packed", (ptr(offs),), (ptr(lens2),)        # (a NULL lens2: a dense known side)
        extents, rows = (b, total, nmax, m), (total, 3)
        flag, variant = (1 if global_idx else 0,), (_NN_PACKED_VARIANT[0],)     # the words in front of dist and behind idx
    else:
        shape1, shape2 = xyz1.shape, xyz2.shape
        require(len(shape1) == 3 and shape1[2] == 3, "ThreeNN expects (b,n,3) xyz1 shape")
        require(len(shape2) == 3 and shape2[2] == 3 and shape2[0] == shape1[0], "ThreeNN expects (b,m,3) xyz2 shape")
        dev = same_device(xyz1, xyz2)
        b, n, m = shape1[0], shape1[1], shape2[1]
        entry, _lens1, _lens2, behind1, behind2 = pair_counts(lengths1, lengths2, b, n, m, dev)
        extents, rows = (b, n, m), (b, n, 3)
        flag, variant = (), ((0,) if entry else ())                            # (the counted entries' kernel choice: the library's)
    dist = out_or_empty(out[0] if out is not None else None, rows, torch.float32, dev, "out[0]")
    idx = out_or_empty(out[1] if out is not None else None, rows, torch.int32, dev, "out[1]")
    with on_device(dev):
        rc = getattr(_C.lib(), "pn2_three_nn" + entry)(*extents, ptr(xyz1), *behind1, ptr(xyz2), *behind2, *flag, ptr(dist), ptr(idx),
                                                       *variant, stream_ptr(dev))
    if rc:
        _C.check(rc, "three_nn")
    return dist, idx


def _three_interpolate_launch(points, idx, weight, out=None):
    b, m, c = points.shape
    n = idx.shape[1]
    dev = points.device
    out = out_or_empty(out, (b, n, c), torch.float32, dev)
    with on_device(dev):
        _C.check(_C.lib().pn2_three_interpolate(b, m, c, n, ptr(points), ptr(idx), ptr(weight), ptr(out),
                                                stream_ptr(dev)), "three_interpolate")
    return out


class _ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx, weight, plan=None):
        out = _three_interpolate_launch(points, idx, weight)
        ctx.save_for_backward(idx, weight)
        ctx.shape = tuple(points.shape)
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        b, m, c = ctx.shape
        n = idx.shape[1]
        dev = grad_out.device
        grad_points = torch.empty((b, m, c), dtype=torch.float32, device=dev)   # zero-filled by the library
        with on_device(dev):
            _C.check(scatter_grad(_C.lib(), "three_interpolate", (b, n, c, m, ptr(grad_out)), idx, ctx.plan,
                                  (ptr(weight), ptr(grad_points)), b, m, c, 3 * n, dev), "three_interpolate_grad")
        return grad_points, None, None, None


def three_interpolate(points, idx, weight, out=None, plan=None):
    """points (b, m, c) f32 known features, idx (b, n, 3) i32, weight (b, n, 3) f32
    -> (b, n, c) f32. out: optional preallocated result (inference: no autograd node is built for it).
    plan: an IndexPlan of this idx (index_plan(idx, m, "interpolate")): the backward reduces from it and inverts nothing
    (ignored where the gradient is the atomic scatter: use_segmented_grad).

    reference: tf_interpolate.py:19-28, op ThreeInterpolate tf_interpolate.cpp:191-222.
    """
    points = f32(points, "points")
    idx = i32(idx, "idx")
    weight = f32(weight, "weight")
    require(points.dim() == 3, "ThreeInterpolate expects (b,m,c) points shape")
    b = points.shape[0]
    require(idx.dim() == 3 and idx.shape[0] == b and idx.shape[2] == 3, "ThreeInterpolate expects (b,n,3) idx shape")
    require(weight.dim() == 3 and weight.shape == idx.shape, "ThreeInterpolate expects (b,n,3) weight shape")
    dev = same_device(points, idx, weight)
    if plan is not None:
        plan.check("interpolate", b, points.shape[1], 3 * idx.shape[1], dev)
    if out is not None:
        require(not (points.requires_grad and torch.is_grad_enabled()), "out= is for inference: points requires grad")
        return _three_interpolate_launch(points, idx, weight, out)
    return _ThreeInterpolate.apply(points, idx, weight, plan)


class _FPInterpConcat(torch.autograd.Function):
    """inputs: points2 (b,m,c2), points1 (b,n,c1) or None, idx (b,n,3) i32, dist (b,n,3) f32 (three_nn's), pitch."""

    @staticmethod
    def forward(ctx, points2, points1, idx, dist, pitch, plan=None):
        b, m, c2 = points2.shape
        n = idx.shape[1]
        c1 = points1.shape[2] if points1 is not None else 0
        dev = points2.device
        out = torch.empty((b, n, pitch), dtype=torch.float32, device=dev)
        weight = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
        with on_device(dev):
            _C.check(_C.lib().pn2_fp_interp_concat(b, n, m, c2, c1, pitch, ptr(points2), ptr(points1), ptr(idx), ptr(dist),
                                                   ptr(out), ptr(weight), stream_ptr(dev)), "fp_interp_concat")
        ctx.save_for_backward(idx, weight)
        ctx.dims = (b, n, m, c2, c1, pitch)
        ctx.plan = plan
        ctx.mark_non_differentiable(weight)
        return out, weight

    @staticmethod
    def backward(ctx, grad_x, _unused):
        idx, weight = ctx.saved_tensors
        b, n, m, c2, c1, pitch = ctx.dims
        grad_x = f32(grad_x, "grad_x")
        dev = grad_x.device
        need2, need1 = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and c1 > 0
        g2 = torch.empty((b, m, c2), dtype=torch.float32, device=dev)                 # zero-filled by the library
        g1 = torch.empty((b, n, c1), dtype=torch.float32, device=dev) if need1 else None
        scratch = torch.empty((b, n, c2), dtype=torch.float32, device=dev)
        with on_device(dev):
            if ctx.plan is not None:                                    # idx was inverted where it was born (index_plan.py)
                _C.check(_C.lib().pn2_fp_interp_concat_grad_planned(b, n, m, c2, c1, pitch, ptr(grad_x), ptr(ctx.plan.buffer),
                                                                    ptr(weight), ptr(g2), ptr(g1), ptr(scratch),
                                                                    1 if is_deterministic() else 0, stream_ptr(dev)),
                         "fp_interp_concat_grad")
            else:
                ws = seg_workspace(_C.lib(), b, m, 3 * n, dev)
                _C.check(_C.lib().pn2_fp_interp_concat_grad(b, n, m, c2, c1, pitch, ptr(grad_x), ptr(idx), ptr(weight), ptr(g2), ptr(g1),
                                                            ptr(scratch), ptr(ws), 1 if is_deterministic() else 0, stream_ptr(dev)),
                         "fp_interp_concat_grad")
        return (g2 if need2 else None), g1, None, None, None, None


def fp_interp_concat(points2, points1, idx, dist, pad_to=4, plan=None):
    """The input rows of pointnet_fp_module's layer stack (pointnet_util.py:211-219) in ONE launch: inverse-distance weights
    from three_nn's squared distances, three_interpolate(points2, idx, weight), concat with the skip features points1 (or
    None), zero columns up to a multiple of `pad_to`. -> x (b, n, pitch), weight (b, n, 3). Same formulas as the operators;
    differentiable w.r.t. points2 and points1 (one launch for the split + the segmented scatter of three_interpolate's
    gradient). plan: an IndexPlan of idx (index_plan(idx, m, "interpolate")): the backward inverts nothing."""
    points2 = f32(points2, "points2")
    idx = i32(idx, "idx")
    dist = f32(dist, "dist")
    require(points2.dim() == 3, "ThreeInterpolate expects (b,m,c) points shape")
    b = points2.shape[0]
    require(idx.dim() == 3 and idx.shape[0] == b and idx.shape[2] == 3, "ThreeInterpolate expects (b,n,3) idx shape")
    require(dist.shape == idx.shape, "ThreeInterpolate expects (b,n,3) weight shape")
    c = points2.shape[2]
    if points1 is not None:
        points1 = f32(points1, "points1")
        require(points1.dim() == 3 and tuple(points1.shape[:2]) == (b, idx.shape[1]), "points1 must be (b, n, c1)")
        c += points1.shape[2]
        same_device(points2, points1, idx, dist)
    else:
        same_device(points2, idx, dist)
    pitch = (c + pad_to - 1) // pad_to * pad_to
    if plan is not None:
        plan.check("interpolate", b, points2.shape[1], 3 * idx.shape[1], points2.device)
    return _FPInterpConcat.apply(points2, points1, idx, dist, pitch, plan)
