"""Index plans: the inverse of one index tensor, built once where the tensor is born and read by every gradient that scatters
through it (include/pn2ops.h "index plans", csrc/seg_grad.hip).

The gradients of group_point and three_interpolate are segmented reductions: a counting sort of the references by target row,
then one lane group (or workgroup) per row. The sort depends on idx alone. index_plan() runs it as a call of its own -- kernels
only, so it may be captured, and it may run on another stream than the gradients (geometry.GeometryAhead(..., plans=True)
builds it right behind the launch that wrote idx) -- and the operators / training nodes that are handed the plan launch no
inversion in their backward. A plan is valid for exactly the idx contents it was built from: rebuild it (IndexPlan.rebuild)
when idx is rewritten in place.
"""
import torch

from . import _C
from ._tensors import i32, is_deterministic, on_device, ptr, require, stream_ptr

KINDS = ("group", "interpolate")


class IndexPlan:
    """buffer: the plan's device memory (int32; position-independent, so copy_() of it is a valid plan of the same idx);
    b clouds, `rows` target rows per cloud, `entries` references per cloud (group: m * nsample, interpolate: 3 * n);
    kind "group" (idx (b, m, nsample) of group_point) or "interpolate" (idx (b, n, 3) of three_interpolate);
    sorted: built with the sorting inversion -- such a plan serves both the reproducible and the default mode, an unsorted one
    makes the reproducible mode sum every row in fixed point."""

    __slots__ = ("buffer", "b", "rows", "entries", "kind", "sorted")

    def __init__(self, buffer, b, rows, entries, kind, sorted):
        self.buffer, self.b, self.rows, self.entries, self.kind, self.sorted = buffer, b, rows, entries, kind, bool(sorted)

    def check(self, kind, b, rows, entries, device):
        """Raise ValueError unless this plan describes an index tensor of that kind and shape on that device."""
        if self.kind != kind:
            raise ValueError("index plan of kind %r given where %r is needed" % (self.kind, kind))
        if (self.b, self.rows, self.entries) != (b, rows, entries):
            raise ValueError("index plan for (b, rows, entries) = %s given where %s is needed"
                             % ((self.b, self.rows, self.entries), (b, rows, entries)))
        if self.buffer.device != device:
            raise ValueError("index plan on %s given for tensors on %s" % (self.buffer.device, device))
        return self

    def rebuild(self, idx, sorted=None):
        """Build again, into the same memory, from an idx of the same shape (on the current stream)."""
        return index_plan(idx, self.rows, self.kind, self.sorted if sorted is None else sorted, out=self)


def plan_buffer(b, rows, entries, device):
    nbytes = _C.lib().pn2_seg_plan_bytes(b, rows, entries)
    return torch.empty(((nbytes + 3) // 4,), dtype=torch.int32, device=device)


def index_plan(idx, rows, kind, sorted=None, out=None):
    """idx: (b, m, nsample) i32 for kind "group" (rows = the number of points idx refers to), (b, n, 3) i32 for kind
    "interpolate" (rows = the number of known points). sorted: None = is_deterministic() now. out: an IndexPlan of the same
    shape and kind to overwrite. -> IndexPlan, built on the current stream."""
    require(kind in KINDS, "kind must be 'group' or 'interpolate', got %r" % (kind,))
    idx = i32(idx, "idx")
    require(idx.dim() == 3 and (kind == "group" or idx.shape[2] == 3),
            "idx must be (b, m, nsample)" if kind == "group" else "idx must be (b, n, 3)")
    rows = int(rows)
    require(rows > 0, "rows must be positive")
    b = idx.shape[0]
    entries = idx.shape[1] * idx.shape[2]
    dev = idx.device
    sorted = is_deterministic() if sorted is None else bool(sorted)
    if out is None:
        plan = IndexPlan(plan_buffer(b, rows, entries, dev), b, rows, entries, kind, sorted)
    else:
        plan = out.check(kind, b, rows, entries, dev)
        plan.sorted = sorted
    lib = _C.lib()
    with on_device(dev):
        if kind == "group":
            _C.check(lib.pn2_group_point_plan(b, rows, idx.shape[1], idx.shape[2], ptr(idx), 1 if sorted else 0, ptr(plan.buffer),
                                              stream_ptr(dev)), "group_point_plan")
        else:
            _C.check(lib.pn2_three_interpolate_plan(b, idx.shape[1], rows, ptr(idx), 1 if sorted else 0, ptr(plan.buffer),
                                                    stream_ptr(dev)), "three_interpolate_plan")
    return plan
