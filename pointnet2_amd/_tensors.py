"""Tensor plumbing shared by the op wrappers: validation + raw pointers.

PyTorch is used for device memory and streams only; the compute is in
libpn2ops.so. The checks mirror the OP_REQUIRES validation that the reference
performs in OpKernel::Compute (SURVEY.md section 8b "Error convention"), with
the reference's message text.
"""
import torch


def require(cond, msg):
    if not cond:
        raise ValueError(msg)


def _checked(t, name, dtype, dtype_name):
    # fast path first: the messages below cost more to format than the checks do (every operator call pays them)
    if isinstance(t, torch.Tensor) and t.dtype is dtype and t.is_cuda:
        return t if t.is_contiguous() else t.contiguous()
    require(isinstance(t, torch.Tensor), "%s must be a torch.Tensor" % name)
    require(t.dtype == dtype, "%s must be %s, got %s" % (name, dtype_name, t.dtype))
    require(t.is_cuda, "%s must live on a ROCm device (got %s); there is no CPU path" % (name, t.device))
    return t.contiguous()


def f32(t, name):
    return _checked(t, name, torch.float32, "float32")


def i32(t, name):
    return _checked(t, name, torch.int32, "int32")


def out_or_empty(out, shape, dtype, dev, name="out"):
    """A caller-provided output buffer (the `out=` option of the operators: no allocation on the call path,
    ~1.7 us per tensor saved) or a fresh one. A provided buffer must match exactly; nothing is copied."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (isinstance(out, torch.Tensor) and out.dtype is dtype and tuple(out.shape) == tuple(shape) and out.device == dev
            and out.is_contiguous()):
        raise ValueError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), dev))
    return out


def same_device(*ts):
    dev = ts[0].device
    for t in ts[1:]:
        if t.device != dev:
            raise ValueError("all tensors must be on the same device (%s vs %s)" % (dev, t.device))
    return dev


def ptr(t):
    return t.data_ptr() if t is not None else None


def _lengths_tensor(lengths, name):
    """An int32 / int64 tensor, or a sequence of ints -> an integer tensor (wherever it lives); anything else: ValueError."""
    if not isinstance(lengths, torch.Tensor):
        try:
            lengths = torch.as_tensor(lengths)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("%s must be an int32 / int64 tensor or a sequence of ints" % name)
    require(lengths.dtype in (torch.int32, torch.int64), "%s must be int32 or int64, got %s" % (name, lengths.dtype))
    return lengths


def lengths_for(lengths, ref, name="lengths"):
    """The shape check of ragged_lengths against the batch size of `ref` (the operator's first tensor argument), made before
    anything else is looked at: a wrong lengths shape is reported as such whatever else is wrong with the call."""
    t = _lengths_tensor(lengths, name)
    b = ref.shape[0] if isinstance(ref, torch.Tensor) and ref.dim() >= 1 else None
    require(t.dim() == 1 and (b is None or t.shape[0] == b),
            "%s must have shape (batch_size,)%s, got %s" % (name, "" if b is None else " = (%d,)" % b, tuple(t.shape)))
    return t


def ragged_lengths(lengths, b, dev, name="lengths"):
    """The per-cloud point counts of a ragged batch as the kernels take them: a contiguous int32 tensor (b,) on `dev`.
    Accepts an int32 / int64 tensor or a sequence; a tensor already on the device is converted there (no host
    synchronisation; the VALUES are not looked at -- that is check_lengths, where the batch is built)."""
    t = _lengths_tensor(lengths, name)
    require(t.dim() == 1 and t.shape[0] == b, "%s must have shape (batch_size,) = (%d,), got %s" % (name, b, tuple(t.shape)))
    return t.to(device=dev, dtype=torch.int32).contiguous()


def full_counts(b, n, dev):
    """The count array of a DENSE side for the two-sided ragged entries (they require both arrays): (b,) int32 of n, made on
    `dev` -- no host synchronisation, capturable."""
    return torch.full((b,), int(n), dtype=torch.int32, device=dev)


def pair_counts(lengths1, lengths2, b, n, m, dev, names=("lengths1", "lengths2"), both=False):
    """THE rule for which counted entry a call with optional per-cloud counts on its two sides takes:
    -> (suffix of the C entry, lens1, lens2, behind1, behind2): the count arrays as int32 tensors on `dev` (None where the entry
    takes none; the caller holds them until its launch is enqueued) and their pointers as the tuples that splice into the
    entry's argument list behind the first and behind the second coordinate argument.
      neither given                      ""              no counts
      lengths1 only                      "_ragged"       lens1
      lengths2, with or without lengths1 "_ragged_pair"  lens1 (full_counts of n for a dense first side) and lens2
    both: the caller's entry has no unpaired variant (the level entries of sa_mlp.py): always the last row, a dense second side
    of m rows gets full_counts too. names: what the two arguments are called in messages."""
    if lengths2 is None and not both:
        if lengths1 is None:
            return "", None, None, (), ()
        lens1 = ragged_lengths(lengths1, b, dev, names[0])
        return "_ragged", lens1, None, (lens1.data_ptr(),), ()
    lens1 = ragged_lengths(lengths1, b, dev, names[0]) if lengths1 is not None else full_counts(b, n, dev)
    lens2 = ragged_lengths(lengths2, b, dev, names[1]) if lengths2 is not None else full_counts(b, m, dev)
    return "_ragged_pair", lens1, lens2, (lens1.data_ptr(),), (lens2.data_ptr(),)


def check_lengths(lengths, n, b=None):
    """Validate the per-cloud point counts of a ragged batch padded to n points: an int32 / int64 tensor (or a sequence) of
    shape (b,) with 1 <= lengths[i] <= n. Raises ValueError. This is the ONE place that looks at the values, and it
    synchronises: call it once where the batch is built -- the operators never do (their kernels clamp a bad length into
    1..n for memory safety and compute on that). b: the batch size, when the caller wants the shape checked against it.
    -> lengths as an int32 tensor (on the device it came from)."""
    t = _lengths_tensor(lengths, "lengths")
    require(t.dim() == 1, "lengths must have shape (batch_size,), got %s" % (tuple(t.shape),))
    require(b is None or t.shape[0] == int(b), "lengths must have shape (%s,), got %s" % (b, tuple(t.shape)))
    require(int(n) >= 1, "n must be positive")
    if t.numel():
        lo, hi = int(t.min()), int(t.max())
        require(lo >= 1, "lengths must be at least 1 (found %d)" % lo)
        require(hi <= int(n), "lengths must not exceed the padded size n = %d (found %d)" % (int(n), hi))
    return t.to(torch.int32)


# ---- packed batches: clouds back to back in one (total, 3) array plus offsets (b + 1) -------------------------
def packed_offsets(offsets, dev, b=None, name="offsets"):
    """The offsets of a packed batch as the kernels take them: a contiguous int32 tensor (b + 1,) on `dev`. Accepts an int32 /
    int64 tensor or a sequence; a tensor already on the device is converted there (no host synchronisation; the VALUES are not
    looked at -- that is check_offsets, where the batch is built). b: the batch size where the call has a dense side to tell it."""
    t = _lengths_tensor(offsets, name)
    require(t.dim() == 1 and t.shape[0] >= 1 and (b is None or t.shape[0] == int(b) + 1),
            "%s must have shape (batch_size + 1,)%s, got %s" % (name, "" if b is None else " = (%d,)" % (int(b) + 1), tuple(t.shape)))
    return t.to(device=dev, dtype=torch.int32).contiguous()


def packed_args(offsets, max_points, lengths, flat, what, name="offsets", max_name="max_points", b=None):
    """The checks every operator makes on a packed call before anything else: offsets excludes lengths, max_points is a host
    int (so nothing synchronises), the coordinate argument is (total, 3). -> (offsets int32 on the device, b, total, nmax)."""
    require(lengths is None, "%s: %s and lengths are two layouts of a variable-size batch; give one" % (what, name))
    require(max_points is not None, "%s: %s needs %s, a host int that bounds every cloud's count" % (what, name, max_name))
    require(not isinstance(max_points, torch.Tensor), "%s must be a host int, not a tensor" % max_name)
    nmax = int(max_points)
    require(nmax >= 1, "%s must be positive" % max_name)
    require(isinstance(flat, torch.Tensor) and flat.dim() == 2 and flat.shape[1] == 3,
            "%s: with %s the coordinates are one flat (total, 3) array" % (what, name))
    offs = packed_offsets(offsets, flat.device, b, name)
    total = int(flat.shape[0])
    require(total >= 1, "%s: a packed batch holds at least one point" % what)
    return offs, int(offs.shape[0]) - 1, total, nmax


_packed_pairs = False


def set_packed_pairs(flag):
    """Offer the second side of packed batches ("the second side, packed"): npoints= with offsets= in the sampling
    operators, lengths2= with offsets= in the ball queries, knn= / npoints= with offsets= in sample_and_group and the SA module,
    lengths2= with offsets1= in the FP module. Process-wide, off by default: every such call is refused as before."""
    global _packed_pairs
    require(isinstance(flag, bool), "set_packed_pairs expects a bool")
    _packed_pairs = flag


def packed_pairs():
    return _packed_pairs


def check_offsets(offsets, total, max_points=None):
    """Validate the offsets of a packed batch of `total` rows: an int32 / int64 tensor (or a sequence) of shape (b + 1,) with
    offsets[0] = 0, offsets[b] = total and every cloud's count offsets[c + 1] - offsets[c] in 1..max_points. Raises ValueError.
    Like check_lengths this is the ONE place that looks at the values, and it synchronises: call it once where the batch is
    built -- the operators never do (their kernels clamp for memory safety and compute on that).
    -> offsets as an int32 tensor (on the device it came from)."""
    t = _lengths_tensor(offsets, "offsets")
    require(t.dim() == 1 and t.shape[0] >= 2, "offsets must have shape (batch_size + 1,) with at least one cloud, got %s" % (tuple(t.shape),))
    require(int(total) >= 1, "total must be positive")
    v = t.to(torch.int64).cpu()
    require(int(v[0]) == 0, "offsets[0] must be 0 (found %d)" % int(v[0]))
    require(int(v[-1]) == int(total), "offsets[-1] must be total = %d (found %d)" % (int(total), int(v[-1])))
    counts = v[1:] - v[:-1]
    lo, hi = int(counts.min()), int(counts.max())
    require(lo >= 1, "every cloud of a packed batch holds at least 1 point (found a count of %d)" % lo)
    require(max_points is None or hi <= int(max_points), "a cloud holds %d points, more than max_points = %s" % (hi, max_points))
    return t.to(torch.int32)


def pack_batch(padded, lengths):
    """A padded ragged batch (b, n, c) with lengths (b,) -> (flat (total, c), offsets (b + 1,) int32 on the same device): the
    valid rows back to back. Plain torch, for tests and users building a packed batch; may synchronise."""
    require(isinstance(padded, torch.Tensor) and padded.dim() == 3, "pack_batch expects a (b, n, c) tensor")
    b, n, _ = padded.shape
    lens = check_lengths(lengths, n, b).to(device=padded.device, dtype=torch.int64)
    keep = torch.arange(n, device=padded.device)[None, :] < lens[:, None]
    offsets = torch.zeros((b + 1,), dtype=torch.int32, device=padded.device)
    offsets[1:] = torch.cumsum(lens, 0).to(torch.int32)
    return padded[keep].contiguous(), offsets


def unpack_batch(flat, offsets, n=None, fill=0.0):
    """The inverse: flat (total, c) with offsets (b + 1,) -> (padded (b, n, c) with `fill` in the padding rows, lengths (b,)
    int32). n: the padded size, None = the longest cloud. Plain torch; synchronises."""
    require(isinstance(flat, torch.Tensor) and flat.dim() == 2, "unpack_batch expects a (total, c) tensor")
    offs = check_offsets(offsets, flat.shape[0]).to(device=flat.device, dtype=torch.int64)
    lens = offs[1:] - offs[:-1]
    longest = int(lens.max())
    n = longest if n is None else int(n)
    require(n >= longest, "n = %d is below the longest cloud (%d points)" % (n, longest))
    b = lens.shape[0]
    padded = torch.full((b, n, flat.shape[1]), fill, dtype=flat.dtype, device=flat.device)
    keep = torch.arange(n, device=flat.device)[None, :] < lens[:, None]
    padded[keep] = flat
    return padded, lens.to(torch.int32)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(device):
    """The current HIP stream of `device` as an integer handle (the raw getter skips building a
    torch.cuda.Stream object: ~0.3 us instead of ~2 us per operator call)."""
    if _raw_stream is not None:
        return _raw_stream(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


class on_device:
    """Make `device` current for a launch, like torch.cuda.device(), but free when it already is
    (the common case): torch.cuda.device() alone costs several microseconds per operator call."""

    __slots__ = ("idx", "prev")

    def __init__(self, device):
        self.idx = device.index if device.index is not None else torch.cuda.current_device()
        self.prev = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.idx:
            torch.cuda.set_device(self.idx)
            self.prev = cur
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


_deterministic = False


def set_deterministic(flag):
    """Make the scatter-add gradients (gather_point, group_point, three_interpolate) reproducible: identical
    bits on every run -- sorted segments summed in the reference CPU loop's order, or 64-bit fixed-point sums
    (which rows get which: INTEGRATION.md C''). Off by default, like the reference (fp32 atomics). Also
    switched on by torch.use_deterministic_algorithms(True)."""
    global _deterministic
    _deterministic = bool(flag)


def is_deterministic():
    return _deterministic or torch.are_deterministic_algorithms_enabled()


def det_workspace(lib, b, rows, c, device):
    """Scratch for one deterministic gradient call (int64 accumulators + header)."""
    nbytes = lib.pn2_det_grad_ws_bytes(b, rows, c)
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=device)


# When the scatter-add gradients run as a segmented reduction (csrc/seg_grad.hip) instead of atomics:
# always from 16 channels up; below that only when the index inversion can use the one-workgroup-per-
# cloud LDS path (>= 4 clouds, <= 24576 target rows), where it beats the atomics even at 3 channels.
SEG_GRAD_MIN_CHANNELS = 16


def use_segmented_grad(b, rows, c):
    return c >= SEG_GRAD_MIN_CHANNELS or (b >= 4 and rows <= 24576)


def seg_workspace(lib, b, rows, entries, device):
    nbytes = lib.pn2_seg_grad_ws_bytes(b, rows, entries)
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=device)


def scatter_grad(lib, op, head, idx, plan, tail, b, rows, c, entries, dev):
    """THE rule for which reduction a scatter-add gradient (op = "group_point" / "three_interpolate": `entries` gradient rows
    per cloud summed into (b, rows, c)) takes -- INTEGRATION.md C'' states it, every caller goes through here:
    segmented (use_segmented_grad) from the index plan where idx was inverted when it was born, else inverting idx in a
    workspace; otherwise, in deterministic mode, 64-bit fixed-point sums; otherwise fp32 atomics.
    Calls pn2_<op>_grad{_planned,_seg,_det,}(*head, plan or idx, *tail, [workspace,] [deterministic,] stream) -> its return code."""
    det = 1 if is_deterministic() else 0
    if use_segmented_grad(b, rows, c):
        if plan is not None:
            return getattr(lib, "pn2_%s_grad_planned" % op)(*head, ptr(plan.buffer), *tail, det, stream_ptr(dev))
        ws = seg_workspace(lib, b, rows, entries, dev)
        return getattr(lib, "pn2_%s_grad_seg" % op)(*head, ptr(idx), *tail, ptr(ws), det, stream_ptr(dev))
    if det:
        ws = det_workspace(lib, b, rows, c, dev)
        return getattr(lib, "pn2_%s_grad_det" % op)(*head, ptr(idx), *tail, ptr(ws), stream_ptr(dev))
    return getattr(lib, "pn2_%s_grad" % op)(*head, ptr(idx), *tail, stream_ptr(dev))
