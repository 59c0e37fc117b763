"""Ragged rows are a property of the two training nodes, not nodes of their own: a dense and a ragged call reach the same autograd
node class, and what the node saves for backward is, in order,

    dense   the node's own leading tensors, per layer the weights, the biases that exist, gammas, betas, the pre-norm tensors
            z_l and the (4, C_l) statistics, then the output -- and NO mask;
    ragged  the same, then the validity mask the node owns and the very `lengths` tensor it was given.

Shapes, the smallest the ragged tests use: plain rows at case B of tests/test_train_ragged_gpu.py (b 4, n 200, lengths 200 / 137
/ 1 / 32, stack 32 -> 32 -> 32 -> 64), the FP node at case C of tests/test_fp_level_ragged_gpu.py (b 2, n 96, m 16, lengths 96 /
50, c2 16, c1 16, stack [32]).

The dense call must not have gained a buffer: the peak of allocated bytes over one warm forward + backward (measured as
test_fp_level_ragged_gpu.py::test_module_node_route_never_holds_the_concatenated_tensor measures it) equals, to the byte, what
the commit before the fold allocated at the same shape."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = dict(b=4, n=200, lengths=(200, 137, 1, 32), cin=32, mlp=[32, 32, 64])
FP = dict(b=2, n=96, m=16, lengths=(96, 50), c2=16, c1=16, mlp=[32])
# recorded on commit 8e44fd7 ("tests: ragged training nodes at model widths, every masked kernel"), the parent of the fold, by
# dense_peak_bytes below at these shapes
PARENT_DENSE_PEAK = {"rows": 1756672, "fp": 283648}


def _net(cin, mlp, dev):
    from pointnet2_amd.pointnet_util import _SharedMLP
    torch.manual_seed(7)
    return _SharedMLP(cin, mlp).net.to(dev).train()


def _node(out, name):
    fn = out.grad_fn
    while fn is not None and type(fn).__name__ != name:
        fn = fn.next_functions[0][0]
    assert fn is not None, "no %s behind the output" % name
    return fn


def _rows_call(dev, ragged):
    """fp_mlp_train at ROWS -> net, x, lengths (None: the dense call), out"""
    from pointnet2_amd import train_mlp
    c = ROWS
    net = _net(c["cin"], c["mlp"], dev)
    x = torch.randn(c["b"], c["n"], c["cin"], generator=torch.Generator().manual_seed(8)).to(dev).requires_grad_(True)
    lengths = torch.tensor(c["lengths"], dtype=torch.int32, device=dev) if ragged else None
    return net, x, lengths, train_mlp.fp_mlp_train(net, x, lengths=lengths)


def _fp_call(dev, ragged):
    """fp_level_train at FP -> net, points2, points1, lengths (None: the dense call), out"""
    from pointnet2_amd import train_mlp
    from pointnet2_amd.tf_interpolate import three_nn
    c = FP
    net = _net(c["c2"] + c["c1"], c["mlp"], dev)
    g = torch.Generator().manual_seed(9)
    xyz1, xyz2 = torch.rand(c["b"], c["n"], 3, generator=g).to(dev), torch.rand(c["b"], c["m"], 3, generator=g).to(dev)
    p2 = torch.randn(c["b"], c["m"], c["c2"], generator=g).to(dev).requires_grad_(True)
    p1 = torch.randn(c["b"], c["n"], c["c1"], generator=g).to(dev).requires_grad_(True)
    lengths = torch.tensor(c["lengths"], dtype=torch.int32, device=dev) if ragged else None
    dist, idx = three_nn(xyz1, xyz2, lengths1=lengths)
    return net, p2, p1, lengths, train_mlp.fp_level_train(net, p2, p1, idx, dist, lengths=lengths)


def _check_layers(saved, net, rows):
    """saved: what stands between the node's leading tensors and its output -- per layer group the parameters themselves, then
    z_l (rows, C_l) and the statistics (4, C_l). -> the number of tensors that is"""
    convs = [m for m in net if isinstance(m, torch.nn.Conv2d)]
    bns = [m for m in net if isinstance(m, torch.nn.BatchNorm2d)]
    biases = [c.bias for c in convs if c.bias is not None]
    params = [c.weight for c in convs] + biases + [b.weight for b in bns] + [b.bias for b in bns]
    n, k = len(convs), len(params)
    assert [t.data_ptr() for t in saved[:k]] == [p.data_ptr() for p in params]
    widths = [c.out_channels for c in convs]
    assert [tuple(t.shape) for t in saved[k:k + n]] == [(rows, w) for w in widths]               # z_l: every one kept
    assert [tuple(t.shape) for t in saved[k + n:k + 2 * n]] == [(4, w) for w in widths]
    assert all(t.dtype == torch.float32 for t in saved[k:k + 2 * n])
    return k + 2 * n


def _check_tail(tail, lengths, rows):
    mask, saved_lengths = tail
    assert saved_lengths.data_ptr() == lengths.data_ptr() and saved_lengths.dtype == torch.int32
    assert mask.dtype == torch.int64 and tuple(mask.shape) == (2 + (rows // 32 + 1) // 2,)


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_plain_rows_one_node_and_its_saved_tensors(cuda, ragged):
    rows = ROWS["b"] * ROWS["n"]
    net, x, lengths, out = _rows_call(cuda, ragged)
    saved = _node(out, "_TrainMLPBackward").saved_tensors
    assert saved[0].data_ptr() == x.data_ptr() and tuple(saved[0].shape) == (rows, ROWS["cin"])
    k = 1 + _check_layers(saved[1:], net, rows)
    assert saved[k].data_ptr() == out.data_ptr()                                                  # no pooling tail on plain rows
    if ragged:
        assert len(saved) == k + 3
        _check_tail(saved[k + 1:], lengths, rows)
    else:
        assert len(saved) == k + 1                                                                # ... and no mask


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_fp_level_one_node_and_its_saved_tensors(cuda, ragged):
    rows = FP["b"] * FP["n"]
    net, p2, p1, lengths, out = _fp_call(cuda, ragged)
    saved = _node(out, "_TrainFPBackward").saved_tensors
    assert [t.data_ptr() for t in saved[:2]] == [p2.data_ptr(), p1.data_ptr()]
    assert tuple(saved[2].shape) == (FP["b"], FP["n"], 3) and saved[2].dtype == torch.float32    # the interpolation weights
    k = 3 + _check_layers(saved[3:], net, rows)
    assert saved[k].data_ptr() == out.data_ptr()
    if ragged:
        assert len(saved) == k + 3
        _check_tail(saved[k + 1:], lengths, rows)
    else:
        assert len(saved) == k + 1


def dense_peak_bytes(dev):
    """-> {"rows": ..., "fp": ...}: torch.cuda.max_memory_allocated over one warm dense forward + backward of each node, above what
    was allocated before it"""
    from pointnet2_amd import train_mlp
    from pointnet2_amd.tf_interpolate import three_nn
    g = torch.Generator().manual_seed(10)
    net_r = _net(ROWS["cin"], ROWS["mlp"], dev)
    x = torch.randn(ROWS["b"], ROWS["n"], ROWS["cin"], generator=g).to(dev).requires_grad_(True)
    gout_r = torch.randn(ROWS["b"], ROWS["n"], ROWS["mlp"][-1], generator=g).to(dev)
    c = FP
    net_f = _net(c["c2"] + c["c1"], c["mlp"], dev)
    xyz1, xyz2 = torch.rand(c["b"], c["n"], 3, generator=g).to(dev), torch.rand(c["b"], c["m"], 3, generator=g).to(dev)
    p2 = torch.randn(c["b"], c["m"], c["c2"], generator=g).to(dev).requires_grad_(True)
    p1 = torch.randn(c["b"], c["n"], c["c1"], generator=g).to(dev).requires_grad_(True)
    gout_f = torch.randn(c["b"], c["n"], c["mlp"][-1], generator=g).to(dev)
    dist, idx = three_nn(xyz1, xyz2)
    steps = {"rows": (lambda: train_mlp.fp_mlp_train(net_r, x), [x] + list(net_r.parameters()), gout_r),
             "fp": (lambda: train_mlp.fp_level_train(net_f, p2, p1, idx, dist), [p2, p1] + list(net_f.parameters()), gout_f)}

    def peak(forward, inputs, gout):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = forward()
        grads = torch.autograd.grad(out, inputs, gout)
        torch.cuda.synchronize()
        del out, grads
        return torch.cuda.max_memory_allocated() - base
    for step in steps.values():
        peak(*step)                                                                               # warm: the kernels loaded
    return {name: peak(*step) for name, step in steps.items()}


def test_dense_calls_allocate_what_they_did_before_the_fold(cuda, monkeypatch):
    from pointnet2_amd import train_mlp
    # scripts/train_mlp_check.py (other tests run its cases) leaves the diagnostic "keep the last backward's workspace" on: the
    # kept one would stand in the baseline and be released inside the measured step
    monkeypatch.setattr(train_mlp, "_KEEP_WS", [False, None])
    got = dense_peak_bytes(cuda)
    print("dense peak bytes: %r (before the fold: %r)" % (got, PARENT_DENSE_PEAK))
    assert got == PARENT_DENSE_PEAK
