"""Host side of the sparse InstanceNorm kernels (imf_in_* in csrc/norm_train.hip): the float64 restatement against the
oracle and against torch's float64 autograd of the module's torch body, the C ABI's three symbols and their argument
checks, the item partition the coordinate manager hands out, and the module's fallback with the switch at "hip" on CPU
rows.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import imf_oracle as O
import inst_norm_restate as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("imf_in_workspace_bytes", "imf_in_forward", "imf_in_backward")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


class Rows:
    """The duck-typed carrier of tests/test_cabi_and_host.py::test_instance_norm_module_matches_the_oracle: .F, .C and
    ._like only (imfnet_amd.SparseTensor itself lives on the GPU)."""

    def __init__(self, F, C):
        self.F, self.C = F, C

    def _like(self, F):
        return Rows(F, self.C)


def _coords(sizes):
    item = np.concatenate([np.full(k, i, np.int32) for i, k in enumerate(sizes)])
    z = np.zeros(len(item))
    return item, torch.as_tensor(np.stack([item, np.arange(len(item)), z, z], 1).astype(np.int32))


def _inputs(sizes, c, seed, constant_channel=True):
    """fp32 rows with per-item, per-channel mean in [-4, 4] and sigma in [0.5, 2]; channel 0 of item 0 is the constant
    1.5 (exactly representable, so its sums are exact: variance 0, rstd = 1e4)."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for k in sizes:
        mean, sigma = torch.rand(1, c, generator=g) * 8 - 4, torch.rand(1, c, generator=g) * 1.5 + 0.5
        parts.append(torch.randn(k, c, generator=g) * sigma + mean)
    x = torch.cat(parts)
    if constant_channel:
        x[:sizes[0], 0] = 1.5
    gamma, beta = torch.rand(1, c, generator=g) + 0.5, torch.rand(1, c, generator=g) - 0.5
    res, dy = torch.randn(len(x), c, generator=g), torch.randn(len(x), c, generator=g)
    return x, gamma, beta, res, dy


SIZES = [[37, 5, 120], [129, 1], [1, 128], [64], [1]]


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "-".join(map(str, s)))
def test_restatement_forward_matches_the_oracle(sizes):
    x, gamma, beta, _, _ = _inputs(sizes, 6, 11 + len(sizes))
    item, _ = _coords(sizes)
    fw = IR.forward(x.numpy(), IR.starts_of(sizes), gamma.numpy(), beta.numpy())
    ref = O.instance_norm(x, item, gamma, beta).numpy()                  # float64 inside, rounded to float32 on return
    assert fw["y"].dtype == np.float64
    assert np.abs(fw["y"].astype(np.float32) - ref).max() <= 2.0 ** -23 * max(1.0, np.abs(ref).max())
    if sizes[0] > 1:
        assert fw["rstd"][0, 0] == 1.0 / np.sqrt(IR.EPS) and not fw["xhat"][:sizes[0], 0].any()   # the constant channel
    for b, k in enumerate(sizes):
        if k == 1:                                                       # one row: xhat = 0, y = beta
            r = IR.starts_of(sizes)[b]
            assert not fw["xhat"][r].any() and np.array_equal(fw["y"][r], beta.double().numpy().reshape(-1))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "-".join(map(str, s)))
def test_restatement_matches_torch_float64_autograd_of_the_torch_body(sizes, with_residual, relu):
    """y, dx, dgamma, dbeta and dresidual within 1e-12 relative of the module's torch ops (norm, add, relu) in float64 on
    the CPU, ragged batches with a one-row item and a channel that is constant inside an item (rstd = 1e4)."""
    import imfnet_amd.sparse as ME
    x32, gamma32, beta32, res32, dy32 = _inputs(sizes, 5, 100 * len(sizes) + 2 * with_residual + relu)
    _, coords = _coords(sizes)
    norm = ME.MinkowskiInstanceNorm(5).double()
    with torch.no_grad():
        norm.weight.copy_(gamma32.double())
        norm.bias.copy_(beta32.double())
    x = x32.double().requires_grad_(True)
    res = res32.double().requires_grad_(True) if with_residual else None
    y = norm.forward_fused(Rows(x, coords), residual=res, relu=relu).F
    y.backward(dy32.double())
    starts = IR.starts_of(sizes)
    fw = IR.forward(x32.numpy(), starts, gamma32.numpy(), beta32.numpy(), res32.numpy() if with_residual else None, relu)
    bw = IR.backward(dy32.numpy(), x32.numpy(), fw["y"], starts, gamma32.numpy(), relu)
    assert _rel(fw["y"], y.detach().numpy()) <= 1e-12
    assert _rel(bw["dx"], x.grad.numpy()) <= 1e-12
    assert _rel(bw["dgamma"], norm.weight.grad.numpy().reshape(-1)) <= 1e-12
    assert _rel(bw["dbeta"], norm.bias.grad.numpy().reshape(-1)) <= 1e-12
    if with_residual:
        assert _rel(bw["dresidual"], res.grad.numpy()) <= 1e-12 and np.array_equal(bw["dresidual"], bw["g"])
    for b, k in enumerate(sizes):
        if k == 1:
            assert not bw["dx"][starts[b]].any()                         # an item of one row passes no gradient to x


def test_header_declares_and_library_exports_the_three_symbols():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/imfnet_hip.h"
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    R = L.imf_bn_train_chunk_rows()
    # chunk partials for ceil(n / R) + n_items chunks (every item may end in a partial chunk), then 2c sums per item
    for n, c, items in ((1, 1, 1), (R, 32, 1), (R + 1, 32, 3), (1000, 5, _lib.MAX_BATCH)):
        assert L.imf_in_workspace_bytes(n, c, items) == ((n + R - 1) // R + items) * 2 * c * 8 + items * 2 * c * 8
    assert L.imf_in_workspace_bytes(0, 4, 1) == 0 and L.imf_in_workspace_bytes(4, 0, 1) == 0
    assert L.imf_in_workspace_bytes(4, 4, 0) == 0 and L.imf_in_workspace_bytes(4, 4, _lib.MAX_BATCH + 1) == 0
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = set(line.split()[-1] for line in nm.stdout.splitlines() if line.strip())
        assert set(SYMBOLS) <= exported


def test_argument_errors_return_a_status_without_a_gpu():
    """The argument checks come before any launch, so they answer on a machine without a GPU too."""
    from imfnet_amd import _lib
    L = _lib.lib()
    buf = np.zeros(4096, dtype=np.float64)
    p = buf.ctypes.data
    nbytes = L.imf_in_workspace_bytes(4, 4, 2)
    fwd = lambda n, c, items, ws, x=p, st=p: L.imf_in_forward(x, n, c, st, items, p, p, 1e-8, None, 0, p, p, p, ws, None)
    bwd = lambda n, c, items, ws, dy=p, st=p: L.imf_in_backward(dy, p, None, 0, p, p, st, n, c, items, p, p, p, None, p, ws,
                                                               None)
    for call in (fwd, bwd):
        assert call(0, 4, 2, nbytes) == -1
        assert b"n=0" in L.imf_last_error()
        assert call(4, 0, 2, nbytes) == -1
        assert call(4, 4, 0, nbytes) == -1
        assert b"n_items=0" in L.imf_last_error()
        assert call(4, 4, _lib.MAX_BATCH + 1, 1 << 20) == -1
        assert call(1 << 31, 4, 2, 1 << 40) == -1                         # item_starts is int32
        assert call(4, 4, 2, nbytes - 1) == -1
        assert b"workspace" in L.imf_last_error()
        assert call(4, 4, 2, nbytes, None) == -1                         # a null required pointer
        assert call(4, 4, 2, nbytes, p, None) == -1                      # no item_starts
        assert call(4, 4, 2, nbytes, p, p + 2) == -1                     # misaligned item_starts
    assert L.imf_in_backward(p, p, None, 1, p, p, p, 4, 4, 2, p, p, p, None, p, nbytes, None) == -1   # ReLU mask without y


def test_wrappers_refuse_cpu_tensors_and_bad_partitions_before_the_library():
    from imfnet_amd import ops
    from imfnet_amd._lib import ImfError
    x, w = torch.zeros(4, 4), torch.zeros(4)
    st = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(ImfError):
        ops.in_forward(x, st, w, w, 1e-8)
    with pytest.raises(ImfError):
        ops.in_backward(x, x, None, torch.zeros(1, 8, dtype=torch.float64), w, st)
    assert ops.item_starts_tensor([(0, 3), (3, 5)], "cpu").tolist() == [0, 3, 8]
    assert ops.item_starts_tensor([(0, 7)], "cpu").dtype == torch.int32


def test_coordinate_manager_hands_out_the_partition_only_when_the_rows_are_known_to_be_grouped():
    """CoordinateManager.item_starts: from `n_items` by a search over the batch column (an item without rows included),
    cached per level; None without `n_items`, for a level that is not built, or for a row count that is not the level's."""
    import imfnet_amd.sparse as ME
    from imfnet_amd import ops
    _, coords = _coords([3, 0, 4])
    lv = ops.Level(coords, torch.tensor([7, 0], dtype=torch.int32), None, 0, 1)
    lv.n = 7
    cm = ME.CoordinateManager(lv)
    assert cm.n_items is None and cm.item_starts(1, 7) is None
    cm = ME.CoordinateManager(lv)
    cm.n_items = 3
    st = cm.item_starts(1, 7)
    assert st.dtype == torch.int32 and st.tolist() == [0, 3, 3, 7]
    assert cm.item_starts(1, 7) is st                                    # built once per level
    assert cm.item_starts(1, 6) is None and cm.item_starts(2, 7) is None


def _block_run(switch):
    """Two norm sites as the residual block uses them, on the stand-in carrier and CPU rows, under the given switch."""
    from imfnet_amd import ops, sparse as ME
    prev = ops.set_train_norm(switch)
    try:
        sizes = [37, 5, 120]
        x, gamma, beta, res, dy = _inputs(sizes, 6, 3)
        _, coords = _coords(sizes)
        n1, n2 = ME.MinkowskiInstanceNorm(6), ME.MinkowskiInstanceNorm(6)
        with torch.no_grad():
            for m in (n1, n2):
                m.weight.copy_(gamma)
                m.bias.copy_(beta)
        x = x.requires_grad_(True)
        mid = n1.forward_fused(Rows(x, coords), relu=True)
        plain = n1(Rows(x, coords)).F                                    # forward(): no add, no ReLU
        out = n2.forward_fused(Rows(mid.F * 2.0, coords), residual=Rows(res, coords), relu=True).F
        (out * dy).sum().backward()
        grads = [x.grad] + [p.grad for m in (n1, n2) for p in m.parameters()]
        with torch.no_grad():
            ev = n1.eval().forward_fused(Rows(x.detach(), coords), residual=res, relu=False).F
        return [mid.F.detach(), plain.detach(), out.detach(), ev], grads
    finally:
        ops.set_train_norm(prev)


def test_cpu_rows_with_the_switch_at_hip_are_bit_identical_to_the_switch_at_torch():
    """The fallback is today's ops: on CPU rows and the stand-in carrier the switch changes nothing, bit for bit."""
    a, b = _block_run("torch"), _block_run("hip")
    for part_a, part_b in zip(a, b):
        assert len(part_a) == len(part_b)
        for u, v in zip(part_a, part_b):
            assert torch.equal(u, v)
    item, _ = _coords([37, 5, 120])
    x, gamma, beta, _, _ = _inputs([37, 5, 120], 6, 3)
    assert float((a[0][1] - O.instance_norm(x, item, gamma, beta)).abs().max()) < 1e-5


class _Matmul(torch.nn.Module):
    """Stands in for a sparse convolution on the carrier: rows times a fixed matrix."""

    def __init__(self, c, seed):
        super().__init__()
        self.w = torch.randn(c, c, generator=torch.Generator().manual_seed(seed)) / c ** 0.5

    def forward(self, x):
        return x._like(x.F @ self.w)


def test_in_block_issues_norm_then_add_then_relu_with_the_switch_at_torch():
    """BasicBlockIN.forward with its two convolutions stubbed, against the explicit composition
    relu(norm2(conv2(relu(norm1(conv1(x))))) + x): bit for bit, so the add comes after the norm and before the ReLU."""
    from imfnet_amd import ops
    from imfnet_amd.model.layers import BasicBlockIN
    assert ops.TRAIN_NORM == "torch"
    sizes = [37, 5, 120]
    x, gamma, beta, _, _ = _inputs(sizes, 8, 9)
    _, coords = _coords(sizes)
    blk = BasicBlockIN(8, 8)
    blk.conv1, blk.conv2 = _Matmul(8, 1), _Matmul(8, 2)
    with torch.no_grad():
        for m in (blk.norm1, blk.norm2):
            m.weight.copy_(torch.rand(1, 8, generator=torch.Generator().manual_seed(4)) + 0.5)
            m.bias.copy_(torch.rand(1, 8, generator=torch.Generator().manual_seed(5)) - 0.5)
        got = blk(Rows(x, coords)).F
        h = F.relu(blk.norm1(Rows(x @ blk.conv1.w, coords)).F)
        want = F.relu(blk.norm2(Rows(h @ blk.conv2.w, coords)).F + x)
        other = F.relu(blk.norm2(Rows(h @ blk.conv2.w, coords)).F) + x
    assert torch.equal(got, want) and not torch.equal(got, other)
