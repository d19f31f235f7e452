"""Host side of the training-mode sparse BatchNorm (csrc/norm_train.hip): the float64 restatement against torch's own
float64 autograd, the C ABI's four symbols, the trainer's --norm_kernels option, and the fallback of the module with the
switch at "hip" on CPU rows.  No GPU."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_restate as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("imf_bn_train_chunk_rows", "imf_bn_train_workspace_bytes", "imf_bn_train_forward", "imf_bn_train_backward")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("n,c", [(2, 1), (3, 5), (259, 32)])
def test_restatement_matches_torch_float64_autograd(n, c, with_residual, relu):
    """The yardstick itself: y, dx, dgamma, dbeta, dresidual and the running statistics within 1e-12 relative of
    torch.nn.functional.batch_norm(training=True) + add + relu in float64 on the CPU."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * c + 2 * with_residual + relu)
    x32 = (torch.randn(n, c, generator=gen) * 3 + 1.5)
    gamma32, beta32 = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    res32 = torch.randn(n, c, generator=gen) if with_residual else None
    dy32 = torch.randn(n, c, generator=gen)
    rm32, rv32 = torch.randn(c, generator=gen), torch.rand(c, generator=gen) + 0.5
    eps, mom = 1e-5, 0.05
    x = x32.double().requires_grad_(True)
    gamma, beta = gamma32.double().requires_grad_(True), beta32.double().requires_grad_(True)
    res = res32.double().requires_grad_(True) if with_residual else None
    rm, rv = rm32.double().clone(), rv32.double().clone()
    y = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=mom, eps=eps)
    if with_residual:
        y = y + res
    if relu:
        y = F.relu(y)
    y.backward(dy32.double())
    fw = NR.forward(x32.numpy(), gamma32.numpy(), beta32.numpy(), eps, None if res32 is None else res32.numpy(), relu,
                    rm32.numpy(), rv32.numpy(), mom)
    bw = NR.backward(dy32.numpy(), x32.numpy(), fw["y"], gamma32.numpy(), eps, relu)
    assert fw["y"].dtype == np.float64 and bw["dx"].dtype == np.float64
    assert _rel(fw["y"], y.detach().numpy()) <= 1e-12
    assert _rel(fw["running_mean"], rm.numpy()) <= 1e-12 and _rel(fw["running_var"], rv.numpy()) <= 1e-12
    assert _rel(bw["dx"], x.grad.numpy()) <= 1e-12
    assert _rel(bw["dgamma"], gamma.grad.numpy()) <= 1e-12
    assert _rel(bw["dbeta"], beta.grad.numpy()) <= 1e-12
    if with_residual:
        assert _rel(bw["dresidual"], res.grad.numpy()) <= 1e-12
        assert np.array_equal(bw["dresidual"], bw["g"])


def test_restatement_gives_zero_gradient_where_the_pre_activation_is_exactly_zero():
    """gamma = 0 and beta = 0 in channel 0: its pre-activation is exactly 0 in every row, and its gradient is 0 under the
    mask y > 0 as under torch's ReLU; channel 1 (gamma = 1) is the control."""
    x = np.array([[-1.0, 2.0], [1.0, 5.0], [4.0, -3.0]], dtype=np.float32)
    gamma, beta = np.array([0.0, 1.0], np.float32), np.array([0.0, 0.5], np.float32)
    fw = NR.forward(x, gamma, beta, 1e-5, relu=True)
    assert not fw["pre"][:, 0].any() and not fw["y"][:, 0].any() and fw["y"][:, 1].any()
    bw = NR.backward(np.ones((3, 2), np.float32), x, fw["y"], gamma, 1e-5, relu=True)
    assert not bw["g"][:, 0].any() and not bw["dx"][:, 0].any() and bw["dbeta"][0] == 0 and bw["dbeta"][1] > 0
    xt = torch.tensor(x, dtype=torch.float64)
    gt, bt = torch.tensor(gamma, dtype=torch.float64, requires_grad=True), torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    F.relu(F.batch_norm(xt, None, None, gt, bt, training=True, eps=1e-5)).sum().backward()
    assert bt.grad[0] == 0 and gt.grad[0] == 0                       # torch's ReLU gives 0 there too
    assert _rel(bw["dbeta"], bt.grad.numpy()) <= 1e-12 and _rel(bw["dgamma"], gt.grad.numpy()) <= 1e-12


def test_header_declares_and_library_exports_the_four_symbols():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/imfnet_hip.h"
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    R = L.imf_bn_train_chunk_rows()
    assert R >= 2
    # chunk partials (two fp64 per channel and chunk) and the backward's two sums: grows with the chunk count only
    assert L.imf_bn_train_workspace_bytes(R, 32) == L.imf_bn_train_workspace_bytes(2, 32) > 0
    assert L.imf_bn_train_workspace_bytes(R + 1, 32) - L.imf_bn_train_workspace_bytes(R, 32) == 2 * 32 * 8
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
    nbytes = L.imf_bn_train_workspace_bytes(4, 4)
    fwd = lambda n, c, ws, x=p: L.imf_bn_train_forward(x, n, c, p, p, 1e-5, None, 0, None, None, 0.1, p, p, p, ws, None)
    bwd = lambda n, c, ws, dy=p: L.imf_bn_train_backward(dy, p, None, 0, p, p, n, c, p, p, p, None, p, ws, None)
    for call in (fwd, bwd):
        assert call(1, 4, nbytes) == -1                              # one value per channel
        assert b"n=1" in L.imf_last_error()
        assert call(0, 4, nbytes) == -1
        assert call(4, 0, nbytes) == -1
        assert call(4, 4, nbytes - 1) == -1
        assert b"workspace" in L.imf_last_error()
        assert call(4, 4, nbytes, None) == -1                        # a null required pointer
    assert L.imf_bn_train_backward(p, p, None, 1, p, p, 4, 4, p, p, p, None, p, nbytes, None) == -1   # ReLU mask without y


def test_norm_kernels_option_parses_defaults_to_torch_and_refuses_other_values(capsys):
    from imfnet_amd.train.trainer import parse_config
    assert parse_config([]).norm_kernels == "torch"
    assert parse_config(["--norm_kernels", "torch"]).norm_kernels == "torch"
    assert parse_config(["--norm_kernels", "hip"]).norm_kernels == "hip"
    for bad in ("HIP", "triton", ""):
        with pytest.raises(SystemExit):
            parse_config(["--norm_kernels", bad])
    capsys.readouterr()
    before = set(vars(parse_config([])))
    assert "norm_kernels" in before and {"voxel_size", "bn_momentum", "seed", "model"} <= before


def test_norm_kernels_lands_in_the_saved_config_and_sets_the_switch(tmp_path):
    from imfnet_amd import ops
    from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config
    prev = ops.TRAIN_NORM
    try:
        for choice in ("hip", "torch"):
            out = tmp_path / choice
            cfg = parse_config(["--out_dir", str(out), "--norm_kernels", choice])
            tr = HardestContrastiveTrainer(cfg, None, None, device="cpu")
            tr.pool.shutdown()
            assert ops.TRAIN_NORM == choice
            assert json.load(open(out / "config.json"))["norm_kernels"] == choice
            tr._save(1, "checkpoint")
            ck = torch.load(out / "checkpoint.pth", weights_only=False)
            assert ck["config"]["norm_kernels"] == choice and ck["config"]["voxel_size"] == 0.025
    finally:
        ops.TRAIN_NORM = prev


def test_switch_values():
    from imfnet_amd import ops
    from imfnet_amd._lib import ImfError
    assert ops.TRAIN_NORM_CHOICES == ("torch", "hip")
    prev = ops.set_train_norm("hip")
    try:
        assert ops.TRAIN_NORM == "hip"
        with pytest.raises(ImfError):
            ops.set_train_norm("cuda")
        assert ops.TRAIN_NORM == "hip"
    finally:
        ops.set_train_norm(prev)
    env = dict(os.environ, IMF_TRAIN_NORM="hip", PYTHONPATH=ROOT)
    got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops; print(ops.TRAIN_NORM)"], env=env,
                         capture_output=True, text=True, cwd=ROOT)
    assert got.returncode == 0 and got.stdout.strip() == "hip", got.stderr


class _Rows:
    """Stand-in for a sparse tensor on the CPU (imfnet_amd.SparseTensor itself lives on the GPU only): the two members
    MinkowskiBatchNorm reads."""

    def __init__(self, f):
        self.F = f

    def _like(self, f):
        return _Rows(f)


def _cpu_model_run(switch):
    """norm1 -> relu, then norm2 -> + x -> relu on CPU rows, the residual block's two norm sites; (outputs, gradients,
    buffers) under the given switch."""
    from imfnet_amd import ops, sparse as ME
    prev = ops.set_train_norm(switch)
    try:
        torch.manual_seed(5)
        n1, n2 = ME.MinkowskiBatchNorm(6, momentum=0.05), ME.MinkowskiBatchNorm(6, momentum=0.05)
        with torch.no_grad():
            for m in (n1, n2):
                m.bn.weight.uniform_(0.5, 1.5)
                m.bn.bias.uniform_(-0.5, 0.5)
        n1.train(), n2.train()
        x = torch.randn(37, 6, generator=torch.Generator().manual_seed(6)).requires_grad_(True)
        mid = n1.forward_fused(_Rows(x), relu=True)
        plain = n1(_Rows(x)).F                                        # forward(): no add, no ReLU
        out = n2.forward_fused(_Rows(mid.F * 2.0), residual=x, relu=True).F
        (out.sum() + (plain * plain).sum()).backward()
        grads = [x.grad] + [p.grad for m in (n1, n2) for p in m.parameters()]
        bufs = [b.clone() for m in (n1, n2) for b in m.buffers()]
        n1.eval()
        with torch.no_grad():
            ev = n1.forward_fused(_Rows(x.detach()), residual=_Rows(x.detach()), relu=True).F
        return [mid.F.detach(), plain.detach(), out.detach(), ev], grads, bufs
    finally:
        ops.set_train_norm(prev)


def test_cpu_rows_with_the_switch_at_hip_are_bit_identical_to_the_switch_at_torch():
    """The fallback is today's ops: on CPU rows the switch changes nothing, bit for bit, and forward_fused is
    bn, then add, then relu."""
    a, b = _cpu_model_run("torch"), _cpu_model_run("hip")
    for part_a, part_b in zip(a, b):
        assert len(part_a) == len(part_b)
        for u, v in zip(part_a, part_b):
            assert torch.equal(u, v)
    # ... and those ops are the sequence the block always issued
    from imfnet_amd import sparse as ME
    torch.manual_seed(5)
    n1 = ME.MinkowskiBatchNorm(6, momentum=0.05).train()
    with torch.no_grad():
        n1.bn.weight.uniform_(0.5, 1.5)
        n1.bn.bias.uniform_(-0.5, 0.5)
    x = torch.randn(37, 6, generator=torch.Generator().manual_seed(6))
    assert torch.equal(F.relu(n1.bn(x)), a[0][0])
    assert int(a[2][2]) == 2 and int(a[2][5]) == 1                   # num_batches_tracked: norm1 ran twice, norm2 once
