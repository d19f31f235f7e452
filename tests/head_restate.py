"""The descriptor head of training (csrc/head_train.hip) restated in float64, the torch ops it replaces, and the seeded
cases both are run on.  No GPU, no library call.

    H = relu(U W1[:cu] + S W1[cu:])      Z = H W2 + b      r = sqrt(sum_c Z_c^2)      Y = Z / r   (normalize)  or  Z
    dZ = (dY - Y sum_c(dY Y)) / r  (normalize)  or  dY
    db = sum_rows dZ     dW2 = H^T dZ     dH = (dZ W2^T) [H > 0]     dW1 = [U S]^T dH
    dU = dH W1[:cu]^T    dS = dH W1[cu:]^T

Inputs: U Gaussian, S >= 0 (a ReLU output), W1 and W2 uniform at the modules' initial scale (+-1 / sqrt(fan in)), b in
U(0.1, 0.5) so that no row's norm is near zero, dY Gaussian."""
import functools

import numpy as np
import torch

CU, CS, CH, CO = 64, 32, 64, 32
TENSORS = ("Y", "dU", "dS", "dW1", "dW2", "db")
MAX_ROWS = 2048          # the gate's factor 8 is derived for sums of at most 2048 terms (tests/test_gpu_fusion_train.py)


def row_counts(chunk):
    """The row counts of the GPU tests for a reduction chunk of `chunk` rows: one row, either side of a 32-row boundary,
    either side of a chunk boundary, and two chunks and a ragged tile -- capped at MAX_ROWS."""
    ns = [1, 31, 33, chunk - 1, chunk, chunk + 1, 2 * chunk + 17]
    return sorted({n for n in ns if 1 <= n <= MAX_ROWS})


@functools.lru_cache(maxsize=None)
def case(n, kind="random", seed=0):
    """{U, S, W1, W2, b, dY}: float32 CPU tensors.  kind "dead": U W1 + S W1 < 0 everywhere (H == 0); "alive": > 0
    everywhere; "random": both signs."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    U = torch.randn(n, CU, generator=g)
    S = torch.randn(n, CS, generator=g).abs()
    W1 = (torch.rand(CU + CS, CH, generator=g) * 2 - 1) / np.sqrt(CU + CS)
    W2 = (torch.rand(CH, CO, generator=g) * 2 - 1) / np.sqrt(CH)
    b = 0.1 + 0.4 * torch.rand(1, CO, generator=g)
    dY = torch.randn(n, CO, generator=g)
    if kind in ("dead", "alive"):
        U = U.abs() + 0.01
        W1 = (W1.abs() + 1e-3) * (-1.0 if kind == "dead" else 1.0)
    elif kind != "random":
        raise ValueError(kind)
    return dict(U=U, S=S, W1=W1, W2=W2, b=b, dY=dY, n=n, kind=kind)


def restate(c, normalize=True):
    """The equations of the module docstring in float64 numpy: {Y, dU, dS, dW1, dW2, db, H, r}."""
    U, S, W1, W2, b, dY = (c[k].double().numpy() for k in ("U", "S", "W1", "W2", "b", "dY"))
    H = np.maximum(U @ W1[:CU] + S @ W1[CU:], 0.0)
    Z = H @ W2 + b
    r = np.sqrt((Z * Z).sum(axis=1, keepdims=True))
    if normalize:
        Y = Z / r
        dZ = (dY - Y * (dY * Y).sum(axis=1, keepdims=True)) / r
    else:
        Y, dZ = Z, dY
    dH = (dZ @ W2.T) * (H > 0)
    return dict(Y=Y, dU=dH @ W1[:CU].T, dS=dH @ W1[CU:].T, dW1=np.concatenate([U, S], axis=1).T @ dH, dW2=H.T @ dZ,
                db=dZ.sum(axis=0, keepdims=True), H=H, r=r[:, 0])


@functools.lru_cache(maxsize=None)
def reference(n, kind="random", normalize=True, seed=0):
    """restate() of case(), computed once per process; callers do not write into it."""
    return restate(case(n, kind, seed), normalize)


def torch_path(c, dtype=torch.float32, device="cpu", normalize=True):
    """The module ops the kernels replace, under torch's autograd: cat, the two pointwise convolutions as feature-matrix
    products with the parameters' own [Cin, Cout] kernels, relu, the bias add, torch.norm and the division.  {Y, dU, dS,
    dW1, dW2, db} as tensors of `dtype` on `device`."""
    U, S, W1, W2, b = (c[k].to(device=device, dtype=dtype).clone().requires_grad_(True) for k in ("U", "S", "W1", "W2", "b"))
    dY = c["dY"].to(device=device, dtype=dtype)
    out = torch.relu(torch.cat([U, S], dim=1) @ W1)
    out = out @ W2 + b
    if normalize:
        out = out / torch.norm(out, p=2, dim=1, keepdim=True)
    out.backward(dY)
    return dict(Y=out.detach(), dU=U.grad, dS=S.grad, dW1=W1.grad, dW2=W2.grad, db=b.grad)


def rel_err(a, ref):
    """max|a - ref| / max|ref| in float64."""
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())
