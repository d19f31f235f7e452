"""Descriptor Activation Mapping restated twice: the closed form in NumPy float64, and the literal
procedure of the reference's loop in torch -- 32 backward(retain_graph=True) calls through a 64 -> 32 linear layer with
bias and a row normalisation, reading the ACCUMULATING .grad of the kernel after each."""
import numpy as np
import torch

C_OUT = 32
# max |float32 literal loop - float64 closed form| / max |heat| over the cases of tests/test_dam_host.py, as recorded in
# the reference arithmetic's own error.  The gate is 8x: the value depends on torch's summation order.
LITERAL_F32_ERR = 3.2e-7
LITERAL_F32_GATE = 8 * LITERAL_F32_ERR


def weights(h_t, o_t, accumulate=True):
    """w[0:32] in float64 for one target row: hidden row h_t [c_hid], pre-normalisation row o_t [32].  (w, bad)."""
    h_t, o_t = np.asarray(h_t, dtype=np.float64), np.asarray(o_t, dtype=np.float64)
    r = float(np.sqrt((o_t * o_t).sum()))
    if not (r > 0.0 and np.isfinite(r)):
        return np.zeros(C_OUT), True
    f = o_t / r
    a = np.arange(C_OUT, 0, -1, dtype=np.float64) if accumulate else np.ones(C_OUT)
    s = (a - f * (a * f).sum()) / r
    return h_t.mean() * s, False


def closed_form(h, o, targets, accumulate=True):
    """(pre [T, n] float64 = sum_c w_c o[n, c] before the ReLU, mag [T, n] = sum_c |w_c o[n, c]|, w [T, 32], flags [T])."""
    h, o = np.asarray(h, dtype=np.float64), np.asarray(o, dtype=np.float64)
    n = o.shape[0]
    T = len(targets)
    w, flags = np.zeros((T, C_OUT)), np.zeros(T, dtype=np.int32)
    for i, t in enumerate(targets):
        if not 0 <= int(t) < n:
            flags[i] = 1
            continue
        w[i], bad = weights(h[int(t)], o[int(t)], accumulate)
        flags[i] = int(bad)
    return w @ o.T, np.abs(w) @ np.abs(o).T, w, flags


def heat(h, o, targets, accumulate=True):
    return np.maximum(closed_form(h, o, targets, accumulate)[0], 0.0)


def literal_loop(h, kernel, bias, target, accumulate=True, dtype=torch.float64):
    """The loop itself on torch autograd: o = h K + b, F = o / |o|, one backward per descriptor component of the target
    row, the map of each step = (mean over the hidden axis of kernel.grad) . o, the 32 maps summed, then ReLU.
    accumulate=False clears the gradient before each step.  Returns the heat [n] in `dtype`."""
    h = torch.as_tensor(h).to(dtype)
    K = torch.as_tensor(kernel).to(dtype).clone().requires_grad_(True)
    b = torch.as_tensor(bias).to(dtype).reshape(1, -1).clone().requires_grad_(True)
    o = h @ K + b
    F = o / torch.norm(o, p=2, dim=1, keepdim=True)
    maps = []
    for j in range(F.shape[1]):
        if not accumulate:
            K.grad = None
        F[target, j].backward(retain_graph=True)
        channel = K.grad.detach().t().mean(dim=1)                 # [32]: mean over the hidden axis
        maps.append((channel[:, None] * o.detach().t()).sum(dim=0))
    return torch.clamp(torch.stack(maps).sum(dim=0), min=0)
