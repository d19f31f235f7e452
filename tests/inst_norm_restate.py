"""Float64 NumPy restatement of the two InstanceNorm calls of csrc/norm_train.hip (imf_in_forward / imf_in_backward):
per batch item and channel (x - mean) / sqrt(biased variance + eps) over the item's rows, then gamma * xhat + beta with
the optional residual add and ReLU behind it.  Rows are grouped by item: item b owns rows [starts[b], starts[b + 1]).
Inputs are float32 arrays (or anything np.asarray takes); everything is computed in float64 and returned in float64 -- the
callers round where the kernel rounds.  tests/test_inst_norm_host.py checks this file against oracle.instance_norm and
against torch's float64 autograd of the module's torch body."""
import numpy as np

EPS = 1e-8


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def starts_of(sizes):
    """[0, n_0, n_0 + n_1, ...]: the row starts of items of the given sizes."""
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def item_stats(x, starts, eps=EPS):
    """(mean, rstd), each [n_items, C]; an item without rows gets (0, 0)."""
    x = _f64(x)
    n_items = len(starts) - 1
    mean, rstd = np.zeros((n_items, x.shape[1])), np.zeros((n_items, x.shape[1]))
    for b in range(n_items):
        v = x[starts[b]:starts[b + 1]]
        if len(v):
            mean[b] = v.sum(0) / len(v)
            rstd[b] = 1.0 / np.sqrt(((v - mean[b]) ** 2).sum(0) / len(v) + eps)
    return mean, rstd


def _xhat(x, starts, mean, rstd):
    xhat = np.zeros_like(x)
    for b in range(len(starts) - 1):
        s, e = starts[b], starts[b + 1]
        xhat[s:e] = (x[s:e] - mean[b]) * rstd[b]
    return xhat


def forward(x, starts, gamma, beta, residual=None, relu=False, eps=EPS):
    """dict(y, xhat, pre, mean, rstd): `pre` is the value before the ReLU; mean / rstd are [n_items, C]."""
    x, gamma, beta, residual = _f64(x), _f64(gamma).reshape(-1), _f64(beta).reshape(-1), _f64(residual)
    mean, rstd = item_stats(x, starts, eps)
    xhat = _xhat(x, starts, mean, rstd)
    pre = xhat * gamma + beta
    if residual is not None:
        pre = pre + residual
    y = np.maximum(pre, 0.0) if relu else pre
    return dict(y=y, xhat=xhat, pre=pre, mean=mean, rstd=rstd)


def backward(dy, x, y, starts, gamma, relu=False, eps=EPS):
    """dict(g, dx, dgamma, dbeta, dresidual) of the forward above, in closed form per item:
    dx = gamma rstd_b (g - S1_b / n_b - xhat S2_b / n_b), S1_b = sum_b g, S2_b = sum_b g xhat; dbeta = sum_b S1_b and
    dgamma = sum_b S2_b.  `y` is read only for the ReLU mask y > 0; dresidual is the masked gradient g."""
    dy, x, gamma = _f64(dy), _f64(x), _f64(gamma).reshape(-1)
    mean, rstd = item_stats(x, starts, eps)
    xhat = _xhat(x, starts, mean, rstd)
    g = np.where(np.asarray(y) > 0, dy, 0.0) if relu else dy
    dx = np.zeros_like(x)
    dbeta, dgamma = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for b in range(len(starts) - 1):
        s, e = starts[b], starts[b + 1]
        if e == s:
            continue
        s1, s2 = g[s:e].sum(0), (g[s:e] * xhat[s:e]).sum(0)
        dx[s:e] = gamma * rstd[b] * (g[s:e] - s1 / (e - s) - xhat[s:e] * s2 / (e - s))
        dbeta += s1
        dgamma += s2
    return dict(g=g, xhat=xhat, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta, dresidual=g)
