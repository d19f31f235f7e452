"""Float64 NumPy restatement of the two calls of csrc/norm_train.hip (imf_bn_train_forward / imf_bn_train_backward):
training-mode BatchNorm over the rows of [N, C] features with the optional residual add and ReLU behind it.  Inputs are
float32 arrays (or anything np.asarray takes); everything is computed in float64 and returned in float64 -- the callers
round where the kernel rounds.  tests/test_norm_host.py checks this file against torch's own float64 autograd."""
import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def batch_stats(x, eps):
    """(mean [C], biased variance [C], rstd [C]).  The mean is sum / N: on integer data an exact sum and one division."""
    x = _f64(x)
    n = x.shape[0]
    mean = x.sum(0) / n
    var = ((x - mean) ** 2).sum(0) / n
    return mean, var, 1.0 / np.sqrt(var + eps)


def forward(x, gamma, beta, eps, residual=None, relu=False, running_mean=None, running_var=None, momentum=0.1):
    """dict(y, xhat, pre, mean, var, rstd, running_mean, running_var): `pre` is the value before the ReLU; the running
    statistics are torch's (1 - m) * old + m * new with the unbiased variance, None when none were given."""
    x, gamma, beta, residual = _f64(x), _f64(gamma), _f64(beta), _f64(residual)
    n = x.shape[0]
    mean, var, rstd = batch_stats(x, eps)
    xhat = (x - mean) * rstd
    pre = xhat * gamma + beta
    if residual is not None:
        pre = pre + residual
    y = np.maximum(pre, 0.0) if relu else pre
    out = dict(y=y, xhat=xhat, pre=pre, mean=mean, var=var, rstd=rstd, running_mean=None, running_var=None)
    if running_mean is not None:
        out["running_mean"] = (1.0 - momentum) * _f64(running_mean) + momentum * mean
    if running_var is not None:
        out["running_var"] = (1.0 - momentum) * _f64(running_var) + momentum * (var * n / (n - 1.0))
    return out


def backward(dy, x, y, gamma, eps, relu=False):
    """dict(g, dx, dgamma, dbeta, dresidual) of the forward above.  `y` is read only for the ReLU mask y > 0 (the kernel's
    rule: where the output is exactly 0 the gradient is 0); dresidual is the masked gradient g."""
    dy, x, gamma = _f64(dy), _f64(x), _f64(gamma)
    n = x.shape[0]
    mean, _, rstd = batch_stats(x, eps)
    xhat = (x - mean) * rstd
    g = np.where(np.asarray(y) > 0, dy, 0.0) if relu else dy
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    dx = gamma * rstd * (g - dbeta / n - xhat * dgamma / n)
    return dict(g=g, xhat=xhat, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta, dresidual=g)
