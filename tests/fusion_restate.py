"""Float64 NumPy restatement of the two calls of csrc/fusion_train.hip (imf_fusion_train_forward /
imf_fusion_train_backward): model/fusion.py's AttentionFusion with depth 0, one head and no mask, every batch item at
once, and its closed-form backward.  The parameters are a list in the order of ops.FUSION_TRAIN_PARAMS (the C ABI's
IMF_FT_* indices); `starts` are the items' ascending row starts, len(tokens) + 1 of them."""
import math

import numpy as np

try:
    from scipy.special import erf as _erf
except ImportError:                                     # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])

(LN1_G, LN1_B, LNC_G, LNC_B, WQ, WKV, WO, BO, LN2_G, LN2_B, W1, B1, W2, B2) = range(14)
EPS = 1e-5
INNER, HIDDEN = 128, 1024
SCALE = INNER ** -0.5


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _ln(x, g, b):
    mean = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(-1, keepdims=True) + EPS)
    xh = (x - mean) * rstd
    return xh * g + b, xh, rstd


def _ln_bwd(dn, xh, rstd, g):
    """(dx, dgamma, dbeta) of n = xh * g + b."""
    gg = dn * g
    dx = rstd * (gg - gg.mean(-1, keepdims=True) - xh * (gg * xh).mean(-1, keepdims=True))
    lead = tuple(range(dn.ndim - 1))
    return dx, (dn * xh).sum(lead), dn.sum(lead)


def forward_from_kv(x, starts, k, v, params):
    """(z [n, 256], the intermediates) of everything after K / V: k, v [B, T, 128] as given (the inference entry points of
    csrc/fusion.hip take them packed); the context LayerNorm and to_kv parameters of `params` are not read."""
    x, k, v = _f64(x), _f64(k), _f64(v)
    P = [_f64(p) for p in params]
    starts = [int(s) for s in starts]
    B, T, _ = k.shape
    assert v.shape == k.shape and len(starts) == B + 1 and starts[0] == 0 and starts[-1] == x.shape[0]
    n1, xh1, rstd1 = _ln(x, P[LN1_G], P[LN1_B])
    q = n1 @ P[WQ].T
    p = np.zeros((x.shape[0], T))
    o = np.zeros((x.shape[0], INNER))
    for b in range(B):
        r = slice(starts[b], starts[b + 1])
        s = q[r] @ k[b].T * SCALE
        e = np.exp(s - s.max(-1, keepdims=True)) if s.shape[0] else s
        p[r] = e / e.sum(-1, keepdims=True) if s.shape[0] else e
        o[r] = p[r] @ v[b]
    y = o @ P[WO].T + P[BO] + x
    n2, xh2, rstd2 = _ln(y, P[LN2_G], P[LN2_B])
    h = n2 @ P[W1].T + P[B1]
    a, g = h[:, :HIDDEN], h[:, HIDDEN:]                          # value first, gate second
    cdf = 0.5 * (1.0 + _erf(g / math.sqrt(2.0)))
    u = a * (g * cdf)
    z = u @ P[W2].T + P[B2] + y
    return z, dict(P=P, starts=starts, k=k, v=v, n1=n1, xh1=xh1, rstd1=rstd1, q=q, p=p, o=o, xh2=xh2, rstd2=rstd2, n2=n2,
                   a=a, g=g, cdf=cdf, u=u)


def forward(x, starts, tokens, params):
    """z [n, 256] and the cache for `backward`."""
    tokens = _f64(tokens)
    P = [_f64(p) for p in params]
    assert len(starts) == tokens.shape[0] + 1
    c, ch, crstd = _ln(tokens, P[LNC_G], P[LNC_B])
    kv = c @ P[WKV].T
    k, v = kv[..., :INNER], kv[..., INNER:]                      # K first, V second
    z, cache = forward_from_kv(x, starts, k, v, P)
    cache.update(c=c, ch=ch, crstd=crstd, tokens_shape=tokens.shape)
    return z, cache


def backward(dz, cache):
    """(dx [n, 256], dtokens [B, T, 128], [14 parameter gradients]) for the incoming gradient dz of z."""
    dz = _f64(dz)
    C = cache
    P, starts = C["P"], C["starts"]
    B, T, _ = C["tokens_shape"]
    G = [None] * 14
    G[B2], G[W2] = dz.sum(0), dz.T @ C["u"]
    du = dz @ P[W2]
    g, a, cdf = C["g"], C["a"], C["cdf"]
    pdf = np.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    dh = np.concatenate([du * (g * cdf), du * a * (cdf + g * pdf)], axis=1)
    G[B1], G[W1] = dh.sum(0), dh.T @ C["n2"]
    dy_ln, G[LN2_G], G[LN2_B] = _ln_bwd(dh @ P[W1], C["xh2"], C["rstd2"], P[LN2_G])
    dy = dz + dy_ln
    G[BO], G[WO] = dy.sum(0), dy.T @ C["o"]
    do = dy @ P[WO]
    dq = np.zeros_like(C["q"])
    dk, dv = np.zeros_like(C["k"]), np.zeros_like(C["v"])
    for b in range(B):
        r = slice(starts[b], starts[b + 1])
        p = C["p"][r]
        dv[b] = p.T @ do[r]
        dp = do[r] @ C["v"][b].T
        ds = p * (dp - (p * dp).sum(-1, keepdims=True)) * SCALE
        dq[r] = ds @ C["k"][b]
        dk[b] = ds.T @ C["q"][r]
    G[WQ] = dq.T @ C["n1"]
    dx_ln, G[LN1_G], G[LN1_B] = _ln_bwd(dq @ P[WQ], C["xh1"], C["rstd1"], P[LN1_G])
    dx = dy + dx_ln
    dkv = np.concatenate([dk, dv], axis=-1)
    G[WKV] = dkv.reshape(B * T, -1).T @ C["c"].reshape(B * T, -1)
    dtok, G[LNC_G], G[LNC_B] = _ln_bwd(dkv @ P[WKV], C["ch"], C["crstd"], P[LNC_G])
    return dx, dtok, G
