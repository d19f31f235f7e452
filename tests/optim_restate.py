"""NumPy restatement of csrc/optim.hip: the SGD step with its three roundings, and the two bf16x3 weight images through the
documented index formula (include/imfnet_hip.h, csrc/weight_image.h).  No GPU, no library call."""
import numpy as np


def sgd_step(p, g, b, lr, momentum, weight_decay, first, dtype=np.float32):
    """(p', b') of one step, every operation rounded once in `dtype`:
         d = g + wd p (wd == 0: d = g);  b' = mu b + d (first step or mu == 0: b' = d);  p' = p - lr b'.
    b may be None on the first step; b' is None when momentum == 0 (torch keeps no buffer)."""
    T = np.dtype(dtype).type
    p, g = np.asarray(p, dtype=dtype), np.asarray(g, dtype=dtype)
    lr, mu, wd = T(lr), T(momentum), T(weight_decay)
    d = g
    if wd != 0:
        t = wd * p
        d = g + t
    bn = d
    if mu != 0 and not first:
        t = mu * np.asarray(b, dtype=dtype)
        bn = t + d
    t = lr * bn
    pn = p - t
    assert pn.dtype == np.dtype(dtype) and bn.dtype == np.dtype(dtype)
    return pn, (bn.copy() if mu != 0 else None)


def bf16_bits(x):
    """float32 -> bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split_b3(x):
    """x = p0 + p1 + p2 exactly: p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1), as bit patterns."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    p0 = bf16_bits(x)
    r1 = x - bf16_value(p0)
    p1 = bf16_bits(r1)
    p2 = bf16_bits(r1 - bf16_value(p1))
    return p0, p1, p2


def image_b3(k3):
    """The bf16x3 image of a kernel [kvol, cin, cout] (cin % 32 == 0, cout % 32 == 0) as uint16 [kvol cin cout 3]:
    [y][k][cc][q = 3 cb + part][lane][t], ci = 32 cc + 16 (t >> 2) + 4 (lane >> 4) + (t & 3), co = y CW + 16 cb + (lane & 15),
    CB = 4 when cout % 64 == 0 else 2, CW = 16 CB."""
    k3 = np.ascontiguousarray(k3, dtype=np.float32)
    kvol, cin, cout = k3.shape
    assert cin % 32 == 0 and cout % 32 == 0
    CB = 4 if cout % 64 == 0 else 2
    CW, ncc = 16 * CB, cin // 32
    out = np.zeros(kvol * cin * cout * 3, dtype=np.uint16)
    k, ci, co = np.meshgrid(np.arange(kvol), np.arange(cin), np.arange(cout), indexing="ij")
    y, cb, cc, c32 = co // CW, (co % CW) // 16, ci // 32, ci % 32
    lane = ((c32 % 16) // 4) * 16 + co % 16
    t = (c32 // 16) * 4 + c32 % 4
    q0 = ((((y * kvol + k) * ncc + cc) * (3 * CB) + 3 * cb) * 64 + lane).astype(np.int64)
    for part, bits in enumerate(split_b3(k3)):
        out[(q0 + 64 * part) * 8 + t] = bits
    return out


def me_backward_source(kernel, flip):
    """The tensor autograd.SparseConvFunction packs for the input gradient: transpose(1, 2) [+ flip(0)] of [kvol, cin, cout]."""
    k3 = kernel if kernel.ndim == 3 else kernel[None]
    wt = k3.transpose(0, 2, 1)
    return np.ascontiguousarray(wt[::-1] if flip else wt)


def torch_forward_source(weight):
    co, ci, kh, kw = weight.shape
    return np.ascontiguousarray(weight.transpose(2, 3, 1, 0).reshape(kh * kw, ci, co))


def torch_backward_source(weight, flip):
    """autograd.DenseConvFunction's: permute(2, 3, 0, 1).reshape(kvol, cout, cin) [+ flip(0)] of [cout, cin, kh, kw]."""
    co, ci, kh, kw = weight.shape
    wt = weight.transpose(2, 3, 0, 1).reshape(kh * kw, co, ci)
    return np.ascontiguousarray(wt[::-1] if flip else wt)
