"""The sparse convolution and its two gradients restated in float64, plus the data and the kernel maps the backward tests
run on (tests/test_backward_host.py on the CPU, tests/test_gpu_backward_exact.py against csrc/backward.hip and
imfnet_amd/autograd.py).

    out[o] = sum_k feat[nbr[o, k]] @ W[k]            over the pairs (i = nbr[o, k] >= 0, o) of every offset k
    dX[i] += g[o] @ W[k]^T                           the same pairs
    dW[k]  = sum over the pairs of feat[i]^T g[o]

Integer data (features in [-3, 3], weights in [-2, 2], gradients in [-3, 3], stored as float32): every product and every
partial sum is an integer far below 2^24, so ANY correct fp32-accumulating kernel returns exactly the integers float64
returns here, in any summation order and in any of the three arithmetics (bf16x3 and split-f16 carry such operands in their
first part).  The comparison is torch.equal; one missing, duplicated or misrouted pair changes the result.  A power-of-two
scale of an operand is an exponent shift and keeps all of it exact.  Operands whose LATER parts carry bits (the f16 lo
half, bf16x3's second and third part) and still sum exactly: the generators of tests/spconv_cases.py.

Kernel maps come in two shapes: the oracle's `nbr [n_out, K]` (row of the input per output row and offset, -1 = none) and
the library's tiled one (`tile_rows [n_slots]` = output row of every slot, -1 = padding; `nbr [K, n_slots]`), see
include/imfnet_hip.h."""
import numpy as np
import torch

EXACT_LIMIT = 1 << 24            # integers of smaller magnitude are exact in float32, and so are their sums below it


def int_tensor(gen, shape, bound):
    """float32 tensor of integers drawn uniformly from [-bound, bound] (torch.Generator `gen`)."""
    return torch.randint(-bound, bound + 1, tuple(shape), generator=gen).to(torch.float32)


def int_case(gen, n_in, n_out, kvol, cin, cout):
    """(feat [n_in, cin] in [-3, 3], W [kvol, cin, cout] in [-2, 2], grad_out [n_out, cout] in [-3, 3])."""
    return int_tensor(gen, (n_in, cin), 3), int_tensor(gen, (kvol, cin, cout), 2), int_tensor(gen, (n_out, cout), 3)


def _pairs(nbr, k, n_out):
    if nbr is None:                                   # 1x1x1: out row o reads in row o
        o = torch.arange(n_out)
        return o, o
    col = torch.as_tensor(np.asarray(nbr)[:, k].astype(np.int64))
    o = torch.nonzero(col >= 0).squeeze(1)
    return col[o], o


def conv_restate(feat, W, grad_out, nbr, n_in=None):
    """float64 (out [n_out, cout], dX [n_in, cin], dW [K, cin, cout]).  W [K, cin, cout] or [cin, cout]; nbr [n_out, K]
    or None (K == 1, identity).  `grad_out` None: only `out`."""
    feat, W = torch.as_tensor(feat).double(), torch.as_tensor(W).double()
    W = W.unsqueeze(0) if W.dim() == 2 else W
    n_out = feat.shape[0] if nbr is None else np.asarray(nbr).shape[0]
    out = torch.zeros(n_out, W.shape[2], dtype=torch.float64)
    for k in range(W.shape[0]):
        i, o = _pairs(nbr, k, n_out)
        out.index_add_(0, o, feat[i] @ W[k])
    if grad_out is None:
        return out
    g = torch.as_tensor(grad_out).double()
    dX = torch.zeros(feat.shape[0] if n_in is None else n_in, W.shape[1], dtype=torch.float64)
    dW = torch.zeros_like(W)
    for k in range(W.shape[0]):
        i, o = _pairs(nbr, k, n_out)
        dX.index_add_(0, i, g[o] @ W[k].t())
        dW[k] = feat[i].t() @ g[o]
    return out, dX, dW


def wgrad_abs_sum(feat, grad_out, nbr):
    """(S [K, cin, cout] = the float64 sum of |in| * |grad| over every element's pairs, n_k [K] = pairs per offset):
    the terms of the any-order summation bound on dW."""
    fa, ga = torch.as_tensor(feat).double().abs(), torch.as_tensor(grad_out).double().abs()
    K = 1 if nbr is None else np.asarray(nbr).shape[1]
    S = torch.zeros(K, fa.shape[1], ga.shape[1], dtype=torch.float64)
    n_k = np.zeros(K, np.int64)
    for k in range(K):
        i, o = _pairs(nbr, k, ga.shape[0])
        S[k] = fa[i].t() @ ga[o]
        n_k[k] = len(o)
    return S, n_k


def magnitude_bounds(nbr, n_in, cin, cout, feat_bound=3, w_bound=2, grad_bound=3):
    """A-priori ceilings of |out|, |dX|, |dW| (and of every partial sum on the way) for integer data within the given
    bounds on this map: (pairs per output row) * cin * 3 * 2, (pairs per input row) * cout * 3 * 2, (pairs of the fullest
    offset) * 3 * 3.  The exactness argument needs all three below EXACT_LIMIT."""
    if nbr is None:
        return cin * feat_bound * w_bound, cout * grad_bound * w_bound, n_in * feat_bound * grad_bound
    nbr = np.asarray(nbr)
    hit = nbr >= 0
    per_in = np.bincount(nbr[hit].astype(np.int64), minlength=n_in).max() if hit.any() else 0
    return (int(hit.sum(1).max()) * cin * feat_bound * w_bound, int(per_in) * cout * grad_bound * w_bound,
            int(hit.sum(0).max()) * feat_bound * grad_bound)


# ---- the two map shapes ----------------------------------------------------------------------------------------------
def tiled_to_rows(tile_rows, nbr_tiled, n_out):
    """Tiled map -> [n_out, K].  tile_rows None: slot == row.  Every row must sit in exactly one slot."""
    nbr_tiled = np.asarray(nbr_tiled)
    K, n_slots = nbr_tiled.shape
    tr = np.where(np.arange(n_slots) < n_out, np.arange(n_slots), -1) if tile_rows is None else np.asarray(tile_rows)
    slots = np.nonzero(tr >= 0)[0]
    assert np.array_equal(np.sort(tr[slots]), np.arange(n_out)), "a row is missing from the slots, or sits in two"
    rows = np.full((n_out, K), -1, np.int32)
    rows[tr[slots]] = nbr_tiled[:, slots].T
    return rows


def rows_to_tiled(nbr_rows, n_slots, tile_rows=None):
    """[n_out, K] -> (tile_rows int32 [n_slots], nbr int32 [K, n_slots]).  tile_rows: a slot order to follow (default:
    the identity, padding last); padding slots carry -1 in every offset."""
    nbr_rows = np.asarray(nbr_rows)
    n_out, K = nbr_rows.shape
    assert n_slots >= n_out
    if tile_rows is None:
        tile_rows = np.where(np.arange(n_slots) < n_out, np.arange(n_slots), -1)
    tile_rows = np.asarray(tile_rows, np.int32)
    nbr = np.full((K, n_slots), -1, np.int32)
    used = tile_rows >= 0
    nbr[:, used] = nbr_rows[tile_rows[used]].T
    return tile_rows, nbr


def synthetic_map(gen, n_out, n_in, kvol, n_slots=None, density=0.3, permute=False, empty_offsets=()):
    """A random kernel map in both shapes: (nbr_rows [n_out, kvol], tile_rows [n_slots], nbr_tiled [kvol, n_slots]).
    Every (row, offset) holds an input row with probability `density`; the offsets of `empty_offsets` hold none.
    n_slots defaults to n_out rounded up to 64 (the library's tile); a larger value adds padding slots.  `permute`
    shuffles the slots, padding included, so that padding lies between rows (the occupancy-sorted maps do that)."""
    rng = np.random.default_rng(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen)))
    n_slots = (n_out + 63) // 64 * 64 if n_slots is None else n_slots
    nbr_rows = np.where(rng.random((n_out, kvol)) < density, rng.integers(0, n_in, (n_out, kvol)), -1).astype(np.int32)
    nbr_rows[:, list(empty_offsets)] = -1
    tile_rows = np.where(np.arange(n_slots) < n_out, np.arange(n_slots), -1)
    if permute:
        tile_rows = tile_rows[rng.permutation(n_slots)]
    tile_rows, nbr_tiled = rows_to_tiled(nbr_rows, n_slots, tile_rows)
    return nbr_rows, tile_rows, nbr_tiled


# ---- the opposite map: where the input gradient is a forward convolution ---------------------------------------------
def opposite(W, kind, geometry, level):
    """(W', map) with dX = conv(grad_out, W', map), as imfnet_amd/autograd.py documents it.  kind: "k3" / "k5" (stride 1
    at `level`: the same map, W'[k] = W[K-1-k]^T), "down" (level -> level + 1: the transposed map, W'[k] = W[k]^T),
    "up" (level + 1 -> level: the strided map, W'[k] = W[k]^T)."""
    Wt = torch.as_tensor(W).transpose(1, 2)
    if kind == "k3":
        return Wt.flip(0), geometry.k3[level]
    if kind == "k5":
        return Wt.flip(0), geometry.k_first
    if kind == "down":
        return Wt, geometry.up[level]
    assert kind == "up"
    return Wt, geometry.down[level]


def layer_map(geometry, transposed, ksize, stride, ts):
    """The oracle map of one convolution layer whose INPUT lives at tensor stride `ts`:
    (nbr or None, kind and level for `opposite`, n_in, n_out)."""
    lv = int(ts).bit_length() - 1
    assert 1 << lv == ts
    n = [len(c) for c in geometry.levels]
    if ksize == 1:
        assert stride == 1
        return None, "k1", lv, n[lv], n[lv]
    if transposed:
        assert ksize == 3 and stride == 2 and lv >= 1
        return geometry.up[lv - 1], "up", lv - 1, n[lv], n[lv - 1]
    if stride == 2:
        assert ksize == 3
        return geometry.down[lv], "down", lv, n[lv], n[lv + 1]
    if ksize == 5:
        assert lv == 0 and geometry.k_first.shape[1] == 125
        return geometry.k_first, "k5", 0, n[0], n[0]
    assert ksize == 3
    return geometry.k3[lv], "k3", lv, n[lv], n[lv]


def batched_voxels(point_sets, voxel):
    """What one training batch is made of: per item the voxel representatives (float64 points, first occurrence order),
    and the oracle's batched coordinates int32 [M, 4] of all items, rows grouped by item."""
    import imf_oracle as O
    reps, coords = [], []
    for b, xyz in enumerate(point_sets):
        xyz = np.asarray(xyz, np.float64)
        c, inds = O.voxelize(xyz, voxel, batch_index=b)
        reps.append(xyz[inds])
        coords.append(c)
    return reps, np.concatenate(coords)


def inner_products(feat, W, grad_out, out, dX, dW):
    """The three sums that one convolution makes equal: <conv(x), g>, <x, dX>, <W, dW>; as exact Python integers."""
    def dot(a, b):
        return int((torch.as_tensor(a).double().cpu().reshape(-1) * torch.as_tensor(b).double().cpu().reshape(-1)).sum())
    return dot(out, grad_out), dot(feat, dX), dot(W, dW)
