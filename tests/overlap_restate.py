"""The fragment overlap of data/compute_overlap.py:93-141 restated in NumPy, as csrc/overlap.hip pins it:

    for every point j of q (ascending):
        d2[i] = (dx * dx + dy * dy) + dz * dz      float32 arrays, one rounding per operation (NumPy fuses nothing)
        i* = argmin d2                             (np.argmin returns the lowest index among equal minima)
        keep (i*, j) when sqrt(d2[i*]) <= float32(thresh)
    ratio = rows / max(n_p, n_q)

`nearest` is the brute force over all of p.  `nearest_windowed` gives the same rows from less work: q is walked in
blocks sorted along one axis, and a block only looks at the points of p whose coordinate on that axis lies within
`window` of the block's range.  A point of p outside the window is farther than `window` > thresh from every query of
the block along that axis alone, so it can be no kept neighbour; where the window's nearest point is beyond thresh the
row is dropped, as it would be with the true nearest one (which is at least as far)."""
import numpy as np

from imfnet_amd.overlap import candidate_pairs, downsample, overlap_ratio   # noqa: F401  (one definition, shared)


def _block(p, q):
    """(argmin index, min d2) of every row of q over all of p; float32 throughout."""
    d = p[None, :, :] - q[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    i = np.argmin(d2, axis=1)
    return i, d2[np.arange(len(q)), i]


def nearest(p, q, block=256):
    """int64 [n_q] nearest index in p and float32 [n_q] its d2."""
    p, q = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(q, np.float32)
    idx, d2 = np.zeros(len(q), np.int64), np.zeros(len(q), np.float32)
    for b in range(0, len(q), block):
        idx[b:b + block], d2[b:b + block] = _block(p, q[b:b + block])
    return idx, d2


def correspondences(p, q, thresh, idx_d2=None):
    """int64 [n,2] rows (index in p, index in q), ascending in q."""
    idx, d2 = nearest(p, q) if idx_d2 is None else idx_d2
    keep = np.sqrt(d2) <= np.float32(thresh)
    assert np.sqrt(d2).dtype == np.float32
    return np.stack([idx[keep], np.nonzero(keep)[0]], axis=1).astype(np.int64)


def nearest_windowed(p, q, thresh, block=512, window=None):
    """(idx, d2, valid): as `nearest` wherever a point of p lies inside the block's window; valid False elsewhere
    (no neighbour within thresh can exist there)."""
    p, q = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(q, np.float32)
    window = 1.25 * float(thresh) if window is None else window
    assert window > float(thresh) * 1.001
    axis = int(np.argmax(np.ptp(np.concatenate([p, q]).astype(np.float64), axis=0))) if len(p) and len(q) else 0
    po = np.argsort(p[:, axis], kind="stable")
    pk = p[po, axis].astype(np.float64)
    qo = np.argsort(q[:, axis], kind="stable")
    idx, d2, valid = np.zeros(len(q), np.int64), np.full(len(q), np.inf, np.float32), np.zeros(len(q), bool)
    for b in range(0, len(q), block):
        rows = qo[b:b + block]
        qk = q[rows, axis].astype(np.float64)
        lo, hi = np.searchsorted(pk, qk.min() - window, "left"), np.searchsorted(pk, qk.max() + window, "right")
        if hi <= lo:
            continue
        cand = np.sort(po[lo:hi])                            # ascending original index: argmin's tie rule carries over
        i, d = _block(p[cand], q[rows])
        idx[rows], d2[rows], valid[rows] = cand[i], d, True
    return idx, d2, valid


def correspondences_windowed(p, q, thresh):
    idx, d2, valid = nearest_windowed(p, q, thresh)
    keep = valid & (np.sqrt(d2) <= np.float32(thresh))
    return np.stack([idx[keep], np.nonzero(keep)[0]], axis=1).astype(np.int64)


def sequence_overlap(clouds, thresh=0.075, min_overlap=0.3, numbers=None, counts=None, pair_fn=correspondences_windowed):
    """{(i, j): (ratio, rows)} of the kept pairs; `counts` (a dict) receives every candidate pair's row count."""
    clouds = [np.ascontiguousarray(c, np.float32) for c in clouds]
    numbers = list(range(len(clouds))) if numbers is None else list(numbers)
    out = {}
    for i, j in candidate_pairs(numbers):
        if not len(clouds[i]) or not len(clouds[j]):
            continue
        rows = pair_fn(clouds[i], clouds[j], thresh)
        if counts is not None:
            counts[(i, j)] = len(rows)
        ratio = overlap_ratio(len(rows), len(clouds[i]), len(clouds[j]))
        if ratio < min_overlap:
            continue
        out[(i, j)] = (ratio, rows)
    return out


def cell_bound(p, q, cell):
    """The prefilter restated: the points of q whose cell (floor(x / cell) in float64) has an occupied cell of p among
    its 27 neighbours."""
    cp = {tuple(c) for c in np.floor(np.asarray(p, np.float64) * (1.0 / cell)).astype(np.int64).tolist()}
    cq, cnt = np.unique(np.floor(np.asarray(q, np.float64) * (1.0 / cell)).astype(np.int64), axis=0, return_counts=True)
    total = 0
    for (x, y, z), c in zip(cq.tolist(), cnt.tolist()):
        if any((x + dx, y + dy, z + dz) in cp for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)):
            total += c
    return total


def slab_sequence(cloud, max_points=30000):
    """The GPU test's sequence: fragments cut from one cloud as overlapping slabs along its longest axis (bounds as
    quantiles of that axis), each sub-sampled with its own seed so that no two share all their points; the last slab
    holds more than max_points and is down-sampled.  Returns (float32 clouds, fragment numbers)."""
    cloud = np.asarray(cloud)
    axis = int(np.argmax(np.ptp(cloud.astype(np.float64), axis=0)))
    order = np.argsort(cloud[:, axis], kind="stable")
    n = len(cloud)
    clouds = []
    for k, (lo, hi, share) in enumerate(SLABS):
        rows = order[int(lo * n):int(hi * n)]
        rng = np.random.default_rng(100 + k)
        rows = np.sort(rng.choice(rows, int(share * len(rows)), replace=False))
        clouds.append(downsample(cloud[rows], max_points, (0, "slabs", k))[0])
    return clouds, list(range(len(SLABS)))


# (lower quantile, upper quantile, share of the slab's points kept)
SLABS = [(0.00, 0.40, 0.28), (0.05, 0.45, 0.28), (0.20, 0.60, 0.28), (0.30, 0.66, 0.28), (0.52, 0.90, 0.28),
         (0.31, 0.75, 0.25), (0.70, 1.00, 0.30), (0.55, 1.00, 0.30)]
