"""Float64 NumPy restatement of imf_fpfh_features (csrc/fpfh.hip) and the catalogue of point sets its tests share.
Plain helper module: tests/test_fpfh_host.py proves it on the CPU, tests/test_gpu_fpfh.py runs the kernels against it.
No GPU dependency.

The rules restated (every product and sum rounds one by one, NumPy never fuses): the neighbours of point i are the first
counts[i] entries of nbr[i] minus every entry equal to i (and anything outside [0, n)), m_i of them.  Pair (i, j):
d = p_j - p_i, d2 = (dx*dx + dy*dy) + dz*dz, L = sqrt(d2); L == 0 gives three zero features; a1 = (n_i . d) / L,
a2 = (n_j . d) / L; |a1| < |a2| swaps the roles (n1 = n_j, n2 = n_i, d = -d, f2 = -a2), otherwise n1 = n_i, n2 = n_j,
f2 = a1; v = d x n1, |v| == 0 gives three zero features, else v /= |v|; w = n1 x v, f1 = v . n2,
f0 = atan2(w . n2, n1 . n2).  Bins: floor of 11 (f0 + pi) / (2 pi), 11 (f1 + 1) / 2 and 11 (f2 + 1) / 2, clamped to 0..10,
in three groups of 11.  cnt_i = the pairs per bin, spfh_i = cnt_i * (100 / m_i).  acc_i = the sum over the neighbours with
d2 != 0, in list order, of spfh_j / d2; S = the group sums in ascending bin order;
out = (S != 0 ? acc * (100 / S) : 0) + spfh_i.

A pair is *undecided* when one of its three scaled features is closer than EDGE to an integer (the device's atan2, sqrt
or division may differ from libm in the last place there); a point is *clean* when neither it nor any of its neighbours
has an undecided pair."""
import os
from typing import NamedTuple, Optional

import numpy as np

import normals_restate as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = 1e-9
BINS = 33
VIEWPOINT = np.zeros(3)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def restate(points, normals, nbr, counts):
    """dict(valid bool [n, knn], m int [n], hist int32 [n, 33], spfh, out float64 [n, 33], gap float64 [n, knn, 3] (the
    distance of every pair's scaled features to the nearest integer), undecided bool [n, knn], clean bool [n])."""
    pts, nrm = np.asarray(points, np.float64), np.asarray(normals, np.float64)
    nbr, counts = np.asarray(nbr), np.asarray(counts)
    n, knn = nbr.shape
    rows = np.arange(n)[:, None]
    valid = (np.arange(knn)[None, :] < counts[:, None]) & (nbr >= 0) & (nbr < n) & (nbr != rows)
    j = np.where(valid, nbr, 0)
    ni, nj = np.broadcast_to(nrm[:, None, :], (n, knn, 3)), nrm[j]
    d = pts[j] - pts[:, None, :]
    d2 = _dot(d, d)
    L = np.sqrt(d2)
    Ls = np.where(L == 0.0, 1.0, L)
    a1, a2 = _dot(ni, d) / Ls, _dot(nj, d) / Ls
    swap = np.abs(a1) < np.abs(a2)
    n1, n2 = np.where(swap[..., None], nj, ni), np.where(swap[..., None], ni, nj)
    ds = np.where(swap[..., None], -d, d)
    v = _cross(ds, n1)
    vl = np.sqrt(_dot(v, v))
    zero = (L == 0.0) | (vl == 0.0)
    v = v / np.where(zero, 1.0, vl)[..., None]
    w = _cross(n1, v)
    f0 = np.where(zero, 0.0, np.arctan2(_dot(w, n2), _dot(n1, n2)))
    f1 = np.where(zero, 0.0, _dot(v, n2))
    f2 = np.where(zero, 0.0, np.where(swap, -a2, a1))
    t = np.stack([(11.0 * (f0 + np.pi)) / (2.0 * np.pi), (11.0 * (f1 + 1.0)) * 0.5, (11.0 * (f2 + 1.0)) * 0.5], -1)
    bins = np.clip(np.floor(t), 0.0, 10.0).astype(np.int64) + np.array([0, 11, 22])
    gap = np.abs(t - np.rint(t))
    undecided = valid & (gap < EDGE).any(-1)

    hist = np.zeros((n, BINS), np.int32)
    for k in range(3):
        np.add.at(hist, (np.broadcast_to(rows, (n, knn))[valid], bins[..., k][valid]), 1)
    m = valid.sum(1)
    scale = np.where(m > 0, 100.0 / np.maximum(m, 1), 0.0)
    spfh = hist.astype(np.float64) * scale[:, None]

    acc = np.zeros((n, BINS))
    for e in range(knn):                                               # in list order, one after the other
        use = valid[:, e] & (d2[:, e] != 0.0)
        term = spfh[j[:, e]] / np.where(use, d2[:, e], 1.0)[:, None]
        acc = np.where(use[:, None], acc + term, acc)
    S = np.zeros((n, 3))
    for k in range(11):                                                # ascending bin order
        S = S + acc[:, k::11][:, :3]
    Sb = np.repeat(S, 11, axis=1)
    out = np.where(Sb != 0.0, acc * (100.0 / np.where(Sb != 0.0, Sb, 1.0)), 0.0) + spfh

    bad = undecided.any(1)
    clean = ~bad & ~(valid & bad[j]).any(1)
    return dict(valid=valid, m=m, hist=hist, spfh=spfh, acc=acc, out=out, gap=gap, undecided=undecided, clean=clean)


def neighbors(points, knn, max_radius):
    """The lists of imf_estimate_normals on the CPU: normals_restate.neighbors by brute force for a small set, cKDTree
    candidates re-sorted by the restated (d^2, index) for a large one (16 spare candidates cover a group of equal d^2 across
    the last place)."""
    pts = np.asarray(points, np.float64)
    n = len(pts)
    if n <= 2048:
        return NR.neighbors(pts, knn, max_radius)
    from scipy.spatial import cKDTree
    K = min(n, knn + 16)
    _, j = cKDTree(pts).query(pts, k=K, distance_upper_bound=max_radius * (1 + 1e-9))
    j = j.reshape(n, K)
    found = j < n
    e = pts[np.where(found, j, 0)] - pts[:, None, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    d2 = np.where(found & (d2 <= max_radius * max_radius), d2, np.inf)
    by_index = np.argsort(j, axis=1, kind="stable")
    j, d2 = np.take_along_axis(j, by_index, 1), np.take_along_axis(d2, by_index, 1)
    by_d2 = np.argsort(d2, axis=1, kind="stable")[:, :knn]
    j, d2 = np.take_along_axis(j, by_d2, 1), np.take_along_axis(d2, by_d2, 1)
    ok = np.isfinite(d2)
    nbr = np.full((n, knn), -1, np.int32)
    nbr[:, :j.shape[1]] = np.where(ok, j, -1)
    return nbr, ok.sum(1).astype(np.int32)


# ---- the cases ---------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    points: np.ndarray
    knn: int                    # max_nn of the lists
    radius: float
    normals: Optional[np.ndarray]   # given, or None = estimate_normals(knn=30, max_radius=radius, viewpoint=origin)


def fixture_points():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))
    return z["cloud_bin_0"][::16].astype(np.float64)


def cases():
    rng = np.random.default_rng(11)
    out = []
    uv = rng.uniform(-0.5, 0.5, (1500, 2))
    patch = np.concatenate([uv, np.sqrt(4.0 - (uv ** 2).sum(1))[:, None]], 1) + rng.normal(0.0, 0.004, (1500, 3))
    out.append(Case("curved_patch_knn64", patch, 64, 0.15, None))              # ~100 points in the radius: full lists
    out.append(Case("curved_patch_knn16_padded", patch, 16, 0.04, None))       # ~7 in the radius: lists padded with -1
    g = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), indexing="ij"), -1).reshape(-1, 2)
    lattice = np.concatenate([g, np.full((400, 1), 2.0)], 1)[rng.permutation(400)]
    out.append(Case("lattice_identical_normals", lattice, 16, 2.5, np.tile([[0.0, 0.0, 1.0]], (400, 1))))
    base = patch[:300]
    dup = np.concatenate([base, base[rng.integers(0, 300, 120)], base[:30]])
    out.append(Case("exact_duplicates", dup[rng.permutation(len(dup))], 16, 0.3, None))
    blob = rng.uniform(0.0, 0.5, (200, 3))
    out.append(Case("lonely_point", np.concatenate([blob, [[9.0, 9.0, 9.0]]]), 32, 0.3, None))
    trio = np.array([[5.0, 5.0, 5.0], [5.1, 5.02, 5.0], [5.03, 5.12, 5.05]])
    out.append(Case("isolated_trio", np.concatenate([blob, trio]), 32, 0.3, None))
    axis = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.25], [0.2, 0.1, 0.05], [0.1, -0.2, 0.3]])
    slant = np.array([0.3, -0.2, 0.9]) / np.linalg.norm([0.3, -0.2, 0.9])
    out.append(Case("normal_parallel_to_d", axis, 8, 1.0, np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], slant, [0.0, 1.0, 0.0]])))
    out.append(Case("fixture_every_16th", fixture_points(), 64, 0.125, None))
    return out


_REF = {}


def host_inputs(case):
    """(normals, nbr, counts) of a case from the CPU restatements alone, computed once per process."""
    if case.name not in _REF:
        nbr, counts = neighbors(case.points, case.knn, case.radius)
        nrm = case.normals
        if nrm is None:
            nn, nc = neighbors(case.points, 30, case.radius)
            nrm = NR.orient(NR.jacobi_smallest(NR.covariances(case.points, nn, nc)), case.points, nc, VIEWPOINT)
        _REF[case.name] = (nrm, nbr, counts)
    return _REF[case.name]


_HOST = {}


def host_reference(case):
    """The restatement of a case on the CPU's own lists and normals, computed once per process and left unchanged."""
    if case.name not in _HOST:
        nrm, nbr, counts = host_inputs(case)
        _HOST[case.name] = restate(case.points, nrm, nbr, counts)
    return _HOST[case.name]
