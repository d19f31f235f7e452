"""Float64 NumPy restatement of imf_estimate_normals (csrc/normals.hip) and the catalogue of point sets its tests share.
Plain helper module: tests/test_normals_host.py proves it on the CPU (cKDTree, numpy.linalg.eigh),
tests/test_gpu_normals.py runs the kernel against it.  No GPU dependency.

The rules restated: the neighbour set of point i is the knn smallest of (d^2, index) among the points with
d^2 <= max_radius^2, itself included, d^2 = (ex*ex + ey*ey) + ez*ez rounded step by step (NumPy never fuses); the normal is
the eigenvector of the smallest eigenvalue of the two-pass covariance, by cyclic Jacobi with the kernel's sweep rule; fewer
than 3 points give (0, 0, 1), unsigned; otherwise the sign faces the viewpoint, or makes the largest component positive."""
import os
from typing import NamedTuple, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-3                  # (l1 - l0) / l2 from which the direction is compared
VIEWPOINT = np.array([0.3, -0.2, 5.0])


def dist2(p, q):
    """[len(p), len(q)] squared distances as the kernel forms them."""
    e = q[None, :, :] - p[:, None, :]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def neighbors(points, knn, max_radius):
    """(nbr int32 [n, knn] padded with -1, counts int32 [n]) by brute force."""
    pts = np.asarray(points, np.float64)
    n, r2 = len(pts), max_radius * max_radius
    nbr = np.full((n, knn), -1, np.int32)
    counts = np.zeros(n, np.int32)
    k = min(knn, n)
    for a in range(0, n, 512):
        D = dist2(pts[a:a + 512], pts)
        D = np.where(D <= r2, D, np.inf)                               # NaN compares false
        order = np.argsort(D, axis=1, kind="stable")[:, :k]            # stable: equal d^2 by ascending index
        ok = np.isfinite(np.take_along_axis(D, order, 1))
        nbr[a:a + 512, :k] = np.where(ok, order, -1)
        counts[a:a + 512] = ok.sum(1)
    return nbr, counts


def covariances(points, nbr, counts):
    """[n, 3, 3] two-pass covariance of every set, in list order (zeros for an empty set)."""
    pts = np.asarray(points, np.float64)
    mask = nbr >= 0
    P = np.where(mask[..., None], pts[np.maximum(nbr, 0)], 0.0)
    cnt = np.maximum(counts, 1)[:, None].astype(np.float64)
    m = P.sum(1) / cnt
    E = np.where(mask[..., None], P - m[:, None, :], 0.0)
    return np.einsum("nka,nkb->nab", E, E) / cnt[:, :, None]


def jacobi_smallest(C):
    """Unit eigenvector of the smallest eigenvalue of every symmetric C [n, 3, 3]: the kernel's cyclic Jacobi."""
    a = np.array(C, np.float64)
    n = len(a)
    v = np.tile(np.eye(3), (n, 1, 1))
    for _ in range(12):
        off = np.abs(a[:, 0, 1]) + np.abs(a[:, 0, 2]) + np.abs(a[:, 1, 2])
        live = off > 2.0 ** -70 * (np.abs(a[:, 0, 0]) + np.abs(a[:, 1, 1]) + np.abs(a[:, 2, 2]))
        if not live.any():
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = a[:, p, q]
            do = live & (apq != 0.0)
            safe = np.where(do, apq, 1.0)
            theta = (a[:, q, q] - a[:, p, p]) / (2.0 * safe)
            t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            c, s = np.where(do, c, 1.0), np.where(do, s, 0.0)
            for m in (a, v):
                mp, mq = m[:, :, p].copy(), m[:, :, q].copy()
                m[:, :, p] = c[:, None] * mp - s[:, None] * mq
                m[:, :, q] = s[:, None] * mp + c[:, None] * mq
            ap, aq = a[:, p, :].copy(), a[:, q, :].copy()
            a[:, p, :] = c[:, None] * ap - s[:, None] * aq
            a[:, q, :] = s[:, None] * ap + c[:, None] * aq
            a[do, p, q] = 0.0
            a[do, q, p] = 0.0
    diag = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], 1)
    m = np.zeros(n, np.int64)
    m = np.where(diag[:, 1] < diag[np.arange(n), m], 1, m)
    m = np.where(diag[:, 2] < diag[np.arange(n), m], 2, m)
    vec = v[np.arange(n), :, m]
    return vec / np.linalg.norm(vec, axis=1, keepdims=True)


def orient(normals, points, counts, viewpoint):
    nrm = np.array(normals, np.float64)
    if viewpoint is not None:
        flip = (nrm * (np.asarray(viewpoint, np.float64)[None] - points)).sum(1) < 0.0
    else:
        k = np.argmax(np.abs(nrm), 1)                                  # the first of equal magnitudes
        flip = nrm[np.arange(len(nrm)), k] < 0.0
    nrm[flip] = -nrm[flip]
    nrm[counts < 3] = (0.0, 0.0, 1.0)
    return nrm


def restate(points, knn, max_radius, viewpoint=None):
    """dict(nbr, counts, cov, normals) of the restatement."""
    pts = np.asarray(points, np.float64)
    nbr, counts = neighbors(pts, knn, max_radius)
    C = covariances(pts, nbr, counts)
    return dict(nbr=nbr, counts=counts, cov=C, normals=orient(jacobi_smallest(C), pts, counts, viewpoint))


def check_normals(normals, points, ref, viewpoint):
    """The gates of the issue on `normals` (the kernel's, or the restatement's own) against the restatement `ref` and
    numpy.linalg.eigh of its covariances.  Returns dict(unit, rayleigh, angle, under_gap) of the measured maxima."""
    nrm, pts = np.asarray(normals, np.float64), np.asarray(points, np.float64)
    counts, C = ref["counts"], ref["cov"]
    lam = np.linalg.eigvalsh(C)
    unit = float(np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max())
    assert unit <= 1e-14, unit
    few = counts < 3
    assert (nrm[few] == np.array([0.0, 0.0, 1.0])).all()               # the fallback, unsigned
    ray = np.einsum("na,nab,nb->n", nrm, C, nrm)
    excess = np.where(few, 0.0, ray - lam[:, 0] - 1e-12 * lam[:, 2])
    assert (excess <= 0.0).all(), float(excess.max())
    gap = (lam[:, 1] - lam[:, 0]) / np.where(lam[:, 2] > 0, lam[:, 2], 1.0)
    sure = ~few & (lam[:, 2] > 0) & (gap >= GAP)
    cosang = np.abs((nrm * ref["normals"]).sum(1))
    sinang = np.linalg.norm(np.cross(nrm, ref["normals"]), axis=1)
    angle = np.arctan2(sinang, cosang)
    worst = float(angle[sure].max()) if sure.any() else 0.0
    assert worst <= 1e-9, worst
    live = ~few
    if viewpoint is not None:
        to_v = np.asarray(viewpoint, np.float64)[None] - pts
        d = (nrm * to_v).sum(1)
        assert (d[live] >= -4e-16 * np.linalg.norm(to_v, axis=1)[live]).all()      # the rounding of a 3-term dot product
    else:
        k = np.argmax(np.abs(nrm), 1)
        assert (nrm[np.arange(len(nrm)), k][live] > 0.0).all()
    return dict(unit=unit, rayleigh=float(excess.max()), angle=worst, under_gap=float((live & ~sure).sum() / max(1, live.sum())))


# ---- the cases ---------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    points: np.ndarray
    knn: int
    max_radius: float
    generic: bool               # non-degenerate: at most 10 % of its points may fall under the gap


def fixture_points():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))
    return z["cloud_bin_0"][::64].astype(np.float64)


def cases():
    rng = np.random.default_rng(5)
    out = []
    small = rng.uniform(-0.3, 0.3, (5, 3))
    for n in (1, 2, 3):
        out.append(Case(f"n{n}_knn30", small[:n], 30, 1.0, False))
    out.append(Case("n5_knn8", small, 8, 1.0, False))
    g = np.stack(np.meshgrid(np.arange(16.0), np.arange(16.0), indexing="ij"), -1).reshape(-1, 2)
    lattice = np.concatenate([g, np.full((256, 1), 2.0)], 1)
    out.append(Case("lattice_plane_ties", lattice[rng.permutation(256)], 10, 3.0, False))   # 9 within d^2 <= 2, 4 at d^2 = 4
    base = rng.uniform(0.0, 1.0, (200, 3))
    dup = np.concatenate([base, base[rng.integers(0, 200, 80)], base[:20]])
    out.append(Case("exact_duplicates", dup[rng.permutation(len(dup))], 8, 0.5, False))
    edge = 0.25                                                         # the cell edge of max_radius = 0.5
    xs = np.concatenate([[k * edge, np.nextafter(k * edge, -9.0), np.nextafter(k * edge, 9.0)] for k in range(-4, 5)])
    ys = np.array([-edge, 0.0, 0.11, edge, 0.37])
    zs = np.array([0.0, 0.05, edge])
    cells = np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3)
    out.append(Case("cell_boundaries", cells[rng.permutation(len(cells))], 12, 0.5, False))
    t = rng.uniform(-1.0, 1.0, 40)
    out.append(Case("collinear_generic", t[:, None] * np.array([[1.0, 2.0, 3.0]]) + 0.5, 5, 10.0, False))
    out.append(Case("collinear_axis", np.arange(12.0)[:, None] * np.array([[0.0, 0.125, 0.0]]), 5, 10.0, False))
    two = np.concatenate([rng.uniform(0, 0.2, (10, 3)), rng.uniform(0, 0.2, (10, 3)) + 10.0])
    out.append(Case("two_clusters", two, 30, 1.0, False))
    uv = rng.uniform(-0.5, 0.5, (1500, 2))
    sphere = np.concatenate([uv, np.sqrt(4.0 - (uv ** 2).sum(1))[:, None]], 1)
    out.append(Case("curved_patch_3600m", sphere + np.array([3000.0, -2000.0, 500.0]), 30, 0.3, True))
    cloud = rng.uniform(0.0, 1.0, (2000, 3))
    for knn in (1, 30, 64):
        out.append(Case(f"random_knn{knn}", cloud, knn, 0.25, knn > 1))
    out.append(Case("fixture_every_64th", fixture_points(), 30, 0.3, True))
    return out


_REF = {}


def reference(case, viewpoint):
    """The restatement of a case, computed once per process and left unchanged."""
    key = (case.name, viewpoint is not None)
    if key not in _REF:
        base = _REF.get((case.name, not key[1]))
        if base is None:
            _REF[key] = restate(case.points, case.knn, case.max_radius, viewpoint)
        else:                                                          # the same sets and covariances, the other sign rule
            _REF[key] = dict(base, normals=orient(jacobi_smallest(base["cov"]), case.points, base["counts"], viewpoint))
    return _REF[key]
