"""Plain NumPy fp64 restatement of the robust transform estimator that `imf_robust_transform` replaces (20 reweighted
rounds of the small-angle linear fit), the synthetic correspondence sets of tests/golden/robust_transform.npz, and
access to that fixture.  Test helper: no GPU, no torch."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robust_transform.npz")
SEEDS = (0, 1, 2)
# family -> n, box (lo, hi), rotation (deg), translation (m), inlier share, noise sigma (m), explicit weights,
# coordinate grid (m; a power of two: the fixture stores a point as int16 multiples of it, exact in float32)
INDOOR = ((0.0, 0.0, 0.0), (4.0, 4.0, 2.5))
OUTDOOR = ((-60.0, -60.0, -2.0), (60.0, 60.0, 4.0))
FAMILIES = {
    "indoor_8deg": dict(n=5000, box=INDOOR, deg=8.0, shift=0.3, inliers=0.40, sigma=0.01, weights=False, grid=2.0 ** -10),
    "indoor_20deg": dict(n=5000, box=INDOOR, deg=20.0, shift=0.5, inliers=0.15, sigma=0.01, weights=False, grid=2.0 ** -10),
    "outdoor_5deg": dict(n=5000, box=OUTDOOR, deg=5.0, shift=10.0, inliers=0.40, sigma=0.05, weights=False, grid=2.0 ** -8),
    "outdoor_10deg": dict(n=5000, box=OUTDOOR, deg=10.0, shift=11.0, inliers=0.20, sigma=0.05, weights=False, grid=2.0 ** -8),
    "indoor_300": dict(n=300, box=INDOOR, deg=8.0, shift=0.3, inliers=0.40, sigma=0.01, weights=False, grid=2.0 ** -10),
    "indoor_weights": dict(n=5000, box=INDOOR, deg=8.0, shift=0.3, inliers=0.40, sigma=0.01, weights=True, grid=2.0 ** -10),
}


def rotation(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def counter_uniform(stream, count):
    """`count` uniforms in [0, 1) with 32 bits each from a counter hashed by splitmix64's finaliser: integer
    arithmetic only, so the same values on every machine and library version (numpy's own streams promise less)."""
    with np.errstate(over="ignore"):
        x = (np.arange(count, dtype=np.uint64) + np.uint64(stream) * np.uint64(0x1000000)) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(32)).astype(np.float64) / 4294967296.0


def source_points(n, box, grid, seed):
    """pts0 of a case: uniform in the box on the grid, from counter_uniform.  The fixture does not store them: they
    are rebuilt from here, exactly."""
    lo, hi = np.asarray(box[0]), np.asarray(box[1])
    u = counter_uniform(2 * seed + 1, 3 * n).reshape(n, 3)
    return (np.round((lo + (hi - lo) * u) / grid) * grid).astype(np.float32)


def source_weights(n, seed):
    return (0.1 + 0.9 * counter_uniform(2 * seed + 2, n)).astype(np.float32)


def make_case(n, box, deg, shift, inliers, sigma, weights, grid, seed):
    """(pts0, pts1 float32 [n, 3], weight float32 [n] or None, planted 4x4): pts0 uniform in the box; an inlier's
    pts1 = R pts0 + t + N(0, sigma); an outlier's pts1 uniform in the box; everything rounded to `grid`."""
    g = np.random.default_rng(seed)
    lo, hi = np.asarray(box[0]), np.asarray(box[1])
    p0 = source_points(n, box, grid, seed).astype(np.float64)
    T = np.eye(4)
    T[:3, :3] = rotation(g.normal(size=3), deg)
    d = g.normal(size=3)
    T[:3, 3] = shift * d / np.linalg.norm(d)
    p1 = p0 @ T[:3, :3].T + T[:3, 3] + g.normal(0.0, sigma, (n, 3))
    out = g.random(n) >= inliers
    p1[out] = (lo + (hi - lo) * g.random((n, 3)))[out]
    p1 = np.round(p1 / grid) * grid
    w = source_weights(n, seed) if weights else None
    return p0.astype(np.float32), p1.astype(np.float32), w, T


def euler_zyx(x):
    """Rz(x[2]) Ry(x[1]) Rx(x[0])."""
    (sa, sb, sc), (ca, cb, cc) = np.sin(x[:3]), np.cos(x[:3])
    return np.array([[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa],
                     [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa],
                     [-sb, cb * sa, cb * ca]])


def robust_transform_f64(pts0, pts1, weight=None, rounds=20):
    """The 20 rounds in fp64 with the 3n x 6 system materialised: A = w J(cur), b = w (pts1 - cur), x = (A^T A)^-1 A^T b,
    cur <- [Rz Ry Rx | t] cur, w <- par / (|cur - pts1| + par), par = 1 halved at rounds 5, 10, 15."""
    cur = np.asarray(pts0, np.float64).copy()
    q = np.asarray(pts1, np.float64)
    n = len(cur)
    w = np.ones(n) if weight is None else np.asarray(weight, np.float64).reshape(n).copy()
    T = np.eye(4)
    par = 1.0
    for i in range(rounds):
        if i > 0 and i % 5 == 0:
            par /= 2.0
        x, y, z = cur.T
        o, l = np.zeros(n), np.ones(n)
        A = np.concatenate([np.stack([o, z, -y, l, o, o], 1), np.stack([-z, o, x, o, l, o], 1),
                            np.stack([y, -x, o, o, o, l], 1)]) * np.tile(w, 3)[:, None]
        b = np.concatenate([(q - cur)[:, 0], (q - cur)[:, 1], (q - cur)[:, 2]]) * np.tile(w, 3)
        sol = np.linalg.inv(A.T @ A) @ (A.T @ b)
        U = np.eye(4)
        U[:3, :3] = euler_zyx(sol)
        U[:3, 3] = sol[3:]
        cur = cur @ U[:3, :3].T + U[:3, 3]
        w = par / (np.linalg.norm(cur - q, axis=1) + par)
        T = U @ T
    return T


def load_cases():
    """[(family, seed, pts0, pts1, weight or None, T_upstream float32 4x4, gap_R, gap_t)] of the fixture.  pts1 is the
    stored int16 grid multiples times the family's grid (exact); pts0 and the explicit weights are rebuilt by
    source_points / source_weights (integer arithmetic, exact), which keeps the file at half the size."""
    z = np.load(GOLDEN)
    out = []
    for fam in FAMILIES:
        for seed in SEEDS:
            k = f"{fam}_{seed}_"
            grid = np.float32(FAMILIES[fam]["grid"])
            kw = FAMILIES[fam]
            p0 = source_points(kw["n"], kw["box"], kw["grid"], seed)
            p1 = z[k + "pts1_q"].astype(np.float32) * grid
            out.append((fam, seed, p0, p1, source_weights(kw["n"], seed) if kw["weights"] else None,
                        z[k + "T_upstream"], float(z[k + "gap_R"]), float(z[k + "gap_t"])))
    return out


def family_tolerance(cases, family, factor=4.0):
    """(tol_R, tol_t): `factor` x the largest stored float32-vs-fp64 gap of the family."""
    rows = [c for c in cases if c[0] == family]
    return factor * max(c[6] for c in rows), factor * max(c[7] for c in rows)
