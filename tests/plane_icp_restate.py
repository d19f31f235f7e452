"""Float64 NumPy restatement of imf_icp_point_to_plane (csrc/icp.hip) and the cases its tests share.  Plain helper module:
tests/test_normals_host.py exercises it on the CPU, tests/test_gpu_plane_icp.py runs the kernels against it.

The loop is kitti_restate.icp_restated's (Open3D RegistrationICP, [RECALLED]) on registration_cases.nearest_brute (strict
d^2 < r^2, ties to the lowest target index); the update is TransformationEstimationPointToPlane's: r = (p - q) . n,
J = [p x n, n], (J^T J) x = -(J^T r) by LDL^T without pivoting, update = [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5]; a pivot
<= 1e-12 times the largest diagonal entry of J^T J (or an empty correspondence set) makes the update the identity."""
import numpy as np

from kitti_restate import rigid
from registration_cases import nearest_brute


def ldl_solve(A, rhs):
    """x of A x = rhs, or None under the singular rule."""
    L, D = np.eye(6), np.zeros(6)
    big = max(A[k, k] for k in range(6))
    for j in range(6):
        d = A[j, j] - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
        if not d > 1e-12 * big:
            return None
        D[j] = d
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / d
    y = np.zeros(6)
    for i in range(6):
        y[i] = rhs[i] - sum(L[i, k] * y[k] for k in range(i))
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = y[i] / D[i] - sum(L[k, i] * x[k] for k in range(i + 1, 6))
    return x


def update_from(x):
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    U = np.eye(4)
    U[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                 [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                 [-sb, cb * sa, cb * ca]]
    U[:3, 3] = x[3:]
    return U


def plane_update(P, Q, N):
    if len(P) == 0:
        return np.eye(4)
    r = ((P - Q) * N).sum(1)
    J = np.concatenate([np.cross(P, N), N], 1)
    x = ldl_solve(J.T @ J, -(J.T @ r))
    return np.eye(4) if x is None else update_from(x)


def icp_plane_restated(src, dst, normals, r, init=None, max_iteration=30):
    """(T, fitness, rmse, iterations, n_corr)."""
    src, dst, normals = (np.asarray(a, np.float64) for a in (src, dst, normals))
    T = np.eye(4) if init is None else np.array(init, np.float64)
    pcd = src @ T[:3, :3].T + T[:3, 3]

    def corr(p):
        ok, j, d2 = nearest_brute(p, dst, r)
        n = int(ok.sum())
        return np.flatnonzero(ok), j[ok], (n / len(p) if n else 0.0), (float(np.sqrt(d2[ok].sum() / n)) if n else 0.0)

    i_s, i_d, fit, rmse = corr(pcd)
    iters = 0
    for it in range(max_iteration):
        upd = plane_update(pcd[i_s], dst[i_d], normals[i_d])
        T = upd @ T
        pcd = pcd @ upd[:3, :3].T + upd[:3, 3]
        f0, r0 = fit, rmse
        i_s, i_d, fit, rmse = corr(pcd)
        iters = it + 1
        if abs(f0 - fit) < 1e-6 and abs(r0 - rmse) < 1e-6:
            break
    return T, fit, rmse, iters, len(i_s)


def bumpy_surface(n_side=40, seed=3):
    """(points [n, 3], unit normals [n, 3]) of z = 0.05 sin(3x) cos(2y) + 0.03 sin(5y + 1) over [-1, 1]^2, jittered."""
    rng = np.random.default_rng(seed)
    g = np.linspace(-1.0, 1.0, n_side)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2) + rng.uniform(-0.01, 0.01, (n_side * n_side, 2))
    x, y = xy[:, 0], xy[:, 1]
    z = 0.05 * np.sin(3 * x) * np.cos(2 * y) + 0.03 * np.sin(5 * y + 1)
    zx = 0.15 * np.cos(3 * x) * np.cos(2 * y)
    zy = -0.1 * np.sin(3 * x) * np.sin(2 * y) + 0.15 * np.cos(5 * y + 1)
    nrm = np.stack([-zx, -zy, np.ones_like(z)], 1)
    return np.stack([x, y, z], 1), nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def bumpy_case():
    """A 1600-point bumpy target with analytic normals; the source is every other target point moved back by a
    3 degree / 2 cm motion.  Returns (src, dst, normals, r, truth)."""
    dst, nrm = bumpy_surface()
    truth = rigid(3.0, [0.3, -0.5, 1.0], np.array([0.012, -0.010, 0.0125]))       # |t| = 2 cm
    sub = dst[::2]
    src = (sub - truth[:3, 3]) @ truth[:3, :3]
    return src, dst, nrm, 0.15, truth


def tolerances(src, dst, normals, r, init, max_iteration):
    """The restatement forward, the same with the source in reversed order, and the bounds the kernel gets: 16 times how
    far T, fitness and rmse moved between the two, at least 1e-12."""
    fwd = icp_plane_restated(src, dst, normals, r, init, max_iteration)
    rev = icp_plane_restated(src[::-1], dst, normals, r, init, max_iteration)
    moved = (float(np.abs(fwd[0] - rev[0]).max()), abs(fwd[1] - rev[1]), abs(fwd[2] - rev[2]))
    return fwd, rev, moved, tuple(max(16.0 * m, 1e-12) for m in moved)
