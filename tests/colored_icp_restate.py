"""Float64 NumPy restatement of imf_color_gradient and imf_icp_colored (csrc/colored_icp.hip, csrc/icp.hip), the cases
their tests share and the tolerance functions.  Plain helper module: tests/test_colored_icp_host.py exercises it on the
CPU, tests/test_gpu_colored_icp.py runs the kernels against it.  No GPU dependency.

The rules restated ([RECALLED] from Open3D's registration_colored_icp; Park, Zhou, Koltun, ICCV 2017):
  intensity  I = (r + g + b) / 765, the integer sum first, one division;
  gradient   per point p (unit normal n, list j_0 .. j_{m-1} of normals_restate.neighbors, the point itself included):
             u = (p' - p) - ((p' - p) . n) n, b = I_p' - I_p per listed neighbour; (sum u u^T + (m - 1)^2 n n^T) g = sum u b by
             LDL^T without pivoting; a pivot <= 1e-12 times the largest diagonal entry (or NaN) gives g = 0, as does m < 4;
  joint fit  plane_icp_restate's loop; per correspondence r_G = (p - q) . n, J_G = [p x n, n], pt = p - r_G n,
             r_I = I_s - (I_q + g . (pt - q)), M = -g + (n . g) n, J_I = [p x M, M]; the 6x6 system is
             lambda J_G^T J_G + (1 - lambda) J_I^T J_I, its right-hand side -(lambda J_G^T r_G + (1 - lambda) J_I^T r_I).
The nine sums of the gradient are taken over the list positions in a chosen order: "forward", "reversed" (the pair that
sets the tolerance) or "butterfly" (the kernel's xor butterfly over 64 lanes: what the kernel computes, bit for bit, when
its products and sums round one by one)."""
import numpy as np

import normals_restate as NR
import plane_icp_restate as PR
from registration_cases import nearest_brute

LAMBDA = 0.968


def intensity(rgb):
    return np.asarray(rgb, np.uint8).astype(np.int64).sum(1).astype(np.float64) / 765.0


# ---- the colour gradient -----------------------------------------------------------------------------------------------
def _rows(points, normals, inten, nbr, counts):
    """(U [n, knn, 3], B [n, knn], m [n]): every list position's projected offset and intensity difference, zero where the
    position holds nothing."""
    pts, nrm, I = (np.asarray(a, np.float64) for a in (points, normals, inten))
    n, knn = nbr.shape
    m = np.clip(counts, 0, knn)
    mine = (np.arange(knn)[None, :] < m[:, None]) & (nbr >= 0) & (nbr < n)
    j = np.where(mine, nbr, 0)
    E = pts[j] - pts[:, None, :]
    d = (E[..., 0] * nrm[:, None, 0] + E[..., 1] * nrm[:, None, 1]) + E[..., 2] * nrm[:, None, 2]
    U = E - d[..., None] * nrm[:, None, :]
    B = I[j] - I[:, None]
    return np.where(mine[..., None], U, 0.0), np.where(mine, B, 0.0), m


def _sum_positions(X, order):
    """Sum X [n, knn] over the list positions in the given order."""
    n, knn = X.shape
    if order == "butterfly":
        v = np.zeros((n, 64))
        v[:, :knn] = X
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ o]
        return v[:, 0].copy()
    acc = np.zeros(n)
    for k in (range(knn) if order == "forward" else range(knn - 1, -1, -1)):
        acc = acc + X[:, k]
    return acc


def gradient_restated(points, normals, inten, nbr, counts, order="forward"):
    """float64 [n, 3]."""
    U, B, m = _rows(points, normals, inten, nbr, counts)
    nrm = np.asarray(normals, np.float64)
    n = len(U)
    S = lambda X: _sum_positions(X, order)
    w2 = ((m - 1).astype(np.float64)) ** 2
    A = {}
    for a in range(3):
        for b in range(a, 3):
            A[a, b] = S(U[..., a] * U[..., b]) + w2 * (nrm[:, a] * nrm[:, b])
    rhs = [S(U[..., a] * B) for a in range(3)]
    with np.errstate(all="ignore"):
        big = np.maximum(A[0, 0], np.maximum(A[1, 1], A[2, 2]))
        d0 = A[0, 0]
        ok = (m >= 4) & (d0 > 1e-12 * big)
        l10, l20 = A[0, 1] / d0, A[0, 2] / d0
        d1 = A[1, 1] - l10 * l10 * d0
        ok &= d1 > 1e-12 * big
        l21 = (A[1, 2] - l20 * l10 * d0) / d1
        d2 = (A[2, 2] - l20 * l20 * d0) - l21 * l21 * d1
        ok &= d2 > 1e-12 * big
        y0 = rhs[0]
        y1 = rhs[1] - l10 * y0
        y2 = (rhs[2] - l20 * y0) - l21 * y1
        gz = y2 / d2
        gy = y1 / d1 - l21 * gz
        gx = (y0 / d0 - l10 * gy) - l20 * gz
    g = np.stack([gx, gy, gz], 1)
    g[~ok] = 0.0
    return g


def gradient_floor(points, normals, inten, nbr, counts):
    """[n]: 1e-12 times the sum over the listed neighbours of |I_p' - I_p| / |u| (neighbours with u = 0 left out)."""
    U, B, _ = _rows(points, normals, inten, nbr, counts)
    length = np.linalg.norm(U, axis=2)
    with np.errstate(all="ignore"):
        return 1e-12 * np.where(length > 0, np.abs(B) / length, 0.0).sum(1)


def gradient_tolerance(points, normals, inten, nbr, counts):
    """(forward [n, 3], moved [n], bound [n]): the restatement, how far a row moved between the forward and the reversed
    order of its list positions (largest component), and what the kernel gets: 16 times that, at least the floor."""
    fwd = gradient_restated(points, normals, inten, nbr, counts, "forward")
    rev = gradient_restated(points, normals, inten, nbr, counts, "reversed")
    moved = np.abs(fwd - rev).max(1)
    return fwd, moved, np.maximum(16.0 * moved, gradient_floor(points, normals, inten, nbr, counts))


# ---- the joint fit -----------------------------------------------------------------------------------------------------
def jacobians(P, Q, N, G):
    """(J_G [k, 6], J_I [k, 6]) of current source points P on targets Q with normals N and gradients G, rotation first."""
    M = -G + (N * G).sum(1)[:, None] * N
    return np.concatenate([np.cross(P, N), N], 1), np.concatenate([np.cross(P, M), M], 1)


def residuals(P, Is, Q, N, Iq, G):
    """(r_G [k], r_I [k])."""
    rg = ((P - Q) * N).sum(1)
    Pt = P - rg[:, None] * N
    return rg, Is - (Iq + (G * (Pt - Q)).sum(1))


def colored_update(P, Is, Q, N, Iq, G, lam):
    if len(P) == 0:
        return np.eye(4)
    rg, ri = residuals(P, Is, Q, N, Iq, G)
    JG, JI = jacobians(P, Q, N, G)
    A = lam * (JG.T @ JG) + (1.0 - lam) * (JI.T @ JI)
    x = PR.ldl_solve(A, -(lam * (JG.T @ rg) + (1.0 - lam) * (JI.T @ ri)))
    return np.eye(4) if x is None else PR.update_from(x)


def icp_colored_restated(src, src_I, dst, normals, dst_I, grad, r, lam=LAMBDA, init=None, max_iteration=30):
    """(T, fitness, rmse, iterations, n_corr): plane_icp_restate.icp_plane_restated with the coloured update."""
    src, src_I, dst, normals, dst_I, grad = (np.asarray(a, np.float64) for a in (src, src_I, dst, normals, dst_I, grad))
    T = np.eye(4) if init is None else np.array(init, np.float64)
    pcd = src @ T[:3, :3].T + T[:3, 3]

    def corr(p):
        ok, j, d2 = nearest_brute(p, dst, r)
        n = int(ok.sum())
        return np.flatnonzero(ok), j[ok], (n / len(p) if n else 0.0), (float(np.sqrt(d2[ok].sum() / n)) if n else 0.0)

    i_s, i_d, fit, rmse = corr(pcd)
    iters = 0
    for it in range(max_iteration):
        upd = colored_update(pcd[i_s], src_I[i_s], dst[i_d], normals[i_d], dst_I[i_d], grad[i_d], lam)
        T = upd @ T
        pcd = pcd @ upd[:3, :3].T + upd[:3, 3]
        f0, r0 = fit, rmse
        i_s, i_d, fit, rmse = corr(pcd)
        iters = it + 1
        if abs(f0 - fit) < 1e-6 and abs(r0 - rmse) < 1e-6:
            break
    return T, fit, rmse, iters, len(i_s)


def tolerances(src, src_I, dst, normals, dst_I, grad, r, lam, init, max_iteration):
    """The restatement forward, the same with the source rows in reversed order, how far T, fitness and rmse moved between
    the two, and the bounds the kernel gets: 16 times that, at least 1e-12."""
    fwd = icp_colored_restated(src, src_I, dst, normals, dst_I, grad, r, lam, init, max_iteration)
    rev = icp_colored_restated(src[::-1], src_I[::-1], dst, normals, dst_I, grad, r, lam, init, max_iteration)
    moved = (float(np.abs(fwd[0] - rev[0]).max()), abs(fwd[1] - rev[1]), abs(fwd[2] - rev[2]))
    return fwd, rev, moved, tuple(max(16.0 * m, 1e-12) for m in moved)


def off(T, truth):
    """(|dR|_F, |dt|) of T against the truth."""
    return float(np.linalg.norm(T[:3, :3] - truth[:3, :3])), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


# ---- the C ABI's refusals ----------------------------------------------------------------------------------------------
def check_refusals(L):
    """Every refusal of the two entry points comes before any launch, so it answers with host pointers and without a GPU:
    a NULL array (named in the message), knn outside 1..64, a bad lambda_geometric, a workspace one byte short."""
    buf = np.zeros(1 << 16, dtype=np.float64)
    p = buf.ctypes.data
    p += (-p) % 256
    EINVAL = -1

    def grad(n=8, knn=30, null=None):
        a = {k: (None if k == null else p) for k in ("points", "normals", "intensity", "neighbors", "counts", "out_grad")}
        return L.imf_color_gradient(a["points"], a["normals"], a["intensity"], a["neighbors"], a["counts"], n, knn,
                                    a["out_grad"], None)

    for kw in (dict(n=0), dict(n=-1), dict(n=1 << 30), dict(knn=0), dict(knn=65), dict(knn=-4)):
        assert grad(**kw) == EINVAL, kw
    assert grad(knn=65) == EINVAL and b"knn" in L.imf_last_error()
    for null in ("points", "normals", "intensity", "neighbors", "counts", "out_grad"):
        assert grad(null=null) == EINVAL and null.encode() in L.imf_last_error(), null

    full = L.imf_icp_colored_workspace_bytes(8, 8)
    assert full == L.imf_icp_plane_workspace_bytes(8, 8) > 0
    assert L.imf_icp_colored_workspace_bytes(0, 5) == 0 and L.imf_icp_colored_workspace_bytes(5, 0) == 0

    def colored(n_src=8, n_dst=8, r=0.1, lam=0.968, it=30, null=None, ws=full):
        a = {k: (None if k == null else p) for k in ("src", "src_intensity", "dst", "nrm", "dst_intensity", "dst_gradient",
                                                     "T", "stats", "meta", "workspace")}
        return L.imf_icp_colored(a["src"], a["src_intensity"], n_src, a["dst"], a["nrm"], a["dst_intensity"],
                                 a["dst_gradient"], n_dst, r, lam, None, it, a["T"], a["stats"], a["meta"], a["workspace"],
                                 ws, None)

    for kw in (dict(n_src=0), dict(n_dst=0), dict(n_src=1 << 30), dict(r=0.0), dict(r=float("nan")), dict(it=-1),
               dict(ws=0), dict(ws=full - 1)):
        assert colored(**kw) == EINVAL, kw
    assert b"workspace" in L.imf_last_error()
    for lam in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        assert colored(lam=lam) == EINVAL and b"lambda_geometric" in L.imf_last_error(), lam
    for null in ("src", "dst", "nrm", "T", "stats", "meta", "workspace"):
        assert colored(null=null) == EINVAL and b"null" in L.imf_last_error(), null
    for null in ("src_intensity", "dst_intensity", "dst_gradient"):
        assert colored(null=null) == EINVAL and null.encode() in L.imf_last_error(), null


# ---- the cases ---------------------------------------------------------------------------------------------------------
R_CORR, GRAD_KNN, GRAD_RADIUS = 0.075, 30, 0.2
TRUTH = PR.update_from(np.concatenate([np.deg2rad([0.5, -0.3, 1.0]), [0.03, -0.02, 0.01]]))


def texture(p):
    """The smooth intensity painted on the world, in [0, 1], from the x and y of points [n, 3]."""
    x, y = p[:, 0], p[:, 1]
    return 0.5 + 0.2 * np.sin(3 * x + 0.5) + 0.2 * np.cos(2.5 * y) + 0.1 * np.sin(2 * x - 3 * y)


def _lattice(half, step, jitter, rng):
    g = np.arange(-half, half + step / 2, step)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    return xy + rng.uniform(-jitter, jitter, xy.shape)


def _moved_back(true_src):
    return (true_src - TRUTH[:3, 3]) @ TRUTH[:3, :3]                    # R^T (p - t)


def _case(true_src, dst, nrm):
    nbr, counts = NR.neighbors(dst, GRAD_KNN, GRAD_RADIUS)
    dst_I = texture(dst)
    return dict(src=_moved_back(true_src), src_I=texture(true_src), dst=dst, normals=nrm, dst_I=dst_I, nbr=nbr, counts=counts,
                grad=gradient_restated(dst, nrm, dst_I, nbr, counts), r=R_CORR, lam=LAMBDA, truth=TRUTH)


_CASES = {}


def exact_cases():
    """The gradient's exact cases: dicts(name, points, normals, inten, nbr, counts, want).  want is the expected gradient
    [n, 3]; it holds exactly (==) unless `to_bound` is set, where it holds to gradient_tolerance's bound."""
    if "exact" in _CASES:
        return _CASES["exact"]
    rng = np.random.default_rng(21)
    out = []

    def add(name, pts, nrm, inten, knn, radius, want, to_bound=False):
        nbr, counts = NR.neighbors(pts, knn, radius)
        out.append(dict(name=name, points=pts, normals=nrm, inten=inten, nbr=nbr, counts=counts, want=want,
                        to_bound=to_bound))

    surf, nrm = PR.bumpy_surface(41, seed=3)
    pick = rng.permutation(len(surf))[:300]
    add("constant_intensity", surf[pick], nrm[pick], np.full(300, 0.37), 30, 0.5, np.zeros((300, 3)))
    flat = np.concatenate([_lattice(0.4, 0.05, 0.015, rng), np.zeros((17 * 17, 1))], 1)
    up = np.tile([[0.0, 0.0, 1.0]], (len(flat), 1))
    a = np.array([0.3, -0.2, 0.5])
    add("linear_on_a_jittered_plane", flat, up, flat @ a + 0.4, 30, 0.2, np.tile(a - a[2] * up[0], (len(flat), 1)),
        to_bound=True)
    three = rng.uniform(-0.1, 0.1, (3, 3))
    add("m3", three, np.tile([[0.6, 0.0, 0.8]], (3, 1)), rng.uniform(0, 1, 3), 30, 1.0, np.zeros((3, 3)))
    line = 0.5 + np.array([0.0, 0.31, 0.55, 1.0])[:, None] * np.array([[0.07, -0.04, 0.02]])
    add("m4_collinear", line, np.tile([[0.6, 0.0, 0.8]], (4, 1)), rng.uniform(0, 1, 4), 30, 1.0, np.zeros((4, 3)))
    _CASES["exact"] = out
    return out


def textured_plane():
    """The case that justifies the feature: a flat target (41 x 41 jittered lattice, z = 0, normals (0, 0, 1)), a 27 x 27
    source on the same plane moved back by TRUTH, both painted with `texture` at their true positions.  Built once."""
    if "plane" not in _CASES:
        rng = np.random.default_rng(11)
        dst = np.concatenate([_lattice(1.0, 0.05, 0.015, rng), np.zeros((41 * 41, 1))], 1)
        true_src = np.concatenate([_lattice(0.8, 0.0625, 0.015, rng), np.zeros((27 * 27, 1))], 1)
        _CASES["plane"] = _case(true_src, dst, np.tile([[0.0, 0.0, 1.0]], (len(dst), 1)))
    return _CASES["plane"]


def painted_bumpy():
    """plane_icp_restate.bumpy_surface (41 x 41, analytic normals) painted with `texture`; the source is another sampling
    of the surface (27 x 27, its points within [-0.8, 0.8]^2) moved back by TRUTH.  Built once."""
    if "bumpy" not in _CASES:
        dst, nrm = PR.bumpy_surface(41, seed=3)
        other, _ = PR.bumpy_surface(27, seed=4)
        true_src = other[(np.abs(other[:, :2]) <= 0.8).all(1)]
        _CASES["bumpy"] = _case(true_src, dst, nrm)
    return _CASES["bumpy"]
