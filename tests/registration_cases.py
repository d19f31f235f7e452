"""Adversarial point sets and brute-force float64 restatements for the registration back end (csrc/icp.hip: the cell-CSR
grid, imf_icp_point_to_point, imf_radius_count, imf_radius_pairs; csrc/registration.h: the rigid fit; csrc/ransac.hip).
Plain helper module: tests/test_registration_host.py proves the catalogue on the CPU, tests/test_gpu_registration_exact.py
runs it against the kernels.  No GPU dependency.

Exactness.  Exact cases use dyadic coordinates, multiples of Q = 2^-10 with |x| < 2^10, and transforms with dyadic entries
(identity, axis permutations, quarter turns, dyadic translations).  Every difference, square and sum of three squares is
then a multiple of 2^-20 below 2^24: exact in fp64 whether or not the compiler contracts to FMA, so those comparisons
carry no tolerance.  Degenerate fits keep their zeros exact: constant coordinates are 0, otherwise the correspondence
count is a power of two (the mean is exact).

The grid (csrc/icp.hip).  cell = floor(x * inv_cell), inv_cell = (1 - 1e-9) / r; targets are accepted in cells
[-(2^17 - 1), 2^17 - 2] per axis, queries search from cells [-2^17, 2^17 - 1]; beyond that (and NaN) a target is an
error and a query finds nothing.  Keys keep 18 bits per axis."""
from typing import NamedTuple, Optional

import numpy as np

import imf_oracle as O
from kitti_restate import icp_restated, rigid, scene_points

Q = 2.0 ** -10
KEY_LIM = 1 << 17
TARGET_CELLS = (-(KEY_LIM - 1), KEY_LIM - 2)      # first and last permitted target cell
QUERY_CELLS = (-KEY_LIM, KEY_LIM - 1)             # first and last cell a query searches from


# ---- transforms with dyadic entries ---------------------------------------------------------------------------------
def transform(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


QUARTER_Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
PERM_XYZ = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
EXACT_TRANSFORMS = (None, transform(QUARTER_Z, [0.5, -0.25, 0.125]), transform(PERM_XYZ, [-0.375, 0.0, 0.75]),
                    transform(np.eye(3), [0.0625, -0.125, 0.25]))


def apply_T(T, p):
    p = np.asarray(p, np.float64)
    return p if T is None else p @ T[:3, :3].T + T[:3, 3]


def unapply_T(T, p):
    """src with apply_T(T, src) == p, exact for the signed permutations above."""
    return p if T is None else (p - T[:3, 3]) @ T[:3, :3]


# ---- the grid's cell of a coordinate ---------------------------------------------------------------------------------
def inv_cell(r):
    return (1.0 - 1e-9) / r


def cell_of(x, r):
    return np.floor(np.asarray(x, np.float64) * inv_cell(r))


def in_cell(c, r):
    """A coordinate in the middle of cell c."""
    return (c + 0.5) * r


# ---- brute-force restatements (float64, chunked) ---------------------------------------------------------------------
def _chunks(n, m):
    step = max(1, (1 << 22) // max(m, 1))
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def dist2(p, q):
    """[len(p), len(q)] squared distances, (ex^2 + ey^2) + ez^2 of e = q - p as the kernels form it."""
    e = q[None, :, :] - p[:, None, :]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def nearest_brute(p, dst, r):
    """Nearest target within d^2 < r^2 (strict), ties to the lowest target index: (ok bool, j, d2) per row of p."""
    p, dst = np.asarray(p, np.float64), np.asarray(dst, np.float64)
    r2 = r * r
    ok, j, d2 = np.zeros(len(p), bool), np.zeros(len(p), np.int64), np.zeros(len(p))
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b in _chunks(len(p), len(dst)):
            D = dist2(p[a:b], dst)
            D = np.where(D < r2, D, np.inf)               # NaN compares false
            k = np.argmin(D, 1)                           # the first minimum: the lowest index
            d = D[np.arange(b - a), k]
            ok[a:b] = np.isfinite(d)
            j[a:b] = np.where(ok[a:b], k, 0)
            d2[a:b] = np.where(ok[a:b], d, 0.0)
    return ok, j, d2


def radius_brute(src, dst, T, r):
    """Every (i, j) with |T src_i - dst_j|^2 <= r^2, rows ascending in i then j: (pairs int32 [P, 2], offsets int64
    [n_src + 1], counts int32 [n_src])."""
    p, dst = apply_T(T, src), np.asarray(dst, np.float64)
    r2 = r * r
    rows, counts = [], np.zeros(len(p), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b in _chunks(len(p), len(dst)):
            hit = dist2(p[a:b], dst) <= r2
            i, j = np.nonzero(hit)
            rows.append(np.stack([i + a, j], 1))
            counts[a:b] = hit.sum(1)
    pairs = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 2), np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    return pairs, offsets, counts


def icp_brute(src, dst, r, init=None, max_iteration=30, rotation=None):
    """kitti_restate.icp_restated on the brute-force neighbour search (ties to the lowest index)."""
    dst = np.asarray(dst, np.float64)
    return icp_restated(src, dst, r, init, max_iteration, nearest=lambda p: nearest_brute(p, dst, r), rotation=rotation)


def rotation_svd(H):
    """The rotation of the fit before the rank rule: V diag(1, 1, det) U^T of LAPACK's SVD."""
    U, _, Vt = np.linalg.svd(H)
    return Vt.T @ np.diag([1, 1, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T


def fit_ruled(src, dst):
    """The rank-ruled fit, row-major 3x4 [R | t] (imf_oracle.rigid_fit: two-pass covariance, `rigid_rotation`)."""
    return O.rigid_fit(np.asarray(src, np.float64), np.asarray(dst, np.float64))[:3]


def rotation_defects(R):
    """(max |R^T R - I|, |det R - 1|): the two gates of a proper rotation."""
    R = np.asarray(R, np.float64)
    return float(np.abs(R.T @ R - np.eye(3)).max()), float(abs(np.linalg.det(R) - 1.0))


def residual(T, src, dst):
    T = np.asarray(T, np.float64)
    e = np.asarray(src, np.float64) @ T[:3, :3].T + T[:3, 3] - np.asarray(dst, np.float64)
    return float((e * e).sum())


# ---- radius / neighbour cases ------------------------------------------------------------------------------------------
class PairCase(NamedTuple):
    name: str
    src: np.ndarray
    dst: np.ndarray
    r: float
    T: Optional[np.ndarray]
    exact: bool                 # dyadic: every d^2 is exact


def _dyadic(rng, n, lo, hi):
    return rng.integers(lo, hi, (n, 3)).astype(np.float64) * Q


LAUNCH_N_SRC = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 65793)
LAUNCH_N_DST = (1, 2, 511, 512, 513, 1025)


def launch_cases():
    """Block, wavefront and scan edges of the per-point launches and of the two one-workgroup scans; table capacities
    1024 (n_dst <= 512), 2048 and 4096; 258 partial-sum rows at n_src = 65 793 (more than one per thread of k_icp_fit)."""
    out = []
    for k, n_src in enumerate(LAUNCH_N_SRC):
        n_dst = 513 if n_src == 65793 else LAUNCH_N_DST[k % len(LAUNCH_N_DST)]
        rng = np.random.default_rng(1000 + n_src)
        T = EXACT_TRANSFORMS[k % len(EXACT_TRANSFORMS)]
        dst = _dyadic(rng, n_dst, -1024, 1024) if n_dst > 2 else _dyadic(rng, n_dst, -128, 128)
        moved = _dyadic(rng, n_src, -1024, 1024) if n_src > 1 else dst[:1] + np.array([[16, -8, 4]]) * Q
        out.append(PairCase(f"launch_{n_src}x{n_dst}", unapply_T(T, moved), dst, 0.25, T, True))
    return out


R_EDGE = 0.625


def boundary_cases():
    """Cell boundaries (multiples of r on both sides of 0) and the bound itself: pairs at exactly r along an axis and on
    a diagonal ((0.375, 0.5, 0) at r = 0.625) count for the radius search and not for ICP; r -+ one ulp of a coordinate."""
    r = R_EDGE
    g = np.arange(-3, 4) * r
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    out = [PairCase("multiples_of_r", lattice, lattice, r, None, True)]
    at_r = []
    for base in (np.zeros(3), np.array([-3 * r, 2 * r, -r])):
        for ax in range(3):
            for sgn in (1.0, -1.0):
                e = np.zeros(3); e[ax] = sgn * r
                at_r.append(base + e)
        for sx in (1.0, -1.0):
            for sy in (1.0, -1.0):
                at_r.append(base + np.array([sx * 0.375, sy * 0.5, 0.0]))
                at_r.append(base + np.array([0.0, sx * 0.375, sy * 0.5]))
    bases = np.array([[0.0, 0.0, 0.0], [-3 * r, 2 * r, -r]])
    out.append(PairCase("exactly_r", np.array(at_r), bases, r, None, True))
    ulp = []
    for ax in range(3):
        for sgn in (1.0, -1.0):
            for toward in (0.0, 2.0):                                     # r - ulp (inside), r + ulp (outside)
                e = np.zeros(3); e[ax] = sgn * np.nextafter(r, toward)
                ulp.append(e)
    out.append(PairCase("r_plus_minus_ulp", np.array(ulp), np.zeros((1, 3)), r, None, False))
    return out


R_RANGE = 2.0 ** -7                                   # the key range ends near |x| = 2^17 r = 1024


def range_cases():
    """Targets in the last permitted cell of every axis and sign; queries in the outermost cell (one of them within r of
    such a target), beyond it, and NaN; queries at one end of the key range with targets at the other end, where the 18-bit
    key of a neighbour cell wraps: no pair."""
    r = R_RANGE
    mid = in_cell(5, r)
    dst, src, wrap_dst, wrap_src = [], [], {1.0: [], -1.0: []}, {1.0: [], -1.0: []}
    for ax in range(3):
        for last, outer, beyond, step in ((TARGET_CELLS[1], QUERY_CELLS[1], QUERY_CELLS[1] + 1, 1.0),
                                          (TARGET_CELLS[0], QUERY_CELLS[0], QUERY_CELLS[0] - 1, -1.0)):
            t = np.full(3, mid); t[ax] = in_cell(last, r)
            dst.append(t)
            src.append(t.copy())                                           # the target itself
            q = t.copy(); q[ax] += step * 0.75 * r; src.append(q)          # outermost cell, within r of the target
            q = t.copy(); q[ax] = in_cell(outer, r) + step * 0.25 * r; src.append(q)   # outermost cell, beyond r
            q = t.copy(); q[ax] = in_cell(beyond, r); src.append(q)        # beyond the range
            w = np.full(3, mid); w[ax] = in_cell(last, r); wrap_dst[step].append(w)
            w = np.full(3, mid); w[ax] = in_cell(QUERY_CELLS[0] if step > 0 else QUERY_CELLS[1], r); wrap_src[step].append(w)
    src.append(np.array([np.nan, mid, mid]))
    src.append(np.array([mid, mid, np.nan]))
    return [PairCase("range_last_cells", np.array(src), np.array(dst), r, None, False),
            PairCase("range_key_wrap_high_targets", np.array(wrap_src[1.0]), np.array(wrap_dst[1.0]), r, None, True),
            PairCase("range_key_wrap_low_targets", np.array(wrap_src[-1.0]), np.array(wrap_dst[-1.0]), r, None, True)]


def refused_targets():
    """(name, dst, r): a target in the first refused cell of an axis and sign, and a NaN target -> ImfError."""
    r = R_RANGE
    mid = in_cell(5, r)
    out = []
    for ax in range(3):
        for c in (TARGET_CELLS[1] + 1, TARGET_CELLS[0] - 1):
            d = np.full((3, 3), mid); d[1, ax] = in_cell(c, r)
            out.append((f"refused_axis{ax}_{'pos' if c > 0 else 'neg'}", d, r))
    d = np.full((3, 3), mid); d[2, 1] = np.nan
    out.append(("refused_nan", d, r))
    return out


def crowded_cases():
    """One cell holding 1 500 targets with exact duplicates; one target in every cell of eight 4x4x4-cell blocks (the hash's
    64-slot windows); 3 000 cells spread over +-2^16 that all want the first slot of their window (double hashing)."""
    rng = np.random.default_rng(77)
    r = 0.25
    distinct = 0.25 + rng.integers(8, 248, (400, 3)).astype(np.float64) * Q
    dst = distinct[rng.integers(0, 400, 1500)]
    src = 0.25 + rng.integers(-128, 384, (64, 3)).astype(np.float64) * Q
    out = [PairCase("crowded_cell", src, dst, r, None, True)]
    c = np.stack(np.meshgrid(*[np.arange(-4, 4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    dst = (c * 256 + rng.integers(16, 240, c.shape)).astype(np.float64) * Q          # cell c, 256 Q = r per cell
    out.append(PairCase("block_lattice", _dyadic(rng, 1025, -1100, 1100), dst[rng.permutation(len(dst))], r,
                        EXACT_TRANSFORMS[1], True))
    r = R_RANGE
    cells = np.unique(4 * rng.integers(-(1 << 14), 1 << 14, (3000, 3)), axis=0)
    cells = cells[rng.permutation(len(cells))]
    dst = in_cell(cells, r)
    src = np.concatenate([dst[::3] + np.array([0.5 * r, 0.0, 0.0]), dst[1::7] + np.array([0.0, -r, 0.0]),
                          dst[2::11] + np.array([0.25 * r, 0.25 * r, 1.5 * r])])
    out.append(PairCase("far_cells_double_hash", src, dst, r, None, True))
    return out


def tie_cases():
    """Two and three targets at one exact distance from the query, the lowest index in the cell that the 27-cell probe
    reaches LAST (+1, +1, +1), the others in earlier cells; exact duplicates of the nearest target."""
    r = 0.25
    q = np.full(3, 0.25 - Q)                                               # cell (0, 0, 0), one step from (1, 1, 1)
    a = 2 * Q
    t0 = q + np.array([a, a, a])                                           # cell (1, 1, 1)
    t1 = q + np.array([-a, -a, -a])                                        # cell (0, 0, 0)
    t2 = q + np.array([a, -a, a])                                          # cell (1, 0, 1)
    far = q + np.array([0.125, 0.0, 0.0])
    return [PairCase("tie_two", q[None], np.array([t0, t1, far]), r, None, True),
            PairCase("tie_three", q[None], np.array([t0, t2, t1, far]), r, None, True),
            PairCase("duplicates", q[None], np.array([far, t1, t1, t1, t0 + Q]), r, None, True)]


def random_pair_cases():
    """Non-tie random scenes, where cKDTree is a second reference for the restatements."""
    rng = np.random.default_rng(4)
    a = scene_points(rng, 3000).astype(np.float64)
    b = scene_points(rng, 2500).astype(np.float64)
    return [PairCase("scene_r045", a, b, 0.45, rigid(1.0, [0, 0, 1], [0.2, -0.1, 0.0]), False),
            PairCase("scene_r0075", a, a[::2] + rng.normal(0, 0.02, a[::2].shape), 0.075, None, False)]


def pair_cases():
    return launch_cases() + boundary_cases() + range_cases() + crowded_cases() + tie_cases() + random_pair_cases()


# ---- ICP cases -------------------------------------------------------------------------------------------------------
class IcpCase(NamedTuple):
    name: str
    src: np.ndarray
    dst: np.ndarray
    r: float
    init: Optional[np.ndarray]
    max_iteration: int
    kind: str                   # "dyadic": exact first stage, T to 1e-12 (1 + max |x|); "random": 1e-9; "degenerate": + the gates
    rank: int                   # rank of the first update's covariance (3 = full)


def _icp_lattice_case(n_src, n_dst, max_iteration, seed):
    """Targets on a 0.5 lattice (dyadic jitter <= 2^-5), every source point a jittered, shifted copy of one target: its
    correspondence is unique by a wide margin at every stage; one source point in ten is far from every target."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(-6, 6)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[np.argsort(np.abs(g).sum(1), kind="stable")]                     # the origin first
    dst = g[:n_dst] * 0.5
    if n_dst > 2:
        dst = dst + rng.integers(-32, 33, dst.shape) * Q
    src = dst[rng.integers(0, n_dst, n_src)] + rng.integers(-32, 33, (n_src, 3)) * Q + np.array([32, -16, 16]) * Q
    far = rng.random(n_src) < 0.1
    src[far] += 64.0
    return IcpCase(f"icp_launch_{n_src}x{n_dst}_it{max_iteration}", src, dst, 0.25, None, max_iteration, "dyadic",
                   0 if n_dst == 1 else (1 if n_dst == 2 else 3))


def icp_cases():
    out = []
    its = (3, 0, 1)
    for k, n_src in enumerate(LAUNCH_N_SRC):
        n_dst = 513 if n_src == 65793 else LAUNCH_N_DST[k % len(LAUNCH_N_DST)]
        if n_src < 4 and n_dst > 2:
            continue
        out.append(_icp_lattice_case(n_src, n_dst, its[k % 3], 2000 + n_src))
    # the bound and the ties: one stage, the statistics and the chosen target are the result
    for c in boundary_cases():
        out.append(IcpCase("icp_" + c.name, c.src, c.dst, c.r, None, 0, "dyadic", 3))
    for c in tie_cases():
        out.append(IcpCase("icp_" + c.name, c.src, c.dst, c.r, None, 1, "degenerate", 0))
    for c in range_cases():
        out.append(IcpCase("icp_" + c.name, c.src, c.dst, c.r, None, 1, "dyadic", 3))
    c = crowded_cases()[0]
    out.append(IcpCase("icp_crowded_cell", c.src, c.dst, c.r, None, 1, "dyadic", 3))
    # degenerate fits
    near = np.array([[16, -8, 4], [-32, 8, 0], [8, 8, 8], [0, -16, 24], [40, 0, -8]]) * Q
    far = np.array([[9.0, 9.0, 9.0], [-7.0, 3.0, 1.0]])
    for it in (0, 1, 3):
        out.append(IcpCase(f"one_target_at_0_it{it}", np.concatenate([near, far]), np.zeros((1, 3)), 0.25, None, it,
                           "degenerate", 0))
    d = np.array([[0.5, -0.25, 1.0]])
    out.append(IcpCase("one_target_four_sources", np.concatenate([d + near[:4], far]), d, 0.25, None, 3, "degenerate", 0))
    g = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.5
    out.append(IcpCase("one_source_within_r", np.concatenate([g[37:38] + near[:1], far + 20.0]), g, 0.25, None, 3,
                       "degenerate", 0))
    out.append(IcpCase("two_correspondences", np.array([[-0.125, -0.03125, 0.0], [0.125, 0.03125, 0.0]]),
                       np.array([[0.0, -0.125, 0.0], [0.0, 0.125, 0.0]]), 0.25, None, 1, "degenerate", 1))
    line = np.arange(4)[:, None] * np.array([[0.5, 0.0, 0.0]])
    out.append(IcpCase("collinear_on_axis", line + np.array([0.0625, 0.0, 0.0]), line, 0.25, None, 3, "degenerate", 1))
    out.append(IcpCase("collinear_on_axis_quarter_init", unapply_T(transform(QUARTER_Z, [0.0, 0.0, 0.0]),
                                                                  line + np.array([0.0625, 0.0, 0.0])), line, 0.25,
                       transform(QUARTER_Z, [0.0, 0.0, 0.0]), 3, "degenerate", 1))
    plane = np.stack(np.meshgrid(np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 2) * 0.5
    plane = np.concatenate([plane, np.zeros((16, 1))], 1)
    Tz = rigid(3.0, [0, 0, 1], [0.03, -0.02, 0.0])
    out.append(IcpCase("coplanar_rank2", (plane - Tz[:3, 3]) @ Tz[:3, :3], plane, 0.25, None, 3, "degenerate", 2))
    out.append(IcpCase("no_correspondence", near + 50.0, g, 0.25, transform(QUARTER_Z, [0.5, 0.0, 0.0]), 3, "dyadic", 3))
    # random full rank
    rng = np.random.default_rng(21)
    dst = scene_points(rng, 1025).astype(np.float64)
    Tt = rigid(2.0, [0.2, 0.3, 1.0], [0.2, 0.0, 0.05])
    src = ((dst - Tt[:3, 3]) @ Tt[:3, :3] + rng.normal(0, 0.002, dst.shape))
    src = np.concatenate([src, src[:1024] + rng.normal(0, 0.01, (1024, 3))])
    out.append(IcpCase("scene_full_rank", src, dst, 1.0, None, 30, "random", 3))
    out.append(IcpCase("scene_full_rank_init", src, dst, 0.5, rigid(1.5, [0.2, 0.3, 1.0], [0.15, 0.02, 0.0]), 3, "random", 3))
    return out


def offset_scene():
    """A street-like scene 3.6 km from the origin, one iteration: the conditioning of the one-pass covariance
    sum s d^T - (sum s) md^T.  Returns (src, dst, r)."""
    rng = np.random.default_rng(31)
    dst = scene_points(rng, 4000).astype(np.float64)
    Tt = rigid(2.0, [0.2, 0.3, 1.0], [0.2, 0.0, 0.05])
    src = (dst - Tt[:3, 3]) @ Tt[:3, :3] + rng.normal(0, 0.002, dst.shape)
    off = np.array([3000.0, -2000.0, 500.0])
    return src + off, dst + off, 1.0


def offset_scene_references(src, dst, r):
    """(T_ld, T_onepass64, n_corr): the first update on the brute-force correspondences, by a numpy.longdouble two-pass
    (centred) covariance, and by a float64 evaluation of the one-pass formula; the rotation of either from LAPACK."""
    ok, j, _ = nearest_brute(src, dst, r)
    S, D = src[ok], dst[j[ok]]
    Sl, Dl = S.astype(np.longdouble), D.astype(np.longdouble)
    msl, mdl = Sl.sum(0) / len(Sl), Dl.sum(0) / len(Dl)
    Hl = (Sl - msl).T @ (Dl - mdl)
    R = rotation_svd(Hl.astype(np.float64))
    T_ld = np.eye(4)
    T_ld[:3, :3] = R
    T_ld[:3, 3] = (mdl - R.astype(np.longdouble) @ msl).astype(np.float64)
    n = float(len(S))
    ss, sd = S.sum(0), D.sum(0)
    ms, md = ss * (1.0 / n), sd * (1.0 / n)
    H = S.T @ D - np.outer(ss, md)
    R = rotation_svd(H)
    T_64 = np.eye(4)
    T_64[:3, :3] = R
    T_64[:3, 3] = md - R @ ms
    return T_ld, T_64, int(ok.sum())


# ---- the fit's own cases (through imf_host_rigid_fit) -----------------------------------------------------------------
def fit_cases():
    """(name, src, dst, rank, expected R or None).  Exact zeros: constant coordinates are 0, counts are powers of two."""
    I = np.eye(3)
    line = np.array([[1.0, 0, 0], [2.0, 0, 0], [4.0, 0, 0], [5.0, 0, 0]])
    half_y = np.diag([-1.0, 1.0, -1.0])                                    # opposite along x: e_y is the axis
    out = [("one_pair", [[1.0, 2.0, 3.0]], [[4.0, 5.0, 6.0]], 0, I),
           ("shared_target", [[1.0, 2, 3], [2.0, -1, 0], [0.5, 0.25, 4], [-3.0, 1, 1]], [[4.0, 5.0, 6.0]] * 4, 0, I),
           ("shared_source", [[4.0, 5.0, 6.0]] * 2, [[1.0, 2, 3], [2.0, -1, 0]], 0, I),
           ("all_identical", [[0.5, 0.5, 0.5]] * 4, [[1.0, 2.0, 3.0]] * 4, 0, I),
           ("axis_collinear_issue", [[1.0, 0, 0], [2.0, 0, 0], [4.0, 0, 0]], [[1.0, 0, 0], [2.0, 0, 0], [4.0, 0, 0]], 1, I),
           ("axis_collinear_shift", line, line + np.array([0.5, 0, 0]), 1, I),
           ("axis_collinear_quarter", line, line @ QUARTER_Z.T, 1, QUARTER_Z),
           ("axis_collinear_opposite", line, -line, 1, half_y),
           ("axis_y_opposite", line[:, [1, 0, 2]], -line[:, [1, 0, 2]], 1, np.diag([1.0, -1.0, -1.0])),
           ("axis_z_to_x", line[:, [1, 2, 0]], line, 1, np.array([[0.0, 0, 1], [0, 1, 0], [-1.0, 0, 0]])),
           ("two_pairs_diagonal", [[1.0, 1, 0], [-1.0, -1, 0]], [[-1.0, 1, 0], [1.0, -1, 0]], 1, QUARTER_Z),
           ("two_pairs_generic", [[-0.125, -0.03125, 0.0], [0.125, 0.03125, 0.0]], [[0.0, -0.125, 0.0], [0.0, 0.125, 0.0]], 1,
            None)]
    plane = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), indexing="ij"), -1).reshape(-1, 2)
    plane = np.concatenate([plane, np.zeros((16, 1))], 1)
    out.append(("coplanar_quarter", plane, plane @ QUARTER_Z.T + np.array([0.5, 0, 0]), 2, QUARTER_Z))
    Tz = rigid(33.0, [0, 0, 1], [0.3, -0.2, 0.0])
    out.append(("coplanar_rotated", plane, plane @ Tz[:3, :3].T + Tz[:3, 3], 2, Tz[:3, :3]))
    return [(n, np.asarray(s, np.float64), np.asarray(d, np.float64), k, R) for n, s, d, k, R in out]


def full_rank_fit_cases():
    rng = np.random.default_rng(8)
    out = []
    for n in (3, 4, 5, 64, 1000, 20000):
        s = rng.normal(0, 3.0, (n, 3))
        T = rigid(rng.uniform(0, 170), rng.normal(size=3), rng.normal(size=3))
        out.append((f"full_{n}", s, s @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.01, s.shape)))
    s = rng.normal(0, 3.0, (6, 3))
    out.append(("reflection_wanted", s, s * np.array([1.0, 1.0, -1.0]) + rng.normal(0, 0.01, s.shape)))
    return out


def near_collinear_fit_cases():
    """Generic, inexact near-collinear sets: the covariance is rank 1 up to rounding, the completion is arbitrary."""
    rng = np.random.default_rng(9)
    out = []
    for k, n in enumerate((2, 3, 7, 16, 100)):
        dirn = rng.normal(size=3)
        s = rng.normal(size=(n, 1)) * dirn + rng.normal(size=3)
        T = rigid(rng.uniform(0, 179), rng.normal(size=3), rng.normal(size=3))
        d = s @ T[:3, :3].T + T[:3, 3]
        if k % 2:
            d = d + rng.normal(0, 1e-13, d.shape)
        out.append((f"near_collinear_{n}", s, d))
    s = np.arange(5.0)[:, None] * np.array([[1.0, 2.0, 3.0]])
    out.append(("near_opposite", s, -s + rng.normal(0, 1e-9, s.shape)))
    return out


# ---- RANSAC cases ------------------------------------------------------------------------------------------------------
class RansacCase(NamedTuple):
    name: str
    src: np.ndarray
    dst: np.ndarray
    corres: np.ndarray
    ransac_n: int
    max_dist: float
    edge: float
    max_iter: int
    seed: int
    kind: str                   # "generic", "lattice" (an exact quarter turn: every full-rank hypothesis fits all), "tie"


def _generic_ransac(rng, n):
    src = rng.uniform(-1.0, 1.0, (n, 3))
    Tg = rigid(25.0, [0.3, -0.2, 1.0], [0.4, 0.1, -0.3])
    dst = src @ Tg[:3, :3].T + Tg[:3, 3] + rng.normal(0, 0.005, src.shape)
    bad = rng.random(n) < 0.3
    if n > 5:
        dst[bad] += rng.normal(0, 0.5, (int(bad.sum()), 3))
    perm = rng.permutation(n)
    inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
    return src, dst[perm], inv.astype(np.int32)


def ransac_cases():
    out = []
    iters = (1, 1023, 1024, 1025)
    for k, n in enumerate((3, 4, 5, 63, 64, 65)):
        rng = np.random.default_rng(300 + n)
        src, dst, corres = _generic_ransac(rng, n)
        for m, it in enumerate(iters if n in (3, 65) else (iters[k % 4], 1025)):
            out.append(RansacCase(f"generic_n{n}_it{it}", src, dst, corres, 3 + (k + m) % 2, 0.075, 0.9, it, 10 + k, "generic"))
    # a dyadic lattice under an exact quarter turn: every full-rank hypothesis fits every point, but through a Jacobi /
    # LAPACK rotation that is exact only to rounding, so their rmse are 1e-16 noise, not 0, and WHICH of them wins is
    # not comparable between two implementations; the count, nvalid and T are.  The exact ties are the "tie" cases below.
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.25
    T = transform(QUARTER_Z, [0.5, -0.25, 0.125])
    for n, rn, it in ((5, 3, 1024), (64, 4, 1025), (64, 3, 1023)):
        out.append(RansacCase(f"lattice_n{n}_rn{rn}_it{it}", g[:n], apply_T(T, g[:n]), np.arange(n, dtype=np.int32), rn, 0.075,
                              0.9, it, 3, "lattice"))
    # exact ties: every valid hypothesis is a pure translation (rank 0) with every member of its cluster as an exact
    # inlier and rmse == 0; mixed samples fail the edge-length checker.  The earliest valid hypothesis must win.
    same_s, same_d = np.tile([[0.5, 0.25, -1.0]], (64, 1)), np.tile([[1.5, -0.75, 2.0]], (64, 1))
    for rn, it in ((3, 1), (4, 1025)):
        out.append(RansacCase(f"all_identical_rn{rn}_it{it}", same_s, same_d, np.arange(64, dtype=np.int32), rn, 0.075, 0.9,
                              it, 5, "tie"))
    s2, d2 = same_s.copy(), same_d.copy()
    s2[1::2] = [2.0, 2.0, 2.0]
    d2[1::2] = [-8.0, 4.0, 16.0]
    for rn, it, seed in ((3, 1025, 0), (4, 1025, 1), (3, 1024, 2)):
        out.append(RansacCase(f"two_clusters_rn{rn}_it{it}_s{seed}", s2, d2, np.arange(64, dtype=np.int32), rn, 0.075, 0.9, it,
                              seed, "tie"))
    return out


def ransac_table(c):
    """Per hypothesis, as imf_oracle.ransac_registration scores them: (picks [it, n], valid bool [it], inlier count
    [it] (-1 invalid), rmse [it], T [it, 4, 4])."""
    src, dst = np.asarray(c.src, np.float64), np.asarray(c.dst, np.float64)
    n = len(src)
    it = np.arange(c.max_iter, dtype=np.uint64)
    picks = np.stack([(O._splitmix64(np.uint64(c.seed) ^ (it * np.uint64(4) + np.uint64(j))) % np.uint64(n)).astype(np.int64)
                      for j in range(c.ransac_n)], 1)
    S, D = src[picks], dst[c.corres[picks]]
    ok = np.ones(c.max_iter, bool)
    for i in range(c.ransac_n):
        for j in range(i + 1, c.ransac_n):
            ds = np.linalg.norm(S[:, i] - S[:, j], axis=1)
            dd = np.linalg.norm(D[:, i] - D[:, j], axis=1)
            ok &= ~((ds < dd * c.edge) | (dd < ds * c.edge))
    T = O.rigid_fit(S, D)
    moved = S @ np.swapaxes(T[:, :3, :3], 1, 2) + T[:, None, :3, 3]
    ok &= ~(np.linalg.norm(moved - D, axis=2) > c.max_dist).any(1)
    tgt = dst[c.corres]
    dis = np.linalg.norm(src[None] @ np.swapaxes(T[:, :3, :3], 1, 2) + T[:, None, :3, 3] - tgt[None], axis=2)
    inl = dis < c.max_dist
    count = np.where(ok, inl.sum(1), -1)
    rmse = np.sqrt(np.where(inl, dis * dis, 0.0).sum(1) / np.maximum(inl.sum(1), 1))
    return picks, ok, count, rmse, T
