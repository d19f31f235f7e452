"""Float64 NumPy restatement of imf_information_matrix (csrc/information.hip) and the point sets its tests share.
Plain helper module, no GPU dependency.

The rules ([RECALLED] from Open3D's GetInformationMatrixFromPointClouds; no Open3D to check against):
  correspondences: p = T . src[s]; ICP's rule (registration_cases.nearest_brute): the nearest target with d^2 < r^2,
    strict, d^2 = (ex ex + ey ey) + ez ez, ties to the lowest target index; a source row with a NaN has none; a target
    that is NaN or outside the grid's key range (cell edge r) raises the flag;
  the matrix: Lambda = sum G^T G with G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]] of the TARGET point
    q = (x, y, z) = dst[j], rotation first: G (w, v) = w x q + v;
  arithmetic: ten sums K, Sx, Sy, Sz, A00 = sum (y y + z z), A11 = sum (x x + z z), A22 = sum (x x + y y), Pxy, Pxz, Pyz,
    every product and every two-product sum rounded once; L01 = 0 - Pxy, L02 = 0 - Pxz, L04 = 0 - Sz, L05 = Sy, L12 = 0 - Pyz,
    L13 = Sz, L15 = 0 - Sx, L23 = 0 - Sy, L24 = Sx, L33 = L44 = L55 = K, mirrored; an empty set gives 36 times +0.0.
`restate` sums the addends with math.fsum (the correctly rounded sum of the rounded addends: the kernel's fixed-order sum
may differ from it by the bound the GPU test states) and also returns sum |addend| per entry."""
import math
from typing import NamedTuple, Optional

import numpy as np

import registration_cases as RC

NAMES = ("K", "Sx", "Sy", "Sz", "A00", "A11", "A22", "Pxy", "Pxz", "Pyz")
# upper entry (a, b) -> (index into NAMES, sign)
ENTRIES = {(0, 0): (4, 1), (0, 1): (7, -1), (0, 2): (8, -1), (0, 4): (3, -1), (0, 5): (2, 1),
           (1, 1): (5, 1), (1, 2): (9, -1), (1, 3): (3, 1), (1, 5): (1, -1),
           (2, 2): (6, 1), (2, 3): (2, -1), (2, 4): (1, 1),
           (3, 3): (0, 1), (4, 4): (0, 1), (5, 5): (0, 1)}


def G_of(q):
    x, y, z = (float(v) for v in q)
    return np.array([[0.0, z, -y, 1.0, 0.0, 0.0], [-z, 0.0, x, 0.0, 1.0, 0.0], [y, -x, 0.0, 0.0, 0.0, 1.0]])


def correspondences(src, dst, T, r):
    """(ok bool [n_src], j int64 [n_src], flag): ICP's correspondence of every T . src row, and the target error flag."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    p = RC.apply_T(None if T is None else np.asarray(T, np.float64).reshape(4, 4), src)
    ok, j, _ = RC.nearest_brute(p, dst, r)
    ok &= np.isfinite(p).all(1)
    with np.errstate(invalid="ignore"):
        c = RC.cell_of(dst, r)
        flag = int(not bool(((c >= RC.TARGET_CELLS[0]) & (c <= RC.TARGET_CELLS[1])).all()))
    return ok, j, flag


def addends(q):
    """[K, 10] the ten addends of every target point q [K, 3], each rounded as the kernel rounds it."""
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    return np.stack([np.ones(len(q)), x, y, z, yy + zz, xx + zz, xx + yy, x * y, x * z, y * z], 1)


def assemble(sums):
    L = np.zeros((6, 6))
    for (a, b), (k, sign) in ENTRIES.items():
        L[a, b] = L[b, a] = sums[k] if sign > 0 else 0.0 - sums[k]
    return L


def information_from_points(q):
    """Lambda (fsum) of target points q [K, 3]: the matrix of a correspondence set given by its target points."""
    A = addends(np.asarray(q, np.float64).reshape(-1, 3))
    return assemble([math.fsum(A[:, k]) for k in range(10)])


def restate(src, dst, T, r):
    """dict(info 6x6 by math.fsum, n_corr, flag, abs_sum 6x6 = sum |addend| per entry, ok, j)."""
    dst = np.asarray(dst, np.float64)
    ok, j, flag = correspondences(src, dst, T, r)
    A = addends(dst[j[ok]])
    sums = [math.fsum(A[:, k]) for k in range(10)]
    abs_sums = [math.fsum(np.abs(A[:, k])) for k in range(10)]
    return dict(info=assemble(sums), n_corr=int(ok.sum()), flag=flag, abs_sum=np.abs(assemble(abs_sums)), ok=ok, j=j)


class InfoCase(NamedTuple):
    name: str
    src: np.ndarray
    dst: np.ndarray
    T: Optional[np.ndarray]
    r: float
    exact: bool                      # integer lattice: every addend and every sum is an integer below 2^53


def _lattice(rng, n, lim=1 << 10):
    return rng.integers(-lim, lim + 1, (n, 3)).astype(np.float64)


def _lattice_case(name, n_src, n_dst, seed, r=3.0):
    """Integer coordinates |x| <= 2^10, T an integer translation: a share of the sources sits within r of a target."""
    rng = np.random.default_rng(seed)
    dst = _lattice(rng, n_dst)
    t = np.array([5.0, -3.0, 7.0])
    src = _lattice(rng, n_src)
    near = rng.random(n_src) < 0.7
    pick = rng.integers(0, n_dst, n_src)
    src[near] = dst[pick[near]] + rng.integers(-1, 2, (int(near.sum()), 3)) - t
    return InfoCase(name, src, dst, RC.transform(np.eye(3), t), r, True)


def _rotation(rng, angle):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def cases():
    out = [InfoCase("single_pair", np.array([[1.0, 2.0, 3.0]]), np.array([[2.0, 2.0, 4.0]]), None, 2.0, True)]
    for n in (255, 256, 257):
        out.append(_lattice_case(f"lattice_{n}x300", n, 300, n))
    out.append(_lattice_case("lattice_3000x3000", 3000, 3000, 7, r=4.0))
    # general case: ~3000 x 3000 points over many cells (a 2 m cube at r = 0.0375 is ~150 000 cells), non-identity T
    rng = np.random.default_rng(11)
    dst = rng.uniform(-1.0, 1.0, (3000, 3))
    T = RC.transform(_rotation(rng, 0.3), [0.2, -0.1, 0.05])
    moved = dst[rng.permutation(3000)[:2900]] + rng.normal(scale=0.01, size=(2900, 3))
    src = np.concatenate([(moved - T[:3, 3]) @ T[:3, :3], rng.uniform(-3.0, 3.0, (101, 3))])
    out.append(InfoCase("general_3001x3000", src, dst, T, 0.0375, False))
    for n in (255, 256, 257):
        rng = np.random.default_rng(100 + n)
        dst = rng.uniform(-0.5, 0.5, (300, 3))
        src = dst[rng.integers(0, 300, n)] + rng.normal(scale=0.02, size=(n, 3))
        out.append(InfoCase(f"general_{n}x300", src, dst, None, 0.05, False))
    # nothing within r
    out.append(InfoCase("empty", _lattice(np.random.default_rng(5), 300, 64) + 4096.0, _lattice(np.random.default_rng(6), 300, 64),
                        None, 1.5, True))
    return out


def decision_cases():
    """name -> InfoCase with hand-made decisions; every one is on the integer lattice."""
    out = {}
    # 3-4-5: d^2 = 25 exactly
    out["at_r_excluded"] = InfoCase("at_r_excluded", np.array([[3.0, 4.0, 0.0]]), np.array([[0.0, 0.0, 0.0], [100.0, 0.0, 7.0]]),
                                    None, 5.0, True)
    out["at_r_next_up"] = out["at_r_excluded"]._replace(name="at_r_next_up", r=float(np.nextafter(5.0, 6.0)))
    # two targets at d^2 = 4 from the source; the lower index must enter G, and the two give different matrices.  The
    # higher index comes first in x so that a scan in cell order would meet it first.
    out["tie_lowest_index"] = InfoCase("tie_lowest_index", np.array([[10.0, 20.0, 30.0]]),
                                       np.array([[12.0, 20.0, 30.0], [8.0, 20.0, 30.0], [10.0, 22.0, 30.0]]), None, 3.0, True)
    out["tie_lowest_index_swapped"] = out["tie_lowest_index"]._replace(
        name="tie_lowest_index_swapped", dst=out["tie_lowest_index"].dst[[1, 0, 2]].copy())
    rng = np.random.default_rng(21)
    base = _lattice(rng, 40, 32)
    dst = np.concatenate([base, base[:20], base[5:15]])                # every one of the first 20 twice or three times
    out["duplicate_targets"] = InfoCase("duplicate_targets", dst[rng.integers(0, len(dst), 130)] + [1.0, 0.0, 0.0], dst, None,
                                        2.0, True)
    src = base + [0.0, 1.0, 0.0]
    src[3, 1] = np.nan
    src[17] = np.nan
    out["nan_source_rows"] = InfoCase("nan_source_rows", src, base, None, 2.0, True)
    return out


def nan_target_case():
    rng = np.random.default_rng(31)
    dst = _lattice(rng, 50, 32)
    dst[7, 2] = np.nan
    return InfoCase("nan_target", dst[:20] + [0.0, 0.0, 1.0], dst, None, 2.0, True)
