"""CPU tests (no GPU) of the registration catalogue (tests/registration_cases.py) and of the rigid fit itself: every exact
case is exact, every tie / boundary / range case contains what it is named for, the brute-force restatements agree with
cKDTree where cKDTree is defined, and csrc/registration.h's fit -- through the host entry imf_host_rigid_fit, the same
rigid_from_cov the kernels call -- returns a proper rotation for every rank and follows the rank rule."""
from fractions import Fraction

import numpy as np
import pytest

import imf_oracle as O
import registration_cases as RC
from kitti_restate import icp_restated, rigid, scene_points

PAIR_CASES = RC.pair_cases()
ICP_CASES = RC.icp_cases()
RANSAC_CASES = RC.ransac_cases()
GATE = 1e-12        # orthonormality and determinant: three orders above a dozen fp64 plane rotations, twelve below det = 0


def host_fit(src, dst):
    from imfnet_amd import _lib
    s, d = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(dst, np.float64)
    T = np.full(12, np.nan)
    assert _lib.lib().imf_host_rigid_fit(s.ctypes.data, d.ctypes.data, len(s), T.ctypes.data) == 0
    return T.reshape(3, 4)


def _svd_T(src, dst):
    """The plain SVD fit (any of the optimal rotations when the rank is below 2): the residual to compare with."""
    R = RC.rotation_svd((src - src.mean(0)).T @ (dst - dst.mean(0)))
    return np.concatenate([R, (dst.mean(0) - R @ src.mean(0))[:, None]], 1)


def _as_units(x):
    u = np.asarray(x, np.float64) / RC.Q
    assert np.array_equal(u, np.round(u)) and np.abs(x).max() < 2.0 ** 10, "not dyadic: multiples of 2^-10 below 2^10"
    return u.astype(np.int64)


# ---- exactness ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in PAIR_CASES if c.exact], ids=lambda c: c.name)
def test_exact_cases_are_exact(c):
    """d^2 in integers scaled by 2^20 equals the float64 value of every pair: no comparison of these cases rounds."""
    p, q = _as_units(RC.apply_T(c.T, c.src)), _as_units(c.dst)
    pf, qf = RC.apply_T(c.T, c.src), np.asarray(c.dst, np.float64)
    for a, b in RC._chunks(len(p), len(q)):
        e = q[None] - p[a:b, None]
        exact = (e * e).sum(-1)                                            # int64, below 2^44
        assert np.array_equal(RC.dist2(pf[a:b], qf) * 2.0 ** 20, exact.astype(np.float64))
    assert RC.Q * round(c.r / RC.Q) == c.r and (c.r * c.r) * 2.0 ** 20 == round(c.r / RC.Q) ** 2


def test_dyadic_icp_cases_are_dyadic():
    for c in ICP_CASES:
        if c.kind == "dyadic" and not np.isnan(c.src).any() and not c.name.startswith("icp_r_plus"):
            _as_units(RC.apply_T(c.init, c.src)), _as_units(c.dst)


# ---- preconditions -----------------------------------------------------------------------------------------------------
def _case(name):
    return next(c for c in PAIR_CASES if c.name == name)


def test_boundary_cases_hold_the_boundary():
    c = _case("exactly_r")
    D = RC.dist2(c.src, c.dst)
    assert (D == c.r * c.r).sum() == len(c.src) and ((D == c.r * c.r).sum(1) == 1).all()      # each query: one pair AT r
    assert any(np.count_nonzero(s - b) == 2 for s in c.src for b in c.dst if ((s - b) ** 2).sum() == c.r ** 2)   # diagonal
    assert RC.radius_brute(c.src, c.dst, None, c.r)[2].sum() == len(c.src)                    # counted by the radius search
    assert not RC.nearest_brute(c.src, c.dst, c.r)[0].any()                                   # excluded by ICP
    c = _case("multiples_of_r")
    k = c.dst / c.r
    assert np.array_equal(k, np.round(k)) and k.min() < 0 < k.max()
    cells = RC.cell_of(c.dst, c.r)
    assert np.array_equal(cells[k > 0], k[k > 0] - 1) and np.array_equal(cells[k <= 0], k[k <= 0])   # x = k r sits in cell k - 1 for k > 0
    counts = RC.radius_brute(c.src, c.dst, None, c.r)[2]
    assert counts.max() == 7 and counts.min() == 4                                             # itself + the axis neighbours at r
    c = _case("r_plus_minus_ulp")
    r2 = Fraction(c.r) ** 2
    inside = np.array([sum(Fraction(float(v)) ** 2 for v in s) < r2 for s in c.src])
    assert inside.sum() == len(c.src) // 2 and all(sum(Fraction(float(v)) ** 2 for v in s) != r2 for s in c.src)
    assert np.array_equal(RC.radius_brute(c.src, c.dst, None, c.r)[2] == 1, inside)           # the float64 test agrees
    assert np.array_equal(RC.nearest_brute(c.src, c.dst, c.r)[0], inside)
    assert all(abs(abs(s).max() - c.r) == np.spacing(c.r) for s in c.src)                     # one ulp of the coordinate


def test_tie_cases_hold_the_tie():
    for name, n_tied in (("tie_two", 2), ("tie_three", 3)):
        c = _case(name)
        D = RC.dist2(c.src, c.dst)[0]
        tied = np.flatnonzero(D == D.min())
        assert len(tied) == n_tied and tied[0] == 0 and D.min() < c.r ** 2
        cells = RC.cell_of(c.dst, c.r) - RC.cell_of(c.src[0], c.r)
        assert np.array_equal(cells[0], [1, 1, 1])                          # the lowest index: the cell probed last
        assert all((cells[t] != 1).any() for t in tied[1:])
        assert RC.nearest_brute(c.src, c.dst, c.r)[1][0] == 0
    c = _case("duplicates")
    D = RC.dist2(c.src, c.dst)[0]
    tied = np.flatnonzero(D == D.min())
    assert np.array_equal(tied, [1, 2, 3]) and (c.dst[tied] == c.dst[1]).all()
    assert RC.nearest_brute(c.src, c.dst, c.r)[1][0] == 1


def test_range_cases_land_in_their_cells():
    c = _case("range_last_cells")
    r = c.r
    lo, hi = RC.TARGET_CELLS
    cd = RC.cell_of(c.dst, r)
    assert cd.min() == lo and cd.max() == hi
    for ax in range(3):
        assert {lo, hi} <= set(cd[:, ax])                                   # every axis, both signs
    cs = RC.cell_of(c.src, r)
    qlo, qhi = RC.QUERY_CELLS
    finite = ~np.isnan(c.src).any(1)
    assert np.isnan(c.src).any() and (cs[finite] == qhi).any() and (cs[finite] == qlo).any()
    assert (cs[finite] == qhi + 1).any() and (cs[finite] == qlo - 1).any()
    pairs, _, counts = RC.radius_brute(c.src, c.dst, None, r)
    outer = finite & ((cs == qhi) | (cs == qlo)).any(1)
    beyond = ~finite | ((cs > qhi) | (cs < qlo)).any(1)
    assert counts[outer].max() == 1 and counts[outer].min() == 0 and counts[beyond].sum() == 0
    for w in (_case("range_key_wrap_high_targets"), _case("range_key_wrap_low_targets")):
        cs, cd = RC.cell_of(w.src, w.r).astype(np.int64), RC.cell_of(w.dst, w.r).astype(np.int64)
        for s, d in zip(cs, cd):
            ax = int(np.flatnonzero(s != d)[0])
            assert (s[ax], d[ax]) in ((qlo, hi), (qhi, lo))
            step = -1 if s[ax] == qlo else 1
            assert ((s[ax] + step) & 0x3FFFF) == ((d[ax] - step) & 0x3FFFF)     # the neighbour's key wraps next to the target's
        assert RC.radius_brute(w.src, w.dst, None, w.r)[2].sum() == 0
    for name, dst, r in RC.refused_targets():
        cd = RC.cell_of(dst, r)
        bad = np.isnan(dst) | (cd < lo) | (cd > hi)
        assert bad.sum() == 1, name
        if not np.isnan(dst).any():
            assert cd[bad][0] in (lo - 1, hi + 1)


def _hash_capacity(n):
    cap = 1024
    while cap < 2 * n:
        cap *= 2
    return cap


def test_crowded_cases_are_crowded():
    c = _case("crowded_cell")
    cells = RC.cell_of(c.dst, c.r)
    assert len(c.dst) == 1500 and (cells == cells[0]).all() and len(c.src) <= 64
    assert len(np.unique(c.dst, axis=0)) < len(c.dst)
    assert RC.radius_brute(c.src, c.dst, None, c.r)[2].max() > 1000
    c = _case("block_lattice")
    cells = RC.cell_of(c.dst, c.r)
    assert len(np.unique(cells, axis=0)) == 512 == len(c.dst) and cells.min() == -4 and cells.max() == 3
    c = _case("far_cells_double_hash")
    cells = RC.cell_of(c.dst, c.r).astype(np.int64)
    assert (cells % 4 == 0).all() and np.abs(cells).max() > 1 << 15 and len(np.unique(cells, axis=0)) == len(cells)
    assert len(cells) > _hash_capacity(len(cells)) // 64                    # more keys than windows: first slots collide
    from imfnet_amd import _lib
    assert _lib.lib().imf_hash_capacity(len(cells)) == _hash_capacity(len(cells))
    assert [_hash_capacity(n) for n in RC.LAUNCH_N_DST] == [1024, 1024, 1024, 1024, 2048, 4096]
    assert RC.radius_brute(c.src, c.dst, None, c.r)[2].sum() > 1000


def test_catalogue_covers_the_launch_edges_and_stays_small():
    names = {c.name for c in PAIR_CASES}
    for k, n in enumerate(RC.LAUNCH_N_SRC):
        assert any(name.startswith(f"launch_{n}x") for name in names)
    assert {len(c.dst) for c in RC.launch_cases()} == set(RC.LAUNCH_N_DST)
    assert (65793 + 255) // 256 == 258                                      # partial-sum rows: more than one per thread of k_icp_fit
    for c in PAIR_CASES + ICP_CASES:
        assert len(c.src) <= 70000 and len(c.dst) <= 70000
    assert {c.max_iteration for c in ICP_CASES if c.kind == "degenerate"} >= {0, 1, 3}
    assert max(c.max_iteration for c in ICP_CASES) <= 30
    assert {len(c.src) for c in RANSAC_CASES} >= {3, 4, 5, 63, 64, 65}
    assert {c.max_iter for c in RANSAC_CASES} == {1, 1023, 1024, 1025} and {c.ransac_n for c in RANSAC_CASES} == {3, 4}


@pytest.mark.parametrize("c", [c for c in ICP_CASES if c.name.startswith("icp_launch") or c.kind == "degenerate"],
                         ids=lambda c: c.name)
def test_icp_cases_have_no_near_ties_after_the_first_stage(c):
    """The first stage is exact (ties and boundary pairs are decided exactly); afterwards the points have moved by a
    rounded update, so every later stage must choose its neighbour, and pass the bound, by a margin far above rounding."""
    dst = np.asarray(c.dst, np.float64)
    stages = []

    def nearest(p):
        D = RC.dist2(p, dst)
        two = np.sort(D, 1)[:, :2] if len(dst) > 1 else np.concatenate([D, np.full_like(D, np.inf)], 1)
        stages.append((np.abs(two[:, 0] - c.r ** 2).min(), (two[:, 1] - two[:, 0])[two[:, 0] < c.r ** 2]))
        return RC.nearest_brute(p, dst, c.r)

    icp_restated(c.src, dst, c.r, c.init, c.max_iteration, nearest=nearest)
    for to_bound, gaps in stages[1:]:
        assert to_bound > 1e-6 and (len(gaps) == 0 or gaps.min() > 1e-6 or len(np.unique(dst, axis=0)) < len(dst))


# ---- restatements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RC.random_pair_cases(), ids=lambda c: c.name)
def test_brute_force_equals_ckdtree_on_random_scenes(c):
    from scipy.spatial import cKDTree
    tree = cKDTree(c.dst)
    moved = RC.apply_T(c.T, c.src)
    pairs, offsets, counts = RC.radius_brute(c.src, c.dst, c.T, c.r)
    ref = tree.query_ball_point(moved, c.r)
    assert np.array_equal(counts, [len(x) for x in ref]) and offsets[-1] == len(pairs) == counts.sum()
    assert np.array_equal(pairs, np.array([(i, j) for i, row in enumerate(ref) for j in sorted(row)], np.int32))
    assert np.array_equal(offsets[1:] - offsets[:-1], counts)
    ok, j, d2 = RC.nearest_brute(moved, c.dst, c.r)
    d, jr = tree.query(moved, k=1, distance_upper_bound=c.r)
    assert np.array_equal(ok, np.isfinite(d)) and np.array_equal(j[ok], jr[ok]) and ok.any() and not ok.all()
    assert np.allclose(np.sqrt(d2[ok]), d[ok], rtol=1e-13, atol=0)


def test_icp_restatement_brute_force_and_rank_rule_leave_full_rank_unchanged():
    """The existing full-rank ICP scenes (tests/test_gpu_kitti.py, smaller): the loop on the brute-force search equals the
    loop on cKDTree, and the rank-ruled rotation equals the plain SVD formula bit for bit."""
    rng = np.random.default_rng(12)
    dst = scene_points(rng, 3000).astype(np.float64)
    Tt = rigid(3.0, [0.2, 0.3, 1.0], [0.5, 0.0, 0.0])
    src = (dst - Tt[:3, 3]) @ Tt[:3, :3] + rng.normal(0, 0.002, dst.shape)
    init = rigid(2.5, [0.2, 0.3, 1.0], [0.45, 0.02, 0.0])
    for r, init_, it in ((1.0, None, 30), (0.2, init, 30), (0.2, init, 3), (0.5, None, 0)):
        old = icp_restated(src, dst, r, init_, it, rotation=RC.rotation_svd)
        new = icp_restated(src, dst, r, init_, it)
        brute = RC.icp_brute(src, dst, r, init_, it)
        assert np.array_equal(old[0], new[0]) and old[1:] == new[1:]
        assert np.array_equal(brute[0], new[0]) and brute[1] == new[1] and brute[3:] == new[3:]
        assert abs(brute[2] - new[2]) <= 1e-13 * new[2]


# ---- the fit, through imf_host_rigid_fit -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,src,dst", RC.full_rank_fit_cases(), ids=[c[0] for c in RC.full_rank_fit_cases()])
def test_host_fit_full_rank_matches_the_oracle(name, src, dst):
    T = host_fit(src, dst)
    assert np.abs(T - O.rigid_fit(src, dst)[:3]).max() <= 1e-12
    assert np.abs(T[:, :3] - RC.rotation_svd((src - src.mean(0)).T @ (dst - dst.mean(0)))).max() <= 1e-12   # unchanged
    orth, det = RC.rotation_defects(T[:, :3])
    assert orth <= GATE and det <= GATE


@pytest.mark.parametrize("name,src,dst,rank,R_expected", RC.fit_cases(), ids=[c[0] for c in RC.fit_cases()])
def test_host_fit_rank_deficient_follows_the_rank_rule(name, src, dst, rank, R_expected):
    T = host_fit(src, dst)
    R = T[:, :3]
    orth, det = RC.rotation_defects(R)
    print(f"{name}: rank {rank}, max|R^T R - I| = {orth:.3e}, det R = {np.linalg.det(R):.17g}")
    assert orth <= GATE, f"{name}: R is not orthonormal: max|R^T R - I| = {orth}, det R = {np.linalg.det(R)}"
    assert det <= GATE, f"{name}: det R = {np.linalg.det(R)}"
    H = (src - src.mean(0)).T @ (dst - dst.mean(0))
    sg = O.jacobi_column_norms(H)
    assert int((sg > sg.max() * 2.0 ** -52).sum()) == rank                 # the case has the rank it is named for
    tol = 1e-12 * (1.0 + max(np.abs(src).max(), np.abs(dst).max()))
    assert np.abs(T - RC.fit_ruled(src, dst)).max() <= tol
    if R_expected is not None:
        assert np.abs(R - R_expected).max() <= 1e-12
        assert np.abs(T[:, 3] - (dst.mean(0) - R_expected @ src.mean(0))).max() <= tol
    if rank == 0:
        assert np.array_equal(R, np.eye(3)) and np.array_equal(T[:, 3], dst.mean(0) - src.mean(0))   # the pure translation
    if rank == 2:
        assert np.abs(R - RC.rotation_svd(H)).max() <= 1e-12              # unique: the SVD answer
    scale = max(np.abs(src).max(), np.abs(dst).max())
    assert RC.residual(T, src, dst) <= RC.residual(_svd_T(src, dst), src, dst) + 1e-12 * scale ** 2


@pytest.mark.parametrize("name,src,dst", RC.near_collinear_fit_cases(), ids=[c[0] for c in RC.near_collinear_fit_cases()])
def test_host_fit_near_collinear_properties(name, src, dst):
    """Rank 1 up to rounding: which completion comes out is not pinned, that it is a proper rotation and as good a fit as
    the SVD's is."""
    T = host_fit(src, dst)
    orth, det = RC.rotation_defects(T[:, :3])
    assert orth <= GATE and det <= GATE
    scale = max(np.abs(src).max(), np.abs(dst).max())
    assert RC.residual(T, src, dst) <= RC.residual(_svd_T(src, dst), src, dst) + 1e-12 * scale ** 2


def test_rotation_between_is_least_angle_and_pins_the_half_turn():
    rng = np.random.default_rng(3)
    u = rng.normal(size=(200, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = rng.normal(size=(200, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    R = O.rotation_between(u, v)
    assert np.abs(np.einsum("nij,nj->ni", R, u) - v).max() < 1e-13
    assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() < 1e-13 and np.abs(np.linalg.det(R) - 1).max() < 1e-13
    axis = np.cross(u, v)
    assert np.abs(np.einsum("nij,nj->ni", R, axis) - axis).max() < 1e-13   # the axis is u x v: no roll about the line
    assert np.abs((np.trace(R, axis1=1, axis2=2) - 1) / 2 - (u * v).sum(1)).max() < 1e-13
    assert np.array_equal(O.rotation_between(u[:3], u[:3]).round(15), np.broadcast_to(np.eye(3), (3, 3, 3)))
    for e, expect in (([1.0, 0, 0], [-1.0, 1, -1]), ([0, 1.0, 0], [1.0, -1, -1]), ([0, 0, 1.0], [1.0, -1, -1])):
        assert np.array_equal(O.rotation_between(np.array(e), -np.array(e)), np.diag(expect))
    w = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)                            # smallest |u_j| is x: the axis is e_x made perpendicular
    Rw = O.rotation_between(w, -w)
    ax = np.array([1.0, 0, 0]) - w[0] * w
    assert np.abs(Rw @ w + w).max() < 1e-15 and np.abs(Rw @ ax - ax).max() < 1e-15


# ---- RANSAC preconditions ----------------------------------------------------------------------------------------------
def test_ransac_tie_cases_are_exact_ties():
    for c in RANSAC_CASES:
        picks, ok, count, rmse, T = RC.ransac_table(c)
        if c.kind == "tie":
            for x in np.unique(np.concatenate([c.src, c.dst])):
                assert ((x + x) + x) * (1.0 / 3.0) == x and (((x + x) + x) + x) * 0.25 == x      # the sample means are exact
            assert ok.any() and (rmse[ok] == 0).all() and len(set(count[ok])) == 1               # every valid one ties
            assert (T[ok][:, :3, :3] == np.eye(3)).all()
            same = (c.src[picks] == c.src[picks][:, :1]).all((1, 2))
            assert np.array_equal(ok, same)                                                      # mixed samples fail
            if "two_clusters" in c.name and c.max_iter > 1:
                first = int(np.flatnonzero(ok)[0])
                other = ok & (T[:, 0, 3] != T[first, 0, 3])
                assert first > 0 and other.any()               # the earliest valid is not hypothesis 0; both clusters tie
        elif c.kind == "lattice":
            repeated = np.array([len(set(p)) < len(p) for p in picks])
            assert ok.all() and repeated.any() and count.max() == len(c.src)
        else:
            assert len(c.src) > 5 or np.array([len(set(p)) < len(p) for p in picks]).mean() > 0.3 or c.max_iter == 1
