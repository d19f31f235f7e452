"""The registration back end on the GPU against the brute-force restatements of tests/registration_cases.py (proved on
the CPU by tests/test_registration_host.py): imf_radius_count / imf_radius_pairs bit for bit over the whole catalogue,
imf_icp_point_to_point on exact, degenerate and random cases and on a scene far from the origin, imf_ransac_registration
hypothesis by hypothesis.  Comparisons called exact use array_equal or ==."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import imf_oracle as O
import registration_cases as RC

pytestmark = pytest.mark.gpu

PAIR_CASES = RC.pair_cases()
ICP_CASES = RC.icp_cases()
RANSAC_CASES = RC.ransac_cases()
GATE = 1e-12
CANARY = 0x5A5A5A5A
GUARD_ROWS = 8


@functools.lru_cache(maxsize=None)
def _radius_ref(name):
    c = next(c for c in PAIR_CASES if c.name == name)
    return RC.radius_brute(c.src, c.dst, c.T, c.r)


def _guarded_pairs(c, capacity):
    """One imf_radius_pairs call whose pair buffer is pre-filled and has GUARD_ROWS rows beyond `capacity`."""
    from imfnet_amd import _lib
    from imfnet_amd._lib import check
    L = _lib.lib()
    s = torch.from_numpy(np.ascontiguousarray(c.src, np.float64)).cuda()
    d = torch.from_numpy(np.ascontiguousarray(c.dst, np.float64)).cuda()
    Th = None if c.T is None else np.ascontiguousarray(c.T, np.float64)
    n_src, n_dst = s.shape[0], d.shape[0]
    nbytes = L.imf_radius_pairs_workspace_bytes(n_src, n_dst)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    offsets = torch.full((n_src + 1,), -7, dtype=torch.int64, device="cuda")
    pairs = torch.full((capacity + GUARD_ROWS, 2), CANARY, dtype=torch.int32, device="cuda")
    out = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    out[1] = 0
    check(L.imf_radius_pairs(s.data_ptr(), n_src, d.data_ptr(), n_dst, Th.ctypes.data_as(C.c_void_p) if Th is not None else None,
                             float(c.r), offsets.data_ptr(), pairs.data_ptr(), int(capacity), out.data_ptr(),
                             out[1:].data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream),
          "imf_radius_pairs")
    total, err = out.tolist()
    return pairs.cpu().numpy(), offsets.cpu().numpy(), int(total), err & 0xFFFFFFFF


@pytest.mark.parametrize("c", PAIR_CASES, ids=lambda c: c.name)
def test_radius_count_and_pairs_equal_the_restatement(c):
    from imfnet_amd.matching import radius_count, radius_pairs
    ref_pairs, ref_offsets, ref_counts = _radius_ref(c.name)
    total = len(ref_pairs)
    n, per = radius_count(c.src, c.dst, c.T, c.r, per_point=True)
    assert n == total and np.array_equal(per, ref_counts)
    assert radius_count(c.src, c.dst, c.T, c.r) == total                    # without the per-point buffer
    pairs, offsets, got_total, err = _guarded_pairs(c, total)               # capacity exactly total: written
    assert err == 0 and got_total == total == n
    assert np.array_equal(offsets, ref_offsets) and np.array_equal(pairs[:total], ref_pairs)
    assert (pairs[total:] == CANARY).all()                                  # nothing beyond total
    assert np.array_equal(np.diff(offsets), per)                            # count and pairs agree with each other
    again = _guarded_pairs(c, total)
    assert np.array_equal(again[0], pairs) and np.array_equal(again[1], offsets) and again[2:] == (total, 0)
    if total:
        short = _guarded_pairs(c, total - 1)                                # one row short: nothing is written
        assert (short[0] == CANARY).all() and short[2] == total and np.array_equal(short[1], ref_offsets)
    wp, wo = radius_pairs(c.src, c.dst, c.T, c.r)                           # the public wrapper (and its second call)
    assert np.array_equal(wp.cpu().numpy(), ref_pairs) and np.array_equal(wo.cpu().numpy(), ref_offsets)


@pytest.mark.parametrize("name,dst,r", RC.refused_targets(), ids=[t[0] for t in RC.refused_targets()])
def test_targets_beyond_the_key_range_are_refused(name, dst, r):
    from imfnet_amd._lib import ImfError
    from imfnet_amd.matching import icp_point_to_point, radius_count, radius_pairs
    src = dst[:1].copy()
    src[np.isnan(src)] = 0.0
    with pytest.raises(ImfError):
        radius_count(src, dst, None, r)
    with pytest.raises(ImfError):
        radius_pairs(src, dst, None, r)
    with pytest.raises(ImfError):
        icp_point_to_point(src, dst, r, None, 1)
    assert radius_count(src, dst[:1], None, r) == 1                         # the permitted rows alone are fine


def _scale(c):
    p = RC.apply_T(c.init, c.src)
    return 1.0 + max(np.abs(p[np.isfinite(p)]).max(), np.abs(c.dst).max())


@pytest.mark.parametrize("c", ICP_CASES, ids=lambda c: c.name)
def test_icp_equals_the_restatement(c):
    from imfnet_amd.matching import icp_point_to_point
    got = icp_point_to_point(c.src, c.dst, c.r, c.init, c.max_iteration)
    ref = RC.icp_brute(c.src, c.dst, c.r, c.init, c.max_iteration)
    T, fit, rmse, iters, n_corr = got
    assert iters == ref[3] and n_corr == ref[4] and fit == ref[1]           # exact
    if c.kind == "random":
        assert np.abs(T - ref[0]).max() < 1e-9 and abs(rmse - ref[2]) <= 1e-9 * ref[2]
    else:
        tol = 1e-12 * _scale(c)
        assert np.abs(T - ref[0]).max() <= tol and abs(rmse - ref[2]) <= tol
    again = icp_point_to_point(c.src, c.dst, c.r, c.init, c.max_iteration)
    assert np.array_equal(again[0], T) and again[1:] == got[1:]             # bit-identical runs
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    orth, det = RC.rotation_defects(T[:3, :3])
    assert orth <= GATE and det <= GATE, f"rotation block: max|R^T R - I| = {orth}, |det - 1| = {det}"
    if c.rank == 0 and c.init is None:
        assert np.array_equal(T[:3, :3], np.eye(3))                         # rank 0: the pure translation
    if len(c.dst) == 1 and c.max_iteration > 0 and n_corr:
        p = c.src[np.linalg.norm(c.src - c.dst[0], axis=1) < c.r]
        assert np.abs(T[:3, 3] - (c.dst[0] - p.mean(0))).max() <= 1e-12 * _scale(c)
    if c.name.startswith("icp_tie") or c.name == "icp_duplicates":
        winner = 1 if c.name == "icp_duplicates" else 0
        assert np.array_equal(T[:3, 3], c.dst[winner] - c.src[0]) and n_corr == 1 and rmse == 0.0


def test_icp_offset_scene_conditioning():
    """One iteration 3.6 km from the origin.  The device forms the covariance in one pass, sum s d^T - (sum s) md^T, which
    cancels ~10 digits there; the gate is 8 times the error that a float64 numpy evaluation of the SAME one-pass formula
    makes against a numpy.longdouble two-pass (centred) restatement.  Measured on the MI355X: see DESIGN.md section 10."""
    from imfnet_amd.matching import icp_point_to_point
    src, dst, r = RC.offset_scene()
    T_ld, T_64, n_ref = RC.offset_scene_references(src, dst, r)
    T, fit, rmse, iters, n_corr = icp_point_to_point(src, dst, r, None, 1)
    err_dev, err_64 = np.abs(T - T_ld).max(), np.abs(T_64 - T_ld).max()
    print(f"offset scene: max|T_device - T_ld| = {err_dev:.3e}, max|T_onepass_f64 - T_ld| = {err_64:.3e}, "
          f"ratio {err_dev / err_64:.2f}")
    assert iters == 1 and n_ref > 3000
    assert err_dev <= 8.0 * err_64
    again = icp_point_to_point(src, dst, r, None, 1)
    assert np.array_equal(again[0], T) and again[1:] == (fit, rmse, iters, n_corr)


@pytest.mark.parametrize("c", RANSAC_CASES, ids=lambda c: c.name)
def test_ransac_equals_the_oracle_hypothesis_by_hypothesis(c):
    """nvalid, the inlier count and the fitness are exact.  The winner is exact wherever the oracle's own scores decide it:
    hypotheses drawn from the same sample set in another order tie up to rounding (1e-16 in rmse), and between those either
    may win; exact ties (kind "tie": rmse == 0 on both sides) must go to the earliest valid hypothesis."""
    from imfnet_amd.matching import ransac_registration
    args = (c.src, c.dst, c.corres, c.ransac_n, c.max_dist, c.edge, c.max_iter, c.seed)
    got = ransac_registration(*args)
    ref = O.ransac_registration(*args)
    picks, ok, count, rmse, Ts = RC.ransac_table(c)
    T, it, inl, nvalid, fit, rm = got
    assert nvalid == int(ok.sum()) == ref[3]
    if not (count > 0).any():                                               # nothing wins: Open3D's default result
        assert it == ref[1] == -1 and inl == 0 and fit == 0.0 and rm == 0.0 and np.array_equal(T, np.eye(4))
        return
    assert ref[1] >= 0 and it >= 0 and ok[it]
    assert inl == ref[2] == count[ok].max() == count[it] and fit == ref[4]
    cand = np.flatnonzero(ok & (count == inl))
    best = rmse[cand].min()
    assert rmse[it] <= best + 1e-12
    if c.kind == "tie":
        assert rm == 0.0 and rmse[it] == 0.0 and it == ref[1] == cand[0]    # the earliest valid hypothesis
        assert np.array_equal(T, Ts[it])
    elif (rmse[cand] <= best + 1e-12).sum() == 1:
        assert it == ref[1]                                                 # decided by the scores: exact
    assert np.abs(T - Ts[it]).max() < 1e-9 and abs(rm - rmse[it]) < 1e-12
    if it == ref[1]:
        assert np.abs(T - ref[0]).max() < 1e-9 and abs(rm - ref[5]) < 1e-12
    orth, det = RC.rotation_defects(T[:3, :3])
    assert orth <= GATE and det <= GATE
    if c.kind == "lattice":
        Tx = RC.transform(RC.QUARTER_Z, [0.5, -0.25, 0.125])
        assert inl == len(c.src) and np.abs(T - Tx).max() < 1e-9 and rm < 1e-12
    again = ransac_registration(*args)
    assert np.array_equal(again[0], T) and again[1:] == got[1:]
