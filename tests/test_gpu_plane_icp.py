"""imf_icp_point_to_plane (csrc/icp.hip) against the NumPy restatement (tests/plane_icp_restate.py).

Tolerances.  For every compared case the restatement runs twice on the CPU, with the source in forward and in reversed
order; the kernel gets 16 times what T, fitness and rmse moved between the two, at least 1e-12
(plane_icp_restate.tolerances).  The iteration count and the number of correspondences must be equal."""
import numpy as np
import pytest

import plane_icp_restate as PR
import registration_cases as RC

pytestmark = pytest.mark.gpu


def _compare(src, dst, nrm, r, init, max_iteration, name):
    from imfnet_amd.matching import icp_point_to_plane
    fwd, rev, moved, tol = PR.tolerances(src, dst, nrm, r, init, max_iteration)
    T, fit, rmse, iters, n_corr = icp_point_to_plane(src, dst, nrm, r, init=init, max_iteration=max_iteration)
    err = (float(np.abs(T - fwd[0]).max()), abs(fit - fwd[1]), abs(rmse - fwd[2]))
    print(f"{name}: iterations {iters} (restated {fwd[3]}), n_corr {n_corr} (restated {fwd[4]}), order moved {moved}, "
          f"bounds {tol}, kernel off by {err}")
    assert fwd[3] == rev[3] and fwd[4] == rev[4]
    assert iters == fwd[3] and n_corr == fwd[4]
    assert err[0] <= tol[0] and err[1] <= tol[1] and err[2] <= tol[2]
    again = icp_point_to_plane(src, dst, nrm, r, init=init, max_iteration=max_iteration)
    assert again[0].tobytes() == T.tobytes() and again[1:] == (fit, rmse, iters, n_corr)      # equal bits
    return T, fwd


@pytest.fixture(scope="module")
def bumpy():
    return PR.bumpy_case()


def test_one_iteration_from_a_known_init(bumpy):
    src, dst, nrm, r, truth = bumpy
    init = truth @ PR.rigid(1.0, [1.0, 0.2, -0.4], np.array([0.004, 0.003, -0.002]))
    T, fwd = _compare(src, dst, nrm, r, init, 1, "one iteration")
    assert fwd[3] == 1 and fwd[4] == len(src) <= 2048 and np.abs(T - init).max() > 1e-3


def test_convergence_from_three_degrees_and_two_centimetres(bumpy):
    src, dst, nrm, r, truth = bumpy
    T, fwd = _compare(src, dst, nrm, r, None, 30, "convergence")
    assert 2 <= fwd[3] < 30 and np.abs(fwd[0] - truth).max() < 1e-6 and np.abs(T - truth).max() < 1e-6


def test_ties_go_to_the_lowest_target_index(bumpy):
    """Exact duplicates of 300 targets are appended with other normals: the first occurrence, and its normal, must win."""
    src, dst, nrm, r, truth = bumpy
    junk = np.roll(nrm[:300], 1, axis=1) * np.array([1.0, -1.0, 1.0])
    dst2, nrm2 = np.concatenate([dst, dst[:300]]), np.concatenate([nrm, junk])
    init = truth @ PR.rigid(1.0, [1.0, 0.2, -0.4], np.array([0.004, 0.003, -0.002]))
    T, fwd = _compare(src, dst2, nrm2, r, init, 1, "duplicated targets")
    plain = PR.icp_plane_restated(src, dst, nrm, r, init, 1)
    assert np.array_equal(plain[0], fwd[0])                               # the restatement never saw the junk normals


def test_the_bound_is_strict_at_exactly_r():
    c = {c.name: c for c in RC.boundary_cases()}["exactly_r"]
    src = np.concatenate([c.src, c.dst])                                  # every point at exactly r, then the two targets
    nrm = np.tile([[0.0, 0.6, 0.8]], (len(c.dst), 1))
    from imfnet_amd.matching import icp_point_to_plane
    T, fit, rmse, iters, n_corr = icp_point_to_plane(src, c.dst, nrm, c.r, max_iteration=0)
    ref = PR.icp_plane_restated(src, c.dst, nrm, c.r, None, 0)
    assert n_corr == ref[4] == 2 and iters == ref[3] == 0 and fit == ref[1] == 2 / len(src) and rmse == ref[2] == 0.0
    assert np.array_equal(T, np.eye(4))


def test_an_empty_correspondence_set_leaves_the_init():
    c = {c.name: c for c in RC.icp_cases()}["no_correspondence"]
    nrm = np.tile([[0.0, 0.0, 1.0]], (len(c.dst), 1))
    from imfnet_amd.matching import icp_point_to_plane
    got = icp_point_to_plane(c.src, c.dst, nrm, c.r, init=c.init, max_iteration=3)
    ref = PR.icp_plane_restated(c.src, c.dst, nrm, c.r, c.init, 3)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[0], c.init)
    assert got[1:] == (0.0, 0.0, 1, 0) and tuple(ref[1:]) == (0.0, 0.0, 1, 0)


@pytest.mark.parametrize("tilt", [None, (31.0, [0.3, 1.0, -0.2])], ids=["axis_plane", "tilted_plane"])
def test_a_single_plane_target_is_singular_and_the_update_is_the_identity(tilt):
    """J^T J has rank 3 on one plane: a pivot falls under 1e-12 of the largest diagonal entry (exactly 0 on the axis
    plane, rounding noise on the tilted one) and T stays the init."""
    from imfnet_amd.matching import icp_point_to_plane
    g = np.random.default_rng(12)
    plane = np.concatenate([g.uniform(-1, 1, (600, 2)), np.zeros((600, 1))], 1)
    nrm = np.tile([[0.0, 0.0, 1.0]], (600, 1))
    src = plane[::2] + np.array([0.01, -0.005, 0.02])
    if tilt is not None:
        R = PR.rigid(tilt[0], tilt[1], np.zeros(3))[:3, :3]
        plane, nrm, src = plane @ R.T + 0.3, nrm @ R.T, src @ R.T + 0.3
    init = PR.rigid(0.5, [0.0, 0.0, 1.0], np.array([0.001, 0.0, 0.0])) if tilt is None else None
    got = icp_point_to_plane(src, plane, nrm, 0.2, init=init, max_iteration=5)
    ref = PR.icp_plane_restated(src, plane, nrm, 0.2, init, 5)
    want = np.eye(4) if init is None else init
    assert np.array_equal(ref[0], want) and ref[3] == 1
    assert np.array_equal(got[0], want) and got[3] == 1 and got[4] == ref[4] == len(src)
    assert abs(got[1] - ref[1]) == 0.0 and abs(got[2] - ref[2]) <= 1e-12
