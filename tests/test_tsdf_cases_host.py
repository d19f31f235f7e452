"""The self-checks of the TSDF catalogue (tests/tsdf_cases.py), without a GPU: every case reaches what it was built to reach
(the words of the frame mask, the six cull conditions, the thresholds at exact equality, the float32 poses' distance from
rigid), and the restatement alone, with a fused projection against the plain one, stays inside both caps of the comparison
rule that tests/test_gpu_tsdf_exact.py applies to the kernels."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsdf_cases as TC           # noqa: E402
import tsdf_color_restate as CR   # noqa: E402
import tsdf_restate as R          # noqa: E402
from test_tsdf_color_host import STATE_CAP   # noqa: E402


def fused_against_plain(name, plain, fused):
    d = TC.state_differences(fused, plain)
    print(f"{name}: a fused projection moves (tsdf, w) of {d['differ']} of {d['seen']} voxels, at most {d['worst_unit']} "
          f"in one unit; colour differs alone in {d['colour']}")
    TC.assert_state_rule(d, STATE_CAP)


@pytest.mark.parametrize("offset", TC.A_OFFSETS)
def test_case_a_reaches_every_mask_word_and_stays_inside_the_caps(offset):
    case = TC.case_a(offset)
    assert len(case["units"]) == 64 and case["units"].min() == -2 and case["units"].max() == 1
    assert case["K"][0, 0] != case["K"][1, 1] and case["depth"].shape == (257, 24, 32)
    zeros = (case["depth"] == 0).mean()
    live = case["depth"][case["depth"] != 0]
    assert 0.03 < zeros < 0.07 and live.min() >= 400 and live.max() <= 440
    states, trace = TC.restate_a(case)
    assert trace.shape == (257, 64)
    TC.check_a(case, states, trace)
    per_frame = (trace > 0).sum(1)
    print(f"offset {offset}: units updated per frame min {per_frame.min()} median {int(np.median(per_frame))} max "
          f"{per_frame.max()}; largest weight {states[257][1].max():.0f}")
    fused, _ = TC.restate_a(case, fused=True)
    for F in TC.A_FRAMES:
        fused_against_plain(f"A offset {offset} F={F}", states[F], fused[F])


def test_case_b_cuts_every_cull_condition_through_updated_units():
    case = TC.case_b()
    assert len(case["units"]) == 216 and case["units"].min() == -3 and case["units"].max() == 2
    assert 4 <= len(case["Ks"]) <= 6
    assert any(K[0, 2] < 0 for K in case["Ks"]) and any(abs(K[0, 0] / K[1, 1] - 2.0) < 0.1 for K in case["Ks"])
    half = 3 * R.RES * case["p"]["voxel_length"]
    assert (np.abs(case["poses"][:, :3, 3]) < half).all()                         # every eye inside the block
    assert TC.B_RAW / 1000.0 < case["p"]["depth_trunc"] < 2 * half
    for T in case["poses"]:                                                       # rolled and tilted: no axis stays put
        assert np.abs(T[:3, :3]).max() < 0.97
    trace = []
    plain = TC.restate_b(case, trace=trace)
    count = TC.mixed_pairs(case, np.stack(trace))
    print("mixed (unit, frame) pairs with at least 64 updated voxels:", count)
    assert set(count) == set(R.CULL_CONDITIONS) and len(count) == 6
    assert min(count.values()) >= 8, count
    fused_against_plain("B", plain, TC.restate_b(case, fused=True))


def test_case_b_float32_poses_are_inside_the_rigid_bound():
    case = TC.case_b_float32()
    err = TC.rigid_error(TC.world2cam(case["poses"]))
    print(f"float32 relative poses: worst |singular value - 1| of world2cam {err:.3e}")
    assert 0.0 < err < TC.RIGID_TOL
    assert err < 5e-7                                                             # the figure, whatever the constant says
    assert TC.rigid_error(TC.world2cam(TC.case_b()["poses"])) < 1e-12
    trace = []
    plain = TC.restate_b(case, trace=trace)
    count = TC.mixed_pairs(case, np.stack(trace))
    print("mixed pairs under the float32 poses:", count)
    assert sum(count.values()) >= 48
    fused_against_plain("B float32", plain, TC.restate_b(case, fused=True))


@pytest.mark.parametrize("name", R.CULL_CONDITIONS)
def test_case_b_corner_sees_one_voxel_by_a_clear_margin(name):
    case = TC.case_b_corner(name)
    p, vl = case["p"], case["p"]["voxel_length"]
    assert TC.rigid_error(TC.world2cam(case["poses"])) < 1e-12
    ref = CR.integrate_rgb(case["units"], case["depth"], case["color"], TC.world2cam(case["poses"]), case["K"], p)
    assert (ref[1] != 0).sum() == 1 and ref[1][(0,) + case["corner"]] == 1.0
    c = R.cull_conditions(case["units"], TC.world2cam(case["poses"])[0], case["K"], p, case["height"], case["width"])
    alone = c[name] & c["front"]                                                  # the image sides mean something in front
    assert alone.sum() == 1 and alone[(0,) + case["corner"]]                      # the condition alone singles it out
    # the eye moved by 0.05 voxels along the plane's normal either way: the same single voxel, so nothing is near rounding
    for shift in (-0.05, 0.05):
        moved = case["poses"].copy()
        moved[0, :3, 3] += shift * vl * case["normal"]
        again = R.integrate(case["units"], case["depth"], TC.world2cam(moved), case["K"], p)
        assert ((again[1] != 0) == (ref[1] != 0)).all()
    out = case["poses"].copy()                                                    # and by 0.07: the voxel is out
    out[0, :3, 3] += 0.07 * vl * case["normal"]
    assert (R.integrate(case["units"], case["depth"], TC.world2cam(out), case["K"], p)[1] == 0).all()
    assert TC.B_CORNER_SLACK < 0.5 * 0.01 * 7.5 * 3 ** 0.5 < 0.58 - TC.B_CORNER_SLACK
    f = CR.integrate_rgb(case["units"], case["depth"], case["color"], TC.world2cam(case["poses"]), case["K"], p, fused=True)
    assert TC.state_differences(f, ref)["differ"] == 0


@pytest.mark.parametrize("make", [TC.case_c1, TC.case_c2, lambda: TC.case_c_trunc(500), lambda: TC.case_c_trunc(501),
                                  lambda: TC.case_c_trunc(0)], ids=["c1", "c2", "raw500", "raw501", "raw0"])
def test_case_c_literals_hold_in_the_restatement(make):
    """The catalogue's constructors assert the exact equalities in fp64; here the literals against the restatement, and a
    fused projection changes nothing at all (the arithmetic is exact)."""
    case = make()
    w2c = TC.world2cam(case["poses"])
    tsdf, w, col = CR.integrate_rgb(case["units"], case["depth"], case["color"], w2c, case["K"], case["p"])
    for g, (want_t, want_w) in case["expect"].items():
        got = float(TC.c_voxel(tsdf, case["units"], g)), float(TC.c_voxel(w, case["units"], g))
        assert got == (want_t, want_w), (g, got)
    assert (w != 0).any() == case.get("updates", True)
    assert (col[w != 0] == np.array(TC.C_COLOUR, np.float32)).all() and (col[w == 0] == 0).all()
    f = CR.integrate_rgb(case["units"], case["depth"], case["color"], w2c, case["K"], case["p"], fused=True)
    assert TC.state_differences(f, (tsdf, w, col))["differ"] == 0


def test_case_d_catalogue():
    for case in TC.cases_d_cameras():
        units = R.allocate(case["depth"], case["poses"], case["K"], case["p"])
        assert len(units) > 50 and units.min() < -1, case["name"]
    for case in TC.cases_d_sampling():
        units = R.allocate(case["depth"], case["poses"], case["K"], case["p"])
        assert (case["depth"] != 0).any() and (len(units) == 0) == case["empty"], case["name"]
    b = TC.case_d_boundaries()
    assert (R.allocate(b["depth"], b["poses"], b["K"], b["p"]) == b["expect"]).all()
    assert b["expect"][:, 0].min() == -3 and b["expect"][:, 2].min() == -2
    for case in TC.cases_d_reach():
        assert len(R.allocate(case["depth"], case["poses"], case["K"], case["p"])) == case["n_units"]
    cases = TC.cases_d_range()
    assert len(cases) == 12
    for case in cases:
        e = case["expect"]
        if case["in_range"]:                                                      # the units reach the extreme coordinate
            assert (e[:, case["axis"]] == case["extreme"]).any() and len(e) == 180, case["name"]
        else:                                                                     # the pushed frame loses samples
            assert 90 <= len(e) < 180, case["name"]
        assert np.abs(e).max() < TC.COORD_LIM                                     # the frame at the origin: 6 x 5 x 3 units


def test_cull_conditions_agree_with_integrate():
    """A voxel is updated only where all six conditions hold (the helper restates them one by one)."""
    case = TC.case_b()
    w2c = TC.world2cam(case["poses"])
    for f in (0, 1):
        c = R.cull_conditions(case["units"], w2c[f], case["Ks"][f], case["p"], case["height"], case["width"])
        _, w = R.integrate(case["units"], case["depth"][f:f + 1], w2c[f:f + 1], case["Ks"][f], case["p"])
        every = np.logical_and.reduce([c[n] for n in R.CULL_CONDITIONS])
        assert (w != 0).sum() > 1000 and every[w != 0].all()
        assert (every & (w == 0)).sum() < (w != 0).sum()       # the rest is sdf <= -sdf_trunc short of the far plane


def test_rigid_pose_check():
    """TSDFVolume refuses a finite pose with scale, names the frame, and keeps NaN poses as frames to skip."""
    from imfnet_amd import fuse
    assert fuse.RIGID_TOL == TC.RIGID_TOL == 5e-7
    good = TC.case_b()["poses"]
    fuse.check_rigid(good, "integrate")
    fuse.check_rigid(TC.case_b_float32()["poses"], "integrate")
    with_nan = good.copy()
    with_nan[2] = np.nan
    fuse.check_rigid(with_nan, "integrate")
    fuse.check_rigid(np.zeros((0, 4, 4)), "integrate")
    scaled = good.copy()
    scaled[4, :3, :3] *= 1.001
    with pytest.raises(ValueError, match=r"integrate: pose 4 is not rigid"):
        fuse.check_rigid(scaled, "integrate")
    sheared = good.copy()
    sheared[1, 0, 1] += 2e-6
    with pytest.raises(ValueError, match=r"allocate: pose 1 is not rigid"):
        fuse.check_rigid(sheared, "allocate")
    singular = good.copy()
    singular[0, :3, :3] = 0.0
    with pytest.raises(ValueError, match=r"pose 0 is not rigid"):
        fuse.check_rigid(singular, "allocate")
