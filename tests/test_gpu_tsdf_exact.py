"""imf_tsdf_allocate and imf_tsdf_integrate(_rgb) (csrc/tsdf.hip) on the adversarial frames and cameras of
tests/tsdf_cases.py, against the un-culled NumPy restatement and literal values.  The integrate calls are driven raw, on
hand-made unit lists; tests/test_tsdf_cases_host.py shows without a GPU that every case reaches what it is meant to reach
and that the restatement alone stays inside the caps of the comparison rule (tsdf_cases.assert_state_rule).

Measured on the MI355X (every test prints its counts): 0 voxels differ from the restatement in every case -- A at 32, 33,
65 and 257 frames with 206 144 to 259 086 observed voxels, both lattice offsets; B with 348 306 (fp64 poses) and 260 020
(float32 relative poses); the six corner units; C; the volume fed float32 poses (369 860) -- and every unit list of D
equals the restatement's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsdf_cases as TC           # noqa: E402
import tsdf_restate as R          # noqa: E402
from test_tsdf_color_host import STATE_CAP   # noqa: E402

pytestmark = pytest.mark.gpu


class RawVolume:
    """A hand-made unit list with zeroed state on the device, and the raw integrate calls on it."""

    def __init__(self, units, rgb):
        import torch
        from imfnet_amd import _lib
        self.L, self.rgb, self.n = _lib.lib(), rgb, len(units)
        dev = torch.device("cuda:0")
        self.units = torch.from_numpy(np.ascontiguousarray(units, np.int32)).to(dev)
        self.meta = torch.tensor([self.n, 0], dtype=torch.int32, device=dev)
        self.vox = torch.zeros((self.n, 4096, 2), dtype=torch.float32, device=dev)
        self.col = torch.zeros((self.n, 3, 4096), dtype=torch.float32, device=dev) if rgb else None

    def integrate(self, case, K, frames):
        import torch
        from imfnet_amd import _lib
        dev, p = self.units.device, case["p"]
        params = _lib.TsdfParams(K[0, 0], K[1, 1], K[0, 2], K[1, 2], p["voxel_length"], p["sdf_trunc"], p["depth_scale"],
                                 p["depth_trunc"], p["lattice_offset"], case["height"], case["width"])
        ptr = lambda t: C.c_void_p(t.data_ptr())
        d = torch.from_numpy(np.ascontiguousarray(case["depth"][frames]).view(np.int16)).to(dev)
        w2c = TC.world2cam(case["poses"][frames])
        w2c = torch.from_numpy(np.ascontiguousarray(w2c[:, :3, :].reshape(-1, 12))).to(dev)
        if self.rgb:
            c = torch.from_numpy(np.ascontiguousarray(case["color"][frames])).to(dev)
            rc = self.L.imf_tsdf_integrate_rgb(ptr(d), ptr(c), len(d), ptr(w2c), C.byref(params), ptr(self.units),
                                               ptr(self.meta), self.n, ptr(self.vox), ptr(self.col), None)
        else:
            rc = self.L.imf_tsdf_integrate(ptr(d), len(d), ptr(w2c), C.byref(params), ptr(self.units), ptr(self.meta),
                                           self.n, ptr(self.vox), None)
        _lib.check(rc, "imf_tsdf_integrate_rgb" if self.rgb else "imf_tsdf_integrate")
        torch.cuda.synchronize()

    def state(self):
        v = self.vox.cpu().numpy().reshape(self.n, 16, 16, 16, 2)
        out = (np.ascontiguousarray(v[..., 0]), np.ascontiguousarray(v[..., 1]))
        if self.rgb:
            out += (np.ascontiguousarray(self.col.permute(0, 2, 1).cpu().numpy()).reshape(self.n, 16, 16, 16, 3),)
        return out


def both(case, calls):
    """The calls (K, frames) on a fresh plain and a fresh coloured volume: the coloured state, after the check that the two
    instantiations leave the same (tsdf, w) bits."""
    states = []
    for rgb in (False, True):
        vol = RawVolume(case["units"], rgb)
        for K, frames in calls:
            vol.integrate(case, K, frames)
        states.append(vol.state())
    plain, coloured = states
    assert plain[0].tobytes() == coloured[0].tobytes() and plain[1].tobytes() == coloured[1].tobytes()
    return coloured


def against_restatement(name, got, ref):
    d = TC.state_differences(got, ref)
    print(f"{name}: (tsdf, w) differ in {d['differ']} of {d['seen']} voxels with w != 0, at most {d['worst_unit']} in one "
          f"unit; colour differs alone in {d['colour']}")
    TC.assert_state_rule(d, STATE_CAP)
    return d


@pytest.fixture(scope="module", params=TC.A_OFFSETS)
def case_a(request):
    case = TC.case_a(request.param)
    states, _ = TC.restate_a(case)
    return case, states


@pytest.mark.parametrize("F", TC.A_FRAMES)
def test_frame_counts_in_one_call(case_a, F):
    """32, 33, 65 and 257 frames in one call: every word of the frame mask, the second trip of its fill loop (F = 257), NaN
    poses among them.  Measured: 0 differing voxels at every F and both lattice offsets."""
    case, states = case_a
    got = both(case, [(case["K"], slice(0, F))])
    against_restatement(f"A offset {case['p']['lattice_offset']} F={F}", got, states[F])


def test_frames_in_two_calls_give_the_bits_of_one(case_a):
    """65 frames as 40 + 25: the bits of the single call, the colour too."""
    case, _ = case_a
    one = both(case, [(case["K"], slice(0, 65))])
    two = both(case, [(case["K"], slice(0, 40)), (case["K"], slice(40, 65))])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, two))
    assert (one[1] != 0).sum() > 100000


@pytest.mark.parametrize("make", [TC.case_b, TC.case_b_float32], ids=["fp64 poses", "float32 relative poses"])
def test_cull_changes_no_result(make):
    """Single-frame calls with the eye inside a dense block: each of the six cull conditions cuts through units the frame
    updates.  Measured: 0 differing voxels for both pose sets."""
    case = make()
    got = both(case, [(K, slice(f, f + 1)) for f, K in enumerate(case["Ks"])])
    against_restatement("B " + ("float32" if make is TC.case_b_float32 else "fp64"), got, TC.restate_b(case))


@pytest.mark.parametrize("name", R.CULL_CONDITIONS)
def test_unit_seen_by_one_corner_voxel(name):
    """The plane of one cull condition square to the unit's diagonal, 0.06 voxels inside the corner sample: the bounding
    sphere must not be smaller than the unit.  One voxel is updated and not one differs from the restatement."""
    import tsdf_color_restate as CR
    case = TC.case_b_corner(name)
    got = both(case, [(case["K"], slice(0, 1))])
    ref = CR.integrate_rgb(case["units"], case["depth"], case["color"], TC.world2cam(case["poses"]), case["K"], case["p"])
    d = TC.state_differences(got, ref)
    print(f"B corner {name}: {d}")
    assert d["seen"] == 1 and d["differ"] == 0 and d["colour"] == 0
    assert got[1][(0,) + case["corner"]] == 1.0 and (got[1] != 0).sum() == 1


@pytest.mark.parametrize("make", [TC.case_c1, TC.case_c2, lambda: TC.case_c_trunc(500), lambda: TC.case_c_trunc(501),
                                  lambda: TC.case_c_trunc(0)], ids=["c1", "c2", "raw500", "raw501", "raw0"])
def test_thresholds_at_equality(make):
    """uf == 0 in, uf == W out, z == 0 out, d == depth_trunc in, sdf == -sdf_trunc out, sdf >= sdf_trunc gives 1: the
    literals, and not one voxel differs from the restatement; a constant colour stays that colour."""
    import tsdf_color_restate as CR
    case = make()
    tsdf, w, col = both(case, [(case["K"], slice(0, 1))])
    for g, want in case["expect"].items():
        got = float(TC.c_voxel(tsdf, case["units"], g)), float(TC.c_voxel(w, case["units"], g))
        assert got == want, (g, got, want)
    ref = CR.integrate_rgb(case["units"], case["depth"], case["color"], TC.world2cam(case["poses"]), case["K"], case["p"])
    d = TC.state_differences((tsdf, w, col), ref)
    print(f"C raw {case['raw']}: {d}")
    assert d["differ"] == 0 and d["colour"] == 0 and (d["seen"] > 0) == case.get("updates", True)
    assert (col[w != 0] == np.array(TC.C_COLOUR, np.float32)).all() and (col[w == 0] == 0).all()


def allocated(case, unit_capacity=1 << 12):
    from imfnet_amd.fuse import TSDFVolume
    p = case["p"]
    vol = TSDFVolume(case["K"], case["height"], case["width"], p["voxel_length"], p["sdf_trunc"], p["depth_scale"],
                     p["depth_trunc"], p["lattice_offset"], unit_capacity=unit_capacity)
    vol.allocate(case["depth"], case["poses"])
    return vol


def test_allocate_on_odd_images_and_negative_coordinates():
    """Image sides that are no multiple of the stride, cameras that open negative unit coordinates; depth only where the
    sampling never looks; depth only in the last sampled column and row."""
    for case in TC.cases_d_cameras() + TC.cases_d_sampling():
        vol = allocated(case)
        want = R.allocate(case["depth"], case["poses"], case["K"], case["p"])
        units = vol.units
        print(f"{case['name']}: {len(units)} units")
        assert vol.flags == 0 and units.shape == want.shape and (units == want).all(), case["name"]
        assert (len(units) == 0) == case.get("empty", False)


def test_allocate_on_unit_boundaries_and_every_reach():
    from imfnet_amd import _lib
    case = TC.case_d_boundaries()
    vol = allocated(case)
    assert vol.flags == 0 and vol.units.shape == case["expect"].shape and (vol.units == case["expect"]).all()
    for case in TC.cases_d_reach():
        if case["reach"] > 4:
            with pytest.raises(_lib.ImfError, match="reaches 5 units"):
                allocated(case)
            continue
        vol = allocated(case)
        want = R.allocate(case["depth"], case["poses"], case["K"], case["p"])
        assert vol.flags == 0 and len(want) == case["n_units"]
        assert vol.units.shape == want.shape and (vol.units == want).all()


def test_allocate_at_the_coordinate_limit():
    """The last (first) permitted unit coordinate opens its units without a flag; one unit further raises the range flag,
    opens nothing for that sample and still opens every sample that is in range."""
    from imfnet_amd.fuse import FLAG_RANGE
    for case in TC.cases_d_range():
        vol = allocated(case)
        units = vol.units
        assert vol.flags == (0 if case["in_range"] else FLAG_RANGE), case["name"]
        assert units.shape == case["expect"].shape and (units == case["expect"]).all(), case["name"]


def test_volume_refuses_a_pose_with_scale_and_takes_float32_poses():
    from imfnet_amd.fuse import TSDFVolume
    case = TC.case_b_float32()
    p, K = case["p"], case["Ks"][0]
    vol = TSDFVolume(K, case["height"], case["width"], p["voxel_length"], p["sdf_trunc"], p["depth_scale"], p["depth_trunc"],
                     p["lattice_offset"], unit_capacity=1 << 12)
    scaled = case["poses"].copy()
    scaled[3, :3, :3] *= 1.001
    with pytest.raises(ValueError, match="allocate: pose 3 is not rigid"):
        vol.allocate(case["depth"], scaled)
    with_nan = case["poses"].copy()
    with_nan[1] = np.nan
    vol.allocate(case["depth"], with_nan)                    # float32-rounded poses pass; a NaN pose is a frame to skip
    assert vol.n_units > 0
    with pytest.raises(ValueError, match="integrate: pose 3 is not rigid"):
        vol.integrate(case["depth"], scaled)
    vol.integrate(case["depth"], with_nan)
    skipped = np.delete(np.arange(len(with_nan)), 1)
    want = R.integrate(vol.units, case["depth"][skipped], TC.world2cam(with_nan[skipped]), K, p)
    got = vol.voxels().reshape(-1, 16, 16, 16, 2)
    against_restatement("volume, float32 poses", (got[..., 0], got[..., 1]), want)
