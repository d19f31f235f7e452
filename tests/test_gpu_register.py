"""`python -m imfnet_amd.register` on the fixture fragments: the refinement path from a known start (both refinements
return a known rigid motion) and the whole flow on the seeded weights.  The command's `main` runs in this process; its
`--help` as a child process is in tests/test_normals_host.py."""
import json
import os

import numpy as np
import pytest

from kitti_restate import rigid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE = os.path.join(ROOT, "tests", "golden", "cloud_bin_0_0.png")
KEYS = {"fitness", "rmse", "iterations", "n_corr", "times", "T"}


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """The fixture fragment (every 4th point) and a rigidly moved copy of it, as PLY files, with the motion and a start
    that is off by 2 degrees about the fragment's middle and 3 cm."""
    from imfnet_amd.dataio import read_ply_points
    from imfnet_amd.fuse_fragments import write_ply
    d = tmp_path_factory.mktemp("register")
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))
    write_ply(str(d / "a.ply"), z["cloud_bin_0"][::4].astype(np.float64))
    write_ply(str(d / "c.ply"), z["cloud_bin_1"][::4].astype(np.float64))
    a = read_ply_points(str(d / "a.ply"))
    truth = rigid(11.0, [0.2, 1.0, -0.3], np.array([0.31, -0.12, 0.22]))
    write_ply(str(d / "b.ply"), a @ truth[:3, :3].T + truth[:3, 3])
    mid = a.mean(0)
    off = rigid(2.0, [1.0, -0.4, 0.5], np.zeros(3))
    off[:3, 3] = mid - off[:3, :3] @ mid + np.array([0.02, -0.02, 0.01])          # |t| = 3 cm
    np.savetxt(str(d / "init.txt"), truth @ off, fmt="%.17g")
    return d, truth


def _run(capsys, argv):
    from imfnet_amd.register import main
    capsys.readouterr()
    assert main(argv) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.parametrize("refine", ["plane", "point"])
def test_refinement_returns_a_known_motion(pair, capsys, refine):
    """A functional bound, not a precision claim: 1e-3 in rotation (Frobenius) and 2 mm in translation.  The target is a
    rigid copy, but it is voxelised on its own, so the two sets of representatives sample the surface differently and the
    refinements end at the millimetre (measured on an MI355X: plane 5 iterations, 5.9e-4 / 1.3 mm; point 17 iterations,
    7.3e-4 / 1.6 mm).  The iteration counts are printed, not gated."""
    d, truth = pair
    out = str(d / f"T_{refine}.txt")
    res = _run(capsys, ["--source", str(d / "a.ply"), "--source_image", IMAGE, "--target", str(d / "b.ply"),
                        "--target_image", IMAGE, "--skip_global", "--init", str(d / "init.txt"), "--refine", refine,
                        "--out", out])
    T = np.loadtxt(out)
    rot, tr = float(np.linalg.norm(T[:3, :3] - truth[:3, :3])), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))
    with capsys.disabled():
        print(f"\nregister --refine {refine}: {res['iterations']} iterations, rotation off {rot:.3e}, translation off "
              f"{tr:.3e} m, fitness {res['fitness']:.4f}, rmse {res['rmse']:.3e}, times {res['times']}")
    assert set(res) == KEYS and np.array_equal(np.array(res["T"]), T)
    assert rot <= 1e-3 and tr <= 2e-3
    assert "global" not in res["times"] and "features" in res["times"] and ("normals" in res["times"]) == (refine == "plane")


def test_full_flow_on_the_seeded_weights(pair, capsys):
    d, _ = pair
    out = str(d / "T_full.txt")
    res = _run(capsys, ["--source", str(d / "a.ply"), "--source_image", IMAGE, "--target", str(d / "c.ply"),
                        "--target_image", IMAGE, "--ransac_iter", "4096", "--num_keypoints", "1000", "--out", out])
    T = np.loadtxt(out)
    R = T[:3, :3]
    assert set(res) == KEYS and {"features", "global", "normals", "refine"} <= set(res["times"])
    assert np.isfinite(T).all() and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0
    assert 0.0 <= res["fitness"] <= 1.0 and res["rmse"] >= 0.0 and res["iterations"] >= 0 and res["n_corr"] >= 0
