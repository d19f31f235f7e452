"""`python -m imfnet_amd.register --descriptor fpfh` and `python -m imfnet_amd.fpfh_desc` on the fixture fragment: the
global stage (keypoints, nearest FPFH descriptor, RANSAC) must bring a rigid copy of the fragment close enough for the
refinement to return the known motion, with no checkpoint, no image, no start and the default seed."""
import json
import os
import shutil

import numpy as np
import pytest

from kitti_restate import rigid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE = os.path.join(ROOT, "tests", "golden", "cloud_bin_0_0.png")
KEYS = {"fitness", "rmse", "iterations", "n_corr", "times", "T"}


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """The fixture fragment (every 4th point) and a rigid copy of it at 11 degrees and about 0.4 m, as PLY files."""
    from imfnet_amd.dataio import read_ply_points
    from imfnet_amd.fuse_fragments import write_ply
    d = tmp_path_factory.mktemp("register_fpfh")
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))
    write_ply(str(d / "a.ply"), z["cloud_bin_0"][::4].astype(np.float64))
    a = read_ply_points(str(d / "a.ply"))
    truth = rigid(11.0, [0.2, 1.0, -0.3], np.array([0.31, -0.12, 0.22]))
    write_ply(str(d / "b.ply"), a @ truth[:3, :3].T + truth[:3, 3])
    return d, truth


def _run(capsys, argv):
    from imfnet_amd.register import main
    capsys.readouterr()
    assert main(argv) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _off(T, truth):
    return float(np.linalg.norm(T[:3, :3] - truth[:3, :3])), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


def test_fpfh_registration_returns_the_known_motion(pair, capsys):
    """The bound is the one tests/test_gpu_register.py takes for this pair and this refinement from a known start: 1e-3 in
    rotation (Frobenius) and 2 mm in translation.  It holds exactly when RANSAC (50 000 hypotheses, seed 0) lands inside the
    1.5-voxel basin of the point-to-plane ICP.  The unrefined pose and the inlier ratio of the nearest-descriptor matches
    under the true motion are printed."""
    from imfnet_amd.dataio import read_ply_points
    from imfnet_amd.extract import voxel_representatives
    from imfnet_amd.matching import feature_match, select_keypoints
    from imfnet_amd.register import fpfh_descriptors
    d, truth = pair
    base = ["--descriptor", "fpfh", "--source", str(d / "a.ply"), "--target", str(d / "b.ply")]
    raw = _run(capsys, base + ["--refine", "none", "--out", str(d / "T_none.txt")])
    res = _run(capsys, base + ["--refine", "plane", "--out", str(d / "T_plane.txt")])
    T0, T = np.loadtxt(str(d / "T_none.txt")), np.loadtxt(str(d / "T_plane.txt"))

    # the matches register_pair makes, judged by the true motion
    rng = np.random.RandomState(0)
    kp, desc = [], []
    for name in ("a.ply", "b.ply"):
        pts = read_ply_points(str(d / name))
        xyz = voxel_representatives(pts, 0.025)
        keys = select_keypoints(pts[rng.choice(len(pts), min(5000, len(pts)), replace=False)], xyz, 0.025)
        kp.append(xyz[keys])
        desc.append(fpfh_descriptors(xyz, 0.025)[keys])
    n_inl, ratio, match2, _ = feature_match(kp[1], desc[1], kp[0], desc[0], truth, inlier_thresh=0.1)

    (rot0, tr0), (rot, tr) = _off(T0, truth), _off(T, truth)
    with capsys.disabled():
        print(f"\nregister --descriptor fpfh: keypoints {len(kp[0])} / {len(kp[1])}, mutual matches {len(match2)}, inlier "
              f"ratio under the true motion {ratio:.4f} ({n_inl} within 0.1 m)\n  before refinement: rotation off "
              f"{rot0:.3e}, translation off {tr0:.3e} m, fitness {raw['fitness']:.4f}\n  after --refine plane "
              f"({res['iterations']} iterations): rotation off {rot:.3e}, translation off {tr:.3e} m, fitness "
              f"{res['fitness']:.4f}, rmse {res['rmse']:.3e}, times {res['times']}")
    assert set(res) == KEYS and np.array_equal(np.array(res["T"]), T)
    assert {"features", "global", "normals", "refine"} <= set(res["times"])
    assert rot <= 1e-3 and tr <= 2e-3


def test_fpfh_desc_writes_the_descriptor_tree(pair, tmp_path, capsys):
    from imfnet_amd.dataio import read_ply_points
    from imfnet_amd.fpfh_desc import main
    d, _ = pair
    seq = tmp_path / "src" / "scene-x" / "seq-01"
    os.makedirs(seq)
    for k, name in enumerate(("a.ply", "b.ply")):
        shutil.copy(d / name, seq / f"cloud_bin_{k}.ply")
    assert main(["--source", str(tmp_path / "src"), "--target", str(tmp_path / "desc")]) == 0
    assert "2 fragments" in capsys.readouterr().out
    for k, name in enumerate(("a.ply", "b.ply")):
        z = np.load(tmp_path / "desc" / "scene-x" / "seq-01" / f"cloud_bin_{k}.npz")
        assert set(z.files) == {"points", "xyz", "feature"}
        pts, xyz, feat = z["points"], z["xyz"], z["feature"]
        assert np.array_equal(pts, read_ply_points(str(d / name)))
        assert xyz.ndim == 2 and xyz.shape[1] == 3 and 1000 < len(xyz) < len(pts)
        assert feat.shape == (len(xyz), 64) and feat.dtype == np.float32
        assert not feat[:, 33:].any() and np.isfinite(feat).all() and (feat >= 0).all()
        sums = feat[:, :33].astype(np.float64).reshape(-1, 3, 11).sum(2)
        assert (np.abs(sums - 200.0) < 1e-3).mean() > 0.99          # three groups of 200 wherever a point has neighbours
        voxels = np.floor(xyz / 0.025).astype(np.int64)
        assert len(np.unique(voxels, axis=0)) == len(xyz)           # one representative per voxel, each a point of the file
        assert len(np.unique(np.floor(pts / 0.025).astype(np.int64), axis=0)) == len(xyz)
    # the representatives are the ones the network path returns for this voxel size
    import torch
    from imfnet_amd.extract import extract_features
    from imfnet_amd.register import load_image, load_network
    model, cfg = load_network(None, torch.device("cuda"))
    with torch.no_grad():
        want, _ = extract_features(model, read_ply_points(str(d / "b.ply")), voxel_size=0.025, device=torch.device("cuda"),
                                   skip_check=True, image=load_image(IMAGE, cfg))
    assert np.array_equal(np.asarray(want, np.float64), xyz)
