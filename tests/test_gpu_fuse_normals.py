"""`fuse_fragments --normals` on the synthetic sequence of tests/tsdf_scene.py: the PLY gains nx, ny, nz, keeps the x, y, z
bytes of the run without the flag, and on the room's far wall the normals are the wall's, facing the camera."""
import os

import numpy as np
import pytest

import tsdf_scene as S

pytestmark = pytest.mark.gpu


def _read_rows(path):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    width = head.count(b"property float")
    return head, np.frombuffer(body, "<f4").reshape(-1, width)


def test_normals_flag_adds_normals_and_keeps_the_points(tmp_path):
    from imfnet_amd import fuse_fragments as FF
    from imfnet_amd.dataio import read_ply_points
    seq = S.make_sequence(160, 120, n_frames=4)
    raw = str(tmp_path / "raw")
    S.write_tree(raw, seq)
    common = ["--dataset_root", raw, "--height", "120", "--width", "160", "--frames_per_frag", "4", "--voxel_length", "0.006",
              "--lattice_offset", "0"]
    assert FF.main(common + ["--out_root", str(tmp_path / "plain")]) == 0
    assert FF.main(common + ["--out_root", str(tmp_path / "normals"), "--normals"]) == 0
    name = os.path.join("scene-a", "seq-01", "cloud_bin_0.ply")
    plain, with_n = str(tmp_path / "plain" / name), str(tmp_path / "normals" / name)
    a, b = read_ply_points(plain), read_ply_points(with_n)
    assert len(a) > 10000 and a.tobytes() == b.tobytes()                  # through imf_ply_read_points: extra properties skipped
    head, rows = _read_rows(with_n)
    assert b"property float nx\nproperty float ny\nproperty float nz\n" in head and rows.shape == (len(a), 6)
    assert rows[:, :3].tobytes() == _read_rows(plain)[1].tobytes()
    nrm = rows[:, 3:].astype(np.float64)
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-6         # float32 in the file
    lone = (nrm == np.array([0.0, 0.0, 1.0])).all(1)                      # fewer than 3 points within 5 voxels: the fallback
    facing = (nrm * -a).sum(1) >= -1e-6 * np.linalg.norm(a, axis=1)       # towards the first camera, the origin
    assert lone.mean() < 0.01 and facing[~lone].all()
    # the far wall z = ROOM_MAX[2], away from the other surfaces by more than the search radius
    T0 = seq["poses"][0].astype(np.float32).astype(np.float64)
    world = a @ T0[:3, :3].T + T0[:3, 3]
    others = [np.abs(world[:, :2] - S.ROOM_MIN[:2]).min(1), np.abs(world[:, :2] - S.ROOM_MAX[:2]).min(1),
              np.abs(world @ S.PLANE_N - S.PLANE_D), np.abs(np.linalg.norm(world - S.SPHERE_C, axis=1) - S.SPHERE_R)]
    wall = (np.abs(world[:, 2] - S.ROOM_MAX[2]) < 0.012) & (np.min(others, 0) > 0.08)
    assert wall.sum() > 500
    wall_n = T0[:3, :3].T @ np.array([0.0, 0.0, -1.0])                    # into the room, in the first camera's frame
    cosang = np.clip(nrm[wall] @ wall_n, -1.0, 1.0)
    worst = float(np.degrees(np.arccos(cosang)).max())
    print(f"far wall: {int(wall.sum())} points, largest angle to the wall's normal {worst:.3f} degrees")
    assert worst <= 5.0
