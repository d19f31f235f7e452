"""The synthetic KITTI odometry tree of the training tests and of tools/train_kitti_time.py (plain helper module): two
drives of street-sized views of the fixture clouds, one frame moved 150 m off, and a lattice drive for validation."""
import os

import numpy as np

from kitti_restate import rigid, write_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS = 30000
FAR_FRAME = (1, 5)                     # drive 1, frame 5: its scan sits 150 m off its pose


def _poses(n):
    P = np.tile(np.eye(4), (n, 1, 1))
    for t in range(n):
        P[t, :3, :3] = rigid(0.4 * t, [0, 1, 0], [0, 0, 0])[:3, :3]
        P[t, 0, 3] = 5.0 * t
    return P


def _views(world, P, rng, crop, n_points):
    from imfnet_amd.kitti import VELO2CAM
    Vc = VELO2CAM.T
    scans = {}
    for t in range(len(P)):
        A = np.linalg.inv(P[t] @ Vc)                                  # world (camera 0 frame) -> velodyne t
        local = world @ A[:3, :3].T + A[:3, 3]
        if crop:
            sel = rng.permutation(np.flatnonzero(np.linalg.norm(local[:, :2], axis=1) < 30.0))[:n_points]
            local = local[sel]
        scans[t] = local.astype(np.float32)
    return scans


def build_tree(root, clouds):
    """Drives 0 and 1: the two fixture clouds scaled by 12 to street extent (about 40 m), seven frames 5 m apart on a
    straight track, every scan a 30 000-point view of the scene from its frame; pairs (0, 2) and (3, 5) each.  Frame 5
    of drive 1 is moved 150 m off.  Drive 2 (validation): a jittered 1.2 m lattice seen whole from every frame, so
    that a voxel holds one point in either scan and every point has its exact partner."""
    rng = np.random.default_rng(33)
    P = _poses(7)
    positions, scans = {}, {}
    for drive in (0, 1):
        c = clouds[drive].astype(np.float64)
        world = (c - c.mean(0)) * 12.0
        world = world[:, [0, 2, 1]] * [1.0, -1.0, 1.0]                  # the room's floor under the camera's x-z plane
        positions[drive], scans[drive] = P, _views(world, P, rng, True, N_POINTS)
    scans[FAR_FRAME[0]][FAR_FRAME[1]] = scans[FAR_FRAME[0]][FAR_FRAME[1]] + np.float32([150.0, 0.0, 0.0])
    g = np.stack(np.meshgrid(np.arange(-20, 20, 1.2), np.arange(-2, 2, 1.2), np.arange(-20, 22, 1.2),
                             indexing="ij"), -1).reshape(-1, 3)
    lattice = g + rng.uniform(-0.2, 0.2, g.shape)
    positions[2], scans[2] = P, _views(lattice, P, rng, False, 0)
    write_tree(str(root), positions, scans, image=os.path.join(ROOT, "tests", "golden", "cloud_bin_0_0.png"))
    (root / "train.txt").write_text("0 1\n")
    (root / "val.txt").write_text("2\n")
    return positions, scans
