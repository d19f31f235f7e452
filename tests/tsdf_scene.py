"""A seeded synthetic RGB-D sequence for the fragment fusion tests: the inside of a box room with a sphere in it and one
corner cut off by a slanted plane, seen from a handful of camera poses on a short arc.  Depth is computed analytically
along the ray through every pixel centre and stored as uint16 millimetres; a seeded share of the pixels is zeroed (no
measurement).  `write_tree` lays the sequence out as the 3DMatch raw download does."""
import os

import numpy as np

ROOM_MIN = np.array([-1.37, -1.13, -1.29])
ROOM_MAX = np.array([1.41, 1.09, 1.33])
SPHERE_C = np.array([0.23, -0.31, 0.71])
SPHERE_R = 0.36
PLANE_N = np.array([0.48, 0.28, 0.83]) / np.linalg.norm([0.48, 0.28, 0.83])    # free space: n . p < PLANE_D
PLANE_D = 0.93


def intrinsic(width, height):
    """The 3DMatch sensors' 585-pixel focal length at 640 x 480, scaled to the image."""
    s = width / 640.0
    return np.array([[585.0 * s, 0.0, 320.0 * s - 0.5 * (1 - s)], [0.0, 585.0 * s, 240.0 * s - 0.5 * (1 - s)],
                     [0.0, 0.0, 1.0]])


def camera_poses(n_frames, seed=0, arc=0.5):
    """cam2world [n, 4, 4]: cameras on an arc of `arc` radians around the room's middle, looking at the sphere's side."""
    rng = np.random.default_rng(seed)
    target = np.array([0.1, -0.1, 1.0])
    out = []
    for i in range(n_frames):
        a = -0.5 * arc + arc * (i / max(1, n_frames - 1)) + 0.01 * rng.standard_normal()
        eye = np.array([0.75 * np.sin(a), 0.05 * np.cos(3 * a), -0.55 - 0.2 * np.cos(a)]) + 0.01 * rng.standard_normal(3)
        z = target - eye
        z /= np.linalg.norm(z)
        x = np.cross(np.array([0.0, -1.0, 0.0]), z)          # image y points down
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        T = np.eye(4)
        T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
        out.append(T)
    return np.stack(out)


def render_depth(T, K, width, height):
    """Depth (the camera-frame z of the first surface along each pixel centre's ray) in metres, float64 [H, W]."""
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    d_cam = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)    # z = 1: t is the depth
    d = d_cam @ T[:3, :3].T
    o = T[:3, 3]
    t = np.full(u.shape, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):                                   # walls, from inside
            for bound in (ROOM_MIN[a], ROOM_MAX[a]):
                ta = (bound - o[a]) / d[..., a]
                t = np.where((ta > 0) & (ta < t), ta, t)
        tp = (PLANE_D - PLANE_N @ o) / (d @ PLANE_N)         # the slanted plane
        t = np.where((tp > 0) & (tp < t), tp, t)
        oc = o - SPHERE_C                                    # the sphere, from outside
        A, B, C = (d * d).sum(-1), 2.0 * (d @ oc), oc @ oc - SPHERE_R ** 2
        disc = B * B - 4 * A * C
        ts = (-B - np.sqrt(np.where(disc > 0, disc, np.nan))) / (2 * A)
        t = np.where((ts > 0) & (ts < t), ts, t)
    return t


def surface_distance(points):
    """Distance of world points to the nearest analytic surface (walls, plane, sphere; the primitives unclipped)."""
    p = np.asarray(points, np.float64)
    d = [np.abs(p - ROOM_MIN).min(1), np.abs(p - ROOM_MAX).min(1), np.abs(p @ PLANE_N - PLANE_D),
         np.abs(np.linalg.norm(p - SPHERE_C, axis=1) - SPHERE_R)]
    return np.min(d, 0)


def make_sequence(width=160, height=120, n_frames=5, seed=0, holes=0.02, arc=0.5):
    """dict(depth uint16 [F, H, W] in millimetres, poses cam2world [F, 4, 4], K [3, 3])."""
    rng = np.random.default_rng(seed + 1)
    K = intrinsic(width, height)
    poses = camera_poses(n_frames, seed, arc)
    depth = np.zeros((n_frames, height, width), np.uint16)
    for f in range(n_frames):
        mm = np.rint(render_depth(poses[f], K, width, height) * 1000.0)
        mm[~np.isfinite(mm) | (mm > 65535)] = 0
        mm[rng.random(mm.shape) < holes] = 0
        depth[f] = mm.astype(np.uint16)
    return dict(depth=depth, poses=poses, K=K)


def write_tree(root, seq, scene="scene-a", seq_name="seq-01", nan_pose=(), world=None):
    """<root>/<scene>/camera-intrinsics.txt and <scene>/<seq>/frame-XXXXXX.{color.jpg, depth.png, pose.txt}.  `world`: a
    4x4 applied to every pose (the raw data's poses are not relative to a fragment); `nan_pose`: frames whose pose file
    holds NaN, as the raw data marks a lost track."""
    from PIL import Image
    sdir = os.path.join(root, scene, seq_name)
    os.makedirs(sdir, exist_ok=True)
    np.savetxt(os.path.join(root, scene, "camera-intrinsics.txt"), seq["K"])
    world = np.eye(4) if world is None else world
    F, H, W = seq["depth"].shape
    rng = np.random.default_rng(5)
    for f in range(F):
        stem = os.path.join(sdir, "frame-%06d" % f)
        Image.fromarray(seq["depth"][f]).save(stem + ".depth.png")
        rgb = (rng.random((H, W, 3)) * 40 + (seq["depth"][f][..., None] // 16 % 200)).astype(np.uint8)
        Image.fromarray(rgb).save(stem + ".color.jpg", quality=90)
        T = world @ seq["poses"][f]
        np.savetxt(stem + ".pose.txt", np.full((4, 4), np.nan) if f in nan_pose else T)
    return sdir
