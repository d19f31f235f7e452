"""Integrate a whole scene: every frame of every fragment goes into ONE TSDF volume with the fragment's optimised pose,
and the surface comes out as a triangle mesh -- the last step of Choi, Zhou, Koltun 2015, after fuse_fragments and
reconstruct.

    python -m imfnet_amd.integrate_scene --fragments DIR --raw_seq DIR --trajectory SCENE/trajectory.log --out SCENE
        [--voxel_length 0.005859375] [--sdf_trunc 0.04] [--depth_trunc 6.0] [--lattice_offset 0.5]
        [--height 480] [--width 640] [--depth_scale 1000] [--threads 0] [--device cuda] [--color]

--fragments holds what fuse_fragments wrote (cloud_bin_K.pose.npy, cloud_bin_K.frames.pkl), --raw_seq the sequence they
were fused from (<frame>.depth.png, <frame>.pose.txt; camera-intrinsics.txt in the scene directory above it, as
fuse_fragments finds it), --trajectory the `k k N` + X_k records of reconstruct (X_k: fragment k into the scene frame).
A fragment whose X_k is not finite (no kept pair reaches it) or that the trajectory does not list is skipped and reported.

Frame f of fragment K gets the scene pose X_K . inv(base_K) . pose_f: base_K from cloud_bin_K.pose.npy, pose_f read as
float32, the relative pose inv(base_K) . pose_f formed in float32 exactly as fuse_fragments.select_frames forms it, the
product with X_K in fp64.  A frames.pkl that holds "poses" (fuse_fragments --poses odometry) gives the relative poses
itself, in fp64, and no .pose.txt is read.  The frame files are found by the basenames recorded in cloud_bin_K.frames.pkl.  All fragments
are allocated first (the unit rows must be final before the first frame is integrated), then integrated fragment by
fragment in order, at most 4096 frames per call; the next fragment is decoded while the GPU works on the current one.
Writes SCENE/scene_mesh.ply (fuse_fragments.write_ply_mesh; TSDFVolume.extract_mesh) and prints one JSON
line: fragments used and skipped, frames, units, vertices, triangles, whether colour was integrated, stage times.
--color also decodes every frame's <frame>.color.jpg, integrates it with the depth and gives the mesh
uchar red, green, blue per vertex.  The frames stay resident on the device between the allocate phase and the integrate
phase: 2 height width bytes of depth per frame (614 400 at 640 x 480) and, under --color, 3 height width bytes of colour
beside them (921 600: 2.5 times the memory per frame, 1.5 GB per thousand frames instead of 0.6).
"""
import argparse
import concurrent.futures as cf
import json
import os
import pickle
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the native library is loaded: both must share one HIP runtime)

from .evaluate import read_log
from .files import ensure_dir
from .fuse_fragments import cpu_quota, read_color_jpg, read_depth_png, read_extrinsic, write_ply_mesh

MAX_FRAMES_PER_CALL = 4096


def scene_poses(fragments, raw_seq, k, X):
    """[(frame stem in raw_seq, cam2scene fp64 [4,4])] of fragment k; a frame whose pose file holds a NaN is left out."""
    base = np.load(os.path.join(fragments, f"cloud_bin_{k}.pose.npy"))
    base_inv = np.linalg.inv(base)
    with open(os.path.join(fragments, f"cloud_bin_{k}.frames.pkl"), "rb") as fh:
        record = pickle.load(fh)
    stems = record["frames"]
    if "poses" in record:                                    # fuse_fragments --poses odometry: no pose file is read
        rel = np.asarray(record["poses"], np.float64)
        return [(os.path.join(raw_seq, os.path.basename(stem)), np.matmul(X, np.matmul(base_inv.astype(np.float64), T)))
                for stem, T in zip(stems, rel)]
    out = []
    for stem in stems:
        stem = os.path.join(raw_seq, os.path.basename(stem))
        pose = read_extrinsic(stem + ".pose.txt")
        if pose is None:
            continue
        out.append((stem, np.matmul(X, np.matmul(base_inv, pose).astype(np.float64))))
    return out


def load_frames(frames, height, width, pool, color=False):
    """(depth uint16 [F,H,W], poses fp64 [F,4,4]) of scene_poses' list; with color=True (depth, poses, uint8 [F,H,W,3])."""
    rgb = pool.map(lambda fr: read_color_jpg(fr[0] + ".color.jpg", height, width), frames) if color else None
    depth = list(pool.map(lambda fr: read_depth_png(fr[0] + ".depth.png", height, width), frames))
    depth = np.stack(depth) if depth else np.zeros((0, height, width), np.uint16)
    poses = np.stack([p for _, p in frames]) if frames else np.zeros((0, 4, 4))
    if not color:
        return depth, poses
    rgb = list(rgb)
    return depth, poses, (np.stack(rgb) if rgb else np.zeros((0, height, width, 3), np.uint8))


def integrate_scene(fragments, raw_seq, trajectory, out, voxel_length=3.0 / 512, sdf_trunc=0.04, depth_trunc=6.0,
                    lattice_offset=0.5, height=480, width=640, depth_scale=1000.0, device="cuda", threads=0, log=print,
                    color=False):
    """The command as a function; returns the dict it prints.  `vertices` / `triangles` of the mesh are in the file
    <out>/scene_mesh.ply."""
    from .fuse import TSDFVolume, _color_to_device, _depth_to_device
    t_start = time.perf_counter()
    intrinsic = np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(raw_seq)), "camera-intrinsics.txt"),
                           dtype=np.float32).astype(np.float64)
    used, skipped, jobs = [], [], []
    for rec in read_log(trajectory):
        k, X = rec.indices[0], rec.transformation
        if not np.isfinite(X).all() or not os.path.exists(os.path.join(fragments, f"cloud_bin_{k}.frames.pkl")):
            skipped.append(k)
            continue
        used.append(k)
        jobs.append(scene_poses(fragments, raw_seq, k, X))
    vol = TSDFVolume(intrinsic, height, width, voxel_length, sdf_trunc, depth_scale, depth_trunc, lattice_offset, device,
                     color=color)
    times = dict(decode=0.0, allocate=0.0, integrate=0.0, mesh=0.0, write=0.0)
    resident = []                                            # per fragment: (depth on the device, poses, colour or None)
    n_threads = max(1, min(threads or cpu_quota(), cpu_quota()))
    with cf.ThreadPoolExecutor(n_threads) as pool, cf.ThreadPoolExecutor(1) as ahead:
        submit = lambda frames: ahead.submit(load_frames, frames, height, width, pool, color)
        nxt = submit(jobs[0]) if jobs else None
        for i in range(len(jobs)):
            t = time.perf_counter()
            depth, poses, *rgb = nxt.result()
            nxt = submit(jobs[i + 1]) if i + 1 < len(jobs) else None      # decoded while the GPU opens this one's units
            times["decode"] += time.perf_counter() - t
            t = time.perf_counter()
            d = _depth_to_device(depth, vol.device)
            for a in range(0, len(poses), MAX_FRAMES_PER_CALL):
                vol.allocate(d[a:a + MAX_FRAMES_PER_CALL], poses[a:a + MAX_FRAMES_PER_CALL])
            resident.append((d, poses, _color_to_device(rgb[0], vol.device) if color else None))
            times["allocate"] += time.perf_counter() - t
    t = time.perf_counter()
    n_frames = 0
    for i in range(len(resident)):
        d, poses, c = resident[i]
        resident[i] = None
        for a in range(0, len(poses), MAX_FRAMES_PER_CALL):
            vol.integrate(d[a:a + MAX_FRAMES_PER_CALL], poses[a:a + MAX_FRAMES_PER_CALL],
                          c[a:a + MAX_FRAMES_PER_CALL] if color else None)
        n_frames += len(poses)
    if vol.device.type == "cuda":
        torch.cuda.synchronize(vol.device)
    times["integrate"] = time.perf_counter() - t
    t = time.perf_counter()
    vertices, triangles, *vertex_rgb = vol.extract_mesh(colors=True) if color else vol.extract_mesh()
    times["mesh"] = time.perf_counter() - t
    t = time.perf_counter()
    ensure_dir(out)
    write_ply_mesh(os.path.join(out, "scene_mesh.ply"), vertices, triangles, vertex_rgb[0] if color else None)
    times["write"] = time.perf_counter() - t
    times["total"] = time.perf_counter() - t_start
    res = dict(fragments_used=used, fragments_skipped=skipped, frames=n_frames, units=int(vol.n_units), flags=int(vol.flags),
               vertices=int(len(vertices)), triangles=int(len(triangles)), color=bool(color), seconds={k: round(v, 4) for k, v in times.items()})
    log(json.dumps(res))
    return res


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fragments", required=True, help="the directory fuse_fragments wrote for the sequence")
    ap.add_argument("--raw_seq", required=True, help="the raw sequence directory the fragments were fused from")
    ap.add_argument("--trajectory", required=True, help="trajectory.log of reconstruct")
    ap.add_argument("--out", required=True)
    ap.add_argument("--voxel_length", type=float, default=3.0 / 512)
    ap.add_argument("--sdf_trunc", type=float, default=0.04)
    ap.add_argument("--depth_trunc", type=float, default=6.0)
    ap.add_argument("--lattice_offset", type=float, default=0.5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--depth_scale", type=float, default=1000.0)
    ap.add_argument("--threads", type=int, default=0, help="decode threads (0 = the CPU quota)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--color", action="store_true",
                    help="integrate every frame's .color.jpg too: scene_mesh.ply gets uchar red, green, blue per vertex")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    integrate_scene(a.fragments, a.raw_seq, a.trajectory, a.out, a.voxel_length, a.sdf_trunc, a.depth_trunc, a.lattice_offset,
                    a.height, a.width, a.depth_scale, a.device, a.threads, color=a.color)
    return 0


if __name__ == "__main__":
    sys.exit(main())
