"""Fragments from raw RGB-D sequences: data/fuse_fragments_3DMatch.py with the same options and directory contract, the
volume on the GPU (imfnet_amd/fuse.py, csrc/tsdf.hip).

    python -m imfnet_amd.fuse_fragments --dataset_root <raw> --out_root <fragments>

    <raw>/<scene>/camera-intrinsics.txt, <raw>/<scene>/<seq>/*.color.jpg + .depth.png + .pose.txt
 -> <out>/<scene>/<seq>/cloud_bin_K.ply, cloud_bin_K.pose.npy, cloud_bin_K.frames.pkl (--mesh: cloud_bin_K.mesh.ply too)

Kept from upstream: sequences and colour files in alphanumeric order; fragments of --frames_per_frag frames; poses read
as float32 and made relative to the fragment's first frame; a frame whose pose holds a NaN is skipped; a fragment whose
first frame has no pose writes nothing; voxel length --tsdf_cubic_size / 512 and a 0.04 m truncation.
The project's own: --voxel_length and --lattice_offset (0.5 = upstream's voxel centres; 0 with --voxel_length 0.006
gives the lattice of the published 3DMatch fragments); --write_image copies the first integrated frame's
colour file to cloud_bin_K_0.jpg, the name generate_desc and the trainer look for (upstream writes no image; which frame
its data set used is not recorded).  The PLY holds float x, y, z only; --color integrates every frame's .color.jpg with its
depth (upstream's RGB8 volume; the rule at the head of csrc/tsdf.hip) and adds uchar red, green, blue after the float
properties, in Open3D's order x y z [nx ny nz] red green blue; --normals adds float nx, ny, nz as
upstream's fragments carry them (estimate_normals after the extract: knn 30, within 5 voxel lengths, facing the
fragment's first camera, the origin; upstream signs them by the TSDF gradient and sums the covariance as cumulants).
--mesh also writes the surface of the same volume as triangles (TSDFVolume.extract_mesh) to
cloud_bin_K.mesh.ply (with --color: with vertex colours); cloud_bin_K.ply keeps its bytes.
--threads sizes the decode pool (upstream: joblib workers); the next fragment's depth (and, under --color, colour) files
are decoded while the GPU works on the current one.  Without --color every file has the bytes it had before the flag
existed.
--poses odometry is for a sequence without .pose.txt files (one somebody recorded themselves): no pose file is read, every
frame's colour file is decoded, and the fragment's camera poses come from frame-to-frame RGB-D odometry on the GPU
(imfnet_amd/odometry.py `track`; --odometry_levels, --odometry_max_depth_diff, --odometry_depth_max).  A frame
the odometry loses is left out as a frame with a NaN pose is (the fragment's first frame is the reference and always
kept, so every fragment is written); cloud_bin_K.pose.npy is the float32 identity (the fragment
lives in its own first camera, what reconstruct expects of unposed fragments) and cloud_bin_K.frames.pkl gains "poses":
float64 [F,4,4] of the kept frames relative to the fragment's first, which integrate_scene uses in place of the pose files.
With --poses file (the default) every output byte is what it was before the option existed.
"""
import argparse
import concurrent.futures as cf
import ctypes as C
import math
import os
import pickle
import shutil
import sys

import numpy as np
import torch  # noqa: F401  (before the native library is loaded: both must share one HIP runtime)

from . import _lib
from .files import ensure_dir, sorted_alphanum

SDF_TRUNC = 0.04


def cpu_quota():
    """CPUs this process may use: its affinity mask, a cgroup quota and OMP_NUM_THREADS, whichever is least."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    try:
        n = min(n, max(1, int(os.environ["OMP_NUM_THREADS"])))
    except (KeyError, ValueError):
        pass
    return max(1, n)


def list_folders(path, alphanum=True):
    names = [f for f in os.listdir(path) if os.path.isdir(os.path.join(path, f))]
    return sorted_alphanum(names) if alphanum else names


def list_color_files(seq_folder):
    return sorted_alphanum([f for f in os.listdir(seq_folder) if f.endswith(".color.jpg")])


def read_extrinsic(path):
    """float32 4x4, or None when the file holds a NaN (a lost track) -- upstream's read_extrinsic."""
    m = np.loadtxt(path, dtype=np.float32)
    return None if np.isnan(m).any() else m


def read_depth_png(path, height, width):
    """uint16 [height, width] (imf_png_read_u16; PIL for the kinds of PNG the native reader leaves out)."""
    L = _lib.lib()
    out = np.empty((height, width), np.uint16)
    h, w = C.c_int(), C.c_int()
    rc = L.imf_png_read_u16(os.fsencode(path), out.ctypes.data_as(C.c_void_p), out.size, C.byref(h), C.byref(w))
    if rc == -3:                                             # IMF_EUNSUPPORTED
        from PIL import Image
        with Image.open(path) as im:
            a = np.asarray(im)
        if a.shape != (height, width):
            raise ValueError(f"{path}: {a.shape}, expected ({height}, {width})")
        return a.astype(np.uint16)
    _lib.check(rc, f"imf_png_read_u16({path})")
    if (h.value, w.value) != (height, width):
        raise ValueError(f"{path}: {h.value} x {w.value}, expected {height} x {width} (--height / --width)")
    return out


def read_color_jpg(path, height, width):
    """uint8 [height, width, 3] = R, G, B (imf_jpeg_read_u8, bit-identical to PIL on baseline files; PIL for the kinds of
    JPEG the native reader leaves out)."""
    L = _lib.lib()
    out = np.empty((height, width, 3), np.uint8)
    h, w, c = C.c_int(), C.c_int(), C.c_int()
    rc = L.imf_jpeg_read_u8(os.fsencode(path), out.ctypes.data_as(C.c_void_p), out.size, C.byref(h), C.byref(w), C.byref(c))
    if rc == -3:                                             # IMF_EUNSUPPORTED
        from PIL import Image
        with Image.open(path) as im:
            a = np.asarray(im.convert("RGB"))
        if a.shape != (height, width, 3):
            raise ValueError(f"{path}: {a.shape[0]} x {a.shape[1]}, expected {height} x {width} (--height / --width)")
        return np.ascontiguousarray(a, np.uint8)
    _lib.check(rc, f"imf_jpeg_read_u8({path})")
    if (h.value, w.value) != (height, width):
        raise ValueError(f"{path}: {h.value} x {w.value}, expected {height} x {width} (--height / --width)")
    return out


def fragment_ranges(n_frames, frames_per_frag):
    """[(frag_id, first frame, one past the last)]."""
    n_frags = int(math.ceil(float(n_frames) / frames_per_frag))
    return [(k, k * frames_per_frag, min((k + 1) * frames_per_frag, n_frames)) for k in range(n_frags)]


def select_frames(color_paths, sid, eid, read_pose=read_extrinsic):
    """Upstream's loop over a fragment's frames without the volume: (base pose or None, [(frame stem, relative pose)]).
    A NaN pose skips the frame; if that was the first frame there is no base pose and the fragment ends at the next frame
    that has one, empty."""
    base = base_inv = None
    frames = []
    for fid in range(sid, eid):
        stem = color_paths[fid][:-10]
        pose = read_pose(stem + ".pose.txt")
        if pose is None:
            continue
        if fid == sid:
            base, base_inv = pose, np.linalg.inv(pose)
        if base_inv is None:
            break
        frames.append((stem, np.matmul(base_inv, pose)))
    return base, frames


def load_unposed_fragment(cfg, color_paths, sid, eid, pool):
    """--poses odometry: every frame's depth and colour, no pose file read; `poses` is None until `run` has tracked them."""
    stems = [color_paths[fid][:-10] for fid in range(sid, eid)]
    color = pool.map(lambda s: read_color_jpg(s + ".color.jpg", cfg.height, cfg.width), stems)
    depth = list(pool.map(lambda s: read_depth_png(s + ".depth.png", cfg.height, cfg.width), stems))
    return dict(base=np.eye(4, dtype=np.float32), stems=stems, depth=np.stack(depth), color=np.stack(list(color)), poses=None)


def gpu_track(cfg, intrinsic, frag):
    """(poses cam2first float64 [F,4,4], kept bool [F]) of an unposed fragment's frames (imfnet_amd.odometry.track)."""
    from .odometry import track
    levels = cfg.odometry_levels
    iterations = tuple(5 * 2 ** k for k in range(levels))[::-1]          # 5 at level 0, doubling per level: (20, 10, 5) for 3
    return track(frag["depth"], frag["color"], intrinsic[:3, :3], levels=levels, iterations=iterations,
                 max_depth_diff=cfg.odometry_max_depth_diff, depth_scale=cfg.depth_scale, depth_max=cfg.odometry_depth_max,
                 device=cfg.device)


def apply_track(frag, poses, kept):
    """Leaves out the frames the odometry dropped, exactly as select_frames leaves out NaN poses."""
    keep = np.flatnonzero(kept)
    frag["stems"] = [frag["stems"][i] for i in keep]
    frag["depth"], frag["color"] = frag["depth"][keep], frag["color"][keep]
    frag["poses"] = frag["tracked"] = np.ascontiguousarray(poses[keep], np.float64)


def load_fragment(cfg, color_paths, sid, eid, pool):
    """Poses and decoded depth of one fragment (under --color: `color` uint8 [F,H,W,3] of the same frames too), or None when
    it writes nothing."""
    if getattr(cfg, "poses", "file") == "odometry":
        return load_unposed_fragment(cfg, color_paths, sid, eid, pool)
    base, frames = select_frames(color_paths, sid, eid)
    if base is None:
        return None
    want_color = getattr(cfg, "color", False)
    color = pool.map(lambda fr: read_color_jpg(fr[0] + ".color.jpg", cfg.height, cfg.width), frames) if want_color else None
    depth = list(pool.map(lambda fr: read_depth_png(fr[0] + ".depth.png", cfg.height, cfg.width), frames))
    depth = np.stack(depth) if depth else np.zeros((0, cfg.height, cfg.width), np.uint16)
    poses = np.stack([p for _, p in frames]).astype(np.float64) if frames else np.zeros((0, 4, 4))
    frag = dict(base=base, stems=[s for s, _ in frames], depth=depth, poses=poses)
    if want_color:
        color = list(color)
        frag["color"] = np.stack(color) if color else np.zeros((0, cfg.height, cfg.width, 3), np.uint8)
    return frag


def _rgb_rows(path, rgb, n):
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.shape != (n, 3):
        raise ValueError(f"{path}: rgb must be uint8 [{n}, 3], got {rgb.dtype} {rgb.shape}")
    return rgb


def _vertex_records(path, floats, rgb):
    """float32 [n, k] and uint8 [n, 3] -> the packed vertex records `k floats, uchar red, green, blue`."""
    rec = np.empty(len(floats), np.dtype([("f", "<f4", (floats.shape[1],)), ("c", "u1", (3,))]))
    rec["f"], rec["c"] = floats, _rgb_rows(path, rgb, len(floats))
    return rec


RGB_PROPERTIES = "property uchar red\nproperty uchar green\nproperty uchar blue\n"


def write_ply(path, xyz, rgb=None):
    """float x, y, z (imf_ply_write_points); with `rgb` (uint8 [n,3]) the same header and floats with uchar red, green,
    blue after them, the file appearing under its name only when it is complete."""
    if rgb is not None:
        body = _vertex_records(path, np.asarray(xyz, np.float64).reshape(-1, 3).astype("<f4"), rgb)
        head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(body)}\nproperty float x\nproperty float y\n"
                f"property float z\n{RGB_PROPERTIES}end_header\n")
        with open(path + ".tmp", "wb") as fh:
            fh.write(head.encode("ascii"))
            fh.write(body.tobytes())
        os.replace(path + ".tmp", path)
        return
    xyz = np.ascontiguousarray(xyz, np.float64)
    rc = _lib.lib().imf_ply_write_points(os.fsencode(path), xyz.ctypes.data_as(C.c_void_p), len(xyz))
    _lib.check(rc, f"imf_ply_write_points({path})")


def write_ply_normals(path, xyz, normals, rgb=None):
    """write_ply's layout (binary little-endian, float32, the same x, y, z bytes) with `float nx, ny, nz` after them and,
    with `rgb`, uchar red, green, blue after those; the file appears under its name only when it is complete."""
    body = np.concatenate([np.asarray(xyz, np.float64), np.asarray(normals, np.float64)], 1).astype("<f4")
    if rgb is not None:
        body = _vertex_records(path, body, rgb)
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(body)}\nproperty float x\nproperty float y\n"
            "property float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
            + (RGB_PROPERTIES if rgb is not None else "") + "end_header\n")
    with open(path + ".tmp", "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(body.tobytes())
    os.replace(path + ".tmp", path)


def write_ply_mesh(path, vertices, triangles, rgb=None):
    """A triangle mesh in write_ply's layout (binary little-endian, float x, y, z; with `rgb` uchar red, green, blue per
    vertex after them) followed by `element face` with `property list uchar int vertex_indices`; the file appears under
    its name only when it is complete."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3).astype("<f4")
    if rgb is not None:
        v = _vertex_records(path, v, rgb)
    t = np.asarray(triangles).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError(f"{path}: triangle indices outside [0, {len(v)})")
    faces = np.empty(len(t), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    faces["n"], faces["v"] = 3, t
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\n"
            f"property float z\n{RGB_PROPERTIES if rgb is not None else ''}element face {len(t)}\n"
            "property list uchar int vertex_indices\nend_header\n")
    with open(path + ".tmp", "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(faces.tobytes())
    os.replace(path + ".tmp", path)


def fragment_normals(cfg, xyz):
    from .matching import estimate_normals
    if len(xyz) == 0:
        return np.zeros((0, 3))
    return estimate_normals(xyz, knn=30, max_radius=5.0 * cfg.voxel_length, viewpoint=np.zeros(3), device=cfg.device)[0]


def write_fragment(cfg, out_folder, frag_id, frag, xyz, normals=None, mesh=None, rgb=None):
    """`mesh`: (vertices, triangles) or, coloured, (vertices, triangles, rgb); `rgb`: the colours of xyz."""
    if mesh is not None:
        write_ply_mesh(os.path.join(out_folder, f"cloud_bin_{frag_id}.mesh.ply"), *mesh)
    if normals is None:
        write_ply(os.path.join(out_folder, f"cloud_bin_{frag_id}.ply"), xyz, rgb)
    else:
        write_ply_normals(os.path.join(out_folder, f"cloud_bin_{frag_id}.ply"), xyz, normals, rgb)
    np.save(os.path.join(out_folder, f"cloud_bin_{frag_id}.pose.npy"), frag["base"])
    with open(os.path.join(out_folder, f"cloud_bin_{frag_id}.frames.pkl"), "wb") as fh:
        record = {"frames": frag["stems"]}
        if "tracked" in frag:                                # --poses odometry: what integrate_scene reads instead of .pose.txt
            record["poses"] = frag["tracked"]
        pickle.dump(record, fh, protocol=pickle.HIGHEST_PROTOCOL)
    if cfg.write_image and frag["stems"]:
        shutil.copyfile(frag["stems"][0] + ".color.jpg", os.path.join(out_folder, f"cloud_bin_{frag_id}_0.jpg"))


def gpu_fuse(cfg, intrinsic, frag):
    """The fragment's points; under --mesh (points, (vertices, triangles)) of the same volume.  Under --color a dict:
    points, rgb and, under --mesh, mesh = (vertices, triangles, vertex rgb)."""
    from .fuse import fuse_volume
    color = frag["color"] if getattr(cfg, "color", False) else None
    vol = fuse_volume(frag["depth"], frag["poses"], intrinsic, voxel_length=cfg.voxel_length, sdf_trunc=SDF_TRUNC,
                      depth_scale=cfg.depth_scale, depth_trunc=cfg.depth_trunc, lattice_offset=cfg.lattice_offset,
                      device=cfg.device, color=color)
    if color is not None:
        points, rgb = vol.extract(colors=True)
        return dict(points=points, rgb=rgb, mesh=vol.extract_mesh(colors=True) if getattr(cfg, "mesh", False) else None)
    return (vol.extract(), vol.extract_mesh()) if getattr(cfg, "mesh", False) else vol.extract()


def run(cfg, fuse=gpu_fuse, log=print, normals=fragment_normals, track=gpu_track):
    """Walks the tree; `fuse(cfg, intrinsic, fragment) -> float64 [n,3]` (under --mesh: `(points, (vertices, triangles))`;
    under --color: dict(points, rgb, mesh = (vertices, triangles, rgb) or None)) does the volume work, `normals(cfg, xyz)`
    the normals under --normals, `track(cfg, intrinsic, fragment) -> (poses, kept)` the poses under --poses odometry.
    Returns the fragments written."""
    if cfg.voxel_length is None:
        cfg.voxel_length = cfg.tsdf_cubic_size / 512.0
    ensure_dir(cfg.out_root)
    jobs = []                                                # (scene, seq, intrinsic, color paths, frag id, sid, eid)
    for scene in list_folders(cfg.dataset_root, alphanum=False):
        intrinsic = np.loadtxt(os.path.join(cfg.dataset_root, scene, "camera-intrinsics.txt"), dtype=np.float32)
        for seq in list_folders(os.path.join(cfg.dataset_root, scene)):
            folder = os.path.join(cfg.dataset_root, scene, seq)
            colors = [os.path.join(folder, f) for f in list_color_files(folder)]
            ensure_dir(os.path.join(cfg.out_root, scene, seq))
            for k, sid, eid in fragment_ranges(len(colors), cfg.frames_per_frag):
                jobs.append((scene, seq, intrinsic.astype(np.float64), colors, k, sid, eid))
    written = 0
    threads = max(1, min(cfg.threads or cpu_quota(), cpu_quota()))
    with cf.ThreadPoolExecutor(threads) as pool, cf.ThreadPoolExecutor(1) as ahead:
        submit = lambda j: ahead.submit(load_fragment, cfg, j[3], j[5], j[6], pool)
        nxt = submit(jobs[0]) if jobs else None
        for i, (scene, seq, intrinsic, colors, k, sid, eid) in enumerate(jobs):
            frag = nxt.result()
            nxt = submit(jobs[i + 1]) if i + 1 < len(jobs) else None      # decoded while the GPU fuses this one
            if frag is None:
                log(f"    {scene}/{seq} fragment {k}: no pose for its first frame, nothing written")
                continue
            if frag["poses"] is None:                        # --poses odometry
                apply_track(frag, *track(cfg, intrinsic, frag))
            xyz = fuse(cfg, intrinsic, frag)
            rgb = None
            if isinstance(xyz, dict):
                xyz, rgb, mesh = xyz["points"], xyz.get("rgb"), xyz.get("mesh")
            else:
                xyz, mesh = xyz if isinstance(xyz, tuple) else (xyz, None)
            nrm = normals(cfg, xyz) if cfg.normals else None
            write_fragment(cfg, os.path.join(cfg.out_root, scene, seq), k, frag, xyz, nrm, mesh, rgb)
            written += 1
            log(f"    {scene}/{seq}/cloud_bin_{k}: {len(frag['stems'])} frames, {len(xyz)} points"
                + (f", {len(mesh[1])} triangles" if mesh is not None else ""))
    return written


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset_root", required=True)
    ap.add_argument("--out_root", required=True)
    ap.add_argument("--depth_scale", type=float, default=1000.0)
    ap.add_argument("--depth_trunc", type=float, default=6.0)
    ap.add_argument("--frames_per_frag", type=int, default=50)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--threads", type=int, default=0, help="decode threads (0 = the CPU quota)")
    ap.add_argument("--tsdf_cubic_size", type=float, default=3.0)
    ap.add_argument("--voxel_length", type=float, default=None, help="metres (default: tsdf_cubic_size / 512)")
    ap.add_argument("--lattice_offset", type=float, default=0.5,
                    help="0.5 = voxel centres (upstream); 0 = voxel corners (the published fragments, with --voxel_length 0.006)")
    ap.add_argument("--write_image", action="store_true", help="copy the first integrated frame's colour file to cloud_bin_K_0.jpg")
    ap.add_argument("--normals", action="store_true",
                    help="add float nx, ny, nz to the PLY: k-NN PCA normals (knn 30, 5 voxel lengths) facing the first camera")
    ap.add_argument("--mesh", action="store_true",
                    help="also write cloud_bin_K.mesh.ply: the triangle mesh of the same volume (marching tetrahedra)")
    ap.add_argument("--color", action="store_true",
                    help="integrate every frame's .color.jpg too: uchar red, green, blue in the PLY (and, with --mesh, in the mesh)")
    ap.add_argument("--poses", choices=("file", "odometry"), default="file",
                    help="file = every frame's .pose.txt (the data set's); odometry = frame-to-frame RGB-D odometry on the GPU")
    ap.add_argument("--odometry_levels", type=int, default=3, help="pyramid levels of the odometry, 1..5; 5 stages at the finest level, twice as many at each coarser one (3: 20, 10, 5)")
    ap.add_argument("--odometry_max_depth_diff", type=float, default=0.03, help="metres between a pixel and its match")
    ap.add_argument("--odometry_depth_max", type=float, default=4.0, help="metres; depth beyond it is ignored by the odometry")
    ap.add_argument("--device", default="cuda")
    return ap.parse_args(argv)


def main(argv=None):
    cfg = parse_args(argv)
    n = run(cfg)
    print(f"{n} fragments written to {cfg.out_root}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
