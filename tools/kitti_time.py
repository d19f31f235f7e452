"""Stage times of one synthetic KITTI-sized pair (about 120k points per scan) through the KITTI evaluator's GPU path
(imfnet_amd/evaluate_kitti.py), with torch.cuda.Events around every stage:

  quant5cm   the 5 cm float32-quotient voxelisation of both scans (imf_voxelize, mode 2)
  icp        imf_icp_point_to_point, 0.2 m, 200 iterations at most (iterations run reported)
  icp_offset the same from a start 0.1 m / 1 deg off the truth
  radius     imf_radius_count of the 0.3 m voxels at 0.45 m
  forward    the 0.3 m voxelisation + descriptors of both fragments (extract_features, quantize="f32")
  nn         nn_search over all voxels
  ransac     RANSAC, ransac_n 4, max_iter hypotheses (4 000 000 by default)
  total      the pair end to end: cold = ICP included (no cache file), warm = ground truth read from the cache

Usage: python tools/kitti_time.py [--points 120000] [--max_iter 4000000] [--reps 3] [--out FILE.json]
Prints one JSON line (milliseconds, the median of --reps repetitions after one warm-up)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from imfnet_amd import kitti as K                      # noqa: E402
from imfnet_amd.evaluate_kitti import build_model, describe, evaluate_pair   # noqa: E402
from imfnet_amd.matching import icp_point_to_point, nn_search, radius_count, ransac_registration   # noqa: E402
from kitti_restate import rigid, scene_points, write_tree   # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--max_iter", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    world = scene_points(rng, 3 * args.points, extent=50.0).astype(np.float64)
    P = np.tile(np.eye(4), (3, 1, 1))
    for t in range(3):
        P[t, :3, :3] = rigid(0.5 * t, [0, 1, 0], [0, 0, 0])[:3, :3]
        P[t, 0, 3] = 5.5 * t
    Vc = K.VELO2CAM.T
    scans = {}
    for t in range(3):
        A = np.linalg.inv(P[t] @ Vc)
        local = world @ A[:3, :3].T + A[:3, 3]
        keep = np.flatnonzero(np.linalg.norm(local[:, :2], axis=1) < 45.0)
        scans[t] = local[rng.permutation(keep)[:args.points]].astype(np.float32)
    xyz0, xyz1 = scans[0], scans[2]
    img = np.random.default_rng(1).uniform(0, 1, (1, 3, 120, 160)).astype(np.float32)
    model = build_model(None, 0, dev)
    M = K.pose_from_positions(P[0], P[2])

    def stages():
        r = {}
        r["quant5cm"], (s0, s1) = timed(lambda: (K.voxel_first_indices(xyz0, 0.05, dev),
                                                 K.voxel_first_indices(xyz1, 0.05, dev)))
        a = K.apply_transform(xyz0[s0], M)
        b = xyz1[s1].astype(np.float64)
        a_d, b_d = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        r["icp"], icp = timed(lambda: icp_point_to_point(a_d, b_d, 0.2, None, 200, device=dev))
        r["icp_iterations"], r["icp_points"] = icp[3], [len(a), len(b)]
        # the synthetic scans are exact views of one scene, so M is already right and ICP stops after a few
        # iterations; from a start 0.1 m / 1 deg off it has work to do (iterations reported)
        off = rigid(1.0, [0.3, 0.2, 1.0], [0.1, 0.05, 0.0])
        r["icp_offset"], icp2 = timed(lambda: icp_point_to_point(a_d, b_d, 0.2, off, 200, device=dev))
        r["icp_offset_iterations"] = icp2[3]
        T_gt = M @ icp[0]
        v0, v1 = K.voxel_first_indices(xyz0, 0.3, dev), K.voxel_first_indices(xyz1, 0.3, dev)
        p0, p1 = torch.from_numpy(xyz0[v0].astype(np.float64)).to(dev), torch.from_numpy(xyz1[v1].astype(np.float64)).to(dev)
        r["radius"], n = timed(lambda: radius_count(p0, p1, T_gt, 0.45, device=dev))
        r["matches"] = n
        r["forward"], (d0, d1) = timed(lambda: (describe(model, xyz0, 0.3, img, dev), describe(model, xyz1, 0.3, img, dev)))
        r["voxels"] = [len(d0[0]), len(d1[0])]
        r["nn"], corres = timed(lambda: nn_search(d0[1], d1[1]))
        r["ransac"], res = timed(lambda: ransac_registration(d0[0], d1[0], corres, 4, 0.3, 0.9, args.max_iter, 0, dev))
        return r

    with tempfile.TemporaryDirectory() as root:
        write_tree(root, {8: P}, {8: scans}, image=os.path.join(ROOT, "tests", "golden", "cloud_bin_0_0.png"))
        stages()                                             # warm-up (library load, allocator, capacities)
        runs = [stages() for _ in range(args.reps)]
        keys = ["quant5cm", "icp", "icp_offset", "radius", "forward", "nn", "ransac"]
        out = {k: float(np.median([r[k] for r in runs])) for k in keys}
        for k in ("icp_iterations", "icp_offset_iterations", "icp_points", "matches", "voxels"):
            out[k] = runs[-1][k]

        def pair(cold):
            if cold:
                for f in os.listdir(os.path.join(root, "icp")) if os.path.isdir(os.path.join(root, "icp")) else []:
                    os.remove(os.path.join(root, "icp", f))
            return timed(lambda: evaluate_pair(model, root, 8, 0, 2, P, 0.3, args.max_iter, 0, False, dev))[0]
        pair(True)
        out["total_cold"] = float(np.median([pair(True) for _ in range(args.reps)]))
        out["total_warm"] = float(np.median([pair(False) for _ in range(args.reps)]))
    out.update(points=args.points, max_iter=args.max_iter, reps=args.reps, device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
