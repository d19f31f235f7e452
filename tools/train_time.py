"""Time of one hardest-contrastive training iteration (imfnet_amd/train) on the in-tree fixture pair, split by stage,
and imf_radius_pairs against scipy's cKDTree.

  decode     host decode of the batch's PLY files and images (sequential here; the trainer overlaps it on threads)
  geometry   random rotation, upload and first-occurrence voxelisation of every fragment of the batch
  pairs      radius_pairs (imf_radius_pairs) of every item at voxel x 1.5
  forward    the two batched training-mode forwards (forward_layers; --fusion_kernels hip: csrc/fusion_train.hip,
             --head_kernels hip: csrc/head_train.hip)
  loss       hardest-contrastive loss (sampling, two nn_search calls, masks; --loss_kernels hip: csrc/loss.hip)
  backward   loss.backward()
  step       optimizer.step() (--optim_kernels hip: one launch of csrc/optim.hip, which also leaves the weight images)
  iteration  the sum
The stages are separated by device synchronisations, so their sum is a little above a free-running iteration.

radius_pairs at S25 (the fixture pair voxelised at 2.5 cm) and S50k (the fixture x 1.7, the bench's shape) under a 4 deg
rigid motion, r = 3.75 cm, with the pair count; cpu_ckdtree is cKDTree(dst).query_ball_point(T src, r) on the host
(one thread) for the same sets.

Usage: python tools/train_time.py [--iters 10] [--warmup 3] [--batch 2] [--norm_kernels torch|hip] [--loss_kernels torch|hip]
       [--fusion_kernels torch|hip] [--image_kernels torch|hip] [--optim_kernels torch|hip] [--head_kernels torch|hip]
       [--model ResUNetIN2C] [--out FILE.json]
Prints one JSON line (milliseconds, medians)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imfnet_amd import ops                                   # noqa: E402
from imfnet_amd.matching import radius_pairs                 # noqa: E402
from imfnet_amd.train.data import IndoorPairDataset          # noqa: E402
from imfnet_amd.train.repro import SWITCHES, write_tree      # noqa: E402
from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config   # noqa: E402

STAGES = ("decode", "geometry", "pairs", "forward", "loss", "backward", "step")


def voxel_reps(x, voxel):
    t = torch.as_tensor(x).to("cuda")
    lv = ops.voxelize(t, voxel)
    ops.sync_levels([lv])
    return t[lv.first_idx.long()].contiguous()


def time_pairs(src, dst, T, r, reps):
    from scipy.spatial import cKDTree
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p, _ = radius_pairs(src, dst, T, r)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    s, d = src.cpu().numpy(), dst.cpu().numpy()
    c0 = time.perf_counter()
    hits = cKDTree(d).query_ball_point(s @ T[:3, :3].T + T[:3, 3], r)
    cpu = (time.perf_counter() - c0) * 1e3
    assert sum(len(h) for h in hits) == p.shape[0]
    return float(np.median(ts[1:])), int(p.shape[0]), cpu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    for s in SWITCHES:
        ap.add_argument("--" + s, default="torch", choices=("torch", "hip"))
    ap.add_argument("--model", default=None, help="the trainer's --model (default: the trainer's own, ResUNetBN2C)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))
    im = np.load(os.path.join(ROOT, "tests", "golden", "fixture_images.npz"))
    clouds = {0: z["cloud_bin_0"].astype(np.float64), 1: z["cloud_bin_1"].astype(np.float64)}
    images = {0: im["image_0"], 1: im["image_1"]}
    res = {}
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, clouds, images)
        cfg = parse_config(["--threed_match_dir", root, "--overlap_path", os.path.join(root, "overlap"),
                            "--batch_size", str(a.batch), "--out_dir", os.path.join(root, "out")] +
                           [v for s in SWITCHES for v in ("--" + s, getattr(a, s))] +
                           (["--model", a.model] if a.model else []))
        ds = IndoorPairDataset("train", ["sceneA"], cfg, seed=0)
        tr = HardestContrastiveTrainer(cfg, ds, None)
        rows, n_vox, n_pairs = [], [], []
        for it in range(a.warmup + a.iters):
            tm = {}
            t0 = time.perf_counter()
            raws = [ds.load(k % len(ds)) for k in range(a.batch)]
            tm["decode"] = time.perf_counter() - t0
            tr.train_step([raws], timings=tm)
            if it >= a.warmup:
                rows.append(tm)
            if it == 0:
                items = [ds.prepare(r) for r in raws]
                n_vox = [[int(i["xyz0"].shape[0]), int(i["xyz1"].shape[0])] for i in items]
                n_pairs = [int(i["matches"].shape[0]) for i in items]
        tr.pool.shutdown()
    for k in STAGES:
        res[k] = float(np.median([r.get(k, 0.0) for r in rows])) * 1e3
    res["iteration"] = float(np.median([sum(r.get(k, 0.0) for k in STAGES) for r in rows])) * 1e3
    res.update({s: getattr(a, s) for s in SWITCHES})
    res["model"] = cfg.model
    res["iteration_spread"] = float(np.ptp([sum(r.get(k, 0.0) for k in STAGES) for r in rows])) * 1e3
    res.update(batch=a.batch, voxels=n_vox, positive_pairs=n_pairs, rotation=True, scale=False)
    T = np.eye(4)
    ang = np.deg2rad(4.0)
    T[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    T[:3, 3] = [0.02, -0.01, 0.01]
    for name, scale in (("S25", 1.0), ("S50k", 1.7)):
        src, dst = voxel_reps(clouds[0] * scale, 0.025), voxel_reps(clouds[1] * scale, 0.025)
        ms, n, cpu = time_pairs(src, dst, T, 0.0375, 5)
        res[f"radius_pairs_{name}"] = ms
        res[f"radius_pairs_{name}_pairs"] = n
        res[f"radius_pairs_{name}_voxels"] = [int(src.shape[0]), int(dst.shape[0])]
        res[f"cpu_ckdtree_{name}"] = cpu
    res.update(iters=a.iters, device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
