"""Time of matching.robust_transform (imf_robust_transform) and of one KITTI training iteration, split by stage.

  robust_transform  one call at n = 5 000 host to host (upload, one launch, the 136-byte download)
  torch_loop_gpu    the same 20 rounds written with torch operations on the same GPU (float32, as upstream), host to host
  torch_loop_cpu    that loop on the host's CPUs (at most 16 threads)
  iteration         one hardest-contrastive iteration at batch 2 on a synthetic odometry tree (tests/kitti_tree.py),
                    stages as tools/train_time.py splits them; `geometry` includes the ground truth (ICP on the first visit, the cache afterwards)

Usage: python tools/train_kitti_time.py [--iters 10] [--warmup 3] [--out FILE.json]
Prints one JSON line (milliseconds, medians)."""
import argparse
import json
import os
import pathlib
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = ("decode", "geometry", "pairs", "forward", "loss", "backward", "step")


def torch_loop(p0, p1):
    """The 20 rounds with torch operations on p0's device, float32."""
    cur, T, par = p0, torch.eye(4, device=p0.device), 1.0
    n = p0.shape[0]
    w = torch.ones(n, 1, device=p0.device)
    o, l = torch.zeros(n, device=p0.device), torch.ones(n, device=p0.device)
    for i in range(20):
        if i > 0 and i % 5 == 0:
            par /= 2.0
        x, y, z = cur[:, 0], cur[:, 1], cur[:, 2]
        A = torch.cat([torch.stack([o, z, -y, l, o, o], 1), torch.stack([-z, o, x, o, l, o], 1),
                       torch.stack([y, -x, o, o, o, l], 1)]) * w.repeat(3, 1)
        b = (p1 - cur).t().reshape(-1, 1) * w.repeat(3, 1)
        s = (torch.inverse(A.t() @ A) @ (A.t() @ b)).reshape(-1)
        sa, sb, sc = torch.sin(s[:3])
        ca, cb, cc = torch.cos(s[:3])
        R = torch.stack([torch.stack([cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa]),
                         torch.stack([sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa]),
                         torch.stack([-sb, cb * sa, cb * ca])])
        U = torch.eye(4, device=p0.device)
        U[:3, :3], U[:3, 3] = R, s[3:]
        cur = cur @ R.t() + s[3:]
        w = par / ((cur - p1).norm(dim=1, keepdim=True) + par)
        T = U @ T
    return T


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import robust_restate as RR
    import kitti_tree as TK
    from imfnet_amd.matching import robust_transform
    from imfnet_amd.train.data import KITTINMPairDataset
    from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config
    dev = "cuda:0"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p0, p1, _, _ = RR.make_case(seed=0, **RR.FAMILIES["outdoor_5deg"])
    res = {"n": len(p0), "iters": a.iters, "warmup": a.warmup}
    res["robust_transform_ms"] = median_ms(lambda: robust_transform(p0, p1, device=dev), a.iters, a.warmup)
    t0, t1 = torch.from_numpy(p0), torch.from_numpy(p1)
    res["torch_loop_gpu_ms"] = median_ms(lambda: torch_loop(t0.to(dev), t1.to(dev)).cpu(), a.iters, a.warmup)
    res["torch_loop_cpu_ms"] = median_ms(lambda: torch_loop(t0, t1), a.iters, a.warmup)
    res["cpu_threads"] = torch.get_num_threads()
    T_gpu, _ = robust_transform(p0, p1, device=dev)
    res["max_abs_diff_vs_torch_loop"] = float(np.abs(T_gpu - torch_loop(t0, t1).numpy()).max())

    z = np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))
    with tempfile.TemporaryDirectory() as tmp:
        root = pathlib.Path(tmp)
        TK.build_tree(root, {0: z["cloud_bin_0"], 1: z["cloud_bin_1"]})
        cfg = parse_config(["--dataset", "KITTINMPairDataset", "--kitti_root", str(root), "--batch_size", "2",
                            "--out_dir", str(root / "out")])
        ds = KITTINMPairDataset("train", [0], cfg, seed=0, device=dev)
        tr = HardestContrastiveTrainer(cfg, ds, None, device=dev)
        rows = []
        for k in range(a.warmup + a.iters):
            t = time.perf_counter()
            raws = [[ds.load(0), ds.load(1)]]
            tm = {"decode": time.perf_counter() - t}
            tr.train_step(raws, tm)
            if k >= a.warmup:
                rows.append(tm)
        tr.pool.shutdown()
        res["points_per_scan"], res["voxel_size"], res["batch_size"] = TK.N_POINTS, cfg.voxel_size, 2
    res["iteration_ms"] = {s: float(np.median([r.get(s, 0.0) for r in rows]) * 1e3) for s in STAGES}
    res["iteration_ms"]["iteration"] = float(sum(res["iteration_ms"].values()))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
