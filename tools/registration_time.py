#!/usr/bin/env python3
"""Times of the registration refinements on S25 (the fixture pair voxelised at 2.5 cm), quoted in DESIGN.md section 15:

    python tools/registration_time.py [--reps 200]

estimate_normals(target, knn 30, 10 cm, viewpoint at the origin) and the point-to-plane / point-to-point ICP calls at
r = 3.75 cm from a 4 degree / 2.4 cm start, at max_iteration 0 (the grid and one correspondence stage) and 1 (one more
stage and one update), and information_matrix on the same pair, radius and start.  The coloured
leg paints both clouds with a smooth intensity of the position and times color_gradient alone
(the target's lists: knn 30 within 10 cm) and icp_colored with that gradient at max_iteration 0 and 1.  Each figure
is the median of --reps calls after a warm-up, host clock around a call that takes device tensors and ends with its
results on the host; `iteration` is the difference of the two medians."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def voxel_reps(x, voxel):
    from imfnet_amd import ops
    t = torch.as_tensor(x).to("cuda")
    lv = ops.voxelize(t, voxel)
    ops.sync_levels([lv])
    return t[lv.first_idx.long()].contiguous()


def timed(fn, reps):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    from imfnet_amd.matching import (color_gradient, estimate_normals, icp_colored, icp_point_to_plane, icp_point_to_point,
                                     information_matrix)
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))
    src = voxel_reps(z["cloud_bin_0"].astype(np.float64), 0.025)
    dst = voxel_reps(z["cloud_bin_1"].astype(np.float64), 0.025)
    ang = np.deg2rad(4.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
    T[:3, 3] = [0.02, -0.01, 0.01]
    res = dict(n_src=int(src.shape[0]), n_dst=int(dst.shape[0]))
    res["estimate_normals"] = timed(lambda: estimate_normals(dst, 30, 0.1, viewpoint=np.zeros(3)), a.reps)
    normals, counts = estimate_normals(dst, 30, 0.1, viewpoint=np.zeros(3))
    res["mean_neighbours"] = float(counts.mean())
    nrm = torch.from_numpy(normals).to("cuda")
    for name, fn in (("plane", lambda it: icp_point_to_plane(src, dst, nrm, 0.0375, init=T, max_iteration=it)),
                     ("point", lambda it: icp_point_to_point(src, dst, 0.0375, init=T, max_iteration=it))):
        t0, t1 = timed(lambda: fn(0), a.reps), timed(lambda: fn(1), a.reps)
        res[name] = dict(max_iteration_0=t0, max_iteration_1=t1, iteration_ms=t1["median_ms"] - t0["median_ms"],
                         n_corr=int(fn(1)[4]), iterations_to_stop=int(fn(30)[3]))
    paint = lambda p: 0.5 + 0.2 * torch.sin(3.1 * p[:, 0] + 0.3) + 0.2 * torch.cos(2.3 * p[:, 1]) + 0.1 * torch.sin(3.7 * p[:, 2])
    src_i, dst_i = paint(src @ torch.from_numpy(T[:3, :3].T).to("cuda") + torch.from_numpy(T[:3, 3]).to("cuda")), paint(dst)
    _, counts, nbr = estimate_normals(dst, 30, 0.1, viewpoint=np.zeros(3), return_neighbors=True)
    nbr, counts = torch.from_numpy(nbr).to("cuda"), torch.from_numpy(counts).to("cuda")
    res["color_gradient"] = timed(lambda: color_gradient(dst, nrm, dst_i, nbr, counts), a.reps)
    grad = torch.from_numpy(color_gradient(dst, nrm, dst_i, nbr, counts)).to("cuda")
    fn = lambda it: icp_colored(src, src_i, dst, nrm, dst_i, 0.0375, init=T, max_iteration=it, dst_gradient=grad)
    t0, t1 = timed(lambda: fn(0), a.reps), timed(lambda: fn(1), a.reps)
    res["color"] = dict(max_iteration_0=t0, max_iteration_1=t1, iteration_ms=t1["median_ms"] - t0["median_ms"],
                        n_corr=int(fn(1)[4]), iterations_to_stop=int(fn(30)[3]),
                        gradient_rows_zero=int((grad == 0).all(1).sum().item()))
    res["information_matrix"] = dict(timed(lambda: information_matrix(src, dst, T=T, max_corr_dist=0.0375), a.reps),
                                     n_corr=int(information_matrix(src, dst, T=T, max_corr_dist=0.0375)[1]))
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
