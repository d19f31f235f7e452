"""KITTI registration evaluation on the GPU -- scripts/evaluation_kitti_open3d_12.py (the third command of the
reference's README) over a KITTI odometry tree.

Per pair (imfnet_amd/kitti.py for the data side): the refined ground truth (ICP on the GPU, cached as the reference
caches it), the 0.3 m voxels of both scans in the float32-quotient mode, the overlap test (`radius_count` >= 1000
within 1.5 voxel, else the pair is skipped), descriptors for both fragments, correspondences = nearest target
descriptor of every source voxel (`nn_search` over all voxels), RANSAC with ransac_n=4, max_corr_dist = voxel, edge
similarity 0.9 and 4 000 000 hypotheses (`--max_iter` may lower it), then RTE / RRE / success in the reference's
float32 expressions.  One line per pair goes to `<out_root>/kitti_pairs.txt`:
`drive t0 t1 n_matches rte rre success` (a skipped pair: `drive t0 t1 n_matches skipped`), and one JSON summary line
is printed.  Ranks (torchrun env): pair k belongs to rank k % world; rank 0 merges the parts in pair order.
"""
import argparse
import json
import os

import numpy as np
import torch

from . import dist as idist
from . import kitti as K
from .matching import nn_search, radius_count, ransac_registration

RANSAC_ITERS = 4_000_000               # RANSACConvergenceCriteria(4000000, 10000): never stops early in Open3D 0.12
MATCH_MULT = 1.5                       # positive_pair_search_voxel_size_multiplier (config_kitti.py)


def build_model(checkpoint=None, seed=0, device="cuda"):
    """config_kitti.py's network (ResUNetBN2C, 32 outputs, conv1 5, normalised, bn_momentum 0.05); seeded weights
    (imfnet_amd.seeded, `seed`) when no checkpoint is given."""
    from .checkpoint import load_checkpoint
    from .model import load_model
    from .seeded import seeded_state_dict
    if checkpoint is not None:
        sd, cfg = load_checkpoint(checkpoint)
        name, n_out = cfg.get("model", "ResUNetBN2C"), cfg.get("model_n_out", 32)
        conv1, norm = cfg.get("conv1_kernel_size", 5), cfg.get("normalize_feature", True)
    else:
        sd = seeded_state_dict(seed=seed, with_unused_image_layers=True)
        name, n_out, conv1, norm = "ResUNetBN2C", 32, 5, True
    model = load_model(name)(1, n_out, bn_momentum=0.05, normalize_feature=norm, conv1_kernel_size=conv1, D=3,
                             config=None)
    model.load_state_dict(sd, strict=True)
    return model.eval().to(device)


def describe(model, xyz_f32, voxel_size, image, device):
    """(voxel representatives float64 [M,3], descriptors float32 device [M,32]) with the float32-quotient voxels."""
    from .extract import extract_features
    with torch.no_grad():
        return extract_features(model, xyz_f32, voxel_size=voxel_size, device=device, skip_check=True, image=image,
                                quantize="f32", host_descriptors=False)


def register_pair(xyz0, F0, xyz1, F1, voxel_size, max_iter=RANSAC_ITERS, seed=0, device="cuda"):
    """scripts/evaluation_kitti_open3d_12.py:103-117: correspondences over all voxels, RANSAC (ransac_n 4, distance
    checker and inlier bound = voxel, edge 0.9).  Returns the RANSAC tuple of `ransac_registration`."""
    f0 = torch.as_tensor(F0).to(device=device, dtype=torch.float32).contiguous()
    f1 = torch.as_tensor(F1).to(device=device, dtype=torch.float32).contiguous()
    corres = nn_search(f0, f1)
    return ransac_registration(xyz0, xyz1, corres, ransac_n=4, max_corr_dist=voxel_size, edge_similarity=0.9,
                               max_iter=max_iter, seed=seed, device=device)


def evaluate_pair(model, kitti_root, drive, t0, t1, positions, voxel_size, max_iter, seed, own_image, device):
    """One pair -> dict(n_matches, skipped, and for evaluated pairs T_ransac, T_gt, rte, rre, success)."""
    xyz0 = K.read_scan(K.velodyne_path(kitti_root, drive, t0))
    xyz1 = K.read_scan(K.velodyne_path(kitti_root, drive, t1))
    T_gt, _ = K.ground_truth(kitti_root, drive, t0, t1, xyz0, xyz1, positions, device)
    sel0 = K.voxel_first_indices(xyz0, voxel_size, device)
    sel1 = K.voxel_first_indices(xyz1, voxel_size, device)
    n_matches = radius_count(xyz0[sel0].astype(np.float64), xyz1[sel1].astype(np.float64), T_gt,
                             MATCH_MULT * voxel_size, device=device)
    out = dict(drive=drive, t0=t0, t1=t1, n_matches=n_matches, skipped=n_matches < K.MIN_MATCHES)
    if out["skipped"]:                                   # the loader raises ValueError; the script counts and skips it
        return out
    p0, p1 = K.pair_image_paths(kitti_root, drive, t0, t1, own_image)
    pts0, F0 = describe(model, xyz0, voxel_size, K.load_image(p0), device)
    pts1, F1 = describe(model, xyz1, voxel_size, K.load_image(p1), device)
    T = register_pair(pts0, F0, pts1, F1, voxel_size, max_iter, seed, device)[0]
    rte, rre = K.pair_errors(T, T_gt)
    out.update(T_ransac=T, T_gt=T_gt, rte=float(rte), rre=float(rre), success=K.is_success(rte, rre))
    return out


def pair_line(r):
    head = f"{r['drive']} {r['t0']} {r['t1']} {r['n_matches']}"
    if r["skipped"]:
        return head + " skipped"
    return head + f" {r['rte']!r} {r['rre']!r} {int(r['success'])}"


def summarize(lines):
    """The JSON summary from the per-pair lines (so that a merged file and the summary cannot disagree)."""
    meters = K.KittiMeters()
    skipped = 0
    for line in lines:
        f = line.split()
        if f[4] == "skipped":
            skipped += 1
            continue
        meters.update(np.float32(f[4]), np.float32(f[5]))
    s = meters.summary()
    s["skipped"] = skipped
    return s


def main(argv=None):
    ap = argparse.ArgumentParser(description="KITTI odometry registration evaluation on the GPU")
    ap.add_argument("--kitti_root", required=True, help="<root>/dataset/{sequences,poses}; ICP cache in <root>/icp")
    ap.add_argument("--out_root", required=True)
    ap.add_argument("-m", "--model", default=None, help="checkpoint .pth (default: seeded weights)")
    ap.add_argument("--voxel_size", type=float, default=0.3)
    ap.add_argument("--max_iter", type=int, default=RANSAC_ITERS)
    ap.add_argument("--seed", type=int, default=0, help="RANSAC draws (and the seeded weights)")
    ap.add_argument("--own_image", action="store_true", help="fragment 1 uses its own scan's image (the reference "
                    "reads scan t0's image for both, lib/data_loaders.py:508-509)")
    ap.add_argument("--sequences", default=None, help="file of sequence numbers (default 8 9 10, config/test_kitti.txt)")
    args = ap.parse_args(argv)
    rank, world, local = idist.init_from_env()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    os.makedirs(args.out_root, exist_ok=True)
    seqs = K.read_test_sequences(args.sequences)
    seqs = [d for d in seqs if os.path.isdir(os.path.join(args.kitti_root, "dataset", "sequences", "%02d" % d))]
    files = K.pair_list(args.kitti_root, seqs)
    positions = {d: K.read_poses(args.kitti_root, d) for d in seqs}
    model = build_model(args.model, args.seed, device)
    mine = []
    for k, (drive, t0, t1) in enumerate(files):
        if k % world != rank:
            continue
        r = evaluate_pair(model, args.kitti_root, drive, t0, t1, positions[drive], args.voxel_size, args.max_iter,
                          args.seed, args.own_image, device)
        mine.append(pair_line(r))
    base = os.path.join(args.out_root, "kitti_pairs")
    if world > 1:
        with open(f"{base}.part{rank}.txt", "w") as fh:
            fh.write("".join(l + "\n" for l in mine))
        import torch.distributed as dist
        dist.barrier()
    if rank == 0:
        if world > 1:                                      # merge the ranks' parts in pair order
            parts = [open(f"{base}.part{r}.txt").read().splitlines() for r in range(world)]
            lines = [parts[k % world][k // world] for k in range(sum(len(p) for p in parts))]
        else:
            lines = mine
        with open(base + ".txt", "w") as fh:
            fh.write("".join(l + "\n" for l in lines))
        print(json.dumps(summarize(lines)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
