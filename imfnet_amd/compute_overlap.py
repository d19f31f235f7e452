"""The 3DMatch training pairs from fused fragments: data/compute_overlap.py with the same directory contract, the
nearest-neighbour search on the GPU (imfnet_amd/overlap.py, csrc/overlap.hip), plus the pair lists the trainer reads.

    python -m imfnet_amd.compute_overlap --dataset_root <fragments> --out_root <overlaps> --list_root <lists>
                                         [--world_root <fragments in one frame>]

    <fragments>/<scene>/<seq>/cloud_bin_K.ply [+ cloud_bin_K.pose.npy, cloud_bin_K_0.png|jpg]
 -> <out>/<scene>/<seq>/cloud_bin_P-cloud_bin_Q.npy            int64 [n,2] rows (index in P, index in Q)
    <out>/<scene>/<seq>/cloud_bin_P-cloud_bin_Q-overlap.txt    the ratio n / max(n_P, n_Q)
    <lists>/<scene>@<seq>-<min_overlap>.txt                     "<scene>/<seq>/cloud_bin_P.ply <scene>/<seq>/cloud_bin_Q.ply <ratio>"

Kept from upstream: scenes in directory order, sequences and cloud_bin_*.ply in alphanumeric order, fragment number =
int(stem[10:]); a sequence whose output folder exists is skipped; clouds above --max_points are down-sampled by a choice
without replacement and become float32 (the row indices refer to the down-sampled clouds); pairs (P, Q) with
number(P) < number(Q), consecutive numbers left out; the tree is over P and every point of Q asks for one neighbour, kept
when sqrt(d^2) <= 0.075; pairs below a ratio of 0.3 write nothing.
Changed: the neighbour is the exact nearest one, ties to the lowest index (upstream: FLANN's approximate forest); the
down-sampling choice is seeded by --seed, scene, sequence and fragment name (upstream: unseeded); the .npz under
--temp_root holds points and indices only (upstream also pickles normals=None); the skip is decided before the
sequence is read (upstream down-samples it first).
The project's own: --list_root writes, per sequence, the pair list `python -m imfnet_amd.train` reads through
--overlap_path (upstream ships no producer for those files; the format is this project's), through a temporary file
and a rename once the sequence is complete.  --world_root moves every fragment by its cloud_bin_K.pose.npy (the two
lines upstream left commented out), writes it there with its image, and computes the overlap on what that file holds
(float32), so that the trainer's identity ground truth is true; the list's paths are then relative to --world_root,
which is what --threed_match_dir has to name.  --dist_thresh and --min_overlap are options (upstream: literals).
--threads sizes the host decode / write pool; the next sequence is decoded while the GPU works on the current one.
"""
import argparse
import concurrent.futures as cf
import glob
import os
import shutil
import sys

import numpy as np
import torch  # noqa: F401  (before the native library is loaded: both must share one HIP runtime)

from .dataio import read_ply_points
from .files import ensure_dir, sorted_alphanum
from .fuse_fragments import cpu_quota, list_folders, write_ply
from .overlap import DIST_THRESH, MAX_POINTS, MIN_OVERLAP, downsample


def fragment_number(stem):
    return int(stem[10:])                                    # "cloud_bin_K"


def list_fragments(folder):
    """The stems of the folder's cloud_bin_*.ply, alphanumeric (without the cloud_bin_K.mesh.ply of fuse_fragments --mesh)."""
    names = [os.path.basename(p) for p in glob.glob(os.path.join(glob.escape(folder), "cloud_bin_*.ply"))]
    names = [name for name in names if not name.endswith(".mesh.ply")]
    return [name[:-4] for name in sorted_alphanum(names)]


def load_cloud(cfg, scene, seq, stem):
    """One fragment: decoded, moved and written to --world_root when asked for, down-sampled, saved to --temp_root."""
    folder = os.path.join(cfg.dataset_root, scene, seq)
    xyz = read_ply_points(os.path.join(folder, stem + ".ply"))
    if cfg.world_root:
        pose_path = os.path.join(folder, stem + ".pose.npy")
        if not os.path.exists(pose_path):
            raise FileNotFoundError(f"--world_root needs {pose_path}")
        pose = np.load(pose_path).astype(np.float64)
        xyz = xyz @ pose[:3, :3].T + pose[:3, 3]
        out = os.path.join(cfg.world_root, scene, seq)
        ensure_dir(out)
        write_ply(os.path.join(out, stem + ".ply"), xyz)
        for ext in ("_0.png", "_0.jpg"):
            if os.path.exists(os.path.join(folder, stem + ext)):
                shutil.copyfile(os.path.join(folder, stem + ext), os.path.join(out, stem + ext))
    xyz = xyz.astype(np.float32)                             # what the PLY holds
    points, indices = downsample(xyz, cfg.max_points, (cfg.seed, scene, seq, stem))
    if cfg.temp_root:
        tmp = os.path.join(cfg.temp_root, scene, seq)
        os.makedirs(tmp, exist_ok=True)
        np.savez(os.path.join(tmp, stem + ".npz"), points=points, indices=indices)
    return points


def load_sequence(cfg, scene, seq, pool):
    stems = list_fragments(os.path.join(cfg.dataset_root, scene, seq))
    clouds = list(pool.map(lambda s: load_cloud(cfg, scene, seq, s), stems))
    return stems, clouds


def gpu_overlap(cfg, clouds, numbers):
    from .overlap import sequence_overlap
    return sequence_overlap(clouds, cfg.dist_thresh, cfg.min_overlap, numbers=numbers, device=cfg.device)


def write_pair(folder, p, q, ratio, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 2)
    np.save(os.path.join(folder, f"{p}-{q}.npy"), rows)
    with open(os.path.join(folder, f"{p}-{q}-overlap.txt"), "w") as f:
        f.write(f"{float(ratio)}")


def list_path(cfg, scene, seq):
    return os.path.join(cfg.list_root, f"{scene}@{seq}-{cfg.min_overlap:.2f}.txt")


def write_list(cfg, scene, seq, stems, kept):
    path = list_path(cfg, scene, seq)
    with open(path + ".tmp", "w") as f:
        for (i, j) in sorted(kept):
            f.write(f"{scene}/{seq}/{stems[i]}.ply {scene}/{seq}/{stems[j]}.ply {float(kept[(i, j)][0])}\n")
    os.replace(path + ".tmp", path)


def run(cfg, overlap=gpu_overlap, log=print):
    """Walks the tree; `overlap(cfg, clouds, numbers) -> {(i, j): (ratio, int64 [n,2])}` does the search for one sequence
    (clouds: the down-sampled float32 fragments in list order, numbers: their fragment numbers).  Returns the pairs
    written."""
    os.makedirs(cfg.out_root, exist_ok=True)
    os.makedirs(cfg.list_root, exist_ok=True)
    jobs = []
    for scene in list_folders(cfg.dataset_root, alphanum=False):
        for seq in list_folders(os.path.join(cfg.dataset_root, scene)):
            if os.path.exists(os.path.join(cfg.out_root, scene, seq)):
                log(f"    {scene}/{seq}: Skip...")
                continue
            jobs.append((scene, seq))
    written = 0
    threads = max(1, min(cfg.threads or cpu_quota(), cpu_quota()))
    with cf.ThreadPoolExecutor(threads) as pool, cf.ThreadPoolExecutor(1) as ahead:
        submit = lambda j: ahead.submit(load_sequence, cfg, j[0], j[1], pool)
        nxt = submit(jobs[0]) if jobs else None
        for n, (scene, seq) in enumerate(jobs):
            stems, clouds = nxt.result()
            nxt = submit(jobs[n + 1]) if n + 1 < len(jobs) else None      # decoded while the GPU searches this one
            folder = os.path.join(cfg.out_root, scene, seq)
            os.makedirs(folder)
            kept = overlap(cfg, clouds, [fragment_number(s) for s in stems])
            list(pool.map(lambda ij: write_pair(folder, stems[ij[0]], stems[ij[1]], *kept[ij]), sorted(kept)))
            write_list(cfg, scene, seq, stems, kept)
            written += len(kept)
            log(f"    {scene}/{seq}: {len(stems)} fragments, {len(kept)} pairs kept")
    return written


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset_root", required=True, help="the fragments (the output of imfnet_amd.fuse_fragments)")
    ap.add_argument("--out_root", required=True, help="correspondences and ratios")
    ap.add_argument("--list_root", required=True, help="pair lists for the trainer's --overlap_path")
    ap.add_argument("--temp_root", default=None, help="keep the down-sampled clouds here as .npz")
    ap.add_argument("--world_root", default=None, help="write the fragments moved by their pose here and pair those")
    ap.add_argument("--max_points", type=int, default=MAX_POINTS)
    ap.add_argument("--dist_thresh", type=float, default=DIST_THRESH)
    ap.add_argument("--min_overlap", type=float, default=MIN_OVERLAP)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threads", type=int, default=0, help="decode / write threads (0 = the CPU quota)")
    ap.add_argument("--device", default="cuda")
    return ap.parse_args(argv)


def main(argv=None):
    cfg = parse_args(argv)
    n = run(cfg)
    print(f"{n} pairs written to {cfg.out_root}, lists in {cfg.list_root}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
