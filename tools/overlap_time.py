"""Time of the fragment-overlap engine (imfnet_amd/overlap.py, csrc/overlap.hip) on one synthetic sequence: the fixture
fragment (258 342 points) under seeded rigid motions along a path (0.1 m and 3 degrees a step), so that the overlap of
fragments k and k + d falls from above 0.3 to nothing as d grows.

  index_build_ms          one fragment's index, points resident (median over the fragments of the median run)
  bound_ms                the prefilter over all candidate pairs, one launch
  pair_ms                 the exact pass + emit + the read of the count, per surviving pair (min / median / max)
  bound_rejected_share    pairs the bound removes / candidate pairs
  sequence_ms             sequence_overlap host to host: upload, indices, bound, exact passes, download of the kept rows
  sequence_with_io_ms     the same behind compute_overlap.run on a tree of PLY files (decode, .npy / .txt / list writes)
  yardstick_ms            the parent's primitive on the same candidate pairs: a loop of matching.icp_point_to_point(
                          src=q, dst=p, max_corr_dist=thresh, max_iteration=0), points resident as fp64; it yields the
                          count only
  speedup                 yardstick_ms / sequence_ms

Usage: python tools/overlap_time.py [--fragments 40] [--iters 5] [--warmup 2] [--no-yardstick] [--no-io] [--out FILE.json]
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

THRESH, MIN_OVERLAP = 0.075, 0.3


def make_sequence(n_fragments, step=0.10, degrees=3.0):
    from scipy.spatial.transform import Rotation
    cloud = np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))["cloud_bin_0"].astype(np.float64)
    axis = int(np.argmax(np.ptp(cloud, axis=0)))
    centre = cloud.mean(0)
    rot_axis = np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1])
    rng = np.random.default_rng(0)
    out = []
    for k in range(n_fragments):
        Rm = Rotation.from_rotvec(np.deg2rad(degrees * k + rng.normal(0, 0.3)) * rot_axis).as_matrix()
        t = 0.01 * rng.standard_normal(3)
        t[axis] += step * k
        out.append(((cloud - centre) @ Rm.T + centre + t).astype(np.float32))
    return out


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=40)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--no-io", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from imfnet_amd import compute_overlap as CO
    from imfnet_amd import overlap as OV
    from imfnet_amd.matching import icp_point_to_point
    assert torch.cuda.is_available(), "overlap_time needs a GPU"
    dev = torch.device("cuda:0")
    clouds = make_sequence(a.fragments)
    pairs = OV.candidate_pairs(range(len(clouds)))
    res = {"device": torch.cuda.get_device_name(0), "fragments": len(clouds), "points_per_fragment": len(clouds[0]),
           "candidate_pairs": len(pairs), "iters": a.iters, "warmup": a.warmup, "thresh": THRESH, "min_overlap": MIN_OVERLAP}
    cell = float(np.float32(THRESH)) * OV.CELL_MARGIN
    resident = [torch.from_numpy(c).to(dev) for c in clouds]
    res["index_bytes_per_fragment"] = OV.FragmentIndex.device_bytes(len(clouds[0]))
    build = [float(np.median(timed(lambda: OV.FragmentIndex(r, cell, dev), a.iters, a.warmup))) for r in resident[:8]]
    res["index_build_ms"] = float(np.median(build))
    indices = OV.build_indices(clouds, THRESH, dev)
    res["cells_per_fragment"] = int(np.median([ix.n_cells for ix in indices]))
    res["chunks_per_fragment"] = int(np.median([ix.n_chunks for ix in indices]))
    res["bound_ms"] = float(np.median(timed(lambda: OV.overlap_bounds(indices, pairs, dev), a.iters, a.warmup)))
    bounds = OV.overlap_bounds(indices, pairs, dev)
    n = len(clouds[0])
    survivors = [p for p, b in zip(pairs, bounds.tolist()) if b / n >= MIN_OVERLAP]
    res["bound_survivors"] = len(survivors)
    res["bound_rejected_share"] = 1.0 - len(survivors) / len(pairs)
    buffers = OV.PairBuffers(n, dev)
    per_pair, counts = [], {}
    for i, j in survivors:
        ms = timed(lambda: counts.__setitem__((i, j), OV.pair_overlap(indices[i], indices[j], THRESH, buffers)[0]), a.iters,
                   1 if per_pair else a.warmup)
        per_pair.append(float(np.median(ms)))
    res["pair_ms"] = {"min": min(per_pair), "median": float(np.median(per_pair)), "max": max(per_pair), "sum": sum(per_pair)}
    res["kept_pairs"] = sum(1 for k, c in counts.items() if c / n >= MIN_OVERLAP)
    del indices, buffers
    seq_ms = timed(lambda: OV.sequence_overlap(clouds, THRESH, MIN_OVERLAP, device=dev), a.iters, a.warmup)
    res["sequence_ms"] = float(np.median(seq_ms))
    if not a.no_io:
        with tempfile.TemporaryDirectory() as tmp:
            folder = os.path.join(tmp, "frag", "scene", "seq")
            os.makedirs(folder)
            for k, c in enumerate(clouds):
                CO.write_ply(os.path.join(folder, f"cloud_bin_{k}.ply"), c)
            runs = []
            for r in range(1):                               # one run: it writes every kept pair's rows
                cfg = CO.parse_args(["--dataset_root", os.path.join(tmp, "frag"), "--out_root", os.path.join(tmp, f"out{r}"),
                                     "--list_root", os.path.join(tmp, f"list{r}")])
                t = time.perf_counter()
                written = CO.run(cfg, log=lambda s: None)
                runs.append((time.perf_counter() - t) * 1e3)
            res["sequence_with_io_ms"], res["sequence_with_io_runs"], res["pairs_written"] = float(np.median(runs)), 1, written
    if not a.no_yardstick:
        res64 = [r.double() for r in resident]
        icp_counts = {}

        def yardstick():
            for i, j in pairs:
                icp_counts[(i, j)] = icp_point_to_point(res64[j], res64[i], THRESH, max_iteration=0, device=dev)[4]

        icp_point_to_point(res64[2], res64[0], THRESH, max_iteration=0, device=dev)      # warm-up: one pair
        res["yardstick_ms"] = float(np.median(timed(yardstick, 1, 0)))
        res["yardstick_runs"] = 1
        res["speedup"] = res["yardstick_ms"] / res["sequence_ms"]
        # the same question, fp64 and a strict bound there: the counts agree to within the points at the threshold
        res["max_count_difference_vs_yardstick"] = max(abs(icp_counts[k] - c) for k, c in counts.items())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
