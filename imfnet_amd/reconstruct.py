"""Reconstruct a sequence: register the fragments of a directory pairwise, weigh every pair with its information matrix,
optimise the pose graph with line processes over the loop closures, and write the fragments' poses.

    python -m imfnet_amd.reconstruct --fragments DIR [--descriptor fpfh | --descriptor imfnet -m checkpoint.pth]
                                     [--voxel_size 0.025] [--refine plane|color] [--min_fitness 0.3] [--pairs all|FILE]
                                     [--preference_loop_closure 1.0] [--merge_voxel V] --out DIR

The pipeline of Choi, Zhou, Koltun 2015 after the fragments: DIR holds cloud_bin_K.ply, K = 0..N-1 (with --descriptor
imfnet also cloud_bin_K_0.png|jpg, found as generate_desc finds them).  Every fragment's features are computed once
(`register.fragment_features`, the normals point-to-plane ICP needs and, with --refine color, the intensities and the
colour gradient coloured ICP needs: every cloud_bin_K.ply must then carry red, green, blue as `fuse_fragments --color`
writes them).  Every pair i < j -- all of them, or the lines
`i j` of --pairs FILE -- is registered with source = j onto target = i (`register.register_features`, seeded with --seed +
the pair's number), and `matching.information_matrix(src = j, dst = i, T)` is taken at 1.5 voxel.  The pair becomes an edge
when ICP's fitness is at least --min_fitness; the edge is uncertain (it has a line process) unless j = i + 1.
`pose_graph.optimize` then finds the poses X_k that map fragment k into fragment 0's frame.

Writes into --out:
  trajectory.log   records `k k N` + X_k (NaN for a fragment no kept pair reaches);
  pairs.log        the edges that survived, `i j N` + T_ij (fragment j into fragment i's frame): the gt.log format;
  pairs.info       their information matrices in the gt.info block order (translation first, pose_graph.benchmark_order),
                   so that `evaluate --benchmark_root` accepts pairs.log / pairs.info as a scene's gt.log / gt.info;
  graph.json       per edge: i, j, fitness, rmse, n_corr (of the information matrix), uncertain, l, kept; the pairs below
                   --min_fitness; the unreached fragments; the stage times;
  scene.ply        with --merge_voxel V: all fragments moved by their poses, then `extract.voxel_representatives` at V.
Prints one JSON line: fragments, pairs, edges, kept, unreached, E first and last, the stage times.
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

from .register import DESCRIPTOR_CHOICES, REFINE_CHOICES


def list_fragments(directory):
    """The cloud_bin_K.ply of a directory, K = 0..N-1 without a gap, in the order of K."""
    found = {}
    for name in os.listdir(directory):
        m = re.fullmatch(r"cloud_bin_(\d+)\.ply", name)
        if m:
            found[int(m.group(1))] = os.path.join(directory, name)
    if sorted(found) != list(range(len(found))) or not found:
        raise ValueError(f"{directory}: expected cloud_bin_0.ply .. cloud_bin_N-1.ply, found numbers {sorted(found)}")
    return [found[k] for k in range(len(found))]


def read_pairs(spec, n):
    """"all": every i < j; else a file of lines `i j` (i < j, blank lines and # comments skipped)."""
    if spec == "all":
        return [(i, j) for i in range(n) for j in range(i + 1, n)]
    pairs = []
    for line in open(spec).read().splitlines():
        line = line.split("#")[0].split()
        if not line:
            continue
        i, j = int(line[0]), int(line[1])
        if not 0 <= i < j < n:
            raise ValueError(f"{spec}: pair ({i}, {j}) with {n} fragments; expected 0 <= i < j < {n}")
        pairs.append((i, j))
    return pairs


def reconstruct(points, images=None, model=None, cfg=None, descriptor="fpfh", voxel_size=0.025, refine="plane",
                min_fitness=0.3, pairs="all", preference_loop_closure=1.0, seed=0, device="cuda", colors=None):
    """points: the fragments' float64 [n, 3] arrays; images: their [1, C, H, W] arrays (descriptor="imfnet"); colors: their
    uint8 [n, 3] colours (refine="color").  Returns
    dict(poses [N, 4, 4], edges (list of dicts: i, j, T, info, fitness, rmse, n_corr, uncertain, l, kept), rejected (pairs
    below min_fitness), unreached, E, times)."""
    from .matching import estimate_normals, information_matrix
    from .pose_graph import PoseGraph, optimize
    from .register import check_colors, down_intensity, fragment_features, register_features, target_color_terms
    n = len(points)
    check_colors(refine, [(f"fragment {k}", points[k], colors[k] if colors is not None else None) for k in range(n)])
    dev = torch.device(device)
    pair_list = read_pairs(pairs, n) if isinstance(pairs, str) else [(int(i), int(j)) for i, j in pairs]
    r = 1.5 * voxel_size
    times = {}

    def timed(name, t0):
        torch.cuda.synchronize(dev)
        times[name] = times.get(name, 0.0) + time.time() - t0

    t0 = time.time()
    down, feat, normals = [], [], []
    for k in range(n):
        xyz, F = fragment_features(model, cfg, points[k], images[k] if images is not None else None, voxel_size=voxel_size,
                                   device=dev, descriptor=descriptor)
        down.append(xyz)
        feat.append(F)
    timed("features", t0)
    if refine in ("plane", "color"):
        t0 = time.time()
        targets = {i for i, _ in pair_list}
        normals = [estimate_normals(down[k], knn=30, max_radius=4.0 * voxel_size, viewpoint=np.zeros(3), device=dev)[0]
                   if k in targets else None for k in range(n)]
        timed("normals", t0)
    inten, color_terms = [None] * n, [None] * n
    if refine == "color":                                 # every fragment's intensities, every target's gradient: once
        t0 = time.time()
        inten = [down_intensity(points[k], colors[k], down[k], voxel_size, dev) for k in range(n)]
        color_terms = [target_color_terms(down[k], normals[k], inten[k], voxel_size, dev) if k in targets else None
                       for k in range(n)]
        timed("gradient", t0)

    graph = PoseGraph(n)
    edges, rejected = [], []
    for number, (i, j) in enumerate(pair_list):
        t0 = time.time()
        res = register_features(points[j], points[i], (down[j], down[i]), (feat[j], feat[i]), voxel_size=voxel_size,
                                seed=seed + number, refine=refine, device=dev,
                                target_normals=normals[i] if refine in ("plane", "color") else None,
                                source_intensity=inten[j], target_color=color_terms[i])
        timed("register", t0)
        if not (res["fitness"] >= min_fitness and np.isfinite(res["T"]).all()):
            rejected.append(dict(i=i, j=j, fitness=res["fitness"], rmse=res["rmse"]))
            continue
        t0 = time.time()
        info, n_corr = information_matrix(down[j], down[i], T=res["T"], max_corr_dist=r, device=dev)
        timed("information", t0)
        uncertain = j != i + 1
        graph.add_edge(i, j, res["T"], info, uncertain, fitness=res["fitness"])
        edges.append(dict(i=i, j=j, T=res["T"], info=info, fitness=res["fitness"], rmse=res["rmse"], n_corr=n_corr,
                          uncertain=uncertain))
    t0 = time.time()
    poses, l, kept, E = optimize(graph, r, preference_loop_closure=preference_loop_closure)
    times["optimize"] = time.time() - t0
    for ed, lk, kk in zip(edges, l, kept):
        ed["l"], ed["kept"] = float(lk), bool(kk)
    unreached = [k for k in range(n) if not np.isfinite(poses[k]).all()]
    return dict(poses=poses, edges=edges, rejected=rejected, unreached=unreached, E=E, times=times)


def write_outputs(out_dir, result, points=None, merge_voxel=None, device="cuda"):
    """trajectory.log, pairs.log, pairs.info, graph.json and, with merge_voxel, scene.ply (see the module's head)."""
    from .pose_graph import benchmark_order, write_info, write_log
    os.makedirs(out_dir, exist_ok=True)
    poses, n = result["poses"], len(result["poses"])
    write_log(os.path.join(out_dir, "trajectory.log"), [(k, k, n, poses[k]) for k in range(n)])
    kept = [ed for ed in result["edges"] if ed["kept"]]
    write_log(os.path.join(out_dir, "pairs.log"), [(ed["i"], ed["j"], n, ed["T"]) for ed in kept])
    write_info(os.path.join(out_dir, "pairs.info"), [(ed["i"], ed["j"], n, benchmark_order(ed["info"])) for ed in kept])
    num = lambda v: None if not np.isfinite(v) else float(v)
    graph = dict(fragments=n,
                 edges=[dict(i=ed["i"], j=ed["j"], fitness=ed["fitness"], rmse=ed["rmse"], n_corr=ed["n_corr"],
                             uncertain=ed["uncertain"], l=num(ed["l"]), kept=ed["kept"]) for ed in result["edges"]],
                 rejected=result["rejected"], unreached=result["unreached"], E=result["E"],
                 times={k: round(v, 6) for k, v in result["times"].items()})
    with open(os.path.join(out_dir, "graph.json"), "w") as fh:
        json.dump(graph, fh, indent=1)
    if merge_voxel:
        from .extract import voxel_representatives
        from .fuse_fragments import write_ply
        moved = [points[k] @ poses[k][:3, :3].T + poses[k][:3, 3] for k in range(n) if k not in result["unreached"]]
        scene = voxel_representatives(np.concatenate(moved), merge_voxel, torch.device(device))
        write_ply(os.path.join(out_dir, "scene.ply"), scene)
        graph["scene_points"] = len(scene)
    return graph


def make_parser():
    ap = argparse.ArgumentParser(prog="python -m imfnet_amd.reconstruct", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fragments", required=True, help="directory of cloud_bin_K.ply (and cloud_bin_K_0.png|jpg for imfnet)")
    ap.add_argument("--descriptor", choices=DESCRIPTOR_CHOICES, default="fpfh",
                    help="fpfh: hand-crafted, no checkpoint and no images; imfnet: the network's descriptors")
    ap.add_argument("-m", "--model", default=None, help="checkpoint (.pth) for --descriptor imfnet; default: seeded weights")
    ap.add_argument("--voxel_size", type=float, default=0.025)
    ap.add_argument("--refine", choices=REFINE_CHOICES, default="plane")
    ap.add_argument("--min_fitness", type=float, default=0.3, help="a pair becomes an edge at this ICP fitness")
    ap.add_argument("--pairs", default="all", help="all, or a file of lines `i j` with i < j")
    ap.add_argument("--preference_loop_closure", type=float, default=1.0)
    ap.add_argument("--merge_voxel", type=float, default=None, help="write scene.ply, one point per voxel of this size")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None):
    args = make_parser().parse_args(argv)
    from .dataio import read_ply_colors, read_ply_points
    files = list_fragments(args.fragments)
    colors = None
    if args.refine == "color":
        colors = [read_ply_colors(f) for f in files]
        for f, c in zip(files, colors):
            if c is None:
                raise SystemExit(f"--refine color: {f} has no red, green, blue")
    points = [np.array(read_ply_points(f), np.float64) for f in files]
    model = cfg = images = None
    if args.descriptor == "imfnet":
        from .generate_desc import load_image
        from .register import load_network
        model, cfg = load_network(args.model, torch.device(args.device))
        images = [load_image(f, cfg) for f in files]
    pairs = read_pairs(args.pairs, len(files))
    result = reconstruct(points, images, model, cfg, descriptor=args.descriptor, voxel_size=args.voxel_size,
                         refine=args.refine, min_fitness=args.min_fitness, pairs=pairs,
                         preference_loop_closure=args.preference_loop_closure, seed=args.seed, device=args.device,
                         colors=colors)
    graph = write_outputs(args.out, result, points, args.merge_voxel, args.device)
    E = result["E"]
    print(json.dumps(dict(fragments=len(files), pairs=len(pairs), edges=len(result["edges"]),
                          kept=sum(ed["kept"] for ed in result["edges"]), unreached=result["unreached"],
                          E_first=E[0] if E else None, E_last=E[-1] if E else None, times=graph["times"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
