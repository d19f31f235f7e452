"""Register one pair of fragments end to end: descriptors, keypoints, RANSAC, ICP refinement.

    python -m imfnet_amd.register --source A.ply --source_image A.png --target B.ply --target_image B.png
                                  [-m checkpoint.pth] [--refine {none,point,plane}] [--out T.txt]
    python -m imfnet_amd.register --descriptor fpfh --source A.ply --target B.ply
    python -m imfnet_amd.register --descriptor fpfh --source A.ply --target B.ply --refine color      (coloured fragments)

The stages are the library's own, in the order scripts/evaluation_3dmatch.py and scripts/benchmark_util.py use them:
`extract_features` on both fragments, the keypoint draw (`num_keypoints` raw points without replacement from
RandomState(seed), source first) and `select_keypoints`, RANSAC on the nearest-descriptor correspondences (ransac_n = 3,
1.5 voxel, edge similarity 0.9), then ICP on the voxel representatives at 1.5 voxel: point-to-point, or point-to-plane
against the target's `estimate_normals(knn=30, max_radius=4 voxel, viewpoint=origin)`, or coloured ICP (--refine color:
both files must carry red, green, blue as `fuse_fragments --color` writes them; a representative has its own point's
colour; those normals, the colour gradient over the 30 nearest representatives within 4 voxel, 30 iterations,
lambda_geometric 0.968).  --skip_global starts the refinement from --init (identity when absent); the descriptors are
still extracted.  Without -m the network runs on the seeded weights of the test oracle: the global stage is then
meaningless, the plumbing is the same.
--descriptor fpfh needs neither a checkpoint nor the images (they are not read): the descriptors are `compute_fpfh` on the
voxel representatives (radius 5 voxel, max_nn 64, normals at 2 voxel facing the origin, zero-padded to 64 columns); the
keypoints, RANSAC and the refinement are the same.

Writes the 4x4 source->target matrix to --out (np.savetxt) and prints one JSON line: fitness, rmse, iterations, n_corr,
the stage times in seconds and the matrix.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFINE_CHOICES = ("none", "point", "plane", "color")
DESCRIPTOR_CHOICES = ("imfnet", "fpfh")


def load_network(checkpoint, device):
    """(model on the device, config) of a checkpoint, or of the seeded weights (oracle/imf_oracle.py) when it is None."""
    from .checkpoint import Config, load_checkpoint
    from .model import load_model
    if checkpoint:
        sd, cfg = load_checkpoint(checkpoint)
    else:
        oracle = os.path.join(ROOT, "oracle")
        if oracle not in sys.path:
            sys.path.insert(0, oracle)
        import imf_oracle
        sd, cfg = imf_oracle.seeded_state_dict(seed=0, with_unused_image_layers=True), Config()
    model = load_model(cfg.model)(1, cfg.model_n_out, bn_momentum=cfg.bn_momentum, normalize_feature=cfg.normalize_feature,
                                  conv1_kernel_size=cfg.conv1_kernel_size, D=3, config=cfg)
    model.load_state_dict(sd, strict=True)
    return model.eval().to(device), cfg


def load_image(path, cfg):
    from .dataio import image_to_nchw, process_image, read_image
    img = read_image(path)
    if img.shape[0] != cfg.image_H or img.shape[1] != cfg.image_W:
        img = process_image(image=img, aim_H=cfg.image_H, aim_W=cfg.image_W)
    return image_to_nchw(img)


def fpfh_descriptors(xyz_down, voxel_size, device="cuda"):
    """The FPFH descriptors of voxel representatives as this command and imfnet_amd.fpfh_desc compute them: float32 device
    tensor [M, 64], columns 33.. zero."""
    from .matching import compute_fpfh
    return compute_fpfh(xyz_down, radius=5.0 * voxel_size, max_nn=64, normal_knn=30, normal_radius=2.0 * voxel_size,
                        viewpoint=np.zeros(3), width=64, device=device)


def fragment_features(model, cfg, points, image, voxel_size=0.025, device="cuda", descriptor="imfnet"):
    """One fragment's voxel representatives and their descriptors: (xyz_down float64 numpy [M, 3], device tensor [M, C]).
    With descriptor="fpfh" model, cfg and image are not used."""
    from .extract import extract_features, voxel_representatives
    if descriptor not in DESCRIPTOR_CHOICES:
        raise ValueError(f"descriptor must be one of {DESCRIPTOR_CHOICES}, got {descriptor!r}")
    dev = torch.device(device)
    with torch.no_grad():
        if descriptor == "fpfh":
            xyz = voxel_representatives(np.asarray(points, np.float64), voxel_size, dev)
            F = fpfh_descriptors(xyz, voxel_size, dev)
        else:
            xyz, F = extract_features(model, np.asarray(points, np.float64), voxel_size=voxel_size, device=dev,
                                      skip_check=True, image=image)
    return np.asarray(xyz, np.float64), F


def check_colors(refine, named):
    """refine="color" needs uint8 [n, 3] colours for every fragment: refused here, before any GPU work."""
    if refine != "color":
        return
    for name, pts, rgb in named:
        if rgb is None:
            raise ValueError(f"refine='color': {name} has no colours (red, green, blue)")
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8 or rgb.shape != (len(pts), 3):
            raise ValueError(f"refine='color': the colours of {name} must be uint8 [{len(pts)}, 3], got {rgb.dtype} "
                             f"{rgb.shape}")


def down_intensity(points, colors, down, voxel_size, device="cuda"):
    """`matching.intensity` of the voxel representatives `down` of `points`: every representative's own point's colour."""
    from .extract import voxel_representatives
    from .matching import intensity
    xyz, index = voxel_representatives(np.asarray(points, np.float64), voxel_size, torch.device(device), return_index=True)
    if not np.array_equal(xyz, down):
        raise ValueError("down_intensity: `down` is not the voxel representatives of `points` at this voxel size")
    return intensity(np.asarray(colors)[index])


def target_color_terms(down, normals, inten, voxel_size, device="cuda"):
    """What coloured ICP needs of a target besides its normals: dict(intensity [M], gradient [M, 3]), the gradient over
    the lists of `estimate_normals(knn=30, max_radius=4 voxel)`."""
    from .matching import color_gradient, estimate_normals
    _, counts, nbr = estimate_normals(down, knn=30, max_radius=4.0 * voxel_size, device=device, return_neighbors=True)
    return dict(intensity=inten, gradient=color_gradient(down, normals, inten, nbr, counts, device=device))


def register_features(source, target, down, feat, voxel_size=0.025, num_keypoints=5000, ransac_iter=50000, seed=0,
                      init=None, skip_global=False, refine="plane", device="cuda", times=None, target_normals=None,
                      source_colors=None, target_colors=None, source_intensity=None, target_color=None):
    """The keypoint draw, RANSAC and the refinement on two fragments' features.  source / target: the raw points; down,
    feat: (source's, target's) `fragment_features`.  target_normals: the target's `estimate_normals(knn=30, max_radius=4
    voxel, viewpoint=origin)` when the caller holds them (refine="plane" or "color"), else computed here.  refine="color":
    source_colors / target_colors are the raw points' uint8 [n, 3] colours; source_intensity (`down_intensity` of the
    source) and target_color (`target_color_terms` of the target) replace them when the caller holds those.  times: a dict
    that receives the stage times.  Returns dict(T 4x4 numpy source->target, fitness, rmse, iterations, n_corr, times)."""
    from .matching import (estimate_normals, icp_colored, icp_point_to_plane, icp_point_to_point, nn_search,
                           ransac_registration, select_keypoints)
    if refine not in REFINE_CHOICES:
        raise ValueError(f"refine must be one of {REFINE_CHOICES}, got {refine!r}")
    check_colors(refine, [(name, pts, rgb) for name, pts, rgb, held in
                           (("the source", source, source_colors, source_intensity),
                            ("the target", target, target_colors, target_color)) if held is None])
    dev = torch.device(device)
    times = {} if times is None else times

    def timed(name, t0):
        torch.cuda.synchronize(dev)
        times[name] = time.time() - t0

    r = 1.5 * voxel_size
    T = np.eye(4) if init is None else np.asarray(init, np.float64).reshape(4, 4)
    if not skip_global:
        t0 = time.time()
        rng = np.random.RandomState(seed)
        keys = []
        for pts, xyz in zip((source, target), down):
            pts = np.asarray(pts, np.float64)
            sample = pts[rng.choice(len(pts), min(num_keypoints, len(pts)), replace=False)]
            keys.append(select_keypoints(sample, xyz, voxel_size, device=dev))
        f0 = feat[0][torch.as_tensor(keys[0], device=dev)].float().contiguous()
        f1 = feat[1][torch.as_tensor(keys[1], device=dev)].float().contiguous()
        T = ransac_registration(down[0][keys[0]], down[1][keys[1]], nn_search(f0, f1), ransac_n=3, max_corr_dist=r,
                                edge_similarity=0.9, max_iter=ransac_iter, seed=seed, device=dev)[0]
        timed("global", t0)

    t0 = time.time()
    if refine == "plane":
        normals = target_normals
        if normals is None:
            normals, _ = estimate_normals(down[1], knn=30, max_radius=4.0 * voxel_size, viewpoint=np.zeros(3), device=dev)
        timed("normals", t0)
        t0 = time.time()
        T, fitness, rmse, iters, n_corr = icp_point_to_plane(down[0], down[1], normals, r, init=T, device=dev)
    elif refine == "color":
        normals = target_normals
        if normals is None:
            normals, _ = estimate_normals(down[1], knn=30, max_radius=4.0 * voxel_size, viewpoint=np.zeros(3), device=dev)
        timed("normals", t0)
        t0 = time.time()
        if source_intensity is None:
            source_intensity = down_intensity(source, source_colors, down[0], voxel_size, dev)
        if target_color is None:
            target_color = target_color_terms(down[1], normals, down_intensity(target, target_colors, down[1], voxel_size,
                                                                                 dev), voxel_size, dev)
        timed("gradient", t0)
        t0 = time.time()
        T, fitness, rmse, iters, n_corr = icp_colored(down[0], source_intensity, down[1], normals, target_color["intensity"],
                                                      r, init=T, max_iteration=30, lambda_geometric=0.968,
                                                      dst_gradient=target_color["gradient"], device=dev)
    elif refine == "point":
        T, fitness, rmse, iters, n_corr = icp_point_to_point(down[0], down[1], r, init=T, max_iteration=30, device=dev)
    else:                                                 # the statistics of the unrefined pose: one correspondence stage
        T, fitness, rmse, iters, n_corr = icp_point_to_point(down[0], down[1], r, init=T, max_iteration=0, device=dev)
    timed("refine", t0)
    return dict(T=T, fitness=fitness, rmse=rmse, iterations=iters, n_corr=n_corr, times=times)


def register_pair(model, cfg, source, source_image, target, target_image, voxel_size=0.025, num_keypoints=5000,
                  ransac_iter=50000, seed=0, init=None, skip_global=False, refine="plane", device="cuda",
                  descriptor="imfnet", source_colors=None, target_colors=None):
    """source / target: float64 [n, 3] points; *_image: [1, C, H, W] arrays as generate_desc feeds them.  With
    descriptor="fpfh" model, cfg and the images are not used (None will do).  source_colors / target_colors: the points'
    uint8 [n, 3] colours, required by refine="color".  Returns dict(T 4x4 numpy source->target,
    fitness, rmse, iterations, n_corr, times)."""
    if refine not in REFINE_CHOICES:
        raise ValueError(f"refine must be one of {REFINE_CHOICES}, got {refine!r}")
    if descriptor not in DESCRIPTOR_CHOICES:
        raise ValueError(f"descriptor must be one of {DESCRIPTOR_CHOICES}, got {descriptor!r}")
    check_colors(refine, (("the source", source, source_colors), ("the target", target, target_colors)))
    dev = torch.device(device)
    times = {}
    t0 = time.time()
    down, feat = [], []
    for pts, img in ((source, source_image), (target, target_image)):
        xyz, F = fragment_features(model, cfg, pts, img, voxel_size=voxel_size, device=dev, descriptor=descriptor)
        down.append(xyz)
        feat.append(F)
    torch.cuda.synchronize(dev)
    times["features"] = time.time() - t0
    return register_features(source, target, down, feat, voxel_size=voxel_size, num_keypoints=num_keypoints,
                             ransac_iter=ransac_iter, seed=seed, init=init, skip_global=skip_global, refine=refine,
                             device=dev, times=times, source_colors=source_colors, target_colors=target_colors)


def make_parser():
    ap = argparse.ArgumentParser(prog="python -m imfnet_amd.register", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", required=True, help="source fragment (.ply)")
    ap.add_argument("--source_image", default=None, help="required with --descriptor imfnet; not read with fpfh")
    ap.add_argument("--target", required=True, help="target fragment (.ply)")
    ap.add_argument("--target_image", default=None, help="required with --descriptor imfnet; not read with fpfh")
    ap.add_argument("--descriptor", choices=DESCRIPTOR_CHOICES, default="imfnet",
                    help="imfnet: the network's descriptors; fpfh: hand-crafted, no checkpoint and no images")
    ap.add_argument("-m", "--model", default=None, help="checkpoint (.pth); default: seeded weights")
    ap.add_argument("--voxel_size", type=float, default=0.025)
    ap.add_argument("--num_keypoints", type=int, default=5000)
    ap.add_argument("--ransac_iter", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--init", default=None, help="4x4 text matrix the refinement starts from with --skip_global")
    ap.add_argument("--skip_global", action="store_true", help="no RANSAC: refine from --init (identity when absent)")
    ap.add_argument("--refine", choices=REFINE_CHOICES, default="plane")
    ap.add_argument("--out", default=None, help="write the 4x4 source->target matrix here")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None):
    ap = make_parser()
    args = ap.parse_args(argv)
    from .dataio import read_ply_colors, read_ply_points
    colors = [None, None]
    if args.refine == "color":
        for k, path in enumerate((args.source, args.target)):
            colors[k] = read_ply_colors(path)
            if colors[k] is None:
                ap.error(f"--refine color: {path} has no red, green, blue")
    if args.descriptor == "fpfh":
        model = cfg = src_image = dst_image = None
    else:
        if args.source_image is None or args.target_image is None:
            ap.error("--source_image and --target_image are required with --descriptor imfnet")
        model, cfg = load_network(args.model, torch.device(args.device))
        src_image, dst_image = load_image(args.source_image, cfg), load_image(args.target_image, cfg)
    init = np.loadtxt(args.init, dtype=np.float64).reshape(4, 4) if args.init else None
    res = register_pair(model, cfg, read_ply_points(args.source), src_image, read_ply_points(args.target), dst_image,
                        voxel_size=args.voxel_size, num_keypoints=args.num_keypoints, ransac_iter=args.ransac_iter,
                        seed=args.seed, init=init, skip_global=args.skip_global, refine=args.refine, device=args.device,
                        descriptor=args.descriptor, source_colors=colors[0], target_colors=colors[1])
    if args.out:
        np.savetxt(args.out, res["T"], fmt="%.17g")
    print(json.dumps(dict(fitness=res["fitness"], rmse=res["rmse"], iterations=res["iterations"], n_corr=res["n_corr"],
                          times={k: round(v, 6) for k, v in res["times"].items()}, T=res["T"].tolist())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
