#!/usr/bin/env python3
"""FPFH descriptors over a 3DMatch-layout tree: the tree `imfnet_amd.generate_desc` writes, without a network or images.

    python -m imfnet_amd.fpfh_desc --source <3DMatch_test> --target <desc_dir> [--voxel_size 0.025]

    <source>/<scene>/seq-01/cloud_bin_K.ply
 -> <target>/<scene>/seq-01/cloud_bin_K.npz  {points f64[N,3], xyz f64[M,3], feature f32[M,64]}

`xyz` holds the voxel representatives `extract_features` returns for that voxel size; `feature` is `compute_fpfh` on them
as `imfnet_amd.register --descriptor fpfh` computes it (radius 5 voxel, max_nn 64, normals at 2 voxel facing the origin),
33 bins zero-padded to the 64 columns `nn_search` takes.  `python -m imfnet_amd.evaluate --desc_root <desc_dir> ...` runs
on the result unchanged: the FPFH baseline row.
"""
import argparse
import os
import sys
import time

import torch

from .dataio import read_ply_points, save_descriptors
from .files import ensure_dir


def make_parser():
    ap = argparse.ArgumentParser(prog="python -m imfnet_amd.fpfh_desc", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", required=True, help="the 3DMatch test tree: <scene>/seq-01/*.ply")
    ap.add_argument("--target", required=True, help="where the descriptor tree is written")
    ap.add_argument("--voxel_size", type=float, default=0.025)
    ap.add_argument("--device", default="cuda")
    return ap


def describe_tree(source, target, voxel_size=0.025, device="cuda"):
    """Writes one .npz per fragment; returns the list of the files written."""
    from .extract import voxel_representatives
    from .generate_desc import list_fragments
    from .register import fpfh_descriptors
    written = []
    for scene, ply in list_fragments(source):
        points = read_ply_points(ply)
        xyz = voxel_representatives(points, voxel_size, device)
        feature = fpfh_descriptors(xyz, voxel_size, device)
        out_dir = os.path.join(target, os.path.basename(scene), "seq-01")
        ensure_dir(out_dir)
        written.append(os.path.join(out_dir, os.path.basename(ply).replace(".ply", ".npz")))
        save_descriptors(written[-1], points, xyz, feature)
    return written


def main(argv=None):
    args = make_parser().parse_args(argv)
    ensure_dir(args.target)
    t0 = time.time()
    written = describe_tree(args.source, args.target, args.voxel_size, args.device)
    torch.cuda.synchronize()
    print(f"{len(written)} fragments in {time.time() - t0:.2f} s -> {args.target}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
