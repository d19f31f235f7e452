"""Does one training step give the same gradient bits twice?  The measurement; tests/test_gpu_train_repro.py is the gate
(both run imfnet_amd/train/repro.py).

One hardest-contrastive training step (imfnet_amd/train) on the in-tree fixture pair, run twice in one process from the same
seed -- a fresh data set and a fresh trainer each time, so the initialisation, the augmentation and the loss samples are the
same -- with the six kernel switches (--norm_kernels, --loss_kernels, --fusion_kernels, --image_kernels, --optim_kernels,
--head_kernels) all at `hip`, and for contrast all at `torch`.  For every parameter: whether the two gradients agree bit for bit (a parameter without a
gradient in both runs counts as agreeing and is listed under `no_gradient`).

Usage: python tools/train_repro.py [--batch 2] [--out FILE.json]
Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imfnet_amd.train.repro import compare, write_tree        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))
    im = np.load(os.path.join(ROOT, "tests", "golden", "fixture_images.npz"))
    clouds = {0: z["cloud_bin_0"].astype(np.float64), 1: z["cloud_bin_1"].astype(np.float64)}
    images = {0: im["image_0"], 1: im["image_1"]}
    res = dict(batch=a.batch, device=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, clouds, images)
        for choice in ("hip", "torch"):
            res["all_" + choice] = compare(root, a.batch, choice)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
