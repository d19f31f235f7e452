"""Does one training step give the same gradient bits twice?  A measurement, not a gate.

One hardest-contrastive training step (imfnet_amd/train) on the in-tree fixture pair, run twice in one process from the same
seed -- a fresh data set and a fresh trainer each time, so the initialisation, the augmentation and the loss samples are the
same -- with the five kernel switches (--norm_kernels, --loss_kernels, --fusion_kernels, --image_kernels, --optim_kernels)
all at `hip`, and for contrast all at `torch`.  For every parameter: whether the two gradients agree bit for bit (a parameter without a
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from train_time import write_tree                              # noqa: E402
from imfnet_amd.train.data import IndoorPairDataset          # noqa: E402
from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config   # noqa: E402

SWITCHES = ("norm_kernels", "loss_kernels", "fusion_kernels", "image_kernels", "optim_kernels")


def one_step(root, batch, choice, tag):
    args = ["--threed_match_dir", root, "--overlap_path", os.path.join(root, "overlap"), "--batch_size", str(batch),
            "--out_dir", os.path.join(root, "out_" + tag)]
    for s in SWITCHES:
        args += ["--" + s, choice]
    cfg = parse_config(args)
    ds = IndoorPairDataset("train", ["sceneA"], cfg, seed=0)
    tr = HardestContrastiveTrainer(cfg, ds, None)
    raws = [ds.load(k % len(ds)) for k in range(batch)]
    loss = tr.train_step([raws])
    torch.cuda.synchronize()
    tr.pool.shutdown()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in tr.model.named_parameters()}
    return loss, grads


def group_of(name):
    if name.startswith("img_encoder."):
        return "img_encoder"
    if name.startswith("attention_fusion."):
        return "attention_fusion"
    return "sparse network"


def compare(root, batch, choice):
    (la, a), (lb, b) = one_step(root, batch, choice, choice + "_a"), one_step(root, batch, choice, choice + "_b")
    differing, no_grad, groups = [], [], {}
    for k in a:
        g = groups.setdefault(group_of(k), dict(parameters=0, agree=0))
        g["parameters"] += 1
        if a[k] is None and b[k] is None:
            no_grad.append(k)
            same = True
        elif a[k] is None or b[k] is None:                     # a gradient in one run only: a failure of its own kind
            same = False
            differing.append(dict(name=k, one_sided=True, max_abs_diff=None,
                                  max_abs=float((a[k] if b[k] is None else b[k]).abs().max())))
        else:
            same = torch.equal(a[k], b[k])
            if not same:
                differing.append(dict(name=k, one_sided=False, max_abs_diff=float((a[k] - b[k]).abs().max()),
                                      max_abs=float(a[k].abs().max())))
        g["agree"] += int(same)
    return dict(parameters=len(a), agree=len(a) - len(differing), loss_a=list(la), loss_b=list(lb),
                loss_bits_agree=bool(np.array_equal(np.array(la), np.array(lb))), groups=groups, differing=differing,
                no_gradient=len(no_grad))


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
