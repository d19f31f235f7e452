"""One hardest-contrastive training step, run twice from the same seed, and the comparison of the two gradients bit for
bit: what tools/train_repro.py measures and tests/test_gpu_train_repro.py gates.

A run is a fresh data set and a fresh trainer over a two-fragment scene tree (`write_tree`), so the initialisation, the
augmentation and the loss samples are the same; the six kernel switches (`SWITCHES`) are all set to one choice."""
import os

import numpy as np
import torch

SWITCHES = ("norm_kernels", "loss_kernels", "fusion_kernels", "image_kernels", "optim_kernels", "head_kernels")


def write_tree(root, clouds, images):
    """A 3DMatch-style tree of one scene with two fragments (clouds[k] [n, 3], images[k] [H, W, 3] in 0 .. 1) and its
    overlap list under `root`."""
    from PIL import Image
    seq = os.path.join(root, "sceneA", "seq-01")
    os.makedirs(seq)
    for k in (0, 1):
        pts = np.ascontiguousarray(clouds[k], dtype="<f4")
        with open(os.path.join(seq, f"cloud_bin_{k}.ply"), "wb") as f:
            f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n"
                    b"property float y\nproperty float z\nend_header\n" % len(pts))
            f.write(pts.tobytes())
        Image.fromarray((images[k] * 255).round().astype(np.uint8)).save(os.path.join(seq, f"cloud_bin_{k}_0.png"))
    os.makedirs(os.path.join(root, "overlap"))
    a, b = "sceneA/seq-01/cloud_bin_0.ply", "sceneA/seq-01/cloud_bin_1.ply"
    with open(os.path.join(root, "overlap", "sceneA@seq-01-0.30.txt"), "w") as f:
        f.write(f"{a} {b} 0.3\n{b} {a} 0.3\n")


def one_step(root, batch, choice, tag, extra_args=()):
    """(loss triple, {parameter name: gradient or None}) of one training step over the tree at `root` with every switch
    at `choice`; `tag` names the run's output directory below `root`."""
    from .data import IndoorPairDataset
    from .trainer import HardestContrastiveTrainer, parse_config
    args = ["--threed_match_dir", root, "--overlap_path", os.path.join(root, "overlap"), "--batch_size", str(batch),
            "--out_dir", os.path.join(root, "out_" + tag)]
    for s in SWITCHES:
        args += ["--" + s, choice]
    cfg = parse_config(args + list(extra_args))
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


def compare(root, batch, choice, extra_args=()):
    """Two runs of `one_step`: how many parameters' gradients agree bit for bit (a parameter without a gradient in both
    runs agrees and is counted under `no_gradient`), per parameter group, which differ and by how much, and whether the
    logged losses agree."""
    (la, a), (lb, b) = (one_step(root, batch, choice, choice + "_a", extra_args),
                        one_step(root, batch, choice, choice + "_b", extra_args))
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
