#!/usr/bin/env python3
"""Descriptor Activation Mapping -- the reference's dam.py / pytorch_dam (base_dam.py:120-173, dam.py:15-21,
utils/image.py:111-162): for a chosen point, colour the fragment by how much each voxel's activation in `model.final`
supports that point's descriptor.

    python -m imfnet_amd.dam -m checkpoint.pth --ply files/cloud_bin_0.ply --image files/cloud_bin_0_0.png \
        --target 780 [--target ...] [--no_accumulate] --out 3D_head_map.ply

The reference takes 32 backward passes through the whole network per target and reads only final.kernel.grad.  `final` is a
1x1x1 convolution followed by a row-wise L2 normalisation, so that gradient is known in closed form:
here one forward under torch.no_grad(), a hook on `final`, and ONE call of imf_dam_heat (csrc/dam.hip) give the maps of
any number of targets.  Autograd is never used.

Kept: the accumulating .grad of the reference's loop (zero_grad() is called once, before it), because it produced the
published figures -- accumulate=False is what the loop would compute if it cleared the gradient at every step.
Changed: a constant heat map (max == min) gives an all-grey cloud with the black target; the reference divides by zero.
"""
import argparse
import os
import sys

import numpy as np
import torch

from . import _lib, ops
from ._lib import ImfError

GREY = 144                                   # round(0.5627450980392157 * 255), utils/image.py:139
# matplotlib's 256-entry `hsv` table as round(c * 255): 256 rows of R, G, B (tests compare it with matplotlib's own
# when that can be imported; nothing here imports it)
_HSV_HEX = (
    "ff0000ff0600ff0c00ff1200ff1800ff1e00ff2300ff2900ff2f00ff3500ff3b00ff4100ff4700ff4d00ff5300ff5900"
    "ff5f00ff6400ff6a00ff7000ff7600ff7c00ff8200ff8800ff8e00ff9400ff9a00ff9f00ffa500ffab00ffb100ffb700"
    "ffbd00ffc300ffc900ffcf00ffd500ffdb00ffe000ffe600ffec00fef100fcf500faf900f8fd00f4ff00eeff00e8ff00"
    "e2ff00ddff00d7ff00d1ff00cbff00c5ff00bfff00b9ff00b3ff00adff00a7ff00a2ff009cff0096ff0090ff008aff00"
    "84ff007eff0078ff0072ff006cff0066ff0061ff005bff0055ff004fff0049ff0043ff003dff0037ff0031ff002bff00"
    "25ff0020ff001aff0014ff000eff0008ff0006ff0404ff0802ff0c00ff1000ff1600ff1b00ff2100ff2700ff2d00ff33"
    "00ff3900ff3f00ff4500ff4b00ff5100ff5700ff5c00ff6200ff6800ff6e00ff7400ff7a00ff8000ff8600ff8c00ff92"
    "00ff9700ff9d00ffa300ffa900ffaf00ffb500ffbb00ffc100ffc700ffcd00ffd300ffd800ffde00ffe400ffea00fff0"
    "00fff600fffc00fcff00f6ff00f0ff00eaff00e5ff00dfff00d9ff00d3ff00cdff00c7ff00c1ff00bbff00b5ff00afff"
    "00aaff00a4ff009eff0098ff0092ff008cff0086ff0080ff007aff0074ff006eff0069ff0063ff005dff0057ff0051ff"
    "004bff0045ff003fff0039ff0033ff002dff0028ff0022ff001cff0016ff0010ff020cff0408ff0604ff0800ff0e00ff"
    "1300ff1900ff1f00ff2500ff2b00ff3100ff3700ff3d00ff4300ff4900ff4f00ff5400ff5a00ff6000ff6600ff6c00ff"
    "7200ff7800ff7e00ff8400ff8a00ff9000ff9500ff9b00ffa100ffa700ffad00ffb300ffb900ffbf00ffc500ffcb00ff"
    "d000ffd600ffdc00ffe200ffe800ffee00fff400fff800fdfa00f9fc00f5fe00f1ff00edff00e7ff00e1ff00dbff00d5"
    "ff00cfff00c9ff00c3ff00bdff00b7ff00b1ff00acff00a6ff00a0ff009aff0094ff008eff0088ff0082ff007cff0076"
    "ff0071ff006bff0065ff005fff0059ff0053ff004dff0047ff0041ff003bff0035ff0030ff002aff0024ff001eff0018")
HSV_TABLE = np.frombuffer(bytes.fromhex(_HSV_HEX), dtype=np.uint8).reshape(256, 3)


class DAM:
    """DAM(model)(stensor, image, targets) -> (heat [T, N] float32 on the device, flags [T] int32).  After a call,
    `descriptors` holds the model's output of that forward (the normalised [N, 32] rows), `minmax` the per-target
    (min, max) of the heat and `hidden` / `prenorm` what the hook on `final` saw."""

    def __init__(self, model, target_layer=None):
        final = getattr(model, "final", None)
        if final is None or (target_layer is not None and target_layer is not final):
            raise ImfError("DAM supports model.final as the target layer only (its closed form is that of a 1x1x1 "
                           "convolution followed by the L2 normalisation)")
        if final.kernel_volume != 1 or final.out_channels != 32:
            raise ImfError("DAM needs final to be a 1x1x1 convolution with 32 outputs")
        self.model, self.final = model, final
        self.descriptors = self.minmax = self.hidden = self.prenorm = None

    def dam(self, stensor, image, targets, accumulate=True):
        seen = {}

        def hook(module, inputs, output):
            assert not torch.is_grad_enabled(), "DAM runs without autograd"
            seen["h"], seen["o"] = inputs[0].F, output.F

        was_training = self.model.training
        self.model.eval()
        handle = self.final.register_forward_hook(hook)
        try:
            with torch.no_grad():
                out = self.model.forward_layers(stensor, image)
        finally:
            handle.remove()
            if was_training:
                self.model.train()
        h, o = seen["h"].contiguous(), seen["o"].contiguous()
        t = torch.as_tensor(np.asarray(targets, dtype=np.int64).reshape(-1) if not torch.is_tensor(targets) else targets)
        t = t.reshape(-1).to(device=o.device, dtype=torch.int32).contiguous()
        heat, minmax, flags, _ = ops.dam_heat(o, h, t, accumulate=accumulate)
        self.descriptors, self.minmax, self.hidden, self.prenorm = out.F, minmax, h, o
        return heat, flags

    __call__ = dam


def dam_colors(heat_row, target):
    """The colouring, utils/image.py:111-144, on the host: v = 0.1 + 0.9 (heat - min) / (max - min); rows at the minimum are
    grey, every other row gets hsv[int(v * 256) clipped to 255], the target row is black; stored as round(c * 255).
    A constant heat map gives all grey.  Returns uint8 [N, 3]."""
    heat = np.asarray(heat_row.detach().cpu() if torch.is_tensor(heat_row) else heat_row, dtype=np.float64).reshape(-1)
    n = heat.shape[0]
    if not 0 <= int(target) < n:
        raise ImfError(f"target {target} is outside the {n} rows")
    rgb = np.full((n, 3), GREY, dtype=np.uint8)
    lo, hi = float(heat.min()), float(heat.max())
    if hi > lo:
        v = 0.1 + (0.9 / (hi - lo)) * (heat - lo)
        idx = np.minimum((v * 256.0).astype(np.int64), 255)
        coloured = heat != lo
        rgb[coloured] = HSV_TABLE[idx[coloured]]
    rgb[int(target)] = 0
    return rgb


def write_head_map(path, xyz, rgb):
    """The coloured cloud as Open3D writes it (binary little-endian, double x, y, z + uchar red, green, blue)."""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64))
    rgb = np.ascontiguousarray(np.asarray(rgb, dtype=np.uint8))
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
        raise ImfError(f"write_head_map: xyz {xyz.shape} and rgb {rgb.shape} must both be [N, 3]")
    rc = _lib.lib().imf_ply_write_points_rgb(os.fsencode(path), xyz.ctypes.data, rgb.ctypes.data, len(xyz))
    _lib.check(rc, f"imf_ply_write_points_rgb({path})")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("-m", "--model", default=None, type=str, help="checkpoint.pth; without it: RANDOM weights (smoke use only)")
    p.add_argument("--ply", required=True, type=str, help="the fragment, e.g. files/cloud_bin_0.ply")
    p.add_argument("--image", required=True, type=str, help="its image, e.g. files/cloud_bin_0_0.png")
    p.add_argument("--target", action="append", type=int, default=None, help="target row of the voxelised cloud (repeatable; default 780)")
    p.add_argument("--no_accumulate", action="store_true", help="clear the gradient at every step instead of accumulating it")
    p.add_argument("--out", default="3D_head_map.ply", type=str)
    p.add_argument("--seed", type=int, default=0, help="seed of the random weights when no checkpoint is given")
    args = p.parse_args(argv)
    if not args.target:
        args.target = [780]
    return args


def output_paths(out, targets):
    """One file for one target; `<out stem>_<target>.ply` per target for several."""
    if len(targets) == 1:
        return [out]
    stem, ext = os.path.splitext(out)
    return [f"{stem}_{t}{ext or '.ply'}" for t in targets]


def main(argv=None):
    args = parse_args(argv)
    from .checkpoint import Config, load_checkpoint
    from .dataio import image_to_nchw, process_image, read_image, read_ply_points
    from .extract import sparse_tensor_from_points
    from .model import load_model
    device = torch.device("cuda", torch.cuda.current_device())
    if args.model is not None:
        state_dict, config = load_checkpoint(args.model)
    else:
        print(f"no checkpoint given: RANDOM weights from seed {args.seed} -- the map shows the plumbing, not the network")
        state_dict, config = None, Config()
        torch.manual_seed(args.seed)
    model = load_model(config.model)(1, config.model_n_out, bn_momentum=0.05, normalize_feature=config.normalize_feature,
                                     conv1_kernel_size=config.conv1_kernel_size, D=3, config=config)
    if state_dict is not None:
        model.load_state_dict(state_dict)
    model = model.eval().to(device)
    xyz = read_ply_points(args.ply)
    img = read_image(args.image)
    if img.shape[0] != config.image_H or img.shape[1] != config.image_W:
        img = process_image(image=img, aim_H=config.image_H, aim_W=config.image_W)
    image = torch.as_tensor(image_to_nchw(img)).to(device)
    with torch.no_grad():
        st, inds = sparse_tensor_from_points(xyz, config.voxel_size, device)
    xyz_down = np.asarray(xyz)[inds.cpu().numpy()].astype(np.float64)
    print(f"Point cloud : {args.ply}\nImage : {args.image}\nTarget Point Index: {args.target}")
    heat, flags = DAM(model)(st, image, args.target, accumulate=not args.no_accumulate)
    heat, flags = heat.cpu().numpy(), flags.cpu().numpy()
    for t, path, row, bad in zip(args.target, output_paths(args.out, args.target), heat, flags):
        if bad:
            raise ImfError(f"target {t}: outside the {len(xyz_down)} rows, or its pre-normalisation row is zero or not finite")
        write_head_map(path, xyz_down, dam_colors(row, t))
        print(f"Saving : {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
