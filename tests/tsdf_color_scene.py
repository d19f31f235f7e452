"""Colour for the synthetic RGB-D sequence of tsdf_scene.py: a smooth texture painted on the WORLD, so that the colour a
pixel sees depends only on the surface point it hits.  Every channel has its own direction, spatial rate and phase:

    texture(p)[k] = 127.5 + 100 sin(RATE[k] (DIR[k] . p) + PHASE[k])          27.5 .. 227.5, never clamped

A channel swap, an x / y transposition, a wrong frame or a wrong pixel therefore shows up as an error of tens of levels,
not as noise.  `render_color` evaluates it at the hit point of every pixel centre's ray (tsdf_scene.render_depth's ray and
depth) and rounds to uint8."""
import numpy as np

import tsdf_scene as S

DIR = np.array([[0.8, 0.36, 0.48], [-0.28, 0.96, 0.0], [0.6, 0.0, -0.8]])      # unit vectors, one per channel
RATE = np.array([3.1, 4.3, 2.3])                                                # radians per metre
PHASE = np.array([0.3, 1.7, 4.1])


def texture(points):
    """float64 [n, 3] = (R, G, B) on the 0..255 scale at world points [n, 3] (any leading shape)."""
    p = np.asarray(points, np.float64)
    return 127.5 + 100.0 * np.sin(RATE * (p @ DIR.T) + PHASE)


def render_color(T, K, width, height):
    """uint8 [H, W, 3]: the texture at the world point each pixel centre's ray hits (black where it hits nothing)."""
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    t = S.render_depth(T, K, width, height)
    d_cam = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    hit = np.isfinite(t)
    p = (d_cam * np.where(hit, t, 0.0)[..., None]) @ T[:3, :3].T + T[:3, 3]
    return np.where(hit[..., None], np.rint(texture(p)), 0.0).astype(np.uint8)


def make_colors(seq):
    """uint8 [F, H, W, 3] for a sequence of tsdf_scene.make_sequence."""
    F, H, W = seq["depth"].shape
    return np.stack([render_color(seq["poses"][f], seq["K"], W, H) for f in range(F)])


def write_color_files(sdir, colors, quality=95):
    """Replaces frame-XXXXXX.color.jpg of a tree of tsdf_scene.write_tree with these frames (4:2:0 baseline JPEG)."""
    import os

    from PIL import Image
    for f, rgb in enumerate(colors):
        Image.fromarray(rgb).save(os.path.join(sdir, "frame-%06d.color.jpg" % f), quality=quality)
