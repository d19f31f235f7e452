"""NumPy restatement of the colour rule of the TSDF volume (the head of csrc/tsdf.hip), on top of tsdf_restate.py and
tsdf_mesh_restate.py, which it does not edit:

  integrate   whenever a frame updates a voxel's tsdf (every skip of tsdf_restate.integrate has passed), with the same
              pixel (u, v) and the weight w BEFORE the increment, per channel k in float32 on the 0..255 scale:
                  c[k] = (c[k] * w + (float32)rgb[v][u][k]) / (w + 1)
  point / vertex between the samples lo and hi:  t = |f_lo| / (|f_lo| + |f_hi|) in fp64 (the t of the position),
              c = c_lo + t * (c_hi - c_lo) in fp64, uint8 = floor(c + 0.5) clamped to [0, 255].

The pixel choice is not restated a second time: `integrate_rgb` runs tsdf_restate.integrate itself, one frame at a time,
on a depth image that remembers which pixel every voxel read, so (tsdf, w) ARE tsdf_restate's and the colour is read at
literally the pixel the depth was read at.  The colour state is float32 [n, 16, 16, 16, 3] (z, y, x, channel), which is
TSDFVolume.colors() reshaped."""
import numpy as np

import tsdf_mesh_restate as M
import tsdf_restate as R

RES = R.RES


class _RememberingDepth:
    """One depth frame as tsdf_restate.integrate indexes it (`depth[f][iv, iu]`); keeps the (iv, iu) it was asked for."""

    def __init__(self, frame):
        self.frame = frame
        self.shape = (1,) + frame.shape
        self.pixel = None

    def __getitem__(self, key):
        if isinstance(key, tuple):
            self.pixel = key
            return self.frame[key]
        assert key == 0
        return self


def integrate_rgb(units, depth, color, world2cam, K, p, state=None, fused=False, trace=None):
    """(tsdf, w, colour) after the frames in order; `state` = (tsdf, w, colour) continues an earlier call; `trace` as in
    tsdf_restate.integrate (per frame, the number of voxels updated in every unit)."""
    n = len(units)
    shape = (n, RES, RES, RES)
    if state is None:
        tsdf, w, col = np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.zeros(shape + (3,), np.float32)
    else:
        tsdf, w, col = (np.array(a, np.float32) for a in state)
    if n == 0:
        return tsdf, w, col
    one = np.float32(1.0)
    for f in range(depth.shape[0]):
        seen = _RememberingDepth(depth[f])
        new_tsdf, new_w = R.integrate(units, seen, world2cam[f:f + 1], K, p, state=(tsdf, w), fused=fused, trace=trace)
        updated = new_w != w                                  # the weight moves exactly when the tsdf is updated
        iv, iu = seen.pixel
        rgb = color[f][iv, iu].astype(np.float32)             # [n, 16, 16, 16, 3]; junk where not updated, not used
        mean = ((col * w[..., None] + rgb) / (w + one)[..., None]).astype(np.float32)
        col = np.where(updated[..., None], mean, col).astype(np.float32)
        tsdf, w = new_tsdf, new_w
    return tsdf, w, col


def _unit_code(c):
    c = np.asarray(c, np.int64) + (1 << 20)
    return (c[..., 2] << 42) | (c[..., 1] << 21) | c[..., 0]


def _sample(units, values, g):
    """values [n, 16, 16, 16, ...] at the global voxel coordinates g int64 [m, 3] = (x, y, z); every unit must exist."""
    code = _unit_code(units)
    order = np.argsort(code)
    want = _unit_code(g >> 4)
    at = np.searchsorted(code[order], want)
    assert (at < len(code)).all() and (code[order][at] == want).all()
    l = g & 15
    return values[order[at], l[:, 2], l[:, 1], l[:, 0]]


def to_uint8(c):
    """floor(c + 0.5) clamped to [0, 255]; a NaN gives 0."""
    q = np.floor(np.asarray(c, np.float64) + 0.5)
    with np.errstate(invalid="ignore"):
        return np.where(~(q >= 0.0), 0.0, np.where(q > 255.0, 255.0, q)).astype(np.uint8)


def edge_colors(units, tsdf, col, g_lo, g_hi):
    """uint8 [m, 3] of the surface points on the edges g_lo -> g_hi (global voxel coordinates, int64 [m, 3])."""
    if len(g_lo) == 0:
        return np.zeros((0, 3), np.uint8)
    f_lo = np.abs(_sample(units, tsdf, g_lo).astype(np.float64))
    f_hi = np.abs(_sample(units, tsdf, g_hi).astype(np.float64))
    t = f_lo / (f_lo + f_hi)
    c_lo, c_hi = _sample(units, col, g_lo).astype(np.float64), _sample(units, col, g_hi).astype(np.float64)
    return to_uint8(c_lo + t[:, None] * (c_hi - c_lo))


def extract_rgb(units, tsdf, w, col, p):
    """tsdf_restate.extract's (points, keys) and the colour of every point, uint8 [m, 3]."""
    pts, keys = R.extract(units, tsdf, w, p)
    g_lo = keys[:, :3]
    g_hi = g_lo.copy()
    g_hi[np.arange(len(keys)), keys[:, 3]] += 1
    return pts, keys, edge_colors(np.asarray(units), tsdf, col, g_lo, g_hi)


def mesh_rgb(units, tsdf, w, col, voxel_length, lattice_offset):
    """tsdf_mesh_restate.mesh's dict with `rgb` uint8 [V, 3], the vertex colours in its vertex order."""
    units = np.asarray(units)
    m = M.mesh(units, tsdf, w, voxel_length, lattice_offset)
    keys = m["keys"]
    slot, rest = keys % 7, keys // 7
    vox, owner = rest % RES ** 3, rest // RES ** 3
    local = np.stack([vox % RES, (vox // RES) % RES, vox // (RES * RES)], 1)
    d = np.array(M.DIRS, np.int64)[slot]
    if len(keys) == 0:
        m["rgb"] = np.zeros((0, 3), np.uint8)
        return m
    g_lo = RES * units[owner].astype(np.int64) + local
    g_hi = g_lo + np.stack([d & 1, (d >> 1) & 1, (d >> 2) & 1], 1)
    m["rgb"] = edge_colors(units, np.asarray(tsdf, np.float32).reshape(len(units), RES, RES, RES),
                           np.asarray(col, np.float32).reshape(len(units), RES, RES, RES, 3), g_lo, g_hi)
    return m
