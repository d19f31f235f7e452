"""NumPy restatement of the fragment fusion (csrc/tsdf.hip: allocate / integrate / extract), written from the loop in
that file's header: dense over the opened units, fp64 geometry, float32 tsdf and weight, the same operation order and
the same output order (units ascending in (z, y, x); points by unit, voxel (z * 16 + y) * 16 + x, axis).

`fused=True` evaluates the projection's multiply-adds in extended precision and rounds once, the way a fused
multiply-add would: the check that contraction could move only a negligible share of the points of a scene."""
import math

import numpy as np

RES = 16
DEFAULTS = dict(voxel_length=3.0 / 512, sdf_trunc=0.04, depth_scale=1000.0, depth_trunc=6.0, lattice_offset=0.5)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _depth_m(raw, p):
    """raw / depth_scale in float32 (as the depth image is converted), widened."""
    return (raw.astype(np.float32) / np.float32(p["depth_scale"])).astype(np.float64)


def _affine(M, x, y, z, row, fused):
    a, b, c, d = (M[row, k] for k in range(4))
    if fused:
        L = np.longdouble
        return np.asarray(L(a) * x.astype(L) + L(b) * y.astype(L) + L(c) * z.astype(L) + L(d), dtype=np.float64)
    return a * x + b * y + c * z + d


def allocate(depth, cam2world, K, p, stride=4):
    """Unit coordinates int32 [n, 3] = (x, y, z), ascending in (z, y, x)."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ul = float(RES) * p["voxel_length"]
    reach = int(math.ceil(p["sdf_trunc"] / ul))
    F, H, W = depth.shape
    v, u = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    found = set()
    for f in range(F):
        raw = depth[f][v, u]
        d = _depth_m(raw, p)
        ok = (raw != 0) & ~(d > p["depth_trunc"])
        d, uu, vv = d[ok], u[ok].astype(np.float64), v[ok].astype(np.float64)
        xc, yc = (uu - cx) * d / fx, (vv - cy) * d / fy
        M = cam2world[f]
        q = np.stack([np.floor((M[r, 0] * xc + M[r, 1] * yc + M[r, 2] * d + M[r, 3]) / ul) for r in range(3)], 1)
        q = np.unique(q[np.isfinite(q).all(1)].astype(np.int64), axis=0)
        for dz in range(-reach, reach + 1):
            for dy in range(-reach, reach + 1):
                for dx in range(-reach, reach + 1):
                    found.update(map(tuple, q + np.array([dx, dy, dz])))
    if not found:
        return np.zeros((0, 3), np.int32)
    units = np.array(sorted(found, key=lambda c: (c[2], c[1], c[0])), dtype=np.int32)
    return units


def _positions(units, p):
    """Sample positions of all voxels: three arrays broadcastable to [n, 16(z), 16(y), 16(x)]."""
    l = np.arange(RES)
    off, vl = p["lattice_offset"], p["voxel_length"]
    px = ((RES * units[:, 0].astype(np.int64)[:, None] + l).astype(np.float64) + off) * vl
    py = ((RES * units[:, 1].astype(np.int64)[:, None] + l).astype(np.float64) + off) * vl
    pz = ((RES * units[:, 2].astype(np.int64)[:, None] + l).astype(np.float64) + off) * vl
    return px[:, None, None, :], py[:, None, :, None], pz[:, :, None, None]


CULL_CONDITIONS = ("front", "left", "right", "top", "bottom", "near")


def cull_conditions(units, M, K, p, height, width):
    """Per voxel, the outcome of each single condition that the kernel's frustum cull tests on a unit's bounding sphere,
    for one frame with world2cam M: bool [n, 16, 16, 16] under the names of CULL_CONDITIONS =
    z > 0, uf >= 0, uf < width, vf >= 0, vf < height, z <= depth_trunc + sdf_trunc.  The four image sides are the rule's
    own expressions, so they mean something only where z > 0."""
    units = np.asarray(units)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    shape = (len(units), RES, RES, RES)
    px, py, pz = (np.broadcast_to(a, shape) for a in _positions(units, p))
    with np.errstate(all="ignore"):
        z = _affine(M, px, py, pz, 2, False)
        x, y = _affine(M, px, py, pz, 0, False), _affine(M, px, py, pz, 1, False)
        uf, vf = fx * x / z + cx + 0.5, fy * y / z + cy + 0.5
        return dict(front=z > 0.0, left=uf >= 0.0, right=uf < float(width), top=vf >= 0.0, bottom=vf < float(height),
                    near=z <= p["depth_trunc"] + p["sdf_trunc"])


def integrate(units, depth, world2cam, K, p, state=None, fused=False, trace=None):
    """(tsdf, weight) float32 [n, 16, 16, 16] (z, y, x) after the frames in order; `state` continues an earlier call.
    `trace`: a list that gets, per frame, the number of voxels the frame updates in every unit (int64 [n])."""
    n = len(units)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    F, H, W = depth.shape
    shape = (n, RES, RES, RES)
    tsdf, w = (np.zeros(shape, np.float32), np.zeros(shape, np.float32)) if state is None else (state[0].copy(), state[1].copy())
    if n == 0:
        return tsdf, w
    px, py, pz = (np.broadcast_to(a, shape) for a in _positions(units, p))
    with np.errstate(all="ignore"):
        for f in range(F):
            M = world2cam[f]
            z = _affine(M, px, py, pz, 2, fused)
            ok = z > 0.0
            x, y = _affine(M, px, py, pz, 0, fused), _affine(M, px, py, pz, 1, fused)
            uf, vf = fx * x / z + cx + 0.5, fy * y / z + cy + 0.5
            ok &= (uf >= 0.0) & (uf < float(W)) & (vf >= 0.0) & (vf < float(H))
            iu, iv = np.where(ok, uf, 0.0).astype(np.int64), np.where(ok, vf, 0.0).astype(np.int64)
            raw = depth[f][iv, iu]
            ok &= raw != 0
            d = _depth_m(raw, p)
            ok &= ~(d > p["depth_trunc"])
            a, b = (iu.astype(np.float64) - cx) / fx, (iv.astype(np.float64) - cy) / fy
            sdf = (d - z) * np.sqrt(a * a + b * b + 1.0)
            ok &= ~(sdf <= -p["sdf_trunc"])
            new = np.minimum(1.0, sdf / p["sdf_trunc"]).astype(np.float32)
            avg = (tsdf * w + new) / (w + np.float32(1.0))
            tsdf = np.where(ok, avg, tsdf).astype(np.float32)
            w = np.where(ok, w + np.float32(1.0), w).astype(np.float32)
            if trace is not None:
                trace.append(ok.reshape(n, -1).sum(1))
    return tsdf, w


def extract(units, tsdf, w, p):
    """points float64 [m, 3] and keys int64 [m, 4] = (global voxel x, y, z, axis), in the defined output order."""
    n = len(units)
    if n == 0:
        return np.zeros((0, 3)), np.zeros((0, 4), np.int64)
    row = {tuple(c): i for i, c in enumerate(units.tolist())}
    side = (w != 0) & (tsdf < np.float32(0.98)) & (tsdf != 0)
    f1 = np.zeros((3,) + tsdf.shape, np.float32)           # the +x, +y, +z neighbour's tsdf
    s1 = np.zeros((3,) + tsdf.shape, bool)
    f1[0][..., :-1], s1[0][..., :-1] = tsdf[..., 1:], side[..., 1:]
    f1[1][:, :, :-1, :], s1[1][:, :, :-1, :] = tsdf[:, :, 1:, :], side[:, :, 1:, :]
    f1[2][:, :-1], s1[2][:, :-1] = tsdf[:, 1:], side[:, 1:]
    for i, (ux, uy, uz) in enumerate(units.tolist()):
        j = row.get((ux + 1, uy, uz))
        if j is not None:
            f1[0][i, :, :, -1], s1[0][i, :, :, -1] = tsdf[j, :, :, 0], side[j, :, :, 0]
        j = row.get((ux, uy + 1, uz))
        if j is not None:
            f1[1][i, :, -1, :], s1[1][i, :, -1, :] = tsdf[j, :, 0, :], side[j, :, 0, :]
        j = row.get((ux, uy, uz + 1))
        if j is not None:
            f1[2][i, -1], s1[2][i, -1] = tsdf[j, 0], side[j, 0]
    cross = np.stack([side & s1[a] & (tsdf * f1[a] < 0) for a in range(3)], -1)     # [n, z, y, x, axis]
    iu, lz, ly, lx, ax = np.nonzero(cross)                  # C order = unit, z, y, x, axis
    k = np.stack([RES * units[iu, 0].astype(np.int64) + lx, RES * units[iu, 1].astype(np.int64) + ly,
                  RES * units[iu, 2].astype(np.int64) + lz], 1)
    pts = (k.astype(np.float64) + p["lattice_offset"]) * p["voxel_length"]
    r0 = np.abs(tsdf[iu, lz, ly, lx].astype(np.float64))
    r1 = np.abs(f1[ax, iu, lz, ly, lx].astype(np.float64))
    m = np.arange(len(ax))
    pts[m, ax] = pts[m, ax] + p["voxel_length"] * (r0 / (r0 + r1))
    return pts, np.concatenate([k, ax[:, None].astype(np.int64)], 1)


def fuse(depth, poses_cam2world, K, fused=False, **kw):
    """The three steps on one fragment: (points, keys, units)."""
    p = params(**kw)
    c2w = np.asarray(poses_cam2world, np.float64)
    units = allocate(depth, c2w, K, p)
    tsdf, w = integrate(units, depth, np.linalg.inv(c2w), K, p, fused=fused)
    pts, keys = extract(units, tsdf, w, p)
    return pts, keys, units


def point_keys(points, voxel_length, lattice_offset):
    """(global voxel x, y, z, axis) of extracted points from their coordinates alone: two coordinates lie on the sample
    lattice, the third lies strictly inside the edge that starts at the voxel."""
    g = np.asarray(points, np.float64) / voxel_length - lattice_offset
    dist = np.abs(g - np.round(g))
    ax = np.argmax(dist, 1)
    k = np.round(g).astype(np.int64)
    m = np.arange(len(g))
    k[m, ax] = np.floor(g[m, ax]).astype(np.int64)
    return np.concatenate([k, ax[:, None].astype(np.int64)], 1)


def lattice_census(points, voxel_length, lattice_offset=0.0, tol=2e-3):
    """Per point, how many of its three coordinates lie on the sample lattice (within tol voxels)."""
    g = np.asarray(points, np.float64) / voxel_length - lattice_offset
    return (np.abs(g - np.round(g)) < tol).sum(1)
