"""Frame-to-frame RGB-D odometry on the device (csrc/odometry.hip, whose head states the rules):
Open3D's compute_rgbd_odometry with the hybrid term, restated.  `prepare_frame` builds a frame's pyramids once,
`rgbd_odometry` fits one prepared frame onto another, `track` chains a sequence into camera poses relative to its first
frame -- what fuse_fragments --poses odometry uses in place of the data set's .pose.txt files.  There is no CPU path."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ImfError, check

ITERATIONS = (20, 10, 5)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class RGBDFrame:
    """The prepared pyramids of one frame: an opaque device block (imf_rgbd_prepare) and the shape it was made for."""

    def __init__(self, block, height, width, levels, intrinsic):
        self.block, self.height, self.width, self.levels, self.intrinsic = block, height, width, levels, intrinsic

    @property
    def device(self):
        return self.block.device

    def level_shape(self, level):
        return self.height >> level, self.width >> level

    def images(self, level):
        """dict(Is, D, Isx, Isy, Dx, Dy) of float64 numpy [H_l, W_l] and the level's fx, fy, cx, cy (for the tests; the
        layout is csrc/odometry.hip's: a 256-byte header, then six planes per level, each rounded up to 256 bytes)."""
        plane = lambda l: ((self.height >> l) * (self.width >> l) * 8 + 255) // 256 * 256
        off = 256 + sum(6 * plane(l) for l in range(level))
        h, w = self.level_shape(level)
        raw = self.block.cpu().numpy()
        out = {}
        for k, name in enumerate(("Is", "D", "Isx", "Isy", "Dx", "Dy")):
            a = off + k * plane(level)
            out[name] = raw[a:a + h * w * 8].view(np.float64).reshape(h, w).copy()
        K = raw[24 + 32 * level:24 + 32 * level + 32].view(np.float64)
        out.update(fx=float(K[0]), fy=float(K[1]), cx=float(K[2]), cy=float(K[3]))
        return out


def prepare_frame(depth_u16, color_u8, intrinsic, levels=3, depth_scale=1000.0, depth_min=0.0, depth_max=4.0,
                  depth_edge=0.06, device="cuda"):
    """depth uint16 [H, W] and colour uint8 [H, W, 3] (arrays or tensors) with the 3 x 3 intrinsic -> RGBDFrame."""
    if not isinstance(depth_u16, torch.Tensor):
        a = np.ascontiguousarray(depth_u16)
        if a.dtype != np.uint16:
            raise ImfError(f"prepare_frame: depth must be uint16, got {a.dtype}")
        depth_u16 = torch.from_numpy(a.view(np.int16))       # the same bits, as imfnet_amd.fuse carries depth
    d = depth_u16 if depth_u16.dtype == torch.int16 else depth_u16.view(torch.int16)
    c = torch.as_tensor(color_u8)
    if d.dim() != 2 or c.dim() != 3 or tuple(c.shape) != (d.shape[0], d.shape[1], 3):
        raise ImfError(f"prepare_frame: depth {tuple(d.shape)} and colour {tuple(c.shape)}, expected [H, W] and [H, W, 3]")
    if c.dtype != torch.uint8:
        raise ImfError(f"prepare_frame: colour must be uint8, got {c.dtype}")
    d = d.to(device).contiguous()
    c = c.to(d.device).contiguous()
    K = np.asarray(intrinsic, np.float64)
    h, w = int(d.shape[0]), int(d.shape[1])
    L = _lib.lib()
    nbytes = L.imf_rgbd_frame_bytes(h, w, int(levels))
    block = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=d.device)
    check(L.imf_rgbd_prepare(d.data_ptr(), c.data_ptr(), h, w, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                             float(K[1, 2]), float(depth_scale), float(depth_min), float(depth_max), float(depth_edge),
                             int(levels), block.data_ptr(), nbytes, _stream()), "imf_rgbd_prepare")
    return RGBDFrame(block, h, w, int(levels), K.copy())


def _pair(src, dst, what):
    if not isinstance(src, RGBDFrame) or not isinstance(dst, RGBDFrame):
        raise ImfError(f"{what}: src and dst must be RGBDFrame (prepare_frame)")
    if (src.height, src.width, src.levels) != (dst.height, dst.width, dst.levels) or src.device != dst.device:
        raise ImfError(f"{what}: the frames were prepared for different shapes or devices")
    L = _lib.lib()
    nbytes = L.imf_rgbd_odometry_workspace_bytes(src.height, src.width, src.levels)
    return L, nbytes, torch.empty(nbytes, dtype=torch.uint8, device=src.device)


def rgbd_odometry_device(src, dst, init=None, iterations=ITERATIONS, max_depth_diff=0.03, lambda_depth=0.968, min_corr=30):
    """imf_rgbd_odometry; returns the device tensors (T [16], info [36], stats [2], meta int32 [4]) without copying."""
    L, nbytes, ws = _pair(src, dst, "rgbd_odometry")
    dev = src.device
    T = torch.empty(16, dtype=torch.float64, device=dev)
    info = torch.empty(36, dtype=torch.float64, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    meta = torch.zeros(4, dtype=torch.int32, device=dev)
    its = (C.c_int * len(iterations))(*[int(i) for i in iterations])
    init = None if init is None else np.ascontiguousarray(init, np.float64).reshape(16)
    check(L.imf_rgbd_odometry(src.block.data_ptr(), dst.block.data_ptr(),
                              init.ctypes.data_as(C.c_void_p) if init is not None else None, its, len(iterations),
                              float(max_depth_diff), float(lambda_depth), int(min_corr), T.data_ptr(), info.data_ptr(),
                              stats.data_ptr(), meta.data_ptr(), ws.data_ptr(), nbytes, _stream()), "imf_rgbd_odometry")
    return T, info, stats, meta


def rgbd_odometry(src, dst, init=None, iterations=ITERATIONS, max_depth_diff=0.03, lambda_depth=0.968, min_corr=30):
    """Fits the prepared frame `src` onto `dst`: (T float64 [4, 4] source camera -> target camera, info [6, 6], dict(n,
    fitness, cost, lost, flags, stages, n_valid)).  One device-to-host copy at the end."""
    T, info, stats, meta = rgbd_odometry_device(src, dst, init, iterations, max_depth_diff, lambda_depth, min_corr)
    host = torch.cat([T, info, stats, meta.to(torch.float64)]).cpu().numpy()
    n, flags, stages, n_valid = (int(v) for v in host[54:58])
    return host[:16].reshape(4, 4).copy(), host[16:52].reshape(6, 6).copy(), dict(
        n=n, fitness=float(host[52]), cost=float(host[53]), lost=bool(flags & 2), flags=flags, stages=stages, n_valid=n_valid)


def odometry_stage(src, dst, level, T, max_depth_diff=0.03, lambda_depth=0.968):
    """One stage at one level with the transformation T (imf_rgbd_odometry_stage, for the tests): (winner int32 [H_l, W_l],
    the 29 sums)."""
    L, nbytes, ws = _pair(src, dst, "odometry_stage")
    h, w = src.level_shape(max(0, min(int(level), src.levels - 1)))
    Td = torch.as_tensor(np.ascontiguousarray(T, np.float64).reshape(16)).to(src.device)
    winner = torch.empty(h * w, dtype=torch.int32, device=src.device)
    sums = torch.empty(29, dtype=torch.float64, device=src.device)
    check(L.imf_rgbd_odometry_stage(src.block.data_ptr(), dst.block.data_ptr(), int(level), Td.data_ptr(),
                                    float(max_depth_diff), float(lambda_depth), winner.data_ptr(), sums.data_ptr(),
                                    ws.data_ptr(), nbytes, _stream()), "imf_rgbd_odometry_stage")
    return winner.cpu().numpy().reshape(h, w), sums.cpu().numpy()


def track(depth, color, intrinsic, levels=3, iterations=ITERATIONS, max_depth_diff=0.03, lambda_depth=0.968, min_corr=30,
          depth_scale=1000.0, depth_min=0.0, depth_max=4.0, depth_edge=0.06, device="cuda"):
    """depth uint16 [F, H, W], colour uint8 [F, H, W, 3] -> (poses cam2first float64 [F, 4, 4], kept bool [F]).  Frame 0 is
    the identity; frame f is fitted as source onto the last kept frame from the identity, pose_f = pose_last . T; a lost
    pair drops frame f (NaN pose, kept False) and the next frame meets the same last kept frame.  Every frame is prepared
    once."""
    F = len(depth)
    poses = np.full((F, 4, 4), np.nan)
    kept = np.zeros(F, bool)
    prep = lambda f: prepare_frame(depth[f], color[f], intrinsic, levels, depth_scale, depth_min, depth_max, depth_edge, device)
    last = last_frame = None
    for f in range(F):
        frame = prep(f)
        if last is None:
            poses[f], kept[f], last, last_frame = np.eye(4), True, f, frame
            continue
        T, _, res = rgbd_odometry(frame, last_frame, None, iterations, max_depth_diff, lambda_depth, min_corr)
        if res["lost"]:
            continue
        poses[f], kept[f], last, last_frame = poses[last] @ T, True, f, frame
    return poses, kept
