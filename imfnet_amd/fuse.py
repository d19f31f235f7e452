"""Fragment fusion on the GPU: depth frames -> sparse TSDF volume -> surface points (csrc/tsdf.hip) or a triangle mesh
(csrc/tsdf_mesh.hip).

Replaces what data/fuse_fragments_3DMatch.py:47-96 does with Open3D's `ScalableTSDFVolume`: `integrate` per frame and
`extract_point_cloud`.  Colour is opt-in (`TSDFVolume(color=True)`: upstream's RGB8 volume, the rule at the head of
csrc/tsdf.hip); no normals.  There is no CPU path: a missing library or a failing call raises.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

UNIT_VOXELS = 4096
FLAG_RANGE, FLAG_CAPACITY = 1, 2
# integrate's frustum cull (csrc/tsdf.hip: k_tsdf_integrate) bounds a unit by a sphere in the camera's frame and gives its
# radius r0 a relative margin of 1e-6.  A voxel at q and the unit's centre c lie |M (q - c)| <= s_max |q - c| <= s_max r0 apart
# in the camera's frame (M: world2cam's rotation block, s_max its largest singular value), so the sphere holds the unit
# exactly when s_max <= 1 + 1e-6.  Half of the margin is accepted here, on either side of 1; the other half is left to the
# rounding of the check itself and of the kernel's fp64 sphere tests (both orders of magnitude smaller).  Float32-rounded
# relative poses, as the fragment command line forms them, measure about 1e-7.
RIGID_TOL = 5e-7


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _depth_to_device(depth, device):
    """uint16 [F,H,W] (numpy, or a torch int16 / uint16 tensor holding the same bits) -> an int16-typed device tensor."""
    if isinstance(depth, torch.Tensor):
        t = depth if depth.dtype == torch.int16 else depth.view(torch.int16)
    else:
        a = np.ascontiguousarray(depth)
        if a.dtype != np.uint16:
            raise TypeError(f"depth must be uint16, got {a.dtype}")
        t = torch.from_numpy(a.view(np.int16))
    if t.dim() != 3:
        raise ValueError(f"depth must be [frames, height, width], got {tuple(t.shape)}")
    return t.to(device, non_blocking=True).contiguous()


def _color_to_device(color, device):
    """uint8 [F,H,W,3] (numpy or a torch uint8 tensor) -> a contiguous device tensor."""
    if isinstance(color, torch.Tensor):
        if color.dtype != torch.uint8:
            raise ValueError(f"color must be uint8, got {color.dtype}")
        t = color
    else:
        a = np.ascontiguousarray(color)
        if a.dtype != np.uint8:
            raise ValueError(f"color must be uint8, got {a.dtype}")
        t = torch.from_numpy(a)
    if t.dim() != 4 or t.shape[3] != 3:
        raise ValueError(f"color must be [frames, height, width, 3], got {tuple(t.shape)}")
    return t.to(device, non_blocking=True).contiguous()


def check_rigid(poses_cam2world, what):
    """ValueError for the first finite pose whose world2cam rotation block has |singular value - 1| > RIGID_TOL (world2cam's
    singular values are the reciprocals of cam2world's).  A pose that holds a NaN or an infinity stays what it was: a frame
    to skip."""
    P = np.asarray(poses_cam2world, np.float64)
    finite = np.flatnonzero(np.isfinite(P).all((1, 2)))
    if len(finite) == 0:
        return
    s = np.linalg.svd(P[finite, :3, :3], compute_uv=False)
    with np.errstate(divide="ignore"):
        err = np.abs(1.0 / s - 1.0).max(1)
    bad = np.flatnonzero(~(err <= RIGID_TOL))
    if len(bad):
        raise ValueError(f"TSDFVolume.{what}: pose {finite[bad[0]]} is not rigid: a singular value of its world2cam rotation "
                         f"block is {err[bad[0]]:.3g} away from 1 (at most {RIGID_TOL:g}; the frustum cull relies on it)")


class TSDFVolume:
    """A sparse TSDF volume in device memory.  `allocate` opens the 16^3-voxel units around the depth samples of a batch of
    frames (any number of calls, all before the first `integrate`), `integrate` folds a batch of frames into the running
    average in frame order, `extract` returns the surface points as float64 [n,3] in a defined order, `extract_mesh` the
    surface as vertices and triangles; `voxels` / `load_voxels` save and restore the state.  Frames fed in
    several goes give the bits of one go.  Poses are rigid (RIGID_TOL; a ValueError names the first frame that is not) or
    hold a NaN, which skips the frame.  lattice_offset: 0.5 samples the voxel centres (Open3D), 0 the voxel corners
    (the lattice the published 3DMatch fragments lie on).  color=True keeps a running mean colour per voxel beside the
    tsdf: every `integrate` then takes the colour frames too, `extract(colors=True)` / `extract_mesh(colors=True)` return
    uint8 colours row for row, `colors` / `load_colors` save and restore the colour state.  The geometry of a coloured
    volume is the plain volume's, bit for bit."""

    def __init__(self, intrinsic, height, width, voxel_length=3.0 / 512, sdf_trunc=0.04, depth_scale=1000.0,
                 depth_trunc=6.0, lattice_offset=0.5, device="cuda", unit_capacity=1 << 14, color=False):
        self.L = _lib.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.ImfError("TSDFVolume runs on the GPU only (device='cuda')")
        K = np.asarray(intrinsic, np.float64)
        self.params = _lib.TsdfParams(K[0, 0], K[1, 1], K[0, 2], K[1, 2], voxel_length, sdf_trunc, depth_scale, depth_trunc,
                                      lattice_offset, int(height), int(width))
        self.unit_capacity = int(unit_capacity)
        self._pending = []          # the (depth, cam2world) batches of allocate, kept until the rows are final
        self._voxels = None
        self.color = bool(color)
        self._colors = None         # float32 [rows, 3, 4096] on the device, allocated with _voxels
        self.n_units = 0
        self.flags = 0
        self._tables()

    def _tables(self):
        cap, dev = self.unit_capacity, self.device
        self.table_capacity = int(self.L.imf_hash_capacity(cap))
        self._table = torch.empty(self.table_capacity * 2, dtype=torch.int64, device=dev)
        self._units = torch.zeros((cap, 3), dtype=torch.int32, device=dev)
        self._meta = torch.zeros(2, dtype=torch.int32, device=dev)
        ws = self.L.imf_tsdf_allocate_workspace_bytes(cap)
        if ws == 0:
            raise _lib.ImfError(f"imf_tsdf_allocate_workspace_bytes refuses unit_capacity={cap}")
        self._ws = torch.empty(ws, dtype=torch.uint8, device=dev)

    def _check_frames(self, depth, poses, what):
        d = _depth_to_device(depth, self.device)
        P = np.asarray(poses, np.float64)
        if P.shape != (d.shape[0], 4, 4):
            raise ValueError(f"poses must be [{d.shape[0]},4,4], got {P.shape}")
        if tuple(d.shape[1:]) != (self.params.height, self.params.width):
            raise ValueError(f"depth frames are {tuple(d.shape[1:])}, the volume expects "
                             f"({self.params.height}, {self.params.width})")
        check_rigid(P, what)
        return d, P

    def _allocate_call(self, d, c2w, reset):
        rc = self.L.imf_tsdf_allocate(_ptr(d), d.shape[0], _ptr(c2w), C.byref(self.params), int(reset), _ptr(self._table),
                                      self.table_capacity, _ptr(self._units), self.unit_capacity, _ptr(self._meta),
                                      _ptr(self._ws), self._ws.numel(), _stream(self.device))
        _lib.check(rc, "imf_tsdf_allocate")

    def allocate(self, depth_u16, poses_cam2world):
        if self._voxels is not None:
            raise _lib.ImfError("TSDFVolume.allocate after integrate: the unit rows are final once frames are integrated")
        d, P = self._check_frames(depth_u16, poses_cam2world, "allocate")
        c2w = torch.from_numpy(np.ascontiguousarray(P[:, :3, :].reshape(-1, 12))).to(self.device)
        first = not self._pending
        self._pending.append((d, c2w))
        self._allocate_call(d, c2w, first)
        n, flags = self._meta.tolist()
        while flags & FLAG_CAPACITY:                         # more units than room: grow and open them all again
            self.unit_capacity *= 2
            self._tables()
            for i, (di, ci) in enumerate(self._pending):
                self._allocate_call(di, ci, i == 0)
            n, flags = self._meta.tolist()
        self.n_units, self.flags = int(n), int(flags)
        return self.n_units

    @property
    def units(self):
        """int32 [n,3] unit coordinates (x, y, z), ascending in (z, y, x)."""
        return self._units[:self.n_units].cpu().numpy()

    def _open_state(self):
        """The end of the allocation phase: the zeroed state, once."""
        if self._voxels is None:
            self._pending = []
            self._voxels = torch.zeros((max(1, self.n_units), UNIT_VOXELS, 2), dtype=torch.float32, device=self.device)
        if self.color and self._colors is None:
            self._colors = torch.zeros((max(1, self.n_units), 3, UNIT_VOXELS), dtype=torch.float32, device=self.device)

    def _need_color(self, what):
        if not self.color:
            raise _lib.ImfError(f"TSDFVolume.{what}: the volume keeps no colour (TSDFVolume(color=True))")

    def integrate(self, depth_u16, poses_cam2world, color=None):
        d, P = self._check_frames(depth_u16, poses_cam2world, "integrate")
        if color is None and self.color:
            raise _lib.ImfError("TSDFVolume.integrate: a coloured volume integrates every frame with its colour image")
        if color is not None:
            self._need_color("integrate(color=...)")
            c = _color_to_device(color, self.device)
            if tuple(c.shape) != tuple(d.shape) + (3,):
                raise ValueError(f"color frames are {tuple(c.shape)}, the depth frames {tuple(d.shape)}")
        self._open_state()
        if self.n_units == 0 or d.shape[0] == 0:
            return
        with np.errstate(all="ignore"):
            w2c = np.stack([np.linalg.inv(T) if np.isfinite(T).all() else np.full((4, 4), np.nan) for T in P])
        w2c = torch.from_numpy(np.ascontiguousarray(w2c[:, :3, :].reshape(-1, 12))).to(self.device)
        if self.color:
            rc = self.L.imf_tsdf_integrate_rgb(_ptr(d), _ptr(c), d.shape[0], _ptr(w2c), C.byref(self.params), _ptr(self._units),
                                               _ptr(self._meta), self.n_units, _ptr(self._voxels), _ptr(self._colors),
                                               _stream(self.device))
            _lib.check(rc, "imf_tsdf_integrate_rgb")
            return
        rc = self.L.imf_tsdf_integrate(_ptr(d), d.shape[0], _ptr(w2c), C.byref(self.params), _ptr(self._units),
                                       _ptr(self._meta), self.n_units, _ptr(self._voxels), _stream(self.device))
        _lib.check(rc, "imf_tsdf_integrate")

    def extract(self, colors=False):
        """Surface points, float64 [n,3] on the host, ordered by (unit, voxel, axis); with colors=True (points, uint8
        [n,3] = R, G, B of every point)."""
        if colors:
            self._need_color("extract(colors=True)")
            return self._extract_rgb()
        if self._voxels is None or self.n_units == 0:
            return np.zeros((0, 3), np.float64)
        dev, n_u = self.device, self.n_units
        ws_bytes = self.L.imf_tsdf_extract_workspace_bytes(n_u)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out_n = torch.zeros(1, dtype=torch.int64, device=dev)

        def call(out, capacity):
            rc = self.L.imf_tsdf_extract(_ptr(self._voxels), _ptr(self._units), _ptr(self._meta), n_u, _ptr(self._table),
                                         self.table_capacity, C.byref(self.params), _ptr(out) if out is not None else None,
                                         capacity, _ptr(out_n), _ptr(ws), ws_bytes, _stream(dev))
            _lib.check(rc, "imf_tsdf_extract")

        call(None, 0)                                        # count, then the points into a buffer of that size
        n = int(out_n.item())
        if n == 0:
            return np.zeros((0, 3), np.float64)
        out = torch.empty((n, 3), dtype=torch.float64, device=dev)
        call(out, n)
        return out.cpu().numpy()

    def _extract_rgb(self):
        none = np.zeros((0, 3), np.float64), np.zeros((0, 3), np.uint8)
        if self._voxels is None or self.n_units == 0:
            return none
        dev, n_u = self.device, self.n_units
        ws_bytes = self.L.imf_tsdf_extract_workspace_bytes(n_u)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out_n = torch.zeros(1, dtype=torch.int64, device=dev)

        def call(out, rgb, capacity):
            rc = self.L.imf_tsdf_extract_rgb(_ptr(self._voxels), _ptr(self._colors), _ptr(self._units), _ptr(self._meta), n_u,
                                             _ptr(self._table), self.table_capacity, C.byref(self.params),
                                             _ptr(out) if out is not None else None, _ptr(rgb) if rgb is not None else None,
                                             capacity, _ptr(out_n), _ptr(ws), ws_bytes, _stream(dev))
            _lib.check(rc, "imf_tsdf_extract_rgb")

        call(None, None, 0)
        n = int(out_n.item())
        if n == 0:
            return none
        out = torch.empty((n, 3), dtype=torch.float64, device=dev)
        rgb = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        call(out, rgb, n)
        return out.cpu().numpy(), rgb.cpu().numpy()

    def extract_mesh(self, colors=False):
        """The surface as a triangle mesh (csrc/tsdf_mesh.hip: marching tetrahedra on the Kuhn split): vertices float64
        [n,3] ordered by (unit, voxel, edge slot) and triangles int32 [m,3] ordered by (unit, cell, tetrahedron, triangle),
        counter-clockwise seen from free space, on the host; with colors=True (vertices, triangles, uint8 [n,3] = R, G, B
        of every vertex)."""
        none = np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int32)
        if colors:
            self._need_color("extract_mesh(colors=True)")
            none = none + (np.zeros((0, 3), np.uint8),)
        if self._voxels is None or self.n_units == 0:
            return none
        dev, n_u = self.device, self.n_units
        ws_bytes = self.L.imf_tsdf_mesh_workspace_bytes(n_u)
        if ws_bytes == 0:
            raise _lib.ImfError(f"imf_tsdf_mesh_workspace_bytes refuses {n_u} units")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out_n = torch.zeros(2, dtype=torch.int64, device=dev)

        def call(vertices, triangles, rgb=None):
            opt = lambda x: _ptr(x) if x is not None else None
            n_v, n_t = (0 if x is None else len(x) for x in (vertices, triangles))
            if colors:
                rc = self.L.imf_tsdf_mesh_rgb(_ptr(self._voxels), _ptr(self._colors), _ptr(self._units), _ptr(self._meta), n_u,
                                              _ptr(self._table), self.table_capacity, C.byref(self.params), opt(vertices),
                                              opt(rgb), n_v, opt(triangles), n_t, _ptr(out_n), _ptr(ws), ws_bytes, _stream(dev))
                _lib.check(rc, "imf_tsdf_mesh_rgb")
                return
            rc = self.L.imf_tsdf_mesh(_ptr(self._voxels), _ptr(self._units), _ptr(self._meta), n_u, _ptr(self._table),
                                      self.table_capacity, C.byref(self.params), opt(vertices), n_v, opt(triangles), n_t,
                                      _ptr(out_n), _ptr(ws), ws_bytes, _stream(dev))
            _lib.check(rc, "imf_tsdf_mesh")

        call(None, None)                                     # count, then the mesh into buffers of that size
        n_v, n_t = out_n.tolist()
        if n_v == 0 or n_t == 0:
            return none
        if n_v > 2 ** 31 - 1:
            raise _lib.ImfError(f"TSDFVolume.extract_mesh: {n_v} vertices do not fit int32 indices")
        vertices = torch.empty((n_v, 3), dtype=torch.float64, device=dev)
        triangles = torch.empty((n_t, 3), dtype=torch.int32, device=dev)
        if colors:
            rgb = torch.empty((n_v, 3), dtype=torch.uint8, device=dev)
            call(vertices, triangles, rgb)
            return vertices.cpu().numpy(), triangles.cpu().numpy(), rgb.cpu().numpy()
        call(vertices, triangles)
        return vertices.cpu().numpy(), triangles.cpu().numpy()

    def voxels(self):
        """The state as a host copy: float32 [n_units, 4096, 2] = (tsdf, weight) of voxel (z * 16 + y) * 16 + x."""
        if self._voxels is None or self.n_units == 0:
            return np.zeros((self.n_units, UNIT_VOXELS, 2), np.float32)
        return self._voxels[:self.n_units].cpu().numpy()

    def load_voxels(self, array):
        """Replaces the state with float32 [n_units, 4096, 2] (what `voxels` returns).  Allowed once the unit rows are
        final, that is after `allocate`; like `integrate` it ends the allocation phase."""
        a = np.ascontiguousarray(array, np.float32)
        if a.shape != (self.n_units, UNIT_VOXELS, 2):
            raise ValueError(f"voxels must be [{self.n_units}, {UNIT_VOXELS}, 2], got {a.shape}")
        if self.n_units == 0:
            raise _lib.ImfError("TSDFVolume.load_voxels: no units are open (call allocate first)")
        self._pending = []
        self._voxels = torch.from_numpy(a).to(self.device).contiguous()
        if self.color and self._colors is None:
            self._colors = torch.zeros((self.n_units, 3, UNIT_VOXELS), dtype=torch.float32, device=self.device)

    def colors(self):
        """The colour state as a host copy: float32 [n_units, 4096, 3] = (R, G, B) on the 0..255 scale of voxel
        (z * 16 + y) * 16 + x, whatever the device layout (three planes per unit) is."""
        self._need_color("colors")
        if self._colors is None or self.n_units == 0:
            return np.zeros((self.n_units, UNIT_VOXELS, 3), np.float32)
        return self._colors[:self.n_units].permute(0, 2, 1).contiguous().cpu().numpy()

    def load_colors(self, array):
        """Replaces the colour state with float32 [n_units, 4096, 3] (what `colors` returns); like `load_voxels` it ends
        the allocation phase, and a volume that has no state yet gets a zeroed one."""
        self._need_color("load_colors")
        a = np.ascontiguousarray(array, np.float32)
        if a.shape != (self.n_units, UNIT_VOXELS, 3):
            raise ValueError(f"colors must be [{self.n_units}, {UNIT_VOXELS}, 3], got {a.shape}")
        if self.n_units == 0:
            raise _lib.ImfError("TSDFVolume.load_colors: no units are open (call allocate first)")
        self._open_state()
        self._colors = torch.from_numpy(a).to(self.device).permute(0, 2, 1).contiguous()


def fuse_volume(depth_u16, poses_cam2world, intrinsic, voxel_length=3.0 / 512, sdf_trunc=0.04, depth_scale=1000.0,
                depth_trunc=6.0, lattice_offset=0.5, device="cuda", color=None):
    """The volume of one fragment, allocated and integrated; a coloured one when `color` (uint8 [F,H,W,3]) is given."""
    depth = depth_u16 if isinstance(depth_u16, torch.Tensor) else np.asarray(depth_u16)
    vol = TSDFVolume(intrinsic, depth.shape[1], depth.shape[2], voxel_length, sdf_trunc, depth_scale, depth_trunc,
                     lattice_offset, device, color=color is not None)
    d = _depth_to_device(depth, vol.device)
    vol.allocate(d, poses_cam2world)
    vol.integrate(d, poses_cam2world, color)
    return vol


def fuse_mesh(depth_u16, poses_cam2world, intrinsic, voxel_length=3.0 / 512, sdf_trunc=0.04, depth_scale=1000.0,
              depth_trunc=6.0, lattice_offset=0.5, device="cuda", color=None):
    """One fragment as a mesh: the arguments of fuse_fragment -> (vertices float64 [n,3], triangles int32 [m,3]); with
    `color` also the vertex colours, uint8 [n,3]."""
    return fuse_volume(depth_u16, poses_cam2world, intrinsic, voxel_length, sdf_trunc, depth_scale, depth_trunc,
                       lattice_offset, device, color).extract_mesh(colors=color is not None)


def fuse_fragment(depth_u16, poses_cam2world, intrinsic, voxel_length=3.0 / 512, sdf_trunc=0.04, depth_scale=1000.0,
                  depth_trunc=6.0, lattice_offset=0.5, device="cuda", color=None):
    """One fragment: depth_u16 [F,H,W] uint16, poses_cam2world [F,4,4], intrinsic [3,3] -> float64 [n,3]; with `color`
    (uint8 [F,H,W,3]) -> (points, uint8 [n,3])."""
    return fuse_volume(depth_u16, poses_cam2world, intrinsic, voxel_length, sdf_trunc, depth_scale, depth_trunc,
                       lattice_offset, device, color).extract(colors=color is not None)
