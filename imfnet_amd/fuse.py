"""Fragment fusion on the GPU: depth frames -> sparse TSDF volume -> surface points (csrc/tsdf.hip) or a triangle mesh
(csrc/tsdf_mesh.hip).

Replaces what data/fuse_fragments_3DMatch.py:47-96 does with Open3D's `ScalableTSDFVolume`: `integrate` per frame and
`extract_point_cloud`.  No colour, no normals (nothing downstream reads them).  There is no CPU path: a missing library or
a failing call raises.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

UNIT_VOXELS = 4096
FLAG_RANGE, FLAG_CAPACITY = 1, 2


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


class TSDFVolume:
    """A sparse TSDF volume in device memory.  `allocate` opens the 16^3-voxel units around the depth samples of a batch of
    frames (any number of calls, all before the first `integrate`), `integrate` folds a batch of frames into the running
    average in frame order, `extract` returns the surface points as float64 [n,3] in a defined order, `extract_mesh` the
    surface as vertices and triangles; `voxels` / `load_voxels` save and restore the state.  Frames fed in
    several goes give the bits of one go.  lattice_offset: 0.5 samples the voxel centres (Open3D), 0 the voxel corners
    (the lattice the published 3DMatch fragments lie on)."""

    def __init__(self, intrinsic, height, width, voxel_length=3.0 / 512, sdf_trunc=0.04, depth_scale=1000.0,
                 depth_trunc=6.0, lattice_offset=0.5, device="cuda", unit_capacity=1 << 14):
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

    def _check_frames(self, depth, poses):
        d = _depth_to_device(depth, self.device)
        P = np.asarray(poses, np.float64)
        if P.shape != (d.shape[0], 4, 4):
            raise ValueError(f"poses must be [{d.shape[0]},4,4], got {P.shape}")
        if tuple(d.shape[1:]) != (self.params.height, self.params.width):
            raise ValueError(f"depth frames are {tuple(d.shape[1:])}, the volume expects "
                             f"({self.params.height}, {self.params.width})")
        return d, P

    def _allocate_call(self, d, c2w, reset):
        rc = self.L.imf_tsdf_allocate(_ptr(d), d.shape[0], _ptr(c2w), C.byref(self.params), int(reset), _ptr(self._table),
                                      self.table_capacity, _ptr(self._units), self.unit_capacity, _ptr(self._meta),
                                      _ptr(self._ws), self._ws.numel(), _stream(self.device))
        _lib.check(rc, "imf_tsdf_allocate")

    def allocate(self, depth_u16, poses_cam2world):
        if self._voxels is not None:
            raise _lib.ImfError("TSDFVolume.allocate after integrate: the unit rows are final once frames are integrated")
        d, P = self._check_frames(depth_u16, poses_cam2world)
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

    def integrate(self, depth_u16, poses_cam2world):
        d, P = self._check_frames(depth_u16, poses_cam2world)
        if self._voxels is None:
            self._pending = []
            self._voxels = torch.zeros((max(1, self.n_units), UNIT_VOXELS, 2), dtype=torch.float32, device=self.device)
        if self.n_units == 0 or d.shape[0] == 0:
            return
        with np.errstate(all="ignore"):
            w2c = np.stack([np.linalg.inv(T) if np.isfinite(T).all() else np.full((4, 4), np.nan) for T in P])
        w2c = torch.from_numpy(np.ascontiguousarray(w2c[:, :3, :].reshape(-1, 12))).to(self.device)
        rc = self.L.imf_tsdf_integrate(_ptr(d), d.shape[0], _ptr(w2c), C.byref(self.params), _ptr(self._units),
                                       _ptr(self._meta), self.n_units, _ptr(self._voxels), _stream(self.device))
        _lib.check(rc, "imf_tsdf_integrate")

    def extract(self):
        """Surface points, float64 [n,3] on the host, ordered by (unit, voxel, axis)."""
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

    def extract_mesh(self):
        """The surface as a triangle mesh (csrc/tsdf_mesh.hip: marching tetrahedra on the Kuhn split): vertices float64
        [n,3] ordered by (unit, voxel, edge slot) and triangles int32 [m,3] ordered by (unit, cell, tetrahedron, triangle),
        counter-clockwise seen from free space, on the host."""
        none = np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int32)
        if self._voxels is None or self.n_units == 0:
            return none
        dev, n_u = self.device, self.n_units
        ws_bytes = self.L.imf_tsdf_mesh_workspace_bytes(n_u)
        if ws_bytes == 0:
            raise _lib.ImfError(f"imf_tsdf_mesh_workspace_bytes refuses {n_u} units")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out_n = torch.zeros(2, dtype=torch.int64, device=dev)

        def call(vertices, triangles):
            rc = self.L.imf_tsdf_mesh(_ptr(self._voxels), _ptr(self._units), _ptr(self._meta), n_u, _ptr(self._table),
                                      self.table_capacity, C.byref(self.params),
                                      _ptr(vertices) if vertices is not None else None, 0 if vertices is None else len(vertices),
                                      _ptr(triangles) if triangles is not None else None,
                                      0 if triangles is None else len(triangles), _ptr(out_n), _ptr(ws), ws_bytes, _stream(dev))
            _lib.check(rc, "imf_tsdf_mesh")

        call(None, None)                                     # count, then the mesh into buffers of that size
        n_v, n_t = out_n.tolist()
        if n_v == 0 or n_t == 0:
            return none
        if n_v > 2 ** 31 - 1:
            raise _lib.ImfError(f"TSDFVolume.extract_mesh: {n_v} vertices do not fit int32 indices")
        vertices = torch.empty((n_v, 3), dtype=torch.float64, device=dev)
        triangles = torch.empty((n_t, 3), dtype=torch.int32, device=dev)
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


def fuse_volume(depth_u16, poses_cam2world, intrinsic, voxel_length=3.0 / 512, sdf_trunc=0.04, depth_scale=1000.0,
                depth_trunc=6.0, lattice_offset=0.5, device="cuda"):
    """The volume of one fragment, allocated and integrated."""
    depth = depth_u16 if isinstance(depth_u16, torch.Tensor) else np.asarray(depth_u16)
    vol = TSDFVolume(intrinsic, depth.shape[1], depth.shape[2], voxel_length, sdf_trunc, depth_scale, depth_trunc,
                     lattice_offset, device)
    d = _depth_to_device(depth, vol.device)
    vol.allocate(d, poses_cam2world)
    vol.integrate(d, poses_cam2world)
    return vol


def fuse_mesh(depth_u16, poses_cam2world, intrinsic, voxel_length=3.0 / 512, sdf_trunc=0.04, depth_scale=1000.0,
              depth_trunc=6.0, lattice_offset=0.5, device="cuda"):
    """One fragment as a mesh: the arguments of fuse_fragment -> (vertices float64 [n,3], triangles int32 [m,3])."""
    return fuse_volume(depth_u16, poses_cam2world, intrinsic, voxel_length, sdf_trunc, depth_scale, depth_trunc,
                       lattice_offset, device).extract_mesh()


def fuse_fragment(depth_u16, poses_cam2world, intrinsic, voxel_length=3.0 / 512, sdf_trunc=0.04, depth_scale=1000.0,
                  depth_trunc=6.0, lattice_offset=0.5, device="cuda"):
    """One fragment: depth_u16 [F,H,W] uint16, poses_cam2world [F,4,4], intrinsic [3,3] -> float64 [n,3]."""
    return fuse_volume(depth_u16, poses_cam2world, intrinsic, voxel_length, sdf_trunc, depth_scale, depth_trunc,
                       lattice_offset, device).extract()
