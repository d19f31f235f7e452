"""KITTI odometry pairs and their ground truth, test phase -- `KITTINMPairDataset` of lib/data_loaders.py:620-713 with
IS_ODOMETRY, no rotation, no scale, no jitter, restated for the evaluator (imfnet_amd/evaluate_kitti.py).

Host side: the pair list, the pose algebra, the cache of refined ground truths, the point / image loading.  The two
expensive steps run on the GPU: the ground-truth refinement is `matching.icp_point_to_point` on the 5 cm
first-occurrence subsets (quantised by `imf_voxelize` in the float32-quotient mode), the overlap test is
`matching.radius_count`.  The reference's quirks are kept; each one is listed in DESIGN.md §10.
"""
import glob
import os

import numpy as np
import torch

from . import _lib
from ._lib import ImfError, check

MIN_DIST = 10                          # lib/data_loaders.py:630
SEARCH_WINDOW = 100                    # :672
DROPPED_PAIRS = [(8, 15, 58)]          # :706-712 "problematic sequence"
ICP_VOXEL = 0.05                       # :531-533
ICP_MAX_CORR = 0.2                     # :539
ICP_MAX_ITER = 200                     # :542
MIN_MATCHES = 1000                     # :587

# lib/data_loaders.py:408-420 -- including the trailing .T of the 4x4
_R_VELO2CAM = np.array([7.533745e-03, -9.999714e-01, -6.166020e-04, 1.480249e-02, 7.280733e-04, -9.998902e-01,
                        9.998621e-01, 7.523790e-03, 1.480755e-02]).reshape(3, 3)
_T_VELO2CAM = np.array([-4.069766e-03, -7.631618e-02, -2.717806e-01]).reshape(3, 1)
VELO2CAM = np.vstack((np.hstack([_R_VELO2CAM, _T_VELO2CAM]), [0, 0, 0, 1])).T


def read_test_sequences(path=None):
    """config/test_kitti.txt: the odometry sequences of the test phase."""
    if path is None:
        return [8, 9, 10]
    return [int(v) for v in open(path).read().split()]


def read_poses(kitti_root, drive):
    """dataset/poses/%02d.txt as 4x4 matrices (get_video_odometry + odometry_to_positions, :421-452)."""
    odo = np.genfromtxt(os.path.join(kitti_root, "dataset", "poses", "%02d.txt" % drive))
    odo = np.atleast_2d(odo)
    return np.array([np.vstack((o.reshape(3, 4), [0, 0, 0, 1])) for o in odo])


def frame_numbers(kitti_root, drive):
    fnames = glob.glob(os.path.join(kitti_root, "dataset", "sequences", "%02d" % drive, "velodyne", "*.bin"))
    if not fnames:
        raise ImfError(f"no velodyne scans under {kitti_root}/dataset/sequences/{drive:02d}")
    return sorted(int(os.path.split(f)[-1][:-4]) for f in fnames)


def pairs_of_sequence(drive, inames, positions):
    """lib/data_loaders.py:658-682 for one sequence.  inames: the sorted frame numbers; positions: [n,4,4] poses
    indexed by frame number.  Kept: the window [t, t+100), the `first_hit + t - 1` offset (the reference's port of
    3DFeatNet's 1-based MATLAB), the pair only when that frame exists.  An empty window advances t by one and adds no
    pair (the reference gets there through `empty_array in inames`, whose truth value is False)."""
    Ts = positions[:, :3, 3]
    pdist = np.sqrt(((Ts.reshape(1, -1, 3) - Ts.reshape(-1, 1, 3)) ** 2).sum(-1))
    valid = pdist > MIN_DIST
    names = set(inames)
    out = []
    t = inames[0]
    while t in names:
        hits = np.where(valid[t][t:t + SEARCH_WINDOW])[0]
        if len(hits) == 0:
            t += 1
            continue
        nxt = int(hits[0]) + t - 1
        if nxt in names:
            out.append((drive, t, nxt))
            t = nxt + 1
    return out


def pair_list(kitti_root, sequences=None):
    files = []
    for drive in sequences if sequences is not None else read_test_sequences():
        files += pairs_of_sequence(drive, frame_numbers(kitti_root, drive), read_poses(kitti_root, drive))
    for item in DROPPED_PAIRS:
        if item in files:
            files.pop(files.index(item))
    return files


def pose_from_positions(P0, P1):
    """lib/data_loaders.py:536-537: M = (velo2cam @ P0.T @ inv(P1.T) @ inv(velo2cam)).T."""
    return (VELO2CAM @ P0.T @ np.linalg.inv(P1.T) @ np.linalg.inv(VELO2CAM)).T


def apply_transform(pts, trans):
    """lib/data_loaders.py:137-141 (float32 points @ float64 matrix -> float64)."""
    return pts @ trans[:3, :3].T + trans[:3, 3]


def velodyne_path(kitti_root, drive, t):
    return os.path.join(kitti_root, "dataset", "sequences", "%02d" % drive, "velodyne", "%06d.bin" % t)


def read_scan(path):
    """float32 xyzr -> xyz float32 [n,3] (lib/data_loaders.py:521-525)."""
    return np.ascontiguousarray(np.fromfile(path, dtype=np.float32).reshape(-1, 4)[:, :3])


def voxel_first_indices(xyz_f32, voxel_size, device="cuda"):
    """ME.utils.sparse_quantize(xyz_f32 / voxel_size, return_index=True) with the float32 quotient (numpy's or torch's
    float32 division, lib/data_loaders.py:532-533, 578-579): ascending first-occurrence indices, int64 numpy.
    imf_voxelize in mode IMF_XYZ_F32_QUOTIENT."""
    pts = torch.from_numpy(np.ascontiguousarray(xyz_f32, dtype=np.float32)).to(device)
    _, first = voxelize_f32(pts, voxel_size)
    return first.cpu().numpy().astype(np.int64)


def voxelize_f32(pts, voxel_size):
    """Device float32 points -> (coords int32 [M,4] (b, x, y, z), first_idx int32 [M]) in the float32-quotient mode."""
    if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
        raise ImfError(f"voxelize_f32: float32 [n>0, 3] points, got {pts.dtype} {tuple(pts.shape)}")
    pts = pts.contiguous()
    n, dev = pts.shape[0], pts.device
    L = _lib.lib()
    cap = L.imf_hash_capacity(n)
    coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    meta = torch.zeros(2, dtype=torch.int32, device=dev)           # [0] M, [1] range error
    table = torch.empty(cap * 16, dtype=torch.uint8, device=dev)
    ws = torch.empty(L.imf_unique_workspace_bytes(n), dtype=torch.uint8, device=dev)
    check(L.imf_voxelize(pts.data_ptr(), _lib.XYZ_F32_QUOTIENT, n, float(voxel_size), 0, coords.data_ptr(),
                         first.data_ptr(), meta.data_ptr(), table.data_ptr(), cap, ws.data_ptr(), meta[1:].data_ptr(),
                         torch.cuda.current_stream(dev).cuda_stream), "imf_voxelize")
    m, err = meta.tolist()
    if err:
        raise ImfError("voxelize_f32: a coordinate is NaN or out of range")
    return coords[:m], first[:m]


def icp_cache_path(kitti_root, drive, t0, t1):
    return os.path.join(kitti_root, "icp", "%d_%d_%d.npy" % (drive, t0, t1))


def refine_ground_truth(xyz0, xyz1, M, device="cuda"):
    """lib/data_loaders.py:529-547: ICP (0.2 m, identity init, 200 iterations) of the 5 cm subset of scan 0, moved by
    M in fp64, onto the 5 cm subset of scan 1; returns (M @ T_icp, the ICP result tuple)."""
    from .matching import icp_point_to_point
    sel0 = voxel_first_indices(xyz0, ICP_VOXEL, device)
    sel1 = voxel_first_indices(xyz1, ICP_VOXEL, device)
    xyz0_t = apply_transform(xyz0[sel0], M)
    res = icp_point_to_point(xyz0_t, xyz1[sel1].astype(np.float64), ICP_MAX_CORR, None, ICP_MAX_ITER, device=device)
    return M @ res[0], res


def ground_truth(kitti_root, drive, t0, t1, xyz0, xyz1, positions, device="cuda"):
    """The refined pose of a pair through the reference's cache: `<kitti_root>/icp/<drive>_<t0>_<t1>.npy` (4x4 fp64,
    np.save) is read as it is when present; otherwise ICP runs and the file is written by temporary file + rename."""
    path = icp_cache_path(kitti_root, drive, t0, t1)
    if os.path.exists(path):
        return np.load(path), False
    M = pose_from_positions(positions[t0], positions[t1])
    M2, _ = refine_ground_truth(xyz0, xyz1, M, device)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tmp = f"{path}.tmp{os.getpid()}.npy"
    np.save(tmp, M2)
    os.replace(tmp, path)
    return M2, True


def pair_image_paths(kitti_root, drive, t0, t1, own_image=False):
    """lib/data_loaders.py:508-509 reads fname0's PNG for BOTH fragments (kept by default); own_image=True uses t1's."""
    f0 = velodyne_path(kitti_root, drive, t0)
    f1 = velodyne_path(kitti_root, drive, t1)
    return f0.replace(".bin", ".png"), (f1 if own_image else f0).replace(".bin", ".png")


def load_image(path, H=120, W=160):
    """matplotlib's imread + process_image when the size differs (:510-519), as [1,3,H,W] float32."""
    from .dataio import process_image, read_image
    img = read_image(path)
    if img.shape[0] != H or img.shape[1] != W:
        img = process_image(image=img, aim_H=H, aim_W=W)
    return np.ascontiguousarray(np.transpose(img, (2, 0, 1))[None], dtype=np.float32)


# ---- metrics (scripts/evaluation_kitti_open3d_12.py:116-150) ----------------------------------------------------------

class AverageMeter:
    """lib/timer.py:4-24 (var = sq_sum / count - avg^2)."""

    def __init__(self):
        self.val = self.avg = self.sum = self.sq_sum = 0.0
        self.count = 0
        self.var = None

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count
        self.sq_sum += val ** 2 * n
        self.var = self.sq_sum / self.count - self.avg ** 2


def pair_errors(T_ransac, T_gt):
    """(rte, rre) in the reference's float32 expressions: T_ransac float32 (ransac_result.transformation.astype(
    np.float32)), T_gt float32 (the collate's .float()); rre = arccos((tr(R^T R_gt) - 1) / 2) may be NaN."""
    Tr = torch.from_numpy(np.asarray(T_ransac).astype(np.float32))
    Tg = torch.as_tensor(np.asarray(T_gt)).float()
    rte = np.linalg.norm(Tr[:3, 3] - Tg[:3, 3])
    with np.errstate(invalid="ignore"):
        rre = np.arccos((np.trace(Tr[:3, :3].t() @ Tg[:3, :3]) - 1) / 2)
    return rte, rre


def is_success(rte, rre):
    return bool(rte < 2 and not np.isnan(rre) and rre < np.pi / 180 * 5)


class KittiMeters:
    """success / RTE / RRE meters of the script; each error meter only takes its own kind of success (rte < 2 m,
    rre < 5 deg and not NaN).  `summary()` reports None for an empty meter (the reference divides by zero)."""

    def __init__(self):
        self.success, self.rte, self.rre = AverageMeter(), AverageMeter(), AverageMeter()
        self.nan_rre = 0

    def update(self, rte, rre):
        if rte < 2:                                   # float32 values: the meters add in float32, as the script's do
            self.rte.update(rte)
        if np.isnan(rre):
            self.nan_rre += 1
        elif rre < np.pi / 180 * 5:
            self.rre.update(rre)
        ok = is_success(rte, rre)
        self.success.update(1 if ok else 0)
        return ok

    def summary(self):
        def mv(m):
            return (float(m.avg), float(m.var)) if m.count else (None, None)
        rte_mean, rte_var = mv(self.rte)
        rre_mean, rre_var = mv(self.rre)
        return dict(pairs=self.success.count, successes=int(self.success.sum),
                    rate=float(self.success.avg) if self.success.count else None,
                    rte_mean=rte_mean, rte_var=rte_var, rre_mean=rre_mean, rre_var=rre_var, nan_rre=self.nan_rre)
