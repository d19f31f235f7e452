"""Descriptor matching for the feature-match-recall evaluation, host side.

Mirrors the reference's names: `knn_search` is util/uio.py:245-258, the mutual check and the inlier
ratio are scripts/evaluation_3dmatch.py:207-234.  Everything runs in libimfnet_hip.so
(`imf_nn_search`, `imf_mutual_inliers`); there is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ImfError, check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _descs(x, device, name):
    t = torch.as_tensor(x)
    if t.dim() != 2:
        raise ImfError(f"{name} must be [n, dim], got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32).contiguous()


def nn_search(query, db, return_dist2=False):
    """Device tensors in, device tensors out: nn int32 [n_query] (and squared fp64 distances).  A db row with a NaN or
    an infinity is never chosen; a query left without a row (its own row is not finite, or no db row is) gets nn = -1 and
    dist2 = NaN.  Mask nn >= 0 before gathering with it: -1 would wrap to the last row."""
    if query.shape[1] != db.shape[1]:
        raise ImfError(f"descriptor widths differ: {query.shape[1]} vs {db.shape[1]}")
    if db.shape[0] == 0:
        raise ImfError("knn_search on an empty destination set")
    nq, nd, dim = query.shape[0], db.shape[0], query.shape[1]
    dev = query.device
    L = _lib.lib()
    ws_bytes = L.imf_nn_workspace_bytes(nq, nd)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    nn = torch.empty(nq, dtype=torch.int32, device=dev)
    d2 = torch.empty(nq, dtype=torch.float64, device=dev) if return_dist2 else None
    check(L.imf_nn_search(query.data_ptr(), nq, db.data_ptr(), nd, dim, nn.data_ptr(),
                          d2.data_ptr() if return_dist2 else None, ws.data_ptr(), ws_bytes, _stream()),
          "imf_nn_search")
    return (nn, d2) if return_dist2 else nn


def knn_search(points_src, points_dst, k=1, device="cuda"):
    """util/uio.py:245-258: for every row of points_src the index of its nearest row of points_dst
    (exact, fp64 distances).  Returns int32 numpy [len(points_src)]; only k=1 (the only value the
    evaluation uses, scripts/evaluation_3dmatch.py:207-210)."""
    if k != 1:
        raise NotImplementedError("knn_search: the evaluation path uses k=1 only")
    nn = nn_search(_descs(points_src, device, "points_src"), _descs(points_dst, device, "points_dst"))
    return nn.cpu().numpy()


def select_keypoints(sample_points, coords, voxel_size, device="cuda"):
    """scripts/evaluation_3dmatch.py:162-171: indices (ascending, int64 numpy like `np.where`) of the
    rows of `coords` (the descriptor file's `xyz`) whose voxel key occurs among the voxel keys of
    `sample_points` (the randomly drawn raw points)."""
    s = torch.as_tensor(sample_points).to(device=device, dtype=torch.float64).contiguous()
    c = torch.as_tensor(coords).to(device=device, dtype=torch.float64).contiguous()
    if s.dim() != 2 or c.dim() != 2 or s.shape[1] != 3 or c.shape[1] != 3:
        raise ImfError(f"expected [n,3] arrays, got {tuple(s.shape)} and {tuple(c.shape)}")
    ns, m = s.shape[0], c.shape[0]
    L = _lib.lib()
    ws_bytes = L.imf_keypoint_workspace_bytes(ns, m)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=s.device)
    inds = torch.empty(max(m, 1), dtype=torch.int32, device=s.device)
    count = torch.zeros(1, dtype=torch.int32, device=s.device)
    check(L.imf_select_keypoints(s.data_ptr(), ns, c.data_ptr(), m, float(voxel_size), inds.data_ptr(),
                                 count.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "imf_select_keypoints")
    return inds[:int(count.item())].cpu().numpy().astype(np.int64)


def mutual_inliers(nn21, nn12, kpts1=None, kpts2=None, pose=None, inlier_thresh=0.1):
    """scripts/evaluation_3dmatch.py:212-233 on device tensors.  Returns (frag2_match_indices int32
    device tensor, n_matches, n_inliers); n_inliers is 0 when no geometry is given."""
    dev = nn21.device
    n2, n1 = nn21.shape[0], nn12.shape[0]
    match2 = torch.empty(max(n2, 1), dtype=torch.int32, device=dev)
    meta = torch.zeros(2, dtype=torch.int32, device=dev)
    geo = kpts1 is not None and kpts2 is not None and pose is not None
    if geo:
        kpts1 = torch.as_tensor(kpts1).to(device=dev, dtype=torch.float64).contiguous()
        kpts2 = torch.as_tensor(kpts2).to(device=dev, dtype=torch.float64).contiguous()
        if kpts1.shape != (n1, 3) or kpts2.shape != (n2, 3):
            raise ImfError(f"keypoints must be [{n1},3] and [{n2},3], got {tuple(kpts1.shape)}, {tuple(kpts2.shape)}")
        T = np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(4, 4))
        pose_p = T.ctypes.data_as(C.c_void_p)
    check(_lib.lib().imf_mutual_inliers(nn21.data_ptr(), n2, nn12.data_ptr(), n1,
                                        kpts1.data_ptr() if geo else None, kpts2.data_ptr() if geo else None,
                                        pose_p if geo else None, float(inlier_thresh), match2.data_ptr(),
                                        meta.data_ptr(), _stream()), "imf_mutual_inliers")
    n_matches, n_inliers = meta.tolist()
    return match2[:n_matches], n_matches, n_inliers


def feature_match(frag1_kpts, frag1_descs, frag2_kpts, frag2_descs, gt_pose, inlier_thresh=0.1,
                  device="cuda"):
    """The FMR part of `register_fragment_pair` (scripts/evaluation_3dmatch.py:207-234): both
    nearest-neighbour searches, the mutual check, the ground-truth transform and the inlier count.
    Returns (num_inliers, inlier_ratio, frag2_match_indices, frag21_nnindices); inlier_ratio is nan
    when there is no mutual match (the reference divides 0 by 0).  frag21_nnindices holds -1 where `nn_search` found
    no neighbour (a non-finite descriptor row); such a keypoint is never a mutual match."""
    d1 = _descs(frag1_descs, device, "frag1_descs")
    d2 = _descs(frag2_descs, device, "frag2_descs")
    nn21 = nn_search(d2, d1)
    nn12 = nn_search(d1, d2)
    match2, n_matches, n_inliers = mutual_inliers(nn21, nn12, frag1_kpts, frag2_kpts, gt_pose, inlier_thresh)
    ratio = n_inliers / n_matches if n_matches else float("nan")
    return n_inliers, ratio, match2.cpu().numpy(), nn21.cpu().numpy()


def ransac_registration(src, dst, corres, ransac_n=3, max_corr_dist=0.075, edge_similarity=0.9, max_iter=50000,
                        seed=0, device="cuda"):
    """Device RANSAC on given correspondences (imf_ransac_registration).  Returns (T 4x4 numpy
    source->target, winning iteration, inliers, hypotheses that passed the checkers, fitness, rmse).  corres[i] < 0 or
    >= len(dst) means "no correspondence" (`nn_search`'s -1): never drawn into a surviving hypothesis, never an inlier."""
    s = torch.as_tensor(src).to(device=device, dtype=torch.float64).contiguous()
    d = torch.as_tensor(dst).to(device=device, dtype=torch.float64).contiguous()
    c = torch.as_tensor(corres).to(device=s.device, dtype=torch.int32).contiguous()
    if s.dim() != 2 or s.shape[1] != 3 or d.dim() != 2 or d.shape[1] != 3 or c.shape != (s.shape[0],):
        raise ImfError("ransac_registration: src [n,3], dst [m,3], corres [n]")
    L = _lib.lib()
    nbytes = L.imf_ransac_workspace_bytes(int(max_iter))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    T = torch.empty(16, dtype=torch.float64, device=s.device)
    meta = torch.empty(3, dtype=torch.int32, device=s.device)
    stats = torch.empty(2, dtype=torch.float64, device=s.device)
    check(L.imf_ransac_registration(s.data_ptr(), s.shape[0], d.data_ptr(), d.shape[0], c.data_ptr(), int(ransac_n),
                                    float(max_corr_dist), float(edge_similarity), int(max_iter), int(seed),
                                    T.data_ptr(), meta.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes, _stream()),
          "imf_ransac_registration")
    it, inl, nvalid = meta.tolist()
    fit, rmse = stats.tolist()
    return T.cpu().numpy().reshape(4, 4), it, inl, nvalid, fit, rmse


def run_ransac(xyz0, xyz1, feat0, feat1, voxel_size, ransac_n=4, seed=0, device="cuda"):
    """scripts/benchmark_util.py:16-34: feature correspondences (nearest xyz1 feature of every xyz0
    point), then RANSAC with the edge-length (0.9) and distance (1.5 voxel) checkers, 50 000
    hypotheses.  Returns the 4x4 transformation xyz0 -> xyz1 like `result_ransac.transformation`."""
    f0, f1 = _descs(feat0, device, "feat0"), _descs(feat1, device, "feat1")
    corres = nn_search(f0, f1)
    return ransac_registration(xyz0, xyz1, corres, ransac_n=ransac_n, max_corr_dist=voxel_size * 1.5,
                               edge_similarity=0.9, max_iter=50000, seed=seed, device=device)[0]


def _points(x, device, name):
    t = torch.as_tensor(x).to(device=device, dtype=torch.float64).contiguous()
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] == 0:
        raise ImfError(f"{name} must be [n>0, 3], got {tuple(t.shape)}")
    return t


def _host_T(T):
    if T is None:
        return None
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4))


def _icp(name, src, dst, normals, max_corr_dist, init, max_iteration, device):
    """Both ICP entry points: normals None = imf_icp_point_to_point, else imf_icp_point_to_plane."""
    s = _points(src, device, "src")
    d = _points(dst, s.device, "dst")
    L = _lib.lib()
    if normals is None:
        nbytes = L.imf_icp_workspace_bytes(s.shape[0], d.shape[0])
    else:
        nrm = _points(normals, s.device, "dst_normals")
        if nrm.shape != d.shape:
            raise ImfError(f"{name}: dst_normals {tuple(nrm.shape)} for dst {tuple(d.shape)}")
        nbytes = L.imf_icp_plane_workspace_bytes(s.shape[0], d.shape[0])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    T = torch.empty(16, dtype=torch.float64, device=s.device)
    stats = torch.empty(2, dtype=torch.float64, device=s.device)
    meta = torch.zeros(3, dtype=torch.int32, device=s.device)
    init = _host_T(init)
    tail = (float(max_corr_dist), init.ctypes.data_as(C.c_void_p) if init is not None else None, int(max_iteration),
            T.data_ptr(), stats.data_ptr(), meta.data_ptr(), ws.data_ptr(), nbytes, _stream())
    if normals is None:
        check(L.imf_icp_point_to_point(s.data_ptr(), s.shape[0], d.data_ptr(), d.shape[0], *tail), "imf_" + name)
    else:
        check(L.imf_icp_point_to_plane(s.data_ptr(), s.shape[0], d.data_ptr(), nrm.data_ptr(), d.shape[0], *tail),
              "imf_" + name)
    iters, n_corr, err = meta.tolist()
    if err:
        raise ImfError(f"{name}: a target point is NaN or beyond the grid's range")
    fitness, rmse = stats.tolist()
    return T.cpu().numpy().reshape(4, 4), fitness, rmse, iters, n_corr


def icp_point_to_point(src, dst, max_corr_dist, init=None, max_iteration=200, device="cuda"):
    """Open3D 0.12 registration_icp(src, dst, max_corr_dist, init, TransformationEstimationPointToPoint(),
    ICPConvergenceCriteria(max_iteration)) on the device (imf_icp_point_to_point; the loop is restated in
    csrc/icp.hip).  Returns (T 4x4 numpy source->target, fitness, inlier RMSE, iterations run, correspondences)."""
    return _icp("icp_point_to_point", src, dst, None, max_corr_dist, init, max_iteration, device)


def icp_point_to_plane(src, dst, dst_normals, max_corr_dist, init=None, max_iteration=30, device="cuda"):
    """Open3D registration_icp(src, dst, max_corr_dist, init, TransformationEstimationPointToPlane(),
    ICPConvergenceCriteria(max_iteration)) on the device (imf_icp_point_to_plane; restated in csrc/icp.hip).  dst_normals:
    [n_dst, 3], row j the normal of dst row j.  Returns what icp_point_to_point returns: (T 4x4 numpy source->target,
    fitness, inlier RMSE over point distances, iterations run, correspondences)."""
    if dst_normals is None:
        raise ImfError("icp_point_to_plane: dst_normals is required")
    return _icp("icp_point_to_plane", src, dst, dst_normals, max_corr_dist, init, max_iteration, device)


def intensity(rgb):
    """The intensity coloured ICP reads: (r + g + b) / 765 in float64 from uint8 colours [n, 3] -- the integer sum first,
    then one division -- in [0, 1].  Host only."""
    c = np.asarray(rgb)
    if c.dtype != np.uint8 or c.ndim != 2 or c.shape[1] != 3:
        raise ImfError(f"intensity: colours must be uint8 [n, 3], got {c.dtype} {c.shape}")
    return c.astype(np.int64).sum(1).astype(np.float64) / 765.0


def _scalars(x, n, device, name):
    t = torch.as_tensor(x).to(device=device, dtype=torch.float64).contiguous()
    if t.shape != (n,):
        raise ImfError(f"{name} must be [{n}], got {tuple(t.shape)}")
    return t


def _color_gradient_device(p, nrm, inten, nbr, counts):
    """imf_color_gradient on device tensors; returns the device float64 [n, 3] tensor."""
    n, knn = p.shape[0], nbr.shape[1]
    out = torch.empty((n, 3), dtype=torch.float64, device=p.device)
    check(_lib.lib().imf_color_gradient(p.data_ptr(), nrm.data_ptr(), inten.data_ptr(), nbr.data_ptr(), counts.data_ptr(),
                                        n, knn, out.data_ptr(), _stream()), "imf_color_gradient")
    return out


def color_gradient(points, normals, intensity, neighbors, counts, device="cuda"):
    """The colour gradient of a cloud for coloured ICP (imf_color_gradient; the rule is stated in csrc/colored_icp.hip):
    per point the least-squares gradient of `intensity` [n] over its neighbour list, pinned into the tangent plane of its
    normal.  neighbors int32 [n, knn <= 64] and counts int32 [n] are `estimate_normals(..., return_neighbors=True)`'s.
    Returns float64 numpy [n, 3]; 0 where a list has fewer than 4 entries or the system is singular."""
    p = _points(points, device, "points")
    n = p.shape[0]
    nrm = _points(normals, p.device, "normals")
    if nrm.shape != p.shape:
        raise ImfError(f"color_gradient: normals {tuple(nrm.shape)} for points {tuple(p.shape)}")
    inten = _scalars(intensity, n, p.device, "intensity")
    nbr = torch.as_tensor(neighbors).to(device=p.device, dtype=torch.int32).contiguous()
    if nbr.dim() != 2 or nbr.shape[0] != n or not 1 <= nbr.shape[1] <= 64:
        raise ImfError(f"color_gradient: neighbors must be [{n}, 1..64], got {tuple(nbr.shape)}")
    cnt = torch.as_tensor(counts).to(device=p.device, dtype=torch.int32).contiguous()
    if cnt.shape != (n,):
        raise ImfError(f"color_gradient: counts must be [{n}], got {tuple(cnt.shape)}")
    return _color_gradient_device(p, nrm, inten, nbr, cnt).cpu().numpy()


def icp_colored(src, src_intensity, dst, dst_normals, dst_intensity, max_corr_dist, init=None, max_iteration=30,
                lambda_geometric=0.968, dst_gradient=None, gradient_knn=30, gradient_radius=None, device="cuda"):
    """Open3D registration_colored_icp(src, dst, max_corr_dist, init, TransformationEstimationForColoredICP(
    lambda_geometric), ICPConvergenceCriteria(max_iteration)) on the device (imf_icp_colored; restated in
    csrc/colored_icp.hip).  src_intensity [n_src] and dst_intensity [n_dst] are `intensity` of the rows' colours;
    dst_normals [n_dst, 3] are the caller's.  dst_gradient: `color_gradient` of the target, or None = computed here over
    the lists of `estimate_normals(dst, knn=gradient_knn, max_radius=gradient_radius or 2 max_corr_dist,
    return_neighbors=True)` (Open3D's hybrid search of twice the distance; that call's normals are discarded).  Returns what the other ICPs return: (T 4x4 numpy
    source->target, fitness, inlier RMSE over point distances, iterations run, correspondences)."""
    if dst_normals is None:
        raise ImfError("icp_colored: dst_normals is required")
    s = _points(src, device, "src")
    d = _points(dst, s.device, "dst")
    nrm = _points(dst_normals, s.device, "dst_normals")
    if nrm.shape != d.shape:
        raise ImfError(f"icp_colored: dst_normals {tuple(nrm.shape)} for dst {tuple(d.shape)}")
    si = _scalars(src_intensity, s.shape[0], s.device, "src_intensity")
    di = _scalars(dst_intensity, d.shape[0], s.device, "dst_intensity")
    if dst_gradient is None:
        _, counts, nbr = estimate_normals(d, knn=int(gradient_knn), max_radius=gradient_radius or 2.0 * max_corr_dist,
                                          device=s.device, return_neighbors=True)
        grad = _color_gradient_device(d, nrm, di, torch.as_tensor(nbr).to(s.device).contiguous(),
                                      torch.as_tensor(counts).to(s.device).contiguous())
    else:
        grad = _points(dst_gradient, s.device, "dst_gradient")
        if grad.shape != d.shape:
            raise ImfError(f"icp_colored: dst_gradient {tuple(grad.shape)} for dst {tuple(d.shape)}")
    L = _lib.lib()
    nbytes = L.imf_icp_colored_workspace_bytes(s.shape[0], d.shape[0])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    T = torch.empty(16, dtype=torch.float64, device=s.device)
    stats = torch.empty(2, dtype=torch.float64, device=s.device)
    meta = torch.zeros(3, dtype=torch.int32, device=s.device)
    init = _host_T(init)
    check(L.imf_icp_colored(s.data_ptr(), si.data_ptr(), s.shape[0], d.data_ptr(), nrm.data_ptr(), di.data_ptr(),
                            grad.data_ptr(), d.shape[0], float(max_corr_dist), float(lambda_geometric),
                            init.ctypes.data_as(C.c_void_p) if init is not None else None, int(max_iteration), T.data_ptr(),
                            stats.data_ptr(), meta.data_ptr(), ws.data_ptr(), nbytes, _stream()), "imf_icp_colored")
    iters, n_corr, err = meta.tolist()
    if err:
        raise ImfError("icp_colored: a target point is NaN or beyond the grid's range")
    fitness, rmse = stats.tolist()
    return T.cpu().numpy().reshape(4, 4), fitness, rmse, iters, n_corr


def information_matrix(src, dst, T=None, max_corr_dist=0.0375, device="cuda"):
    """Open3D get_information_matrix_from_point_clouds(src, dst, max_corr_dist, T) on the device (imf_information_matrix;
    the rules are restated in csrc/information.hip): the sum of G^T G over ICP's correspondences of T . src in dst, G =
    [-[q]x | I] of the target point q, rotation first -- the matrix of a gt.info record and the weight of a pose-graph
    edge.  Returns (6x6 float64 numpy, exactly symmetric, the number of correspondences)."""
    s = _points(src, device, "src")
    d = _points(dst, s.device, "dst")
    L = _lib.lib()
    nbytes = L.imf_information_workspace_bytes(s.shape[0], d.shape[0])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    info = torch.empty(36, dtype=torch.float64, device=s.device)
    meta = torch.zeros(2, dtype=torch.int32, device=s.device)
    Th = _host_T(T)
    check(L.imf_information_matrix(s.data_ptr(), s.shape[0], d.data_ptr(), d.shape[0],
                                   Th.ctypes.data_as(C.c_void_p) if Th is not None else None, float(max_corr_dist),
                                   info.data_ptr(), meta.data_ptr(), ws.data_ptr(), nbytes, _stream()),
          "imf_information_matrix")
    n_corr, err = meta.tolist()
    if err:
        raise ImfError("information_matrix: a target point is NaN or beyond the grid's range")
    return info.cpu().numpy().reshape(6, 6), n_corr


def estimate_normals(points, knn=30, max_radius=0.1, viewpoint=None, device="cuda", return_neighbors=False):
    """o3d.geometry.PointCloud.estimate_normals(KDTreeSearchParamKNN(knn)) on the device, exactly (imf_estimate_normals;
    the rules are stated in csrc/normals.hip): the PCA normal of every point's knn nearest cloud points within max_radius,
    itself included.  viewpoint: 3 numbers the normals face, or None = the largest component positive.  Returns (normals
    float64 numpy [n, 3], counts int32 numpy [n]) and, with return_neighbors=True, the neighbour lists int32 [n, knn]
    in (d^2, index) order padded with -1."""
    p = _points(points, device, "points")
    n = p.shape[0]
    vp = None
    if viewpoint is not None:
        vp = np.ascontiguousarray(np.asarray(viewpoint, dtype=np.float64).reshape(3))
    L = _lib.lib()
    nbytes = L.imf_normals_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    normals = torch.empty((n, 3), dtype=torch.float64, device=p.device)
    counts = torch.empty(n + 1, dtype=torch.int32, device=p.device)          # [n] the error flag
    nbr = torch.empty((n, int(knn)), dtype=torch.int32, device=p.device) if return_neighbors else None
    check(L.imf_estimate_normals(p.data_ptr(), n, int(knn), float(max_radius),
                                 vp.ctypes.data_as(C.c_void_p) if vp is not None else None, normals.data_ptr(),
                                 counts.data_ptr(), nbr.data_ptr() if return_neighbors else None, counts[n:].data_ptr(),
                                 ws.data_ptr(), nbytes, _stream()), "imf_estimate_normals")
    counts = counts.cpu().numpy()
    if counts[n]:
        raise ImfError("estimate_normals: a point is NaN or beyond the grid's range")
    out = (normals.cpu().numpy(), counts[:n].copy())
    return out + (nbr.cpu().numpy(),) if return_neighbors else out


def compute_fpfh(points, normals=None, radius=0.125, max_nn=64, normal_knn=30, normal_radius=None, viewpoint=None,
                 width=33, device="cuda", return_hist=False):
    """o3d.pipelines.registration.compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)) on the device
    (imf_fpfh_features; the rules are stated in csrc/fpfh.hip): the 33-bin Fast Point Feature Histogram of every point
    over its max_nn nearest cloud points within radius, the lists being `estimate_normals(points, knn=max_nn,
    max_radius=radius, return_neighbors=True)`.  normals: [n, 3], or None = `estimate_normals(knn=normal_knn,
    max_radius=normal_radius or radius, viewpoint=viewpoint)`.  width: 33, or 64 = zero-padded to a width `nn_search`
    takes (the distances are the same).  Returns a float32 device tensor [n, width] and, with return_hist=True, the int32
    device tensor [n, 33] of the SPFH pair counts."""
    if not 1 <= int(max_nn) <= 64:
        raise ImfError(f"compute_fpfh: max_nn={max_nn}, expected 1..64")
    if width not in (33, 64):
        raise ImfError(f"compute_fpfh: width={width}, expected 33 or 64")
    p = _points(points, device, "points")
    n = p.shape[0]
    _, counts, nbr = estimate_normals(p, knn=int(max_nn), max_radius=radius, device=p.device, return_neighbors=True)
    if normals is None:
        normals, _ = estimate_normals(p, knn=normal_knn, max_radius=normal_radius or radius, viewpoint=viewpoint,
                                      device=p.device)
    nrm = _points(normals, p.device, "normals")
    if nrm.shape != p.shape:
        raise ImfError(f"compute_fpfh: normals {tuple(nrm.shape)} for points {tuple(p.shape)}")
    nbr = torch.as_tensor(nbr).to(p.device).contiguous()
    counts = torch.as_tensor(counts).to(p.device).contiguous()
    L = _lib.lib()
    nbytes = L.imf_fpfh_workspace_bytes(n, int(max_nn))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    out = torch.empty((n, width), dtype=torch.float32, device=p.device)
    hist = torch.empty((n, 33), dtype=torch.int32, device=p.device) if return_hist else None
    check(L.imf_fpfh_features(p.data_ptr(), nrm.data_ptr(), n, nbr.data_ptr(), counts.data_ptr(), int(max_nn), int(width),
                              out.data_ptr(), hist.data_ptr() if return_hist else None, ws.data_ptr(), nbytes, _stream()),
          "imf_fpfh_features")
    return (out, hist) if return_hist else out


def radius_count(src, dst, T=None, r=0.45, per_point=False, device="cuda"):
    """len(get_matching_indices(src, dst, T, r)) of util/pointcloud.py:56-69: the number of pairs (i, j) with
    |T src_i - dst_j| <= r (imf_radius_count).  Returns the int count, or (count, int32 numpy [n_src] per-point
    counts) with per_point=True."""
    s = _points(src, device, "src")
    d = _points(dst, s.device, "dst")
    L = _lib.lib()
    nbytes = L.imf_radius_count_workspace_bytes(d.shape[0])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    out = torch.zeros(2, dtype=torch.int64, device=s.device)       # [0] count, [1] the error flag (low word)
    pp = torch.empty(s.shape[0], dtype=torch.int32, device=s.device) if per_point else None
    Th = _host_T(T)
    check(L.imf_radius_count(s.data_ptr(), s.shape[0], d.data_ptr(), d.shape[0],
                             Th.ctypes.data_as(C.c_void_p) if Th is not None else None, float(r), out.data_ptr(),
                             pp.data_ptr() if per_point else None, out[1:].data_ptr(), ws.data_ptr(), nbytes,
                             _stream()), "imf_radius_count")
    count, err = out.tolist()
    if err & 0xFFFFFFFF:
        raise ImfError("radius_count: a target point is NaN or beyond the grid's range")
    return (int(count), pp.cpu().numpy()) if per_point else int(count)


def _pair_points(x, device, name):
    t = torch.as_tensor(x).to(device=device, dtype=torch.float64)
    if t.numel() == 0:
        t = t.reshape(0, 3)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ImfError(f"{name} must be [n, 3], got {tuple(t.shape)}")
    return t.contiguous()


def radius_pairs_call(s, d, Th, r, capacity):
    """One imf_radius_pairs call on device fp64 points.  Returns (pairs int32 [capacity, 2], offsets int64
    [n_src+1], total, err); the pairs are written only when total <= capacity."""
    L = _lib.lib()
    n_src, n_dst = s.shape[0], d.shape[0]
    nbytes = L.imf_radius_pairs_workspace_bytes(n_src, n_dst)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device) if nbytes else None
    offsets = torch.empty(n_src + 1, dtype=torch.int64, device=s.device)
    pairs = torch.empty((capacity, 2), dtype=torch.int32, device=s.device)
    out = torch.zeros(2, dtype=torch.int64, device=s.device)       # [0] total, [1] the error flag (low word)
    check(L.imf_radius_pairs(s.data_ptr() if n_src else None, n_src, d.data_ptr() if n_dst else None, n_dst,
                             Th.ctypes.data_as(C.c_void_p) if Th is not None else None, float(r), offsets.data_ptr(),
                             pairs.data_ptr() if capacity else None, int(capacity), out.data_ptr(), out[1:].data_ptr(),
                             ws.data_ptr() if ws is not None else None, nbytes, _stream()), "imf_radius_pairs")
    total, err = out.tolist()
    return pairs, offsets, int(total), err & 0xFFFFFFFF


def radius_pairs(src, dst, T=None, r=None, device="cuda", capacity=None):
    """get_matching_indices(src, dst, T, r) of util/pointcloud.py:56-69 on the device (imf_radius_pairs): every (i, j)
    with |T src_i - dst_j| <= r.  Returns (pairs int32 CUDA [P, 2] = (i, j), offsets int64 CUDA [n_src+1], the CSR row
    start of every source point).  Within a row j ascends (FLANN orders by distance; the set is the same).  One host
    read per call; a second call when the first guess of the capacity (32 pairs per source point) was too small."""
    if r is None:
        raise ImfError("radius_pairs: r is required")
    s = _pair_points(src, device, "src")
    d = _pair_points(dst, s.device, "dst")
    Th = _host_T(T)
    cap = int(capacity) if capacity is not None else 32 * s.shape[0]
    pairs, offsets, total, err = radius_pairs_call(s, d, Th, r, cap)
    if err:
        raise ImfError("radius_pairs: a target point is NaN or beyond the grid's range")
    if total > cap:
        pairs, offsets, total, err = radius_pairs_call(s, d, Th, r, total)
    return pairs[:total], offsets


def robust_transform_device(p0, p1, weight=None):
    """One imf_robust_transform launch on device fp64 tensors [n, 3] (weight: device fp64 [n] or None).  Returns the
    device buffer of 136 bytes: 16 doubles of T (row-major 4x4), then the int32 flag.  No host synchronisation."""
    for name, t in (("pts0", p0), ("pts1", p1)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == 3
                and t.is_contiguous()):
            raise ImfError(f"robust_transform_device: {name} must be a contiguous CUDA float64 [n, 3] tensor")
    if p1.shape != p0.shape or p1.device != p0.device:
        raise ImfError(f"robust_transform_device: pts0 {tuple(p0.shape)} on {p0.device}, pts1 {tuple(p1.shape)} on {p1.device}")
    if weight is not None and not (torch.is_tensor(weight) and weight.device == p0.device and weight.is_contiguous()
                                   and weight.dtype == torch.float64 and weight.shape == (p0.shape[0],)):
        raise ImfError(f"robust_transform_device: weight must be a contiguous float64 [{p0.shape[0]}] tensor on {p0.device}")
    L = _lib.lib()
    n, dev = p0.shape[0], p0.device
    nbytes = L.imf_robust_transform_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    out = torch.empty(136, dtype=torch.uint8, device=dev)
    check(L.imf_robust_transform(p0.data_ptr() if n else None, p1.data_ptr() if n else None,
                                 weight.data_ptr() if weight is not None and n else None, n, out.data_ptr(),
                                 out[128:].data_ptr(), ws.data_ptr() if ws is not None else None, nbytes,
                                 torch.cuda.current_stream(dev).cuda_stream), "imf_robust_transform")
    return out


def robust_transform(pts0, pts1, weight=None, device="cuda"):
    """util/transform_estimation.py:89-116 est_quad_linear_robust(pts0, pts1, weight) on the device, in fp64
    (imf_robust_transform; the loop is restated in csrc/robust.hip): the transform that takes pts0 [n, 3] onto its
    correspondences pts1 [n, 3] after 20 reweighted rounds.  Returns (T float64 4x4 numpy, ok); ok is False and T the
    identity when a round's system could not be solved (upstream raises).  One device-to-host copy per call."""
    p0 = _pair_points(pts0, device, "pts0")
    p1 = _pair_points(pts1, p0.device, "pts1")
    if p0.shape != p1.shape:
        raise ImfError(f"robust_transform: pts0 {tuple(p0.shape)} and pts1 {tuple(p1.shape)} differ")
    w = None
    if weight is not None:
        w = torch.as_tensor(weight).to(device=p0.device, dtype=torch.float64).reshape(-1).contiguous()
        if w.shape[0] != p0.shape[0]:
            raise ImfError(f"robust_transform: {w.shape[0]} weights for {p0.shape[0]} pairs")
    raw = robust_transform_device(p0, p1, w).cpu().numpy()
    return raw[:128].view(np.float64).reshape(4, 4).copy(), not bool(raw[128:].view(np.int32)[0])
