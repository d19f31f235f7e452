"""CPU restatements for the KITTI evaluation tests (plain helper module, imported by test_kitti_host.py and
test_gpu_kitti.py): the reference's pair loop written out literally, Open3D's point-to-point ICP loop on
scipy's cKDTree, and a synthetic odometry tree."""
import os

import numpy as np


def reference_pairs(drive, inames, all_pos, min_dist=10):
    """lib/data_loaders.py:660-682 and :706-712, line for line, on given poses (the empty-window branch made explicit:
    `next_time` stays an empty array there, and `empty in inames` is False)."""
    files = []
    Ts = all_pos[:, :3, 3]
    pdist = (Ts.reshape(1, -1, 3) - Ts.reshape(-1, 1, 3)) ** 2
    pdist = np.sqrt(pdist.sum(-1))
    valid_pairs = pdist > min_dist
    curr_time = inames[0]
    while curr_time in inames:
        next_time = np.where(valid_pairs[curr_time][curr_time:curr_time + 100])[0]
        if len(next_time) == 0:
            curr_time += 1
            found = False
        else:
            next_time = next_time[0] + curr_time - 1
            found = True
        if found and next_time in inames:
            files.append((drive, curr_time, next_time))
            curr_time = next_time + 1
    for item in [(8, 15, 58)]:
        if item in files:
            files.pop(files.index(item))
    return files


def poses_text(positions):
    """KITTI poses file: one 3x4 row-major matrix per line."""
    return "".join(" ".join(f"{v:.9e}" for v in P[:3].reshape(-1)) + "\n" for P in positions)


def icp_restated(src, dst, r, init=None, max_iteration=200, nearest=None, rotation=None):
    """Open3D 0.12 RegistrationICP, point-to-point, relative fitness / rmse 1e-6, on cKDTree (distance_upper_bound=r:
    strict).  Returns (T, fitness, rmse, iterations, n_corr).  The update's rotation follows the rank rule of
    imf_oracle.rigid_rotation (full rank: the SVD answer, unchanged).  `nearest(p) -> (ok bool [n], j int [n], d2 [n])`
    replaces the cKDTree search (registration_cases.nearest_brute: ties to the lowest target index); `rotation(H) -> R`
    replaces the rotation of the update (the tests pass the plain SVD formula to show that full rank is unchanged)."""
    import imf_oracle as O
    rotation = rotation or O.rigid_rotation
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    if nearest is None:
        from scipy.spatial import cKDTree
        tree = cKDTree(dst)

        def nearest(p):
            d, j = tree.query(p, k=1, distance_upper_bound=r)
            ok = np.isfinite(d)
            return ok, np.where(ok, j, 0), np.where(ok, d, 0.0) ** 2
    T = np.eye(4) if init is None else np.array(init, np.float64)
    pcd = src @ T[:3, :3].T + T[:3, 3]

    def corr(p):
        ok, j, d2 = nearest(p)
        n = int(ok.sum())
        fit = n / len(p) if n else 0.0
        rmse = float(np.sqrt(d2[ok].sum() / n)) if n else 0.0
        return np.flatnonzero(ok), j[ok], fit, rmse

    i_s, i_d, fit, rmse = corr(pcd)
    iters = 0
    for it in range(max_iteration):
        if len(i_s):
            S, D = pcd[i_s], dst[i_d]
            ms, md = S.mean(0), D.mean(0)
            H = (S - ms).T @ (D - md)
            R = rotation(H)
            upd = np.eye(4)
            upd[:3, :3] = R
            upd[:3, 3] = md - R @ ms
        else:
            upd = np.eye(4)
        T = upd @ T
        pcd = pcd @ upd[:3, :3].T + upd[:3, 3]
        f0, r0 = fit, rmse
        i_s, i_d, fit, rmse = corr(pcd)
        iters = it + 1
        if abs(f0 - fit) < 1e-6 and abs(r0 - rmse) < 1e-6:
            break
    return T, fit, rmse, iters, len(i_s)


def rigid(deg, axis, t):
    a = np.deg2rad(deg)
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    T[:3, 3] = t
    return T


def scene_points(rng, n, extent=20.0):
    """A street-like scene: ground plane, two walls, a few boxes (well-conditioned for registration)."""
    parts = []
    m = n // 4
    g = rng.uniform(-extent, extent, (m, 3)); g[:, 2] = -1.7 + rng.normal(0, 0.01, m); parts.append(g)
    w1 = rng.uniform(-extent, extent, (m, 3)); w1[:, 1] = 6.0 + rng.normal(0, 0.01, m); w1[:, 2] = rng.uniform(-1.7, 3, m)
    parts.append(w1)
    w2 = rng.uniform(-extent, extent, (m, 3)); w2[:, 0] = -9.0; w2[:, 2] = rng.uniform(-1.7, 3, m); parts.append(w2)
    k = n - 3 * m
    c = rng.uniform(-extent / 2, extent / 2, (8, 3)); c[:, 2] = -1.0
    b = c[rng.integers(0, 8, k)] + rng.uniform(-0.8, 0.8, (k, 3))
    parts.append(b)
    return np.concatenate(parts).astype(np.float32)


def write_tree(root, positions_by_drive, scans_by_drive, image=None):
    """<root>/dataset/poses/%02d.txt, <root>/dataset/sequences/%02d/velodyne/%06d.bin (+ .png beside each)."""
    os.makedirs(os.path.join(root, "dataset", "poses"), exist_ok=True)
    for drive, pos in positions_by_drive.items():
        open(os.path.join(root, "dataset", "poses", "%02d.txt" % drive), "w").write(poses_text(pos))
        vd = os.path.join(root, "dataset", "sequences", "%02d" % drive, "velodyne")
        os.makedirs(vd, exist_ok=True)
        for t, xyz in scans_by_drive[drive].items():
            xyzr = np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], 1).astype(np.float32)
            xyzr.tofile(os.path.join(vd, "%06d.bin" % t))
            if image is not None:
                import shutil
                shutil.copyfile(image, os.path.join(vd, "%06d.png" % t))
