"""The KITTI evaluation on the GPU: the float32-quotient voxel mode, imf_icp_point_to_point against Open3D's loop
restated on cKDTree, imf_radius_count against cKDTree, the evaluator CLI end to end on a synthetic odometry tree, and
the success path of a pair registration."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import imf_oracle as O
from kitti_restate import icp_restated, rigid, scene_points, write_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _straddling_points(rng, vs, n=20000):
    """float32 points on and next to multiples of the voxel, where the float32 and the float64 quotients floor apart."""
    k = rng.integers(-400, 400, (n, 3)).astype(np.float64)
    x = (k * vs).astype(np.float32)
    x = np.nextafter(x, rng.choice([-np.inf, np.inf], x.shape).astype(np.float32))
    return np.concatenate([x, rng.uniform(-60, 60, (n, 3)).astype(np.float32)]).astype(np.float32)


@pytest.mark.parametrize("vs", [0.3, 0.05])
def test_voxelize_f32_quotient_mode(vs):
    from imfnet_amd.kitti import voxelize_f32
    rng = np.random.default_rng(int(vs * 100))
    x = _straddling_points(rng, vs)
    coords, first = voxelize_f32(torch.from_numpy(x).cuda(), vs)
    c = torch.floor(torch.from_numpy(x) / vs).numpy().astype(np.int64)          # the KITTI loader's expression
    c4 = np.concatenate([np.zeros((len(c), 1), np.int64), c], 1)
    inds = O.first_occurrence_unique(O.pack_keys(c4))
    assert np.array_equal(first.cpu().numpy(), inds)
    assert np.array_equal(coords.cpu().numpy(), c4[inds].astype(np.int32))
    c1, i1 = O.voxelize(x.astype(np.float64), vs)                               # mode 1 (float64 quotient)
    assert len(i1) != len(inds) or not np.array_equal(c1, c4[inds].astype(np.int32)), "no row differs from mode 1"


def test_modes_0_and_1_unchanged():
    from imfnet_amd import _lib
    from imfnet_amd._lib import check
    rng = np.random.default_rng(5)
    x = _straddling_points(rng, 0.3, 5000)
    L = _lib.lib()
    for mode, pts in ((0, torch.from_numpy(x)), (1, torch.from_numpy(x.astype(np.float64)))):
        pts = pts.cuda()
        n = pts.shape[0]
        cap = L.imf_hash_capacity(n)
        coords = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        first = torch.empty(n, dtype=torch.int32, device="cuda")
        meta = torch.zeros(2, dtype=torch.int32, device="cuda")
        table = torch.empty(cap * 16, dtype=torch.uint8, device="cuda")
        ws = torch.empty(L.imf_unique_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        check(L.imf_voxelize(pts.data_ptr(), mode, n, 0.3, 0, coords.data_ptr(), first.data_ptr(), meta.data_ptr(),
                             table.data_ptr(), cap, ws.data_ptr(), meta[1:].data_ptr(),
                             torch.cuda.current_stream().cuda_stream), "imf_voxelize")
        m = int(meta[0])
        ref_c, ref_i = O.voxelize(x.astype(np.float64), 0.3)                     # float32 widened == float64 values
        assert np.array_equal(first[:m].cpu().numpy(), ref_i) and np.array_equal(coords[:m].cpu().numpy(), ref_c)


def test_extract_features_quantize_f32_uses_mode_2_voxels(images):
    from imfnet_amd.extract import extract_features
    from imfnet_amd.kitti import voxelize_f32
    from imfnet_amd.model import load_model
    rng = np.random.default_rng(2)
    x = scene_points(rng, 6000)
    sd = O.seeded_state_dict(seed=0, with_unused_image_layers=True)
    model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3,
                                      config=None)
    model.load_state_dict(sd, strict=True)
    model = model.eval().cuda()
    with torch.no_grad():
        xd, F = extract_features(model, x, voxel_size=0.3, device="cuda:0", skip_check=True, image=images[0],
                                 quantize="f32")
    coords, first = voxelize_f32(torch.from_numpy(x).cuda(), 0.3)
    assert np.array_equal(xd, x[first.cpu().numpy()].astype(np.float64))
    F_ref = O.resunet_forward(sd, coords.cpu().numpy(), images[0])
    assert float((F.cpu() - F_ref).abs().max()) < 1e-4


def _icp_case(seed, n=20000, noise=0.002):
    rng = np.random.default_rng(seed)
    dst = scene_points(rng, n).astype(np.float64)
    T_true = rigid(3.0, [0.2, 0.3, 1.0], [0.5, 0.0, 0.0])
    src = (dst - T_true[:3, 3]) @ T_true[:3, :3] + rng.normal(0, noise, dst.shape)     # dst ~ T_true src
    return src, dst, T_true


def test_icp_matches_restatement_and_recovers_offset():
    from imfnet_amd.matching import icp_point_to_point
    src, dst, T_true = _icp_case(11)
    got = icp_point_to_point(src, dst, 1.0, None, 200)
    ref = icp_restated(src, dst, 1.0, None, 200)
    T, fit, rmse, iters, n_corr = got
    assert iters == ref[3] and n_corr == ref[4]
    assert np.abs(T - ref[0]).max() < 1e-9
    assert abs(rmse - ref[2]) <= 1e-9 * ref[2] and fit == ref[1]
    again = icp_point_to_point(src, dst, 1.0, None, 200)
    assert np.array_equal(again[0], T) and again[1:] == got[1:]                           # bit-identical runs
    dR = T[:3, :3] @ T_true[:3, :3].T
    assert np.linalg.norm(T[:3, 3] - T_true[:3, 3]) < 0.01
    assert np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))) < 0.05


def test_icp_kitti_parameters_and_init():
    """0.2 m bound (the ground-truth refinement), a non-identity init, a capped iteration count, and no
    correspondences at all."""
    from imfnet_amd.matching import icp_point_to_point
    src, dst, T_true = _icp_case(12, n=12000)
    init = rigid(2.5, [0.2, 0.3, 1.0], [0.45, 0.02, 0.0])
    for r, init_, it in ((0.2, init, 200), (0.2, init, 3), (0.5, None, 0)):
        T, fit, rmse, iters, n_corr = icp_point_to_point(src, dst, r, init_, it)
        rT, rfit, rrmse, riters, rn = icp_restated(src, dst, r, init_, it)
        assert iters == riters and n_corr == rn and np.abs(T - rT).max() < 1e-9
        assert abs(rmse - rrmse) <= 1e-9 * max(rrmse, 1e-300)
    T, fit, rmse, iters, n_corr = icp_point_to_point(src + 100.0, dst, 0.2, None, 50)
    assert n_corr == 0 and fit == 0.0 and rmse == 0.0 and np.array_equal(T, np.eye(4)) and iters == 1


def test_radius_count_matches_ckdtree():
    from scipy.spatial import cKDTree
    from imfnet_amd.matching import radius_count
    rng = np.random.default_rng(4)
    a = scene_points(rng, 15000).astype(np.float64)
    b = scene_points(rng, 12000).astype(np.float64)
    T = rigid(1.0, [0, 0, 1], [0.2, -0.1, 0.0])
    moved = a @ T[:3, :3].T + T[:3, 3]
    for r in (0.45, 0.075):
        ref = cKDTree(b).query_ball_point(moved, r, return_length=True)
        n, per = radius_count(a, b, T, r, per_point=True)
        assert n == int(ref.sum()) and np.array_equal(per, ref.astype(np.int32))
    # the evaluator's skip: far apart clouds have fewer than 1000 matches
    from imfnet_amd.kitti import MIN_MATCHES
    assert radius_count(a, b + 50.0, T, 0.45) < MIN_MATCHES <= radius_count(a, b, T, 0.45)


def _synthetic_tree(root, n_points=30000):
    """Sequence 8, frames 0-9, 5 m apart along x: pairs (0, 2), (3, 5), (6, 8) (frame 9 is the hit of the last
    window); each scan is one world scene seen from
    its frame (velodyne coordinates through the constant velo2cam), float32 xyz + reflectance, a PNG beside it."""
    from imfnet_amd.kitti import VELO2CAM
    rng = np.random.default_rng(21)
    world = scene_points(rng, 4 * n_points, extent=40.0).astype(np.float64)
    Vc = VELO2CAM.T                                                   # velodyne -> camera
    P = np.tile(np.eye(4), (10, 1, 1))
    for t in range(10):
        P[t, :3, :3] = rigid(0.4 * t, [0, 1, 0], [0, 0, 0])[:3, :3]
        P[t, 0, 3] = 5.0 * t
    scans = {}
    for t in range(10):
        A = np.linalg.inv(P[t] @ Vc)                                  # world (camera 0 frame) -> velodyne t
        local = world @ A[:3, :3].T + A[:3, 3]
        keep = np.linalg.norm(local[:, :2], axis=1) < 30.0
        sel = rng.permutation(np.flatnonzero(keep))[:n_points]
        scans[t] = local[sel].astype(np.float32)
    write_tree(root, {8: P}, {8: scans}, image=os.path.join(ROOT, "tests", "golden", "cloud_bin_0_0.png"))
    return P, scans


def test_evaluate_kitti_cli_end_to_end(tmp_path):
    from imfnet_amd import kitti as K
    from imfnet_amd.evaluate_kitti import build_model, describe, register_pair
    root, out = str(tmp_path / "kitti"), str(tmp_path / "out")
    P, scans = _synthetic_tree(root)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "imfnet_amd.evaluate_kitti", "--kitti_root", root, "--out_root", out,
           "--max_iter", "20000", "--seed", "0"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    summary = json.loads(res.stdout.strip().splitlines()[-1])
    lines = open(os.path.join(out, "kitti_pairs.txt")).read().splitlines()
    assert [tuple(int(v) for v in l.split()[:3]) for l in lines] == [(8, 0, 2), (8, 3, 5), (8, 6, 8)]
    assert sorted(os.listdir(os.path.join(root, "icp"))) == ["8_0_2.npy", "8_3_5.npy", "8_6_8.npy"]
    evaluated = [l.split() for l in lines if l.split()[4] != "skipped"]
    assert summary["pairs"] == len(evaluated) and summary["skipped"] == len(lines) - len(evaluated)
    assert summary["successes"] == sum(int(f[6]) for f in evaluated)
    assert len(evaluated) == 3
    # the refined ground truth: close to the constructed pose (the scans are exact views of one scene)
    for f in evaluated:
        t0, t1 = int(f[1]), int(f[2])
        M2 = np.load(K.icp_cache_path(root, 8, t0, t1))
        M = K.pose_from_positions(P[t0], P[t1])
        assert np.abs(M2 - M).max() < 0.02
    # every pair again in process: descriptors vs the oracle, RANSAC vs the oracle on the GPU's own descriptors
    sd = O.seeded_state_dict(seed=0, with_unused_image_layers=True)
    model = build_model(None, 0, "cuda:0")
    for k, f in enumerate(evaluated):
        t0, t1 = int(f[1]), int(f[2])
        T_gt = np.load(K.icp_cache_path(root, 8, t0, t1))
        img = K.load_image(K.pair_image_paths(root, 8, t0, t1)[0])
        pts, F = [], []
        for t in (t0, t1):
            p_, F_ = describe(model, scans[t], 0.3, img, "cuda:0")
            pts.append(p_)
            F.append(F_.cpu().numpy())
        if k == 0:
            coords, _ = K.voxelize_f32(torch.from_numpy(scans[t0]).cuda(), 0.3)
            F_ref = O.resunet_forward(sd, coords.cpu().numpy(), img)
            assert float(np.abs(F[0] - F_ref.numpy()).max()) < 1e-4
        got = register_pair(pts[0], F[0], pts[1], F[1], 0.3, 20000, 0)
        corres = O.knn_search(F[0], F[1])
        ref = O.ransac_registration(pts[0], pts[1], corres, 4, 0.3, 0.9, 20000, 0)
        assert got[1] == ref[1] and got[2] == ref[2]
        assert np.abs(got[0] - ref[0]).max() < 1e-9
        rte, rre = K.pair_errors(got[0], T_gt)
        assert repr(float(rte)) == f[4] and repr(float(rre)) == f[5]


def test_register_pair_success_path():
    from imfnet_amd import kitti as K
    from imfnet_amd.evaluate_kitti import register_pair
    rng = np.random.default_rng(8)
    xyz0 = scene_points(rng, 4000).astype(np.float64)
    T_gt = rigid(7.0, [0.1, 0.0, 1.0], [9.5, 0.4, 0.1])
    xyz1 = xyz0 @ T_gt[:3, :3].T + T_gt[:3, 3]
    F = rng.standard_normal((len(xyz0), 32)).astype(np.float32)
    F /= np.linalg.norm(F, axis=1, keepdims=True)
    T, it, inl, nvalid, fit, rmse = register_pair(xyz0, F, xyz1, F.copy(), 0.3, 20000, 0)
    rte, rre = K.pair_errors(T, T_gt)
    assert inl == len(xyz0) and rte < 0.05 and K.is_success(rte, rre)
    m = K.KittiMeters()
    assert m.update(rte, rre) and m.summary()["successes"] == 1
