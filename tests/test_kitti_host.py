"""The KITTI evaluator's host side (imfnet_amd/kitti.py, evaluate_kitti.py) against literal restatements of
lib/data_loaders.py:527-556, :655-713 and scripts/evaluation_kitti_open3d_12.py:116-150.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from kitti_restate import poses_text, reference_pairs


def _positions(steps):
    """Poses whose translations advance by `steps[k]` metres along x at frame k (rotation: identity)."""
    x = np.concatenate([[0.0], np.cumsum(steps)])
    P = np.tile(np.eye(4), (len(x), 1, 1))
    P[:, 0, 3] = x
    return P


def _tricky_positions():
    # the scans start at frame 15; frames 15-58 crawl and frame 59 jumps more than 10 m away (first hit 44 -> the pair
    # (8, 15, 58) through the `- 1` offset, the pair the reference drops), then 0.3 m steps, then a stall whose
    # windows are empty
    steps = [0.05] * 15 + [0.01] * 43 + [12.0] + [0.3] * 60 + [0.0] * 30
    return _positions(steps)


def test_pair_list_matches_reference_restatement(tmp_path):
    from imfnet_amd import kitti as K
    P = _tricky_positions()
    inames = list(range(15, len(P)))
    got = K.pairs_of_sequence(8, inames, P)
    ref = reference_pairs(8, inames, P)
    assert (8, 15, 58) not in ref
    assert (8, 15, 58) in got                             # the per-sequence list still has it: pair_list drops it
    assert [g for g in got if g != (8, 15, 58)] == ref
    # the `- 1` offset: the pair's second frame is one before the first frame beyond 10 m
    Ts = P[:, :3, 3]
    for _, t0, t1 in ref:
        d = np.linalg.norm(Ts[t0 + 1:t0 + 100] - Ts[t0], axis=1)
        assert t1 == t0 + int(np.argmax(d > 10))          # first hit h (>= 1) -> h + t0 - 1 = t0 + (index in t0+1..)
    # the whole tree: sequence file layout, sorted frame names, the dropped pair
    vd = tmp_path / "dataset" / "sequences" / "08" / "velodyne"
    vd.mkdir(parents=True)
    for t in inames:
        (vd / ("%06d.bin" % t)).write_bytes(b"")
    (tmp_path / "dataset" / "poses").mkdir(parents=True)
    (tmp_path / "dataset" / "poses" / "08.txt").write_text(poses_text(P))
    assert K.pair_list(str(tmp_path), [8]) == ref


def test_pair_list_empty_window_advances_by_one():
    from imfnet_amd import kitti as K
    P = _positions([0.01] * 150 + [20.0] + [0.01] * 10)
    inames = list(range(len(P)))
    assert K.pairs_of_sequence(9, inames, P) == reference_pairs(9, inames, P)
    assert K.pairs_of_sequence(9, inames, P)[0][1] == 52  # frame 151 jumps: frames 0..51 have empty windows


def test_pose_from_positions_matches_reference_formula():
    from imfnet_amd import kitti as K
    rng = np.random.default_rng(3)
    R = np.array([7.533745e-03, -9.999714e-01, -6.166020e-04, 1.480249e-02, 7.280733e-04, -9.998902e-01,
                  9.998621e-01, 7.523790e-03, 1.480755e-02]).reshape(3, 3)
    T = np.array([-4.069766e-03, -7.631618e-02, -2.717806e-01]).reshape(3, 1)
    velo2cam = np.vstack((np.hstack([R, T]), [0, 0, 0, 1])).T
    for _ in range(3):
        q0, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        q1, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        P0, P1 = np.eye(4), np.eye(4)
        P0[:3, :3], P1[:3, :3] = q0, q1
        P0[:3, 3], P1[:3, 3] = rng.uniform(-50, 50, 3), rng.uniform(-50, 50, 3)
        M = (velo2cam @ P0.T @ np.linalg.inv(P1.T) @ np.linalg.inv(velo2cam)).T
        assert np.array_equal(K.pose_from_positions(P0, P1), M)


def test_reference_icp_cache_is_used(tmp_path, monkeypatch):
    from imfnet_amd import kitti as K
    M2 = np.arange(16, dtype=np.float64).reshape(4, 4) / 7.0
    (tmp_path / "icp").mkdir()
    np.save(str(tmp_path / "icp" / "8_10_20.npy"), M2)      # what the reference's np.save(filename, M2) writes

    def boom(*a, **k):
        raise AssertionError("ICP must not run when the cache file exists")
    monkeypatch.setattr(K, "refine_ground_truth", boom)
    got, computed = K.ground_truth(str(tmp_path), 8, 10, 20, None, None, None)
    assert not computed and np.array_equal(got, M2)


def test_new_cache_file_is_written_atomically(tmp_path, monkeypatch):
    from imfnet_amd import kitti as K
    M2 = np.eye(4) * 2.0
    monkeypatch.setattr(K, "refine_ground_truth", lambda *a, **k: (M2, None))
    P = np.tile(np.eye(4), (30, 1, 1))
    got, computed = K.ground_truth(str(tmp_path), 9, 1, 25, None, None, P)
    assert computed and np.array_equal(got, M2)
    assert sorted(os.listdir(tmp_path / "icp")) == ["9_1_25.npy"]
    assert np.array_equal(np.load(str(tmp_path / "icp" / "9_1_25.npy")), M2)


def _reference_metrics(T_ransac64, T_gt64):
    """scripts/evaluation_kitti_open3d_12.py:116-128 literally."""
    T_ransac = torch.from_numpy(T_ransac64.astype(np.float32))
    T_gth = torch.from_numpy(T_gt64).float()
    rte = np.linalg.norm(T_ransac[:3, 3] - T_gth[:3, 3])
    rre = np.arccos((np.trace(T_ransac[:3, :3].t() @ T_gth[:3, :3]) - 1) / 2)
    return rte, rre


class _RefMeter:                                          # lib/timer.py:4-24
    def __init__(self):
        self.sum = self.sq_sum = 0.0
        self.count = 0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count
        self.sq_sum += val ** 2 * n
        self.var = self.sq_sum / self.count - self.avg ** 2


def test_metrics_match_reference_float32_expressions():
    from imfnet_amd import kitti as K
    from kitti_restate import rigid
    rng = np.random.default_rng(7)
    T_gt = rigid(10.0, [0.1, 0.2, 1.0], [12.0, -1.0, 0.3])
    nan_pose, g = None, np.random.default_rng(0)
    while nan_pose is None:                                # an estimate equal to the truth whose float32 trace exceeds 3
        T = rigid(g.uniform(0, 90), g.standard_normal(3), [1, 2, 3])
        if np.isnan(_reference_metrics(T, T)[1]):
            nan_pose = T
    cases = [(nan_pose, nan_pose), (T_gt, T_gt),
             rigid(0.5, [1, 0, 0], [0.2, 0.1, 0]) @ T_gt,
             rigid(3.0, [0, 1, 1], [1.5, 0.0, 0.0]) @ T_gt,
             rigid(30.0, [0, 0, 1], [0.1, 0, 0]) @ T_gt,
             rigid(1.0, [1, 1, 0], [4.0, 0, 0]) @ T_gt]
    for _ in range(20):
        cases.append(rigid(rng.uniform(0, 8), rng.standard_normal(3), rng.uniform(-3, 3, 3)) @ T_gt)
    cases = [c if isinstance(c, tuple) else (c, T_gt) for c in cases]
    meters, ref_s, ref_rte, ref_rre = K.KittiMeters(), _RefMeter(), _RefMeter(), _RefMeter()
    n_nan = 0
    for T, T_gt in cases:
        rte, rre = K.pair_errors(T, T_gt)
        r_rte, r_rre = _reference_metrics(T, T_gt)
        assert rte == r_rte and (rre == r_rre or (np.isnan(rre) and np.isnan(r_rre)))
        ok = meters.update(rte, rre)
        if r_rte < 2:
            ref_rte.update(r_rte)
        if not np.isnan(r_rre) and r_rre < np.pi / 180 * 5:
            ref_rre.update(r_rre)
        ref_ok = r_rte < 2 and not np.isnan(r_rre) and r_rre < np.pi / 180 * 5
        ref_s.update(1 if ref_ok else 0)
        assert ok == ref_ok
        n_nan += int(np.isnan(r_rre))
    assert n_nan >= 1, "the float32 NaN RRE case is missing"
    s = meters.summary()
    assert s["pairs"] == ref_s.count and s["successes"] == ref_s.sum and s["rate"] == ref_s.avg
    assert s["rte_mean"] == ref_rte.avg and s["rte_var"] == ref_rte.var
    assert s["rre_mean"] == ref_rre.avg and s["rre_var"] == ref_rre.var
    assert s["nan_rre"] == n_nan


def test_empty_meters_report_null():
    from imfnet_amd import kitti as K
    from imfnet_amd.evaluate_kitti import summarize
    m = K.KittiMeters()
    m.update(np.float32(5.0), np.float32(np.nan))          # a failure of both kinds: both error meters stay empty
    s = m.summary()
    assert s["rte_mean"] is None and s["rre_var"] is None and s["rate"] == 0.0 and s["nan_rre"] == 1
    s2 = summarize(["8 0 12 20 skipped"])
    assert s2["pairs"] == 0 and s2["skipped"] == 1 and s2["rate"] is None
    json.dumps(s2)


def test_pair_line_round_trips_through_summary():
    from imfnet_amd.evaluate_kitti import pair_line, summarize
    from imfnet_amd import kitti as K
    rows = [dict(drive=8, t0=0, t1=10, n_matches=5000, skipped=False, rte=0.25, rre=0.01, success=True),
            dict(drive=8, t0=11, t1=20, n_matches=10, skipped=True),
            dict(drive=8, t0=21, t1=30, n_matches=4000, skipped=False, rte=3.5, rre=float("nan"), success=False)]
    lines = [pair_line(r) for r in rows]
    s = summarize(lines)
    assert s["pairs"] == 2 and s["skipped"] == 1 and s["successes"] == 1 and s["nan_rre"] == 1
    m = K.KittiMeters()
    m.update(np.float32(0.25), np.float32(0.01))
    m.update(np.float32(3.5), np.float32("nan"))
    assert s["rte_mean"] == m.summary()["rte_mean"]


def test_icp_restatement_recovers_a_known_offset():
    """The CPU restatement the GPU test holds the device ICP to: it recovers a 0.5 m / 3 deg offset."""
    pytest.importorskip("scipy")
    from kitti_restate import icp_restated, rigid, scene_points
    rng = np.random.default_rng(1)
    dst = scene_points(rng, 8000).astype(np.float64)
    T_true = rigid(3.0, [0.2, 0.3, 1.0], [0.5, 0.0, 0.0])
    src = (dst - T_true[:3, 3]) @ T_true[:3, :3]             # dst = T_true src
    T, fit, rmse, iters, n = icp_restated(src, dst, 1.0, None, 200)
    assert np.abs(T[:3, 3] - T_true[:3, 3]).max() < 0.01 and iters < 200 and fit > 0.99
