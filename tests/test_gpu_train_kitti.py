"""KITTI training on the GPU (imfnet_amd/train with --dataset KITTINMPairDataset): the data set on a synthetic odometry
tree (pair list, cached ICP ground truth, positive pairs against cKDTree, the scale draw, the skipped pair), the
validation metrics pinned by descriptors that encode the ground-truth correspondence, SGD steps that lower the loss,
and the command line end to end with --resume."""
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from kitti_restate import reference_pairs
from kitti_tree import FAR_FRAME, N_POINTS, build_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
VOXEL = 0.3


def _apply(T, p):
    return p @ T[:3, :3].T + T[:3, 3]


def _voxels_f32(xyz, vs):
    """First-occurrence representatives under the float32 quotient, on the host."""
    q = np.floor(xyz.astype(np.float32) / np.float32(vs)).astype(np.int64)
    _, first = np.unique(q, axis=0, return_index=True)
    return xyz[np.sort(first)]


def _ref_pairs(src, dst, T, r):
    hits = cKDTree(dst).query_ball_point(_apply(T, src), r)
    rows = [np.stack([np.full(len(h), i), np.sort(h)], 1) for i, h in enumerate(hits) if len(h)]
    return np.concatenate(rows).astype(np.int64) if rows else np.zeros((0, 2), np.int64)


@pytest.fixture(scope="module")
def tree(tmp_path_factory, clouds):
    root = tmp_path_factory.mktemp("kitti")
    positions, scans = build_tree(root, clouds)
    return root, positions, scans


def _config(root, **kw):
    from imfnet_amd.train.trainer import parse_config
    c = parse_config(["--dataset", "KITTINMPairDataset", "--kitti_root", str(root)])
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_dataset_pairs_ground_truth_matches_scale_and_skip(tree, caplog):
    from imfnet_amd import kitti as K
    from imfnet_amd.train.data import KITTINMPairDataset
    root, positions, scans = tree
    ds = KITTINMPairDataset("val", [0, 1], _config(root), seed=0, device=DEV)
    assert ds.files == K.pair_list(str(root), [0, 1]) == [(0, 0, 2), (0, 3, 5), (1, 0, 2), (1, 3, 5)]
    assert ds.files == sum((reference_pairs(d, list(range(7)), positions[d]) for d in (0, 1)), [])
    assert not os.path.exists(root / "icp")
    far = ds.files.index((FAR_FRAME[0], 3, FAR_FRAME[1]))
    with caplog.at_level(logging.WARNING, logger="imfnet_amd.train"):
        items = [ds[i] for i in range(len(ds))]
    # the pair 150 m off is skipped and logged with drive, t0, t1; no other pair is
    assert [it is None for it in items] == [i == far for i in range(len(ds))]
    assert list(ds.skipped) == [(1, 3, 5)] and ds.skipped[(1, 3, 5)] < K.MIN_MATCHES and "1, 3, 5" in caplog.text
    assert sorted(os.listdir(root / "icp")) == ["0_0_2.npy", "0_3_5.npy", "1_0_2.npy", "1_3_5.npy"]
    for (drive, t0, t1), it in zip(ds.files, items):
        if it is None:
            continue
        cached = np.load(K.icp_cache_path(str(root), drive, t0, t1))
        assert np.array_equal(it["trans"], cached) and it["key"] == (drive, t0, t1)
        assert np.abs(cached - K.pose_from_positions(positions[drive][t0], positions[drive][t1])).max() < 0.05
        # the item's own voxels: the float32-quotient representatives, and cKDTree's pair set on them
        v = [it["xyz0"].cpu().numpy(), it["xyz1"].cpu().numpy()]
        for k, t in ((0, t0), (1, t1)):
            assert np.array_equal(v[k], _voxels_f32(scans[drive][t], VOXEL).astype(np.float64))
            assert np.array_equal(it[f"coords{k}"].cpu().numpy(),
                                  np.floor(v[k].astype(np.float32) / np.float32(VOXEL)).astype(np.int32))
        ref = _ref_pairs(v[0], v[1], cached, VOXEL * 1.5)
        assert len(ref) >= K.MIN_MATCHES                                  # the tree's own condition
        assert np.array_equal(it["matches"].cpu().numpy().astype(np.int64), ref)
        assert it["search_radius"] == VOXEL * 1.5 and it["image0"].shape == (3, 120, 160)
        assert float(it["feats0"].min()) == float(it["feats0"].max()) == 1.0           # val phase: no Jitter

    # the second epoch reads the cache: a file marked by hand (one entry moved by 1e-3, which no ICP run would give)
    # comes back as it is, and nothing is written; the mark is taken off again afterwards
    path = K.icp_cache_path(str(root), 0, 0, 2)
    original = np.load(path)
    marked = original.copy()
    marked[0, 3] += 1e-3
    np.save(path, marked)
    before = {f: os.stat(root / "icp" / f).st_mtime_ns for f in os.listdir(root / "icp")}
    again = ds[0]
    assert np.array_equal(again["trans"], marked) and not np.array_equal(again["trans"], items[0]["trans"])
    assert before == {f: os.stat(root / "icp" / f).st_mtime_ns for f in os.listdir(root / "icp")}
    np.save(path, original)
    marked = original
    ds[3]                                                               # skipped again: one record per pair, not per visit
    assert list(ds.skipped) == [(1, 3, 5)]

    # train phase: the scale draw multiplies points, radius and the translation alike; rotation stays off
    tr = KITTINMPairDataset("train", [0, 1], _config(root), seed=5, device=DEV)
    assert tr.random_scale and not tr.random_rotation and tr.jitter
    g = np.random.default_rng(5)
    assert g.random() < 0.95                                            # this seed draws a scale
    scale = 0.8 + 0.4 * g.random()
    it = tr[0]
    s32 = np.float32(scale)
    assert it["search_radius"] == VOXEL * 1.5 * scale
    assert np.array_equal(it["xyz0"].cpu().numpy(), _voxels_f32(s32 * scans[0][0], VOXEL).astype(np.float64))
    assert np.array_equal(it["trans"][:3, :3], marked[:3, :3]) and np.allclose(it["trans"][:3, 3], scale * marked[:3, 3],
                                                                               rtol=1e-7)
    x0, x1 = it["xyz0"].cpu().numpy(), it["xyz1"].cpu().numpy()
    m = it["matches"].cpu().numpy().astype(np.int64)
    d = np.linalg.norm(_apply(it["trans"], x0[m[:, 0]]) - x1[m[:, 1]], axis=1)
    assert len(m) >= K.MIN_MATCHES and d.max() <= it["search_radius"] * (1 + 1e-12)
    f = it["feats0"].cpu().numpy()
    assert f.shape == (len(x0), 1) and abs(f.mean() - 1) < 0.01 and 0.005 < f.std() < 0.02     # Jitter drawn
    # the same seed replays the same item
    tr.reset_seed(5)
    it2 = tr[0]
    assert torch.equal(it2["feats0"], it["feats0"]) and torch.equal(it2["matches"], it["matches"])


class _Truth(torch.nn.Module):
    """Stands in for the network: side 0 answers with T_gt x0, side 1 with x1, so that the nearest descriptor of every
    row is its ground-truth partner (what a one-hot code of the correspondence would select)."""

    def __init__(self, items):
        super().__init__()
        self.items, self.calls = items, 0

    def forward(self, st, image):
        it = self.items[self.calls // 2]
        side = self.calls % 2
        self.calls += 1
        x = it["xyz0"] @ torch.as_tensor(it["trans"][:3, :3].T, device=DEV) + torch.as_tensor(it["trans"][:3, 3], device=DEV) \
            if side == 0 else it["xyz1"]
        assert st.F.shape[0] == x.shape[0]
        out = type("Out", (), {})()
        out.F = torch.nn.functional.pad(x.float(), (0, 13)).contiguous()     # nn_search takes 16 / 32 / 64 columns
        return out


def test_valid_epoch_metric_chain(tree):
    from imfnet_amd.train.data import KITTINMPairDataset
    from imfnet_amd.train.trainer import HardestContrastiveTrainer
    root, positions, scans = tree
    cfg = _config(root, out_dir=str(root / "valid"), val_max_iter=0)
    val = KITTINMPairDataset("val", [2], cfg, seed=0, device=DEV)
    assert len(val) == 2
    tr = HardestContrastiveTrainer(cfg, val, val, device=DEV)
    out = tr.valid_epoch()                                              # the random network: six finite values
    assert set(out) == {"loss", "rre", "rte", "feat_match_ratio", "hit_ratio", "success"}
    assert all(np.isfinite(v) for v in out.values()), out
    assert not val.skipped
    items = [val[i] for i in range(len(val))]
    assert all(it["xyz0"].shape[0] == scans[2][0].shape[0] <= 5000 for it in items)    # one point per voxel, no subsample
    real, tr.model = tr.model, _Truth(items)
    try:
        out = tr.valid_epoch()
    finally:
        tr.model = real
        tr.pool.shutdown()
    print("valid_epoch with ground-truth correspondences:", out)
    # nothing to average (every pair skipped): rte and rre are NaN, which never is the best epoch, not a winning 0
    from imfnet_amd.train.trainer import is_better, worst_value
    val.prepare = lambda raw, timings=None: None
    empty = tr.valid_epoch()
    del val.prepare
    assert np.isnan(empty["rte"]) and np.isnan(empty["rre"]) and empty["success"] == 0.0 and empty["hit_ratio"] == 0.0
    assert not is_better("rte", empty["rte"], worst_value("rte")) and not is_better("rre", empty["rre"], 0.3)
    assert out["success"] == 1.0 and out["hit_ratio"] == 1.0 and out["feat_match_ratio"] == 1.0
    assert out["rte"] < 1e-3 and out["rre"] < 1e-4 and out["loss"] < 1e-3


def test_sgd_steps_lower_the_loss(tree):
    """30 SGD steps (lr 0.1, momentum 0.8) on one fixed KITTI pair, no scale, no Jitter: the bar of the 3DMatch test."""
    from imfnet_amd.train.data import KITTINMPairDataset
    from imfnet_amd.train.trainer import HardestContrastiveTrainer
    root, _, _ = tree
    cfg = _config(root, use_random_scale=False, batch_size=1, out_dir=str(root / "steps"))
    ds = KITTINMPairDataset("val", [0], cfg, seed=0, device=DEV)
    tr = HardestContrastiveTrainer(cfg, ds, None, device=DEV)
    raw = ds.load(0)
    losses = []
    for _ in range(30):
        losses.append(tr.train_step([[raw]])[0])
        for name, p in tr.model.named_parameters():
            if p.grad is not None:
                assert torch.isfinite(p.grad).all(), name
    tr.pool.shutdown()
    print("losses", [round(v, 4) for v in losses])
    assert all(np.isfinite(losses))
    first, last = losses[0], float(np.mean(losses[-5:]))
    assert last < 0.85 * first, (first, last)
    assert float(np.mean(losses[-5:])) < float(np.mean(losses[:5])) - 0.1


def test_cli_end_to_end_with_resume(tree, tmp_path):
    from imfnet_amd.checkpoint import load_checkpoint
    from imfnet_amd.evaluate_kitti import build_model
    root, _, scans = tree
    out = tmp_path / "out"
    args = [sys.executable, "-m", "imfnet_amd.train", "--dataset", "KITTINMPairDataset", "--kitti_root", str(root),
            "--train_list", str(root / "train.txt"), "--val_list", str(root / "val.txt"), "--out_dir", str(out),
            "--batch_size", "2", "--stat_freq", "1", "--val_max_iter", "2", "--seed", "1", "--best_val_metric", "success"]
    r = subprocess.run(args + ["--max_epoch", "2"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    losses = [float(v) for v in re.findall(r"Current Loss: (\S+)", r.stdout)]
    assert len(losses) == 4 and all(np.isfinite(losses)), r.stdout
    assert "4 training pairs, 2 validation pairs" in r.stdout and "skipped pair 1, 3, 5" in r.stdout
    assert len(re.findall(r"Final Loss: \S+ RTE: \S+ RRE: \S+ Hit Ratio: \S+ Feat Match Ratio: \S+", r.stdout)) == 3
    keys = {"epoch", "state_dict", "optimizer", "scheduler", "config", "best_val", "best_val_epoch", "best_val_metric"}
    ck = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert set(ck) == keys and isinstance(ck["config"], dict) and ck["epoch"] == 2
    assert ck["best_val_metric"] == "success" and ck["config"]["voxel_size"] == 0.3
    assert ck["config"]["dataset"] == "KITTINMPairDataset" and ck["config"]["use_random_scale"] is True

    sd, cfg = load_checkpoint(str(out / "checkpoint.pth"))
    assert (cfg.model, cfg.model_n_out, cfg.conv1_kernel_size, cfg.normalize_feature) == ("ResUNetBN2C", 32, 5, True)
    model = build_model(str(out / "checkpoint.pth"), 0, DEV)            # as evaluate_kitti -m loads it
    from imfnet_amd.evaluate_kitti import describe
    from imfnet_amd import kitti as K
    _, F = describe(model, scans[0][0], cfg.voxel_size, K.load_image(K.pair_image_paths(str(root), 0, 0, 2)[0]), DEV)
    F = F.cpu()
    assert torch.isfinite(F).all() and float((F.norm(dim=1) - 1).abs().max()) < 1e-4

    r = subprocess.run(args + ["--max_epoch", "3", "--resume", str(out)], cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Train Epoch: 3 [0/2]" in r.stdout and "Train Epoch: 1 " not in r.stdout and "Train Epoch: 2 " not in r.stdout
    assert torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)["epoch"] == 3
