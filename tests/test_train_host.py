"""Host-side pieces of the trainer (imfnet_amd/train): the random rotation, the collate step, the pair lists, the
negative mask's key and the command line.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.linalg import expm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_random_trans_is_the_skew_exponential():
    from imfnet_amd.train.data import sample_random_trans
    pcd = np.random.default_rng(1).normal(size=(500, 3)) + [1.0, -2.0, 3.0]
    T = sample_random_trans(pcd, np.random.default_rng(7), 360)
    # the same draws, by hand: axis = rand(3) - 0.5, theta = 2 pi (rand(1) - 0.5)
    g = np.random.default_rng(7)
    axis = g.random(3) - 0.5
    theta = 2 * np.pi * (g.random(1) - 0.5)
    w = axis / np.linalg.norm(axis) * theta
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = expm(K)
    assert np.allclose(T[:3, :3], R, atol=1e-12)
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12)
    assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-12
    assert np.allclose(T[:3, 3], -R @ pcd.mean(0), atol=1e-12)
    assert np.array_equal(T[3], [0, 0, 0, 1])


def _item(n0, n1, p, b):
    g = np.random.default_rng(b)
    return dict(xyz0=torch.rand(n0, 3, dtype=torch.float64), xyz1=torch.rand(n1, 3, dtype=torch.float64),
                coords0=torch.randint(-9, 9, (n0, 3), dtype=torch.int32),
                coords1=torch.randint(-9, 9, (n1, 3), dtype=torch.int32),
                feats0=torch.ones(n0, 1), feats1=torch.ones(n1, 1) * 2,
                matches=torch.as_tensor(np.stack([g.integers(0, n0, p), g.integers(0, n1, p)], 1).astype(np.int32)),
                trans=np.eye(4) * (b + 1), image0=np.full((3, 4, 5), b, np.float32),
                image1=np.full((3, 4, 5), 10 + b, np.float32))


def test_collate_offsets_batch_column_and_images():
    from imfnet_amd.train.data import collate_pair_fn
    items = [_item(7, 5, 4, 0), _item(3, 9, 6, 1), _item(4, 2, 1, 2)]
    out = collate_pair_fn(items)
    assert out["len_batch"] == [[7, 5], [3, 9], [4, 2]]
    C0 = out["sinput0_C"]
    assert C0.shape == (14, 4) and C0.dtype == torch.int32
    assert C0[:, 0].tolist() == [0] * 7 + [1] * 3 + [2] * 4
    assert torch.equal(C0[7:10, 1:], items[1]["coords0"])
    assert out["sinput1_C"][:, 0].tolist() == [0] * 5 + [1] * 9 + [2] * 2
    corr = out["correspondences"]
    assert corr.dtype == torch.int32 and corr.shape == (11, 2)
    assert torch.equal(corr[:4], items[0]["matches"])
    assert torch.equal(corr[4:10], items[1]["matches"] + torch.tensor([7, 5], dtype=torch.int32))
    assert torch.equal(corr[10:], items[2]["matches"] + torch.tensor([10, 14], dtype=torch.int32))
    assert out["image0"].shape == (3, 3, 4, 5) and out["image1"].shape == (3, 3, 4, 5)
    assert out["image0"][:, 0, 0, 0].tolist() == [0, 1, 2] and out["image1"][:, 0, 0, 0].tolist() == [10, 11, 12]
    assert out["sinput1_F"].shape == (16, 1) and float(out["sinput1_F"].sum()) == 32
    assert out["T_gt"].shape == (12, 4)
    assert torch.equal(out["pcd0"][7:10], items[1]["xyz0"])


def test_pair_lists_subset_and_jpg_fallback(tmp_path):
    from imfnet_amd.train.data import image_path, read_pair_files, read_scene_list
    ov = tmp_path / "overlap"
    ov.mkdir()
    (ov / "sceneA-x@seq-01-0.30.txt").write_text("sceneA/seq-01/cloud_bin_0.ply sceneA/seq-01/cloud_bin_1.ply 0.5\n"
                                                 "sceneA/seq-01/cloud_bin_0.ply sceneA/seq-01/cloud_bin_2.ply 0.4\n")
    (ov / "sceneA-x@seq-02-0.30.txt").write_text("sceneA/seq-02/cloud_bin_3.ply sceneA/seq-02/cloud_bin_4.ply 0.7\n")
    (ov / "sceneB@seq-01-0.30.txt").write_text("sceneB/seq-01/cloud_bin_0.ply sceneB/seq-01/cloud_bin_1.ply 0.9\n")
    lst = tmp_path / "train.txt"
    lst.write_text("sceneA\n")
    files = read_pair_files(str(ov), read_scene_list(str(lst)))
    assert files == [("sceneA/seq-01/cloud_bin_0.ply", "sceneA/seq-01/cloud_bin_1.ply"),
                     ("sceneA/seq-01/cloud_bin_0.ply", "sceneA/seq-01/cloud_bin_2.ply"),
                     ("sceneA/seq-02/cloud_bin_3.ply", "sceneA/seq-02/cloud_bin_4.ply")]
    with pytest.raises(FileNotFoundError):
        read_pair_files(str(ov), ["sceneC"])
    ply = tmp_path / "cloud_bin_0.ply"
    assert image_path(str(ply)).endswith("cloud_bin_0_0.jpg")          # neither exists: the .jpg name
    (tmp_path / "cloud_bin_0_0.png").write_bytes(b"")
    assert image_path(str(ply)).endswith("cloud_bin_0_0.png")


def test_hash_key_and_mask_on_cpu():
    from imfnet_amd.train.loss import hash_keys
    N0, N1 = 50, 70
    M = max(N0, N1)
    pos = torch.tensor([[3, 4], [10, 69], [49, 0]])
    keys = hash_keys(pos[:, 0], pos[:, 1], M)
    # util/misc.py _hash: sum_d arr[:, d] * M^d
    assert keys.tolist() == [3 + 4 * M, 10 + 69 * M, 49]
    ii, jj = torch.meshgrid(torch.arange(N0), torch.arange(N1), indexing="ij")
    allk = hash_keys(ii.reshape(-1), jj.reshape(-1), M)
    assert allk.unique().numel() == N0 * N1                            # injective over the index box
    neg_i, neg_j = torch.tensor([3, 3, 10, 49, 1]), torch.tensor([4, 5, 69, 0, 1])
    mask = ~torch.isin(hash_keys(neg_i, neg_j, M), keys)
    assert mask.tolist() == [False, True, False, False, True]


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "imfnet_amd.train", *args], cwd=ROOT, capture_output=True, text=True,
                          timeout=120)


def test_help_lists_upstream_option_names():
    r = _cli("--help")
    assert r.returncode == 0, r.stderr
    for name in ("--trainer", "--batch_size", "--num_pos_per_batch", "--num_hn_samples_per_batch", "--neg_thresh",
                 "--pos_thresh", "--neg_weight", "--use_random_scale", "--min_scale", "--max_scale",
                 "--use_random_rotation", "--rotation_range", "--stat_freq", "--val_max_iter", "--val_epoch_freq",
                 "--positive_pair_search_voxel_size_multiplier", "--hit_ratio_thresh", "--model", "--model_n_out",
                 "--conv1_kernel_size", "--normalize_feature", "--best_val_metric", "--max_epoch", "--lr",
                 "--momentum", "--weight_decay", "--iter_size", "--bn_momentum", "--exp_gamma", "--resume",
                 "--voxel_size", "--threed_match_dir", "--overlap_path", "--image_W", "--image_H", "--out_dir"):
        assert name in r.stdout, name


def test_defaults_are_config_3dmatch():
    from imfnet_amd.train.trainer import parse_config
    c = parse_config([])
    assert (c.batch_size, c.num_pos_per_batch, c.num_hn_samples_per_batch) == (2, 1024, 256)
    assert (c.neg_thresh, c.pos_thresh, c.neg_weight, c.voxel_size) == (1.4, 0.1, 1, 0.025)
    assert c.positive_pair_search_voxel_size_multiplier == 1.5
    assert (c.lr, c.momentum, c.weight_decay, c.exp_gamma, c.iter_size) == (0.1, 0.8, 1e-4, 0.99, 1)


def test_unknown_trainer_is_refused():
    r = _cli("--trainer", "TripletLossTrainer")
    assert r.returncode != 0
    assert "only HardestContrastiveLossTrainer" in r.stderr
