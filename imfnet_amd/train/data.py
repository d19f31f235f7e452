"""The training pairs: IndoorPairDataset (3DMatch, lib/data_loaders.py:244-345) and KITTINMPairDataset (KITTI odometry,
:500-714), sample_random_trans (:95-101), Jitter (lib/transforms.py:18-30) and collate_pair_fn (:23-84).

An item is made in two halves.  `load(idx)` decodes the two PLY files and images on the host; it touches no GPU and
runs on the trainer's decode threads.  `prepare(raw)` runs in the trainer's process on its current stream: random
scale and rotation (host fp64, upstream's expressions), first-occurrence voxelisation on the GPU (fp64 quotient, the
existing geometry path) and the positive pairs by `radius_pairs` (imf_radius_pairs).  Every random draw comes from
the dataset's own `numpy.random.Generator`, in the order scale, rotation T0, rotation T1, jitter 0, jitter 1; upstream
mixes `random`, `np.random` and a RandomState and cannot be replayed.
"""
import glob
import logging
import os

import numpy as np
import torch
from scipy.linalg import expm

from ..dataio import process_image, read_image, read_ply_points

LOG = logging.getLogger("imfnet_amd.train")


def M(axis, theta):
    """Rotation about `axis` by theta: expm(cross(I, axis / |axis| * theta))."""
    return expm(np.cross(np.eye(3), axis / np.linalg.norm(axis) * theta))


def sample_random_trans(pcd, rng, rotation_range=360):
    """lib/data_loaders.py:95-101 with rng.random in place of randg.rand: T = [R | R . (-mean(pcd))]."""
    T = np.eye(4)
    R = M(rng.random(3) - 0.5, rotation_range * np.pi / 180.0 * (rng.random(1) - 0.5))
    T[:3, :3] = R
    T[:3, 3] = R.dot(-np.mean(pcd, axis=0))
    return T


def apply_transform(pts, trans):
    return pts @ trans[:3, :3].T + trans[:3, 3]


def read_scene_list(path):
    """config/train_3dmatch.txt format: whitespace-separated scene names."""
    with open(path) as f:
        return f.read().split()


def read_pair_files(overlap_path, scenes):
    """Every line of every `overlap_path/<scene>*` file: its first two fields (paths relative to threed_match_dir)."""
    files = []
    for name in scenes:
        found = sorted(glob.glob(os.path.join(overlap_path, name + "*")))
        if not found:
            raise FileNotFoundError(f"Make sure that the path {overlap_path} has data {name}")
        for fname in found:
            with open(fname) as f:
                for line in f:
                    parts = line.strip().split()
                    if len(parts) >= 2:
                        files.append((parts[0], parts[1]))
    return files


def image_path(ply_path):
    """The fragment's `_0.png`, falling back to `_0.jpg` (lib/data_loaders.py:252-257)."""
    p = ply_path.replace(".ply", "_0.png")
    return p if os.path.exists(p) else ply_path.replace(".ply", "_0.jpg")


def load_image_chw(path, H, W):
    img = read_image(path)
    if img.shape[0] != H or img.shape[1] != W:
        img = process_image(image=img, aim_H=H, aim_W=W)
    return np.ascontiguousarray(np.transpose(img, (2, 0, 1)), dtype=np.float32)


class IndoorPairDataset:
    """phase "train" applies the configured random scale / rotation and Jitter; any other phase none of them
    (make_data_loader, lib/data_loaders.py:658-682).  `config` needs threed_match_dir, overlap_path, voxel_size,
    positive_pair_search_voxel_size_multiplier, min_scale, max_scale, rotation_range, use_random_scale,
    use_random_rotation, image_H, image_W."""

    def __init__(self, phase, scenes, config, seed=0, device="cuda"):
        self.phase, self.config = phase, config
        self.root = config.threed_match_dir
        self.files = read_pair_files(config.overlap_path, scenes)
        train = phase in ("train", "trainval")
        self.random_scale = train and bool(config.use_random_scale)
        self.random_rotation = train and bool(config.use_random_rotation)
        self.jitter = train
        self.voxel_size = float(config.voxel_size)
        self.matching_search_voxel_size = self.voxel_size * float(config.positive_pair_search_voxel_size_multiplier)
        self.device = torch.device(device)
        self.reset_seed(seed)

    def reset_seed(self, seed=0):
        self.rng = np.random.default_rng(seed)

    def __len__(self):
        return len(self.files)

    def load(self, idx):
        """Host decode of pair idx: (xyz0, xyz1 float64 [N,3], image0, image1 float32 [3,H,W])."""
        f0, f1 = (os.path.join(self.root, f) for f in self.files[idx])
        H, W = int(self.config.image_H), int(self.config.image_W)
        return (read_ply_points(f0), read_ply_points(f1), load_image_chw(image_path(f0), H, W),
                load_image_chw(image_path(f1), H, W))

    def prepare(self, raw, timings=None):
        """Scale, rotation, voxelisation and positive pairs on the GPU.  Returns the item dict: xyz0 / xyz1 (device
        float64 voxel representatives), coords0 / coords1 (device int32 floor(xyz / voxel)), feats0 / feats1 (device
        float32 [n, 1]), matches (device int32 [P, 2]), trans (4x4 float64), search_radius, image0 / image1 ([3,H,W] float32)."""
        from .. import ops
        from ..matching import radius_pairs
        xyz0, xyz1, image0, image1 = raw
        rng, dev = self.rng, self.device
        r = self.matching_search_voxel_size
        t0 = _tick(timings, dev)
        if self.random_scale and rng.random() < 0.95:
            scale = self.config.min_scale + (self.config.max_scale - self.config.min_scale) * rng.random()
            r *= scale
            xyz0, xyz1 = scale * xyz0, scale * xyz1
        if self.random_rotation:
            T0 = sample_random_trans(xyz0, rng, self.config.rotation_range)
            T1 = sample_random_trans(xyz1, rng, self.config.rotation_range)
            trans = T1 @ np.linalg.inv(T0)
            xyz0, xyz1 = apply_transform(xyz0, T0), apply_transform(xyz1, T1)
        else:
            trans = np.identity(4)
        p0 = torch.from_numpy(np.ascontiguousarray(xyz0, dtype=np.float64)).to(dev)
        p1 = torch.from_numpy(np.ascontiguousarray(xyz1, dtype=np.float64)).to(dev)
        lv0, lv1 = ops.voxelize(p0, self.voxel_size), ops.voxelize(p1, self.voxel_size)
        ops.sync_levels([lv0, lv1])
        v0, v1 = p0[lv0.first_idx.long()], p1[lv1.first_idx.long()]
        t1 = _tick(timings, dev)
        matches, _ = radius_pairs(v0, v1, trans, r, device=dev)
        t2 = _tick(timings, dev)
        if timings is not None:
            timings["geometry"] = timings.get("geometry", 0.0) + t1 - t0
            timings["pairs"] = timings.get("pairs", 0.0) + t2 - t1
        feats = []
        for n in (lv0.n, lv1.n):
            f = np.ones((n, 1))
            if self.jitter and rng.random() < 0.95:                      # Jitter(mu=0, sigma=0.01)
                f = f + rng.normal(0.0, 0.01, (n, 1))
            feats.append(torch.from_numpy(f.astype(np.float32)).to(dev))
        return dict(xyz0=v0, xyz1=v1, coords0=lv0.coords[:, 1:], coords1=lv1.coords[:, 1:], feats0=feats[0],
                    feats1=feats[1], matches=matches, trans=trans, search_radius=r, image0=image0, image1=image1)

    def __getitem__(self, idx):
        return self.prepare(self.load(idx))


class KITTINMPairDataset:
    """The KITTI odometry pairs (lib/data_loaders.py:626-714 for the pair list, :500-623 for an item; IS_ODOMETRY),
    train and val phases, with IndoorPairDataset's item dict and load / prepare split.  `sequences`: the odometry
    sequence numbers of the phase (config/train_kitti.txt, val_kitti.txt).  `config` needs kitti_root, voxel_size,
    positive_pair_search_voxel_size_multiplier, min_scale, max_scale, use_random_scale, image_H, image_W and may carry
    own_image.

    Kept: the pair list (kitti.pairs_of_sequence per sequence, minus kitti.DROPPED_PAIRS); the ground truth through
    the `<kitti_root>/icp` cache shared with the evaluator (kitti.ground_truth: pose algebra, then the GPU ICP on 5 cm
    voxels); no random rotation in any phase (upstream forces it off for the odometry layout); the random scale of
    the train phase on the float32 scan and the search radius (probability 0.95, a factor in [min_scale, max_scale]);
    the float32-quotient first-occurrence voxels (kitti.voxelize_f32); ones as features, with Jitter in the train
    phase; both images read from frame t0 unless own_image.
    Changed: a drawn scale also multiplies the translation of `trans` (upstream leaves the matrix as it is, so a scaled
    pair's points and ground truth disagree by (1 - scale) t, metres on KITTI); a pair with fewer than
    kitti.MIN_MATCHES positive pairs is logged and `prepare` returns None (upstream raises ValueError and the epoch
    ends); the draws come from the data set's own Generator in the order scale coin, scale, jitter 0, jitter 1."""
    quantize = "f32"                       # the trainer voxelises the representatives as the loader did

    def __init__(self, phase, sequences, config, seed=0, device="cuda"):
        from .. import kitti as K
        self.phase, self.config = phase, config
        self.root = config.kitti_root
        self.own_image = bool(getattr(config, "own_image", False))
        self.positions = {d: K.read_poses(self.root, d) for d in sequences}
        self.files = K.pair_list(self.root, list(sequences))
        train = phase in ("train", "trainval")
        self.random_scale = train and bool(config.use_random_scale)
        self.random_rotation = False
        self.jitter = train
        self.voxel_size = float(config.voxel_size)
        self.matching_search_voxel_size = self.voxel_size * float(config.positive_pair_search_voxel_size_multiplier)
        self.device = torch.device(device)
        self.skipped = {}                  # (drive, t0, t1) -> positive pairs, of every pair `prepare` refused
        self.reset_seed(seed)

    def reset_seed(self, seed=0):
        self.rng = np.random.default_rng(seed)

    def __len__(self):
        return len(self.files)

    def load(self, idx):
        """Host decode of pair idx: ((drive, t0, t1), xyz0, xyz1 float32 [N,3], image0, image1 float32 [3,H,W])."""
        from .. import kitti as K
        drive, t0, t1 = self.files[idx]
        H, W = int(self.config.image_H), int(self.config.image_W)
        f0, f1 = K.pair_image_paths(self.root, drive, t0, t1, self.own_image)
        return ((drive, t0, t1), K.read_scan(K.velodyne_path(self.root, drive, t0)),
                K.read_scan(K.velodyne_path(self.root, drive, t1)), K.load_image(f0, H, W)[0], K.load_image(f1, H, W)[0])

    def prepare(self, raw, timings=None):
        """Ground truth (cache or GPU ICP), scale, voxelisation and positive pairs on the GPU.  Returns
        IndoorPairDataset.prepare's item dict plus `key` = (drive, t0, t1), or None for a pair with too few positive
        pairs."""
        from .. import kitti as K
        from ..matching import radius_pairs
        (drive, t0, t1), xyz0, xyz1, image0, image1 = raw
        rng, dev = self.rng, self.device
        r = self.matching_search_voxel_size
        tk0 = _tick(timings, dev)
        trans, _ = K.ground_truth(self.root, drive, t0, t1, xyz0, xyz1, self.positions[drive], dev)
        if self.random_scale and rng.random() < 0.95:
            scale = self.config.min_scale + (self.config.max_scale - self.config.min_scale) * rng.random()
            r *= scale
            xyz0, xyz1 = np.float32(scale) * xyz0, np.float32(scale) * xyz1
            trans = trans.copy()
            trans[:3, 3] *= float(np.float32(scale))
        sides = []
        for xyz in (xyz0, xyz1):
            pts = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).to(dev)
            coords, first = K.voxelize_f32(pts, self.voxel_size)
            sides.append((pts[first.long()].double(), coords[:, 1:].contiguous()))
        (v0, c0), (v1, c1) = sides
        tk1 = _tick(timings, dev)
        matches, _ = radius_pairs(v0, v1, trans, r, device=dev)
        tk2 = _tick(timings, dev)
        if timings is not None:
            timings["geometry"] = timings.get("geometry", 0.0) + tk1 - tk0
            timings["pairs"] = timings.get("pairs", 0.0) + tk2 - tk1
        if matches.shape[0] < K.MIN_MATCHES:
            self.skipped[(drive, t0, t1)] = int(matches.shape[0])
            LOG.warning(f"skipped pair {drive}, {t0}, {t1}: {matches.shape[0]} positive pairs (< {K.MIN_MATCHES})")
            return None
        feats = []
        for n in (v0.shape[0], v1.shape[0]):
            f = np.ones((n, 1))
            if self.jitter and rng.random() < 0.95:                      # Jitter(mu=0, sigma=0.01)
                f = f + rng.normal(0.0, 0.01, (n, 1))
            feats.append(torch.from_numpy(f.astype(np.float32)).to(dev))
        return dict(xyz0=v0, xyz1=v1, coords0=c0, coords1=c1, feats0=feats[0], feats1=feats[1], matches=matches,
                    trans=trans, search_radius=r, image0=image0, image1=image1, key=(drive, t0, t1))

    def __getitem__(self, idx):
        return self.prepare(self.load(idx))


def _tick(timings, dev):
    if timings is None:
        return 0.0
    import time
    torch.cuda.synchronize(dev)
    return time.perf_counter()


def collate_pair_fn(items):
    """lib/data_loaders.py:23-84 on the item dicts: points and features concatenated, coordinates with the batch
    column in front, correspondences offset by the running (N0, N1), images stacked [B, 3, H, W]."""
    out = {k: [] for k in ("pcd0", "pcd1", "C0", "C1", "F0", "F1", "corr", "T", "image0", "image1")}
    len_batch = []
    n0 = n1 = 0
    for b, it in enumerate(items):
        N0, N1 = it["coords0"].shape[0], it["coords1"].shape[0]
        out["pcd0"].append(it["xyz0"])
        out["pcd1"].append(it["xyz1"])
        for key, c in (("C0", it["coords0"]), ("C1", it["coords1"])):
            c = torch.as_tensor(c).int()
            out[key].append(torch.cat([torch.full((c.shape[0], 1), b, dtype=torch.int32, device=c.device), c], 1))
        out["F0"].append(torch.as_tensor(it["feats0"]).float())
        out["F1"].append(torch.as_tensor(it["feats1"]).float())
        m = torch.as_tensor(it["matches"])
        out["corr"].append(m.int() + torch.tensor([n0, n1], dtype=torch.int32, device=m.device))
        out["T"].append(torch.as_tensor(np.asarray(it["trans"])))
        out["image0"].append(torch.as_tensor(it["image0"])[None])
        out["image1"].append(torch.as_tensor(it["image1"])[None])
        len_batch.append([N0, N1])
        n0 += N0
        n1 += N1
    return {
        "pcd0": torch.cat(out["pcd0"], 0), "pcd1": torch.cat(out["pcd1"], 0),
        "image0": torch.cat(out["image0"], 0).float(), "image1": torch.cat(out["image1"], 0).float(),
        "sinput0_C": torch.cat(out["C0"], 0), "sinput0_F": torch.cat(out["F0"], 0),
        "sinput1_C": torch.cat(out["C1"], 0), "sinput1_F": torch.cat(out["F1"], 0),
        "correspondences": torch.cat(out["corr"], 0), "T_gt": torch.cat(out["T"], 0).float(),
        "len_batch": len_batch,
    }
