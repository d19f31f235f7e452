"""HardestContrastiveLossTrainer (lib/trainer.py:28-200, 381-493) and its command line (config_3dmatch.py,
train_3DMatch.py) on the GPU.

One training iteration: decode of the batch's files on at most 16 host threads (prefetched one batch ahead), then in
this process on its stream: per item the random scale / rotation, voxelisation and positive-pair search
(data.IndoorPairDataset.prepare), collate, one batched forward per side through `forward_layers` (training mode),
the hardest-contrastive loss, backward and SGD.  No worker process opens the GPU and nothing forks.

Kept from upstream: the option names and defaults, SGD with `momentum` (0.8; upstream ignores `sgd_momentum`),
ExponentialLR(exp_gamma) stepped once per epoch, `iter_size` accumulation, validation every `val_epoch_freq` epochs
with `find_corr` on a 5 000-row subsample, hit ratio and feat_match_ratio = hit_ratio > 0.05, and the checkpoint keys.
Changed: the checkpoints are `checkpoint.pth` (every epoch) and `best_val_checkpoint.pth` (by best_val_metric), not
one file per epoch; `config` in them is a plain dict; `--resume` takes the output directory (or a checkpoint file)
and continues at the epoch after the saved one; validation has no RTE / RRE (upstream's te.est_quad_linear_robust);
losses are logged as plain lines (no tensorboardX).  Only HardestContrastiveLossTrainer and the 3DMatch pairs exist.
"""
import argparse
import json
import logging
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .data import collate_pair_fn
from .loss import hardest_contrastive_loss

TRAINERS = ("HardestContrastiveLossTrainer",)
LOG = logging.getLogger("imfnet_amd.train")


def str2bool(v):
    return str(v).lower() in ("true", "1", "yes", "y", "t")


def make_parser():
    """config_3dmatch.py's options that the 3DMatch hardest-contrastive path reads, with upstream's names and defaults."""
    p = argparse.ArgumentParser(prog="python -m imfnet_amd.train",
                                description="Train IMFNet with the hardest-contrastive loss on 3DMatch pairs (GPU).")
    a = p.add_argument
    a("--out_dir", type=str, default="outputs/checkpoints")
    a("--trainer", type=str, default="HardestContrastiveLossTrainer")
    a("--save_freq_epoch", type=int, default=1)
    a("--batch_size", type=int, default=2)
    a("--val_batch_size", type=int, default=1)
    a("--num_pos_per_batch", type=int, default=1024)
    a("--num_hn_samples_per_batch", type=int, default=256)
    a("--neg_thresh", type=float, default=1.4)
    a("--pos_thresh", type=float, default=0.1)
    a("--neg_weight", type=float, default=1)
    a("--use_random_scale", type=str2bool, default=False)
    a("--min_scale", type=float, default=0.8)
    a("--max_scale", type=float, default=1.2)
    a("--use_random_rotation", type=str2bool, default=True)
    a("--rotation_range", type=float, default=360)
    a("--train_phase", type=str, default="train")
    a("--val_phase", type=str, default="val")
    a("--stat_freq", type=int, default=40)
    a("--test_valid", type=str2bool, default=True)
    a("--val_max_iter", type=int, default=400)
    a("--val_epoch_freq", type=int, default=1)
    a("--positive_pair_search_voxel_size_multiplier", type=float, default=1.5)
    a("--hit_ratio_thresh", type=float, default=0.1)
    a("--model", type=str, default="ResUNetBN2C")
    a("--model_n_out", type=int, default=32)
    a("--conv1_kernel_size", type=int, default=5)
    a("--normalize_feature", type=str2bool, default=True)
    a("--best_val_metric", type=str, default="feat_match_ratio")
    a("--optimizer", type=str, default="SGD")
    a("--max_epoch", type=int, default=200)
    a("--lr", type=float, default=1e-1)
    a("--momentum", type=float, default=0.8)
    a("--weight_decay", type=float, default=1e-4)
    a("--iter_size", type=int, default=1)
    a("--bn_momentum", type=float, default=0.05)
    a("--exp_gamma", type=float, default=0.99)
    a("--scheduler", type=str, default="ExpLR")
    a("--weights", type=str, default=None)
    a("--resume", type=str, default=None, help="output directory (its checkpoint.pth) or a checkpoint file")
    a("--train_num_thread", type=int, default=2)
    a("--voxel_size", type=float, default=0.025)
    a("--threed_match_dir", type=str, default="data/threedmatch")
    a("--overlap_path", type=str, default="data/overlap30")
    a("--train_list", type=str, default=None, help="scene list of the train phase (config/train_3dmatch.txt format)")
    a("--val_list", type=str, default=None, help="scene list of the val phase (config/val_3dmatch.txt format)")
    a("--image_W", type=int, default=160)
    a("--image_H", type=int, default=120)
    a("--seed", type=int, default=0)
    return p


def parse_config(argv=None):
    cfg = make_parser().parse_args(argv)
    if cfg.trainer not in TRAINERS:
        raise SystemExit(f"--trainer {cfg.trainer}: only {', '.join(TRAINERS)} is implemented "
                         f"(the plain-contrastive and triplet trainers are not)")
    if cfg.optimizer != "SGD" or cfg.scheduler != "ExpLR":
        raise SystemExit("only --optimizer SGD with --scheduler ExpLR is implemented")
    if cfg.best_val_metric != "feat_match_ratio":
        raise SystemExit("--best_val_metric: only feat_match_ratio (validation has no RTE / RRE)")
    return cfg


def _sparse_input(xyz_list, feats, voxel, device):
    """One batched sparse tensor from the items' voxel representatives (rows grouped by item in first-occurrence order,
    the same rows as the items' own voxelisation) with the given per-voxel input features."""
    from ..extract import sparse_tensor_from_points, start_geometry
    fut = start_geometry(list(xyz_list), voxel, device) if len(xyz_list) > 1 else start_geometry(xyz_list[0], voxel,
                                                                                                   device)
    st, inds = sparse_tensor_from_points(None, voxel, device, geometry=fut)
    if feats is not None:
        if feats.shape[0] != st.F.shape[0]:
            raise RuntimeError("batched voxelisation changed the row count of the items")
        st._F = feats.to(device=st.F.device, dtype=torch.float32).contiguous()
        st._all_ones = False
    return st


class HardestContrastiveTrainer:
    def __init__(self, config, train_set, val_set=None, device="cuda"):
        from ..model import load_model
        self.config = config
        self.device = torch.device(device)
        torch.manual_seed(config.seed)
        self.rng = np.random.default_rng(config.seed)        # loss samples and find_corr subsamples
        Model = load_model(config.model)
        self.model = Model(1, config.model_n_out, bn_momentum=config.bn_momentum,
                           normalize_feature=config.normalize_feature, conv1_kernel_size=config.conv1_kernel_size,
                           D=3, config=None)
        if config.weights:
            from ..checkpoint import load_checkpoint
            sd, _ = load_checkpoint(config.weights)
            self.model.load_state_dict(sd)
        self.model = self.model.to(self.device)
        self.optimizer = torch.optim.SGD(self.model.parameters(), lr=config.lr, momentum=config.momentum,
                                         weight_decay=config.weight_decay)
        self.scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, config.exp_gamma)
        self.train_set, self.val_set = train_set, val_set
        self.start_epoch = 1
        self.best_val, self.best_val_epoch, self.best_val_metric = -np.inf, -np.inf, config.best_val_metric
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(16, int(config.train_num_thread))))
        os.makedirs(config.out_dir, exist_ok=True)
        with open(os.path.join(config.out_dir, "config.json"), "w") as f:
            json.dump(dict(vars(config)), f, indent=4)
        if config.resume:
            self.resume(config.resume)

    # ---- checkpoints ---------------------------------------------------------------------------------------------
    def _save(self, epoch, filename):
        state = {"epoch": epoch, "state_dict": self.model.state_dict(), "optimizer": self.optimizer.state_dict(),
                 "scheduler": self.scheduler.state_dict(), "config": dict(vars(self.config)),
                 "best_val": self.best_val, "best_val_epoch": self.best_val_epoch,
                 "best_val_metric": self.best_val_metric}
        path = os.path.join(self.config.out_dir, filename + ".pth")
        LOG.info(f"Saving checkpoint: {path} ...")
        torch.save(state, path)

    def resume(self, where):
        path = os.path.join(where, "checkpoint.pth") if os.path.isdir(where) else where
        if not os.path.isfile(path):
            raise ValueError(f"=> no checkpoint found at '{path}'")
        LOG.info(f"=> loading checkpoint '{path}'")
        state = torch.load(path, map_location=self.device, weights_only=False)
        self.model.load_state_dict(state["state_dict"])
        self.optimizer.load_state_dict(state["optimizer"])
        self.scheduler.load_state_dict(state["scheduler"])
        self.start_epoch = int(state["epoch"]) + 1
        self.best_val, self.best_val_epoch = state["best_val"], state["best_val_epoch"]
        self.best_val_metric = state["best_val_metric"]

    # ---- one step --------------------------------------------------------------------------------------------------
    def forward_pair(self, batch):
        """(F0, F1) of a collated batch, training mode (forward_layers, BatchNorm batch statistics)."""
        c, dev = self.config, self.device
        outs = []
        for side in "01":
            lens = [lb[int(side)] for lb in batch["len_batch"]]
            pts = torch.split(batch["pcd" + side], lens)
            st = _sparse_input(pts, batch[f"sinput{side}_F"], c.voxel_size, dev)
            outs.append(self.model(st, batch["image" + side].to(dev)).F)
        return outs

    def train_step(self, raws, timings=None):
        """One optimizer step over iter_size batches of decoded pairs (`raws`: iter_size lists of dataset.load
        results).  Returns (loss, pos, neg) summed over the accumulation as upstream logs them."""
        c = self.config
        self.model.train()
        self.optimizer.zero_grad()
        tot = [0.0, 0.0, 0.0]
        for raw_batch in raws:
            batch = collate_pair_fn([self.train_set.prepare(r, timings) for r in raw_batch])
            t0 = _tick(timings, self.device)
            F0, F1 = self.forward_pair(batch)
            t1 = _tick(timings, self.device)
            pos, neg = hardest_contrastive_loss(F0, F1, batch["correspondences"],
                                                num_pos=c.num_pos_per_batch * c.batch_size,
                                                num_hn_samples=c.num_hn_samples_per_batch * c.batch_size,
                                                pos_thresh=c.pos_thresh, neg_thresh=c.neg_thresh, rng=self.rng)
            pos, neg = pos / c.iter_size, neg / c.iter_size
            loss = pos + c.neg_weight * neg
            t2 = _tick(timings, self.device)
            loss.backward()
            t3 = _tick(timings, self.device)
            for i, v in enumerate((loss, pos, neg)):
                tot[i] += float(v.detach())
            if timings is not None:
                for k, v in (("forward", t1 - t0), ("loss", t2 - t1), ("backward", t3 - t2)):
                    timings[k] = timings.get(k, 0.0) + v
        t4 = _tick(timings, self.device)
        self.optimizer.step()
        if timings is not None:
            timings["step"] = timings.get("step", 0.0) + _tick(timings, self.device) - t4
        return tuple(tot)

    # ---- epochs ----------------------------------------------------------------------------------------------------
    def _batches(self, n_iter, epoch):
        c = self.config
        order = np.random.default_rng([c.seed, epoch]).permutation(len(self.train_set))   # shuffle=True per epoch
        per = c.batch_size * c.iter_size
        groups = [order[k * per:(k + 1) * per] for k in range(n_iter)]
        return [[g[b * c.batch_size:(b + 1) * c.batch_size] for b in range(c.iter_size)] for g in groups]

    def _submit(self, group):
        return [[self.pool.submit(self.train_set.load, int(i)) for i in b] for b in group]

    def train_epoch(self, epoch):
        c = self.config
        n_iter = len(self.train_set) // c.batch_size // c.iter_size                        # drop_last=True
        groups = self._batches(n_iter, epoch)
        pending = self._submit(groups[0]) if groups else None
        data_t = total_t = 0.0
        n_meas = 0
        for it in range(n_iter):
            t0 = time.perf_counter()
            raws = [[f.result() for f in b] for b in pending]
            if it + 1 < n_iter:
                pending = self._submit(groups[it + 1])                                  # decode one batch ahead
            t1 = time.perf_counter()
            loss, pos, neg = self.train_step(raws)
            torch.cuda.synchronize(self.device)
            t2 = time.perf_counter()
            data_t += t1 - t0
            total_t += t2 - t0
            n_meas += 1
            if it % c.stat_freq == 0:
                LOG.info(f"Train Epoch: {epoch} [{it}/{n_iter}], Current Loss: {loss:.3e} Pos: {pos:.3f} "
                         f"Neg: {neg:.3f}\tData time: {data_t / n_meas:.4f}, Train time: "
                         f"{(total_t - data_t) / n_meas:.4f}, Iter time: {total_t / n_meas:.4f}")
                data_t = total_t = 0.0
                n_meas = 0

    @torch.no_grad()
    def valid_epoch(self):
        """lib/trainer.py:313-410 without RTE / RRE: hit ratio and feat_match_ratio over at most val_max_iter pairs."""
        from ..matching import nn_search
        c, dev = self.config, self.device
        self.model.eval()
        self.val_set.reset_seed(0)
        rng = np.random.default_rng(c.seed)
        n = len(self.val_set) if c.val_max_iter <= 0 else min(c.val_max_iter, len(self.val_set))
        hits, fmr = [], []
        for idx in range(n):
            it = self.val_set.prepare(self.val_set.load(idx))
            Fs = []
            for side in "01":
                st = _sparse_input([it["xyz" + side]], None, c.voxel_size, dev)
                Fs.append(self.model(st, torch.as_tensor(it["image" + side])[None].to(dev)).F)
            xyz0, xyz1 = it["xyz0"], it["xyz1"]
            F0, F1 = Fs
            if len(F0) > 5000:                                   # find_corr(subsample_size=5000)
                i0 = torch.as_tensor(rng.choice(len(F0), min(len(F0), 5000), replace=False)).to(dev)
                i1 = torch.as_tensor(rng.choice(len(F1), min(len(F1), 5000), replace=False)).to(dev)
                nn = nn_search(F0[i0].contiguous(), F1[i1].contiguous()).long()
                x0, x1 = xyz0[i0], xyz1[i1[nn]]
            else:
                nn = nn_search(F0.contiguous(), F1.contiguous()).long()
                x0, x1 = xyz0, xyz1[nn]
            T = torch.as_tensor(it["trans"], dtype=torch.float64, device=dev)
            x0 = x0 @ T[:3, :3].t() + T[:3, 3]
            dist = torch.sqrt(((x0 - x1) ** 2).sum(1) + 1e-6)
            hr = float((dist < c.hit_ratio_thresh).double().mean())
            hits.append(hr)
            fmr.append(float(hr > 0.05))
        out = {"hit_ratio": float(np.mean(hits)) if hits else 0.0,
               "feat_match_ratio": float(np.mean(fmr)) if fmr else 0.0}
        LOG.info(f"Final Hit Ratio: {out['hit_ratio']:.3f}, Feat Match Ratio: {out['feat_match_ratio']:.3f}")
        return out

    def train(self):
        c = self.config
        if self.val_set is not None and self.start_epoch == 1:
            self.valid_epoch()                                   # baseline of the random features
        for epoch in range(self.start_epoch, c.max_epoch + 1):
            LOG.info(f" Epoch: {epoch}, LR: {self.scheduler.get_last_lr()}")
            self.train_epoch(epoch)
            self.scheduler.step()
            val = None
            if self.val_set is not None and epoch % c.val_epoch_freq == 0:
                val = self.valid_epoch()
            if val is not None and self.best_val < val[self.best_val_metric]:
                LOG.info(f"Saving the best val model with {self.best_val_metric}: {val[self.best_val_metric]}")
                self.best_val, self.best_val_epoch = val[self.best_val_metric], epoch
                self._save(epoch, "best_val_checkpoint")
            if epoch % c.save_freq_epoch == 0 or epoch == c.max_epoch:
                self._save(epoch, "checkpoint")
        self.pool.shutdown()


def _tick(timings, dev):
    if timings is None:
        return 0.0
    torch.cuda.synchronize(dev)
    return time.perf_counter()


def main(argv=None):
    cfg = parse_config(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s", datefmt="%m/%d %H:%M:%S",
                        stream=sys.stdout)
    from .data import IndoorPairDataset, read_scene_list
    if not cfg.train_list:
        raise SystemExit("--train_list is required (a scene list in config/train_3dmatch.txt's format)")
    train_set = IndoorPairDataset(cfg.train_phase, read_scene_list(cfg.train_list), cfg, seed=cfg.seed)
    val_set = None
    if cfg.test_valid:
        if not cfg.val_list:
            raise SystemExit("--val_list is required with --test_valid true")
        val_set = IndoorPairDataset(cfg.val_phase, read_scene_list(cfg.val_list), cfg, seed=0)
    LOG.info(f"{len(train_set)} training pairs, {len(val_set) if val_set else 0} validation pairs")
    HardestContrastiveTrainer(cfg, train_set, val_set).train()
    return 0
