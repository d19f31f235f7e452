"""HardestContrastiveLossTrainer (lib/trainer.py:28-200, 381-493) and its command line (config_3dmatch.py /
config_kitti.py, train_3DMatch.py / train_Kitti.py) on the GPU.

One training iteration: decode of the batch's files on at most 16 host threads (prefetched one batch ahead), then in
this process on its stream: per item the random scale / rotation, voxelisation and positive-pair search
(data.IndoorPairDataset.prepare), collate, one batched forward per side through `forward_layers` (training mode),
the hardest-contrastive loss, backward and SGD (`--optim_kernels hip`: train.optim.FusedSGD, one launch per step that
also leaves the packed convolution weights).  No worker process opens the GPU and nothing forks.

Kept from upstream: the option names and defaults, SGD with `momentum` (0.8; upstream ignores `sgd_momentum`),
ExponentialLR(exp_gamma) stepped once per epoch, `iter_size` accumulation, validation every `val_epoch_freq` epochs
with `find_corr` on a 5 000-row subsample, the robust transform of the correspondences (matching.robust_transform,
upstream's te.est_quad_linear_robust as one fp64 launch) with loss / RTE / RRE / success, hit ratio and
feat_match_ratio = hit_ratio > 0.05, and the checkpoint keys.
Changed: the checkpoints are `checkpoint.pth` (every epoch) and `best_val_checkpoint.pth` (by best_val_metric), not
one file per epoch; `config` in them is a plain dict; `--resume` takes the output directory (or a checkpoint file)
and continues at the epoch after the saved one; for `--best_val_metric rte` / `rre` lower is better (upstream keeps
the epoch with the LARGEST value of every metric); a pair with too few positive pairs is logged and skipped instead of
ending the epoch; losses are logged as plain lines (no tensorboardX).  Only HardestContrastiveLossTrainer exists; the
data set is the 3DMatch pairs or the KITTI odometry pairs (`--dataset`).
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
DATASETS = ("ThreeDMatchPairDataset", "KITTINMPairDataset")
VAL_METRICS = ("feat_match_ratio", "success", "rte", "rre")
LOWER_IS_BETTER = ("rte", "rre")
# the options whose default depends on --dataset: (config_3dmatch.py, config_kitti.py)
DATASET_DEFAULTS = {"voxel_size": (0.025, 0.3), "hit_ratio_thresh": (0.1, 0.3), "use_random_scale": (False, True),
                    "best_val_metric": ("feat_match_ratio", "success")}
LOG = logging.getLogger("imfnet_amd.train")


def str2bool(v):
    return str(v).lower() in ("true", "1", "yes", "y", "t")


def make_parser():
    """config_3dmatch.py's / config_kitti.py's options that the hardest-contrastive path reads, with upstream's names
    and defaults.  The four options of DATASET_DEFAULTS parse to None when absent; parse_config fills them in."""
    p = argparse.ArgumentParser(prog="python -m imfnet_amd.train",
                                description="Train IMFNet with the hardest-contrastive loss on 3DMatch or KITTI "
                                            "odometry pairs (GPU).")
    a = p.add_argument
    a("--dataset", type=str, default="ThreeDMatchPairDataset", choices=DATASETS)
    a("--kitti_root", type=str, default="data/kitti", help="holds dataset/sequences, dataset/poses and the icp/ cache")
    a("--own_image", type=str2bool, default=False, help="KITTI: fragment 1 with its own image (upstream reads t0's twice)")
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
    a("--use_random_scale", type=str2bool, default=None, help="default: false (3DMatch), true (KITTI)")
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
    a("--hit_ratio_thresh", type=float, default=None, help="default: 0.1 (3DMatch), 0.3 (KITTI)")
    a("--model", type=str, default="ResUNetBN2C")
    a("--model_n_out", type=int, default=32)
    a("--conv1_kernel_size", type=int, default=5)
    a("--normalize_feature", type=str2bool, default=True)
    a("--best_val_metric", type=str, default=None,
      help=f"one of {', '.join(VAL_METRICS)}; default: feat_match_ratio (3DMatch), success (KITTI)")
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
    a("--voxel_size", type=float, default=None, help="default: 0.025 (3DMatch), 0.3 (KITTI)")
    a("--threed_match_dir", type=str, default="data/threedmatch")
    a("--overlap_path", type=str, default="data/overlap30")
    a("--train_list", type=str, default=None,
      help="scene list of the train phase (config/train_3dmatch.txt format; KITTI: sequence numbers, train_kitti.txt)")
    a("--val_list", type=str, default=None,
      help="scene list of the val phase (config/val_3dmatch.txt format; KITTI: sequence numbers, val_kitti.txt)")
    a("--image_W", type=int, default=160)
    a("--image_H", type=int, default=120)
    a("--seed", type=int, default=0)
    a("--norm_kernels", type=str, default="torch", choices=("torch", "hip"),
      help="the norms of the sparse path -- training-mode BatchNorm, and the InstanceNorm of the ResUNetIN2* residual "
           "blocks --: torch ops, or the fused deterministic HIP kernels (fp64 statistics in a fixed order, ReLU and "
           "residual add folded in, no host wait)")
    a("--loss_kernels", type=str, default="torch", choices=("torch", "hip"),
      help="the hardest-contrastive loss and its gradient: torch ops, or the deterministic HIP kernels "
           "(fp64 terms in a fixed order, no host wait)")
    a("--fusion_kernels", type=str, default="torch", choices=("torch", "hip"),
      help="the bottleneck point <-> image attention block and its gradients: torch ops per batch item, or the "
           "deterministic HIP kernels (all items in one call, fixed summation order, no host wait)")
    a("--image_kernels", type=str, default="torch", choices=("torch", "hip"),
      help="the image encoder (16 convolutions, 16 BatchNorm2d, the max pool) and its gradients: torch modules, or the "
           "deterministic HIP kernels over static pixel tables (fixed summation order, no floating-point atomics)")
    a("--optim_kernels", type=str, default="torch", choices=("torch", "hip"),
      help="the SGD step: torch.optim.SGD, or one HIP launch over every parameter that also leaves the packed operand "
           "images of the convolution weights, so that an iteration packs no weight again")
    a("--head_kernels", type=str, default="torch", choices=("torch", "hip"),
      help="the descriptor head (concatenation with the stride-1 skip, conv1_tr, ReLU, final, L2 normalisation) and its "
           "gradients: torch ops, or the deterministic HIP kernels (one forward and one backward call, fixed summation "
           "order, no host wait)")
    return p


def parse_config(argv=None):
    cfg = make_parser().parse_args(argv)
    if cfg.trainer not in TRAINERS:
        raise SystemExit(f"--trainer {cfg.trainer}: only {', '.join(TRAINERS)} is implemented "
                         f"(the plain-contrastive and triplet trainers are not)")
    if cfg.optimizer != "SGD" or cfg.scheduler != "ExpLR":
        raise SystemExit("only --optimizer SGD with --scheduler ExpLR is implemented")
    kitti = cfg.dataset == "KITTINMPairDataset"
    for name, by_dataset in DATASET_DEFAULTS.items():
        if getattr(cfg, name) is None:
            setattr(cfg, name, by_dataset[int(kitti)])
    if cfg.best_val_metric not in VAL_METRICS:
        raise SystemExit(f"--best_val_metric {cfg.best_val_metric}: one of {', '.join(VAL_METRICS)}")
    return cfg


def is_better(metric, value, best):
    """Whether a validation value beats the best one so far: lower for rte / rre, higher for the other two (upstream
    compares `best < value` for all four, which keeps the worst rte / rre).  NaN never wins."""
    return bool(value < best) if metric in LOWER_IS_BETTER else bool(value > best)


def worst_value(metric):
    return np.inf if metric in LOWER_IS_BETTER else -np.inf


def _sparse_input(xyz_list, feats, voxel, device, quantize="f64"):
    """One batched sparse tensor from the items' voxel representatives (rows grouped by item in first-occurrence order,
    the same rows as the items' own voxelisation) with the given per-voxel input features.  quantize: the data set's
    voxel arithmetic ("f32": the representatives go back to the float32 values the KITTI loader quantised)."""
    from ..extract import sparse_tensor_from_points, start_geometry
    if quantize == "f32":
        xyz_list = [x.float() for x in xyz_list]
    fut = (start_geometry(list(xyz_list), voxel, device, quantize=quantize) if len(xyz_list) > 1
           else start_geometry(xyz_list[0], voxel, device, quantize=quantize))
    st, inds = sparse_tensor_from_points(None, voxel, device, geometry=fut, quantize=quantize)
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
        from .. import ops
        ops.set_train_norm(getattr(config, "norm_kernels", "torch"))
        ops.set_train_loss(getattr(config, "loss_kernels", "torch"))
        ops.set_train_fusion(getattr(config, "fusion_kernels", "torch"))
        ops.set_train_image(getattr(config, "image_kernels", "torch"))
        ops.set_train_optim(getattr(config, "optim_kernels", "torch"))
        ops.set_train_head(getattr(config, "head_kernels", "torch"))
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
        if ops.TRAIN_OPTIM == "hip":
            from .optim import FusedSGD                       # one launch per step; a checkpoint of either loads into both
            self.optimizer = FusedSGD(self.model.parameters(), lr=config.lr, momentum=config.momentum,
                                      weight_decay=config.weight_decay, model=self.model)
        else:
            self.optimizer = torch.optim.SGD(self.model.parameters(), lr=config.lr, momentum=config.momentum,
                                             weight_decay=config.weight_decay)
        self.scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, config.exp_gamma)
        self.train_set, self.val_set = train_set, val_set
        self.start_epoch = 1
        self.best_val_metric = config.best_val_metric
        self.best_val, self.best_val_epoch = worst_value(self.best_val_metric), -np.inf
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
            st = _sparse_input(pts, batch[f"sinput{side}_F"], c.voxel_size, dev,
                               getattr(self.train_set, "quantize", "f64"))
            outs.append(self.model(st, batch["image" + side].to(dev)).F)
        return outs

    def train_step(self, raws, timings=None):
        """One optimizer step over iter_size batches of decoded pairs (`raws`: iter_size lists of dataset.load
        results).  Returns (loss, pos, neg) summed over the accumulation as upstream logs them."""
        c = self.config
        self.model.train()
        self.optimizer.zero_grad()
        tot = [0.0, 0.0, 0.0]
        n_batches = 0
        for raw_batch in raws:
            items = [it for it in (self.train_set.prepare(r, timings) for r in raw_batch) if it is not None]
            if not items:                                     # every pair of the batch was skipped (and logged)
                continue
            batch = collate_pair_fn(items)
            n_batches += 1
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
        if not n_batches:                                     # nothing accumulated: no step
            return tuple(tot)
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
        """lib/trainer.py:332-414: over at most val_max_iter pairs, find_corr on a 5 000-row subsample, the robust
        transform of the correspondences, then loss (corr_dist over all of xyz0, clamped at 1), RTE, RRE (left out of
        its mean when NaN; the mean itself is NaN when nothing entered it, and so is rte's, and NaN never is the best
        epoch), success (rte < 2 and rre < 5 deg), hit ratio and feat_match_ratio.  One device-to-host copy per pair.  A flagged estimate
        (matching.robust_transform: ok false) counts as rre = NaN, success = 0, rte against the identity.  fp64
        (upstream: float32), and the cosine of rre is clipped to [-1, 1], so only a flagged estimate gives NaN.  A pair that the data set skips (too few positive pairs) is left out."""
        from ..matching import nn_search, robust_transform_device
        c, dev = self.config, self.device
        self.model.eval()
        self.val_set.reset_seed(0)
        rng = np.random.default_rng(c.seed)
        n = len(self.val_set) if c.val_max_iter <= 0 else min(c.val_max_iter, len(self.val_set))
        hits, fmr, losses, rtes, rres, succ = [], [], [], [], [], []
        for idx in range(n):
            it = self.val_set.prepare(self.val_set.load(idx))
            if it is None:
                continue
            Fs = []
            for side in "01":
                st = _sparse_input([it["xyz" + side]], None, c.voxel_size, dev,
                                   getattr(self.val_set, "quantize", "f64"))
                Fs.append(self.model(st, torch.as_tensor(it["image" + side])[None].to(dev)).F)
            xyz0, xyz1 = it["xyz0"], it["xyz1"]
            F0, F1 = Fs
            if len(F0) > 5000:                                   # find_corr(subsample_size=5000)
                i0 = torch.as_tensor(rng.choice(len(F0), min(len(F0), 5000), replace=False)).to(dev)
                i1 = torch.as_tensor(rng.choice(len(F1), min(len(F1), 5000), replace=False)).to(dev)
                nn = nn_search(F0[i0].contiguous(), F1[i1].contiguous()).long()
                x0, x1 = xyz0[i0], xyz1[i1[nn.clamp_min(0)]]
            else:
                nn = nn_search(F0.contiguous(), F1.contiguous()).long()
                x0, x1 = xyz0, xyz1[nn.clamp_min(0)]
            found = nn >= 0        # nn_search: -1 = no neighbour (a non-finite feature row); row 0 stands in, never a hit
            T = torch.as_tensor(it["trans"], dtype=torch.float64, device=dev)
            raw = robust_transform_device(x0.contiguous(), x1.contiguous())
            x0 = x0 @ T[:3, :3].t() + T[:3, 3]
            dist = torch.sqrt(((x0 - x1) ** 2).sum(1) + 1e-6)
            hr_dev = ((dist < c.hit_ratio_thresh) & found).double().mean()
            T_est = raw[:128].view(torch.float64).reshape(4, 4)
            d = (xyz0 @ T_est[:3, :3].t() + T_est[:3, 3]) - (xyz0 @ T[:3, :3].t() + T[:3, 3])
            loss = torch.clamp(torch.sqrt((d ** 2).sum(1)), max=1.0).mean()        # corr_dist, lib/metrics.py:13-19
            # the pair's one device-to-host copy and host wait: T (16), the flag, the hit ratio, the loss
            host = torch.cat([T_est.reshape(16), raw[128:132].view(torch.int32).double(), hr_dev.reshape(1),
                              loss.reshape(1)]).cpu().numpy()
            Te, ok, hr, loss = host[:16].reshape(4, 4), not bool(host[16]), float(host[17]), float(host[18])
            hits.append(hr)
            fmr.append(float(hr > 0.05))
            Tg = np.asarray(it["trans"], dtype=np.float64)
            rte = float(np.linalg.norm(Te[:3, 3] - Tg[:3, 3]))
            # two rotations: the cosine leaves [-1, 1] by rounding only (an exact estimate gives 1 + 1e-16), so it is
            # clipped; upstream's float32 arccos answers NaN there and the pair counts as a failure
            cos = np.clip((np.trace(Te[:3, :3].T @ Tg[:3, :3]) - 1) / 2, -1.0, 1.0)
            rre = float(np.arccos(cos)) if ok else float("nan")
            losses.append(loss)
            rtes.append(rte)
            if not np.isnan(rre):
                rres.append(rre)
            succ.append(float(rte < 2 and not np.isnan(rre) and rre < np.pi / 180 * 5))

        def mean(v, empty=0.0):
            return float(np.mean(v)) if v else empty
        # an empty rte / rre mean is NaN, not upstream's 0: lower is better for them, and 0 would win the selection
        nan = float("nan")
        out = {"loss": mean(losses), "rre": mean(rres, nan), "rte": mean(rtes, nan), "feat_match_ratio": mean(fmr),
               "hit_ratio": mean(hits), "success": mean(succ)}
        LOG.info(f"Final Loss: {out['loss']:.3f}, RTE: {out['rte']:.3f}, RRE: {out['rre']:.3f}, "
                 f"Hit Ratio: {out['hit_ratio']:.3f}, Feat Match Ratio: {out['feat_match_ratio']:.3f}")
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
            if val is not None and is_better(self.best_val_metric, val[self.best_val_metric], self.best_val):
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


def make_data_set(cfg, phase, list_path, seed):
    if cfg.dataset == "KITTINMPairDataset":
        from ..kitti import read_test_sequences
        from .data import KITTINMPairDataset
        return KITTINMPairDataset(phase, read_test_sequences(list_path), cfg, seed=seed)
    from .data import IndoorPairDataset, read_scene_list
    return IndoorPairDataset(phase, read_scene_list(list_path), cfg, seed=seed)


def main(argv=None):
    cfg = parse_config(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s", datefmt="%m/%d %H:%M:%S",
                        stream=sys.stdout)
    kitti = cfg.dataset == "KITTINMPairDataset"
    what = "the sequence numbers of config/train_kitti.txt" if kitti else "a scene list in config/train_3dmatch.txt's format"
    if not cfg.train_list:
        raise SystemExit(f"--train_list is required ({what})")
    train_set = make_data_set(cfg, cfg.train_phase, cfg.train_list, cfg.seed)
    val_set = None
    if cfg.test_valid:
        if not cfg.val_list:
            raise SystemExit("--val_list is required with --test_valid true")
        val_set = make_data_set(cfg, cfg.val_phase, cfg.val_list, 0)
    LOG.info(f"{len(train_set)} training pairs, {len(val_set) if val_set else 0} validation pairs")
    HardestContrastiveTrainer(cfg, train_set, val_set).train()
    return 0
