"""The hardest-contrastive loss of lib/trainer.py:440-493 (`contrastive_hardest_negative_loss`).

Restated term by term:
  sel0, sel1  min(N, num_hn_samples) rows of F0 / F1 drawn without replacement;
  pos_sel     num_pos of the positive pairs drawn without replacement when there are more than that;
  D01ind      the row of subF1 nearest to every posF0 row (and D10ind: of subF0 to posF1), found by `nn_search`
              (imf_nn_search: exact, fp64 distances, ties to the lowest index) on detached features.  Upstream builds
              the [num_pos, num_hn] `pdist` matrix and takes `.min(1)`; here no such matrix exists;
  D01         sqrt(|posF0 - subF1[D01ind]|^2 + 1e-7), computed again in torch so that autograd sees it.  min() routes
              its gradient to the argmin only, so this is exactly the gradient of upstream's pdist(...).min(1);
  mask        a hardest negative is dropped when its pair is a positive: key i + j * max(N0, N1) (util/misc.py
              `_hash`), injective, so `torch.isin` over int64 keys on the device is exact;
  pos_loss    relu(|posF0 - posF1|^2 - pos_thresh).mean();
  neg_loss    (relu(neg_thresh - D01)^2[mask0].mean() + relu(neg_thresh - D10)^2[mask1].mean()) / 2.

Randomness: upstream draws the samples from the global `np.random` stream, which nothing seeds and which the data
loader's workers share, so no run of it can be reproduced.  Here the draws come from a `numpy.random.Generator` the
caller owns (the trainer seeds it from --seed), in the order sel0, sel1, pos_sel.

Kernels (`kernels=`, default ops.TRAIN_LOSS): "torch" is the body described above; "hip" draws the same samples from
the same `rng` and hands them to csrc/loss.hip (autograd.HardestContrastiveLossFunction): the same quantities with every
term in fp64 and every sum in a fixed order, forward and backward, without a host wait.
"""
import numpy as np
import torch
import torch.nn.functional as F_

from ..matching import nn_search


def hash_keys(i, j, hash_seed):
    """util/misc.py `_hash` of the columns (i, j) with M = hash_seed: i + j * M, int64."""
    return i.long() + j.long() * int(hash_seed)


def sample_indices(rng, N0, N1, n_pos_pairs, num_pos, num_hn_samples):
    """(sel0, sel1, pos_sel) as upstream draws them; pos_sel is None when every positive pair is kept."""
    sel0 = rng.choice(N0, min(N0, num_hn_samples), replace=False)
    sel1 = rng.choice(N1, min(N1, num_hn_samples), replace=False)
    pos_sel = rng.choice(n_pos_pairs, num_pos, replace=False) if n_pos_pairs > num_pos else None
    return sel0, sel1, pos_sel


def _dev_index(a, device):
    return torch.as_tensor(np.asarray(a, dtype=np.int64)).to(device)


def hardest_contrastive_loss(F0, F1, positive_pairs, num_pos=5192, num_hn_samples=2048, pos_thresh=0.1,
                             neg_thresh=1.4, rng=None, sel0=None, sel1=None, pos_sel=None, return_indices=False,
                             kernels=None):
    """(pos_loss, neg_loss) of lib/trainer.py:440-493.  F0 [N0, C], F1 [N1, C] device float32 (with autograd);
    positive_pairs: [P, 2] integer tensor of (row of F0, row of F1).  Draws sel0 / sel1 / pos_sel from `rng` unless
    they are given (pos_sel=None with more than num_pos pairs and no rng is an error).  return_indices=True also
    returns the hardest negatives as global rows: (D01ind into F1, D10ind into F0), int64 device tensors.
    kernels: "torch" or "hip" (csrc/loss.hip); None reads ops.TRAIN_LOSS."""
    from .. import ops
    kernels = ops.TRAIN_LOSS if kernels is None else kernels
    if kernels not in ops.TRAIN_LOSS_CHOICES:
        raise ops.ImfError(f"loss kernels {kernels!r}: one of {', '.join(ops.TRAIN_LOSS_CHOICES)}")
    dev = F0.device
    N0, N1 = F0.shape[0], F1.shape[0]
    P = positive_pairs.shape[0]
    if P == 0:
        raise ValueError("hardest_contrastive_loss: no positive pairs")
    hash_seed = max(N0, N1)
    if sel0 is None or sel1 is None or (pos_sel is None and P > num_pos):
        if rng is None:
            raise ValueError("hardest_contrastive_loss: pass rng, or sel0, sel1 and pos_sel")
        d0, d1, dp = sample_indices(rng, N0, N1, P, num_pos, num_hn_samples)
        sel0 = d0 if sel0 is None else sel0
        sel1 = d1 if sel1 is None else sel1
        pos_sel = dp if pos_sel is None else pos_sel
    pairs = positive_pairs.to(dev).long()
    if kernels == "hip":
        from ..autograd import HardestContrastiveLossFunction
        out = HardestContrastiveLossFunction.apply(F0, F1, pairs.contiguous(),
                                                   None if pos_sel is None else _dev_index(pos_sel, dev),
                                                   _dev_index(sel0, dev), _dev_index(sel1, dev), pos_thresh, neg_thresh)
        return out if return_indices else out[:2]
    sample = pairs if pos_sel is None else pairs[_dev_index(pos_sel, dev)]
    s0, s1 = _dev_index(sel0, dev), _dev_index(sel1, dev)
    subF0, subF1 = F0[s0], F1[s1]
    pos_ind0, pos_ind1 = sample[:, 0], sample[:, 1]
    posF0, posF1 = F0[pos_ind0], F1[pos_ind1]

    d01 = nn_search(posF0.detach().float().contiguous(), subF1.detach().float().contiguous()).long()
    d10 = nn_search(posF1.detach().float().contiguous(), subF0.detach().float().contiguous()).long()
    # nn_search answers -1 for a row without a neighbour (a non-finite feature row): gather row 0 instead of wrapping to
    # the last row, and leave the pair out of the negative term
    has01, has10 = d01 >= 0, d10 >= 0
    d01, d10 = d01.clamp_min(0), d10.clamp_min(0)
    D01min = torch.sqrt((posF0 - subF1[d01]).pow(2).sum(1) + 1e-7)
    D10min = torch.sqrt((posF1 - subF0[d10]).pow(2).sum(1) + 1e-7)

    pos_keys = hash_keys(pairs[:, 0], pairs[:, 1], hash_seed)
    D01ind, D10ind = s1[d01], s0[d10]
    mask0 = ~torch.isin(hash_keys(pos_ind0, D01ind, hash_seed), pos_keys) & has01
    mask1 = ~torch.isin(hash_keys(D10ind, pos_ind1, hash_seed), pos_keys) & has10
    pos_loss = F_.relu((posF0 - posF1).pow(2).sum(1) - pos_thresh)
    neg_loss0 = F_.relu(neg_thresh - D01min[mask0]).pow(2)
    neg_loss1 = F_.relu(neg_thresh - D10min[mask1]).pow(2)
    out = (pos_loss.mean(), (neg_loss0.mean() + neg_loss1.mean()) / 2)
    return out + (D01ind, D10ind) if return_indices else out
