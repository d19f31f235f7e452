"""Float64 NumPy restatement of the two calls of csrc/loss.hip (imf_hc_loss_forward / imf_hc_loss_backward): the
hardest-contrastive loss of lib/trainer.py:440-493 for given samples, and its gradient by the closed form.

With (i_s, j_s) = pairs[pos_sel[s]], a_s = f0[i_s], b_s = f1[j_s]:
  hard01[s] = sel1[argmin_k |a_s - f1[sel1[k]]|^2]   (first minimum), hard10[s] = sel0[argmin_k |b_s - f0[sel0[k]]|^2];
  keep01[s] = (i_s, hard01[s]) is not one of the pairs; keep10[s] = (hard10[s], j_s) is not one of the pairs;
  pos_loss  = mean relu(|a - b|^2 - pos_thresh);
  neg_loss  = (mean_keep01 relu(neg_thresh - D01)^2 + mean_keep10 relu(neg_thresh - D10)^2) / 2, D = sqrt(|.|^2 + 1e-7);
  gradient  cP_s (a - b) with cP_s = gp 2 / n_pos where the hinge is open; c01_s (a - h) with
            c01_s = -gn relu(neg_thresh - D01) / (count01 D01) where kept -- on the anchor's row, and the opposite on the
            other row.  An empty keep set gives a NaN mean and no gradient.
Distances are evaluated as sums of squared differences in float64 (the inputs are float32 values, so the differences
are exact).  `abs_terms0` / `abs_terms1` hold per element the sum of the absolute values of the addends: the scale of
the kernels' one rounding.
"""
import numpy as np

EPS = 1e-7


def dist2_matrix(A, B, chunk=256):
    """[len(A), len(B)] float64 squared distances as sums of squared differences."""
    out = np.empty((len(A), len(B)), dtype=np.float64)
    for r in range(0, len(A), chunk):
        d = A[r:r + chunk, None, :] - B[None, :, :]
        out[r:r + chunk] = (d * d).sum(2)
    return out


def restate(f0, f1, pairs, sel0, sel1, pos_sel, pos_thresh, neg_thresh, grad=(1.0, 1.0)):
    """Everything the two entry points define, in float64.  pos_sel None = every pair in order."""
    f0, f1 = np.asarray(f0, dtype=np.float64), np.asarray(f1, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64)
    sel0, sel1 = np.asarray(sel0, dtype=np.int64), np.asarray(sel1, dtype=np.int64)
    sp = pairs if pos_sel is None else pairs[np.asarray(pos_sel, dtype=np.int64)]
    i, j = sp[:, 0], sp[:, 1]
    n_pos = len(sp)
    a, b = f0[i], f1[j]
    m01, m10 = dist2_matrix(a, f1[sel1]), dist2_matrix(b, f0[sel0])
    k01, k10 = m01.argmin(1), m10.argmin(1)                          # numpy's argmin: the first minimum
    hard01, hard10 = sel1[k01], sel0[k10]
    M = max(len(f0), len(f1))
    keys = np.unique(pairs[:, 0] + pairs[:, 1] * M)
    keep01 = ~np.isin(i + hard01 * M, keys)
    keep10 = ~np.isin(hard10 + j * M, keys)
    d2p = ((a - b) ** 2).sum(1)
    h01, h10 = f1[hard01], f0[hard10]
    D01 = np.sqrt(((a - h01) ** 2).sum(1) + EPS)
    D10 = np.sqrt(((b - h10) ** 2).sum(1) + EPS)
    r01, r10 = np.maximum(neg_thresh - D01, 0.0), np.maximum(neg_thresh - D10, 0.0)
    n01, n10 = int(keep01.sum()), int(keep10.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        pos_loss = np.maximum(d2p - pos_thresh, 0.0).sum() / n_pos
        neg_loss = (np.float64((r01 ** 2)[keep01].sum()) / n01 + np.float64((r10 ** 2)[keep10].sum()) / n10) / 2

    gp, gn = float(grad[0]), float(grad[1])
    cP = np.where(d2p - pos_thresh > 0, gp * 2.0 / n_pos, 0.0)
    c01 = np.where(keep01, -gn * r01 / (max(n01, 1) * D01), 0.0)
    c10 = np.where(keep10, -gn * r10 / (max(n10, 1) * D10), 0.0)
    df0, df1 = np.zeros_like(f0), np.zeros_like(f1)
    ab0, ab1 = np.zeros_like(f0), np.zeros_like(f1)
    touched0, touched1 = np.zeros(len(f0), dtype=bool), np.zeros(len(f1), dtype=bool)
    for rows, add, df, ab, touched in (
            (i, cP[:, None] * (a - b), df0, ab0, touched0), (i, c01[:, None] * (a - h01), df0, ab0, touched0),
            (hard10, c10[:, None] * (h10 - b), df0, ab0, touched0),
            (j, cP[:, None] * (b - a), df1, ab1, touched1), (j, c10[:, None] * (b - h10), df1, ab1, touched1),
            (hard01, c01[:, None] * (h01 - a), df1, ab1, touched1)):
        np.add.at(df, rows, add)
        np.add.at(ab, rows, np.abs(add))
        touched[rows] = True
    return {"pos_loss": float(pos_loss), "neg_loss": float(neg_loss), "hard01": hard01, "hard10": hard10,
            "keep01": keep01, "keep10": keep10, "count01": n01, "count10": n10, "df0": df0, "df1": df1,
            "abs_terms0": ab0, "abs_terms1": ab1, "touched0": touched0, "touched1": touched1, "d2_pos": d2p,
            "dist2_01": m01, "dist2_10": m10, "D01": D01, "D10": D10}


def min_gap(dist2, db):
    """The smallest difference, over the queries, between the two smallest squared distances to DISTINCT database rows
    (bit-identical rows count as one); inf with one distinct row."""
    db = np.ascontiguousarray(db)
    _, first = np.unique(db.view(np.dtype((np.void, db.dtype.itemsize * db.shape[1]))).ravel(), return_index=True)
    d = dist2[:, np.sort(first)]
    if d.shape[1] < 2:
        return np.inf
    part = np.partition(d, 1, axis=1)
    return float((part[:, 1] - part[:, 0]).min())
