"""The evaluation path on the GPU against the catalogue of tests/matching_cases.py (proved on the CPU by
tests/test_matching_cases_host.py): imf_nn_search against exact arithmetic on the float32 rows, gated by the bound E of
csrc/matching.hip; imf_mutual_inliers and imf_select_keypoints bit for bit; imf_ransac_registration against the oracle
with the "no correspondence" rule, at the gates of test_gpu_matching.py::test_ransac_matches_oracle."""
import functools

import numpy as np
import pytest
import torch

import imf_oracle as O
import matching_cases as MC

pytestmark = pytest.mark.gpu

NN_CASES = MC.nn_shape_cases() + MC.nn_tie_cases() + MC.nn_zero_cases() + MC.nn_mixed_cases()
NN_NONFINITE = MC.nn_nonfinite_cases()
MUTUAL = MC.mutual_cases()
KEYPOINT = MC.keypoint_cases()
RANSAC = MC.ransac_cases()
CANARY = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def _nn_ref(name):
    c = next(c for c in NN_CASES if c.name == name)
    return MC.nn_reference(c.q, c.d)


def _search(q, d):
    from imfnet_amd.matching import nn_search
    nn, d2 = nn_search(torch.from_numpy(np.ascontiguousarray(q)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda(),
                       return_dist2=True)
    return nn.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("c", NN_CASES, ids=lambda c: c.name)
def test_nn_search_against_exact_arithmetic(c):
    """Index: the exact argmin wherever the gap rule pins it, within E(got) + E(argmin) of it everywhere, the lowest of
    bitwise equal rows always.  dist2 within 2 E.  Tie and zero-query cases name the row every query must return."""
    ref = _nn_ref(c.name)
    nn, d2 = _search(c.q, c.d)
    assert nn.dtype == np.int32 and nn.shape == (len(c.q),)
    bad = MC.nn_gate(c.q, c.d, ref, nn, d2)
    assert bad == [], "\n".join(bad[:8])
    if c.want is not None:
        assert np.array_equal(nn, c.want)
    from imfnet_amd.matching import knn_search
    assert np.array_equal(knn_search(c.q, c.d), nn)                            # without the distance output


@pytest.mark.parametrize("c", NN_NONFINITE, ids=lambda c: c.name)
def test_nn_search_non_finite_rows(c):
    """The affected queries, and only they, answer (-1, NaN); every other query answers what the same call gives with the
    non-finite rows removed, the indices shifted back, the distances bit for bit (a score does not depend on where its
    row sits)."""
    nn, d2 = _search(c.q, c.d)
    assert np.array_equal(nn < 0, c.bad_q) and (nn[c.bad_q] == -1).all()
    assert np.array_equal(np.isnan(d2), c.bad_q)
    if c.bad_d.all():
        return
    keep_q, keep_d = np.flatnonzero(~c.bad_q), np.flatnonzero(~c.bad_d)
    nn_clean, d2_clean = _search(c.q[keep_q], c.d[keep_d])
    assert np.array_equal(nn[keep_q], keep_d[nn_clean]) and np.array_equal(d2[keep_q], d2_clean)
    ref = MC.nn_reference(c.q[keep_q], c.d[keep_d])
    assert MC.nn_gate(c.q[keep_q], c.d[keep_d], ref, nn_clean, d2_clean) == []


def test_non_finite_rows_are_no_match_and_no_gather_wraps():
    """feature_match with a NaN row on each side: nn21 holds -1 for the NaN query, the NaN rows are never a mutual match,
    and the result is the one of the same call without those two keypoints."""
    from imfnet_amd.matching import feature_match
    rng = np.random.default_rng(12)
    d1, d2 = MC.unit_rows(rng, 90, 32), MC.unit_rows(rng, 70, 32)
    d2[:40] = d1[20:60] + 0.01 * MC.unit_rows(rng, 40, 32)
    k1 = rng.integers(-64, 64, (90, 3)) / 8.0
    k2 = rng.integers(-64, 64, (70, 3)) / 8.0
    k2[:40] = k1[20:60]
    d1n, d2n = d1.copy(), d2.copy()
    d1n[89, 4] = np.nan                                                        # the last row: where a -1 would wrap to
    d2n[5, 0] = np.nan
    inl, ratio, m2, nn21 = feature_match(k1, d1n, k2, d2n, np.eye(4), 0.1)
    inl0, ratio0, m20, nn210 = feature_match(k1[:89], d1[:89], np.delete(k2, 5, 0), np.delete(d2, 5, 0), np.eye(4), 0.1)
    assert nn21[5] == -1 and (np.delete(nn21, 5) == nn210).all() and 89 not in nn21
    assert inl == inl0 > 0 and ratio == ratio0 and np.array_equal(m2 - (m2 > 5), m20)


def test_loss_paths_mask_a_query_without_a_neighbour():
    """The hardest-contrastive loss on features with a NaN row on each side, through torch and through csrc/loss.hip: the
    pair whose anchor is NaN has no hardest negative (row sel1[0] stands in, the pair is left out of the negative term),
    the NaN row of F1 is nobody's negative, the negative loss is finite and the same on both paths."""
    from imfnet_amd.train.loss import hardest_contrastive_loss
    rng = np.random.default_rng(3)
    F0, F1 = MC.unit_rows(rng, 300, 32), MC.unit_rows(rng, 280, 32)
    pairs = np.stack([np.arange(100), rng.permutation(280)[:100]], 1)
    sel0, sel1 = rng.permutation(300)[:128], rng.permutation(280)[:128]
    bad1 = int(next(j for j in sel1[1:] if j not in pairs[:, 1]))              # a sampled F1 row that anchors no pair
    F0[pairs[17, 0], 3] = np.nan
    F1[bad1, 30] = np.nan
    out = {}
    for kernels in ("torch", "hip"):
        pos, neg, d01, d10 = hardest_contrastive_loss(torch.from_numpy(F0).cuda(), torch.from_numpy(F1).cuda(),
                                                      torch.from_numpy(pairs).cuda(), num_pos=100, sel0=sel0, sel1=sel1,
                                                      return_indices=True, kernels=kernels)
        out[kernels] = (float(pos), float(neg), d01.cpu().numpy(), d10.cpu().numpy())
        assert np.isfinite(out[kernels][1])                    # (the positive term reads the NaN anchor: not compared)
        assert out[kernels][2][17] == sel1[0] and bad1 not in out[kernels][2]
    assert np.array_equal(out["torch"][2], out["hip"][2]) and np.array_equal(out["torch"][3], out["hip"][3])
    assert abs(out["torch"][1] - out["hip"][1]) <= 1e-6 * abs(out["torch"][1])


# ---- mutual check and inliers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", MUTUAL, ids=lambda c: c.name)
def test_mutual_inliers_equal_the_reference(c):
    from imfnet_amd import _lib
    from imfnet_amd._lib import check
    import ctypes as C
    ref_m2, ref_inl = MC.mutual_reference(c)
    n2, n1 = len(c.nn21), len(c.nn12)
    nn21 = torch.from_numpy(c.nn21.copy()).cuda()
    nn12 = torch.from_numpy(c.nn12.copy()).cuda()
    match2 = torch.full((n2 + 8,), CANARY, dtype=torch.int32, device="cuda")
    meta = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    geo = c.kp1 is not None
    kp1 = torch.from_numpy(np.ascontiguousarray(c.kp1)).cuda() if geo else None
    kp2 = torch.from_numpy(np.ascontiguousarray(c.kp2)).cuda() if geo else None
    pose = np.ascontiguousarray(c.pose, np.float64) if geo else None
    check(_lib.lib().imf_mutual_inliers(nn21.data_ptr(), n2, nn12.data_ptr(), n1, kp1.data_ptr() if geo else None,
                                        kp2.data_ptr() if geo else None, pose.ctypes.data_as(C.c_void_p) if geo else None,
                                        float(c.thresh), match2.data_ptr(), meta.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "imf_mutual_inliers")
    n_matches, n_inl = meta.tolist()
    got = match2.cpu().numpy()
    assert n_matches == len(ref_m2) and np.array_equal(got[:n_matches], ref_m2)        # ascending, equal to the reference
    assert (got[n_matches:] == CANARY).all()                                           # nothing beyond the matches
    assert n_inl == ref_inl


# ---- keypoint selection ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", KEYPOINT, ids=lambda c: c.name)
def test_select_keypoints_equal_the_oracle(c):
    from imfnet_amd.matching import select_keypoints
    with np.errstate(invalid="ignore"):
        ref = O.select_keypoints(c.samples, c.coords, c.voxel)
    got = select_keypoints(c.samples, c.coords, c.voxel)
    assert got.dtype == ref.dtype == np.int64 and got.shape == ref.shape and np.array_equal(got, ref)
    assert np.array_equal(select_keypoints(c.samples, c.coords, c.voxel), got)


# ---- RANSAC --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RANSAC, ids=lambda c: c.name)
def test_ransac_equals_the_oracle(c):
    """Winning iteration, inlier count and meta[2] exact; T to 1e-9, fitness to 1e-15, rmse to 1e-12.  Two calls give the
    same bits."""
    from imfnet_amd.matching import ransac_registration
    args = (c.src, c.dst, c.corres, c.ransac_n, c.max_dist, c.edge, c.max_iter, c.seed)
    ref = O.ransac_registration(*args)
    got = ransac_registration(*args)
    print(f"{c.name}: winner {got[1]} / {ref[1]}, inliers {got[2]} / {ref[2]}, valid {got[3]} / {ref[3]}, "
          f"|dT| {np.abs(got[0] - ref[0]).max():.2e}, |dfit| {abs(got[4] - ref[4]):.2e}, |drmse| {abs(got[5] - ref[5]):.2e}")
    assert got[1] == ref[1] and got[2] == ref[2] and got[3] == ref[3]
    assert np.abs(got[0] - ref[0]).max() < 1e-9
    assert abs(got[4] - ref[4]) < 1e-15 and abs(got[5] - ref[5]) < 1e-12
    if ref[1] >= 0:
        assert MC.winner_count_longdouble(c, got[0]) == got[2]
    else:
        assert np.array_equal(got[0], np.eye(4)) and got[2] == 0 and got[4] == 0.0 and got[5] == 0.0
    if c.kind == "empty":
        assert got[1] == -1 and got[3] > 0
    if c.kind == "invalid" and not ((c.corres >= 0) & (c.corres < len(c.dst))).any():
        assert got[1] == -1 and got[3] == 0
    again = ransac_registration(*args)
    assert np.array_equal(again[0], got[0]) and again[1:] == got[1:]


def test_run_ransac_with_a_nan_descriptor_row_on_each_side():
    """End to end: the NaN query has no correspondence, the NaN target row is nobody's neighbour; the transform is
    finite and the one the oracle gives for the correspondences of the finite rows."""
    from imfnet_amd.matching import nn_search, run_ransac
    src, dst, f0, f1, voxel = MC.end_to_end_case()
    T = run_ransac(src, dst, f0, f1, voxel, ransac_n=3, seed=2)
    assert T.shape == (4, 4) and np.isfinite(T).all()
    corres = nn_search(torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda()).cpu().numpy()
    fin0, fin1 = np.isfinite(f0).all(1), np.isfinite(f1).all(1)
    want = np.full(len(f0), -1, np.int64)
    want[fin0] = np.flatnonzero(fin1)[O.knn_search(f0[fin0], f1[fin1])]
    assert np.array_equal(corres, want) and corres[7] == -1 and 11 not in corres
    ref = O.ransac_registration(src, dst, want, 3, voxel * 1.5, 0.9, 50000, 2)
    assert ref[1] >= 0 and np.abs(T - ref[0]).max() < 1e-9
