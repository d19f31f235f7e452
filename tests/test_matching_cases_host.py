"""Proof of the catalogue of tests/matching_cases.py on the CPU: every case meets the conditions it is named for, the
references agree with imf_oracle on generic data, and the shares of queries that the gap rule pins are computed from the
exact reference alone, printed (run with -s) and held to their caps."""
import functools

import numpy as np
import pytest

import imf_oracle as O
import matching_cases as MC

NN_SHAPES = MC.nn_shape_cases()
NN_TIES = MC.nn_tie_cases()
NN_ZERO = MC.nn_zero_cases()
NN_MIXED = MC.nn_mixed_cases()
NN_NONFINITE = MC.nn_nonfinite_cases()
MUTUAL = MC.mutual_cases()
KEYPOINT = MC.keypoint_cases()
RANSAC = MC.ransac_cases()


@functools.lru_cache(maxsize=None)
def _ref(group, name):
    c = next(c for c in group_cases(group) if c.name == name)
    return MC.nn_reference(c.q, c.d)


def group_cases(group):
    return {"shape": NN_SHAPES, "tie": NN_TIES, "zero": NN_ZERO, "mixed": NN_MIXED}[group]


# ---- nearest neighbour -------------------------------------------------------------------------------------------------
def test_exact_integers_restate_the_float32_values():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(50) * 10.0 ** rng.integers(-30, 30, 50), [0.0, -0.0, 1e-45, 3.4e38, -1.0]])
    x = x.astype(np.float32)
    (xi,), e = MC.exact_ints(x)
    for v, n in zip(x, xi):
        assert MC.Fraction(float(v)) == MC.Fraction(n) * MC.Fraction(2) ** e


def test_split_table_is_what_nn_splits_gives_and_covers_the_edges():
    for c in NN_SHAPES + NN_TIES + NN_ZERO + NN_MIXED:
        assert (c.splits, c.split_len) == MC.nn_splits(len(c.q), len(c.d)), c.name
        assert c.q.dtype == c.d.dtype == np.float32 and c.q.shape[1] == c.d.shape[1]
    shapes = {(c.q.shape[1], len(c.q), len(c.d)) for c in NN_SHAPES}
    for dim in (16, 32, 64):
        for nq in MC.NQ_EDGES:
            for nd in MC.ND_EDGES:
                assert (dim, nq, nd) in shapes
        assert (dim, 129, 4097) in shapes
    assert (32, 1000, 70) in shapes
    assert MC.nn_splits(64, 129) == (3, 64)                                   # nq <= 64: three splits of 64
    s, L = MC.nn_splits(129, 4097)
    assert (s, L) == (64, 128) and sum(1 for k in range(s) if k * L >= 4097) == 31     # 31 empty splits meet real ones
    s, L = MC.nn_splits(1000, 70)
    assert (s, L) == (2, 64) and 70 - L == 6                                  # the second split holds 6 rows


@pytest.mark.parametrize("dim", [16, 32, 64])
def test_generic_shapes_are_pinned_and_agree_with_the_oracle(dim):
    """At least 95 % of the queries of every generic case are pinned by the gap rule (computed from the exact reference
    alone); on those the oracle's fp64 search must give the exact argmin, and everywhere it must pass the gate."""
    worst = 1.0
    for c in NN_SHAPES:
        if c.q.shape[1] != dim:
            continue
        ref = _ref("shape", c.name)
        share = float(ref.pinned.mean())
        worst = min(worst, share)
        print(f"{c.name}: pinned {int(ref.pinned.sum())} of {len(c.q)} = {share:.3f}")
        assert share >= 0.95, c.name
        got = O.knn_search(c.q, c.d)
        assert (got[ref.pinned] == ref.argmin[ref.pinned]).all(), c.name
        assert MC.nn_gate(c.q, c.d, ref, got) == [], c.name
    print(f"dim {dim}: lowest pinned share {worst:.3f}")


@pytest.mark.parametrize("c", NN_TIES, ids=lambda c: c.name)
def test_tie_cases_hold_one_pair_of_equal_rows_that_is_nearest(c):
    ref = _ref("tie", c.name)
    a = int(c.want[0])
    pname = c.name[len("tie_"):].rsplit("_", 2)[0]
    b = MC.tie_pairs(len(c.d), c.split_len)[pname][1]
    assert MC.tie_pairs(len(c.d), c.split_len)[pname][0] == a < b < len(c.d)
    assert c.d[a].tobytes() == c.d[b].tobytes()
    fe = ref.first_equal
    assert fe[b] == a and (np.delete(fe, b) == np.delete(np.arange(len(c.d)), b)).all()      # the only equal rows
    assert (ref.argmin == a).all() and ref.pinned.all()                       # nearest to every query, by more than E
    # positions: what the pair is named for
    if pname == "next_lane":
        assert a // 16 == b // 16 and (a % 16) % 4 + 1 == (b % 16) % 4
    if pname == "next_register":
        assert a // 16 == b // 16 and (a % 16) % 4 == (b % 16) % 4 and (b % 16) // 4 == (a % 16) // 4 + 1
    if pname == "next_block":
        assert b == a + 16 and a // 64 == b // 64
    if pname == "next_tile":
        assert b == a + 64 and (a // c.split_len == b // c.split_len) == (c.split_len == 128)
    if pname == "across_split":
        assert a // c.split_len + 1 == b // c.split_len and b % c.split_len == 0
    d2 = ((c.d.astype(np.float64)[None] - c.q.astype(np.float64)[:, None]) ** 2).sum(-1)
    rest = np.delete(d2, [a, b], axis=1).min(1) / d2[:, a]
    assert (rest > 100.0).all() if "_far_" in c.name else ((rest > 1.5) & (rest < 20.0)).all()


@pytest.mark.parametrize("c", NN_ZERO, ids=lambda c: c.name)
def test_zero_query_cases(c):
    ref = _ref("zero", c.name)
    assert not c.q[0].any() and (np.linalg.norm(c.d.astype(np.float64), axis=1) > 0.2).all()
    assert (ref.argmin == c.want).all() and ref.pinned.all()
    assert len(c.d) == 1 or len(c.d) % c.split_len == 1                        # the last split holds one row


def test_mixed_magnitude_shares_are_reported():
    """No cap for these: the measured shares are printed here and recorded as a comment in the catalogue."""
    for c in NN_MIXED:
        ref = _ref("mixed", c.name)
        print(f"{c.name}: pinned {int(ref.pinned.sum())} of {len(c.q)} = {ref.pinned.mean():.3f}")
        assert MC.nn_gate(c.q, c.d, ref, O.knn_search(c.q, c.d)) == []
    x = NN_MIXED[0].d.astype(np.float64)
    assert (np.abs(x[:, 0] - 1000.0) <= 0.5).all() and (np.abs(x[:, 1:] - 1.0) <= 0.5).all()
    assert np.allclose(np.linalg.norm(NN_MIXED[1].d.astype(np.float64), axis=1), 2.0 ** -60, rtol=1e-6)
    assert np.allclose(np.linalg.norm(NN_MIXED[2].d.astype(np.float64), axis=1), 2.0 ** 40, rtol=1e-6)


def test_nonfinite_cases_plant_what_they_name():
    names = {c.name for c in NN_NONFINITE}
    assert {f"{side}_{v}" for side in ("query", "db") for v in ("nan", "pinf", "ninf")} | {"db_all_nonfinite"} <= names
    for c in NN_NONFINITE:
        assert (c.bad_d == ~np.isfinite(c.d).all(1)).all()
        assert (c.bad_q == (~np.isfinite(c.q).all(1) | c.bad_d.all())).all()   # no finite row left: every query is affected
        assert c.bad_q.any() or c.bad_d.any()
        if c.name == "db_all_nonfinite":
            assert c.bad_d.all() and {"nan", "inf", "-inf"} == {str(v) for v in c.d[:, 3]}
        elif c.name.startswith("db_"):
            assert list(np.flatnonzero(c.bad_d)) == [0, 63, 64, 149] and not c.bad_q.any()
        elif c.name.startswith("query_"):
            assert list(np.flatnonzero(c.bad_q)) == [0, 15, 16, 39] and not c.bad_d.any()


# ---- mutual check ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", MUTUAL, ids=lambda c: c.name)
def test_mutual_cases(c):
    m2, inl = MC.mutual_reference(c)
    n2, n1 = len(c.nn21), len(c.nn12)
    assert m2.dtype == np.int32 and (np.diff(m2) > 0).all()
    ok = (c.nn21 >= 0) & (c.nn21 < n1)
    if ok.all():                                                               # the oracle's statement, where it is defined
        assert np.array_equal(m2, O.mutual_match_indices(c.nn21, c.nn12))
    if c.name.endswith("_all"):
        assert len(m2) == int(ok.sum()) and (n2 < 63 or not ok.all())
    if c.name.endswith("_none"):
        assert len(m2) == 0
    if c.name.endswith("_chunk_edges"):
        want = sorted({j for c0 in range(0, n2, 1024) for j in (c0, min(c0 + 1023, n2 - 1))})
        assert list(m2) == want
    if n2 >= 63 and not c.name.endswith("_none") and c.name.startswith("n") and c.kp1 is not None:
        assert {-1, n1, MC.I32_MAX} <= set(c.nn21.tolist())
    if c.kp1 is not None and len(m2) > 2 and c.name.startswith("n"):
        assert 0 < inl < len(m2)                                               # both outcomes occur
    if c.kp1 is not None:                                                      # every distance^2 is exact and off the bound
        k2 = O.transform_points(c.kp2[m2], c.pose)
        d2 = ((c.kp1[c.nn21[m2]] - k2) ** 2).sum(1)
        assert (d2 * 2.0 ** 12 == np.round(d2 * 2.0 ** 12)).all()
        if not c.name.startswith("strict"):
            assert (np.abs(np.sqrt(d2) - c.thresh) > 1e-3).all()
    if c.name == "strict_at_equality":
        assert inl == 0 and c.thresh == 0.625 == float(np.sqrt(0.375 ** 2 + 0.5 ** 2))
    if c.name == "strict_above_equality":
        assert inl == 1
    if c.name.startswith("projective"):
        assert c.pose[3, 3] != 1.0 and 0 < inl < 65


# ---- keypoint selection ------------------------------------------------------------------------------------------------
def test_keypoint_cases():
    names = {c.name for c in KEYPOINT}
    for m in MC.KP_M:
        assert {f"m{m}_ns0", f"m{m}_ns1", f"m{m}_all_selected", f"m{m}_none_selected"} <= names
    with np.errstate(invalid="ignore"):
        refs = {c.name: O.select_keypoints(c.samples, c.coords, c.voxel) for c in KEYPOINT}
    for c in KEYPOINT:
        r = refs[c.name]
        assert r.dtype == np.int64 and np.isfinite(c.samples).all() and np.isfinite(c.coords).all()
        m = len(c.coords)
        if c.name.endswith("_ns0") or c.name.endswith("_none_selected"):
            assert len(r) == 0
        if c.name.endswith("_ns1"):
            assert len(c.samples) == 1 and len(r) >= min(m, 1)
        if c.name.endswith("_all_selected"):
            assert np.array_equal(r, np.arange(m))
        if c.name.endswith("_block_edges"):
            assert list(r) == sorted({k for b in range(0, m, 1024) for k in (b, min(b + 1023, m - 1))})
    rep = next(c for c in KEYPOINT if c.name == "repeated_samples")
    assert len(rep.samples) == 300 and len(np.unique(rep.samples, axis=0)) == 3
    assert {3, 700, 1499} <= set(refs["repeated_samples"].tolist()) and len(refs["repeated_samples"]) < 10
    neg = next(c for c in KEYPOINT if c.name == "negative_and_minus_zero")
    assert list(refs[neg.name])[:2] == [0, 4] and (np.signbit(neg.coords) & (neg.coords == 0)).any() and (neg.coords < 0).any()
    assert 0.15 / 0.05 < 3.0 and -0.15 / 0.05 > -3.0                           # the quotient rounds below the integer
    assert list(refs["face_quotient_rounds_below"]) == [0, 1, 2]
    big = next(c for c in KEYPOINT if c.name.startswith("quotients_beyond"))
    qt = np.abs(np.floor(big.coords / big.voxel))
    assert (qt > 2.0 ** 31).any() and (qt >= 2.0 ** 52 - 2).any() and (qt < 2.0 ** 53).all()
    assert list(refs[big.name]) == [1, 2, 4, 7, 8]
    assert list(refs["quotients_scaled_voxel"]) == [0, 3, 6]
    a, b = MC.colliding_cells()
    ka, kb = MC.cell_key(a), MC.cell_key(b)
    assert a != b and ka != kb and MC.hash64(ka) & 1023 == MC.hash64(kb) & 1023 and MC.hash_capacity(2) == 1024
    assert list(refs["shared_slot_absent_key"]) == [1]                         # the colliding cell's rows are not selected
    assert list(refs["shared_slot_both_present"]) == [0, 2]
    assert list(refs["shared_slot_other_order"]) == [1]


# ---- RANSAC --------------------------------------------------------------------------------------------------------------
def test_ransac_catalogue_covers_the_edges():
    names = {c.name for c in RANSAC}
    assert {f"iter_{it}" for it in MC.ITER_EDGES} <= names
    for n in MC.NSRC_EDGES:
        for rn in (3, 4):
            assert any(c.kind in ("generic", "tie") and len(c.src) == n and c.ransac_n == rn and c.name.startswith("nsrc")
                       for c in RANSAC)
    assert max(c.max_iter for c in RANSAC) <= 2048


@pytest.mark.parametrize("c", RANSAC, ids=lambda c: c.name)
def test_ransac_cases_are_decided_and_off_the_bounds(c):
    """The table of every hypothesis agrees with imf_oracle.ransac_registration; the winner is decided (one best
    hypothesis by more than 1e-9 in rmse, or exact ties); every distance of every valid hypothesis, every checker
    residual and every edge comparison is further than 1e-9 from its bound, except in the equality cases, which sit on
    it; the winner's count is the same with every distance in long double."""
    picks, ok, count, rmse, T, dis, resid, ds, dd = MC.ransac_table(c)
    ref = O.ransac_registration(c.src, c.dst, c.corres, c.ransac_n, c.max_dist, c.edge, c.max_iter, c.seed)
    assert ref[3] == int(ok.sum())
    cor = np.asarray(c.corres, np.int64)
    has = (cor >= 0) & (cor < len(c.dst))
    assert has[picks[ok]].all()                                                # a valid hypothesis drew no invalid entry
    if c.kind not in ("equality", "empty"):
        assert (np.abs(dis[ok][:, has] - c.max_dist) > 1e-9).all()
        sampled = has[picks].all(1)
        edges_pass = sampled & ~((ds < dd * c.edge) | (dd < ds * c.edge)).any(1)
        assert (np.abs(resid[edges_pass] - c.max_dist) > 1e-9).all()
        both = (ds[sampled] > 0) | (dd[sampled] > 0)                           # a repeated pick compares 0 with 0
        assert (np.abs(ds[sampled] - dd[sampled] * c.edge)[both] > 1e-9).all()
        assert (np.abs(dd[sampled] - ds[sampled] * c.edge)[both] > 1e-9).all()
    if not (count > 0).any():
        assert ref[1] == -1 and ref[2] == 0 and np.array_equal(ref[0], np.eye(4))
    else:
        best_c = count[ok].max()
        cand = np.flatnonzero(ok & (count == best_c))
        best_r = rmse[cand].min()
        close = cand[rmse[cand] <= best_r + 1e-9]
        assert len(close) == 1 or (rmse[close] == best_r).all(), "the winner hangs on rounding"
        assert ref[1] == close[0] and ref[2] == best_c
        assert MC.winner_count_longdouble(c, T[ref[1]]) == best_c
        if c.kind == "tie":
            assert len(close) > 1 and best_r == 0.0
    if c.kind == "empty":
        assert ref[3] > 0 and ref[1] == -1
    if c.name.startswith("iter_"):
        assert ok[0] and count[0] > 0 and len(c.src) == 200                     # even max_iter = 1 has a winner
    if c.name == "edge_check_at_equality":
        at = ok & ((dd == ds * c.edge) & (ds > 0)).any(1)
        assert at.any() and at[ref[1]] and ref[2] == 2                        # passes AT equality, and such a draw wins
    if c.name == "distance_check_at_equality":
        at = ok & (resid == c.max_dist).all(1)
        assert at.any() and (count[at] == 0).all() and ref[2] == 1
    if c.kind == "invalid":
        assert not has.all() and {-1, len(c.dst), MC.I32_MAX} <= set(cor[~has].tolist())
        if not has.any():
            assert ref[3] == 0 and ref[1] == -1
        else:
            assert 0 < ref[3] < c.max_iter and ref[1] >= 0 and abs(ref[4] - ref[2] / len(c.src)) == 0.0
    if c.name.startswith("nsrc1_"):
        assert ref[1] == 0 and ref[2] == 1 and ok.all()
    if c.name.startswith("nsrc2_"):
        assert len({tuple(p) for p in picks}) == 2 ** c.ransac_n and 0.5 ** c.ransac_n < ok.mean() < 4 * 0.5 ** c.ransac_n


def test_a_tie_case_starts_late_and_reaches_the_second_stride():
    """The tie tests can tell a wrong tie rule from a right one only if the earliest valid hypothesis is not iteration 0
    (so a higher thread holds the winner) and the ties reach beyond iteration 1024 (so a thread holds two of them)."""
    late = 0
    for c in RANSAC:
        if c.kind == "tie" and c.max_iter > 1024:
            ok = MC.ransac_table(c)[1]
            first = int(np.flatnonzero(ok)[0])
            late += first > 0 and ok[1024:].any() and ok[first + 1024 if first + 1024 < c.max_iter else first]
    assert late >= 1
    one = next(c for c in RANSAC if c.name == "nsrc1_rn3")
    assert one.max_iter > 1024                                                 # thread 0 holds iterations 0 and 1024, tied


def test_oracle_rule_for_invalid_correspondences_leaves_valid_sets_alone():
    """The "no correspondence" rule changes nothing for a set without such entries: the restatement with the rule and a
    plain restatement without it agree hypothesis by hypothesis."""
    c = next(c for c in RANSAC if c.name == "iter_1025")
    picks, ok, count, rmse, T = MC.ransac_table(c)[:5]
    import registration_cases as RC
    p2, ok2, count2, rmse2, T2 = RC.ransac_table(RC.RansacCase(*c[:9], "generic"))
    assert np.array_equal(picks, p2) and np.array_equal(ok, ok2) and np.array_equal(count, count2)
    assert np.array_equal(rmse, rmse2) and np.array_equal(T, T2)


def test_end_to_end_case_holds_one_nan_row_on_each_side():
    src, dst, f0, f1, voxel = MC.end_to_end_case()
    assert list(np.flatnonzero(~np.isfinite(f0).all(1))) == [7] and list(np.flatnonzero(~np.isfinite(f1).all(1))) == [11]
