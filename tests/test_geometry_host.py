"""The geometry restatement (tests/geometry_restate.py) and its case catalogue, checked on the CPU: against the oracle
(oracle/imf_oracle.py: 18-bit packed keys, a sort per lookup) and against the C twins (oracle/imf_cpu_twins.c: the library's
layouts, a sequential hash map) -- three statements of the same integer work that share no code -- and the conditions that make
every case the stress it claims to be.  tests/test_gpu_geometry_exact.py runs the same catalogue against the HIP kernels."""
import numpy as np
import pytest

import geometry_restate as R
import imf_cpu_twins as TW
import imf_oracle as O


class _Map:
    def __init__(self, rows, nbr, mask):
        self.tile_rows, self.nbr, self.tile_mask, self.n_slots = rows, nbr, mask, len(rows)


def _restated(name):
    """(level-0 rows, first indices or None, Geometry-shaped maps) of a case; a batched case is built from its batched points."""
    c = R.case(name)
    if c.n_items == 1:
        return R.geometry(name)
    pts, starts = c.batched_points()
    rows, first = R.voxelize(pts, c.vs, item_starts=starts)
    return rows, first, R.Geometry(rows)


def _assert_geometry_equal(g, ref, rows0):
    for i in range(4):
        assert np.array_equal(g.levels[i], ref.levels[i]), f"level {i}"
    assert np.array_equal(g.k_first, ref.k_first), R.first_difference(g.k_first, ref.k_first, rows0, 5)
    for i in range(4):
        assert np.array_equal(g.k3[i], ref.k3[i]), (i, R.first_difference(g.k3[i], ref.k3[i], g.levels[i]))
    for i in range(3):
        assert np.array_equal(g.down[i], ref.down[i]), (i, R.first_difference(g.down[i], ref.down[i], g.levels[i + 1]))
        assert np.array_equal(g.up[i], ref.up[i]), (i, R.first_difference(g.up[i], ref.up[i], g.levels[i]))


# ------------------------------------------------------------------------------------------------ the catalogue's conditions
def test_every_case_has_exact_points_and_shuffled_duplicates():
    for name in R.CASES:
        c = R.case(name)                                   # (the constructor asserts the exact quotient and floor)
        assert np.array_equal(np.floor(c.points / c.vs), c.coords[c.voxel_of])
        per = np.bincount(c.voxel_of, minlength=len(c.coords))
        assert per.min() >= 1 and (per.max() <= 6 or name in R.CHAINS)
        rows, first = c.rows()
        assert len(rows) == len(c.coords) and sorted(map(tuple, rows[:, 1:].tolist())) == sorted(map(tuple, c.coords.tolist()))
        if len(rows) > 100:
            assert not np.array_equal(rows[:, 1:], c.coords)                     # first-occurrence order is not the set's order
    for name in ("solid", "far_negative", "faces", "large"):
        assert R.case(name).dup_span() > 1024              # duplicates of one voxel in different 1 024-point workgroups


def test_solid_interior_has_every_neighbour():
    rows, _, g = R.geometry("solid")
    inner3 = (np.abs(rows[:, 1:] + 0.5) < 19).all(1)       # -19 .. 18
    inner5 = (np.abs(rows[:, 1:] + 0.5) < 18).all(1)
    assert inner3.sum() == 38 ** 3 and (g.k3[0][inner3] >= 0).all()
    assert inner5.sum() == 36 ** 3 and (g.k_first[inner5] >= 0).all()
    assert (g.k3[0][~inner3] < 0).any(axis=1).all()


def test_faces_every_out_of_range_probe_direction_has_an_occupied_alias():
    rows, _, g = R.geometry("faces")                       # (the builder asserts the same on the coordinate set)
    rep = R.faces_alias_report(rows)
    for i in range(4):
        assert (rep[f"k3@{1 << i}"][list(R.AXIS_K3)] > 0).all()
    assert rep["k5@1"][[60, 61, 63, 64, 52, 57, 67, 72, 12, 37, 87, 112]].min() > 0       # the 12 axis-aligned 5x5x5 offsets
    assert all(rep[f"down{1 << i}"].sum() > 0 and rep[f"up{1 << i}"].sum() > 0 for i in range(3))
    # and the restated maps hold -1 at every one of them: a row on the +x face has no +x neighbour although -2^17 is occupied
    on_hi = rows[:, 1] == R.LIM - 1
    assert on_hi.any() and (g.k3[0][on_hi][:, 14] == -1).all() and (g.k_first[on_hi][:, [63, 64]] == -1).all()
    assert rows[:, 1:].min() == -R.LIM and rows[:, 1:].max() == R.LIM - 1


def test_chains_predict_long_probe_sequences():
    for shift, name in enumerate(R.CHAINS):
        c = R.case(name)
        assert c.n_points <= 512 and TW._capacity(c.n_points) == 1024
        assert c.predicted_probes.max() >= 8 and (c.predicted_probes > 1).sum() > 200, c.predicted_probes.max()
        assert (c.coords % (4 << shift) == 0).all()


def test_lattices_have_the_inactive_offsets_and_empty_classes_they_claim():
    for name in ("even", "odd", "parity101"):
        rows, _, g = R.geometry(name)
        off_centre = [k for k in range(27) if k != 13]
        assert (g.k3[0][:, off_centre] == -1).all() and (g.k3[0][:, 13] == np.arange(len(rows))).all()
        assert len(np.unique(R.parity_class(rows, 1))) == 1
        n = (len(rows) + 63) // 64 * 64
        assert (g.up_rows[0][:len(rows)] >= 0).all() and (g.up_rows[0][n:] == -1).all()    # seven classes take no tile
    rows, _, g = R.geometry("parity_ts2")
    assert len(np.unique(R.parity_class(g.levels[1], 2))) == 1 and len(np.unique(R.parity_class(rows, 1))) == 8
    rows, _, g = R.geometry("spacing3")
    assert (g.k3[0][:, [k for k in range(27) if k != 13]] == -1).all() and (g.k3[1] >= 0).sum() > len(g.levels[1])


def test_small_and_large_sizes():
    assert [len(R.case(n).coords) for n in R.SMALL] == [1, 2, 63, 64, 65, 18]
    big = R.case("large")
    assert len(big.coords) >= 10 ** 6 and TW._capacity(big.n_points) >= 1 << 21
    # x-fastest offset order: the 7-voxel line along x has -x / +x neighbours at k = 12 / 14 and nowhere else
    rows, _, g = R.geometry("lines")
    on_x = np.flatnonzero((rows[:, 2] == 0) & (rows[:, 3] == 0) & (np.abs(rows[:, 1]) <= 3))
    assert len(on_x) == 7
    for o in on_x:
        want = {13} | ({12} if rows[o, 1] > -3 else set()) | ({14} if rows[o, 1] < 3 else set())
        assert set(np.flatnonzero(g.k3[0][o] >= 0).tolist()) == want


# ------------------------------------------------------------------------------------------------ restatement == oracle
@pytest.mark.parametrize("name", R.CASES)
def test_restatement_equals_oracle(name):
    c = R.case(name)
    rows, first, g = _restated(name)
    if c.n_items == 1:
        c_ref, i_ref = O.voxelize(c.points, c.vs, batch_index=c.batch_index)
        assert np.array_equal(rows, c_ref) and np.array_equal(first, i_ref)
    ref = O.Geometry(rows.astype(np.int32))
    _assert_geometry_equal(g, ref, rows)


# ------------------------------------------------------------------------------------------------ restatement == C twins
@pytest.mark.parametrize("name", R.CASES)
def test_restatement_equals_twins(name):
    c = R.case(name)
    rows, first, g = _restated(name)
    if c.n_items == 1:
        lv0, err = TW.voxelize(c.points, c.vs, batch_index=c.batch_index)
        assert err == 0 and np.array_equal(lv0.first_idx, first)
    else:                                                  # (the twin voxelises one item per call: its table from the rows)
        lv0 = TW.downsample(TW.Level(np.ascontiguousarray(rows, np.int32), np.empty(0, TW._SLOT)), 1)
    lv = [lv0]
    for i in range(3):
        lv.append(TW.downsample(lv[-1], 2 << i))
    for i in range(4):
        assert np.array_equal(lv[i].coords, g.levels[i]), f"level {i}"
    R.check_rulebook(_Map(*TW.rulebook_conv(lv[0], lv[0], 1, 5)), g.k_first, True)
    for i in range(4):
        R.check_rulebook(_Map(*TW.rulebook_conv(lv[i], lv[i], 1 << i, 3)), g.k3[i], True)
    for i in range(3):
        R.check_rulebook(_Map(*TW.rulebook_conv(lv[i], lv[i + 1], 1 << i, 3)), g.down[i], True)
        R.check_transposed(_Map(*TW.rulebook_transpose(lv[i + 1], lv[i], 1 << i)), g.up[i], g.up_rows[i])


# ------------------------------------------------------------------------------------------------ batches, the edge, errors
@pytest.mark.parametrize("name", R.BATCHED)
def test_batched_items_are_shifted_copies_and_never_neighbours(name):
    c = R.case(name)
    rows, first, g = _restated(name)
    rows1, first1, g1 = R.geometry("batch511")             # the same voxel set and points as one item
    sh = R.shifted_items(g1, c.n_items)
    for i in range(4):
        want = sh.levels[i].copy()
        assert np.array_equal(g.levels[i][:, 1:], want[:, 1:]) and np.array_equal(g.levels[i][:, 0], want[:, 0])
        assert R.item_starts(g.levels[i], c.n_items) == sh.starts[i]
    sh.levels = g.levels
    _assert_geometry_equal(g, sh, rows)
    assert np.array_equal(first, np.concatenate([first1 + b * c.n_points for b in range(c.n_items)]))
    for i in range(3):
        assert np.array_equal(g.up_rows[i], sh.up_rows[i])
    m = len(rows1)
    item_of = np.arange(len(rows)) // m
    hit = g.k_first >= 0
    assert (np.where(hit, g.k_first // m, item_of[:, None]) == item_of[:, None]).all()     # no entry points into another item


def test_just_outside_is_a_range_error_everywhere():
    for pts in R.just_outside():
        with pytest.raises(R.CoordinateRangeError):
            R.voxelize(pts, R.VS)
        with pytest.raises(AssertionError):
            O.voxelize(pts, R.VS)
        assert TW.voxelize(pts, R.VS)[1] == 1


def test_the_contract_at_the_edge_in_all_three_statements():
    """Voxels on opposite faces are not neighbours, in either direction, at stride 1 and across the stride-2 maps."""
    L = R.LIM
    rows = np.array([[0, L - 1, 5, 5], [0, -L, 5, 5], [0, 5, -L, 5], [0, 5, L - 1, 5], [0, 5, 5, L - 2], [0, 5, 5, -L + 1]], np.int64)
    g = R.Geometry(rows)
    assert (g.k3[0] >= 0).sum() == 6 and (g.k_first >= 0).sum() == 6           # only the centres
    assert all((g.k3[i] >= 0).sum() == len(g.levels[i]) for i in range(4))
    _assert_geometry_equal(g, O.Geometry(rows.astype(np.int32)), rows)
    lv = [TW.downsample(TW.Level(rows.astype(np.int32), np.empty(0, TW._SLOT)), 1)]
    for i in range(3):
        lv.append(TW.downsample(lv[-1], 2 << i))
    for i in range(4):
        R.check_rulebook(_Map(*TW.rulebook_conv(lv[i], lv[i], 1 << i, 3)), g.k3[i], True)
    for i in range(3):
        R.check_transposed(_Map(*TW.rulebook_transpose(lv[i + 1], lv[i], 1 << i)), g.up[i], g.up_rows[i])
    # beyond the range the restatement still answers (no packing): a probe from 2^17 - 1 by +8 is simply absent
    assert R.Index(rows).find(np.zeros(1, np.int64), np.array([[L + 7, 5, 5]]))[0] == -1
