"""The cases of tests/spconv_cases.py, proven on the CPU before a GPU sees them: the maps are what they claim to be, the
operands meet their exactness conditions and exercise the parts they name, and the CPU twin of imf_spconv_fwd
(oracle/imf_cpu_twins.c, fp32 FMA chain) returns the float64 restatement bit for bit on every map."""
import numpy as np
import pytest
import torch

import backward_restate as R
import imf_cpu_twins as T
import spconv_cases as S
from test_cpu_twins import pack_weights_f32

MAPS = S.adversarial_maps()
IDS = [name for name, _ in MAPS]


@pytest.mark.parametrize("name", IDS)
def test_map_round_trips_and_its_mask_is_the_brute_force_one(name):
    m = S.map_named(name)
    S.check_map(m)
    if m.nbr_rows is None:
        return
    rows = R.tiled_to_rows(m.tile_rows, m.nbr_tiled, m.n_out)
    assert np.array_equal(rows, m.nbr_rows)
    tr, tiled = R.rows_to_tiled(rows, m.n_slots, m.tile_rows)
    assert np.array_equal(tr, m.tile_rows) and np.array_equal(tiled, m.nbr_tiled)
    want = np.zeros((m.n_slots // 64, 4), np.uint32)
    hit = m.nbr_tiled >= 0
    for k in range(m.kvol):
        for t in np.unique(np.nonzero(hit[k])[0] // 64):
            want[t, k // 32] |= np.uint32(1 << (k % 32))
    assert np.array_equal(S.tile_mask_of(m.nbr_tiled), want) and np.array_equal(m.mask, want)


def test_the_maps_hold_what_the_kernels_index_arithmetic_turns_on():
    names = set(IDS)
    for n in S.IDENTITY_ROWS:
        assert f"identity_n{n}" in names
    for t, n in ((7, 447), (8, 512), (9, 513)):
        a, b = S.map_named(f"tiles{t}_n{n}"), S.map_named(f"tiles{t}_n{n}_two_padding_tiles")
        assert a.n_slots == S.roundup64(n) == t * 64 and b.n_slots == a.n_slots + 128 and not b.mask[-2:].any()
    chip = S.map_named(f"chip_filling_n{S.CHIP_ROWS}")
    assert chip.n_slots // 64 == 514 > 512 and S.channels_for(chip) == S.CHANNELS[:2]
    lonely = S.map_named("lonely_rows_n192")
    alone = [k for k in range(27) if (lonely.nbr_rows[:, k] >= 0).sum() == 1]
    assert len(alone) == 8 and sorted(int(np.nonzero(lonely.nbr_rows[:, k] >= 0)[0][0]) % 64 for k in alone) == list(S.LONELY_POSITIONS)
    assert (lonely.nbr_rows[:, S.CENTRE] >= 0).all()
    hot = S.map_named("hot_rows_n500_of_40_inputs")
    e = hot.nbr_rows[hot.nbr_rows >= 0]
    assert hot.n_in == 40 and 0.45 < np.isin(e, (0, 39)).mean() < 0.6
    for name, m in MAPS:
        if m.nbr_rows is not None and m.kvol > 1 and not name.startswith("chip"):
            assert m.n_in != m.n_out, name
    assert max(S.max_pairs(S.map_named(n)) for n in ("two_inputs_per_row_n200", "k2_map_n300_of_384_permuted")) == 2


def test_tile_mask_of_fills_all_four_words():
    nbr = np.full((125, 128), -1, np.int32)
    for k, slot in ((0, 0), (31, 63), (32, 5), (63, 64), (64, 127), (95, 1), (96, 70), (124, 2)):
        nbr[k, slot] = 0
    want = np.array([[1 | 1 << 31, 1, 1 << 31, 1 << 28], [0, 1 << 31, 1, 1]], np.uint32)
    assert np.array_equal(S.tile_mask_of(nbr), want)


@pytest.mark.parametrize("name", IDS)
def test_integer_operands_are_exact_on_every_channel_set(name):
    m = S.map_named(name)
    for ca, cb, cout in S.channels_for(m):
        S.int_operands(m, ca + cb, cout)


@pytest.mark.parametrize("case", S.SPLIT_OPERANDS, ids=[c[0] for c in S.SPLIT_OPERANDS])
def test_split_operand_generators_exercise_their_part_and_stay_exact(case):
    """Beyond the generators' own assertions: a float32 sum in a random order returns the float64 restatement."""
    name, make, variants, channel_sets, fits = case
    ran = 0
    for map_name in S.SPLIT_OPERAND_MAPS:
        m = S.map_named(map_name)
        if not fits(m):
            continue
        for ca, cb, cout in channel_sets:
            feat, w = make(m, ca + cb, cout)
            want = S.restate(m, feat, w)
            assert torch.equal(want.float().double(), want)
            ran += 1
            if ran > 3 or m.nbr_rows is None:
                continue
            rng = np.random.default_rng(ran)
            for o in rng.integers(0, m.n_out, 4):
                ks = np.nonzero(m.nbr_rows[o] >= 0)[0]
                terms = torch.cat([feat[m.nbr_rows[o, k]].unsqueeze(1) * w[k] for k in ks]) if len(ks) else torch.zeros(1, cout)
                acc = torch.zeros(cout)
                for t in rng.permutation(len(terms)):
                    acc = acc + terms[t]                                        # float32, one rounding per addition
                assert torch.equal(acc.double(), want[o])
    assert ran >= 2


def _twin(m, fa, fb, w, cout, scale=None, shift=None, residual=None, relu=False, l2norm=False):
    from imfnet_amd._lib import ConvArgs
    c = lambda x, dt=np.float32: None if x is None else np.ascontiguousarray(np.asarray(x), dt)   # noqa: E731
    fa, fb, wp = c(fa), c(fb), pack_weights_f32(c(w))
    scale, shift, residual = c(scale), c(shift), c(residual)
    rows, nbr, mask = c(m.tile_rows, np.int32), c(m.nbr_tiled, np.int32), c(m.mask, np.uint32)
    out = np.full((m.n_out, cout), np.nan, np.float32)
    p = lambda x: None if x is None else x.ctypes.data                          # noqa: E731
    a = ConvArgs()
    a.in_a, a.c_a, a.in_b, a.c_b = p(fa), fa.shape[1], p(fb), 0 if fb is None else fb.shape[1]
    a.w_packed, a.kvol, a.cout = p(wp), m.kvol, cout
    a.tile_rows, a.nbr, a.tile_mask = p(rows), p(nbr), p(mask)
    a.n_slots, a.n_out = m.n_slots, m.n_out
    a.scale, a.shift, a.residual, a.relu, a.l2norm = p(scale), p(shift), p(residual), int(relu), int(l2norm)
    a.out, a.variant, a.split_k = p(out), 0, 1
    T.spconv_fwd(a)
    return torch.as_tensor(out)


@pytest.mark.parametrize("name", IDS)
def test_cpu_twin_equals_the_restatement(name):
    """Variant 0's twin on integer data, plain and under the epilogues of the GPU tests.  Every live row is written --
    rows without input as relu(shift + residual)."""
    m = S.map_named(name)
    for ca, cb, cout in S.channels_for(m):
        feat, w = S.int_operands(m, ca + cb, cout)
        fa, fb = feat[:, :ca].contiguous(), (feat[:, ca:].contiguous() if cb else None)
        acc = S.restate(m, feat, w)
        got = _twin(m, fa, fb, w, cout)
        assert torch.equal(got.double(), acc), (name, ca, cb, cout)
        if m.n_out > S.LARGE_MAP_ROWS:
            continue
        scale, shift, res = S.epilogue_operands(cout, m.n_out)
        for relu in (False, True):
            got = _twin(m, fa, fb, w, cout, scale, shift, res, relu)
            assert torch.equal(got.double(), S.epilogue_restate(acc, scale, shift, res, relu)), (name, ca, cb, cout, relu)
        if m.nbr_rows is not None:
            bare = torch.as_tensor((m.nbr_rows >= 0).sum(1) == 0)
            assert torch.equal(got[bare].double(), torch.relu(shift.double() + res[bare].double()))
