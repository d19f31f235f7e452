"""Adversarial kernel maps, exact operands and the float64 restatement of the fused epilogue for the forward sparse
convolution (tests/test_spconv_exact_host.py on the CPU, tests/test_gpu_spconv_exact.py against imf_spconv_fwd).  No GPU
dependency.  Built on tests/backward_restate.py: the maps in both shapes, `conv_restate`, the integer data.

Maps.  `adversarial_maps()` lays out what the project's own map builders never produce: row counts on and around 16, 32,
48 and 64, 7 / 8 / 9 tiles with and without trailing padding tiles, more than 512 tiles, padding between rows and a whole
padding tile between live tiles, tiles with one and with all 27 active offsets, an offset present in a single row, tiles
whose offset lists do not intersect, many rows reading input row 0 or n_in - 1, live rows without any input, kvol 1 / 2 /
8 / 125.  Every map honours the precondition of include/imfnet_hip.h: a tile that holds a live row has at least one active
offset (unsplit launches skip a tile whose mask is 0 whole).

Operands.  The sums must be exact in float32 in ANY order, so that torch.equal against float64 is the comparison.  Let u_f
and u_w be the smallest bit present in the features and the weights.  Every operand PART (the f16 hi / lo halves, the three
bf16 parts, the fp32 value itself) is a multiple of its operand's unit, every product a multiple of u_f * u_w, and if

    (max pairs per output row) * cin * (max|feature| / u_f) * (max|weight| / u_w)  <  2^24

every partial sum is such a multiple below 2^24 units: exact, whatever the order, the split into partitions or the
arithmetic.  Integer data (`int_case`) lives in the FIRST part of a split operand; the `wide_*`, `three_level_*` and
`both_wide` generators put bits into the later parts and prove on the host, with torch's own f16 / bf16 conversions, that
they do."""
from typing import NamedTuple, Optional

import numpy as np
import torch

from backward_restate import EXACT_LIMIT, conv_restate, int_tensor, magnitude_bounds, rows_to_tiled, synthetic_map  # noqa: F401

TILE = 64
MASK_WORDS = 4
CENTRE = 13


class Map(NamedTuple):
    nbr_rows: Optional[np.ndarray]       # [n_out, kvol], -1 = none; None: kvol == 1, out row o reads in row o
    tile_rows: Optional[np.ndarray]      # [n_slots] output row of every slot, -1 = padding; None: slot == row
    nbr_tiled: Optional[np.ndarray]      # [kvol, n_slots]
    mask: Optional[np.ndarray]           # uint32 [n_slots / 64, 4]
    n_in: int
    n_out: int
    n_slots: int
    kvol: int


def roundup64(n):
    return (n + TILE - 1) // TILE * TILE


def tile_mask_of(nbr_tiled):
    """uint32 [n_tiles, 4]: bit k % 32 of word k / 32 set iff some slot of the tile has nbr[k][slot] >= 0
    (include/imfnet_hip.h, tile_mask)."""
    nbr_tiled = np.asarray(nbr_tiled)
    K, n_slots = nbr_tiled.shape
    assert n_slots % TILE == 0 and K <= 32 * MASK_WORDS
    active = (nbr_tiled.reshape(K, n_slots // TILE, TILE) >= 0).any(2)             # [K, n_tiles]
    mask = np.zeros((n_slots // TILE, MASK_WORDS), np.uint32)
    for k in range(K):
        mask[:, k // 32] |= active[k].astype(np.uint32) << np.uint32(k % 32)
    return mask


def live_tiles(tile_rows, n_slots, n_out):
    """bool [n_tiles]: the tile holds at least one output row."""
    tr = np.where(np.arange(n_slots) < n_out, 0, -1) if tile_rows is None else np.asarray(tile_rows)
    return (tr.reshape(-1, TILE) >= 0).any(1)


def _finish(nbr_rows, n_in, n_slots=None, tile_rows=None, rng=None):
    """Map of `nbr_rows` in the given slot order.  With `rng`: a tile that holds live rows but no input at all gets one
    (first live slot, a random offset and input row), so that the precondition holds; without: it must hold already."""
    nbr_rows = np.array(nbr_rows, np.int32)
    n_out, kvol = nbr_rows.shape
    n_slots = roundup64(n_out) if n_slots is None else n_slots
    tile_rows, tiled = rows_to_tiled(nbr_rows, n_slots, tile_rows)
    if rng is not None:
        bare = live_tiles(tile_rows, n_slots, n_out) & ~(tiled.reshape(kvol, -1, TILE) >= 0).any((0, 2))
        for t in np.nonzero(bare)[0]:
            slot = t * TILE + int(np.nonzero(tile_rows[t * TILE:(t + 1) * TILE] >= 0)[0][0])
            nbr_rows[tile_rows[slot], rng.integers(kvol)] = rng.integers(n_in)
        tile_rows, tiled = rows_to_tiled(nbr_rows, n_slots, tile_rows)
    m = Map(nbr_rows, tile_rows, tiled, tile_mask_of(tiled), n_in, n_out, n_slots, kvol)
    check_map(m)
    return m


def check_map(m):
    """Indices in [0, n_in) or -1, every row in exactly one slot, padding slots empty, and the mask-0 precondition."""
    if m.nbr_rows is None:
        assert m.kvol == 1 and m.tile_rows is None and m.nbr_tiled is None and m.mask is None and m.n_in == m.n_out
        assert m.n_slots % TILE == 0 and m.n_slots >= m.n_out
        return
    assert m.nbr_rows.shape == (m.n_out, m.kvol) and m.nbr_tiled.shape == (m.kvol, m.n_slots) and m.n_slots % TILE == 0
    assert m.nbr_rows.min() >= -1 and m.nbr_rows.max() < m.n_in
    live = m.tile_rows >= 0
    assert np.array_equal(np.sort(m.tile_rows[live]), np.arange(m.n_out))
    assert (m.nbr_tiled[:, ~live] == -1).all()
    assert m.mask.shape == (m.n_slots // TILE, MASK_WORDS) and m.mask.dtype == np.uint32
    has_offset = m.mask.any(1)
    assert (has_offset | ~live_tiles(m.tile_rows, m.n_slots, m.n_out)).all(), "a tile with a live row and mask 0"


def _identity_k1(n_out, n_slots=None):
    return Map(None, None, None, None, n_out, n_out, roundup64(n_out) if n_slots is None else n_slots, 1)


def _random(seed, n_out, kvol=27, density=0.3, n_in=None, n_slots=None, permute=False):
    gen = torch.Generator().manual_seed(seed)
    n_in = max(1, n_out // 2 + 7) if n_in is None else n_in
    rows, tr, _ = synthetic_map(gen, n_out, n_in, kvol, n_slots=n_slots, density=density, permute=permute)
    return _finish(rows, n_in, len(tr), tr, rng=np.random.default_rng(seed))


IDENTITY_ROWS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129)
LONELY_POSITIONS = (0, 15, 16, 31, 32, 47, 48, 63)
CHIP_ROWS = 513 * TILE + 5
_CACHE = {}


def adversarial_maps():
    """[(name, Map)], built once per process.  Names are the test ids."""
    if "maps" in _CACHE:
        return _CACHE["maps"]
    maps = []
    add = lambda name, m: maps.append((name, m))          # noqa: E731
    for i, n in enumerate(IDENTITY_ROWS):
        add(f"identity_n{n}", _random(100 + i, n))
    for i, n in enumerate((7 * TILE - 1, 8 * TILE, 8 * TILE + 1)):             # the XCD range cut: 7, 8, 9 tiles
        add(f"tiles{7 + i}_n{n}", _random(200 + i, n))
        add(f"tiles{7 + i}_n{n}_two_padding_tiles", _random(210 + i, n, n_slots=roundup64(n) + 2 * TILE))
    add("tiles8_n499_partial_last_tile", _random(220, 8 * TILE - 13))
    add(f"chip_filling_n{CHIP_ROWS}", _random(230, CHIP_ROWS, density=0.1))
    add("permuted_n300_of_384", _random(240, 300, n_slots=384, permute=True))
    add("permuted_n1000_of_1280_padding_tile", _permuted_with_padding_tile(241, 1000, 1280))
    # one offset per tile: tile t has only offset (5 t) % 27, in every live row
    rng = np.random.default_rng(250)
    n, n_in = 5 * TILE + 10, 171
    rows = np.full((n, 27), -1, np.int32)
    rows[np.arange(n), (5 * (np.arange(n) // TILE)) % 27] = rng.integers(0, n_in, n)
    add("one_offset_per_tile_n330", _finish(rows, n_in))
    assert all(bin(int(w)).count("1") == 1 for w in maps[-1][1].mask[:, 0])
    add("all_offsets_n130", _random(251, 130, density=1.0))
    assert (maps[-1][1].mask[:, 0] == (1 << 27) - 1).all()
    add("lonely_rows_n192", _lonely_rows(252))
    # disjoint neighbours: even tiles use offsets 0..12, odd tiles 14..26
    rng = np.random.default_rng(253)
    n, n_in = 4 * TILE + 20, 150
    rows = np.where(rng.random((n, 27)) < 0.4, rng.integers(0, n_in, (n, 27)), -1).astype(np.int32)
    odd = (np.arange(n) // TILE) % 2 == 1
    rows[np.ix_(~odd, np.arange(13, 27))] = -1
    rows[np.ix_(odd, np.arange(0, 14))] = -1
    add("disjoint_neighbours_n276", _finish(rows, n_in))
    m = maps[-1][1].mask[:, 0]
    assert all(int(m[t]) & int(m[t + 1]) == 0 and m[t] and m[t + 1] for t in range(len(m) - 1))
    # hot rows: half of all entries point at input row 0 or 39
    rng = np.random.default_rng(254)
    rows = np.where(rng.random((500, 27)) < 0.3, rng.integers(0, 40, (500, 27)), -1).astype(np.int32)
    hot = (rows >= 0) & (rng.random(rows.shape) < 0.5)
    rows[hot] = np.where(rng.random(int(hot.sum())) < 0.5, 0, 39)
    add("hot_rows_n500_of_40_inputs", _finish(rows, 40, rng=rng))
    add("no_input_rows_n700", _random(255, 700, density=0.02))
    assert ((maps[-1][1].nbr_rows >= 0).sum(1) == 0).sum() >= 200
    # at most two inputs per row (27 offsets): short offset walks, most partitions of a split launch empty
    rng = np.random.default_rng(256)
    n, n_in = 200, 90
    rows = np.full((n, 27), -1, np.int32)
    for _ in range(2):
        rows[np.arange(n), rng.integers(0, 27, n)] = rng.integers(0, n_in, n)
    add("two_inputs_per_row_n200", _finish(rows, n_in))
    for n in (1, 63, 64, 65, 1000):
        add(f"k1_identity_n{n}", _identity_k1(n))
    add("k1_map_n300_of_384_permuted", _random(260, 300, kvol=1, density=0.7, n_slots=384, permute=True))
    add("k2_map_n300_of_384_permuted", _random(261, 300, kvol=2, density=0.7, n_slots=384, permute=True))
    add("k8_map_n300_of_384_permuted", _random(262, 300, kvol=8, density=0.5, n_slots=384, permute=True))
    add("k125_map_n300_of_384_permuted", _random(263, 300, kvol=125, density=0.1, n_slots=384, permute=True))
    assert len({name for name, _ in maps}) == len(maps)
    _CACHE["maps"] = maps
    return maps


def map_named(name):
    return dict(adversarial_maps())[name]


def _permuted_with_padding_tile(seed, n_out, n_slots):
    """Permuted slots, padding between the rows, and the middle tile padding only (a random permutation would not hold a
    whole padding tile in any reasonable number of draws: the generator places it and then checks)."""
    rng = np.random.default_rng(seed)
    n_tiles, mid = n_slots // TILE, n_slots // TILE // 2
    rest = np.where(np.arange(n_slots - TILE) < n_out, np.arange(n_slots - TILE), -1)[rng.permutation(n_slots - TILE)]
    tile_rows = np.concatenate([rest[:mid * TILE], np.full(TILE, -1), rest[mid * TILE:]]).astype(np.int32)
    n_in = n_out // 2 + 7
    rows = np.where(rng.random((n_out, 27)) < 0.3, rng.integers(0, n_in, (n_out, 27)), -1).astype(np.int32)
    m = _finish(rows, n_in, n_slots, tile_rows, rng=rng)
    live = live_tiles(m.tile_rows, n_slots, n_out)
    assert not live[mid] and live[:mid].all() and live[mid + 1:].all() and 0 < mid < n_tiles - 1
    assert (m.tile_rows[:mid * TILE] < 0).any()                    # padding between rows as well
    return m


def _lonely_rows(seed):
    """192 rows, identity order.  Every row has the centre offset; offset k_p (all distinct, none the centre) is present
    only in the row at slot p of tile (index of p) % 3."""
    rng = np.random.default_rng(seed)
    n, n_in = 3 * TILE, 77
    rows = np.full((n, 27), -1, np.int32)
    rows[:, CENTRE] = rng.integers(0, n_in, n)
    ks = [k for k in rng.permutation(27) if k != CENTRE][:len(LONELY_POSITIONS)]
    for i, (p, k) in enumerate(zip(LONELY_POSITIONS, ks)):
        rows[(i % 3) * TILE + p, k] = rng.integers(0, n_in)
    m = _finish(rows, n_in)
    for k in ks:
        assert (m.nbr_rows[:, k] >= 0).sum() == 1
    return m


# ---- channels ------------------------------------------------------------------------------------------------------
CHANNELS = [(32, 0, 32), (64, 0, 64), (96, 0, 96), (32, 32, 64), (64, 32, 64), (32, 64, 128), (128, 128, 64), (256, 0, 256)]
LARGE_MAP_ROWS = 1300                        # the float64 restatement of a larger map runs on the first two sets only


def channels_for(m):
    return CHANNELS[:2] if m.n_out > LARGE_MAP_ROWS else CHANNELS


# ---- operands ------------------------------------------------------------------------------------------------------
def max_pairs(m):
    return 1 if m.nbr_rows is None else int((m.nbr_rows >= 0).sum(1).max())


def assert_exact(m, feat, w, unit_f, unit_w):
    """The condition of the module docstring, on the data itself."""
    f, wt = feat.double() / unit_f, w.double() / unit_w
    assert torch.equal(f, f.round()) and torch.equal(wt, wt.round()), "an operand is not a multiple of its unit"
    cin = feat.shape[1]
    assert w.shape[1] == cin
    bound = max_pairs(m) * cin * float(f.abs().max()) * float(wt.abs().max())
    assert bound < EXACT_LIMIT, f"partial sums up to {bound:.3g} units"
    return bound


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f16_parts(x):
    hi = x.to(torch.float16).float()
    return hi, (x - hi).to(torch.float16).float()


def _bf16_parts(x):
    p0 = x.to(torch.bfloat16).float()
    p1 = (x - p0).to(torch.bfloat16).float()
    return p0, p1, x - p0 - p1


def _assert_part(wide, shift, three=False):
    """The part the generator names is non-zero in at least a quarter of the elements, and the parts add up exactly."""
    hi, lo = _f16_parts(wide)
    p0, p1, p2 = _bf16_parts(wide)
    assert torch.equal(p0 + p1 + p2, wide) and torch.equal(p2.to(torch.bfloat16).float(), p2)
    if three:
        assert float((p2 != 0).float().mean()) >= 0.25
    elif shift == 11:
        assert torch.equal(hi + lo, wide)
        assert float((lo != 0).float().mean()) >= 0.25
    else:
        assert shift == 8 and float((p1 != 0).float().mean()) >= 0.25


def _wide(gen, shape, shift):
    x = int_tensor(gen, shape, 3) + int_tensor(gen, shape, 3) * 2.0 ** -shift
    _assert_part(x, shift)
    return x


def _three_level(gen, shape):
    x = int_tensor(gen, shape, 1) + int_tensor(gen, shape, 1) * 2.0 ** -9 + int_tensor(gen, shape, 1) * 2.0 ** -18
    _assert_part(x, 18, three=True)
    return x


def int_operands(m, cin, cout, seed=0):
    """(feat [n_in, cin] in [-3, 3], W [kvol, cin, cout] in [-2, 2]): backward_restate.int_case's forward operands."""
    gen = _gen(seed)
    feat, w = int_tensor(gen, (m.n_in, cin), 3), int_tensor(gen, (m.kvol, cin, cout), 2)
    assert_exact(m, feat, w, 1.0, 1.0)
    assert magnitude_bounds(m.nbr_rows, m.n_in, cin, cout)[0] < EXACT_LIMIT
    return feat, w


def wide_features(m, cin, cout, shift, seed=1):
    """Features a + b 2^-shift (a, b integers in [-3, 3]), integer weights in [-2, 2].  shift 11: the f16 lo half carries
    bits; shift 8: bf16x3's second part does."""
    gen = _gen(seed)
    feat, w = _wide(gen, (m.n_in, cin), shift), int_tensor(gen, (m.kvol, cin, cout), 2)
    assert_exact(m, feat, w, 2.0 ** -shift, 1.0)
    return feat, w


def wide_weights(m, cin, cout, shift, seed=2):
    """The mirror image: weights a + b 2^-shift, integer features in [-2, 2]."""
    gen = _gen(seed)
    feat, w = int_tensor(gen, (m.n_in, cin), 2), _wide(gen, (m.kvol, cin, cout), shift)
    assert_exact(m, feat, w, 1.0, 2.0 ** -shift)
    return feat, w


def three_level_features(m, cin, cout, seed=3):
    """Features a + b 2^-9 + c 2^-18 (a, b, c in {-1, 0, 1}), integer weights in [-1, 1]: bf16x3's third part carries bits
    wherever a, b and c are all non-zero (8 / 27 of the elements).  The levels are 9 bits apart, not 8: with 2^-8 and 2^-16
    round-to-nearest folds the value into two parts (1 + 2^-8 + 2^-16 = (1 + 2^-7) - (2^-8 - 2^-16), eight bits each) and the
    third is zero everywhere; the assertion of _three_level shows it.  The unit is 2^-18 then: 32 terms of magnitude
    (2^18 + 2^9 + 1) * 1 stay below 2^24, so these operands run on one input per row and 32 input channels."""
    gen = _gen(seed)
    feat, w = _three_level(gen, (m.n_in, cin)), int_tensor(gen, (m.kvol, cin, cout), 1)
    assert_exact(m, feat, w, 2.0 ** -18, 1.0)
    return feat, w


def three_level_weights(m, cin, cout, seed=4):
    gen = _gen(seed)
    feat, w = int_tensor(gen, (m.n_in, cin), 1), _three_level(gen, (m.kvol, cin, cout))
    assert_exact(m, feat, w, 1.0, 2.0 ** -18)
    return feat, w


def both_wide(m, cin, cout, seed=5):
    """Features and weights both a + b 2^-9 (a, b in {-1, 0, 1}): second part times second part.  kvol 1, cin 32.
    (2^-9, not 2^-8: 1 - 2^-8 is eight bits, one bf16 part, and only 2 / 9 of the elements would carry a second part; 1 - 2^-9
    and 1 + 2^-9 both need nine.)"""
    assert m.kvol == 1 and cin == 32
    gen = _gen(seed)

    def two(shape):
        x = int_tensor(gen, shape, 1) + int_tensor(gen, shape, 1) * 2.0 ** -9
        assert float((_bf16_parts(x)[1] != 0).float().mean()) >= 0.25
        return x
    feat, w = two((m.n_in, cin)), two((m.kvol, cin, cout))
    assert_exact(m, feat, w, 2.0 ** -9, 2.0 ** -9)
    return feat, w


# (name, generator, the variants it is for, (c_a, c_b, cout) sets, what a map must satisfy)
SPLIT_OPERANDS = [
    ("wide_features_2^-11", lambda m, ci, co: wide_features(m, ci, co, 11), (6, 3, 0), [(32, 0, 32), (32, 0, 64)],
     lambda m: m.kvol <= 27),
    ("wide_weights_2^-11", lambda m, ci, co: wide_weights(m, ci, co, 11), (6, 3, 0), [(32, 0, 32), (32, 0, 64)],
     lambda m: m.kvol <= 27),
    ("wide_features_2^-8", lambda m, ci, co: wide_features(m, ci, co, 8), (3, 0, 6), [(32, 0, 32), (64, 32, 64), (256, 0, 256)],
     lambda m: m.kvol <= 27),
    ("wide_weights_2^-8", lambda m, ci, co: wide_weights(m, ci, co, 8), (3, 0, 6), [(32, 0, 32), (64, 32, 64), (256, 0, 256)],
     lambda m: m.kvol <= 27),
    ("three_level_features", three_level_features, (3, 0), [(32, 0, 32), (32, 0, 64)], lambda m: max_pairs(m) <= 1),
    ("three_level_weights", three_level_weights, (3, 0), [(32, 0, 32), (32, 0, 64)], lambda m: max_pairs(m) <= 1),
    ("both_wide", both_wide, (3, 0), [(32, 0, 32), (32, 0, 64)], lambda m: m.kvol == 1),
]
SPLIT_OPERAND_MAPS = ("identity_n65", "permuted_n300_of_384", "all_offsets_n130", "lonely_rows_n192", "two_inputs_per_row_n200",
                      "one_offset_per_tile_n330", "k1_identity_n65", "k1_map_n300_of_384_permuted", "k2_map_n300_of_384_permuted")


# ---- the restatement ------------------------------------------------------------------------------------------------
def restate(m, feat, w):
    """float64 out [n_out, cout] = sum_k feat[nbr[o, k]] @ W[k]."""
    return conv_restate(feat, w, None, m.nbr_rows)


def epilogue_operands(cout, n_out, seed=9):
    """(scale [cout] powers of two from 1/4 to 4, shift [cout] and residual [n_out, cout] integers in [-3, 3]): with
    integer sums every step of the epilogue is exact in float32."""
    gen = _gen(seed)
    scale = 2.0 ** torch.randint(-2, 3, (cout,), generator=gen).to(torch.float32)
    return scale, int_tensor(gen, (cout,), 3), int_tensor(gen, (n_out, cout), 3)


def epilogue_restate(acc, scale=None, shift=None, residual=None, relu=False):
    """float64: relu(acc * scale + shift + residual), the expression of conv_epilogue (csrc/spconv_shared.h)."""
    v = acc.double()
    if scale is not None:
        v = v * scale.double()
    if shift is not None:
        v = v + shift.double()
    if residual is not None:
        v = v + residual.double()
    return torch.relu(v) if relu else v


def l2norm_restate(v):
    """float64 v / sqrt(sum v^2) per row, no epsilon (model/resunet.py:230): an all-zero row is NaN."""
    return v / v.pow(2).sum(1, keepdim=True).sqrt()


def assert_square_sum_exact(v, unit):
    """The l2norm bound's premise: the fp32 sum of squares of a row is exact (all terms are multiples of unit^2 and the
    total stays below 2^24 of them), so sqrtf and the division are the only roundings."""
    q = v.double() / unit
    assert torch.equal(q, q.round()) and float(q.pow(2).sum(1).max()) < EXACT_LIMIT
