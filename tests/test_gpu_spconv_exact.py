"""imf_spconv_fwd, exactly, on maps no builder of the project produces (tests/spconv_cases.py; proven on the CPU by
tests/test_spconv_exact_host.py).

Every kernel family (k_spconv_g, k_spconv_w in all its builds, k_spconv_mfma, k_spconv_mfma_simple, k_spconv_reduce behind
forced splits) under every arithmetic it has (fp32 MFMA, bf16x3, split-f16) runs every adversarial map on eight channel
sets.  The output has 64 guard rows and is NaN before the launch: rows < n_out must torch.equal the float64 restatement,
the guard rows must still be NaN.  A combination is left out only where imf_spconv_fwd refuses it by a written rule; the
test then checks that it does refuse.  On top: the fused epilogues (exact by construction), the split-f16 operand images
and their range flag, l2norm within a derived 2^-21, capacity mode with poisoned tables, operands whose later parts carry
bits, bit-reproducibility, the top 4 KiB of the LDS-DMA kernels' input window, and that the matrix holds every launch
shape the network's policy picks."""
import numpy as np
import pytest
import torch

import spconv_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD = 64

# arithmetic (imf_conv_args.variant) -> the `staging` names of ops.spconv it runs under
FAMILIES = {
    0: (None, "regs", "wave8", "wave4", "wave8u"),
    1: (None,),
    3: (None, "wave8", "wave4", "wave4h", "wave8u", "wave4u", "wave4o", "wave4h4", "wave8h4"),
    6: (None, "wave8", "wave4", "wave8u"),
}
# forced split_k per (variant, staging); every other family is unsplit by construction.  27 partitions of a tile with fewer
# active offsets leaves partitions empty (total < S)
SPLITS = {(0, None): (1, 2, 5, 8, 27), (0, "regs"): (1, 2, 5, 8, 27), (3, None): (1, 2, 5, 8), (6, None): (1, 2, 5)}
PAIRS = [(v, s) for v in (0, 1, 3, 6) for s in FAMILIES[v]]
PAIR_IDS = [f"v{v}-{s or 'default'}" for v, s in PAIRS]
MAP_IDS = [name for name, _ in S.adversarial_maps()]
CHIP = f"chip_filling_n{S.CHIP_ROWS}"


def rule_against(variant, staging, kvol, ca, cb, cout, l2norm=False):
    """The rule of imf_spconv_fwd (csrc/spconv.hip) that refuses the launch, quoted; None if the library accepts it."""
    cin = ca + cb
    regs, wave, v16 = staging == "regs", str(staging).startswith("wave"), variant in (3, 6)
    if l2norm and cout not in (32, 64):
        return "imf_spconv_fwd: l2norm needs cout in {32, 64}"
    if v16 and kvol >= 28:
        return "imf_spconv_fwd: variants 6 / 3 (split-f16 / bf16x3 weights) need kvol <= 27"
    if v16 and kvol * (cin // 32) >= 27 * 8 + 8:
        return "imf_spconv_fwd: variants 6 / 3 need kvol * cin / 32 < 224 and <= 1024 channels per source"
    if variant == 3 and regs:
        return "imf_spconv_fwd: variant 3 has no register-staged kernel"
    if variant == 6 and regs:
        return "imf_spconv_fwd: variant 6 has no register-staged kernel (IMF_TAG_REGS): it belongs to variant 0"
    j16 = 64 if cin % 64 == 0 else 32
    simple = not v16 and (variant == 1 or kvol >= 28 or (cb > 0 and ca % j16 != 0))
    dma0 = variant == 0 and not simple and not regs and kvol * (cin // 32) < 27 * 8 + 8
    if (v16 or dma0) and wave and not (cout % 64 == 0 and (kvol > 1 or cin >= 256)):
        return "imf_spconv_fwd: the wave-split kernel needs cout % 64 == 0 and kvol > 1 or cin >= 256"
    return None


# ---- device-side caches: a map, its operands and their restatement are built once per module -----------------------
_RB, _OPS, _PACKED = {}, {}, {}


def _dev(x, dtype=None):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x).to(DEV, dtype)


def rulebook(name):
    from imfnet_amd import ops
    if name not in _RB:
        m = S.map_named(name)
        if m.nbr_rows is None:
            _RB[name] = ops.Rulebook(None, None, None, m.n_slots, m.n_out, 1)
        else:
            _RB[name] = ops.Rulebook(_dev(m.tile_rows), _dev(m.nbr_tiled).view(-1), _dev(m.mask.view(np.int32)).view(-1),
                                     m.n_slots, m.n_out, m.kvol)
    return _RB[name]


class Operands:
    def __init__(self, m, ca, cb, feat, w):
        self.feat, self.w = feat, w
        self.fa, self.fb = feat[:, :ca].contiguous().to(DEV), (feat[:, ca:].contiguous().to(DEV) if cb else None)
        self.acc = S.restate(m, feat, w)                              # float64, on the host
        assert torch.equal(self.acc.float().double(), self.acc) and float(self.acc.abs().max()) > 0
        self.want = self.acc.float().to(DEV)


def operands(name, ch, kind="int", make=None):
    key = (name, ch, kind)
    if key not in _OPS:
        m = S.map_named(name)
        feat, w = (S.int_operands if make is None else make)(m, ch[0] + ch[1], ch[2])
        _OPS[key] = Operands(m, ch[0], ch[1], feat, w)
    return _OPS[key]


def packed(name, ch, kind, variant):
    from imfnet_amd import ops
    key = (name, ch, kind, variant)
    if key not in _PACKED:
        _PACKED[key] = ops.pack_weights(_OPS[(name, ch, kind)].w.to(DEV), variant=variant if variant in (3, 6) else None)
    return _PACKED[key]


def launch(name, ch, kind, variant, staging, split_k=0, rb=None, rows=None, **kw):
    """ops.spconv into a NaN-filled output with GUARD rows beyond the map's."""
    from imfnet_amd import ops
    o = _OPS[(name, ch, kind)]
    rb = rulebook(name) if rb is None else rb
    out = torch.full(((rb.n_out if rows is None else rows) + GUARD, ch[2]), NAN, device=DEV)
    ops.spconv(o.fa, packed(name, ch, kind, variant), ch[2], rb, in_b=o.fb, out=out, split_k=split_k, variant=variant,
               staging=staging, **kw)
    return out


def differs(out, want, n_out):
    """None, or what is wrong with a launch's output: live rows against `want` (bits), guard rows against NaN."""
    live, guard = out[:n_out], out[n_out:]
    msg = []
    if not torch.isnan(guard).all():
        msg.append(f"{int((~torch.isnan(guard)).any(1).sum())} guard rows written")
    if not torch.equal(live, want):
        unwritten = torch.isnan(live) & ~torch.isnan(want)
        bad = ((live != want) & ~(torch.isnan(live) & torch.isnan(want))).any(1)
        rows = torch.nonzero(bad).squeeze(1)
        msg.append(f"{int(bad.sum())} of {n_out} rows differ (first {rows[:6].tolist()}, last {rows[-2:].tolist()}), "
                   f"{int(unwritten.any(1).sum())} rows never written")
    return "; ".join(msg) or None


def refused(name, ch, variant, staging, **kw):
    from imfnet_amd import ImfError, ops
    m, rb = S.map_named(name), rulebook(name)
    cin = ch[0] + ch[1]
    fa = torch.zeros((m.n_in, ch[0]), device=DEV)
    fb = torch.zeros((m.n_in, ch[1]), device=DEV) if ch[1] else None
    L = ops._lib.lib()
    need = (L.imf_packed_weight_floats_split16 if variant == 6 else L.imf_packed_weight_floats_bf16x3 if variant == 3
            else L.imf_packed_weight_floats)(m.kvol, cin, ch[2])
    out = torch.full((m.n_out, ch[2]), NAN, device=DEV)
    with pytest.raises(ImfError):
        ops.spconv(fa, torch.zeros(need, device=DEV), ch[2], rb, in_b=fb, out=out, variant=variant, staging=staging, **kw)
    assert torch.isnan(out).all()                                     # refused before anything was launched


def run_matrix(name, variant, staging, kind="int", make=None, channel_sets=None):
    """Every channel set and forced split of one (map, arithmetic, family); the failures of all of them in one message."""
    m = S.map_named(name)
    ran, rules, bad = 0, [], []
    for ch in (S.channels_for(m) if channel_sets is None else channel_sets):
        rule = rule_against(variant, staging, m.kvol, *ch)
        if rule:
            rules.append(rule)
            refused(name, ch, variant, staging)
            continue
        o = operands(name, ch, kind, make)
        for split_k in SPLITS.get((variant, staging), (0,)):
            out = launch(name, ch, kind, variant, staging, split_k)
            why = differs(out, o.want, m.n_out)
            if why:
                bad.append(f"channels {ch} split_k {split_k}: {why}")
            ran += 1
    assert not bad, f"{len(bad)} of {ran} launches wrong: " + " | ".join(bad[:10])
    if not ran:
        pytest.skip("; ".join(sorted(set(rules))))
    return ran


# ======================================================================================================================
# 1. families x arithmetics x maps x channels, integer operands
# ======================================================================================================================
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", [n for n in MAP_IDS if n != CHIP])
def test_forward_is_exact_on_adversarial_maps(name, pair):
    variant, staging = pair
    run_matrix(name, variant, staging)


@pytest.mark.parametrize("pair", [(v, s) for v in (0, 3, 6) for s in (None, "wave4")], ids=lambda p: f"v{p[0]}-{p[1] or 'default'}")
def test_forward_is_exact_on_the_chip_filling_map(pair):
    """514 tiles: more than 512 workgroups, where k_spconv_g takes its other buffer ring.  32 -> 32 and 64 -> 64, integer data."""
    assert S.channels_for(S.map_named(CHIP)) == [(32, 0, 32), (64, 0, 64)]
    assert run_matrix(CHIP, pair[0], pair[1]) >= 1


def test_the_matrix_covers_what_the_network_launches():
    """Every tag imf_resunet_conv_kernel_tag answers is a staging of ops.spconv, and that staging is in FAMILIES for the
    arithmetic: levels 0-3, every (kvol, cin, cout) of the network's convolutions, one to three fragments per forward."""
    from imfnet_amd import _lib, ops
    from imfnet_amd import sparse as ME
    from imfnet_amd.model import load_model
    model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3, config=None)
    triples = set()
    for mod in model.modules():
        if isinstance(mod, ME._ConvBase):
            ks = mod.kernel_size if isinstance(mod.kernel_size, int) else mod.kernel_size[0]
            triples.add((ks ** 3, mod.in_channels, mod.out_channels))
    assert len(triples) >= 8 and (27, 64, 64) in triples and (27, 256, 256) in triples
    name_of = {tag: s for s, tag in ops.STAGING_TAGS.items() if s != "dma"}
    tag = _lib.lib().imf_resunet_conv_kernel_tag
    seen = set()
    for variant in (0, 3, 6):
        for level in range(4):
            for kvol, cin, cout in sorted(triples):
                for n_items in (1, 2, 3):
                    t = tag(level, kvol, cin, cout, variant, n_items)
                    assert t in name_of, (level, kvol, cin, cout, variant, n_items, t)
                    assert name_of[t] in FAMILIES[variant], (variant, name_of[t])
                    seen.add((variant, name_of[t]))
    assert {(3, "wave4u"), (3, "wave4h4"), (3, "wave8h4"), (3, "wave4o"), (3, "wave8u"), (0, "wave8u"), (6, "wave4")} <= seen


# ======================================================================================================================
# 2. the fused epilogue, exact by construction
# ======================================================================================================================
EPILOGUE_MAPS = ["permuted_n300_of_384", "permuted_n1000_of_1280_padding_tile", "lonely_rows_n192", "no_input_rows_n700"] + \
                [n for n in MAP_IDS if n.startswith("k1_")]
EPILOGUE_CHANNELS = [(32, 0, 32), (64, 32, 64), (96, 0, 96), (128, 128, 64), (256, 0, 256)]
# unsplit and split, where the family has both
EPILOGUE_SPLITS = {(0, None): (1, 3), (0, "regs"): (1, 3), (3, None): (1, 3), (6, None): (1, 3)}
_EPI = {}


def epilogue_case(name, ch, which):
    """(keyword arguments of ops.spconv on the device, float32 `want` on the device)."""
    key = (name, ch, which)
    if key not in _EPI:
        m, o = S.map_named(name), operands(name, ch)
        scale, shift, res = S.epilogue_operands(ch[2], m.n_out)
        kw = {"all": dict(scale=scale, shift=shift, residual=res, relu=False),
              "all_relu": dict(scale=scale, shift=shift, residual=res, relu=True),
              "shift_relu": dict(shift=shift, relu=True),
              "shift_residual_relu": dict(shift=shift, residual=res, relu=True),
              "residual": dict(residual=res)}[which]
        want = S.epilogue_restate(o.acc, **kw)
        assert torch.equal(want.float().double(), want)
        if m.nbr_rows is not None and which == "all_relu":               # a live row without input: relu(shift + residual)
            bare = torch.as_tensor((m.nbr_rows >= 0).sum(1) == 0)
            assert torch.equal(want[bare], torch.relu(shift.double() + res[bare].double()))
        _EPI[key] = ({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}, want.float().to(DEV))
    return _EPI[key]


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", EPILOGUE_MAPS)
def test_epilogues_are_exact(name, pair):
    variant, staging = pair
    m = S.map_named(name)
    ran, rules, bad = 0, [], []
    for ch in EPILOGUE_CHANNELS:
        rule = rule_against(variant, staging, m.kvol, *ch)
        if rule:
            rules.append(rule)
            continue
        for which in ("all", "all_relu", "shift_relu", "residual"):
            kw, want = epilogue_case(name, ch, which)
            for split_k in EPILOGUE_SPLITS.get(pair, (0,)):
                why = differs(launch(name, ch, "int", variant, staging, split_k, **kw), want, m.n_out)
                if why:
                    bad.append(f"channels {ch} {which} split_k {split_k}: {why}")
                ran += 1
    assert not bad, f"{len(bad)} of {ran} launches wrong: " + " | ".join(bad[:10])
    if not ran:
        pytest.skip("; ".join(sorted(set(rules))))


@pytest.mark.parametrize("staging", FAMILIES[6], ids=lambda s: s or "default")
@pytest.mark.parametrize("name", ["permuted_n300_of_384", "lonely_rows_n192", "no_input_rows_n700", "k1_identity_n65",
                                  "k1_map_n300_of_384_permuted"])
def test_split_f16_operand_images_are_exact_and_leave_the_range_flag_clear(name, staging):
    """Variant 6 with in_a / in_b, the residual and the output as operand images (hi + lo f16 halves).  Integer data below
    2^22 and below 65504: hi + lo is the value, the flag word stays 0.  Features a + b 2^-11 as images put bits into the
    lo halves the kernel reads without converting (fp32 output: their sums need 23 bits)."""
    from imfnet_amd import ops
    m, rb = S.map_named(name), rulebook(name)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    ran, bad = 0, []
    for ch in [(32, 0, 32), (64, 32, 64), (32, 32, 64), (128, 128, 64), (256, 0, 256)]:
        if rule_against(6, staging, m.kvol, *ch):
            continue
        for kind, make, fmt, which in (("int", None, ops.FMT_A_SPLIT | ops.FMT_RES_SPLIT | ops.FMT_OUT_SPLIT, "all_relu"),
                                       ("int", None, ops.FMT_RES_SPLIT | ops.FMT_OUT_SPLIT, "all"),
                                       ("wide_f11", lambda m_, ci, co: S.wide_features(m_, ci, co, 11), ops.FMT_A_SPLIT, None)):
            if kind == "wide_f11" and ch[0] + ch[1] != 32:
                continue
            o = operands(name, ch, kind, make)
            kw, want = epilogue_case(name, ch, which) if which else ({}, o.want)
            assert float(want.abs().max()) < 65504 and float(want.abs().max()) < 2 ** 22
            kw = dict(kw)
            if fmt & ops.FMT_RES_SPLIT:
                kw["residual"] = ops.to_operand_image(kw["residual"])
            fa = ops.to_operand_image(o.fa) if fmt & ops.FMT_A_SPLIT else o.fa
            fb = ops.to_operand_image(o.fb) if (fmt & ops.FMT_A_SPLIT and o.fb is not None) else o.fb
            if fmt & ops.FMT_A_SPLIT:
                assert torch.equal(ops.from_operand_image(fa), o.fa)
            out = torch.full((m.n_out + GUARD, ch[2]), NAN, device=DEV)
            ops.spconv(fa, packed(name, ch, kind, 6), ch[2], rb, in_b=fb, out=out, split_k=1, variant=6, staging=staging,
                       operand_format=fmt, flags=flags, **kw)
            if fmt & ops.FMT_OUT_SPLIT:
                out = torch.cat([ops.from_operand_image(out[:m.n_out]), out[m.n_out:]])
            why = differs(out, want, m.n_out)
            if why:
                bad.append(f"channels {ch} {kind} format {fmt}: {why}")
            ran += 1
    assert not bad, " | ".join(bad[:10])
    assert int(flags) == 0
    if not ran:
        pytest.skip("imf_spconv_fwd: the wave-split kernel needs cout % 64 == 0 and kvol > 1 or cin >= 256")


@pytest.mark.parametrize("staging", (None, "wave4"), ids=lambda s: s or "default")
def test_range_flag_is_raised_by_one_output_beyond_f16(staging):
    """256 * 512 = 2^17: both operands are f16 numbers, the single non-zero output is not: IMF_FLAG_RANGE (32)."""
    from imfnet_amd import ops
    n, kvol = (1, 1) if staging is None else (65, 27)
    feat, w = torch.zeros(n, 64), torch.zeros(kvol, 64, 64)
    feat[n - 1, 63], w[kvol - 1, 63, 0] = 256.0, 512.0
    if staging is None:
        rb = ops.Rulebook(None, None, None, 64, 1, 1)
        row = 0
    else:
        nbr = np.full((65, 27), -1, np.int32)
        nbr[:, 13], nbr[17, 26] = 0, 64                               # row 17 alone reads the hot input row at the hot offset
        tr, tiled = S.rows_to_tiled(nbr, 128)
        rb = ops.Rulebook(_dev(tr), _dev(tiled).view(-1), _dev(S.tile_mask_of(tiled).view(np.int32)).view(-1), 128, 65, 27)
        row = 17
    for variant, expect in ((6, 32), (3, 0), (0, 0)):                  # fp32 / bf16x3 operands: a large value is a value
        flags = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = ops.spconv(feat.to(DEV), ops.pack_weights(w.to(DEV), variant=variant if variant else None), 64, rb, split_k=1,
                         variant=variant, staging=staging, flags=flags)
        want = torch.zeros(rb.n_out, 64)
        want[row, 0] = 2.0 ** 17
        assert torch.equal(out.cpu(), want) and int(flags) == expect, (variant, int(flags))


L2_MAPS = ["permuted_n300_of_384", "lonely_rows_n192", "no_input_rows_n700", "k1_identity_n65", "k1_map_n300_of_384_permuted"]
L2_BOUND = 2.0 ** -21


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", L2_MAPS)
def test_l2norm_is_within_two_roundings_and_a_zero_row_is_nan(name, pair):
    """The pre-norm row is exact and so is its sum of squares (asserted on the reference), so out = v / sqrtf(ss) carries the
    rounding of sqrtf (<= 1 ulp), of the division (<= 1 ulp) and nothing else: under 2^-22 relative; the bound is twice that.
    Derived, not measured.  A live row of zeros is 0 / 0 = NaN in every family: no epsilon (model/resunet.py:230)."""
    variant, staging = pair
    m = S.map_named(name)
    ran, rules, bad = 0, [], []
    for ch in [(32, 0, 32), (64, 0, 64), (32, 32, 64), (128, 128, 64)]:
        rule = rule_against(variant, staging, m.kvol, *ch, l2norm=True)
        if rule:
            rules.append(rule)
            continue
        o = operands(name, ch)
        for which in (None, "shift_residual_relu"):                    # (no scale: the squares stay small integers)
            kw, pre = epilogue_case(name, ch, which) if which else ({}, o.want)
            pre = pre.cpu().double()
            S.assert_square_sum_exact(pre, 1.0)
            want = S.l2norm_restate(pre)
            zero = (pre == 0).all(1)
            assert torch.equal(torch.isnan(want).any(1), zero) and torch.equal(torch.isnan(want).all(1), zero)
            if name == "no_input_rows_n700" and which is None:
                assert int(zero.sum()) >= 200
            for split_k in EPILOGUE_SPLITS.get(pair, (0,)):
                out = launch(name, ch, "int", variant, staging, split_k, l2norm=True, **kw).cpu().double()
                got, guard = out[:m.n_out], out[m.n_out:]
                ok = torch.isnan(guard).all() and torch.equal(torch.isnan(got), torch.isnan(want))
                err = ((got - want).abs() / want.abs())[~torch.isnan(want) & (want != 0)]
                exact_zeros = torch.equal(got[want == 0], want[want == 0])
                worst = float(err.max()) if err.numel() else 0.0       # (a NaN where the reference has a number: NaN, fails)
                if not (ok and exact_zeros and worst <= L2_BOUND):
                    bad.append(f"channels {ch} {which} split_k {split_k}: NaN pattern / guards ok {bool(ok)}, zeros {exact_zeros}, "
                               f"max relative error {worst:.3g} (bound {L2_BOUND:.3g})")
                ran += 1
    assert not bad, " | ".join(bad[:10])
    if not ran:
        pytest.skip("; ".join(sorted(set(rules))))


# ======================================================================================================================
# 3. capacity mode on poisoned tables
# ======================================================================================================================
CAPACITY_MAPS = ["tiles8_n499_partial_last_tile", "tiles9_n513", "disjoint_neighbours_n276"]
CAPACITY_STAGINGS = (None, "wave4", "wave8", "wave8u", "wave4u", "wave4h4", "wave8h4")


def capacity_rulebook(m):
    """Tables for roundup64(n_out + 200) rows around the map's own: beyond the live tiles every slot is a row of its own
    (the rows n_out ...), reads input row 0 at every offset, and its tile's mask has all 27 bits: in range everywhere, so a
    tile that runs although the device-side count excludes it shows as a written guard row, never as a fault."""
    from imfnet_amd import ops
    cap, live = S.roundup64(m.n_out + 200), S.roundup64(m.n_out)
    assert m.n_slots == live and m.n_out % 48 and m.n_out % 32 and cap - live >= 128
    tile_rows = np.concatenate([m.tile_rows, m.n_out + np.arange(cap - live)]).astype(np.int32)
    nbr = np.concatenate([m.nbr_tiled, np.zeros((m.kvol, cap - live), np.int32)], 1)
    mask = np.concatenate([m.mask, np.tile(np.array([[0x7FFFFFF, 0, 0, 0]], np.uint32), ((cap - live) // 64, 1))])
    assert tile_rows.max() < cap and nbr.min() >= -1 and nbr.max() < m.n_in
    return ops.Rulebook(_dev(tile_rows), _dev(nbr).view(-1), _dev(mask.view(np.int32)).view(-1), cap, cap, m.kvol), cap


@pytest.mark.parametrize("staging", CAPACITY_STAGINGS, ids=lambda s: s or "default")
@pytest.mark.parametrize("variant", (0, 3))
@pytest.mark.parametrize("name", CAPACITY_MAPS)
def test_capacity_mode_is_the_exact_size_launch_and_writes_no_row_beyond_the_count(name, variant, staging):
    m = S.map_named(name)
    rb_cap, cap = capacity_rulebook(m)
    word = torch.tensor([m.n_out], dtype=torch.int32, device=DEV)
    ran, bad = 0, []
    for ch in S.CHANNELS:
        if rule_against(variant, staging, m.kvol, *ch):
            continue
        o = operands(name, ch)
        exact = launch(name, ch, "int", variant, staging, 1)
        out = launch(name, ch, "int", variant, staging, 1, rb=rb_cap, rows=cap - GUARD, n_out_dev=word)
        assert out.shape[0] == cap
        why = differs(exact, o.want, m.n_out) or differs(out, o.want, m.n_out)        # rows >= n_out_dev: the guard rows here
        if why or not torch.equal(out[:m.n_out], exact[:m.n_out]):
            bad.append(f"channels {ch}: {why}")
        ran += 1
    assert not bad, " | ".join(bad[:10])
    assert ran >= 4


# ======================================================================================================================
# 4. operands whose later parts carry bits
# ======================================================================================================================
# (generator, map) wherever the generator's exactness condition admits the map (spconv_cases.SPLIT_OPERANDS says which)
SPLIT_CASES = [(c, n) for c in S.SPLIT_OPERANDS for n in S.SPLIT_OPERAND_MAPS if c[4](S.map_named(n))]


@pytest.mark.parametrize("case,name", SPLIT_CASES, ids=[f"{c[0]}-{n}" for c, n in SPLIT_CASES])
def test_split_operands_are_multiplied_exactly(case, name):
    """Every family of the arithmetics the generator is for, forced splits included, torch.equal."""
    kind, make, variants, channel_sets, fits = case
    m = S.map_named(name)
    ran = 0
    for variant in variants:
        for staging in FAMILIES[variant]:
            sets = [ch for ch in channel_sets if not rule_against(variant, staging, m.kvol, *ch)]
            if sets:
                ran += run_matrix(name, variant, staging, kind, make, sets)
    assert ran >= len(variants)


def test_every_split_operand_generator_runs_on_several_maps():
    for c in S.SPLIT_OPERANDS:
        assert sum(1 for cc, _ in SPLIT_CASES if cc is c) >= 2, c[0]


# ======================================================================================================================
# 5. bit-reproducibility
# ======================================================================================================================
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_two_launches_return_the_same_bits(pair):
    variant, staging = pair
    name = "permuted_n1000_of_1280_padding_tile"
    m = S.map_named(name)

    def gaussian(m_, cin, cout):
        gen = torch.Generator().manual_seed(77)
        return torch.randn(m_.n_in, cin, generator=gen), torch.randn(m_.kvol, cin, cout, generator=gen) / (27 * cin) ** 0.5
    ran = 0
    for ch in [(32, 0, 32), (64, 32, 64), (256, 0, 256)]:
        if rule_against(variant, staging, m.kvol, *ch):
            continue
        key = (name, ch, "gauss")
        if key not in _OPS:
            o = _OPS[key] = Operands.__new__(Operands)
            o.feat, o.w = gaussian(m, ch[0] + ch[1], ch[2])
            o.fa, o.fb = o.feat[:, :ch[0]].contiguous().to(DEV), (o.feat[:, ch[0]:].contiguous().to(DEV) if ch[1] else None)
        for split_k in SPLITS.get(pair, (0,)):
            a = launch(name, ch, "gauss", variant, staging, split_k)
            b = launch(name, ch, "gauss", variant, staging, split_k)
            assert torch.equal(a[:m.n_out], b[:m.n_out]) and not torch.isnan(a[:m.n_out]).any() and torch.isnan(a[m.n_out:]).all()
            ran += 1
    assert ran


# ======================================================================================================================
# 6. the top 4 KiB of the LDS-DMA kernels' input window
# ======================================================================================================================
WINDOW = 0x7FFFF000                  # num_records of the row descriptors of k_spconv_g / k_spconv_w


def test_rows_in_the_top_4_kib_below_2_gib_are_read_or_refused():
    """An input of 2^31 - 128 bytes whose last 64 rows hold ones; a 64-row map that reads only those rows; integer weights.
    The LDS-DMA kernels' row descriptors end at 0x7FFFF000 (that is what makes the `no row` index read as zeros for every row
    stride), so the rows above it cannot reach them: ops.spconv sends variant 0 to the register-staged kernel and refuses
    variants 3 / 6 from that size on.  All indices are in range."""
    from imfnet_amd import ImfError, ops
    n_in, cin, cout = 16_777_215, 32, 32
    assert n_in * cin * 4 == 2 ** 31 - 128 > WINDOW
    in_a = torch.empty((n_in, cin), device=DEV)
    in_a[-64:] = 1.0
    gen = torch.Generator().manual_seed(5)
    nbr = np.where(np.random.default_rng(5).random((64, 27)) < 0.5, n_in - 1 - np.random.default_rng(6).integers(0, 64, (64, 27)), -1)
    nbr[:, 13] = n_in - 1 - np.arange(64)
    nbr = nbr.astype(np.int32)
    assert nbr[nbr >= 0].min() >= n_in - 64 and (nbr[nbr >= 0].astype(np.int64) * cin * 4 >= WINDOW - 64 * 128).all()
    assert ((nbr[nbr >= 0].astype(np.int64) + 1) * cin * 4 > WINDOW).sum() >= 27        # rows that end above the window
    tr, tiled = S.rows_to_tiled(nbr, 64)
    rb = ops.Rulebook(_dev(tr), _dev(tiled).view(-1), _dev(S.tile_mask_of(tiled).view(np.int32)).view(-1), 64, 64, 27)
    w = S.int_tensor(gen, (27, cin, cout), 2)
    want = torch.zeros(64, cout, dtype=torch.float64)
    for k in range(27):
        want[torch.as_tensor(nbr[:, k] >= 0)] += w[k].double().sum(0)                 # every input row read is all ones
    want = want.float().to(DEV)

    def run(variant, staging):
        out = torch.full((64 + GUARD, cout), NAN, device=DEV)
        ops.spconv(in_a, ops.pack_weights(w.to(DEV), variant=variant if variant else None), cout, rb, out=out, split_k=1,
                   variant=variant, staging=staging)
        return differs(out, want, 64)
    assert run(0, "regs") is None                                     # the yardstick: plain loads, no window
    assert run(0, None) is None                                       # routed to the register-staged kernel
    for variant in (3, 6):
        with pytest.raises(ImfError, match="buffer window"):
            run(variant, None)
    small = in_a.view(-1)[: WINDOW // 4].view(-1, cin)                # exactly the window: every kernel reads all of it
    assert small.numel() * 4 == WINDOW
    last = small.shape[0] - 1
    rb_s = ops.Rulebook(_dev(tr), _dev(np.where(tiled >= 0, last - (n_in - 1 - tiled), -1).astype(np.int32)).view(-1),
                        rb.tile_mask, 64, 64, 27)
    small[-64:] = 1.0
    for variant in (0, 3, 6):
        out = torch.full((64 + GUARD, cout), NAN, device=DEV)
        ops.spconv(small, ops.pack_weights(w.to(DEV), variant=variant if variant else None), cout, rb_s, out=out, split_k=1,
                   variant=variant)
        assert differs(out, want, 64) is None, variant


# ======================================================================================================================
# 7. the comparison itself: one wrong pair, one lost low bit
# ======================================================================================================================
@pytest.mark.parametrize("variant", (0, 3, 6))
def test_the_comparison_notices_one_misrouted_pair_and_one_lost_low_part(variant):
    """What a subtly wrong kernel would return, made by hand: a single neighbour entry that points at another (valid) input
    row, and a single feature whose smallest part is dropped.  Both must show as a difference from the restatement."""
    from imfnet_amd import ops
    name, ch = "permuted_n300_of_384", (32, 0, 64)
    m, rb = S.map_named(name), rulebook(name)
    o = operands(name, ch)
    assert differs(launch(name, ch, "int", variant, None, 1), o.want, m.n_out) is None
    k, slot = [int(x[0]) for x in np.nonzero(m.nbr_tiled >= 0)]
    other = (int(m.nbr_tiled[k, slot]) + 1) % m.n_in
    assert not torch.equal(o.feat[other], o.feat[m.nbr_tiled[k, slot]])
    nbr = rb.nbr.clone()
    nbr[k * m.n_slots + slot] = other
    wrong = ops.Rulebook(rb.tile_rows, nbr, rb.tile_mask, m.n_slots, m.n_out, m.kvol)
    why = differs(launch(name, ch, "int", variant, None, 1, rb=wrong), o.want, m.n_out)
    assert why is not None and why.startswith("1 of 300 rows differ"), why
    kind, make, bit = (("three", S.three_level_features, 2.0 ** -18) if variant != 6 else
                       ("wide11", lambda m_, ci, co: S.wide_features(m_, ci, co, 11), 2.0 ** -11))
    name = "one_offset_per_tile_n330"
    m = S.map_named(name)
    o = operands(name, ch, kind, make)
    assert differs(launch(name, ch, kind, variant, None, 1), o.want, m.n_out) is None
    used = int(m.nbr_rows[m.nbr_rows >= 0][0])                         # an input row some output reads
    low = o.feat[used] - o.feat[used].to(torch.bfloat16 if variant != 6 else torch.float16).float()
    c = int(torch.nonzero(low.abs() >= bit)[0])
    keep = o.fa
    try:
        o.fa = keep.clone()
        o.fa[used, c] -= bit * float(torch.sign(low[c]))               # one unit of the smallest part, gone
        assert differs(launch(name, ch, kind, variant, None, 1), o.want, m.n_out) is not None
    finally:
        o.fa = keep
