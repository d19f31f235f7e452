"""The inference fusion block (csrc/fusion.hip: k_fusion_attn, the GEGLU GEMM on k_spconv_g, the K = 1024 GEMM on
k_spconv_w) at operator level, on the forward catalogue of tests/fusion_cases.py: row counts round the 16-row workgroup and
the 32 / 48 / 64-row units of the feed-forward, batched items, 1 .. 320 tokens, scores far outside the range in which a
softmax without the maximum survives -- against the float64 restatement (fusion_restate.forward_from_kv), and the exact
relations: reproducible bits, indifference to the padding of K^T / V, a row's independence of its position and of the other
items, the capacity entry equal to the exact one, nothing written outside the rows, the flag word.

The gate: e(A) = max|A - A64| / max|A64| per ITEM, e_torch = torch's fp32 ops on the same GPU from the same fp32 K / V.
Variants 3 (bf16x3: fp32-exact operands) and 0 (fp32 MFMA) are fp32 accumulations of the products torch sums and take the
gate of tests/test_gpu_fusion_train.py, e_hip <= 8 * max(e_torch, 2^-24).  Variant 6 multiplies operands cut to 22
significant bits (two f16 halves), an error torch's path does not have; its factor V6_FACTOR is twice the largest ratio
measured over the whole catalogue on an MI355X (profiles/fusion_forward_error.json), rounded up to a power of two."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

import fusion_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR, FLOOR = 8.0, 2.0 ** -24
V6_FACTOR = 4.0
SENTINEL = -7.25
BIG = 1.0e30
NAMES = sorted(FC.FORWARD_SHAPES)


@functools.lru_cache(maxsize=None)
def _weights(q_scale, variant):
    from imfnet_amd import ops
    module = copy.deepcopy(FC.forward_module(q_scale)).to(DEV)
    fw = ops.FusionKernelWeights(module, variant=variant)
    assert fw.supported
    return fw


def _padding(shape, fill):
    """`fill` with alternating signs (0: zeros)."""
    if fill == 0.0:
        return torch.zeros(shape)
    i, j = torch.meshgrid(torch.arange(shape[0]), torch.arange(shape[1]), indexing="ij")
    return (fill * (1.0 - 2.0 * ((i + j) % 2))).float()


def _packed(c, order=None, k_fill=0.0, v_fill=0.0):
    """([K^T images], [V images]) of the case's items (in `order`), padded to Tp columns / rows with `fill`."""
    from imfnet_amd import ops
    T, Tp = c["T"], c["Tp"]
    kts, vs = [], []
    for b in (range(len(c["rows"])) if order is None else order):
        kt, v = _padding((128, Tp), k_fill), _padding((Tp, 128), v_fill)
        kt[:, :T] = c["k"][b].t()
        v[:T] = c["v"][b]
        kts.append(ops.pack_weights(kt.to(DEV)))
        vs.append(ops.pack_weights(v.to(DEV)))
    return kts, vs


def _items(rows):
    starts = np.concatenate([[0], np.cumsum(rows)])
    return [(int(s), int(n)) for s, n in zip(starts[:-1], rows)]


def _exact(c, variant, x=None, packed=None, rows=None, out=None):
    """(out, flag word) of one imf_fusion_attention_batched_v call."""
    from imfnet_amd import ops
    kts, vs = _packed(c) if packed is None else packed
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    x = c["x"].to(DEV) if x is None else x
    z = ops.fusion_attention_batched(x, _items(c["rows"] if rows is None else rows), kts, vs, c["T"], c["Tp"],
                                     _weights(c["q_scale"], variant), out=out, flags=flags, variant=variant)
    return z, int(flags.item())


def _dyn(c, variant, n_cap, starts=None, n=None, packed=None):
    """(out [n_cap, 256] pre-filled with SENTINEL, flag word) of one imf_fusion_attention_dyn_v call with the count and the
    starts on the device; x's rows from the count on hold other finite data."""
    from imfnet_amd import ops
    kts, vs = _packed(c) if packed is None else packed
    n_rows = c["x"].shape[0]
    x = torch.randn(n_cap, 256, generator=torch.Generator().manual_seed(11)).to(DEV)
    x[:n_rows] = c["x"].to(DEV)
    out = torch.full((n_cap, 256), SENTINEL, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    n_dev = torch.tensor([n_rows if n is None else n], dtype=torch.int32, device=DEV)
    st = torch.tensor(list(c["starts"][:-1]) if starts is None else list(starts), dtype=torch.int32, device=DEV)
    ops.fusion_attention_dyn(x, n_dev, st, len(st), kts, vs, c["T"], c["Tp"], _weights(c["q_scale"], variant), out, flags,
                             variant)
    return out, int(flags.item())


# ======================================================================================================================
# a. against float64
# ======================================================================================================================
@pytest.mark.parametrize("variant", FC.FORWARD_VARIANTS)
@pytest.mark.parametrize("name", NAMES)
def test_every_item_within_the_gate_of_torchs_own_fp32_error(name, variant):
    c = FC.forward_case(name)
    ref = FC.forward_reference(name)
    z, flag = _exact(c, variant)
    assert flag == 0 and z.shape == ref.shape and bool(torch.isfinite(z).all())
    e_hip = FC.item_errors(z, ref, c["starts"])
    e_torch = FC.item_errors(FC.forward_torch_path(c, device=DEV), ref, c["starts"])
    factor = V6_FACTOR if variant == 6 else FACTOR
    ratios = [h / max(t, FLOOR) for h, t in zip(e_hip, e_torch)]
    for b, (h, t, r) in enumerate(zip(e_hip, e_torch, ratios)):
        print(f"{name} variant {variant} item {b} ({c['rows'][b]} rows): e_hip {h:.3e}  e_torch {t:.3e}  "
              f"e_hip / max(e_torch, 2^-24) = {r:.3f}")
    path = os.environ.get("IMF_FUSION_FORWARD_ERROR_JSON")             # the measurement kept under profiles/
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": name, "variant": variant, "rows": list(c["rows"]), "tokens": c["T"],
                                "q_scale": c["q_scale"], "e_hip": e_hip, "e_torch": e_torch, "ratio": ratios}) + "\n")
    late = [(b, h, factor * max(t, FLOOR)) for b, (h, t) in enumerate(zip(e_hip, e_torch)) if not h <= factor * max(t, FLOOR)]
    assert not late, late


# ======================================================================================================================
# b. exact relations
# ======================================================================================================================
@pytest.mark.parametrize("variant", FC.FORWARD_VARIANTS)
@pytest.mark.parametrize("name", ["rows_17", "items_3_64_2_47_1_16_33_15", "tokens_65", "softmax_t300_x256"])
def test_two_calls_give_the_same_bits(name, variant):
    c = FC.forward_case(name)
    a, fa = _exact(c, variant)
    b, fb = _exact(c, variant)
    assert fa == 0 and fb == 0 and torch.equal(a, b)


@pytest.mark.parametrize("variant", FC.FORWARD_VARIANTS)
@pytest.mark.parametrize("name", ["tokens_1", "tokens_63", "tokens_65", "tokens_129", "tokens_255", "tokens_300", "rows_33"])
def test_finite_padding_of_kt_columns_and_v_rows_changes_no_bit(name, variant):
    """Columns [T, Tp) of K^T and rows [T, Tp) of V at +-1e30 instead of zero: a padded score never enters the softmax
    (select on c < n_tokens) and its probability is exactly 0, so 0 * 1e30 adds +-0 to the P V sums."""
    c = FC.forward_case(name)
    assert c["Tp"] > c["T"]
    zero, f0 = _exact(c, variant)
    for k_fill, v_fill in ((BIG, 0.0), (0.0, BIG), (BIG, BIG)):
        got, f = _exact(c, variant, packed=_packed(c, k_fill=k_fill, v_fill=v_fill))
        assert f == 0 and f0 == 0 and torch.equal(got, zero), (k_fill, v_fill)


@pytest.mark.parametrize("variant", FC.FORWARD_VARIANTS)
def test_a_rows_output_does_not_depend_on_its_position(variant):
    """(17, 5) against (5, 17) with the items (rows and images) swapped: the same two items, the same feed-forward kernel
    shape, every row 5 places up or 17 places down -- in another 16-row workgroup slot, another tile row."""
    c = FC.forward_case("items_17_5")
    a, fa = _exact(c, variant)
    x = c["x"].to(DEV)
    b, fb = _exact(c, variant, x=torch.cat([x[17:], x[:17]]).contiguous(), packed=_packed(c, order=(1, 0)), rows=(5, 17))
    assert fa == 0 and fb == 0
    assert torch.equal(b[:5], a[17:]) and torch.equal(b[5:], a[:17])
    # and the catalogue's own (5, 17) is the same kernel path on its own data: its reference is checked in (a)


@pytest.mark.parametrize("variant", FC.FORWARD_VARIANTS)
@pytest.mark.parametrize("name, keep", [("items_1_16_33", 1), ("items_1_16_33", 0), ("items_48_48_1", 2), ("items_31_33", 0)])
def test_a_rows_output_does_not_depend_on_the_other_items_rows(name, keep, variant):
    c = FC.forward_case(name)
    a, fa = _exact(c, variant)
    s = c["starts"]
    x = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(12)) * 3.0
    x[s[keep]:s[keep + 1]] = c["x"][s[keep]:s[keep + 1]]
    b, fb = _exact(c, variant, x=x.to(DEV))
    assert fa == 0 and fb == 0
    assert torch.equal(a[s[keep]:s[keep + 1]], b[s[keep]:s[keep + 1]])
    assert not torch.equal(a, b)


@pytest.mark.parametrize("variant", FC.FORWARD_VARIANTS)
@pytest.mark.parametrize("name", ["rows_17", "items_1_16_33"])
def test_capacity_call_gives_the_exact_calls_bits_and_leaves_the_surplus_rows_alone(name, variant):
    """imf_fusion_attention_dyn_v with the capacity one row above the count, and beyond the next multiple of 48 and of 64
    (192 = their least common multiple)."""
    c = FC.forward_case(name)
    n = c["x"].shape[0]
    want, f0 = _exact(c, variant)
    assert f0 == 0
    for n_cap in (n + 1, (n + 191) // 192 * 192 + 1):
        got, f = _dyn(c, variant, n_cap)
        assert f == 0, (n_cap, f)
        assert torch.equal(got[:n], want), n_cap
        assert bool((got[n:] == SENTINEL).all()), n_cap


@pytest.mark.parametrize("variant", FC.FORWARD_VARIANTS)
@pytest.mark.parametrize("name", ["rows_1", "rows_33", "items_17_5"])
def test_exact_call_writes_nothing_outside_its_rows(name, variant):
    c = FC.forward_case(name)
    n, guard = c["x"].shape[0], 64
    buf = torch.full((n + 2 * guard, 256), SENTINEL, device=DEV)
    want, _ = _exact(c, variant)
    got, f = _exact(c, variant, out=buf[guard:guard + n])
    assert f == 0 and got.data_ptr() == buf[guard:].data_ptr()
    assert torch.equal(buf[guard:guard + n], want)
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all())


# ======================================================================================================================
# c. flags
# ======================================================================================================================
@pytest.mark.parametrize("starts, flagged", [((0, 1, 17), False), ((-1, 0, 17), True), ((0, -1, 17), True), ((0, 17, -1), True),
                                             ((0, 40, 40), True), ((0, 0, 17), True), ((0, 17, 50), True)],
                         ids=["good", "absent_first", "absent_middle", "absent_last", "empty_middle", "empty_first",
                              "empty_last"])
def test_capacity_call_flags_an_item_without_rows(starts, flagged):
    """include/imfnet_hip.h: "an item without rows raises bit 3 (value 8)" -- the producer's -1 for an absent item, and an
    item whose range is empty (s1 == s0; the last one: its start at the count).  50 rows, capacity 64; every start lies
    inside [0, count], so the items that do have rows stay inside the buffers."""
    c = FC.forward_case("items_1_16_33")
    out, f = _dyn(c, 3, 64, starts=starts)
    assert bool(f & 8) == flagged, f
    if not flagged:
        assert f == 0
    assert bool((out[50:] == SENTINEL).all())
