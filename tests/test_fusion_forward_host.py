"""Host side of the inference fusion block's tests (csrc/fusion.hip): the restatement factored at K / V
(fusion_restate.forward_from_kv) against the `forward` it came out of, the forward catalogue's torch fp32 error that the GPU
gate of tests/test_gpu_fusion_forward.py is measured against, and the argument checks of every fusion entry point, which
all answer before a launch.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import fusion_cases as FC
import fusion_restate as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ENTRIES = ("imf_fusion_attention", "imf_fusion_attention_batched", "imf_fusion_attention_batched_flags",
           "imf_fusion_attention_batched_v", "imf_fusion_attention_dyn", "imf_fusion_attention_dyn_v")


def _forward_before_the_split(x, starts, tokens, params):
    """fusion_restate.forward as it stood before forward_from_kv was factored out of it, statement for statement (z only):
    what `forward` is compared with bit for bit below.  A recorded hash cannot serve: the float64 products go through the
    BLAS, whose summation order changes with the thread count (measured: rows_17's z differs in its last bits between 1 and
    8 threads), so the bits are a property of the machine; the same BLAS in the same process gives the same bits twice."""
    _f64, _ln, _erf = FR._f64, FR._ln, FR._erf
    x, tokens = _f64(x), _f64(tokens)
    P = [_f64(p) for p in params]
    starts = [int(s) for s in starts]
    B, T, _ = tokens.shape
    c, ch, crstd = _ln(tokens, P[FR.LNC_G], P[FR.LNC_B])
    kv = c @ P[FR.WKV].T
    k, v = kv[..., :FR.INNER], kv[..., FR.INNER:]
    n1, xh1, rstd1 = _ln(x, P[FR.LN1_G], P[FR.LN1_B])
    q = n1 @ P[FR.WQ].T
    p = np.zeros((x.shape[0], T))
    o = np.zeros((x.shape[0], FR.INNER))
    for b in range(B):
        r = slice(starts[b], starts[b + 1])
        s = q[r] @ k[b].T * FR.SCALE
        e = np.exp(s - s.max(-1, keepdims=True)) if s.shape[0] else s
        p[r] = e / e.sum(-1, keepdims=True) if s.shape[0] else e
        o[r] = p[r] @ v[b]
    y = o @ P[FR.WO].T + P[FR.BO] + x
    n2, xh2, rstd2 = _ln(y, P[FR.LN2_G], P[FR.LN2_B])
    h = n2 @ P[FR.W1].T + P[FR.B1]
    a, g = h[:, :FR.HIDDEN], h[:, FR.HIDDEN:]
    cdf = 0.5 * (1.0 + _erf(g / math.sqrt(2.0)))
    u = a * (g * cdf)
    return u @ P[FR.W2].T + P[FR.B2] + y


@pytest.mark.parametrize("name", ["rows_17", "tokens_65", "rows_40_0_7"])
def test_forward_did_not_move_by_a_bit_when_forward_from_kv_was_factored_out(name):
    """The training tests' reference is `forward`: its z equals, bit for bit, the statements it consisted of before; its
    cache still holds every key `backward` reads; and z / dx stay within float64 round-off (1e-13 relative: sums of at
    most 1024 products, whatever the BLAS's order) of the arrays recorded from the parent commit in tests/golden."""
    c = FC.case(name)
    P = [w.numpy() for w in FC.weights(c["module"])]
    z, cache = FR.forward(c["x"].numpy(), c["starts"], c["tokens"].numpy(), P)
    before = _forward_before_the_split(c["x"].numpy(), c["starts"], c["tokens"].numpy(), P)
    assert z.dtype == np.float64 and np.array_equal(z, before)
    assert {"P", "starts", "c", "ch", "crstd", "k", "v", "n1", "xh1", "rstd1", "q", "p", "o", "xh2", "rstd2", "n2", "a", "g",
            "cdf", "u", "tokens_shape"} == set(cache)
    # forward_from_kv on the cache's own K / V: the same bits again
    z2, _ = FR.forward_from_kv(c["x"].numpy(), c["starts"], cache["k"], cache["v"], P)
    assert np.array_equal(z2, z)
    recorded = np.load(os.path.join(ROOT, "tests", "golden", "fusion_restate_parent.npz"))
    if name + ".z" in recorded:
        ref = FC.reference(name)
        for key in ("z", "dx"):
            want = recorded[f"{name}.{key}"]
            assert np.abs(ref[key] - want).max() <= 1e-13 * np.abs(want).max(), key


def test_forward_catalogue_holds_the_cases_and_leaves_the_training_catalogue_alone():
    S = FC.FORWARD_SHAPES
    assert list(FC.SHAPES) == ["rows_1", "rows_15", "rows_16", "rows_17", "rows_1_16_33", "rows_40_0_7",
                               "two_chunks_and_a_row", "tokens_65"]
    one = {rows[0] for rows, T, f in S.values() if len(rows) == 1 and T == 300 and f == 1.0}
    assert one >= {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 97}
    items = {rows for rows, T, f in S.values() if len(rows) > 1 and T == 300}
    assert items >= {(1, 16, 33), (31, 33), (48, 48, 1), (17, 5), (5, 17), (1,) * 8, (3, 64, 2, 47, 1, 16, 33, 15)}
    assert {T for rows, T, f in S.values() if rows == (17, 5)} >= {1, 63, 64, 65, 128, 129, 255, 256, 300, 320}
    assert {(T, f) for rows, T, f in S.values() if f != 1.0} == {(65, 64.0), (65, 256.0), (300, 64.0), (300, 256.0)}
    assert all(FC.tokens_padded(T) % 64 == 0 and T <= FC.tokens_padded(T) < T + 64 and FC.tokens_padded(T) <= 320 for _, T, _ in S.values())
    assert max(sum(rows) for rows, _, _ in S.values()) < 256 and all(min(rows) >= 1 for rows, _, _ in S.values())


@pytest.mark.parametrize("name", sorted(FC.FORWARD_SHAPES))
def test_torch_fp32_path_errs_below_1e_5_against_the_restatement_on_every_forward_case(name):
    """e_torch of every item (CPU fp32, from the same fp32 K / V) is above 0 and below 1e-5, so neither a broken reference
    nor a zero can move the GPU gate 8 * max(e_torch, 2^-24); torch in float64 agrees with the restatement to 1e-12."""
    c = FC.forward_case(name)
    ref = FC.forward_reference(name)
    assert ref.dtype == np.float64 and ref.shape == (sum(c["rows"]), 256) and np.isfinite(ref).all()
    assert c["k"].dtype == torch.float32 and c["k"].shape == c["v"].shape == (len(c["rows"]), c["T"], 128)
    e64 = FC.item_errors(FC.forward_torch_path(c, dtype=torch.float64), ref, c["starts"])
    assert max(e64) <= 1e-12, e64
    e = FC.item_errors(FC.forward_torch_path(c), ref, c["starts"])
    print(f"{name}: e_torch(cpu) per item = {['%.3e' % v for v in e]}")
    assert all(0.0 < v < 1e-5 for v in e), e


@pytest.mark.parametrize("name, low", [("softmax_t65_x64", 40.0), ("softmax_t300_x64", 40.0), ("softmax_t65_x256", 160.0),
                                       ("softmax_t300_x256", 160.0), ("rows_17", 0.0)])
def test_softmax_cases_leave_the_range_in_which_exp_without_the_max_survives(name, low):
    """expf overflows fp32 from 88.7 on.  The scaled cases put a score beyond `low` (and the x256 ones beyond 88.7) in
    every row's maximum's neighbourhood, with one token taking most of the weight; the default module stays inside +-3."""
    c = FC.forward_case(name)
    P = [w.numpy() for w in FC.weights(c["module"])]
    _, cache = FR.forward_from_kv(c["x"].numpy(), c["starts"], c["k"].numpy(), c["v"].numpy(), P)
    s = cache["q"] @ cache["k"][0].T * FR.SCALE
    top = np.abs(s).max(-1)
    print(f"{name}: max|score| per row {top.min():.1f} .. {top.max():.1f}, mean max probability {cache['p'].max(-1).mean():.3f}")
    if low:
        assert top.max() > low and cache["p"].max(-1).mean() > 0.5
    else:
        assert top.max() < 3.0 and cache["p"].max(-1).max() < 0.1


def test_header_declares_and_library_exports_every_fusion_entry_point():
    from imfnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "imfnet_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ENTRIES + ("imf_fusion_workspace_bytes", "imf_fusion_workspace_bytes_cap"):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/imfnet_hip.h"
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.imf_fusion_workspace_bytes(10) == L.imf_fusion_workspace_bytes_cap(10) == 10 * (2 * 256 + 1024) * 4


def test_argument_errors_of_every_fusion_entry_point_return_before_a_launch():
    """Host pointers and no GPU: each refusal is IMF_EINVAL with the entry's name in imf_last_error()."""
    from imfnet_amd import _lib
    L = _lib.lib()
    m = re.search(r"#define\s+IMF_EINVAL\s+(-?\d+)", open(os.path.join(ROOT, "include", "imfnet_hip.h")).read())
    assert m and int(m.group(1)) == EINVAL
    buf = np.zeros(1 << 14, dtype=np.float64)
    p = buf.ctypes.data
    p += (-p) % 16
    n = 8
    nbytes = L.imf_fusion_workspace_bytes(n)
    assert 0 < nbytes <= buf.nbytes - 32
    fields = [f for f, _ in _lib.FusionWeights._fields_]

    def weights(null=None):
        return _lib.FusionWeights(**{f: (None if f == null else p) for f in fields})

    def arr(kind, values):
        return (kind * len(values))(*values)

    def call(entry, null=None, n_items=1, rows=(n,), T=300, Tp=320, ws=p, wb=nbytes, w=None, item_null=None, n_cap=n):
        """One call of `entry` with good arguments except those named."""
        q = {k: (None if k == null else p) for k in ("x", "row0", "rows", "kt", "v", "w", "out", "n_dev", "starts", "err")}
        B = max(n_items, 1)
        kt = arr(C.c_void_p, [None if item_null == ("kt", b) else p for b in range(B)]) if q["kt"] else None
        vv = arr(C.c_void_p, [None if item_null == ("v", b) else p for b in range(B)]) if q["v"] else None
        wt = (w if w is not None else weights())
        wref = C.byref(wt) if q["w"] else None
        rows = tuple(rows) + (n,) * (B - len(rows))
        r0 = arr(C.c_int64, [0] * B) if q["row0"] else None
        rn = arr(C.c_int64, list(rows[:B])) if q["rows"] else None
        if entry == "imf_fusion_attention":
            return L.imf_fusion_attention(q["x"], rows[0], q["kt"], q["v"], T, Tp, wref, C.c_float(0.1), q["out"], ws, wb, None)
        if entry == "imf_fusion_attention_batched":
            return L.imf_fusion_attention_batched(q["x"], n_items, r0, rn, kt, vv, T, Tp, wref, C.c_float(0.1), q["out"], ws, wb,
                                                  None)
        if entry == "imf_fusion_attention_batched_flags":
            return L.imf_fusion_attention_batched_flags(q["x"], n_items, r0, rn, kt, vv, T, Tp, wref, C.c_float(0.1), q["out"],
                                                        ws, wb, None, None)
        if entry == "imf_fusion_attention_batched_v":
            return L.imf_fusion_attention_batched_v(q["x"], n_items, r0, rn, kt, vv, T, Tp, wref, C.c_float(0.1), q["out"], ws,
                                                    wb, None, 3, None)
        if entry == "imf_fusion_attention_dyn":
            return L.imf_fusion_attention_dyn(q["x"], n_cap, q["n_dev"], q["starts"], n_items, q["err"], kt, vv, T, Tp, wref,
                                              C.c_float(0.1), q["out"], ws, wb, None)
        assert entry == "imf_fusion_attention_dyn_v"
        return L.imf_fusion_attention_dyn_v(q["x"], n_cap, q["n_dev"], q["starts"], n_items, q["err"], kt, vv, T, Tp, wref,
                                            C.c_float(0.1), q["out"], ws, wb, 3, None)

    for entry in ENTRIES:
        single, dyn = entry == "imf_fusion_attention", "_dyn" in entry
        nulls = ("x", "kt", "v", "w", "out") + (("n_dev", "starts", "err") if dyn else () if single else ("row0", "rows"))
        for null in nulls:
            assert call(entry, null=null) == EINVAL, (entry, null)
            assert b"null" in L.imf_last_error() or (single and null in ("kt", "v")), (entry, null, L.imf_last_error())
        assert call(entry, ws=None) == EINVAL, entry
        for f in fields[:11]:                                           # (w1_f32 / w2_f32 may be NULL)
            assert call(entry, w=weights(null=f)) == EINVAL, (entry, f)
            assert b"null weight" in L.imf_last_error()
        for T, Tp in ((300, 300), (300, 330), (10, 32), (300, 384), (321, 384), (320, 256), (65, 64), (0, 64), (-1, 64),
                      (1, 0)):
            assert call(entry, T=T, Tp=Tp) == EINVAL, (entry, T, Tp)
            assert b"tokens" in L.imf_last_error()
        assert call(entry, wb=nbytes - 1) == EINVAL and b"workspace" in L.imf_last_error(), entry
        assert call(entry, wb=0) == EINVAL
        assert call(entry, ws=p + 4) == EINVAL and b"aligned" in L.imf_last_error(), entry
        if not single:
            for n_items in (0, 9, -1):
                assert call(entry, n_items=n_items) == EINVAL, (entry, n_items)
                assert b"n_items" in L.imf_last_error()
            for which in ("kt", "v"):
                assert call(entry, n_items=2, rows=(4, 4), item_null=(which, 1)) == EINVAL, (entry, which)
                assert b"item 1" in L.imf_last_error()
        if dyn:
            assert call(entry, n_cap=0) == EINVAL and call(entry, n_cap=-3) == EINVAL, entry
            assert call(entry, n_cap=n + 1) == EINVAL and b"workspace" in L.imf_last_error()   # sized by the capacity
        else:
            assert call(entry, rows=(0,)) == EINVAL and call(entry, rows=(-2,)) == EINVAL, entry     # an item without rows
            if not single:
                assert call(entry, n_items=3, rows=(3, 0, 5)) == EINVAL and b"item 1" in L.imf_last_error(), entry
        assert entry.encode() in L.imf_last_error() or b"imf_fusion_attention" in L.imf_last_error()
