"""The attention-fusion training kernels (csrc/fusion_train.hip) on the GPU: forward, backward and the 14 parameter
gradients against the float64 restatement tests/fusion_restate.py, gated by the error of torch's own fp32 path on the same
GPU and inputs; the exact properties (reproducible bits, every output written, +0.0 for an item without rows, batched rows
equal to the items run alone, null outputs, bad starts); and the wiring into ResUNet2.transformer.

The gate: e(A) = max|A - A64| / max|A64| per output tensor, and e_hip(A) <= 8 * max(e_torch(A), 2^-24).  Both paths are
fp32 accumulations of the same products and differ only in summation order: a sequential chain of K terms errs like
sqrt(K), a library's blocked order with block b like sqrt(K / b); with K <= 2048 and blocks up to 64 the factor is at most
sqrt(64) = 8.  tests/test_fusion_train_host.py checks that e_torch > 0 on these inputs."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import fusion_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR, FLOOR = 8.0, 2.0 ** -24
GUARD = 64                                 # floats on each side of a guarded buffer (keeps 16-byte alignment)


def _inputs(name):
    from imfnet_amd import ops
    c = FC.case(name)
    x, tokens, dz = c["x"].to(DEV), c["tokens"].to(DEV), c["dz"].to(DEV)
    starts = torch.as_tensor(c["starts"]).to(DEV)
    w = FC.weights(c["module"], device=DEV)
    assert len(w) == len(ops.FUSION_TRAIN_PARAMS)
    return c, x, starts, tokens, dz, w


def _run(x, starts, tokens, dz, w, want_dx=True, want_dtokens=True, want=None):
    """{tensor name: result} of one forward and one backward call, and the two meta words."""
    from imfnet_amd import ops
    z, saved, meta_f = ops.fusion_train_forward(x, starts, tokens, w)
    dx, dtok, grads, meta_b = ops.fusion_train_backward(dz, x, starts, tokens, w, saved, want_dx, want_dtokens, want)
    out = {"z": z, "dx": dx, "dtokens": dtok}
    out.update(dict(zip(FC.PARAMS, grads)))
    return out, int(meta_f.item()), int(meta_b.item())


@pytest.mark.parametrize("name", sorted(FC.SHAPES))
def test_every_output_within_eight_times_torchs_own_fp32_error(name):
    c, x, starts, tokens, dz, w = _inputs(name)
    ref = FC.reference(name)
    hip, mf, mb = _run(x, starts, tokens, dz, w)
    assert mf == 0 and mb == 0
    tor = FC.torch_path(c, dtype=torch.float32, device=DEV)
    rows, late = {}, []
    for key in FC.TENSORS:
        e_hip, e_torch = FC.rel_err(hip[key], ref[key]), FC.rel_err(tor[key], ref[key])
        bound = FACTOR * max(e_torch, FLOOR)
        rows[key] = dict(e_hip=e_hip, e_torch=e_torch, ratio=e_hip / max(e_torch, FLOOR))
        print(f"{name} {key}: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}  e_hip / max(e_torch, 2^-24) = {rows[key]['ratio']:.3f}")
        if not e_hip <= bound:
            late.append((key, e_hip, bound))
    path = os.environ.get("IMF_FUSION_ERROR_JSON")                     # the measurement kept under profiles/
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": name, "rows": list(c["rows"]), "tokens": c["T"], "tensors": rows}) + "\n")
    assert not late, late


@pytest.mark.parametrize("name", ["rows_40_0_7", "two_chunks_and_a_row", "tokens_65"])
def test_two_calls_give_the_same_bits_and_nan_prefilled_outputs_come_back_written(name):
    from imfnet_amd import ops
    c, x, starts, tokens, dz, w = _inputs(name)
    a, _, _ = _run(x, starts, tokens, dz, w)
    nan = float("nan")
    z = torch.full_like(x, nan)
    outputs = (torch.full_like(x, nan), torch.full_like(tokens, nan), [torch.full_like(t, nan) for t in w])
    z2, saved, _ = ops.fusion_train_forward(x, starts, tokens, w, z=z)
    dx, dtok, grads, _ = ops.fusion_train_backward(dz, x, starts, tokens, w, saved, outputs=outputs)
    assert z2 is z and dx is outputs[0] and dtok is outputs[1]
    b = {"z": z, "dx": dx, "dtokens": dtok}
    b.update(dict(zip(FC.PARAMS, grads)))
    for key in FC.TENSORS:
        assert not torch.isnan(b[key]).any(), key
        assert torch.equal(a[key], b[key]), key
    if name == "rows_40_0_7":                                          # the item without rows: exactly +0.0
        bits = dtok[1].contiguous().view(torch.int32)
        assert int(bits.abs().max()) == 0
        assert float(dtok[0].abs().max()) > 0 and float(dtok[2].abs().max()) > 0


@pytest.mark.parametrize("name", ["rows_1_16_33", "rows_40_0_7"])
def test_forward_rows_of_a_batched_call_equal_each_item_run_alone(name):
    from imfnet_amd import ops
    c, x, starts, tokens, dz, w = _inputs(name)
    z, _, _ = ops.fusion_train_forward(x, starts, tokens, w)
    s = c["starts"]
    for b, n in enumerate(c["rows"]):
        one = torch.tensor([0, n], dtype=torch.int32, device=DEV)
        zb, _, meta = ops.fusion_train_forward(x[s[b]:s[b + 1]].contiguous(), one, tokens[b:b + 1].contiguous(), w)
        assert int(meta.item()) == 0 and zb.shape[0] == n
        assert torch.equal(zb, z[s[b]:s[b + 1]]), b


def test_null_gradient_pointers_leave_the_other_outputs_bits_unchanged():
    c, x, starts, tokens, dz, w = _inputs("rows_1_16_33")
    full, _, _ = _run(x, starts, tokens, dz, w)
    rng = np.random.default_rng(3)
    masks = [(False, True, [True] * 14), (True, False, [True] * 14), (False, False, [False] * 12 + [True, True]),
             (True, False, [False] * 14), (False, True, [False] * 14),
             (False, False, [k in (2, 3, 5) for k in range(14)]),       # the context side alone
             (False, False, [k in (8, 11) for k in range(14)])]
    masks += [(bool(rng.integers(2)), bool(rng.integers(2)), [bool(v) for v in rng.integers(0, 2, 14)]) for _ in range(5)]
    for want_dx, want_dtok, want in masks:
        part, _, _ = _run(x, starts, tokens, dz, w, want_dx, want_dtok, want)
        flags = dict(zip(FC.TENSORS, [True, want_dx, want_dtok] + list(want)))
        for key in FC.TENSORS:
            if flags[key]:
                assert torch.equal(part[key], full[key]), (key, want_dx, want_dtok, want)
            else:
                assert part[key] is None, key


def _guarded(shape, fill):
    """(whole buffer, interior view of `shape`): GUARD floats of the pattern on both sides."""
    n = int(np.prod(shape))
    n4 = (n + 3) // 4 * 4
    buf = torch.full((n4 + 2 * GUARD,), fill, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


@pytest.mark.parametrize("bad", [(0, 30, 20, 57), (0, 20, 40, 60), (0, 20, 70, 57), (-3, 20, 40, 57), (5, 20, 40, 57),
                                 (0, 20, 40, 50), (0, 2 ** 31 - 1, -2 ** 31, 57)],
                         ids=["not_monotonic", "beyond_n", "middle_beyond_n", "negative", "not_from_zero", "short",
                              "extremes"])
def test_bad_starts_raise_the_flag_and_leave_the_guard_bands_untouched(bad):
    """Every buffer either call may write -- z, saved, dx, dtokens, the 14 gradients, the workspace -- sits between guard
    bands; starts that are no partition of the 57 rows raise the flag and nothing outside the buffers changes.  The good
    partition on the same buffers raises nothing."""
    import ctypes as C
    from imfnet_amd import _lib, ops
    L = _lib.lib()
    c, x, _, tokens, dz, w = _inputs("rows_1_16_33")
    x, dz = torch.cat([x, x[:7]]).contiguous(), torch.cat([dz, dz[:7]]).contiguous()          # 57 rows
    n, B, T = x.shape[0], tokens.shape[0], tokens.shape[1]
    sbytes, wbytes = L.imf_fusion_train_saved_bytes(n, B, T), L.imf_fusion_train_workspace_bytes(n, B, T)
    PATTERN = -7.25
    bufs = {"z": _guarded(x.shape, PATTERN), "saved": _guarded((sbytes // 4,), PATTERN), "ws": _guarded((wbytes // 4,), PATTERN),
            "dx": _guarded(x.shape, PATTERN), "dtok": _guarded(tokens.shape, PATTERN)}
    for k, t in enumerate(w):
        bufs[f"g{k}"] = _guarded(t.shape, PATTERN)
    wptr = (C.c_void_p * 14)(*[t.data_ptr() for t in w])
    gptr = (C.c_void_p * 14)(*[bufs[f"g{k}"][1].data_ptr() for k in range(14)])
    meta = torch.zeros(2, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for starts_host, flag in ((bad, ops.FUSION_TRAIN_FLAG_STARTS), ((0, 1, 17, 57), 0)):
        starts = torch.tensor(starts_host, dtype=torch.int32, device=DEV)
        rc = L.imf_fusion_train_forward(x.data_ptr(), n, starts.data_ptr(), B, tokens.data_ptr(), T, *ops.FUSION_TRAIN_DIMS,
                                        wptr, bufs["z"][1].data_ptr(), bufs["saved"][1].data_ptr(), sbytes,
                                        meta[0:].data_ptr(), stream)
        assert rc == 0, L.imf_last_error()
        rc = L.imf_fusion_train_backward(dz.data_ptr(), x.data_ptr(), n, starts.data_ptr(), B, tokens.data_ptr(), T,
                                         *ops.FUSION_TRAIN_DIMS, wptr, bufs["saved"][1].data_ptr(), sbytes,
                                         bufs["dx"][1].data_ptr(), bufs["dtok"][1].data_ptr(), gptr, meta[1:].data_ptr(),
                                         bufs["ws"][1].data_ptr(), wbytes, stream)
        assert rc == 0, L.imf_last_error()
        torch.cuda.synchronize()
        assert meta.tolist() == [flag, flag], (starts_host, meta.tolist())
        for key, (buf, view) in bufs.items():
            n_in = view.numel()
            assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n_in:] == PATTERN).all()), key
    # the good partition came last: every output is written (no pattern left would be too strict for values; no NaN)
    for key in ("z", "dx", "dtok") + tuple(f"g{k}" for k in range(14)):
        assert bool(torch.isfinite(bufs[key][1]).all()), key


def test_no_rows_launch_nothing_and_autograd_returns_zero_gradients():
    from imfnet_amd import ops
    from imfnet_amd.autograd import AttentionFusionFunction
    c, _, _, tokens, _, w = _inputs("rows_17")
    x = torch.zeros(0, 256, device=DEV, requires_grad=True)
    starts = torch.zeros(2, dtype=torch.int32, device=DEV)
    params = [t.clone().requires_grad_(True) for t in w]
    tok = tokens.clone().requires_grad_(True)
    z = AttentionFusionFunction.apply(x, starts, tok, *params)
    assert z.shape == (0, 256)
    z.sum().backward()
    assert tok.grad is not None and not tok.grad.any() and all(p.grad is not None and not p.grad.any() for p in params)


def test_autograd_function_honours_needs_input_grad():
    from imfnet_amd.autograd import AttentionFusionFunction
    c, x, starts, tokens, dz, w = _inputs("rows_1_16_33")
    full, _, _ = _run(x, starts, tokens, dz, w)
    params = [t.clone().requires_grad_(k % 2 == 0) for k, t in enumerate(w)]
    xg = x.clone().requires_grad_(True)
    z = AttentionFusionFunction.apply(xg, starts, tokens, *params)          # tokens: no gradient wanted
    assert torch.equal(z, full["z"])
    z.backward(dz)
    assert torch.equal(xg.grad, full["dx"]) and tokens.grad is None
    for k, p in enumerate(params):
        if k % 2 == 0:
            assert torch.equal(p.grad, full[FC.PARAMS[k]]), k
        else:
            assert p.grad is None


# ======================================================================================================================
# wiring: ResUNet2.transformer inside one training forward + backward of the fixture pair
# ======================================================================================================================
@contextlib.contextmanager
def _switch(name):
    from imfnet_amd import ops
    prev = ops.set_train_fusion(name)
    try:
        yield
    finally:
        ops.set_train_fusion(prev)


def test_model_with_the_switch_at_hip_trains_through_the_op(clouds, images, seeded_sd):
    import backward_restate as R
    import test_gpu_backward_exact as BX
    from imfnet_amd import ops
    from imfnet_amd.autograd import AttentionFusionFunction
    from imfnet_amd.train.trainer import _sparse_input
    point_sets, imgs = BX.whole_network_case(clouds, images, "batch")
    reps, _ = R.batched_voxels(point_sets, 0.05)
    m = BX._new_model(seeded_sd).train()
    st = _sparse_input([torch.as_tensor(r).to(DEV) for r in reps], None, 0.05, torch.device(DEV))
    seen = []
    inner = m.transformer

    def spy(images, F, xyz):
        out = inner(images, F, xyz)
        seen.append((images.detach().clone(), F.detach().clone(), xyz.detach().clone(), out.detach().clone(), out.grad_fn))
        return out

    m.transformer = spy
    with _switch("hip"):
        F = m(st, torch.as_tensor(imgs).to(DEV)).F
        T = torch.randn(F.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
        (F * T).sum().backward()
    assert len(seen) == 1
    im, Fin, xyz, out, grad_fn = seen[0]
    assert "AttentionFusionFunction" in type(grad_fn).__name__
    assert im.shape[0] == 2 and set(xyz[:, 0].tolist()) == {0, 1}
    fusion = dict(m.attention_fusion.named_parameters())
    assert set(fusion) == set(FC.PARAMS)
    for key, p in fusion.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, key
    # the image encoder: the gradient reaches it through dtokens.  The parameters it uses (the ResNet is cut after layer2;
    # what lies behind never receives one) are those the torch switch reaches, finite, not zero, and close to torch's
    enc = {k: p.grad for k, p in m.img_encoder.named_parameters() if p.grad is not None}
    m2 = BX._new_model(seeded_sd).train()
    with _switch("torch"):
        F2 = m2(_sparse_input([torch.as_tensor(r).to(DEV) for r in reps], None, 0.05, torch.device(DEV)),
                torch.as_tensor(imgs).to(DEV)).F
        (F2 * T).sum().backward()
    enc2 = {k: p.grad for k, p in m2.img_encoder.named_parameters() if p.grad is not None}
    assert enc and set(enc) == set(enc2)
    for key, g in enc.items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, key
        scale = float(enc2[key].abs().max())
        assert float((g - enc2[key]).abs().max()) <= BX.REL_TOL * scale + BX.ABS_TOL, key
    # the op alone on the same inputs: the same bits
    tokens = im.flatten(2).transpose(1, 2).contiguous()
    starts = ops.fusion_item_starts(xyz[:, 0], im.shape[0])
    assert starts.tolist()[0] == 0 and starts.tolist()[-1] == Fin.shape[0]
    alone = AttentionFusionFunction.apply(Fin, starts, tokens, *[fusion[k].detach() for k in FC.PARAMS])
    assert torch.equal(alone, out)
    # and with the switch at torch the same call runs the torch body
    with _switch("torch"):
        z = inner(im, Fin.clone().requires_grad_(True), xyz)
    assert "AttentionFusionFunction" not in type(z.grad_fn).__name__
    assert float((z.detach() - out).abs().max()) < 1e-3 * float(out.abs().max())
