"""The descriptor-head training kernels (csrc/head_train.hip) on the GPU: Y and the five gradients against the float64
restatement tests/head_restate.py, gated by the error of torch's own fp32 path on the same GPU and inputs; the exact
properties (reproducible bits, every output written and nothing beyond, rows split at a chunk boundary, the two degenerate
ReLU masks, null outputs, no normalisation, no rows); and the wiring into ResUNet2.forward_layers.

The gate is the one of tests/test_gpu_fusion_train.py, where its factor is derived: e(A) = max|A - A64| / max|A64| per
output tensor and e_hip(A) <= 8 * max(e_torch(A), 2^-24), for sums of at most 2048 terms -- hence head_restate.MAX_ROWS.
tests/test_head_train_host.py checks that e_torch > 0 on these inputs.

Measured on one MI355X, e_hip / max(e_torch, 2^-24), the worst over the seven row counts: Y 1.37, dU 1.49, dS 1.13,
dW1 1.37, dW2 1.58, db 1.69."""
import contextlib

import numpy as np
import pytest
import torch

import head_restate as HR

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR, FLOOR = 8.0, 2.0 ** -24
GUARD = 64                                 # floats on each side of a guarded buffer (keeps 16-byte alignment)
NAN = float("nan")


def _chunk():
    from imfnet_amd import ops
    return ops.head_train_chunk_rows()


def _dev(c):
    return {k: c[k].to(DEV) for k in ("U", "S", "W1", "W2", "b", "dY")}


def _run(d, normalize=True, want=None):
    """{tensor name: result} of one forward and one backward call, and the two meta words."""
    from imfnet_amd import ops
    h, r, y, meta_f = ops.head_train_forward(d["U"], d["S"], d["W1"], d["W2"], d["b"], normalize)
    du, ds, dw1, dw2, db, meta_b = ops.head_train_backward(d["dY"], y, r, h, d["U"], d["S"], d["W1"], d["W2"], normalize, want)
    return dict(Y=y, dU=du, dS=ds, dW1=dw1, dW2=dw2, db=db, H=h, r=r), int(meta_f.item()), int(meta_b.item())


def _gate(hip, tor, ref, label):
    late = []
    for key in HR.TENSORS:
        e_hip, e_torch = HR.rel_err(hip[key], ref[key]), HR.rel_err(tor[key], ref[key])
        ratio = e_hip / max(e_torch, FLOOR)
        print(f"{label} {key}: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}  e_hip / max(e_torch, 2^-24) = {ratio:.3f}")
        if not e_hip <= FACTOR * max(e_torch, FLOOR):
            late.append((key, e_hip, e_torch))
    return late


def test_every_output_within_eight_times_torchs_own_fp32_error():
    ns = HR.row_counts(_chunk())
    assert len(ns) >= 6 and max(ns) <= HR.MAX_ROWS
    late = []
    for n in ns:
        c = HR.case(n)
        hip, mf, mb = _run(_dev(c))
        assert mf == 0 and mb == 0
        tor = HR.torch_path(c, dtype=torch.float32, device=DEV)
        late += [(n,) + row for row in _gate(hip, tor, HR.reference(n), f"n={n}")]
        assert HR.rel_err(hip["H"], HR.reference(n)["H"]) < 1e-5 and HR.rel_err(hip["r"], HR.reference(n)["r"]) < 1e-5
    assert not late, late


def test_without_the_normalisation_the_same_gate_holds_and_r_is_not_written():
    n = _chunk() + 1
    c = HR.case(n)
    hip, mf, mb = _run(_dev(c), normalize=False)
    assert hip["r"] is None and mf == 0 and mb == 0
    tor = HR.torch_path(c, dtype=torch.float32, device=DEV, normalize=False)
    late = _gate(hip, tor, HR.reference(n, normalize=False), f"n={n} normalize=0")
    assert not late, late


def _guarded(shape, fill=NAN):
    """(whole buffer, interior view of `shape`): GUARD floats of the pattern on both sides."""
    n = int(np.prod(shape))
    n4 = (n + 3) // 4 * 4
    buf = torch.full((n4 + 2 * GUARD,), fill, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def test_two_calls_give_the_same_bits_and_write_every_element_and_nothing_beyond():
    """The second call writes into NaN-filled buffers between NaN-filled guard bands: every element of every output comes
    back written, bit-equal to the first call's, and the bands (and the padding up to a multiple of four) stay NaN."""
    from imfnet_amd import ops
    R = _chunk()
    for n in (1, 33, 2 * R + 17):
        d = _dev(HR.case(n))
        a, _, _ = _run(d)
        shapes = dict(H=(n, 64), r=(n,), Y=(n, 32), dU=(n, 64), dS=(n, 32), dW1=(96, 64), dW2=(64, 32), db=(1, 32))
        g = {k: _guarded(s) for k, s in shapes.items()}
        h, r, y, _ = ops.head_train_forward(d["U"], d["S"], d["W1"], d["W2"], d["b"], True, out=(g["H"][1], g["r"][1], g["Y"][1]))
        assert h is g["H"][1] and y is g["Y"][1]
        outs = tuple(g[k][1] for k in ("dU", "dS", "dW1", "dW2", "db"))
        got = ops.head_train_backward(d["dY"], y, r, h, d["U"], d["S"], d["W1"], d["W2"], True, outputs=outs)
        assert all(t is o for t, o in zip(got[:5], outs))
        torch.cuda.synchronize()
        for key, (buf, view) in g.items():
            assert not torch.isnan(view).any(), (n, key)
            assert torch.equal(view, a[key]), (n, key)
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + view.numel():]).all()), (n, key)


def test_rows_split_at_a_chunk_boundary_equal_one_call_bit_for_bit():
    R = _chunk()
    n = 2 * R + 17
    d = _dev(HR.case(n))
    whole, _, _ = _run(d)
    for cut in (R, 2 * R):
        parts = []
        for lo, hi in ((0, cut), (cut, n)):
            p = dict(d, U=d["U"][lo:hi].contiguous(), S=d["S"][lo:hi].contiguous(), dY=d["dY"][lo:hi].contiguous())
            parts.append(_run(p)[0])
        for key in ("Y", "dU", "dS"):
            assert torch.equal(torch.cat([parts[0][key], parts[1][key]]), whole[key]), (cut, key)


def test_dead_and_alive_relu_masks():
    """H == 0 everywhere: every Y row is b / |b| (all rows the same bits), dW1, dW2, dU and dS are exactly +0.0 and db is
    not; H > 0 everywhere: the gate, with every mask bit set."""
    n = 40
    c = HR.case(n, "dead")
    hip, mf, mb = _run(_dev(c))
    assert mf == 0 and mb == 0 and not hip["H"].any()
    want = (c["b"].double() / c["b"].double().norm()).to(DEV)[0]
    assert torch.equal(hip["Y"], hip["Y"][:1].expand(n, 32))
    # Z = +0.0 + b exactly; r^2 is two roundings per lane and four tree adds, halved by the root, then the root's and the
    # division's own rounding: 5 * 2^-24 relative
    assert float((hip["Y"][0].double() - want).abs().max()) <= 5 * FLOOR * float(want.abs().max())
    for key in ("dW1", "dU", "dS", "dW2"):                                            # dW2 = H^T dZ with H = 0
        assert int(hip[key].view(torch.int32).abs().max()) == 0, key                  # +0.0, not -0.0
    ref, tor = HR.reference(n, "dead"), HR.torch_path(c, dtype=torch.float32, device=DEV)
    assert hip["db"].any()
    for key in ("Y", "db"):
        e_hip, e_torch = HR.rel_err(hip[key], ref[key]), HR.rel_err(tor[key], ref[key])
        print(f"dead {key}: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}")
        assert e_hip <= FACTOR * max(e_torch, FLOOR), key
    c = HR.case(n, "alive")
    hip, _, _ = _run(_dev(c))
    assert bool((hip["H"] > 0).all())
    late = _gate(hip, HR.torch_path(c, dtype=torch.float32, device=DEV), HR.reference(n, "alive"), "alive")
    assert not late, late


def test_null_gradient_pointers_leave_the_other_outputs_bits_unchanged():
    d = _dev(HR.case(33))
    keys = ("dU", "dS", "dW1", "dW2", "db")
    for normalize in (True, False):
        full, _, _ = _run(d, normalize)
        masks = [[j != k for j in range(5)] for k in range(5)] + [[j == k for j in range(5)] for k in range(5)]
        masks += [[False] * 5, [False, False, False, True, True]]
        for want in masks:
            part, _, mb = _run(d, normalize, want)
            assert mb == 0
            for key, k in zip(keys, want):
                if k:
                    assert torch.equal(part[key], full[key]), (key, want, normalize)
                else:
                    assert part[key] is None, key


def test_no_rows_write_plus_zero_parameter_gradients_and_autograd_agrees():
    from imfnet_amd import ops
    from imfnet_amd.autograd import HeadFunction
    c = _dev(HR.case(4))
    u, s, dy = c["U"][:0].contiguous(), c["S"][:0].contiguous(), c["dY"][:0].contiguous()
    h, r, y, meta = ops.head_train_forward(u, s, c["W1"], c["W2"], c["b"])
    assert h.shape == (0, 64) and r.shape == (0,) and y.shape == (0, 32) and int(meta.item()) == 0
    outs = (None, None, torch.full((96, 64), NAN, device=DEV), torch.full((64, 32), NAN, device=DEV), None)
    got = ops.head_train_backward(dy, y, r, h, u, s, c["W1"], c["W2"], outputs=outs)
    assert got[4] is None and all(int(t.view(torch.int32).abs().max()) == 0 for t in got[2:4])
    du, ds, dw1, dw2, db, _ = ops.head_train_backward(dy, y, r, h, u, s, c["W1"], c["W2"])
    assert du.shape == (0, 64) and ds.shape == (0, 32)
    assert all(int(t.view(torch.int32).abs().max()) == 0 for t in (dw1, dw2, db))
    params = [c[k].clone().requires_grad_(True) for k in ("W1", "W2", "b")]
    ug = u.clone().requires_grad_(True)
    out = HeadFunction.apply(ug, s, *params, True)
    out.sum().backward()
    assert out.shape == (0, 32) and ug.grad.shape == (0, 64) and all(p.grad is not None and not p.grad.any() for p in params)


def test_autograd_function_honours_needs_input_grad():
    from imfnet_amd.autograd import HeadFunction
    d = _dev(HR.case(33))
    full, _, _ = _run(d)
    u = d["U"].clone().requires_grad_(True)
    w1, w2, b = d["W1"].clone().requires_grad_(True), d["W2"].clone(), d["b"].clone().requires_grad_(True)
    y = HeadFunction.apply(u, d["S"], w1, w2, b, True)                   # s and w2: no gradient wanted
    assert torch.equal(y, full["Y"])
    y.backward(d["dY"])
    assert torch.equal(u.grad, full["dU"]) and torch.equal(w1.grad, full["dW1"]) and torch.equal(b.grad, full["db"])
    assert w2.grad is None and d["S"].grad is None


def test_rows_without_a_norm_raise_the_flag_word():
    """Not a test of the values at r == 0 (there is no epsilon, as in the reference): only that the meta word says so, and
    that the next call clears it."""
    from imfnet_amd import ops
    d = _dev(HR.case(33))
    good, _, _ = _run(d)
    _, _, y, meta = ops.head_train_forward(d["U"], d["S"], d["W1"], torch.zeros_like(d["W2"]), torch.zeros_like(d["b"]))
    assert int(meta.item()) == ops.HEAD_TRAIN_FLAG_NORM
    _, _, y2, meta2 = ops.head_train_forward(d["U"], d["S"], d["W1"], d["W2"], d["b"])
    assert int(meta2.item()) == 0 and torch.equal(y2, good["Y"])


# ======================================================================================================================
# wiring: ResUNet2.forward_layers inside one training forward + backward of the fixture pair
# ======================================================================================================================
@contextlib.contextmanager
def _switch(name):
    from imfnet_amd import ops
    prev = ops.set_train_head(name)
    try:
        yield
    finally:
        ops.set_train_head(prev)


def test_model_with_the_switch_at_hip_trains_through_the_op(clouds, images, seeded_sd, monkeypatch):
    import backward_restate as R
    import test_gpu_backward_exact as BX
    from imfnet_amd import ops
    from imfnet_amd.model import load_model
    from imfnet_amd.train.trainer import _sparse_input
    point_sets, imgs = BX.whole_network_case(clouds, images, "batch")
    reps, _ = R.batched_voxels(point_sets, 0.05)
    entered = []
    inner = ops.head_train_forward

    def spy(u, s, *a, **k):
        entered.append((tuple(u.shape), tuple(s.shape)))
        return inner(u, s, *a, **k)

    monkeypatch.setattr(ops, "head_train_forward", spy)                 # autograd.HeadFunction.forward calls it by name
    runs = {}
    for name in ("hip", "torch"):
        m = BX._new_model(seeded_sd).train()
        seen = {}
        m.block2_tr.register_forward_hook(lambda mod, args, res, seen=seen: seen.setdefault("block2_tr", res))
        m.block1.register_forward_hook(lambda mod, args, res, seen=seen: seen.setdefault("block1", res))
        st = _sparse_input([torch.as_tensor(r).to(DEV) for r in reps], None, 0.05, torch.device(DEV))
        before = len(entered)
        with _switch(name):
            out = m(st, torch.as_tensor(imgs).to(DEV))
            F = out.F
            T = torch.randn(F.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
            (F * T).sum().backward()
        if name == "hip":
            assert entered[before:] == [((F.shape[0], 64), (F.shape[0], 32))]
            assert "HeadFunction" in type(F.grad_fn).__name__
            assert out.coordinate_map_key == st.coordinate_map_key
        else:
            assert len(entered) == before                                # the torch switch never enters the op
            assert "HeadFunction" not in type(F.grad_fn).__name__
        runs[name] = (F.detach(), {k: p.grad for k, p in m.named_parameters() if p.grad is not None}, seen, T)
    (Fh, gh, seen_h, T), (Ft, gt, seen, _) = runs["hip"], runs["torch"]
    assert set(gh) == set(gt) and len(gh) > 100
    err = float((Fh - Ft).abs().max())
    print(f"descriptors, head switch hip against torch: max abs {err:.3e} over {Fh.shape[0]} rows")
    assert err <= 1e-4
    # the head's three parameters under the gate: each run against the float64 head on the rows that run fed its head (with
    # the other switches at torch the layers before the head do not give the same bits twice, so the rows differ a little)
    def head64(seen, T):
        U, S = torch.relu(seen["block2_tr"].F.detach()), seen["block1"].F.detach()
        return HR.restate(dict(U=U.cpu(), S=S.cpu(), W1=m.conv1_tr.kernel.detach().cpu(), W2=m.final.kernel.detach().cpu(),
                               b=m.final.bias.detach().cpu(), dY=T.cpu()))

    ref_h, ref_t = head64(seen_h, T), head64(seen, T)
    assert HR.rel_err(Fh, ref_h["Y"]) < 1e-5 and HR.rel_err(Ft, ref_t["Y"]) < 1e-5
    late = []
    for key, pname in (("dW1", "conv1_tr.kernel"), ("dW2", "final.kernel"), ("db", "final.bias")):
        e_hip, e_torch = HR.rel_err(gh[pname], ref_h[key]), HR.rel_err(gt[pname], ref_t[key])
        print(f"wiring {pname}: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}  ratio {e_hip / max(e_torch, FLOOR):.3f}")
        if not e_hip <= FACTOR * max(e_torch, FLOOR):
            late.append((pname, e_hip, e_torch))
    assert not late, late
    # covered / not covered on GPU rows: the predicate itself
    o, s1 = seen["block2_tr"], seen["block1"]
    with _switch("hip"):
        assert m.train()._head_kernels_apply(o, s1) is True
        with torch.no_grad():
            assert m._head_kernels_apply(o, s1) is False
        assert m.eval()._head_kernels_apply(o, s1) is False
        small = load_model("ResUNetBN2")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3,
                                         config=None).to(DEV).train()
        assert small._head_kernels_apply(o, s1) is False
    with _switch("torch"):
        assert m.train()._head_kernels_apply(o, s1) is False
