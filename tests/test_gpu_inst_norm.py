"""The sparse InstanceNorm on the GPU (imf_in_* in csrc/norm_train.hip, autograd.SparseInstanceNormFunction,
sparse.MinkowskiInstanceNorm.forward_fused) against the float64 restatement tests/inst_norm_restate.py.

Forward gate, per element (include/imfnet_hip.h states where each term comes from):
    |y - y64| <= 4 * 2^-24 * (|gamma xh64| + |beta| + |res|) + 2^-36 * |gamma|
The first term is the BatchNorm kernel's own bound (three fp32 roundings and a unit for the second-order terms).  The second
covers the fp64 statistics' rounding: for n <= 600, |x| <= 12 and rstd <= 2 it is below 600 * 2^-53 * 12 * 2 ~ 2^-39, and the
term keeps a factor 8 over it.  The hostile case evaluates that term for its own data (`_stat_term`).
Gradient gate, the project's own from the fusion and head tests:
    e(A) = max|A - A64| / max|A64|,   e_hip <= 8 * max(e_torch, 2^-24)
with e_torch from the module's torch body in fp32 on the same GPU and inputs; applied to dx, dgamma, dbeta, dresidual, and
to y as a second check.  Where A64 is zero everywhere (an item of one row passes no gradient to x) A must be zero too.
Under a ReLU the backward's contract is in terms of the forward's own output (g = 0 where not y > 0), so each side's A64
is the restatement's backward under the mask of that side's own y, as tests/test_gpu_norm_train.py does."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

import imf_oracle as O
import inst_norm_restate as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
K_FWD, K_GRAD = 4, 8
STAT = 2.0 ** -36

# item sizes around the 64-lane wavefront and the 128-row chunk; item starts land on odd rows
BATCHES = {"1x257": [257], "1x1": [1], "1x64": [64], "2a": [129, 1], "2b": [1, 128], "3": [37, 5, 120],
           "8a": [1, 2, 63, 64, 65, 127, 128, 129], "8b": [257, 1, 65, 2, 127, 63, 129, 64]}
# every batch meets a vector width (32, 64, 128, 256) and the scalar path (3, 5)
CASES = [("1x257", 32), ("1x257", 3), ("1x1", 64), ("1x1", 5), ("1x64", 128), ("1x64", 3), ("2a", 32), ("2a", 5),
         ("2b", 256), ("2b", 3), ("3", 64), ("3", 3), ("8a", 128), ("8a", 5), ("8b", 256), ("8b", 32), ("8b", 3)]
CASE_IDS = [f"{b}_C={c}" for b, c in CASES]
COMBOS = list(itertools.product((False, True), (False, True)))           # (relu, residual)


def _np(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def _switch(name):
    from imfnet_amd import ops
    prev = ops.set_train_norm(name)
    try:
        yield
    finally:
        ops.set_train_norm(prev)


def _inputs(sizes, c, seed, mean=None, sigma=None):
    """x Gaussian with per-item, per-channel mean in [-4, 4] and sigma in [0.5, 2] (or the given ones), gamma in
    U(0.5, 1.5), beta in U(-0.5, 0.5), Gaussian residual and incoming gradient."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for k in sizes:
        m = torch.rand(1, c, generator=g) * 8 - 4 if mean is None else torch.full((1, c), float(mean))
        s = torch.rand(1, c, generator=g) * 1.5 + 0.5 if sigma is None else torch.full((1, c), float(sigma))
        parts.append(torch.randn(k, c, generator=g) * s + m)
    x = torch.cat(parts)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) - 0.5
    return x, gamma, beta, torch.randn(len(x), c, generator=g), torch.randn(len(x), c, generator=g)


def _starts_dev(sizes):
    return torch.as_tensor(IR.starts_of(sizes), dtype=torch.int32).to(DEV)


def _coords_dev(sizes):
    item = np.concatenate([np.full(k, i, np.int32) for i, k in enumerate(sizes)])
    z = np.zeros(len(item))
    return torch.as_tensor(np.stack([item, np.arange(len(item)), z, z], 1).astype(np.int32)).to(DEV)


class Rows:
    """The stand-in carrier (.F, .C, ._like): the module's torch body on GPU rows, whatever the switch."""

    def __init__(self, F, C):
        self.F, self.C = F, C

    def _like(self, F):
        return Rows(F, self.C)


def _hip(x, sizes, gamma, beta, res, relu, dy):
    from imfnet_amd import ops
    st = _starts_dev(sizes)
    xd, gd = x.to(DEV), gamma.to(DEV)
    y, stats = ops.in_forward(xd, st, gd, beta.to(DEV), IR.EPS, None if res is None else res.to(DEV), relu)
    dx, dgamma, dbeta, dres = ops.in_backward(dy.to(DEV), xd, y, stats, gd, st, relu, want_dresidual=True)
    return dict(y=y, stats=stats, dx=dx, dgamma=dgamma, dbeta=dbeta, dresidual=dres)


def _torch_body(x, sizes, gamma, beta, res, relu, dy):
    """Today's torch ops (norm, add, relu) in fp32 on the GPU and torch's autograd of them."""
    import imfnet_amd.sparse as ME
    norm = ME.MinkowskiInstanceNorm(x.shape[1]).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(gamma.reshape(1, -1))
        norm.bias.copy_(beta.reshape(1, -1))
    xd = x.to(DEV).requires_grad_(True)
    rd = None if res is None else res.to(DEV).requires_grad_(True)
    with _switch("torch"):
        y = norm.forward_fused(Rows(xd, _coords_dev(sizes)), residual=rd, relu=relu).F
    y.backward(dy.to(DEV))
    return dict(y=y.detach(), dx=xd.grad, dgamma=norm.weight.grad.reshape(-1), dbeta=norm.bias.grad.reshape(-1),
                dresidual=None if rd is None else rd.grad)


def _e(a, a64):
    """max|A - A64| / max|A64|; 0 when both are zero everywhere, inf when only A64 is."""
    a, a64 = _np(a).astype(np.float64).reshape(a64.shape), np.asarray(a64)
    err, scale = float(np.abs(a - a64).max()), float(np.abs(a64).max())
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


def _references(x, sizes, gamma, beta, res, relu, dy, y_of):
    starts = IR.starts_of(sizes)
    fw = IR.forward(x.numpy(), starts, gamma.numpy(), beta.numpy(), None if res is None else res.numpy(), relu)
    bw = IR.backward(dy.numpy(), x.numpy(), _np(y_of), starts, gamma.numpy(), relu)      # the mask of that side's own y
    return fw, dict(y=fw["y"], dx=bw["dx"], dgamma=bw["dgamma"], dbeta=bw["dbeta"], dresidual=bw["dresidual"])


def _forward_bound(fw, gamma, beta, res, stat):
    ga = np.abs(gamma.numpy().astype(np.float64))
    return K_FWD * U * (ga * np.abs(fw["xhat"]) + np.abs(beta.numpy().astype(np.float64))
                        + (np.abs(res.numpy().astype(np.float64)) if res is not None else 0.0)) + stat


def _check(x, sizes, gamma, beta, res_t, dy, label, stat_of=None):
    """All four relu x residual combinations of one input: the forward bound per element and the gradient gate per tensor.
    Returns the worst e_hip / max(e_torch, 2^-24) per tensor and the torch body's worst e."""
    worst = {k: 0.0 for k in ("y", "dx", "dgamma", "dbeta", "dresidual")}
    worst_torch = dict(worst)
    for relu, with_res in COMBOS:
        res = res_t if with_res else None
        hip = _hip(x, sizes, gamma, beta, res, relu, dy)
        tor = _torch_body(x, sizes, gamma, beta, res, relu, dy)
        fw, ref_hip = _references(x, sizes, gamma, beta, res, relu, dy, hip["y"])
        _, ref_tor = _references(x, sizes, gamma, beta, res, relu, dy, tor["y"])
        stat = STAT * np.abs(gamma.numpy().astype(np.float64)) if stat_of is None else stat_of(fw)
        bound = _forward_bound(fw, gamma, beta, res, stat)
        err = np.abs(_np(hip["y"]).astype(np.float64) - fw["y"])
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        e_y_torch = _e(tor["y"], ref_tor["y"])
        print(f"{label} relu={relu} res={with_res}: forward err/bound {ratio:.3f}  (torch body e(y) = {e_y_torch:.3e})")
        assert (err <= bound).all(), (label, relu, with_res, ratio, f"torch body e(y) = {e_y_torch:.3e}")
        if relu:
            assert float(_np(hip["y"]).min()) >= 0.0
        assert np.array_equal(_np(hip["dresidual"]).astype(np.float64), ref_hip["dresidual"])   # dresidual == g exactly
        for key in worst:
            e_hip = _e(hip[key], ref_hip[key])
            e_tor = 0.0 if tor[key] is None else _e(tor[key], ref_tor[key])      # no residual: torch has no dresidual
            r = e_hip / max(e_tor, U)
            worst[key], worst_torch[key] = max(worst[key], r), max(worst_torch[key], e_tor)
            print(f"{label} relu={relu} res={with_res} {key}: e_hip {e_hip:.3e} e_torch {e_tor:.3e} ratio {r:.3f}")
            assert e_hip <= K_GRAD * max(e_tor, U), (label, key, relu, with_res, e_hip, f"torch body e = {e_tor:.3e}")
    return worst, worst_torch


def test_cases_cover_the_item_sizes_batches_and_channels():
    from imfnet_amd import _lib, ops
    assert ops.bn_train_chunk_rows() == 128                              # the sizes below sit around this and the 64 lanes
    assert {k for b in BATCHES.values() for k in b} == {1, 2, 5, 37, 120, 63, 64, 65, 127, 128, 129, 257}
    assert max(len(b) for b in BATCHES.values()) == _lib.MAX_BATCH and {len(b) for b in BATCHES.values()} == {1, 2, 3, 8}
    assert {c for _, c in CASES} == {32, 64, 128, 256, 3, 5} and {b for b, _ in CASES} == set(BATCHES)
    assert any(s % 2 for b in BATCHES.values() for s in IR.starts_of(b)[1:-1])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_forward_and_backward_meet_their_gates(case):
    sizes, c = BATCHES[case[0]], case[1]
    x, gamma, beta, res, dy = _inputs(sizes, c, 7919 * CASES.index(case) + 1)
    worst, _ = _check(x, sizes, gamma, beta, res, dy, f"{case[0]}_C={c}")
    print(f"{case}: worst e_hip / max(e_torch, 2^-24) {worst}")


def test_one_row_items_give_beta_and_pass_no_gradient_to_x():
    sizes, c = [129, 1], 32
    x, gamma, beta, res, dy = _inputs(sizes, c, 5)
    got = _hip(x, sizes, gamma, beta, None, False, dy)
    assert torch.equal(got["y"][129], beta.to(DEV)) and not got["dx"][129].any()
    got = _hip(x, sizes, gamma, beta, res, False, dy)
    assert torch.equal(got["y"][129], beta.to(DEV) + res[129].to(DEV))


def test_a_channel_that_is_constant_inside_an_item_has_rstd_1e4_and_xh_zero():
    sizes, c = [37, 5, 120], 8
    x, gamma, beta, _, dy = _inputs(sizes, c, 6)
    x[:37, 0] = 1.7                                                      # not a dyadic value: fp32(1.7) in every row
    got = _hip(x, sizes, gamma, beta, None, False, dy)
    stats = _np(got["stats"])
    assert stats.shape == (3, 2 * c) and stats[0, 0] == float(np.float32(1.7))       # variance 0: the mean is the value
    assert abs(stats[0, c] * np.sqrt(IR.EPS) - 1.0) <= 1e-15
    assert torch.equal(got["y"][:37, 0], beta[0].to(DEV).expand(37))
    fw, ref = _references(x, sizes, gamma, beta, None, False, dy, got["y"])
    assert _e(got["dx"], ref["dx"]) <= K_GRAD * U                        # dx of that channel is 1e4 * gamma * (g - mean g)


def _stat_term(fw, x, sizes, gamma):
    """The statistics term of the forward bound for the data at hand, from include/imfnet_hip.h with the gate's factor 8:
        8 * |gamma| * rstd_b * 2^-53 * (n_b * max_b |x - p| + 2 |mean_b|),   p = the item's first row,
    per item b and channel, broadcast over the item's rows."""
    starts = IR.starts_of(sizes)
    x64, ga = x.numpy().astype(np.float64), np.abs(gamma.numpy().astype(np.float64))
    out = np.zeros_like(x64)
    for b in range(len(sizes)):
        s, e = starts[b], starts[b + 1]
        d = np.abs(x64[s:e] - x64[s]).max(0)
        out[s:e] = 8 * ga * fw["rstd"][b] * 2.0 ** -53 * ((e - s) * d + 2 * np.abs(fw["mean"][b]))
    return out


def test_hostile_statistics_mean_1000_sigma_1():
    """|mean| / sigma = 1000 in every channel: the kernels centre in fp64 about the item's first row, so both gates hold;
    the torch body's own error is in the printed lines and in every assertion message."""
    sizes, c = [129, 65, 257], 32
    x, gamma, beta, res, dy = _inputs(sizes, c, 77, mean=1000.0, sigma=1.0)
    worst, worst_torch = _check(x, sizes, gamma, beta, res, dy, "hostile",
                                stat_of=lambda fw: _stat_term(fw, x, sizes, gamma))
    print(f"hostile: worst ratio {worst}; torch body e {worst_torch}")


def test_same_bits_twice():
    sizes, c = BATCHES["8b"], 32
    x, gamma, beta, res, dy = _inputs(sizes, c, 9)
    a, b = (_hip(x, sizes, gamma, beta, res, True, dy) for _ in range(2))
    for key in a:
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("c", [32, 5])
def test_an_items_bits_depend_on_that_item_alone(c):
    """Rows of item 0, and of the last item (which starts on a row that is no multiple of 4), from a batch of three are
    bit-equal in y and dx to running that item as a batch of one."""
    sizes = [65, 129, 127]
    x, gamma, beta, res, dy = _inputs(sizes, c, 10)
    full = _hip(x, sizes, gamma, beta, res, True, dy)
    starts = IR.starts_of(sizes)
    assert starts[2] % 4 != 0
    for b in (0, 2):
        s, e = int(starts[b]), int(starts[b + 1])
        one = _hip(x[s:e].contiguous(), [e - s], gamma, beta, res[s:e].contiguous(), True, dy[s:e].contiguous())
        assert torch.equal(full["y"][s:e], one["y"]) and torch.equal(full["dx"][s:e], one["dx"]), b
        assert torch.equal(full["stats"][b], one["stats"][0])


def test_an_item_without_rows_writes_nothing_and_disturbs_nothing():
    from imfnet_amd import ops
    x, gamma, beta, res, dy = _inputs([5, 7], 32, 12)
    want = _hip(x, [5, 7], gamma, beta, res, True, dy)
    st = torch.tensor([0, 5, 5, 12], dtype=torch.int32, device=DEV)
    xd, gd = x.to(DEV), gamma.to(DEV)
    y, stats = ops.in_forward(xd, st, gd, beta.to(DEV), IR.EPS, res.to(DEV), True)
    got = ops.in_backward(dy.to(DEV), xd, y, stats, gd, st, True, want_dresidual=True)
    assert torch.equal(y, want["y"]) and not stats[1].any()
    assert torch.equal(stats[0], want["stats"][0]) and torch.equal(stats[2], want["stats"][1])
    for a, key in zip(got, ("dx", "dgamma", "dbeta", "dresidual")):
        assert torch.equal(a, want[key]), key


def test_null_outputs_skip_work_but_do_not_change_the_others():
    from imfnet_amd import ops
    sizes = [37, 5, 120]
    x, gamma, beta, _, dy = (t.to(DEV) for t in _inputs(sizes, 32, 13))
    st = _starts_dev(sizes)
    y, stats = ops.in_forward(x, st, gamma, beta, IR.EPS, None, True)
    full = ops.in_backward(dy, x, y, stats, gamma, st, True, want_dresidual=True)
    for mask in itertools.product((False, True), repeat=4):
        part = ops.in_backward(dy, x, y, stats, gamma, st, True, *mask)
        for want, a, b in zip(mask, part, full):
            assert (a is None) if not want else torch.equal(a, b), mask
    nomask = ops.in_backward(dy, x, None, stats, gamma, st, False, want_dresidual=True)
    assert torch.equal(nomask[3], dy)


def test_wrappers_refuse_what_the_kernels_do_not_take():
    from imfnet_amd import ops
    from imfnet_amd._lib import ImfError
    sizes = [5, 7]
    x, gamma, beta, _, _ = (t.to(DEV) for t in _inputs(sizes, 8, 14))
    st = _starts_dev(sizes)
    y, stats = ops.in_forward(x, st, gamma, beta, IR.EPS)
    for call in (lambda: ops.in_forward(x.double(), st, gamma, beta, IR.EPS),
                 lambda: ops.in_forward(x, st.long(), gamma, beta, IR.EPS),
                 lambda: ops.in_forward(x, st.cpu(), gamma, beta, IR.EPS),
                 lambda: ops.in_forward(x, st[:1], gamma, beta, IR.EPS),
                 lambda: ops.in_forward(x, torch.zeros(10, dtype=torch.int32, device=DEV), gamma, beta, IR.EPS),
                 lambda: ops.in_forward(x, st, gamma[:5], beta, IR.EPS),
                 lambda: ops.in_forward(x, st, gamma, beta, IR.EPS, residual=x[:4]),
                 lambda: ops.in_forward(x[:0], st, gamma, beta, IR.EPS),
                 lambda: ops.in_backward(x, x, y, stats.reshape(-1), gamma, st),
                 lambda: ops.in_backward(x, x, None, stats, gamma, st, relu=True)):
        with pytest.raises(ImfError):
            call()


# ======================================================================================================================
# module level
# ======================================================================================================================
@pytest.fixture(scope="module")
def batched(clouds):
    """A batched SparseTensor as the trainer builds it (train/trainer.py): two fragments through the batched pyramid."""
    from imfnet_amd.extract import sparse_tensor_from_points, start_geometry
    fut = start_geometry([np.asarray(clouds[0])[::8], np.asarray(clouds[1])[::8]], 0.05, torch.device(DEV))
    st, _ = sparse_tensor_from_points(None, 0.05, torch.device(DEV), geometry=fut)
    return st


def _module(c, seed=21):
    import imfnet_amd.sparse as ME
    g = torch.Generator().manual_seed(seed)
    norm = ME.MinkowskiInstanceNorm(c).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(1, c, generator=g) + 0.5)
        norm.bias.copy_(torch.rand(1, c, generator=g) - 0.5)
    return norm


@contextlib.contextmanager
def _count_hip_forwards(monkeypatch):
    from imfnet_amd.autograd import SparseInstanceNormFunction as Fn
    calls, inner = [], Fn.forward

    def counted(ctx, *a):
        calls.append(1)
        return inner(ctx, *a)
    with monkeypatch.context() as m:
        m.setattr(Fn, "forward", staticmethod(counted))
        yield calls


@contextlib.contextmanager
def _no_device_to_host_copy(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("device-to-host copy inside the norm")
    with monkeypatch.context() as m:
        for name in ("item", "cpu", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, refuse)
        yield


@pytest.mark.parametrize("ts", [1, 2])
def test_module_takes_the_hip_op_on_a_batched_tensor_without_a_device_to_host_copy(batched, monkeypatch, ts):
    """With the switch at hip, on the trainer's batched tensor: the HIP op runs (training with autograd, no_grad and eval
    alike), nothing in the forward copies from the device, and the result is the restatement's within the forward bound.
    With the switch at torch the HIP op never runs."""
    import imfnet_amd.sparse as ME
    cm = batched.coordinate_manager
    lv = cm.level(ts)
    sizes = [cnt for _, cnt in lv.items]
    assert len(sizes) == 2 and sum(sizes) == lv.n
    c = 32
    x, _, _, res, dy = _inputs(sizes, c, 22 + ts)
    norm = _module(c)
    gamma, beta = norm.weight.detach().cpu().reshape(-1), norm.bias.detach().cpu().reshape(-1)
    xin = x.to(DEV).requires_grad_(True)
    rin = res.to(DEV).requires_grad_(True)
    st = ME.SparseTensor(xin, coordinate_map_key=ME.CoordinateMapKey(ts), coordinate_manager=cm)
    rt = ME.SparseTensor(rin, coordinate_map_key=ME.CoordinateMapKey(ts), coordinate_manager=cm)
    with _switch("hip"), _count_hip_forwards(monkeypatch) as calls:
        with _no_device_to_host_copy(monkeypatch):
            out = norm.forward_fused(st, residual=rt, relu=True).F
            plain = norm(st).F
            with torch.no_grad():
                ng = norm.forward_fused(st, residual=rt, relu=True).F
            ev = norm.eval().forward_fused(st, residual=rin, relu=True).F
            norm.train()
        assert len(calls) == 4
        out.backward(dy.to(DEV))
    assert torch.equal(out.detach(), ng) and torch.equal(ng, ev.detach()) and ng.requires_grad is False
    fw, ref = _references(x, sizes, gamma, beta, res, True, dy, out)
    bound = _forward_bound(fw, gamma, beta, res, STAT * np.abs(gamma.numpy().astype(np.float64)))
    assert (np.abs(_np(out).astype(np.float64) - fw["y"]) <= bound).all()
    assert (np.abs(_np(plain).astype(np.float64) - IR.forward(x.numpy(), IR.starts_of(sizes), gamma.numpy(),
                                                             beta.numpy())["y"]) <= bound).all()
    for key, got in (("dx", xin.grad), ("dgamma", norm.weight.grad), ("dbeta", norm.bias.grad), ("dresidual", rin.grad)):
        assert _e(got, ref[key]) <= K_GRAD * U, key
    assert norm.weight.grad.shape == norm.weight.shape and norm.bias.grad.shape == norm.bias.shape
    with _switch("torch"), _count_hip_forwards(monkeypatch) as calls:
        tor = norm.forward_fused(st, residual=rt, relu=True).F
        with torch.no_grad():
            norm.eval().forward_fused(st, relu=True)
        norm.train()
        assert not calls
    assert float((tor - out).detach().abs().max()) < 1e-4


def test_the_torch_body_waits_for_the_device_and_the_hip_path_does_not(batched, monkeypatch):
    """What the switch removes: with torch, the module's forward reads a value back from the device (Tensor.item) on every
    call; with hip it never does."""
    import imfnet_amd.sparse as ME
    lv = batched.coordinate_manager.level(1)
    st = ME.SparseTensor(torch.randn(lv.n, 32, device=DEV), coordinate_map_key=ME.CoordinateMapKey(1),
                         coordinate_manager=batched.coordinate_manager)
    norm = _module(32)
    with _switch("torch"), _no_device_to_host_copy(monkeypatch), pytest.raises(AssertionError, match="device-to-host"):
        norm(st)
    with _switch("hip"), _no_device_to_host_copy(monkeypatch):
        norm(st)


def test_user_coordinates_know_their_partition_from_construction_or_stay_on_torch(monkeypatch):
    """ME.SparseTensor(coordinates=...): built with the switch at hip it learns at construction -- where the host waits for
    the row count anyway -- that its rows are grouped by item, and every level's norm then runs on the HIP op without a
    copy; rows that are not grouped, and a tensor built with the switch at torch, stay on the torch ops."""
    import imfnet_amd.sparse as ME
    g = torch.Generator().manual_seed(31)
    xyz = torch.randint(0, 12, (400, 3), generator=g).unique(dim=0)
    cut = len(xyz) // 3 | 1
    coords = torch.cat([torch.cat([torch.zeros(cut, 1, dtype=torch.long), xyz[:cut]], 1),
                        torch.cat([torch.ones(len(xyz) - cut, 1, dtype=torch.long), xyz[cut:]], 1)]).int()
    feats = torch.randn(len(coords), 8, generator=g)
    norm = _module(8)
    with _switch("hip"):
        st = ME.SparseTensor(feats, coordinates=coords, device=DEV)
        shuffled = ME.SparseTensor(feats, coordinates=coords.flip(0), device=DEV)
    with _switch("torch"):
        late = ME.SparseTensor(feats, coordinates=coords, device=DEV)
    assert st.coordinate_manager.n_items == 2 and shuffled.coordinate_manager.n_items is None
    assert late.coordinate_manager.n_items is None
    n2 = st.coordinate_manager.level(2).n
    coarse = st._like(torch.randn(n2, 8, generator=g).to(DEV), 2)
    item2 = st.coordinate_manager.coords(2)[:, 0].cpu().numpy()
    assert (np.diff(item2) >= 0).all()                                   # the coarser level keeps the rows grouped
    with _switch("hip"), _count_hip_forwards(monkeypatch) as calls:
        with _no_device_to_host_copy(monkeypatch):
            a, b = norm(st).F, norm(coarse).F
        assert len(calls) == 2
        assert st.coordinate_manager.item_starts(1, len(coords)).tolist() == [0, cut, len(coords)]
        c, d = norm(shuffled).F, norm(late).F
        assert len(calls) == 2
    a, b, c, d = (t.detach() for t in (a, b, c, d))
    ref =O.instance_norm(feats, coords[:, 0].numpy(), norm.weight.detach().cpu(), norm.bias.detach().cpu())
    assert float((a.cpu() - ref).abs().max()) < 1e-5 and float((d.cpu() - ref).abs().max()) < 1e-5
    ref2 = O.instance_norm(coarse.F.cpu(), item2, norm.weight.detach().cpu(), norm.bias.detach().cpu())
    assert float((b.cpu() - ref2).abs().max()) < 1e-5
    ref3 = O.instance_norm(feats, coords.flip(0)[:, 0].numpy(), norm.weight.detach().cpu(), norm.bias.detach().cpu())
    assert float((c.cpu() - ref3).abs().max()) < 1e-5


# ======================================================================================================================
# model level
# ======================================================================================================================
def _in_state_dict(seeded_sd, seed=5):
    """The seeded BN state dict with the seven residual blocks' norms replaced by InstanceNorm parameters ([1, C] weight /
    bias, no running statistics): the schema of ResUNetIN2C (tests/test_gpu_parity.py builds the same)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in seeded_sd.items():
        if k.startswith("block") and ".bn." in k:
            if k.endswith(".bn.weight"):
                sd[k.replace(".bn.weight", ".weight")] = (torch.rand(1, v.numel(), generator=g) + 0.5)
            elif k.endswith(".bn.bias"):
                sd[k.replace(".bn.bias", ".bias")] = (torch.rand(1, v.numel(), generator=g) - 0.5) * 0.2
            continue
        sd[k] = v
    return sd


def test_resunet_in2c_with_the_switch_at_hip_matches_the_oracle(seeded_sd, clouds, images, monkeypatch):
    """ResUNetIN2C in eval mode on the fixture pair as a batch of two, every fourth point: descriptors within 1e-4 of
    oracle.resunet_forward (the bound of test_gpu_parity.py::test_instance_norm_variant_matches_oracle), item 0 alone
    within 2e-5 of its rows in the batch, and all fourteen block norms of each forward on the HIP op."""
    import imfnet_amd.sparse as ME
    from imfnet_amd.model import load_model
    sd = _in_state_dict(seeded_sd)
    m = load_model("ResUNetIN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3)
    m.load_state_dict(sd, strict=True)
    m = m.eval().to(DEV)
    cs = [O.voxelize(clouds[i].astype(np.float64)[::4], 0.05)[0] for i in (0, 1)]
    coords = np.concatenate([np.concatenate([np.full((len(c), 1), i, np.int32), c[:, 1:]], 1) for i, c in enumerate(cs)])
    img = np.concatenate([images[0], images[1]])
    with _switch("hip"), _count_hip_forwards(monkeypatch) as calls, torch.no_grad():
        st = ME.SparseTensor(torch.ones(len(coords), 1), coordinates=torch.as_tensor(coords), device=DEV)
        Fb = m(st, torch.as_tensor(img).to(DEV)).F.cpu()
        assert len(calls) == 14
        st0 = ME.SparseTensor(torch.ones(len(cs[0]), 1), coordinates=torch.as_tensor(coords[:len(cs[0])]), device=DEV)
        F0 = m(st0, torch.as_tensor(images[0]).to(DEV)).F.cpu()
        assert len(calls) == 28
    Fr = O.resunet_forward(sd, coords, img)
    assert Fb.shape == Fr.shape and float((Fb - Fr).abs().max()) < 1e-4
    assert float((F0 - Fb[:len(cs[0])]).abs().max()) < 2e-5
