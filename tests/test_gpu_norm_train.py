"""Training-mode sparse BatchNorm on the GPU (csrc/norm_train.hip, autograd.SparseBatchNormFunction,
sparse.MinkowskiBatchNorm.forward_fused) against the float64 restatement tests/norm_restate.py.

The bounds are counted from the kernel's roundings (the comment at the head of csrc/norm_train.hip):
  forward   |y - y_ref| <= K_FWD * 2^-24 * (|gamma xh| + |beta| + |residual|),  K_FWD = 4: three fp32 roundings (xh, the
            fma, the residual add) and one unit for the second-order terms and what fp64 carries;
  backward  every fp32 output is one rounding of an fp64 value, K_BWD = 2 with the second unit for what fp64 carries:
            dx against |gamma| rstd (|g| + |dbeta| / N + |xh dgamma| / N), dgamma against sum |g xh|, dbeta against sum |g|.
The same K_FWD holds at |mean| / sigma = 1e4: the kernel centres in fp64."""
import contextlib
import copy
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_restate as NR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
EPS = 1e-5
K_FWD, K_BWD = 4, 2
U = 2.0 ** -24
EINVAL = -1

# N in terms of R = imf_bn_train_chunk_rows(); every N meets every kind of C (1, odd, the vector widths) at least once
N_NAMES = {"2": lambda R: 2, "3": lambda R: 3, "R-1": lambda R: R - 1, "R": lambda R: R, "R+1": lambda R: R + 1,
           "2R+3": lambda R: 2 * R + 3}
CASES = [("2", 1), ("2", 32), ("2", 48), ("3", 3), ("3", 256), ("R-1", 1), ("R-1", 48), ("R", 3), ("R", 32), ("R", 256),
         ("R+1", 48), ("R+1", 256), ("2R+3", 1), ("2R+3", 3), ("2R+3", 32), ("2R+3", 48), ("2R+3", 256)]
CASE_IDS = [f"N={n}_C={c}" for n, c in CASES]
COMBOS = list(itertools.product((False, True), (False, True)))           # (relu, residual)


def _rows(name):
    from imfnet_amd import ops
    return N_NAMES[name](ops.bn_train_chunk_rows())


def _gen(case, salt=0):
    return torch.Generator().manual_seed(7919 * CASES.index(case) + salt)


def _ints(gen, shape):
    return torch.randint(-8, 9, shape, generator=gen).float()


def _affine(gen, c):
    return torch.randn(c, generator=gen) + 1.0, torch.randn(c, generator=gen)


def _forward(x, gamma, beta, res=None, relu=False, rm=None, rv=None, mom=0.0):
    from imfnet_amd import ops
    y, stats = ops.bn_train_forward(x.to(DEV), gamma.to(DEV), beta.to(DEV), EPS, None if res is None else res.to(DEV),
                                    relu, rm, rv, mom)
    return y, stats


def _np(t):
    return t.detach().cpu().numpy()


def test_chunk_rows_is_a_constant_of_the_build():
    from imfnet_amd import ops
    R = ops.bn_train_chunk_rows()
    assert R == ops.bn_train_chunk_rows() and R >= 4
    assert sorted({_rows(n) for n, _ in CASES}) == [2, 3, R - 1, R, R + 1, 2 * R + 3]
    assert {c for _, c in CASES} == {1, 3, 32, 48, 256}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_statistics_are_exact_on_integer_data(case):
    """x holds integers in [-8, 8]: the fp64 mean is an exact integer sum and one correctly rounded division, bit-equal
    to the restatement's; rstd within 1e-12 relative."""
    n, c = _rows(case[0]), case[1]
    g = _gen(case)
    x = _ints(g, (n, c))
    gamma, beta = _affine(g, c)
    _, stats = _forward(x, gamma, beta)
    mean, _, rstd = NR.batch_stats(x.numpy(), EPS)
    got = _np(stats)
    assert got.dtype == np.float64 and got.shape == (2 * c,)
    assert np.array_equal(got[:c], mean), np.abs(got[:c] - mean).max()
    rel = np.abs(got[c:] - rstd) / rstd
    print(f"{case}: max relative rstd error {rel.max():.2e}")
    assert (rel <= 1e-12).all()


def _check_forward_backward(case, x, label):
    """All four relu x residual combinations of one input: forward and backward against the restatement."""
    from imfnet_amd import ops
    n, c = x.shape
    g = _gen(case, salt=1)
    gamma, beta = _affine(g, c)
    res_t = torch.randn(n, c, generator=g)
    dy = torch.randn(n, c, generator=g)
    dy_int = _ints(g, (n, c))
    worst = {"y": 0.0, "dx": 0.0, "dgamma": 0.0, "dbeta": 0.0}
    for relu, with_res in COMBOS:
        res = res_t if with_res else None
        y, stats = _forward(x, gamma, beta, res, relu)
        fw = NR.forward(x.numpy(), gamma.numpy(), beta.numpy(), EPS, None if res is None else res.numpy(), relu)
        bound = K_FWD * U * (np.abs(gamma.numpy().astype(np.float64) * fw["xhat"]) + np.abs(beta.numpy().astype(np.float64))
                             + (np.abs(res.numpy().astype(np.float64)) if with_res else 0.0))
        err = np.abs(_np(y).astype(np.float64) - fw["y"])
        worst["y"] = max(worst["y"], float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (label, relu, with_res, float((err / np.maximum(bound, 1e-300)).max()))
        if relu:
            assert float(_np(y).min()) >= 0.0
        for grad in (dy, dy_int):
            dx, dgamma, dbeta, dres = ops.bn_train_backward(grad.to(DEV), x.to(DEV), y, stats, gamma.to(DEV), relu,
                                                            want_dresidual=True)
            bw = NR.backward(grad.numpy(), x.numpy(), _np(y), gamma.numpy(), EPS, relu)     # the mask of the GPU's own y
            assert np.array_equal(_np(dres).astype(np.float64), bw["g"])                    # dresidual == g exactly
            ga = np.abs(gamma.numpy().astype(np.float64))
            b_dx = K_BWD * U * ga * bw["rstd"] * (np.abs(bw["g"]) + np.abs(bw["dbeta"]) / n
                                                  + np.abs(bw["xhat"] * bw["dgamma"]) / n)
            b_dg = K_BWD * U * np.abs(bw["g"] * bw["xhat"]).sum(0)
            b_db = K_BWD * U * np.abs(bw["g"]).sum(0)
            for key, got, bnd in (("dx", dx, b_dx), ("dgamma", dgamma, b_dg), ("dbeta", dbeta, b_db)):
                e = np.abs(_np(got).astype(np.float64) - bw[key])
                ok = e <= bnd
                ratio = float((e / np.maximum(bnd, 1e-300))[bnd > 0].max()) if (bnd > 0).any() else 0.0
                worst[key] = max(worst[key], ratio)
                assert ok.all(), (label, key, relu, with_res, ratio)
            if grad is dy_int:                       # integer gradients: the masked sum is exact, so is its fp32 value
                want = torch.as_tensor(bw["dbeta"]).float()
                assert torch.equal(want.double(), torch.as_tensor(bw["dbeta"]))
                assert torch.equal(dbeta.cpu(), want)
    print(f"{label} {case}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_forward_and_backward_on_gaussian_data_stay_within_the_counted_bounds(case):
    n, c = _rows(case[0]), case[1]
    _check_forward_backward(case, torch.randn(n, c, generator=_gen(case)) * 2.0 + 0.5, "gaussian")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_forward_and_backward_at_mean_over_sigma_1e4_stay_within_the_same_bounds(case):
    """x = 1000 + 0.1 * noise: fp32 statistics or an fp32 centring would lose 1e4 ulp here; the same k holds."""
    n, c = _rows(case[0]), case[1]
    _check_forward_backward(case, 1000.0 + 0.1 * torch.randn(n, c, generator=_gen(case)), "adversarial")


def test_zero_pre_activation_gives_zero_gradient_as_torch_does():
    """Channels with gamma = beta = 0 (and a zero residual): pre-activation exactly 0, so y = 0 and the mask y > 0 passes
    no gradient; torch's ReLU backward gives 0 there as well."""
    n, c = _rows("R+1"), 8
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(n, c, generator=g), torch.randn(n, c, generator=g).abs() + 0.1
    gamma, beta = _affine(g, c)
    gamma[::2], beta[::2] = 0.0, 0.0
    res = torch.randn(n, c, generator=g)
    res[:, ::2] = 0.0
    from imfnet_amd import ops
    for with_res in (False, True):
        r = res if with_res else None
        y, stats = _forward(x, gamma, beta, r, True)
        assert not y[:, ::2].any()
        dx, dgamma, dbeta, dres = ops.bn_train_backward(dy.to(DEV), x.to(DEV), y, stats, gamma.to(DEV), True,
                                                        want_dresidual=True)
        assert not dres[:, ::2].any() and not dx[:, ::2].any() and not dbeta[::2].any() and not dgamma[::2].any()
        assert dbeta[1::2].abs().min() > 0
        xt, gt, bt = (t.to(DEV).requires_grad_(True) for t in (x, gamma, beta))
        rt = None if r is None else r.to(DEV).requires_grad_(True)
        yt = F.batch_norm(xt, None, None, gt, bt, training=True, eps=EPS)
        yt = F.relu(yt if rt is None else yt + rt)
        yt.backward(dy.to(DEV))
        assert not bt.grad[::2].any() and not xt.grad[:, ::2].any()
        if rt is not None:
            assert not rt.grad[:, ::2].any()


def _within_ulps(got, want64, ulps):
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)).astype(np.float64)).all()


@pytest.mark.parametrize("case", [("2", 3), ("R+1", 48), ("2R+3", 32)], ids=["N=2_C=3", "N=R+1_C=48", "N=2R+3_C=32"])
def test_running_statistics_after_two_calls(case):
    """running_mean, running_var (unbiased) and num_batches_tracked after two consecutive training calls through the
    autograd function, against the restatement chained through its own fp32 roundings, within 2 ulp."""
    from imfnet_amd.autograd import SparseBatchNormFunction
    n, c = _rows(case[0]), case[1]
    g = torch.Generator().manual_seed(11 + n + c)
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=0.05).to(DEV).train()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g))
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    rm, rv = _np(bn.running_mean), _np(bn.running_var)
    for call in range(2):
        x = torch.randn(n, c, generator=g) * (1.0 + call) + 3.0
        y = SparseBatchNormFunction.apply(x.to(DEV).requires_grad_(True), bn.weight, bn.bias, None, bn, call == 1)
        assert y.requires_grad
        fw = NR.forward(x.numpy(), _np(bn.weight), _np(bn.bias), EPS, None, call == 1, rm, rv, 0.05)
        assert _within_ulps(_np(bn.running_mean), fw["running_mean"], 2)
        assert _within_ulps(_np(bn.running_var), fw["running_var"], 2)
        rm, rv = _np(bn.running_mean), _np(bn.running_var)          # chain through the stored fp32 values
    assert int(bn.num_batches_tracked) == 2
    # untracked statistics and eval-mode buffers do not move
    bn2 = torch.nn.BatchNorm1d(c, eps=EPS, momentum=0.05, track_running_stats=False).to(DEV).train()
    y = SparseBatchNormFunction.apply(x.to(DEV), bn2.weight, bn2.bias, None, bn2, False)
    assert bn2.running_mean is None and y.shape == (n, c)
    from imfnet_amd._lib import ImfError
    bn3 = torch.nn.BatchNorm1d(c, momentum=None).to(DEV).train()
    with pytest.raises(ImfError):
        SparseBatchNormFunction.apply(x.to(DEV), bn3.weight, bn3.bias, None, bn3, False)
    assert int(bn3.num_batches_tracked) == 0


def test_two_calls_give_the_same_bits():
    from imfnet_amd import ops
    n, c = _rows("2R+3"), 64
    g = torch.Generator().manual_seed(21)
    x, res, dy = (torch.randn(n, c, generator=g).to(DEV) for _ in range(3))
    gamma, beta = (t.to(DEV) for t in _affine(g, c))
    runs = []
    for _ in range(2):
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        y, stats = ops.bn_train_forward(x, gamma, beta, EPS, res, True, rm, rv, 0.1)
        runs.append((y, stats, rm, rv) + ops.bn_train_backward(dy, x, y, stats, gamma, True, want_dresidual=True))
    for a, b in zip(*runs):
        assert not torch.isnan(a).any() and torch.equal(a, b)


def test_outputs_that_are_not_wanted_are_not_produced():
    from imfnet_amd import ops
    n, c = _rows("R+1"), 32
    g = torch.Generator().manual_seed(22)
    x, dy = torch.randn(n, c, generator=g).to(DEV), torch.randn(n, c, generator=g).to(DEV)
    gamma, beta = (t.to(DEV) for t in _affine(g, c))
    y, stats = ops.bn_train_forward(x, gamma, beta, EPS, None, True)
    full = ops.bn_train_backward(dy, x, y, stats, gamma, True, want_dresidual=True)
    for mask in ((True, False, False, False), (False, True, True, False), (False, False, False, True), (True, True, False, True)):
        part = ops.bn_train_backward(dy, x, y, stats, gamma, True, *mask)
        for want, got, ref in zip(mask, part, full):
            assert (got is None) != want
            if want:
                assert torch.equal(got, ref)


def _raw_forward(n, c, ws_delta=0, n_arg=None):
    """The C call with NaN-filled outputs: (rc, y, stats, workspace)."""
    from imfnet_amd import _lib
    L = _lib.lib()
    x = torch.randn(max(n, 2), c, device=DEV)
    gamma, beta = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    y = torch.full_like(x, NAN)
    stats = torch.full((2 * c,), NAN, dtype=torch.float64, device=DEV)
    nbytes = L.imf_bn_train_workspace_bytes(max(n, 2), c)
    ws = torch.full((nbytes // 8 + 1,), NAN, dtype=torch.float64, device=DEV)
    rc = L.imf_bn_train_forward(x.data_ptr(), n if n_arg is None else n_arg, c, gamma.data_ptr(), beta.data_ptr(), EPS, None,
                                0, None, None, 0.1, y.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes + ws_delta,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, y, stats, ws


@pytest.mark.parametrize("what", ["n_one", "n_zero", "workspace_one_byte_short"])
def test_bad_arguments_return_a_status_and_launch_nothing(what):
    from imfnet_amd import _lib, ops
    kw = {"n_one": dict(n_arg=1), "n_zero": dict(n_arg=0), "workspace_one_byte_short": dict(ws_delta=-1)}[what]
    rc, y, stats, ws = _raw_forward(5, 8, **kw)
    assert rc == EINVAL
    assert torch.isnan(y).all() and torch.isnan(stats).all() and torch.isnan(ws).all()     # nothing was launched
    rc, y, stats, _ = _raw_forward(5, 8)                            # the same arguments, unbroken, are accepted
    assert rc == 0 and not torch.isnan(y).any() and not torch.isnan(stats).any()
    gamma, beta = torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    if what != "workspace_one_byte_short":                          # ... and through the wrapper
        rows = 1 if what == "n_one" else 0
        with pytest.raises(_lib.ImfError):
            ops.bn_train_forward(torch.randn(rows, 8, device=DEV), gamma, beta, EPS)
        with pytest.raises(_lib.ImfError):
            ops.bn_train_backward(torch.randn(rows, 8, device=DEV), torch.randn(rows, 8, device=DEV), None,
                                  torch.ones(16, dtype=torch.float64, device=DEV), gamma)


def test_wrong_dtype_or_device_is_refused_by_the_wrapper():
    from imfnet_amd import _lib, ops
    x = torch.randn(5, 8, device=DEV)
    gamma, beta = torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    y, stats = ops.bn_train_forward(x, gamma, beta, EPS)
    bad_calls = [
        lambda: ops.bn_train_forward(x.double(), gamma, beta, EPS),
        lambda: ops.bn_train_forward(x.cpu(), gamma, beta, EPS),
        lambda: ops.bn_train_forward(x, gamma.half(), beta, EPS),
        lambda: ops.bn_train_forward(x, gamma, beta.cpu(), EPS),
        lambda: ops.bn_train_forward(x, gamma, beta, EPS, residual=x[:4]),
        lambda: ops.bn_train_forward(x.t(), gamma[:5], beta[:5], EPS),
        lambda: ops.bn_train_backward(x, x, y, stats.float(), gamma),
        lambda: ops.bn_train_backward(x.cpu(), x, y, stats, gamma),
        lambda: ops.bn_train_backward(x, x, None, stats, gamma, relu=True),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(_lib.ImfError):
            call()
        assert k >= 0


# ======================================================================================================================
# module level: the residual block
# ======================================================================================================================
@contextlib.contextmanager
def _switch(name):
    from imfnet_amd import ops
    prev = ops.set_train_norm(name)
    try:
        yield
    finally:
        ops.set_train_norm(prev)


@pytest.fixture(scope="module")
def geo(clouds):
    """The batched geometry the backward tests build (test_gpu_backward_exact._Batch): the tensor as the trainer makes
    it, beside the oracle's maps of the same rows."""
    import test_gpu_backward_exact as BX
    return BX._Batch([clouds[0][::8], clouds[1][::8]], 0.05)


@pytest.fixture(scope="module")
def block_case(geo):
    """A BasicBlockBN(32, 32) at tensor stride 2 with random weights, its input, the gradient fed back, and the float64
    restatement of the block (convolutions over the oracle's map, norms by tests/norm_restate.py)."""
    import backward_restate as R
    from imfnet_amd.model.layers import BasicBlockBN
    torch.manual_seed(31)
    blk = BasicBlockBN(32, 32, bn_momentum=0.05).to(DEV).train()
    with torch.no_grad():
        for nm in (blk.norm1, blk.norm2):
            nm.bn.weight.uniform_(0.5, 1.5)
            nm.bn.bias.uniform_(-0.5, 0.5)
    nbr = geo.geo.k3[1]
    n = len(geo.geo.levels[1])
    g = torch.Generator().manual_seed(32)
    x, dout = torch.randn(n, 32, generator=g), torch.randn(n, 32, generator=g)
    W1, W2 = blk.conv1.kernel.detach().cpu(), blk.conv2.kernel.detach().cpu()
    p = {k: _np(v) for k, v in (("g1", blk.norm1.bn.weight), ("b1", blk.norm1.bn.bias), ("g2", blk.norm2.bn.weight),
                                ("b2", blk.norm2.bn.bias))}
    c1 = R.conv_restate(x, W1, None, nbr)
    f1 = NR.forward(c1.numpy(), p["g1"], p["b1"], EPS, None, True)
    c2 = R.conv_restate(f1["y"], W2, None, nbr)
    f2 = NR.forward(c2.numpy(), p["g2"], p["b2"], EPS, x.numpy(), True)
    b2 = NR.backward(dout.numpy(), c2.numpy(), f2["y"], p["g2"], EPS, True)
    _, da, dW2 = R.conv_restate(f1["y"], W2, b2["dx"], nbr)
    b1 = NR.backward(da.numpy(), c1.numpy(), f1["y"], p["g1"], EPS, True)
    _, dx, dW1 = R.conv_restate(x, W1, b1["dx"], nbr)
    ref = {"out": f2["y"], "x": dx.numpy() + b2["dresidual"], "conv1.kernel": dW1.numpy(), "conv2.kernel": dW2.numpy(),
           "norm1.bn.weight": b1["dgamma"], "norm1.bn.bias": b1["dbeta"], "norm2.bn.weight": b2["dgamma"],
           "norm2.bn.bias": b2["dbeta"]}
    return blk, x, dout, ref


def _run_block(blk, geo, x, dout, forward=None):
    from imfnet_amd import sparse as ME
    blk = copy.deepcopy(blk)
    xin = x.to(DEV).requires_grad_(True)
    st = ME.SparseTensor(xin, coordinate_map_key=ME.CoordinateMapKey(2), coordinate_manager=geo.st.coordinate_manager)
    out = (blk if forward is None else forward(blk))(st).F
    out.backward(dout.to(DEV))
    got = {"out": out.detach(), "x": xin.grad}
    got.update({k: v.grad for k, v in blk.named_parameters()})
    got.update({"buf." + k: v.detach().clone() for k, v in blk.named_buffers()})
    return got


@pytest.mark.parametrize("switch", ["torch", "hip"])
def test_residual_block_matches_its_float64_restatement(geo, block_case, switch):
    """Each side against the float64 restatement of the block, not against each other.  The tolerance is the rule the
    whole-network gradient test applies to fp32 training gradients (test_gpu_backward_exact: REL_TOL * scale + ABS_TOL
    per tensor): propagating the per-element counted bounds through two 27-offset convolutions is not practical."""
    import test_gpu_backward_exact as BX
    blk, x, dout, ref = block_case
    with _switch(switch):
        got = _run_block(blk, geo, x, dout)
    for key, want in ref.items():
        scale = float(np.abs(want).max())
        err = float(np.abs(_np(got[key]).astype(np.float64).reshape(want.shape) - want).max())
        tol = BX.REL_TOL * scale + BX.ABS_TOL
        print(f"{switch} {key}: scale {scale:.3e} err {err:.3e} err/tol {err / tol:.4f}")
        assert err < tol, (key, err, tol)
    assert int(got["buf.norm1.bn.num_batches_tracked"]) == 1 and int(got["buf.norm2.bn.num_batches_tracked"]) == 1
    assert got["buf.norm1.bn.running_mean"].abs().max() > 0


def test_residual_block_with_the_switch_at_torch_is_the_op_sequence_it_always_was(geo, block_case):
    from imfnet_amd import sparse as ME

    def parent_forward(blk):
        def run(x):
            relu = ME.MinkowskiFunctional.relu
            y = relu(x._like(blk.norm1.bn(blk.conv1(x).F)))
            y = x._like(blk.norm2.bn(blk.conv2(y).F))
            y += x
            return relu(y)
        return run

    blk, x, dout, _ = block_case
    with _switch("torch"):
        a = _run_block(blk, geo, x, dout)
    b = _run_block(blk, geo, x, dout, forward=parent_forward)
    assert set(a) == set(b)
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_hip_switch_is_used_only_where_it_applies(geo, block_case):
    """eval mode and no_grad run the torch ops whatever the switch: the same bits as with the switch at torch."""
    from imfnet_amd import sparse as ME
    blk, x, _, _ = block_case
    nm = copy.deepcopy(blk.norm1)
    st = ME.SparseTensor(x.to(DEV), coordinate_map_key=ME.CoordinateMapKey(2), coordinate_manager=geo.st.coordinate_manager)
    outs = {}
    for switch in ("torch", "hip"):
        with _switch(switch):
            m = copy.deepcopy(nm).train()
            with torch.no_grad():
                a = m.forward_fused(st, residual=st, relu=True).F
            b = m.eval().forward_fused(st, relu=True).F
            outs[switch] = (a, b, m.bn.running_mean.clone())
    for u, v in zip(outs["torch"], outs["hip"]):
        assert torch.equal(u, v)


# ======================================================================================================================
# whole network
# ======================================================================================================================
def test_whole_network_gradients_with_the_hip_norms_stay_within_the_oracle_rule(clouds, images, seeded_sd):
    """The train_single case of test_gpu_backward_exact with the switch at "hip": descriptors within 1e-4 of the oracle,
    every parameter gradient within that file's rule max(REL_TOL * scale + ABS_TOL, ORDER_FACTOR * yard), yard from the
    oracle's fp32-against-float64 run.  The worst err / tol is printed beside the torch switch's on the same case."""
    import backward_restate as R
    import test_gpu_backward_exact as BX
    from imfnet_amd.train.trainer import _sparse_input
    point_sets, imgs = BX.whole_network_case(clouds, images, "single")
    reps, coords = R.batched_voxels(point_sets, 0.05)
    T = torch.randn((len(coords), 32), generator=torch.Generator().manual_seed(9))
    F_ref, ref = BX.oracle_gradients(seeded_sd, coords, imgs, T, bn_training=True)
    _, ref64 = BX.oracle_gradients(seeded_sd, coords, imgs, T, bn_training=True, double=True)
    yard = {k: float((ref[k].double() - r64).abs().max()) for k, r64 in ref64.items()}
    worst = {}
    for switch in ("torch", "hip"):
        with _switch(switch):
            m = BX._new_model(seeded_sd).train()
            st = _sparse_input([torch.as_tensor(r).to(DEV) for r in reps], None, 0.05, torch.device(DEV))
            assert np.array_equal(st.C.cpu().numpy(), coords)
            Fg = m(st, torch.as_tensor(imgs).to(DEV)).F
            (Fg * T.to(DEV)).sum().backward()
        err_f = float((Fg.detach().cpu() - F_ref).abs().max())
        grads = dict(m.named_parameters())
        w, late, checked = (0.0, None), [], 0
        for k, r in ref.items():
            scale = float(r.abs().max())
            if scale < 1e-7:
                continue
            err = float((grads[k].grad.cpu() - r).abs().max())
            tol = max(BX.REL_TOL * scale + BX.ABS_TOL, BX.ORDER_FACTOR * yard.get(k, 0.0))
            w = max(w, (err / tol, k))
            checked += 1
            if not err < tol:
                late.append((k, err, tol))
        worst[switch] = (w, err_f, late, checked)
        print(f"norm kernels {switch}: max|F - oracle| = {err_f:.2e}, {checked} parameters, worst err / tol = {w[0]:.3f} ({w[1]})")
    (w, err_f, late, checked) = worst["hip"]
    assert err_f < 1e-4
    assert not late, late
    assert checked > 100
    assert int(m.norm3.bn.num_batches_tracked) == 1
