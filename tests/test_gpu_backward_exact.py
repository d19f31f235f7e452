"""The sparse-convolution backward, exactly, on the maps training really uses (csrc/backward.hip, imfnet_amd/autograd.py).

a. imf_spconv_wgrad at the C ABI on synthetic maps: integer data (tests/backward_restate.py), so the comparison with the
   float64 restatement is torch.equal; channel counts off the 32-wide block, slot counts on and around the 4096-slot chunk
   and the 64-row stage, padding, permuted slots, empty offsets, the kvol == 1 NULL / NULL branch; bit-reproducibility and
   the any-order summation bound on Gaussian data; the argument checks.
b. every convolution layer of the network (enumerated from the model) on the batched tensor trainer._sparse_input
   builds: forward, weight gradient and input gradient against the restatement over the oracle's map, torch.equal.
c. b under each arithmetic (ops.CONV_VARIANT 3, 0, 6) at unit scale and with power-of-two scales that leave f16's range.
d. whole-network gradients on a batch of two fragments, and with training-mode BatchNorm, against the oracle."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import backward_restate as R
import imf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CHUNK, STAGE = 4096, 64                       # csrc/backward.hip: slots per workgroup, rows staged per step
EINVAL = -1


# ======================================================================================================================
# a. imf_spconv_wgrad at the C ABI
# ======================================================================================================================
def _call_wgrad(feat, grad, tile_rows, nbr, n_slots, n_out, kvol, cin=None, cout=None, ws_bytes_delta=0):
    """(return code, dW, workspace) with dW and the workspace filled with NaN before the call."""
    from imfnet_amd import _lib
    L = _lib.lib()
    cin_a, cout_a = feat.shape[1] if cin is None else cin, grad.shape[1] if cout is None else cout
    dw = torch.full((kvol, feat.shape[1], grad.shape[1]), NAN, dtype=torch.float32, device=DEV)
    nbytes = L.imf_spconv_wgrad_workspace_bytes(max(n_slots, 1), kvol, feat.shape[1], grad.shape[1])
    assert nbytes < 1 << 30
    ws = torch.full((nbytes // 4 + 1,), NAN, dtype=torch.float32, device=DEV)
    rc = L.imf_spconv_wgrad(feat.data_ptr(), cin_a, grad.data_ptr(), cout_a,
                            None if tile_rows is None else tile_rows.data_ptr(), None if nbr is None else nbr.data_ptr(),
                            n_slots, n_out, kvol, dw.data_ptr(), ws.data_ptr(), nbytes + ws_bytes_delta,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, dw, ws


class _Map:
    """One synthetic case: the map in both shapes, on the host and on the GPU."""

    def __init__(self, seed, n_out, kvol, mode="map", n_in=None, n_slots=None, permute=False, empty=(), density=0.3):
        self.gen = torch.Generator().manual_seed(seed)
        self.n_out, self.kvol = n_out, kvol
        if mode == "null":                                # kvol == 1, nbr == NULL, tile_rows == NULL: slot == row == input
            assert kvol == 1
            self.n_in, self.rows, self.tile_rows, self.nbr = n_out, None, None, None
            self.n_slots = (n_out + STAGE - 1) // STAGE * STAGE if n_slots is None else n_slots
        else:
            self.n_in = n_in if n_in is not None else max(1, n_out // 2 + 7)
            self.rows, tr, tiled = R.synthetic_map(self.gen, n_out, self.n_in, kvol, n_slots=n_slots, density=density,
                                                   permute=permute, empty_offsets=empty)
            self.n_slots = len(tr)
            self.tile_rows = torch.as_tensor(tr).to(DEV)
            self.nbr = torch.as_tensor(tiled).contiguous().to(DEV)
        self.chunks = (self.n_slots + CHUNK - 1) // CHUNK

    def wgrad(self, feat, grad, **kw):
        return _call_wgrad(feat.to(DEV).contiguous(), grad.to(DEV).contiguous(), self.tile_rows, self.nbr, self.n_slots,
                           self.n_out, self.kvol, **kw)


# (id, n_out, cin, cout, kvol, keyword arguments of _Map).  Channels: both ragged / one ragged / neither (32-wide blocks).
WGRAD_CASES = [
    ("n1_3x31", 1, 3, 31, 27, {}),
    ("n63_31x33", 63, 31, 33, 27, {}),
    ("n64_32x32", 64, 32, 32, 27, {}),
    ("n65_33x1", 65, 33, 1, 27, {}),
    ("n4095_4x64", 4095, 4, 64, 27, {}),
    ("n4096_64x32", 4096, 64, 32, 27, {}),
    ("n4097_96x31", 4097, 96, 31, 27, {}),
    ("n4097_256x256", 4097, 256, 256, 27, {}),
    ("n8193_32x33_permuted", 8193, 32, 33, 27, dict(permute=True)),
    ("n40000_64x64_permuted_padded", 40000, 64, 64, 27, dict(permute=True, n_slots=10 * CHUNK, density=0.5)),
    ("n4097_31x31_empty_offsets", 4097, 31, 31, 27, dict(empty=(0, 13, 26))),
    ("n4000_of_4096_slots_32x64", 4000, 32, 64, 27, dict(n_slots=CHUNK)),
    ("n5000_of_8192_slots_permuted_64x33", 5000, 64, 33, 27, dict(n_slots=2 * CHUNK, permute=True)),
    ("n100_of_4160_slots_padding_chunk", 100, 32, 32, 27, dict(n_slots=CHUNK + STAGE)),      # second chunk: padding only
    ("k1_null_n4096_256x32", 4096, 256, 32, 1, dict(mode="null")),
    ("k1_null_n8193_96x64", 8193, 96, 64, 1, dict(mode="null")),
    ("k1_null_n40000_33x31", 40000, 33, 31, 1, dict(mode="null")),
    ("k1_null_n5000_of_8192_slots_64x32", 5000, 64, 32, 1, dict(mode="null", n_slots=2 * CHUNK)),
    ("k1_map_n4097_1x256_permuted", 4097, 1, 256, 1, dict(permute=True, density=0.7)),
    ("k1_map_n63_3x1", 63, 3, 1, 1, {}),
    ("k125_n4097_1x32", 4097, 1, 32, 125, {}),
    ("k125_n65_3x33_empty", 65, 3, 33, 125, dict(empty=(0, 62, 124), density=0.1)),
    ("k125_n8193_4x32_permuted", 8193, 4, 32, 125, dict(permute=True, density=0.2)),
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad_is_exact_on_integer_data(case):
    name, n_out, cin, cout, kvol, kw = case
    m = _Map(1000 + WGRAD_CASES.index(case), n_out, kvol, **kw)
    feat, _, grad = R.int_case(m.gen, m.n_in, n_out, kvol, cin, cout)
    assert max(R.magnitude_bounds(m.rows, m.n_in, cin, cout)) < R.EXACT_LIMIT
    _, _, want = R.conv_restate(feat, torch.zeros(kvol, cin, cout), grad, m.rows, n_in=m.n_in)
    rc, dw, _ = m.wgrad(feat, grad)
    assert rc == 0
    got = dw.cpu()
    assert not torch.isnan(got).any(), f"{int(torch.isnan(got).sum())} elements of dW were never written"
    bad = (got.double() != want)
    assert not bad.any(), (f"{int(bad.sum())} of {bad.numel()} elements differ; offsets "
                           f"{sorted(set(torch.nonzero(bad)[:, 0].tolist()))[:8]}, chunks {m.chunks}")
    assert torch.equal(got.double(), want)
    for k in kw.get("empty", ()):
        assert not got[k].any()
    if kvol > 1 or kw.get("mode") == "null":
        assert float(want.abs().max()) > 0


# Gaussian data: (id, n_out, cin, cout, kvol, _Map keywords).  The first case has ~60 pairs per offset: its bound is
# ~4e-6 * S, while operands rounded to f16 (2^-11 each) or bf16 (2^-8) would leave ~6e-5 * S or more: a silent move of the
# weight gradient to 16-bit operands breaks it.  The bound grows with the pair count; on the large cases it only catches
# gross loss of precision.
FLOAT_CASES = [
    ("n200_64x33_tight", 200, 64, 33, 27, {}),
    ("n1500_33x64_permuted", 1500, 33, 64, 27, dict(permute=True)),
    ("n8193_32x32_permuted", 8193, 32, 32, 27, dict(permute=True)),
    ("n40000_64x64_padded", 40000, 64, 64, 27, dict(n_slots=10 * CHUNK)),
    ("k1_null_n8193_96x64", 8193, 96, 64, 1, dict(mode="null")),
    ("k125_n4097_1x32", 4097, 1, 32, 125, {}),
]


@pytest.mark.parametrize("case", FLOAT_CASES, ids=[c[0] for c in FLOAT_CASES])
def test_wgrad_on_float_data_is_reproducible_and_within_the_summation_bound(case):
    """|dW - dW_f64| <= g / (1 - g) * S per element, g = (n_k + n_chunks) * 2^-24, S = sum of |in| * |grad| over the
    element's pairs: one rounding per product and one per addition (n_k - 1 in the chunks, n_chunks in the reduction), in
    any order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  Derived, not measured."""
    name, n_out, cin, cout, kvol, kw = case
    m = _Map(2000 + FLOAT_CASES.index(case), n_out, kvol, **kw)
    feat = torch.randn(m.n_in, cin, generator=m.gen)
    grad = torch.randn(n_out, cout, generator=m.gen)
    rc, dw, _ = m.wgrad(feat, grad)
    rc2, dw2, _ = m.wgrad(feat, grad)
    assert rc == 0 and rc2 == 0
    assert not torch.isnan(dw).any()
    assert torch.equal(dw, dw2)                                     # the weight gradient is bit-reproducible
    _, _, want = R.conv_restate(feat, torch.zeros(kvol, cin, cout), grad, m.rows, n_in=m.n_in)
    S, n_k = R.wgrad_abs_sum(feat, grad, m.rows)
    g = (torch.as_tensor(n_k, dtype=torch.float64) + m.chunks) * 2.0 ** -24
    bound = (g / (1 - g)).reshape(-1, 1, 1) * S
    err = (dw.cpu().double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: pairs per offset <= {int(n_k.max())}, chunks {m.chunks}, max err / bound = {worst:.3f}, "
          f"max err / S = {float((err / S.clamp_min(1e-300)).max()):.2e}")
    assert (err <= bound).all(), worst
    if name.endswith("tight"):
        assert int(n_k.max()) <= 512


REJECTIONS = ["workspace_one_byte_short", "nbr_null_kvol27", "cin_zero", "n_slots_zero"]


@pytest.mark.parametrize("what", REJECTIONS)
def test_wgrad_rejects_bad_arguments_before_any_launch(what):
    m = _Map(7, 300, 27)
    feat, _, grad = R.int_case(m.gen, m.n_in, 300, 27, 32, 32)
    f, g = feat.to(DEV), grad.to(DEV)
    args = dict(tile_rows=m.tile_rows, nbr=m.nbr, n_slots=m.n_slots, n_out=m.n_out, kvol=27)
    kw = {}
    if what == "workspace_one_byte_short":
        kw["ws_bytes_delta"] = -1
    elif what == "nbr_null_kvol27":
        args["nbr"] = None
    elif what == "cin_zero":
        kw["cin"] = 0
    else:
        args["n_slots"] = 0
    rc, dw, ws = _call_wgrad(f, g, args["tile_rows"], args["nbr"], args["n_slots"], args["n_out"], args["kvol"], **kw)
    assert rc == EINVAL
    assert torch.isnan(dw).all() and torch.isnan(ws).all()          # nothing was launched
    rc, dw, _ = m.wgrad(feat, grad)                                 # the same arguments, unbroken, are accepted
    assert rc == 0 and not torch.isnan(dw).any()


# ======================================================================================================================
# b / c. every convolution layer of the network on training's own maps
# ======================================================================================================================
def _new_model(seeded_sd=None):
    from imfnet_amd.model import load_model
    m = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3, config=None)
    if seeded_sd is not None:
        m.load_state_dict(seeded_sd, strict=True)
    return m.to(DEV)


class _Batch:
    """The tensor of one training batch, built as the trainer builds it, beside the oracle's geometry of the same rows."""

    def __init__(self, point_sets, voxel):
        from imfnet_amd.train.trainer import _sparse_input
        self.reps, self.coords = R.batched_voxels(point_sets, voxel)
        self.voxel = voxel
        self.st = _sparse_input([torch.as_tensor(r).to(DEV) for r in self.reps], None, voxel, torch.device(DEV))
        assert np.array_equal(self.st.C.cpu().numpy(), self.coords)            # row for row
        self.geo = O.Geometry(self.coords)
        cm = self.st.coordinate_manager
        for lv in range(4):
            assert np.array_equal(cm.coords(1 << lv).cpu().numpy(), self.geo.levels[lv]), lv
        self.expected = {}                                                      # signature -> unit-scale restatement

    def tensor(self):
        from imfnet_amd.train.trainer import _sparse_input
        return _sparse_input([torch.as_tensor(r).to(DEV) for r in self.reps], None, self.voxel, torch.device(DEV))


@pytest.fixture(scope="module")
def batch2(clouds):
    b = _Batch([clouds[0], clouds[1]], 0.05)
    assert set(b.coords[:, 0].tolist()) == {0, 1}
    return b


@pytest.fixture(scope="module")
def single25(clouds):
    b = _Batch([clouds[0]], 0.025)
    assert len(b.coords) > 3 * CHUNK                     # the level-0 weight gradient spans at least four chunks
    return b


@pytest.fixture(scope="module")
def layers(batch2, images):
    """{signature: module} of EVERY _ConvBase of the model, signature = (transposed, kernel_size, stride, tensor stride
    of the input, cin, cout); the tensor strides are observed in one forward of the model itself."""
    from imfnet_amd import sparse as ME
    model = _new_model().train()
    seen, hooks = {}, []
    convs = [(n, m) for n, m in model.named_modules() if isinstance(m, ME._ConvBase)]
    def note(name):
        def hook(mod_, args):                                       # returns None: the input goes on unchanged
            seen.setdefault(name, args[0].coordinate_map_key.tensor_stride)
        return hook

    for name, mod in convs:
        hooks.append(mod.register_forward_pre_hook(note(name)))
    img = torch.as_tensor(np.concatenate([images[0], images[1]])).to(DEV)
    with torch.no_grad():
        model(batch2.tensor(), img)
    for h in hooks:
        h.remove()
    assert sorted(seen) == sorted(n for n, _ in convs)              # every convolution of the model ran
    out = {}
    for name, mod in convs:
        sig = (bool(mod._transposed), mod.kernel_size, mod.stride, seen[name], mod.in_channels, mod.out_channels)
        out.setdefault(sig, (name, mod))
    assert len(convs) == sum(k.endswith(".kernel") for k in model.state_dict()) and len(out) >= 12
    return out


@contextlib.contextmanager
def _variant(v):
    from imfnet_amd import ops
    prev = ops.CONV_VARIANT
    ops.CONV_VARIANT = v
    try:
        yield
    finally:
        ops.CONV_VARIANT = prev


def _expected(batch, sig):
    """Unit-scale integer operands of one layer and their float64 restatement over the oracle's map (cached)."""
    if sig not in batch.expected:
        tr, ks, st, ts, cin, cout = sig
        nbr, kind, lv, n_in, n_out = R.layer_map(batch.geo, tr, ks, st, ts)
        gen = torch.Generator().manual_seed(sum(int(v) * p for v, p in zip(sig, (7, 11, 13, 17, 19, 23))))
        feat, W, g = R.int_case(gen, n_in, n_out, ks ** 3, cin, cout)
        assert max(R.magnitude_bounds(nbr, n_in, cin, cout)) < R.EXACT_LIMIT
        out, dX, dW = R.conv_restate(feat, W, g, nbr)
        a, b, c = R.inner_products(feat, W, g, out, dX, dW)
        assert a == b == c
        batch.expected[sig] = (feat, W, g, out, dX, dW)
    return batch.expected[sig]


def _run_layer(batch, sig, mod, s_feat=1.0, s_grad=1.0):
    """One layer under autograd on the GPU with integer operands times exact powers of two.  Returns the list of what
    differs from the restatement (empty: all equal)."""
    from imfnet_amd import sparse as ME
    from imfnet_amd._lib import ImfError
    tr, ks, st, ts, cin, cout = sig
    feat, W, g, out64, dX64, dW64 = _expected(batch, sig)
    mod = copy.deepcopy(mod)
    with torch.no_grad():
        mod.kernel.copy_(W.reshape(mod.kernel.shape).to(DEV))
        if mod.bias is not None:
            mod.bias.zero_()                                       # torch adds it after the convolution: + 0 is exact
    cm = batch.st.coordinate_manager
    problems = []

    def forward(requires_grad):
        mod.zero_grad()
        f = (feat * s_feat).to(DEV).requires_grad_(requires_grad)
        x = ME.SparseTensor(f, coordinate_map_key=ME.CoordinateMapKey(ts), coordinate_manager=cm)
        y = mod(x)
        assert y.coordinate_map_key.tensor_stride == (ts // st if tr else ts * st)
        return f, y.F

    want_dx = cin != 1                                              # conv1: its input features never require grad
    if not want_dx:
        f, y = forward(True)
        with pytest.raises(ImfError):
            y.backward((g * s_grad).to(DEV))
    f, y = forward(want_dx)
    y.backward((g * s_grad).to(DEV))
    got = {"out": y.detach().cpu(), "dW": mod.kernel.grad.detach().cpu().reshape(dW64.shape)}
    exact = {"out": out64 * s_feat, "dW": dW64 * (s_feat * s_grad)}
    if want_dx:
        got["dX"], exact["dX"] = f.grad.detach().cpu(), dX64 * s_grad
    for key, e in exact.items():
        want = e.float()
        assert torch.equal(want.double(), e)                        # a power-of-two scale of an integer: exact in float32
        if got[key].shape != want.shape or not torch.equal(got[key], want):
            bad = int((got[key] != want).sum()) if got[key].shape == want.shape else -1
            problems.append(f"{key}: {bad} of {want.numel()} elements differ")
    if s_feat == 1.0 and s_grad == 1.0 and not problems:            # the GPU's own results, as integers
        dx = got["dX"] if want_dx else dX64
        a, b, c = R.inner_products(feat, W, g, got["out"], dx, got["dW"])
        if not (a == b == c):
            problems.append(f"inner products {a} {b} {c}")
    return problems


def _walk(batch, layers, **scales):
    failures, covered = {}, 0
    for sig, (name, mod) in layers.items():
        p = _run_layer(batch, sig, mod, **scales)
        covered += 1
        if p:
            failures[f"{name} {sig}"] = p
    assert covered == len(layers)                                   # no layer skipped
    assert not failures, failures


def test_every_conv_layer_is_exact_on_the_trainers_batched_maps(batch2, layers):
    _walk(batch2, layers)


def test_every_conv_layer_is_exact_on_a_single_fragment_at_2_5_cm(single25, layers):
    """15-19 k voxels at level 0: the weight gradient of the level-0 layers sums four or more chunks."""
    _walk(single25, layers)


def test_occupancy_sorted_twin_gives_the_same_weight_gradient(batch2):
    from imfnet_amd import ops
    from imfnet_amd.autograd import spconv_wgrad
    cm = batch2.st.coordinate_manager
    for ts, cin, cout in ((1, 32, 33), (2, 64, 64)):
        lv = ts.bit_length() - 1
        rb = cm.conv_rulebook(ts, 3, 1)
        rbs = ops.rulebook_sorted(rb)
        assert not torch.equal(rb.tile_rows, rbs.tile_rows)         # the twin really is in another slot order
        n = len(batch2.geo.levels[lv])
        rows = R.tiled_to_rows(rbs.tile_rows.cpu().numpy(), rbs.nbr.view(27, -1).cpu().numpy(), n)
        assert np.array_equal(rows, batch2.geo.k3[lv])
        feat, _, g = R.int_case(torch.Generator().manual_seed(3 + ts), n, n, 27, cin, cout)
        _, _, want = R.conv_restate(feat, torch.zeros(27, cin, cout), g, batch2.geo.k3[lv])
        a = spconv_wgrad(feat.to(DEV), g.to(DEV), rb, 27)
        b = spconv_wgrad(feat.to(DEV), g.to(DEV), rbs, 27)
        assert torch.equal(a, b) and torch.equal(a.cpu().double(), want)


# unit scale; gradients below f16's smallest subnormal (3 * 2^-30 < 2^-24) with features at 2^-10; gradients beyond f16's
# largest number (2^20 > 65504)
SCALES = {"unit": (1.0, 1.0), "small": (2.0 ** -10, 2.0 ** -30), "large": (1.0, 2.0 ** 20)}


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("variant", [3, 0, 6])
def test_every_conv_layer_is_exact_under_each_arithmetic(batch2, layers, variant, scale, request):
    """Training must be right under every process-wide arithmetic.  Variant 6 (split f16) cannot carry gradients of
    1e-9 or activations of 1e6: SparseConvFunction runs its forward and its input gradient on bf16x3 (variant 3) when
    the process variant is 6, which is what makes the scaled cases pass there."""
    from imfnet_amd import ops
    s_feat, s_grad = SCALES[scale]
    if variant == 6:
        request.getfixturevalue("fast_mode")
        assert ops.CONV_VARIANT == 6
        _walk(batch2, layers, s_feat=s_feat, s_grad=s_grad)
    else:
        with _variant(variant):
            _walk(batch2, layers, s_feat=s_feat, s_grad=s_grad)


# ======================================================================================================================
# d. whole-network gradients: batched, and with training-mode BatchNorm
# ======================================================================================================================
# Per parameter: |grad - oracle| < REL_TOL * max|oracle grad| + ABS_TOL, the bound of tests/test_gpu_backward.py.  With
# training-mode BatchNorm that is tighter than the oracle itself: its fp32 run differs from its own float64 run (spconv_f64,
# .double() weights, same loss) by up to 4e-2 of a parameter's scale on the single fragment and 3.4e-2 on the batch of two
# (LAB_NOTES has the figures; eval mode: 2e-6).  There the bound of a parameter is the larger of the constant and
# ORDER_FACTOR times that parameter's measured fp32-against-float64 deviation of the ORACLE (never of the GPU result): the
# GPU sums in another order than the fp32 oracle.
REL_TOL, ABS_TOL, ORDER_FACTOR = 2e-3, 1e-6, 4.0


def oracle_gradients(seeded_sd, coords, imgs, T, bn_training, double=False):
    """(F, {name: gradient}) of loss = <F, T> through the oracle; double: the float64 run of the same oracle (spconv_f64,
    .double() weights), the yardstick the fp32 oracle's own error is measured against."""
    dt = torch.float64 if double else torch.float32
    sd = {k: (v.detach().to(dt).clone().requires_grad_(True) if v.is_floating_point() and "running" not in k
              else (v.detach().to(dt).clone() if v.is_floating_point() else v.clone())) for k, v in seeded_sd.items()}
    prev = O.spconv
    if double:
        O.spconv = O.spconv_f64
    try:
        F_ref = O.resunet_forward(sd, coords, imgs, bn_training=bn_training)
    finally:
        O.spconv = prev
    assert F_ref.dtype == dt
    (F_ref * T.to(dt)).sum().backward()
    return F_ref.detach(), {k: v.grad for k, v in sd.items() if getattr(v, "requires_grad", False) and v.grad is not None}


def whole_network_case(clouds, images, which):
    """(point sets, images [B, 3, H, W]) of the two geometries of part d."""
    if which == "single":
        return [clouds[1][::6]], images[1]
    return [clouds[0][::4], clouds[1][::4]], np.concatenate([images[0], images[1]])


@pytest.mark.parametrize("which,train", [("batch", False), ("single", True), ("batch", True)],
                         ids=["eval_batch_of_two", "train_single", "train_batch_of_two"])
def test_whole_network_gradients_match_the_oracle_batched_and_in_training_mode(clouds, images, seeded_sd, which, train):
    from imfnet_amd.train.trainer import _sparse_input
    point_sets, imgs = whole_network_case(clouds, images, which)
    reps, coords = R.batched_voxels(point_sets, 0.05)
    m = _new_model(seeded_sd)
    m = m.train() if train else m.eval()
    st = _sparse_input([torch.as_tensor(r).to(DEV) for r in reps], None, 0.05, torch.device(DEV))
    assert np.array_equal(st.C.cpu().numpy(), coords)
    rm0 = m.norm3.bn.running_mean.clone()
    F = m(st, torch.as_tensor(imgs).to(DEV)).F
    assert F.requires_grad and F.shape[0] == len(coords)
    T = torch.randn(F.shape, generator=torch.Generator().manual_seed(9))
    (F * T.to(DEV)).sum().backward()
    assert torch.equal(m.norm3.bn.running_mean, rm0) != train       # training mode updates the running statistics
    F_ref, ref = oracle_gradients(seeded_sd, coords, imgs, T, bn_training=train)
    err_f = float((F.detach().cpu() - F_ref).abs().max())
    print(f"{which} train={train}: rows {len(coords)}, max|F - oracle| = {err_f:.2e}")
    assert err_f < 1e-4
    yard = {}
    if train:
        _, ref64 = oracle_gradients(seeded_sd, coords, imgs, T, bn_training=True, double=True)
        yard = {k: float((ref[k].double() - r64).abs().max()) for k, r64 in ref64.items()}
    grads = dict(m.named_parameters())
    checked, worst, late = set(), (0.0, None), []
    for k, r in ref.items():
        got = grads[k].grad
        assert got is not None and torch.isfinite(got).all(), k
        scale = float(r.abs().max())
        if scale < 1e-7:
            continue
        err = float((got.cpu() - r).abs().max())
        tol = max(REL_TOL * scale + ABS_TOL, ORDER_FACTOR * yard.get(k, 0.0))
        worst = max(worst, (err / tol, k))
        print(f"  {k}: scale {scale:.3e} err {err:.3e} oracle fp32-f64 {yard.get(k, 0.0):.3e} err/tol {err / tol:.3f}")
        if not err < tol:
            late.append((k, err, tol, scale))
        checked.add(k)
    print(f"{which} train={train}: {len(checked)} parameters checked, worst err / tol = {worst[0]:.3f} ({worst[1]})")
    assert not late, late
    assert len(checked) > 100
    from imfnet_amd import sparse as ME
    kernels = {n + ".kernel" for n, mod in m.named_modules() if isinstance(mod, ME._ConvBase)}
    assert len(kernels) >= 20 and kernels <= checked                # every convolution's weight gradient was compared
    for name, p in m.named_parameters():
        used = not any(s in name for s in ("layer3", "layer4", ".fc."))          # stored, never executed
        if used:
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
