"""The image encoder's training kernels on the GPU (csrc/image_train.hip, autograd.DenseConvFunction / MaxPoolRowsFunction,
model/image_encoder.py's kernel path) against tests/image_train_restate.py: the tables as integers, the max pool and every
convolution geometry exactly on integer data, the whole trunk within the error gate of DESIGN.md §11 with the decisions the
kernel path took, bit-reproducibility, and the model with the switch on."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_train_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EPS = 2.0 ** -24


def _switch(name):
    from imfnet_amd import ops

    class _S:
        def __enter__(self):
            self.prev = ops.set_train_image(name)

        def __exit__(self, *a):
            ops.set_train_image(self.prev)
    return _S()


# ---- tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 8, 8), (1, 36, 52), (3, 16, 24)])
def test_tables_equal_the_restatement_as_integers(shape):
    from imfnet_amd import ops
    B, H, W = shape
    tabs = ops.ImageTrainTables(B, H, W, DEV)
    ref = R.tables(B, H, W)
    assert tabs.shapes == R.trunk_shapes(H, W)
    for name in R.TABLE_NAMES:
        rb, t = getattr(tabs, name), ref[name]
        assert (rb.n_slots, rb.n_out, rb.kvol) == (t["n_slots"], t["n_out"], t["kvol"]), name
        assert np.array_equal(rb.tile_rows.cpu().numpy(), t["tile_rows"]), name
        assert np.array_equal(rb.nbr.cpu().numpy().reshape(t["kvol"], -1), t["nbr"]), name
        assert np.array_equal(rb.tile_mask.cpu().numpy().view(np.uint32).reshape(-1, 4), t["tile_mask"]), name
    for fwd, opp in (("t48", "t48T"), ("td", "tdT")):                   # nbrT[k][i] = o <=> nbr[k][o] = i, on the GPU's own arrays
        f, o = getattr(tabs, fwd), getattr(tabs, opp)
        nf, no = f.nbr.cpu().numpy().reshape(f.kvol, -1), o.nbr.cpu().numpy().reshape(o.kvol, -1)
        for k in range(f.kvol):
            src = np.nonzero(nf[k] >= 0)[0]
            assert np.array_equal(no[k][nf[k][src]], src)
            back = np.nonzero(no[k] >= 0)[0]
            assert np.array_equal(nf[k][no[k][back]], back)
    assert tabs.stem.n_out == B * tabs.shapes[0][0] * tabs.shapes[0][1] and tabs.stem.nbr is None


def test_im2col_is_the_restated_patch_matrix():
    from imfnet_amd import ops
    image = R.seeded_inputs(2, 36, 52, 4)[0]
    got = ops.image_im2col7(image.to(DEV))
    assert torch.equal(got.cpu(), R.im2col7(image))


# ---- max pool ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 64])
@pytest.mark.parametrize("shape", [(2, 4, 4), (1, 18, 26), (1, 5, 7), (3, 1, 1)])
def test_max_pool_equals_the_restatement_on_data_full_of_ties(shape, C):
    from imfnet_amd import ops
    B, Hin, Win = shape
    Hout, Wout = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1
    gen = torch.Generator().manual_seed(Hin * 1000 + Win * 10 + C)
    x = torch.randint(-3, 3, (B, Hin, Win, C), generator=gen).clamp(min=0).float()
    dout = torch.randint(-4, 5, (B, Hout, Wout, C), generator=gen).float()
    out_ref, tap_ref = R.maxpool_forward(x.numpy())
    out, tap = ops.image_maxpool_forward(x.view(-1, C).to(DEV), B, Hin, Win)
    assert torch.equal(out.cpu().double(), torch.from_numpy(out_ref).view(-1, C))
    assert torch.equal(tap.cpu(), torch.from_numpy(tap_ref).view(-1, C))
    din = torch.full((B * Hin * Win, C), float("nan"), device=DEV)
    ops.image_maxpool_backward(dout.view(-1, C).to(DEV), tap, B, Hin, Win, din=din)
    din_ref = R.maxpool_backward(dout.numpy(), tap_ref, Hin, Win)
    assert torch.equal(din.cpu().double(), torch.from_numpy(din_ref).view(-1, C))          # every element written
    # Gaussian gradients: one rounding of an exact (fp64) sum of at most four terms, and the same bits twice
    g = torch.randn((B * Hout * Wout, C), generator=gen)
    a = ops.image_maxpool_backward(g.to(DEV), tap, B, Hin, Win)
    b = ops.image_maxpool_backward(g.to(DEV), tap, B, Hin, Win)
    exact = R.maxpool_backward(g.double().numpy().reshape(B, Hout, Wout, C), tap_ref, Hin, Win).reshape(-1, C)
    assert torch.equal(a, b)
    assert (np.abs(a.cpu().double().numpy() - exact) <= EPS * np.abs(exact)).all()
    # through autograd
    xr = x.view(-1, C).to(DEV).requires_grad_(True)
    from imfnet_amd.autograd import MaxPoolRowsFunction
    y, t2 = MaxPoolRowsFunction.apply(xr, B, Hin, Win)
    assert not t2.requires_grad and torch.equal(t2, tap)
    y.backward(dout.view(-1, C).to(DEV))
    assert torch.equal(xr.grad, din)


# ---- every convolution geometry, exactly ---------------------------------------------------------------------------------
GEOMETRIES = {   # name: (table, opposite, flip, cin, cout, ksize, stride, pad, resolution of the input)
    "3x3_s1_64": ("t4", "t4", True, 64, 64, 3, 1, 1, 1),
    "3x3_s2_64_128": ("t48", "t48T", False, 64, 128, 3, 2, 1, 1),
    "1x1_s2_64_128": ("td", "tdT", False, 64, 128, 1, 2, 0, 1),
    "3x3_s1_128": ("t8", "t8", True, 128, 128, 3, 1, 1, 2),
}


@pytest.fixture(scope="module")
def tables36():
    from imfnet_amd import ops
    return {B: ops.ImageTrainTables(B, 36, 52, DEV) for B in (1, 3)}


def _with_variant(v, fn):
    from imfnet_amd import ops
    prev = ops.CONV_VARIANT
    ops.CONV_VARIANT = v
    try:
        return fn()
    finally:
        ops.CONV_VARIANT = prev


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("variant", [3, 0])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_each_geometry_is_exact_on_integer_data(tables36, name, variant, B):
    """Small integers: every partial sum stays below 2^24 (K <= 1152 products of magnitude <= 6), so any correct
    fp32-accumulating kernel equals F.conv2d's float64 autograd exactly."""
    from imfnet_amd import ops
    from imfnet_amd.autograd import DenseConvFunction, training_variant
    tname, oname, flip, ci, co, ks, stride, pad, res = GEOMETRIES[name]
    tabs = tables36[B]
    (_, _), (h4, w4), (h8, w8) = tabs.shapes
    assert (h4, w4, h8, w8) == (9, 13, 5, 7)
    hin, win = (h4, w4) if res == 1 else (h8, w8)
    gen = torch.Generator().manual_seed(len(name) * 7 + B)
    x = torch.randint(-3, 4, (B, ci, hin, win), generator=gen).double().requires_grad_(True)
    w = torch.randint(-2, 3, (co, ci, ks, ks), generator=gen).double().requires_grad_(True)
    y = F.conv2d(x, w, stride=stride, padding=pad)
    g = torch.randint(-2, 3, y.shape, generator=gen).double()
    y.backward(g)
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()     # noqa: E731
    xr = rows(x).float().to(DEV).requires_grad_(True)
    wr = w.detach().float().to(DEV).requires_grad_(True)

    def run():
        out = DenseConvFunction.apply(xr, wr, getattr(tabs, tname), getattr(tabs, oname), flip)
        out.backward(rows(g).float().to(DEV))
        return out
    out = _with_variant(variant, run)
    assert torch.equal(out.detach().cpu().double(), rows(y))
    assert torch.equal(xr.grad.cpu().double(), rows(x.grad))
    assert torch.equal(wr.grad.cpu().double(), w.grad)
    if name == "1x1_s2_64_128":
        # the opposite table alone, into a NaN-prefilled buffer: pixels with an odd coordinate come back as +0.0
        v = _with_variant(variant, lambda: training_variant(1))
        buf = torch.full((B * h4 * w4, ci), float("nan"), device=DEV)
        wt = wr.detach().permute(2, 3, 0, 1).reshape(1, co, ci).contiguous()
        ops.spconv(rows(g).float().to(DEV), ops.pack_weights(wt, variant=v), ci, tabs.tdT, variant=v, split_k=1, out=buf)
        got = buf.cpu().view(B, h4, w4, ci)
        assert torch.equal(got.double().view(-1, ci), rows(x.grad))
        odd = torch.ones(h4, w4, dtype=torch.bool)
        odd[::2, ::2] = False
        assert odd.sum() == h4 * w4 - h8 * w8
        z = got[:, odd]
        assert (z == 0).all() and not torch.signbit(z).any()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("variant", [3, 0])
def test_the_stem_is_exact_on_integer_data(tables36, variant, B):
    """7x7 / 2 / pad 3, 3 -> 64 on 36 x 52: im2col + a pointwise convolution over 160 columns; no input gradient."""
    from imfnet_amd import ops
    from imfnet_amd.autograd import DenseConvFunction
    tabs = tables36[B]
    gen = torch.Generator().manual_seed(50 + B)
    x = torch.randint(-3, 4, (B, 3, 36, 52), generator=gen).double()
    w = torch.randint(-2, 3, (64, 3, 7, 7), generator=gen).double().requires_grad_(True)
    y = F.conv2d(x, w, stride=2, padding=3)
    g = torch.randint(-2, 3, y.shape, generator=gen).double()
    y.backward(g)
    wr = w.detach().float().to(DEV).requires_grad_(True)

    def run():
        m = wr.permute(2, 3, 1, 0).reshape(147, 64)
        m = torch.cat([m, m.new_zeros((13, 64))]).t().reshape(64, 160, 1, 1)
        out = DenseConvFunction.apply(ops.image_im2col7(x.float().to(DEV)), m, tabs.stem, None, False)
        out.backward(g.permute(0, 2, 3, 1).reshape(-1, 64).float().to(DEV))
        return out
    out = _with_variant(variant, run)
    assert torch.equal(out.detach().cpu().double(), y.detach().permute(0, 2, 3, 1).reshape(-1, 64))
    assert torch.equal(wr.grad.cpu().double(), w.grad)


# ---- the whole trunk --------------------------------------------------------------------------------------------------------
def _fixture_batch(images):
    return torch.from_numpy(np.concatenate([images[0], images[1]])).float()


def _trunk_case(case, images):
    kind, seed = case
    if kind == "fixture":
        image = _fixture_batch(images)
        grad_out = R.seeded_inputs(2, 120, 160, seed)[1]
    else:
        image, grad_out = R.seeded_inputs(*kind, seed)
    return image, grad_out, seed


def _gpu_step(seed, image, grad_out, switch, trace=None):
    enc = R.seeded_encoder(seed).to(DEV)
    with _switch(switch):
        if switch == "hip":
            assert enc.train()._kernels_apply(image.to(DEV))
        res = R.module_step(enc, image.to(DEV), grad_out.to(DEV), trace=trace)
    torch.cuda.synchronize()
    return enc, res


TRUNK_CASES = [((3, 16, 24), 0), ((3, 16, 24), 1), ((3, 16, 24), 2), ((1, 36, 52), 0), ((1, 36, 52), 1), ((1, 36, 52), 2),
               ("fixture", 0)]


@pytest.mark.parametrize("case", TRUNK_CASES, ids=[f"{c[0]}-{c[1]}".replace(" ", "") for c in TRUNK_CASES])
def test_trunk_is_within_the_gate_of_the_restatement_run_with_its_own_decisions(case, images):
    """e(A) = max|A - A64| / max|A64| per tensor; e_hip (against the float64 restatement run with the ReLU masks and pool
    taps the kernel path took) <= 8 * max(e_torch, 2^-24), e_torch = torch's fp32 module on the same GPU and inputs,
    free-running against the free-running restatement.  The tokens are also held against the free-running restatement, and
    the decisions may differ from the free-running ones in at most 1e-4 of the elements.

    Measured on an MI355X (profiles/image_train_error.json, written through IMF_IMAGE_ERROR_JSON): the
    largest ratio over the seven cases and 82 tensors is 1.51 (layer2.2.bn2.weight at 3x16x24, seed 0); 0, 0 and 2 of
    69 120, 118 208 and 2 304 000 decisions differ."""
    image, grad_out, seed = _trunk_case(case, images)
    state = R.seeded_encoder(seed).state_dict()
    trace = []
    enc, hip = _gpu_step(seed, image, grad_out, "hip", trace=trace)
    enc_t, tor = _gpu_step(seed, image, grad_out, "torch")
    assert len(trace) == 16 and trace[1].dtype == torch.uint8
    decisions = [t.cpu().numpy() if t.dtype == torch.uint8 else (t > 0).cpu().numpy() for t in trace]
    free = R.trunk(state, image, grad_out)
    forced = R.trunk(state, image, grad_out, decisions=decisions)
    total = sum(d.size for d in decisions)
    differ = sum(int((a != b).sum()) for a, b in zip(decisions, free["decisions"]))
    assert all(a.shape == b.shape for a, b in zip(decisions, free["decisions"]))
    rows, late = [], []

    def gate(name, got, ref_forced, t, ref_free):
        e_hip, e_torch = R.rel_err(got, ref_forced), R.rel_err(t, ref_free)
        ratio = e_hip / max(e_torch, EPS)
        rows.append(dict(tensor=name, e_hip=e_hip, e_torch=e_torch, ratio=ratio))
        print(f"{case} {name}: e_hip = {e_hip:.3e}  e_torch = {e_torch:.3e}  ratio = {ratio:.2f}")
        if not e_hip <= 8 * max(e_torch, EPS):
            late.append((name, e_hip, e_torch))

    gate("tokens", hip["out"], forced["out"], tor["out"], free["out"])
    gate("tokens (free-running)", hip["out"], free["out"], tor["out"], free["out"])
    for part in ("grads", "stats"):
        for k in hip[part]:
            gate(k, hip[part][k], forced[part][k], tor[part][k], free[part][k])
    assert len(rows) == 2 + 48 + 32
    print(f"{case}: {differ} of {total} decisions differ from the free-running restatement")
    path = os.environ.get("IMF_IMAGE_ERROR_JSON")                      # the measurement kept under profiles/
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": str(case), "shape": list(image.shape), "decisions": total,
                                "decisions_differing": differ, "tensors": rows}) + "\n")
    assert differ <= 1e-4 * total, (differ, total)
    assert not late, late
    for m, m_t in zip(enc.executed_norms(), enc_t.executed_norms()):
        assert int(m.num_batches_tracked) == 1 == int(m_t.num_batches_tracked)
    named, named_t = dict(enc.named_parameters()), dict(enc_t.named_parameters())
    unused = [k for k in named if k not in R.grad_names()]
    assert len(unused) == len(named) - 48 and any("layer3" in k for k in unused) and "backbone.fc.weight" in unused
    assert all(named[k].grad is None and named_t[k].grad is None for k in unused)
    assert all(int(m.num_batches_tracked) == 0 for m in enc.backbone.layer3.modules() if isinstance(m, torch.nn.BatchNorm2d))


def test_trunk_twice_on_the_fixture_batch_gives_the_same_bits(images):
    image, grad_out, seed = _trunk_case(("fixture", 0), images)
    runs = []
    for _ in range(2):
        trace = []
        _, res = _gpu_step(seed, image, grad_out, "hip", trace=trace)
        runs.append((res, [t.clone() for t in trace]))
    (a, ta), (b, tb) = runs
    assert np.array_equal(a["out"], b["out"])
    for part in ("grads", "stats"):
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k]), k
    assert all(torch.equal(x, y) for x, y in zip(ta, tb))


def test_kernel_path_is_taken_only_when_every_condition_holds():
    from imfnet_amd import ops
    enc = R.seeded_encoder(0).to(DEV).train()
    image = R.seeded_inputs(2, 16, 24, 0)[0].to(DEV)
    assert not enc._kernels_apply(image)                                # the switch is off
    with _switch("hip"):
        assert enc._kernels_apply(image)
        assert not enc._kernels_apply(image.cpu()) and not enc._kernels_apply(image.double())
        assert not enc._kernels_apply(image.clone().requires_grad_(True))
        assert not enc._kernels_apply(image[:1, :, :8, :8])               # one row per channel in layer2
        assert enc._kernels_apply(image[:, :, :8, :8])
        with torch.no_grad():
            assert not enc._kernels_apply(image)
        enc.backbone.layer2[1].bn1.eval()
        assert not enc._kernels_apply(image)
        enc.train()
        enc.backbone.layer1[0].bn2.momentum = None                        # cumulative average: the torch body
        assert not enc._kernels_apply(image)
        enc.backbone.layer1[0].bn2.momentum = 0.1
        enc.backbone.layer3[0].bn1.eval()                               # not executed: does not matter
        assert enc._kernels_apply(image)
        enc.eval()
        assert not enc._kernels_apply(image)
        want = enc(image)                                                # eval: today's body
        assert want.is_contiguous() and want.shape == (2, 128, 2, 3)
        out = enc.train()(image)
        assert out.shape == (2, 128, 2, 3) and out.requires_grad and len(enc._train_tables) == 1
        for h in (24, 32, 40, 48, 56):                                    # the cache keeps the last few shapes only
            enc(R.seeded_inputs(1, h, 16, 0)[0].to(DEV))
        assert len(enc._train_tables) == enc.MAX_TRAIN_TABLES and (image.device, 1, 56, 16) in enc._train_tables
        assert (image.device, 2, 16, 24) not in enc._train_tables
        assert not any("table" in k for k in enc.state_dict())
    assert ops.TRAIN_IMAGE == "torch"


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _write_tree(root, clouds, images):
    from PIL import Image
    seq = root / "sceneA" / "seq-01"
    seq.mkdir(parents=True)
    for k in (0, 1):
        a = clouds[k][::3]
        pts = np.ascontiguousarray(a[a[:, 0] < 0.3], dtype="<f4")
        with open(seq / f"cloud_bin_{k}.ply", "wb") as f:
            f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n"
                    b"property float y\nproperty float z\nend_header\n" % len(pts))
            f.write(pts.tobytes())
        u8 = (np.transpose(images[k][0], (1, 2, 0)) * 255).round().astype(np.uint8)
        Image.fromarray(u8).save(seq / f"cloud_bin_{k}_0.png")
    (root / "overlap").mkdir()
    a, b = "sceneA/seq-01/cloud_bin_0.ply", "sceneA/seq-01/cloud_bin_1.ply"
    (root / "overlap" / "sceneA@seq-01-0.30.txt").write_text(f"{a} {b} 0.5\n{b} {a} 0.5\n")


def test_model_descriptors_agree_and_a_step_with_every_switch_at_hip_is_finite(tmp_path, clouds, images):
    from imfnet_amd import ops
    from imfnet_amd.train.data import IndoorPairDataset, collate_pair_fn
    from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config
    _write_tree(tmp_path, clouds, images)
    cfg = parse_config(["--threed_match_dir", str(tmp_path), "--overlap_path", str(tmp_path / "overlap"), "--batch_size", "2",
                        "--out_dir", str(tmp_path / "out")])
    cfg.use_random_rotation = cfg.use_random_scale = False
    prev = (ops.TRAIN_NORM, ops.TRAIN_LOSS, ops.TRAIN_FUSION, ops.TRAIN_IMAGE)
    try:
        ds = IndoorPairDataset("train", ["sceneA"], cfg, seed=0, device=DEV)
        tr = HardestContrastiveTrainer(cfg, ds, None, device=DEV)
        raws = [ds.load(0), ds.load(1)]
        batch = collate_pair_fn([ds.prepare(r) for r in raws])
        tr.model.train()
        assert batch["image0"].shape == (2, 3, 120, 160)
        feats = {}
        for name in ("torch", "hip"):
            ops.set_train_image(name)
            tr.model.zero_grad(set_to_none=True)
            F0, F1 = tr.forward_pair(batch)
            feats[name] = (F0.detach().clone(), F1.detach().clone())
            if name == "hip":
                assert tr.model.img_encoder._train_tables
                (F0.sum() + F1.square().sum()).backward()
                named = dict(tr.model.img_encoder.named_parameters())
                for k in R.grad_names():
                    assert named[k].grad is not None and torch.isfinite(named[k].grad).all(), k
        for a, b in zip(feats["torch"], feats["hip"]):
            err = float((a - b).abs().max())
            print(f"descriptors, image switch hip against torch: max abs {err:.3e}")
            assert err <= 1e-4
        cfg.norm_kernels = cfg.loss_kernels = cfg.fusion_kernels = cfg.image_kernels = "hip"
        tr.pool.shutdown()
        tr = HardestContrastiveTrainer(cfg, ds, None, device=DEV)
        assert (ops.TRAIN_NORM, ops.TRAIN_LOSS, ops.TRAIN_FUSION, ops.TRAIN_IMAGE) == ("hip",) * 4
        loss = tr.train_step([raws])
        tr.pool.shutdown()
        assert all(np.isfinite(loss)) and loss[0] > 0
    finally:
        ops.set_train_norm(prev[0]), ops.set_train_loss(prev[1]), ops.set_train_fusion(prev[2]), ops.set_train_image(prev[3])
