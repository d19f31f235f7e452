"""The one-launch SGD step on the GPU (csrc/optim.hip, train/optim.py FusedSGD, ops.weight_image) against
tests/optim_restate.py bit for bit, against torch.optim.SGD within the derived rounding bound, its two weight images against
ops.pack_weights of the tensors autograd.py packs, the validity rule of ops.weight_image, and the trainer with all five
kernel switches at `hip`: no re-packing of owned weights, bit-reproducible steps, no stale inference cache, checkpoints
that resume under either optimizer."""
import contextlib

import numpy as np
import pytest
import torch

import optim_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, MU, WD, GAMMA = 0.1, 0.8, 1e-4, 0.9


@contextlib.contextmanager
def _optim_switch(name):
    from imfnet_amd import ops
    prev = ops.set_train_optim(name)
    try:
        yield
    finally:
        ops.set_train_optim(prev)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _mixed_set():
    """name -> (shape, convolution record or None, kind): the shapes the issue names.  Record: (layout, kvol, cin, cout, flip,
    backward image)."""
    from imfnet_amd import _lib
    ME, TORCH, chunk = _lib.SGD_ME, _lib.SGD_TORCH, _lib.SGD_CHUNK
    return {
        "me_27_32_64": ((27, 32, 64), (ME, 27, 32, 64, True, True), "step"),
        "me_27_64_32": ((27, 64, 32), (ME, 27, 64, 32, True, True), "step"),
        "me_tr_8_32_32": ((8, 32, 32), (ME, 8, 32, 32, False, True), "step"),            # transposed, stride 2: no flip
        "me_pw_64_32": ((64, 32), (ME, 1, 64, 32, True, False), "step"),                 # kvol 1, 2-D: no backward image
        "torch_64_32_3_3": ((64, 32, 3, 3), (TORCH, 9, 32, 64, True, True), "step"),
        "torch_128_64_1_1": ((128, 64, 1, 1), (TORCH, 1, 64, 128, False, True), "step"),
        "conv1_125_1_32": ((125, 1, 32), None, "step"),
        "bias_32": ((32,), None, "step"),
        "one": ((1,), None, "step"),
        "chunk_minus_1": ((chunk - 1,), None, "step"),
        "chunk": ((chunk,), None, "step"),
        "chunk_plus_1": ((chunk + 1,), None, "step"),
        "gradless": ((40,), None, "gradless"),
        "frozen": ((40,), None, "frozen"),
    }


def _forward_source(p):
    """The tensor autograd.py packs for the forward."""
    w = p.detach()
    if w.dim() == 4:
        co, ci, kh, kw = w.shape
        return w.float().permute(2, 3, 1, 0).reshape(kh * kw, ci, co).contiguous()
    return w if w.dim() == 3 else w.unsqueeze(0)


def _backward_source(p, flip):
    """The tensor autograd.py packs for the input gradient: transpose(1, 2) [+ flip(0)] (ME), permute(2, 3, 0, 1).reshape
    [+ flip(0)] (torch)."""
    w = p.detach()
    if w.dim() == 4:
        co, ci, kh, kw = w.shape
        wt = w.float().permute(2, 3, 0, 1).reshape(kh * kw, co, ci)
    else:
        wt = (w if w.dim() == 3 else w.unsqueeze(0)).transpose(1, 2)
    if flip:
        wt = wt.flip(0)
    return wt.contiguous()


def test_one_launch_over_a_mixed_parameter_set_three_steps():
    """Three steps, the learning rate decayed by ExponentialLR between them.  Before every step the torch twin is set to the
    fused optimizer's parameters and buffers, so each step is compared from identical inputs and the per-step bound applies:
    every value is the result of at most three roundings of 2^-24 relative to the magnitudes of its terms, two orderings
    (torch may contract a + alpha b into a fused multiply-add) differ by at most twice that, 2^-21 with margin:
      |dp| <= 2^-21 (|p| + lr |b'|),   |db| <= 2^-21 (mu |b| + |g| + wd |p|).
    Against the float32 restatement the parameters, the buffers and both images are bit-equal after every step.
    Whether the two optimizers are in fact bit-equal is printed, not gated: measured on an MI355X, they are not."""
    from imfnet_amd import ops
    from imfnet_amd.train.optim import FusedSGD
    spec = _mixed_set()
    gen = torch.Generator().manual_seed(11)
    params, twins = {}, {}
    for name, (shape, _, kind) in spec.items():
        init = torch.randn(shape, generator=gen) * 0.1
        params[name] = torch.nn.Parameter(init.to(DEV), requires_grad=kind != "frozen")
        twins[name] = torch.nn.Parameter(init.to(DEV), requires_grad=kind != "frozen")
    convs = {id(params[n]): rec for n, (_, rec, _) in spec.items() if rec is not None}
    initial = {n: _bits(p).copy() for n, p in params.items()}
    with _optim_switch("hip"):
        opt = FusedSGD(list(params.values()), lr=LR, momentum=MU, weight_decay=WD, convs=convs)
        ref = torch.optim.SGD(list(twins.values()), lr=LR, momentum=MU, weight_decay=WD)
        sched, sched_ref = (torch.optim.lr_scheduler.ExponentialLR(o, GAMMA) for o in (opt, ref))
        assert opt.image_bytes() >= sum(int(np.prod(s)) * 6 * (2 if rec[5] else 1) for s, rec, _ in spec.values() if rec)
        mine = {n: p.detach().cpu().numpy().copy() for n, p in params.items()}
        bufs = {n: None for n in params}
        stepped = [n for n, (_, _, kind) in spec.items() if kind == "step"]
        bit_equal_to_torch = True
        for step in range(3):
            lr = opt.param_groups[0]["lr"]
            assert lr == ref.param_groups[0]["lr"] == pytest.approx(LR * GAMMA ** step)
            versions = {n: p._version for n, p in params.items()}
            before = {}
            with torch.no_grad():
                for n in stepped:                                  # identical inputs for both optimizers
                    twins[n].copy_(params[n])
                    if step:
                        ref.state[twins[n]]["momentum_buffer"].copy_(opt.state[params[n]]["momentum_buffer"])
            for n in stepped:
                g = (torch.randn(spec[n][0], generator=gen) * (0.5 if step != 1 else 3e-3)).to(DEV)
                params[n].grad, twins[n].grad = g, g.clone()
                before[n] = (mine[n].copy(), None if bufs[n] is None else bufs[n].copy(), g.cpu().numpy())
                mine[n], bufs[n] = R.sgd_step(mine[n], before[n][2], bufs[n], lr, MU, WD, first=step == 0)
            opt.step()
            ref.step()
            torch.cuda.synchronize()
            for n in stepped:
                p, t = params[n], twins[n]
                b, bt = opt.state[p]["momentum_buffer"], ref.state[t]["momentum_buffer"]
                assert np.array_equal(_bits(p), mine[n].view(np.uint32)), (step, n)
                assert np.array_equal(_bits(b), bufs[n].view(np.uint32)), (step, n)
                p0, b0, g = before[n]
                b0 = np.zeros_like(p0) if b0 is None else b0
                dp = np.abs(p.detach().cpu().numpy().astype(np.float64) - t.detach().cpu().numpy().astype(np.float64))
                db = np.abs(b.cpu().numpy().astype(np.float64) - bt.cpu().numpy().astype(np.float64))
                bound_p = 2.0 ** -21 * (np.abs(p0).astype(np.float64) + lr * np.abs(bufs[n]).astype(np.float64))
                bound_b = 2.0 ** -21 * (MU * np.abs(b0).astype(np.float64) + np.abs(g).astype(np.float64) +
                                        WD * np.abs(p0).astype(np.float64))
                assert (dp <= bound_p).all(), (step, n, float((dp - bound_p).max()))
                assert (db <= bound_b).all(), (step, n, float((db - bound_b).max()))
                bit_equal_to_torch &= bool(dp.max() == 0 and db.max() == 0)
                assert p._version > versions[n], (step, n)
            for n in ("gradless", "frozen"):                       # untouched: no write, no version, no buffer
                assert np.array_equal(_bits(params[n]), initial[n]) and params[n]._version == versions[n]
                assert "momentum_buffer" not in opt.state.get(params[n], {})
            for n, (shape, rec, _) in spec.items():                # both images, bit-equal after each step
                if rec is None:
                    assert opt.images(params[n]) is None
                    continue
                p = params[n]
                fwd, bwd = opt.images(p)
                want = ops.pack_weights(_forward_source(p), variant=3)
                assert np.array_equal(_bits(fwd), _bits(want)), (step, n)
                assert np.array_equal(fwd.cpu().numpy().view(np.uint16), R.image_b3(_forward_source(p).cpu().numpy())), (step, n)
                assert (bwd is not None) == rec[5]
                if bwd is not None:
                    want = ops.pack_weights(_backward_source(p, rec[4]), variant=3)
                    assert np.array_equal(_bits(bwd), _bits(want)), (step, n)
                    src = (R.torch_backward_source if p.dim() == 4 else R.me_backward_source)(mine[n], rec[4])
                    assert np.array_equal(bwd.cpu().numpy().view(np.uint16), R.image_b3(src)), (step, n)
                # and weight_image hands out exactly these tensors
                assert ops.weight_image(p, "forward", 3).data_ptr() == fwd.data_ptr()
                if bwd is not None:
                    assert ops.weight_image(p, "backward", 3, flip=rec[4]).data_ptr() == bwd.data_ptr()
            sched.step()
            sched_ref.step()
        print(f"FusedSGD against torch.optim.SGD over three steps from identical inputs: bit-equal = {bit_equal_to_torch}")


def test_momentum_zero_and_no_weight_decay_follow_the_restatement():
    from imfnet_amd.train.optim import FusedSGD
    gen = torch.Generator().manual_seed(3)
    for mu, wd in ((0.0, 1e-2), (0.9, 0.0)):
        p = torch.nn.Parameter((torch.randn(3000, generator=gen)).to(DEV))
        opt = FusedSGD([p], lr=0.05, momentum=mu, weight_decay=wd)
        mine, buf = p.detach().cpu().numpy().copy(), None
        for step in range(2):
            g = torch.randn(3000, generator=gen)
            p.grad = g.to(DEV)
            mine, buf = R.sgd_step(mine, g.numpy(), buf, 0.05, mu, wd, first=step == 0)
            opt.step()
            assert np.array_equal(_bits(p), mine.view(np.uint32))
            if mu == 0:
                assert "momentum_buffer" not in opt.state.get(p, {})
            else:
                assert np.array_equal(_bits(opt.state[p]["momentum_buffer"]), buf.view(np.uint32))


def _conv_module():
    from imfnet_amd import sparse
    torch.manual_seed(0)
    return sparse.MinkowskiConvolution(32, 64, kernel_size=3, stride=1, dimension=3).to(DEV)


def _stepped(conv):
    from imfnet_amd.train.optim import FusedSGD
    opt = FusedSGD(conv.parameters(), lr=LR, momentum=MU, weight_decay=WD, model=conv)
    conv.kernel.grad = torch.full_like(conv.kernel, 0.25)
    opt.step()
    return opt


def test_weight_image_returns_the_cached_images_and_repacks_after_a_foreign_write():
    """Right after a step the optimizer's tensors come back (same data_ptr).  After an in-place write under no_grad, and after
    load_state_dict, the parameter's `_version` has moved on: the image is packed from the parameter as it is now.  With the
    switch at `torch` the optimizer's images are never handed out."""
    from imfnet_amd import ops
    conv = _conv_module()
    p = conv.kernel
    with _optim_switch("hip"):
        opt = _stepped(conv)
        fwd, bwd = opt.images(p)
        assert bwd is not None                                    # found through the module walk: stride 1 -> flipped taps
        assert ops.weight_image(p, "forward", 3).data_ptr() == fwd.data_ptr()
        assert ops.weight_image(p, "backward", 3, flip=True).data_ptr() == bwd.data_ptr()
        assert ops.weight_image(p, "backward", 3).data_ptr() == bwd.data_ptr()
        other = ops.weight_image(p, "backward", 3, flip=False)   # not the image the optimizer keeps: packed
        assert other.data_ptr() != bwd.data_ptr()
        assert np.array_equal(_bits(other), _bits(ops.pack_weights(_backward_source(p, False), variant=3)))
        assert ops.weight_image(p, "forward", 0).data_ptr() != fwd.data_ptr()      # another arithmetic: packed
        with _optim_switch("torch"):
            assert ops.weight_image(p, "forward", 3).data_ptr() != fwd.data_ptr()
        with torch.no_grad():
            p.add_(1)
        for which, source in (("forward", _forward_source(p)), ("backward", _backward_source(p, True))):
            got = ops.weight_image(p, which, 3, flip=True)
            assert got.data_ptr() not in (fwd.data_ptr(), bwd.data_ptr())
            assert np.array_equal(_bits(got), _bits(ops.pack_weights(source, variant=3)))
        # the next step makes the images current again
        p.grad = torch.full_like(p, -0.5)
        opt.step()
        assert ops.weight_image(p, "forward", 3).data_ptr() == fwd.data_ptr()
        assert np.array_equal(_bits(fwd), _bits(ops.pack_weights(_forward_source(p), variant=3)))
        state = {k: v.clone() + 2 for k, v in conv.state_dict().items()}
        conv.load_state_dict(state)
        got = ops.weight_image(p, "forward", 3)
        assert got.data_ptr() != fwd.data_ptr()
        assert np.array_equal(_bits(got), _bits(ops.pack_weights(_forward_source(p), variant=3)))
        assert torch.equal(p.detach(), state["kernel"])


def test_weight_image_repacks_after_a_write_through_data():
    """The issue's case `p.data.add_(1)`.  torch gives the tensor `.data` returns a version counter of its own, so the write
    leaves `p._version` where it was (printed; measured on an MI355X with torch 2.10: 2 before, 2 after): the version rule
    alone cannot see it.  A parameter with images is therefore watched for `.data` accesses (ops._WatchedParameter), which
    mark the images stale until the next step."""
    from imfnet_amd import ops
    conv = _conv_module()
    p = conv.kernel
    with _optim_switch("hip"):
        opt = _stepped(conv)
        fwd, _ = opt.images(p)
        assert ops.weight_image(p, "forward", 3).data_ptr() == fwd.data_ptr()
        version = p._version
        p.data.add_(1)
        print(f"p._version before / after p.data.add_(1): {version} / {p._version}")
        got = ops.weight_image(p, "forward", 3)
        assert got.data_ptr() != fwd.data_ptr()
        assert np.array_equal(_bits(got), _bits(ops.pack_weights(_forward_source(p), variant=3)))
        back = ops.weight_image(p, "backward", 3, flip=True)
        assert back.data_ptr() != opt.images(p)[1].data_ptr()
        assert np.array_equal(_bits(back), _bits(ops.pack_weights(_backward_source(p, True), variant=3)))
        p.grad = torch.full_like(p, 0.5)                          # the next step makes the images current again
        opt.step()
        assert ops.weight_image(p, "forward", 3).data_ptr() == fwd.data_ptr()
        assert np.array_equal(_bits(fwd), _bits(ops.pack_weights(_forward_source(p), variant=3)))
        p.data.copy_(torch.zeros_like(p))                         # and `p.data.copy_`, the issue's other spelling
        assert ops.weight_image(p, "forward", 3).data_ptr() != fwd.data_ptr()


# ---- the trainer ----------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def tree(tmp_path_factory, clouds, images):
    from imfnet_amd import ops
    root = tmp_path_factory.mktemp("optim_tree")
    _write_tree(root, clouds, images)
    prev = (ops.TRAIN_NORM, ops.TRAIN_LOSS, ops.TRAIN_FUSION, ops.TRAIN_IMAGE, ops.TRAIN_OPTIM)
    yield root
    for setter, value in zip((ops.set_train_norm, ops.set_train_loss, ops.set_train_fusion, ops.set_train_image,
                              ops.set_train_optim), prev):
        setter(value)


def _trainer(root, tag, optim="hip", resume=None):
    from imfnet_amd.train.data import IndoorPairDataset
    from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config
    args = ["--threed_match_dir", str(root), "--overlap_path", str(root / "overlap"), "--batch_size", "2",
            "--out_dir", str(root / tag), "--norm_kernels", "hip", "--loss_kernels", "hip", "--fusion_kernels", "hip",
            "--image_kernels", "hip", "--optim_kernels", optim]
    if resume is not None:
        args += ["--resume", str(resume)]
    cfg = parse_config(args)
    cfg.use_random_rotation = cfg.use_random_scale = False
    ds = IndoorPairDataset("train", ["sceneA"], cfg, seed=0, device=DEV)
    tr = HardestContrastiveTrainer(cfg, ds, None, device=DEV)
    return tr, ds, [ds.load(0), ds.load(1)]


def _descriptors(model, item, cfg):
    """Eval-mode descriptors of one fragment, as valid_epoch computes them."""
    from imfnet_amd.train.trainer import _sparse_input
    model.eval()
    with torch.no_grad():
        st = _sparse_input([item["xyz0"]], None, cfg.voxel_size, torch.device(DEV), "f64")
        return model(st, torch.as_tensor(item["image0"])[None].to(DEV)).F.clone()


def test_trainer_packs_no_owned_weight_is_reproducible_and_leaves_no_stale_cache(tree, monkeypatch):
    from imfnet_amd import ops
    from imfnet_amd.model import load_model
    from imfnet_amd.train.data import IndoorPairDataset
    from imfnet_amd.train.optim import FusedSGD
    tr, ds, raws = _trainer(tree, "a")
    assert isinstance(tr.optimizer, FusedSGD) and ops.TRAIN_OPTIM == "hip"
    n_sparse = sum(tr.optimizer.images(m.kernel) is not None for m in tr.model.modules() if hasattr(m, "kernel_volume"))
    n_dense = sum(tr.optimizer.images(c.weight) is not None for c, _ in tr.model.img_encoder.executed_convs())
    print(f"weights with images: {n_sparse} sparse, {n_dense} dense; arena {tr.optimizer.image_bytes() / 2 ** 20:.1f} MiB")
    assert n_sparse >= 20 and n_dense == 15
    # the fragment of the eval-mode checks comes from a data set of its own: prepare() draws from the data set's generator
    item = IndoorPairDataset("train", ["sceneA"], tr.config, seed=0, device=DEV).prepare(raws[0])
    _descriptors(tr.model, item, tr.config)                       # fills every inference cache keyed on `_version`
    calls = []
    real = ops.pack_weights

    def counting(kernel, *a, **k):
        calls.append(tuple(kernel.shape))
        return real(kernel, *a, **k)
    monkeypatch.setattr(ops, "pack_weights", counting)
    losses, per_step = [], []
    for _ in range(2):
        calls.clear()
        losses.append(tr.train_step([raws]))
        per_step.append(list(calls))
    monkeypatch.setattr(ops, "pack_weights", real)
    assert all(np.isfinite(v) for loss in losses for v in loss) and losses[0][0] > 0
    # the second step: only the stem's derived [160, 64] matrix is packed (once per side), nothing the optimizer owns
    print(f"pack_weights calls: step 1 {len(per_step[0])}, step 2 {len(per_step[1])}")
    assert per_step[1] and all(shape == (1, 160, 64) for shape in per_step[1]), per_step[1]
    assert len(per_step[1]) == 2
    # a second trainer from the same seed: bit-identical parameters after two steps
    tr2, _, raws2 = _trainer(tree, "b")
    for _ in range(2):
        tr2.train_step([raws2])
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(tr.model.named_parameters(), tr2.model.named_parameters()):
        assert torch.equal(a, b), k
    tr2.pool.shutdown()
    # stale-cache check: eval descriptors after the steps against a fresh model loaded from state_dict()
    got = _descriptors(tr.model, item, tr.config)
    c = tr.config
    fresh = load_model(c.model)(1, c.model_n_out, bn_momentum=c.bn_momentum, normalize_feature=c.normalize_feature,
                                conv1_kernel_size=c.conv1_kernel_size, D=3, config=None)
    fresh.load_state_dict(tr.model.state_dict())
    want = _descriptors(fresh.to(DEV), item, c)
    tr.pool.shutdown()
    assert got.shape == want.shape and torch.equal(got, want)


def test_checkpoints_resume_under_either_optimizer(tree):
    from imfnet_amd.train.optim import FusedSGD
    for first, second in (("hip", "torch"), ("torch", "hip")):
        tr, _, raws = _trainer(tree, f"ckpt_{first}", optim=first)
        assert isinstance(tr.optimizer, FusedSGD) == (first == "hip")
        tr.train_step([raws])
        tr._save(1, "checkpoint")
        tr.pool.shutdown()
        tr2, _, raws2 = _trainer(tree, f"ckpt_{first}_resumed", optim=second, resume=tree / f"ckpt_{first}")
        assert isinstance(tr2.optimizer, FusedSGD) == (second == "hip") and tr2.start_epoch == 2
        n = 0
        for (k, a), (_, b) in zip(tr.model.named_parameters(), tr2.model.named_parameters()):
            assert torch.equal(a, b), k
            sa, sb = tr.optimizer.state.get(a, {}), tr2.optimizer.state.get(b, {})
            assert ("momentum_buffer" in sa) == ("momentum_buffer" in sb), k
            if "momentum_buffer" in sa:
                assert np.array_equal(_bits(sa["momentum_buffer"]), _bits(sb["momentum_buffer"])), k
                n += 1
        assert n >= 100
        loss = tr2.train_step([raws2])                               # and training goes on from the loaded buffers
        tr2.pool.shutdown()
        assert all(np.isfinite(loss))
