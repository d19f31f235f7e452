"""Host side of the image encoder's training kernels (csrc/image_train.hip): the float64 restatement against torch's
float64 autograd of the unchanged ImageEncoder module, its max pool on data full of ties, its tables, the C ABI's symbols
and their argument checks, the --image_kernels option and the IMF_TRAIN_IMAGE switch, and the fallback of the module with
the switch at "hip" on CPU tensors.  No GPU."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_train_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("imf_image_train_tables_bytes", "imf_image_train_tables_build", "imf_image_im2col7",
           "imf_image_maxpool_forward", "imf_image_maxpool_backward")


@pytest.mark.parametrize("shape,seed", [((3, 16, 24), 0), ((1, 36, 52), 1), ((2, 40, 24), 2)])
def test_restatement_matches_torch_float64_autograd_of_the_module(shape, seed):
    """The yardstick itself: the output, the 48 parameter gradients and the 32 running statistics within 1e-12 relative of
    the unchanged module in float64 under torch's autograd; and its own decisions handed back in change nothing."""
    enc = R.seeded_encoder(seed, torch.float64)
    image, grad_out = R.seeded_inputs(*shape, seed)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    ref = R.trunk(state, image, grad_out)
    want = R.module_step(enc, image.double(), grad_out.double())
    assert len(R.grad_names()) == 48 and len(R.stat_names()) == 32
    assert R.rel_err(ref["out"], want["out"]) <= 1e-12
    for k in R.grad_names():
        assert ref["grads"][k].shape == want["grads"][k].shape and np.abs(want["grads"][k]).max() > 0, k
        assert R.rel_err(ref["grads"][k], want["grads"][k]) <= 1e-12, k
    for k in R.stat_names():
        assert R.rel_err(ref["stats"][k], want["stats"][k]) <= 1e-12, k
    named = dict(enc.named_parameters())
    assert all(named[k].grad is None for k in named if k not in R.grad_names())
    # 15 ReLU masks and the pool's taps, in execution order
    d = ref["decisions"]
    assert len(d) == 16 and d[1].dtype == np.uint8 and sum(m.dtype == np.bool_ for m in d) == 15
    again = R.trunk(state, image, grad_out, decisions=d)
    assert np.array_equal(again["out"], ref["out"])
    assert all(np.array_equal(again["grads"][k], ref["grads"][k]) for k in R.grad_names())


def test_forced_decisions_move_the_gradient():
    """The `decisions` argument is used: with one ReLU mask emptied, the gradients below it vanish."""
    enc = R.seeded_encoder(0, torch.float64)
    image, grad_out = R.seeded_inputs(3, 16, 24, 0)
    state = enc.state_dict()
    ref = R.trunk(state, image, grad_out)
    d = [m.copy() for m in ref["decisions"]]
    d[0][:] = False
    got = R.trunk(state, image, grad_out, decisions=d)
    assert not got["grads"]["backbone.conv1.weight"].any() and ref["grads"]["backbone.conv1.weight"].any()


@pytest.mark.parametrize("shape", [(2, 4, 4, 4), (1, 18, 26, 8), (1, 5, 7, 4), (3, 1, 1, 4)])
def test_pool_restatement_routes_ties_like_torch(shape):
    """Integers clamped at 0 (ties are the rule): values, winners and the routed gradient equal torch's float64 max pool."""
    B, Hin, Win, C = shape
    gen = torch.Generator().manual_seed(Hin * 100 + Win)
    x = torch.randint(-3, 3, shape, generator=gen).clamp(min=0).double()
    dout_shape = (B, (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1, C)
    dout = torch.randint(-4, 5, dout_shape, generator=gen).double()
    out, tap = R.maxpool_forward(x.numpy())
    din = R.maxpool_backward(dout.numpy(), tap, Hin, Win)
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yt, idx = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    yt.backward(dout.permute(0, 3, 1, 2).contiguous())
    assert np.array_equal(out, yt.detach().permute(0, 2, 3, 1).numpy())
    assert np.array_equal(din, xt.grad.permute(0, 2, 3, 1).numpy())
    oy, ox = np.meshgrid(np.arange(dout_shape[1]), np.arange(dout_shape[2]), indexing="ij")
    iy, ix = 2 * oy[None, :, :, None] + tap // 3 - 1, 2 * ox[None, :, :, None] + tap % 3 - 1
    assert np.array_equal(iy * Win + ix, idx.permute(0, 2, 3, 1).numpy())
    assert np.array_equal(R.maxpool_select(x.numpy(), tap), out)
    if Hin > 1:
        assert (x == 0).float().mean() > 0.3 and len(np.unique(tap)) > 3


@pytest.mark.parametrize("shape", [(2, 8, 8), (1, 36, 52), (3, 16, 24)])
def test_restated_tables(shape):
    B, H, W = shape
    (h2, w2), (h4, w4), (h8, w8) = R.trunk_shapes(H, W)
    T = R.tables(B, H, W)
    assert set(T) == set(R.TABLE_NAMES)
    for name, rows, src, kvol in (("t4", h4 * w4, h4 * w4, 9), ("t48", h8 * w8, h4 * w4, 9), ("t48T", h4 * w4, h8 * w8, 9),
                                  ("td", h8 * w8, h4 * w4, 1), ("tdT", h4 * w4, h8 * w8, 1), ("t8", h8 * w8, h8 * w8, 9)):
        t = T[name]
        assert t["n_out"] == B * rows and t["kvol"] == kvol and t["n_slots"] % 64 == 0 and 0 <= t["n_slots"] - t["n_out"] < 64
        assert t["nbr"].shape == (kvol, t["n_slots"]) and t["nbr"].max() < B * src and t["nbr"].min() >= -1
        assert (t["nbr"][:, t["n_out"]:] == -1).all() and (t["tile_rows"][t["n_out"]:] == -1).all()
        assert t["tile_mask"].shape == (t["n_slots"] // 64, 4) and not t["tile_mask"][:, 1:].any()
    # a stride-1 table is its own opposite with the taps flipped; the strided ones by the relation of the header
    for name in ("t4", "t8"):
        assert np.array_equal(R.opposite_table(T[name], T[name]["n_out"])["nbr"], T[name]["nbr"][::-1])
    for fwd, opp in (("t48", "t48T"), ("td", "tdT")):
        for k in range(T[fwd]["kvol"]):
            for o in range(T[fwd]["n_out"]):
                i = T[fwd]["nbr"][k][o]
                if i >= 0:
                    assert T[opp]["nbr"][k][i] == o
        assert (T[opp]["nbr"] >= 0).sum() == (T[fwd]["nbr"] >= 0).sum()
    odd = np.array([((r % (h4 * w4)) // w4) % 2 == 1 or (r % w4) % 2 == 1 for r in range(B * h4 * w4)])
    assert ((T["tdT"]["nbr"][0][: B * h4 * w4] < 0) == odd).all()
    assert (T["tdT"]["tile_mask"][:, 0] == 1).all()
    # the centre tap of a stride-1 table is the pixel itself: the convolution of a one-hot weight is the identity
    assert np.array_equal(T["t4"]["nbr"][4][: B * h4 * w4], np.arange(B * h4 * w4))
    x = torch.arange(B * h4 * w4 * 2, dtype=torch.float64).view(-1, 2)
    wgt = torch.zeros(2, 2, 3, 3, dtype=torch.float64)
    wgt[0, 0, 0, 2] = wgt[1, 1, 2, 1] = 1.0
    want = F.conv2d(x.view(B, h4, w4, 2).permute(0, 3, 1, 2), wgt, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, 2)
    assert torch.equal(R.table_conv(x, wgt, T["t48"]), want)


def test_header_declares_and_library_exports_the_symbols():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/imfnet_hip.h"
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    for name in _lib.IMAGE_TRAIN_TABLES:
        assert re.search(r"\b%s\b" % name, text), name
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = set(line.split()[-1] for line in nm.stdout.splitlines() if line.strip())
        assert set(SYMBOLS) <= exported
    # sizes: the six tables of the restatement, 0 for shapes the build refuses
    for B, H, W in ((2, 8, 8), (1, 36, 52), (3, 16, 24), (2, 120, 160)):
        T = R.tables(B, H, W)
        words = sum(t["n_slots"] * (1 + t["kvol"]) + t["n_slots"] // 64 * 4 for t in T.values())
        assert L.imf_image_train_tables_bytes(B, H, W) == (4 * words + 255) // 256 * 256
    for bad in ((0, 16, 16), (-1, 16, 16), (1, 7, 16), (1, 16, 7), (1, 0, 0)):
        assert L.imf_image_train_tables_bytes(*bad) == 0, bad


def test_argument_errors_return_a_status_without_a_gpu():
    """Every refusal comes before any device call, so it answers on a machine without a GPU (host pointers here)."""
    import ctypes as C
    from imfnet_amd import _lib
    L = _lib.lib()
    EINVAL = -1
    m = re.search(r"#define\s+IMF_EINVAL\s+(-?\d+)", open(os.path.join(ROOT, "include", "imfnet_hip.h")).read())
    assert m and int(m.group(1)) == EINVAL
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    p += (-p) % 256
    out = _lib.ImageTrainTables()
    need = L.imf_image_train_tables_bytes(2, 16, 24)
    assert 0 < need < (1 << 15)

    def build(B=2, H=16, W=24, storage=p, nbytes=need, o=C.byref(out)):
        return L.imf_image_train_tables_build(B, H, W, storage, nbytes, o, None)

    assert build(B=0) == EINVAL and build(B=-3) == EINVAL and build(H=7) == EINVAL and build(W=7) == EINVAL
    assert build(nbytes=need - 1) == EINVAL and b"small" in L.imf_last_error()
    assert build(nbytes=0) == EINVAL
    assert build(storage=None) == EINVAL and b"null" in L.imf_last_error()
    assert build(o=None) == EINVAL and b"null" in L.imf_last_error()
    assert build(storage=p + 16) == EINVAL and b"aligned" in L.imf_last_error()

    assert L.imf_image_im2col7(None, 1, 16, 16, p, None) == EINVAL and L.imf_image_im2col7(p, 1, 16, 16, None, None) == EINVAL
    assert L.imf_image_im2col7(p, 0, 16, 16, p, None) == EINVAL and L.imf_image_im2col7(p, 1, 7, 16, p, None) == EINVAL

    def fwd(x=p, B=1, Hin=4, Win=4, c=8, o=p, tap=p):
        return L.imf_image_maxpool_forward(x, B, Hin, Win, c, o, tap, None)

    def bwd(dout=p, tap=p, B=1, Hin=4, Win=4, c=8, din=p):
        return L.imf_image_maxpool_backward(dout, tap, B, Hin, Win, c, din, None)

    for call in (fwd, bwd):
        for c in (0, 1, 2, 3, 6, 63, -4):
            assert call(c=c) == EINVAL, c
        assert b"C %" in L.imf_last_error()
        assert call(B=0) == EINVAL and call(Hin=0) == EINVAL and call(Win=0) == EINVAL and call(tap=None) == EINVAL
        assert call(tap=p + 1) == EINVAL and b"aligned" in L.imf_last_error()
    assert fwd(x=None) == EINVAL and fwd(o=None) == EINVAL and fwd(x=p + 4) == EINVAL
    assert bwd(dout=None) == EINVAL and bwd(din=None) == EINVAL and bwd(din=p + 8) == EINVAL


def test_image_kernels_option_parses_defaults_to_torch_and_refuses_other_values(capsys):
    from imfnet_amd.train.trainer import make_parser, parse_config
    assert parse_config([]).image_kernels == "torch"
    assert parse_config(["--image_kernels", "torch"]).image_kernels == "torch"
    assert parse_config(["--image_kernels", "hip"]).image_kernels == "hip"
    for bad in ("HIP", "triton", ""):
        with pytest.raises(SystemExit):
            parse_config(["--image_kernels", bad])
    capsys.readouterr()
    assert "--image_kernels {torch,hip}" in make_parser().format_help()
    cfg = parse_config(["--image_kernels", "hip"])
    assert cfg.norm_kernels == "torch" and cfg.loss_kernels == "torch" and cfg.fusion_kernels == "torch"


def test_image_kernels_lands_in_the_saved_config_and_sets_the_switch(tmp_path):
    from imfnet_amd import ops
    from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config
    prev = ops.TRAIN_IMAGE
    try:
        for choice in ("hip", "torch"):
            out = tmp_path / choice
            cfg = parse_config(["--out_dir", str(out), "--image_kernels", choice])
            tr = HardestContrastiveTrainer(cfg, None, None, device="cpu")
            tr.pool.shutdown()
            assert ops.TRAIN_IMAGE == choice
            assert ops.TRAIN_NORM == "torch" and ops.TRAIN_LOSS == "torch" and ops.TRAIN_FUSION == "torch"
            assert json.load(open(out / "config.json"))["image_kernels"] == choice
    finally:
        ops.TRAIN_IMAGE = prev


def test_switch_values_and_the_environment_variable():
    from imfnet_amd import ops
    from imfnet_amd._lib import ImfError
    assert ops.TRAIN_IMAGE_CHOICES == ("torch", "hip")
    assert ops.TRAIN_IMAGE == os.environ.get("IMF_TRAIN_IMAGE", "torch")
    prev = ops.set_train_image("hip")
    try:
        assert ops.TRAIN_IMAGE == "hip"
        with pytest.raises(ImfError):
            ops.set_train_image("cuda")
        assert ops.TRAIN_IMAGE == "hip"
    finally:
        ops.set_train_image(prev)
    env = {k: v for k, v in os.environ.items() if k != "IMF_TRAIN_IMAGE"}
    for value, want in ((None, "torch"), ("hip", "hip"), ("torch", "torch")):
        e = dict(env, PYTHONPATH=ROOT, **({} if value is None else {"IMF_TRAIN_IMAGE": value}))
        got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops; print(ops.TRAIN_IMAGE)"], env=e,
                             capture_output=True, text=True, cwd=ROOT)
        assert got.returncode == 0 and got.stdout.strip() == want, got.stderr
    e = dict(env, IMF_TRAIN_IMAGE="triton", PYTHONPATH=ROOT)
    got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops"], env=e, capture_output=True, text=True,
                         cwd=ROOT)
    assert got.returncode != 0 and "IMF_TRAIN_IMAGE" in got.stderr and "ImfError" in got.stderr
    with pytest.raises(ImfError):                                     # the kernels have no CPU twin: CPU rows are an error
        ops.image_maxpool_forward(torch.zeros(16, 4), 1, 4, 4)
    with pytest.raises(ImfError):
        ops.image_im2col7(torch.zeros(1, 3, 16, 16))
    assert ops.image_trunk_shapes(120, 160) == ((60, 80), (30, 40), (15, 20)) == R.trunk_shapes(120, 160)
    assert ops.image_trunk_shapes(36, 52) == ((18, 26), (9, 13), (5, 7))


def test_cpu_module_with_the_switch_at_hip_runs_the_torch_body_bit_for_bit():
    """A CPU ImageEncoder in training mode: the kernels do not apply, so the switch changes nothing -- output, gradients
    and running statistics bit-identical; the model's state_dict keeps its 361 keys."""
    from imfnet_amd import ops
    from imfnet_amd.model import load_model
    image, grad_out = R.seeded_inputs(2, 32, 40, 3)
    runs = {}
    for switch in ("torch", "hip"):
        prev = ops.set_train_image(switch)
        try:
            enc = R.seeded_encoder(3)
            runs[switch] = R.module_step(enc, image, grad_out)
            assert all(int(n.num_batches_tracked) == 1 for n in enc.executed_norms()) and len(enc.executed_norms()) == 16
            assert not enc._kernels_apply(image)
        finally:
            ops.set_train_image(prev)
    for part in ("grads", "stats"):
        for k, v in runs["torch"][part].items():
            assert np.array_equal(v, runs["hip"][part][k]), k
    assert np.array_equal(runs["torch"]["out"], runs["hip"]["out"])
    model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3, config=None)
    keys = list(model.state_dict())
    assert len(keys) == 361 and not any("table" in k for k in keys)
    assert sum(k.startswith("img_encoder.") for k in keys) == len(model.img_encoder.state_dict())


def test_cached_tables_are_bounded_and_stay_out_of_copies_and_pickles():
    """The per-shape table cache keeps the last few shapes only, and copy.deepcopy / pickle leave it behind (stand-in
    entries here: the real ones are device tensors)."""
    import copy
    import pickle
    from imfnet_amd.model.image_encoder import ImageEncoder, trunk_supported
    enc = ImageEncoder()
    enc._train_tables[("cpu", 1, 8, 8)] = object()
    for twin in (copy.deepcopy(enc), pickle.loads(pickle.dumps(enc))):
        assert len(twin._train_tables) == 0 and list(twin.state_dict()) == list(enc.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(twin.state_dict().values(), enc.state_dict().values()))
    assert len(enc._train_tables) == 1 and ImageEncoder.MAX_TRAIN_TABLES >= 2
    assert not trunk_supported(enc.backbone)                          # CPU weights: neither kernel path applies
