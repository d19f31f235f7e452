"""Host side of the one-launch SGD step (csrc/optim.hip, train/optim.py FusedSGD): the --optim_kernels option and the
IMF_TRAIN_OPTIM switch, the C ABI's symbols, the ctypes mirror of imf_sgd_record against the library's own layout, the
refusals of FusedSGD, and the restatement (tests/optim_restate.py) against torch.optim.SGD in float64.  No GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import optim_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("imf_sgd_step", "imf_sgd_record_layout", "imf_sgd_chunk")


def test_optim_kernels_option_parses_defaults_to_torch_and_refuses_other_values(capsys):
    from imfnet_amd.train.trainer import make_parser, parse_config
    assert parse_config([]).optim_kernels == "torch"
    assert parse_config(["--optim_kernels", "torch"]).optim_kernels == "torch"
    assert parse_config(["--optim_kernels", "hip"]).optim_kernels == "hip"
    for bad in ("HIP", "triton", ""):
        with pytest.raises(SystemExit):
            parse_config(["--optim_kernels", bad])
    capsys.readouterr()
    assert "--optim_kernels {torch,hip}" in make_parser().format_help()
    cfg = parse_config(["--optim_kernels", "hip"])
    assert (cfg.norm_kernels, cfg.loss_kernels, cfg.fusion_kernels, cfg.image_kernels) == ("torch",) * 4


def test_optim_kernels_lands_in_the_saved_config_and_picks_the_optimizer(tmp_path):
    from imfnet_amd import ops
    from imfnet_amd.train.optim import FusedSGD
    from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config
    prev = ops.TRAIN_OPTIM
    try:
        for choice in ("hip", "torch"):
            out = tmp_path / choice
            cfg = parse_config(["--out_dir", str(out), "--optim_kernels", choice])
            tr = HardestContrastiveTrainer(cfg, None, None, device="cpu")
            tr.pool.shutdown()
            assert ops.TRAIN_OPTIM == choice
            assert (ops.TRAIN_NORM, ops.TRAIN_LOSS, ops.TRAIN_FUSION, ops.TRAIN_IMAGE) == ("torch",) * 4
            assert json.load(open(out / "config.json"))["optim_kernels"] == choice
            assert isinstance(tr.optimizer, torch.optim.SGD) and isinstance(tr.optimizer, FusedSGD) == (choice == "hip")
            group = tr.optimizer.param_groups[0]
            assert (group["lr"], group["momentum"], group["weight_decay"]) == (cfg.lr, cfg.momentum, cfg.weight_decay)
            assert len(group["params"]) == len(list(tr.model.parameters()))
    finally:
        ops.TRAIN_OPTIM = prev


def test_switch_values_and_the_environment_variable():
    from imfnet_amd import ops
    from imfnet_amd._lib import ImfError
    assert ops.TRAIN_OPTIM_CHOICES == ("torch", "hip")
    assert ops.TRAIN_OPTIM == os.environ.get("IMF_TRAIN_OPTIM", "torch")
    prev = ops.set_train_optim("hip")
    try:
        assert ops.TRAIN_OPTIM == "hip"
        with pytest.raises(ImfError):
            ops.set_train_optim("cuda")
        assert ops.TRAIN_OPTIM == "hip"
    finally:
        ops.set_train_optim(prev)
    env = {k: v for k, v in os.environ.items() if k != "IMF_TRAIN_OPTIM"}
    for value, want in ((None, "torch"), ("hip", "hip"), ("torch", "torch")):
        e = dict(env, PYTHONPATH=ROOT, **({} if value is None else {"IMF_TRAIN_OPTIM": value}))
        got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops; print(ops.TRAIN_OPTIM)"], env=e,
                             capture_output=True, text=True, cwd=ROOT)
        assert got.returncode == 0 and got.stdout.strip() == want, got.stderr
    e = dict(env, IMF_TRAIN_OPTIM="triton", PYTHONPATH=ROOT)
    got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops"], env=e, capture_output=True, text=True,
                         cwd=ROOT)
    assert got.returncode != 0 and "IMF_TRAIN_OPTIM" in got.stderr and "ImfError" in got.stderr


def test_header_declares_and_library_exports_the_symbols():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/imfnet_hip.h"
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert re.search(r"typedef struct imf_sgd_record\s*\{", text)
    for macro, value in (("IMF_SGD_PLAIN", _lib.SGD_PLAIN), ("IMF_SGD_ME", _lib.SGD_ME), ("IMF_SGD_TORCH", _lib.SGD_TORCH),
                         ("IMF_SGD_CHUNK", _lib.SGD_CHUNK), ("IMF_SGD_RECORD_FIELDS", len(_lib.SgdRecord._fields_))):
        m = re.search(r"#define\s+%s\s+(\d+)" % macro, text)
        assert m and int(m.group(1)) == value, macro
    assert L.imf_sgd_chunk() == _lib.SGD_CHUNK
    # argument errors answer before any device call
    assert L.imf_sgd_step(None, 0, None, 0, 0.1, 0.8, 1e-4, None) == 0          # nothing to do
    assert L.imf_sgd_step(None, 1, None, 1, 0.1, 0.8, 1e-4, None) == -1 and b"null" in L.imf_last_error()
    assert L.imf_sgd_step(None, -1, None, 0, 0.1, 0.8, 1e-4, None) == -1
    buf = np.zeros(1024, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    assert L.imf_sgd_step(p, 1, p + 256, 1, 0.1, -0.5, 0.0, None) == -1 and b"momentum" in L.imf_last_error()
    assert L.imf_sgd_step(p + 4, 1, p + 256, 1, 0.1, 0.5, 0.0, None) == -1 and b"aligned" in L.imf_last_error()


def test_ctypes_record_equals_the_layout_the_library_reports():
    """Field by field in the header's declaration order: name order, offset and size; and the struct's size."""
    from imfnet_amd import _lib
    from imfnet_amd.train.optim import _record_dtype
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    body = re.search(r"typedef struct imf_sgd_record\s*\{(.*?)\}\s*imf_sgd_record;", text, flags=re.S).group(1)
    declared = []
    for statement in body.split(";"):
        names = re.sub(r"^\s*(const\s+)?\w+\s+", "", statement.strip())
        declared += [n.strip().lstrip("*") for n in names.split(",") if n.strip()]
    assert declared == [n for n, _ in _lib.SgdRecord._fields_]
    off, size = C.c_size_t(), C.c_size_t()
    assert L.imf_sgd_record_layout(-1, C.byref(off), C.byref(size)) == 0
    assert (off.value, size.value) == (0, C.sizeof(_lib.SgdRecord))
    dt = _record_dtype()
    assert dt.itemsize == size.value
    for i, (name, ctype) in enumerate(_lib.SgdRecord._fields_):
        assert L.imf_sgd_record_layout(i, C.byref(off), C.byref(size)) == 0
        assert (off.value, size.value) == (getattr(_lib.SgdRecord, name).offset, C.sizeof(ctype)), name
        assert dt.fields[name][1] == off.value and dt.fields[name][0].itemsize == size.value, name
    assert L.imf_sgd_record_layout(len(_lib.SgdRecord._fields_), C.byref(off), C.byref(size)) == -1
    assert L.imf_sgd_record_layout(0, None, C.byref(size)) == -1


def test_fused_sgd_refuses_what_it_does_not_implement():
    from imfnet_amd._lib import ImfError
    from imfnet_amd.train.optim import FusedSGD
    m = torch.nn.Linear(3, 2)
    with pytest.raises(ImfError, match="Nesterov"):
        FusedSGD(m.parameters(), lr=0.1, momentum=0.9, nesterov=True)
    with pytest.raises(ImfError, match="dampening"):
        FusedSGD(m.parameters(), lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ImfError, match="maximize"):
        FusedSGD(m.parameters(), lr=0.1, maximize=True)
    with pytest.raises(ImfError, match="one parameter group"):
        FusedSGD([{"params": [m.weight]}, {"params": [m.bias], "lr": 0.01}], lr=0.1)
    opt = FusedSGD(m.parameters(), lr=0.1, momentum=0.8, weight_decay=1e-4)
    with pytest.raises(ImfError, match="one parameter group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})
    # torch's optimizer in everything else: the state_dict of one loads into the other
    ref = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.8, weight_decay=1e-4)
    assert opt.state_dict()["param_groups"] == ref.state_dict()["param_groups"]
    m.weight.grad, m.bias.grad = torch.ones_like(m.weight), torch.ones_like(m.bias)
    ref.step()
    opt.load_state_dict(ref.state_dict())
    assert torch.equal(opt.state[m.weight]["momentum_buffer"], ref.state[m.weight]["momentum_buffer"])
    with pytest.raises(ImfError, match="no CPU path"):                # the step has no CPU twin
        opt.step()
    opt.param_groups[0]["nesterov"] = True                            # e.g. from a foreign checkpoint
    with pytest.raises(ImfError, match="Nesterov"):
        opt.step()


@pytest.mark.parametrize("momentum,weight_decay", [(0.8, 1e-4), (0.9, 0.0), (0.0, 1e-2)])
def test_restated_step_in_float64_agrees_with_torch_sgd_over_three_steps(momentum, weight_decay):
    """Three steps with the learning rate decayed between them, gradients from a fixed generator; one with grad None at the
    second step.  float64 both ways: agreement to a few ulp (torch may contract a + alpha b)."""
    gen = torch.Generator().manual_seed(5)
    shapes = [(27, 4, 8), (5,), (1,), (3, 7)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.SGD(params, lr=0.1, momentum=momentum, weight_decay=weight_decay)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.9)
    mine = [p.detach().numpy().copy() for p in params]
    bufs = [None] * len(params)
    for step in range(3):
        lr = opt.param_groups[0]["lr"]
        for i, p in enumerate(params):
            skip = step == 1 and i == 2
            p.grad = None if skip else torch.randn(p.shape, generator=gen, dtype=torch.float64)
            if not skip:
                mine[i], bufs[i] = R.sgd_step(mine[i], p.grad.numpy(), bufs[i], lr, momentum, weight_decay,
                                              first=bufs[i] is None, dtype=np.float64)
        opt.step()
        sched.step()
        for i, p in enumerate(params):
            want = p.detach().numpy()
            assert np.abs(mine[i] - want).max() <= 4 * 2.0 ** -52 * np.abs(want).max(), (step, i)
            buf = opt.state[p].get("momentum_buffer")
            assert (buf is None) == (bufs[i] is None)
            if buf is not None:
                assert np.abs(bufs[i] - buf.numpy()).max() <= 4 * 2.0 ** -52 * max(np.abs(buf.numpy()).max(), 1e-300)
    assert opt.param_groups[0]["lr"] == pytest.approx(0.1 * 0.9 ** 3)


def test_restated_images_follow_the_documented_index_formula():
    """The restated image is a permutation of the three parts' bit patterns, the parts sum back to the value exactly, and
    element (k, ci, co) sits where the header says (spot checks by the formula's inverse reading)."""
    rng = np.random.default_rng(0)
    for kvol, cin, cout in ((27, 32, 64), (8, 32, 32), (1, 64, 32)):
        w = rng.standard_normal((kvol, cin, cout)).astype(np.float32)
        img = R.image_b3(w)
        p0, p1, p2 = R.split_b3(w)
        assert np.array_equal(R.bf16_value(p0) + R.bf16_value(p1) + R.bf16_value(p2), w)
        assert np.array_equal(np.sort(img), np.sort(np.concatenate([p0.ravel(), p1.ravel(), p2.ravel()])))
        CB = 4 if cout % 64 == 0 else 2
        entries = img.reshape(-1, kvol, cin // 32, 3 * CB, 64, 8)          # [y][k][cc][q][lane][t]
        for y, k, cc, cb, lane, t in ((0, 0, 0, 0, 0, 0), (cout // (16 * CB) - 1, kvol - 1, cin // 32 - 1, CB - 1, 63, 7),
                                      (0, kvol // 2, 0, 1, 37, 5)):
            ci, co = 32 * cc + 16 * (t >> 2) + 4 * (lane >> 4) + (t & 3), y * 16 * CB + 16 * cb + (lane & 15)
            for part, bits in enumerate((p0, p1, p2)):
                assert entries[y, k, cc, 3 * cb + part, lane, t] == bits[k, ci, co]
    # the two backward sources: W'[k'][co][ci] = W[k][ci][co], k' = kvol - 1 - k when flipped
    w = rng.standard_normal((27, 32, 64)).astype(np.float32)
    assert R.me_backward_source(w, True)[26 - 5, 7, 3] == w[5, 3, 7] and R.me_backward_source(w, False)[5, 7, 3] == w[5, 3, 7]
    wt = rng.standard_normal((64, 32, 3, 3)).astype(np.float32)
    assert R.torch_forward_source(wt)[1 * 3 + 2, 4, 9] == wt[9, 4, 1, 2]
    assert R.torch_backward_source(wt, True)[8 - 5, 9, 4] == wt[9, 4, 1, 2] and R.torch_backward_source(wt, False)[5, 9, 4] == wt[9, 4, 1, 2]


def test_a_parameter_with_images_is_watched_for_data_accesses():
    """`p.data.add_(1)` moves no version counter, so a registered parameter's class observes `.data`: reading or assigning
    it marks the images stale; nothing on the training path does; the class goes back when the images are dropped; pickles
    and state_dicts hold plain tensors / Parameters."""
    import copy
    import io
    from imfnet_amd import ops
    m = torch.nn.Linear(4, 3)
    p = m.weight
    ent = ops.WeightImages(p, None, None, False)
    ops.register_weight_images(p, ent)
    try:
        assert type(p) is ops._WatchedParameter and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        assert [n for n, _ in m.named_parameters()] == ["weight", "bias"]
        ent.version = version = p._version
        m(torch.ones(2, 4)).sum().backward()                       # forward, backward
        sd = m.state_dict()
        assert type(sd["weight"]) is torch.Tensor
        opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9)
        opt.zero_grad()
        assert ent.version == version == p._version                # none of these took `.data`
        p.data.add_(1)
        assert p._version == version and ent.version == -1         # unseen by the counter, seen by the class
        ent.version = p._version
        p.data = torch.zeros(3, 4)
        assert ent.version == -1 and p.shape == (3, 4) and float(p.abs().sum()) == 0
        buf = io.BytesIO()
        torch.save(m, buf)
        buf.seek(0)
        assert type(torch.load(buf, weights_only=False).weight) is torch.nn.Parameter
        twin = copy.deepcopy(m)
        assert torch.equal(twin.weight, p) and twin.weight is not p
    finally:
        ops.unregister_weight_images(ent)
    assert type(p) is torch.nn.Parameter and not any(e is ent for e in ops._WEIGHT_IMAGES.values())
