"""Host side of the attention-fusion training kernels (csrc/fusion_train.hip): the float64 restatement against torch's
float64 autograd of model/fusion.py, the torch fp32 error that the GPU gate is measured against, the C ABI's symbols and
their argument checks, the --fusion_kernels option and the IMF_TRAIN_FUSION switch, and the fallback of the model with
the switch at "hip" on CPU tensors.  No GPU."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import fusion_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("imf_fusion_train_chunk_rows", "imf_fusion_train_saved_bytes", "imf_fusion_train_workspace_bytes",
           "imf_fusion_train_forward", "imf_fusion_train_backward")
DIMS = (256, 128, 128, 1024)


@pytest.mark.parametrize("name", ["rows_40_0_7", "rows_17", "tokens_65"])
def test_restatement_matches_torch_float64_autograd_of_the_module(name):
    """The yardstick itself: z, dx, dtokens and the 14 parameter gradients within 1e-12 relative of AttentionFusion in
    float64 under torch's autograd; rows_40_0_7 is a batch of three items, the middle one empty."""
    c = FC.case(name)
    ref = FC.reference(name)
    want = FC.torch_path(c, dtype=torch.float64)
    assert set(ref) == set(FC.TENSORS) == set(want)
    for key in FC.TENSORS:
        assert ref[key].dtype == np.float64
        e = FC.rel_err(want[key], ref[key])
        assert e <= 1e-12, (key, e)
    if name == "rows_40_0_7":
        assert not ref["dtokens"][1].any() and ref["dtokens"][0].any() and ref["dtokens"][2].any()


@pytest.mark.parametrize("name", sorted(FC.SHAPES))
def test_torch_fp32_error_is_not_zero_so_the_gpu_gate_is_not_its_floor(name):
    """The GPU gate is e_hip <= 8 * max(e_torch, 2^-24): torch's CPU fp32 run of the same inputs must err on every tensor,
    else the gate would degenerate to the floor.  One tensor cannot: with a single row, the gradient of net.2.bias is the
    incoming gradient itself, exact in any arithmetic -- there e_torch must be exactly 0 (and the gate is the floor)."""
    c = FC.case(name)
    ref = FC.reference(name)
    got = FC.torch_path(c, dtype=torch.float32)
    for key in FC.TENSORS:
        e = FC.rel_err(got[key], ref[key])
        print(f"{name} {key}: e_torch(cpu) = {e:.3e}")
        if sum(c["rows"]) == 1 and key == "cross_attend_blocks.1.fn.net.2.bias":
            assert e == 0.0
        else:
            assert 0.0 < e < 1e-4, (key, e)


def test_case_parameters_are_the_default_initialisation_with_noise_on_the_norms():
    c = FC.case("rows_17")
    sd = dict(c["module"].named_parameters())
    assert list(sd) and set(sd) == set(FC.PARAMS)
    for key in FC.PARAMS:
        if ".norm" in key:
            base = 1.0 if key.endswith("weight") else 0.0
            assert 0 < float((sd[key].detach() - base).abs().max()) < 1.0, key
    from imfnet_amd import ops
    assert tuple(p[0] for p in ops.FUSION_TRAIN_PARAMS) == FC.PARAMS
    assert all(tuple(sd[k].shape) == shape for k, shape in ops.FUSION_TRAIN_PARAMS)


def test_header_declares_and_library_exports_the_symbols():
    from imfnet_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/imfnet_hip.h"
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.imf_fusion_train_chunk_rows() == FC.CHUNK == ops.fusion_train_chunk_rows()
    m = re.search(r"#define\s+IMF_FT_FLAG_STARTS\s+(\d+)", text)
    assert m and int(m.group(1)) == ops.FUSION_TRAIN_FLAG_STARTS
    assert re.search(r"IMF_FT_LN1_G\s*=\s*0", text) and "IMF_FT_NPARAM" in text
    # sizes: 0 for arguments the calls refuse, growing with the rows and with the items
    assert L.imf_fusion_train_saved_bytes(100, 2, 300) > L.imf_fusion_train_saved_bytes(99, 2, 300) > 0
    assert L.imf_fusion_train_saved_bytes(100, 3, 300) > L.imf_fusion_train_saved_bytes(100, 2, 300)
    assert L.imf_fusion_train_workspace_bytes(100, 2, 300) > 0
    assert L.imf_fusion_train_workspace_bytes(2 * FC.CHUNK + 1, 1, 300) > L.imf_fusion_train_workspace_bytes(2 * FC.CHUNK, 1, 300)
    for bad in ((-1, 1, 300), (10, 0, 300), (10, 1, 0), (10, 1, 321)):
        assert L.imf_fusion_train_saved_bytes(*bad) == 0 and L.imf_fusion_train_workspace_bytes(*bad) == 0, bad
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = set(line.split()[-1] for line in nm.stdout.splitlines() if line.strip())
        assert set(SYMBOLS) <= exported


def test_argument_errors_return_a_status_without_a_gpu():
    """Every refusal comes before any device call, so it answers on a machine without a GPU (host pointers here)."""
    import ctypes as C
    from imfnet_amd import _lib
    L = _lib.lib()
    buf = np.zeros(1 << 12, dtype=np.float64)
    p = buf.ctypes.data
    p += (-p) % 16
    good = dict(n=8, n_items=2, T=300, dims=DIMS)
    sbytes, wbytes = L.imf_fusion_train_saved_bytes(8, 2, 300), L.imf_fusion_train_workspace_bytes(8, 2, 300)
    assert sbytes > 0 and wbytes > 0
    FWD = ("x", "item_starts", "tokens", "z", "saved", "meta")
    BWD = ("dz", "x", "item_starts", "tokens", "saved", "meta", "workspace")

    def arrays(null_weight=None, weights=True, misaligned=None):
        w = (C.c_void_p * 14)(*[None if i == null_weight else (p + 4 if i == misaligned else p) for i in range(14)])
        return w if weights else None

    def fwd(null=None, sb=None, wb=None, w=None, **kw):
        a = dict(good, **kw)
        q = {k: (None if k == null else p) for k in FWD}
        return L.imf_fusion_train_forward(q["x"], a["n"], q["item_starts"], a["n_items"], q["tokens"], a["T"], *a["dims"],
                                          arrays() if w is None else w(), q["z"], q["saved"],
                                          sbytes if sb is None else sb, q["meta"], None)

    def bwd(null=None, sb=None, wb=None, w=None, grads=True, **kw):
        a = dict(good, **kw)
        q = {k: (None if k == null else p) for k in BWD}
        g = (C.c_void_p * 14)(*([p] * 14)) if grads else None
        return L.imf_fusion_train_backward(q["dz"], q["x"], a["n"], q["item_starts"], a["n_items"], q["tokens"], a["T"],
                                           *a["dims"], arrays() if w is None else w(), q["saved"],
                                           sbytes if sb is None else sb, p, p, g, q["meta"], q["workspace"],
                                           wbytes if wb is None else wb, None)

    EINVAL = -1
    m = re.search(r"#define\s+IMF_EINVAL\s+(-?\d+)", open(os.path.join(ROOT, "include", "imfnet_hip.h")).read())
    assert m and int(m.group(1)) == EINVAL
    for call, names in ((fwd, FWD), (bwd, BWD)):
        for dims in ((512, 128, 128, 1024), (256, 64, 128, 1024), (256, 128, 64, 1024), (256, 128, 128, 512), (0, 0, 0, 0)):
            assert call(dims=dims) == EINVAL, dims
        assert b"dims" in L.imf_last_error()
        for T in (321, 0, -5, 1 << 20):
            assert call(T=T) == EINVAL, T
        assert b"n_tokens" in L.imf_last_error()
        assert call(n=-1) == EINVAL and call(n_items=0) == EINVAL and call(n=(1 << 22) + 1, sb=1 << 60, wb=1 << 60) == EINVAL
        for null in names:
            assert call(null=null) == EINVAL, null
            assert b"null" in L.imf_last_error()
        assert call(w=lambda: None) == EINVAL
        for i in range(14):
            assert call(w=lambda i=i: arrays(null_weight=i)) == EINVAL, i
            assert b"null" in L.imf_last_error()
        assert call(w=lambda: arrays(misaligned=3)) == EINVAL and b"aligned" in L.imf_last_error()
        assert call(sb=sbytes - 1) == EINVAL and b"saved" in L.imf_last_error()
        assert call(sb=0) == EINVAL
    assert bwd(wb=wbytes - 1) == EINVAL and b"workspace" in L.imf_last_error()
    assert bwd(grads=False) == EINVAL
    # no rows: nothing to launch, success -- before any device call too
    assert fwd(n=0) == 0 and bwd(n=0) == 0


def test_fusion_kernels_option_parses_defaults_to_torch_and_refuses_other_values(capsys):
    from imfnet_amd.train.trainer import make_parser, parse_config
    assert parse_config([]).fusion_kernels == "torch"
    assert parse_config(["--fusion_kernels", "torch"]).fusion_kernels == "torch"
    assert parse_config(["--fusion_kernels", "hip"]).fusion_kernels == "hip"
    for bad in ("HIP", "triton", ""):
        with pytest.raises(SystemExit):
            parse_config(["--fusion_kernels", bad])
    capsys.readouterr()
    assert "--fusion_kernels {torch,hip}" in make_parser().format_help()
    cfg = parse_config(["--fusion_kernels", "hip"])
    assert cfg.norm_kernels == "torch" and cfg.loss_kernels == "torch"
    assert {"voxel_size", "bn_momentum", "seed", "model"} <= set(vars(cfg))


def test_fusion_kernels_lands_in_the_saved_config_and_sets_the_switch(tmp_path):
    from imfnet_amd import ops
    from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config
    prev = ops.TRAIN_FUSION
    try:
        for choice in ("hip", "torch"):
            out = tmp_path / choice
            cfg = parse_config(["--out_dir", str(out), "--fusion_kernels", choice])
            tr = HardestContrastiveTrainer(cfg, None, None, device="cpu")
            tr.pool.shutdown()
            assert ops.TRAIN_FUSION == choice and ops.TRAIN_NORM == "torch" and ops.TRAIN_LOSS == "torch"
            assert json.load(open(out / "config.json"))["fusion_kernels"] == choice
            tr._save(1, "checkpoint")
            ck = torch.load(out / "checkpoint.pth", weights_only=False)
            assert ck["config"]["fusion_kernels"] == choice
    finally:
        ops.TRAIN_FUSION = prev


def test_switch_values_and_the_environment_variable():
    from imfnet_amd import ops
    from imfnet_amd._lib import ImfError
    assert ops.TRAIN_FUSION_CHOICES == ("torch", "hip")
    assert ops.TRAIN_FUSION == os.environ.get("IMF_TRAIN_FUSION", "torch")
    prev = ops.set_train_fusion("hip")
    try:
        assert ops.TRAIN_FUSION == "hip"
        with pytest.raises(ImfError):
            ops.set_train_fusion("cuda")
        assert ops.TRAIN_FUSION == "hip"
    finally:
        ops.set_train_fusion(prev)
    env = {k: v for k, v in os.environ.items() if k != "IMF_TRAIN_FUSION"}
    for value, want in ((None, "torch"), ("hip", "hip"), ("torch", "torch")):
        e = dict(env, PYTHONPATH=ROOT, **({} if value is None else {"IMF_TRAIN_FUSION": value}))
        got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops; print(ops.TRAIN_FUSION)"], env=e,
                             capture_output=True, text=True, cwd=ROOT)
        assert got.returncode == 0 and got.stdout.strip() == want, got.stderr
    e = dict(env, IMF_TRAIN_FUSION="triton", PYTHONPATH=ROOT)
    got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops"], env=e, capture_output=True, text=True,
                         cwd=ROOT)
    assert got.returncode != 0 and "IMF_TRAIN_FUSION" in got.stderr and "ImfError" in got.stderr
    with pytest.raises(ImfError):                                     # the kernels have no CPU twin: CPU rows are an error
        ops.fusion_train_forward(torch.zeros(4, 256), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 300, 128),
                                 [torch.zeros(s) for _, s in ops.FUSION_TRAIN_PARAMS])


def test_cpu_tensors_with_the_switch_at_hip_run_the_torch_body_bit_for_bit():
    """ResUNet2.transformer on CPU tensors: the kernels do not apply, so the switch changes nothing -- output and every
    gradient bit-identical, in training mode under autograd, for one image and for a batch (the host loop)."""
    from imfnet_amd import ops
    from imfnet_amd.model import load_model
    torch.manual_seed(5)
    model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3,
                                      config=None).train()
    g = torch.Generator().manual_seed(6)
    for rows in ((9,), (5, 0, 7)):
        n, B = sum(rows), len(rows)
        images = torch.randn(B, 128, 15, 20, generator=g)
        xyz = torch.zeros(n, 4, dtype=torch.int32)
        xyz[:, 0] = torch.repeat_interleave(torch.arange(B), torch.tensor(rows)).int()
        feat = torch.randn(n, 256, generator=g)
        dz = torch.randn(n, 256, generator=g)
        runs = {}
        for switch in ("torch", "hip"):
            prev = ops.set_train_fusion(switch)
            try:
                model.zero_grad(set_to_none=True)
                F, im = feat.clone().requires_grad_(True), images.clone().requires_grad_(True)
                z = model.transformer(im, F, xyz)
                z.backward(dz)
                runs[switch] = [z.detach(), F.grad, im.grad] + [p.grad.clone() for p in model.attention_fusion.parameters()]
            finally:
                ops.set_train_fusion(prev)
        assert len(runs["hip"]) == 3 + 14
        for a, b in zip(runs["torch"], runs["hip"]):
            assert torch.equal(a, b)
        starts = ops.fusion_item_starts(xyz[:, 0], B)                  # the partition the kernels would be handed
        assert starts.dtype == torch.int32 and starts.tolist() == np.concatenate([[0], np.cumsum(rows)]).tolist()
