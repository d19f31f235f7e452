"""Host side of the descriptor-head training kernels (csrc/head_train.hip): the float64 restatement against torch's float64
autograd of the ops it replaces, the torch fp32 error that the GPU gate is measured against, the C ABI's symbols and their
argument checks, the --head_kernels option and the IMF_TRAIN_HEAD switch, and the predicate that keeps every uncovered
call on the torch ops.  No GPU."""
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import head_restate as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("imf_head_train_chunk_rows", "imf_head_train_workspace_bytes", "imf_head_train_forward",
           "imf_head_train_backward")
DIMS = (64, 32, 64, 32)
EINVAL = -1


def _chunk():
    from imfnet_amd import _lib
    return _lib.lib().imf_head_train_chunk_rows()


def _cases():
    """The GPU tests' row counts, for the chunk size the header documents (checked against the library below)."""
    return HR.row_counts(256)


@pytest.mark.parametrize("n", [1, 33, 257])
@pytest.mark.parametrize("normalize", [True, False])
def test_restatement_matches_torch_float64_autograd_of_the_ops(n, normalize):
    c = HR.case(n)
    ref = HR.reference(n, normalize=normalize)
    want = HR.torch_path(c, dtype=torch.float64, normalize=normalize)
    for key in HR.TENSORS:
        assert ref[key].dtype == np.float64 and ref[key].shape == tuple(want[key].shape), key
        assert np.allclose(want[key].numpy(), ref[key], rtol=1e-12, atol=1e-12), key
        assert HR.rel_err(want[key], ref[key]) <= 1e-12, key


def test_degenerate_masks_are_what_they_say():
    dead, alive = HR.reference(40, "dead"), HR.reference(40, "alive")
    assert not dead["H"].any() and (alive["H"] > 0).all()
    assert not dead["dW1"].any() and not dead["dU"].any() and not dead["dS"].any() and dead["dW2"].shape == (64, 32)
    b = HR.case(40, "dead")["b"].double().numpy()
    assert np.allclose(dead["Y"], np.broadcast_to(b / np.linalg.norm(b), dead["Y"].shape), rtol=0, atol=1e-15)
    assert alive["dW1"].any() and alive["dU"].any()


def test_torch_fp32_error_is_not_zero_so_the_gpu_gate_is_not_its_floor():
    """The GPU gate is e_hip <= 8 * max(e_torch, 2^-24): torch's fp32 run of the same inputs must err on every tensor of
    every case, else the gate would degenerate to the floor."""
    assert _chunk() == 256
    for n in _cases():
        c, ref = HR.case(n), HR.reference(n)
        got = HR.torch_path(c, dtype=torch.float32)
        for key in HR.TENSORS:
            e = HR.rel_err(got[key], ref[key])
            print(f"n={n} {key}: e_torch(cpu) = {e:.3e}")
            assert 0.0 < e < 1e-4, (n, key, e)


def test_row_counts_cover_the_tile_and_chunk_edges_and_stay_within_the_gates_derivation():
    assert HR.row_counts(256) == [1, 31, 33, 255, 256, 257, 529]
    assert HR.row_counts(1024) == [1, 31, 33, 1023, 1024, 1025]          # 2R + 17 beyond the cap is dropped, R + 1 kept
    assert max(HR.row_counts(_chunk())) <= HR.MAX_ROWS == 2048


def test_header_declares_and_library_exports_the_symbols():
    from imfnet_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    m = re.search(r"#define\s+IMF_HT_FLAG_NORM\s+(\d+)", text)
    assert m and int(m.group(1)) == ops.HEAD_TRAIN_FLAG_NORM
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/imfnet_hip.h"
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    R = L.imf_head_train_chunk_rows()
    assert R == ops.head_train_chunk_rows() and R >= 16
    assert ops.HEAD_TRAIN_DIMS == DIMS == (HR.CU, HR.CS, HR.CH, HR.CO)
    # the workspace: 0 for a row count the calls refuse or need nothing for, growing with the rows and with the chunks
    assert L.imf_head_train_workspace_bytes(-1) == 0 and L.imf_head_train_workspace_bytes(0) == 0
    assert L.imf_head_train_workspace_bytes((1 << 22) + 1) == 0
    assert L.imf_head_train_workspace_bytes(100) > L.imf_head_train_workspace_bytes(10) > 0
    assert L.imf_head_train_workspace_bytes(R + 1) - L.imf_head_train_workspace_bytes(R) >= (96 * 64 + 64 * 32) * 4
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = set(line.split()[-1] for line in nm.stdout.splitlines() if line.strip())
        assert set(SYMBOLS) <= exported


def test_argument_errors_return_a_status_without_a_gpu():
    """Every refusal comes before any device call, so it answers on a machine without a GPU (host pointers here)."""
    from imfnet_amd import _lib
    L = _lib.lib()
    m = re.search(r"#define\s+IMF_EINVAL\s+(-?\d+)", open(os.path.join(ROOT, "include", "imfnet_hip.h")).read())
    assert m and int(m.group(1)) == EINVAL
    buf = np.zeros(1 << 12, dtype=np.float64)
    p = buf.ctypes.data
    p += (-p) % 16
    n = 8
    wbytes = L.imf_head_train_workspace_bytes(n)
    FWD = ("u", "s", "w1", "w2", "bias", "h", "r", "y", "meta")
    BWD = ("dy", "y", "r", "h", "u", "s", "w1", "w2", "workspace", "meta")

    def fwd(null=None, dims=DIMS, n=n, normalize=1, off=None):
        q = {k: (None if k == null else p + (4 if k == off else 0)) for k in FWD}
        cu, cs, ch, co = dims
        return L.imf_head_train_forward(q["u"], cu, q["s"], cs, n, q["w1"], ch, q["w2"], co, q["bias"], normalize, q["h"],
                                        q["r"], q["y"], q["meta"], None)

    def bwd(null=None, dims=DIMS, n=n, normalize=1, wb=None, off=None):
        q = {k: (None if k == null else p + (4 if k == off else 0)) for k in BWD}
        cu, cs, ch, co = dims
        return L.imf_head_train_backward(q["dy"], q["y"], q["r"], q["h"], q["u"], cu, q["s"], cs, n, q["w1"], ch, q["w2"], co,
                                         normalize, p, p, p, p, p, q["workspace"], wbytes if wb is None else wb, q["meta"],
                                         None)

    for call, names in ((fwd, FWD), (bwd, BWD)):
        for dims in ((48, 32, 64, 32), (64, 64, 64, 32), (64, 32, 32, 32), (64, 32, 64, 16), (0, 0, 0, 0)):
            assert call(dims=dims) == EINVAL, dims
            assert b"channels" in L.imf_last_error()
        assert call(n=-1) == EINVAL and b"n=-1" in L.imf_last_error()
        assert call(n=(1 << 22) + 1) == EINVAL
        for null in names:
            assert call(null=null) == EINVAL, null
            assert b"null" in L.imf_last_error()
        for off in ("w1", "w2"):
            assert call(off=off) == EINVAL and b"aligned" in L.imf_last_error()
    assert bwd(wb=wbytes - 1) == EINVAL and b"workspace" in L.imf_last_error()
    assert bwd(wb=0) == EINVAL
    assert bwd(off="dy") == EINVAL and b"aligned" in L.imf_last_error()
    # no rows: the forward has nothing to launch and looks at no pointer
    assert fwd(n=0) == 0 and fwd(n=0, null="u") == 0
    assert fwd(n=0, dims=(48, 32, 64, 32)) == EINVAL


def test_head_kernels_option_parses_defaults_to_torch_and_refuses_other_values(capsys):
    from imfnet_amd.train.trainer import make_parser, parse_config
    assert parse_config([]).head_kernels == "torch"
    assert parse_config(["--head_kernels", "torch"]).head_kernels == "torch"
    assert parse_config(["--head_kernels", "hip"]).head_kernels == "hip"
    for bad in ("HIP", "triton", ""):
        with pytest.raises(SystemExit):
            parse_config(["--head_kernels", bad])
    capsys.readouterr()
    assert "--head_kernels {torch,hip}" in make_parser().format_help()
    cfg = parse_config(["--head_kernels", "hip"])
    assert (cfg.norm_kernels, cfg.loss_kernels, cfg.fusion_kernels, cfg.image_kernels, cfg.optim_kernels) == ("torch",) * 5


def test_head_kernels_lands_in_the_saved_config_and_sets_the_switch(tmp_path):
    from imfnet_amd import ops
    from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config
    prev = ops.TRAIN_HEAD
    try:
        for choice in ("hip", "torch"):
            out = tmp_path / choice
            cfg = parse_config(["--out_dir", str(out), "--head_kernels", choice])
            tr = HardestContrastiveTrainer(cfg, None, None, device="cpu")
            tr.pool.shutdown()
            assert ops.TRAIN_HEAD == choice
            assert (ops.TRAIN_NORM, ops.TRAIN_LOSS, ops.TRAIN_FUSION, ops.TRAIN_IMAGE, ops.TRAIN_OPTIM) == ("torch",) * 5
            assert json.load(open(out / "config.json"))["head_kernels"] == choice
            tr._save(1, "checkpoint")
            ck = torch.load(out / "checkpoint.pth", weights_only=False)
            assert ck["config"]["head_kernels"] == choice and "head_kernels" not in ck
    finally:
        ops.TRAIN_HEAD = prev


def test_switch_values_and_the_environment_variable():
    from imfnet_amd import ops
    from imfnet_amd._lib import ImfError
    assert ops.TRAIN_HEAD_CHOICES == ("torch", "hip")
    assert ops.TRAIN_HEAD == os.environ.get("IMF_TRAIN_HEAD", "torch")
    prev = ops.set_train_head("hip")
    try:
        assert ops.TRAIN_HEAD == "hip"
        with pytest.raises(ImfError):
            ops.set_train_head("cuda")
        assert ops.TRAIN_HEAD == "hip"
    finally:
        ops.set_train_head(prev)
    env = {k: v for k, v in os.environ.items() if k != "IMF_TRAIN_HEAD"}
    for value, want in ((None, "torch"), ("hip", "hip"), ("torch", "torch")):
        e = dict(env, PYTHONPATH=ROOT, **({} if value is None else {"IMF_TRAIN_HEAD": value}))
        got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops; print(ops.TRAIN_HEAD)"], env=e,
                             capture_output=True, text=True, cwd=ROOT)
        assert got.returncode == 0 and got.stdout.strip() == want, got.stderr
    e = dict(env, IMF_TRAIN_HEAD="triton", PYTHONPATH=ROOT)
    got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops"], env=e, capture_output=True, text=True,
                         cwd=ROOT)
    assert got.returncode != 0 and "IMF_TRAIN_HEAD" in got.stderr and "ImfError" in got.stderr
    c = HR.case(4)
    with pytest.raises(ImfError):                                     # the kernels have no CPU twin: CPU rows are an error
        ops.head_train_forward(c["U"], c["S"], c["W1"], c["W2"], c["b"])


def _rows(model, n=5, cu=64, cs=32):
    key = object()
    return (types.SimpleNamespace(F=torch.randn(n, cu), coordinate_map_key=key),
            types.SimpleNamespace(F=torch.randn(n, cs), coordinate_map_key=key))


def test_predicate_is_false_for_everything_the_kernels_do_not_cover():
    """With the switch at hip: CPU rows, eval mode, no_grad and ResUNetBN2 (conv1_tr 96 -> 32) all stay on the torch ops;
    with the switch at torch the predicate is false whatever else holds."""
    from imfnet_amd import ops
    from imfnet_amd.model import load_model
    make = lambda name: load_model(name)(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3,  # noqa: E731
                                         config=None)
    m = make("ResUNetBN2C").train()
    assert tuple(m.conv1_tr.kernel.shape) == (96, 64) and tuple(m.final.kernel.shape) == (64, 32)
    assert m.conv1_tr.bias is None and tuple(m.final.bias.shape) == (1, 32)
    small = make("ResUNetBN2").train()
    assert tuple(small.conv1_tr.kernel.shape) == (96, 32)
    prev = ops.set_train_head("hip")
    try:
        assert m._head_kernels_apply(*_rows(m)) is False                # CPU tensors
        assert m.eval()._head_kernels_apply(*_rows(m)) is False
        m.train()
        with torch.no_grad():
            assert m._head_kernels_apply(*_rows(m)) is False
        assert small._head_kernels_apply(*_rows(small)) is False
    finally:
        ops.set_train_head(prev)
    if ops.TRAIN_HEAD == "torch":
        assert m._head_kernels_apply(*_rows(m)) is False
