"""Host side of the hardest-contrastive loss kernels (csrc/loss.hip): the float64 restatement against torch's float64
autograd of upstream's literal formula (full pdist matrices, .min(1), np.isin masks), the all-masked case, the
--loss_kernels option and the IMF_TRAIN_LOSS switch, the C ABI's three symbols and their argument checks.  No GPU."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import loss_restate as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("imf_hc_loss_workspace_bytes", "imf_hc_loss_forward", "imf_hc_loss_backward")
POS_THRESH, NEG_THRESH = 0.1, 1.4


def _unit_rows(g, n, c):
    x = g.normal(size=(n, c))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def _literal(F0, F1, pairs, sel0, sel1, pos_sel, pos_thresh, neg_thresh):
    """lib/trainer.py:440-493 in torch float64 with the full pdist matrices and .min(1)."""
    def pdist(A, B):
        return torch.sqrt(((A.unsqueeze(1) - B.unsqueeze(0)) ** 2).sum(2) + 1e-7)
    hs = max(len(F0), len(F1))
    sp = pairs[pos_sel]
    posF0, posF1 = F0[torch.as_tensor(sp[:, 0])], F1[torch.as_tensor(sp[:, 1])]
    D01min, D01ind = pdist(posF0, F1[torch.as_tensor(sel1)]).min(1)
    D10min, D10ind = pdist(posF1, F0[torch.as_tensor(sel0)]).min(1)
    pos_keys = pairs[:, 0] + pairs[:, 1] * hs
    D01ind, D10ind = sel1[D01ind.numpy()], sel0[D10ind.numpy()]
    mask0 = torch.from_numpy(~np.isin(sp[:, 0] + D01ind * hs, pos_keys))
    mask1 = torch.from_numpy(~np.isin(D10ind + sp[:, 1] * hs, pos_keys))
    pos_loss = torch.relu((posF0 - posF1).pow(2).sum(1) - pos_thresh)
    neg0 = torch.relu(neg_thresh - D01min[mask0]).pow(2)
    neg1 = torch.relu(neg_thresh - D10min[mask1]).pow(2)
    return pos_loss.mean(), (neg0.mean() + neg1.mean()) / 2, D01ind, D10ind, mask0.numpy(), mask1.numpy()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("n0,n1,n_pos,n_sel", [(40, 37, 25, 9), (300, 280, 128, 64)])
def test_restatement_matches_torch_float64_autograd_of_the_literal_formula(n0, n1, n_pos, n_sel):
    g = np.random.default_rng(100 * n0 + n_pos)
    f0, f1 = _unit_rows(g, n0, 32), _unit_rows(g, n1, 32)
    P0 = 2 * n_pos
    pairs = np.stack([g.integers(0, n0, P0), g.integers(0, n1, P0)], 1)
    sel0, sel1 = g.choice(n0, n_sel, replace=False), g.choice(n1, n_sel, replace=False)
    pos_sel = g.choice(P0, n_pos, replace=False)
    # some hardest negatives made positives (the mask must drop them): pairs appended after the sample
    first = LR.restate(f0, f1, pairs, sel0, sel1, pos_sel, POS_THRESH, NEG_THRESH)
    sp, q = pairs[pos_sel], n_pos // 4
    extra = np.concatenate([np.stack([sp[:q, 0], first["hard01"][:q]], 1),
                            np.stack([first["hard10"][q:2 * q], sp[q:2 * q, 1]], 1)])
    pairs = np.concatenate([pairs, extra])

    t0 = torch.from_numpy(f0).double().requires_grad_(True)
    t1 = torch.from_numpy(f1).double().requires_grad_(True)
    rp, rn, d01, d10, m0, m1 = _literal(t0, t1, pairs, sel0, sel1, pos_sel, POS_THRESH, NEG_THRESH)
    gp, gn = 0.75, 1.5
    (gp * rp + gn * rn).backward()
    got = LR.restate(f0, f1, pairs, sel0, sel1, pos_sel, POS_THRESH, NEG_THRESH, grad=(gp, gn))
    assert int((~m0).sum()) >= q and int((~m1).sum()) >= q
    assert np.array_equal(got["hard01"], d01) and np.array_equal(got["hard10"], d10)
    assert np.array_equal(got["keep01"], m0) and np.array_equal(got["keep10"], m1)
    assert got["count01"] == int(m0.sum()) and got["count10"] == int(m1.sum())
    assert abs(got["pos_loss"] - float(rp.detach())) <= 1e-12 * abs(float(rp.detach())) and float(rp.detach()) > 0
    assert abs(got["neg_loss"] - float(rn.detach())) <= 1e-12 * abs(float(rn.detach())) and float(rn.detach()) > 0
    assert _rel(got["df0"], t0.grad.numpy()) <= 1e-12 and _rel(got["df1"], t1.grad.numpy()) <= 1e-12
    assert (got["abs_terms0"] >= np.abs(got["df0"]) * (1 - 1e-12)).all()
    assert (got["abs_terms1"] >= np.abs(got["df1"]) * (1 - 1e-12)).all()
    assert not got["df0"][~got["touched0"]].any() and not got["abs_terms0"][~got["touched0"]].any()
    # pos_sel None is every pair in order
    every = LR.restate(f0, f1, pairs, sel0, sel1, None, POS_THRESH, NEG_THRESH)
    same = LR.restate(f0, f1, pairs, sel0, sel1, np.arange(len(pairs)), POS_THRESH, NEG_THRESH)
    assert every["pos_loss"] == same["pos_loss"] and np.array_equal(every["df1"], same["df1"])


def test_an_empty_keep_set_gives_a_nan_loss_and_no_gradient_from_that_half():
    """sel1 is one row and every (i_s, that row) is a positive pair: keep01 is empty.  torch's mean of nothing is NaN and
    its gradient is nothing; the 10 half and the positive term still send theirs."""
    g = np.random.default_rng(8)
    n0, n1, n_pos = 30, 28, 12
    f0, f1 = _unit_rows(g, n0, 16), _unit_rows(g, n1, 16)
    sel0, sel1 = g.choice(n0, 7, replace=False), np.array([5])
    sampled = np.stack([g.integers(0, n0, n_pos), g.integers(0, n1, n_pos)], 1)
    pairs = np.concatenate([sampled, np.stack([sampled[:, 0], np.full(n_pos, 5)], 1)])
    pos_sel = np.arange(n_pos)
    got = LR.restate(f0, f1, pairs, sel0, sel1, pos_sel, POS_THRESH, NEG_THRESH)
    assert got["count01"] == 0 and not got["keep01"].any() and got["count10"] > 0
    assert np.isnan(got["neg_loss"]) and np.isfinite(got["pos_loss"])
    assert np.isfinite(got["df0"]).all() and np.isfinite(got["df1"]).all() and got["df0"].any() and got["df1"].any()

    t0 = torch.from_numpy(f0).double().requires_grad_(True)
    t1 = torch.from_numpy(f1).double().requires_grad_(True)
    rp, rn, _, _, m0, m1 = _literal(t0, t1, pairs, sel0, sel1, pos_sel, POS_THRESH, NEG_THRESH)
    assert not m0.any() and torch.isnan(rn)
    (rp + rn).backward()
    assert _rel(got["df0"], t0.grad.numpy()) <= 1e-12 and _rel(got["df1"], t1.grad.numpy()) <= 1e-12
    # the same gradient as the loss without the 01 half (times the half's 1/2)
    u0 = torch.from_numpy(f0).double().requires_grad_(True)
    u1 = torch.from_numpy(f1).double().requires_grad_(True)
    sp = torch.as_tensor(sampled)
    a, b, h = u0[sp[:, 0]], u1[sp[:, 1]], u0[torch.as_tensor(got["hard10"])]
    d10 = torch.sqrt((b - h).pow(2).sum(1) + 1e-7)[torch.from_numpy(got["keep10"])]
    (torch.relu((a - b).pow(2).sum(1) - POS_THRESH).mean() + torch.relu(NEG_THRESH - d10).pow(2).mean() / 2).backward()
    assert _rel(got["df0"], u0.grad.numpy()) <= 1e-12 and _rel(got["df1"], u1.grad.numpy()) <= 1e-12


def test_min_gap_counts_bit_identical_rows_once():
    db = np.array([[0, 0], [1, 0], [1, 0], [3, 0]], dtype=np.float32)
    q = np.array([[0.9, 0.0]], dtype=np.float32)
    d2 = LR.dist2_matrix(q.astype(np.float64), db.astype(np.float64))
    assert abs(LR.min_gap(d2, db) - (0.81 - 0.01)) < 1e-6
    assert LR.min_gap(d2[:, 1:3], db[1:3]) == np.inf


def test_header_declares_and_library_exports_the_three_symbols():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/imfnet_hip.h"
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = set(line.split()[-1] for line in nm.stdout.splitlines() if line.strip())
        assert set(SYMBOLS) <= exported
    ws = L.imf_hc_loss_workspace_bytes
    base = ws(3000, 2800, 32, 4120, 2048, 512, 512)
    assert base > 0 and ws(3000, 2800, 32, 4120, 4096, 512, 512) > base and ws(1, 1, 16, 1, 1, 1, 1) > 0
    assert ws(10 ** 6, 10 ** 6, 64, 1 << 20, 8192, 4096, 4096) > 0          # the sizes the caps must admit
    for bad in ((3000, 2800, 8, 4120, 2048, 512, 512), (3000, 2800, 32, 0, 2048, 512, 512),
                (3000, 2800, 32, 4120, 0, 512, 512), (3000, 2800, 32, 4120, 2048, 0, 512),
                (3000, 2800, 32, 4120, 2048, 512, 0), (3000, 2800, 32, 4120, (1 << 16) + 1, 512, 512)):
        assert ws(*bad) == 0, bad


def test_argument_errors_return_a_status_without_a_gpu():
    """Every refusal comes before any device call, so it answers on a machine without a GPU (host pointers here)."""
    from imfnet_amd import _lib
    L = _lib.lib()
    buf = np.zeros(1 << 16, dtype=np.float64)
    p = buf.ctypes.data
    p += (-p) % 16
    good = dict(n0=8, n1=8, c=32, n_pairs=6, n_pos=4, n_sel0=3, n_sel1=3)
    nbytes = L.imf_hc_loss_workspace_bytes(*good.values())
    assert 0 < nbytes

    def fwd(ws=None, null=None, pos_sel=p, **kw):
        a = dict(good, **kw)
        ptr = {k: (None if k == null else p) for k in ("f0", "f1", "pairs", "sel0", "sel1", "loss", "hard01", "hard10",
                                                       "keep01", "keep10", "meta", "workspace")}
        return L.imf_hc_loss_forward(ptr["f0"], a["n0"], ptr["f1"], a["n1"], a["c"], ptr["pairs"], a["n_pairs"], pos_sel,
                                     a["n_pos"], ptr["sel0"], a["n_sel0"], ptr["sel1"], a["n_sel1"], POS_THRESH,
                                     NEG_THRESH, ptr["loss"], ptr["hard01"], ptr["hard10"], ptr["keep01"], ptr["keep10"],
                                     ptr["meta"], ptr["workspace"], nbytes if ws is None else ws, None)

    def bwd(ws=None, null=None, pos_sel=p, **kw):
        a = dict(good, **kw)
        ptr = {k: (None if k == null else p) for k in ("f0", "f1", "pairs", "sel0", "sel1", "hard01", "hard10", "keep01",
                                                       "keep10", "meta", "grad", "df0", "df1", "workspace")}
        return L.imf_hc_loss_backward(ptr["f0"], a["n0"], ptr["f1"], a["n1"], a["c"], ptr["pairs"], a["n_pairs"], pos_sel,
                                      a["n_pos"], ptr["sel0"], a["n_sel0"], ptr["sel1"], a["n_sel1"], POS_THRESH,
                                      NEG_THRESH, ptr["hard01"], ptr["hard10"], ptr["keep01"], ptr["keep10"], ptr["meta"],
                                      ptr["grad"], ptr["df0"], ptr["df1"], ptr["workspace"], nbytes if ws is None else ws,
                                      None)

    EINVAL, EUNSUPPORTED = -1, -3
    for name, code in (("IMF_EINVAL", EINVAL), ("IMF_EUNSUPPORTED", EUNSUPPORTED)):
        m = re.search(r"#define\s+%s\s+(-?\d+)" % name, open(os.path.join(ROOT, "include", "imfnet_hip.h")).read())
        assert m and int(m.group(1)) == code, name
    for call, nulls in ((fwd, ("f0", "f1", "pairs", "sel0", "sel1", "loss", "hard01", "hard10", "keep01", "keep10", "meta",
                               "workspace")),
                        (bwd, ("f0", "f1", "pairs", "sel0", "sel1", "hard01", "hard10", "keep01", "keep10", "meta", "grad",
                               "df0", "df1", "workspace"))):
        for c in (0, 8, 24, 48, 128):
            assert call(c=c) == EINVAL, c
        assert b"{16,32,64}" in L.imf_last_error()
        for key in ("n_pos", "n_sel0", "n_sel1", "n_pairs"):
            assert call(**{key: 0}) == EINVAL and call(**{key: -3}) == EINVAL, key
        assert call(ws=nbytes - 1) == EINVAL
        assert b"workspace" in L.imf_last_error()
        assert call(ws=0) == EINVAL
        for null in nulls:
            assert call(null=null) == EINVAL, null
        assert b"null" in L.imf_last_error()
        assert call(pos_sel=None) == EINVAL                            # NULL takes every pair: n_pos must be n_pairs
        assert call(n_pos=(1 << 16) + 1, n_pairs=1 << 17, ws=1 << 40) == EUNSUPPORTED
        assert call(n_pairs=(1 << 26) + 1, ws=1 << 40) == EUNSUPPORTED


def test_loss_kernels_option_parses_defaults_to_torch_and_refuses_other_values(capsys):
    from imfnet_amd.train.trainer import make_parser, parse_config
    assert parse_config([]).loss_kernels == "torch"
    assert parse_config(["--loss_kernels", "torch"]).loss_kernels == "torch"
    assert parse_config(["--loss_kernels", "hip"]).loss_kernels == "hip"
    for bad in ("HIP", "triton", ""):
        with pytest.raises(SystemExit):
            parse_config(["--loss_kernels", bad])
    capsys.readouterr()
    assert "--loss_kernels {torch,hip}" in make_parser().format_help()
    cfg = parse_config(["--loss_kernels", "hip"])
    assert cfg.norm_kernels == "torch" and {"voxel_size", "bn_momentum", "seed", "model"} <= set(vars(cfg))
    with pytest.raises(SystemExit):                                   # the other trainers stay refused
        parse_config(["--loss_kernels", "hip", "--trainer", "TripletLossTrainer"])


def test_loss_kernels_lands_in_the_saved_config_and_sets_the_switch(tmp_path):
    from imfnet_amd import ops
    from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config
    prev = ops.TRAIN_LOSS
    try:
        for choice in ("hip", "torch"):
            out = tmp_path / choice
            cfg = parse_config(["--out_dir", str(out), "--loss_kernels", choice])
            tr = HardestContrastiveTrainer(cfg, None, None, device="cpu")
            tr.pool.shutdown()
            assert ops.TRAIN_LOSS == choice and ops.TRAIN_NORM == "torch"
            assert json.load(open(out / "config.json"))["loss_kernels"] == choice
            tr._save(1, "checkpoint")
            ck = torch.load(out / "checkpoint.pth", weights_only=False)
            assert ck["config"]["loss_kernels"] == choice
    finally:
        ops.TRAIN_LOSS = prev


def test_switch_values_and_the_keyword():
    from imfnet_amd import ops
    from imfnet_amd._lib import ImfError
    from imfnet_amd.train.loss import hardest_contrastive_loss
    assert ops.TRAIN_LOSS_CHOICES == ("torch", "hip") and ops.TRAIN_LOSS == os.environ.get("IMF_TRAIN_LOSS", "torch")
    prev = ops.set_train_loss("hip")
    try:
        assert ops.TRAIN_LOSS == "hip"
        with pytest.raises(ImfError):
            ops.set_train_loss("cuda")
        assert ops.TRAIN_LOSS == "hip"
    finally:
        ops.set_train_loss(prev)
    for value, want in (("hip", "hip"), ("torch", "torch")):
        env = dict(os.environ, IMF_TRAIN_LOSS=value, PYTHONPATH=ROOT)
        got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops; print(ops.TRAIN_LOSS)"], env=env,
                             capture_output=True, text=True, cwd=ROOT)
        assert got.returncode == 0 and got.stdout.strip() == want, got.stderr
    env = dict(os.environ, IMF_TRAIN_LOSS="triton", PYTHONPATH=ROOT)
    got = subprocess.run([os.sys.executable, "-c", "from imfnet_amd import ops"], env=env, capture_output=True, text=True,
                         cwd=ROOT)
    assert got.returncode != 0 and "IMF_TRAIN_LOSS" in got.stderr and "ImfError" in got.stderr
    x = torch.zeros(4, 32)
    with pytest.raises(ImfError):                                     # an unknown value is refused before any work
        hardest_contrastive_loss(x, x, torch.zeros(3, 2, dtype=torch.int64), kernels="triton")
    with pytest.raises(ImfError):                                     # the hip path has no CPU twin: CPU rows are an error
        hardest_contrastive_loss(x, x, torch.zeros(3, 2, dtype=torch.int64), num_pos=8, kernels="hip",
                                 sel0=np.arange(2), sel1=np.arange(2))
