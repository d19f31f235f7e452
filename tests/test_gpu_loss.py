"""The hardest-contrastive loss kernels on the GPU (csrc/loss.hip, autograd.HardestContrastiveLossFunction,
train/loss.py kernels="hip", the trainer's --loss_kernels hip) against the float64 restatement tests/loss_restate.py.

The gates are derived, not measured: indices, masks and counts are exact; each loss is a sum of non-negative fp64 terms
rounded once to fp32, so |loss - exact| <= 2^-23 |exact|; each gradient element is one fp64 sum of its addends rounded
once, so |got - exact| <= 2^-23 * sum |addends|; a row without a term is +0.0; two calls give the same bits.
The inputs must keep the decisions away from rounding, and every case asserts that from the restatement: the two nearest
distinct database rows of every query differ by more than 1e-12 in squared distance, and no |a - b|^2 is within 1e-9 of
pos_thresh (seeded unit Gaussian rows are far from both: gaps of 1e-6 and more)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_restate as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
POS_THRESH, NEG_THRESH = 0.1, 1.4
U = 2.0 ** -23


def _unit_rows(g, n, c):
    x = g.normal(size=(n, c))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


# name: (seed, n0, n1, c, n_pairs, n_pos (None: pos_sel = NULL, every pair), n_sel0, n_sel1, flavour)
CASES = {
    "smallest": (1, 1, 2, 16, 3, 1, 1, 1, None),
    "one_sel0_row": (2, 63, 64, 32, 100, 63, 1, 64, None),                 # one row of f0 collects every 10 term
    "all_pairs": (3, 65, 257, 64, 65, None, 64, 64, None),                 # pos_sel = NULL
    "one_i": (4, 3001, 3001, 32, 3000, 2048, 512, 64, "one_i"),             # every sampled pair shares its row of f0
    "masked_and_tied": (5, 3001, 3001, 32, 4000, 2048, 512, 512, "masked_and_tied"),
    "empty_keep01": (6, 257, 2, 16, 200, 63, 64, 1, "empty_keep01"),
    "wide": (7, 257, 3001, 64, 2500, 2048, 64, 512, "close"),                  # some positive hinges closed
    "odd": (8, 64, 65, 16, 300, 65, 64, 1, None),
}


def make_case(name):
    """(f0, f1, pairs, sel0, sel1, pos_sel) as NumPy arrays, float32 rows and int64 indices."""
    seed, n0, n1, c, n_pairs, n_pos, n_sel0, n_sel1, flavour = CASES[name]
    g = np.random.default_rng(seed)
    f0, f1 = _unit_rows(g, n0, c), _unit_rows(g, n1, c)
    pairs = np.stack([g.integers(0, n0, n_pairs), g.integers(0, n1, n_pairs)], 1)   # with replacement: rows repeat
    sel0, sel1 = g.choice(n0, n_sel0, replace=False), g.choice(n1, n_sel1, replace=False)
    pos_sel = None if n_pos is None else g.choice(n_pairs, n_pos, replace=False)
    if flavour == "one_i":
        pairs[:, 0] = 17
        # one anchor row has one hardest negative; keep that pair out of the positives, or keep01 would be empty
        h = LR.restate(f0, f1, pairs, sel0, sel1, pos_sel, POS_THRESH, NEG_THRESH)["hard01"][0]
        pairs[pairs[:, 1] == h, 1] = (h + 1) % n1
    elif flavour == "masked_and_tied":
        sp = pairs[pos_sel]
        # two bit-identical rows inside sel1 (k = 3 and k = 7), the nearest of sample 0: the tie goes to k = 3
        f1[sel1[3]] = f1[sel1[7]] = (f0[sp[0, 0]] * np.float32(0.99)).astype(np.float32)
        # 60 hardest negatives made positives on each side: pairs appended after the sample
        r = LR.restate(f0, f1, pairs, sel0, sel1, pos_sel, POS_THRESH, NEG_THRESH)
        extra = np.concatenate([np.stack([sp[100:160, 0], r["hard01"][100:160]], 1),
                                np.stack([r["hard10"][160:220], sp[160:220, 1]], 1)])
        pairs = np.concatenate([pairs, extra])
    elif flavour == "close":
        sp = pairs[pos_sel][:300]
        noise = g.normal(size=(300, c))
        f1[sp[:, 1]] = f0[sp[:, 0]] + (0.2 * noise / np.linalg.norm(noise, axis=1, keepdims=True)).astype(np.float32)
    elif flavour == "empty_keep01":
        sp = pairs[pos_sel]
        pairs = np.concatenate([pairs, np.stack([sp[:, 0], np.full(len(sp), sel1[0])], 1)])
    return f0, f1, pairs.astype(np.int64), sel0.astype(np.int64), sel1.astype(np.int64), pos_sel


_REF = {}


def reference(name):
    """The case and its restatement (gradients for upstream (1, 1)), computed once and shared."""
    if name not in _REF:
        case = make_case(name)
        _REF[name] = (case, LR.restate(*case, POS_THRESH, NEG_THRESH))
    return _REF[name]


def _dev(case):
    f0, f1, pairs, sel0, sel1, pos_sel = case
    t = lambda a: None if a is None else torch.as_tensor(a).to(DEV)
    return t(f0), t(f1), t(pairs), t(pos_sel), t(sel0), t(sel1)


def _check_conditions(case, ref):
    f0, f1, pairs, sel0, sel1, pos_sel = case
    assert LR.min_gap(ref["dist2_01"], f1[sel1]) > 1e-12 and LR.min_gap(ref["dist2_10"], f0[sel0]) > 1e-12
    assert np.abs(ref["d2_pos"] - POS_THRESH).min() > 1e-9


def _check_loss(got, exact):
    print("loss", got, "exact", exact, "bound", U * abs(exact))
    if np.isnan(exact):
        assert np.isnan(got)
    else:
        assert abs(float(got) - exact) <= U * abs(exact)


def _check_grad(got, exact, abs_terms, touched, side):
    got = got.cpu().numpy()
    err = np.abs(got.astype(np.float64) - exact)
    worst = float((err / np.maximum(abs_terms, 1e-300)).max()) if abs_terms.any() else 0.0
    print(f"df{side}: max |got - exact| / sum|addends| = {worst:.3e} (bound {U:.3e}), {int(touched.sum())} rows touched")
    assert (err <= U * abs_terms).all()
    untouched = got[~touched]
    assert not untouched.any() and not np.signbit(untouched).any()          # exactly +0.0


@pytest.mark.parametrize("name", list(CASES))
def test_ops_forward_and_backward_against_the_restatement(name):
    from imfnet_amd import ops
    case, ref = reference(name)
    _check_conditions(case, ref)
    f0, f1, pairs, pos_sel, sel0, sel1 = _dev(case)
    loss, hard01, hard10, keep01, keep10, meta = ops.hc_loss_forward(f0, f1, pairs, pos_sel, sel0, sel1, POS_THRESH,
                                                                     NEG_THRESH)
    assert np.array_equal(hard01.cpu().numpy(), ref["hard01"]) and np.array_equal(hard10.cpu().numpy(), ref["hard10"])
    assert np.array_equal(keep01.cpu().numpy().astype(bool), ref["keep01"])
    assert np.array_equal(keep10.cpu().numpy().astype(bool), ref["keep10"])
    flags = (1 if ref["count01"] == 0 else 0) | (2 if ref["count10"] == 0 else 0)
    assert meta.cpu().tolist() == [ref["count01"], ref["count10"], flags, 0]
    host = loss.cpu().numpy()
    _check_loss(host[0], ref["pos_loss"])
    _check_loss(host[1], ref["neg_loss"])
    grad = torch.ones(2, dtype=torch.float32, device=DEV)
    df0 = torch.full_like(f0, float("nan"))
    df1 = torch.full_like(f1, float("nan"))
    out = ops.hc_loss_backward(f0, f1, pairs, pos_sel, sel0, sel1, POS_THRESH, NEG_THRESH, hard01, hard10, keep01, keep10,
                               meta, grad, df0=df0, df1=df1)
    assert out[0] is df0 and out[1] is df1
    _check_grad(df0, ref["df0"], ref["abs_terms0"], ref["touched0"], 0)
    _check_grad(df1, ref["df1"], ref["abs_terms1"], ref["touched1"], 1)


def test_the_flavours_are_what_they_claim():
    """The cases' special shapes, read from the restatement."""
    case, ref = reference("masked_and_tied")
    f0, f1, pairs, sel0, sel1, pos_sel = case
    assert np.array_equal(f1[sel1[3]], f1[sel1[7]]) and ref["hard01"][0] == sel1[3]
    assert ref["dist2_01"][0, 3] == ref["dist2_01"][0, 7] == ref["dist2_01"][0].min()
    assert int((~ref["keep01"]).sum()) >= 60 and int((~ref["keep10"]).sum()) >= 60
    case, ref = reference("empty_keep01")
    assert ref["count01"] == 0 and ref["count10"] > 0 and np.isnan(ref["neg_loss"]) and ref["df0"].any()
    case, ref = reference("one_i")
    assert int(ref["touched0"].sum()) <= 1 + 512 and ref["abs_terms0"][17].all() and ref["count01"] > 0
    case, ref = reference("wide")
    closed = int((ref["d2_pos"] < POS_THRESH).sum())
    assert 100 <= closed <= 400 and ref["count01"] > 0 and ref["count10"] > 0
    case, ref = reference("one_sel0_row")
    assert len(np.unique(ref["hard10"])) == 1
    assert reference("all_pairs")[0][5] is None


def test_upstream_gradients_are_read_on_the_device_and_scale_the_two_parts():
    """grad = (0.5, -2): the closed form with those two scalars, within the same bound."""
    from imfnet_amd import ops
    case, _ = reference("odd")
    ref = LR.restate(*case, POS_THRESH, NEG_THRESH, grad=(0.5, -2.0))
    f0, f1, pairs, pos_sel, sel0, sel1 = _dev(case)
    fw = ops.hc_loss_forward(f0, f1, pairs, pos_sel, sel0, sel1, POS_THRESH, NEG_THRESH)
    grad = torch.tensor([0.5, -2.0], dtype=torch.float32, device=DEV)
    df0, df1 = ops.hc_loss_backward(f0, f1, pairs, pos_sel, sel0, sel1, POS_THRESH, NEG_THRESH, *fw[1:], grad)
    _check_grad(df0, ref["df0"], ref["abs_terms0"], ref["touched0"], 0)
    _check_grad(df1, ref["df1"], ref["abs_terms1"], ref["touched1"], 1)


def test_two_calls_give_the_same_bits():
    from imfnet_amd import ops
    case, _ = reference("masked_and_tied")
    f0, f1, pairs, pos_sel, sel0, sel1 = _dev(case)
    grad = torch.tensor([1.0, 0.75], dtype=torch.float32, device=DEV)
    runs = []
    for _ in range(2):
        fw = ops.hc_loss_forward(f0, f1, pairs, pos_sel, sel0, sel1, POS_THRESH, NEG_THRESH)
        bw = ops.hc_loss_backward(f0, f1, pairs, pos_sel, sel0, sel1, POS_THRESH, NEG_THRESH, *fw[1:], grad)
        runs.append(tuple(fw) + tuple(bw))
    assert len(runs[0]) == 8
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][0]).all() and runs[0][6].any()


@pytest.mark.parametrize("name", ["masked_and_tied", "all_pairs", "empty_keep01"])
def test_hardest_contrastive_loss_with_hip_kernels_against_the_restatement(name):
    """Through train/loss.py and autograd: (pos + neg).backward() is the closed form for upstream (1, 1)."""
    from imfnet_amd.train.loss import hardest_contrastive_loss
    case, ref = reference(name)
    f0, f1, pairs, sel0, sel1, pos_sel = case
    g0 = torch.as_tensor(f0).to(DEV).requires_grad_(True)
    g1 = torch.as_tensor(f1).to(DEV).requires_grad_(True)
    n_pos = len(pairs) if pos_sel is None else len(pos_sel)
    pos, neg, d01, d10 = hardest_contrastive_loss(g0, g1, torch.as_tensor(pairs.astype(np.int32)).to(DEV), num_pos=n_pos,
                                                  num_hn_samples=512, pos_thresh=POS_THRESH, neg_thresh=NEG_THRESH,
                                                  sel0=sel0, sel1=sel1, pos_sel=pos_sel, return_indices=True,
                                                  kernels="hip")
    assert pos.dim() == 0 and neg.dim() == 0 and pos.is_cuda and d01.dtype == torch.int64 and not d01.requires_grad
    assert np.array_equal(d01.cpu().numpy(), ref["hard01"]) and np.array_equal(d10.cpu().numpy(), ref["hard10"])
    _check_loss(float(pos.detach()), ref["pos_loss"])
    _check_loss(float(neg.detach()), ref["neg_loss"])
    (pos + neg).backward()
    _check_grad(g0.grad, ref["df0"], ref["abs_terms0"], ref["touched0"], 0)
    _check_grad(g1.grad, ref["df1"], ref["abs_terms1"], ref["touched1"], 1)
    short = hardest_contrastive_loss(g0.detach(), g1.detach(), torch.as_tensor(pairs).to(DEV), num_pos=n_pos,
                                     sel0=sel0, sel1=sel1, pos_sel=pos_sel, kernels="hip")
    assert len(short) == 2 and torch.equal(short[0], pos.detach())


def test_hip_and_torch_kernels_agree_and_draw_the_same_samples():
    """The (3000, 2800, 2048, 512) case of tests/test_gpu_train.py: the same indices, losses and gradients within that
    test's 1e-5, with the samples drawn from equally seeded generators on both paths."""
    from imfnet_amd import ops
    from imfnet_amd.train.loss import hardest_contrastive_loss
    g = np.random.default_rng(5)
    F0, F1 = _unit_rows(g, 3000, 32), _unit_rows(g, 2800, 32)
    pairs = np.stack([g.integers(0, 3000, 4000), g.integers(0, 2800, 4000)], 1)
    sel0, sel1 = g.choice(3000, 512, replace=False), g.choice(2800, 512, replace=False)
    pos_sel = g.choice(4000, 2048, replace=False)
    r = LR.restate(F0, F1, pairs, sel0, sel1, pos_sel, POS_THRESH, NEG_THRESH)
    sp = pairs[pos_sel]
    pairs = np.concatenate([pairs, np.stack([sp[:60, 0], r["hard01"][:60]], 1),
                            np.stack([r["hard10"][60:120], sp[60:120, 1]], 1)])
    pp = torch.as_tensor(pairs.astype(np.int32)).to(DEV)
    out = {}
    for kernels in ("torch", "hip"):
        g0 = torch.as_tensor(F0).to(DEV).requires_grad_(True)
        g1 = torch.as_tensor(F1).to(DEV).requires_grad_(True)
        pos, neg, d01, d10 = hardest_contrastive_loss(g0, g1, pp, num_pos=2048, num_hn_samples=512, pos_thresh=POS_THRESH,
                                                      neg_thresh=NEG_THRESH, sel0=sel0, sel1=sel1, pos_sel=pos_sel,
                                                      return_indices=True, kernels=kernels)
        (pos + neg).backward()
        out[kernels] = (pos.detach(), neg.detach(), d01, d10, g0.grad, g1.grad)
    t, h = out["torch"], out["hip"]
    assert torch.equal(t[2], h[2]) and torch.equal(t[3], h[3])
    for a, b in ((h[0], t[0]), (h[1], t[1])):
        assert abs(float(a) - float(b)) / abs(float(b)) < 1e-5
    for a, b in ((h[4], t[4]), (h[5], t[5])):
        err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
        print("gradient, hip against torch:", err)
        assert err < 1e-5, err
    # drawn, not given: one seed gives the same samples on both paths, and None reads the switch
    drawn = {}
    prev = ops.TRAIN_LOSS
    try:
        for kernels in ("torch", "hip"):
            ops.set_train_loss(kernels)
            with torch.no_grad():
                drawn[kernels] = hardest_contrastive_loss(torch.as_tensor(F0).to(DEV), torch.as_tensor(F1).to(DEV), pp,
                                                          num_pos=1024, num_hn_samples=256,
                                                          rng=np.random.default_rng(11), return_indices=True)
    finally:
        ops.set_train_loss(prev)
    assert torch.equal(drawn["torch"][2], drawn["hip"][2]) and torch.equal(drawn["torch"][3], drawn["hip"][3])
    assert abs(float(drawn["hip"][1]) - float(drawn["torch"][1])) / float(drawn["torch"][1]) < 1e-5


# ---- a temporary 3DMatch-shaped tree (as tests/test_gpu_train.py builds it) ---------------------------------------------
def _write_ply(path, pts):
    pts = np.ascontiguousarray(pts, dtype="<f4")
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n"
                b"property float y\nproperty float z\nend_header\n" % len(pts))
        f.write(pts.tobytes())


def _crop(a):
    a = a[::3]
    return a[a[:, 0] < 0.3]


@pytest.fixture(scope="module")
def tree(tmp_path_factory, clouds, images):
    """sceneA/seq-01: cloud_bin_0 (fixture 0, PNG), cloud_bin_1 (fixture 1, JPEG only), cloud_bin_2 (fixture 0 moved by
    1 cm, PNG); four pairs in the overlap list."""
    from PIL import Image
    root = tmp_path_factory.mktemp("threedmatch_loss")
    seq = root / "sceneA" / "seq-01"
    seq.mkdir(parents=True)
    frags = [_crop(clouds[0]), _crop(clouds[1]), _crop(clouds[0]) + np.array([0.01, 0.0, 0.0])]
    for k, (pts, img) in enumerate(zip(frags, (images[0], images[1], images[0]))):
        _write_ply(seq / f"cloud_bin_{k}.ply", pts)
        u8 = (np.transpose(img[0], (1, 2, 0)) * 255).round().astype(np.uint8)
        Image.fromarray(u8).save(seq / (f"cloud_bin_{k}_0.jpg" if k == 1 else f"cloud_bin_{k}_0.png"))
    ov = root / "overlap"
    ov.mkdir()
    names = [f"sceneA/seq-01/cloud_bin_{k}.ply" for k in range(3)]
    (ov / "sceneA@seq-01-0.30.txt").write_text(
        "".join(f"{names[a]} {names[b]} 0.5\n" for a, b in ((0, 2), (0, 1), (1, 2), (2, 0))))
    (root / "scenes.txt").write_text("sceneA\n")
    return root


def test_sgd_steps_with_hip_loss_kernels_lower_the_loss(tree):
    """30 SGD steps (lr 0.1, momentum 0.8) on one fixed pair without augmentation, the criterion of
    tests/test_gpu_train.py::test_sgd_steps_lower_the_loss, with the trainer configured with loss_kernels="hip"."""
    from imfnet_amd import ops
    from imfnet_amd.train.data import IndoorPairDataset
    from imfnet_amd.train.trainer import HardestContrastiveTrainer, parse_config
    cfg = parse_config(["--threed_match_dir", str(tree), "--overlap_path", str(tree / "overlap"), "--loss_kernels", "hip",
                        "--use_random_rotation", "false", "--use_random_scale", "false", "--batch_size", "1",
                        "--out_dir", str(tree / "steps")])
    prev = ops.TRAIN_LOSS
    try:
        ds = IndoorPairDataset("val", ["sceneA"], cfg, seed=0, device=DEV)
        tr = HardestContrastiveTrainer(cfg, ds, None, device=DEV)
        assert ops.TRAIN_LOSS == "hip"
        raw = ds.load(0)                                                # cloud_bin_0 -> its 1 cm shifted copy
        losses = []
        for _ in range(30):
            losses.append(tr.train_step([[raw]])[0])
            for name, p in tr.model.named_parameters():
                if p.grad is not None:
                    assert torch.isfinite(p.grad).all(), name
        tr.pool.shutdown()
    finally:
        ops.set_train_loss(prev)
    assert all(np.isfinite(losses))
    first, last = losses[0], float(np.mean(losses[-5:]))
    print("losses", [round(v, 4) for v in losses])
    assert last < 0.85 * first, (first, last)
    assert float(np.mean(losses[-5:])) < float(np.mean(losses[:5])) - 0.1


def test_cli_with_loss_kernels_hip_runs_an_epoch_and_saves_the_option(tree, tmp_path):
    out = tmp_path / "out"
    args = [sys.executable, "-m", "imfnet_amd.train", "--threed_match_dir", str(tree), "--overlap_path",
            str(tree / "overlap"), "--train_list", str(tree / "scenes.txt"), "--test_valid", "false", "--out_dir", str(out),
            "--batch_size", "2", "--stat_freq", "1", "--seed", "1", "--max_epoch", "1", "--loss_kernels", "hip"]
    r = subprocess.run(args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Train Epoch: 1 [1/2]" in r.stdout and "nan" not in r.stdout.lower()
    ck = torch.load(out / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["config"]["loss_kernels"] == "hip" and ck["config"]["norm_kernels"] == "torch"
