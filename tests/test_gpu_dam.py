"""Descriptor Activation Mapping on the GPU (csrc/dam.hip, imfnet_amd/dam.py): the kernel against the float64 restatement
within the derived bound, its min / max, reproducibility, the row cap and the flags; the whole model against the
restatement on the hooked activations and against the reference's literal loop run through this project's autograd;
the command line."""
import os

import numpy as np
import pytest
import torch

import dam_restate as DR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
# |heat - exact| <= 40 u sum_c |w_c| |o[n, c]|: one rounding of w and the 32-term fp32 FMA chain (gamma_33), csrc/dam.hip
BOUND_UNITS = 40
MAX_LEFT_OUT = 1e-3          # share of elements whose exact pre-ReLU value is within the bound of zero


def kernel_inputs(n, T, c_hid):
    """Random normal h [n, c_hid], o [n, 32] and T targets: rows 0 and n - 1 and a duplicate wherever T allows."""
    rng = np.random.default_rng(7 + 1000003 * n + 1009 * T + c_hid)
    h = rng.standard_normal((n, c_hid)).astype(np.float32)
    o = rng.standard_normal((n, 32)).astype(np.float32)
    targets = [n - 1] if T == 1 else ([0, n - 1, 0] + rng.integers(0, n, size=T - 3).tolist())
    return h, o, np.asarray(targets, dtype=np.int32)


def near_zero_share(pre, mag, targets):
    """The share of elements whose exact pre-ReLU value is within the bound of zero, where the computed sign may differ.
    A target's own element is not counted: there the exact value IS zero (the gradient of a normalised row is orthogonal
    to the row), one element per target whatever the inputs -- 1 / n of a case, which no choice of seed changes."""
    near = np.abs(pre) <= BOUND_UNITS * U * mag
    own = np.zeros_like(near)
    for i, t in enumerate(targets):
        if 0 <= t < pre.shape[1]:
            own[i, t] = True
    assert near[own].all()
    return float((near & ~own).sum() / max(1, (~own).sum()))


def left_out_share(n, T, c_hid, accumulate):
    """Float64 only (runs without a GPU)."""
    h, o, targets = kernel_inputs(n, T, c_hid)
    pre, mag, _, _ = DR.closed_form(h, o, targets, accumulate)
    return near_zero_share(pre, mag, targets)


def check_against_restatement(heat, h, o, targets, accumulate, what):
    """Every element within the bound of the exact map: the ReLU is 1-Lipschitz, so an element whose exact value is within
    the bound of zero needs no exemption -- whichever sign the fp32 sum takes, |relu(got) - relu(exact)| <= |got - exact|.
    The share of such elements is gated all the same (MAX_LEFT_OUT)."""
    pre, mag, _, flags = DR.closed_form(h, o, targets, accumulate)
    bound = BOUND_UNITS * U * mag
    share = near_zero_share(pre, mag, targets)
    err = np.abs(np.asarray(heat, dtype=np.float64) - np.maximum(pre, 0.0))
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"{what}: max err / bound = {ratio:.3f}, near zero {share:.2e}")
    assert share <= MAX_LEFT_OUT
    assert (err <= bound).all()
    return flags


@pytest.mark.parametrize("c_hid", [64, 96])
@pytest.mark.parametrize("T", [1, 3, 65])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_kernel_matches_the_float64_restatement(n, T, c_hid):
    from imfnet_amd import ops
    h, o, targets = kernel_inputs(n, T, c_hid)
    hd, od, td = (torch.as_tensor(a).to(DEV) for a in (h, o, targets))
    for accumulate in (True, False):
        heat, minmax, flags, weights = ops.dam_heat(od, hd, td, accumulate=accumulate)
        again = ops.dam_heat(od, hd, td, accumulate=accumulate)
        heat_h = heat.cpu().numpy()
        want_flags = check_against_restatement(heat_h, h, o, targets, accumulate, f"n={n} T={T} c_hid={c_hid} acc={accumulate}")
        assert heat.shape == (T, n) and not want_flags.any() and not flags.cpu().numpy().any()
        w64 = DR.closed_form(h, o, targets, accumulate)[2]
        assert (np.abs(weights.cpu().numpy() - w64) <= 1.01 * U * np.abs(w64)).all()           # one rounding of w
        # min and max of the rows that came back, bit for bit; two calls, bit for bit
        mm = minmax.cpu().numpy()
        assert np.array_equal(mm[:, 0].view(np.uint32), heat_h.min(axis=1).view(np.uint32))
        assert np.array_equal(mm[:, 1].view(np.uint32), heat_h.max(axis=1).view(np.uint32))
        for a, b in zip((heat, minmax, flags, weights), again):
            assert torch.equal(a, b)
        if T >= 3:                                                   # the duplicate target gives the same row
            assert np.array_equal(heat_h[0], heat_h[2])


def test_device_row_count_caps_the_rows():
    from imfnet_amd import ops
    n, cap = 300, 131
    h, o, _ = kernel_inputs(n, 3, 64)
    targets = np.asarray([0, cap - 1, cap], dtype=np.int32)          # the last one lies beyond the cap
    hd, od, td = (torch.as_tensor(a).to(DEV) for a in (h, o, targets))
    sentinel = -7.0
    heat = torch.full((3, n), sentinel, dtype=torch.float32, device=DEV)
    n_dev = torch.tensor([cap], dtype=torch.int32, device=DEV)
    out, minmax, flags, _ = ops.dam_heat(od, hd, td, n_dev=n_dev, heat=heat)
    assert out is heat
    got = heat.cpu().numpy()
    assert (got[:, cap:] == sentinel).all() and (got[:, :cap] != sentinel).all()
    assert flags.cpu().tolist() == [0, 0, 1] and not got[2, :cap].any()
    check_against_restatement(got[:2, :cap], h[:cap], o[:cap], targets[:2], True, "capped")
    mm = minmax.cpu().numpy()
    assert np.array_equal(mm[:, 0], got[:, :cap].min(axis=1)) and np.array_equal(mm[:, 1], got[:, :cap].max(axis=1))


def test_flagged_targets_give_zero_rows():
    """Valid inputs to a guarded kernel: a target outside the rows (either side), a row whose pre-normalisation output is
    zero, and one that is not finite."""
    from imfnet_amd import ops
    n = 70
    h, o, _ = kernel_inputs(n, 3, 64)
    o[5] = 0.0
    o[9, 3] = np.inf
    targets = np.asarray([n, -1, 5, 9, 2], dtype=np.int32)
    hd, od, td = (torch.as_tensor(a).to(DEV) for a in (h, o, targets))
    heat, minmax, flags, weights = ops.dam_heat(od, hd, td)
    assert flags.cpu().tolist() == [1, 1, 1, 1, 0]
    got = heat.cpu().numpy()
    assert not got[:4].any() and not weights[:4].cpu().numpy().any() and not minmax[:4].cpu().numpy().any()
    assert np.isfinite(got[4][np.arange(n) != 9]).all() and got[4].max() > 0
    assert DR.closed_form(h, o, targets, True)[3].tolist() == [1, 1, 1, 1, 0]


def test_wrapper_argument_checks():
    from imfnet_amd import ops
    from imfnet_amd._lib import ImfError
    o, h = torch.zeros(4, 32, device=DEV), torch.zeros(4, 64, device=DEV)
    t = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ImfError):
        ops.dam_heat(torch.zeros(4, 16, device=DEV), h, t)
    with pytest.raises(ImfError):
        ops.dam_heat(o, torch.zeros(4, 48, device=DEV), t)
    with pytest.raises(ImfError):
        ops.dam_heat(o, torch.zeros(5, 64, device=DEV), t)
    with pytest.raises(ImfError):
        ops.dam_heat(o, h, t.long())
    with pytest.raises(ImfError):
        ops.dam_heat(o.cpu(), h, t)
    heat, minmax, flags, _ = ops.dam_heat(o, h, t[:0])
    assert heat.shape == (0, 4) and minmax.shape == (0, 2) and flags.shape == (0,)


# ---- whole model --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fragment(clouds, images, seeded_sd):
    from imfnet_amd.model import load_model
    m = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3, config=None)
    m.load_state_dict(seeded_sd, strict=True)
    m = m.eval().to(DEV)
    xyz = clouds[1][::6].astype(np.float64)
    return m, xyz, torch.as_tensor(images[1]).to(DEV)


def _tensor(xyz):
    from imfnet_amd.extract import sparse_tensor_from_points
    with torch.no_grad():
        return sparse_tensor_from_points(xyz, 0.05, torch.device(DEV))[0]


def test_model_map_matches_the_restatement_and_the_literal_loop(fragment):
    from imfnet_amd.dam import DAM
    model, xyz, img = fragment
    st = _tensor(xyz)
    n = st.F.shape[0]
    assert 200 <= n <= 5000
    targets = [0, n // 2, n - 1]
    dam = DAM(model)
    heat, flags = dam(st, img, targets)
    assert heat.shape == (3, n) and heat.dtype == torch.float32 and heat.is_cuda and flags.cpu().tolist() == [0, 0, 0]
    assert not torch.is_grad_enabled() or all(p.grad is None for p in model.parameters())
    h, o = dam.hidden.cpu().numpy(), dam.prenorm.cpu().numpy()
    assert h.shape == (n, 64) and o.shape == (n, 32) and (h >= 0).all()
    heat_h = heat.cpu().numpy()
    check_against_restatement(heat_h, h, o, targets, True, "model")
    # the descriptors of that forward are the model's own on the same call path
    with torch.no_grad():
        F = model.forward_layers(_tensor(xyz), img).F
    assert torch.equal(dam.descriptors, F)
    assert torch.equal(dam.descriptors, dam.prenorm / torch.norm(dam.prenorm, p=2, dim=1, keepdim=True))

    # the reference's loop through this project's autograd, for one target: gradients to `final` only
    t = targets[1]
    seen = {}
    handle = model.final.register_forward_hook(lambda mod, i, out: seen.__setitem__("o", out.F.detach()))
    for p in model.parameters():
        p.requires_grad_(False)
    for p in model.final.parameters():
        p.requires_grad_(True)
    try:
        model.zero_grad()
        F = model(_tensor(xyz), img).F
        assert F.requires_grad
        maps = []
        for j in range(32):
            F[t, j].backward(retain_graph=True)
            channel = model.final.kernel.grad.detach().t().mean(dim=1)
            maps.append((channel[:, None] * seen["o"].t()).sum(dim=0))
        literal = torch.clamp(torch.stack(maps).sum(dim=0), min=0).cpu().numpy().astype(np.float64)
    finally:
        handle.remove()
        model.zero_grad()
        for p in model.parameters():
            p.requires_grad_(True)
    pre, mag, _, _ = DR.closed_form(h, o, [t], True)
    scale = float(np.maximum(pre, 0).max())
    err = np.abs(heat_h[1] - literal)
    print(f"literal loop: max err = {err.max():.3e} = {err.max() / scale:.3e} of max|heat| (gate {DR.LITERAL_F32_GATE:.1e})")
    # the literal loop is within its gate of the exact map, the kernel within its bound: triangle inequality
    assert (err <= DR.LITERAL_F32_GATE * scale + BOUND_UNITS * U * mag[0]).all()


def test_command_line_writes_the_coloured_cloud(tmp_path, clouds):
    import ctypes as C
    from imfnet_amd import _lib
    from imfnet_amd import dam as D
    from imfnet_amd.dataio import read_ply_points
    pts = np.ascontiguousarray(clouds[0][::4].astype(np.float64))
    ply = tmp_path / "cloud.ply"
    _lib.check(_lib.lib().imf_ply_write_points(os.fsencode(str(ply)), pts.ctypes.data_as(C.c_void_p), len(pts)), "write")
    out = tmp_path / "map.ply"
    targets = [5, 780]
    argv = ["--ply", str(ply), "--image", os.path.join(ROOT, "tests", "golden", "cloud_bin_0_0.png"), "--out", str(out)]
    assert D.main(argv + [a for t in targets for a in ("--target", str(t))]) == 0
    table = {tuple(int(v) for v in row) for row in D.HSV_TABLE} | {(144, 144, 144)}
    counts = set()
    for t, path in zip(targets, D.output_paths(str(out), targets)):
        raw = open(path, "rb").read()
        end = raw.index(b"end_header\n") + 11
        rows = np.frombuffer(raw[end:], dtype=np.dtype([("xyz", "<f8", 3), ("rgb", "u1", 3)]))
        n = len(rows)
        counts.add(n)
        assert f"element vertex {n}\n".encode() in raw[:end] and n > t
        assert np.flatnonzero((rows["rgb"] == 0).all(axis=1)).tolist() == [t]
        assert {tuple(int(v) for v in c) for c in np.delete(rows["rgb"], t, axis=0)} <= table
        assert len(read_ply_points(path)) == n
    assert len(counts) == 1
