"""Host side of Descriptor Activation Mapping (imfnet_amd/dam.py, csrc/dam.hip, imf_ply_write_points_rgb): the closed form
against the reference's literal loop on torch autograd, the colour stage against the bytes the reference wrote
(tests/golden/head_map_rgb.npz = the colours of its files/3D_head_map.ply), the coloured PLY, the C ABI.  No GPU."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dam_restate as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("imf_dam_heat", "imf_ply_write_points_rgb")
TARGET = 780
LITERAL_F32_ERR, LITERAL_F32_GATE = DR.LITERAL_F32_ERR, DR.LITERAL_F32_GATE

CASES = [(n, acc, t) for n in (1, 7, 300) for acc in (True, False) for t in sorted({0, n - 1})]


def _layer(n, seed):
    gen = torch.Generator().manual_seed(seed)
    h = torch.relu(torch.randn(n, 64, generator=gen)).numpy()
    K = (torch.randn(64, 32, generator=gen) / 8).numpy()
    b = (torch.randn(32, generator=gen) / 8).numpy()
    return h, K, b


def _case(n, acc, t):
    """(h, K, b, float64 closed-form heat [n], scale).  scale = max |heat|, except for n = 1: the map's value at the target
    row itself is 0 in exact arithmetic (the gradient of a normalised row is orthogonal to the row), so with one row
    max |heat| is rounding noise and the yardstick is the size of the terms that cancel, max sum_c |w_c o[n, c]|."""
    h, K, b = _layer(n, 100 + n)
    o = h.astype(np.float64) @ K.astype(np.float64) + b.astype(np.float64)
    pre, mag, _, _ = DR.closed_form(h, o, [t], acc)
    heat = np.maximum(pre[0], 0.0)
    scale = float(np.abs(heat).max()) if n > 1 else float(mag.max())
    assert scale > 1e-3
    return h, K, b, heat, scale


@pytest.mark.parametrize("n,acc,t", CASES)
def test_closed_form_equals_the_literal_loop_in_float64(n, acc, t):
    h, K, b, want, scale = _case(n, acc, t)
    got = DR.literal_loop(h, K, b, t, acc, torch.float64).numpy()
    assert np.abs(got - want).max() <= 1e-12 * scale


def test_float32_literal_loop_is_within_its_recorded_distance():
    worst = 0.0
    for n, acc, t in CASES:
        h, K, b, want, scale = _case(n, acc, t)
        got = DR.literal_loop(h, K, b, t, acc, torch.float32).numpy().astype(np.float64)
        worst = max(worst, float(np.abs(got - want).max() / scale))
    print(f"float32 literal loop vs float64 closed form: {worst:.3e} of max|heat| (recorded {LITERAL_F32_ERR:.1e})")
    assert worst <= LITERAL_F32_GATE


def test_accumulation_matters():
    """The two settings are different maps: the accumulating gradient weights component j by 32 - j."""
    acc, scale = _case(300, True, 0)[3:]
    assert np.abs(acc - _case(300, False, 0)[3]).max() > 0.1 * scale


# ---- colour stage -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def head_rgb():
    return np.load(os.path.join(GOLDEN, "head_map_rgb.npz"))["rgb"]


def test_fixture_is_what_the_issue_counted(head_rgb, head_map):
    assert head_rgb.shape == (18977, 3) == head_map.shape and head_rgb.dtype == np.uint8
    black = np.flatnonzero((head_rgb == 0).all(axis=1))
    assert black.tolist() == [TARGET]
    grey = (head_rgb == 144).all(axis=1)
    assert int(grey.sum()) == 11346
    rest = head_rgb[~grey & ~(head_rgb == 0).all(axis=1)]
    assert len(rest) == 7630 and len({tuple(r) for r in rest}) == 190


def test_dam_colors_reproduces_the_reference_bytes(head_rgb):
    from imfnet_amd.dam import HSV_TABLE, dam_colors
    assert HSV_TABLE.shape == (256, 3) and len({tuple(r) for r in HSV_TABLE}) == 256      # injective
    index = {tuple(int(v) for v in row): i for i, row in enumerate(HSV_TABLE)}
    grey = (head_rgb == 144).all(axis=1)
    heat = np.zeros(len(head_rgb))
    idx = np.full(len(head_rgb), -1)
    for r in np.flatnonzero(~grey):
        if r == TARGET:
            continue
        idx[r] = index[tuple(int(v) for v in head_rgb[r])]          # KeyError: a colour that is not a table entry
    col = idx >= 0
    assert idx[col].min() == 25 and idx[col].max() == 255
    # the middle of each bin's part inside [0.1, 1]: bin 25 = [25/256, 26/256) starts below v = 0.1, and its plain middle
    # would be a negative heat, i.e. a new minimum; every other bin's middle is (i + 0.5) / 256
    v_mid = (np.maximum(idx[col] / 256, 0.1) + (idx[col] + 1) / 256) / 2
    heat[col] = (v_mid - 0.1) / 0.9
    assert heat.min() == 0.0 and (heat[col] > 0).all()
    heat[np.flatnonzero(idx == 255)[0]] = 1.0
    got = dam_colors(heat, TARGET)
    assert got.dtype == np.uint8 and np.array_equal(got, head_rgb)
    assert np.array_equal(dam_colors(heat.astype(np.float32), TARGET), head_rgb)


def test_table_is_matplotlibs_hsv():
    cm = pytest.importorskip("matplotlib.cm")
    from imfnet_amd.dam import HSV_TABLE
    want = np.round(np.asarray(cm.hsv(np.arange(256)))[:, :3] * 255).astype(np.uint8)
    assert np.array_equal(HSV_TABLE, want)


def test_product_code_does_not_import_matplotlib():
    got = subprocess.run([os.sys.executable, "-c", "import sys, imfnet_amd.dam; print('matplotlib' in sys.modules)"],
                         env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, cwd=ROOT)
    assert got.returncode == 0 and got.stdout.strip() == "False", got.stderr


@pytest.mark.parametrize("value", [0.0, 3.5])
def test_constant_heat_is_all_grey_with_a_black_target(value):
    from imfnet_amd.dam import dam_colors
    got = dam_colors(np.full(50, value, dtype=np.float32), 7)
    want = np.full((50, 3), 144, dtype=np.uint8)
    want[7] = 0
    assert np.array_equal(got, want)


def test_dam_colors_refuses_a_target_outside_the_rows():
    from imfnet_amd._lib import ImfError
    from imfnet_amd.dam import dam_colors
    for bad in (-1, 5):
        with pytest.raises(ImfError):
            dam_colors(np.arange(5.0), bad)


def test_write_head_map_reproduces_the_reference_file(tmp_path, head_rgb, head_map):
    from imfnet_amd.dam import write_head_map
    from imfnet_amd.dataio import read_ply_points
    meta = json.load(open(os.path.join(GOLDEN, "head_map_ply.json")))
    path = tmp_path / "3D_head_map.ply"
    write_head_map(str(path), head_map, head_rgb)
    raw = path.read_bytes()
    assert len(raw) == meta["bytes"] and hashlib.sha256(raw).hexdigest() == meta["sha256"]
    assert not os.path.exists(str(path) + ".tmp")
    assert np.array_equal(read_ply_points(str(path)), head_map.astype(np.float64))


def test_write_head_map_argument_errors(tmp_path):
    from imfnet_amd import _lib
    from imfnet_amd.dam import write_head_map
    with pytest.raises(_lib.ImfError):
        write_head_map(str(tmp_path / "a.ply"), np.zeros((3, 3)), np.zeros((2, 3), np.uint8))
    with pytest.raises(_lib.ImfError):
        write_head_map(str(tmp_path / "no_such_dir" / "a.ply"), np.zeros((3, 3)), np.zeros((3, 3), np.uint8))
    L = _lib.lib()
    assert L.imf_ply_write_points_rgb(None, None, None, 0) == -1
    assert L.imf_ply_write_points_rgb(os.fsencode(str(tmp_path / "b.ply")), None, None, 2) == -1
    write_head_map(str(tmp_path / "empty.ply"), np.zeros((0, 3)), np.zeros((0, 3), np.uint8))
    assert L.imf_ply_vertex_count(os.fsencode(str(tmp_path / "empty.ply"))) == 0


# ---- C ABI and Python surface ------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbols():
    from imfnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "imfnet_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/imfnet_hip.h"
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        assert set(SYMBOLS) <= set(line.split()[-1] for line in nm.stdout.splitlines() if line.strip())


def test_argument_checks_answer_before_any_launch():
    from imfnet_amd import _lib
    L = _lib.lib()
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data
    call = lambda n, c_hid, c_out, T, out=p: L.imf_dam_heat(out, n, None, p, c_hid, c_out, p, T, 1, p, p, p, p, None)
    assert call(4, 64, 16, 1) == -3 and b"c_out=16" in L.imf_last_error()          # IMF_EUNSUPPORTED
    assert call(4, 48, 32, 1) == -3 and b"c_hid=48" in L.imf_last_error()
    assert call(4, 0, 32, 1) == -1 and call(-1, 64, 32, 1) == -1 and call(4, 64, 32, -1) == -1
    assert call(4, 64, 32, 1, None) == -1                                          # a null required pointer
    assert call(4, 64, 32, 1, p + 4) == -1 and b"aligned" in L.imf_last_error()
    assert call(4, 64, 32, 0) == 0                                                 # no targets: nothing is launched
    assert not buf.any()


def test_only_final_is_a_supported_target_layer():
    from imfnet_amd._lib import ImfError
    from imfnet_amd.dam import DAM
    from imfnet_amd.model import load_model
    m = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3, config=None)
    assert DAM(m).final is m.final and DAM(m, m.final).final is m.final
    with pytest.raises(ImfError, match="final"):
        DAM(m, m.conv1_tr)
    with pytest.raises(ImfError, match="final"):
        DAM(torch.nn.Linear(2, 2))


def test_cli_parses_repeated_targets_and_names_one_file_per_target():
    from imfnet_amd.dam import output_paths, parse_args
    base = ["--ply", "a.ply", "--image", "a_0.png"]
    a = parse_args(base)
    assert a.target == [780] and a.model is None and not a.no_accumulate and a.out == "3D_head_map.ply"
    a = parse_args(base + ["--target", "5", "--target", "780", "--no_accumulate", "--out", "x/map.ply", "-m", "c.pth"])
    assert a.target == [5, 780] and a.no_accumulate and a.model == "c.pth"
    assert output_paths(a.out, a.target) == ["x/map_5.ply", "x/map_780.ply"]
    assert output_paths("map.ply", [3]) == ["map.ply"]
    with pytest.raises(SystemExit):
        parse_args(["--ply", "a.ply"])
