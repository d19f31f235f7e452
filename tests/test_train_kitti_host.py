"""Host-side pieces of KITTI training and of the validation metrics: the robust-transform fixture guards itself (the fp64
restatement against upstream's stored float32 results), the command line's data-set options and defaults, the
direction of every validation metric, and the C ABI's declaration of imf_robust_transform.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import robust_restate as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return RR.load_cases()


def test_fixture_cases_are_the_generators(cases):
    """The stored points are exactly what make_case builds (the generator and the fixture cannot drift apart), every
    family has its three seeds, and no stored gap marks an ill-conditioned case."""
    assert len(cases) == len(RR.FAMILIES) * len(RR.SEEDS)
    for fam, seed, p0, p1, w, T_up, gap_R, gap_t in cases:
        kw = RR.FAMILIES[fam]
        assert p0.dtype == np.float32 and p0.shape == (kw["n"], 3) and p1.shape == p0.shape
        assert (w is not None) == kw["weights"]
        assert T_up.dtype == np.float32 and T_up.shape == (4, 4)
        assert 0 < gap_R < 1e-4 and 0 < gap_t < 1e-4, (fam, seed, gap_R, gap_t)
    fam, seed, p0, p1, w, *_ = cases[0]
    q0, q1, _, _ = RR.make_case(seed=seed, **RR.FAMILIES[fam])
    assert np.array_equal(p0, q0) and np.array_equal(p1, q1)


def test_restatement_reproduces_upstream_within_the_stored_gaps(cases):
    """The fp64 NumPy restatement against upstream's recorded float32 result: within the gap the generator stored (a
    hair of slack for another BLAS summing in another order)."""
    for fam, seed, p0, p1, w, T_up, gap_R, gap_t in cases:
        T = RR.robust_transform_f64(p0, p1, w)
        dR = np.abs(T[:3, :3] - T_up[:3, :3].astype(np.float64)).max()
        dt = np.abs(T[:3, 3] - T_up[:3, 3].astype(np.float64)).max()
        print(f"{fam} seed {seed}: |dR| {dR:.2e} (stored {gap_R:.2e}), |dt| {dt:.2e} (stored {gap_t:.2e})")
        assert dR <= gap_R * 1.01 + 1e-12 and dt <= gap_t * 1.01 + 1e-12, (fam, seed)
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12) and np.array_equal(T[3], [0, 0, 0, 1])


def test_restatement_recovers_the_planted_motion():
    p0, p1, w, planted = RR.make_case(seed=0, **RR.FAMILIES["indoor_8deg"])
    T = RR.robust_transform_f64(p0, p1, w)
    assert np.linalg.norm(T[:3, 3] - planted[:3, 3]) < 0.01
    assert np.rad2deg(np.arccos((np.trace(T[:3, :3].T @ planted[:3, :3]) - 1) / 2)) < 0.1


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "imfnet_amd.train", *args], cwd=ROOT, capture_output=True, text=True,
                          timeout=120)


def test_help_lists_the_data_set_options():
    r = _cli("--help")
    assert r.returncode == 0, r.stderr
    for name in ("--dataset", "--kitti_root", "KITTINMPairDataset", "ThreeDMatchPairDataset", "--own_image"):
        assert name in r.stdout, name


def test_parse_config_accepts_the_four_metrics_and_refuses_others():
    from imfnet_amd.train.trainer import parse_config
    for m in ("feat_match_ratio", "success", "rte", "rre"):
        assert parse_config(["--best_val_metric", m]).best_val_metric == m
        assert parse_config(["--dataset", "KITTINMPairDataset", "--best_val_metric", m]).best_val_metric == m
    with pytest.raises(SystemExit):
        parse_config(["--best_val_metric", "loss"])
    with pytest.raises(SystemExit):
        parse_config(["--dataset", "ModelNet"])


def test_kitti_defaults_only_with_the_kitti_data_set():
    from imfnet_amd.train.trainer import parse_config
    c = parse_config([])
    assert c.dataset == "ThreeDMatchPairDataset"
    assert (c.voxel_size, c.hit_ratio_thresh, c.use_random_scale, c.best_val_metric) == (0.025, 0.1, False,
                                                                                          "feat_match_ratio")
    k = parse_config(["--dataset", "KITTINMPairDataset", "--kitti_root", "/data/kitti"])
    assert (k.voxel_size, k.hit_ratio_thresh, k.use_random_scale, k.best_val_metric) == (0.3, 0.3, True, "success")
    assert k.kitti_root == "/data/kitti" and (k.min_scale, k.max_scale) == (0.8, 1.2)
    assert k.positive_pair_search_voxel_size_multiplier == 1.5 and (k.batch_size, k.lr) == (2, 0.1)
    # an option that is given wins over the data set's default, either way
    k = parse_config(["--dataset", "KITTINMPairDataset", "--voxel_size", "0.2", "--use_random_scale", "false",
                      "--best_val_metric", "rte", "--hit_ratio_thresh", "0.5"])
    assert (k.voxel_size, k.hit_ratio_thresh, k.use_random_scale, k.best_val_metric) == (0.2, 0.5, False, "rte")
    c = parse_config(["--voxel_size", "0.3", "--use_random_scale", "true"])
    assert (c.voxel_size, c.use_random_scale, c.hit_ratio_thresh) == (0.3, True, 0.1)


def test_better_is_lower_for_rte_and_rre():
    from imfnet_amd.train.trainer import is_better, worst_value
    for m in ("rte", "rre"):
        assert is_better(m, 0.5, 0.7) and not is_better(m, 0.7, 0.5) and not is_better(m, 0.5, 0.5)
        assert is_better(m, 3.0, worst_value(m)) and not is_better(m, float("nan"), 1.0)
        # an epoch with nothing to average reports NaN (valid_epoch), which must not beat anything, the start included
        assert not is_better(m, float("nan"), worst_value(m)) and not is_better(m, float("nan"), 0.0)
    for m in ("feat_match_ratio", "success"):
        assert is_better(m, 0.7, 0.5) and not is_better(m, 0.5, 0.7) and not is_better(m, 0.5, 0.5)
        assert is_better(m, 0.0, worst_value(m)) and not is_better(m, float("nan"), 0.1)


def test_header_declares_and_library_exports_the_estimator():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    assert re.search(r"\bint imf_robust_transform\(const double \*pts0, const double \*pts1, const double \*weight, "
                     r"int64_t n,", text)
    assert re.search(r"\bsize_t imf_robust_transform_workspace_bytes\(int64_t n\);", text)
    for name in ("imf_robust_transform", "imf_robust_transform_workspace_bytes"):
        assert name in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "imf_robust_transform") and hasattr(handle, "imf_robust_transform_workspace_bytes")
    fn = handle.imf_robust_transform_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int64]
    assert fn(0) == 0 and fn(5000) == 0 and fn(5120) == 0             # a thread's share fits its registers
    assert fn(5121) >= 5121 * 32 and fn(70000) % 256 == 0 and fn(70000) >= 70000 * 32
