"""Host side of the FPFH descriptor: the NumPy restatement (tests/fpfh_restate.py) on a hand-computed case and on its own
invariants, the share of points the GPU comparison may not decide, the C ABI's refusals and the command lines.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fpfh_restate as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("imf_fpfh_workspace_bytes", "imf_fpfh_features")
CASES = FR.cases()
IDS = [c.name for c in CASES]


def test_restatement_on_a_hand_computed_three_point_case():
    """p0 = 0, p1 = e_x, p2 = e_y with normals e_z, e_z, e_x, everybody everybody's neighbour.
    (0,1): both normals e_z, d in the plane: f = (0, 0, 0), bins 5, 16, 27.
    (0,2): d = e_y, a1 = a2 = 0, v = e_y x e_z = e_x, w = e_z x e_x = e_y, f1 = v . e_x = 1 (bin 10 of its group: 21),
           f0 = atan2(0, 0) = 0 (5), f2 = 0 (27); (2,0) the same by symmetry.
    (1,2): d = (-1, 1, 0), a1 = 0, a2 = -1/sqrt 2: swapped, f2 = +1/sqrt 2 -> 11 * 1.7071 / 2 = 9.39 (bin 9: 31),
           v = (1, -1, 0) x e_x = e_z, f1 = e_z . e_z = 1 (21), f0 = atan2(0, 0) (5); (2,1): a1 = 1/sqrt 2, not swapped, the same."""
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    nbr = np.array([[0, 1, 2], [1, 0, 2], [2, 0, 1]], np.int32)
    got = FR.restate(pts, nrm, nbr, np.array([3, 3, 3], np.int32))
    want = np.zeros((3, 33), np.int32)
    for i, pairs in enumerate(([(5, 16, 27), (5, 21, 27)], [(5, 16, 27), (5, 21, 31)], [(5, 21, 27), (5, 21, 31)])):
        for bins in pairs:
            want[i, list(bins)] += 1
    assert np.array_equal(got["hist"], want) and np.array_equal(got["m"], [2, 2, 2])
    assert np.array_equal(got["spfh"], want * 50.0)
    # point 0: both neighbours at d2 = 1: acc = spfh_1 + spfh_2, every group sums to 200
    acc0 = (want[1] + want[2]) * 50.0
    assert np.array_equal(got["acc"][0], acc0)
    assert np.allclose(got["out"][0], acc0 * 0.5 + want[0] * 50.0, rtol=0, atol=1e-12)
    # point 1: p0 at d2 = 1, p2 at d2 = 2
    acc1 = want[0] * 50.0 + want[2] * 25.0
    assert np.allclose(got["out"][1], acc1 * (100.0 / 150.0) + want[1] * 50.0, rtol=0, atol=1e-12)
    # f1 = 1 sits on the edge 11 of its group (clamped into bin 10): the pairs with p2 are undecided, (0,1) is not
    assert np.array_equal(got["undecided"], [[False, False, True], [False, False, True], [False, True, True]])
    assert not got["clean"].any()
    # a list that names nothing but the point itself, padding and rubbish
    lone = FR.restate(pts, nrm, np.array([[0, -1, 7], [1, -5, -1], [2, 2, -1]], np.int32), np.array([3, 3, 3], np.int32))
    assert not lone["hist"].any() and not lone["out"].any() and lone["clean"].all()
    # counts cuts the list
    cut = FR.restate(pts, nrm, nbr, np.array([2, 2, 1], np.int32))
    assert np.array_equal(cut["m"], [1, 1, 0]) and not cut["out"][2].any()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_groups_sum_to_what_the_rules_say_and_few_points_are_undecided(case):
    ref = FR.host_reference(case)
    n = len(case.points)
    assert ref["hist"].shape == (n, 33) and np.array_equal(ref["hist"].sum(1), 3 * ref["m"])
    groups = ref["hist"].reshape(n, 3, 11).sum(2)
    assert (groups == ref["m"][:, None]).all()
    spfh = ref["spfh"].reshape(n, 3, 11).sum(2)
    live = ref["m"] > 0
    assert np.abs(spfh[live] - 100.0).max(initial=0.0) <= 1e-9 and not spfh[~live].any()
    S = ref["acc"].reshape(n, 3, 11).sum(2)
    want = np.where(S != 0.0, 100.0, 0.0) + np.where(live, 100.0, 0.0)[:, None]
    assert np.abs(ref["out"].reshape(n, 3, 11).sum(2) - want).max() <= 1e-9
    assert (ref["out"] >= 0.0).all() and np.isfinite(ref["out"]).all()
    share = 1.0 - ref["clean"].mean()
    print(f"{case.name}: n = {n}, mean m = {ref['m'].mean():.1f}, non-clean share {share:.4%}")
    assert share <= 0.01, share                                        # the cap of the GPU comparison, held by the seed


def test_case_catalogue_has_the_edges_it_claims():
    by = {c.name: c for c in CASES}
    ref = {name: FR.host_reference(c) for name, c in by.items()}
    assert (FR.host_inputs(by["curved_patch_knn64"])[2] == 64).mean() > 0.8
    padded = FR.host_inputs(by["curved_patch_knn16_padded"])[2]
    assert (padded < 16).mean() > 0.5 and (FR.host_inputs(by["curved_patch_knn16_padded"])[1] == -1).any()
    lat = ref["lattice_identical_normals"]                             # every feature is zero: the middle bins only
    assert (lat["hist"][:, [5, 16, 27]] == lat["m"][:, None]).all() and (np.abs(lat["gap"][lat["valid"]] - 0.5) < 1e-12).all()
    dup_case = by["exact_duplicates"]
    nrm, nbr, counts = FR.host_inputs(dup_case)
    d2 = ((dup_case.points[np.maximum(nbr, 0)] - dup_case.points[:, None, :]) ** 2).sum(2)
    assert (ref["exact_duplicates"]["valid"] & (d2 == 0.0)).sum() >= 100      # pairs of zero length, counted mid-bin
    lonely = ref["lonely_point"]
    assert lonely["m"][-1] == 0 and not lonely["out"][-1].any() and lonely["m"][:-1].min() > 0
    trio = ref["isolated_trio"]
    assert (trio["m"][-3:] == 2).all() and (FR.host_inputs(by["isolated_trio"])[1][-3:].max(1) >= len(by["isolated_trio"].points) - 3).all()
    par = ref["normal_parallel_to_d"]                                  # the pair (0, 1): |v| == 0, all three features zero
    assert np.abs(par["gap"][0][FR.host_inputs(by["normal_parallel_to_d"])[1][0] == 1] - 0.5).max() < 1e-12
    assert len(by["fixture_every_16th"].points) == 16147


def test_large_set_lists_match_the_brute_force_ones():
    pts = np.random.default_rng(3).uniform(0.0, 1.0, (2100, 3))
    a, ac = FR.neighbors(pts, 20, 0.12)
    b, bc = FR.NR.neighbors(pts, 20, 0.12)
    assert np.array_equal(a, b) and np.array_equal(ac, bc) and (bc < 20).any() and (bc == 20).any()


def test_header_declares_and_library_exports_the_symbols():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    assert "compute_fpfh_feature" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.imf_fpfh_workspace_bytes(0, 30) == 0 and L.imf_fpfh_workspace_bytes(1 << 30, 30) == 0
    assert L.imf_fpfh_workspace_bytes(8, 0) == 0 and L.imf_fpfh_workspace_bytes(8, 65) == 0
    assert 0 < L.imf_fpfh_workspace_bytes(1, 1) < L.imf_fpfh_workspace_bytes(100000, 64)
    assert L.imf_fpfh_workspace_bytes(100000, 64) >= 100000 * 34 * 4 and L.imf_fpfh_workspace_bytes(100000, 64) % 256 == 0


def test_argument_errors_return_a_status_without_a_gpu():
    """Every refusal comes before any device call, so it answers on a machine without a GPU (host pointers here)."""
    from imfnet_amd import _lib
    L = _lib.lib()
    buf = np.zeros(1 << 16, dtype=np.float64)
    p = buf.ctypes.data
    p += (-p) % 256
    EINVAL = -1
    names = ("points", "normals", "nbr", "counts", "out", "hist", "workspace")

    def fpfh(n=8, knn=30, width=33, null=None, ws=None, ws_ptr=None):
        ptr = {k: (None if k == null else p) for k in names}
        if ws_ptr is not None:
            ptr["workspace"] = ws_ptr
        nbytes = L.imf_fpfh_workspace_bytes(8, 30) if ws is None else ws
        return L.imf_fpfh_features(ptr["points"], ptr["normals"], n, ptr["nbr"], ptr["counts"], knn, width, ptr["out"],
                                   ptr["hist"], ptr["workspace"], nbytes, None)

    for kw in (dict(n=0), dict(n=-1), dict(n=1 << 30), dict(knn=0), dict(knn=65), dict(knn=-4), dict(width=32),
               dict(width=0), dict(width=34), dict(width=128), dict(ws=0), dict(ws=L.imf_fpfh_workspace_bytes(8, 30) - 1),
               dict(ws_ptr=p + 8)):
        assert fpfh(**kw) == EINVAL, kw
    assert b"imf_fpfh_features" in L.imf_last_error() and b"aligned" in L.imf_last_error()
    for null in ("points", "normals", "nbr", "counts", "out", "workspace"):
        assert fpfh(null=null) == EINVAL, null
    assert b"imf_fpfh_features: null" in L.imf_last_error()
    assert fpfh(knn=65) == EINVAL and b"knn" in L.imf_last_error()
    assert fpfh(width=32) == EINVAL and b"width" in L.imf_last_error()
    assert fpfh(ws=16) == EINVAL and b"workspace" in L.imf_last_error()


def test_python_wrapper_refuses_bad_arguments_before_any_device_work():
    from imfnet_amd._lib import ImfError
    from imfnet_amd.matching import compute_fpfh
    pts = np.zeros((4, 3))
    with pytest.raises(ImfError, match="max_nn"):
        compute_fpfh(pts, max_nn=65, device="cpu")
    with pytest.raises(ImfError, match="max_nn"):
        compute_fpfh(pts, max_nn=0, device="cpu")
    with pytest.raises(ImfError, match="width"):
        compute_fpfh(pts, width=32, device="cpu")
    with pytest.raises(ImfError):
        compute_fpfh(np.zeros((4, 2)), device="cpu")


def test_command_lines_show_their_options():
    env = dict(os.environ, PYTHONPATH=ROOT)
    got = subprocess.run([sys.executable, "-m", "imfnet_amd.register", "--help"], env=env, cwd=ROOT, capture_output=True,
                         text=True)
    assert got.returncode == 0, got.stderr
    assert "--descriptor {imfnet,fpfh}" in got.stdout
    got = subprocess.run([sys.executable, "-m", "imfnet_amd.fpfh_desc", "--help"], env=env, cwd=ROOT, capture_output=True,
                         text=True)
    assert got.returncode == 0, got.stderr
    for opt in ("--source", "--target", "--voxel_size"):
        assert opt in got.stdout, opt
    from imfnet_amd.fpfh_desc import make_parser as desc_parser
    from imfnet_amd.register import make_parser
    args = make_parser().parse_args(["--source", "a", "--source_image", "b", "--target", "c", "--target_image", "d"])
    assert args.descriptor == "imfnet"
    args = make_parser().parse_args(["--source", "a", "--target", "c", "--descriptor", "fpfh"])
    assert args.descriptor == "fpfh" and args.source_image is None and args.target_image is None
    with pytest.raises(SystemExit):
        make_parser().parse_args(["--source", "a", "--target", "c", "--descriptor", "shot"])
    from imfnet_amd.register import main
    with pytest.raises(SystemExit):                                    # imfnet still wants its images, before anything is read
        main(["--source", "a", "--target", "c"])
    assert desc_parser().parse_args(["--source", "a", "--target", "b"]).voxel_size == 0.025
