"""Host side of the k-NN normals, the point-to-plane ICP and `python -m imfnet_amd.register`: the NumPy restatements
(tests/normals_restate.py, tests/plane_icp_restate.py) against independent CPU references (scipy's cKDTree,
numpy.linalg.eigh), the C ABI's refusals, the command lines, the PLY with normals through the native reader.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import normals_restate as NR
import plane_icp_restate as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("imf_normals_workspace_bytes", "imf_estimate_normals", "imf_icp_plane_workspace_bytes", "imf_icp_point_to_plane")
CASES = NR.cases()


def _kdtree_lists(case):
    """The neighbour lists from cKDTree's candidates, re-sorted by (d^2, index) with the restated d^2: 16 more than knn are
    asked for, so a group of equal d^2 across the knn-th place is seen whole (the largest group here has 12 members)."""
    from scipy.spatial import cKDTree
    pts, n = case.points, len(case.points)
    k = min(n, case.knn + 16)
    _, j = cKDTree(pts).query(pts, k=k, distance_upper_bound=case.max_radius * (1 + 1e-9))
    j = j.reshape(n, k)
    out = np.full((n, case.knn), -1, np.int32)
    counts = np.zeros(n, np.int32)
    r2 = case.max_radius * case.max_radius
    for i in range(n):
        cand = j[i][j[i] < n]
        d2 = NR.dist2(pts[i:i + 1], pts[cand])[0]
        keep = d2 <= r2
        cand, d2 = cand[keep], d2[keep]
        order = np.lexsort((cand, d2))[:case.knn]
        out[i, :len(order)] = cand[order]
        counts[i] = len(order)
    return out, counts


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_restated_neighbours_match_ckdtree_and_normals_pass_the_gates(case):
    ref = NR.reference(case, None)
    nbr, counts = _kdtree_lists(case)
    assert np.array_equal(ref["counts"], counts)
    assert np.array_equal(ref["nbr"], nbr)
    assert (ref["nbr"][:, 0] >= 0).all()                               # every point finds itself or an earlier duplicate
    for vp in (None, NR.VIEWPOINT):
        got = NR.check_normals(NR.reference(case, vp)["normals"], case.points, ref, vp)
        if case.generic:
            assert got["under_gap"] <= 0.10, got                       # the seed keeps the restatement itself within the cap
    # the direction against LAPACK where the gap decides it
    lam, vec = np.linalg.eigh(ref["cov"])
    sure = (counts >= 3) & (lam[:, 2] > 0) & ((lam[:, 1] - lam[:, 0]) >= NR.GAP * lam[:, 2])
    n0 = vec[:, :, 0]
    sin = np.linalg.norm(np.cross(n0, ref["normals"]), axis=1)
    assert not sure.any() or float(sin[sure].max()) <= 1e-9


def test_case_catalogue_has_the_edges_it_claims():
    by = {c.name: c for c in CASES}
    assert all(len(c.points) <= 4096 for c in CASES)
    lat = NR.reference(by["lattice_plane_ties"], None)
    inner = lat["counts"] == 10
    assert inner.any()
    pts = by["lattice_plane_ties"].points
    d2 = ((pts[lat["nbr"][inner, 9]] - pts[inner]) ** 2).sum(1)
    assert (d2 == 4.0).any()                                            # the 10th place sits inside a group of four at d^2 = 4
    assert (np.linalg.eigvalsh(lat["cov"])[:, 0] == 0.0).all() and (lat["normals"] == [0.0, 0.0, 1.0]).all()
    assert (NR.reference(by["two_clusters"], None)["counts"] == 10).all()
    assert (NR.reference(by["n2_knn30"], None)["normals"] == [0.0, 0.0, 1.0]).all()
    dup = NR.reference(by["exact_duplicates"], None)
    assert (dup["nbr"][:, 0] != np.arange(len(dup["nbr"]))).sum() >= 50  # a later duplicate lists the first occurrence first
    col = NR.reference(by["collinear_axis"], None)
    assert (np.linalg.eigvalsh(col["cov"])[:, 1] == 0.0).all()


def test_plane_restatement_recovers_a_known_motion_and_moves_little_with_the_order():
    src, dst, nrm, r, truth = PR.bumpy_case()
    init = truth @ PR.rigid(1.0, [1.0, 0.2, -0.4], np.array([0.004, 0.003, -0.002]))
    fwd, rev, moved, tol = PR.tolerances(src, dst, nrm, r, init, 30)
    assert fwd[3] == rev[3] and fwd[4] == rev[4] == len(src)
    assert np.abs(fwd[0] - truth).max() < 1e-6 and fwd[3] < 30
    assert moved[0] < 1e-9 and all(t >= 1e-12 for t in tol)
    # the solver against LAPACK, and the singular rule on a single-plane target
    g = np.random.default_rng(2)
    A = g.normal(size=(40, 6))
    A, b = A.T @ A, g.normal(size=6)
    assert np.abs(PR.ldl_solve(A, b) - np.linalg.solve(A, b)).max() < 1e-12
    plane = np.concatenate([g.uniform(-1, 1, (50, 2)), np.zeros((50, 1))], 1)
    up = np.tile([[0.0, 0.0, 1.0]], (50, 1))
    assert np.array_equal(PR.plane_update(plane + [0.01, 0.0, 0.02], plane, up), np.eye(4))
    assert np.array_equal(PR.plane_update(plane[:0], plane[:0], up[:0]), np.eye(4))


def test_header_declares_and_library_exports_the_symbols():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    assert "Replaces: o3d.geometry.PointCloud.estimate_normals" in text and "KDTreeSearchParamKNN(knn=30)" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.imf_normals_workspace_bytes(0) == 0 and L.imf_normals_workspace_bytes(1 << 30) == 0
    assert 0 < L.imf_normals_workspace_bytes(1) < L.imf_normals_workspace_bytes(100000)
    assert L.imf_icp_plane_workspace_bytes(0, 5) == 0 and L.imf_icp_plane_workspace_bytes(5, 0) == 0
    assert L.imf_icp_plane_workspace_bytes(1000, 1000) > L.imf_icp_workspace_bytes(1000, 1000)


def test_argument_errors_return_a_status_without_a_gpu():
    """Every refusal comes before any device call, so it answers on a machine without a GPU (host pointers here)."""
    from imfnet_amd import _lib
    L = _lib.lib()
    buf = np.zeros(1 << 16, dtype=np.float64)
    p = buf.ctypes.data
    p += (-p) % 256
    EINVAL = -1
    vp = np.zeros(3)

    def normals(n=8, knn=30, radius=0.1, view=vp, null=None, ws=None, ws_ptr=None):
        ptr = {k: (None if k == null else p) for k in ("points", "normals", "counts", "nbr", "err", "workspace")}
        if ws_ptr is not None:
            ptr["workspace"] = ws_ptr
        nbytes = L.imf_normals_workspace_bytes(8) if ws is None else ws
        return L.imf_estimate_normals(ptr["points"], n, knn, radius, view.ctypes.data if view is not None else None,
                                      ptr["normals"], ptr["counts"], ptr["nbr"], ptr["err"], ptr["workspace"], nbytes, None)

    for kw in (dict(n=0), dict(n=-1), dict(n=1 << 30), dict(knn=0), dict(knn=65), dict(knn=-4), dict(radius=0.0),
               dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
               dict(view=np.array([0.0, float("nan"), 0.0])), dict(view=np.array([float("inf"), 0.0, 0.0])),
               dict(ws=0), dict(ws=L.imf_normals_workspace_bytes(8) - 1), dict(ws_ptr=p + 8)):
        assert normals(**kw) == EINVAL, kw
    assert b"aligned" in L.imf_last_error()
    for null in ("points", "normals", "counts", "err", "workspace"):
        assert normals(null=null) == EINVAL, null
    assert b"null" in L.imf_last_error()
    assert normals(knn=65) == EINVAL and b"knn" in L.imf_last_error()

    def plane(n_src=8, n_dst=8, r=0.1, it=30, null=None, ws=None):
        ptr = {k: (None if k == null else p) for k in ("src", "dst", "nrm", "T", "stats", "meta", "workspace")}
        nbytes = L.imf_icp_plane_workspace_bytes(8, 8) if ws is None else ws
        return L.imf_icp_point_to_plane(ptr["src"], n_src, ptr["dst"], ptr["nrm"], n_dst, r, None, it, ptr["T"],
                                        ptr["stats"], ptr["meta"], ptr["workspace"], nbytes, None)

    for kw in (dict(n_src=0), dict(n_dst=0), dict(n_src=1 << 30), dict(r=0.0), dict(r=float("nan")), dict(r=1e6),
               dict(it=-1), dict(it=100001), dict(ws=0), dict(ws=L.imf_icp_plane_workspace_bytes(8, 8) - 1)):
        assert plane(**kw) == EINVAL, kw
    assert b"workspace" in L.imf_last_error()
    for null in ("src", "dst", "nrm", "T", "stats", "meta", "workspace"):
        assert plane(null=null) == EINVAL, null
    assert b"null" in L.imf_last_error()


def test_python_wrappers_refuse_bad_shapes_before_any_device_work():
    from imfnet_amd._lib import ImfError
    from imfnet_amd.matching import estimate_normals, icp_point_to_plane
    with pytest.raises(ImfError):
        estimate_normals(np.zeros((0, 3)), device="cpu")
    with pytest.raises(ImfError):
        estimate_normals(np.zeros((4, 2)), device="cpu")
    with pytest.raises(ImfError):
        icp_point_to_plane(np.zeros((4, 3)), np.zeros((5, 3)), np.zeros((4, 3)), 0.1, device="cpu")


def test_command_lines_show_their_options():
    env = dict(os.environ, PYTHONPATH=ROOT)
    got = subprocess.run([sys.executable, "-m", "imfnet_amd.register", "--help"], env=env, cwd=ROOT, capture_output=True,
                         text=True)
    assert got.returncode == 0, got.stderr
    for opt in ("--source", "--source_image", "--target", "--target_image", "-m", "--voxel_size", "--num_keypoints",
                "--ransac_iter", "--seed", "--init", "--skip_global", "--refine {none,point,plane}", "--out"):
        assert opt in got.stdout, opt
    from imfnet_amd import fuse_fragments as FF
    from imfnet_amd.register import make_parser
    args = make_parser().parse_args(["--source", "a", "--source_image", "b", "--target", "c", "--target_image", "d"])
    assert (args.voxel_size, args.num_keypoints, args.ransac_iter, args.seed, args.refine) == (0.025, 5000, 50000, 0, "plane")
    assert args.model is None and args.init is None and not args.skip_global
    with pytest.raises(SystemExit):
        make_parser().parse_args(["--source", "a", "--source_image", "b", "--target", "c", "--target_image", "d",
                                  "--refine", "gicp"])
    assert FF.parse_args(["--dataset_root", "a", "--out_root", "b"]).normals is False
    assert FF.parse_args(["--dataset_root", "a", "--out_root", "b", "--normals"]).normals is True


def test_ply_with_normals_reads_back_with_the_bytes_of_the_plain_file(tmp_path):
    """imf_ply_read_points skips the extra vertex properties by stride."""
    from imfnet_amd.dataio import read_ply_points, read_ply_points_numpy
    from imfnet_amd.fuse_fragments import write_ply, write_ply_normals
    g = np.random.default_rng(1)
    xyz = g.normal(size=(257, 3))
    nrm = g.normal(size=(257, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    write_ply(str(tmp_path / "plain.ply"), xyz)
    write_ply_normals(str(tmp_path / "normals.ply"), xyz, nrm)
    a, b = read_ply_points(str(tmp_path / "plain.ply")), read_ply_points(str(tmp_path / "normals.ply"))
    assert a.tobytes() == b.tobytes() == xyz.astype(np.float32).astype(np.float64).tobytes()
    assert np.array_equal(read_ply_points_numpy(str(tmp_path / "normals.ply")), a)
    head, body = open(tmp_path / "normals.ply", "rb").read().split(b"end_header\n", 1)
    assert b"property float nx\nproperty float ny\nproperty float nz\n" in head and len(body) == 257 * 24
    rows = np.frombuffer(body, "<f4").reshape(257, 6)
    assert np.array_equal(rows[:, 3:], nrm.astype(np.float32)) and not os.path.exists(tmp_path / "normals.ply.tmp")
    write_ply_normals(str(tmp_path / "empty.ply"), np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(read_ply_points(str(tmp_path / "empty.ply"))) == 0
