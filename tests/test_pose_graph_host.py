"""Host side of the sequence reconstruction: the pose-graph optimiser (imfnet_amd/pose_graph.py) on a seeded graph with
false loop closures, its gauge and reachability rules, the gt.log / gt.info writers, the convention of the information
matrix's restatement (tests/information_restate.py), the C ABI's refusals and the command line.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import information_restate as IR
from imfnet_amd import pose_graph as PG
from imfnet_amd.evaluate import read_info_file, read_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CORR = 0.0375
N_NODES = 8
TRUE_LOOPS = ((0, 2), (0, 3), (1, 3), (1, 4), (2, 5), (3, 5), (3, 6), (4, 6), (4, 7), (0, 7))
FALSE_LOOPS = ((1, 6), (2, 7), (0, 5))


def _pose(rng, angle, shift):
    T = PG.euler_matrix(np.concatenate([rng.uniform(-angle, angle, 3), rng.uniform(-shift, shift, 3)]))
    return T


def _noise(rng, rot_sigma, trans_sigma):
    return PG.euler_matrix(np.concatenate([rng.normal(scale=rot_sigma, size=3), rng.normal(scale=trans_sigma, size=3)]))


def make_graph(seed, rot_sigma=0.0, trans_sigma=0.0):
    """8 nodes, 7 chain edges (certain), 10 true loop edges and 3 false ones (uncertain).  Every information matrix is
    the restatement's on 500 random points in [-1.5, 1.5]^3.  Returns (graph, true poses, is_false per edge)."""
    rng = np.random.default_rng(seed)
    truth = np.stack([np.eye(4)] + [_pose(rng, 1.0, 2.0) for _ in range(N_NODES - 1)])
    g = PG.PoseGraph(N_NODES)
    false = []
    pairs = [(k, k + 1, False, False) for k in range(N_NODES - 1)] + [(i, j, True, False) for i, j in TRUE_LOOPS] + \
            [(i, j, True, True) for i, j in FALSE_LOOPS]
    for i, j, uncertain, wrong in pairs:
        T = PG.rigid_inverse(truth[i]) @ truth[j]                    # maps fragment j's points into fragment i's frame
        if wrong:
            T = T @ _pose(rng, 0.8, 1.0)
        elif rot_sigma or trans_sigma:
            T = T @ _noise(rng, rot_sigma, trans_sigma)
        g.add_edge(i, j, T, IR.information_from_points(rng.uniform(-1.5, 1.5, (500, 3))), uncertain)
        false.append(wrong)
    return g, truth, np.array(false)


def pose_errors(X, truth):
    """(Frobenius on R, norm on t) per node."""
    return (np.linalg.norm(X[:, :3, :3] - truth[:, :3, :3], axis=(1, 2)), np.linalg.norm(X[:, :3, 3] - truth[:, :3, 3], axis=1))


def test_exact_edges_with_false_loops_recover_the_truth():
    g, truth, false = make_graph(0)
    X, l, kept, E = PG.optimize(g, MAX_CORR)
    assert np.array_equal(~kept, false), (kept, l)
    assert (l[~false] >= 0.99).all(), l
    assert (np.diff(E) <= 0.0).all(), E
    er, et = pose_errors(X, truth)
    print(f"exact edges: worst R error {er.max():.3g}, worst t error {et.max():.3g}, false l {l[false]}, "
          f"min true l {l[~false].min():.17g}, {len(E)} values of E, last {E[-1]:.3g}")
    assert er.max() <= 1e-12 and et.max() <= 1e-12, (er, et)
    assert np.array_equal(X[0], np.eye(4))


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_noisy_edges_prune_the_false_loops_and_beat_the_initial_poses(seed):
    g, truth, false = make_graph(seed, rot_sigma=0.002, trans_sigma=0.002)
    X0 = g.initial_poses()
    X, l, kept, E = PG.optimize(g, MAX_CORR)
    assert np.array_equal(~kept, false), (kept, l)
    assert (l[~false] >= 0.5).all(), l
    assert (np.diff(E) <= 0.0).all(), E
    worst = lambda P: max(max(a + b for a, b in zip(*pose_errors(P, truth))), 0.0)
    print(f"seed {seed}: worst pose error (|dR|_F + |dt|) initial {worst(X0):.3g}, optimised {worst(X):.3g} "
          f"({worst(X0) / worst(X):.1f} times smaller), min true l {l[~false].min():.3f}, max false l {l[false].max():.3g}")
    assert worst(X) < worst(X0)
    er0, et0 = pose_errors(X0, truth)
    er, et = pose_errors(X, truth)
    assert er.max() < er0.max() and et.max() < et0.max()


def test_gauge_reachability_and_a_graph_without_uncertain_edges():
    g, truth, _ = make_graph(4, rot_sigma=0.002, trans_sigma=0.002)
    X, _, _, _ = PG.optimize(g, MAX_CORR)
    assert X[0].tobytes() == np.eye(4).tobytes()                      # bit for bit
    # node 8 has no edge, node 9 hangs on node 8 only: both are left out and reported
    g2 = PG.PoseGraph(N_NODES + 2)
    for ed in g.edges:
        g2.add_edge(*ed)
    g2.add_edge(8, 9, np.eye(4), np.eye(6), False)
    init = g2.initial_poses()
    assert np.isnan(init[8:]).all() and np.isfinite(init[:8]).all()
    X2, l2, kept2, _ = PG.optimize(g2, MAX_CORR)
    assert np.isnan(X2[8:]).all() and np.array_equal(X2[:8], X)
    assert np.isnan(l2[-1]) and not kept2[-1] and np.isfinite(l2[:-1]).all()
    # certain edges only: no mu is needed (max_corr_dist is not even a number here), l is 1 and everything is kept
    g3 = PG.PoseGraph(4)
    rng = np.random.default_rng(5)
    t3 = np.stack([np.eye(4)] + [_pose(rng, 1.0, 2.0) for _ in range(3)])
    for i, j in ((0, 1), (1, 2), (2, 3), (0, 3), (3, 1)):
        g3.add_edge(i, j, PG.rigid_inverse(t3[i]) @ t3[j], IR.information_from_points(rng.uniform(-1.5, 1.5, (500, 3))), False)
    X3, l3, kept3, E3 = PG.optimize(g3, float("nan"))
    er, et = pose_errors(X3, t3)
    assert kept3.all() and (l3 == 1.0).all() and np.isfinite(E3).all() and er.max() <= 1e-12 and et.max() <= 1e-12
    # the traversal order: certain first, then higher fitness, then (i, j); an edge is walked against its direction too
    g4 = PG.PoseGraph(3)
    A, B, Cm = (_pose(rng, 1.0, 1.0) for _ in range(3))
    g4.add_edge(0, 1, A, np.eye(6), True, fitness=0.9)
    g4.add_edge(0, 1, B, np.eye(6), True, fitness=0.95)
    g4.add_edge(2, 1, Cm, np.eye(6), False, fitness=0.1)
    assert g4.traversal_order() == [2, 1, 0]
    X4 = g4.initial_poses()
    assert np.allclose(X4[1], B, rtol=0, atol=0) and np.allclose(X4[2], B @ PG.rigid_inverse(Cm), rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        g4.add_edge(0, 3, A, np.eye(6), True)
    with pytest.raises(ValueError):
        g4.add_edge(1, 1, A, np.eye(6), True)


def test_log_and_info_writers_round_trip(tmp_path):
    rng = np.random.default_rng(6)
    logs = [(0, 1, 4, _pose(rng, 1.0, 2.0)), (1, 3, 4, _pose(rng, 1.0, 2.0)), (2, 2, 4, np.eye(4))]
    infos = [(i, j, n, IR.information_from_points(rng.uniform(-1.5, 1.5, (50, 3)))) for i, j, n, _ in logs]
    PG.write_log(tmp_path / "a.log", logs)
    PG.write_info(tmp_path / "a.info", infos)
    back = read_log(tmp_path / "a.log")
    assert len(back) == 3
    for (i, j, n, T), got in zip(logs, back):
        assert got.indices == [i, j, n] and np.array_equal(got.transformation, T)          # %.17g: bit for bit
    back = read_info_file(tmp_path / "a.info")
    assert len(back) == 3
    for (i, j, n, M), got in zip(infos, back):
        assert got["test_pair"] == [i, j] and got["num_fragments"] == n
        assert got["covariance"].dtype == np.float32 and np.array_equal(got["covariance"], M.astype(np.float32))
    # one record of the 3DMatch benchmark's own gt.info (tests/golden, data only): read, write, read
    golden = os.path.join(ROOT, "tests", "golden", "redkitchen_gt_info_record.txt")
    rec = read_info_file(golden)
    assert len(rec) == 1 and rec[0]["test_pair"] == [0, 1] and rec[0]["num_fragments"] == 60
    cov = rec[0]["covariance"]
    assert cov[0, 0] == 5000.0 and np.array_equal(cov, cov.T)
    PG.write_info(tmp_path / "b.info", [(0, 1, 60, cov)])
    again = read_info_file(tmp_path / "b.info")
    assert len(again) == 1 and again[0]["test_pair"] == [0, 1] and again[0]["num_fragments"] == 60
    assert np.array_equal(again[0]["covariance"], cov)
    # the benchmark stores translation first: benchmark_order moves a rotation-first matrix there and back
    P = PG.benchmark_order(cov.astype(np.float64))
    assert (np.diag(P)[3:] == 5000.0).all() and np.array_equal(PG.benchmark_order(P), cov)
    assert (P[:3, 3:] == -P[:3, 3:].T).all()


@pytest.mark.parametrize("s", (1e-6, 1e-5, 1e-4, 1e-3))
def test_restatement_convention_rotation_first_target_point(s):
    """e^T L e is the first-order sum of squared displacements of the points L was built from: with D = U(e),
    |e^T L e - sum |D q - q|^2| <= 4 s sum |D q - q|^2 for |e|_inf = s (measured at most 0.40 s on 200 draws; the bound is ten
    times that).  A translation-first matrix or the opposite sign of G misses that gate on most draws."""
    rng = np.random.default_rng(int(round(-np.log10(s))))
    worst, missed = 0.0, np.zeros(2, int)
    flip = np.ones((6, 6))
    flip[:3, 3:] = flip[3:, :3] = -1.0
    for _ in range(50):
        q = rng.normal(size=(40, 3))
        q *= (rng.uniform(0.0, 2.0, 40) / np.linalg.norm(q, axis=1))[:, None]
        e = rng.uniform(-s, s, 6)
        e[rng.integers(0, 6)] = s * rng.choice([-1.0, 1.0])
        L = IR.information_from_points(q)
        D = PG.euler_matrix(e)
        moved = q @ D[:3, :3].T + D[:3, 3]
        want = ((moved - q) ** 2).sum()
        got = e @ L @ e
        worst = max(worst, abs(got - want) / (s * want))
        assert abs(got - want) <= 4.0 * s * want, (got, want)
        G = IR.G_of(q[0])
        assert np.allclose(G @ e, np.cross(e[:3], q[0]) + e[3:], rtol=0, atol=1e-18)      # G (w, v) = w x q + v
        for k, wrong in enumerate((PG.benchmark_order(L), L * flip)):  # translation first; the opposite sign of G
            missed[k] += abs(e @ wrong @ e - want) > 4.0 * s * want
    assert (missed > 25).all(), missed                                # the wrong conventions miss the gate on most draws
    print(f"s = {s:g}: worst |e^T L e - sum| / (s sum) = {worst:.3f}")


def test_restatement_on_a_hand_computed_pair():
    """q = (2, 2, 4): G^T G by hand."""
    r = IR.restate(np.array([[1.0, 2.0, 3.0]]), np.array([[2.0, 2.0, 4.0]]), None, 2.0)
    x, y, z = 2.0, 2.0, 4.0
    want = np.array([[y * y + z * z, -x * y, -x * z, 0, -z, y], [-x * y, x * x + z * z, -y * z, z, 0, -x],
                     [-x * z, -y * z, x * x + y * y, -y, x, 0], [0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]])
    assert r["n_corr"] == 1 and r["flag"] == 0 and np.array_equal(r["info"], want)
    assert np.array_equal(want, IR.G_of([x, y, z]).T @ IR.G_of([x, y, z]))
    empty = IR.restate(np.array([[1.0, 2.0, 3.0]]), np.array([[2.0, 2.0, 4.0]]), None, 1.0)
    assert empty["n_corr"] == 0 and empty["info"].tobytes() == np.zeros((6, 6)).tobytes()
    for case in IR.cases():
        ref = IR.restate(case.src, case.dst, case.T, case.r)
        assert ref["flag"] == 0 and (ref["n_corr"] == 0) == (case.name == "empty"), case.name
        assert case.name in ("empty", "single_pair") or 0.4 * len(case.src) < ref["n_corr"] < len(case.src), (case.name, ref["n_corr"])
    dec = IR.decision_cases()
    assert IR.restate(*dec["at_r_excluded"][1:5])["n_corr"] == 0 and IR.restate(*dec["at_r_next_up"][1:5])["n_corr"] == 1
    a, b = IR.restate(*dec["tie_lowest_index"][1:5]), IR.restate(*dec["tie_lowest_index_swapped"][1:5])
    assert a["j"][0] == 0 and b["j"][0] == 0 and not np.array_equal(a["info"], b["info"])
    assert IR.restate(*dec["nan_source_rows"][1:5])["n_corr"] == 38
    assert IR.restate(*IR.nan_target_case()[1:5])["flag"] == 1


def test_header_declares_and_library_exports_the_symbols():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    assert "GetInformationMatrixFromPointClouds" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.lib()
    for name in ("imf_information_workspace_bytes", "imf_information_matrix"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.imf_information_workspace_bytes(0, 8) == 0 and L.imf_information_workspace_bytes(8, 0) == 0
    assert L.imf_information_workspace_bytes(1 << 30, 8) == 0 and L.imf_information_workspace_bytes(8, 1 << 30) == 0
    assert 0 < L.imf_information_workspace_bytes(1, 1) < L.imf_information_workspace_bytes(100000, 100000)
    assert L.imf_information_workspace_bytes(257, 300) % 256 == 0


def test_argument_errors_return_a_status_without_a_gpu():
    """Every refusal comes before any device call, so it answers on a machine without a GPU (host pointers here)."""
    from imfnet_amd import _lib
    L = _lib.lib()
    buf = np.zeros(1 << 16, dtype=np.float64)
    p = buf.ctypes.data
    p += (-p) % 256
    EINVAL = -1
    names = ("src", "dst", "T", "info", "meta", "workspace")
    need = L.imf_information_workspace_bytes(8, 8)

    def call(n_src=8, n_dst=8, r=0.1, null=None, ws=need, ws_ptr=None):
        ptr = {k: (None if k == null else p) for k in names}
        if ws_ptr is not None:
            ptr["workspace"] = ws_ptr
        return L.imf_information_matrix(ptr["src"], n_src, ptr["dst"], n_dst, ptr["T"], r, ptr["info"], ptr["meta"],
                                        ptr["workspace"], ws, None)

    for kw in (dict(n_src=0), dict(n_dst=0), dict(n_src=-1), dict(n_src=1 << 30), dict(n_dst=1 << 30), dict(r=0.0),
               dict(r=-1.0), dict(r=float("nan")), dict(r=1e6), dict(ws=0), dict(ws=need - 1), dict(ws_ptr=p + 8)):
        assert call(**kw) == EINVAL, kw
    assert b"imf_information_matrix" in L.imf_last_error() and b"aligned" in L.imf_last_error()
    for null in ("src", "dst", "info", "meta", "workspace"):
        assert call(null=null) == EINVAL, null
    assert b"imf_information_matrix: null" in L.imf_last_error()
    assert call(ws=need - 1) == EINVAL and b"workspace" in L.imf_last_error()


def test_command_line_and_the_split_of_register_pair():
    env = dict(os.environ, PYTHONPATH=ROOT)
    got = subprocess.run([sys.executable, "-m", "imfnet_amd.reconstruct", "--help"], env=env, cwd=ROOT, capture_output=True,
                         text=True)
    assert got.returncode == 0, got.stderr
    for opt in ("--fragments", "--descriptor {imfnet,fpfh}", "--voxel_size", "--refine", "--min_fitness", "--pairs",
                "--preference_loop_closure", "--merge_voxel", "--out", "--seed"):
        assert opt in got.stdout, opt
    from imfnet_amd.reconstruct import make_parser, read_pairs
    args = make_parser().parse_args(["--fragments", "d", "--out", "o"])
    assert args.descriptor == "fpfh" and args.voxel_size == 0.025 and args.refine == "plane" and args.min_fitness == 0.3
    assert args.pairs == "all" and args.preference_loop_closure == 1.0 and args.merge_voxel is None
    assert read_pairs("all", 4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    from imfnet_amd import register
    assert callable(register.fragment_features) and callable(register.register_features) and callable(register.register_pair)
