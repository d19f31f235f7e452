"""`python -m imfnet_amd.reconstruct --descriptor fpfh` on four overlapping windows of the fixture fragment, each moved by
a known rigid motion: the consecutive pairs must become kept edges, the files must parse, and every optimised pose must be
the known one within the per-edge bound of tests/test_gpu_register_fpfh.py accumulated along the longest path from
fragment 0.  No checkpoint, no images."""
import json
import os

import numpy as np
import pytest

from kitti_restate import rigid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4
WIDTH, STEP = 1.0 / 1.84, 0.28 / 1.84                 # windows in rank along the longest axis: consecutive ones share 72 %
POSES = (np.eye(4), rigid(9.0, [0.2, 1.0, -0.3], [0.31, -0.12, 0.22]), rigid(15.0, [-1.0, 0.3, 0.5], [-0.2, 0.4, 0.1]),
         rigid(12.0, [0.4, -0.2, 1.0], [0.25, 0.3, -0.3]))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Fragment k = X_k^-1 . window k as cloud_bin_k.ply, and one run of the command on them."""
    from imfnet_amd.dataio import read_ply_points
    from imfnet_amd.fuse_fragments import write_ply
    from imfnet_amd.pose_graph import rigid_inverse
    from imfnet_amd.reconstruct import main
    d = tmp_path_factory.mktemp("reconstruct")
    os.makedirs(d / "frags")
    cloud = np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))["cloud_bin_0"][::4].astype(np.float64)
    axis = int(np.argmax(cloud.max(0) - cloud.min(0)))
    rank = np.empty(len(cloud))
    rank[np.argsort(cloud[:, axis], kind="stable")] = (np.arange(len(cloud)) + 0.5) / len(cloud)
    members, frags = [], []
    for k in range(N):
        inside = (rank >= k * STEP) & (rank < k * STEP + WIDTH)
        members.append(inside)
        inv = rigid_inverse(POSES[k])
        write_ply(str(d / "frags" / f"cloud_bin_{k}.ply"), cloud[inside] @ inv[:3, :3].T + inv[:3, 3])
        frags.append(read_ply_points(str(d / "frags" / f"cloud_bin_{k}.ply")))
    import contextlib
    import io
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert main(["--fragments", str(d / "frags"), "--descriptor", "fpfh", "--merge_voxel", "0.025", "--out",
                     str(d / "out")]) == 0
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return d / "out", json.loads(lines[0]), members, frags


def test_windows_overlap_as_the_test_claims(run):
    _, _, members, _ = run
    for k in range(N - 1):
        both = (members[k] & members[k + 1]).sum()
        assert both >= 0.7 * members[k].sum() and both >= 0.7 * members[k + 1].sum()
    assert 0 < (members[0] & members[3]).sum() < 0.2 * members[0].sum()
    for k in range(1, N):
        R, t = POSES[k][:3, :3], POSES[k][:3, 3]
        assert np.degrees(np.arccos((np.trace(R) - 1) / 2)) <= 15.0 + 1e-9 and np.linalg.norm(t) <= 0.5


def test_reconstruct_returns_the_known_poses_and_writes_a_benchmark_tree(run):
    from imfnet_amd.dataio import read_ply_points
    from imfnet_amd.evaluate import read_info_file, read_log
    from imfnet_amd.pose_graph import rigid_inverse
    out, line, _, frags = run
    graph = json.load(open(out / "graph.json"))
    edges = {(e["i"], e["j"]): e for e in graph["edges"]}
    print("\nreconstruct, 4 windows of the fixture fragment:")
    for (i, j), e in sorted(edges.items()):
        print(f"  edge ({i}, {j}): fitness {e['fitness']:.4f}, n_corr {e['n_corr']}, uncertain {e['uncertain']}, "
              f"l {e['l']}, kept {e['kept']}")
    print(f"  below --min_fitness: {graph['rejected']}\n  times {graph['times']}, {len(graph['E'])} values of E, "
          f"first {graph['E'][0]:.3e}, last {graph['E'][-1]:.3e}")
    # the three consecutive edges are kept, and certain
    for k in range(N - 1):
        assert (k, k + 1) in edges and edges[(k, k + 1)]["kept"] and not edges[(k, k + 1)]["uncertain"]
    assert all(e["uncertain"] for (i, j), e in edges.items() if j != i + 1)
    assert graph["unreached"] == [] and graph["fragments"] == N and (np.diff(graph["E"]) <= 0).all()
    assert {"features", "register", "information", "optimize"} <= set(graph["times"])
    assert line["fragments"] == N and line["pairs"] == 6 and line["edges"] == len(edges) and line["unreached"] == []
    assert line["kept"] == sum(e["kept"] for e in edges.values())

    # the files parse; pairs.log / pairs.info are the kept edges, in the benchmark's layout
    kept = sorted(k for k, e in edges.items() if e["kept"])
    logs, infos = read_log(out / "pairs.log"), read_info_file(out / "pairs.info")
    assert [tuple(p.indices) for p in logs] == [(i, j, N) for i, j in kept]
    assert [tuple(r["test_pair"]) for r in infos] == kept and all(r["num_fragments"] == N for r in infos)
    for (i, j), p, r in zip(kept, logs, infos):
        T, cov = p.transformation, r["covariance"]
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), rtol=0, atol=1e-9) and np.array_equal(T[3], [0, 0, 0, 1])
        assert cov[0, 0] == cov[1, 1] == cov[2, 2] == edges[(i, j)]["n_corr"] and np.array_equal(cov, cov.T)
        assert not cov[:3, :3][~np.eye(3, dtype=bool)].any() and (np.diag(cov)[3:] > 0).all()
    traj = read_log(out / "trajectory.log")
    assert [tuple(p.indices) for p in traj] == [(k, k, N) for k in range(N)]
    assert np.array_equal(traj[0].transformation, np.eye(4))

    # every pose within the accumulated per-edge bound: 1e-3 in rotation (Frobenius), 2 mm + 1e-3 times the longest lever
    # arm in translation, times the N - 1 edges of the longest path from fragment 0
    lever = max(float(np.linalg.norm(f, axis=1).max()) for f in frags)
    rot_bound, tr_bound = (N - 1) * 1e-3, (N - 1) * (2e-3 + 1e-3 * lever)
    print(f"  lever arm {lever:.3f} m: bounds {rot_bound:.1e} and {tr_bound:.3e} m")
    worst = [0.0, 0.0]
    for k in range(N):
        X = traj[k].transformation
        rot, tr = float(np.linalg.norm(X[:3, :3] - POSES[k][:3, :3])), float(np.linalg.norm(X[:3, 3] - POSES[k][:3, 3]))
        print(f"  pose {k}: rotation off {rot:.3e}, translation off {tr:.3e} m")
        worst = [max(worst[0], rot), max(worst[1], tr)]
    for (i, j), p in zip(kept, logs):
        want = rigid_inverse(POSES[i]) @ POSES[j]
        print(f"  kept edge ({i}, {j}): rotation off {np.linalg.norm(p.transformation[:3, :3] - want[:3, :3]):.3e}, "
              f"translation off {np.linalg.norm(p.transformation[:3, 3] - want[:3, 3]):.3e} m")
    assert worst[0] <= rot_bound and worst[1] <= tr_bound, worst

    # scene.ply: one point per 2.5 cm voxel, more than any fragment has, fewer than all of them together
    from imfnet_amd.extract import voxel_representatives
    scene = read_ply_points(str(out / "scene.ply"))
    counts = [len(voxel_representatives(f, 0.025)) for f in frags]
    print(f"  scene.ply: {len(scene)} points; the fragments' voxel counts {counts}")
    assert 0.9 * max(counts) < len(scene) < sum(counts)
