"""imf_color_gradient and imf_icp_colored (csrc/colored_icp.hip, csrc/icp.hip) against the NumPy restatement
(tests/colored_icp_restate.py), and `--refine color` of `register` and `reconstruct`.

Tolerances.  The gradient of a point gets 16 times what the restatement moved between the forward and the reversed order
of its list positions, at least 1e-12 times the sum over its listed neighbours of |I_p' - I_p| / |u|
(colored_icp_restate.gradient_tolerance).  The joint fit gets 16 times what T, fitness and rmse moved between the forward
and the reversed order of the source rows, at least 1e-12 (colored_icp_restate.tolerances); the iteration count and the
number of correspondences must be equal.  Both movements are measured on the CPU when the test runs."""
import json
import os

import numpy as np
import pytest

import colored_icp_restate as CR
import normals_restate as NR
import plane_icp_restate as PR
from kitti_restate import rigid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the gradient ------------------------------------------------------------------------------------------------------
def _gradient_cases():
    surf, nrm = PR.bumpy_surface(41, seed=3)
    order = np.random.default_rng(31).permutation(len(surf))
    out = []
    for n in (1, 3, 4, 63, 64, 65):                                     # full lanes and the cloud-size edge
        out.append((f"n{n}_knn64", surf[order[:n]], nrm[order[:n]], 64, 10.0))
    for n in (255, 256, 257):                                           # workgroup edges (4 points per workgroup)
        out.append((f"n{n}_knn30", surf[order[:n]], nrm[order[:n]], 30, 0.4))
    out.append(("short_lists_knn30", surf, nrm, 30, 0.06))              # most counts far below knn: -1 padding
    return out


GRADIENT_CASES = _gradient_cases()


def _check_gradient(name, pts, nrm, inten, nbr, counts):
    from imfnet_amd.matching import color_gradient
    fwd, moved, bound = CR.gradient_tolerance(pts, nrm, inten, nbr, counts)
    got = color_gradient(pts, nrm, inten, nbr, counts)
    err = np.abs(got - fwd).max(1)
    same = (got == CR.gradient_restated(pts, nrm, inten, nbr, counts, "butterfly")).all(1).sum()
    share = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    print(f"{name}: n {len(pts)}, counts {counts.min()}..{counts.max()}, order moved <= {moved.max():.2e}, kernel off <= "
          f"{err.max():.2e}, worst share of its bound {share.max():.2e}; {same} rows equal the butterfly restatement's bits")
    assert got.dtype == np.float64 and got.shape == (len(pts), 3)
    assert (err <= bound).all()
    assert (got[counts < 4] == 0.0).all()
    assert color_gradient(pts, nrm, inten, nbr, counts).tobytes() == got.tobytes()        # equal bits
    return got


@pytest.mark.parametrize("case", GRADIENT_CASES, ids=[c[0] for c in GRADIENT_CASES])
def test_gradient_against_the_restatement(case):
    name, pts, nrm, knn, radius = case
    nbr, counts = NR.neighbors(pts, knn, radius)
    if name.startswith("short"):
        assert np.median(counts) < 10 and (counts < 4).any() and (nbr[:, -1] == -1).all()
    _check_gradient(name, pts, nrm, CR.texture(pts), nbr, counts)


def test_gradient_of_the_painted_bumpy_cloud_and_of_the_textured_plane():
    for name, c in (("painted bumpy", CR.painted_bumpy()), ("textured plane", CR.textured_plane())):
        assert len(c["dst"]) == 1681
        _check_gradient(name, c["dst"], c["normals"], c["dst_I"], c["nbr"], c["counts"])


@pytest.mark.parametrize("case", CR.exact_cases(), ids=[c["name"] for c in CR.exact_cases()])
def test_exact_cases_of_the_gradient_hold_on_the_gpu(case):
    from imfnet_amd.matching import color_gradient
    args = (case["points"], case["normals"], case["inten"], case["nbr"], case["counts"])
    got = color_gradient(*args)
    if case["to_bound"]:
        _, _, bound = CR.gradient_tolerance(*args)
        assert (np.abs(got - case["want"]).max(1) <= bound).all()
    else:
        assert (got == case["want"]).all()


def test_lists_of_estimate_normals_feed_the_gradient():
    """The lists the wrapper computes on the device are the restatement's, so the two paths of icp_colored agree in bits."""
    from imfnet_amd.matching import color_gradient, estimate_normals, icp_colored
    c = CR.painted_bumpy()
    _, counts, nbr = estimate_normals(c["dst"], knn=CR.GRAD_KNN, max_radius=CR.GRAD_RADIUS, return_neighbors=True)
    assert np.array_equal(nbr, c["nbr"]) and np.array_equal(counts, c["counts"])
    grad = color_gradient(c["dst"], c["normals"], c["dst_I"], nbr, counts)
    a = icp_colored(c["src"], c["src_I"], c["dst"], c["normals"], c["dst_I"], c["r"], dst_gradient=grad)
    b = icp_colored(c["src"], c["src_I"], c["dst"], c["normals"], c["dst_I"], c["r"], gradient_knn=CR.GRAD_KNN,
                    gradient_radius=CR.GRAD_RADIUS)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]


# ---- the joint fit -----------------------------------------------------------------------------------------------------
def _compare(c, rows, max_iteration, name, init=None):
    from imfnet_amd.matching import icp_colored
    src, src_I = c["src"][:rows], c["src_I"][:rows]
    args = (c["dst"], c["normals"], c["dst_I"])
    fwd, rev, moved, tol = CR.tolerances(src, src_I, *args, c["grad"], c["r"], c["lam"], init, max_iteration)
    run = lambda: icp_colored(src, src_I, *args, c["r"], init=init, max_iteration=max_iteration, lambda_geometric=c["lam"],
                              dst_gradient=c["grad"])
    T, fit, rmse, iters, n_corr = run()
    err = (float(np.abs(T - fwd[0]).max()), abs(fit - fwd[1]), abs(rmse - fwd[2]))
    print(f"{name}: {len(src)} rows, iterations {iters} (restated {fwd[3]}), n_corr {n_corr} (restated {fwd[4]}), order "
          f"moved {moved}, bounds {tol}, kernel off by {err}")
    assert fwd[3] == rev[3] and fwd[4] == rev[4]
    assert iters == fwd[3] and n_corr == fwd[4]
    assert err[0] <= tol[0] and err[1] <= tol[1] and err[2] <= tol[2]
    again = run()
    assert again[0].tobytes() == T.tobytes() and again[1:] == (fit, rmse, iters, n_corr)      # equal bits
    return T, fwd


@pytest.mark.parametrize("rows", [1, 255, 256, 257])
@pytest.mark.parametrize("target", ["plane", "bumpy"])
def test_one_iteration_at_the_block_edges(target, rows):
    c = CR.textured_plane() if target == "plane" else CR.painted_bumpy()
    T, fwd = _compare(c, rows, 1, f"one iteration, {target}")
    assert fwd[3] == 1 and fwd[4] == rows
    if rows == 1:
        assert np.array_equal(T, np.eye(4))                               # one row: singular, the identity update
    else:
        assert np.abs(T - np.eye(4)).max() > 1e-3


def test_textured_plane_colour_finds_the_motion_point_to_plane_cannot():
    from imfnet_amd.matching import icp_point_to_plane
    c = CR.textured_plane()
    T, fwd = _compare(c, len(c["src"]), 30, "convergence, textured plane")
    plane = icp_point_to_plane(c["src"], c["dst"], c["normals"], c["r"], max_iteration=30)
    start, end = CR.off(np.eye(4), c["truth"]), CR.off(T, c["truth"])
    print(f"textured plane on the GPU: start {start[0]:.2e} / {start[1] * 1e3:.2f} mm, colour ends {end[0]:.2e} / "
          f"{end[1] * 1e3:.3f} mm off after {fwd[3]} iterations; point-to-plane ended at iteration {plane[3]}")
    assert np.array_equal(plane[0], np.eye(4)) and plane[3] <= 1
    assert 10.0 * end[0] <= start[0] and 10.0 * end[1] <= start[1]


def test_painted_bumpy_surface_converges_like_the_restatement():
    from imfnet_amd.matching import icp_point_to_plane
    c = CR.painted_bumpy()
    T, fwd = _compare(c, len(c["src"]), 30, "convergence, painted bumpy surface")
    plane = icp_point_to_plane(c["src"], c["dst"], c["normals"], c["r"], max_iteration=30)
    p, k = CR.off(plane[0], c["truth"]), CR.off(T, c["truth"])
    print(f"painted bumpy surface on the GPU: point-to-plane {p[0]:.2e} / {p[1] * 1e3:.3f} mm, colour {k[0]:.2e} / "
          f"{k[1] * 1e3:.3f} mm")
    assert 2 <= fwd[3] < 30 and k[0] <= 2.0 * p[0] + 1e-4 and k[1] <= 2.0 * p[1] + 1e-4


@pytest.mark.parametrize("target", ["plane", "bumpy"])
def test_lambda_one_equals_point_to_plane(target):
    from imfnet_amd.matching import icp_colored, icp_point_to_plane
    c = CR.textured_plane() if target == "plane" else CR.painted_bumpy()
    for it in (1, 30):
        plane = icp_point_to_plane(c["src"], c["dst"], c["normals"], c["r"], max_iteration=it)
        color = icp_colored(c["src"], c["src_I"], c["dst"], c["normals"], c["dst_I"], c["r"], max_iteration=it,
                            lambda_geometric=1.0, dst_gradient=c["grad"])
        assert np.array_equal(plane[0], color[0]) and plane[1:] == color[1:]
    if target == "bumpy":
        assert plane[3] >= 2 and not np.array_equal(plane[0], np.eye(4))


def test_constant_colour_on_the_plane_is_singular_like_point_to_plane():
    from imfnet_amd.matching import icp_colored
    c = CR.textured_plane()
    grey_s, grey_d = np.full(len(c["src"]), 0.5), np.full(len(c["dst"]), 0.5)
    T, fit, rmse, iters, n_corr = icp_colored(c["src"], grey_s, c["dst"], c["normals"], grey_d, c["r"], max_iteration=5,
                                              gradient_knn=CR.GRAD_KNN, gradient_radius=CR.GRAD_RADIUS)
    assert np.array_equal(T, np.eye(4)) and iters <= 1 and n_corr == len(c["src"])


def test_no_iteration_counts_the_correspondences_of_point_to_point():
    from imfnet_amd.matching import icp_colored, icp_point_to_point
    c = CR.painted_bumpy()
    far = c["src"] + np.array([0.5, 0.0, 0.0])                          # the rows pushed off the target's edge find nothing
    color = icp_colored(far, c["src_I"], c["dst"], c["normals"], c["dst_I"], c["r"], max_iteration=0, dst_gradient=c["grad"])
    point = icp_point_to_point(far, c["dst"], c["r"], max_iteration=0)
    assert np.array_equal(color[0], np.eye(4)) and color[1:] == point[1:] and 0 < color[4] < len(far) and color[3] == 0


def test_contract_refusals_and_a_nan_target():
    from imfnet_amd import _lib
    from imfnet_amd._lib import ImfError
    from imfnet_amd.matching import icp_colored
    CR.check_refusals(_lib.lib())
    c = CR.painted_bumpy()
    bad = c["dst"].copy()
    bad[5, 1] = np.nan
    with pytest.raises(ImfError):
        icp_colored(c["src"], c["src_I"], bad, c["normals"], c["dst_I"], c["r"], dst_gradient=c["grad"])
    for lam in (-0.1, 1.1, float("nan")):
        with pytest.raises(ImfError, match="lambda_geometric"):
            icp_colored(c["src"], c["src_I"], c["dst"], c["normals"], c["dst_I"], c["r"], lambda_geometric=lam,
                        dst_gradient=c["grad"])


# ---- register and reconstruct ------------------------------------------------------------------------------------------
PAINT_DIR = np.array([[0.8, 0.36, 0.48], [-0.28, 0.96, 0.0], [0.6, 0.0, -0.8]])      # unit vectors, one per channel
PAINT_RATE = np.array([3.1, 3.7, 2.3])                                               # radians per metre
PAINT_PHASE = np.array([0.3, 1.7, 4.1])
ROT_BOUND, TR_BOUND = 1e-3, 2e-3 + 1e-3 * 3.98                          # the per-edge bound of this fixture


def paint(points):
    """uint8 [n, 3]: a smooth colour of the position, every channel with its own direction, rate and phase."""
    p = np.asarray(points, np.float64)
    return np.rint(127.5 + 100.0 * np.sin(PAINT_RATE * (p @ PAINT_DIR.T) + PAINT_PHASE)).astype(np.uint8)


def _fixture_cloud():
    return np.load(os.path.join(ROOT, "tests", "golden", "fixture_clouds.npz"))["cloud_bin_0"][::4].astype(np.float64)


def test_voxel_representatives_return_their_rows():
    from imfnet_amd.extract import voxel_representatives
    cloud = _fixture_cloud()
    xyz, index = voxel_representatives(cloud, 0.025, return_index=True)
    assert index.dtype == np.int64 and index.shape == (len(xyz),) and len(np.unique(index)) == len(index)
    assert np.array_equal(cloud[index], xyz) and np.array_equal(voxel_representatives(cloud, 0.025), xyz)


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """The fixture fragment (every 4th point) painted by its position, a rigidly moved copy with the same colours, a start
    off by 2 degrees about the middle and 3 cm, and an unpainted copy."""
    from imfnet_amd.dataio import read_ply_points
    from imfnet_amd.fuse_fragments import write_ply
    d = tmp_path_factory.mktemp("register_color")
    cloud = _fixture_cloud()
    rgb = paint(cloud)
    write_ply(str(d / "a.ply"), cloud, rgb=rgb)
    a = read_ply_points(str(d / "a.ply"))
    truth = rigid(11.0, [0.2, 1.0, -0.3], np.array([0.31, -0.12, 0.22]))
    write_ply(str(d / "b.ply"), a @ truth[:3, :3].T + truth[:3, 3], rgb=rgb)
    write_ply(str(d / "plain.ply"), a)
    mid = a.mean(0)
    off = rigid(2.0, [1.0, -0.4, 0.5], np.zeros(3))
    off[:3, 3] = mid - off[:3, :3] @ mid + np.array([0.02, -0.02, 0.01])          # |t| = 3 cm
    np.savetxt(str(d / "init.txt"), truth @ off, fmt="%.17g")
    return d, truth


def _register(capsys, argv):
    from imfnet_amd.register import main
    capsys.readouterr()
    assert main(argv) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_register_refine_color_returns_the_known_motion(pair, capsys):
    d, truth = pair
    base = ["--descriptor", "fpfh", "--source", str(d / "a.ply"), "--target", str(d / "b.ply"), "--skip_global", "--init",
            str(d / "init.txt")]
    got = {}
    for refine in ("plane", "color"):
        out = str(d / f"T_{refine}.txt")
        res = _register(capsys, base + ["--refine", refine, "--out", out])
        got[refine] = (res, CR.off(np.loadtxt(out), truth))
    with capsys.disabled():
        for refine, (res, (rot, tr)) in got.items():
            print(f"\nregister --refine {refine}: {res['iterations']} iterations, rotation off {rot:.3e}, translation off "
                  f"{tr * 1e3:.3f} mm, fitness {res['fitness']:.4f}, rmse {res['rmse']:.3e}, times {res['times']}")
    assert {"features", "normals", "gradient", "refine"} <= set(got["color"][0]["times"])
    assert "gradient" not in got["plane"][0]["times"]
    rot, tr = got["color"][1]
    assert rot <= ROT_BOUND and tr <= TR_BOUND


def test_register_refuses_a_fragment_without_colours(pair, capsys):
    from imfnet_amd.register import main
    d, _ = pair
    with pytest.raises(SystemExit):
        main(["--descriptor", "fpfh", "--source", str(d / "a.ply"), "--target", str(d / "plain.ply"), "--refine", "color"])
    assert "plain.ply has no red, green, blue" in capsys.readouterr().err


N = 4
WIDTH, STEP = 1.0 / 1.84, 0.28 / 1.84                 # the windows and poses of tests/test_gpu_reconstruct.py
POSES = (np.eye(4), rigid(9.0, [0.2, 1.0, -0.3], [0.31, -0.12, 0.22]), rigid(15.0, [-1.0, 0.3, 0.5], [-0.2, 0.4, 0.1]),
         rigid(12.0, [0.4, -0.2, 1.0], [0.25, 0.3, -0.3]))


def test_reconstruct_refine_color_returns_the_known_poses_and_keeps_the_pairs_of_plane(tmp_path):
    from imfnet_amd.dataio import read_ply_colors, read_ply_points
    from imfnet_amd.fuse_fragments import write_ply
    from imfnet_amd.pose_graph import rigid_inverse
    from imfnet_amd.reconstruct import reconstruct
    cloud = _fixture_cloud()
    rgb = paint(cloud)                                                  # painted on the scene: fragments agree on a point
    axis = int(np.argmax(cloud.max(0) - cloud.min(0)))
    rank = np.empty(len(cloud))
    rank[np.argsort(cloud[:, axis], kind="stable")] = (np.arange(len(cloud)) + 0.5) / len(cloud)
    frags, colors = [], []
    for k in range(N):
        inside = (rank >= k * STEP) & (rank < k * STEP + WIDTH)
        inv = rigid_inverse(POSES[k])
        path = str(tmp_path / f"cloud_bin_{k}.ply")
        write_ply(path, cloud[inside] @ inv[:3, :3].T + inv[:3, 3], rgb=rgb[inside])
        frags.append(np.array(read_ply_points(path), np.float64))
        colors.append(read_ply_colors(path))
    plane = reconstruct(frags, descriptor="fpfh", refine="plane")
    color = reconstruct(frags, descriptor="fpfh", refine="color", colors=colors)
    kept = lambda res: sorted((e["i"], e["j"]) for e in res["edges"] if e["kept"])
    lever = max(float(np.linalg.norm(f, axis=1).max()) for f in frags)
    rot_bound, tr_bound = (N - 1) * 1e-3, (N - 1) * (2e-3 + 1e-3 * lever)
    print(f"\nreconstruct on four painted windows: lever arm {lever:.3f} m, bounds {rot_bound:.1e} and {tr_bound:.3e} m; "
          f"kept with plane {kept(plane)}, with colour {kept(color)}; times with colour {color['times']}")
    worst = {}
    for name, res in (("plane", plane), ("color", color)):
        offs = [CR.off(res["poses"][k], POSES[k]) for k in range(N)]
        for k, (rot, tr) in enumerate(offs):
            print(f"  {name}, pose {k}: rotation off {rot:.3e}, translation off {tr * 1e3:.3f} mm")
        worst[name] = (max(o[0] for o in offs), max(o[1] for o in offs))
    assert color["unreached"] == [] and kept(color) == kept(plane)
    assert all((k, k + 1) in kept(color) for k in range(N - 1))
    assert {"features", "normals", "gradient", "register", "information", "optimize"} <= set(color["times"])
    assert worst["color"][0] <= rot_bound and worst["color"][1] <= tr_bound, worst
