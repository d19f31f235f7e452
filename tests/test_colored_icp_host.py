"""Host side of coloured ICP: the NumPy restatement (tests/colored_icp_restate.py) against central differences, its exact
cases, the textured plane that justifies the feature, lambda = 1 against the point-to-plane restatement, the C ABI's
refusals and the plumbing of `register` / `reconstruct`.  No GPU."""
import os
import re

import numpy as np
import pytest

import colored_icp_restate as CR
import plane_icp_restate as PR
from imfnet_amd.matching import color_gradient, icp_colored, intensity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("imf_color_gradient", "imf_icp_colored_workspace_bytes", "imf_icp_colored")


# ---- the Jacobians -----------------------------------------------------------------------------------------------------
def _central_differences(p, Is, q, n, Iq, g, h=1e-6):
    """d r_G / dx and d r_I / dx [6] at x = 0 of the residuals of update_from(x) . p."""
    out = np.zeros((2, 6))
    for k in range(6):
        r = []
        for s in (h, -h):
            x = np.zeros(6)
            x[k] = s
            U = PR.update_from(x)
            r.append(CR.residuals((p @ U[:3, :3].T + U[:3, 3])[None], Is, q[None], n[None], Iq, g[None]))
        out[0, k] = (r[0][0][0] - r[1][0][0]) / (2 * h)
        out[1, k] = (r[0][1][0] - r[1][1][0]) / (2 * h)
    return out


def test_jacobians_agree_with_central_differences_and_the_mutations_do_not():
    """J_G = [p x n, n] and J_I = [p x M, M], M = -g + (n . g) n, are the derivatives of r_G and r_I under the update
    [Rz Ry Rx | t], rotation first.  Gate 1e-8 absolute at step 1e-6 over 200 draws: the truncation error of a central
    difference is h^2 / 6 times a third derivative of order |p| |g| (1e-12 here) and its rounding error is eps |r| / h
    (1e-10).  A flipped sign of M, or translation-first columns, must miss the gate on every draw."""
    rng = np.random.default_rng(17)
    worst = np.zeros(2)
    for _ in range(200):
        p, q = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        g = rng.uniform(-1, 1, 3)                                       # not tangent on purpose: M projects it
        Is, Iq = rng.uniform(0, 1, 2)
        num = _central_differences(p, Is, q, n, Iq, g)
        JG, JI = CR.jacobians(p[None], q[None], n[None], g[None])
        err = np.array([np.abs(JG[0] - num[0]).max(), np.abs(JI[0] - num[1]).max()])
        worst = np.maximum(worst, err)
        assert np.abs(-JI[0] - num[1]).max() > 1e-3                      # the sign of M
        swapped = np.concatenate([JI[0, 3:], JI[0, :3]])                # translation first
        assert np.abs(swapped - num[1]).max() > 1e-3
        assert np.abs(np.concatenate([JG[0, 3:], JG[0, :3]]) - num[0]).max() > 1e-3
    print(f"Jacobians against central differences: J_G off {worst[0]:.2e}, J_I off {worst[1]:.2e}")
    assert worst[0] <= 1e-8 and worst[1] <= 1e-8


# ---- the gradient ------------------------------------------------------------------------------------------------------
ORDERS = ("forward", "reversed", "butterfly")


@pytest.mark.parametrize("case", CR.exact_cases(), ids=[c["name"] for c in CR.exact_cases()])
def test_exact_cases_of_the_gradient(case):
    args = (case["points"], case["normals"], case["inten"], case["nbr"], case["counts"])
    _, moved, bound = CR.gradient_tolerance(*args)
    for order in ORDERS:
        g = CR.gradient_restated(*args, order)
        if case["to_bound"]:
            err = np.abs(g - case["want"]).max(1)
            print(f"{case['name']} ({order}): off {err.max():.2e}, the bound's smallest {bound.min():.2e}")
            assert (err <= bound).all()
        else:
            assert (g == case["want"]).all()
    by = {c["name"]: c for c in CR.exact_cases()}
    assert (by["m3"]["counts"] == 3).all() and (by["m4_collinear"]["counts"] == 4).all()
    assert (by["linear_on_a_jittered_plane"]["counts"] >= 4).all()


@pytest.mark.parametrize("name", ["plane", "bumpy"])
def test_gradient_lies_in_the_tangent_plane_and_the_butterfly_order_is_within_the_bound(name):
    """g . n = 0 to rounding on every row, and the kernel's summation order (restated here bit for bit) stays within what
    the kernel is granted: the CPU's forecast of the GPU test."""
    c = CR.textured_plane() if name == "plane" else CR.painted_bumpy()
    args = (c["dst"], c["normals"], c["dst_I"], c["nbr"], c["counts"])
    fwd, moved, bound = CR.gradient_tolerance(*args)
    assert np.array_equal(fwd, c["grad"]) and (np.abs(fwd).max(1) > 0).all()
    along = np.abs((fwd * c["normals"]).sum(1))
    err = np.abs(CR.gradient_restated(*args, "butterfly") - fwd).max(1)
    print(f"{name}: |g . n| <= {along.max():.2e}, order moved <= {moved.max():.2e}, butterfly off <= {err.max():.2e}, "
          f"worst share of its bound {(err / bound).max():.2e}")
    assert (along <= bound).all() and (err <= bound).all()
    # the painted gradient is the texture's: d/dx and d/dy of `texture` at the point, projected into the tangent plane
    x, y = c["dst"][:, 0], c["dst"][:, 1]
    want = np.stack([0.6 * np.cos(3 * x + 0.5) + 0.2 * np.cos(2 * x - 3 * y),
                     -0.5 * np.sin(2.5 * y) - 0.3 * np.cos(2 * x - 3 * y), np.zeros_like(x)], 1)
    want -= (want * c["normals"]).sum(1)[:, None] * c["normals"]
    # a linear fit over offsets of at most 0.2 m is off by at most |H| 0.2 / 2; the texture's second derivatives are at
    # most 2.2 (xx), 2.15 (yy) and 0.6 (xy), so |H| <= 2.8.  Gradients reach 0.8: a flipped or transposed one misses by more
    print(f"{name}: gradient off the texture's by <= {np.abs(fwd - want).max():.3f}")
    assert np.abs(fwd - want).max() <= 0.5 * 2.8 * 0.2 and np.abs(want).max() > 0.7


# ---- the joint fit -----------------------------------------------------------------------------------------------------
def _both(c, lam=None, max_iteration=30):
    plane = PR.icp_plane_restated(c["src"], c["dst"], c["normals"], c["r"], None, max_iteration)
    color = CR.icp_colored_restated(c["src"], c["src_I"], c["dst"], c["normals"], c["dst_I"], c["grad"], c["r"],
                                    c["lam"] if lam is None else lam, None, max_iteration)
    return plane, color


def test_textured_plane_point_to_plane_stays_and_colour_finds_the_motion():
    c = CR.textured_plane()
    assert len(c["dst"]) == 1681 and len(c["src"]) == 729 and (c["dst"][:, 2] == 0).all()
    plane, color = _both(c)
    start, end = CR.off(np.eye(4), c["truth"]), CR.off(color[0], c["truth"])
    print(f"textured plane: start off {start[0]:.2e} / {start[1] * 1e3:.2f} mm; point-to-plane ends at iteration {plane[3]} "
          f"on the start; colour ends after {color[3]} iterations {end[0]:.2e} / {end[1] * 1e3:.3f} mm off "
          f"({start[0] / end[0]:.0f}x, {start[1] / end[1]:.0f}x)")
    assert np.array_equal(plane[0], np.eye(4)) and plane[3] <= 1          # singular at stage 0: the start pose
    assert abs(start[0] - 2.9e-2) < 1e-3 and abs(start[1] - 0.0374) < 1e-4
    assert 10.0 * end[0] <= start[0] and 10.0 * end[1] <= start[1]
    assert color[4] == len(c["src"]) and color[1] == 1.0


def test_painted_bumpy_surface_colour_ends_no_further_than_point_to_plane():
    c = CR.painted_bumpy()
    plane, color = _both(c)
    p, k = CR.off(plane[0], c["truth"]), CR.off(color[0], c["truth"])
    print(f"painted bumpy surface: point-to-plane ends {p[0]:.2e} / {p[1] * 1e3:.3f} mm off after {plane[3]} iterations, "
          f"colour {k[0]:.2e} / {k[1] * 1e3:.3f} mm after {color[3]}")
    assert k[0] <= 2.0 * p[0] + 1e-4 and k[1] <= 2.0 * p[1] + 1e-4


@pytest.mark.parametrize("name", ["plane", "bumpy"])
def test_lambda_one_is_point_to_plane_as_numbers(name):
    c = CR.textured_plane() if name == "plane" else CR.painted_bumpy()
    for it in (1, 30):
        plane, color = _both(c, lam=1.0, max_iteration=it)
        assert np.array_equal(plane[0], color[0]) and tuple(plane[1:]) == tuple(color[1:])
    if name == "bumpy":
        assert not np.array_equal(plane[0], np.eye(4)) and plane[3] >= 2


def test_the_restatement_moves_little_with_the_order_of_the_source():
    c = CR.painted_bumpy()
    fwd, rev, moved, tol = CR.tolerances(c["src"], c["src_I"], c["dst"], c["normals"], c["dst_I"], c["grad"], c["r"], c["lam"],
                                         None, 30)
    print(f"source order moved T, fitness, rmse by {moved}")
    assert fwd[3] == rev[3] and fwd[4] == rev[4] and moved[0] < 1e-12 and all(t >= 1e-12 for t in tol)


# ---- the library and the plumbing --------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbols():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    assert "TransformationEstimationForColoredICP" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name


def test_argument_errors_return_a_status_without_a_gpu():
    from imfnet_amd import _lib
    CR.check_refusals(_lib.lib())


def test_intensity_is_the_sum_over_765():
    rgb = np.array([[0, 0, 0], [255, 255, 255], [1, 2, 3], [255, 0, 0], [200, 100, 50]], np.uint8)
    got = intensity(rgb)
    assert got.dtype == np.float64 and got.tolist() == [0.0, 1.0, 6 / 765, 255 / 765, 350 / 765]
    assert np.array_equal(got, CR.intensity(rgb))
    from imfnet_amd._lib import ImfError
    for bad in (rgb.astype(np.float64), rgb[:, :2], rgb[0]):
        with pytest.raises(ImfError):
            intensity(bad)


def test_python_wrappers_refuse_bad_shapes_before_any_device_work():
    from imfnet_amd._lib import ImfError
    z3, z = np.zeros((4, 3)), np.zeros(4)
    nbr, cnt = np.zeros((4, 30), np.int32), np.zeros(4, np.int32)
    for bad in (dict(normals=np.zeros((5, 3))), dict(intensity=np.zeros(5)), dict(neighbors=np.zeros((4, 65), np.int32)),
                dict(neighbors=np.zeros((5, 30), np.int32)), dict(counts=np.zeros(3, np.int32))):
        with pytest.raises(ImfError):
            color_gradient(**dict(dict(points=z3, normals=z3, intensity=z, neighbors=nbr, counts=cnt, device="cpu"), **bad))
    for bad in (dict(dst_normals=None), dict(dst_normals=np.zeros((5, 3))), dict(src_intensity=np.zeros(5)),
                dict(dst_intensity=np.zeros(3)), dict(dst_gradient=np.zeros((5, 3)))):
        with pytest.raises(ImfError):
            icp_colored(**dict(dict(src=z3, src_intensity=z, dst=z3, dst_normals=z3, dst_intensity=z, max_corr_dist=0.1,
                                    dst_gradient=z3, device="cpu"), **bad))


def test_refine_color_is_a_choice_of_both_commands_and_needs_colours():
    from imfnet_amd import reconstruct, register
    assert register.REFINE_CHOICES == ("none", "point", "plane", "color")
    assert register.make_parser().parse_args(["--source", "a.ply", "--target", "b.ply", "--refine", "color"]).refine == "color"
    assert reconstruct.make_parser().parse_args(["--fragments", "d", "--out", "o", "--refine", "color"]).refine == "color"
    pts, rgb = np.zeros((4, 3)), np.zeros((4, 3), np.uint8)
    with pytest.raises(ValueError, match="the source has no colours"):
        register.register_features(pts, pts, None, None, refine="color", device="cpu")
    with pytest.raises(ValueError, match="the target has no colours"):
        register.register_features(pts, pts, None, None, refine="color", device="cpu", source_colors=rgb)
    with pytest.raises(ValueError, match="uint8"):
        register.register_pair(None, None, pts, None, pts, None, refine="color", descriptor="fpfh", device="cpu",
                               source_colors=rgb.astype(np.float32), target_colors=rgb)
    with pytest.raises(ValueError, match="fragment 1 has no colours"):
        reconstruct.reconstruct([pts, pts], refine="color", device="cpu", colors=[rgb, None])


def test_commands_refuse_a_fragment_without_colours_and_name_the_file(tmp_path, capsys):
    from imfnet_amd import reconstruct, register
    from imfnet_amd.fuse_fragments import write_ply
    pts = np.random.default_rng(0).uniform(0, 1, (20, 3))
    rgb = np.random.default_rng(1).integers(0, 256, (20, 3)).astype(np.uint8)
    os.makedirs(tmp_path / "frags")
    write_ply(str(tmp_path / "frags" / "cloud_bin_0.ply"), pts, rgb=rgb)
    write_ply(str(tmp_path / "frags" / "cloud_bin_1.ply"), pts)
    with pytest.raises(SystemExit):
        register.main(["--descriptor", "fpfh", "--source", str(tmp_path / "frags" / "cloud_bin_0.ply"), "--target",
                       str(tmp_path / "frags" / "cloud_bin_1.ply"), "--refine", "color", "--device", "cpu"])
    assert "cloud_bin_1.ply has no red, green, blue" in capsys.readouterr().err
    with pytest.raises(SystemExit, match="cloud_bin_1.ply has no red, green, blue"):
        reconstruct.main(["--fragments", str(tmp_path / "frags"), "--refine", "color", "--out", str(tmp_path / "out"),
                          "--device", "cpu"])


def test_a_written_coloured_ply_round_trips_into_the_intensities(tmp_path):
    from imfnet_amd.dataio import read_ply_colors, read_ply_points
    from imfnet_amd.fuse_fragments import write_ply
    c = CR.textured_plane()
    level = np.rint(254.0 * CR.texture(c["dst"])).astype(np.uint8)      # at most 254: one level of room
    rgb = np.stack([level, level, level], 1)
    rgb[::3, 0] += 1                                                    # the three channels differ on some rows
    path = str(tmp_path / "plane.ply")
    write_ply(path, c["dst"], rgb=rgb)
    back = read_ply_colors(path)
    assert back.dtype == np.uint8 and np.array_equal(back, rgb) and len(read_ply_points(path)) == len(rgb)
    got = intensity(back)
    assert np.array_equal(got, rgb.astype(np.int64).sum(1) / 765.0) and 0.0 <= got.min() and got.max() <= 1.0
    assert np.abs(got - CR.texture(c["dst"])).max() <= 2.0 / 255          # half a level, the 254 / 255 scale, the added 1 / 765
