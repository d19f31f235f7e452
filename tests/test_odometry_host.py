"""Host side of the RGB-D odometry: the NumPy restatement (tests/odometry_restate.py) against central differences, its
pyramid and occlusion rules on hand-made images, its accuracy on the synthetic sequence, how much the summation order moves
it, the C ABI's refusals and the plumbing of fuse_fragments / integrate_scene.  No GPU."""
import os
import pickle

import numpy as np
import pytest

import odometry_restate as OR
import plane_icp_restate as PR
import tsdf_color_scene as CS
import tsdf_scene as S
from imfnet_amd import odometry  # noqa: F401  (the feature: without it nothing here runs)

EINVAL = -1


# ---- (a) the Jacobian rows -----------------------------------------------------------------------------------------------
def _linearised(X, g, own, fx, fy, x):
    """v0 + g . (pi(X'(x)) - pi(X'(0))) - own z'(x), without the constants: the residual whose derivative the row is."""
    U = PR.update_from(x)
    Xp = U[:3, :3] @ X + U[:3, 3]
    return g[0] * (fx * Xp[0] / Xp[2]) + g[1] * (fy * Xp[1] / Xp[2]) - own * Xp[2]


def test_rows_agree_with_central_differences_and_the_mutations_do_not():
    """The row is the derivative of the linearised residual under the update [Rz Ry Rx | t], rotation first; the
    nearest-pixel cost itself is piecewise constant and cannot be differenced.  Gate 1e-6 relative to the row's largest entry
    at step 1e-6 over 200 draws: the truncation error of a central difference is h^2 / 6 times a third derivative (1e-12
    times the row's scale), its rounding error eps |r| / h (1e-10 times it).  A flipped sign or translation-first columns
    must miss by more than 1e-3 of the scale on every draw."""
    rng = np.random.default_rng(23)
    worst = 0.0
    for _ in range(200):
        X = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.5, 3.0)])
        g = rng.uniform(-1, 1, 2)
        fx, fy = rng.uniform(100, 600, 2)
        for own in (0.0, 1.0):
            J = OR.rows(g[:1], g[1:], fx, fy, X[:1], X[1:2], X[2:], own)[0]
            num = np.zeros(6)
            for k in range(6):
                e = np.zeros(6)
                e[k] = 1e-6
                num[k] = (_linearised(X, g, own, fx, fy, e) - _linearised(X, g, own, fx, fy, -e)) / 2e-6
            scale = np.abs(J).max()
            worst = max(worst, np.abs(J - num).max() / scale)
            assert np.abs(-J - num).max() > 1e-3 * scale
            assert np.abs(np.concatenate([J[3:], J[:3]]) - num).max() > 1e-3 * scale
    print(f"rows against central differences: off {worst:.2e} of the row's largest entry")
    assert worst <= 1e-6


# ---- (b) the pyramid ------------------------------------------------------------------------------------------------------
K8 = np.array([[8.0, 0, 3.5], [0, 8.0, 3.5], [0, 0, 1]])


def _grey(h=8, w=8, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def test_pyramid_depth_is_the_mean_of_the_valid_pixels():
    d = np.zeros((8, 8), np.uint16)
    d[0:2, 0:2] = [[1000, 0], [0, 0]]                        # one valid
    d[0:2, 2:4] = [[1000, 1004], [0, 0]]                     # two
    d[2:4, 0:2] = [[1000, 1004], [1010, 0]]                  # three
    d[2:4, 2:4] = [[1000, 1004], [1010, 1022]]               # four
    fr = OR.prepare(d, _grey(), K8, levels=2)
    D0, D1 = fr["levels"][0]["D"], fr["levels"][1]["D"]
    assert D1.shape == (4, 4) and np.isnan(D0[0, 1]) and D0[0, 0] == 1.0
    assert D1[0, 0] == 1.0
    assert D1[0, 1] == ((1.0 + 1.004) + (0.0 + 0.0)) / 2.0
    assert D1[1, 0] == ((1.0 + 1.004) + (1.01 + 0.0)) / 3.0
    assert D1[1, 1] == ((1.0 + 1.004) + (1.01 + 1.022)) / 4.0
    assert np.isnan(D1[2:, :]).all() and np.isnan(D1[:, 2:]).all()          # no valid pixel: NaN
    # the range: u16 = 0, d <= depth_min and d >= depth_max are invalid (strict on both sides)
    d2 = np.full((8, 8), 2000, np.uint16)
    d2[0, 0], d2[0, 1], d2[0, 2] = 500, 4000, 3999
    D = OR.prepare(d2, _grey(), K8, levels=1, depth_min=0.5, depth_max=4.0)["levels"][0]["D"]
    assert np.isnan(D[0, 0]) and np.isnan(D[0, 1]) and D[0, 2] == 3.999 and D[1, 1] == 2.0


def test_depth_edges_mask_the_gradient_and_the_border_is_nan():
    for step, finite in ((59, True), (61, False)):
        d = np.full((8, 8), 1000, np.uint16)
        d[:, 4:] = 1000 + step
        L = OR.prepare(d, _grey(), K8, levels=1, depth_edge=0.06)["levels"][0]
        for P in ("Isx", "Isy", "Dx", "Dy"):
            assert np.isnan(L[P][0]).all() and np.isnan(L[P][-1]).all() and np.isnan(L[P][:, 0]).all() \
                and np.isnan(L[P][:, -1]).all()
        assert np.isfinite(L["Isx"][1:-1, 1:-1]).all() and np.isfinite(L["Isy"][1:-1, 1:-1]).all()
        assert np.isfinite(L["Dx"][1:-1, 1:3]).all() and np.isfinite(L["Dx"][1:-1, 5:7]).all()     # away from the step
        assert np.isfinite(L["Dx"][1:-1, 3:5]).all() == finite and np.isnan(L["Dx"][1:-1, 3:5]).all() == (not finite)
        if finite:                                            # (c - a) + 2 (f - d) + (i - g) = 4 steps, over 8
            assert np.allclose(L["Dx"][1:-1, 3:5], step / 2000.0, rtol=0, atol=1e-15) and (L["Dy"][1:-1, 1:-1] == 0).all()
    hole = np.full((8, 8), 1000, np.uint16)
    hole[4, 4] = 0
    L = OR.prepare(hole, _grey(), K8, levels=1)["levels"][0]
    assert np.isnan(L["Dx"][3:6, 3:6]).all() and np.isfinite(L["Dx"][1:3, 1:3]).all()


def test_smoothing_sobel_and_the_intrinsics_rule():
    rgb = np.zeros((8, 8, 3), np.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = 255, 255, 255
    fr = OR.prepare(np.full((8, 8), 1000, np.uint16), rgb, K8, levels=2)
    assert (fr["levels"][0]["Is"] == 1.0).all() and (fr["levels"][1]["Is"] == 1.0).all()      # (r + g + b) / 765
    ramp = np.zeros((8, 8, 3), np.uint8)
    ramp[..., 0] = 3 * np.arange(8)[None, :]                 # I = u / 255: the Gaussian keeps a ramp, Sobel gives its slope
    L = OR.prepare(np.full((8, 8), 1000, np.uint16), ramp, K8, levels=1)["levels"][0]
    assert np.allclose(L["Is"][:, 1:-1], np.arange(1, 7)[None, :] / 255.0, rtol=0, atol=1e-16)
    assert np.allclose(L["Isx"][1:-1, 2:-2], 1.0 / 255.0, rtol=0, atol=1e-16) and np.abs(L["Isy"][1:-1, 1:-1]).max() < 1e-16
    assert L["Is"][0, 0] == ((0.0 + 0.0) + 1.0 / 255.0) / 4.0                                  # the border replicated
    seq_k = S.intrinsic(160, 120)
    fr = OR.prepare(np.full((120, 160), 1000, np.uint16), _grey(120, 160), seq_k, levels=3)
    for l, (w, h) in enumerate(((160, 120), (80, 60), (40, 30))):
        want = S.intrinsic(w, h)
        got = fr["levels"][l]
        assert fr["levels"][l]["D"].shape == (h, w)
        assert np.allclose([got["fx"], got["fy"], got["cx"], got["cy"]], [want[0, 0], want[1, 1], want[0, 2], want[1, 2]],
                           rtol=0, atol=1e-12)
    for bad in (dict(levels=0), dict(levels=6), dict(levels=4)):                                # 8 / 8 = 1 < 3
        with pytest.raises(ValueError):
            OR.prepare(np.zeros((8, 8), np.uint16), _grey(), K8, **bad)
    with pytest.raises(ValueError):
        OR.prepare(np.zeros((10, 12), np.uint16), _grey(10, 12), K8, levels=3)                  # 10 is not divisible by 4


# ---- (c) occlusion ----------------------------------------------------------------------------------------------------------
def _two_on_one(d_a, d_b):
    """Source pixels (4, 4) and (4, 5) of an 8 x 8 frame land on target pixel (4, 4) of a camera with half the focal length."""
    src_d = np.zeros((8, 8), np.uint16)
    src_d[4, 4], src_d[4, 5] = d_a, d_b
    src = OR.prepare(src_d, _grey(seed=2), K8, levels=1)
    Kt = np.array([[4.0, 0, 3.5], [0, 4.0, 3.5], [0, 0, 1]])
    dst = OR.prepare(np.full((8, 8), 1000, np.uint16), _grey(seed=3), Kt, levels=1)
    return OR.stage(src, dst, 0, np.eye(4), max_depth_diff=0.5)


def test_the_nearer_candidate_wins_and_a_tie_goes_to_the_lower_index():
    a, b = 4 * 8 + 4, 4 * 8 + 5
    for d_a, d_b, want in ((950, 900, b), (900, 950, a), (900, 900, a)):
        st = _two_on_one(d_a, d_b)
        assert st["sums"][0] == 1 and st["n_valid"] == 2
        assert st["winner"][4, 4] == want and (np.delete(st["winner"].ravel(), 4 * 8 + 4) == -1).all()
    assert _two_on_one(950, 900)["margins"]["z_gap"] == pytest.approx(0.05, abs=1e-12)
    assert _two_on_one(900, 900)["margins"]["z_gap"] == np.inf              # an exact tie is no near-tie


# ---- (d) against the ground truth -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(OR.MEASURED), ids=lambda a: f"arc{a}")
def sequence(request):
    seq = S.make_sequence(160, 120, n_frames=5, seed=0, holes=0.02, arc=request.param)
    seq["color"] = CS.make_colors(seq)
    seq["arc"] = request.param
    return seq


def test_restatement_against_the_ground_truth(sequence):
    """Rotation and translation error of every pair f -> f - 1 and of every pose of `track` (the last one is the drift).
    The gate is twice what the restatement itself gave where the constants of odometry_restate.MEASURED were recorded: the
    margin covers another BLAS or NumPy."""
    seq, m = sequence, OR.MEASURED[sequence["arc"]]
    frames = [OR.prepare(seq["depth"][f], seq["color"][f], seq["K"]) for f in range(5)]
    pair = np.zeros(2)
    for f in range(1, 5):
        T, info, res = OR.odometry(frames[f], frames[f - 1])
        e = OR.pose_error(T, OR.pair_truth(seq["poses"], f, f - 1))
        print(f"arc {seq['arc']}: pair {f} -> {f - 1}: {e[0]:.4f} deg, {1000 * e[1]:.3f} mm, n {res['n']}, fitness "
              f"{res['fitness']:.3f}")
        assert not res["lost"] and res["flags"] == 0 and res["n"] > 10000 and (info == info.T).all()
        pair = np.maximum(pair, e)
    poses, kept = OR.track(seq["depth"], seq["color"], seq["K"])
    assert kept.all() and (poses[0] == np.eye(4)).all()
    errs = np.array([OR.pose_error(poses[f], OR.pair_truth(seq["poses"], f, 0)) for f in range(5)])
    print(f"arc {seq['arc']}: worst pair {pair[0]!r} deg {pair[1]!r} m; track worst {errs[:, 0].max()!r} deg "
          f"{errs[:, 1].max()!r} m; drift at the last frame {errs[4, 0]:.4f} deg {1000 * errs[4, 1]:.3f} mm")
    assert pair[0] <= 2 * m["pair"][0] and pair[1] <= 2 * m["pair"][1]
    assert errs[:, 0].max() <= 2 * m["track"][0] and errs[:, 1].max() <= 2 * m["track"][1]


# ---- (e) the C ABI's refusals -----------------------------------------------------------------------------------------------
def test_the_c_abi_refuses_bad_arguments_without_a_device():
    """Every refusal below comes before any launch or copy, so it answers with host pointers and without a GPU."""
    from imfnet_amd import _lib
    L = _lib.lib()
    buf = np.zeros(1 << 12, dtype=np.float64)
    p = buf.ctypes.data
    p += (-p) % 256
    plane = lambda n: -(-n * 8 // 256) * 256                # six fp64 planes per level, each rounded up to 256 bytes
    assert L.imf_rgbd_frame_bytes(120, 160, 3) == 256 + 6 * (plane(120 * 160) + plane(60 * 80) + plane(30 * 40))
    for h, w, lv in ((120, 160, 0), (120, 160, 6), (10, 12, 3), (8, 8, 3), (2, 8, 1), (0, 0, 1), (-4, 8, 1)):
        assert L.imf_rgbd_frame_bytes(h, w, lv) == 0 and L.imf_rgbd_odometry_workspace_bytes(h, w, lv) == 0, (h, w, lv)
    assert L.imf_rgbd_frame_bytes(12, 20, 3) > 0 and L.imf_rgbd_odometry_workspace_bytes(12, 20, 3) > 0
    full = L.imf_rgbd_frame_bytes(8, 8, 2)

    def prepare(h=8, w=8, fx=8.0, scale=1000.0, dmin=0.0, dmax=4.0, edge=0.06, lv=2, nbytes=full, null=None, frame=p):
        a = {k: (None if k == null else p) for k in ("depth_u16", "color_u8")}
        return L.imf_rgbd_prepare(a["depth_u16"], a["color_u8"], h, w, fx, 8.0, 3.5, 3.5, scale, dmin, dmax, edge, lv,
                                  None if null == "frame" else frame, nbytes, None)

    for kw in (dict(lv=0), dict(lv=6), dict(lv=3), dict(h=10), dict(w=0), dict(fx=0.0), dict(fx=float("nan")),
               dict(scale=0.0), dict(dmax=0.0), dict(dmin=float("nan")), dict(edge=0.0), dict(edge=float("nan")),
               dict(nbytes=full - 1), dict(nbytes=0), dict(frame=p + 8)):
        assert prepare(**kw) == EINVAL, kw
    assert prepare(lv=6) == EINVAL and b"levels" in L.imf_last_error()
    for null in ("depth_u16", "color_u8", "frame"):
        assert prepare(null=null) == EINVAL and null.encode() in L.imf_last_error(), null

    import ctypes as C

    def odo(its=(20, 10, 5), mdd=0.03, lam=0.968, min_corr=30, ws=1 << 20, null=None, wsp=p):
        a = {k: (None if k == null else p) for k in ("src_frame", "dst_frame", "T", "info", "stats", "meta")}
        arr = None if null == "iterations" else (C.c_int * max(len(its), 1))(*its)
        return L.imf_rgbd_odometry(a["src_frame"], a["dst_frame"], None, arr, len(its), mdd, lam, min_corr, a["T"],
                                   a["info"], a["stats"], a["meta"], None if null == "workspace" else wsp, ws, None)

    for kw in (dict(its=()), dict(its=(1,) * 6), dict(its=(20, 0, 5)), dict(its=(20, 10, -1)), dict(mdd=0.0),
               dict(mdd=float("nan")), dict(min_corr=-1), dict(ws=0), dict(wsp=p + 8)):
        assert odo(**kw) == EINVAL, kw
    assert odo(its=(20, 0, 5)) == EINVAL and b"iterations[1]" in L.imf_last_error()
    for lam in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        assert odo(lam=lam) == EINVAL and b"lambda_depth" in L.imf_last_error(), lam
    for null in ("src_frame", "dst_frame", "iterations", "T", "info", "stats", "meta", "workspace"):
        assert odo(null=null) == EINVAL and b"null pointer" in L.imf_last_error(), null

    def stage(lam=0.968, mdd=0.03, null=None, ws=1 << 20):
        a = {k: (None if k == null else p) for k in ("src", "dst", "T", "winner", "sums", "workspace")}
        return L.imf_rgbd_odometry_stage(a["src"], a["dst"], 0, a["T"], mdd, lam, a["winner"], a["sums"], a["workspace"],
                                         ws, None)

    for kw in (dict(lam=1.5), dict(lam=float("nan")), dict(mdd=-1.0), dict(ws=0)):
        assert stage(**kw) == EINVAL, kw
    for null in ("src", "dst", "T", "winner", "sums", "workspace"):
        assert stage(null=null) == EINVAL, null


def test_the_wrappers_refuse_before_the_library_is_called():
    from imfnet_amd._lib import ImfError
    from imfnet_amd.odometry import prepare_frame, rgbd_odometry
    with pytest.raises(ImfError):
        prepare_frame(np.zeros((8, 8), np.uint16), np.zeros((8, 9, 3), np.uint8), K8, device="cpu")
    with pytest.raises(ImfError):
        prepare_frame(np.zeros((8, 8), np.float32), np.zeros((8, 8, 3), np.uint8), K8, device="cpu")
    with pytest.raises(ImfError):
        rgbd_odometry(None, None)


# ---- (f) fuse_fragments and integrate_scene ---------------------------------------------------------------------------------
def _tiny_tree(tmp_path):
    seq = S.make_sequence(32, 24, n_frames=3)
    return seq, S.write_tree(str(tmp_path / "raw"), seq)


def test_fuse_fragments_arguments_and_the_unchanged_default(tmp_path):
    from imfnet_amd import fuse_fragments as FF
    base = ["--dataset_root", str(tmp_path / "raw"), "--out_root", str(tmp_path / "out"), "--height", "24", "--width", "32"]
    cfg = FF.parse_args(base)
    assert cfg.poses == "file" and cfg.odometry_levels == 3 and cfg.odometry_max_depth_diff == 0.03 \
        and cfg.odometry_depth_max == 4.0
    assert FF.parse_args(base + ["--poses", "odometry"]).poses == "odometry"
    with pytest.raises(SystemExit):
        FF.parse_args(base + ["--poses", "guess"])
    seq, _ = _tiny_tree(tmp_path)
    seen = []

    def fake_fuse(cfg, intrinsic, frag):
        seen.append(frag)
        return np.zeros((4, 3))

    def no_track(*a):
        raise AssertionError("--poses file must not track")

    assert FF.run(cfg, fuse=fake_fuse, log=lambda *a: None, track=no_track) == 1
    folder = tmp_path / "out" / "scene-a" / "seq-01"
    with open(folder / "cloud_bin_0.frames.pkl", "rb") as fh:
        record = pickle.load(fh)
    assert sorted(record) == ["frames"] and len(record["frames"]) == 3
    assert np.array_equal(np.load(folder / "cloud_bin_0.pose.npy"), seq["poses"][0].astype(np.float32))
    assert "color" not in seen[0] and seen[0]["poses"].shape == (3, 4, 4)


def test_fuse_fragments_with_odometry_reads_no_pose_file(tmp_path):
    """A fake `track` drops the middle frame: it is left out as a NaN pose is, the record gains "poses" for the kept frames,
    the base is the float32 identity, and integrate_scene's scene_poses uses the record without a .pose.txt in the tree."""
    from imfnet_amd import fuse_fragments as FF
    from imfnet_amd.integrate_scene import scene_poses
    seq, sdir = _tiny_tree(tmp_path)
    for f in os.listdir(sdir):
        if f.endswith(".pose.txt"):
            os.remove(os.path.join(sdir, f))
    cfg = FF.parse_args(["--dataset_root", str(tmp_path / "raw"), "--out_root", str(tmp_path / "out"), "--height", "24",
                         "--width", "32", "--poses", "odometry"])
    rel = np.stack([np.eye(4), np.full((4, 4), np.nan), OR.pair_truth(seq["poses"], 2, 0)])
    seen = []

    def fake_track(cfg, intrinsic, frag):
        assert frag["depth"].shape == (3, 24, 32) and frag["color"].shape == (3, 24, 32, 3) and intrinsic.shape == (3, 3)
        return rel, np.array([True, False, True])

    def fake_fuse(cfg, intrinsic, frag):
        seen.append(frag)
        return np.zeros((4, 3))

    assert FF.run(cfg, fuse=fake_fuse, log=lambda *a: None, track=fake_track) == 1
    assert seen[0]["depth"].shape == (2, 24, 32) and np.array_equal(seen[0]["poses"], rel[[0, 2]])
    folder = str(tmp_path / "out" / "scene-a" / "seq-01")
    with open(os.path.join(folder, "cloud_bin_0.frames.pkl"), "rb") as fh:
        record = pickle.load(fh)
    assert [os.path.basename(s) for s in record["frames"]] == ["frame-000000", "frame-000002"]
    assert record["poses"].dtype == np.float64 and np.array_equal(record["poses"], rel[[0, 2]])
    base = np.load(os.path.join(folder, "cloud_bin_0.pose.npy"))
    assert base.dtype == np.float32 and np.array_equal(base, np.eye(4, dtype=np.float32))
    X = PR.update_from(np.array([0.1, -0.2, 0.3, 1.0, 2.0, 3.0]))
    got = scene_poses(folder, sdir, 0, X)
    assert [os.path.basename(s) for s, _ in got] == ["frame-000000", "frame-000002"]
    assert np.array_equal(got[0][1], X) and np.allclose(got[1][1], X @ rel[2], rtol=0, atol=1e-15)


# ---- (g) the order of the sums ------------------------------------------------------------------------------------------------
def test_the_order_of_the_sums_moves_the_result_by_rounding_only():
    """The loop on pair 1 -> 0 at arc 0.12 with NumPy's sums and with the same sums in reversed pixel order: every stage
    keeps its winner map, and T moves by delta (recorded in DESIGN.md 22; the GPU test grants the kernel 100 delta)."""
    fwd, rev, delta, delta_info = OR.order_sensitivity()
    assert len(fwd[2]["winners"]) == 36 and fwd[2]["n"] == rev[2]["n"]
    assert all(np.array_equal(a, b) for a, b in zip(fwd[2]["winners"], rev[2]["winners"]))
    print(f"delta = {delta!r} on T, {delta_info!r} of the largest entry on info")
    assert 0 < delta < 1e-12 and delta_info < 1e-11
