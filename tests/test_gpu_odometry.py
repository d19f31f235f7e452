"""RGB-D odometry on the GPU (csrc/odometry.hip through imfnet_amd/odometry.py) against the NumPy restatement
(tests/odometry_restate.py) on the synthetic sequence of tests/tsdf_scene.py with the colours of tests/tsdf_color_scene.py,
on small and awkward frames, and from the command line of fuse_fragments to integrate_scene."""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import odometry_restate as OR   # noqa: E402
import tsdf_color_scene as CS   # noqa: E402
import tsdf_scene as S          # noqa: E402

pytestmark = pytest.mark.gpu

IMAGES = ("Is", "D", "Isx", "Isy", "Dx", "Dy")
# the stage cases take their depth edges at 60.1 mm: the depths are whole millimetres (and their means at the coarser levels
# multiples of 1/2, 1/3, 1/4 mm, ...), so at the default 60 mm thousands of neighbourhood differences sit within one rounding
# of the threshold (margin 5.6e-17) whatever the seed; at 60.1 mm the nearest is 0.1 mm away at level 0 and 4.2e-6 m over
# all levels (`edge_margin` of odometry_restate.prepare, asserted in the stage test).  This departs from the default on
# purpose; `prepare` at the default 60 mm is compared exactly below and the loop and `track` run there.
STAGE_EDGE = 0.0601


@pytest.fixture(scope="module")
def seqs():
    return {arc: OR.sequence(arc) for arc in (0.12, 0.3, 0.5)}


@pytest.fixture(scope="module")
def delta():
    """(delta, delta_info) of host test (g), taken again where the kernels run."""
    _, _, d, d_info = OR.order_sensitivity()
    print(f"delta = {d!r}, on info {d_info!r}")
    assert 0 < d < 1e-12
    return d, d_info


def _both(depth, color, K, **kw):
    from imfnet_amd.odometry import prepare_frame
    return prepare_frame(depth, color, K, **kw), OR.prepare(depth, color, K, **kw)


def _same_images(frame, restated):
    for l, want in enumerate(restated["levels"]):
        got = frame.images(l)
        for name in IMAGES:
            assert got[name].shape == want[name].shape, (l, name)
            assert np.array_equal(np.isnan(got[name]), np.isnan(want[name])), (l, name)
            ok = ~np.isnan(want[name])
            assert np.array_equal(got[name][ok], want[name][ok]), (l, name, np.abs(got[name][ok] - want[name][ok]).max())
        for k in ("fx", "fy", "cx", "cy"):
            assert got[k] == want[k], (l, k)


def _same_stage(frames, restated, level, T, **kw):
    """The winner map and n equal, every sum within n 2^-52 sum |addend| (one fp64 sum of n terms in any order)."""
    from imfnet_amd.odometry import odometry_stage
    want = OR.stage(restated[0], restated[1], level, T, **{dict(max_depth_diff="max_depth_diff", lambda_depth="lam")[k]: v
                                                           for k, v in kw.items()})
    winner, sums = odometry_stage(frames[0], frames[1], level, T, **kw)
    assert winner.dtype == np.int32 and np.array_equal(winner, want["winner"])
    n = int(want["sums"][0])
    assert sums[0] == n == int((winner >= 0).sum())
    bound = n * 2.0 ** -52 * want["abs_sums"]
    err = np.abs(sums - want["sums"])
    print(f"level {level}: n {n}, worst share of the bound {(err[1:] / np.maximum(bound[1:], 1e-300)).max():.3f}")
    assert (err <= bound).all(), (err, bound)
    return want, winner, sums


# ---- prepare ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 1])
def test_prepare_equals_the_restatement_in_every_bit(seqs, f):
    seq = seqs[0.12]
    _same_images(*_both(seq["depth"][f], seq["color"][f], seq["K"]))


@pytest.mark.parametrize("h,w,levels", [(8, 8, 2), (12, 20, 3), (24, 40, 1), (48, 80, 5)])
def test_prepare_on_small_shapes(h, w, levels):
    rng = np.random.default_rng(h * w)
    depth = rng.integers(400, 4400, (h, w)).astype(np.uint16)           # beyond depth_max too
    depth[rng.random((h, w)) < 0.2] = 0
    depth[:, w // 2:] //= 2                                              # a step
    color = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    K = S.intrinsic(w, h)
    frame, restated = _both(depth, color, K, levels=levels, depth_edge=0.3, depth_min=0.25)
    _same_images(frame, restated)
    assert restated["levels"][-1]["D"].shape == (h >> (levels - 1), w >> (levels - 1))


# ---- one stage ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stage_pair(seqs):
    seq = seqs[0.12]
    a = _both(seq["depth"][1], seq["color"][1], seq["K"], depth_edge=STAGE_EDGE)
    b = _both(seq["depth"][0], seq["color"][0], seq["K"], depth_edge=STAGE_EDGE)
    return (a[0], b[0]), (a[1], b[1]), OR.pair_truth(seq["poses"], 1, 0)


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("at", ["identity", "truth"])
def test_stage_equals_the_restatement(stage_pair, level, at):
    frames, restated, truth = stage_pair
    T = np.eye(4) if at == "identity" else truth
    margins = OR.stage(restated[0], restated[1], level, T)["margins"]
    edge = min(restated[0]["edge_margin"], restated[1]["edge_margin"])
    print(f"margins: {margins}, depth edge {edge:.3e}")
    assert margins["pixel"] > 1e-9 and margins["depth_diff"] > 1e-9 and edge > 1e-9 and margins["z_gap"] >= 1e-12
    want, _, _ = _same_stage(frames, restated, level, T)
    assert want["sums"][0] > (10000 if level == 0 else 500)


def test_prepared_stage_frames_equal_the_restatement(stage_pair):
    frames, restated, _ = stage_pair
    for f, r in zip(frames, restated):
        _same_images(f, r)


# ---- awkward frames ---------------------------------------------------------------------------------------------------------
def _flat(h, w, mm=1000, seed=0):
    return np.full((h, w), mm, np.uint16), np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


@pytest.mark.parametrize("h,w,levels", [(8, 8, 2), (12, 20, 3)])
def test_stage_and_loop_on_small_frames(h, w, levels):
    from imfnet_amd.odometry import rgbd_odometry
    rng = np.random.default_rng(7)
    K = S.intrinsic(w, h)
    pairs = []
    for seed in (1, 2):
        depth = (1000 + 40 * np.sin(np.arange(w) / 3.0)[None, :] + 5 * rng.random((h, w))).astype(np.uint16)
        depth[rng.random((h, w)) < 0.05] = 0
        pairs.append(_both(depth, _flat(h, w, seed=seed)[1], K, levels=levels))
    frames, restated = [p[0] for p in pairs], [p[1] for p in pairs]
    for level in range(levels):
        _same_stage(frames, restated, level, np.eye(4))
    its = (3,) * levels
    T, info, res = rgbd_odometry(frames[0], frames[1], iterations=its, min_corr=6)
    Tr, info_r, res_r = OR.odometry(restated[0], restated[1], iterations=its, min_corr=6)
    assert res["stages"] == 3 * levels + 1 and res["n_valid"] == res_r["n_valid"]
    assert np.isfinite(T).all() and np.isfinite(info).all() and (info == info.T).all()
    assert res["flags"] == res_r["flags"] and res["lost"] == res_r["lost"]


def test_no_valid_depth_gives_the_identity_and_the_flags():
    from imfnet_amd.odometry import rgbd_odometry
    K = S.intrinsic(8, 8)
    d, c = _flat(8, 8)
    empty, empty_r = _both(np.zeros((8, 8), np.uint16), c, K, levels=2)
    full, full_r = _both(d, c, K, levels=2)
    for pair, pair_r in (((empty, full), (empty_r, full_r)), ((full, empty), (full_r, empty_r))):
        want, winner, sums = _same_stage(pair, pair_r, 0, np.eye(4))
        assert sums[0] == 0 and (winner == -1).all() and (sums == 0).all()
        T, info, res = rgbd_odometry(*pair, iterations=(2, 2))
        assert np.array_equal(T, np.eye(4)) and (info == 0).all()
        assert res["n"] == 0 and res["flags"] == 3 and res["lost"] and res["fitness"] == 0.0 and res["cost"] == 0.0
        assert res["n_valid"] == (0 if pair[0] is empty else 64) and res["stages"] == 5


def test_a_source_that_projects_outside_and_a_target_with_one_valid_pixel():
    K = S.intrinsic(16, 16)
    d, c = _flat(16, 16, seed=3)
    full, full_r = _both(d, c, K, levels=1)
    away = np.eye(4)
    away[0, 3] = 50.0
    _, winner, sums = _same_stage((full, full), (full_r, full_r), 0, away)
    assert sums[0] == 0 and (winner == -1).all()
    behind = np.eye(4)
    behind[2, 3] = -5.0                                                  # z' < 0
    _, winner, sums = _same_stage((full, full), (full_r, full_r), 0, behind, max_depth_diff=100.0)
    assert sums[0] == 0
    one = np.zeros((16, 16), np.uint16)
    one[7, 9] = 1000
    single, single_r = _both(one, c, K, levels=1)
    _, winner, sums = _same_stage((full, single), (full_r, single_r), 0, np.eye(4))
    assert sums[0] == 0                                                  # a lone depth has no gradient
    block = np.zeros((16, 16), np.uint16)
    block[6:9, 8:11] = 1000                                              # nine valid: exactly one pixel has a gradient
    nine, nine_r = _both(block, c, K, levels=1)
    _, winner, sums = _same_stage((full, nine), (full_r, nine_r), 0, np.eye(4))
    assert sums[0] == 1 and winner[7, 9] == 7 * 16 + 9


def test_many_source_pixels_on_one_target_pixel():
    """A 16 x 16 block of the source collapses onto one pixel of a target camera with a sixteenth of the focal length: the
    winner is the exact minimum of z', the lowest index among equal ones."""
    rng = np.random.default_rng(11)
    Ks = np.array([[32.0, 0, 15.5], [0, 32.0, 15.5], [0, 0, 1]])
    Kt = np.array([[2.0, 0, 15.0], [0, 2.0, 15.0], [0, 0, 1]])
    depth = np.zeros((32, 32), np.uint16)
    depth[8:24, 8:24] = rng.integers(1000, 1040, (16, 16))               # 256 draws of 40 values: the minimum is tied
    c = _flat(32, 32, seed=5)[1]
    src, src_r = _both(depth, c, Ks, levels=1)
    dst, dst_r = _both(_flat(32, 32, 1100)[0], c, Kt, levels=1)
    want, winner, sums = _same_stage((src, dst), (src_r, dst_r), 0, np.eye(4), max_depth_diff=0.5)
    flat = depth.ravel().astype(np.int64)
    best = int(np.flatnonzero(flat == flat[flat > 0].min())[0])
    assert (flat == flat[best]).sum() > 1                                # the tie is there
    assert sums[0] == 1 and winner[15, 15] == best and (np.delete(winner.ravel(), 15 * 32 + 15) == -1).all()


def test_frames_of_another_shape_and_a_short_workspace_are_refused():
    import torch
    from imfnet_amd import _lib
    from imfnet_amd.odometry import _stream, prepare_frame
    L = _lib.lib()
    a = prepare_frame(*_flat(8, 8), S.intrinsic(8, 8), levels=2)
    b = prepare_frame(*_flat(12, 20), S.intrinsic(20, 12), levels=2)
    out = torch.zeros(64, dtype=torch.float64, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    its = (C.c_int * 2)(2, 2)
    call = lambda s, d, n, nbytes: L.imf_rgbd_odometry(s, d, None, its, n, 0.03, 0.968, 30, out.data_ptr(), out.data_ptr() + 128,
                                                       out.data_ptr() + 416, out.data_ptr() + 432, ws.data_ptr(), nbytes,
                                                       _stream())
    assert call(a.block.data_ptr(), b.block.data_ptr(), 2, 1 << 20) == -1 and b"different shapes" in L.imf_last_error()
    assert call(a.block.data_ptr(), out.data_ptr(), 2, 1 << 20) == -1 and b"not a frame block" in L.imf_last_error()
    need = L.imf_rgbd_odometry_workspace_bytes(8, 8, 2)
    assert call(a.block.data_ptr(), a.block.data_ptr(), 2, need - 1) == -1 and b"workspace" in L.imf_last_error()
    its3 = (C.c_int * 3)(2, 2, 2)
    assert L.imf_rgbd_odometry(a.block.data_ptr(), a.block.data_ptr(), None, its3, 3, 0.03, 0.968, 30, out.data_ptr(),
                               out.data_ptr() + 128, out.data_ptr() + 416, out.data_ptr() + 432, ws.data_ptr(), 1 << 20,
                               _stream()) == -1 and b"iteration counts" in L.imf_last_error()
    assert call(a.block.data_ptr(), a.block.data_ptr(), 2, need) == 0
    torch.cuda.synchronize()


# ---- the loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arc", [0.12, 0.5])
def test_loop_against_the_restatement(seqs, delta, arc):
    """n equal; |T - T_restated| <= 100 delta elementwise and info within 100 delta of its largest entry, delta from host
    test (g): the factor covers an order that differs at every stage instead of at one.  Two calls give the same bits."""
    import torch
    from imfnet_amd.odometry import rgbd_odometry, rgbd_odometry_device
    seq = seqs[arc]
    (src, src_r), (dst, dst_r) = (_both(seq["depth"][f], seq["color"][f], seq["K"]) for f in (1, 0))
    T, info, res = rgbd_odometry(src, dst)
    Tr, info_r, res_r = OR.odometry(src_r, dst_r)
    off_T = float(np.abs(T - Tr).max())
    off_info = float(np.abs(info - info_r).max() / np.abs(info_r).max())
    e = OR.pose_error(T, OR.pair_truth(seq["poses"], 1, 0))
    print(f"arc {arc}: n {res['n']}, |T - restated| {off_T:.3e} (delta {delta[0]:.3e}), info off {off_info:.3e} of its "
          f"largest entry; against the truth {e[0]:.4f} deg {1000 * e[1]:.3f} mm")
    assert res["n"] == res_r["n"] and res["n_valid"] == res_r["n_valid"] and res["stages"] == 36
    assert res["flags"] == 0 and not res["lost"] and (info == info.T).all()
    assert off_T <= 100 * delta[0]
    assert off_info <= 100 * delta[0]
    assert abs(res["fitness"] - res_r["fitness"]) <= 1e-15 and abs(res["cost"] - res_r["cost"]) <= 1e-12 * res_r["cost"]
    first, second = rgbd_odometry_device(src, dst), rgbd_odometry_device(src, dst)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    init = OR.pair_truth(seq["poses"], 1, 0)
    T2, _, res2 = rgbd_odometry(src, dst, init=init, iterations=(1, 1, 1))
    Tr2, _, res2_r = OR.odometry(src_r, dst_r, init=init, iterations=(1, 1, 1))
    assert res2["n"] == res2_r["n"] and np.abs(T2 - Tr2).max() <= 100 * delta[0]


# ---- track ------------------------------------------------------------------------------------------------------------------
def test_track_keeps_every_frame_and_follows_the_camera(seqs):
    from imfnet_amd.odometry import track
    seq, m = seqs[0.3], OR.MEASURED[0.3]["track"]
    poses, kept = track(seq["depth"], seq["color"], seq["K"])
    assert kept.all() and np.array_equal(poses[0], np.eye(4))
    errs = np.array([OR.pose_error(poses[f], OR.pair_truth(seq["poses"], f, 0)) for f in range(5)])
    print(f"track at arc 0.3: worst {errs[:, 0].max():.4f} deg {1000 * errs[:, 1].max():.3f} mm")
    assert errs[:, 0].max() <= 2 * m[0] and errs[:, 1].max() <= 2 * m[1]


def test_track_drops_a_frame_without_depth_and_matches_the_next_against_the_one_before(seqs):
    from imfnet_amd.odometry import prepare_frame, rgbd_odometry, track
    seq = seqs[0.3]
    depth = seq["depth"].copy()
    depth[2] = 0
    poses, kept = track(depth, seq["color"], seq["K"])
    assert kept.tolist() == [True, True, False, True, True] and np.isnan(poses[2]).all()
    f1, f3 = (prepare_frame(depth[f], seq["color"][f], seq["K"]) for f in (1, 3))
    T31, _, res = rgbd_odometry(f3, f1)
    assert not res["lost"] and np.array_equal(poses[3], poses[1] @ T31)
    e = OR.pose_error(poses[4], OR.pair_truth(seq["poses"], 4, 0))
    assert e[0] < 1.0 and e[1] < 0.02


# ---- from the command line ------------------------------------------------------------------------------------------------
RESTATED_MAX_DISTANCE = 0.006486261656614145      # tests/test_gpu_tsdf.py: what the posed run is held to on this scene, before its 1e-6


def _tree(tmp_path, seq):
    raw = str(tmp_path / "raw")
    sdir = S.write_tree(raw, seq)
    CS.write_color_files(sdir, seq["color"])
    return raw, sdir


def test_fragments_from_a_sequence_without_poses(tmp_path, seqs):
    """fuse_fragments --poses odometry --color on a tree without any .pose.txt, then integrate_scene on what it wrote.  The
    points, moved by the first frame's true pose, lie within the posed run's surface bound (the restatement's distance plus
    1e-6 m, as tests/test_gpu_tsdf.py has it) plus the odometry's drift: the restatement's worst `track` pose error of host
    test (d) as measured, its translation plus its rotation taken at the farthest point."""
    from imfnet_amd import fuse_fragments as FF
    from imfnet_amd.dataio import read_ply_points
    from imfnet_amd.integrate_scene import integrate_scene
    seq = seqs[0.5]
    raw, sdir = _tree(tmp_path, seq)
    for f in os.listdir(sdir):
        if f.endswith(".pose.txt"):
            os.remove(os.path.join(sdir, f))
    out = str(tmp_path / "out")
    assert FF.main(["--dataset_root", raw, "--out_root", out, "--height", "120", "--width", "160", "--frames_per_frag", "5",
                    "--poses", "odometry", "--color"]) == 0
    folder = os.path.join(out, "scene-a", "seq-01")
    with open(os.path.join(folder, "cloud_bin_0.frames.pkl"), "rb") as fh:
        record = pickle.load(fh)
    assert len(record["frames"]) == 5 and record["poses"].shape == (5, 4, 4) and record["poses"].dtype == np.float64
    assert np.array_equal(record["poses"][0], np.eye(4))
    assert np.array_equal(np.load(os.path.join(folder, "cloud_bin_0.pose.npy")), np.eye(4, dtype=np.float32))
    errs = np.array([OR.pose_error(record["poses"][f], OR.pair_truth(seq["poses"], f, 0)) for f in range(5)])
    xyz = read_ply_points(os.path.join(folder, "cloud_bin_0.ply"))
    m = OR.MEASURED[0.5]["track"]
    far = float(np.linalg.norm(xyz, axis=1).max())
    bound = RESTATED_MAX_DISTANCE + 1e-6 + m[1] + far * np.radians(m[0])
    world = xyz @ seq["poses"][0][:3, :3].T + seq["poses"][0][:3, 3]
    d = S.surface_distance(world)
    print(f"poses off by at most {errs[:, 0].max():.4f} deg {1000 * errs[:, 1].max():.3f} mm; {len(xyz)} points, distance to "
          f"the surface max {d.max():.6e} m, bound {bound:.6e} m")
    assert len(xyz) > 10000 and d.max() <= bound
    traj = str(tmp_path / "trajectory.log")
    with open(traj, "w") as fh:
        fh.write("0 0 1\n" + "\n".join(" ".join(str(v) for v in row) for row in np.eye(4)) + "\n")
    res = integrate_scene(folder, sdir, traj, str(tmp_path / "scene"), height=120, width=160, color=True, log=lambda *a: None)
    assert res["frames"] == 5 and res["fragments_used"] == [0] and res["triangles"] > 10000
    assert os.path.exists(os.path.join(str(tmp_path / "scene"), "scene_mesh.ply"))


def test_the_default_pose_source_writes_the_bytes_it_wrote(tmp_path, seqs):
    """--poses file against the path that was there before the option: the library calls the command made then, made here
    by hand (select_frames, fuse_fragment, write_ply, the one-key record)."""
    from imfnet_amd import fuse_fragments as FF
    from imfnet_amd.fuse import fuse_fragment
    seq = seqs[0.5]
    raw, sdir = _tree(tmp_path, seq)
    base = ["--dataset_root", raw, "--height", "120", "--width", "160", "--frames_per_frag", "5"]
    outs = [str(tmp_path / "a"), str(tmp_path / "b")]
    assert FF.main(base + ["--out_root", outs[0], "--poses", "file"]) == 0
    assert FF.main(base + ["--out_root", outs[1]]) == 0
    read = lambda out, name: open(os.path.join(out, "scene-a", "seq-01", name), "rb").read()
    colors = [os.path.join(sdir, f) for f in FF.list_color_files(sdir)]
    pose0, frames = FF.select_frames(colors, 0, 5)
    K = np.loadtxt(os.path.join(raw, "scene-a", "camera-intrinsics.txt"), dtype=np.float32).astype(np.float64)
    want = fuse_fragment(seq["depth"], np.stack([p for _, p in frames]).astype(np.float64), K, voxel_length=3.0 / 512)
    FF.write_ply(str(tmp_path / "want.ply"), want)
    ply = open(str(tmp_path / "want.ply"), "rb").read()
    pkl = pickle.dumps({"frames": [s for s, _ in frames]}, protocol=pickle.HIGHEST_PROTOCOL)
    for out in outs:
        assert read(out, "cloud_bin_0.ply") == ply and read(out, "cloud_bin_0.frames.pkl") == pkl
        assert np.array_equal(np.load(os.path.join(out, "scene-a", "seq-01", "cloud_bin_0.pose.npy")), pose0)
