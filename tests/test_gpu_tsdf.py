"""Fragment fusion on the GPU (csrc/tsdf.hip through imfnet_amd/fuse.py) against the NumPy restatement
(tests/tsdf_restate.py) on the synthetic sequence of tests/tsdf_scene.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsdf_restate as R   # noqa: E402
import tsdf_scene as S     # noqa: E402

pytestmark = pytest.mark.gpu

VL = 3.0 / 512
# the largest distance of a restatement point to the analytic surface on make_sequence(160, 120, 5), measured on the CPU:
RESTATED_MAX_DISTANCE = {0.5: 0.006486261656614145, 0.0: 0.006443731760188309}     # (VL, 0.5) and (0.006, 0)


@pytest.fixture(scope="module")
def seq():
    return S.make_sequence(160, 120, n_frames=5)


@pytest.fixture(scope="module")
def restated(seq):
    return R.fuse(seq["depth"], seq["poses"], seq["K"])


@pytest.fixture(scope="module")
def fused(seq):
    from imfnet_amd.fuse import TSDFVolume
    vol = TSDFVolume(seq["K"], 120, 160, unit_capacity=1 << 12)
    vol.allocate(seq["depth"], seq["poses"])
    vol.integrate(seq["depth"], seq["poses"])
    return vol, vol.extract()


def test_unit_list_equals_the_restatement(fused, restated):
    vol, _ = fused
    units = vol.units
    assert vol.flags == 0 and units.dtype == np.int32
    assert units.shape == restated[2].shape and (units == restated[2]).all()


def test_points_match_the_restatement_by_key(fused, restated):
    """Keys (voxel, axis) on one side only: at most 0.1 % of the restatement's count (a sdf within rounding of a threshold
    may fall either way; measured on the CPU: the restatement with a fused projection differs in 0 of 134 828 keys).
    Matched points agree to 1e-6 m."""
    _, pts = fused
    ref, ref_keys, _ = restated
    keys = R.point_keys(pts, VL, 0.5)
    a = {tuple(k): i for i, k in enumerate(ref_keys.tolist())}
    b = {tuple(k): i for i, k in enumerate(keys.tolist())}
    assert len(b) == len(keys)
    only = len(set(a) ^ set(b))
    common = sorted(set(a) & set(b))
    err = np.abs(ref[[a[k] for k in common]] - pts[[b[k] for k in common]]).max()
    print(f"points {len(pts)} vs {len(ref)}, one-sided keys {only}, max |difference| of matched points {err:.3e} m")
    assert only <= 1e-3 * len(ref)
    assert err <= 1e-6


def test_points_lie_on_the_analytic_surface(fused):
    """Bound: what the restatement reaches on this scene (0.006486261656614145 m, measured on the CPU; the far tail is
    the depth discontinuity around the sphere) plus 1e-6 m."""
    _, pts = fused
    d = S.surface_distance(pts)
    print(f"distance to the surface: max {d.max():.6e} m, median {np.median(d):.3e} m")
    assert len(pts) > 10000 and d.max() <= RESTATED_MAX_DISTANCE[0.5] + 1e-6


def test_lattice_offset_zero(seq):
    """Voxel 0.006 m, offset 0: every vertex has exactly two coordinates on the 0.006 m lattice, as the published fragments
    have; the third lies strictly inside its edge.  The same surface bound, from the restatement at these settings."""
    from imfnet_amd.fuse import fuse_fragment
    pts = fuse_fragment(seq["depth"], seq["poses"], seq["K"], voxel_length=0.006, lattice_offset=0.0)
    g = pts / 0.006
    dist = np.sort(np.abs(g - np.round(g)), 1)
    assert len(pts) > 10000
    assert (dist[:, 1] < 1e-9).all() and (dist[:, 2] > 0).all()
    assert (R.lattice_census(pts, 0.006, 0.0) >= 2).all()
    d = S.surface_distance(pts)
    print(f"offset 0: {len(pts)} points, distance to the surface max {d.max():.6e} m")
    assert d.max() <= RESTATED_MAX_DISTANCE[0.0] + 1e-6
    centred = fuse_fragment(seq["depth"], seq["poses"], seq["K"], voxel_length=0.006, lattice_offset=0.5)
    assert (R.lattice_census(centred, 0.006, 0.0) <= 1).all()


def test_two_runs_are_bit_identical_and_ordered(seq, fused, restated):
    from imfnet_amd.fuse import fuse_fragment
    _, pts = fused
    again = fuse_fragment(seq["depth"], seq["poses"], seq["K"])
    assert again.shape == pts.shape and (again.view(np.int64) == pts.view(np.int64)).all()
    keys = R.point_keys(pts, VL, 0.5)
    rank = {tuple(c): i for i, c in enumerate(restated[2].tolist())}
    u, l = keys[:, :3] // 16, keys[:, :3] % 16
    order = (np.array([rank[tuple(c)] for c in u.tolist()], np.int64) * 4096 * 3
             + ((l[:, 2] * 16 + l[:, 1]) * 16 + l[:, 0]) * 3 + keys[:, 3])
    assert (np.diff(order) > 0).all()


def test_frames_in_two_goes_give_the_bits_of_one(seq, fused):
    from imfnet_amd.fuse import TSDFVolume
    _, pts = fused
    vol = TSDFVolume(seq["K"], 120, 160, unit_capacity=256)          # too small on purpose: the list grows
    vol.allocate(seq["depth"][:2], seq["poses"][:2])
    vol.allocate(seq["depth"][2:], seq["poses"][2:])
    assert vol.unit_capacity > 256 and vol.flags == 0
    vol.integrate(seq["depth"][:2], seq["poses"][:2])
    vol.integrate(seq["depth"][2:], seq["poses"][2:])
    two = vol.extract()
    assert two.shape == pts.shape and (two.view(np.int64) == pts.view(np.int64)).all()


def test_cli_end_to_end(tmp_path, seq, seeded_sd):
    """frames -> fragments -> descriptors: the command line on the synthetic tree (one pose file holds NaN), the PLY through
    the project's reader, extract_features on the written fragment."""
    import torch
    from imfnet_amd.dataio import process_image, read_image, read_ply_points
    from imfnet_amd.extract import extract_features
    from imfnet_amd.generate_desc import image_to_nchw
    from imfnet_amd.model import load_model
    raw, out = str(tmp_path / "raw"), str(tmp_path / "out")
    S.write_tree(raw, seq, nan_pose=(3,))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "imfnet_amd.fuse_fragments", "--dataset_root", raw, "--out_root", out, "--height", "120",
           "--width", "160", "--frames_per_frag", "4", "--voxel_length", "0.006", "--lattice_offset", "0", "--write_image"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    folder = os.path.join(out, "scene-a", "seq-01")
    for k in (0, 1):
        for ext in (".ply", ".pose.npy", ".frames.pkl", "_0.jpg"):
            assert os.path.exists(os.path.join(folder, f"cloud_bin_{k}{ext}"))
    xyz = read_ply_points(os.path.join(folder, "cloud_bin_0.ply"))
    # frames 0, 1, 2 (3 has no pose), relative to frame 0: the in-process result moved into frame 0's camera, as float32
    from imfnet_amd.fuse import fuse_fragment
    base_inv = np.linalg.inv(seq["poses"][0].astype(np.float32))
    rel = np.stack([np.matmul(base_inv, T.astype(np.float32)) for T in seq["poses"][:3]])
    want = fuse_fragment(seq["depth"][:3], rel.astype(np.float64), seq["K"].astype(np.float32).astype(np.float64),
                         voxel_length=0.006, lattice_offset=0.0)
    assert len(xyz) > 10000 and xyz.shape == want.shape and (xyz == want.astype(np.float32).astype(np.float64)).all()
    assert (R.lattice_census(xyz, 0.006, 0.0) >= 2).all()
    img = read_image(os.path.join(folder, "cloud_bin_0_0.jpg"))
    img = image_to_nchw(process_image(image=img, aim_H=120, aim_W=160))
    model = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3, config=None)
    model.load_state_dict(seeded_sd, strict=True)
    model = model.eval().to("cuda:0")
    with torch.no_grad():
        xyz_down, F = extract_features(model, xyz, voxel_size=0.025, device=torch.device("cuda:0"), skip_check=True, image=img)
    n_vox = len(np.unique(np.floor(xyz / 0.025).astype(np.int64), axis=0))
    assert F.shape == (n_vox, 32) and len(xyz_down) == n_vox and bool(torch.isfinite(F).all())


def test_edge_cases(seq):
    """No valid depth: n = 0.  The workspace queries answer 0 exactly for the sizes the calls refuse."""
    import torch
    from imfnet_amd import _lib
    from imfnet_amd.fuse import TSDFVolume, fuse_fragment
    empty = np.zeros_like(seq["depth"])
    assert fuse_fragment(empty, seq["poses"], seq["K"]).shape == (0, 3)
    far = np.full_like(seq["depth"], 7000)                              # beyond depth_trunc
    assert fuse_fragment(far, seq["poses"], seq["K"]).shape == (0, 3)
    L = _lib.lib()
    vol = TSDFVolume(seq["K"], 120, 160, unit_capacity=4096)
    vol.allocate(seq["depth"][:1], seq["poses"][:1])
    assert 0 < vol.n_units <= 4096 and vol.unit_capacity == 4096
    dev = vol.device
    p = lambda t: C.c_void_p(t.data_ptr())
    d = torch.from_numpy(seq["depth"][:1].view(np.int16).copy()).to(dev)
    c2w = torch.from_numpy(seq["poses"][:1, :3, :].reshape(-1, 12).copy()).to(dev)
    out_n = torch.zeros(1, dtype=torch.int64, device=dev)
    vox = torch.zeros((vol.n_units, 4096, 2), dtype=torch.float32, device=dev)
    big = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    for cap in (0, -1, (1 << 22) + 1):
        assert L.imf_tsdf_allocate_workspace_bytes(cap) == 0 and L.imf_tsdf_extract_workspace_bytes(cap) == 0
        rc = L.imf_tsdf_allocate(p(d), 1, p(c2w), C.byref(vol.params), 1, p(vol._table), vol.table_capacity, p(vol._units),
                                 cap, p(vol._meta), p(big), big.numel(), None)
        assert rc == -1 and b"unit_capacity" in L.imf_last_error()
        rc = L.imf_tsdf_extract(p(vox), p(vol._units), p(vol._meta), cap, p(vol._table), vol.table_capacity,
                                C.byref(vol.params), None, 0, p(out_n), p(big), big.numel(), None)
        assert rc == -1 and b"max_units" in L.imf_last_error()
    for cap in (1, 4096, 1 << 22):
        assert L.imf_tsdf_allocate_workspace_bytes(cap) > 0 and L.imf_tsdf_extract_workspace_bytes(cap) > 0
    # a workspace one byte short, a table that is no power of two, a lattice offset outside [0, 1): refused, nothing launched
    need = L.imf_tsdf_extract_workspace_bytes(vol.n_units)
    rc = L.imf_tsdf_extract(p(vox), p(vol._units), p(vol._meta), vol.n_units, p(vol._table), vol.table_capacity,
                            C.byref(vol.params), None, 0, p(out_n), p(big), need - 1, None)
    assert rc == -1 and b"workspace" in L.imf_last_error()
    rc = L.imf_tsdf_extract(p(vox), p(vol._units), p(vol._meta), vol.n_units, p(vol._table), vol.table_capacity - 1,
                            C.byref(vol.params), None, 0, p(out_n), p(big), big.numel(), None)
    assert rc == -1 and b"table_capacity" in L.imf_last_error()
    bad = _lib.TsdfParams.from_buffer_copy(vol.params)
    bad.lattice_offset = 1.0
    rc = L.imf_tsdf_integrate(p(d), 1, p(c2w), C.byref(bad), p(vol._units), p(vol._meta), vol.n_units, p(vox), None)
    assert rc == -1 and b"lattice_offset" in L.imf_last_error()
    torch.cuda.synchronize()
