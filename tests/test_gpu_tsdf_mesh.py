"""Mesh extraction on the GPU (csrc/tsdf_mesh.hip through imfnet_amd/fuse.py) against the NumPy restatement of its rule
(tests/tsdf_mesh_restate.py): bit for bit on the state the GPU integrated, on analytic spheres laid across unit faces,
edges and a corner, with a unit missing; the call's contract; frames -> fragments -> trajectory -> scene mesh."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsdf_mesh_restate as M   # noqa: E402
import tsdf_restate as R        # noqa: E402
import tsdf_scene as S          # noqa: E402

pytestmark = pytest.mark.gpu

# The slab of the sphere tests: one frame of a flat wall 1.04 m in front of a camera at the origin, voxels of 0.01 m (units
# of 0.16 m) and a truncation of 0.2 m, which reaches 2 units: the units -6..5 x -5..4 x 4..8 open, voxel indices 64..143 in
# z.  The sphere (indices, not metres) has radius 12 = 1.5 units of diameter and sits on the unit corner (0, 0, 112), so it
# crosses a unit face on every axis, the three unit edges and the corner: its cells read all seven + neighbours.  Its values
# are clip(sd / 2 voxels, -1, 1), so the valid band (< 0.98) ends 1.96 voxels outside: within 14 voxels of the centre.
SLAB = dict(voxel_length=0.01, sdf_trunc=0.2)
SPHERE_R = 12.0
CENTRES = {"off_lattice": (0.3, 0.7, 112.1), "on_lattice": (0.0, 0.0, 112.0)}
# The end-to-end scene (six frames of make_sequence(160, 120, 6) in two fragments, the scene poses of scene_frame_poses):
# tsdf_restate.allocate / integrate and tsdf_mesh_restate.mesh on the same frames and poses, measured on the CPU, give 2 197
# units, 409 777 vertices, 808 070 triangles and this largest distance of a vertex to the analytic surface (the tail is the
# depth discontinuity around the sphere, on an axis edge: extract's points reach the same figure; the median is 0.27 mm).
E2E_RESTATED_MAX_DISTANCE = 0.006063918720075279
E2E_RESTATED_UNITS = 2197
E2E_RESTATED_COUNTS = (409777, 808070)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def restate(vol, state=None):
    state = vol.voxels() if state is None else state
    n = len(state)
    return M.mesh(vol.units, state[..., 0].reshape(n, 16, 16, 16), state[..., 1].reshape(n, 16, 16, 16),
                  vol.params.voxel_length, vol.params.lattice_offset)


@pytest.fixture(scope="module")
def seq():
    return S.make_sequence(160, 120, n_frames=5)


@pytest.fixture(scope="module")
def scene(seq):
    """The volume of the existing scene, its mesh from the GPU and from the restatement on the SAME float32 state."""
    from imfnet_amd.fuse import TSDFVolume
    vol = TSDFVolume(seq["K"], 120, 160, unit_capacity=1 << 12)
    vol.allocate(seq["depth"], seq["poses"])
    vol.integrate(seq["depth"], seq["poses"])
    v, t = vol.extract_mesh()
    return vol, v, t, restate(vol)


def open_slab():
    from imfnet_amd.fuse import TSDFVolume
    vol = TSDFVolume(S.intrinsic(160, 120), 120, 160, unit_capacity=1 << 10, **SLAB)
    vol.allocate(np.full((1, 120, 160), 1040, np.uint16), np.eye(4)[None])
    assert vol.flags == 0 and vol.n_units > 0
    return vol


def sphere_state(units, centre, radius=SPHERE_R):
    """float32 [n, 4096, 2]: tsdf = clip(sd / 2, -1, 1) of the sphere in voxel indices, weight 1."""
    l = np.arange(16)
    g = [(16 * units[:, a].astype(np.int64)[:, None] + l).astype(np.float64) - centre[a] for a in range(3)]
    sd = np.sqrt(g[0][:, None, None, :] ** 2 + g[1][:, None, :, None] ** 2 + g[2][:, :, None, None] ** 2) - radius
    val = np.clip(sd / 2.0, -1.0, 1.0).astype(np.float32)
    return np.stack([val, np.ones_like(val)], -1).reshape(len(units), 4096, 2)


def band_is_open(units, centre, radius=SPHERE_R):
    """Every unit that holds a sample within radius + 2 voxels of the centre is opened."""
    have = set(map(tuple, units.tolist()))
    lo = [int(np.floor((c - radius - 2.0) / 16.0)) for c in centre]
    hi = [int(np.floor((c + radius + 2.0) / 16.0)) for c in centre]
    return all((x, y, z) in have for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1)
               for z in range(lo[2], hi[2] + 1))


@pytest.fixture(scope="module")
def slab():
    return open_slab()


@pytest.fixture(scope="module")
def spheres(slab):
    """name -> (state, GPU vertices, GPU triangles, restatement) on the one opened slab."""
    out = {}
    for name, c in CENTRES.items():
        assert band_is_open(slab.units, c)
        state = sphere_state(slab.units, c)
        slab.load_voxels(state)
        v, t = slab.extract_mesh()
        out[name] = (state, v, t, restate(slab, state))
    return out


def test_scene_mesh_equals_the_restatement_bit_for_bit(scene):
    vol, v, t, ref = scene
    print(f"scene: {vol.n_units} units, {len(v)} vertices, {len(t)} triangles (restatement {len(ref['vertices'])}, "
          f"{len(ref['triangles'])})")
    assert len(v) > 10000 and len(t) > 10000
    assert v.dtype == np.float64 and t.dtype == np.int32
    assert same_bits(v, ref["vertices"])
    assert same_bits(t, ref["triangles"])
    top = M.topology(len(v), t)
    assert top["unreferenced"] == 0 and top["repeated"] == 0 and t.min() >= 0 and t.max() < len(v)


def test_axis_vertices_are_extracts_points(scene):
    """The vertices on slots 0..2 whose two ends are non-zero are rows of extract(), bit for bit."""
    vol, v, _, ref = scene
    pts = vol.extract()
    slot = ref["keys"] % 7
    sel = (slot < 3) & (ref["ends"][:, 0] != 0) & (ref["ends"][:, 1] != 0)
    rows = set(r.tobytes() for r in pts)
    assert sel.sum() > 10000 and len(rows) == len(pts)
    missing = sum(1 for r in v[sel] if r.tobytes() not in rows)
    print(f"{int(sel.sum())} axis vertices with non-zero ends of {len(v)}, extract has {len(pts)} points, {missing} missing")
    assert missing == 0


@pytest.mark.parametrize("name", list(CENTRES))
def test_sphere_across_unit_faces_is_closed(spheres, slab, name):
    state, v, t, ref = spheres[name]
    assert same_bits(v, ref["vertices"]) and same_bits(t, ref["triangles"])
    top = M.topology(len(v), t)
    # the cells' corners come from all seven + neighbours: the owners of the vertices span the eight units at the corner
    owners = set(map(tuple, slab.units[np.unique(ref["keys"] // 7 // 4096)].tolist()))
    zero_area = int((np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1) == 0).sum())
    print(f"{name}: V {top['V']} E {top['E']} F {top['F']} chi {top['chi']}, zero-area triangles {zero_area}, "
          f"exact zeros {(state[..., 0] == 0).sum()}")
    assert {(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (6, 7)} <= owners
    assert top["chi"] == 2 and top["closed"] and top["unreferenced"] == 0
    if name == "on_lattice":
        assert (state[..., 0] == 0).sum() >= 6 and zero_area > 0
    vol_m = M.signed_volume(v, t)
    assert 0 < vol_m < 4.0 / 3.0 * np.pi * (SPHERE_R * 0.01) ** 3


def test_missing_neighbour_opens_the_surface_there_only(spheres, slab):
    """The off-lattice sphere with every sample of unit (0, 0, 7) invalid (w = 0): equal to the restatement, and every
    boundary edge lies on the cells that lost a corner: the samples 16 U - 1 .. 16 U + 16 of that unit."""
    state = spheres["off_lattice"][0].copy()
    units = slab.units
    hole = int(np.flatnonzero((units == np.array([0, 0, 7])).all(1))[0])
    state[hole, :, 1] = 0.0
    slab.load_voxels(state)
    v, t = slab.extract_mesh()
    ref = restate(slab, state)
    assert same_bits(v, ref["vertices"]) and same_bits(t, ref["triangles"])
    top = M.topology(len(v), t)
    assert top["repeated"] == 0 and top["unreferenced"] == 0 and len(top["unpaired"]) > 0
    ti, ei = top["unpaired"][:, 0], top["unpaired"][:, 1]
    ends = np.concatenate([v[t[ti, ei]], v[t[ti, (ei + 1) % 3]]]) / 0.01 - 0.5         # in voxel indices
    lo, hi = 16.0 * np.array([0, 0, 7]) - 1.0, 16.0 * np.array([0, 0, 7]) + 16.0
    print(f"missing unit: {len(t)} triangles, {len(ti)} boundary edges")
    assert (ends >= lo - 1e-9).all() and (ends <= hi + 1e-9).all()
    # and away from that unit nothing changed: the triangles of cells that do not touch it are the closed sphere's
    assert len(t) < len(spheres["off_lattice"][2])


def raw_mesh(vol, v_cap, t_cap, ws_bytes=None, fill=7):
    """One imf_tsdf_mesh call with its own buffers -> (rc, out_n, vertices, triangles); the buffers start as `fill`."""
    import torch
    from imfnet_amd import _lib
    L = _lib.lib()
    dev = vol.device
    p = lambda x: C.c_void_p(x.data_ptr())
    need = L.imf_tsdf_mesh_workspace_bytes(vol.n_units)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out_n = torch.full((2,), -5, dtype=torch.int64, device=dev)
    v = torch.full((max(1, v_cap), 3), float(fill), dtype=torch.float64, device=dev)
    t = torch.full((max(1, t_cap), 3), fill, dtype=torch.int32, device=dev)
    rc = L.imf_tsdf_mesh(p(vol._voxels), p(vol._units), p(vol._meta), vol.n_units, p(vol._table), vol.table_capacity,
                         C.byref(vol.params), p(v) if v_cap else None, v_cap, p(t) if t_cap else None, t_cap, p(out_n), p(ws),
                         need if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return rc, out_n.tolist(), v.cpu().numpy(), t.cpu().numpy(), L


def test_contract(spheres, slab):
    state, v, t, _ = spheres["off_lattice"]
    slab.load_voxels(state)
    n_v, n_t = len(v), len(t)
    rc, n, _, _, L = raw_mesh(slab, 0, 0)                               # count only
    assert rc == 0 and n == [n_v, n_t]
    rc, n, gv, gt, _ = raw_mesh(slab, n_v, n_t)                         # exact room: the bytes of extract_mesh
    assert rc == 0 and n == [n_v, n_t] and same_bits(gv, v) and same_bits(gt, t)
    rc, n, gv2, gt2, _ = raw_mesh(slab, n_v + 5, n_t + 3)               # a second call, more room: the same bytes
    assert rc == 0 and same_bits(gv2[:n_v], v) and same_bits(gt2[:n_t], t) and (gv2[n_v:] == 7).all() and (gt2[n_t:] == 7).all()
    for v_cap, t_cap in ((n_v - 1, n_t), (n_v, n_t - 1)):               # one short on either side: nothing is written
        rc, n, gv, gt, _ = raw_mesh(slab, v_cap, t_cap)
        assert rc == 0 and n == [n_v, n_t] and (gv == 7).all() and (gt == 7).all()
    need = L.imf_tsdf_mesh_workspace_bytes(slab.n_units)
    rc, n, gv, gt, _ = raw_mesh(slab, n_v, n_t, ws_bytes=need - 1)      # refused before any launch
    assert rc == -1 and b"workspace" in L.imf_last_error() and n == [-5, -5] and (gv == 7).all()
    for cap in (0, -1, (1 << 22) + 1):
        assert L.imf_tsdf_mesh_workspace_bytes(cap) == 0
    assert need >= slab.n_units * 4096 * 5
    again = slab.extract_mesh()
    assert same_bits(again[0], v) and same_bits(again[1], t)


def test_empty_volumes(seq, slab):
    from imfnet_amd.fuse import TSDFVolume, fuse_mesh
    v, t = fuse_mesh(np.zeros_like(seq["depth"]), seq["poses"], seq["K"])          # no unit opens
    assert v.shape == (0, 3) and t.shape == (0, 3) and v.dtype == np.float64 and t.dtype == np.int32
    vol = TSDFVolume(seq["K"], 120, 160)
    assert vol.voxels().shape == (0, 4096, 2) and vol.extract_mesh()[1].shape == (0, 3)
    slab.load_voxels(np.zeros((slab.n_units, 4096, 2), np.float32))                 # units, but nothing observed
    rc, n, _, _, _ = raw_mesh(slab, 0, 0)
    assert rc == 0 and n == [0, 0]
    v, t = slab.extract_mesh()
    assert v.shape == (0, 3) and t.shape == (0, 3)
    with pytest.raises(ValueError):
        slab.load_voxels(np.zeros((slab.n_units + 1, 4096, 2), np.float32))
    back = np.random.default_rng(0).random((slab.n_units, 4096, 2)).astype(np.float32)
    slab.load_voxels(back)
    assert same_bits(slab.voxels(), back)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """6 frames as a raw tree whose poses carry a world transform, fused into two fragments of 3 frames, with --mesh."""
    from imfnet_amd import fuse_fragments as FF
    seq6 = S.make_sequence(160, 120, n_frames=6)
    root = tmp_path_factory.mktemp("mesh_tree")
    raw, out, plain = str(root / "raw"), str(root / "out"), str(root / "plain")
    a = 0.3
    world = np.array([[np.cos(a), -np.sin(a), 0.0, 0.4], [np.sin(a), np.cos(a), 0.0, -0.2], [0.0, 0.0, 1.0, 0.1],
                      [0.0, 0.0, 0.0, 1.0]])
    sdir = S.write_tree(raw, seq6, world=world)
    common = ["--dataset_root", raw, "--height", "120", "--width", "160", "--frames_per_frag", "3"]
    assert FF.run(FF.parse_args(common + ["--out_root", out, "--mesh"]), log=lambda *_: None) == 2
    assert FF.run(FF.parse_args(common + ["--out_root", plain]), log=lambda *_: None) == 2
    return dict(seq=seq6, raw_seq=sdir, frags=os.path.join(out, "scene-a", "seq-01"),
                plain=os.path.join(plain, "scene-a", "seq-01"), root=str(root))


def test_mesh_flag_leaves_the_cloud_alone(tree):
    from imfnet_amd.dataio import read_ply_mesh, read_ply_points
    for k in (0, 1):
        with open(os.path.join(tree["frags"], f"cloud_bin_{k}.ply"), "rb") as a, \
                open(os.path.join(tree["plain"], f"cloud_bin_{k}.ply"), "rb") as b:
            assert a.read() == b.read()
        assert not os.path.exists(os.path.join(tree["plain"], f"cloud_bin_{k}.mesh.ply"))
        v, t = read_ply_mesh(os.path.join(tree["frags"], f"cloud_bin_{k}.mesh.ply"))
        assert len(v) > 10000 and len(t) > 10000 and t.max() < len(v)
        assert (read_ply_points(os.path.join(tree["frags"], f"cloud_bin_{k}.mesh.ply")) == v).all()


def scene_frame_poses(tree):
    """The scene poses of the six frames as integrate_scene forms them, from the files: fragment 0's frame is the scene's."""
    from imfnet_amd.fuse_fragments import read_extrinsic
    raw = [read_extrinsic(os.path.join(tree["raw_seq"], "frame-%06d.pose.txt" % f)) for f in range(6)]
    base = [np.load(os.path.join(tree["frags"], f"cloud_bin_{k}.pose.npy")) for k in (0, 1)]
    X = [np.eye(4), np.linalg.inv(base[0].astype(np.float64)) @ base[1].astype(np.float64)]
    poses = [X[f // 3] @ np.matmul(np.linalg.inv(base[f // 3]), raw[f]).astype(np.float64) for f in range(6)]
    return X, np.stack(poses)


def test_integrate_scene_end_to_end(tree):
    """Every vertex of scene_mesh.ply lies within the distance of the analytic surface that the restatement reaches on
    the same frames and poses (E2E_RESTATED_MAX_DISTANCE), plus 1e-6 m.  The scene frame is fragment 0's first camera, so
    the vertices are moved back into the analytic scene's world by that frame's true pose first."""
    from imfnet_amd.dataio import read_ply_mesh
    from imfnet_amd.integrate_scene import integrate_scene
    from imfnet_amd.pose_graph import write_log
    X, poses = scene_frame_poses(tree)
    seq6 = tree["seq"]
    out = os.path.join(tree["root"], "scene")
    os.makedirs(out, exist_ok=True)
    traj = os.path.join(out, "trajectory.log")
    write_log(traj, [(k, k, 2, X[k]) for k in (0, 1)])
    lines = []
    res = integrate_scene(tree["frags"], tree["raw_seq"], traj, out, height=120, width=160, log=lines.append)
    assert res["fragments_used"] == [0, 1] and res["fragments_skipped"] == [] and res["frames"] == 6 and res["flags"] == 0
    assert len(lines) == 1 and lines[0].startswith("{")
    v, t = read_ply_mesh(os.path.join(out, "scene_mesh.ply"))
    assert res["vertices"] == len(v) > 10000 and res["triangles"] == len(t) > 10000
    top = M.topology(len(v), t)
    assert top["unreferenced"] == 0 and top["repeated"] == 0
    K = np.loadtxt(os.path.join(os.path.dirname(tree["raw_seq"]), "camera-intrinsics.txt"), dtype=np.float32).astype(np.float64)
    assert res["units"] == len(R.allocate(seq6["depth"], poses, K, R.params())) == E2E_RESTATED_UNITS
    to_world = seq6["poses"][0]                               # scene frame = frame 0's camera -> the analytic scene's world
    d = S.surface_distance(v @ to_world[:3, :3].T + to_world[:3, 3])
    print(f"scene mesh: {len(v)} vertices, {len(t)} triangles (restatement {E2E_RESTATED_COUNTS}), distance to the surface "
          f"max {d.max():.6e} m, median {np.median(d):.3e} m; restatement max {E2E_RESTATED_MAX_DISTANCE:.6e} m")
    assert d.max() <= E2E_RESTATED_MAX_DISTANCE + 1e-6
    # a fragment with a NaN pose is skipped and reported
    write_log(traj, [(0, 0, 2, X[0]), (1, 1, 2, np.full((4, 4), np.nan))])
    res = integrate_scene(tree["frags"], tree["raw_seq"], traj, out, height=120, width=160, log=lines.append)
    assert res["fragments_used"] == [0] and res["fragments_skipped"] == [1] and res["frames"] == 3
    assert 0 < res["triangles"] < len(t)
