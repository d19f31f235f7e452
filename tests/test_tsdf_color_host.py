"""Colour in the TSDF volume, the parts that need no GPU: the NumPy restatement of the colour rule against the plain
restatement and against the analytic texture (tests/tsdf_color_restate.py, tests/tsdf_color_scene.py), the PLY writers
with and without colours and the colour reader (imfnet_amd/fuse_fragments.py, imfnet_amd/dataio.py), and the command
line's colour decode with the fusion stubbed."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsdf_color_restate as CR   # noqa: E402
import tsdf_color_scene as CS     # noqa: E402
import tsdf_restate as R          # noqa: E402
import tsdf_scene as S            # noqa: E402

# |colour of a restated point - texture(point)|, the largest of the three channels, over the 134 828 points of
# make_sequence(160, 120, 5) with make_colors(seq), measured on the CPU with tsdf_color_restate.integrate_rgb / extract_rgb
# (this file's `small` fixture; the test below prints the figures it finds).  The median is the working figure: half a level
# of uint8 rounding twice over.  The tail (99 % below 18.9, 99.9 % below 34.4) is the depth discontinuity around the sphere,
# where a voxel's running mean mixes the sphere's colour with the wall's behind it -- the same voxels that carry
# RESTATED_MAX_DISTANCE in tests/test_gpu_tsdf.py.  The 499 870 mesh vertices: max 45.968, median 0.521.
RESTATED_POINT_COLOR_MAX = 47.3541923494526
RESTATED_POINT_COLOR_MEDIAN = 0.5543350727997804
RESTATED_POINTS = 134828
# voxels whose (tsdf, w) bits differ between the restatement and the restatement with a fused projection, measured here: 1
# of the 3 722 852 voxels with w != 0 (its colour is the same: the pixel did not change, only z's last bit).  The GPU test
# allows 0.1 % of the voxels with w != 0, the cap tests/test_gpu_tsdf.py uses for keys.
STATE_CAP = 1e-3

PLY_HEAD = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
PLY_NORMALS = "property float nx\nproperty float ny\nproperty float nz\n"
PLY_RGB = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
PLY_FACES = "element face %d\nproperty list uchar int vertex_indices\n"


@pytest.fixture(scope="module")
def small():
    seq = S.make_sequence(160, 120, n_frames=5)
    color = CS.make_colors(seq)
    p = R.params()
    units = R.allocate(seq["depth"], seq["poses"], seq["K"], p)
    w2c = np.linalg.inv(seq["poses"])
    state = CR.integrate_rgb(units, seq["depth"], color, w2c, seq["K"], p)
    return dict(seq=seq, color=color, p=p, units=units, w2c=w2c, state=state)


def test_texture_tells_channels_axes_and_frames_apart():
    seq = S.make_sequence(160, 120, n_frames=5)
    c = CS.make_colors(seq).astype(np.float64)
    assert c.shape == (5, 120, 160, 3)
    hit = seq["depth"] != 0
    assert c[hit].min() >= 27 and c[hit].max() <= 228       # never clamped
    for a, b in ((0, 1), (0, 2), (1, 2)):                   # a channel swap is tens of levels in the mean
        assert np.abs(c[..., a] - c[..., b])[hit].mean() > 30
    assert np.abs(c[0] - c[4]).mean() > 10                  # another frame
    assert np.abs(c[0, :, :120] - c[0, :, :120].transpose(1, 0, 2)).mean() > 20   # x / y transposed
    # the texture at the back-projected depth pixel is the pixel's colour (millimetre depth: well within one level)
    K, T = seq["K"], seq["poses"][2]
    v, u = np.nonzero(hit[2])
    d = seq["depth"][2][v, u] / 1000.0
    p = np.stack([(u - K[0, 2]) * d / K[0, 0], (v - K[1, 2]) * d / K[1, 1], d], 1) @ T[:3, :3].T + T[:3, 3]
    assert np.abs(CS.texture(p) - c[2][v, u]).max() < 1.5


def test_restated_geometry_is_the_plain_restatement(small):
    seq, p, units = small["seq"], small["p"], small["units"]
    tsdf, w, col = small["state"]
    plain = R.integrate(units, seq["depth"], small["w2c"], seq["K"], p)
    assert tsdf.tobytes() == plain[0].tobytes() and w.tobytes() == plain[1].tobytes()
    pts, keys, rgb = CR.extract_rgb(units, tsdf, w, col, p)
    ref, ref_keys = R.extract(units, plain[0], plain[1], p)
    assert pts.tobytes() == ref.tobytes() and (keys == ref_keys).all()
    assert rgb.shape == (len(pts), 3) and rgb.dtype == np.uint8 and len(pts) == RESTATED_POINTS
    assert (col[w == 0] == 0).all()                         # no colour without an observation


def test_restated_colors_follow_the_texture(small):
    tsdf, w, col = small["state"]
    pts, _, rgb = CR.extract_rgb(small["units"], tsdf, w, col, small["p"])
    err = np.abs(rgb.astype(np.float64) - CS.texture(pts)).max(1)
    print(f"{len(pts)} points: |colour - texture| max {err.max()!r}, median {np.median(err)!r}, "
          f"99 % {np.percentile(err, 99):.3f}, 99.9 % {np.percentile(err, 99.9):.3f}")
    assert err.max() <= RESTATED_POINT_COLOR_MAX + 1e-9 and np.median(err) <= RESTATED_POINT_COLOR_MEDIAN + 1e-9
    # what the bound is worth: with two channels swapped the median error is far beyond it
    swapped = np.abs(rgb[:, [1, 0, 2]].astype(np.float64) - CS.texture(pts)).max(1)
    assert np.median(swapped) > 20 * RESTATED_POINT_COLOR_MEDIAN
    m = CR.mesh_rgb(small["units"], tsdf, w, col, small["p"]["voxel_length"], small["p"]["lattice_offset"])
    e2 = np.abs(m["rgb"].astype(np.float64) - CS.texture(m["vertices"])).max(1)
    print(f"{len(e2)} vertices: max {e2.max():.3f}, median {np.median(e2):.3f}")
    assert m["rgb"].shape == (len(m["vertices"]), 3) and e2.max() <= RESTATED_POINT_COLOR_MAX and np.median(e2) < 1.0
    # axis vertices with non-zero ends are extract's points and carry their colours
    slot = m["keys"] % 7
    sel = (slot < 3) & (m["ends"][:, 0] != 0) & (m["ends"][:, 1] != 0)
    by_point = {r.tobytes(): c.tobytes() for r, c in zip(pts, rgb)}
    assert sel.sum() > 10000 and all(by_point[r.tobytes()] == c.tobytes() for r, c in zip(m["vertices"][sel], m["rgb"][sel]))


def test_restated_constant_colour_two_goes_and_fused_projection(small):
    seq, p, units, w2c, color = small["seq"], small["p"], small["units"], small["w2c"], small["color"]
    tsdf, w, col = small["state"]
    const = np.broadcast_to(np.array([200, 0, 255], np.uint8), color.shape)
    k = CR.integrate_rgb(units, seq["depth"], const, w2c, seq["K"], p)
    assert (k[2][k[1] != 0] == np.array([200, 0, 255], np.float32)).all()          # the running mean does not drift
    _, _, rgb = CR.extract_rgb(units, k[0], k[1], k[2], p)
    assert (rgb == np.array([200, 0, 255], np.uint8)).all()
    b = CR.integrate_rgb(units, seq["depth"][:3], color[:3], w2c[:3], seq["K"], p)
    b = CR.integrate_rgb(units, seq["depth"][3:], color[3:], w2c[3:], seq["K"], p, state=b)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((tsdf, w, col), b))
    f = CR.integrate_rgb(units, seq["depth"], color, w2c, seq["K"], p, fused=True)
    differ = int(((f[0] != tsdf) | (f[1] != w)).sum())
    seen = int((w != 0).sum())
    print(f"a fused projection moves (tsdf, w) of {differ} of {seen} voxels, the colour of "
          f"{int((f[2] != col).any(-1).sum())}")
    assert differ <= STATE_CAP * seen
    assert CR.to_uint8([-3.0, -0.5, 0.49, 0.5, 254.5, 255.49, 300.0, np.nan]).tolist() == [0, 0, 0, 1, 255, 255, 255, 0]


def test_ply_writers_without_colours_write_the_bytes_they_wrote(tmp_path):
    from imfnet_amd import fuse_fragments as FF
    rng = np.random.default_rng(3)
    xyz, nrm = rng.standard_normal((77, 3)) * 2, rng.standard_normal((77, 3))
    tri = rng.integers(0, 77, (50, 3)).astype(np.int32)
    p = str(tmp_path / "a.ply")
    f4 = lambda *a: np.concatenate(a, 1).astype("<f4").tobytes()
    FF.write_ply(p, xyz)
    assert open(p, "rb").read() == (PLY_HEAD % 77 + "end_header\n").encode() + f4(xyz)
    FF.write_ply_normals(p, xyz, nrm)
    assert open(p, "rb").read() == (PLY_HEAD % 77 + PLY_NORMALS + "end_header\n").encode() + f4(xyz, nrm)
    FF.write_ply_mesh(p, xyz, tri)
    faces = b"".join(b"\x03" + t.astype("<i4").tobytes() for t in tri)
    assert open(p, "rb").read() == (PLY_HEAD % 77 + PLY_FACES % 50 + "end_header\n").encode() + f4(xyz) + faces
    assert os.listdir(tmp_path) == ["a.ply"]


def test_ply_writers_with_colours_round_trip(tmp_path):
    from imfnet_amd import fuse_fragments as FF
    from imfnet_amd.dataio import read_ply_colors, read_ply_mesh, read_ply_points, read_ply_points_numpy
    rng = np.random.default_rng(4)
    xyz, nrm = rng.standard_normal((91, 3)) * 2, rng.standard_normal((91, 3))
    rgb = rng.integers(0, 256, (91, 3)).astype(np.uint8)
    rgb[0], rgb[1] = (0, 128, 255), (255, 0, 1)
    tri = rng.integers(0, 91, (40, 3)).astype(np.int32)
    as_f32 = xyz.astype(np.float32).astype(np.float64)
    p = str(tmp_path / "c.ply")
    rows = lambda fl: b"".join(a.astype("<f4").tobytes() + c.tobytes() for a, c in zip(fl, rgb))

    FF.write_ply(p, xyz, rgb)
    assert open(p, "rb").read() == (PLY_HEAD % 91 + PLY_RGB + "end_header\n").encode() + rows(xyz)
    assert (read_ply_colors(p) == rgb).all() and read_ply_colors(p).dtype == np.uint8
    assert (read_ply_points(p) == as_f32).all() and (read_ply_points_numpy(p) == as_f32).all()    # the readers skip the colours

    FF.write_ply_normals(p, xyz, nrm, rgb)
    assert open(p, "rb").read() == (PLY_HEAD % 91 + PLY_NORMALS + PLY_RGB + "end_header\n").encode() + rows(np.concatenate([xyz, nrm], 1))
    assert (read_ply_colors(p) == rgb).all() and (read_ply_points(p) == as_f32).all()
    assert (read_ply_points_numpy(p) == as_f32).all()

    FF.write_ply_mesh(p, xyz, tri, rgb)
    v, t = read_ply_mesh(p)
    assert (v == as_f32).all() and (t == tri).all() and (read_ply_colors(p) == rgb).all()
    assert (read_ply_points(p) == as_f32).all()
    head = open(p, "rb").read().split(b"end_header\n")[0].decode()
    assert head == PLY_HEAD % 91 + PLY_RGB + PLY_FACES % 40

    for plain in (lambda: FF.write_ply(p, xyz), lambda: FF.write_ply_normals(p, xyz, nrm), lambda: FF.write_ply_mesh(p, xyz, tri)):
        plain()
        assert read_ply_colors(p) is None
    FF.write_ply(p, np.zeros((0, 3)), np.zeros((0, 3), np.uint8))
    assert read_ply_colors(p).shape == (0, 3) and read_ply_points(p).shape == (0, 3)
    for bad in (rgb[:-1], rgb.astype(np.float32), rgb[:, :2]):
        with pytest.raises(ValueError):
            FF.write_ply(p, xyz, bad)
    assert os.listdir(tmp_path) == ["c.ply"]


def test_header_and_signatures_declare_the_colour_entry_points():
    from imfnet_amd import _lib
    text = open(os.path.join(ROOT, "include", "imfnet_hip.h")).read()
    for name in ("imf_tsdf_integrate_rgb", "imf_tsdf_extract_rgb", "imf_tsdf_mesh_rgb"):
        assert re.search(r"\b%s\(" % name, text) and name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
        plain = name[:-4]                                   # the plain call's arguments plus two
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[plain][1]) + 2


def test_cli_decodes_the_integrated_frames_colour_files(tmp_path):
    """7 frames in fragments of 3 with the pose rules of test_tsdf_host's walk: under --color the fragment carries exactly
    the decoded colour files of its integrated frames and the files carry the stub's colours; without the flag, and with a
    stub that returns no colours, the files have the bytes the documented headers give."""
    from PIL import Image
    from imfnet_amd import fuse_fragments as FF
    from imfnet_amd.dataio import read_ply_colors, read_ply_mesh, read_ply_points
    seq = S.make_sequence(32, 24, n_frames=7)
    S.write_tree(str(tmp_path / "raw"), seq, nan_pose=(1, 3))
    seen = []
    tri = np.array([[0, 1, 2], [2, 3, 4]], np.int32)

    def points(frag):
        return np.arange(15, dtype=np.float64).reshape(5, 3) + len(frag["stems"])

    def stub(cfg, intrinsic, frag):
        seen.append(frag)
        rgb = np.arange(15, dtype=np.uint8).reshape(5, 3) * 17
        return dict(points=points(frag), rgb=rgb, mesh=(points(frag) + 0.5, tri, rgb[::-1].copy()))

    common = ["--dataset_root", str(tmp_path / "raw"), "--frames_per_frag", "3", "--height", "24", "--width", "32", "--threads", "2"]
    cfg = FF.parse_args(common + ["--out_root", str(tmp_path / "out"), "--color", "--mesh", "--normals"])
    assert cfg.color and not FF.parse_args(common + ["--out_root", "x"]).color
    normals = lambda cfg, xyz: np.tile([0.0, 0.0, 1.0], (len(xyz), 1))
    assert FF.run(cfg, fuse=stub, log=lambda s: None, normals=normals) == 2
    f0, f2 = seen
    assert [os.path.basename(s) for s in f0["stems"]] == ["frame-000000", "frame-000002"]
    assert [os.path.basename(s) for s in f2["stems"]] == ["frame-000006"]
    for frag in seen:
        assert frag["color"].dtype == np.uint8 and frag["color"].shape == (len(frag["stems"]), 24, 32, 3)
        for got, stem in zip(frag["color"], frag["stems"]):
            with Image.open(stem + ".color.jpg") as im:
                assert (got == np.asarray(im)).all()
    assert not (f0["color"][0] == f0["color"][1]).all()
    out = tmp_path / "out" / "scene-a" / "seq-01"
    rgb = np.arange(15, dtype=np.uint8).reshape(5, 3) * 17
    assert (read_ply_colors(str(out / "cloud_bin_0.ply")) == rgb).all()
    assert (read_ply_points(str(out / "cloud_bin_0.ply")) == points(f0)).all()
    v, t = read_ply_mesh(str(out / "cloud_bin_2.mesh.ply"))
    assert (v == points(f2) + 0.5).all() and (t == tri).all()
    assert (read_ply_colors(str(out / "cloud_bin_2.mesh.ply")) == rgb[::-1]).all()
    head = (out / "cloud_bin_0.ply").read_bytes().split(b"end_header\n")[0].decode()
    assert head == PLY_HEAD % 5 + PLY_NORMALS + PLY_RGB
    # a wrong --height / --width is refused with the depth reader's message
    with pytest.raises(ValueError, match=r"24 x 32, expected 25 x 32 \(--height / --width\)"):
        FF.read_color_jpg(f0["stems"][0] + ".color.jpg", 25, 32)

    # no flag, a stub without colours: no colour file is decoded and the bytes are the plain ones
    seen.clear()

    def plain_stub(cfg, intrinsic, frag):
        seen.append(frag)
        return points(frag)

    cfg = FF.parse_args(common + ["--out_root", str(tmp_path / "plain")])
    assert FF.run(cfg, fuse=plain_stub, log=lambda s: None) == 2
    assert all("color" not in frag for frag in seen)
    plain = tmp_path / "plain" / "scene-a" / "seq-01"
    assert (plain / "cloud_bin_0.ply").read_bytes() == (PLY_HEAD % 5 + "end_header\n").encode() + points(f0).astype("<f4").tobytes()
    assert sorted(os.listdir(plain)) == sorted(f"cloud_bin_{k}{e}" for k in (0, 2) for e in (".ply", ".pose.npy", ".frames.pkl"))
