"""The mesh rule on the CPU, restatement only (tests/tsdf_mesh_restate.py): closed analytic surfaces on a 24^3 lattice, an
open one, the case table and its generator, the constant table of csrc/tsdf_mesh.hip, and the mesh PLY files."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsdf_mesh_restate as M   # noqa: E402

N = 24                                                      # the lattice of the surfaces, inside 2 x 2 x 2 units


def lattice(sd_fn, n=N, extra_valid=None):
    """values clip(sd / 2 voxels, -1, 1) as float32 on 32^3 samples, valid = < 0.98 and inside the n^3 lattice."""
    g = np.arange(32, dtype=np.float64)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    val = np.clip(sd_fn(x, y, z) / 2.0, -1.0, 1.0).astype(np.float32)
    valid = (val < np.float32(0.98)) & (x < n) & (y < n) & (z < n)
    if extra_valid is not None:
        valid &= extra_valid(x, y, z)
    return M.lattice_units(val, valid)


def sphere(c, r):
    return lambda x, y, z: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r


def torus(c, R, r):
    def sd(x, y, z):
        q = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - R
        return np.sqrt(q * q + (z - c[2]) ** 2) - r
    return sd


def cube(lo, hi):
    def sd(x, y, z):
        m, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
        q = np.stack([np.abs(x - m) - h, np.abs(y - m) - h, np.abs(z - m) - h])
        return np.linalg.norm(np.maximum(q, 0.0), axis=0) + np.minimum(q.max(0), 0.0)
    return sd


# name -> (signed distance, V, E, F, chi, zero-area triangles, analytic volume, measured shortfall of the mesh volume or None)
# The shortfalls are the restatement's own, measured here: 0.911742 % (sphere) and 2.496785 % (torus); the gate is twice that.
SURFACES = {
    "sphere_off_lattice": (sphere((11.3, 11.7, 12.1), 7.4), 3088, 9258, 6172, 2, 0, 4.0 / 3.0 * np.pi * 7.4 ** 3, 0.00911742),
    "torus": (torus((11.6, 11.4, 11.5), 6.3, 2.6), 3004, 9012, 6008, 0, 0, 2.0 * np.pi ** 2 * 6.3 * 2.6 ** 2, 0.02496785),
    "sphere_on_lattice": (sphere((12.0, 12.0, 12.0), 5.0), 1298, 3888, 2592, 2, 228, 4.0 / 3.0 * np.pi * 125.0, None),
    "cube_on_lattice_planes": (cube(8.0, 16.0), 1094, 3276, 2184, 2, 1512, 512.0, None),
}


@pytest.mark.parametrize("name", list(SURFACES))
def test_closed_surfaces(name):
    sd, V, E, F, chi, zero_area, analytic, shortfall = SURFACES[name]
    units, tsdf, w = lattice(sd)
    r = M.mesh(units, tsdf, w, 1.0, 0.0)
    v, t = r["vertices"], r["triangles"]
    top = M.topology(len(v), t)
    area = np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1)
    vol = M.signed_volume(v, t)
    print(f"{name}: V {top['V']} E {top['E']} F {top['F']} chi {top['chi']}, zero-area {int((area == 0).sum())}, volume {vol:.4f} "
          f"of {analytic:.4f}: {100.0 * (1.0 - vol / analytic):.6f} % below")
    assert (top["V"], top["E"], top["F"], top["chi"]) == (V, E, F, chi)
    assert top["closed"]                                   # every directed edge once, its reverse once
    assert top["unreferenced"] == 0
    assert t.dtype == np.int32 and t.min() >= 0 and t.max() < len(v)
    assert int((area == 0).sum()) == zero_area
    assert 0.0 < vol < analytic
    if shortfall is not None:
        assert vol > analytic * (1.0 - 2.0 * shortfall)
    # vertices in the stated order, each on its edge
    assert (np.diff(r["keys"]) > 0).all()


def test_open_surface_boundary():
    """A slanted plane through a block whose outer samples are invalid: the mesh has a boundary; a boundary edge occurs
    once, and the cell of its triangle touches an unmeshed cell."""
    n = np.array([0.37, 0.21, 0.9]) / np.linalg.norm([0.37, 0.21, 0.9])
    inside_block = lambda x, y, z: (x >= 5) & (x <= 20) & (y >= 4) & (y <= 21) & (z >= 3) & (z <= 22)
    units, tsdf, w = lattice(lambda x, y, z: n[0] * x + n[1] * y + n[2] * z - 14.2, extra_valid=inside_block)
    r = M.mesh(units, tsdf, w, 1.0, 0.0)
    t = r["triangles"]
    top = M.topology(len(r["vertices"]), t)
    assert len(t) > 500 and top["repeated"] == 0 and top["unreferenced"] == 0 and not top["closed"]
    assert len(top["unpaired"]) > 20
    meshed = np.zeros((34, 34, 34), bool)                  # dense, one cell of margin (unmeshed)
    for i, (ux, uy, uz) in enumerate(units.tolist()):
        meshed[1 + 16 * uz:17 + 16 * uz, 1 + 16 * uy:17 + 16 * uy, 1 + 16 * ux:17 + 16 * ux] = r["meshed"][i]
    cells = r["cells"][top["unpaired"][:, 0]]
    gz = 16 * units[cells[:, 0], 2] + cells[:, 1] + 1
    gy = 16 * units[cells[:, 0], 1] + cells[:, 2] + 1
    gx = 16 * units[cells[:, 0], 0] + cells[:, 3] + 1
    for z, y, x in zip(gz, gy, gx):
        assert meshed[z, y, x] and not meshed[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2].all()
    # interior edges are paired: the unpaired ones are a small share
    assert len(top["unpaired"]) < 0.2 * 3 * len(t)


def test_cell_with_an_invalid_corner_emits_nothing():
    units = np.zeros((1, 3), np.int32)
    tsdf = np.ones((1, 16, 16, 16), np.float32)
    w = np.zeros((1, 16, 16, 16), np.float32)
    tsdf[0, 3:5, 7:9, 9:11] = np.float32(0.4)
    tsdf[0, 3, 7, 9] = np.float32(-0.3)
    w[0, 3:5, 7:9, 9:11] = 1.0
    r = M.mesh(units, tsdf, w, 1.0, 0.0)
    assert len(r["triangles"]) == 6 and len(r["vertices"]) == 7        # corner 0 inside: one triangle per tetrahedron
    assert M.topology(7, r["triangles"])["unreferenced"] == 0
    for b in range(1, 8):
        w2 = w.copy()
        w2[0, 3 + (b >> 2), 7 + ((b >> 1) & 1), 9 + (b & 1)] = 0.0
        r = M.mesh(units, tsdf, w2, 1.0, 0.0)
        assert len(r["triangles"]) == 0 and len(r["vertices"]) == 0
    t2 = tsdf.copy()
    t2[0, 4, 8, 10] = np.float32(0.98)                                # not below 0.98: invalid as well
    assert len(M.mesh(units, t2, w, 1.0, 0.0)["triangles"]) == 0
    t2[0, 4, 8, 10] = np.float32(0.0)                                 # a stored 0 is valid and outside
    assert len(M.mesh(units, t2, w, 1.0, 0.0)["triangles"]) == 6


def test_case_table_generator():
    """All 16 cases x 6 tetrahedra: the stated triangle counts, every triangle wound counter-clockwise seen from the outside
    corners with its vertices at the edge midpoints, every vertex on an edge with one end inside; an odd permutation's
    table is the even one's with the last two vertices swapped."""
    assert len(M.PERMS) == 6 and list(M.PERMS) == sorted(M.PERMS)
    assert M.TET_CORNERS == ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
    for q in range(6):
        P = [M.corner_xyz(b) for b in M.TET_CORNERS[q]]
        odd = M.perm_parity(M.PERMS[q])
        assert odd == (np.linalg.det(np.stack([P[1] - P[0], P[2] - P[1], P[3] - P[2]])) < 0)
        for case in range(16):
            ins = [i for i in range(4) if (case >> i) & 1]
            out = [i for i in range(4) if not (case >> i) & 1]
            tris = M.CASES[q][case]
            assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[len(ins)]
            assert tris == [tr if not odd else (tr[0], tr[2], tr[1]) for tr in M.CASES[0][case]]
            for tr in tris:
                mid = []
                for e in tr:
                    lo, hi = M.LOCAL_EDGES[e]
                    assert (lo in ins) != (hi in ins)
                    mid.append(0.5 * (P[lo] + P[hi]))
                normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
                assert np.linalg.norm(normal) > 0
                for i in ins:
                    for o in out:
                        assert normal @ (P[o] - P[i]) > 0          # from every inside corner to every outside corner
            if len(ins) == 2:                                        # the quad (ac, ad, bd, bc), split along ac - bd
                (a, b), (c, d) = ins, out
                quad = [M.EDGE_NO[tuple(sorted(p))] for p in ((a, c), (a, d), (b, d), (b, c))]
                assert {frozenset(tr) for tr in tris} == {frozenset(quad[:3]), frozenset([quad[0], quad[2], quad[3]])}
                assert tris[0][0] == quad[0] and tris[1][0] == quad[0]


def test_hip_constant_table_is_the_generated_one():
    text = open(os.path.join(ROOT, "imfnet_amd", "csrc", "tsdf_mesh.hip")).read()
    body = re.search(r"kTriTable\[16\] = \{(.*?)\};", text, re.S).group(1)
    rows = [[int(v) for v in m.group(1).split(",")] if m.group(1) else []
            for m in re.finditer(r"tri6\(([^)]*)\)|\b0\b", body)]        # tri6(...) entries, and the bare 0 of cases 0 and 15
    assert len(rows) == 16
    want = M.even_table()
    for case in range(16):
        assert rows[case] == [int(v) for v in want[case] if v >= 0], case


def test_ply_mesh_round_trip(tmp_path):
    from imfnet_amd.dataio import read_ply_mesh, read_ply_points, read_ply_points_numpy
    from imfnet_amd.fuse_fragments import write_ply_mesh
    units, tsdf, w = lattice(SURFACES["sphere_on_lattice"][0])
    r = M.mesh(units, tsdf, w, 0.01, 0.5)
    path = str(tmp_path / "mesh.ply")
    write_ply_mesh(path, r["vertices"], r["triangles"])
    assert not os.path.exists(path + ".tmp")
    v, t = read_ply_mesh(path)
    assert v.dtype == np.float64 and t.dtype == np.int32
    assert (v == r["vertices"].astype(np.float32).astype(np.float64)).all() and (t == r["triangles"]).all()
    head = open(path, "rb").read(400).split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    assert head[2:] == [f"element vertex {len(v)}", "property float x", "property float y", "property float z",
                        f"element face {len(t)}", "property list uchar int vertex_indices", ""]
    assert os.path.getsize(path) == len("\n".join(head)) + len("end_header\n") + 12 * len(v) + 13 * len(t)
    # the project's point readers take the vertices of a mesh file unchanged
    assert (read_ply_points(path) == v).all()
    assert (read_ply_points_numpy(path) == v).all()
    empty = str(tmp_path / "empty.ply")
    write_ply_mesh(empty, np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    v0, t0 = read_ply_mesh(empty)
    assert v0.shape == (0, 3) and t0.shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply_mesh(str(tmp_path / "bad.ply"), np.zeros((2, 3)), np.array([[0, 1, 2]], np.int32))


def test_fragment_listings_leave_mesh_files_out(tmp_path):
    """cloud_bin_K.mesh.ply (fuse_fragments --mesh) is a surface, not a fragment: the tools that list a sequence folder's
    fragments do not take it for one."""
    from imfnet_amd import compute_overlap, generate_desc
    folder = tmp_path / "scene-a" / "seq-01"
    folder.mkdir(parents=True)
    for name in ("cloud_bin_0.ply", "cloud_bin_1.ply", "cloud_bin_0.mesh.ply", "cloud_bin_1.mesh.ply"):
        (folder / name).write_bytes(b"")
    assert compute_overlap.list_fragments(str(folder)) == ["cloud_bin_0", "cloud_bin_1"]
    assert [os.path.basename(f) for _, f in generate_desc.list_fragments(str(tmp_path))] == ["cloud_bin_0.ply", "cloud_bin_1.ply"]
