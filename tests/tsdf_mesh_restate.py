"""NumPy restatement of the mesh extraction (csrc/tsdf_mesh.hip), written from the rule at the head of that file: marching
tetrahedra on the Kuhn split of every cell of the sparse TSDF volume.  Imports nothing from the library.

  valid   w != 0 and tsdf < 0.98;   inside  valid and tsdf < 0   (a stored 0 is outside)
  cell    (i, j, k) with the samples (i + bx, j + by, k + bz), corner b = bx + 2 by + 4 bz; it belongs to the unit of its
          corner 0; corners on the far faces come from the + neighbour units (missing unit: invalid); meshed = 8 valid
  tetrahedra   six per cell, one per permutation (a1, a2, a3) of the axes in lexicographic order, corners
          0, bit(a1), bit(a1) | bit(a2), 7
  edges   lo -> hi for every pair of corners with lo a proper subset of hi (12 axis edges, 6 face diagonals, the body
          diagonal); owned by the voxel at lo, slot e = 0..6 for the direction hi - lo = (1, 2, 4, 3, 5, 6, 7)[e]
  vertex  on an owned edge whose ends are valid, exactly one inside, and that lies in at least one meshed cell:
          t = |f_lo| / (|f_lo| + |f_hi|) in fp64, coordinate c = p_lo[c] + (voxel_length * t) where the direction has
          bit c, p_lo[c] elsewhere; p_lo = (16 unit + local + lattice_offset) * voxel_length
  triangles   per tetrahedron and case (CASES below), counter-clockwise seen from the outside (tsdf >= 0) side
  order   vertices (unit, voxel (z 16 + y) 16 + x, slot); triangles (unit, cell, tetrahedron, triangle); int32 indices
"""
import itertools

import numpy as np

RES = 16
DIRS = (1, 2, 4, 3, 5, 6, 7)                     # slot -> direction as a corner number
SLOT_OF = {d: e for e, d in enumerate(DIRS)}
PERMS = tuple(itertools.permutations(range(3)))  # lexicographic
TET_CORNERS = tuple((0, 1 << a[0], (1 << a[0]) | (1 << a[1]), 7) for a in PERMS)
LOCAL_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))     # local edge number -> local corners (lo, hi)
EDGE_NO = {e: i for i, e in enumerate(LOCAL_EDGES)}


def perm_parity(a):
    """0 for an even permutation, 1 for an odd one."""
    return sum(1 for i in range(3) for j in range(i + 1, 3) if a[i] > a[j]) & 1


def corner_xyz(b):
    return np.array([b & 1, (b >> 1) & 1, (b >> 2) & 1], np.float64)


def _edge(x, y):
    return EDGE_NO[(min(x, y), max(x, y))]


def unoriented_triangles(case):
    """The triangles of a case as local edge numbers, before orientation: `case` has bit i set when local corner i is
    inside.  1 inside a, outside b < c < d: (ab, ac, ad).  3 inside a < b < c, outside d: (ad, bd, cd).  2 inside a < b,
    outside c < d: the quad (ac, ad, bd, bc) as (ac, ad, bd) and (ac, bd, bc)."""
    ins = [i for i in range(4) if (case >> i) & 1]
    out = [i for i in range(4) if not (case >> i) & 1]
    if len(ins) == 1:
        a = ins[0]
        return [tuple(_edge(a, o) for o in out)]
    if len(ins) == 3:
        d = out[0]
        return [tuple(_edge(i, d) for i in ins)]
    if len(ins) == 2:
        (a, b), (c, d) = ins, out
        ac, ad, bd, bc = _edge(a, c), _edge(a, d), _edge(b, d), _edge(b, c)
        return [(ac, ad, bd), (ac, bd, bc)]
    return []


def generate_cases():
    """CASES[tetrahedron][case] = list of triangles, each three local edge numbers, oriented counter-clockwise seen from
    the outside: the vertices are placed at the edge midpoints of the real tetrahedron and a triangle whose normal points
    from the outside corners towards the inside ones gets its last two vertices swapped."""
    table = []
    for q in range(6):
        P = [corner_xyz(b) for b in TET_CORNERS[q]]
        mid = [0.5 * (P[lo] + P[hi]) for lo, hi in LOCAL_EDGES]
        row = []
        for case in range(16):
            ins = [i for i in range(4) if (case >> i) & 1]
            out = [i for i in range(4) if not (case >> i) & 1]
            tris = []
            for t in unoriented_triangles(case):
                outward = np.mean([P[i] for i in out], 0) - np.mean([P[i] for i in ins], 0)
                n = np.cross(mid[t[1]] - mid[t[0]], mid[t[2]] - mid[t[0]])
                s = float(n @ outward)
                assert s != 0.0
                tris.append(t if s > 0 else (t[0], t[2], t[1]))
            row.append(tris)
        table.append(row)
    return table


CASES = generate_cases()


def even_table():
    """The 16 x 6 table the HIP file carries: the cases of tetrahedron 0 (an even permutation), -1 where there is no
    triangle.  An odd tetrahedron swaps the last two vertices of each triangle (the host test checks that this is what
    generate_cases gives for all six)."""
    out = -np.ones((16, 6), np.int64)
    for case in range(16):
        flat = [e for t in CASES[0][case] for e in t]
        out[case, :len(flat)] = flat
    return out


def _tables():
    """CASE_OF[q, inside byte of the cell] -> case; TRI_LO / TRI_HI[q, case, triangle, vertex] -> cell corner numbers of
    the edge (or -1)."""
    case_of = np.zeros((6, 256), np.int64)
    lo = -np.ones((6, 16, 2, 3), np.int64)
    hi = -np.ones((6, 16, 2, 3), np.int64)
    for q in range(6):
        for byte in range(256):
            case_of[q, byte] = sum(1 << i for i in range(4) if (byte >> TET_CORNERS[q][i]) & 1)
        for case in range(16):
            for s, t in enumerate(CASES[q][case]):
                for k, e in enumerate(t):
                    lo[q, case, s, k] = TET_CORNERS[q][LOCAL_EDGES[e][0]]
                    hi[q, case, s, k] = TET_CORNERS[q][LOCAL_EDGES[e][1]]
    return case_of, lo, hi


CASE_OF, TRI_LO, TRI_HI = _tables()
CELL_EDGES = tuple((lo, hi) for lo in range(8) for hi in range(8) if lo != hi and (lo & hi) == lo)   # 19


def halo(units, tsdf, w):
    """(F float32 [n,17,17,17], V bool [n,17,17,17], nbr int64 [n,8]): every unit's samples with its far faces read from
    the + neighbour units; nbr[i, o] = row of the unit at offset o = ox + 2 oy + 4 oz, or -1."""
    n = len(units)
    row = {tuple(c): i for i, c in enumerate(np.asarray(units).tolist())}
    F = np.zeros((n, RES + 1, RES + 1, RES + 1), np.float32)
    V = np.zeros((n, RES + 1, RES + 1, RES + 1), bool)
    nbr = -np.ones((n, 8), np.int64)
    valid = (w != 0) & (tsdf < np.float32(0.98))
    sl = (slice(0, RES), slice(RES, RES + 1))               # destination, by offset bit
    src = (slice(0, RES), slice(0, 1))
    for i, (ux, uy, uz) in enumerate(np.asarray(units).tolist()):
        for o in range(8):
            ox, oy, oz = o & 1, (o >> 1) & 1, (o >> 2) & 1
            j = row.get((ux + ox, uy + oy, uz + oz))
            if j is None:
                continue
            nbr[i, o] = j
            F[i, sl[oz], sl[oy], sl[ox]] = tsdf[j, src[oz], src[oy], src[ox]]
            V[i, sl[oz], sl[oy], sl[ox]] = valid[j, src[oz], src[oy], src[ox]]
    return F, V, nbr


def _owner_key(iu, lz, ly, lx, lo, hi, nbr):
    """Vertex key (row of the owning unit * 4096 + voxel) * 7 + slot of the edge lo -> hi (cell corner numbers, arrays)
    of the cells (iu, lz, ly, lx)."""
    x, y, z = lx + (lo & 1), ly + ((lo >> 1) & 1), lz + ((lo >> 2) & 1)
    o = (x >> 4) | ((y >> 4) << 1) | ((z >> 4) << 2)
    owner = nbr[iu, o]
    assert (owner >= 0).all()
    voxel = ((z & 15) * RES + (y & 15)) * RES + (x & 15)
    slot = np.array([SLOT_OF.get(d, -1) for d in range(8)], np.int64)[hi - lo]
    return (owner * RES ** 3 + voxel) * 7 + slot


def mesh(units, tsdf, w, voxel_length, lattice_offset):
    """units int32 [n,3] ascending in (z, y, x), tsdf / w float32 [n,16,16,16] (z, y, x) ->
    dict(vertices float64 [V,3], triangles int32 [T,3], keys int64 [V] = (unit row * 4096 + voxel) * 7 + slot,
    ends float32 [V,2] = the tsdf at the two ends of every vertex's edge, cells int64 [T,4] = (unit row, lz, ly, lx) of
    every triangle, meshed bool [n,16,16,16])."""
    units = np.asarray(units)
    n = len(units)
    empty = dict(vertices=np.zeros((0, 3)), triangles=np.zeros((0, 3), np.int32), keys=np.zeros(0, np.int64),
                 ends=np.zeros((0, 2), np.float32), cells=np.zeros((0, 4), np.int64), meshed=np.zeros((n, RES, RES, RES), bool))
    if n == 0:
        return empty
    tsdf = np.asarray(tsdf, np.float32).reshape(n, RES, RES, RES)
    w = np.asarray(w, np.float32).reshape(n, RES, RES, RES)
    F, V, nbr = halo(units, tsdf, w)
    inside = V & (F < 0)
    meshed = np.ones((n, RES, RES, RES), bool)
    byte = np.zeros((n, RES, RES, RES), np.uint8)
    for b in range(8):
        s = tuple(slice(o, o + RES) for o in ((b >> 2) & 1, (b >> 1) & 1, b & 1))
        meshed &= V[(slice(None),) + s]
        byte |= inside[(slice(None),) + s].astype(np.uint8) << np.uint8(b)
    empty["meshed"] = meshed
    iu, lz, ly, lx = np.nonzero(meshed & (byte != 0) & (byte != 255))      # C order = (unit, cell)
    if len(iu) == 0:
        return empty
    by = byte[iu, lz, ly, lx].astype(np.int64)
    # the vertex set: every edge of a meshed cell with exactly one end inside
    keys = []
    for lo, hi in CELL_EDGES:
        m = ((by >> lo) & 1) != ((by >> hi) & 1)
        keys.append(_owner_key(iu[m], lz[m], ly[m], lx[m], np.int64(lo), np.int64(hi), nbr))
    keys = np.unique(np.concatenate(keys))
    if len(keys) > 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 vertices")
    # positions
    slot, rest = keys % 7, keys // 7
    vox, owner = rest % RES ** 3, rest // RES ** 3
    vx, vy, vz = vox % RES, (vox // RES) % RES, vox // (RES * RES)
    d = np.array(DIRS, np.int64)[slot]
    ends = np.stack([F[owner, vz, vy, vx], F[owner, vz + ((d >> 2) & 1), vy + ((d >> 1) & 1), vx + (d & 1)]], 1)
    f_lo, f_hi = ends[:, 0].astype(np.float64), ends[:, 1].astype(np.float64)
    t = np.abs(f_lo) / (np.abs(f_lo) + np.abs(f_hi))
    step = voxel_length * t
    g = np.stack([RES * units[owner, 0].astype(np.int64) + vx, RES * units[owner, 1].astype(np.int64) + vy,
                  RES * units[owner, 2].astype(np.int64) + vz], 1)
    p_lo = (g.astype(np.float64) + lattice_offset) * voxel_length
    verts = p_lo.copy()
    for c in range(3):
        has = ((d >> c) & 1) == 1
        verts[has, c] = p_lo[has, c] + step[has]
    # triangles, in (cell, tetrahedron, triangle) order
    case = np.stack([CASE_OF[q][by] for q in range(6)], 1)                 # [cells, 6]
    q = np.arange(6)[None, :]
    lo = TRI_LO[q, case]                                                   # [cells, 6, 2, 3]
    hi = TRI_HI[q, case]
    present = lo[..., 0] >= 0                                              # [cells, 6, 2]
    ci, qi, si = np.nonzero(present)
    tri = np.zeros((len(ci), 3), np.int64)
    for k in range(3):
        key = _owner_key(iu[ci], lz[ci], ly[ci], lx[ci], lo[ci, qi, si, k], hi[ci, qi, si, k], nbr)
        at = np.searchsorted(keys, key)
        assert (keys[at] == key).all()
        tri[:, k] = at
    cells = np.stack([iu[ci], lz[ci], ly[ci], lx[ci]], 1)
    return dict(vertices=verts, triangles=tri.astype(np.int32), keys=keys, ends=ends, cells=cells, meshed=meshed)


# ---- helpers of the tests: dense lattices as units, mesh topology -------------------------------------------------------

def lattice_units(values, valid):
    """A dense lattice values / valid [nz, ny, nx] (each a multiple of 16) as (units, tsdf, w) with w = 1 where valid."""
    nz, ny, nx = values.shape
    units, T, W = [], [], []
    for uz in range(nz // RES):
        for uy in range(ny // RES):
            for ux in range(nx // RES):
                s = (slice(uz * RES, (uz + 1) * RES), slice(uy * RES, (uy + 1) * RES), slice(ux * RES, (ux + 1) * RES))
                units.append((ux, uy, uz))
                T.append(values[s])
                W.append(valid[s])
    return np.array(units, np.int32), np.stack(T).astype(np.float32), np.stack(W).astype(np.float32)


def directed_edges(triangles):
    """int64 codes a * 2^32 + b of the three directed edges of every triangle, [T, 3]."""
    t = np.asarray(triangles, np.int64)
    return np.stack([t[:, 0] << 32 | t[:, 1], t[:, 1] << 32 | t[:, 2], t[:, 2] << 32 | t[:, 0]], 1)


def topology(n_vertices, triangles):
    """dict(V, E, F, chi, closed: every directed edge once and its reverse once, unpaired: [triangle, edge] of the
    directed edges without a reverse, repeated: directed edges that occur more than once, unreferenced vertices)."""
    t = np.asarray(triangles, np.int64)
    e = directed_edges(t)
    flat = e.ravel()
    uniq, cnt = np.unique(flat, return_counts=True)
    rev = (flat & 0xFFFFFFFF) << 32 | (flat >> 32)
    has_rev = np.isin(rev, uniq)
    und = np.unique(np.minimum(flat, rev))
    used = np.zeros(n_vertices, bool)
    used[t.ravel()] = True
    return dict(V=int(n_vertices), E=int(len(und)), F=int(len(t)), chi=int(n_vertices - len(und) + len(t)),
                repeated=int((cnt > 1).sum()), unpaired=np.argwhere(~has_rev.reshape(e.shape)),
                closed=bool((cnt == 1).all() and has_rev.all()), unreferenced=int((~used).sum()))


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)
