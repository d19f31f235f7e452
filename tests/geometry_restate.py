"""The integer front end restated in plain NumPy, and the catalogue of adversarial coordinate sets its tests run on
(tests/test_geometry_host.py on the CPU against oracle/imf_oracle.py and the C twins; tests/test_gpu_geometry_exact.py against
csrc/geometry.hip, rulebook_tile.h and common.h through the public path).

Rows are int64 `(b, x, y, z)`.  Nothing here packs 18 bits per axis: rows are looked up per batch item by a WIDE key (21 bits per
axis after adding 2^20), so the restatement stays correct at and beyond +-2^17, where the library's keys would alias.

THE CONTRACT at the edge of the coordinate range: a voxel exists only inside [-2^17, 2^17) on every axis (a point outside raises
the range error), and a neighbour that would lie outside that range DOES NOT EXIST -- its map entry is -1, whatever voxel sits at
the coordinate the 18-bit key would wrap onto.

    voxelize        rows in first-occurrence order of floor(xyz / voxel) in float64, and the first point of every row
    strided         floor(c / stride) * stride, distinct rows in first-occurrence order
    conv_map        nbr[o, k] = row of `in` at out[o] + off_k * ts_in           (k3 and k5 at stride 1, k3 at stride 2)
    transpose_map   nbr[f, k] = row of `coarse` at fine[f] - off_k * ts_fine    (the stride-2 map with in / out swapped, same k)
    transpose_slots the library's slot order of a transposed map: fine rows grouped by the parity of coord / ts per axis, every
                    class padded to whole 64-slot tiles, rows ascending within a class, an empty class takes no tile
    item_starts, bbox
    off_k = (k % K - r, (k / K) % K - r, k / K^2 - r): x fastest.

The cases (CASES / case(name)) are deterministic: each is a set of voxel coordinates plus a shuffled point list with 1 to 6 points
per voxel at (c + f) * vs, f in {0, 1/4, 1/2, 3/4} per axis, vs a power of two -- so the float64 quotient and its floor are exact
by construction (asserted)."""
import functools
import itertools

import numpy as np

LIM = 1 << 17                    # coordinates live in [-LIM, LIM)
TILE = 64
MAX_BATCH = 8
VS = 2.0 ** -5                   # the catalogue's voxel size (a power of two)
_W, _OFF = 21, 1 << 20


class CoordinateRangeError(ValueError):
    """A point falls outside [-2^17, 2^17) voxels."""


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


# ------------------------------------------------------------------------------------------------ the restatement
def _wide(xyz):
    q = np.asarray(xyz, np.int64) + _OFF
    assert ((q >= 0) & (q < (1 << _W))).all(), "coordinate beyond the wide key"
    return (q[:, 0] << (2 * _W)) | (q[:, 1] << _W) | q[:, 2]


def first_occurrence(rows4):
    """Indices of the first occurrence of every distinct (b, x, y, z) row, ascending."""
    rows4 = np.asarray(rows4, np.int64)
    first = []
    for item in np.unique(rows4[:, 0]):
        idx = np.flatnonzero(rows4[:, 0] == item)
        _, f = np.unique(_wide(rows4[idx, 1:]), return_index=True)
        first.append(idx[f])
    return np.sort(np.concatenate(first))


def quantize(points, vs):
    """floor(xyz / vs) in float64 as int64; CoordinateRangeError outside [-2^17, 2^17)."""
    f = np.floor(np.asarray(points, np.float64) / vs)
    if not ((f >= -LIM) & (f < LIM)).all():
        raise CoordinateRangeError("a point lies outside [-2^17, 2^17) voxels")
    return f.astype(np.int64)


def voxelize(points, vs, batch_index=0, item_starts=None):
    """(rows int64 [M, 4], first point int64 [M]).  item_starts: first point of every item of a batch (items 0 .. B-1)."""
    c = quantize(points, vs)
    if item_starts is None:
        b = np.full(len(c), batch_index, np.int64)
    else:
        b = np.searchsorted(np.asarray(item_starts, np.int64), np.arange(len(c)), side="right") - 1
    rows = np.concatenate([b[:, None], c], 1)
    first = first_occurrence(rows)
    return rows[first], first


def strided(rows4, stride):
    q = np.array(rows4, np.int64)
    q[:, 1:] = (q[:, 1:] // stride) * stride            # NumPy's // floors
    return q[first_occurrence(q)]


def kernel_offsets(ksize):
    r = ksize // 2
    return np.array([(k % ksize - r, (k // ksize) % ksize - r, k // (ksize * ksize) - r) for k in range(ksize ** 3)], np.int64)


class Index:
    """row of a coordinate, per batch item; -1 for an absent or out-of-range coordinate"""

    def __init__(self, rows4):
        rows4 = np.asarray(rows4, np.int64)
        self.tabs = {}
        for item in np.unique(rows4[:, 0]):
            idx = np.flatnonzero(rows4[:, 0] == item)
            k = _wide(rows4[idx, 1:])
            o = np.argsort(k, kind="stable")
            self.tabs[int(item)] = (k[o], idx[o])

    def find(self, b, xyz):
        out = np.full(len(b), -1, np.int32)
        ok = ((xyz >= -LIM) & (xyz < LIM)).all(1)        # the contract: nothing exists outside the range
        for item, (sk, rows) in self.tabs.items():
            sel = np.flatnonzero(ok & (b == item))
            if len(sel) == 0:
                continue
            q = _wide(xyz[sel])
            pos = np.minimum(np.searchsorted(sk, q), len(sk) - 1)
            hit = sk[pos] == q
            out[sel[hit]] = rows[pos[hit]]
        return out


def _probe_map(in_rows, out_rows, step, ksize, index=None):
    """nbr[o, k] = index.find(b[o], out[o] + off_k * step) for every offset.  Written per item over the output rows sorted by
    their wide key: adding an offset is adding a constant to the key (no axis can carry: 21 bits hold +-2^17 plus any offset),
    so the sorted order survives and every lookup is a merge of two sorted lists."""
    index = index or Index(in_rows)
    out_rows = np.asarray(out_rows, np.int64)
    offs = kernel_offsets(ksize) * step
    nbr = np.full((len(out_rows), len(offs)), -1, np.int32)
    for item, (sk, rows) in index.tabs.items():
        sel = np.flatnonzero(out_rows[:, 0] == item)
        if len(sel) == 0:
            continue
        xyz = out_rows[sel, 1:]
        key = _wide(xyz)
        order = np.argsort(key, kind="stable")
        sel, xyz, key = sel[order], xyz[order], key[order]
        lo, hi = xyz.min(0), xyz.max(0)
        for k, o in enumerate(offs):
            q = key + ((int(o[0]) << (2 * _W)) + (int(o[1]) << _W) + int(o[2]))
            pos = np.minimum(np.searchsorted(sk, q), len(sk) - 1)
            hit = sk[pos] == q
            if ((lo + o) < -LIM).any() or ((hi + o) >= LIM).any():       # the contract: nothing exists outside the range
                p = xyz + o
                hit &= ((p >= -LIM) & (p < LIM)).all(1)
            nbr[sel[hit], k] = rows[pos[hit]]
    return nbr


def conv_map(in_rows, out_rows, ts_in, ksize, index=None):
    return _probe_map(in_rows, out_rows, ts_in, ksize, index)


def transpose_map(coarse_rows, fine_rows, ts_fine, ksize=3, index=None):
    return _probe_map(coarse_rows, fine_rows, -ts_fine, ksize, index)


def parity_class(rows4, ts):
    q = (np.asarray(rows4, np.int64)[:, 1:] // ts) & 1
    return q[:, 0] | (q[:, 1] << 1) | (q[:, 2] << 2)


def transpose_slot_count(n_fine):
    return ((n_fine + TILE - 1) // TILE + 8) * TILE


def transpose_slots(fine_rows, ts_fine, n_slots=None):
    p = parity_class(fine_rows, ts_fine)
    rows = np.full(transpose_slot_count(len(p)) if n_slots is None else n_slots, -1, np.int32)
    base = 0
    for q in range(8):
        idx = np.flatnonzero(p == q)
        rows[base:base + len(idx)] = idx
        base += (len(idx) + TILE - 1) // TILE * TILE
    return rows


def item_starts(rows4, n_items):
    b = np.asarray(rows4)[:, 0]
    return [int(np.flatnonzero(b == i)[0]) if (b == i).any() else -1 for i in range(n_items)]


def bbox(rows4):
    r = np.asarray(rows4, np.int64)
    return r.min(0).tolist() + r.max(0).tolist()


class Geometry:
    """Four levels and the eight kinds of map the network uses, from level-0 rows."""

    def __init__(self, rows4, conv1_kernel_size=5):
        self.levels = [np.asarray(rows4, np.int64)]
        for l in range(3):
            self.levels.append(strided(self.levels[-1], 2 << l))
        L = self.levels
        ix = [Index(r) for r in L]
        self.k_first = conv_map(L[0], L[0], 1, conv1_kernel_size, ix[0])
        self.k3 = [conv_map(L[i], L[i], 1 << i, 3, ix[i]) for i in range(4)]
        self.down = [conv_map(L[i], L[i + 1], 1 << i, 3, ix[i]) for i in range(3)]
        self.up = [transpose_map(L[i + 1], L[i], 1 << i, 3, ix[i + 1]) for i in range(3)]
        self.up_rows = [transpose_slots(L[i], 1 << i) for i in range(3)]


def shifted_items(g1, n_items):
    """The maps of `n_items` copies of one item (rows of item b = the single item's rows + b * the level's row count): what a
    batched build of identical items must produce.  Returns a Geometry-shaped namespace."""
    class G:
        pass
    g = G()
    n = [len(l) for l in g1.levels]
    g.levels = []
    for l in g1.levels:
        rows = np.tile(l, (n_items, 1))
        rows[:, 0] = np.repeat(np.arange(n_items), len(l))
        g.levels.append(rows)

    def rep(nbr, n_in):
        return np.concatenate([np.where(nbr >= 0, nbr + b * n_in, -1) for b in range(n_items)], 0).astype(np.int32)
    g.k_first = rep(g1.k_first, n[0])
    g.k3 = [rep(g1.k3[i], n[i]) for i in range(4)]
    g.down = [rep(g1.down[i], n[i]) for i in range(3)]
    g.up = [rep(g1.up[i], n[i + 1]) for i in range(3)]
    g.up_rows = [transpose_slots(g.levels[i], 1 << i) for i in range(3)]
    g.starts = [[b * m for b in range(n_items)] for m in n]
    return g


def first_conv_expected(nbr, kernel):
    """conv1 of the all-ones feature with an integer kernel [kvol, 1, cout]: per row, the sum of the kernel rows of the occupied
    offsets (int64)."""
    return (np.asarray(nbr) >= 0).astype(np.int64) @ np.asarray(kernel, np.float64)[:, 0, :].astype(np.int64)


def int_kernel(ksize, cout):
    """Small integers, every offset's row distinct: channel 0 = k + 1, channel c = ((k + 1) * (c + 2)) mod 17 - 8."""
    k = np.arange(ksize ** 3, dtype=np.int64)[:, None] + 1
    c = np.arange(cout, dtype=np.int64)[None, :]
    w = (k * (c + 2)) % 17 - 8
    w[:, 0] = k[:, 0]
    return w[:, None, :].astype(np.float32)


# ------------------------------------------------------------------------------------------------ checking a tiled map
def check_rulebook(rb, nbr_ref, identity_rows):
    """A tiled map (tile_rows [n_slots], nbr [kvol, n_slots], tile_mask [tiles, 4]) against nbr_ref [n_out, kvol]."""
    n_out, kvol = nbr_ref.shape
    rows = _np(rb.tile_rows)
    nbr = _np(rb.nbr).reshape(kvol, rb.n_slots)
    valid = rows >= 0
    assert sorted(rows[valid].tolist()) == list(range(n_out))
    if identity_rows:
        assert (rows[:n_out] == np.arange(n_out)).all()
    assert (nbr[:, valid].T == nbr_ref[rows[valid]]).all()
    assert (nbr[:, ~valid] == -1).all()
    mask = _np(rb.tile_mask).view(np.uint32).reshape(-1, 4)
    act = (nbr.reshape(kvol, -1, 64) >= 0).any(axis=2)                   # [kvol, tiles]
    for k in range(kvol):
        assert (((mask[:, k // 32] >> (k % 32)) & 1).astype(bool) == act[k]).all()
    return mask


def check_transposed(rb, nbr_ref, rows_ref):
    """check_rulebook plus the transposed map's own structure: the slot order is exactly the parity-class layout (tile-aligned
    runs, rows ascending within a class, nothing for an empty class) and no tile has more than 8 active offsets."""
    mask = check_rulebook(rb, nbr_ref, False)
    rows = _np(rb.tile_rows)
    assert np.array_equal(rows, rows_ref)
    pop = np.array([bin(int(w)).count("1") for w in mask.reshape(-1)]).reshape(-1, 4).sum(1)
    assert pop.max() <= 8
    return mask


def first_difference(nbr, nbr_ref, rows4, ksize=3):
    """Where two maps [n_out, kvol] first differ: (row, its coordinates, k, offset, got, expected) -- names the code path."""
    d = np.argwhere(np.asarray(nbr) != np.asarray(nbr_ref))
    if len(d) == 0:
        return None
    o, k = d[0]
    return int(o), np.asarray(rows4)[o].tolist(), int(k), kernel_offsets(ksize)[k].tolist(), int(nbr[o, k]), int(nbr_ref[o, k])


# ------------------------------------------------------------------------------------------------ hash statistics
# Only for the `chains` cases' self-check (how long the probe sequences of the library's table get): the published slot formula of
# csrc/common.h.  No map, level or row order above depends on it.
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _hash64(k):
    k = np.uint64(k)
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k = (k * np.uint64(0xff51afd7ed558ccd)) & _M64
        k ^= k >> np.uint64(33)
        k = (k * np.uint64(0xc4ceb9fe1a85ec53)) & _M64
        k ^= k >> np.uint64(33)
    return int(k) & 0xFFFFFFFF


def _key18(b, x, y, z):
    return (b << 54) | ((x & 0x3FFFF) << 36) | ((y & 0x3FFFF) << 18) | (z & 0x3FFFF)


def _hash_slot(key, shift, capmask):
    low = (3 << shift) * (1 | (1 << 18) | (1 << 36))
    local = (((key >> (36 + shift)) & 3) << 4) | (((key >> (18 + shift)) & 3) << 2) | ((key >> shift) & 3)
    return (((_hash64(key & ~low & 0xFFFFFFFFFFFFFFFF) << 6) & 0xFFFFFFFF) + local) & capmask


def predicted_chains(rows4, shift, capacity):
    """Probes each key of `rows4` needs when the rows are inserted one after the other into an empty table of `capacity` slots
    (first slot: hash_slot at `shift`; then the key's odd stride).  Returns (probes per key, local indices)."""
    capmask, used, probes, local = capacity - 1, set(), [], []
    for b, x, y, z in np.asarray(rows4, np.int64).tolist():
        key = _key18(b, x, y, z)
        s = _hash_slot(key, shift, capmask)
        local.append(s & 63)
        step, n = (_hash64(key) >> 3) | 1, 1
        while s in used:
            s, n = (s + step) & capmask, n + 1
        used.add(s)
        probes.append(n)
    return np.array(probes), np.array(local)


# ------------------------------------------------------------------------------------------------ the case catalogue
class Case:
    """coords int64 [V, 3]: the voxel set; points float64 [N, 3]: 1 .. 6 points per voxel, shuffled; voxel_of [N]."""

    def __init__(self, name, coords, seed, batch_index=0, n_items=1, counts=(1, 6), extra_points=0):
        coords = np.unique(np.asarray(coords, np.int64), axis=0)
        assert ((coords >= -LIM) & (coords < LIM)).all()
        rng = np.random.default_rng(seed)
        coords = coords[rng.permutation(len(coords))]
        per = rng.integers(counts[0], counts[1] + 1, len(coords))
        vox = np.repeat(np.arange(len(coords)), per)
        if extra_points:
            vox = np.concatenate([vox, rng.integers(0, len(coords), extra_points)])
        vox = vox[rng.permutation(len(vox))]
        frac = rng.integers(0, 4, (len(vox), 3)) * 0.25
        points = (coords[vox] + frac) * VS
        # exact by construction: c + f has at most 20 significant bits, vs is a power of two
        assert (points / VS == coords[vox] + frac).all() and (np.floor(points / VS) == coords[vox]).all()
        self.name, self.coords, self.points, self.voxel_of, self.vs = name, coords, points, vox, VS
        self.batch_index, self.n_items = batch_index, n_items

    @property
    def n_points(self):
        return len(self.points)

    def dup_span(self):
        """Largest distance, in points, between two points of one voxel."""
        i = np.arange(len(self.voxel_of))
        lo = np.full(len(self.coords), len(i))
        hi = np.zeros(len(self.coords), np.int64)
        np.minimum.at(lo, self.voxel_of, i)
        np.maximum.at(hi, self.voxel_of, i)
        return int((hi - lo).max())

    def batched_points(self):
        """The points of all items back to back (every item = the same points) and the first point of each item."""
        return np.tile(self.points, (self.n_items, 1)), [b * len(self.points) for b in range(self.n_items)]

    def rows(self):
        """Level-0 rows and first indices as the restatement computes them from the POINTS (single item)."""
        return voxelize(self.points, self.vs, self.batch_index)


def _box(lo, hi):
    r = [np.arange(a, b) for a, b in zip(lo, hi)]
    return np.stack(np.meshgrid(*r, indexing="ij"), -1).reshape(-1, 3)


def _shell(centre, radius):
    c = _box([-radius - 1] * 3, [radius + 2] * 3)
    d = np.sqrt((c * c).sum(1))
    return c[(d >= radius - 0.5) & (d < radius + 0.5)] + np.asarray(centre, np.int64)


def _faces_coords():
    S, vox = 12, []
    wins = [(-6, -6), (-LIM, -6), (LIM - S, 40), (1000, LIM - S)]
    for a in range(3):
        u_ax, v_ax = [i for i in range(3) if i != a]
        for u0, v0 in wins:
            u, v = np.meshgrid(np.arange(u0, u0 + S), np.arange(v0, v0 + S), indexing="ij")
            for t in (-LIM, -LIM + 1, LIM - 2, LIM - 1):               # two voxels thick, the same window on BOTH faces
                c = np.empty((S * S, 3), np.int64)
                c[:, a], c[:, u_ax], c[:, v_ax] = t, u.ravel(), v.ravel()
                vox.append(c)
    for s in itertools.product((0, 1), repeat=3):                      # the eight corners, 6^3 each
        lo = [LIM - 6 if q else -LIM for q in s]
        vox.append(_box(lo, [l + 6 for l in lo]))
    return np.concatenate(vox)


def wrap18(xyz):
    """The coordinate an 18-bit key would alias an out-of-range coordinate onto."""
    return ((np.asarray(xyz, np.int64) + LIM) % (2 * LIM)) - LIM


def aliased_probes(in_rows, out_rows, step, ksize):
    """Per offset k: how many probes out + off_k * step leave the range AND would, wrapped to 18 bits, hit an occupied voxel of
    `in_rows` -- every one of them is a wrong neighbour if the range check were missing."""
    ix, out_rows = Index(in_rows), np.asarray(out_rows, np.int64)
    cnt = []
    for o in kernel_offsets(ksize) * step:
        q = out_rows[:, 1:] + o
        outside = ~((q >= -LIM) & (q < LIM)).all(1)
        cnt.append(int((ix.find(out_rows[outside, 0], wrap18(q[outside])) >= 0).sum()))
    return np.array(cnt)


def faces_alias_report(rows4):
    """{map name: aliased probes per offset} over all the maps of the network, from level-0 rows."""
    L = [np.asarray(rows4, np.int64)]
    for l in range(3):
        L.append(strided(L[-1], 2 << l))
    rep = {"k5@1": aliased_probes(L[0], L[0], 1, 5)}
    for i in range(4):
        rep[f"k3@{1 << i}"] = aliased_probes(L[i], L[i], 1 << i, 3)
    for i in range(3):
        rep[f"down{1 << i}"] = aliased_probes(L[i], L[i + 1], 1 << i, 3)
        rep[f"up{1 << i}"] = aliased_probes(L[i + 1], L[i], -(1 << i), 3)
    return rep


AXIS_K3 = (12, 14, 10, 16, 4, 22)            # the six axis-aligned offsets of the 3x3x3 kernel: -x +x -y +y -z +z


def _faces():
    c = Case("faces", _faces_coords(), 3)
    rows = np.concatenate([np.zeros((len(c.coords), 1), np.int64), c.coords], 1)
    rep = faces_alias_report(rows)
    for i in range(4):                        # every stride: a wrapped probe in each of the six directions hits a real voxel
        assert (rep[f"k3@{1 << i}"][list(AXIS_K3)] > 0).all(), (i, rep[f"k3@{1 << i}"])
    k5 = rep["k5@1"].reshape(5, 5, 5)         # [dz, dy, dx]
    assert all(k5[2, 2, j] > 0 for j in (0, 1, 3, 4)) and all(k5[2, j, 2] > 0 for j in (0, 1, 3, 4)) and \
        all(k5[j, 2, 2] > 0 for j in (0, 1, 3, 4))
    for i in range(3):
        assert rep[f"down{1 << i}"].sum() > 0 and rep[f"up{1 << i}"].sum() > 0
    return c


def _chains(shift):
    """<= 512 voxels (and <= 512 points: the 1 024-slot minimum table at every level) at multiples of 4 * 2^shift: all in distinct
    4x4x4 blocks of level `shift`, all with local index 0 -- 16 possible first slots for hundreds of keys."""
    ts = 1 << shift
    grid = (_box([0] * 3, [10] * 3) - 5) * (4 * ts)
    # After its first slot a key walks on with its own odd stride, so at the table's load of <= 1/2 a chain is a geometric
    # tail, not the whole window's population: the longest of ~500 is 6 to 10 probes.  The selection is the first of the
    # seeded draws whose predicted longest chain reaches 8, so the case cannot silently stop being a stress.
    for draw in range(64):
        rng = np.random.default_rng(100 * draw + shift)
        c = Case(f"chains{shift}", grid[rng.permutation(len(grid))[:480]], 40 + shift, counts=(1, 1), extra_points=32)
        rows, _ = c.rows()
        probes, local = predicted_chains(rows, shift, 1024)
        if probes.max() >= 8:
            break
    assert c.n_points <= 512 and len(c.coords) <= 512 and (c.coords % (4 * ts) == 0).all()
    assert (local == 0).all() and probes.max() >= 8, probes.max()
    c.predicted_probes = probes
    return c


def _small_blob(n):
    return _box([-2, -1, -3], [3, 4, 0])[:n] if n <= 75 else None      # 5 x 5 x 3 block around the origin


def _lines():
    x = np.array([(i, 0, 0) for i in range(-3, 4)])                    # 7 along x
    y = np.array([(20, j, 5) for j in range(4)])                       # 4 along y
    z = np.array([(-20, 7, k) for k in (-1, 0)])                       # 2 along z
    ell = np.array([(40, 0, 0), (41, 0, 0), (42, 0, 0), (42, 1, 0), (42, 1, 1)])
    return np.concatenate([x, y, z, ell])


def _large():
    occ = np.random.default_rng(9).random((256, 256, 256)) < 0.0635
    c = Case("large", np.argwhere(occ) - 128, 10)
    assert len(c.coords) >= 10 ** 6 and 2 * c.n_points >= (1 << 21)    # >= 10^6 voxels, a table of >= 2^21 slots
    return c


_B16 = _box([-8] * 3, [8] * 3)
_BUILDERS = {
    "solid": lambda: Case("solid", _box([-20] * 3, [20] * 3), 1),
    "far_negative": lambda: Case("far_negative", _shell([-130000, -130003, -129998], 60), 2),
    "faces": _faces,
    "corner_lo": lambda: Case("corner_lo", _box([-LIM] * 3, [-LIM + 6] * 3), 4),
    "corner_hi": lambda: Case("corner_hi", _box([LIM - 6] * 3, [LIM] * 3), 5),
    "even": lambda: Case("even", 2 * _B16, 11),
    "odd": lambda: Case("odd", 2 * _B16 + 1, 12),
    "spacing3": lambda: Case("spacing3", 3 * _box([-7] * 3, [7] * 3), 13),
    "parity101": lambda: Case("parity101", 2 * _B16 + np.array([1, 0, 1]), 14),            # one parity class at stride 1
    "parity_ts2": lambda: Case("parity_ts2", np.concatenate(                               # ... and one at stride 2
        [4 * _box([-5] * 3, [5] * 3) + np.array([2 + i, j, 2 + k]) for i, j, k in itertools.product((0, 1), repeat=3)]), 15),
    "chains0": lambda: _chains(0), "chains1": lambda: _chains(1), "chains2": lambda: _chains(2), "chains3": lambda: _chains(3),
    "one": lambda: Case("one", [(-7, 3, 100)], 20),
    "two": lambda: Case("two", [(-7, 3, 100), (9, 3, 100)], 21),
    "n63": lambda: Case("n63", _small_blob(63), 22),
    "n64": lambda: Case("n64", _small_blob(64), 23),
    "n65": lambda: Case("n65", _small_blob(65), 24),
    "lines": lambda: Case("lines", _lines(), 25),
    "large": _large,
    "batched2": lambda: Case("batched2", _shell([-3, 2, 5], 9), 30, n_items=2),
    "batched8": lambda: Case("batched8", _shell([-3, 2, 5], 9), 30, n_items=MAX_BATCH),
    "batch511": lambda: Case("batch511", _shell([-3, 2, 5], 9), 30, batch_index=511),
}
CASES = tuple(_BUILDERS)
LATTICES = ("even", "odd", "spacing3", "parity101", "parity_ts2")
CHAINS = ("chains0", "chains1", "chains2", "chains3")
SMALL = ("one", "two", "n63", "n64", "n65", "lines")
BATCHED = ("batched2", "batched8")


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=4)
def geometry(name):
    """The restated Geometry of a case (single item, the case's batch index), cached: (rows, first, Geometry)."""
    rows, first = case(name).rows()
    return rows, first, Geometry(rows)


def just_outside():
    """Two point lists, each a few hundred valid points with ONE point one voxel beyond the range: at voxel 2^17 on x, and at
    -2^17 - 1 on y.  (The last voxels inside, 2^17 - 1 and -2^17, are in `faces`.)"""
    base = case("batch511").points
    out = []
    for voxel in ((LIM, 0, 0), (0, -LIM - 1, 0)):
        p = base.copy()
        p[len(p) // 2] = (np.array(voxel, np.float64) + 0.5) * VS
        assert np.floor(p[len(p) // 2] / VS).tolist() == list(voxel)
        out.append(p)
    return out
