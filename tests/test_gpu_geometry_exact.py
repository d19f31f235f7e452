"""The integer front end on adversarial coordinates (-m gpu): csrc/geometry.hip, rulebook_tile.h and the hash of common.h
against the restatement of tests/geometry_restate.py, on its whole case catalogue, through the public path (ops.voxelize /
pyramid_from_points, CoordinateManager.build_pyramid(8), conv_rulebook, transpose_rulebook; batches through the batched build the
pair forward and the trainer use; capacity mode through imf_pyramid_build_dyn / imf_rulebook_*_dyn).  Every comparison is
array_equal: there is no tolerance in this file.  Every case is built twice and the two builds must be the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from imfnet_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _expected(name):
    """(level-0 rows, first indices, maps, item start rows per level) the build of a case must produce."""
    c = R.case(name)
    if c.n_items == 1:
        rows, first, g = R.geometry(name)
        return rows, first, g, [[0]] * 4
    rows1, first1, g1 = R.geometry("batch511")             # the same voxel set and points as ONE item
    g = R.shifted_items(g1, c.n_items)                     # every item = the single item's maps shifted by its first row
    first = np.concatenate([first1 + b * c.n_points for b in range(c.n_items)])
    return g.levels[0], first, g, g.starts


def _build(ops, name):
    """The arena build (one library call for the four levels): levels and their CoordinateManager."""
    from imfnet_amd import sparse as ME
    c = R.case(name)
    if c.n_items > 1:
        pts, starts = c.batched_points()
        xyz = torch.as_tensor(pts).to(DEV)
        levels = ops.PyramidFuture(xyz, c.vs, 4, 0, inputs_ready=False, item_starts=starts).result()
    else:
        levels = ops.pyramid_from_points(torch.as_tensor(c.points).to(DEV), c.vs, 4, batch_index=c.batch_index)
    return levels, ME.CoordinateManager.from_levels(levels)


def _build_stepwise(ops, name):
    """ops.voxelize, then CoordinateManager.build_pyramid(8): one table and one launch sequence per level."""
    from imfnet_amd import sparse as ME
    c = R.case(name)
    cm = ME.CoordinateManager(ops.voxelize(torch.as_tensor(c.points).to(DEV), c.vs, batch_index=c.batch_index))
    cm.build_pyramid(8)
    return [cm.level(ts) for ts in (1, 2, 4, 8)], cm


def _maps(cm):
    """Every map of the network, in a fixed order: [(kind, index, Rulebook)]."""
    out = [("k5", 0, cm.conv_rulebook(1, 5, 1))]
    out += [("k3", i, cm.conv_rulebook(1 << i, 3, 1)) for i in range(4)]
    out += [("down", i, cm.conv_rulebook(1 << i, 3, 2)) for i in range(3)]
    out += [("up", i, cm.transpose_rulebook(2 << i, 3, 2)) for i in range(3)]
    return out


def _check_levels(levels, rows, first, g):
    for i in range(4):
        assert levels[i].n == len(g.levels[i]), f"level {i}: {levels[i].n} rows, expected {len(g.levels[i])}"
        assert np.array_equal(levels[i].coords.cpu().numpy(), g.levels[i]), f"level {i}"
    assert np.array_equal(levels[0].first_idx.cpu().numpy(), first)


def _check_maps(cm, g):
    for kind, i, rb in _maps(cm):
        if kind == "up":
            R.check_transposed(rb, g.up[i], g.up_rows[i])
        else:
            R.check_rulebook(rb, {"k5": [g.k_first], "k3": g.k3, "down": g.down}[kind][i], True)


def _same_bits(a, b):
    (la, cma), (lb, cmb) = a, b
    for x, y in zip(la, lb):
        assert x.n == y.n and torch.equal(x.coords, y.coords)
    assert torch.equal(la[0].first_idx, lb[0].first_idx)
    for (kind, i, p), (_, _, q) in zip(_maps(cma), _maps(cmb)):
        assert torch.equal(p.tile_rows, q.tile_rows) and torch.equal(p.nbr, q.nbr) and torch.equal(p.tile_mask, q.tile_mask), (kind, i)


# ------------------------------------------------------------------------------------------------ levels and maps, every case
@pytest.mark.parametrize("name", R.CASES)
def test_levels_and_maps_are_exact(ops, name):
    c = R.case(name)
    rows, first, g, starts = _expected(name)
    levels, cm = _build(ops, name)
    _check_levels(levels, rows, first, g)
    assert list(levels[0].bbox) == R.bbox(rows)                                  # the meta block's level-0 bounding box
    for i in range(4):                                                           # per-item start rows at every level
        assert [s for s, _ in levels[i].items] == starts[i]
        if c.n_items > 1:
            assert starts[i] == R.item_starts(g.levels[i], c.n_items)
        assert sum(n for _, n in levels[i].items) == levels[i].n
    _check_maps(cm, g)
    _same_bits((levels, cm), _build(ops, name))                                  # determinism: a second build, the same bits
    if c.n_items == 1:                                                           # the level-by-level path of the public API
        lv2, cm2 = _build_stepwise(ops, name)
        _check_levels(lv2, rows, first, g)
        if name != "large":
            _check_maps(cm2, g)
            _same_bits((lv2, cm2), _build_stepwise(ops, name))


# ------------------------------------------------------------------------------------------------ conv1's occupancy bit grid
@pytest.mark.parametrize("ks", [3, 5])
@pytest.mark.parametrize("name", ("solid", "faces", "corner_lo", "corner_hi") + R.LATTICES + R.SMALL)
def test_first_conv_counts_exactly_the_occupied_offsets(ops, name, ks):
    """conv_first_bitgrid and conv_first_fused on the all-ones input with an integer kernel: every output is a small integer,
    the sum of the kernel rows of the occupied offsets -- exact in any summation order.  Pins the grid's origin (the bounding
    box's minimum), the five-bit windows at the box's edges and both kernel sizes.  `faces` spans the whole coordinate range:
    its box exceeds the grid limit, conv_first_bitgrid must decline (None) and the hash-probing twin carries the case."""
    rows, first, g, _ = _expected(name)
    levels, _ = _build(ops, name)
    w = R.int_kernel(ks, 32)
    want = R.first_conv_expected(g.k_first if ks == 5 else g.k3[0], w).astype(np.float32)
    wt = torch.as_tensor(w).to(DEV)
    fused = ops.conv_first_fused(levels[0], None, wt, ks)
    assert np.array_equal(fused.cpu().numpy(), want)
    ones = torch.ones(levels[0].n, 1, device=DEV)
    assert np.array_equal(ops.conv_first_fused(levels[0], ones, wt, ks).cpu().numpy(), want)
    bits = ops.conv_first_bitgrid(levels[0], wt, ks)
    if name == "faces":
        assert bits is None
    else:
        assert bits is not None and np.array_equal(bits.cpu().numpy(), want)


class _BitGrid:
    """conv1's public bit-grid entry points called straight through the C ABI on the level-0 rows of a case."""
    SENTINEL = -12345.0

    def __init__(self, ops, name, ks, cout, kernel_scale=1.0):
        from imfnet_amd import _lib
        self.lib, self.L, self.ks, self.cout = _lib, _lib.lib(), ks, cout
        rows, _, g, _ = _expected(name)
        self.levels, _ = _build(ops, name)                       # (kept: the arena owns the coordinate rows)
        self.coords, self.n = self.levels[0].coords.contiguous(), self.levels[0].n      # int32 [n, 4]
        w = R.int_kernel(ks, cout) * np.float32(kernel_scale)
        self.want = R.first_conv_expected(g.k_first if ks == 5 else g.k3[0], w).astype(np.float32)
        self.w = torch.as_tensor(w).to(DEV)
        self.bbox = [int(v) for v in self.levels[0].bbox]
        assert self.coords.shape == (len(rows), 4) and self.bbox == R.bbox(rows)
        self.box = (C.c_int32 * 8)(*self.bbox)
        self.words = int(self.L.imf_bitgrid_words(self.box, ks))
        assert self.words > 0
        self.st = torch.cuda.current_stream().cuda_stream

    def _grid(self, words):
        return torch.full((words,), -1, dtype=torch.int32, device=DEV)          # (all bits set: the launch must clear it)

    def plain(self):
        grid, out = self._grid(self.words), torch.full((self.n, self.cout), self.SENTINEL, device=DEV)
        self.lib.check(self.L.imf_conv_first_bitgrid(self.coords.data_ptr(), self.n, self.box, self.ks, grid.data_ptr(), self.words,
                                                     self.w.data_ptr(), self.cout, None, None, 0, out.data_ptr(), self.st),
                       "imf_conv_first_bitgrid")
        return out.cpu().numpy()

    def flags(self):
        grid, out = self._grid(self.words), torch.full((self.n, self.cout), self.SENTINEL, device=DEV)
        word = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.lib.check(self.L.imf_conv_first_bitgrid_flags(self.coords.data_ptr(), self.n, self.box, self.ks, grid.data_ptr(),
                                                           self.words, self.w.data_ptr(), self.cout, None, None, 0, out.data_ptr(),
                                                           word.data_ptr(), self.st), "imf_conv_first_bitgrid_flags")
        return out.cpu().numpy(), int(word.item())

    def dyn(self, grid_words=None):
        """(out [n_cap, cout], err): capacity mode, n_cap = n + 70 rows, the row count and the box on the device."""
        words = self.words if grid_words is None else grid_words
        n_cap = self.n + 70
        coords = torch.zeros((n_cap, 4), dtype=torch.int32, device=DEV)
        coords[: self.n] = self.coords
        n_dev = torch.tensor([self.n], dtype=torch.int32, device=DEV)
        bbox_dev = torch.tensor(self.bbox, dtype=torch.int32, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        grid, out = self._grid(words), torch.full((n_cap, self.cout), self.SENTINEL, device=DEV)
        self.lib.check(self.L.imf_conv_first_bitgrid_dyn(coords.data_ptr(), n_cap, n_dev.data_ptr(), bbox_dev.data_ptr(),
                                                         err.data_ptr(), self.ks, grid.data_ptr(), words, self.w.data_ptr(),
                                                         self.cout, None, None, 0, out.data_ptr(), self.st),
                       "imf_conv_first_bitgrid_dyn")
        return out.cpu().numpy(), int(err.item())


@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("ks", [3, 5])
@pytest.mark.parametrize("name", ("n63", "n64", "n65", "solid", "batched2"))
def test_every_public_bitgrid_entry_counts_exactly(ops, name, ks, cout):
    """imf_conv_first_bitgrid, _flags and _dyn through the C ABI, both kernel sizes and both widths, against the integer
    expectation: one 64-row block and its partial-block edge (n63 / n64 / n65), windows that straddle 32-bit grid words
    (solid), a grid origin b0 over two items (batched2).  Capacity mode leaves the rows beyond the count untouched."""
    b = _BitGrid(ops, name, ks, cout)
    assert np.array_equal(b.plain(), b.want)
    out, word = b.flags()
    assert np.array_equal(out, b.want) and word == 0
    out, err = b.dyn()
    assert err == 0
    assert np.array_equal(out[: b.n], b.want)
    assert (out[b.n:] == b.SENTINEL).all()


def test_bitgrid_flags_reports_the_f16_range(ops):
    """The integer kernel times 2^14: channel 0 of an interior row of `solid` is sum(k + 1) * 2^14 >= 65504, so
    IMF_FLAG_RANGE (32) must be raised -- and the output is still exact: a power-of-two scale keeps the three-part split of
    the weights exact."""
    b = _BitGrid(ops, "solid", 5, 32, kernel_scale=2.0 ** 14)
    assert b.want[:, 0].max() == 125 * 126 // 2 * 2 ** 14 >= 65504
    out, word = b.flags()
    assert word & 32
    assert np.array_equal(out, b.want)


def test_bitgrid_dyn_declines_a_grid_one_word_short(ops):
    """imf_conv_first_bitgrid_dyn with one grid word fewer than the box needs: IMF_FLAG_BITGRID (4) and the launch does
    nothing -- every output row is still the sentinel."""
    b = _BitGrid(ops, "n65", 5, 32)
    out, err = b.dyn(grid_words=b.words - 1)
    assert err & 4
    assert (out == b.SENTINEL).all()


# ------------------------------------------------------------------------------------------------ capacity mode
class _Rb:
    def __init__(self, tile_rows, nbr, tile_mask, n_slots):
        self.tile_rows, self.nbr, self.tile_mask, self.n_slots = tile_rows, nbr, tile_mask, n_slots


@pytest.mark.parametrize("name", ("solid", "faces") + R.CHAINS)
def test_capacity_mode_builds_the_same_rows_and_maps(ops, name):
    """imf_pyramid_build_dyn / imf_rulebook_conv_dyn / imf_rulebook_transpose_dyn with row capacities above the counts: the same
    rows, the same neighbours, -1 and mask 0 in the padding, no flag.  (A wholly empty tile's neighbour slice is left as the
    caller handed it over -- its mask of 0 keeps every reader away -- so the buffers go in filled with -1.)"""
    from imfnet_amd import _lib
    L = _lib.lib()
    c = R.case(name)
    rows, first, g, _ = _expected(name)
    counts = [len(l) for l in g.levels]
    chains = name in R.CHAINS
    n_cap = 512 if chains else c.n_points + 3000                  # (chains: keep every table at the 1 024-slot minimum)
    caps_l = [512] * 4 if chains else [counts[0] + counts[0] // 4 + 100]
    for i in range(1, 4):
        if not chains:
            caps_l.append(min(caps_l[-1], counts[i] + counts[i] // 4 + 100))
    assert all(cap > n for cap, n in zip(caps_l, counts)) and n_cap >= c.n_points
    caps = (C.c_int64 * 4)(*caps_l)
    nbytes = L.imf_pyramid_arena_bytes_caps(n_cap, 4, caps)
    arena = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    meta = torch.zeros(_lib.META_WORDS, dtype=torch.int32, device=DEV)
    dyn = torch.tensor([c.n_points, 1] + [0] * (_lib.DYN_WORDS - 2), dtype=torch.int32, device=DEV)
    buf = torch.zeros((n_cap, 3), dtype=torch.float64, device=DEV)
    buf[: c.n_points] = torch.as_tensor(c.points).to(DEV)
    descs = (_lib.LevelDesc * 4)()
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.imf_pyramid_build_dyn(buf.data_ptr(), 1, dyn.data_ptr(), n_cap, caps, c.vs, 4, arena.data_ptr(), nbytes,
                                       meta.data_ptr(), descs, st), "imf_pyramid_build_dyn")
    m = meta.cpu().numpy()
    assert [int(m[2 * l]) for l in range(4)] == counts and not any(m[2 * l + 1] for l in range(4))      # counts, error words 0
    assert list(m[8:16]) == R.bbox(rows)

    def view(addr, n_ints):
        off = addr - arena.data_ptr()
        return arena[off:off + 4 * n_ints].view(torch.int32)
    for l in range(4):
        assert np.array_equal(view(descs[l].coords, 4 * counts[l]).view(-1, 4).cpu().numpy(), g.levels[l]), f"level {l}"
    assert np.array_equal(view(descs[0].first_idx, counts[0]).cpu().numpy(), first)

    def new_map(n_slots, kvol):
        return (torch.full((n_slots,), -7, dtype=torch.int32, device=DEV), torch.full((kvol * n_slots,), -1, dtype=torch.int32, device=DEV),
                torch.full((n_slots // 64 * 4,), -1, dtype=torch.int32, device=DEV))

    def conv(l_in, l_out, ksize):
        n_slots = L.imf_rulebook_slots(caps_l[l_out])
        tr, nbr, mask = new_map(n_slots, ksize ** 3)
        _lib.check(L.imf_rulebook_conv_dyn(descs[l_in].table, descs[l_in].capacity, descs[l_out].coords, caps_l[l_out],
                                           meta.data_ptr() + 8 * l_out, 1 << l_in, ksize, tr.data_ptr(), nbr.data_ptr(),
                                           mask.data_ptr(), st), "imf_rulebook_conv_dyn")
        return _Rb(tr, nbr, mask, n_slots)

    def check_padding(rb, n_out):
        mask = rb.tile_mask.cpu().numpy().view(np.uint32).reshape(-1, 4)
        assert (mask[(n_out + 63) // 64:] == 0).all()                                        # padding tiles: mask 0
        assert (rb.tile_rows.cpu().numpy()[n_out:] == -1).all()
    rb = conv(0, 0, 5)
    R.check_rulebook(rb, g.k_first, True)
    check_padding(rb, counts[0])
    for i in range(4):
        rb = conv(i, i, 3)
        R.check_rulebook(rb, g.k3[i], True)
        check_padding(rb, counts[i])
    for i in range(3):
        rb = conv(i, i + 1, 3)
        R.check_rulebook(rb, g.down[i], True)
        check_padding(rb, counts[i + 1])
        n_slots = L.imf_rulebook_transpose_slots(caps_l[i])
        tr, nbr, mask = new_map(n_slots, 27)
        counters = torch.zeros(16, dtype=torch.int32, device=DEV)
        _lib.check(L.imf_rulebook_transpose_dyn(descs[i + 1].table, descs[i + 1].capacity, descs[i].coords, caps_l[i],
                                                meta.data_ptr() + 8 * i, 1 << i, 3, tr.data_ptr(), nbr.data_ptr(), mask.data_ptr(),
                                                n_slots, counters.data_ptr(), st), "imf_rulebook_transpose_dyn")
        up = _Rb(tr, nbr, mask, n_slots)
        R.check_transposed(up, g.up[i], R.transpose_slots(g.levels[i], 1 << i, n_slots))
        empty = (tr.cpu().numpy().reshape(-1, 64) < 0).all(1)
        assert (mask.cpu().numpy().reshape(-1, 4)[empty] == 0).all()
    assert not meta.cpu().numpy()[[1, 3, 5, 7]].any()                                  # still no flag after the maps


# ------------------------------------------------------------------------------------------------ the range error
def test_just_outside_raises_and_the_next_build_is_exact(ops):
    """One point at voxel 2^17, one at -2^17 - 1, each among valid points: the promised range error on both public paths, no
    fault, and the process goes on building exact geometry."""
    from imfnet_amd import ImfError
    for pts in R.just_outside():
        xyz = torch.as_tensor(pts).to(DEV)
        with pytest.raises(ImfError):
            ops.pyramid_from_points(xyz, R.VS, 4)
        lv = ops.voxelize(xyz, R.VS)
        with pytest.raises(ImfError):
            ops.sync_levels([lv])
        rows, first, g, _ = _expected("lines")
        levels, cm = _build(ops, "lines")
        _check_levels(levels, rows, first, g)
        _check_maps(cm, g)
    rows, first, g, _ = _expected("faces")                                             # the last voxels inside are fine
    levels, cm = _build(ops, "faces")
    _check_levels(levels, rows, first, g)
    assert levels[0].bbox[1:4] == [-R.LIM] * 3 and levels[0].bbox[5:8] == [R.LIM - 1] * 3
