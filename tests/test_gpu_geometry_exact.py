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
