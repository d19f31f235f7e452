"""The tail of the map builders against the CPU twins, array against array: the parity-grouped transposed maps (class
grouping without a scan launch or any state between calls; probes only on the coarse lattice) and the occupancy-sorted twin's gather (all 27 loads of a
slot in flight; the run-time loop for other kernel volumes).  The twins probe EVERY offset and group serially, so equality
says that a skipped probe was a miss and that the slot table is the scan's.  Every case is built twice into the same
buffers: the second build starts from the first one's leftovers (the class counts live in the head of the neighbour table,
`counters` is scratch) and must give the same bits."""

import numpy as np
import pytest
import torch

import imf_cpu_twins as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIM = 1 << 17


def _first_unique(a):
    _, idx = np.unique(a, axis=0, return_index=True)
    return np.ascontiguousarray(a[np.sort(idx)])


def _box(rng, n, ts, lo=-12, hi=12, b=0):
    """n distinct voxels of tensor stride ts in [lo, hi)^3 lattice units, in random order."""
    side = hi - lo
    cells = rng.permutation(side ** 3)[:n]
    q = np.stack([cells % side, cells // side % side, cells // (side * side)], 1) + lo
    return np.concatenate([np.full((n, 1), b), q * ts], 1).astype(np.int32)


def _parents(fine, ts):
    c = fine.copy()
    c[:, 1:] = np.floor_divide(fine[:, 1:], 2 * ts) * (2 * ts)
    return _first_unique(c)


def _transposed(fine, ts, coarse=None, cap=None):
    """(GPU (rows, nbr, mask), twin (rows, nbr, mask)) of one transposed map; cap: capacity mode with len(fine) rows on the device."""
    from imfnet_amd import _lib, ops
    L = _lib.lib()
    coarse = _parents(fine, ts) if coarse is None else coarse
    n = len(fine)
    twin = T.rulebook_transpose(T.downsample(T.Level(coarse, np.empty(0, T._SLOT)), 2 * ts), T.Level(fine, np.empty(0, T._SLOT)), ts)
    src = ops.Level(torch.as_tensor(coarse).to(DEV), torch.tensor([len(coarse), 0], dtype=torch.int32, device=DEV), None, 0, ts)
    src.n = len(coarse)
    clv = ops.downsample(src, 2 * ts)                    # distinct multiples of 2 ts: the same rows, in a table of that level
    ops.sync_levels([clv])
    assert clv.n == len(coarse) and np.array_equal(clv.coords.cpu().numpy(), coarse)
    n_cap = n if cap is None else cap
    buf = torch.zeros((n_cap, 4), dtype=torch.int32, device=DEV)
    buf[:n] = torch.as_tensor(fine).to(DEV)
    n_dev = torch.tensor([n, 0], dtype=torch.int32, device=DEV)
    n_slots = L.imf_rulebook_transpose_slots(n_cap)
    rows = torch.full((n_slots,), -7, dtype=torch.int32, device=DEV)
    nbr = torch.full((27 * n_slots,), -9, dtype=torch.int32, device=DEV)
    mask = torch.full((n_slots // 64 * 4,), -1, dtype=torch.int32, device=DEV)
    counters = torch.full((16,), 12345, dtype=torch.int32, device=DEV)           # scratch: nothing may rely on its contents
    st = torch.cuda.current_stream().cuda_stream
    got = []
    for _ in range(2):
        if cap is None:
            _lib.check(L.imf_rulebook_transpose(clv.table.data_ptr(), clv.capacity, buf.data_ptr(), n, ts, 3, rows.data_ptr(),
                                                nbr.data_ptr(), mask.data_ptr(), n_slots, counters.data_ptr(), st), "transpose")
        else:
            _lib.check(L.imf_rulebook_transpose_dyn(clv.table.data_ptr(), clv.capacity, buf.data_ptr(), n_cap, n_dev.data_ptr(), ts, 3,
                                                    rows.data_ptr(), nbr.data_ptr(), mask.data_ptr(), n_slots, counters.data_ptr(),
                                                    st), "transpose_dyn")
        got.append((rows.cpu().numpy(), nbr.cpu().numpy().reshape(27, n_slots), mask.cpu().numpy().view(np.uint32).reshape(-1, 4),
                    counters.cpu().numpy()))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    return got[0], twin


def _check_transposed(fine, ts, coarse=None, cap=None):
    (rows, nbr, mask, counters), (t_rows, t_nbr, t_mask) = _transposed(fine, ts, coarse, cap)
    s = len(t_rows)                                      # capacity mode: the twin's table is the head of the larger one
    assert np.array_equal(rows[:s], t_rows) and (rows[s:] == -1).all()
    assert np.array_equal(mask[:s // 64], t_mask) and (mask[s // 64:] == 0).all()
    if cap is None:
        assert np.array_equal(nbr, t_nbr)                # all 27 slices, padding slots and padding tiles included
    else:                                                # capacity mode leaves the slices of tiles without rows unwritten (mask 0)
        live = np.repeat((rows.reshape(-1, 64) >= 0).any(1), 64)
        assert np.array_equal(nbr[:, :s][:, live[:s]], t_nbr[:, live[:s]]) and not live[s:].any()
    par = (fine[:, 1:] // ts) & 1
    cls = par[:, 0] | par[:, 1] << 1 | par[:, 2] << 2
    total = np.bincount(cls, minlength=8)
    assert np.array_equal(counters[:8], total)
    assert np.array_equal(counters[8:], np.concatenate([[0], np.cumsum((total + 63) // 64 * 64)[:-1]]))
    return rows, nbr, mask, cls


@pytest.mark.parametrize("ts", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 8500])
def test_transposed_map_row_counts(ts, n):
    """One row to more than 32 count chunks (8 500 rows = 34 chunks of 256), all eight classes, negative coordinates."""
    fine = _box(np.random.default_rng(n + ts), n, ts)
    rows, nbr, mask, cls = _check_transposed(fine, ts)
    if n >= 130:
        assert len(np.unique(cls)) == 8 and (fine[:, 1:] < 0).any()
    assert (nbr >= 0).sum() >= n                         # every fine row has its own parent at least


def test_transposed_map_many_groups():
    """More than 256 count chunks: several chunks per counting workgroup, sums over groups and over the chunks inside one."""
    fine = _box(np.random.default_rng(5), 70_000, 1, -21, 21)
    _check_transposed(fine, 1)


@pytest.mark.parametrize("ts", [1, 2, 4])
def test_transposed_map_one_class_and_absent_parents(ts):
    rng = np.random.default_rng(ts)
    q = _box(rng, 200, 1, -6, 6)
    for par in (0, 1):                                   # only class 0 (one offset on the lattice) / only class 7 (eight)
        fine = q.copy()
        fine[:, 1:] = (2 * q[:, 1:] + par) * ts
        rows, nbr, mask, cls = _check_transposed(fine, ts)
        assert (cls == 7 * par).all()
        live = mask[:, 0][mask[:, 0] != 0]               # class 0: the centre; class 7: the eight corners, k = 26 the row's own parent
        lattice = (1 << 13) if par == 0 else 0x5140145
        assert len(live) == 4 and (live & ~np.uint32(lattice) == 0).all() and (live >> (13 if par == 0 else 26) & 1).all()
    # class 0 far from every coarse voxel (its only parent, the voxel itself, is absent) beside a class 7 with all its parents
    a = q[:100].copy()
    a[:, 1:] = 2 * q[:100, 1:] * ts
    a[:, 1] += 1000 * ts
    b = q[100:].copy()
    b[:, 1:] = (2 * q[100:, 1:] + 1) * ts
    fine = np.concatenate([a, b])[rng.permutation(200)]
    rows, nbr, mask, cls = _check_transposed(fine, ts, coarse=_parents(b, ts)[::-1].copy())
    in0 = np.isin(rows, np.flatnonzero(cls == 0))
    assert in0.sum() == 100 and (nbr[:, in0] == -1).all()
    assert (mask[np.flatnonzero(in0.reshape(-1, 64).any(1))] == 0).all()
    assert (nbr[:, np.isin(rows, np.flatnonzero(cls == 7))] >= 0).sum() >= 100


@pytest.mark.parametrize("ts", [1, 2, 4])
def test_transposed_map_range_faces_and_batches(ts):
    """Two-voxel patches on the six faces of the [-2^17, 2^17) cube (a neighbour beyond a face does not exist, and must not wrap
    to the opposite one, which is occupied), all-negative coordinates, and the same geometry in batch items 0 and 1."""
    pts = []
    for axis in range(3):
        for face in (-LIM, LIM - ts):
            for step in (0, 1):
                for other in (0, -3 * ts):
                    p = [other, other, other]
                    p[axis] = face + (step * ts if face < 0 else -step * ts)
                    pts.append([0] + p)
    patches = np.array(pts, np.int32)
    for fine in (patches, _box(np.random.default_rng(9), 300, ts, -40, -20)):
        both = np.concatenate([fine, fine + np.array([1, 0, 0, 0], np.int32)])
        rows, nbr, mask, cls = _check_transposed(both, ts)
        n = len(fine)
        order = np.argsort(np.where(rows >= 0, rows, 1 << 30), kind="stable")[:2 * n]      # slot of row r
        hit0, hit1 = nbr[:, order[:n]], nbr[:, order[n:]]
        assert np.array_equal(hit0 >= 0, hit1 >= 0) and (hit0 >= 0).any()


@pytest.mark.parametrize("n,cap", [(1, 64), (130, 1000), (8500, 9000), (640, 641)])
def test_transposed_map_capacity_mode(n, cap):
    """The row count on the device, below the capacity the table is sized for: class tiles at the end without rows."""
    for ts in (1, 2):
        _check_transposed(_box(np.random.default_rng(n), n, ts), ts, cap=cap)


# ---------------------------------------------------------------------------------------------------- the sorted twin
def _sorted_both(nbr_in, n_out, n_dev):
    from imfnet_amd import _lib
    L, TL = _lib.lib(), T._lib()
    kvol, n_slots = nbr_in.shape
    t_rows, t_nbr, t_mask = np.empty(n_slots, np.int32), np.empty((kvol, n_slots), np.int32), np.empty((n_slots // 64, 4), np.uint32)
    ws = np.empty(TL.imf_cpu_rulebook_sorted_workspace_bytes(n_slots), np.uint8)
    nd = None if n_dev is None else np.array([n_dev, 0], np.int32)
    assert TL.imf_cpu_rulebook_sort_by_occupancy(nbr_in.ctypes.data, kvol, n_slots, n_out, None if nd is None else nd.ctypes.data,
                                                 t_rows.ctypes.data, t_nbr.ctypes.data, t_mask.ctypes.data, ws.ctypes.data, ws.size,
                                                 None) == 0
    src = torch.as_tensor(nbr_in).to(DEV)
    nd_t = None if nd is None else torch.as_tensor(nd).to(DEV)
    got = []
    for _ in range(2):
        rows = torch.full((n_slots,), -7, dtype=torch.int32, device=DEV)
        nbr = torch.full((kvol * n_slots,), -9, dtype=torch.int32, device=DEV)
        mask = torch.full((n_slots // 64 * 4,), -1, dtype=torch.int32, device=DEV)
        wsd = torch.empty(L.imf_rulebook_sorted_workspace_bytes(n_slots), dtype=torch.uint8, device=DEV)
        _lib.check(L.imf_rulebook_sort_by_occupancy(src.data_ptr(), kvol, n_slots, n_out, None if nd_t is None else nd_t.data_ptr(),
                                                    rows.data_ptr(), nbr.data_ptr(), mask.data_ptr(), wsd.data_ptr(), wsd.numel(),
                                                    torch.cuda.current_stream().cuda_stream), "imf_rulebook_sort_by_occupancy")
        got.append((rows.cpu().numpy(), nbr.cpu().numpy().reshape(kvol, n_slots), mask.cpu().numpy().view(np.uint32).reshape(-1, 4)))
    for a, b, t in zip(got[0], got[1], (t_rows, t_nbr, t_mask)):
        assert np.array_equal(a, b) and np.array_equal(a, t)
    return got[0]


@pytest.mark.parametrize("kvol", [27, 8])
@pytest.mark.parametrize("n_slots", [64, 128, 16384, 16448, 65536, 65600])
def test_sorted_twin_gather(kvol, n_slots):
    """kvol 27 (every load in flight up to 65 536 slots, the run-time loop beyond) and 8 (the loop); one tile, two, a whole 16 384-slot
    window and one tile beyond it, the last size of the in-flight kernel and the first of the loop;
    1 and n_slots - 1 rows, exact and with the count on the device; random, full and centre-only maps."""
    rng = np.random.default_rng(kvol * n_slots)
    centre = kvol // 2
    for n in (1, n_slots - 1):
        for kind in ("random", "full", "centre"):
            nbr = np.full((kvol, n_slots), -1, np.int32)
            if kind == "random":
                nbr[:, :n] = np.where(rng.random((kvol, n)) < 0.5, rng.integers(0, n, (kvol, n)), -1)
            elif kind == "full":
                nbr[:, :n] = rng.integers(0, n, (kvol, n))
            else:
                nbr[centre, :n] = np.arange(n)
            rows, out, mask = _sorted_both(nbr, n, None)
            assert np.array_equal(np.sort(rows[rows >= 0]), np.arange(n))
            want = {"full": (1 << kvol) - 1, "centre": 1 << centre}.get(kind)
            if want is not None:
                assert (mask[: (n + 63) // 64, 0] == want).all() and (mask[(n + 63) // 64:] == 0).all()
            # capacity mode: the table sized for n_slots rows, n of them on the device (the slices beyond n hold leftovers)
            stale = nbr.copy()
            stale[:, n:] = rng.integers(0, n_slots, (kvol, n_slots - n))
            rows_c, out_c, mask_c = _sorted_both(stale, n_slots, n)
            assert np.array_equal(rows_c, rows) and np.array_equal(out_c, out) and np.array_equal(mask_c, mask)
