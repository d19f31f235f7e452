"""Fragment overlap on the GPU: the nearest-neighbour correspondences and overlap ratios of every fragment pair of a
sequence (csrc/overlap.hip).

Replaces what data/compute_overlap.py:93-141 does with one pyflann k-d forest per fragment and one query per pair.  Here a
sequence is one job: every fragment's index is built once and stays on the device, a bound over all candidate pairs
rejects most of them from the cell tables alone, and only the survivors run the exact pass.  There is no CPU path: a
missing library or a failing call raises.
"""
import ctypes as C
import hashlib

import numpy as np
import torch

from . import _lib

DIST_THRESH = 0.075
MIN_OVERLAP = 0.3
MAX_POINTS = 300000
CELL_MARGIN = 1.0 + 2.0 ** -16      # cell edge over the threshold: csrc/overlap.hip says why a hair is enough
FLAG_RANGE = 1


def seed_of(seed_key):
    """A 64-bit seed from a tuple of ints and strings (the run's seed, scene, sequence, fragment name): the same for
    the same key whatever was processed before."""
    text = "\x1f".join(str(k) for k in seed_key).encode("utf-8")
    return int.from_bytes(hashlib.sha256(text).digest()[:8], "little")


def downsample(points, max_points, seed_key):
    """Upstream's Cloud.downsample_from with a seeded choice: (float32 [m,3], int64 [m] indices into `points`).  At or
    below max_points every point is kept in its order; above it, max_points of them are drawn without replacement by
    numpy's default_rng(seed_of(seed_key))."""
    points = np.asarray(points)
    n = len(points)
    if n <= max_points:
        return np.ascontiguousarray(points, dtype=np.float32), np.arange(n, dtype=np.int64)
    indices = np.random.default_rng(seed_of(seed_key)).choice(n, int(max_points), replace=False).astype(np.int64)
    return np.ascontiguousarray(points[indices, :], dtype=np.float32), indices


def candidate_pairs(numbers):
    """Upstream's pair loop on the fragment numbers in list order: (i, j) with i before j, consecutive numbers left out."""
    numbers = [int(k) for k in numbers]
    out = []
    for i in range(len(numbers)):
        for j in range(i + 1, len(numbers)):
            if not numbers[i] < numbers[j]:
                raise ValueError(f"fragment numbers must ascend, got {numbers[i]} before {numbers[j]}")
            if numbers[i] + 1 != numbers[j]:
                out.append((i, j))
    return out


def overlap_ratio(n, n_p, n_q):
    return float(n) / max(n_p, n_q)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class FragmentIndex:
    """The resident search index of one fragment: its float32 points sorted by cell, their original indices, the cell
    table, the occupied cells and the query chunks (struct imf_overlap_index), in one device allocation."""

    def __init__(self, points, cell, device="cuda", workspace=None):
        self.L = _lib.lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.ImfError("FragmentIndex runs on the GPU only (device='cuda')")
        pts = torch.as_tensor(points)
        if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] == 0 or pts.dtype != torch.float32:
            raise _lib.ImfError(f"points must be float32 [n>0, 3], got {pts.dtype} {tuple(pts.shape)}")
        pts = pts.to(self.device).contiguous()
        self.n, self.cell = int(pts.shape[0]), float(cell)
        nbytes = self.L.imf_overlap_index_bytes(self.n)
        if nbytes == 0:
            raise _lib.ImfError(f"imf_overlap_index_bytes refuses n={self.n}")
        self.storage = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        ws_bytes = self.L.imf_overlap_index_workspace_bytes(self.n)
        ws = workspace if workspace is not None and workspace.numel() >= ws_bytes else \
            torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        self.desc = _lib.OverlapIndex()
        rc = self.L.imf_overlap_index_build(_ptr(pts), self.n, self.cell, _ptr(self.storage), nbytes, C.byref(self.desc),
                                            _ptr(ws), ws.numel(), _stream(self.device))
        _lib.check(rc, "imf_overlap_index_build")
        self._meta = None

    @staticmethod
    def device_bytes(n):
        """Bytes one index of n points keeps on the device."""
        return int(_lib.lib().imf_overlap_index_bytes(int(n)))

    @property
    def meta(self):
        """(occupied cells, query chunks, flags, points indexed), read from the device once."""
        if self._meta is None:
            off = self.desc.meta - self.storage.data_ptr()
            self._meta = tuple(self.storage[off:off + 16].view(torch.int32).tolist())
            if self._meta[2] & FLAG_RANGE:
                raise _lib.ImfError("FragmentIndex: a point is NaN or beyond the cell range")
        return self._meta

    n_cells = property(lambda self: self.meta[0])
    n_chunks = property(lambda self: self.meta[1])


def descriptor_table(indices, device):
    """The indices' structs as one device array (what imf_overlap_bound reads)."""
    raw = b"".join(bytes(ix.desc) for ix in indices)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def overlap_bounds(indices, pairs, device):
    """int64 [len(pairs)]: for every (i, j) the points of j whose cell has an occupied cell of i around it."""
    out = np.zeros(len(pairs), np.int64)
    if not pairs:
        return out
    L = _lib.lib()
    table = descriptor_table(indices, device)
    max_cells = max(ix.n_cells for ix in indices)
    for b in range(0, len(pairs), 65535):
        part = pairs[b:b + 65535]
        pr = torch.tensor(part, dtype=torch.int32, device=device).contiguous()
        bound = torch.empty(len(part), dtype=torch.int64, device=device)
        _lib.check(L.imf_overlap_bound(_ptr(table), _ptr(pr), len(part), max_cells, _ptr(bound), _stream(device)),
                   "imf_overlap_bound")
        out[b:b + len(part)] = bound.cpu().numpy()
    return out


class PairBuffers:
    """nn_idx, the rows and the emit workspace for queries of up to n_max points, reused from pair to pair."""

    def __init__(self, n_max, device):
        L = _lib.lib()
        self.nn = torch.empty(n_max, dtype=torch.int32, device=device)
        self.pairs = torch.empty((n_max, 2), dtype=torch.int64, device=device)
        self.out_n = torch.zeros(1, dtype=torch.int64, device=device)
        self.ws = torch.empty(max(256, L.imf_overlap_emit_workspace_bytes(n_max)), dtype=torch.uint8, device=device)


def pair_overlap(ip, iq, thresh, buffers=None):
    """The exact pass and the emit for one pair: (n, rows), rows a device int64 [n,2] view of the buffers (valid until
    the next call with them)."""
    L = _lib.lib()
    dev = iq.device
    buf = buffers if buffers is not None else PairBuffers(iq.n, dev)
    st = _stream(dev)
    _lib.check(L.imf_overlap_pair(C.byref(ip.desc), C.byref(iq.desc), float(np.float32(thresh)), iq.n_chunks, _ptr(buf.nn),
                                  st), "imf_overlap_pair")
    _lib.check(L.imf_overlap_emit(_ptr(buf.nn), iq.n, _ptr(buf.pairs), _ptr(buf.out_n), _ptr(buf.ws), buf.ws.numel(), st),
               "imf_overlap_emit")
    n = int(buf.out_n.item())
    return n, buf.pairs[:n]


def build_indices(clouds, thresh, device="cuda"):
    """One FragmentIndex per cloud (float32 [n,3]), after checking that they fit the device's free memory."""
    device = torch.device(device)
    cell = float(np.float32(thresh)) * CELL_MARGIN
    need = sum(FragmentIndex.device_bytes(len(c)) + 12 * len(c) for c in clouds)
    free, _ = torch.cuda.mem_get_info(device)
    if need > 0.9 * free:
        raise _lib.ImfError(f"the indices of {len(clouds)} fragments need {need >> 20} MiB, the device has "
                            f"{free >> 20} MiB free")
    n_max = max((len(c) for c in clouds), default=0)
    ws = torch.empty(_lib.lib().imf_overlap_index_workspace_bytes(n_max), dtype=torch.uint8, device=device) if n_max else None
    indices = [FragmentIndex(torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)), cell, device, ws) for c in clouds]
    for ix in indices:
        ix.meta                                              # one read each, after all builds are queued
    return indices


def sequence_overlap(clouds, thresh=DIST_THRESH, min_overlap=MIN_OVERLAP, numbers=None, prefilter=True, device="cuda",
                     stats=None):
    """All kept pairs of one sequence: {(i, j): (ratio, int64 numpy [n,2] rows (index in i, index in j))}.

    clouds: the down-sampled float32 [n,3] fragments in list order; numbers: their fragment numbers (default: their
    positions), of which consecutive ones form no pair.  Every index is built once; the bound runs over all candidate
    pairs in one launch; the exact pass runs on the pairs whose bound reaches min_overlap (prefilter=False: on all of
    them -- the result is the same).  stats (a dict) receives `bound` {pair: int}, `exact` {pair: n} and `indices`."""
    device = torch.device(device)
    clouds = [np.ascontiguousarray(c, dtype=np.float32) for c in clouds]
    if any(c.ndim != 2 or c.shape[1] != 3 for c in clouds):
        raise ValueError("every cloud must be [n,3]")
    numbers = list(range(len(clouds))) if numbers is None else list(numbers)
    pairs = [(i, j) for i, j in candidate_pairs(numbers) if len(clouds[i]) and len(clouds[j])]
    out = {}
    if stats is not None:
        stats.update(bound={}, exact={}, indices=None)
    if not pairs:
        return out
    used = sorted({k for p in pairs for k in p})
    built = build_indices([clouds[k] for k in used], thresh, device)
    indices = {k: ix for k, ix in zip(used, built)}
    where = {k: n for n, k in enumerate(used)}
    bounds = overlap_bounds(built, [(where[i], where[j]) for i, j in pairs], device)
    buffers = PairBuffers(max(ix.n for ix in built), device)
    if stats is not None:
        stats["indices"] = indices
    for (i, j), bound in zip(pairs, bounds.tolist()):
        n_p, n_q = len(clouds[i]), len(clouds[j])
        if stats is not None:
            stats["bound"][(i, j)] = int(bound)
        if prefilter and overlap_ratio(bound, n_p, n_q) < min_overlap:
            continue
        n, rows = pair_overlap(indices[i], indices[j], thresh, buffers)
        if stats is not None:
            stats["exact"][(i, j)] = n
        ratio = overlap_ratio(n, n_p, n_q)
        if ratio < min_overlap:
            continue
        out[(i, j)] = (ratio, rows.cpu().numpy())
    return out
