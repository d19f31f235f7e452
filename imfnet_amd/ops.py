"""Tensor-level wrappers over the C ABI (include/imfnet_hip.h).  torch is used only for device
memory and streams; every computation below happens in libimfnet_hip.so on the GPU."""
import ctypes as C
import os
import weakref

import torch

from . import _lib
from ._lib import ConvArgs, HeadArgs, ImfError, LevelDesc, TILE_ROWS, MASK_WORDS, check


# When set to a list, every sparse-conv launch is bracketed by HIP events recorded on the launch
# stream right around the main kernel and appended as a dict (bench.py's live roofline
# measurement).  None in normal operation.
TRACE = None


class _Ev:
    """A raw hipEvent_t pair owned by the library side of the C ABI."""

    def __init__(self):
        L = _lib.lib()
        self.begin, self.end = L.imf_event_create(), L.imf_event_create()

    def elapsed_ms(self):
        return _lib.lib().imf_event_elapsed_ms(self.begin, self.end)

    def __del__(self):
        try:
            L = _lib.lib()
            L.imf_event_destroy(self.begin)
            L.imf_event_destroy(self.end)
        except Exception:
            pass


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _req(t, dtype, name, ndim=None):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ImfError(f"{name} must be a CUDA(HIP) tensor -- imfnet_amd has no CPU path")
    if t.dtype != dtype:
        raise ImfError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ImfError(f"{name} must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise ImfError(f"{name} must be {ndim}-D")
    return t


class Level:
    """One coordinate map: rows `coords[:n]` (int32 (b,x,y,z)) at tensor stride `ts`, and the
    voxel hash (`table`: 16-byte {key, row} slots, struct imf_slot) mapping a coordinate to its row."""
    __slots__ = ("coords_buf", "n_dev", "n", "table", "capacity", "ts", "first_idx_buf")

    def __init__(self, coords_buf, n_dev, table, capacity, ts, first_idx_buf=None):
        self.coords_buf, self.n_dev, self.n = coords_buf, n_dev, None
        self.table, self.capacity, self.ts = table, capacity, ts
        self.first_idx_buf = first_idx_buf

    @property
    def coords(self):
        return self.coords_buf[: self.n]

    @property
    def first_idx(self):
        return self.first_idx_buf[: self.n]

    @property
    def device(self):
        return self.coords_buf.device


class _Addr:
    """A raw device address with the `.data_ptr()` face of a tensor (memory owned by an arena)."""
    __slots__ = ("p",)

    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


class ArenaLevel(Level):
    """A Level whose buffers live inside one arena built by imf_pyramid_build (raw addresses; the
    coords / first_idx tensors are materialised as views only when somebody asks for them)."""
    __slots__ = ("arena", "_desc", "_coords_view", "_first_view", "bbox", "items")

    def __init__(self, arena, desc, n_dev):
        Level.__init__(self, _Addr(desc.coords), n_dev, _Addr(desc.table), desc.capacity,
                       desc.tensor_stride, _Addr(desc.first_idx) if desc.first_idx else None)
        self.arena, self._desc, self._coords_view, self._first_view = arena, desc, None, None
        self.bbox = None              # level 0: [min b,x,y,z, max b,x,y,z] (host ints)
        self.items = None             # [(first row, rows)] per batch item

    def _view(self, addr, count):
        off = addr - self.arena.data_ptr()
        return self.arena[off:off + 4 * count].view(torch.int32)

    @property
    def coords(self):
        if self._coords_view is None:
            self._coords_view = self._view(self._desc.coords, 4 * self._desc.cap_rows).view(-1, 4)
        return self._coords_view[: self.n]

    @property
    def first_idx(self):
        if self._first_view is None:
            self._first_view = self._view(self._desc.first_idx, self._desc.cap_rows)
        return self._first_view[: self.n]

    @property
    def device(self):
        return self.arena.device


_AUX_STREAMS = {}
_PINNED = {}


def aux_streams(device):
    """The package's THREE streams of a device: (raw hipStream_t handles, torch views), created through the library one
    right after the other.  HIP multiplexes streams onto four hardware queues (a new stream goes to the least-used one),
    and torch's pool hands its streams out in an order the process's history decides: branches that should overlap then
    share a queue and run one after the other (round 3: the same forward 0.75 or 2.0 ms, the fp32 exact-mode pair 2.3 or
    3.4 ms).  These three, born together, have sat on different queues in every process measured; a FOURTH born right behind
    them has not (LAB_NOTES 4i) -- see `ahead_stream`.  Every executor takes its auxiliary streams from here:
        capacity mode (model/graph.py, stream.py):  main, side (coarse levels + rulebooks), image branch
        exact mode (extract.py, model/plan.py):      geometry, side (rulebooks), image branch
    -- the two modes never run at the same time, and the caller's own stream is the fourth."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    s = _AUX_STREAMS.get(device)
    if s is None:
        L = _lib.lib()
        with torch.cuda.device(device):
            raw = (L.imf_stream_create(), L.imf_stream_create(), L.imf_stream_create())
        if not all(raw):
            raise ImfError("could not create the package's three streams")
        s = _AUX_STREAMS[device] = (raw, tuple(torch.cuda.ExternalStream(r, device=device) for r in raw))
    return s


AHEAD_CANDIDATES = 6
_AHEAD_STREAMS = {}
AHEAD_NOTES = {}          # device -> what `ahead_stream` found there (one line)


def ahead_stream(device):
    """The device's AHEAD stream (raw hipStream_t) for capacity-mode forwards issued back to back
    (imf_fragment_io.ahead_stream: the next forward's encoder beside this one's decoder), or None.  Created on first use, so
    exact-mode callers never pay for it.  It must run BESIDE main, side and image: on a hardware queue one of them uses the
    same issue order is 15 % slower than one chain, on another queue 12 % faster, and which queue a new stream gets depends on
    what the process created before (LAB_NOTES 4i: the stream born right behind the three shared the image stream's queue,
    the third or fourth after them did not).  So it is MEASURED (imf_streams_concurrent, ~1 ms per candidate, once per
    device): the first of AHEAD_CANDIDATES new streams that runs beside all three is kept, the others are destroyed; with
    none, None -- every forward then keeps its one main chain, and a warning says so (AHEAD_NOTES has the line).  HIP has
    four queues and the process's default stream holds one: the queue found is usually that one, so a client that keeps
    torch's DEFAULT stream busy while forwards run shares it with the ahead stream; such a client sets IMF_ENCODER_AHEAD=0."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device in _AHEAD_STREAMS:
        return _AHEAD_STREAMS[device]
    raw = aux_streams(device)[0]
    L = _lib.lib()
    made, found = [], None
    with torch.cuda.device(device):
        for _ in range(AHEAD_CANDIDATES):
            s = L.imf_stream_create()
            if not s:
                break
            made.append(s)
            answers = [L.imf_streams_concurrent(o, s) for o in raw]
            if min(answers) < 0:                      # the probe itself failed: an error, not "shares a queue"
                for m in made:
                    L.imf_stream_destroy(m)
                raise ImfError("imf_streams_concurrent: " + L.imf_last_error().decode())
            if all(a == 1 for a in answers):
                found = s
                break
        for m in made:
            if m != found:
                L.imf_stream_destroy(m)
    if found:
        AHEAD_NOTES[device] = "ahead stream: candidate %d of %d runs beside main, side and image" % (len(made), AHEAD_CANDIDATES)
    else:
        AHEAD_NOTES[device] = ("no ahead stream: none of %d new streams runs beside main, side and image on %s; forwards keep "
                               "one main chain" % (len(made), device))
        import logging
        logging.getLogger("imfnet_amd").warning(AHEAD_NOTES[device])
    _AHEAD_STREAMS[device] = found
    return found


def geometry_stream(device):
    """Dedicated stream for the exact-mode geometry build: its row-count readback must not queue behind the previous
    fragment's convolutions on the caller's stream."""
    return aux_streams(device)[1][0]


class PyramidFuture:
    """Geometry of one fragment queued on the geometry stream; `result()` blocks on ITS event only."""

    def __init__(self, xyz, voxel_size, n_levels=4, batch_index=0, inputs_ready=False, item_starts=None, quantize="f64"):
        if xyz.dtype not in (torch.float64, torch.float32):
            raise ImfError(f"xyz must be float64/float32, got {xyz.dtype}")
        if quantize not in ("f64", "f32"):
            raise ImfError(f"quantize must be 'f64' or 'f32', got {quantize!r}")
        if quantize == "f32" and xyz.dtype != torch.float32:
            raise ImfError("quantize='f32' takes float32 points")
        # xyz_is_f64: 1 float64, 0 float32 widened before the division, 2 float32 quotient (IMF_XYZ_F32_QUOTIENT)
        mode = _lib.XYZ_F32_QUOTIENT if quantize == "f32" else int(xyz.dtype == torch.float64)
        _req(xyz, xyz.dtype, "xyz", 2)
        n, dev = xyz.shape[0], xyz.device
        if n == 0 or xyz.shape[1] != 3:
            raise ImfError(f"xyz must be [N>0, 3], got {tuple(xyz.shape)}")
        L = _lib.lib()
        self.n_levels, self.dev = n_levels, dev
        self.n_items = 1 if item_starts is None else len(item_starts)   # batch of fragments: points back to back
        if self.n_items > _lib.MAX_BATCH:
            raise ImfError(f"at most {_lib.MAX_BATCH} fragments per batch, got {self.n_items}")
        n_meta = 2 * n_levels + 8 + (_lib.MAX_BATCH * n_levels if self.n_items > 1 else 0)
        main = torch.cuda.current_stream(dev)
        gs = geometry_stream(dev)
        if not inputs_ready:
            gs.wait_stream(main)
        pool = _PINNED.setdefault((dev, n_meta), [])
        self.host = pool.pop() if pool else torch.empty(n_meta, dtype=torch.int32).pin_memory()
        self.descs = (LevelDesc * n_levels)()
        with torch.cuda.stream(gs):
            nbytes = L.imf_pyramid_arena_bytes(n, n_levels)
            self.arena = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.meta = torch.empty(n_meta, dtype=torch.int32, device=dev)   # counts/flags + bbox (+ item starts)
            if self.n_items > 1:
                starts = (C.c_int64 * self.n_items)(*[int(v) for v in item_starts])
                check(L.imf_pyramid_build_batched(xyz.data_ptr(), mode, n,
                                                  float(voxel_size), starts, self.n_items, n_levels,
                                                  self.arena.data_ptr(), nbytes, self.meta.data_ptr(), self.descs,
                                                  gs.cuda_stream), "imf_pyramid_build_batched")
            else:
                check(L.imf_pyramid_build(xyz.data_ptr(), mode, n, float(voxel_size),
                                          int(batch_index), n_levels, self.arena.data_ptr(), nbytes,
                                          self.meta.data_ptr(), self.descs, gs.cuda_stream), "imf_pyramid_build")
            self.host.copy_(self.meta, non_blocking=True)
            self.ev = torch.cuda.Event()
            self.ev.record(gs)
        xyz.record_stream(gs)
        self.xyz = xyz
        self._levels = None

    def result(self):
        """Wait for the row counts (the one host wait of the fragment) and hand the levels to the
        CURRENT stream."""
        if self._levels is not None:
            return self._levels
        n_levels = self.n_levels
        self.ev.synchronize()
        main = torch.cuda.current_stream(self.dev)
        main.wait_event(self.ev)
        self.arena.record_stream(main)
        self.meta.record_stream(main)
        counts = self.host.tolist()
        _PINNED[(self.dev, len(counts))].append(self.host)
        self.host = None
        levels = []
        for i in range(n_levels):
            if counts[2 * i + 1] != 0:
                raise ImfError("voxelize: a coordinate fell outside [-2^17, 2^17) voxels (or was NaN)")
            lv = ArenaLevel(self.arena, self.descs[i], self.meta[2 * i:2 * i + 2])
            lv.n = int(counts[2 * i])
            levels.append(lv)
        levels[0].bbox = counts[2 * n_levels:2 * n_levels + 8]
        for i, lv in enumerate(levels):              # (first row, rows) of every batch item at this level
            if self.n_items > 1:
                st = counts[2 * n_levels + 8 + _lib.MAX_BATCH * i:][: self.n_items]
                if any(v < 0 for v in st):
                    raise ImfError("batched pyramid: an item has no voxel")
                lv.items = [(st[b], (st[b + 1] if b + 1 < self.n_items else lv.n) - st[b]) for b in range(self.n_items)]
            else:
                lv.items = [(0, lv.n)]
        self._levels = levels
        return levels


def pyramid_from_points(xyz, voxel_size, n_levels=4, batch_index=0, inputs_ready=False, before_sync=None):
    """Voxelise + coarse levels in ONE library call on the geometry stream, then one event
    synchronisation for the row counts.  xyz: CUDA [N,3] f64/f32 tensor.  `inputs_ready`: xyz is
    known to be complete (e.g. resident data), so the geometry stream need not wait for the main one.
    Returns the list of levels (n set) -- buffers are safe to use on the current stream."""
    fut = PyramidFuture(xyz, voxel_size, n_levels, batch_index, inputs_ready)
    if before_sync is not None:
        before_sync()
    return fut.result()


class Rulebook:
    """Tiled kernel map (see include/imfnet_hip.h)."""
    __slots__ = ("tile_rows", "nbr", "tile_mask", "n_slots", "n_out", "kvol", "max_active")

    def __init__(self, tile_rows, nbr, tile_mask, n_slots, n_out, kvol, max_active=None):
        self.tile_rows, self.nbr, self.tile_mask = tile_rows, nbr, tile_mask
        self.n_slots, self.n_out, self.kvol = n_slots, n_out, kvol
        self.max_active = kvol if max_active is None else max_active   # active offsets per tile


def _new_table(n, device):
    L = _lib.lib()
    cap = L.imf_hash_capacity(n)
    table = torch.empty((cap, 2), dtype=torch.int64, device=device)      # struct imf_slot {u64 key; i32 val; i32 pad}
    ws = torch.empty(L.imf_unique_workspace_bytes(n), dtype=torch.uint8, device=device)
    return cap, table, ws


def new_meta(n_levels, device):
    """Zeroed [n_levels, 2] int32 block of (row count, error flag) words: ONE D2H copy reads every
    level's count back."""
    return torch.zeros((n_levels, 2), dtype=torch.int32, device=device)


def voxelize(xyz, voxel_size, batch_index=0, meta=None):
    """util/misc.py:82-87 on the GPU.  xyz: CUDA [N,3] float64 or float32.  Asynchronous: the
    returned Level has n=None until `sync_levels` reads the counts back."""
    if xyz.dtype not in (torch.float64, torch.float32):
        raise ImfError(f"xyz must be float64/float32, got {xyz.dtype}")
    _req(xyz, xyz.dtype, "xyz", 2)
    n, dev = xyz.shape[0], xyz.device
    if n == 0 or xyz.shape[1] != 3:
        raise ImfError(f"xyz must be [N>0, 3], got {tuple(xyz.shape)}")
    cap, table, ws = _new_table(n, dev)
    coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev)
    if meta is None:
        meta = torch.zeros(2, dtype=torch.int32, device=dev)       # [m, err]
    check(_lib.lib().imf_voxelize(xyz.data_ptr(), int(xyz.dtype == torch.float64), n, float(voxel_size),
                                  int(batch_index), coords.data_ptr(), first.data_ptr(),
                                  meta[0:1].data_ptr(), table.data_ptr(), cap,
                                  ws.data_ptr(), meta[1:2].data_ptr(), _stream()), "imf_voxelize")
    lv = Level(coords, meta, table, cap, 1, first)
    return lv


def downsample(level, out_stride, n_in_max=None, meta=None):
    """coordinate_manager.stride(): level at tensor stride `out_stride` (asynchronous)."""
    n_max = int(n_in_max if n_in_max is not None else level.n)
    dev = level.device
    cap, table, ws = _new_table(n_max, dev)
    coords = torch.empty((n_max, 4), dtype=torch.int32, device=dev)
    m = meta if meta is not None else torch.zeros(2, dtype=torch.int32, device=dev)   # [m, unused]
    check(_lib.lib().imf_downsample(level.coords_buf.data_ptr(), level.n_dev.data_ptr(), n_max,
                                    int(out_stride), coords.data_ptr(), m.data_ptr(), table.data_ptr(),
                                    cap, ws.data_ptr(), _stream()), "imf_downsample")
    return Level(coords, m, table, cap, out_stride)


def level_from_coords(coords):
    """Coordinate map of caller-supplied int32 (b,x,y,z) rows (ME.SparseTensor(coordinates=...),
    util/misc.py:95).  Duplicates collapse to their first occurrence."""
    _req(coords, torch.int32, "coordinates", 2)
    n = coords.shape[0]
    n_dev = torch.tensor([n, 0], dtype=torch.int32, device=coords.device)
    src = Level(coords, n_dev, None, 0, 1)
    src.n = n
    lv = downsample(src, 1)
    lv.ts = 1
    return lv


def sync_levels(levels, meta_block=None):
    """One host synchronisation: read the row counts of `levels` back.  `meta_block`: the shared
    [n,2] count block whose row i belongs to levels[i] (one contiguous D2H copy)."""
    if meta_block is not None:
        counts = meta_block[: len(levels)].cpu().reshape(-1).tolist()
    else:
        counts = torch.cat([lv.n_dev.reshape(-1)[:2] for lv in levels]).cpu().tolist()   # [m, err] per level
    for i, lv in enumerate(levels):
        if counts[2 * i + 1] != 0:
            raise ImfError("voxelize: a coordinate fell outside [-2^17, 2^17) voxels (or was NaN)")
        lv.n = int(counts[2 * i])


def rulebook_conv(in_level, out_level, ksize):
    """Kernel map of ME.MinkowskiConvolution(kernel_size=ksize) from in_level to out_level."""
    L = _lib.lib()
    n_out, dev = out_level.n, out_level.device
    kvol = ksize ** 3
    n_slots = L.imf_rulebook_slots(n_out)
    tile_rows = torch.empty(n_slots, dtype=torch.int32, device=dev)
    nbr = torch.empty(kvol * n_slots, dtype=torch.int32, device=dev)
    mask = torch.empty(n_slots // TILE_ROWS * MASK_WORDS, dtype=torch.int32, device=dev)
    check(L.imf_rulebook_conv(in_level.table.data_ptr(), in_level.capacity,
                              out_level.coords_buf.data_ptr(), n_out, in_level.ts, ksize,
                              tile_rows.data_ptr(), nbr.data_ptr(), mask.data_ptr(), _stream()),
          "imf_rulebook_conv")
    return Rulebook(tile_rows, nbr, mask, n_slots, n_out, kvol)


def rulebook_sorted(rb):
    """imf_rulebook_sort_by_occupancy: the occupancy-sorted twin of a stride-1 map in identity slot order (same rows, same
    inputs, tiles of rows with similar neighbour masks: fewer active (tile, offset) pairs for imf_spconv_fwd to walk)."""
    L = _lib.lib()
    dev = rb.nbr.device
    tile_rows = torch.empty(rb.n_slots, dtype=torch.int32, device=dev)
    nbr = torch.empty(rb.kvol * rb.n_slots, dtype=torch.int32, device=dev)
    mask = torch.empty(rb.n_slots // TILE_ROWS * MASK_WORDS, dtype=torch.int32, device=dev)
    ws = torch.empty(L.imf_rulebook_sorted_workspace_bytes(rb.n_slots), dtype=torch.uint8, device=dev)
    check(L.imf_rulebook_sort_by_occupancy(rb.nbr.data_ptr(), rb.kvol, rb.n_slots, rb.n_out, None, tile_rows.data_ptr(),
                                           nbr.data_ptr(), mask.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "imf_rulebook_sort_by_occupancy")
    return Rulebook(tile_rows, nbr, mask, rb.n_slots, rb.n_out, rb.kvol, rb.max_active)


def rulebook_transpose(coarse_level, fine_level, ksize=3):
    """Kernel map of ME.MinkowskiConvolutionTranspose(kernel_size=3, stride=2): coarse -> fine."""
    L = _lib.lib()
    n_fine, dev = fine_level.n, fine_level.device
    kvol = ksize ** 3
    n_slots = L.imf_rulebook_transpose_slots(n_fine)
    tile_rows = torch.empty(n_slots, dtype=torch.int32, device=dev)
    nbr = torch.empty(kvol * n_slots, dtype=torch.int32, device=dev)
    mask = torch.empty(n_slots // TILE_ROWS * MASK_WORDS, dtype=torch.int32, device=dev)
    counters = torch.empty(16, dtype=torch.int32, device=dev)
    check(L.imf_rulebook_transpose(coarse_level.table.data_ptr(),
                                   coarse_level.capacity, fine_level.coords_buf.data_ptr(), n_fine,
                                   fine_level.ts, ksize, tile_rows.data_ptr(), nbr.data_ptr(),
                                   mask.data_ptr(), n_slots, counters.data_ptr(), _stream()),
          "imf_rulebook_transpose")
    return Rulebook(tile_rows, nbr, mask, n_slots, n_fine, kvol, max_active=8)


def rulebook_identity(n_out, device):
    """kvol == 1 (pointwise) 'rulebook': slot == row, one active offset; nothing to build."""
    return Rulebook(None, None, None, _lib.lib().imf_rulebook_slots(n_out), n_out, 1)


# Sparse-conv arithmetic used by the model layers (include/imfnet_hip.h, imf_conv_args.variant; env IMF_CONV_VARIANT):
#   3 (default since round 5) = "bf16x3": every fp32 operand as three bf16 parts (exact), six bf16 MFMAs per 32 channels,
#       fp32 accumulation -- fp32 operand precision and range on the 16-bit matrix pipe, fp32 buffers, no range guard;
#   6 = split-f16 MFMA: two f16 parts per operand (22 bits), three MFMAs, operand images between layers, ~27 % faster,
#       activations must stay below 65504 (IMF_FLAG_RANGE -> the fragment is redone on variant 0): the FAST mode;
#   0 = fp32 MFMA (v_mfma_f32_16x16x4_f32): the reference's own arithmetic, ~1.6x slower than 3.
CONV_VARIANT = int(os.environ.get("IMF_CONV_VARIANT", "3"))
MAX_PIPELINED_KVOL = 27


def conv_variant_for(kvol):
    """Variants 6 and 3 need kvol <= 27 (their 16-bit weight images are only read by the LDS-DMA kernels)."""
    return CONV_VARIANT if (CONV_VARIANT not in (6, 3) or kvol <= MAX_PIPELINED_KVOL) else 0


def pack_weights(kernel, out=None, split16=False, variant=None):
    """ME kernel tensor [kvol,cin,cout] (or [cin,cout]) -> MFMA fragment-major image: fp32 B
    fragments (variants 0 and 1), with split16 / variant=6 the hi/lo f16 fragments of variant 6 (same size + trailer), with
    variant=3 the three bf16 parts of variant 3 (1.5 x the size)."""
    if variant is not None:
        split16 = variant == 6
    k = kernel.detach()
    if k.dim() == 2:
        k = k.unsqueeze(0)
    k = _req(k.contiguous().float(), torch.float32, "kernel", 3)
    kvol, cin, cout = k.shape
    L = _lib.lib()
    b3 = variant == 3
    need = (L.imf_packed_weight_floats_bf16x3 if b3 else L.imf_packed_weight_floats_split16 if split16
            else L.imf_packed_weight_floats)(kvol, cin, cout)
    packed = out if out is not None else torch.empty(need, dtype=torch.float32, device=k.device)
    if packed.numel() < need:
        raise ImfError(f"packed weight buffer has {packed.numel()} floats, needs {need}")
    fn = L.imf_pack_weights_bf16x3 if b3 else L.imf_pack_weights_split16 if split16 else L.imf_pack_weights
    check(fn(k.data_ptr(), kvol, cin, cout, packed.data_ptr(), _stream()), "imf_pack_weights")
    return packed


# `staging` of spconv -> imf_conv_args.kernel_tag (IMF_TAG_* of include/imfnet_hip.h say what each bit selects)
STAGING_TAGS = {
    None: 0, "dma": 0,                                   # the library default: the LDS-DMA kernel k_spconv_g
    "regs": _lib.TAG_REGS,                               # variant 0: the register-staged k_spconv_mfma
    "wave8": _lib.TAG_WAVE8, "wave4": _lib.TAG_WAVE4,    # the wave-split kernel k_spconv_w, whole tiles
    "wave8u": _lib.TAG_WAVE8 | _lib.TAG_U48, "wave4u": _lib.TAG_WAVE4 | _lib.TAG_U48,                   # 48-row units
    "wave4h": _lib.TAG_WAVE4 | _lib.TAG_HALF,                                                           # half tiles (bf16x3)
    "wave4o": _lib.TAG_WAVE4 | _lib.TAG_OCC,             # bf16x3: the builds for one more wavefront per SIMD
    "wave4h4": _lib.TAG_WAVE4 | _lib.TAG_HALF | _lib.TAG_OCC, "wave8h4": _lib.TAG_WAVE8 | _lib.TAG_HALF | _lib.TAG_OCC,
}
_WAVE = _lib.TAG_WAVE8 | _lib.TAG_WAVE4


def conv_kernel_name(variant, cin, cout, staging=None, kernel_tag=0):
    """Label of the kernel family a launch runs on (bench.py groups by it).  Variant 0 (fp32 MFMA) runs on the LDS-DMA
    kernels too since round 5 (AR = kArF32, csrc/spconv_g.hip / spconv_w.hip): same family names with an `/f32` suffix;
    TAG_REGS / staging="regs" selects the register-staged k_spconv_mfma.  The strings are a recorded contract
    (tests/golden/conv_kernel_names.json) -- including that a `staging` name other than "wave8" reads `k_spconv_w<4>`."""
    if kernel_tag & _lib.TAG_HEAD:
        return "k_pointwise_head_b3" if variant == 3 else "k_pointwise_head"
    tag = kernel_tag | STAGING_TAGS.get(staging, 0)
    cb = 4 if cout % 64 == 0 else 2
    if variant not in (0, 3, 6) or (variant == 0 and tag & _lib.TAG_REGS):
        return f"k_spconv_mfma<{cb},{4 if cin % 64 == 0 else 2}>"
    suffix = {0: "/f32", 3: "/b3"}.get(variant, "")
    if tag & _WAVE:
        return f"k_spconv_w<{8 if (kernel_tag & _lib.TAG_WAVE8 or staging == 'wave8') else 4}>" + suffix
    return f"k_spconv_g<{cb}, 0>" + suffix


FMT_A_SPLIT, FMT_RES_SPLIT, FMT_OUT_SPLIT = 1, 2, 4      # imf_conv_args.operand_format (include/imfnet_hip.h)
CONV_ROW_WINDOW = 0x7FFFF000                             # IMF_CONV_ROW_WINDOW: bytes of an input the LDS-DMA kernels can gather from


def to_operand_image(x):
    """fp32 [n, c] (c % 32 == 0) -> the split-f16 operand image of the same shape and dtype (bytes reinterpreted): per row
    and 32-channel chunk [4 hi pieces | 4 lo pieces], piece j = the 8 halves of channels {4j..4j+3, 16+4j..16+4j+3},
    hi = f16(x), lo = f16(x - hi) (include/imfnet_hip.h, imf_conv_args.operand_format)."""
    n, c = x.shape
    v = x.view(n, c // 32, 2, 4, 4).permute(0, 1, 3, 2, 4).reshape(n, c // 32, 32)      # [.., j, half, t]
    hi = v.to(torch.float16)
    lo = (v - hi.to(torch.float32)).to(torch.float16)
    return torch.cat([hi, lo], dim=-1).contiguous().view(torch.float32).view(n, c)


def from_operand_image(img):
    """The values an operand image carries: hi + lo in fp32 (22 significant bits of the original)."""
    n, c = img.shape
    h = img.contiguous().view(torch.float16).view(n, c // 32, 2, 32).to(torch.float32)
    v = (h[:, :, 0] + h[:, :, 1]).view(n, c // 32, 4, 2, 4).permute(0, 1, 3, 2, 4)
    return v.reshape(n, c).contiguous()


def spconv(in_a, w_packed, cout, rb, in_b=None, scale=None, shift=None, residual=None,
           relu=False, l2norm=False, out=None, split_k=0, variant=0, flags=None, staging=None,
           operand_format=0, n_out_dev=None, slots_extra=0):
    """out[o] = epilogue(sum_k in[nbr[k][o]] @ W[k]) -- imf_spconv_fwd.  `operand_format` (variant 6, unsplit): FMT_A_SPLIT
    | FMT_RES_SPLIT | FMT_OUT_SPLIT -- which of in_a / in_b, residual, out are split-f16 operand images
    (`to_operand_image`) instead of fp32 rows.  `flags`: optional int32[1] device word that
    receives IMF_FLAG_RANGE (32) when an output is NaN or >= 65504 in magnitude.  `staging`: a key of STAGING_TAGS --
    None / "dma" = the library default (LDS-DMA kernel k_spconv_g), "wave*" = a workgroup shape of the wave-split kernel
    for coarse levels (csrc/spconv_w.hip; kvol > 1, cout % 64 == 0, no split-K); "regs" = variant 0's register-staged
    k_spconv_mfma (variants 6 / 3 have none: IMF_EUNSUPPORTED / IMF_EINVAL).  `n_out_dev`: capacity mode -- int32[1]
    device word with the actual row count; `rb`'s tables and `out` are sized for capacities, `slots_extra` = slots the map
    lays out beyond roundup64(rows) (512 for transposed maps); the launch must be unsplit (split_k=1)."""
    _req(in_a, torch.float32, "in_a", 2)
    if in_b is not None:
        _req(in_b, torch.float32, "in_b", 2)
    if out is None:
        out = torch.empty((rb.n_out, cout), dtype=torch.float32, device=in_a.device)
    a = ConvArgs()
    a.in_a, a.in_b = in_a.data_ptr(), _ptr(in_b)
    a.c_a, a.c_b = in_a.shape[1], (0 if in_b is None else in_b.shape[1])
    a.w_packed, a.kvol, a.cout = w_packed.data_ptr(), rb.kvol, cout
    a.tile_rows, a.nbr, a.tile_mask = _ptr(rb.tile_rows), _ptr(rb.nbr), _ptr(rb.tile_mask)
    a.n_slots, a.n_out = rb.n_slots, rb.n_out
    a.scale, a.shift, a.residual = _ptr(scale), _ptr(shift), _ptr(residual)
    a.relu, a.l2norm = int(bool(relu)), int(bool(l2norm))
    a.out = out.data_ptr()
    L = _lib.lib()
    split = 1 if variant == 1 else (int(split_k) if split_k else L.imf_spconv_auto_split(rb.n_slots, cout, rb.max_active))
    if staging not in STAGING_TAGS:
        raise ImfError(f"spconv: staging={staging!r}")
    a.kernel_tag = STAGING_TAGS[staging]
    if rb.kvol == 1 or a.kernel_tag & _WAVE:
        split = 1
    a.split_k, a.variant = split, int(variant)
    a.operand_format = int(operand_format)
    a.dyn_err = None if flags is None else flags.data_ptr()
    ws = None
    nbytes = L.imf_spconv_workspace_bytes(rb.n_slots, cout, split)   # split-K partials
    if nbytes:
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=in_a.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    if n_out_dev is not None:
        _req(n_out_dev, torch.int32, "n_out_dev", 1)
        a.n_out_dev, a.slots_extra = n_out_dev.data_ptr(), int(slots_extra)
    # IMF_CONV_ROW_WINDOW: the LDS-DMA kernels read a row whose bytes lie at or beyond this offset as zeros, silently
    big = max(in_a.numel(), 0 if in_b is None else in_b.numel()) * 4 > CONV_ROW_WINDOW
    if variant in (6, 3) and big:
        raise ImfError("variants 6 / 3 address their inputs through a buffer window of 0x7FFFF000 bytes (2 GiB - 4 KiB): "
                       "use variant 0 for larger matrices")
    if variant == 0 and big:
        a.kernel_tag = _lib.TAG_REGS                      # the LDS-DMA kernels share that window: the register-staged kernel
    need = (L.imf_packed_weight_floats_split16 if variant == 6 else L.imf_packed_weight_floats_bf16x3 if variant == 3
            else L.imf_packed_weight_floats)(rb.kvol, a.c_a + a.c_b, cout)
    if w_packed.numel() != need:
        raise ImfError(f"packed weight has {w_packed.numel()} floats, expected {need} "
                       f"({rb.kvol}x{a.c_a + a.c_b}x{cout}, variant {variant})")
    ev = None
    if TRACE is not None:
        ev = _Ev()
        a.ev_begin, a.ev_end = ev.begin, ev.end
    check(L.imf_spconv_fwd(C.byref(a), _stream()), "imf_spconv_fwd")
    if ev is not None:
        cin = a.c_a + a.c_b
        TRACE.append(dict(kernel=conv_kernel_name(variant, cin, cout, staging),
                          kvol=rb.kvol, cin=cin, cout=cout, rb=rb, split=split, ev=ev))
    return out


def pointwise_head(in_a, in_b, w1_packed, w2_packed, scale1=None, shift1=None, relu1=True, scale2=None, shift2=None,
                   l2norm=True, out=None, flags=None, n_dev=None, a_split=False, variant=6):
    """imf_pointwise_head: conv1_tr + norm1_tr + ReLU + final + L2 normalisation (model/resunet.py:219-233) in one
    launch.  a_split: in_a / in_b are split-f16 operand images (`to_operand_image`).  in_a [n, c_a], in_b [n, c_b] or None; weight images from pack_weights_split16 (kvol 1); hidden width 64,
    output [n, 32].  Bit-identical to two `spconv(..., variant=6)` calls.  variant=3: bf16x3 weight images
    (`pack_weights(..., variant=3)`), fp32 rows, at most 96 input channels, no range flag -- bit-identical to two
    `spconv(..., variant=3)` calls."""
    _req(in_a, torch.float32, "in_a", 2)
    if in_b is not None:
        _req(in_b, torch.float32, "in_b", 2)
        if in_b.shape[0] != in_a.shape[0]:
            raise ImfError("pointwise_head: in_a / in_b row mismatch")
    n = in_a.shape[0]
    if out is None:
        out = torch.empty((n, 32), dtype=torch.float32, device=in_a.device)
    a = HeadArgs()
    a.in_a, a.in_b = in_a.data_ptr(), _ptr(in_b)
    a.c_a, a.c_b = in_a.shape[1], (0 if in_b is None else in_b.shape[1])
    L = _lib.lib()
    if variant not in (3, 6):
        raise ImfError(f"pointwise_head: variant={variant} (6 = split-f16 images, 3 = bf16x3 images)")
    floats = L.imf_packed_weight_floats_bf16x3 if variant == 3 else L.imf_packed_weight_floats_split16
    if w1_packed.numel() != floats(1, a.c_a + a.c_b, 64) or w2_packed.numel() != floats(1, 64, 32):
        raise ImfError("pointwise_head: packed weight images do not match [c_a + c_b, 64] / [64, 32] of this variant")
    a.w1_packed, a.scale1, a.shift1, a.relu1, a.c_mid = w1_packed.data_ptr(), _ptr(scale1), _ptr(shift1), int(bool(relu1)), 64
    a.w2_packed, a.scale2, a.shift2, a.l2norm, a.c_out = w2_packed.data_ptr(), _ptr(scale2), _ptr(shift2), int(bool(l2norm)), 32
    a.n, a.n_dev, a.out = n, _ptr(n_dev), out.data_ptr()
    a.a_split = int(bool(a_split))
    a.variant = int(variant)
    a.flags = None if flags is None else flags.data_ptr()
    check(L.imf_pointwise_head(C.byref(a), _stream()), "imf_pointwise_head")
    return out


def spconv_small_cin(feat, kernel, rb, scale=None, shift=None, relu=False):
    """First-layer conv for cin <= 4 (unpacked ME kernel [kvol,cin,cout])."""
    _req(feat, torch.float32, "feat", 2)
    k = _req(kernel.detach().contiguous(), torch.float32, "kernel", 3)
    kvol, cin, cout = k.shape
    if feat.shape[1] != cin or kvol != rb.kvol:
        raise ImfError("spconv_small_cin: feature / kernel / rulebook mismatch")
    out = torch.empty((rb.n_out, cout), dtype=torch.float32, device=feat.device)
    check(_lib.lib().imf_spconv_small_cin(feat.data_ptr(), cin, k.data_ptr(), kvol, cout,
                                          rb.nbr.data_ptr(), rb.n_slots, rb.n_out, _ptr(scale),
                                          _ptr(shift), int(bool(relu)), out.data_ptr(), _stream()),
          "imf_spconv_small_cin")
    return out


def conv_first_fused(level, feat, kernel, ksize, scale=None, shift=None, relu=False):
    """First-layer conv fused with its kernel map (imf_conv_first_fused).  feat None = all ones."""
    k = _req(kernel.detach().contiguous(), torch.float32, "kernel", 3)
    kvol, cin, cout = k.shape
    if kvol != ksize ** 3 or (feat is not None and feat.shape[1] != cin):
        raise ImfError("conv_first_fused: feature / kernel mismatch")
    if feat is not None:
        _req(feat, torch.float32, "feat", 2)
    out = torch.empty((level.n, cout), dtype=torch.float32, device=k.device)
    check(_lib.lib().imf_conv_first_fused(level.table.data_ptr(), level.capacity,
                                          level.coords_buf.data_ptr(), level.n, level.ts, ksize, _ptr(feat),
                                          cin, k.data_ptr(), cout, _ptr(scale), _ptr(shift), int(bool(relu)),
                                          out.data_ptr(), _stream()), "imf_conv_first_fused")
    return out


def conv_first_bitgrid(level, kernel, ksize, scale=None, shift=None, relu=False):
    """First-layer conv of the all-ones feature on an occupancy bit grid (imf_conv_first_bitgrid).
    Returns None when the level has no bounding box or the box is too large (use conv_first_fused)."""
    bbox = getattr(level, "bbox", None)
    if bbox is None:
        return None
    k = _req(kernel.detach().contiguous(), torch.float32, "kernel", 3)
    kvol, cin, cout = k.shape
    if cin != 1 or kvol != ksize ** 3:
        raise ImfError("conv_first_bitgrid: needs a [ksize^3, 1, cout] kernel")
    L = _lib.lib()
    box = (C.c_int32 * 8)(*bbox)
    words = L.imf_bitgrid_words(box, ksize)
    if words == 0:
        return None
    grid = torch.empty(words, dtype=torch.int32, device=k.device)
    out = torch.empty((level.n, cout), dtype=torch.float32, device=k.device)
    check(L.imf_conv_first_bitgrid(level.coords_buf.data_ptr(), level.n, box, ksize, grid.data_ptr(), words,
                                   k.data_ptr(), cout, _ptr(scale), _ptr(shift), int(bool(relu)),
                                   out.data_ptr(), _stream()), "imf_conv_first_bitgrid")
    return out


class FusionKernelWeights:
    """Packed weights of the bottleneck fusion block for imf_fusion_attention (built once per model)."""

    def __init__(self, attention_fusion, variant=None):
        """variant: the arithmetic of the owning model's convolutions (None: the process default) -- picks the 16-bit image of
        the two feed-forward matrices (bf16x3 for 3, split-f16 otherwise)."""
        from ._lib import FusionWeights
        variant = CONV_VARIANT if variant is None else int(variant)
        blk0, blk1 = attention_fusion.cross_attend_blocks
        att, ff = blk0.fn, blk1.fn.net
        self.dim, self.inner, self.hidden = att.to_q.in_features, att.to_q.out_features, ff[2].in_features
        self.scale = float(att.scale)
        self.supported = (att.heads == 1 and len(attention_fusion.layers) == 0 and self.dim == 256 and
                          self.inner == 128 and self.hidden == 1024 and att.to_q.weight.is_cuda)
        if not self.supported:
            return
        f = lambda t: t.detach().float().contiguous()                     # noqa: E731
        # feed-forward on the split-f16 convolution kernels (include/imfnet_hip.h, imf_fusion_weights): W1^T with its
        # columns interleaved per 64-column slab as [32 values | 32 gates] (GEGLU epilogue), b1 likewise
        H = self.hidden
        j = torch.arange(H // 32).view(-1, 1, 1) * 32
        c = torch.arange(32).view(1, 1, -1)
        perm = (j + c + torch.tensor([0, H]).view(1, 2, 1)).reshape(-1).to(ff[0].weight.device)   # packed col -> torch row
        w1t = f(ff[0].weight)[perm].t().contiguous()                       # [256, 2048], packed column order
        self.t = dict(ln1_g=f(blk0.norm.weight), ln1_b=f(blk0.norm.bias), wq_p=pack_weights(f(att.to_q.weight).t()),
                      wo_p=pack_weights(f(att.to_out.weight).t()), bo=f(att.to_out.bias), ln2_g=f(blk1.norm.weight),
                      # (w1_p / w2_p: the image of the 16-bit variant the process runs -- split-f16 for 6, three bf16 parts for 3)
                      ln2_b=f(blk1.norm.bias), w1_p=pack_weights(w1t, variant=3 if variant == 3 else 6),
                      b1=f(ff[0].bias)[perm].contiguous(),
                      w2_p=pack_weights(f(ff[2].weight).t(), variant=3 if variant == 3 else 6), b2=f(ff[2].bias),
                      # the same two matrices as fp32 images: the feed-forward of the variant-0 (fp32 MFMA) recompute
                      w1_f32=pack_weights(w1t), w2_f32=pack_weights(f(ff[2].weight).t()))
        self.c = FusionWeights(**{k: v.data_ptr() for k, v in self.t.items()})


def fusion_attention_batched(x, items, kt_packed, v_packed, n_tokens, tokens_padded, fw, out=None, flags=None, variant=None):
    """Rows [row0, row0+rows) of x for every (row0, rows) in `items` attend to image b's packed K^T / V
    (lists, one per item): imf_fusion_attention_batched_v.  flags: device int32[1] that receives IMF_FLAG_RANGE when a
    value feeding an f16 operand leaves the f16 range (None: not observed); variant: arithmetic of the feed-forward (6
    split-f16, 0 fp32 MFMA; default: the process-wide CONV_VARIANT, so that the fp32 recompute is fp32 throughout)."""
    _req(x, torch.float32, "x", 2)
    if out is None:
        out = torch.empty_like(x)
    if variant is None:
        variant = CONV_VARIANT if CONV_VARIANT in (6, 3) else 0
    B = len(items)
    L = _lib.lib()
    r0 = (C.c_int64 * B)(*[int(a) for a, _ in items])
    rn = (C.c_int64 * B)(*[int(b) for _, b in items])
    kp = (C.c_void_p * B)(*[t.data_ptr() for t in kt_packed])
    vp = (C.c_void_p * B)(*[t.data_ptr() for t in v_packed])
    nbytes = L.imf_fusion_workspace_bytes(x.shape[0])
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device)
    check(L.imf_fusion_attention_batched_v(x.data_ptr(), B, r0, rn, kp, vp, int(n_tokens), int(tokens_padded),
                                           C.byref(fw.c), C.c_float(fw.scale), out.data_ptr(), ws.data_ptr(), nbytes,
                                           _ptr(flags), int(variant), _stream()), "imf_fusion_attention_batched")
    return out


def fusion_attention_dyn(x, n_dev, item_starts_dev, n_items, kt_packed, v_packed, n_tokens, tokens_padded, fw, out, flags,
                         variant=None):
    """Capacity mode of `fusion_attention_batched` (imf_fusion_attention_dyn_v): x and out [n_cap, 256], the row count in
    n_dev (device int32[1]) and the items' first rows in item_starts_dev (device int32[n_items]; the last item ends at the
    count).  Rows of `out` from the count on are not written.  flags: device int32[1], required -- bit 3 (value 8) for an
    item without rows, IMF_FLAG_RANGE as in the exact call."""
    _req(x, torch.float32, "x", 2)
    _req(out, torch.float32, "out", 2)
    if out.shape != x.shape or n_dev.dtype != torch.int32 or item_starts_dev.dtype != torch.int32 or \
            item_starts_dev.numel() < n_items or flags is None or flags.dtype != torch.int32:
        raise ImfError("fusion_attention_dyn: out as x; n_dev, item_starts_dev [n_items] and flags are device int32")
    if variant is None:
        variant = CONV_VARIANT if CONV_VARIANT in (6, 3) else 0
    B = int(n_items)
    L = _lib.lib()
    kp = (C.c_void_p * B)(*[t.data_ptr() for t in kt_packed])
    vp = (C.c_void_p * B)(*[t.data_ptr() for t in v_packed])
    nbytes = L.imf_fusion_workspace_bytes_cap(x.shape[0])
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=x.device)
    check(L.imf_fusion_attention_dyn_v(x.data_ptr(), x.shape[0], n_dev.data_ptr(), item_starts_dev.data_ptr(), B,
                                       flags.data_ptr(), kp, vp, int(n_tokens), int(tokens_padded), C.byref(fw.c),
                                       C.c_float(fw.scale), out.data_ptr(), ws.data_ptr(), nbytes, int(variant), _stream()),
          "imf_fusion_attention_dyn")
    return out


def fusion_attention(x, kt_packed, v_packed, n_tokens, tokens_padded, fw, out=None, flags=None, variant=None):
    """x [n,256] -> [n,256]: the fusion block for one image (attention kernel + the two feed-forward GEMMs on the conv
    kernels); flags / variant as in `fusion_attention_batched`."""
    return fusion_attention_batched(x, [(0, x.shape[0])], [kt_packed], [v_packed], n_tokens, tokens_padded, fw, out=out,
                                    flags=flags, variant=variant)


# Training-mode BatchNorm of the sparse path (env IMF_TRAIN_NORM; python -m imfnet_amd.train --norm_kernels):
#   "torch" (default) = nn.BatchNorm1d, then the add, then F.relu: the op sequence sparse.MinkowskiBatchNorm always had;
#   "hip"             = csrc/norm_train.hip through autograd.SparseBatchNormFunction: fp64 statistics in a fixed order,
#                       ReLU and residual add folded in, bit-reproducible.  Used only in training mode under autograd on
#                       fp32 GPU features with affine parameters; every other call runs the torch ops whatever the switch.
# The same switch covers the InstanceNorm of the ResUNetIN2* residual blocks (sparse.MinkowskiInstanceNorm):
#   "torch" (default) = the torch ops it always ran (index_add_ sums, one host wait per call), then the add, then F.relu;
#   "hip"             = the imf_in_* calls of csrc/norm_train.hip through autograd.SparseInstanceNormFunction, in training,
#                       eval and no_grad alike (InstanceNorm is the same function in all three), on fp32 GPU rows whose
#                       coordinate manager knows the item partition; every other call runs the torch ops.
TRAIN_NORM_CHOICES = ("torch", "hip")
TRAIN_NORM = os.environ.get("IMF_TRAIN_NORM", "torch")
if TRAIN_NORM not in TRAIN_NORM_CHOICES:
    raise ImfError(f"IMF_TRAIN_NORM={TRAIN_NORM!r}: one of {', '.join(TRAIN_NORM_CHOICES)}")


def set_train_norm(name):
    """Sets the process-wide switch; returns the previous value."""
    global TRAIN_NORM
    if name not in TRAIN_NORM_CHOICES:
        raise ImfError(f"norm kernels {name!r}: one of {', '.join(TRAIN_NORM_CHOICES)}")
    prev, TRAIN_NORM = TRAIN_NORM, name
    return prev


def bn_train_chunk_rows():
    return _lib.lib().imf_bn_train_chunk_rows()


def _bn_workspace(n, c, device):
    nbytes = _lib.lib().imf_bn_train_workspace_bytes(n, c)
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device), nbytes


def _bn_rows(t, name, n, c):
    _req(t, torch.float32, name, 2)
    if tuple(t.shape) != (n, c):
        raise ImfError(f"{name} must be [{n}, {c}], got {tuple(t.shape)}")
    return t


def bn_train_forward(x, gamma, beta, eps, residual=None, relu=False, running_mean=None, running_var=None, momentum=0.0):
    """imf_bn_train_forward: (y [N, C] fp32, stats [2C] fp64 = batch mean, 1 / sqrt(biased variance + eps)).  The running
    statistics, when given, are updated in place."""
    _req(x, torch.float32, "x", 2)
    n, c = x.shape
    for name, t in (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var)):
        if t is not None and (_req(t, torch.float32, name, 1).shape[0] != c):
            raise ImfError(f"{name} must be [{c}]")
    if residual is not None:
        _bn_rows(residual, "residual", n, c)
    y = torch.empty_like(x)
    stats = torch.empty(2 * c, dtype=torch.float64, device=x.device)
    ws, nbytes = _bn_workspace(n, c, x.device)
    check(_lib.lib().imf_bn_train_forward(x.data_ptr(), n, c, gamma.data_ptr(), beta.data_ptr(), float(eps), _ptr(residual),
                                          int(bool(relu)), _ptr(running_mean), _ptr(running_var), float(momentum),
                                          y.data_ptr(), stats.data_ptr(), ws.data_ptr(), nbytes, _stream()),
          "imf_bn_train_forward")
    return y, stats


def bn_train_backward(dy, x, y, stats, gamma, relu=False, want_dx=True, want_dgamma=True, want_dbeta=True,
                      want_dresidual=False):
    """imf_bn_train_backward: (dx, dgamma, dbeta, dresidual), None for each output that is not wanted.  y is read only
    for the ReLU mask y > 0 (may be None when relu is false)."""
    _req(dy, torch.float32, "dy", 2)
    n, c = dy.shape
    _bn_rows(x, "x", n, c)
    if relu or y is not None:
        _bn_rows(y, "y", n, c)
    if _req(stats, torch.float64, "stats", 1).shape[0] != 2 * c or _req(gamma, torch.float32, "gamma", 1).shape[0] != c:
        raise ImfError(f"stats must be [{2 * c}] and gamma [{c}]")
    dx = torch.empty_like(x) if want_dx else None
    dgamma = torch.empty_like(gamma) if want_dgamma else None
    dbeta = torch.empty_like(gamma) if want_dbeta else None
    dres = torch.empty_like(x) if want_dresidual else None
    ws, nbytes = _bn_workspace(n, c, x.device)
    check(_lib.lib().imf_bn_train_backward(dy.data_ptr(), x.data_ptr(), _ptr(y), int(bool(relu)), stats.data_ptr(),
                                           gamma.data_ptr(), n, c, _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(dres),
                                           ws.data_ptr(), nbytes, _stream()), "imf_bn_train_backward")
    return dx, dgamma, dbeta, dres


def item_starts_tensor(items, device):
    """The host-side [(first row, rows)] of a level's batch items as the int32 [n_items + 1] device array the InstanceNorm
    calls take: one small upload, nothing waits for the device."""
    return torch.tensor([s for s, _ in items] + [items[-1][0] + items[-1][1]], dtype=torch.int32, device=device)


def _in_args(x, item_starts, name):
    _req(x, torch.float32, name, 2)
    n, c = x.shape
    if _req(item_starts, torch.int32, "item_starts", 1).device != x.device:
        raise ImfError(f"item_starts is on {item_starts.device}, {name} on {x.device}")
    n_items = item_starts.shape[0] - 1
    if not 1 <= n_items <= _lib.MAX_BATCH:
        raise ImfError(f"item_starts must be [n_items + 1] with 1 <= n_items <= {_lib.MAX_BATCH}, got {tuple(item_starts.shape)}")
    if n < 1:
        raise ImfError(f"{name} must have at least one row")
    return n, c, n_items


def _in_workspace(n, c, n_items, device):
    nbytes = _lib.lib().imf_in_workspace_bytes(n, c, n_items)
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device), nbytes


def in_forward(x, item_starts, gamma, beta, eps, residual=None, relu=False):
    """imf_in_forward: (y [N, C] fp32, stats [n_items, 2C] fp64 = per item the mean and 1 / sqrt(biased variance + eps)).
    item_starts: int32 [n_items + 1] on the device, item b = rows [item_starts[b], item_starts[b + 1]); never read here."""
    n, c, n_items = _in_args(x, item_starts, "x")
    for name, t in (("gamma", gamma), ("beta", beta)):
        if _req(t, torch.float32, name, 1).shape[0] != c:
            raise ImfError(f"{name} must be [{c}]")
    if residual is not None:
        _bn_rows(residual, "residual", n, c)
    y = torch.empty_like(x)
    stats = torch.empty((n_items, 2 * c), dtype=torch.float64, device=x.device)
    ws, nbytes = _in_workspace(n, c, n_items, x.device)
    check(_lib.lib().imf_in_forward(x.data_ptr(), n, c, item_starts.data_ptr(), n_items, gamma.data_ptr(), beta.data_ptr(),
                                    float(eps), _ptr(residual), int(bool(relu)), y.data_ptr(), stats.data_ptr(),
                                    ws.data_ptr(), nbytes, _stream()), "imf_in_forward")
    return y, stats


def in_backward(dy, x, y, stats, gamma, item_starts, relu=False, want_dx=True, want_dgamma=True, want_dbeta=True,
                want_dresidual=False):
    """imf_in_backward: (dx, dgamma, dbeta, dresidual), None for each output that is not wanted.  y is read only for the
    ReLU mask y > 0 (may be None when relu is false)."""
    n, c, n_items = _in_args(dy, item_starts, "dy")
    _bn_rows(x, "x", n, c)
    if relu or y is not None:
        _bn_rows(y, "y", n, c)
    if tuple(_req(stats, torch.float64, "stats", 2).shape) != (n_items, 2 * c) or \
            _req(gamma, torch.float32, "gamma", 1).shape[0] != c:
        raise ImfError(f"stats must be [{n_items}, {2 * c}] and gamma [{c}]")
    dx = torch.empty_like(x) if want_dx else None
    dgamma = torch.empty_like(gamma) if want_dgamma else None
    dbeta = torch.empty_like(gamma) if want_dbeta else None
    dres = torch.empty_like(x) if want_dresidual else None
    ws, nbytes = _in_workspace(n, c, n_items, x.device)
    check(_lib.lib().imf_in_backward(dy.data_ptr(), x.data_ptr(), _ptr(y), int(bool(relu)), stats.data_ptr(),
                                     gamma.data_ptr(), item_starts.data_ptr(), n, c, n_items, _ptr(dx), _ptr(dgamma),
                                     _ptr(dbeta), _ptr(dres), ws.data_ptr(), nbytes, _stream()), "imf_in_backward")
    return dx, dgamma, dbeta, dres


# The hardest-contrastive loss of training (env IMF_TRAIN_LOSS; python -m imfnet_amd.train --loss_kernels):
#   "torch" (default) = the torch ops of train/loss.py around two imf_nn_search calls, differentiated by torch's autograd;
#   "hip"             = csrc/loss.hip through autograd.HardestContrastiveLossFunction: fp64 terms summed in a fixed order,
#                       forward and backward, no floating-point atomics, no host wait, bit-reproducible.
TRAIN_LOSS_CHOICES = ("torch", "hip")
TRAIN_LOSS = os.environ.get("IMF_TRAIN_LOSS", "torch")
if TRAIN_LOSS not in TRAIN_LOSS_CHOICES:
    raise ImfError(f"IMF_TRAIN_LOSS={TRAIN_LOSS!r}: one of {', '.join(TRAIN_LOSS_CHOICES)}")


def set_train_loss(name):
    """Sets the process-wide switch; returns the previous value."""
    global TRAIN_LOSS
    if name not in TRAIN_LOSS_CHOICES:
        raise ImfError(f"loss kernels {name!r}: one of {', '.join(TRAIN_LOSS_CHOICES)}")
    prev, TRAIN_LOSS = TRAIN_LOSS, name
    return prev


def _hc_args(f0, f1, pairs, pos_sel, sel0, sel1):
    """Dtypes, shapes and devices of the loss's inputs (not the index values); the sizes and the workspace."""
    _req(f0, torch.float32, "f0", 2)
    _req(f1, torch.float32, "f1", 2)
    _req(pairs, torch.int64, "pairs", 2)
    _req(sel0, torch.int64, "sel0", 1)
    _req(sel1, torch.int64, "sel1", 1)
    if pos_sel is not None:
        _req(pos_sel, torch.int64, "pos_sel", 1)
    c = f0.shape[1]
    if f1.shape[1] != c or pairs.shape[1] != 2:
        raise ImfError(f"f1 must be [n1, {c}] and pairs [n_pairs, 2], got {tuple(f1.shape)} and {tuple(pairs.shape)}")
    for name, t in (("f1", f1), ("pairs", pairs), ("sel0", sel0), ("sel1", sel1), ("pos_sel", pos_sel)):
        if t is not None and t.device != f0.device:
            raise ImfError(f"{name} is on {t.device}, f0 on {f0.device}")
    n_pairs = pairs.shape[0]
    n_pos = n_pairs if pos_sel is None else pos_sel.shape[0]
    sizes = (f0.shape[0], f1.shape[0], c, n_pairs, n_pos, sel0.shape[0], sel1.shape[0])
    nbytes = _lib.lib().imf_hc_loss_workspace_bytes(*sizes)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=f0.device)
    return sizes, ws, nbytes


def _hc_call(fn, f0, f1, pairs, pos_sel, sel0, sel1, sizes, pos_thresh, neg_thresh, rest, ws, nbytes):
    n0, n1, c, n_pairs, n_pos, n_sel0, n_sel1 = sizes
    return fn(f0.data_ptr(), n0, f1.data_ptr(), n1, c, pairs.data_ptr(), n_pairs, _ptr(pos_sel), n_pos, sel0.data_ptr(),
              n_sel0, sel1.data_ptr(), n_sel1, float(pos_thresh), float(neg_thresh), *[t.data_ptr() for t in rest],
              ws.data_ptr(), nbytes, _stream())


def hc_loss_forward(f0, f1, pairs, pos_sel, sel0, sel1, pos_thresh, neg_thresh):
    """imf_hc_loss_forward: (loss fp32 [2] = (pos_loss, neg_loss), hard01, hard10 int64 [n_pos], keep01, keep10 uint8
    [n_pos], meta int32 [4] = (count of keep01, count of keep10, flags, 0)), all on the device; nothing waits for it.
    pos_sel None takes every pair in order."""
    sizes, ws, nbytes = _hc_args(f0, f1, pairs, pos_sel, sel0, sel1)
    n_pos, dev = sizes[4], f0.device
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    hard01 = torch.empty(n_pos, dtype=torch.int64, device=dev)
    hard10 = torch.empty(n_pos, dtype=torch.int64, device=dev)
    keep01 = torch.empty(n_pos, dtype=torch.uint8, device=dev)
    keep10 = torch.empty(n_pos, dtype=torch.uint8, device=dev)
    meta = torch.empty(4, dtype=torch.int32, device=dev)
    check(_hc_call(_lib.lib().imf_hc_loss_forward, f0, f1, pairs, pos_sel, sel0, sel1, sizes, pos_thresh, neg_thresh,
                   (loss, hard01, hard10, keep01, keep10, meta), ws, nbytes), "imf_hc_loss_forward")
    return loss, hard01, hard10, keep01, keep10, meta


def hc_loss_backward(f0, f1, pairs, pos_sel, sel0, sel1, pos_thresh, neg_thresh, hard01, hard10, keep01, keep10, meta,
                     grad, df0=None, df1=None):
    """imf_hc_loss_backward: (df0, df1) for the upstream gradients grad fp32 [2] (of pos_loss, neg_loss) on the device.
    df0 / df1 may be given; they are written whole."""
    sizes, ws, nbytes = _hc_args(f0, f1, pairs, pos_sel, sel0, sel1)
    n_pos = sizes[4]
    for name, t, dtype, n in (("hard01", hard01, torch.int64, n_pos), ("hard10", hard10, torch.int64, n_pos),
                              ("keep01", keep01, torch.uint8, n_pos), ("keep10", keep10, torch.uint8, n_pos),
                              ("meta", meta, torch.int32, 4), ("grad", grad, torch.float32, 2)):
        if _req(t, dtype, name, 1).shape[0] != n or t.device != f0.device:
            raise ImfError(f"{name} must be [{n}] on {f0.device}")
    df0 = torch.empty_like(f0) if df0 is None else _bn_rows(df0, "df0", *f0.shape)
    df1 = torch.empty_like(f1) if df1 is None else _bn_rows(df1, "df1", *f1.shape)
    check(_hc_call(_lib.lib().imf_hc_loss_backward, f0, f1, pairs, pos_sel, sel0, sel1, sizes, pos_thresh, neg_thresh,
                   (hard01, hard10, keep01, keep10, meta, grad, df0, df1), ws, nbytes), "imf_hc_loss_backward")
    return df0, df1


# The bottleneck attention-fusion block of training (env IMF_TRAIN_FUSION; python -m imfnet_amd.train --fusion_kernels):
#   "torch" (default) = model/fusion.py's torch ops, one batch item at a time, differentiated by torch's autograd;
#   "hip"             = csrc/fusion_train.hip through autograd.AttentionFusionFunction: all items in one call, fp32 MFMA
#                       products, sums over rows in a fixed chunk order, forward and backward, no floating-point
#                       atomics, no host wait, bit-reproducible.  Used only under autograd on fp32 GPU tensors of the one
#                       configuration IMFNet uses; every other call runs the torch ops whatever the switch.
TRAIN_FUSION_CHOICES = ("torch", "hip")
TRAIN_FUSION = os.environ.get("IMF_TRAIN_FUSION", "torch")
if TRAIN_FUSION not in TRAIN_FUSION_CHOICES:
    raise ImfError(f"IMF_TRAIN_FUSION={TRAIN_FUSION!r}: one of {', '.join(TRAIN_FUSION_CHOICES)}")


def set_train_fusion(name):
    """Sets the process-wide switch; returns the previous value."""
    global TRAIN_FUSION
    if name not in TRAIN_FUSION_CHOICES:
        raise ImfError(f"fusion kernels {name!r}: one of {', '.join(TRAIN_FUSION_CHOICES)}")
    prev, TRAIN_FUSION = TRAIN_FUSION, name
    return prev


FUSION_TRAIN_DIMS = (256, 128, 128, 1024)         # latent, context, inner, GEGLU hidden
FUSION_TRAIN_MAX_TOKENS = 320
FUSION_TRAIN_FLAG_STARTS = 1                      # IMF_FT_FLAG_STARTS of the meta word
# The block's 14 parameters in the order of the C ABI's IMF_FT_* indices: (name below AttentionFusion, shape)
FUSION_TRAIN_PARAMS = (
    ("cross_attend_blocks.0.norm.weight", (256,)), ("cross_attend_blocks.0.norm.bias", (256,)),
    ("cross_attend_blocks.0.norm_context.weight", (128,)), ("cross_attend_blocks.0.norm_context.bias", (128,)),
    ("cross_attend_blocks.0.fn.to_q.weight", (128, 256)), ("cross_attend_blocks.0.fn.to_kv.weight", (256, 128)),
    ("cross_attend_blocks.0.fn.to_out.weight", (256, 128)), ("cross_attend_blocks.0.fn.to_out.bias", (256,)),
    ("cross_attend_blocks.1.norm.weight", (256,)), ("cross_attend_blocks.1.norm.bias", (256,)),
    ("cross_attend_blocks.1.fn.net.0.weight", (2048, 256)), ("cross_attend_blocks.1.fn.net.0.bias", (2048,)),
    ("cross_attend_blocks.1.fn.net.2.weight", (256, 1024)), ("cross_attend_blocks.1.fn.net.2.bias", (256,)),
)


def fusion_train_chunk_rows():
    return _lib.lib().imf_fusion_train_chunk_rows()


def fusion_item_starts(batch_column, n_items):
    """int32 [n_items + 1] row starts of the items from the (ascending) batch column of the rows' coordinates, on the
    device: a searchsorted, no host wait."""
    col = batch_column.contiguous()
    edges = torch.arange(n_items + 1, dtype=col.dtype, device=col.device)
    return torch.searchsorted(col, edges).to(torch.int32)


def _fusion_train_args(x, starts, tokens, weights):
    _req(x, torch.float32, "x", 2)
    _req(tokens, torch.float32, "tokens", 3)
    _req(starts, torch.int32, "item_starts", 1)
    n, (n_items, T, ctx) = x.shape[0], tokens.shape
    latent, context, _, _ = FUSION_TRAIN_DIMS
    if x.shape[1] != latent or ctx != context:
        raise ImfError(f"x must be [n, {latent}] and tokens [items, T, {context}], got {tuple(x.shape)} and {tuple(tokens.shape)}")
    if not 1 <= T <= FUSION_TRAIN_MAX_TOKENS or n_items < 1:
        raise ImfError(f"tokens [items >= 1, 1 <= T <= {FUSION_TRAIN_MAX_TOKENS}, {context}], got {tuple(tokens.shape)}")
    if starts.shape[0] != n_items + 1:
        raise ImfError(f"item_starts must be [{n_items + 1}], got {tuple(starts.shape)}")
    if len(weights) != len(FUSION_TRAIN_PARAMS):
        raise ImfError(f"{len(FUSION_TRAIN_PARAMS)} weights in the order of ops.FUSION_TRAIN_PARAMS, got {len(weights)}")
    for t, (name, shape) in zip(weights, FUSION_TRAIN_PARAMS):
        if tuple(_req(t, torch.float32, name).shape) != shape:
            raise ImfError(f"{name} must be {shape}, got {tuple(t.shape)}")
    for name, t in (("tokens", tokens), ("item_starts", starts)) + tuple(zip((p[0] for p in FUSION_TRAIN_PARAMS), weights)):
        if t.device != x.device:
            raise ImfError(f"{name} is on {t.device}, x on {x.device}")
    wptr = (C.c_void_p * len(weights))(*[t.data_ptr() for t in weights])
    return n, n_items, T, wptr


def fusion_train_forward(x, item_starts, tokens, weights, z=None):
    """imf_fusion_train_forward: (z [n, 256], saved fp32 buffer, meta int32 [1]).  x [n, 256], item_starts int32
    [items + 1] on the device (fusion_item_starts), tokens [items, T, 128], weights: the 14 parameters in the order of
    FUSION_TRAIN_PARAMS.  meta[0] & FUSION_TRAIN_FLAG_STARTS: the starts were no partition of the rows; nothing here
    waits for it."""
    n, n_items, T, wptr = _fusion_train_args(x, item_starts, tokens, weights)
    L = _lib.lib()
    if z is None:
        z = torch.empty_like(x)
    elif tuple(_req(z, torch.float32, "z", 2).shape) != tuple(x.shape):
        raise ImfError(f"z must be {tuple(x.shape)}, got {tuple(z.shape)}")
    nbytes = L.imf_fusion_train_saved_bytes(n, n_items, T)
    saved = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=x.device)
    meta = torch.zeros(1, dtype=torch.int32, device=x.device)
    check(L.imf_fusion_train_forward(x.data_ptr(), n, item_starts.data_ptr(), n_items, tokens.data_ptr(), T,
                                     *FUSION_TRAIN_DIMS, wptr, z.data_ptr(), saved.data_ptr(), nbytes, meta.data_ptr(),
                                     _stream()), "imf_fusion_train_forward")
    return z, saved, meta


def fusion_train_backward(dz, x, item_starts, tokens, weights, saved, want_dx=True, want_dtokens=True, want=None,
                          outputs=None):
    """imf_fusion_train_backward: (dx, dtokens, [14 parameter gradients], meta); None for what is not wanted (`want`: 14
    booleans, default all).  `outputs` = (dx, dtokens, [14]) may hand in the tensors to write (None entries: not wanted)."""
    n, n_items, T, wptr = _fusion_train_args(x, item_starts, tokens, weights)
    if tuple(_req(dz, torch.float32, "dz", 2).shape) != tuple(x.shape) or dz.device != x.device:
        raise ImfError(f"dz must be {tuple(x.shape)} on {x.device}")
    L = _lib.lib()
    sbytes = L.imf_fusion_train_saved_bytes(n, n_items, T)
    if _req(saved, torch.float32, "saved", 1).shape[0] * 4 < sbytes or saved.device != x.device:
        raise ImfError(f"saved must hold {sbytes} bytes on {x.device}")
    if outputs is None:
        want = [True] * len(weights) if want is None else list(want)
        dx = torch.empty_like(x) if want_dx else None
        dtok = torch.empty_like(tokens) if want_dtokens else None
        grads = [torch.empty_like(t) if k else None for t, k in zip(weights, want)]
    else:
        dx, dtok, grads = outputs
        for name, t, ref in [("dx", dx, x), ("dtokens", dtok, tokens)] + [(p[0], g, t) for p, g, t in
                                                                         zip(FUSION_TRAIN_PARAMS, grads, weights)]:
            if t is not None and (tuple(_req(t, torch.float32, name).shape) != tuple(ref.shape) or t.device != x.device):
                raise ImfError(f"gradient of {name} must be {tuple(ref.shape)} on {x.device}")
    gptr = (C.c_void_p * len(grads))(*[_ptr(t) for t in grads])
    nbytes = L.imf_fusion_train_workspace_bytes(n, n_items, T)
    ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=x.device)
    meta = torch.zeros(1, dtype=torch.int32, device=x.device)
    check(L.imf_fusion_train_backward(dz.data_ptr(), x.data_ptr(), n, item_starts.data_ptr(), n_items, tokens.data_ptr(),
                                      T, *FUSION_TRAIN_DIMS, wptr, saved.data_ptr(), sbytes, _ptr(dx), _ptr(dtok), gptr,
                                      meta.data_ptr(), ws.data_ptr(), nbytes, _stream()), "imf_fusion_train_backward")
    return dx, dtok, grads, meta


# The descriptor head of training (env IMF_TRAIN_HEAD; python -m imfnet_amd.train --head_kernels):
#   "torch" (default) = ME.cat, conv1_tr, ReLU, final, torch.norm and the division: the op sequence forward_layers always
#                       had, differentiated by torch's autograd;
#   "hip"             = csrc/head_train.hip through autograd.HeadFunction: one forward and one backward call, the
#                       concatenation never built, fp32 MFMA products, the sums over a row's channels as fixed shuffle
#                       trees and the sums over rows in a fixed chunk order, no floating-point atomics, no host wait,
#                       bit-reproducible.  Used only in training mode under autograd on fp32 GPU rows of the one shape
#                       ResUNetBN2C has; every other call runs the torch ops whatever the switch.
TRAIN_HEAD_CHOICES = ("torch", "hip")
TRAIN_HEAD = os.environ.get("IMF_TRAIN_HEAD", "torch")
if TRAIN_HEAD not in TRAIN_HEAD_CHOICES:
    raise ImfError(f"IMF_TRAIN_HEAD={TRAIN_HEAD!r}: one of {', '.join(TRAIN_HEAD_CHOICES)}")


def set_train_head(name):
    """Sets the process-wide switch; returns the previous value."""
    global TRAIN_HEAD
    if name not in TRAIN_HEAD_CHOICES:
        raise ImfError(f"head kernels {name!r}: one of {', '.join(TRAIN_HEAD_CHOICES)}")
    prev, TRAIN_HEAD = TRAIN_HEAD, name
    return prev


HEAD_TRAIN_DIMS = (64, 32, 64, 32)                # cu (decoder rows), cs (the stride-1 skip), ch (hidden), co (descriptor)
HEAD_TRAIN_FLAG_NORM = 1                          # IMF_HT_FLAG_NORM of the meta word


def head_train_chunk_rows():
    return _lib.lib().imf_head_train_chunk_rows()


def _head_train_args(u, s, w1, w2, bias=None):
    """Dtypes, devices and shapes of the head's inputs; (n, cu, cs, ch, co).  The channel counts themselves are the
    library's to refuse."""
    _req(u, torch.float32, "u", 2)
    _req(s, torch.float32, "s", 2)
    _req(w1, torch.float32, "w1", 2)
    _req(w2, torch.float32, "w2", 2)
    n, cu, cs, (ch, co) = u.shape[0], u.shape[1], s.shape[1], w2.shape
    if s.shape[0] != n or tuple(w1.shape) != (cu + cs, ch):
        raise ImfError(f"s must be [{n}, cs] and w1 [{cu} + cs, {ch}], got {tuple(s.shape)} and {tuple(w1.shape)}")
    if bias is not None and tuple(_req(bias, torch.float32, "bias", 2).shape) != (1, co):
        raise ImfError(f"bias must be [1, {co}], got {tuple(bias.shape)}")
    for name, t in (("s", s), ("w1", w1), ("w2", w2), ("bias", bias)):
        if t is not None and t.device != u.device:
            raise ImfError(f"{name} is on {t.device}, u on {u.device}")
    return n, cu, cs, ch, co


def head_train_forward(u, s, w1, w2, bias, normalize=True, out=None):
    """imf_head_train_forward: (h [n, ch], r [n] or None without normalize, y [n, co], meta int32 [1]).  u [n, cu],
    s [n, cs], w1 [cu + cs, ch], w2 [ch, co], bias [1, co].  meta[0] & HEAD_TRAIN_FLAG_NORM: a row's norm was 0 or not
    finite; nothing here waits for it.  `out` = (h, r, y) may hand in the tensors to write."""
    n, cu, cs, ch, co = _head_train_args(u, s, w1, w2, bias)
    if out is None:
        h = torch.empty((n, ch), dtype=torch.float32, device=u.device)
        r = torch.empty((n,), dtype=torch.float32, device=u.device) if normalize else None
        y = torch.empty((n, co), dtype=torch.float32, device=u.device)
    else:
        h, r, y = out
        for name, t, shape in (("h", h, (n, ch)), ("r", r, (n,)), ("y", y, (n, co))):
            if t is not None and (tuple(_req(t, torch.float32, name).shape) != shape or t.device != u.device):
                raise ImfError(f"{name} must be {shape} on {u.device}")
    meta = torch.zeros(1, dtype=torch.int32, device=u.device)
    check(_lib.lib().imf_head_train_forward(_ptr(u), cu, _ptr(s), cs, n, w1.data_ptr(), ch, w2.data_ptr(), co,
                                            bias.data_ptr(), int(bool(normalize)), _ptr(h), _ptr(r), _ptr(y),
                                            meta.data_ptr(), _stream()), "imf_head_train_forward")
    return h, r, y, meta


def head_train_backward(dy, y, r, h, u, s, w1, w2, normalize=True, want=None, outputs=None):
    """imf_head_train_backward: (du, ds, dw1, dw2, dbias, meta); None for what is not wanted (`want`: 5 booleans in that
    order, default all).  `outputs` = (du, ds, dw1, dw2, dbias) may hand in the tensors to write (None: not wanted).
    Without normalize, y and r may be None."""
    n, cu, cs, ch, co = _head_train_args(u, s, w1, w2)
    shapes = ((n, cu), (n, cs), (cu + cs, ch), (ch, co), (1, co))
    names = ("du", "ds", "dw1", "dw2", "dbias")
    for name, t, shape in (("dy", dy, (n, co)), ("h", h, (n, ch))) + ((("y", y, (n, co)), ("r", r, (n,))) if normalize else ()):
        if tuple(_req(t, torch.float32, name).shape) != shape or t.device != u.device:
            raise ImfError(f"{name} must be {shape} on {u.device}")
    if outputs is None:
        want = [True] * 5 if want is None else list(want)
        outputs = [torch.empty(shape, dtype=torch.float32, device=u.device) if k else None for shape, k in zip(shapes, want)]
    else:
        for name, t, shape in zip(names, outputs, shapes):
            if t is not None and (tuple(_req(t, torch.float32, name).shape) != shape or t.device != u.device):
                raise ImfError(f"{name} must be {shape} on {u.device}")
    L = _lib.lib()
    nbytes = L.imf_head_train_workspace_bytes(n)
    ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=u.device)
    meta = torch.zeros(1, dtype=torch.int32, device=u.device)
    check(L.imf_head_train_backward(_ptr(dy), _ptr(y) if normalize else None, _ptr(r) if normalize else None, _ptr(h),
                                    _ptr(u), cu, _ptr(s), cs, n, w1.data_ptr(), ch, w2.data_ptr(), co,
                                    int(bool(normalize)), *[_ptr(t) for t in outputs], ws.data_ptr(), nbytes,
                                    meta.data_ptr(), _stream()), "imf_head_train_backward")
    return (*outputs, meta)


# The image encoder of training (env IMF_TRAIN_IMAGE; python -m imfnet_amd.train --image_kernels):
#   "torch" (default) = the torch modules of model/image_encoder.py (MIOpen / aten convolutions, BatchNorm2d, max pool),
#                       differentiated by torch's autograd;
#   "hip"             = the trunk on NHWC rows: autograd.DenseConvFunction (imf_spconv_fwd / imf_spconv_wgrad over the
#                       static pixel tables of csrc/image_train.hip), autograd.SparseBatchNormFunction with the block's
#                       ReLU and residual add folded in, autograd.MaxPoolRowsFunction: fixed summation orders, no
#                       floating-point atomics, bit-reproducible.  Used only in training mode under autograd on an fp32
#                       GPU image that needs no gradient; every other call runs the torch modules whatever the switch.
TRAIN_IMAGE_CHOICES = ("torch", "hip")
TRAIN_IMAGE = os.environ.get("IMF_TRAIN_IMAGE", "torch")
if TRAIN_IMAGE not in TRAIN_IMAGE_CHOICES:
    raise ImfError(f"IMF_TRAIN_IMAGE={TRAIN_IMAGE!r}: one of {', '.join(TRAIN_IMAGE_CHOICES)}")


def set_train_image(name):
    """Sets the process-wide switch; returns the previous value."""
    global TRAIN_IMAGE
    if name not in TRAIN_IMAGE_CHOICES:
        raise ImfError(f"image kernels {name!r}: one of {', '.join(TRAIN_IMAGE_CHOICES)}")
    prev, TRAIN_IMAGE = TRAIN_IMAGE, name
    return prev


def image_trunk_shapes(H, W):
    """((H2, W2), (H4, W4), (H8, W8)): the stem's, the pool's and layer2's maps of an H x W image."""
    down = lambda v, k, p: (v + 2 * p - k) // 2 + 1                         # noqa: E731
    h2, w2 = down(H, 7, 3), down(W, 7, 3)
    h4, w4 = down(h2, 3, 1), down(w2, 3, 1)
    return (h2, w2), (h4, w4), (down(h4, 3, 1), down(w4, 3, 1))


class ImageTrainTables:
    """The six static pixel tables of imf_image_train_tables_build for (B, H, W) images on `device`, each an
    `ops.Rulebook` over views of one storage tensor: t4, t48, t48T, td, tdT, t8 (include/imfnet_hip.h says what each is),
    plus `stem`, the identity 'rulebook' of the stem's pointwise convolution over the im2col rows."""

    def __init__(self, B, H, W, device):
        L = _lib.lib()
        nbytes = L.imf_image_train_tables_bytes(B, H, W)
        if nbytes == 0:
            raise ImfError(f"image tables: B={B} H={H} W={W} (B >= 1, H and W >= 8)")
        self.B, self.H, self.W = B, H, W
        self.shapes = image_trunk_shapes(H, W)
        self.storage = torch.empty(nbytes, dtype=torch.uint8, device=device)
        c = _lib.ImageTrainTables()
        with torch.cuda.device(self.storage.device):
            check(L.imf_image_train_tables_build(B, H, W, self.storage.data_ptr(), nbytes, C.byref(c), _stream()),
                  "imf_image_train_tables_build")
        base = self.storage.data_ptr()

        def view(addr, words):
            off = addr - base
            return self.storage[off:off + 4 * words].view(torch.int32)

        for name in _lib.IMAGE_TRAIN_TABLES:
            t = getattr(c, name)
            setattr(self, name, Rulebook(view(t.tile_rows, t.n_slots), view(t.nbr, t.kvol * t.n_slots),
                                         view(t.tile_mask, t.n_slots // TILE_ROWS * MASK_WORDS), t.n_slots, t.n_out, t.kvol))
        self.stem = rulebook_identity(B * self.shapes[0][0] * self.shapes[0][1], device)


def image_im2col7(image):
    """imf_image_im2col7: [B,3,H,W] fp32 -> the stem's patch matrix [B*H2*W2, 160]."""
    _req(image, torch.float32, "image", 4)
    B, ch, H, W = image.shape
    if ch != 3:
        raise ImfError(f"image must be [B,3,H,W], got {tuple(image.shape)}")
    (h2, w2), _, _ = image_trunk_shapes(H, W)
    out = torch.empty((B * h2 * w2, 160), dtype=torch.float32, device=image.device)
    with torch.cuda.device(image.device):
        check(_lib.lib().imf_image_im2col7(image.data_ptr(), B, H, W, out.data_ptr(), _stream()), "imf_image_im2col7")
    return out


def _pool_rows(t, dtype, name, rows, c):
    _req(t, dtype, name, 2)
    if tuple(t.shape) != (rows, c):
        raise ImfError(f"{name} must be [{rows}, {c}], got {tuple(t.shape)}")
    return t


def image_maxpool_forward(x, B, Hin, Win):
    """imf_image_maxpool_forward: NHWC rows x [B*Hin*Win, C] -> (out [B*Hout*Wout, C], tap uint8 of the same shape)."""
    c = x.shape[1] if torch.is_tensor(x) and x.dim() == 2 else 0
    _pool_rows(x, torch.float32, "x", B * Hin * Win, c)
    rows = B * ((Hin - 1) // 2 + 1) * ((Win - 1) // 2 + 1)
    out = torch.empty((rows, c), dtype=torch.float32, device=x.device)
    tap = torch.empty((rows, c), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().imf_image_maxpool_forward(x.data_ptr(), B, Hin, Win, c, out.data_ptr(), tap.data_ptr(), _stream()),
              "imf_image_maxpool_forward")
    return out, tap


def image_maxpool_backward(dout, tap, B, Hin, Win, din=None):
    """imf_image_maxpool_backward: din [B*Hin*Win, C], written whole (`din` may be given)."""
    c = dout.shape[1] if torch.is_tensor(dout) and dout.dim() == 2 else 0
    rows = B * ((Hin - 1) // 2 + 1) * ((Win - 1) // 2 + 1)
    _pool_rows(dout, torch.float32, "dout", rows, c)
    _pool_rows(tap, torch.uint8, "tap", rows, c)
    if din is None:
        din = torch.empty((B * Hin * Win, c), dtype=torch.float32, device=dout.device)
    else:
        _pool_rows(din, torch.float32, "din", B * Hin * Win, c)
    with torch.cuda.device(dout.device):
        check(_lib.lib().imf_image_maxpool_backward(dout.data_ptr(), tap.data_ptr(), B, Hin, Win, c, din.data_ptr(),
                                                    _stream()), "imf_image_maxpool_backward")
    return din


def dam_heat(out_prenorm, hidden, targets, accumulate=True, n_dev=None, heat=None):
    """imf_dam_heat (csrc/dam.hip): Descriptor Activation Mapping of T target rows at once.  out_prenorm [N, 32] = the
    output of `final` before normalisation, hidden [N, c_hid] = its input, targets int32 [T] on the device.  Returns
    (heat [T, N] fp32, minmax [T, 2] fp32, flags [T] int32, weights [T, 32] fp32); flags[t] = 1 (and a zero heat row) for
    a target outside the rows, with a zero or a non-finite pre-normalisation row.  n_dev (int32 [1]) caps the rows; `heat`
    may be given to be written in place (rows beyond n_dev are left as they are)."""
    _req(out_prenorm, torch.float32, "out_prenorm", 2)
    _req(hidden, torch.float32, "hidden", 2)
    _req(targets, torch.int32, "targets", 1)
    n, c_out = out_prenorm.shape
    c_hid = hidden.shape[1]
    if hidden.shape[0] != n:
        raise ImfError(f"hidden must have {n} rows, got {hidden.shape[0]}")
    if c_out != 32 or c_hid < 32 or c_hid % 32:
        raise ImfError(f"DAM supports c_out = 32 and c_hid a positive multiple of 32, got c_out={c_out} c_hid={c_hid}")
    T = targets.shape[0]
    if n_dev is not None:
        _req(n_dev, torch.int32, "n_dev")
    dev = out_prenorm.device
    if heat is None:
        heat = torch.empty((T, n), dtype=torch.float32, device=dev)
    elif tuple(_req(heat, torch.float32, "heat", 2).shape) != (T, n):
        raise ImfError(f"heat must be [{T}, {n}], got {tuple(heat.shape)}")
    minmax = torch.zeros((T, 2), dtype=torch.float32, device=dev)
    flags = torch.zeros(T, dtype=torch.int32, device=dev)
    weights = torch.zeros((T, 32), dtype=torch.float32, device=dev)
    if T:
        check(_lib.lib().imf_dam_heat(out_prenorm.data_ptr(), n, _ptr(n_dev), hidden.data_ptr(), c_hid, c_out,
                                      targets.data_ptr(), T, int(bool(accumulate)), weights.data_ptr(), heat.data_ptr(),
                                      minmax.data_ptr(), flags.data_ptr(), _stream()), "imf_dam_heat")
    return heat, minmax, flags, weights


# The optimizer step of training (env IMF_TRAIN_OPTIM; python -m imfnet_amd.train --optim_kernels):
#   "torch" (default) = torch.optim.SGD, and every differentiable convolution packs its weight images on every call;
#   "hip"             = train.optim.FusedSGD: one imf_sgd_step launch over every parameter (csrc/optim.hip), which also
#                       writes the two bf16x3 operand images of every packable convolution weight; `weight_image` hands
#                       them to autograd.SparseConvFunction / DenseConvFunction while the parameter's `_version` is the one
#                       the step left.  Torch does not move `_version` for writes through `.data` (`p.data.add_(1)`), so
#                       a parameter with images is watched for `.data` accesses as well (_WatchedParameter below).
TRAIN_OPTIM_CHOICES = ("torch", "hip")
TRAIN_OPTIM = os.environ.get("IMF_TRAIN_OPTIM", "torch")
if TRAIN_OPTIM not in TRAIN_OPTIM_CHOICES:
    raise ImfError(f"IMF_TRAIN_OPTIM={TRAIN_OPTIM!r}: one of {', '.join(TRAIN_OPTIM_CHOICES)}")


def set_train_optim(name):
    """Sets the process-wide switch; returns the previous value."""
    global TRAIN_OPTIM
    if name not in TRAIN_OPTIM_CHOICES:
        raise ImfError(f"optim kernels {name!r}: one of {', '.join(TRAIN_OPTIM_CHOICES)}")
    prev, TRAIN_OPTIM = TRAIN_OPTIM, name
    return prev


class WeightImages:
    """The image pair an optimizer keeps for one convolution weight: `fwd` / `bwd` (either may be None) hold the bf16x3
    images of the parameter as it was when its `_version` was `version`; `flip`: the backward image's taps are reversed."""
    __slots__ = ("ref", "shape", "fwd", "bwd", "flip", "version", "key")

    def __init__(self, param, fwd, bwd, flip):
        self.ref, self.shape, self.fwd, self.bwd, self.flip = weakref.ref(param), tuple(param.shape), fwd, bwd, bool(flip)
        self.version, self.key = -1, None


_WEIGHT_IMAGES = {}                               # parameter data_ptr -> WeightImages (train.optim.FusedSGD registers them)


_TENSOR_DATA = torch._C.TensorBase.data           # the `.data` descriptor every tensor inherits


class _WatchedParameter(torch.nn.Parameter):
    """The class of a parameter while an optimizer keeps images of it.  A write through `.data` moves no version counter
    (the tensor `.data` returns has one of its own), so `_version` alone would let `p.data.add_(1)` pass unseen.  Here
    every access to `.data`, read or assignment, marks the images stale until the next step -- conservative: whoever takes
    `.data` may write through it.  Nothing on the training path takes it (forward, backward, state_dict, load_state_dict,
    zero_grad, the step).  Still unseen: a write through a `.data` tensor taken BEFORE the step that wrote the images.
    isinstance(p, nn.Parameter) holds, pickling gives a plain Parameter (torch's own __reduce_ex__)."""

    @property
    def data(self):
        _data_taken(self)
        return _TENSOR_DATA.__get__(self)

    @data.setter
    def data(self, value):
        _data_taken(self)
        _TENSOR_DATA.__set__(self, value)


def _data_taken(param):
    for ent in _WEIGHT_IMAGES.values():
        if ent.ref() is param:
            ent.version = -1


def register_weight_images(param, images):
    images.key = param.data_ptr()
    _WEIGHT_IMAGES[images.key] = images
    if type(param) is torch.nn.Parameter:         # other subclasses keep their class (and the `.data` blind spot)
        param.__class__ = _WatchedParameter


def unregister_weight_images(images):
    for key in [k for k, v in _WEIGHT_IMAGES.items() if v is images]:
        del _WEIGHT_IMAGES[key]
    param = images.ref()
    if type(param) is _WatchedParameter and not any(e.ref() is param for e in _WEIGHT_IMAGES.values()):
        param.__class__ = torch.nn.Parameter


def weight_image(param, which, variant, flip=None):
    """The packed operand image of a convolution weight for the differentiable convolutions: `which` = "forward" (the
    image of the kernel itself) or "backward" (of the transposed kernel, its taps reversed when `flip`: the operand of the
    input gradient).  `param`: an ME kernel [kvol, cin, cout] / [cin, cout] or a torch weight [cout, cin, kh, kw].
    With ops.TRAIN_OPTIM == "hip" and variant 3, the image the optimizer wrote at its last step is returned while it is
    still the parameter's (same storage, same `_version`, `.data` not taken since); in every other case the weight is packed here, by the torch
    re-layout ops and the pack launch the convolutions always issued."""
    if which not in ("forward", "backward"):
        raise ImfError(f"weight_image: which={which!r}: 'forward' or 'backward'")
    ent = _WEIGHT_IMAGES.get(param.data_ptr()) if (TRAIN_OPTIM == "hip" and variant == 3 and _WEIGHT_IMAGES) else None
    if ent is not None and (ent.ref() is None or ent.shape != tuple(param.shape)):
        ent = None
    if ent is not None and ent.version == param._version:
        img = ent.fwd if which == "forward" else ent.bwd
        if img is not None and (which == "forward" or flip is None or bool(flip) == ent.flip):
            return img
    if which == "backward" and flip is None:
        if ent is None:
            raise ImfError("weight_image: the backward image of a weight no optimizer owns needs `flip`")
        flip = ent.flip
    return pack_weights(image_source(param, which, flip), variant=variant)


def image_source(param, which, flip=False):
    """The contiguous [kvol, cin', cout'] tensor whose packed image `weight_image` returns: the kernel itself ("forward"),
    or its transpose W'[k'][co][ci] = W[k][ci][co] with k' = kvol - 1 - k when `flip` ("backward")."""
    w = param.detach()
    if w.dim() == 4:
        co, ci, kh, kw = w.shape
        k3 = (w.float().permute(2, 3, 1, 0).reshape(kh * kw, ci, co) if which == "forward"
              else w.float().permute(2, 3, 0, 1).reshape(kh * kw, co, ci))
    else:
        k3 = w if w.dim() == 3 else w.unsqueeze(0)
        if which == "backward":
            k3 = k3.transpose(1, 2)
    if which == "backward" and flip:
        k3 = k3.flip(0)
    return k3.contiguous()
