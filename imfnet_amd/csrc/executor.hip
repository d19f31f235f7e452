// Native executor for the ResUNet layer schedule and for a whole fragment (host code only: no kernels here).
//
// The reference runs one fragment as ~100 Python-level MinkowskiEngine calls
// (model/resunet.py:163-235).  imf_resunet_forward walks the same schedule natively: rulebook
// builds on a side stream joined by events, the first convolution, the encoder, the fused bottleneck
// attention (after the image branch's event), the decoder and the head -- one call per fragment.
//
// Two modes:
//   exact     the row count of every level is known on the host (one D2H readback after the pyramid build);
//             arenas and grids are sized for exactly those rows.
//   capacity  (io->dyn) nothing is read back: arenas, rulebooks and grids are sized for CAPACITIES, the kernels
//             take the actual counts from the pyramid's device meta block.  Every convolution is an unsplit launch
//             in both modes (its kernel is a function of the level and the layer's channels only), and the one
//             choice that depends on the row count (the fusion block's hidden split) is made on the device with the
//             host's rule -- so a capacity-mode forward is bit-identical to the exact one.  Because every address,
//             grid and argument is then a function of the capacities only, the whole fragment
//             (imf_fragment_forward: pyramid + rulebooks + image branch + 23 convolutions + fusion) can be
//             captured ONCE per capacity bucket as a hipGraph and replayed with no host work but one launch.
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "geometry_internal.h"
#include "spconv_shared.h"

namespace imf {
namespace {

struct Rb {   // rulebook inside the int arena
  int32_t *tile_rows = nullptr, *nbr = nullptr;
  uint32_t *tile_mask = nullptr;
  int64_t n_slots = 0, n_out = 0;
  int kvol = 1;
  int level = 0;          // pyramid level of the OUTPUT rows (row count: meta[2 * level] in capacity mode)
  int slots_extra = 0;    // parity-class padding of transposed maps (slots beyond roundup64(rows))
  int side_piece = 0;     // the piece of the side chain that builds it (SideChain): 1 .. 3 = level, 4 = the tail, 0 = none
  int ready_event = -1;   // index into io->events that the main stream must wait on before first use
  // the map's shape, and its tables from byte address p on; returns the first byte behind them
  uintptr_t place(uintptr_t p, int64_t slots, int64_t rows, int kvol_, int level_, int side_piece_) {
    n_slots = slots; n_out = rows; kvol = kvol_; level = level_; side_piece = side_piece_;
    const size_t tables = (size_t)n_slots + (size_t)kvol * n_slots;
    tile_rows = (int32_t *)p;
    nbr = (int32_t *)(p + 4 * (size_t)n_slots);
    tile_mask = (uint32_t *)(p + 4 * tables);
    return p + 4 * (tables + (size_t)(n_slots / IMF_TILE_ROWS) * IMF_MASK_WORDS);
  }
};

struct Sizes {
  int64_t n[4];
  int64_t slots[4], up_slots[3];
  int ch[5], tr[5], dec[3];
  int first_kvol;
  bool small_first;
};

Sizes sizes_of(const imf_resunet_desc *net, const int64_t *n) {
  Sizes s;
  for (int i = 0; i < 4; ++i) {
    s.n[i] = n[i];
    s.slots[i] = imf_rulebook_slots(n[i]);
  }
  for (int i = 0; i < 3; ++i) s.up_slots[i] = imf_rulebook_transpose_slots(n[i]);
  for (int i = 0; i < 5; ++i) {
    s.ch[i] = net->channels[i];
    s.tr[i] = net->tr_channels[i];
  }
  for (int i = 0; i < 3; ++i) s.dec[i] = s.tr[i + 2];
  s.first_kvol = net->first_ksize * net->first_ksize * net->first_ksize;
  s.small_first = net->small_first != 0;
  return s;
}

// feature buffers: e{i}{a,b,c} (encoder level i: conv out, block mid, block out), d{i}{a,b,c}, head, fused
enum { E0A = 0, D0A = 12, HEAD = 21, FUSED = 22, NBUF = 23 };
inline int ebuf(int i, int s) { return E0A + 3 * i + s; }
inline int dbuf(int i, int s) { return D0A + 3 * i + s; }

// Both arenas of one forward.  arena_layout is the ONE place that knows where things are: the four sizing entry points return
// its totals, imf_resunet_forward and imf_fragment_forward take every pointer from it.
//   int arena    [256-byte aligned] first map (rulebook first convolution only) | k3[0..3] | dn[0..2] | up[0..2] | k3s[0..2]
//                | sort workspace (256-byte aligned inside 64 words of slack) | 3 x 16 counters | bit grid
//   float arena  [256-byte aligned] NBUF feature buffers, each rounded up to 64 floats | alignment slack | fusion
//                workspace (256-byte aligned, 64 floats below the end).  No convolution workspace: every launch is unsplit.
struct Layout {
  Rb first, k3[4], dn[3], up[3];   // conv1's map; stride-1 maps; strided maps INTO level i + 1; transposed maps into level i
  Rb k3s[3], id;                   // occupancy-sorted twins of k3[0..2] (csrc/rulebook_sort.hip); pointwise layers: no tables
  int32_t *sort_ws, *counters;     // ONE workspace for the sorts (their stream runs them in turn); 16 words per transposed map
  uint32_t *bitgrid;               // conv1's occupancy grid
  size_t sort_ws_bytes, bitgrid_words, int_bytes;
  float *buf[NBUF], *fusion_ws;
  size_t buf_floats[NBUF], fusion_ws_bytes, float_bytes;
};

// `capacity`: the fusion workspace of capacity mode.  The arenas may be null (the sizing entry points): the totals do not
// depend on the addresses.
Layout arena_layout(const Sizes &s, bool capacity, size_t bitgrid_words, const void *int_arena, const void *float_arena) {
  Layout l;
  const uintptr_t ibase = align256((uintptr_t)int_arena);
  uintptr_t p = ibase;
  if (!s.small_first) p = l.first.place(p, s.slots[0], s.n[0], s.first_kvol, 0, 0);
  for (int i = 0; i < 4; ++i) p = l.k3[i].place(p, s.slots[i], s.n[i], 27, i, i);
  for (int i = 0; i < 3; ++i) p = l.dn[i].place(p, s.slots[i + 1], s.n[i + 1], 27, i + 1, i + 1);
  for (int i = 0; i < 3; ++i) {
    p = l.up[i].place(p, s.up_slots[i], s.n[i], 27, i, 4);
    l.up[i].slots_extra = 8 * IMF_TILE_ROWS;
  }
  for (int i = 0; i < 3; ++i) p = l.k3s[i].place(p, s.slots[i], s.n[i], 27, i, i);
  l.sort_ws = (int32_t *)align256(p);
  l.sort_ws_bytes = imf_rulebook_sorted_workspace_bytes(s.slots[0]);
  p += 4 * (64 /* alignment slack */ + l.sort_ws_bytes / 4);
  l.counters = (int32_t *)p;
  p += 4 * 16 * 3;
  l.bitgrid = (uint32_t *)p;
  l.bitgrid_words = bitgrid_words;
  p += 4 * bitgrid_words;
  l.int_bytes = (size_t)(p - ibase) + 256;
  l.id.n_slots = s.slots[0]; l.id.n_out = s.n[0];
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 3; ++k) l.buf_floats[ebuf(i, k)] = (size_t)s.n[i] * s.ch[i + 1];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) l.buf_floats[dbuf(i, k)] = (size_t)s.n[i] * s.dec[i];
  l.buf_floats[HEAD] = (size_t)s.n[0] * s.tr[1];
  l.buf_floats[FUSED] = (size_t)s.n[3] * s.ch[4];
  const uintptr_t fbase = align256((uintptr_t)float_arena);
  size_t floats = 0;
  for (int i = 0; i < NBUF; ++i) {
    l.buf[i] = (float *)(fbase + 4 * floats);
    floats += (l.buf_floats[i] + 63) / 64 * 64;
  }
  l.fusion_ws_bytes = (capacity ? imf_fusion_workspace_bytes_cap(s.n[3]) : imf_fusion_workspace_bytes(s.n[3])) / 4 * 4;
  l.float_bytes = floats * 4 + l.fusion_ws_bytes + 2048;   // alignment slack of the three carved regions
  l.fusion_ws = (float *)(((uintptr_t)float_arena + l.float_bytes - l.fusion_ws_bytes - 256) & ~(uintptr_t)255);
  return l;
}

// exact mode: the bit grid covers the level-0 bounding box, when the caller knows it
Layout exact_layout(const imf_resunet_desc *net, const int64_t *n, const int32_t *bbox, const void *int_arena,
                    const void *float_arena) {
  const size_t grid_words = net->small_first && bbox ? imf_bitgrid_words(bbox, net->first_ksize) : 0;
  return arena_layout(sizes_of(net, n), false, grid_words, int_arena, float_arena);
}

struct Step {   // one fused convolution of the schedule
  int conv;     // index into imf_resunet_desc::conv
  Rb *rb;
  int in_a, c_a, out, in_b, c_b, residual;   // buffer ids (-1 none; -2 = io->x; -3 = io->out)
};

// The 23 convolutions in the order of model/resunet.py:168-226 (22 with the occupancy-feature conv1, which is no Step): the
// encoder's first n_enc, then the decoder and the two pointwise layers of the head.  twin[i]: the decoder's block on level i
// walks the occupancy-sorted twin of the level's map.  Returns the number of steps.
int build_schedule(const Sizes &s, int in_channels, const bool (&twin)[3], Layout &l, Step (&sched)[24], int &n_enc) {
  int n = 0;
  for (int i = 0; i < 4; ++i) {
    const int c = s.ch[i + 1];
    if (i > 0) sched[n++] = Step{3 * i, &l.dn[i - 1], ebuf(i - 1, 2), s.ch[i], ebuf(i, 0), -1, 0, -1};
    else if (!s.small_first) sched[n++] = Step{0, &l.first, -2, in_channels, ebuf(0, 0), -1, 0, -1};
    sched[n++] = Step{3 * i + 1, &l.k3[i], ebuf(i, 0), c, ebuf(i, 1), -1, 0, -1};
    sched[n++] = Step{3 * i + 2, &l.k3[i], ebuf(i, 1), c, ebuf(i, 2), -1, 0, ebuf(i, 0)};
  }
  n_enc = n;
  for (int i = 2; i >= 0; --i) {   // output level of conv{i+2}_tr
    const int t = s.dec[i];
    const int conv0 = 12 + 3 * (2 - i);
    const int src = i == 2 ? FUSED : dbuf(i + 1, 2), c_src = i == 2 ? s.ch[4] : s.dec[i + 1];
    const int skip = i == 2 ? -1 : ebuf(i + 1, 2), c_skip = i == 2 ? 0 : s.ch[i + 2];
    sched[n++] = Step{conv0, &l.up[i], src, c_src, dbuf(i, 0), skip, c_skip, -1};
    Rb *const rbk = twin[i] ? &l.k3s[i] : &l.k3[i];
    sched[n++] = Step{conv0 + 1, rbk, dbuf(i, 0), t, dbuf(i, 1), -1, 0, -1};
    sched[n++] = Step{conv0 + 2, rbk, dbuf(i, 1), t, dbuf(i, 2), -1, 0, dbuf(i, 0)};
  }
  sched[n++] = Step{21, &l.id, dbuf(0, 2), s.tr[2], HEAD, ebuf(0, 2), s.ch[1], -1};
  sched[n++] = Step{22, &l.id, HEAD, s.tr[1], -3, -1, 0, -1};
  return n;
}

// What imf_fragment_forward hands to imf_resunet_forward through imf_resunet_io::pyramid (internal): the coarse
// pyramid levels still to be built, and the image branch (forked by imf_fragment_forward, ahead of the pyramid).
struct FragmentCtx {
  const PyramidBuild *pb;
  const imf_image_desc *img;
  const imf_fragment_caps *caps;
  imf_fragment_io *fio;
  hipStream_t imgs;
  bool head_on_side;   // level 0 was issued on the SIDE stream (imf_fragment_io.head_on_side): the main stream joins it
  hipStream_t ahead;   // the stream of the launches carried ahead of the main stream (imf_fragment_io.ahead_stream); null: none
};

int fork_image_branch(const FragmentCtx &c, hipStream_t main) {
  imf_fragment_io *fio = c.fio;
  IMF_CHECK_HIP(hipEventRecord((hipEvent_t)fio->events[9], main));
  IMF_CHECK_HIP(hipStreamWaitEvent(c.imgs, (hipEvent_t)fio->events[9], 0));
  const int rc = imf_image_branch(c.img, fio->image, c.caps->n_items, c.caps->img_h, c.caps->img_w, fio->image_ws,
                                  fio->image_ws_bytes, nullptr, fio->kt_packed, fio->v_packed, fio->tokens_padded,
                                  fio->meta + 1, c.imgs);
  if (rc) return rc;
  IMF_CHECK_HIP(hipEventRecord((hipEvent_t)fio->events[10], c.imgs));
  return IMF_OK;
}

#ifndef IMF_SORTED_MAPS_DEFAULT
#define IMF_SORTED_MAPS_DEFAULT 0x07               // sorted twins of the stride-1 maps of levels 0, 1, 2 for the decoder (measured: LAB_NOTES round 6)
#endif
constexpr int kMetaBBox = 8;                        // meta[2 * n_levels + 0..7] with n_levels = 4
constexpr int kMetaStarts = 16;                     // meta[16 + IMF_MAX_BATCH * level + item]
constexpr int kAheadEvent = 13;                     // ahead mode: the end of the launches on the ahead stream, which the main stream joins
constexpr int kAheadMarkBegin = 14, kAheadMarkMain = 15;   // optional diagnostic marks (tools/ahead_timeline.py): the ahead chain's
                                                    // begin, the main chain's begin behind the join
constexpr int kAheadEncoder = 12, kAheadFusion = 13;   // conv1 + the encoder's 11 convolutions; ... and the fusion
#ifndef IMF_ENCODER_AHEAD_DEFAULT
#define IMF_ENCODER_AHEAD_DEFAULT kAheadEncoder     // measured: LAB_NOTES 4i
#endif
thread_local long g_ahead_forwards = 0;             // forwards the CALLING thread issued in ahead mode (imf_fragment_ahead_forwards)

/* ---- imf_resunet_forward in pieces.  The ORDER -- what is issued on which stream, after what -- is in imf_resunet_forward
   itself, at the end; the pieces below issue their own launches and nothing else. ---- */

// What every piece of one forward reads; filled once, constant afterwards.
struct Forward {
  const imf_resunet_desc *net;
  const imf_resunet_io *io;
  const FragmentCtx *fctx;         // fragment forward: coarse levels still to build (pyr), image branch; else null
  const PyramidBuild *pyr;
  Sizes s;
  bool dyn, twin[3];
  const int32_t *meta;
  int32_t *err;                    // flag word: capacity mode collects every flag in the level-0 error word; exact mode takes the caller's (optional)
  hipStream_t main, side, sorts;   // sorts: the stream of the occupancy sorts (issue_sorts)
  // Ahead mode (imf_fragment_io.ahead_stream): the first n_ahead launches of the main chain -- conv1, the encoder's convolutions,
  // the fusion as the 13th -- go to `enc`, which is not ordered behind the previous forward's decoder on `main`; the rest stays
  // on `main`, behind ONE join (events[kAheadEvent]).  Not ahead: enc == main, n_ahead == 0 -- one chain, as ever.
  hipStream_t enc;
  int n_ahead;
  hipStream_t chain_stream(int launch) const { return launch < n_ahead ? enc : main; }
  bool first_and_map;              // conv1 + the level-0 map in one launch (fragment forward; measured against two launches on two streams in round 3)
  Forward(const imf_resunet_desc *net, const imf_resunet_io *io);
};

int validate(const imf_resunet_desc *net, const imf_resunet_io *io, const Layout &l) {
  IMF_REQUIRE(io->int_arena && io->float_arena && io->out, "imf_resunet_forward: null arena / out");
  for (int i = 0; i < 4; ++i)
    IMF_REQUIRE(io->n[i] > 0 && io->level[i].coords && io->level[i].table,
                "imf_resunet_forward: level %d missing", i);
  IMF_REQUIRE(net->small_first || io->x, "imf_resunet_forward: input features required");
  IMF_REQUIRE(io->n_items >= 1 && io->n_items <= IMF_MAX_BATCH, "imf_resunet_forward: n_items=%d", io->n_items);
  if (io->dyn) {
    IMF_REQUIRE(io->meta && io->bitgrid_words > 0, "imf_resunet_forward: capacity mode needs meta and a bit-grid capacity");
    IMF_REQUIRE(net->small_first && io->x_all_ones && net->in_channels == 1 && (net->first_ksize == 3 || net->first_ksize == 5),
                "imf_resunet_forward: capacity mode covers the occupancy-feature first convolution only");
    for (int i = 0; i < 23; ++i)   // variant 6, or variant 0 throughout (the strict-fp32 recompute of a range-flagged fragment)
      IMF_REQUIRE(!net->conv[i].w_packed || net->conv[i].variant == net->conv[12].variant,
                  "imf_resunet_forward: capacity mode needs ONE convolution variant (6 or 0) for all layers");
    IMF_REQUIRE(net->conv[12].variant == 6 || net->conv[12].variant == 0 || net->conv[12].variant == 3,
                "imf_resunet_forward: capacity mode: variant 6, 3 or 0");
  } else {
    IMF_REQUIRE(!io->pyramid, "imf_resunet_forward: a pending pyramid needs capacity mode");
  }
  IMF_REQUIRE(io->int_arena_bytes >= l.int_bytes, "imf_resunet_forward: int arena %zu < %zu bytes", io->int_arena_bytes,
              l.int_bytes);
  IMF_REQUIRE(io->float_arena_bytes >= l.float_bytes, "imf_resunet_forward: float arena %zu < %zu bytes",
              io->float_arena_bytes, l.float_bytes);
  const int n_events = io->pyramid ? 9 : 10;   // (the occupancy-sorted twins have their own joins: up to three)
  for (int i = 0; i < n_events; ++i) IMF_REQUIRE(io->events[i], "imf_resunet_forward: events[%d] missing", i);
  for (int i = 0; i < NBUF; ++i)   // the LDS-DMA kernels gather their input rows through a window of IMF_CONV_ROW_WINDOW bytes
    IMF_REQUIRE(l.buf_floats[i] * sizeof(float) <= (size_t)IMF_CONV_ROW_WINDOW,
                "imf_resunet_forward: feature buffer %d exceeds the convolutions' row window (2 GiB - 4 KiB)", i);
  return IMF_OK;
}

Forward::Forward(const imf_resunet_desc *net_, const imf_resunet_io *io_) : net(net_), io(io_) {
  fctx = (const FragmentCtx *)io->pyramid; pyr = fctx ? fctx->pb : nullptr;
  s = sizes_of(net, io->n);
  dyn = io->dyn != 0; meta = io->meta;
  err = dyn ? const_cast<int32_t *>(meta) + 1 : io->flags;
  main = (hipStream_t)io->main_stream; side = (hipStream_t)io->side_stream;
  first_and_map = dyn && pyr && s.small_first && side != main;
  // Occupancy-sorted TWINS of the stride-1 maps (csrc/rulebook_sort.hip; imf_resunet_sorted_maps() says which levels): the
  // slots re-ordered so that the rows of a tile share their missing offsets -- tiles walk ~78 % of the 27 offsets instead of
  // ~100 %.  The ENCODER's blocks walk the maps as built (a sort in front of them sits on the step's critical path: measured
  // +65 us per sorted level, round 6); the DECODER's blocks (block4_tr on level 2, block3_tr on level 1, block2_tr on level 0)
  // walk the twins, which are sorted under the encoder and the fusion (issue_sorts).
  const int sorted_maps = imf_resunet_sorted_maps_n(net->conv[19].variant, io->n_items);
  for (int i = 0; i < 3; ++i) twin[i] = ((sorted_maps >> i) & 1) != 0 && (i > 0 || s.small_first);
  // The sorts' stream.  Fragment forward: the IMAGE stream, behind the image trunk -- that stream is idle from ~0.45 ms on,
  // whereas the side stream must be free for the next forward's head (streaming pipeline, bench's pipelined mode: with the
  // sorts at the end of the SIDE chain the head of step k + 1 queued behind 240 us of sorts and the steps lost what the twins
  // gain).  Otherwise: the side stream, at the end of its chain.
  sorts = pyr && fctx->imgs && fctx->imgs != side && fctx->imgs != main ? fctx->imgs : side;
  enc = main; n_ahead = 0;
  if (pyr && fctx->ahead && fctx->head_on_side && s.small_first) {
    n_ahead = imf_resunet_encoder_ahead(net->conv[19].variant, io->n_items);
    if (n_ahead > 0) enc = fctx->ahead;
  }
}

int build_map(const Forward &f, Rb &rb, int lin, int lout, int ksize, hipStream_t st) {
  const imf_level &in = f.io->level[lin], &out = f.io->level[lout];
  if (f.dyn)
    return imf_rulebook_conv_dyn(in.table, in.capacity, out.coords, f.s.n[lout], f.meta + 2 * lout,
                                 in.tensor_stride, ksize, rb.tile_rows, rb.nbr, rb.tile_mask, st);
  return imf_rulebook_conv(in.table, in.capacity, out.coords, f.s.n[lout], in.tensor_stride, ksize,
                           rb.tile_rows, rb.nbr, rb.tile_mask, st);
}

// The side stream's chain in pieces: level i + 1 (coordinates, strided map, stride-1 map: what the encoder needs next) and the
// tail (item starts, the three transposed maps, the join).  Fragment forward with sorts off the side stream (round 6): LAZY --
// each piece is ISSUED right before the first main-stream launch that waits for it instead of all of them up front -- on the
// GPU nothing changes while the host runs ahead (the streaming pipeline, the bench's steps), but a forward issued into an
// idle GPU (the synchronous extract_features call) starts its first convolution ~35 launches = ~0.1 ms of host time earlier:
// that call 1.522 -> 1.446 ms host to host, 1.129 -> 1.086 with the inputs on the device (tools/sync_phases.py; the pair step
// and the single-fragment step back to back: unchanged).  (Deferring the ISSUE of the image branch's launches the same way,
// behind block1's: measured, no further gain -- 0.970 instead of 0.950 of the eager call -- and dropped.)
// ... so only THEN: imf_fragment_io.gpu_idle_hint (the pipeline sets it when no earlier forward is still running; with work
// queued the host is ahead anyway and the chain goes up front as before -- the streaming pipeline's host span measured 1-2 %
// worse with the pieces interleaved: 1.198 / 1.183 -> 1.216 / 1.204 ms per pair on one box).  IMF_EAGER_SIDE=1 / 0
// (diagnostic, read once) forces either order.
// The chain also hands out the events the main stream waits on before the first use of a map (mark): the sorts take theirs
// from the same counter.
struct SideChain {
  const Forward &f;
  Layout &l;
  bool lazy;
  bool image_joined_side;   // the image branch's end is waited for by the SIDE stream, in the tail (see there)
  int items_event;          // the tail's join (events[8]), which the main stream waits on in front of the fusion; -1: none
  int levels_issued = 0, next_event = 0;
  bool tail_issued = false;

  SideChain(const Forward &fwd, Layout &lay) : f(fwd), l(lay) {
    static const int eager_env = getenv("IMF_EAGER_SIDE") ? atoi(getenv("IMF_EAGER_SIDE")) != 0 : -1;
    const bool main_idle = eager_env >= 0 ? eager_env == 0 : (f.fctx && f.fctx->fio->gpu_idle_hint != 0);
    lazy = f.pyr && f.sorts != f.side && f.side != f.main && main_idle;
    image_joined_side = f.pyr && f.io->image_ready && f.side != f.main;
    items_event = f.pyr ? 8 : -1;
  }

  int mark(Rb &rb, hipStream_t st) {   // record the next event on `st`; the main stream waits before the map's first use
    IMF_CHECK_HIP(hipEventRecord((hipEvent_t)f.io->events[next_event], st));
    rb.ready_event = next_event++;
    return IMF_OK;
  }

  int level(int i) {
    int rc;
    if (f.pyr && (rc = pyramid_coarse_level(*f.pyr, i + 1, f.side))) return rc;
    if ((rc = build_map(f, l.dn[i], i, i + 1, 3, f.side))) return rc;
    if ((rc = build_map(f, l.k3[i + 1], i + 1, i + 1, 3, f.side))) return rc;
    return mark(l.dn[i], f.side);
  }

  int tail() {
    const imf_resunet_io *io = f.io;
    int rc = IMF_OK;
    if (f.pyr) {   // first row of every item at every level (the fusion reads the stride-8 ones)
      if ((rc = pyramid_item_starts(*f.pyr, f.side, 0, 4))) return rc;
    }
    for (int i = 2; i >= 0; --i) {
      const imf_level &co = io->level[i + 1], &fi = io->level[i];
      Rb &up = l.up[i];
      if (f.dyn)
        rc = imf_rulebook_transpose_dyn(co.table, co.capacity, fi.coords, f.s.n[i], f.meta + 2 * i, 1 << i, 3, up.tile_rows,
                                        up.nbr, up.tile_mask, up.n_slots, l.counters + 16 * i, f.side);
      else
        rc = imf_rulebook_transpose(co.table, co.capacity, fi.coords, f.s.n[i], 1 << i, 3, up.tile_rows, up.nbr,
                                    up.tile_mask, up.n_slots, l.counters + 16 * i, f.side);
      if (rc) return rc;
      if (!f.pyr && (rc = mark(up, f.side))) return rc;
    }
    if (f.pyr) {
      // Fragment forward: ONE join with the side stream for everything the second half of the step needs (item starts for
      // the fusion, the three transposed rulebooks for the decoder), waited for right before the fusion.  A stream-wait
      // costs the main stream ~5 us even when its event completed long ago (tools/step_gaps.py, the gaps in front of
      // the convolutions: 10.6 us instead of 5.3 in front of every one that carried a wait); the side stream's chain ends
      // ~150 us before the main stream gets there.
      // The image branch joins the SIDE stream here (it was forked before this call, its end event is recorded), so the
      // main stream waits once, not twice, in front of the fusion.
      if (image_joined_side) IMF_CHECK_HIP(hipStreamWaitEvent(f.side, (hipEvent_t)io->image_ready, 0));
      IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->events[8], f.side));
    }
    tail_issued = true;
    return IMF_OK;
  }

  // issue the chain up to (and including) level `upto` (1 .. 3); with `with_tail` the rest of the levels and the tail as well
  int ensure(int upto, bool with_tail) {
    int rc;
    if (with_tail && !tail_issued) upto = 3;
    for (; levels_issued < upto; ++levels_issued)
      if ((rc = level(levels_issued))) return rc;
    return with_tail && !tail_issued ? tail() : IMF_OK;
  }

  // ... the piece that builds `rb` (a launch on it, or a sort of it, comes next)
  int ensure_for(const Rb &rb) { return rb.side_piece == 0 ? IMF_OK : ensure(rb.side_piece < 4 ? rb.side_piece : 3, rb.side_piece == 4); }
};

// ---- operand formats --------------------------------------------------------------------------------------------
// With every convolution on the split-f16 pipe, a layer's output is written as the operand image its consumers' main
// loops would otherwise derive from the fp32 rows again (imf_conv_args.operand_format; IMF_PRESPLIT=0: fp32 buffers as
// before).  fp32 stays where something other than a variant-6 convolution reads the buffer: the fusion's input
// (stride-8 block output, read by the fp32-MFMA attention kernel), the descriptors.
struct Formats {
  bool presplit;
  bool is_split[NBUF] = {};   // what each buffer holds NOW: written by the launch that fills it
  Formats(const Forward &f, const Step *sched, int n_steps) {
    presplit = !f.io->fp32_buffers;
    for (int i = 0; i < n_steps; ++i) presplit &= f.net->conv[sched[i].conv].variant == 6;
  }
  bool of(int id) const { return id >= 0 && is_split[id]; }
  bool wants_split(int id) const { return presplit && id >= 0 && id != ebuf(3, 2) && id != HEAD; }
};

// ---- first convolution (Cin <= 4): occupancy bit grid for the all-ones feature, else hash probing; first of the main chain --
int first_convolution(const Forward &f, const Layout &l, Formats &fmt, hipStream_t st) {
  const imf_resunet_desc *net = f.net; const imf_resunet_io *io = f.io;
  const imf_level &l0 = io->level[0]; const Sizes &s = f.s; const int32_t *meta = f.meta;
  float *out = l.buf[ebuf(0, 0)];
  const int first_split = fmt.wants_split(ebuf(0, 0)) ? 1 : 0;
  bool wrote_split = first_split != 0;
  ConvFirstArgs a{};
  a.coords = l0.coords; a.n = s.n[0]; a.err = f.err; a.ksize = net->first_ksize; a.grid = l.bitgrid;
  a.w = net->first_kernel; a.cout = s.ch[1]; a.scale = net->first_scale; a.shift = net->first_shift;
  a.out = out; a.out_split = first_split;
  if (f.dyn) {                       // capacity mode: row count and bounding box from the pyramid's meta block
    a.n_dev = meta; a.bbox_dev = meta + kMetaBBox; a.grid_words = io->bitgrid_words;
  } else {                           // exact size: the host box, where there is one and its grid is not too large
    a.bbox = io->bbox;
    if (io->x_all_ones && io->bbox && net->in_channels == 1) a.grid_words = imf_bitgrid_words(io->bbox, net->first_ksize);
  }
  int rc;
  if (f.first_and_map) {             // ... with the level-0 3x3x3 map from the same launch
    a.grid_filled = true; a.w_image = net->first_kernel_image;
    a.table = l0.table; a.capacity = l0.capacity;
    a.tile_rows = l.k3[0].tile_rows; a.nbr = l.k3[0].nbr; a.tile_mask = l.k3[0].tile_mask;
  } else if (f.dyn && f.pyr) {       // imf_fragment_forward zeroed the grid before the level-0 pyramid, which set the bits
    a.grid_filled = true; a.w_image = net->first_kernel_image;
  }
  if (f.dyn || a.grid_words) {
    rc = conv_first_bitgrid(a, st);
  } else {
    rc = imf_conv_first_fused(l0.table, l0.capacity, l0.coords, s.n[0], 1, net->first_ksize,
                              io->x_all_ones ? nullptr : io->x, net->in_channels, net->first_kernel, s.ch[1],
                              net->first_scale, net->first_shift, 0, out, st);
    wrote_split = false;   // (the hash-probing first layer writes fp32)
  }
  if (rc) return rc;
  fmt.is_split[ebuf(0, 0)] = wrote_split;
  return IMF_OK;
}

// ---- the occupancy-sorted twins, on f.sorts (level 2 first: the decoder reaches it first) ----
int issue_sorts(const Forward &f, Layout &l, SideChain &chain, hipStream_t after) {
  if (!(f.twin[0] || f.twin[1] || f.twin[2])) return IMF_OK;
  const imf_resunet_io *io = f.io;
  if (f.sorts != f.side) {
    // Image stream: ONE dependency, on the main CHAIN at the point of the call (`after`: the stream that carries conv3 --
    // behind conv3's launch it has waited for the side chain's level-1 and level-2 maps, and the level-0 map is its own).  Not on the side
    // stream's events: the side stream may have waited for the image branch (image_joined_side), and two captured streams
    // that wait for each other send hipStreamEndCapture into an endless recursion (ROCm 7.2, found with rocgdb).
    IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->events[6], after));
    IMF_CHECK_HIP(hipStreamWaitEvent(f.sorts, (hipEvent_t)io->events[6], 0));
  } else if (f.twin[0] && f.first_and_map) {   // the level-0 map came out of the first convolution's launch on the MAIN stream
    IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->events[6], after));
    IMF_CHECK_HIP(hipStreamWaitEvent(f.sorts, (hipEvent_t)io->events[6], 0));
  }
  for (int i = 2; i >= 0; --i) {
    if (!f.twin[i]) continue;
    int rc = imf_rulebook_sort_by_occupancy(l.k3[i].nbr, 27, l.k3[i].n_slots, f.s.n[i], f.dyn ? f.meta + 2 * i : nullptr,
                                            l.k3s[i].tile_rows, l.k3s[i].nbr, l.k3s[i].tile_mask, l.sort_ws, l.sort_ws_bytes,
                                            f.sorts);
    if (rc) return rc;
    // an event per twin: the decoder's first block must not wait for the LAST sort (measured, round 6: one event behind all
    // three sorts and one wait: one fragment per forward 0.82 -> 0.875 ms, a pair's one-bucket step 1.187 -> 1.201 -- the
    // level-0 sort ends after the stride-4 block starts; folding the twins into the join in front of the fusion instead:
    // headline leg +0.8 %)
    if (f.sorts != f.main && (rc = chain.mark(l.k3s[i], f.sorts))) return rc;
  }
  return IMF_OK;
}

float *buffer_addr(const Forward &f, const Layout &l, int id) {   // Step's buffer ids
  return id >= 0 ? l.buf[id] : id == -2 ? const_cast<float *>(f.io->x) : id == -3 ? f.io->out : nullptr;
}

// One convolution of the schedule on `stream` (the main stream, or the ahead stream for a launch carried ahead): the side
// chain's piece it waits for (lazy chain), the wait for its map, imf_conv_args, the operand-format bookkeeping, the trace record.
int launch_step(const Forward &f, const Layout &l, const Step &st, SideChain &chain, Formats &fmt, hipStream_t stream) {
  const imf_resunet_io *io = f.io;
  const imf_net_conv &c = f.net->conv[st.conv];
  IMF_REQUIRE(c.w_packed, "imf_resunet_forward: conv %d has no weights", st.conv);
  IMF_REQUIRE(st.c_a + st.c_b == c.cin, "imf_resunet_forward: conv %d expects %d input channels, got %d",
              st.conv, c.cin, st.c_a + st.c_b);
  Rb &rb = *st.rb;
  int rc;
  if ((rc = chain.ensure_for(rb))) return rc;
  if (rb.ready_event >= 0) {
    IMF_CHECK_HIP(hipStreamWaitEvent(stream, (hipEvent_t)io->events[rb.ready_event], 0));
    rb.ready_event = -1;
  }
  imf_conv_args a;
  memset(&a, 0, sizeof(a));
  a.in_a = buffer_addr(f, l, st.in_a); a.in_b = buffer_addr(f, l, st.in_b); a.c_a = st.c_a; a.c_b = st.c_b;
  a.w_packed = c.w_packed; a.kvol = c.kvol; a.cout = c.cout;
  a.tile_rows = rb.tile_rows; a.nbr = rb.nbr; a.tile_mask = rb.tile_mask;
  a.n_slots = rb.n_slots; a.n_out = rb.n_out;
  a.scale = c.scale; a.shift = c.shift; a.residual = buffer_addr(f, l, st.residual);
  a.relu = c.relu; a.l2norm = c.l2norm; a.out = buffer_addr(f, l, st.out);
  a.dyn_err = c.variant == 6 && !c.l2norm ? f.err : nullptr;   // outputs that feed another split-f16 convolution
  if (f.dyn) {
    a.n_out_dev = f.meta + 2 * rb.level;
    a.slots_extra = rb.slots_extra;
    a.dyn_err = f.err;
  }
  // one workgroup (or its wavefronts) owns a tile for all kernel offsets: no split-K partitions, no reduce launch, and
  // the kernel is a function of the level and the layer's channels only -- both modes form the same sums
  a.split_k = 1;
  a.kernel_tag = imf_resunet_conv_kernel_tag(rb.level, c.kvol, c.cin, c.cout, c.variant, io->n_items);
  a.variant = c.variant;
  IMF_REQUIRE(st.in_b < 0 || fmt.of(st.in_a) == fmt.of(st.in_b), "imf_resunet_forward: conv %d concatenates an operand "
              "image with an fp32 buffer", st.conv);
  const bool out_split = fmt.wants_split(st.out) && !c.l2norm;
  a.operand_format = (fmt.of(st.in_a) ? IMF_FMT_A_SPLIT : 0) | (fmt.of(st.residual) ? IMF_FMT_RES_SPLIT : 0) |
                     (out_split ? IMF_FMT_OUT_SPLIT : 0);
  if (st.out >= 0) fmt.is_split[st.out] = out_split;
  if (io->trace) {
    imf_net_trace &t = io->trace[st.conv];
    a.ev_begin = t.ev_begin; a.ev_end = t.ev_end;
    t.nbr = rb.nbr; t.kvol = c.kvol; t.cin = c.cin; t.cout = c.cout; t.split = a.split_k;
    t.n_slots = rb.n_slots; t.n_out = rb.n_out; t.launched = 1;
    t.level = rb.level; t.slots_extra = rb.slots_extra; t.kernel_tag = a.kernel_tag;
  }
  return imf_spconv_fwd(&a, stream);
}

// ---- bottleneck fusion (model/resunet.py:237-273) ----
int fusion_block(const Forward &f, const Layout &l, Formats &fmt, hipStream_t st) {
  const imf_resunet_desc *net = f.net; const imf_resunet_io *io = f.io;
  const int fused_split = fmt.wants_split(FUSED) ? 1 : 0;   // the block's output: conv4_tr's operand image
  const int fusion_variant = (net->conv[12].variant == 6 || net->conv[12].variant == 3) ? net->conv[12].variant : 0;
  fmt.is_split[FUSED] = fused_split != 0;
  if (f.dyn)
    return fusion_attention_dyn_fmt(l.buf[ebuf(3, 2)], f.s.n[3], f.meta + 6, f.meta + kMetaStarts + IMF_MAX_BATCH * 3,
                                    io->n_items, f.err, io->kt_packed, io->v_packed, io->n_tokens, io->tokens_padded,
                                    &net->fusion, net->fusion_scale, l.buf[FUSED], l.fusion_ws, l.fusion_ws_bytes, st,
                                    fused_split, fusion_variant);
  return fusion_attention_batched_fmt(l.buf[ebuf(3, 2)], io->n_items, io->item_row0, io->item_rows, io->kt_packed,
                                      io->v_packed, io->n_tokens, io->tokens_padded, &net->fusion, net->fusion_scale,
                                      l.buf[FUSED], l.fusion_ws, l.fusion_ws_bytes, f.err, st, fused_split,
                                      fusion_variant);
}

// The head (conv1_tr + norm + ReLU + final + L2 norm, model/resunet.py:219-233) as one launch when its shapes are the
// ones imf_pointwise_head serves; bit-identical to the two convolution launches.
bool head_is_fusable(const Forward &f) {
  const Sizes &s = f.s;
  const imf_net_conv &h1 = f.net->conv[21], &h2 = f.net->conv[22];
  const int head_cin = s.tr[2] + s.ch[1];
  const bool head_b3 = h1.variant == 3 && h2.variant == 3;           // bf16x3 images: 64 or 96 input channels (head.hip)
  return h1.w_packed && h2.w_packed && ((h1.variant == 6 && h2.variant == 6) || head_b3) && h1.kvol == 1 &&
         h2.kvol == 1 && h1.cout == 64 && h2.cin == 64 && h2.cout == 32 && h1.cin == head_cin &&
         s.tr[2] % 32 == 0 && s.ch[1] % 32 == 0 && head_cin >= 64 && head_cin <= (head_b3 ? 96 : 128) && !h1.l2norm &&
         (size_t)s.n[0] * (size_t)(s.tr[2] > s.ch[1] ? s.tr[2] : s.ch[1]) * 4 < (1ull << 31);
}

int fused_head(const Forward &f, const Layout &l, const Formats &fmt) {
  const imf_resunet_io *io = f.io;
  const imf_net_conv &h1 = f.net->conv[21], &h2 = f.net->conv[22];
  imf_head_args a;
  memset(&a, 0, sizeof(a));
  a.in_a = l.buf[dbuf(0, 2)]; a.c_a = f.s.tr[2];
  a.in_b = l.buf[ebuf(0, 2)]; a.c_b = f.s.ch[1];
  IMF_REQUIRE(fmt.is_split[dbuf(0, 2)] == fmt.is_split[ebuf(0, 2)], "imf_resunet_forward: the head's two sources differ in format");
  a.a_split = fmt.is_split[dbuf(0, 2)] ? 1 : 0;
  a.variant = h1.variant == 3 && h2.variant == 3 ? 3 : 6;
  a.w1_packed = h1.w_packed; a.scale1 = h1.scale; a.shift1 = h1.shift; a.relu1 = h1.relu; a.c_mid = 64;
  a.w2_packed = h2.w_packed; a.scale2 = h2.scale; a.shift2 = h2.shift; a.l2norm = h2.l2norm; a.c_out = 32;
  a.n = f.s.n[0];
  a.n_dev = f.dyn ? f.meta : nullptr;
  a.out = io->out;
  a.flags = f.err;
  if (io->trace) {   // one record (conv1_tr's) carries the launch; `final` is marked as not launched
    imf_net_trace &t = io->trace[21];
    a.ev_begin = t.ev_begin; a.ev_end = t.ev_end;
    t.nbr = nullptr; t.kvol = 1; t.cin = h1.cin; t.cout = h1.cout; t.split = 1;
    t.n_slots = l.id.n_slots; t.n_out = l.id.n_out; t.launched = 1;
    t.level = 0; t.slots_extra = 0; t.kernel_tag = IMF_TAG_HEAD;
    io->trace[22].launched = 0;
  }
  return imf_pointwise_head(&a, f.main);
}

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

// The rule as a table, first match wins.  Every line was settled by A/B runs in the step; the figures are in LAB_NOTES.md 4h
// (the letter at each line: 4h-b ... 4h-g).  IMF_L0_TAG, IMF_L0_UP_TAG, IMF_L1_TAG, IMF_UP_TAG (diagnostic): another tag for that line.
static int conv_kernel_tag_rule(int level, int kvol, int cin, int cout, int variant, int n_items) {
  const int W8 = IMF_TAG_WAVE8, W4 = IMF_TAG_WAVE4, HALF = IMF_TAG_HALF, U48 = IMF_TAG_U48, OCC = IMF_TAG_OCC;
  const bool b3 = variant == 3;
  if ((variant != 6 && variant != 0 && !b3) || kvol <= 1 || cout % 64 != 0) return 0;   // no wave-split build for the shape
  static const int l0_tag = getenv("IMF_L0_TAG") ? atoi(getenv("IMF_L0_TAG")) : (W4 | U48);
  static const int l0_up_tag = getenv("IMF_L0_UP_TAG") ? atoi(getenv("IMF_L0_UP_TAG")) : (W4 | HALF);
  static const int l1 = getenv("IMF_L1_TAG") ? atoi(getenv("IMF_L1_TAG")) : 0;
  static const int up_tag = getenv("IMF_UP_TAG") ? atoi(getenv("IMF_UP_TAG")) : (W4 | HALF);
  // stride 1: k_spconv_g, except on bf16x3 ...
  if (level <= 0 && b3 && cin > cout && cout == 64) return l0_up_tag;       // ... conv2_tr (128 -> 64, transposed map): half tiles (c)
  if (level <= 0) return (b3 && cin == 64 && cout == 64) ? l0_tag : 0;      // ... the two 64 -> 64 layers: 48-row units of 4 wavefronts (b)
  if (level == 1 && l1 && cin <= cout && b3) return l1;                      // (diagnostic only)
  // one fragment per forward (219 / 61 / 17 tiles): half tiles reach twice the CUs; n_items is static per forward (d)
  if (b3 && n_items == 1) return level >= 2 ? (W8 | HALF | OCC) : (W4 | HALF);
  if (level == 3 && n_items >= 2) return W8 | U48;   // stride 8 of a batch (34 tiles x 4 slabs a pair): 48-row units fill more CUs (e)
  if (level == 2 && n_items >= 3) return W4;         // stride 4 from three fragments on (>= 180 tiles): two workgroups per CU (e)
  if (b3 && cin > cout) return up_tag;               // up-convolutions: 1-8 offsets per tile, short loops -- twice the workgroups (f)
  if (level == 1) return b3 ? (W4 | OCC) : W4;       // 438 tiles a pair: two 4-wavefront workgroups per CU; bf16x3 at three per SIMD (g)
  return W8;                                         // levels 2, 3 (<= 128 tiles): one 8-wavefront workgroup per CU (g)
}

int imf_resunet_conv_kernel_tag(int level, int kvol, int cin, int cout, int variant, int n_items) {
  // bf16x3's half tiles run on the build for four wavefronts per SIMD (LAB_NOTES.md 4h-a).  IMF_HALF_OCC4=0 (diagnostic): for three.
  static const bool occ4 = !getenv("IMF_HALF_OCC4") || atoi(getenv("IMF_HALF_OCC4")) != 0;
  const int tag = conv_kernel_tag_rule(level, kvol, cin, cout, variant, n_items);
  const int shape = IMF_TAG_WAVE4 | IMF_TAG_HALF | IMF_TAG_U48;
  return (occ4 && variant == 3 && (tag & shape) == (IMF_TAG_WAVE4 | IMF_TAG_HALF)) ? (tag | IMF_TAG_OCC) : tag;
}

int imf_resunet_sorted_maps(int variant) {
  // bit i (0 .. 2): the decoder's block on level i walks an occupancy-sorted twin of the level's stride-1 map.  Default: all
  // three on bf16x3, none on fp32 MFMA / split-f16 -- measured on the S50k pair, A/B/A/B on one box (round 6, LAB_NOTES):
  // bf16x3 1.1919 / 1.1886 -> 1.1735 / 1.1733 ms (level 0 alone: 1.1787), fp32 1.914 -> 1.973, split-f16 0.914 -> 0.958: their
  // coarse-level kernels hold a CU's whole LDS, as the sort's workgroups do, and lose more to the sorts running beside them
  // than the decoder gains.  IMF_SORTED_MAP overrides for every arithmetic (A/B; 0 = none).
  return imf_resunet_sorted_maps_n(variant, 2);
}

int imf_resunet_sorted_maps_n(int variant, int n_items) {
  static const int env = getenv("IMF_SORTED_MAP") ? (int)strtol(getenv("IMF_SORTED_MAP"), nullptr, 0) & 0x07 : -1;
  if (env >= 0) return env;
  if (variant != 3) return 0;
  // ONE fragment per forward: its decoder starts ~0.35 ms into the forward, when the sorts of the coarse levels have barely
  // ended, and their blocks are short -- level 0 alone.  A/B x 4 on one box (tools/step_pair.py SINGLE=1, ms): all three
  // 0.8166 / 0.8091 / 0.8182 / 0.8019, level 0 alone 0.8027 / 0.7951 / 0.7915 / 0.7948, none 0.8061 / 0.8046 / 0.8007 / 0.7941.
  return n_items == 1 ? (IMF_SORTED_MAPS_DEFAULT & 1) : IMF_SORTED_MAPS_DEFAULT;
}

int imf_resunet_encoder_ahead(int variant, int n_items) {
  // How many launches of the main chain a forward with an ahead stream carries on it: 0 none (one chain, the order without an
  // ahead stream), 1 .. 12 conv1 and the first n - 1 encoder convolutions, 13 the fusion as well.  A static function of the
  // arithmetic and the number of fragments per forward, like imf_resunet_sorted_maps_n.  IMF_ENCODER_AHEAD (diagnostic, read
  // once) overrides it for every forward.  The arms' figures: LAB_NOTES.md 4i.
  // Ahead only where it was measured against one chain: bf16x3 with one, two and four fragments per forward (0.799 -> 0.662,
  // 1.158 -> 1.019, 2.03 -> 1.90 ms).  split-f16, fp32 MFMA and eight fragments per forward keep one chain until they are measured.
  static const int env = getenv("IMF_ENCODER_AHEAD") ? atoi(getenv("IMF_ENCODER_AHEAD")) : -1;
  const int n = env >= 0 ? env : (variant == 3 && n_items <= 4 ? IMF_ENCODER_AHEAD_DEFAULT : 0);
  return n > kAheadFusion ? kAheadFusion : n;
}

long imf_fragment_ahead_forwards(void) { return g_ahead_forwards; }

size_t imf_abi_sizeof_fragment_io(void) { return sizeof(imf_fragment_io); }

size_t imf_resunet_int_arena_bytes(const imf_resunet_desc *net, const int64_t *n, const int32_t *bbox) {
  return net && n ? exact_layout(net, n, bbox, nullptr, nullptr).int_bytes : 0;
}

size_t imf_resunet_float_arena_bytes(const imf_resunet_desc *net, const int64_t *n) {
  return net && n ? exact_layout(net, n, nullptr, nullptr, nullptr).float_bytes : 0;
}

size_t imf_resunet_int_arena_bytes_cap(const imf_resunet_desc *net, const int64_t *row_caps, size_t bitgrid_words) {
  return net && row_caps ? arena_layout(sizes_of(net, row_caps), true, bitgrid_words, nullptr, nullptr).int_bytes : 0;
}

size_t imf_resunet_float_arena_bytes_cap(const imf_resunet_desc *net, const int64_t *row_caps) {
  return net && row_caps ? arena_layout(sizes_of(net, row_caps), true, 0, nullptr, nullptr).float_bytes : 0;
}


// One forward, in issue order.  Streams: MAIN carries conv1, the 22 convolutions, the fusion and the head; SIDE carries the
// coarse pyramid levels and every map but level 0's (SideChain); the occupancy sorts run on f.sorts (the image stream in a
// fragment forward, else the side stream).  The main stream waits for a map right before the first launch on it
// (Rb::ready_event), and once, in front of the fusion, for the side chain's tail and the image branch.
// Ahead mode (Forward::enc): the first n_ahead launches of the main chain run on the AHEAD stream instead, with their waits,
// and the main stream joins once, behind the last of them; the decoder and the head never leave the main stream.
int imf_resunet_forward(const imf_resunet_desc *net, const imf_resunet_io *io) {
  IMF_REQUIRE(net && io, "imf_resunet_forward: null pointer");
  Layout l = io->dyn ? arena_layout(sizes_of(net, io->n), true, io->bitgrid_words, io->int_arena, io->float_arena)
                     : exact_layout(net, io->n, io->bbox, io->int_arena, io->float_arena);
  int rc;
  if ((rc = validate(net, io, l))) return rc;
  const Forward f(net, io);
  Step sched[24];
  int n_enc = 0;
  const int n_steps = build_schedule(f.s, net->in_channels, f.twin, l, sched, n_enc);
  Formats fmt(f, sched, n_steps);
  SideChain chain(f, l);
  hipStream_t main = f.main, side = f.side;
  // Ahead mode: launch number `launch` of the main chain (conv1 = 0, the encoder's steps, the fusion, the decoder) goes to
  // f.chain_stream(launch).  In front of the first one that stays on the main stream, the ahead stream records its end and the
  // main stream waits for it: from there on the main stream is behind everything this forward has issued on the ahead stream.
  int launch = 0;
  auto join_ahead = [&]() -> int {
    if (f.n_ahead == 0 || launch != f.n_ahead) return IMF_OK;
    IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->events[kAheadEvent], f.enc));
    IMF_CHECK_HIP(hipStreamWaitEvent(main, (hipEvent_t)io->events[kAheadEvent], 0));
    if (io->events[kAheadMarkMain]) IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->events[kAheadMarkMain], main));
    return IMF_OK;
  };

  // level 0 and its maps
  if (f.pyr && f.fctx->head_on_side) {   // level 0 was built on the side stream, ahead of the main stream: the chain joins here
    IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->events[7], side));
    IMF_CHECK_HIP(hipStreamWaitEvent(f.chain_stream(0), (hipEvent_t)io->events[7], 0));
    if (f.n_ahead && io->events[kAheadMarkBegin]) IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->events[kAheadMarkBegin], f.enc));
  } else if (f.pyr) {   // level 0 was built on the main stream: the side stream (coarse levels, rulebooks) starts after it
    IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->events[7], main));
    IMF_CHECK_HIP(hipStreamWaitEvent(side, (hipEvent_t)io->events[7], 0));
  }
  if (!f.s.small_first) {
    if ((rc = build_map(f, l.first, 0, 0, net->first_ksize, main))) return rc;
    if ((rc = build_map(f, l.k3[0], 0, 0, 3, main))) return rc;
  } else if (f.first_and_map) {
    // (fragment forward: conv1 and the level-0 3x3x3 map are ONE launch on the main stream, below)
  } else {   // conv1 needs no rulebook: k3@1 is built under it
    if ((rc = build_map(f, l.k3[0], 0, 0, 3, side))) return rc;
    if ((rc = chain.mark(l.k3[0], side))) return rc;
  }
  // the side chain: everything now, or (lazy) piece by piece from launch_step
  if (!chain.lazy && (rc = chain.ensure(3, true))) return rc;

  if (f.s.small_first) {
    if ((rc = first_convolution(f, l, fmt, f.chain_stream(launch)))) return rc;
    if (f.sorts == side && (rc = issue_sorts(f, l, chain, f.chain_stream(launch)))) return rc;
    ++launch;
  } else if (f.sorts == side && (rc = issue_sorts(f, l, chain, main))) return rc;

  // the encoder
  for (int i = 0; i < n_enc; ++i, ++launch) {
    if ((rc = join_ahead())) return rc;
    const hipStream_t st = f.chain_stream(launch);
    if ((rc = launch_step(f, l, sched[i], chain, fmt, st))) return rc;
    // the sorts on the image stream: behind the launch that made the chain wait for the level-2 map (conv3, the
    // consumer of dn[1]) -- see issue_sorts
    if (f.sorts != side && sched[i].rb == &l.dn[1]) {
      if ((rc = chain.ensure(2, false))) return rc;
      if ((rc = issue_sorts(f, l, chain, st))) return rc;
    }
  }

  // the fusion: behind the side chain's tail (item starts; it carries the image branch's end when image_joined_side)
  // diagnostic marks (tools/branch_times.py hands events[11], [12] in): the chain's arrival at the join, the fusion's end
  if ((rc = chain.ensure(3, true))) return rc;
  if ((rc = join_ahead())) return rc;
  const hipStream_t fst = f.chain_stream(launch);
  const bool diag_marks = f.pyr && io->events[11] && io->events[12];
  if (diag_marks) IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->events[11], fst));
  if (io->image_ready && !chain.image_joined_side) IMF_CHECK_HIP(hipStreamWaitEvent(fst, (hipEvent_t)io->image_ready, 0));
  if (chain.items_event >= 0) IMF_CHECK_HIP(hipStreamWaitEvent(fst, (hipEvent_t)io->events[chain.items_event], 0));
  if ((rc = fusion_block(f, l, fmt, fst))) return rc;
  ++launch;
  if (fst == main && io->fusion_done) IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->fusion_done, main));
  if (diag_marks) IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->events[12], fst));
  if ((rc = join_ahead())) return rc;   // (the fusion went ahead as well: the main stream joins behind it, and fusion_done with it)
  if (fst != main && io->fusion_done) IMF_CHECK_HIP(hipEventRecord((hipEvent_t)io->fusion_done, main));

  // the decoder and the head: always on the main stream, which therefore carries the END of every forward
  const bool one_launch_head = head_is_fusable(f);
  const int n_tail = one_launch_head ? n_steps - 2 : n_steps;
  for (int i = n_enc; i < n_tail; ++i)
    if ((rc = launch_step(f, l, sched[i], chain, fmt, main))) return rc;
  return one_launch_head ? fused_head(f, l, fmt) : IMF_OK;
}

/* ---- one fragment (or batch of fragments), points to descriptors, with no host synchronisation -------- */
size_t imf_fragment_pyramid_bytes(const imf_fragment_caps *caps) {
  if (!caps) return 0;
  return imf_pyramid_arena_bytes_caps(caps->n_points, 4, caps->rows);
}

int imf_fragment_forward(const imf_resunet_desc *net, const imf_image_desc *img, const imf_fragment_caps *caps,
                         imf_fragment_io *fio) {
  IMF_REQUIRE(net && img && caps && fio, "imf_fragment_forward: null pointer");
  IMF_REQUIRE(fio->xyz && fio->dyn && fio->image && fio->meta && fio->pyramid_arena && fio->image_ws && fio->kt_packed &&
                  fio->v_packed && fio->out, "imf_fragment_forward: null buffer");
  IMF_REQUIRE(caps->n_items >= 1 && caps->n_items <= IMF_MAX_BATCH, "imf_fragment_forward: n_items=%d", caps->n_items);
  hipStream_t main = (hipStream_t)fio->main_stream, side = (hipStream_t)fio->side_stream,
              imgs = (hipStream_t)fio->image_stream;
  if (fio->serialize) side = imgs = main;
  else IMF_REQUIRE(side && imgs && side != main && imgs != main && side != imgs, "imf_fragment_forward: three distinct streams");
  for (int i = 0; i < 11; ++i) IMF_REQUIRE(fio->events[i], "imf_fragment_forward: events[%d] missing", i);
  const int ntok = imf_image_tokens(caps->img_h, caps->img_w);
  IMF_REQUIRE(fio->tokens_padded % 64 == 0 && fio->tokens_padded >= ntok && fio->tokens_padded <= 320,
              "imf_fragment_forward: tokens_padded=%d for %d tokens", fio->tokens_padded, ntok);

  // The meta block (row counts, flag words) is reset on the main stream BEFORE the image stream forks: the image branch
  // ORs IMF_FLAG_RANGE into meta[1], which must not race with that reset.
  PyramidBuild pb;
  int rc = pyramid_prepare(pb, fio->xyz, fio->xyz_is_f64, caps->n_points, fio->voxel_size, 0, nullptr, 1, 4, fio->pyramid_arena,
                           fio->pyramid_arena_bytes, fio->meta, fio->levels, fio->dyn, caps->rows);
  if (rc) return rc;
  // conv1's occupancy bit grid (the int arena's tail: arena_layout) is zeroed ahead of the
  // pyramid, by the launch that resets the hash tables (pyramid_init), instead of between the pyramid and conv1
  IMF_REQUIRE(net->first_ksize == 3 || net->first_ksize == 5, "imf_fragment_forward: first_ksize=%d", net->first_ksize);
  IMF_REQUIRE(net->small_first && caps->bitgrid_words > 0 && fio->int_arena, "imf_fragment_forward: needs the occupancy-feature first convolution and a bit-grid capacity");
  const Layout l = arena_layout(sizes_of(net, caps->rows), true, caps->bitgrid_words, fio->int_arena, fio->float_arena);
  IMF_REQUIRE(fio->int_arena_bytes >= l.int_bytes, "imf_fragment_forward: int arena %zu < %zu bytes", fio->int_arena_bytes,
              l.int_bytes);
  IMF_REQUIRE(aligned16(l.bitgrid) && caps->bitgrid_words % 4 == 0, "imf_fragment_forward: bit grid must be 16-byte aligned, a multiple of 4 words");
  // ... and FILLED by the level-0 compaction kernel itself (the bounding box comes out of k_insert_points): no
  // k_bitgrid_fill launch between the pyramid and conv1
  pb.grid = l.bitgrid; pb.grid_words = caps->bitgrid_words; pb.grid_ksize = net->first_ksize;
  // the head (table reset, level 0, image fork): on the main stream, or -- head_on_side -- on the side stream, where it
  // does not queue behind the previous forward's decoder (include/imfnet_hip.h, imf_fragment_io.head_on_side)
  const bool head_on_side = fio->head_on_side && !fio->serialize;
  hipStream_t head = head_on_side ? side : main;
  if (head_on_side) {
    if (fio->reuse_event) IMF_CHECK_HIP(hipStreamWaitEvent(side, (hipEvent_t)fio->reuse_event, 0));
    if (fio->inputs_event) IMF_CHECK_HIP(hipStreamWaitEvent(side, (hipEvent_t)fio->inputs_event, 0));
  }
  if ((rc = pyramid_init(pb, head))) return rc;

  // image branch on its own stream, forked from and later joined to the main one (events 9 / 10), ahead of the pyramid:
  // its ~50 small launches (~0.2 ms as a chain) must be done by the fusion block.  Forking it later in the step -- after
  // block1 / conv2 / block2 / conv3 / block3, beside the levels that leave CUs idle -- was measured slower (1.07 ->
  // 1.15 ... 1.23 ms, round 3): the chain then ends after the encoder and the fusion waits for it.
  // Ahead mode (imf_fragment_io.ahead_stream): with the head on the side stream, the encoder need not queue behind the
  // previous forward's decoder either -- its launches go to the ahead stream, which takes the head's order (events[7]) and with
  // it the caller's two dependencies; the main stream joins behind them (imf_resunet_forward).  Never for a traced step or
  // inside a capture: those keep one chain.
  hipStream_t ahead = nullptr;
  if (head_on_side && fio->ahead_stream && !fio->trace) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    IMF_CHECK_HIP(hipStreamIsCapturing(main, &capturing));
    if (capturing == hipStreamCaptureStatusNone) {
      ahead = (hipStream_t)fio->ahead_stream;
      IMF_REQUIRE(ahead != main && ahead != side && ahead != imgs, "imf_fragment_forward: ahead_stream must be a fourth stream");
      IMF_REQUIRE(fio->events[kAheadEvent], "imf_fragment_forward: ahead_stream needs events[%d]", kAheadEvent);
      if (imf_resunet_encoder_ahead(net->conv[19].variant, caps->n_items) > 0) ++g_ahead_forwards;
      else ahead = nullptr;
    }
  }
  FragmentCtx fctx{&pb, img, caps, fio, imgs, head_on_side, ahead};
  if ((rc = fork_image_branch(fctx, head))) return rc;

  // level 0 of the pyramid on the head's stream (conv1 needs it first); the coarse levels go to the side stream
  if ((rc = pyramid_level0(pb, head, false))) return rc;

  imf_resunet_io io;
  memset(&io, 0, sizeof(io));
  const size_t per = (size_t)128 * fio->tokens_padded;
  for (int i = 0; i < 4; ++i) {
    io.level[i] = fio->levels[i];
    io.n[i] = caps->rows[i];
  }
  io.x_all_ones = 1;
  io.n_items = caps->n_items;
  for (int b = 0; b < caps->n_items; ++b) {
    io.kt_packed[b] = fio->kt_packed + b * per;
    io.v_packed[b] = fio->v_packed + b * per;
  }
  io.n_tokens = ntok; io.tokens_padded = fio->tokens_padded;
  io.image_ready = fio->events[10];
  io.int_arena = fio->int_arena; io.int_arena_bytes = fio->int_arena_bytes;
  io.float_arena = fio->float_arena; io.float_arena_bytes = fio->float_arena_bytes;
  io.out = fio->out;
  for (int i = 0; i < 9; ++i) io.events[i] = fio->events[i];
  io.events[11] = fio->events[11]; io.events[12] = fio->events[12];   // optional diagnostic marks
  for (int i = kAheadEvent; i <= kAheadMarkMain; ++i) io.events[i] = fio->events[i];   // the ahead join and its optional marks
  io.side_stream = side; io.main_stream = main;
  io.trace = fio->trace;
  io.fp32_buffers = fio->fp32_buffers;
  io.dyn = 1; io.meta = fio->meta; io.bitgrid_words = caps->bitgrid_words; io.pyramid = &fctx;
  return imf_resunet_forward(net, &io);
}

/* ---- hipGraph helpers: capture a launch sequence once, replay it per fragment ---------------------------- */
int imf_graph_begin_capture(void *stream) {
  IMF_CHECK_HIP(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
  return IMF_OK;
}

int imf_graph_end_capture(void *stream, void **graph_exec_out, int *n_nodes_out) {
  IMF_REQUIRE(graph_exec_out, "imf_graph_end_capture: null pointer");
  hipGraph_t graph = nullptr;
  IMF_CHECK_HIP(hipStreamEndCapture((hipStream_t)stream, &graph));
  IMF_REQUIRE(graph, "imf_graph_end_capture: the capture was invalidated");
  size_t n_nodes = 0;
  (void)hipGraphGetNodes(graph, nullptr, &n_nodes);
  if (n_nodes_out) *n_nodes_out = (int)n_nodes;
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) {
    set_error("hipGraphInstantiate: %s", hipGetErrorString(e));
    return IMF_ELAUNCH;
  }
  *graph_exec_out = (void *)exec;
  return IMF_OK;
}

int imf_graph_abort_capture(void *stream) {   // after a failed enqueue: leave capture mode, drop the partial graph
  hipGraph_t graph = nullptr;
  (void)hipStreamEndCapture((hipStream_t)stream, &graph);
  if (graph) (void)hipGraphDestroy(graph);
  (void)hipGetLastError();
  return IMF_OK;
}

int imf_graph_launch(void *graph_exec, void *stream) {
  IMF_REQUIRE(graph_exec, "imf_graph_launch: null graph");
  IMF_CHECK_HIP(hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream));
  return IMF_OK;
}

void imf_graph_destroy(void *graph_exec) {
  if (graph_exec) (void)hipGraphExecDestroy((hipGraphExec_t)graph_exec);
}

}  // extern "C"
