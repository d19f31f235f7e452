/* imfnet_hip.h -- C ABI of libimfnet_hip.so: the MI355X (gfx950) sparse-3D-convolution engine
 * behind IMFNet's descriptor-generation path.
 *
 * The reference (XiaoshuiHuang/IMFNet) has no FFI of its own: its hot path calls the
 * MinkowskiEngine 0.5.4 Python API (requirements.txt:5).  Each entry point below states which
 * reference call site(s) it replaces (file:line under /root/reference).  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless marked [host]; the library never
 *     allocates or frees caller-visible memory and keeps no global mutable state (re-entrant per
 *     stream);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - return value: 0 on success, negative IMF_E* on error; imf_last_error() gives the message of
 *     the last failing call on the calling thread;
 *   - coordinates are int32 rows (b, x, y, z); b in [0,512), x/y/z in [-2^17, 2^17) in voxel units;
 *   - feature matrices are row-major float32 [rows, C];
 *   - all kernels are launched asynchronously; counts the caller needs on the host are written to
 *     device int32 words the caller reads back when it chooses to synchronise.
 */
#ifndef IMFNET_HIP_H
#define IMFNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMF_OK            0
#define IMF_EINVAL       -1   /* bad argument (null pointer, unsupported channel count, ...) */
#define IMF_ELAUNCH      -2   /* HIP launch / runtime error */
#define IMF_EUNSUPPORTED -3

#define IMF_TILE_ROWS    64   /* output rows per rulebook tile (= 4 wavefronts x 16-row MFMA blocks) */
#define IMF_MAX_KVOL     125  /* largest kernel volume (5x5x5, config_3dmatch.py:68) */
#define IMF_MAX_BATCH    8    /* items of a batched pyramid / forward */
#define IMF_MASK_WORDS   4    /* 128-bit active-offset mask per tile */
#define IMF_XYZ_F32_QUOTIENT 2 /* xyz_is_f64 value: float32 points, float32 quotient (imf_voxelize) */

int imf_version(void);
const char *imf_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Voxel hash.  Open-addressing table of `capacity` 16-byte slots (power of two):
 *   key   uint64   packed (b,x,y,z) = b:9 | x:18 | y:18 | z:18 (two's complement fields), 0xFFFF... = empty
 *   val   int32    row index of that voxel in its level
 * Key and value share a slot so that a probe that hits is ONE 16-byte load (the rulebook builds are bound by
 * the number of random loads they issue: with separate key / value arrays a hit cost a second random line).
 * Probe sequence (csrc/common.h hash_slot / hash_step; a client that probes a table itself must walk the same one):
 * the level's coordinates are multiples of 2^shift (shift = log2 of the level's tensor stride); the 4 x 4 x 4 block of
 * voxels a key belongs to -- bits shift, shift + 1 of each coordinate field cleared -- is hashed (murmur3 finaliser) to a
 * 64-slot window, the two cleared bits of x, y, z pick the slot inside it (z fastest); a collision moves on by the
 * key-dependent ODD stride (hash(key) >> 3) | 1 (double hashing), modulo the capacity.  The library derives `shift` from the
 * stride arguments of its entry points: imf_rulebook_conv probes `in_table` with shift = log2(ts_in);
 * imf_rulebook_transpose probes the COARSE table with shift = log2(ts_fine) + 1, i.e. it serves coarse stride = 2 x fine
 * stride only (the three transposed convolutions of model/resunet.py:101-134) -- tables of other stride ratios miss.
 * Capacity to use for n keys: imf_hash_capacity(n).
 * ---------------------------------------------------------------------------------------------- */
typedef struct imf_slot {
  uint64_t key;
  int32_t val;
  int32_t pad;
} imf_slot;
int64_t imf_hash_capacity(int64_t n);

/* Bytes of scratch imf_voxelize / imf_downsample need for n input rows. */
size_t imf_unique_workspace_bytes(int64_t n);

/* Replaces: util/misc.py:82-87  coords = np.floor(xyz / voxel_size);
 *           ME.utils.sparse_quantize(coords, return_index=True); ME.utils.batched_coordinates;
 *           and the coordinate-manager insert of ME.SparseTensor(...) at util/misc.py:95.
 * xyz: [n,3] float64 (xyz_is_f64=1) or float32 (=0; widened to double before the division, which is
 *      what Open3D does to the float32 PLY at scripts/generate_desc.py:83,102), or float32 with
 *      xyz_is_f64=IMF_XYZ_F32_QUOTIENT (=2): the quotient is the correctly rounded float32 x / (float)voxel_size,
 *      then floor -- the KITTI loader's torch.from_numpy(xyz_f32) / voxel_size and numpy's xyz_f32 / 0.05
 *      (lib/data_loaders.py:532-533, 574-579).  The same three values are accepted wherever a call takes
 *      xyz_is_f64 (imf_gather_points, the pyramid builds, imf_fragment_io).
 * Division is IEEE (float64, or float32 in mode 2), floor() exact => voxel indices are bit-identical to the reference.
 * Output rows are in FIRST-OCCURRENCE order (ascending first point index):
 *   coords     int32[n,4]  (only the first *m_out rows are written)
 *   first_idx  int32[n]    index of the first point falling in each voxel (`inds`)
 *   m_out      int32[1]    number of voxels M
 *   table      hash of the M voxels (capacity = imf_hash_capacity(n) slots), val = row
 *   err_out    int32[1]    set non-zero if a coordinate was out of range (caller zeroes it)
 */
int imf_voxelize(const void *xyz, int xyz_is_f64, int64_t n, double voxel_size, int batch_index,
                 int32_t *coords, int32_t *first_idx, int32_t *m_out,
                 imf_slot *table, int64_t capacity,
                 void *workspace, int32_t *err_out, void *stream);

/* Replaces: the implicit coordinate_manager.stride() inside every stride-2
 *           ME.MinkowskiConvolution (model/resunet.py:54-85): coarse = floor(c / out_stride) *
 *           out_stride, unique rows, first-occurrence order.
 * n_in_dev: device int32 holding the actual number of input rows (<= n_in_max, which sizes the
 *           grid, the workspace and the table). */
int imf_downsample(const int32_t *coords_in, const int32_t *n_in_dev, int64_t n_in_max,
                   int out_stride,
                   int32_t *coords_out, int32_t *m_out,
                   imf_slot *table, int64_t capacity,
                   void *workspace, void *stream);

/* Replaces: `return_coords = xyz[inds]` (util/misc.py:92, returned at :104): the representative point of every voxel,
 * gathered on the device so that only M rows travel back to the host.  xyz as given to imf_voxelize / imf_pyramid_build
 * (float32 is widened, as Open3D's float64 point array is); first_idx from the same call; m_dev: optional device row
 * count (capacity mode: rows beyond it are not written), m_cap: rows (upper bound).  out: float64 [m_cap, 3]. */
int imf_gather_points(const void *xyz, int xyz_is_f64, const int32_t *first_idx, const int32_t *m_dev, int64_t m_cap,
                      double *out, void *stream);

/* One-call geometry: imf_voxelize followed by (n_levels - 1) imf_downsample (tensor strides 2, 4,
 * ...), all tables and scratch carved out of ONE caller-provided arena, row counts written to
 * meta[level][0] (meta[level][1] = error flag), followed by the bounding box of level 0:
 * meta[2*n_levels + 0..3] = min (b,x,y,z), [4..7] = max -- meta is int32[2*n_levels + 8], initialised
 * by the call.  18 kernel launches, no host synchronisation.  levels_out [host] receives the device
 * addresses inside the arena.
 * Replaces: util/misc.py:82-95 and the implicit cm.stride() chain of model/resunet.py:54-85. */
typedef struct imf_level {
  int32_t *coords;       /* [cap_rows, 4] rows (b,x,y,z), first-occurrence order                 */
  imf_slot *table;       /* hash table [capacity]: voxel key -> row                               */
  int64_t capacity;
  int32_t *first_idx;    /* level 0: index of each voxel's first point; NULL on coarser levels    */
  int64_t cap_rows;      /* rows allocated (upper bound = n points)                               */
  int32_t tensor_stride;
} imf_level;

size_t imf_pyramid_arena_bytes(int64_t n_points, int n_levels);
int imf_pyramid_build(const void *xyz, int xyz_is_f64, int64_t n, double voxel_size, int batch_index,
                      int n_levels, void *arena, size_t arena_bytes, int32_t *meta,
                      imf_level *levels_out /* [host] */, void *stream);
/* The same for a batch of fragments (the reference's ME.utils.batched_coordinates + one SparseTensor,
 * model/resunet.py:241-250): xyz holds the items' points back to back, item b = points
 * [item_starts[b], item_starts[b+1]) ([host], item_starts[0] == 0), batch index b.  Rows come out grouped
 * by item in first-occurrence order, exactly as concatenating the single-fragment results.  meta:
 * int32[2*n_levels + 8 + IMF_MAX_BATCH*n_levels]; the last block holds the first row of item b at level
 * l at [IMF_MAX_BATCH*l + b]. */
int imf_pyramid_build_batched(const void *xyz, int xyz_is_f64, int64_t n, double voxel_size,
                              const int64_t *item_starts /* [host] */, int n_items, int n_levels, void *arena,
                              size_t arena_bytes, int32_t *meta, imf_level *levels_out, void *stream);

/* Capacity mode of the pyramid (for launch sequences captured once and replayed): the point count, the number
 * of items and the items' first points are read from the device (dyn int32[16]: [0] points <= n_points_cap, [1]
 * items, [2 + b] first point of item b); level l holds at most row_caps[l] rows ([host], non-increasing, <=
 * n_points_cap) and its table is sized for the rows that can be inserted into it, so an over-full level cannot
 * fill a table: its count is clamped, the surplus voxels map to "no row" and bit 1 of meta[2l + 1] is raised.
 * meta always has the batched layout (int32[2*n_levels + 8 + IMF_MAX_BATCH*n_levels]). */
size_t imf_pyramid_arena_bytes_caps(int64_t n_points_cap, int n_levels, const int64_t *row_caps /* [host] */);
int imf_pyramid_build_dyn(const void *xyz, int xyz_is_f64, const int32_t *dyn, int64_t n_points_cap,
                          const int64_t *row_caps /* [host] */, double voxel_size, int n_levels, void *arena,
                          size_t arena_bytes, int32_t *meta, imf_level *levels_out /* [host] */, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Rulebook (MinkowskiEngine "kernel map"), tiled for the MFMA kernel:
 *   tile_rows int32[n_slots]             output row of every slot, -1 = padding
 *                                        (n_slots = n_tiles * IMF_TILE_ROWS)
 *   nbr       int32[kvol * n_slots]      nbr[k * n_slots + slot] = input row feeding that output
 *                                        row through kernel offset k, -1 = none
 *   tile_mask uint32[n_tiles * 4]        bit k set <=> some row of the tile has an input at offset k
 * Kernel offset order: k = (dx+r) + K1*(dy+r) + K1^2*(dz+r), x fastest (ME kernel_region.hpp).
 * PRECONDITION of imf_spconv_fwd: every tile that holds a live row (tile_rows >= 0) has at least one active offset.  A
 * tile whose mask is 0 is padding to the convolution kernels: an unsplit launch skips it whole and writes none of its rows
 * (a split launch would write epilogue(0) for them through the reduce kernel, a 48-row unit that shares rows with an active
 * tile writes its part; do not rely on any of it).  Every map builder
 * of this library meets it -- an output row always has its centre, a parent or a child.  A live row WITHOUT input inside a
 * tile that has an active offset is fine and is written as epilogue(0).
 * ---------------------------------------------------------------------------------------------- */

/* Identity slot order (slot == output row), padded to a whole tile. */
int64_t imf_rulebook_slots(int64_t n_out);

/* Replaces: the kernel-map generation implicit in ME.MinkowskiConvolution(kernel_size=ksize,
 *           stride in {1,2}) -- model/resunet.py:42-88,140-158, model/residual_block.py:23-33.
 *   in  = out + off_k * ts_in    (ts_in = tensor stride of the INPUT level)
 * in_table/in_capacity: hash of the input level.  out_coords: the n_out output rows. */
int imf_rulebook_conv(const imf_slot *in_table, int64_t in_capacity,
                      const int32_t *out_coords, int64_t n_out, int ts_in, int ksize,
                      int32_t *tile_rows, int32_t *nbr, uint32_t *tile_mask, void *stream);

/* Occupancy-sorted twin of a kernel map (csrc/rulebook_sort.hip): the same rows and inputs, the SLOTS re-ordered so that the
 * rows of a tile / of a 16-row block have similar neighbour-occupancy patterns -- stable sort inside windows of 16 384
 * consecutive slots by key = gray^-1(r), r = the occupancy bits (nbr_in[k][slot] >= 0) of the 12 edge offsets of the 3x3x3
 * kernel in bits 17 .. 6 (k = 1, 3, .. 25 without 13, in that order from bit 17 down) and of the 6 face offsets (4, 10, 12,
 * 14, 16, 22) in bits 5 .. 0; slots >= the row count stay last in their window (kvol != 27: r = the bits of the first 18
 * offsets).  nbr_in: a map in identity slot order (imf_rulebook_conv(_dyn), kvol
 * <= 27); outputs: tile_rows[slot] = the row now in that slot (-1: padding), nbr_out[k][slot] = nbr_in[k][row], tile_mask
 * recomputed.  A 64-row tile then walks ~78 % of the 27 offsets instead of ~100 % (stride-1 level of a 3DMatch fragment; 1.47
 * issued multiply-adds per useful one instead of 1.91), with no change to imf_spconv_fwd.  n_out_dev: optional
 * device-side row count (capacity mode; n_out is then the capacity).  Three launches: keys, the window sort, the gather.  Replaces:
 * nothing in the reference (MinkowskiEngine's kernel maps have no tile structure); used by the executors for the decoder's
 * stride-1 blocks (model/resunet.py:136-146, imf_resunet_sorted_maps).
 * workspace: imf_rulebook_sorted_workspace_bytes(n_slots) bytes of device memory (the permutation). */
size_t imf_rulebook_sorted_workspace_bytes(int64_t n_slots);
int imf_rulebook_sort_by_occupancy(const int32_t *nbr_in, int kvol, int64_t n_slots, int64_t n_out, const int32_t *n_out_dev,
                                   int32_t *tile_rows, int32_t *nbr_out, uint32_t *tile_mask, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* Capacity mode: tables sized for n_out_cap rows, the actual count read from *n_out_dev; tiles without rows keep
 * mask 0 and their neighbour slices are left unwritten (imf_spconv_fwd never looks at them). */
int imf_rulebook_conv_dyn(const imf_slot *in_table, int64_t in_capacity,
                          const int32_t *out_coords, int64_t n_out_cap, const int32_t *n_out_dev, int ts_in,
                          int ksize, int32_t *tile_rows, int32_t *nbr, uint32_t *tile_mask, void *stream);

/* Upper bound of slots for the transposed rulebook (rows grouped into 8 parity classes, every
 * class padded to whole tiles). */
int64_t imf_rulebook_transpose_slots(int64_t n_fine);

/* Replaces: the kernel map of ME.MinkowskiConvolutionTranspose(kernel_size=3, stride=2)
 *           (model/resunet.py:101-134): the forward fine->coarse map with in/out swapped, same k:
 *           out[f] += in[c] @ W[k]  for  f = c + off_k * ts_fine.
 * Output rows (fine voxels) are grouped by the parity of (coord / ts_fine) so that a tile shares
 * its (at most 8) active offsets.  counters: int32[16] scratch. */
int imf_rulebook_transpose(const imf_slot *coarse_table, int64_t coarse_capacity,
                           const int32_t *fine_coords, int64_t n_fine, int ts_fine, int ksize,
                           int32_t *tile_rows, int32_t *nbr, uint32_t *tile_mask,
                           int64_t n_slots, int32_t *counters, void *stream);

int imf_rulebook_transpose_dyn(const imf_slot *coarse_table, int64_t coarse_capacity,
                               const int32_t *fine_coords, int64_t n_fine_cap, const int32_t *n_fine_dev, int ts_fine,
                               int ksize, int32_t *tile_rows, int32_t *nbr, uint32_t *tile_mask, int64_t n_slots,
                               int32_t *counters, void *stream);   /* n_slots = imf_rulebook_transpose_slots(n_fine_cap) */

/* ------------------------------------------------------------------------------------------------
 * Sparse convolution.
 * ---------------------------------------------------------------------------------------------- */

/* Number of floats of the packed ("fragment-major") weight image for a [kvol, cin, cout] kernel. */
int64_t imf_packed_weight_floats(int kvol, int cin, int cout);

/* Re-lays a MinkowskiEngine kernel tensor W[kvol][cin][cout] (state_dict key '*.kernel';
 * [cin][cout] when kvol == 1) into the order the MFMA kernel streams it.  Done once per model
 * load.  cin % 32 == 0, cout % 32 == 0. */
int imf_pack_weights(const float *w, int kvol, int cin, int cout, float *packed, void *stream);
/* The same weights as hi/lo f16 B fragments for imf_conv_args.variant == 6 (split-f16 MFMA: every
 * fp32 operand x = f16(x) + f16(x - f16(x)); products hi*hi + hi*lo + lo*hi accumulate in fp32).  The kernel
 * is stored scaled by the power of two that puts max|w| in [2^13, 2^14) (keeps the lo halves normal f16
 * numbers; exact) and the convolution multiplies 2^-s back into its fp32 accumulators.  The image is
 * imf_packed_weight_floats_split16 floats: the fp32 image's size + a 64-float trailer holding 2^-s. */
int64_t imf_packed_weight_floats_split16(int kvol, int cin, int cout);
int imf_pack_weights_split16(const float *w, int kvol, int cin, int cout, float *packed, void *stream);
/* The same weights as THREE bf16 parts per value for imf_conv_args.variant == 3 ("bf16x3", round 5): w = p0 + p1 + p2
 * EXACTLY (p0 = bf16(w), p1 = bf16(w - p0), p2 = bf16(w - p0 - p1), round-to-nearest-even: three 8-bit significands carry
 * fp32's 24 bits, and bf16 has fp32's exponent range -- no pre-scaling, no range restriction).  The convolution splits its
 * fp32 input rows the same way in registers and forms a0 w2 + a1 w1 + a2 w0 + a0 w1 + a1 w0 + a0 w0 on the bf16 matrix
 * pipe with fp32 accumulation: every product term down to 2^-16 relative; the three dropped terms are together
 * <= 2^-26 |a| |w|, a quarter of an fp32 ulp of the product.  1.5 x the fp32 image's size.  Same reference as
 * imf_pack_weights (the '*.kernel' tensors of model/resunet.py:42-158, model/residual_block.py:23-33). */
int64_t imf_packed_weight_floats_bf16x3(int kvol, int cin, int cout);
int imf_pack_weights_bf16x3(const float *w, int kvol, int cin, int cout, float *packed, void *stream);

typedef struct imf_conv_args {
  const float *in_a;      /* [n_in, c_a]                                                      */
  const float *in_b;      /* [n_in, c_b] or NULL: second source of a fused ME.cat(a, b)       */
  int32_t c_a, c_b;       /* cin = c_a + c_b; c_a % 32 == 0, c_b % 32 == 0                    */
  const float *w_packed;  /* imf_pack_weights image                                           */
  int32_t kvol, cout;
  const int32_t *tile_rows;         /* NULL = identity (slot == row)                                  */
  const int32_t *nbr;               /* NULL allowed when kvol == 1: input row == output row           */
  const uint32_t *tile_mask;        /* NULL allowed when kvol == 1: every tile active at offset 0.  A tile with mask 0 is
                                       skipped whole by unsplit launches, so a tile that holds a live row must have an
                                       active offset (the rulebook's precondition, above)              */
  int64_t n_slots, n_out;
  const float *scale;     /* [cout] or NULL   y = acc * scale + shift  (folded eval BatchNorm /   */
  const float *shift;     /* [cout] or NULL                             bias)                     */
  const float *residual;  /* [n_out, cout] or NULL   y += residual                                */
  int32_t relu;           /* y = max(y, 0)                                                        */
  int32_t l2norm;         /* y /= ||y||_2 over the row (requires cout <= 64)                      */
  float *out;             /* [n_out, cout]                                                        */
  int32_t split_k;        /* 0 = choose automatically; >= 1 = number of kernel-offset partitions  */
  int32_t variant;        /* 0 = fp32 MFMA (v_mfma_f32_16x16x4_f32: the reference's arithmetic), since round 5 on the LDS-DMA
                                 kernels k_spconv_g / k_spconv_w (AR = kArF32) wherever their tables cover the shape
                                 (kvol <= 27, kvol * cin / 32 < 224, <= 1024 channels per source, inputs within the row window below), else --
                                 or with IMF_TAG_REGS -- on the register-staged k_spconv_mfma;
                             1 = the same arithmetic without any pipeline (simple reference kernel; any kvol);
                             2, 4, 5 = retired round-1 experiments (their measurements: DESIGN.md 4), IMF_EINVAL;
                             3 = "bf16x3": fp32 operands carried exactly by three bf16 parts each, six
                                 v_mfma_f32_16x16x32_bf16 per 32 channels, fp32 accumulation (w_packed from
                                 imf_pack_weights_bf16x3; fp32 rows in, fp32 rows out, no range restriction; kvol <= 27;
                                 in_a / in_b at most IMF_CONV_ROW_WINDOW bytes each).  k_spconv_g / k_spconv_w with AR = kArBf16x3;
                             6 = fp32-class arithmetic on the f16 matrix pipe with split operands, both operands staged
                                 global -> LDS by DMA (k_spconv_g / k_spconv_w)
                                 (w_packed from imf_pack_weights_split16; kvol <= 27; |input| < 65504;
                                 in_a / in_b at most IMF_CONV_ROW_WINDOW bytes each: raw-buffer addressing).
                             THE ROW WINDOW.  k_spconv_g and k_spconv_w (variants 6 and 3 always, variant 0 without
                             IMF_TAG_REGS) gather input rows through buffer descriptors of IMF_CONV_ROW_WINDOW =
                             0x7FFFF000 bytes (2 GiB - 4 KiB: the `no input` row index then lies outside for every row
                             stride).  A row whose bytes lie at or beyond that offset of in_a / in_b is read as ZEROS,
                             without an error -- the library sees pointers, not sizes, so the CALLER keeps each source
                             within the window, or passes variant 0 with IMF_TAG_REGS (plain loads, any size) */
  void *workspace;        /* split-K partial sums (NULL allowed iff split_k resolves to 1) */
  size_t workspace_bytes; /* >= imf_spconv_workspace_bytes(n_slots, cout, split)                  */
  void *ev_begin, *ev_end; /* optional hipEvent_t pair recorded on `stream` immediately around the
                              main MFMA kernel (not the split-K reduce): live roofline timing     */
  /* Capacity mode (any variant), for launch sequences captured once and replayed on fragments of different size:
   * n_out / n_slots (and the rulebook) are sized for a CAPACITY and the actual row count is read from device
   * memory; tiles beyond it exit at once.  A capacity-mode launch is UNSPLIT on every kernel (split_k must resolve
   * to 1, IMF_EINVAL otherwise), so the result is bit-identical to an exact-size unsplit launch.  slots_extra:
   * slots the rulebook lays out beyond roundup64(rows) (512 for imf_rulebook_transpose's parity classes, else 0). */
  const int32_t *n_out_dev;
  int32_t slots_extra;
  int32_t kernel_tag;     /* variants 6, 3 and 0: IMF_TAG_* bits (below) -- which kernel and workgroup shape; 0 = k_spconv_g */
  int32_t *dyn_err;       /* optional device flag word (any mode): IMF_FLAG_RANGE when an OUTPUT value is NaN or
                             |y| >= 65504, i.e. cannot be an operand of a following variant-6 convolution */
  int32_t geglu;          /* variant 6, kvol == 1, cout % 64 == 0, unsplit, no scale / residual / relu / l2norm: GEGLU
                             epilogue of the fusion block's feed-forward (model/attention_fusion.py:20-23,56-63).  The
                             weight image's columns are arranged per 64-column slab y as [32 values | 32 gates] of hidden
                             units 32 y .. 32 y + 31 (shift likewise); out is [n_out, cout / 2]:
                             out[r][32 y + c] = (acc_v + shift_v) * gelu(acc_g + shift_g), exact-erf GELU */
  int32_t operand_format; /* variant 6 (k_spconv_g / k_spconv_w, unsplit launches): which of the row-major [rows, channels]
                             buffers are SPLIT-F16 OPERAND IMAGES instead of fp32 -- IMF_FMT_A_SPLIT: in_a and in_b;
                             IMF_FMT_RES_SPLIT: residual; IMF_FMT_OUT_SPLIT: out is written as one (not with l2norm).
                             An operand image has the size and row stride of the fp32 buffer: per row and 32-channel chunk
                             128 bytes = [4 hi pieces | 4 lo pieces], piece j = the 8 halves of channels {4j..4j+3,
                             16+4j..16+4j+3}, hi = f16(x), lo = f16(x - hi) -- what the kernels' main loops derive from an
                             fp32 row themselves, 27 times per row for a 3x3x3 map; a producer that writes the image spares
                             its consumers the conversions (same products bit for bit).  A residual read takes hi + lo,
                             i.e. the value to 22 significant bits (relative 2^-22). */
} imf_conv_args;
#define IMF_CONV_ROW_WINDOW 0x7FFFF000ll   /* bytes of in_a / in_b the LDS-DMA kernels can gather rows from (imf_conv_args.variant) */
/* imf_conv_args.kernel_tag (variants 6, 3 and 0): which kernel and which workgroup shape a launch takes.  The values are
 * part of the ABI (trace records and C callers carry them as integers).  Bits that do not apply to a launch's arithmetic
 * are ignored (csrc/spconv_w.hip, w_build_of, says which).  Whatever the bits, a row's sums depend on the wavefront
 * count and the unit shape only, never on the row count: exact and capacity mode agree bit for bit. */
#define IMF_TAG_LABEL   1   /* profiling label: the identical kernel under a second symbol (k_spconv_g<.., 1>, whole-tile
                               k_spconv_w of 8 wavefronts: the image branch's dense convolutions) */
#define IMF_TAG_REGS    2   /* variant 0: the register-staged fp32 kernel k_spconv_mfma (the one that serves inputs beyond
                               IMF_CONV_ROW_WINDOW); variants 6 / 3: IMF_EUNSUPPORTED / IMF_EINVAL */
#define IMF_TAG_WAVE8   4   /* the wave-split kernel k_spconv_w (csrc/spconv_w.hip) with 8 wavefronts per workgroup ... */
#define IMF_TAG_WAVE4   8   /* ... or with 4 (WAVE8 wins when both are set) -- for levels of a few hundred 64-row tiles or
                               fewer: one workgroup owns a (unit of rows, 64-column slab) for all kernel offsets, its
                               wavefronts split the (offset, 32-channel chunk) list into contiguous ranges and combine
                               their partial tiles through LDS in wavefront order, epilogue in the same launch.  Needs
                               cout % 64 == 0, kvol > 1 or cin >= 256, split_k <= 1 */
#define IMF_TAG_HEAD   16   /* trace label of the fused pointwise head (imf_net_trace.kernel_tag only; not a launch shape) */
#define IMF_TAG_HALF   64   /* with WAVE4, variant 3 (with OCC also WAVE8): HALF-TILE workgroups -- 32 of a tile's 64 rows
                               each, same offset list and per-row sums: twice the workgroups for levels that leave CUs idle */
#define IMF_TAG_U48   128   /* with WAVE8 (any variant) or WAVE4 (variant 3), not with HALF: 48-ROW UNITS -- a workgroup owns
                               slots 48 u .. 48 u + 47 whatever the tile boundaries and walks the union of the offset lists
                               of the tiles it touches */
#define IMF_TAG_OCC   256   /* variant 3: the build for one more wavefront per SIMD -- with WAVE4 whole tiles for three
                               (168 VGPRs), with HALF half tiles for four (127 VGPRs, 25 KiB of LDS; WAVE4 or WAVE8); the
                               same sums as without the bit, bit for bit */

#define IMF_FMT_A_SPLIT   1
#define IMF_FMT_RES_SPLIT 2
#define IMF_FMT_OUT_SPLIT 4

/* Flag bits the kernels OR into a caller-provided device word (imf_conv_args.dyn_err, imf_resunet_io.flags, meta[1]
 * of the capacity mode).  A flagged result must not be used: redo the fragment (larger capacities / exact mode for
 * 2..8; the fp32-MFMA variant 0 for IMF_FLAG_RANGE).  Bit 16 is RETIRED and not to be reused: recorded flag words carry
 * it (it said that a capacity-mode launch had fewer rows than its device-side split-K rule covered; no kernel raises it
 * since version 101). */
#define IMF_FLAG_COORD_RANGE  1   /* a point fell outside [-2^17, 2^17) voxels or was NaN */
#define IMF_FLAG_CAPACITY     2   /* a pyramid level exceeded its row capacity */
#define IMF_FLAG_BITGRID      4   /* level-0 bounding box larger than the conv1 bit grid */
#define IMF_FLAG_EMPTY_ITEM   8   /* a batch item without voxels */
#define IMF_FLAG_RANGE       32   /* an activation left the f16 range of the split-f16 convolution operands */

/* Kernel-offset partitions imf_spconv_fwd will use for this shape when args.split_k == 0: small
 * levels (few tiles) are latency-bound, so their offsets are spread over several workgroups whose
 * partial sums are combined -- in a fixed order, hence still bit-reproducible -- by a second
 * kernel that also applies the epilogue. */
int imf_spconv_auto_split(int64_t n_slots, int cout, int kvol);
size_t imf_spconv_workspace_bytes(int64_t n_slots, int cout, int split);

/* Replaces: ME.MinkowskiConvolution / ME.MinkowskiConvolutionTranspose forward
 *           (model/resunet.py:168-226, model/residual_block.py:40-48) with the following
 *           ME.MinkowskiBatchNorm (eval), MEF.relu, residual `out += residual`
 *           (residual_block.py:50), ME.cat (resunet.py:197,208,219), `final` bias and the
 *           L2 normalisation (resunet.py:228-233) fused as prologue / epilogue.
 * out[o] = epilogue( sum_k in[nbr[k][o]] @ W[k] ).  args->variant picks the arithmetic: 6 (what the model layers
 * use) = fp32 operands split into f16 hi + lo halves, three v_mfma_f32_16x16x32_f16 per 32 channels with fp32
 * accumulation (fp32-class accuracy; inputs must stay below 65 504, see dyn_err / IMF_FLAG_RANGE); 0 = fp32 MFMA
 * (v_mfma_f32_16x16x4_f32, an exact f32 FMA chain).  Either way the sum order per output element is fixed (k
 * ascending, then input channel) => deterministic. */
int imf_spconv_fwd(const imf_conv_args *args /* [host] */, void *stream);

/* Pointwise head: two chained 1x1x1 convolutions with their epilogues as ONE launch, the [n, 64] intermediate never
 * leaving the registers / LDS of the workgroup that produced it.
 * Replaces: conv1_tr (ME.MinkowskiConvolutionTranspose kernel_size=1 over ME.cat(out_s1_tr, out_s1)) + norm1_tr +
 *           MEF.relu + final (ME.MinkowskiConvolution kernel_size=1, has_bias) + the L2 normalisation
 *           (model/resunet.py:136-158 ctor, 219-233 forward).
 *   hid = relu?((cat(in_a, in_b) @ W1) * scale1 + shift1)      [n, 64]
 *   out = l2norm?((hid @ W2) * scale2 + shift2)                  [n, 32]
 * Same arithmetic and summation order as two imf_spconv_fwd calls with variant 6 (bit-identical result).  Weight
 * images from imf_pack_weights_split16(kvol = 1).  c_a + c_b in {64, 96, 128}; c_mid == 64, c_out == 32. */
typedef struct imf_head_args {
  const float *in_a;       /* [n, c_a] */
  const float *in_b;       /* [n, c_b] or NULL */
  int32_t c_a, c_b;
  const float *w1_packed;  /* split16 image of W1 [1][c_a + c_b][c_mid] */
  const float *scale1, *shift1;   /* [c_mid] or NULL (folded BatchNorm) */
  int32_t relu1, c_mid;
  const float *w2_packed;  /* split16 image of W2 [1][c_mid][c_out] */
  const float *scale2, *shift2;   /* [c_out] or NULL (shift2 = bias) */
  int32_t l2norm, c_out;
  int64_t n;               /* rows (capacity when n_dev is given) */
  const int32_t *n_dev;    /* optional: actual row count on the device (capacity mode) */
  float *out;              /* [n, c_out] */
  int32_t *flags;          /* optional device word: IMF_FLAG_RANGE when a hidden value cannot be a split-f16 operand */
  void *ev_begin, *ev_end; /* optional hipEvent_t pair recorded around the kernel */
  int32_t a_split;         /* in_a / in_b are split-f16 operand images (imf_conv_args.operand_format) */
  int32_t variant;         /* 0 or 6: split16 weight images (above).  3: imf_pack_weights_bf16x3 images, fp32 rows, c_a + c_b
                              <= 96, no range flag -- bit-identical to two imf_spconv_fwd calls with variant 3 */
} imf_head_args;
int imf_pointwise_head(const imf_head_args *args /* [host] */, void *stream);

/* First-layer convolution for a small number of input channels (cin <= 4, e.g. the all-ones
 * occupancy feature of util/misc.py:76-79 through conv1 k=5, model/resunet.py:42-49).
 * w is the UNPACKED ME kernel [kvol][cin][cout], cout in {32, 64}.  Identity slot order. */
int imf_spconv_small_cin(const float *in, int cin, const float *w, int kvol, int cout,
                         const int32_t *nbr, int64_t n_slots, int64_t n_out,
                         const float *scale, const float *shift, int relu,
                         float *out, void *stream);

/* First-layer convolution fused with its own kernel map: probes the input level's voxel hash
 * directly (one wavefront per output voxel) instead of materialising the 125-column neighbour
 * table.  in == NULL means the all-ones occupancy feature of util/misc.py:76-79.
 * Replaces: conv1 + norm1 of model/resunet.py:42-49,168-169 (kernel map included). */
int imf_conv_first_fused(const imf_slot *table, int64_t capacity,
                         const int32_t *coords, int64_t n, int ts, int ksize, const float *in, int cin,
                         const float *w /* [kvol][cin][cout], unpacked */, int cout,
                         const float *scale, const float *shift, int relu, float *out, void *stream);

/* First-layer convolution for the all-ones occupancy feature (util/misc.py:76-79) on a dense
 * occupancy BIT GRID over the level's bounding box (bbox [host] = min b,x,y,z, max b,x,y,z as
 * imf_pyramid_build reports it): 25 five-bit windows per voxel instead of 125 hash probes, then
 * out = occupancy . W on the f16 matrix pipe with exact three-part weights (fp32 arithmetic).
 * grid: caller scratch of >= imf_bitgrid_words(bbox, ksize) uint32 words (0 = box too large: use
 * imf_conv_first_fused).  Tensor stride 1.
 * Replaces: conv1 + norm1 of model/resunet.py:42-49,168-169 (kernel map included). */
size_t imf_bitgrid_words(const int32_t *bbox /* [host] */, int ksize);
int imf_conv_first_bitgrid(const int32_t *coords, int64_t n, const int32_t *bbox /* [host] */, int ksize,
                           uint32_t *grid, size_t grid_words, const float *w /* [kvol][1][cout] */,
                           int cout, const float *scale, const float *shift, int relu, float *out,
                           void *stream);

/* Capacity mode: row count and bounding box (8 ints) read from the device; a box that needs more than grid_words
 * raises bit 2 (value 4) of *err and the launch does nothing. */
/* The same with a flag word for IMF_FLAG_RANGE on the outputs (flags may be NULL). */
int imf_conv_first_bitgrid_flags(const int32_t *coords, int64_t n, const int32_t *bbox /* [host] */, int ksize,
                                 uint32_t *grid, size_t grid_words, const float *w, int cout, const float *scale,
                                 const float *shift, int relu, float *out, int32_t *flags, void *stream);
int imf_conv_first_bitgrid_dyn(const int32_t *coords, int64_t n_cap, const int32_t *n_dev, const int32_t *bbox_dev,
                               int32_t *err, int ksize, uint32_t *grid, size_t grid_words, const float *w, int cout,
                               const float *scale, const float *shift, int relu, float *out, void *stream);

/* Bottleneck fusion block (one image, one attention head, depth 0) as ONE kernel.
 * Replaces: ResUNet2.transformer + AttentionFusion.forward (model/resunet.py:237-273,
 *           model/attention_fusion.py:65-95,132-154) for the N stride-8 point rows x [n,256]:
 *   x = to_out(softmax(to_q(LN(x)) K^T * scale) V) + x ;  x = W2(GEGLU(W1 LN(x))) + x
 * The attention matrices are given in the fragment-major layout of imf_pack_weights(kvol = 1) applied to the
 * TRANSPOSED torch Linear weight ([in, out]): wq_p [256->128], wo_p [128->256]; kt_packed = pack(K^T [128,
 * tokens_padded]), v_packed = pack(V [tokens_padded, 128]) with K, V = chunks of to_kv(LN(image tokens)), zero-padded
 * to tokens_padded (multiple of 64, <= 320).  The feed-forward runs on imf_spconv_fwd's split-f16 kernels (a Linear
 * layer is a 1x1x1 convolution over the rows), so its matrices are imf_pack_weights_split16 images:
 *   w1_p  [1][256][2048] = W1^T with the output columns re-ordered for imf_conv_args.geglu: packed column
 *         64 j + c      (c < 32) = value column 32 j + c        (torch row 32 j + c of ff[0].weight)
 *         64 j + 32 + c          = gate column 1024 + 32 j + c  (the second chunk of GEGLU's `chunk(2, dim=-1)`)
 *   b1    [2048] in the same packed order;  w2_p [1][1024][256] = W2^T;  b2 [256].
 * workspace: imf_fusion_workspace_bytes(n) bytes, 16-byte aligned (y, LN2(y) and the GEGLU hidden, 6 KB per row). */
typedef struct imf_fusion_weights {
  const float *ln1_g, *ln1_b, *wq_p, *wo_p, *bo, *ln2_g, *ln2_b, *w1_p, *b1, *w2_p, *b2;
  /* the same two feed-forward matrices as fp32 imf_pack_weights images (same column order), or NULL: what the block
   * multiplies when the network runs on variant 0 -- the fp32 recompute of a fragment whose activations left the f16
   * range must not pass through f16 operands anywhere (the attention half is fp32 MFMA in either case) */
  const float *w1_f32, *w2_f32;
} imf_fusion_weights;
/* Workspace of the block's three launches (attention half -> GEGLU GEMM -> output GEMM): 6 KB per row. */
size_t imf_fusion_workspace_bytes(int64_t n);
int imf_fusion_attention(const float *x, int64_t n, const float *kt_packed, const float *v_packed,
                         int n_tokens, int tokens_padded, const imf_fusion_weights *w /* [host] */,
                         float scale, float *out, void *workspace, size_t workspace_bytes, void *stream);
/* Batched form (one image per batch item, model/resunet.py:241-250): rows [item_row0[b], +item_rows[b]) of x
 * attend to the tokens of image b (kt_packed[b], v_packed[b]); arrays are [host], n_items <= IMF_MAX_BATCH.
 * Workspace as imf_fusion_workspace_bytes(total rows).
 * Padding: the columns of K^T and the rows of V in [n_tokens, tokens_padded) may hold any FINITE values -- their scores
 * never enter the softmax and their probabilities are exactly 0, so the output's bits do not depend on them.  Non-finite
 * padding is outside the contract (0 x inf in the P V product). */
int imf_fusion_attention_batched(const float *x, int n_items, const int64_t *item_row0, const int64_t *item_rows,
                                 const float *const *kt_packed, const float *const *v_packed, int n_tokens,
                                 int tokens_padded, const imf_fusion_weights *w /* [host] */, float scale, float *out,
                                 void *workspace, size_t workspace_bytes, void *stream);
/* The same with the arithmetic of the feed-forward chosen (variant 6: split-f16 images w1_p / w2_p; variant 3: w1_p / w2_p are
 * imf_pack_weights_bf16x3 images, fp32 rows between the two GEMMs; variant 0: fp32 MFMA on
 * w1_f32 / w2_f32) and a flag word (device int32, may be NULL; caller zeroes) that receives IMF_FLAG_RANGE when a value
 * that feeds an f16 operand -- LN2's output, the GEGLU hidden, the block's output -- is NaN or >= 65504 in magnitude. */
int imf_fusion_attention_batched_v(const float *x, int n_items, const int64_t *item_row0, const int64_t *item_rows,
                                   const float *const *kt_packed, const float *const *v_packed, int n_tokens,
                                   int tokens_padded, const imf_fusion_weights *w /* [host] */, float scale, float *out,
                                   void *workspace, size_t workspace_bytes, int32_t *flags, int variant, void *stream);

typedef struct imf_net_conv {          /* static half of one fused convolution */
  const float *w_packed;               /* imf_pack_weights / imf_pack_weights_split16 image (see variant) */
  int32_t kvol, cin, cout;
  const float *scale, *shift;          /* folded BatchNorm or bias; NULL = identity */
  int32_t relu, l2norm, variant;
} imf_net_conv;

/* ---- Image branch of the fusion block ------------------------------------------------------------
 * Replaces: ImageEncoder / ResNet.forward (model/Img_Encoder.py:15-18, model/resnet.py:195-216: conv7x7/2 -
 *           bn - relu - maxpool3/2 - layer1 (3 BasicBlocks, 64) - layer2 (4 BasicBlocks, 128, first stride 2 with
 *           the 1x1 projection), model/resnet.py:35-72) and the image-only half of the cross attention
 *           (norm_context + to_kv, model/attention_fusion.py:36-46,84; token layout of model/resunet.py:257-261).
 * Every convolution runs on imf_spconv_fwd's kernel over static pixel tables (a dense 3x3 conv is a
 * sparse conv with a full rulebook; rows = NHWC pixels), BatchNorm folded into scale / shift.
 * Weight images (device, built once per model): conv weights torch [co][ci][ky][kx] re-laid as
 * [k = ky*3+kx][ci][co] and packed with imf_pack_weights(_split16) according to `variant`; the stem as a
 * [1][160][64] kernel whose row (ky*7+kx)*3 + ch holds w[co][ch][ky][kx] (rows 147..159 zero);
 * kv_w = to_kv.weight^T [128][256].
 * conv order: layer1.{0,1,2}.{conv1,conv2} (0-5), layer2.0.conv1 (6), layer2.0.downsample (7), layer2.0.conv2 (8),
 * layer2.{1,2,3}.{conv1,conv2} (9-14); relu = 1 on every entry except the projection (7). */
typedef struct imf_image_desc {
  const float *stem_w, *stem_scale, *stem_shift;
  imf_net_conv conv[15];
  const float *ln_g, *ln_b;            /* norm_context (LayerNorm 128, eps 1e-5); NULL if K/V are not wanted */
  const float *kv_w;                   /* packed to_kv^T [1][128][256] */
  int32_t variant;                     /* imf_conv_args.variant of the stem and K/V projections */
} imf_image_desc;

/* Bytes of the per-(B,H,W) workspace: static pixel tables (filled once by imf_image_tables_build) followed
 * by the feature buffers of one pass.  256-byte aligned. */
size_t imf_image_workspace_bytes(int B, int H, int W);
int imf_image_tokens(int H, int W);    /* tokens per image = (H/8)*(W/8) for H, W divisible by 8 */
int imf_image_tables_build(int B, int H, int W, void *workspace, size_t workspace_bytes, void *stream);
/* image: [B,3,H,W] fp32.  feat_out (optional): [B*tokens, 128] = the stride-8 map in NHWC order, i.e.
 * image_features.view(B,128,-1).permute(0,2,1) of model/resunet.py:257-261.  kt_packed / v_packed (optional,
 * both or neither): per image b at offset b*128*tokens_padded floats, K^T [128, tokens_padded] and
 * V [tokens_padded, 128] in imf_pack_weights(kvol = 1) order, zero-padded -- what imf_fusion_attention reads.
 * About 22 launches, no host synchronisation. */
int imf_image_branch(const imf_image_desc *net /* [host] */, const float *image, int B, int H, int W,
                     void *workspace, size_t workspace_bytes, float *feat_out, float *kt_packed,
                     float *v_packed, int tokens_padded, int32_t *flags /* device, optional: IMF_FLAG_RANGE */,
                     void *stream);

/* ---- Training of the image trunk (csrc/image_train.hip) -------------------------------------------------------------------
 * Replaces: ImageEncoder / ResNet.forward in training mode and its autograd (model/resnet.py:195-216 under
 *           loss.backward(), lib/trainer.py:495-569): 16 MIOpen convolutions, 16 training-mode BatchNorm2d, the max pool
 *           and their gradients.  The convolutions are imf_spconv_fwd (forward, and input gradient over the opposite
 *           table) and imf_spconv_wgrad over the static pixel tables below, BatchNorm2d over NCHW is imf_bn_train_* over
 *           the [B*H*W, C] rows (imfnet_amd/autograd.py, model/image_encoder.py); this section adds the tables, the stem's
 *           im2col and the max pool.  Every call takes a stream and synchronises nothing; bad arguments (B < 1, H or W < 8,
 *           a null pointer, a short or misaligned buffer, C % 4 != 0) return IMF_EINVAL before any launch.
 *
 * Tables.  With H2 x W2 the stem's output ((H - 1) / 2 + 1), H4 x W4 the pool's, H8 x W8 layer2's, rows = NHWC pixels
 * (b * H + y) * W + x, taps k = ky * 3 + kx, nbr[k * n_slots + slot] = the pixel the row gathers through tap k or -1, slots
 * beyond n_out padding (tile_rows -1, nbr -1), tile_mask bit k of a 64-slot tile set when any of its rows has a neighbour
 * through tap k -- the layout imf_conv_args reads:
 *   t4    rows H4 x W4  from H4 x W4  9 taps  3x3 stride 1 pad 1 (layer1); its own opposite with taps k <-> 8 - k
 *   t48   rows H8 x W8  from H4 x W4  9 taps  3x3 stride 2 pad 1 (layer2.0.conv1)
 *   t48T  rows H4 x W4  from H8 x W8  9 taps  opposite of t48: nbrT[k][i] = o  <=>  nbr[k][o] = i
 *   td    rows H8 x W8  from H4 x W4  1 tap   1x1 stride 2 (layer2.0.downsample)
 *   tdT   rows H4 x W4  from H8 x W8  1 tap   opposite of td: a pixel with an odd coordinate has no neighbour.  Its mask
 *         has tap 0 set in EVERY tile that holds a row, so that imf_spconv_fwd (which skips a tile with an empty mask)
 *         writes +0.0 to those pixels
 *   t8    rows H8 x W8  from H8 x W8  9 taps  3x3 stride 1 pad 1 (layer2); its own opposite likewise
 * The six tables depend on (B, H, W) only and live in the caller's storage (imf_image_train_tables_bytes, 256-byte
 * aligned); `out` [host] receives their device addresses and counts.  Integer work: the same tables every time. */
typedef struct imf_image_table {
  int32_t *tile_rows, *nbr;
  uint32_t *tile_mask;
  int64_t n_slots, n_out;
  int32_t kvol;
} imf_image_table;
typedef struct imf_image_train_tables {
  imf_image_table t4, t48, t48T, td, tdT, t8;
} imf_image_train_tables;
size_t imf_image_train_tables_bytes(int B, int H, int W);   /* 0 for a shape the build refuses */
int imf_image_train_tables_build(int B, int H, int W, void *storage, size_t storage_bytes,
                                 imf_image_train_tables *out /* [host] */, void *stream);
/* The stem's patch matrix: image [B,3,H,W] fp32 -> out [B*H2*W2, 160], column (ky*7+kx)*3 + ch = the pixel the 7x7 / 2 /
 * pad 3 convolution reads there (0 outside the image), columns 147..159 zero -- the matrix imf_image_branch builds, without
 * its range flag.  A copy: exact. */
int imf_image_im2col7(const float *image_nchw, int B, int H, int W, float *out, void *stream);
/* nn.MaxPool2d(3, 2, 1) (model/resnet.py:144,202) on NHWC rows in [B*Hin*Win, C] -> out [B*Hout*Wout, C], Hout = (Hin - 1) /
 * 2 + 1; C % 4 == 0, 16-byte aligned rows.  The taps inside the map are scanned in (ky, kx) row-major order and a later one
 * replaces the current one only when it is strictly greater (torch's rule: among equal maxima the FIRST receives the
 * gradient) or NaN (a NaN in a window gives NaN; which tap then receives the gradient is unspecified).  tap [B*Hout*Wout, C]
 * uint8 = ky*3+kx of the winner.
 * backward: one thread per input pixel and 4 channels gathers dout from the at most four windows that contain the pixel,
 * in ascending (oy, ox) order, where tap points at it; fp64 sum, one rounding; every element of din [B*Hin*Win, C] is
 * written, zeros included.  No atomics: two calls give the same bits. */
int imf_image_maxpool_forward(const float *in, int B, int Hin, int Win, int C, float *out, uint8_t *tap, void *stream);
int imf_image_maxpool_backward(const float *dout, const uint8_t *tap, int B, int Hin, int Win, int C, float *din,
                               void *stream);

/* imf_fusion_attention_batched + IMF_FLAG_RANGE on the output rows (they feed conv4_tr); flags may be NULL. */
int imf_fusion_attention_batched_flags(const float *x, int n_items, const int64_t *item_row0, const int64_t *item_rows,
                                       const float *const *kt_packed, const float *const *v_packed, int n_tokens,
                                       int tokens_padded, const imf_fusion_weights *w /* [host] */, float scale,
                                       float *out, void *workspace, size_t workspace_bytes, int32_t *flags, void *stream);
/* Capacity mode: x has room for n_cap rows, the count is *n_dev and item b covers rows [item_starts_dev[b],
 * item_starts_dev[b+1]) (the last one up to the count); an item without rows raises bit 3 (value 8) of *err.  The same
 * three launches as the exact-size call (grids sized for the capacity, surplus tiles exit at once): bit-identical.
 * workspace: imf_fusion_workspace_bytes_cap(n_cap). */
size_t imf_fusion_workspace_bytes_cap(int64_t n_cap);
int imf_fusion_attention_dyn(const float *x, int64_t n_cap, const int32_t *n_dev, const int32_t *item_starts_dev,
                             int n_items, int32_t *err, const float *const *kt_packed, const float *const *v_packed,
                             int n_tokens, int tokens_padded, const imf_fusion_weights *w /* [host] */, float scale,
                             float *out, void *workspace, size_t workspace_bytes, void *stream);
/* The same with the arithmetic of the feed-forward chosen, as imf_fusion_attention_batched_v chooses it (6, 3 or 0;
 * imf_fusion_attention_dyn is variant 6). */
int imf_fusion_attention_dyn_v(const float *x, int64_t n_cap, const int32_t *n_dev, const int32_t *item_starts_dev,
                               int n_items, int32_t *err, const float *const *kt_packed, const float *const *v_packed,
                               int n_tokens, int tokens_padded, const imf_fusion_weights *w /* [host] */, float scale,
                               float *out, void *workspace, size_t workspace_bytes, int variant, void *stream);

/* ---- Native executor for the ResUNet layer schedule -----------------------------------------------
 * One call per fragment replaces the ~100 per-layer calls of model/resunet.py:163-235 (rulebook builds
 * on a side stream, first convolution, encoder, bottleneck fusion, decoder, head), in the launch order
 * and with the arithmetic of the per-layer entry points above.  Configuration: batch 1, one attention
 * head, fusion depth 0 (IMFNet's).  All pointers inside the structs are device pointers except where
 * noted; the structs themselves live on the host. */

typedef struct imf_resunet_desc {
  int32_t channels[5], tr_channels[5]; /* CHANNELS / TR_CHANNELS of model/resunet.py:22-23 (index 0 unused) */
  int32_t in_channels, out_channels, first_ksize;
  int32_t small_first;                 /* in_channels <= 4: conv1 runs as imf_conv_first_* (first_* below) */
  /* 0 conv1 | 1,2 block1 | 3 conv2 | 4,5 block2 | 6 conv3 | 7,8 block3 | 9 conv4 | 10,11 block4 |
   * 12 conv4_tr | 13,14 block4_tr | 15 conv3_tr | 16,17 block3_tr | 18 conv2_tr | 19,20 block2_tr |
   * 21 conv1_tr | 22 final */
  imf_net_conv conv[23];
  const float *first_kernel, *first_scale, *first_shift;   /* conv1 [kvol][cin][cout] unpacked + norm1 */
  imf_fusion_weights fusion;
  float fusion_scale;
  const float *first_kernel_image;     /* optional: imf_pack_first_kernel(first_kernel) -- conv1's hi / lo f16 weight image, so
                                          that the fragment forward's conv1 workgroups copy 16 KiB instead of re-splitting the
                                          kernel each (same bits either way); NULL: split in the kernel */
} imf_resunet_desc;
/* conv1 (k = 3 or 5, Cin = 1, Cout 32 / 64, model/resunet.py:42-49) as the f16 matrix pipe reads it: image of
 * imf_first_kernel_image_floats(kvol, cout) floats, 16-byte aligned.  One-time re-layout at model load; replaces nothing. */
int64_t imf_first_kernel_image_floats(int kvol, int cout);
int imf_pack_first_kernel(const float *w /* [kvol][1][cout] */, int kvol, int cout, float *image, void *stream);

typedef struct imf_net_trace {         /* optional per-convolution measurement record (index = conv id) */
  void *ev_begin, *ev_end;             /* in: hipEvent_t pair recorded around the main kernel */
  const int32_t *nbr;                  /* out: the launch's neighbour table (NULL for 1x1x1) */
  int32_t kvol, cin, cout, split;
  int64_t n_slots, n_out;
  int32_t launched;
  int32_t level, slots_extra;          /* out: pyramid level of the output rows; rulebook slots beyond roundup64(rows) */
  int32_t kernel_tag;                  /* out: imf_conv_args.kernel_tag of the launch (imf_resunet_conv_kernel_tag) */
} imf_net_trace;

/* Which LDS-DMA kernel (variants 3, 6 and 0 alike: the arithmetic is a template argument of the same two kernels) the
 * ResUNet executors (imf_resunet_forward, imf_fragment_forward and the Python plan that mirrors them) use for a convolution whose OUTPUT rows live on pyramid level `level` (0 = tensor stride 1):
 * the value for imf_conv_args.kernel_tag.  Level 0 (thousands of 64-row tiles): k_spconv_g, unsplit (variant 3: the
 * wave-split kernel with 4 wavefronts and 48-row units, IMF_TAG_WAVE4 | IMF_TAG_U48, for the 64 -> 64 layers; with half tiles,
 * WAVE4 | HALF | OCC, for the 128 -> 64 up-convolution).  Level 1: the
 * wave-split kernel with 4 wavefronts per workgroup (WAVE4; variant 3: WAVE4 | OCC); levels 2 and 3: with 8 (WAVE8); variant 3 with
 * ONE fragment in the forward (n_items == 1): half-tile workgroups of 4 wavefronts (WAVE4 | HALF | OCC) on level 1 and of 8 (WAVE8 | HALF | OCC) on levels 2-3; every variant
 * with two or more fragments: 48-row units (WAVE8 | U48) on level 3, and from three fragments on 4 wavefronts on level 2.  The choice is
 * a function of the LEVEL, the layer's channel counts and the batch size only -- never of the row count -- so exact mode,
 * capacity mode and a graph replay form every sum in the
 * same order (bit-identical descriptors) without a device-side split rule.  What DOES depend on n_items is the partition of a
 * row's sum (wavefront count, unit shape): the descriptors of a fragment computed alone and computed inside a batch of two
 * or more agree to fp32 round-off (~1e-7), not bit for bit, and the same holds between batch sizes 2 and >= 3; set
 * n_items consistently where reproducibility across batch sizes matters.  No executor launch uses split-K partitions
 * or the k_spconv_reduce pass any more.  0 for shapes the wave-split kernel does not serve (kvol == 1, cout % 64 != 0,
 * a variant other than 6 / 3 / 0).  Replaces: the implicit per-layer algorithm choice inside
 * ME.MinkowskiConvolution (model/resunet.py:168-226). */
int imf_resunet_conv_kernel_tag(int level, int kvol, int cin, int cout, int variant, int n_items);
/* For which pyramid levels (bit i = level i, 0 .. 2) the executors (imf_resunet_forward, imf_fragment_forward, the Python plan)
 * build an occupancy-sorted TWIN of the stride-1 map (imf_rulebook_sort_by_occupancy) that the DECODER's block of the level
 * walks -- block2_tr / block3_tr / block4_tr of model/resunet.py:136-146; the encoder's blocks walk the map as built (a sort in
 * front of them would sit on the critical path).  A function of the arithmetic (imf_conv_args.variant of the layers: 7 for
 * bf16x3, 0 for fp32 MFMA and split-f16, where the sorts cost more than the twins return) and of the process environment
 * (IMF_SORTED_MAP overrides) only, so every execution mode walks the same maps and forms the same sums.  Replaces: nothing in
 * the reference. */
int imf_resunet_sorted_maps(int variant);
/* ... and of the batch size of the forward (static per call, like imf_resunet_conv_kernel_tag's n_items): with ONE fragment
 * only level 0 has a twin (its decoder reaches the coarse levels before their sorts would pay).  imf_resunet_sorted_maps(v) is
 * imf_resunet_sorted_maps_n(v, 2): the superset, which sizes the arenas. */
int imf_resunet_sorted_maps_n(int variant, int n_items);

typedef struct imf_resunet_io {        /* per fragment */
  imf_level level[4];                  /* tensor strides 1, 2, 4, 8 (imf_pyramid_build) */
  int64_t n[4];                        /* rows per level */
  const int32_t *bbox;                 /* [host] level-0 bounding box (8 ints) or NULL */
  const float *x;                      /* [n0, in_channels] input features (may be NULL when x_all_ones) */
  int32_t x_all_ones;                  /* util/misc.py:76-79 occupancy feature */
  int32_t n_items;                     /* fragments in the batch (1..IMF_MAX_BATCH), rows grouped by item */
  int64_t item_row0[IMF_MAX_BATCH];    /* first stride-8 row of item b ... */
  int64_t item_rows[IMF_MAX_BATCH];    /* ... and how many (imf_pyramid_build_batched's meta) */
  const float *kt_packed[IMF_MAX_BATCH], *v_packed[IMF_MAX_BATCH];   /* image b's tokens: K^T / V, packed */
  int32_t n_tokens, tokens_padded;
  void *image_ready;                   /* hipEvent_t the main stream waits on before the fusion, or NULL */
  void *fusion_done;                   /* hipEvent_t recorded on the main stream right after the fusion
                                          (the image tokens' K/V may be overwritten after it), or NULL */
  void *int_arena;  size_t int_arena_bytes;     /* >= imf_resunet_int_arena_bytes   */
  void *float_arena; size_t float_arena_bytes;  /* >= imf_resunet_float_arena_bytes */
  float *out;                          /* [n0, out_channels] descriptors */
  void *events[16];                    /* caller-owned hipEvent_t (imf_event_create): side-stream joins (10 used: seven
                                          maps + up to three sorted twins; 9 with `pyramid`) */
  void *side_stream, *main_stream;
  imf_net_trace *trace;                /* [host] 23 records or NULL */
  /* Capacity mode (dyn != 0): n[] are CAPACITIES (arenas: the *_cap size queries), the row counts, the level-0
   * bounding box and the items' first rows are read on the device from `meta`, the block imf_pyramid_build_dyn
   * writes (item_row0 / item_rows / bbox above are ignored); flags raised by the kernels are OR-ed into meta[1]:
   * 1 coordinate out of range, 2 a level exceeded its capacity, 4 bounding box larger than the bit grid, 8 an item
   * without rows, 16 fewer rows than a quarter of the capacity (split cover exceeded).  A flagged result must be
   * discarded and the fragment redone with larger capacities or in exact mode.  Needs ONE convolution variant for all
   * layers (6, or 0 = the strict-fp32 arithmetic), the all-ones occupancy input and in_channels 1.  Bit-identical to the
   * exact mode of the same variant. */
  int32_t dyn;
  const int32_t *meta;
  size_t bitgrid_words;                /* capacity (uint32 words) of the conv1 occupancy grid inside the int arena */
  const void *pyramid;                 /* internal (imf_fragment_forward): coarse pyramid levels still to be built */
  int32_t *flags;                      /* exact mode, optional: device word the kernels OR IMF_FLAG_RANGE into (caller zeroes) */
  int32_t fp32_buffers;                /* 0 (default): with every convolution on variant 6 the layers hand their outputs on as
                                          split-f16 operand images (imf_conv_args.operand_format) -- residual reads see 22 of
                                          the 24 significant bits; 1: every feature buffer stays fp32 (the arithmetic of the
                                          op-by-op path: each imf_spconv_fwd with operand_format 0) */
} imf_resunet_io;

size_t imf_resunet_int_arena_bytes(const imf_resunet_desc *net, const int64_t *n /* [4] */,
                                   const int32_t *bbox /* [host] or NULL */);
size_t imf_resunet_float_arena_bytes(const imf_resunet_desc *net, const int64_t *n /* [4] */);
int imf_resunet_forward(const imf_resunet_desc *net /* [host] */, const imf_resunet_io *io /* [host] */);
size_t imf_resunet_int_arena_bytes_cap(const imf_resunet_desc *net, const int64_t *row_caps /* [4] */, size_t bitgrid_words);
size_t imf_resunet_float_arena_bytes_cap(const imf_resunet_desc *net, const int64_t *row_caps /* [4] */);

/* ---- Whole fragment in one call, capturable as a hipGraph -----------------------------------------------
 * Replaces: util/misc.py:67-104 extract_features (voxelise -> SparseTensor -> model(stensor, image)) for a fragment
 * or a batch of fragments: pyramid (level 0 on the main stream, coarser levels interleaved with the rulebook
 * builds on the side stream), image branch on its own stream, conv1, encoder, fusion, decoder, head -- about 150
 * launches and no host synchronisation.  Every size below is a CAPACITY; the per-fragment scalars live in `dyn`
 * (device int32[IMF_DYN_WORDS]: [0] points, [1] items, [2 + b] first point of item b), which the caller writes
 * before the launch (or before each replay).  After completion meta (device int32[IMF_META_WORDS]) holds, for
 * level l, the row count at [2l], flags at [1] (imf_resunet_io), the level-0 bounding box at [8..15] and the first
 * row of item b of level l at [16 + IMF_MAX_BATCH*l + b]; out[0 .. meta[0]) are the descriptors, levels[0].first_idx
 * the voxels' first points.  Because addresses and grids depend on the capacities only, the call can be recorded
 * between imf_graph_begin_capture / imf_graph_end_capture on main_stream and replayed for every fragment that
 * fits the capacities (side_stream / image_stream join the capture through the events). */
#define IMF_DYN_WORDS  16
#define IMF_META_WORDS 64
typedef struct imf_fragment_caps {     /* [host] one capacity bucket */
  int64_t n_points;                    /* points (all items together) */
  int64_t rows[4];                     /* voxels at tensor strides 1, 2, 4, 8 */
  int32_t n_items, img_h, img_w;
  size_t bitgrid_words;                /* conv1 occupancy grid: >= imf_bitgrid_words of the largest bounding box, a multiple of 4 */
} imf_fragment_caps;

typedef struct imf_fragment_io {       /* [host]; all buffers device memory owned by the caller */
  const void *xyz; int32_t xyz_is_f64; /* [caps.n_points, 3] */
  double voxel_size;
  const int32_t *dyn;                  /* IMF_DYN_WORDS */
  const float *image;                  /* [n_items, 3, img_h, img_w] */
  int32_t *meta;                       /* IMF_META_WORDS, written */
  void *pyramid_arena; size_t pyramid_arena_bytes;   /* >= imf_fragment_pyramid_bytes(caps), 256-byte aligned */
  void *image_ws; size_t image_ws_bytes;             /* imf_image_workspace_bytes, tables built */
  float *kt_packed, *v_packed; int32_t tokens_padded; /* n_items * 128 * tokens_padded floats each (scratch) */
  void *int_arena; size_t int_arena_bytes;           /* >= imf_resunet_int_arena_bytes_cap   */
  void *float_arena; size_t float_arena_bytes;       /* >= imf_resunet_float_arena_bytes_cap */
  float *out;                          /* [caps.rows[0], out_channels] */
  void *events[16];                    /* 11 caller-owned hipEvent_t */
  void *main_stream, *side_stream, *image_stream;
  imf_net_trace *trace;                /* [host] 23 records or NULL */
  imf_level levels[4];                 /* out [host]: where the levels live inside pyramid_arena */
  int32_t serialize;                   /* measurement aid: issue everything on main_stream (no overlap between branches) */
  int32_t fp32_buffers;                /* as imf_resunet_io.fp32_buffers */
  /* Head on the side stream (a STREAM of forwards over several buckets).  0: the table reset, the level-0 pyramid and the
   * image fork are issued on main_stream, i.e. behind everything the main stream still holds -- the previous forward's
   * decoder.  1: they are issued on side_stream, which is idle from the middle of the previous forward on, and the main
   * stream joins in front of conv1: forward k+1's first ~60 us run under forward k's last convolutions (same kernels,
   * same results).  The head then no longer inherits the main stream's order, so the caller states its two dependencies:
   * inputs_event (NULL: none) = after which xyz / dyn / image are in place; reuse_event (NULL: none) = after which earlier
   * work on ANY stream no longer touches this bucket's buffers (the end of its previous forward and of whatever read its
   * outputs).  Not inside a hipGraph capture. */
  int32_t head_on_side;
  /* Hint, 0 or 1: the GPU is idle when this forward is issued (a synchronous call: nothing queued on main_stream).  The executor
   * then issues the side stream's pieces (coarse levels, rulebooks, transposed maps) right before the first main-stream launch
   * that waits for each instead of all of them ahead of conv1 -- same streams, events and results; the first convolution starts
   * ~0.1 ms of host time earlier.  With work queued ahead (a stream of forwards) leave it 0.  imf_pipeline_* sets it per job. */
  int32_t gpu_idle_hint;
  void *inputs_event, *reuse_event;
  /* Encoder on a fourth stream (a STREAM of forwards over several buckets; needs head_on_side).  NULL: one main chain, exactly
   * the order described above.  A stream distinct from the other three and on a hardware queue of its own (imf_streams_concurrent): conv1 and the encoder's convolutions -- the first
   * imf_resunet_encoder_ahead() launches of the main chain -- are issued on it behind the head (events[7]) instead of on
   * main_stream, so forward k+1's encoder runs beside forward k's decoder: each chain fills the gaps between the other's
   * dependent launches and the CUs its coarse levels leave idle (same kernels in the same per-forward order on the same buffers:
   * same results).  The ahead stream takes the head's two dependencies (inputs_event, reuse_event) through events[7]; it records
   * events[13] (required with this field) behind its last launch, and main_stream waits for that event in front of its own first
   * launch.  The decoder and the head stay on main_stream, which therefore still carries the END of every forward: work enqueued
   * on main_stream behind the call sees finished descriptors, and an event recorded there is a valid reuse_event as before.
   * Everything the ahead launches touch belongs to the bucket, so reuse_event / imf_pipeline_wait's contract
   * cover it.  Ignored -- one chain -- with head_on_side == 0, serialize, a trace, or inside a hipGraph capture.  Optional
   * diagnostic marks: events[14] (the ahead chain may begin), events[15] (the main chain has joined). */
  void *ahead_stream;
} imf_fragment_io;

size_t imf_fragment_pyramid_bytes(const imf_fragment_caps *caps);
size_t imf_abi_sizeof_fragment_io(void);               /* sizeof(imf_fragment_io) as the library was built: binding checks */
/* Launches of the main chain that a forward with an ahead_stream carries on it: 0 none, 1 .. 12 conv1 and the first n - 1 encoder
 * convolutions, 13 the fusion too (a static function of the arithmetic and the fragments per forward: 12 for bf16x3 with up to
 * four fragments, where it was measured, else 0; IMF_ENCODER_AHEAD overrides). */
int imf_resunet_encoder_ahead(int variant, int n_items);
long imf_fragment_ahead_forwards(void);                /* forwards the CALLING THREAD has issued with launches on an ahead stream */
/* 1: a launch on stream b runs beside work on stream a (they sit on different hardware queues), 0: it waits behind it -- MEASURED
 * (~0.7 ms, synchronises both streams).  For choosing an ahead_stream: one that shares a queue with main_stream, side_stream or
 * image_stream serialises the forward instead of overlapping it. */
int imf_streams_concurrent(void *a, void *b);
int imf_fragment_forward(const imf_resunet_desc *net /* [host] */, const imf_image_desc *img /* [host] */,
                         const imf_fragment_caps *caps, imf_fragment_io *io);

/* ---- Streaming pipeline: host arrays in -> descriptors on the host, transfers under the neighbouring forwards ----
 * Replaces: the per-fragment body of scripts/generate_desc.py:99-123 (extract_features(...) on host arrays, then
 * feature.detach().cpu().numpy()) = util/misc.py:82-104 end to end, for a stream of fragments.  A job = one
 * imf_fragment_forward (one fragment or a batch) whose inputs sit in a PINNED host block laid out like the bucket's
 * device input block [dyn | images | points] and whose results land in a pinned block laid out like the device output
 * block [meta | xyz_down | descriptors]:
 *     image stream: host_in -> dev_in            (in_bytes; issued behind the PREVIOUS job's image branch)
 *     main stream : imf_fragment_forward(job->io), then xyz_down = xyz[first_idx] into `sel` (imf_gather_points)
 *     side stream : dev_out -> host_out          (meta, and the meta[0] rows of xyz_down and of the descriptors; with
 *                   defer_download issued behind the NEXT job's launches, i.e. behind its coarse levels and rulebooks)
 * ordered by events, so job k+1's upload and job k-1's download run under job k's kernels, in the idle halves of the two
 * streams a forward has besides its main stream (HIP has four hardware queues: further streams would share one of these
 * queues in an order nobody chose).  The transfers are copy KERNELS that address the pinned blocks directly (no copy
 * command ever sits in front of a launch: a hipMemcpyAsync issued behind queued kernels blocks the calling thread on
 * this stack); IMF_PIPELINE_SDMA_COPIES selects hipMemcpyAsync of the whole blocks instead (A/B).  Every HIP call of a
 * job is made by the pipeline's own worker thread: imf_pipeline_submit only queues a copy of the descriptor and returns
 * a ticket (>= 0) at once, imf_pipeline_wait blocks until that job's results are in host_out (it ends a deferral) and
 * frees the ticket.  The caller owns all memory and must not reuse a bucket (job->io and its blocks) or its pinned blocks
 * before the job's wait has returned; jobs run in submit order.  main_stream: a non-blocking stream distinct from every
 * job's io->side_stream / io->image_stream (all jobs of a pipeline should share those two). */
typedef struct imf_job {               /* [host] */
  const imf_resunet_desc *net;
  const imf_image_desc *img;
  const imf_fragment_caps *caps;
  imf_fragment_io *io;                 /* the bucket; main_stream is set by the pipeline */
  const void *host_in; void *dev_in; size_t in_bytes;       /* pinned -> device, 16-byte aligned */
  const void *dev_out; void *host_out; size_t out_bytes;    /* device -> pinned (whole block; SDMA mode copies all of it) */
  double *sel;                         /* device [caps->rows[0], 3] inside dev_out at sel_offset: xyz[first_idx]; NULL: none */
  size_t sel_offset;                   /* byte offset of `sel` in the output block */
  size_t out_offset; int32_t out_row_bytes;                 /* the descriptors' offset in the output block and bytes per row */
  int32_t defer_download;              /* another job follows: issue this one's download behind that job's launches */
} imf_job;
#define IMF_PIPELINE_SDMA_COPIES 1     /* flags bit 0; bits 8..19: workgroups per copy kernel (0 = 64) */
void *imf_pipeline_create(void *main_stream, int depth /* tickets */, int flags);
void imf_pipeline_destroy(void *pipeline);
int imf_pipeline_submit(void *pipeline, const imf_job *job);          /* ticket >= 0, or IMF_E* */
/* ms [host], 24 floats or NULL.  Device (HIP events): [0] upload, [1] upload done -> forward done (includes queueing behind
 * the previous forward), [2] forward done -> download done (includes a deferral).  Host clock: [3] submit -> taken by the
 * worker, [4] -> forward issued, [5] -> download issued, [6] -> seen complete, [7] time spent inside this call.  Time stamps
 * in ms since imf_pipeline_create -- device clock: [8] upload begins, [9] upload ends, [10] forward begins, [11] forward
 * ends, [12] download ends; host clock: [13] submit, [14] forward issued, [15] this call returns, [16] taken by the worker,
 * [17] / [18] upload issue begins / ends, [19] / [20] download issue begins / ends. */
int imf_pipeline_wait(void *pipeline, int ticket, float *ms);
/* [host pointers] float64 -> float32 when every value is a float32 (PLY points widened by the reader,
 * scripts/generate_desc.py:83-84): returns 1 and dst holds the narrowed values, 0 when some value does not survive
 * (the caller stages the float64 rows instead).  Voxels from the narrowed points are bit-identical (the voxeliser
 * widens before its fp64 divide, util/misc.py:82). */
int imf_host_narrow_points(const double *src, int64_t n_values, float *dst);

/* hipGraph plumbing for the above (thread-local capture mode: other host threads may keep using HIP).
 * imf_graph_end_capture instantiates; the handle is replayed with imf_graph_launch on any stream. */
int imf_graph_begin_capture(void *stream);
int imf_graph_end_capture(void *stream, void **graph_exec_out /* [host] */, int *n_nodes_out /* [host] or NULL */);
int imf_graph_abort_capture(void *stream);
int imf_graph_launch(void *graph_exec, void *stream);
void imf_graph_destroy(void *graph_exec);

/* ---- Descriptor matching for feature-match recall ---------------------------------
 * imf_nn_search replaces util/uio.py:245-258 `knn_search(points_src, points_dst, k=1)` (one Open3D
 * KD-tree query per row, fp64) as called twice at scripts/evaluation_3dmatch.py:207-210: for every
 * row of `query` [n_query, dim] the index of the row of `db` [n_db, dim] with the smallest squared L2
 * distance.  Scores |d|^2 - 2 q.d are formed in fp64 (f64 matrix pipe) from exact products, so each is
 * within E(q, d) = 2 (dim + 2) 2^-53 (|q| + |d|)^2 of its exact value (derived in csrc/matching.hip): the
 * row returned is within E(q, got) + E(q, argmin) of the nearest squared distance, and is the exact argmin
 * wherever the best two distinct distances differ by more than the sum of their E.  Bitwise equal rows
 * score bitwise equally; ties go to the lowest index.
 * dim in {16, 32, 64}.  nn_dist2 (optional, may be null) receives the squared distance in fp64, within
 * 2 E of the exact value.
 * Non-finite rows: a db row holding a NaN or an infinity is never chosen, whatever the query; a query
 * that is left without a row (its own row is not finite, or no db row is) gets nn_index = -1 and
 * nn_dist2 = NaN.  Consumers treat a negative index as "no neighbour".
 * workspace: imf_nn_workspace_bytes(n_query, n_db) bytes of device memory. */
size_t imf_nn_workspace_bytes(int64_t n_query, int64_t n_db);
int imf_nn_search(const float *query, int64_t n_query, const float *db, int64_t n_db, int dim,
                  int32_t *nn_index, double *nn_dist2, void *workspace, size_t workspace_bytes,
                  void *stream);
/* imf_mutual_inliers replaces scripts/evaluation_3dmatch.py:212-234: frag2 index j survives iff
 * nn12[nn21[j]] == j; survivors are written ascending to match_idx2 (capacity n2).  When kpts1
 * [n1,3], kpts2 [n2,3] (device fp64) and pose_host (HOST pointer, 16 doubles, row-major 4x4) are all
 * non-null, each surviving frag2 keypoint is transformed by the pose (homogeneous multiply and
 * divide by w, as Open3D's PointCloud::transform) and counted as an inlier when its distance to
 * kpts1[nn21[j]] is < inlier_thresh.  meta (device int32[2]) = {n_matches, n_inliers}. */
int imf_mutual_inliers(const int32_t *nn21, int64_t n2, const int32_t *nn12, int64_t n1,
                       const double *kpts1, const double *kpts2, const double *pose_host,
                       double inlier_thresh, int32_t *match_idx2, int32_t *meta, void *stream);

/* ---- Keypoint -> voxel selection of the evaluator ----------------------------------
 * Replaces scripts/evaluation_3dmatch.py:162-171: the ascending indices i of the rows of `coords`
 * [n_voxels,3] (the `xyz` array of a descriptor file, device fp64) whose key
 * ME.utils.fnv_hash_vec(floor(coords[i] / voxel_size)) occurs among the keys of `samples`
 * [n_samples,3] (the sampled raw points, device fp64) -- np.where(np.isin(key_coords, key_points))[0].
 * inds: device int32, capacity n_voxels; count: device int32[1].  Same FNV-1a-64 key as the
 * reference, so the selected set is identical even under a key collision. */
size_t imf_keypoint_workspace_bytes(int64_t n_samples, int64_t n_voxels);
int imf_select_keypoints(const double *samples, int64_t n_samples, const double *coords, int64_t n_voxels,
                         double voxel_size, int32_t *inds, int32_t *count, void *workspace,
                         size_t workspace_bytes, void *stream);

/* ---- RANSAC registration on feature correspondences -------------------------------
 * Replaces scripts/benchmark_util.py:16-34 run_ransac = Open3D 0.12
 * registration_ransac_based_on_feature_matching(..., TransformationEstimationPointToPoint(False),
 * ransac_n, [EdgeLength(edge_similarity), Distance(max_corr_dist)], RANSACConvergenceCriteria(max_iter,
 * 1000), mutual_filter=False) given the correspondences corres[i] = nearest target feature of source
 * point i (imf_nn_search(src_feat, dst_feat)).  src [n_src,3], dst [n_dst,3] device fp64.  An entry
 * corres[i] < 0 or >= n_dst is "no correspondence": a hypothesis that draws one fails the checkers (it is
 * not counted in out_meta[2]), the entry is never an inlier, dst is never read outside [0, n_dst); the
 * draws (r % n_src) and the fitness denominator n_src are unaffected.  All
 * max_iter hypotheses are drawn (the reference's second criterion never fires); the draw sequence is a
 * counter-based generator of `seed` (Open3D's clock-seeded one cannot be reproduced), identical in
 * the oracle.  out_T: device 16 doubles, row-major 4x4 source->target (identity if nothing survives);
 * out_meta: device int32[3] = {winning iteration or -1, its inlier count, hypotheses that passed the
 * checkers}; out_stats: device double[2] = {fitness, inlier RMSE}. */
size_t imf_ransac_workspace_bytes(int max_iter);
int imf_ransac_registration(const double *src, int64_t n_src, const double *dst, int64_t n_dst,
                            const int32_t *corres, int ransac_n, double max_corr_dist, double edge_similarity,
                            int max_iter, uint64_t seed, double *out_T, int32_t *out_meta, double *out_stats,
                            void *workspace, size_t workspace_bytes, void *stream);
/* [host pointers, no GPU] The rigid fit dst ~ R src + t that RANSAC's hypotheses and ICP's iterations share
 * (csrc/registration.h), on n >= 1 pairs src, dst [n,3]: T12 receives the row-major 3x4 [R | t].  R is a proper
 * rotation for every input: the SVD answer at rank 3 and 2; at rank 1 the least-angle rotation between the two
 * directions (a half turn about a fixed perpendicular axis when they are opposite); at rank 0 the identity. */
int imf_host_rigid_fit(const double *src, const double *dst, int n, double *T12);

/* ---- Point-to-point ICP and the radius-count overlap test (the KITTI evaluation, imfnet_amd/evaluate_kitti.py) ----
 * imf_icp_point_to_point replaces Open3D 0.12 registration_icp(src, dst, max_corr_dist, init,
 * TransformationEstimationPointToPoint(), ICPConvergenceCriteria(max_iteration)) with the default relative fitness /
 * RMSE of 1e-6, as lib/data_loaders.py:527-556 refines the KITTI ground truth (the loop restated in csrc/icp.hip):
 * correspondence = nearest target point with d^2 < max_corr_dist^2 (strict; ties -> lowest target index), Umeyama
 * update without scaling, incremental transform of the current points, stop when fitness and RMSE both move by
 * < 1e-6.  src [n_src,3], dst [n_dst,3] device fp64; init_host: HOST pointer, 16 doubles row-major, or NULL =
 * identity.  Outputs (device): out_T 16 doubles (row-major 4x4 source->target), out_stats double[2] = {fitness,
 * inlier RMSE}, out_meta int32[3] = {loop iterations run, final correspondences, 1 if a target point was NaN / out of
 * the grid's range}.  Enqueues 2 (max_iteration + 1) + 5 launches, no host synchronisation; fp64 throughout, no
 * floating-point atomics: bit-identical from run to run.  workspace: 256-byte aligned. */
size_t imf_icp_workspace_bytes(int64_t n_src, int64_t n_dst);
int imf_icp_point_to_point(const double *src, int64_t n_src, const double *dst, int64_t n_dst, double max_corr_dist,
                           const double *init_host, int max_iteration, double *out_T, double *out_stats,
                           int32_t *out_meta, void *workspace, size_t workspace_bytes, void *stream);
/* imf_icp_point_to_plane.  Replaces: Open3D registration_icp(src, dst, max_corr_dist, init,
 * TransformationEstimationPointToPlane(), ICPConvergenceCriteria(max_iteration)) on a target with normals (nothing upstream
 * calls it; it is the refinement of imfnet_amd/register.py).  Everything of imf_icp_point_to_point holds -- the loop, the
 * correspondence rule, fitness, rmse over point distances, the stop rule, the outputs, 2 (max_iteration + 1) + 5 launches,
 * bit-identical runs -- except the update: r = (p - q) . n_q, J = [p x n_q, n_q], (sum J^T J) x = -(sum J^T r) by LDL^T,
 * update = [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5].  dst_normals: device fp64 [n_dst,3], row j the normal of dst row j.  The
 * singular rule: a pivot <= 1e-12 times the largest diagonal entry of sum J^T J (a single-plane target, fewer than 6
 * independent rows) makes the update the identity.  workspace: imf_icp_plane_workspace_bytes, 256-byte aligned. */
size_t imf_icp_plane_workspace_bytes(int64_t n_src, int64_t n_dst);
int imf_icp_point_to_plane(const double *src, int64_t n_src, const double *dst, const double *dst_normals, int64_t n_dst,
                           double max_corr_dist, const double *init_host, int max_iteration, double *out_T,
                           double *out_stats, int32_t *out_meta, void *workspace, size_t workspace_bytes, void *stream);
/* imf_color_gradient.  Replaces: nothing upstream; the per-point colour gradient Open3D's registration_colored_icp
 * (TransformationEstimationForColoredICP; Park, Zhou, Koltun, ICCV 2017) prepares for its target, restated -- the rule, and
 * that it is recalled rather than checked, is stated in csrc/colored_icp.hip.  The entry does not search: neighbors int32
 * [n,knn] and counts int32 [n] are the lists imf_estimate_normals wrote for the same points (the point itself included,
 * padded with -1; entries outside [0, n) are skipped).  points, normals: device fp64 [n,3]; intensity: device fp64 [n];
 * 1 <= n < 2^30; 1 <= knn <= 64.  Output (device): out_grad fp64 [n,3], the least-squares gradient of the intensity in the
 * tangent plane of every point, 0 where the list has fewer than 4 entries or the 3x3 system is singular (a pivot <= 1e-12
 * times the largest diagonal entry).  fp64 without fused multiply-add, butterfly sums over the list positions, no
 * floating-point atomics: bit-identical from run to run.  1 launch, no workspace, no host synchronisation. */
int imf_color_gradient(const double *points, const double *normals, const double *intensity, const int32_t *neighbors,
                       const int32_t *counts, int64_t n, int knn, double *out_grad, void *stream);
/* imf_icp_colored.  Replaces: Open3D registration_colored_icp(src, dst, max_corr_dist, init,
 * TransformationEstimationForColoredICP(lambda_geometric), ICPConvergenceCriteria(max_iteration)) (nothing upstream calls
 * it; it is `--refine color` of imfnet_amd/register.py and reconstruct.py).  Everything of imf_icp_point_to_plane holds
 * -- the loop, the correspondence rule, fitness, rmse over point distances, the stop rule, the outputs, the launches, the
 * LDL^T solve and its singular rule, bit-identical runs -- except the sums of the update, which are those of
 * lambda J_G^T J_G + (1 - lambda) J_I^T J_I and lambda J_G r_G + (1 - lambda) J_I r_I (csrc/colored_icp.hip).
 * src_intensity: device fp64 [n_src], row i the intensity of src row i; dst_normals, dst_gradient: device fp64 [n_dst,3],
 * dst_intensity: device fp64 [n_dst], row j belonging to dst row j (dst_gradient: imf_color_gradient's output).
 * 0 <= lambda_geometric <= 1; 1 forms point-to-plane's sums exactly.  workspace: imf_icp_colored_workspace_bytes,
 * 256-byte aligned. */
size_t imf_icp_colored_workspace_bytes(int64_t n_src, int64_t n_dst);
int imf_icp_colored(const double *src, const double *src_intensity, int64_t n_src, const double *dst,
                    const double *dst_normals, const double *dst_intensity, const double *dst_gradient, int64_t n_dst,
                    double max_corr_dist, double lambda_geometric, const double *init_host, int max_iteration, double *out_T,
                    double *out_stats, int32_t *out_meta, void *workspace, size_t workspace_bytes, void *stream);
/* imf_rgbd_prepare, imf_rgbd_odometry.  Replaces: nothing upstream; Open3D's compute_rgbd_odometry with the hybrid term
 * (Steinbruecker 2011; Park, Zhou, Koltun 2017), the frame-to-frame step in front of the fragment fusion of Choi, Zhou,
 * Koltun 2015, restated -- the rules, and that they are recalled rather than checked, are stated in csrc/odometry.hip.
 * imf_rgbd_prepare builds the pyramids of one frame into an opaque device block of imf_rgbd_frame_bytes(h, w, levels) bytes
 * (0 for a shape it refuses), 256-byte aligned: smoothed intensity, depth (NaN where invalid), their Sobel gradients, per
 * level.  depth_u16: device uint16 [h,w]; color_u8: device uint8 [h,w,3]; 1 <= levels <= 5; h and w divisible by
 * 2^(levels-1), the coarsest level at least 3 x 3; depth valid iff u16 > 0 and depth_min < u16 / depth_scale < depth_max;
 * depth_edge > 0: the largest depth step inside a 3 x 3 neighbourhood that still has a depth gradient.  2 levels + 1 launches.
 * imf_rgbd_odometry fits src_frame onto dst_frame (both blocks of imf_rgbd_prepare, of one shape; the two headers are read
 * back once before anything is enqueued, after that the host never waits): iterations: HOST int[n_iterations], coarsest level
 * first, n_iterations = the frames' levels, every count >= 1; init_host: HOST double[16] row-major or NULL = identity;
 * 0 <= lambda_depth <= 1; a stage with fewer than min_corr correspondences has the identity update.  Outputs (device):
 * out_T fp64 [16], source camera into target camera; out_info fp64 [36], the 6 x 6 system matrix of a last stage at level 0,
 * exactly symmetric; out_stats fp64 [2] = fitness (correspondences / valid source pixels at level 0), cost; out_meta int32 [4]
 * = correspondences, flags (bit 0: a stage had too few correspondences or a singular system; bit 1: the last stage had:
 * the pair is lost), stages run (the last included), valid source pixels.  fp64 without fused multiply-add in every per-pixel
 * quantity, fixed summation order, integer atomics only (the occlusion test): bit-identical from run to run.
 * workspace: imf_rgbd_odometry_workspace_bytes(h, w, levels) (0 for a shape refused), 256-byte aligned.
 * imf_rgbd_odometry_stage is the test surface: one stage at `level` with T_dev (DEVICE double[16]); out_winner int32
 * [h_l, w_l] (the source index v w + u that won the target pixel, or -1), out_sums fp64 [29] (correspondences, cost, the 21
 * upper entries of the system matrix row-major, the 6 of the right-hand side). */
size_t imf_rgbd_frame_bytes(int h, int w, int levels);
int imf_rgbd_prepare(const uint16_t *depth_u16, const uint8_t *color_u8, int h, int w, double fx, double fy, double cx,
                     double cy, double depth_scale, double depth_min, double depth_max, double depth_edge, int levels,
                     void *frame, size_t frame_bytes, void *stream);
size_t imf_rgbd_odometry_workspace_bytes(int h, int w, int levels);
int imf_rgbd_odometry(const void *src_frame, const void *dst_frame, const double *init_host, const int *iterations,
                      int n_iterations, double max_depth_diff, double lambda_depth, int min_corr, double *out_T,
                      double *out_info, double *out_stats, int32_t *out_meta, void *workspace, size_t workspace_bytes,
                      void *stream);
int imf_rgbd_odometry_stage(const void *src_frame, const void *dst_frame, int level, const double *T_dev,
                            double max_depth_diff, double lambda_depth, int32_t *out_winner, double *out_sums,
                            void *workspace, size_t workspace_bytes, void *stream);
/* imf_estimate_normals.  Replaces: o3d.geometry.PointCloud.estimate_normals with its default KDTreeSearchParamKNN(knn=30)
 * (data/fuse_fragments_3DMatch.py:89), exactly (the rules are stated in csrc/normals.hip).  points: device fp64 [n,3];
 * 1 <= knn <= 64; max_radius finite and > 0: the neighbour set of point i is the knn smallest of (d^2, index) among the
 * points with d^2 <= max_radius^2, itself included; viewpoint_host: HOST double[3] or NULL.  Outputs (device): normals fp64
 * [n,3], the unit eigenvector of the smallest eigenvalue of the set's two-pass covariance ((0,0,1) for fewer than 3 points),
 * signed so that n . (viewpoint - p) >= 0, or with its largest component positive when viewpoint is NULL; counts int32 [n],
 * the size of every set; nbr: optional int32 [n,knn], the sets in (d^2, index) order padded with -1; out_err int32[1], 1 if
 * a point was NaN / out of the grid's range (cell edge max_radius / 2).  5 launches, no host synchronisation, no
 * floating-point atomics: bit-identical from run to run.  workspace: imf_normals_workspace_bytes(n), 256-byte aligned. */
size_t imf_normals_workspace_bytes(int64_t n);
int imf_estimate_normals(const double *points, int64_t n, int knn, double max_radius, const double *viewpoint_host,
                         double *normals, int32_t *counts, int32_t *nbr, int32_t *out_err, void *workspace,
                         size_t workspace_bytes, void *stream);
/* imf_fpfh_features.  Replaces: nothing upstream; Open3D's compute_fpfh_feature (Rusu 2009) restated -- the rules, and
 * which of them are recalled rather than checked, are stated in csrc/fpfh.hip.  The entry does not search: nbr int32
 * [n,knn] and counts int32 [n] are the lists imf_estimate_normals wrote for the same points (the point itself included,
 * padded with -1); entries equal to i or outside [0, n) are skipped.  points, normals: device fp64 [n,3]; 1 <= n < 2^30;
 * 1 <= knn <= 64; width 33 or 64.  Outputs (device): out fp32 [n,width], the 33 FPFH bins (three groups of 11, each
 * summing to 200, or to 100 where no neighbour is at d^2 > 0) and +0.0f in columns 33..; out_hist: optional int32 [n,33],
 * the integer SPFH pair counts (rows sum to 3 m_i).  fp64 throughout without fused multiply-add, one rounding to fp32.
 * 2 launches, no host synchronisation, no atomics: bit-identical from run to run.  workspace:
 * imf_fpfh_workspace_bytes(n, knn) (0 for arguments out of range), 256-byte aligned. */
size_t imf_fpfh_workspace_bytes(int64_t n, int knn);
int imf_fpfh_features(const double *points, const double *normals, int64_t n, const int32_t *nbr, const int32_t *counts,
                      int knn, int width, float *out, int32_t *out_hist, void *workspace, size_t workspace_bytes,
                      void *stream);
/* imf_information_matrix.  Replaces: nothing upstream computes it; it is the 6x6 matrix of a 3DMatch gt.info record, Open3D's
 * GetInformationMatrixFromPointClouds(source, target, max_corr_dist, T) restated -- the rules, recalled rather than checked,
 * are stated in csrc/information.hip.  Every source point p = T src_s takes imf_icp_point_to_point's correspondence (nearest
 * target with d^2 < max_corr_dist^2, strict; ties -> lowest target index; the same grid), and each correspondence adds G^T G
 * with G = [-[q]x | I] of the TARGET point q (rotation first).  src [n_src,3], dst [n_dst,3]: device fp64; T_host: HOST 16
 * doubles row-major or NULL = identity.  Outputs (device): out_info double[36], row-major, exactly symmetric, entries [3,3] =
 * [4,4] = [5,5] = the number of correspondences, 36 times +0.0 without any; out_meta int32[2] = {correspondences, 1 if a
 * target point was NaN / out of the grid's range}.  6 launches, no host synchronisation, fp64 without fused multiply-add in
 * the sums, no floating-point atomics: bit-identical from run to run.  workspace: imf_information_workspace_bytes(n_src,
 * n_dst) (0 for arguments out of range), 256-byte aligned. */
size_t imf_information_workspace_bytes(int64_t n_src, int64_t n_dst);
int imf_information_matrix(const double *src, int64_t n_src, const double *dst, int64_t n_dst, const double *T_host,
                           double max_corr_dist, double *out_info, int32_t *out_meta, void *workspace,
                           size_t workspace_bytes, void *stream);
/* imf_radius_count replaces len(get_matching_indices(pcd0, pcd1, trans, r)) of util/pointcloud.py:56-69 (the
 * KITTI evaluator's "fewer than 1000 matches" skip, lib/data_loaders.py:586-588): the number of pairs (i, j) with
 * |T src_i - dst_j| <= r.  T_host: HOST 16 doubles row-major or NULL = identity.  out_count: device int64[1];
 * out_per_point: optional device int32[n_src], each source point's count; out_err: device int32[1], 1 if a target
 * point was NaN / out of range.  workspace: imf_radius_count_workspace_bytes(n_dst), 256-byte aligned. */
size_t imf_radius_count_workspace_bytes(int64_t n_dst);
int imf_radius_count(const double *src, int64_t n_src, const double *dst, int64_t n_dst, const double *T_host, double r,
                     int64_t *out_count, int32_t *out_per_point, int32_t *out_err, void *workspace,
                     size_t workspace_bytes, void *stream);
/* imf_radius_pairs replaces the pairs of get_matching_indices(pcd0, pcd1, trans, r) (util/pointcloud.py:56-69), the
 * positive pairs of the training data set (lib/data_loaders.py:313): every (i, j) with |T src_i - dst_j| <= r, the bound
 * and transform arithmetic of imf_radius_count.  offsets: device int64[n_src+1], the CSR row start of every source point
 * (always written); pairs: device int32[capacity][2] = (i, j), 8-byte aligned, row i's j ascending (FLANN orders a row
 * by distance; the set is the same).  out_total: device int64[1], always written; when it exceeds capacity no pair is
 * written (the caller reallocates and calls again).  out_err: device int32[1], 1 if a target point was NaN / out of
 * range.  n_src == 0 or n_dst == 0: total 0, no kernel launched (workspace may be NULL).  Integer counts, no
 * floating-point atomics: bit-identical from run to run.  workspace: imf_radius_pairs_workspace_bytes(n_src, n_dst),
 * 256-byte aligned. */
size_t imf_radius_pairs_workspace_bytes(int64_t n_src, int64_t n_dst);
int imf_radius_pairs(const double *src, int64_t n_src, const double *dst, int64_t n_dst, const double *T_host, double r,
                     int64_t *offsets, int32_t *pairs, int64_t capacity, int64_t *out_total, int32_t *out_err,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- Robust transform from correspondences (the trainer's validation: RTE / RRE / success) ------------------------------
 * imf_robust_transform replaces util/transform_estimation.py:89-116 est_quad_linear_robust(pts0, pts1, weight): 20
 * rounds of the small-angle linear fit (3n x 6 system of the current points, normal equations, Rz Ry Rx and a
 * translation from the six unknowns, points moved, T composed), every pair reweighted by par / (|p0 - p1| + par) with
 * par = 1 halved at rounds 5, 10 and 15 (the loop restated in csrc/robust.hip).  pts0, pts1 [n,3] device fp64, row i
 * of one corresponding to row i of the other; weight: device fp64 [n] for the first round, or NULL = ones.  Outputs
 * (device): out_T 16 doubles (row-major 4x4, pts0 -> pts1), out_meta int32[1] = 1 when a round's system could not be
 * solved (fewer than three usable rows, collinear points, a NaN or infinite input; upstream raises from torch.inverse),
 * in which case out_T is the identity and the call still returns 0.  n == 0: the same flag and the identity, no kernel
 * launched (pts0 / pts1 may be NULL).  ONE launch of one workgroup of 512 threads, no host synchronisation; fp64 throughout (upstream:
 * float32), no floating-point atomics, a fixed summation order: bit-identical from run to run.  workspace:
 * imf_robust_transform_workspace_bytes(n) bytes, 256-byte aligned; 0 (workspace may be NULL) while every thread's rows
 * fit its registers, n <= 5120. */
size_t imf_robust_transform_workspace_bytes(int64_t n);
int imf_robust_transform(const double *pts0, const double *pts1, const double *weight, int64_t n, double *out_T,
                         int32_t *out_meta, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Fragment fusion: depth frames -> sparse TSDF volume -> surface points (imfnet_amd/fuse.py) -------------------------
 * Replace Open3D 0.12 ScalableTSDFVolume(voxel_length, sdf_trunc).integrate(...) per frame and extract_point_cloud() as
 * data/fuse_fragments_3DMatch.py:47-96 builds a fragment (the loop restated in csrc/tsdf.hip; no normals;
 * colour: the _rgb calls below).
 * The volume is a set of units of 16^3 voxels: `table` (imf_slot[table_capacity], a power of two >= 2 unit_capacity:
 * imf_hash_capacity(unit_capacity)) maps a unit's integer coordinate to its row, `units` int32 [unit_capacity,3] = (x, y, z)
 * lists the rows in ascending (z, y, x), `voxels` float32 [rows, 4096, 2] = (tsdf, weight) of voxel (z * 16 + y) * 16 + x,
 * zeroed by the caller.  A voxel's sample position is (16 unit + local + lattice_offset) * voxel_length per axis:
 * lattice_offset 0.5 = Open3D's voxel centres, 0 = the lattice the published 3DMatch fragments lie on.  All buffers are
 * device memory of the caller; depth is uint16 [n_frames, height, width]; the matrices are device fp64 [n_frames, 12],
 * row-major 3x4.  No host synchronisation, integer atomics only, a fixed frame order: bit-identical from run to run.
 * workspace: 256-byte aligned.  The *_workspace_bytes queries answer 0 for a size the call refuses. */
typedef struct imf_tsdf_params {
  double fx, fy, cx, cy;       /* pinhole intrinsics in pixels                                              */
  double voxel_length;         /* m; upstream: tsdf_cubic_size / 512                                        */
  double sdf_trunc;            /* m; upstream: 0.04                                                         */
  double depth_scale;          /* raw depth units per metre (1000); the quotient is taken in float32        */
  double depth_trunc;          /* m; a depth beyond it is no measurement                                    */
  double lattice_offset;       /* in [0, 1): 0.5 or 0                                                       */
  int32_t height, width;
} imf_tsdf_params;
/* Opens the units around every stride-4 depth sample of all frames (cam2world: camera -> volume) and rebuilds the sorted
 * unit list.  reset != 0 empties the table first; reset == 0 adds to it (rows change: only before the first integrate).
 * n_units: device int32[2] = {units in the table, flags: 1 = a sample beyond the coordinate range or a NaN pose was left
 * out, 2 = more than unit_capacity units: list and rows are incomplete, call again with more room}. */
size_t imf_tsdf_allocate_workspace_bytes(int64_t unit_capacity);
int imf_tsdf_allocate(const uint16_t *depth, int n_frames, const double *cam2world, const imf_tsdf_params *params,
                      int reset, imf_slot *table, int64_t table_capacity, int32_t *units, int64_t unit_capacity,
                      int32_t *n_units, void *workspace, size_t workspace_bytes, void *stream);
/* The running average of every voxel of the first min(n_units[0], max_units) units over the frames in frame order
 * (world2cam: volume -> camera).  One workgroup per unit; max_units workgroups are launched.
 * Precondition of imf_tsdf_integrate and imf_tsdf_integrate_rgb: every world2cam is rigid (the singular values of its
 * rotation block within 1e-6 of 1; float32-rounded poses are) or holds a NaN, which skips the frame.  The frustum cull
 * relies on it and the calls do not check it: a pose with scale silently loses voxels of partly visible units. */
int imf_tsdf_integrate(const uint16_t *depth, int n_frames, const double *world2cam, const imf_tsdf_params *params,
                       const int32_t *units, const int32_t *n_units, int64_t max_units, float *voxels, void *stream);
/* One point per sign change between a voxel and its +x / +y / +z neighbour, fp64 [n,3] in the order (unit, voxel, axis).
 * out_n: device int64[1], always written; when it exceeds capacity nothing is written to out (capacity 0: count only,
 * out may be NULL). */
size_t imf_tsdf_extract_workspace_bytes(int64_t max_units);
int imf_tsdf_extract(const float *voxels, const int32_t *units, const int32_t *n_units, int64_t max_units,
                     const imf_slot *table, int64_t table_capacity, const imf_tsdf_params *params, double *out,
                     int64_t capacity, int64_t *out_n, void *workspace, size_t workspace_bytes, void *stream);
/* The triangle mesh of the volume: marching tetrahedra on the Kuhn split of every cell whose eight samples are valid
 * (w != 0 and tsdf < 0.98; inside = tsdf < 0); the rule stands at the head of csrc/tsdf_mesh.hip.  out_vertices fp64 [n,3]
 * in the order (unit, voxel, edge slot), out_triangles int32 [m,3] in the order (unit, cell, tetrahedron, triangle),
 * counter-clockwise seen from the free-space side.  out_n: device int64[2] = {vertices, triangles}, always written; when
 * either exceeds its capacity, or the vertices exceed 2^31 - 1 (the indices are int32), nothing is written to the
 * outputs (both capacities 0: count only, the outputs may be NULL).  No host synchronisation, integer atomics only and
 * none of them decides an output position: two calls give the same bytes. */
size_t imf_tsdf_mesh_workspace_bytes(int64_t max_units);
int imf_tsdf_mesh(const float *voxels, const int32_t *units, const int32_t *n_units, int64_t max_units,
                  const imf_slot *table, int64_t table_capacity, const imf_tsdf_params *params, double *out_vertices,
                  int64_t vertex_capacity, int32_t *out_triangles, int64_t triangle_capacity, int64_t *out_n,
                  void *workspace, size_t workspace_bytes, void *stream);
/* Colour (Open3D's RGB8 volumes; the rule stands at the head of csrc/tsdf.hip).  The three calls below are the three calls
 * above with colour: they leave the same (tsdf, weight) state, points, vertices and triangles, bit for bit, keep the same
 * count-only contract and make the same refusals; a NULL `color`, `colors` or (with a non-zero capacity) `out_rgb` is
 * refused with a message that names the argument.
 * `colors`: the colour state, float32 [rows, 3, 4096] on the 0..255 scale, a buffer of its own beside `voxels` (which
 * keeps its layout), zeroed by the caller: per unit three planes of 4096, plane k = channel k (R, G, B) of voxel
 * (z * 16 + y) * 16 + x.  Planes, not [4096, 3] or a padded [4096, 4]: a wavefront's 64 voxels read and write 64 consecutive
 * dwords per channel, and nothing is padded (12 bytes per voxel).
 * imf_tsdf_integrate_rgb: `color` uint8 [n_frames, height, width, 3] (R, G, B) beside `depth`; whenever a frame updates a
 * voxel's tsdf, c[k] = (c[k] * w + color[v][u][k]) / (w + 1) in float32 with the weight before the increment.
 * imf_tsdf_extract_rgb / imf_tsdf_mesh_rgb: `out_rgb` uint8 [capacity, 3] / [vertex_capacity, 3]; row i is the colour of
 * row i of out / out_vertices: c_lo + t (c_hi - c_lo) in fp64 with the t of the position, floor(c + 0.5) clamped. */
int imf_tsdf_integrate_rgb(const uint16_t *depth, const uint8_t *color, int n_frames, const double *world2cam,
                           const imf_tsdf_params *params, const int32_t *units, const int32_t *n_units, int64_t max_units,
                           float *voxels, float *colors, void *stream);
int imf_tsdf_extract_rgb(const float *voxels, const float *colors, const int32_t *units, const int32_t *n_units,
                         int64_t max_units, const imf_slot *table, int64_t table_capacity, const imf_tsdf_params *params,
                         double *out, uint8_t *out_rgb, int64_t capacity, int64_t *out_n, void *workspace,
                         size_t workspace_bytes, void *stream);
int imf_tsdf_mesh_rgb(const float *voxels, const float *colors, const int32_t *units, const int32_t *n_units,
                      int64_t max_units, const imf_slot *table, int64_t table_capacity, const imf_tsdf_params *params,
                      double *out_vertices, uint8_t *out_rgb, int64_t vertex_capacity, int32_t *out_triangles,
                      int64_t triangle_capacity, int64_t *out_n, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Fragment overlap: the 3DMatch training-pair builder (imfnet_amd/overlap.py, imfnet_amd.compute_overlap) ------------
 * Replace the pyflann nearest-neighbour queries of data/compute_overlap.py:93-141 (the loop restated in csrc/overlap.hip):
 * for a pair (p, q) every point of q gets its EXACT nearest point of p (float32 d2 = (dx dx + dy dy) + dz dz without
 * fused multiply-adds, equal distances to the lowest p index), kept when sqrtf(d2) <= thresh; the rows (i, j) ascend in j.
 * A sequence-level engine: an index per fragment, built once and resident; a bound for all candidate pairs in one launch;
 * the exact pass and the emit per surviving pair.  All buffers are device memory of the caller unless marked HOST; no
 * host synchronisation inside a call, integer atomics only, no atomic decides an output position: bit-identical from run
 * to run.  workspace / storage: 256-byte aligned.  The *_bytes queries answer 0 for a size the call refuses. */
typedef struct imf_overlap_index {
  imf_slot *table;        /* [capacity] key = cell, val = first sorted row, pad = points of the cell             */
  int64_t capacity;       /* imf_hash_capacity(n)                                                                */
  float *xyz;             /* [n,3] the points sorted by cell                                                     */
  int32_t *idx;           /* [n] original index of every sorted row                                              */
  int32_t *cells;         /* [n] slots of the occupied cells, ascending; meta[0] are valid                       */
  int32_t *chunks;        /* [n,2] (slot, first point within the cell) of every run of <= 256 points; meta[1]    */
  int32_t *meta;          /* [4] occupied cells, chunks, flags (1 = a NaN / out-of-range point left out), points */
  int64_t n;
  double cell;            /* cell edge, m                                                                        */
} imf_overlap_index;
/* Builds the index of points float32 [n,3] into `storage` (imf_overlap_index_bytes(n)) and fills the HOST struct *index
 * with pointers into it.  cell: the edge; imf_overlap_pair needs it above thresh (1 + 2^-20), see csrc/overlap.hip. */
size_t imf_overlap_index_bytes(int64_t n);
size_t imf_overlap_index_workspace_bytes(int64_t n);
int imf_overlap_index_build(const float *points, int64_t n, double cell, void *storage, size_t storage_bytes,
                            imf_overlap_index *index, void *workspace, size_t workspace_bytes, void *stream);
/* The prefilter.  indices: DEVICE array of index structs; pairs: device int32 [n_pairs,2] = (p, q) positions in it;
 * bound: device int64 [n_pairs] = the points of q whose cell has an occupied cell of p among its 27 neighbours, an upper
 * bound of the exact pass's row count.  max_cells: at least the largest meta[0] of the q side.  n_pairs <= 65535. */
int imf_overlap_bound(const imf_overlap_index *indices, const int32_t *pairs, int n_pairs, int64_t max_cells,
                      int64_t *bound, void *stream);
/* The exact pass.  p, q: HOST structs.  nn_idx: device int32 [q->n], the nearest p index of every point of q, -1 where
 * none is within thresh.  max_chunks: at least q's meta[1] (workgroups launched). */
int imf_overlap_pair(const imf_overlap_index *p, const imf_overlap_index *q, float thresh, int64_t max_chunks,
                     int32_t *nn_idx, void *stream);
/* Order-preserving compaction: pairs int64 [n_q,2] receives the rows (nn_idx[j], j) with nn_idx[j] >= 0 in ascending j,
 * out_n: device int64[1] their number. */
size_t imf_overlap_emit_workspace_bytes(int64_t n_q);
int imf_overlap_emit(const int32_t *nn_idx, int64_t n_q, int64_t *pairs, int64_t *out_n, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ---- Training backward of the sparse convolution (last item) ---------------------------------------
 * Replaces: the backward of ME.MinkowskiConvolution / ConvolutionTranspose under loss.backward(), lib/trainer.py:495-569.
 * The INPUT gradient is imf_spconv_fwd itself over the opposite kernel map with transposed weights
 * (imfnet_amd/autograd.py: same map with W[K-1-k]^T at stride 1, the transposed map for a strided convolution, the
 * strided map for a transposed one).  The WEIGHT gradient is this entry point:
 *     dw[k][ci][co] = sum over the pairs (i, o) of offset k of  in[i][ci] * grad_out[o][co]
 * over the same rulebook the forward used (tile_rows / nbr as in imf_conv_args; nbr NULL = identity when kvol == 1).
 * Any cin, cout >= 1 (tests/test_gpu_backward_exact.py::test_wgrad_is_exact_on_integer_data: channel counts off the
 * 32-wide block, slot counts on and around the 4096-slot chunk, padding, permuted slots, empty offsets).  Deterministic:
 * chunk partials summed in order, no float atomics, two calls give the same bits
 * (::test_wgrad_on_float_data_is_reproducible_and_within_the_summation_bound).  fp32 on the vector pipe whatever the
 * convolutions' arithmetic.  Bad arguments return IMF_EINVAL before any launch.
 * workspace: imf_spconv_wgrad_workspace_bytes. */
size_t imf_spconv_wgrad_workspace_bytes(int64_t n_slots, int kvol, int cin, int cout);
int imf_spconv_wgrad(const float *in, int cin, const float *grad_out, int cout, const int32_t *tile_rows,
                     const int32_t *nbr, int64_t n_slots, int64_t n_out, int kvol, float *dw /* [kvol][cin][cout] */,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- Training-mode BatchNorm of the sparse path (csrc/norm_train.hip) --------------------------------------------------
 * Replaces: ME.MinkowskiBatchNorm in training mode (nn.BatchNorm1d over the rows of the batched sparse tensor) and the
 * ReLU / residual add that follow it in the residual block (model/residual_block.py:40-56), forward and backward.
 * All features are row-major fp32 [n, c], any c >= 1; rows move as 16-byte vectors when c % 4 == 0 and the pointers are
 * 16-byte aligned.  Batch statistics are fp64 sums over chunks of imf_bn_train_chunk_rows() rows (the cut depends on n
 * only), chunk partials added in chunk order by one workgroup: no floating-point atomics, two calls give the same bits.
 * Every call takes a stream and synchronises nothing.  Bad arguments (n < 2 -- torch refuses one value per channel in
 * training mode, and so does this --, c < 1, a short workspace, a null required pointer) return IMF_EINVAL before any
 * launch.  workspace: imf_bn_train_workspace_bytes(n, c), 8-byte aligned, for either call.
 *
 * forward:  stats[0..c) = batch mean, stats[c..2c) = 1 / sqrt(biased variance + eps), both fp64;
 *           xh = fp32((double(x) - mean) * rstd);  y = fmaf(xh, gamma, beta) (+ residual) (then ReLU when relu != 0).
 *           running_mean / running_var (fp32, either may be NULL) <- (1 - momentum) * old + momentum * new, with the
 *           UNBIASED variance (* n / (n - 1)) as torch; computed in fp64 and rounded once.
 *           Per element |y - exact| <= 4 * 2^-24 * (|gamma xh| + |beta| + |residual|), whatever |mean| / sigma.
 * backward: g = dy, or 0 where relu != 0 and not y > 0;  dbeta = sum g;  dgamma = sum g * xh;
 *           dx = gamma * rstd * (g - dbeta / n - xh * dgamma / n);  dresidual = g.  fp64 up to each fp32 store.
 *           dx, dgamma, dbeta and dresidual may each be NULL: that output is not computed (no dx: no second pass; none of
 *           dx / dgamma / dbeta: no reduction).  y may be NULL when relu == 0. */
int imf_bn_train_chunk_rows(void);
size_t imf_bn_train_workspace_bytes(int64_t n, int c);
int imf_bn_train_forward(const float *x, int64_t n, int c, const float *gamma, const float *beta, double eps,
                         const float *residual /* or NULL */, int relu, float *running_mean /* or NULL */,
                         float *running_var /* or NULL */, double momentum, float *y, double *stats /* [2c] */,
                         void *workspace, size_t workspace_bytes, void *stream);
int imf_bn_train_backward(const float *dy, const float *x, const float *y, int relu, const double *stats,
                          const float *gamma, int64_t n, int c, float *dx, float *dgamma, float *dbeta, float *dresidual,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- InstanceNorm of the sparse path (csrc/norm_train.hip) -------------------------------------------------------------
 * Replaces: ME.MinkowskiInstanceNorm inside the residual blocks of the ResUNetIN2* variants (model/common.py:7-8) and the
 * ReLU / residual add that follow it, forward and backward: the imf_bn_train_* arithmetic with the statistics cut per
 * batch item.  Rows are grouped by item: item b owns rows [item_starts[b], item_starts[b + 1]) of the row-major fp32
 * [n, c] matrices; item_starts is int32 [n_items + 1] ON THE DEVICE and no call reads it on the host (the kernels clamp
 * its values to a non-decreasing sequence inside [0, n], so no content of it makes them leave the matrices; rows before
 * item_starts[0] or from item_starts[n_items] on belong to no item and are not written).  1 <= n_items <= IMF_MAX_BATCH,
 * 1 <= n < 2^31, any c >= 1, 16-byte vectors when c % 4 == 0 and the pointers are 16-byte aligned.
 * Summation order: every item is cut into chunks of imf_bn_train_chunk_rows() rows (the constant of the BatchNorm calls)
 * counted from the item's OWN first row, and one workgroup per item adds that item's chunk partials in chunk order.  The
 * bits of item b's rows of y and dx therefore depend on item b's rows alone: not on the item's place in the batch, the
 * other items, the grid or the CU count.  No floating-point atomics, no workgroup waits for another, two calls give the
 * same bits.  Every call takes a stream and synchronises nothing; bad arguments (n < 1, c < 1, n_items outside
 * 1 .. IMF_MAX_BATCH, a short workspace, a null required pointer) return IMF_EINVAL before any launch.
 * workspace: imf_in_workspace_bytes(n, c, n_items), 8-byte aligned, for either call (0 for arguments a call refuses).
 *
 * forward:  stats[b][0..c) = mean of item b, stats[b][c..2c) = 1 / sqrt(biased variance + eps), both fp64, from fp64 sums
 *           of d = x - p and d^2 about the pivot p = the item's first row (as the BatchNorm call: no cancellation when
 *           |mean| >> sigma);  xh = fp32((double(x) - mean_b) * rstd_b);  y = fmaf(xh, gamma, beta) (+ residual) (then
 *           ReLU when relu != 0).  An item of one row has variance 0: xh = 0 and y = beta (+ residual).  An item without
 *           rows writes no row (its stats are 0, 0).  No running statistics.
 *           Per element  |y - exact| <= 4 * 2^-24 * (|gamma xh| + |beta| + |residual|)
 *                                       + |gamma| * rstd_b * 2^-53 * (n_b * max_b |x - p| + 2 |mean_b|).
 *           The first term is the BatchNorm call's (the three fp32 roundings).  The second is what the fp64 statistics'
 *           own rounding moves xh by -- n_b additions of |d| <= max |x - p| behind sum d, then the addition of n_b p and
 *           the division, each on |mean_b| --: it is multiplied by rstd, which eps = 1e-8 lets reach 1e4 where BatchNorm's
 *           1e-5 stops it at 316 and the first term covered it.  With n_b <= 600, |x| <= 12 and rstd <= 2 it is below
 *           2^-39 |gamma|; a channel that is constant inside an item has d = 0 everywhere, mean = p exactly and xh = 0.
 * backward: g = dy, or 0 where relu != 0 and not y > 0;  per item S1_b = sum_b g, S2_b = sum_b g * xh;
 *           dx = gamma * rstd_b * (g - S1_b / n_b - xh * S2_b / n_b);  dbeta = sum_b S1_b and dgamma = sum_b S2_b, the
 *           items added in item order;  dresidual = g.  fp64 up to each fp32 store.  dx, dgamma, dbeta and dresidual
 *           may each be NULL exactly as in imf_bn_train_backward; y may be NULL when relu == 0. */
size_t imf_in_workspace_bytes(int64_t n, int c, int n_items);
int imf_in_forward(const float *x, int64_t n, int c, const int32_t *item_starts /* device [n_items + 1] */, int n_items,
                   const float *gamma, const float *beta, double eps, const float *residual /* or NULL */, int relu,
                   float *y, double *stats /* [n_items][2c] */, void *workspace, size_t workspace_bytes, void *stream);
int imf_in_backward(const float *dy, const float *x, const float *y, int relu, const double *stats, const float *gamma,
                    const int32_t *item_starts, int64_t n, int c, int n_items, float *dx, float *dgamma, float *dbeta,
                    float *dresidual, void *workspace, size_t workspace_bytes, void *stream);

/* ---- The hardest-contrastive loss of training (csrc/loss.hip) -----------------------------------------------------------
 * Replaces: lib/trainer.py:440-493 `contrastive_hardest_negative_loss` and torch's autograd of it (row gathers whose
 * backward is an atomic index_put, two sort-based isin calls, boolean-mask indexing that waits for the device).
 * f0 [n0, c], f1 [n1, c] row-major fp32, 16-byte aligned; pairs int64 [n_pairs, 2] = (row of f0, row of f1); pos_sel int64
 * [n_pos] rows of `pairs`, or NULL = every pair in order (then n_pos == n_pairs); sel0 [n_sel0] rows of f0, sel1 [n_sel1]
 * rows of f1.  With (i_s, j_s) = pairs[pos_sel[s]], a_s = f0[i_s], b_s = f1[j_s]:
 *   hard01[s] = sel1[argmin_k |a_s - f1[sel1[k]]|^2], hard10[s] = sel0[argmin_k |b_s - f0[sel0[k]]|^2]: imf_nn_search
 *               itself (fp64 scores of the fp32 rows, a tie goes to the lowest k);
 *   keep01[s] = 0 when (i_s, hard01[s]) is one of the n_pairs pairs, else 1; keep10[s] likewise for (hard10[s], j_s); exact,
 *               on the key i + j * max(n0, n1) in an open-addressing set (integer compare-and-swap only);
 *   loss[0]   = mean_s relu(|a_s - b_s|^2 - pos_thresh);
 *   loss[1]   = (mean_{keep01} relu(neg_thresh - D01)^2 + mean_{keep10} relu(neg_thresh - D10)^2) / 2,
 *               D01_s = sqrt(|a_s - f1[hard01_s]|^2 + 1e-7), D10_s = sqrt(|b_s - f0[hard10_s]|^2 + 1e-7);
 *   meta      = (count of keep01, count of keep10, flags, 0); an empty keep set makes loss[1] NaN (the mean of nothing, as
 *               torch), sends no gradient and raises flag bit 0 (keep01) or bit 1 (keep10).
 * Every term is evaluated in fp64 from the fp32 rows, summed in fp64 in an order fixed by s alone, each output rounded
 * once: |loss - exact| <= 2^-23 |exact|.
 * backward: df0 [n0, c], df1 [n1, c] = the closed-form gradient of grad[0] * loss[0] + grad[1] * loss[1]; grad is fp32 [2]
 * ON THE DEVICE.  Row i_s of f0 receives the positive term and the 01 term (as anchor), row hard10[s] the 10 term (as the
 * negative; the minimum routes its gradient to the argmin only); f1 symmetrically.  Each element is one fp64 sum of its
 * addends in an order that depends on the indices and c only, rounded once: |got - exact| <= 2^-23 * sum |addends|.  A row
 * that no term touches is written as +0.0; the call writes all of df0 and df1 (the caller need not zero them).
 * No floating-point atomics: two calls give the same bits.  Every call takes a stream and waits for nothing.
 * IMF_EINVAL before any launch: c not in {16, 32, 64}, n_pos / n_pairs / n_sel0 / n_sel1 / n0 / n1 < 1, pos_sel NULL with
 * n_pos != n_pairs, a null required pointer, a short or misaligned workspace.  IMF_EUNSUPPORTED: n_pos > 65536 (the entries
 * are ranked by counting) or n_pairs > 2^26 (the key set).  Index VALUES are not validated.
 * workspace: imf_hc_loss_workspace_bytes (0 for arguments the calls refuse), 16-byte aligned, for either call; nothing in
 * it is carried from the forward to the backward. */
size_t imf_hc_loss_workspace_bytes(int64_t n0, int64_t n1, int c, int64_t n_pairs, int64_t n_pos, int64_t n_sel0,
                                   int64_t n_sel1);
int imf_hc_loss_forward(const float *f0, int64_t n0, const float *f1, int64_t n1, int c, const int64_t *pairs,
                        int64_t n_pairs, const int64_t *pos_sel /* or NULL */, int64_t n_pos, const int64_t *sel0,
                        int64_t n_sel0, const int64_t *sel1, int64_t n_sel1, double pos_thresh, double neg_thresh,
                        float *loss /* [2] */, int64_t *hard01 /* [n_pos] */, int64_t *hard10, uint8_t *keep01 /* [n_pos] */,
                        uint8_t *keep10, int32_t *meta /* [4] */, void *workspace, size_t workspace_bytes, void *stream);
int imf_hc_loss_backward(const float *f0, int64_t n0, const float *f1, int64_t n1, int c, const int64_t *pairs,
                         int64_t n_pairs, const int64_t *pos_sel /* or NULL */, int64_t n_pos, const int64_t *sel0,
                         int64_t n_sel0, const int64_t *sel1, int64_t n_sel1, double pos_thresh, double neg_thresh,
                         const int64_t *hard01, const int64_t *hard10, const uint8_t *keep01, const uint8_t *keep10,
                         const int32_t *meta, const float *grad /* [2], device */, float *df0, float *df1, void *workspace,
                         size_t workspace_bytes, void *stream);

/* ---- The attention-fusion block in training (csrc/fusion_train.hip) ---------------------------------------------------
 * Replaces: model/attention_fusion.py:132-154 (depth 0, one head, no mask) under autograd, and the host loop over batch
 * items around it (model/resunet.py:237-273).  One configuration: latent 256, context 128, inner 128, GEGLU hidden 1024
 * (passed explicitly; anything else is IMF_EINVAL), 1 <= n_tokens <= 320.
 *   x [n, 256] row-major fp32, the rows of item b are [item_starts[b], item_starts[b + 1]);  item_starts int32
 *   [n_items + 1] ON THE DEVICE, ascending, item_starts[0] = 0, item_starts[n_items] = n, an empty item is legal;
 *   tokens [n_items, n_tokens, 128];  weights: IMF_FT_NPARAM device pointers in the order of the IMF_FT_* indices, each
 *   in its parameter's own row-major [out, in] layout (nothing is packed);  z [n, 256].
 *     c = LNc(tok_b), (k, v) = c Wkv^T;  q = LN1(x) Wq^T;  p = softmax(q k^T * 128^-1/2) over the item's tokens;
 *     y = (p v) Wo^T + bo + x;  h = LN2(y) W1^T + b1 = (a, g);  z = (a * gelu_erf(g)) W2^T + b2 + y.
 * forward: writes z and, into `saved` (imf_fusion_train_saved_bytes), what the backward reads again: the LayerNorm
 *   statistics (mean, rstd per row), LN1(x), q, p, p v, y, LN2(y), h, the GEGLU output, LNc(tok) and (k, v).
 * backward: dz [n, 256] -> dx [n, 256], dtokens [n_items, n_tokens, 128] and grads[IMF_FT_*] in the parameters' layouts.
 *   dx, dtokens and every grads[i] may be NULL: that gradient, and whatever only it needs, is not computed; the bits of
 *   the others do not change.  Every element of every non-NULL output is written (+0.0 in dtokens of an item without rows).
 * fp32 throughout.  Products run on the fp32 MFMA, K ascending; LayerNorm and softmax rows are reduced by fixed xor
 * butterflies; every sum over rows (the 14 parameter gradients, dk / dv per item) is cut into chunks of
 * imf_fusion_train_chunk_rows() rows (counted from the range's first row), chunk partials added in chunk order in fp64
 * and rounded once.  No floating-point atomics: two calls give the same bits, and a row of a batched forward equals that
 * row of its item run alone.  Rows and tokens of padding contribute exactly nothing.
 * meta: one int32 on the device, set to 0 by each call; IMF_FT_FLAG_STARTS is raised when an item's starts are not
 *   0 <= s0 <= s1 <= n or the partition does not begin at 0 / end at n: that item is skipped and nothing outside the
 *   outputs, `saved` and the workspace is ever written.  Neither call copies anything to the host or waits.
 * n == 0 launches nothing and returns IMF_OK (no pointer is looked at, no output written: the gradients of a batch without
 *   rows are the caller's zeros).  IMF_EINVAL before any device call: other dims, n_tokens outside 1 .. 320,
 *   n < 0 or > 2^22, n_items < 1, a null required pointer, a short saved buffer or workspace, a pointer that is not
 *   16-byte aligned.  workspace (backward only): imf_fusion_train_workspace_bytes, 16-byte aligned. */
enum {
  IMF_FT_LN1_G = 0, IMF_FT_LN1_B,      /* cross_attend_blocks.0.norm.{weight,bias}          [256] */
  IMF_FT_LNC_G, IMF_FT_LNC_B,          /* cross_attend_blocks.0.norm_context.{weight,bias}  [128] */
  IMF_FT_WQ,                           /* cross_attend_blocks.0.fn.to_q.weight              [128, 256] */
  IMF_FT_WKV,                          /* cross_attend_blocks.0.fn.to_kv.weight             [256, 128] */
  IMF_FT_WO, IMF_FT_BO,                /* cross_attend_blocks.0.fn.to_out.{weight,bias}     [256, 128], [256] */
  IMF_FT_LN2_G, IMF_FT_LN2_B,          /* cross_attend_blocks.1.norm.{weight,bias}          [256] */
  IMF_FT_W1, IMF_FT_B1,                /* cross_attend_blocks.1.fn.net.0.{weight,bias}      [2048, 256], [2048] */
  IMF_FT_W2, IMF_FT_B2,                /* cross_attend_blocks.1.fn.net.2.{weight,bias}      [256, 1024], [256] */
  IMF_FT_NPARAM
};
#define IMF_FT_FLAG_STARTS 1
int imf_fusion_train_chunk_rows(void);
size_t imf_fusion_train_saved_bytes(int64_t n, int n_items, int n_tokens);
size_t imf_fusion_train_workspace_bytes(int64_t n, int n_items, int n_tokens);
int imf_fusion_train_forward(const float *x, int64_t n, const int32_t *item_starts, int n_items, const float *tokens,
                             int n_tokens, int latent_dim, int context_dim, int inner_dim, int hidden_dim,
                             const float *const *weights /* host array [IMF_FT_NPARAM] */, float *z, float *saved,
                             size_t saved_bytes, int32_t *meta, void *stream);
int imf_fusion_train_backward(const float *dz, const float *x, int64_t n, const int32_t *item_starts, int n_items,
                              const float *tokens, int n_tokens, int latent_dim, int context_dim, int inner_dim,
                              int hidden_dim, const float *const *weights, const float *saved, size_t saved_bytes, float *dx,
                              float *dtokens, float *const *grads /* host array [IMF_FT_NPARAM], entries may be NULL */,
                              int32_t *meta, void *workspace, size_t workspace_bytes, void *stream);

/* ---- The descriptor head in training (csrc/head_train.hip) -------------------------------------------------------------
 * Replaces: model/resunet.py:226-235 under autograd -- ME.cat(out, out_s1), conv1_tr (1x1, no bias), ReLU, final (1x1,
 * bias) and the L2 normalisation -- by one forward and one backward call.  One shape: cu 64, cs 32, ch 64, co 32 (passed
 * explicitly; anything else is IMF_EINVAL), 0 <= n <= 2^22.
 *   u [n, cu], s [n, cs] row-major fp32 (the concatenation is never built; u's channels come first);  w1 [cu + cs, ch],
 *   w2 [ch, co], bias [1, co]: the parameters' own layouts, nothing is packed.
 *     H = relu(u w1[:cu] + s w1[cu:]);  Z = H w2 + bias;  r = sqrt(sum_c Z_c^2);  y = Z / r (normalize) or Z.
 * forward: writes h [n, ch] (saved; doubles as the ReLU mask), y [n, co] and, with normalize, r [n] (else r may be NULL).
 * backward: dy [n, co] -> dZ = (dy - y sum_c(dy y)) / r (normalize; else dZ = dy, y and r may be NULL), then
 *     dbias = sum_rows dZ, dw2 = H^T dZ, dH = (dZ w2^T) [H > 0], dw1 = [u s]^T dH, du = dH w1[:cu]^T, ds = dH w1[cu:]^T.
 *   du, ds, dw1, dw2 and dbias may each be NULL: that gradient, and whatever only it needs, is not computed; the bits of
 *   the others do not change.  Every element of every non-NULL output is written.
 * fp32 throughout.  Products run on the fp32 MFMA, K ascending; the two sums over a row's 32 channels are fixed shuffle
 * trees; the three sums over rows are cut into chunks of imf_head_train_chunk_rows() rows, chunk partials added in chunk
 * order in fp64 and rounded once.  No floating-point atomics: two calls give the same bits, and y, du and ds of a row
 * depend on that row alone.  No epsilon: r == 0 gives what the division gives.
 * meta: one int32 on the device, set to 0 by each call; IMF_HT_FLAG_NORM is raised when a row's r is 0 or not finite
 *   (normalize only).  Neither call copies anything to the host or waits.
 * n == 0: the forward writes nothing; the backward writes +0.0 into every non-NULL dw1, dw2 and dbias; no other pointer is
 *   looked at.  IMF_EINVAL before any device call: other channel counts, n < 0 or > 2^22, a null required pointer, a short
 *   workspace, u / s / w1 / w2 / dy / y / workspace not 16-byte aligned.  workspace (backward only):
 *   imf_head_train_workspace_bytes(n) -- dZ, dH and the chunk partials; 0 for n < 1 or n > 2^22. */
#define IMF_HT_FLAG_NORM 1
int imf_head_train_chunk_rows(void);
size_t imf_head_train_workspace_bytes(int64_t n);
int imf_head_train_forward(const float *u, int cu, const float *s, int cs, int64_t n, const float *w1, int ch,
                           const float *w2, int co, const float *bias, int normalize, float *h, float *r, float *y,
                           int32_t *meta, void *stream);
int imf_head_train_backward(const float *dy, const float *y, const float *r, const float *h, const float *u, int cu,
                            const float *s, int cs, int64_t n, const float *w1, int ch, const float *w2, int co,
                            int normalize, float *du, float *ds, float *dw1, float *dw2, float *dbias, void *workspace,
                            size_t workspace_bytes, int32_t *meta, void *stream);

/* ---- Descriptor Activation Mapping (csrc/dam.hip) ---------------------------------------------------------------------
 * Replaces: pytorch_dam/base_dam.py:120-173 + pytorch_dam/dam.py:15-21 -- 32 backward passes through the whole network per
 * target point, of which only final.kernel.grad is read -- by the closed form of that gradient, for T targets at once.
 *   out_prenorm [n, 32] = the output of `final` before the L2 normalisation (bias included), 16-byte aligned;
 *   hidden [n, c_hid]   = the input of `final`;  targets [T] = row indices, on the device;
 *   r = |o[t]|, f = o[t] / r, a_j = 32 - j (accumulate != 0: the reference's accumulating .grad) or 1 (accumulate == 0);
 *   w_c = mean_k(hidden[t, k]) * (a_c - f_c * sum_j a_j f_j) / r, fp64 sums in a fixed order, rounded once to fp32 and
 *   left in weights [T, 32];  heat[t, i] = max(0, sum_c w_c * o[i, c]) as 32 fp32 FMAs over ascending c, heat [T, n]
 *   (row stride n);  minmax[t] = (min, max) of heat[t, 0:rows), (0, 0) when there are no rows.
 * n_dev (or NULL): device row count, rows = min(n, *n_dev); rows beyond it are neither read nor written.
 * flags[t] = 1 and heat[t, :] = 0 when the target is outside [0, rows), r == 0 or r is not finite; else flags[t] = 0.
 * No atomics: two calls give the same bits.  |heat - exact| <= 40 * 2^-24 * sum_c |w_c o[i, c]|.
 * c_out must be 32 and c_hid a positive multiple of 32: IMF_EUNSUPPORTED otherwise.  T == 0 launches nothing. */
int imf_dam_heat(const float *out_prenorm, int64_t n, const int32_t *n_dev, const float *hidden, int c_hid, int c_out,
                 const int32_t *targets, int T, int accumulate, float *weights /* [T, 32] */, float *heat /* [T, n] */,
                 float *minmax /* [T, 2] */, int32_t *flags /* [T] */, void *stream);

/* ---- The SGD step of training in one launch (csrc/optim.hip) -----------------------------------------------------------
 * Replaces: torch.optim.SGD.step over the model's tensors (lib/trainer.py:62-66, 178) and, for the convolution weights, the
 * re-packing of their operand images on every use.  Per element in fp32, each operation rounded once (no contraction):
 *   d = g + wd p (wd == 0: d = g);  b' = mu b + d (first_step: b' = d; momentum NULL: no buffer, b' = d);  p' = p - lr b'
 * = torch.optim.SGD with dampening 0, no Nesterov, not maximising.
 * One record per tensor, in device memory.  param / grad / momentum: numel contiguous floats each.  layout:
 *   IMF_SGD_PLAIN  any tensor, updated element-wise; the remaining fields are ignored;
 *   IMF_SGD_ME     a convolution kernel [kvol, cin, cout] (2-D [cin, cout] when kvol == 1);
 *   IMF_SGD_TORCH  a convolution weight [cout, cin, kh, kw], kvol = kh kw, tap k = kh_index kw + kw_index;
 * the last two need cin % 32 == 0, cout % 32 == 0, 1 <= kvol <= 27, numel == kvol cin cout (the caller's to guarantee:
 * the records live on the device) and also write, from the updated values, the bf16x3 images imf_pack_weights_bf16x3
 * would build (imf_packed_weight_floats_bf16x3 floats each, 16-byte aligned; either may be NULL):
 *   image_fwd  of W[k][ci][co];
 *   image_bwd  of W'[k'][co][ci] = W[k][ci][co] with k' = kvol - 1 - k when flip != 0, else k' = k -- the operand of the
 *              input gradient (the transposed kernel, its taps flipped for a stride-1 convolution). */
#define IMF_SGD_PLAIN 0
#define IMF_SGD_ME    1
#define IMF_SGD_TORCH 2
#define IMF_SGD_CHUNK 2048          /* elements of one tensor that one workgroup serves */
#define IMF_SGD_RECORD_FIELDS 12
typedef struct imf_sgd_record {
  float *param;
  const float *grad;
  float *momentum;
  float *image_fwd, *image_bwd;
  int64_t numel;
  int32_t first_step;
  int32_t layout;
  int32_t kvol, cin, cout;
  int32_t flip;
} imf_sgd_record;
int imf_sgd_chunk(void);            /* IMF_SGD_CHUNK */
/* Layout of imf_sgd_record as the library was compiled, for mirrors of the struct in other languages: field = 0 ..
 * IMF_SGD_RECORD_FIELDS - 1 in declaration order gives that member's offset and size, field < 0 gives (0, sizeof). [host] */
int imf_sgd_record_layout(int field, size_t *offset, size_t *size);
/* One launch on `stream`, no host wait, no atomics.  block_map [n_blocks][2] int32 on the device: workgroup i serves
 * elements [chunk IMF_SGD_CHUNK, (chunk + 1) IMF_SGD_CHUNK) of record block_map[i][0], chunk = block_map[i][1] (for a
 * packable record: in the order of the forward image); every chunk of every record to be stepped exactly once, records
 * left out are not touched.  n_blocks == 0 launches nothing. */
int imf_sgd_step(const imf_sgd_record *records, int n_records, const int32_t *block_map, int n_blocks, float lr,
                 float momentum, float weight_decay, void *stream);

/* ---- Host-side codecs of the batch path: HOST pointers, no GPU involved ----------------------
 * Replace what the reference does around every fragment with Open3D / matplotlib / OpenCV / numpy
 * (scripts/generate_desc.py:83-97,118-123, util/uio.py:33-40).  All return 0 / a count on success, a negative
 * IMF_E* code otherwise (imf_last_error). */
int64_t imf_ply_vertex_count(const char *path);
/* x,y,z of every vertex as float64 [n,3] = np.array(o3d.io.read_point_cloud(path).points): ascii and both binary
 * byte orders, other scalar vertex properties skipped.  Returns n. */
int64_t imf_ply_read_points(const char *path, double *out /* [capacity,3] */, int64_t capacity);
int imf_png_info(const char *path, int *h, int *w, int *channels);
/* matplotlib.image.imread of a .png: float32 [H,W,C] in [0,1] (8-bit / 255, 16-bit / 65535, palette -> RGB).
 * IMF_EUNSUPPORTED for interlaced or sub-byte files (callers fall back to a generic decoder). */
int imf_png_read_f32(const char *path, float *out, int64_t capacity_floats, int *h, int *w, int *channels);
/* o3d.io.read_image of a depth map (data/fuse_fragments_3DMatch.py:41): 16-bit greyscale PNG, big-endian samples ->
 * host-order uint16 [H,W].  IMF_EUNSUPPORTED for every other kind of PNG. */
int imf_png_read_u16(const char *path, uint16_t *out, int64_t capacity_samples, int *h, int *w);
/* A fragment's points as a binary little-endian PLY with `float x, y, z` per vertex (fp64 [n,3] in, narrowed to
 * float32: the 3DMatch fragments' layout, which imf_ply_read_points reads).  Written through a temporary file and a
 * rename. */
int imf_ply_write_points(const char *path, const double *xyz, int64_t n);
/* Coloured points as Open3D writes them (o3d.io.write_point_cloud of a cloud with colours, pytorch_dam/utils/image.py:162):
 * binary little-endian, `double x, y, z` + `uchar red, green, blue` per vertex, the header of files/3D_head_map.ply.
 * Written through a temporary file and a rename. */
int imf_ply_write_points_rgb(const char *path, const double *xyz, const uint8_t *rgb, int64_t n);

/* matplotlib.image.imread of a .jpg (scripts/generate_desc.py:88-92: PIL = libjpeg's defaults, integer "islow" inverse DCT
 * and fancy chroma upsampling): uint8 [H, W, 3].  Baseline / extended sequential Huffman files with three YCbCr components in
 * one scan, 4:4:4 / 4:2:2 / 4:2:0, restart intervals: bit-identical to PIL (tests/test_cabi_and_host.py).  IMF_EUNSUPPORTED
 * for everything else a JPEG file may hold (progressive, arithmetic, 12-bit, grey, CMYK, other sampling factors): callers
 * fall back to a generic decoder.  [host] */
int imf_jpeg_info(const char *path, int *h, int *w, int *channels);
int imf_jpeg_read_u8(const char *path, uint8_t *out, int64_t capacity_bytes, int *h, int *w, int *channels);
/* cv2.resize(INTER_LINEAR) for float images [H,W,C]; chw != 0 writes [C,H_out,W_out] (generate_desc.py:96-97). */
int imf_resize_bilinear_f32(const float *in, int H, int W, int C, float *out, int H_out, int W_out, int chw);
/* np.savez (level 0) / np.savez_compressed (level 1..9, raw deflate) of n_arrays C-ordered arrays: names[i] (member
 * name), dtype[i] (numpy descr, e.g. "<f8"), ndim[i], their dims concatenated in shape, data[i].  np.load reads the
 * file; the arrays are identical to numpy's own writers'.  Levels 2..9 are zlib's; level 1 uses the library's own raw-deflate
 * producers where the member allows (8-byte items: matches at value granularity -- the float32-valued float64 coordinates of
 * `points` / `xyz` repeat earlier values exactly 98-99 % of the time --; members without LZ77 matches: byte-wise Huffman),
 * zlib level 1 otherwise: scripts/generate_desc.py:118-123 at ~10x numpy's rate per core. */
int imf_npz_write(const char *path, int n_arrays, const char *const *names, const char *const *dtype,
                  const int32_t *ndim, const int64_t *shape, const void *const *data, int level);
/* The same with block-parallel deflate on `threads` host threads (256 KiB blocks as independent raw-deflate segments that
 * end on a byte boundary, concatenated; CRC-32s combined): the file's bytes are a function of the arrays and the level only,
 * never of `threads`.  threads <= 1 is imf_npz_write.  scripts/generate_desc.py:118-123 at the rate of eight GPUs. */
int imf_npz_write_mt(const char *path, int n_arrays, const char *const *names, const char *const *dtype,
                     const int32_t *ndim, const int64_t *shape, const void *const *data, int level, int threads);

/* Measurement helpers (bench.py): HIP events on the caller's stream. */
void *imf_stream_create(void);     /* non-blocking hipStream_t, distinct from any framework pool stream */
void imf_stream_destroy(void *stream);
void *imf_event_create(void);
void imf_event_destroy(void *ev);
int imf_event_record(void *ev, void *stream);                 /* hipEventRecord */
float imf_event_elapsed_ms(void *ev_begin, void *ev_end);   /* < 0 on error (e.g. not completed) */

#ifdef __cplusplus
}
#endif
#endif /* IMFNET_HIP_H */
