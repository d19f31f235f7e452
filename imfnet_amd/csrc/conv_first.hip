// conv1, the first convolution of the network (Cin <= 4, in practice the all-ones occupancy feature), on gfx950:
//   k_spconv_small_cin     table-driven, one thread per output row (any small Cin)
//   k_conv_first_fused     fused with its kernel map: probes the level-0 hash, no neighbour table in HBM
//   k_conv_first_bits      all-ones input: occupancy windows of a dense bit grid x exact three-part f16 weights on the matrix pipe
//   k_conv_first_and_map   the same, with the level-0 3x3x3 neighbour map built by the odd workgroups of the launch
// Every bit-grid route -- the three public imf_conv_first_bitgrid* entry points and the executor's -- goes through
// conv_first_bitgrid(ConvFirstArgs) below.
#include <string.h>

#include "spconv_shared.h"
#include "geometry_internal.h"
#include "rulebook_tile.h"

namespace imf {

// ---- first layer: tiny Cin (all-ones occupancy feature), one thread per output row -------------
template <int COUT>
__global__ void __launch_bounds__(256)
k_spconv_small_cin(const float *__restrict__ in, int cin, const float *__restrict__ w, int kvol,
                   const int32_t *__restrict__ nbr, long long n_slots, long long n_out,
                   const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                   float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  const int nw = kvol * cin * COUT;
  for (int i = threadIdx.x; i < nw; i += blockDim.x) wl[i] = w[i];
  __syncthreads();
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float acc[COUT];
#pragma unroll
  for (int c = 0; c < COUT; ++c) acc[c] = 0.f;
  for (int k = 0; k < kvol; ++k) {
    const int i = (row < n_out) ? nbr[(long long)k * n_slots + row] : -1;
    if (i >= 0) {
      for (int ci = 0; ci < cin; ++ci) {
        const float x = in[(long long)i * cin + ci];
        const float4 *wk = reinterpret_cast<const float4 *>(wl + (k * cin + ci) * COUT);
#pragma unroll
        for (int c4 = 0; c4 < COUT / 4; ++c4) {
          const float4 ww = wk[c4];
          acc[4 * c4 + 0] = fmaf(x, ww.x, acc[4 * c4 + 0]);
          acc[4 * c4 + 1] = fmaf(x, ww.y, acc[4 * c4 + 1]);
          acc[4 * c4 + 2] = fmaf(x, ww.z, acc[4 * c4 + 2]);
          acc[4 * c4 + 3] = fmaf(x, ww.w, acc[4 * c4 + 3]);
        }
      }
    }
  }
  if (row >= n_out) return;
  float4 *o = reinterpret_cast<float4 *>(out + row * COUT);
#pragma unroll
  for (int c4 = 0; c4 < COUT / 4; ++c4) {
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * c4 + e;
      float x = acc[c] * (scale ? scale[c] : 1.f) + (shift ? shift[c] : 0.f);
      y[e] = relu ? fmaxf(x, 0.f) : x;
    }
    o[c4] = make_float4(y[0], y[1], y[2], y[3]);
  }
}


// ---- first layer, fused with its kernel map: no neighbour table is ever written to HBM ----------
// One workgroup = 32 output voxels.  Phase 1: the 256 threads probe the 32 x kvol kernel offsets in
// the input level's hash (16 independent probes per thread) into an LDS neighbour tile.  Phase 2:
// thread = (output channel, row group) walks the offsets in ascending k -- the same sum order as the
// table-driven kernel and the oracle -- with the weights in LDS.  in == nullptr: all-ones input.
constexpr int kFirstRows = 32;

template <int COUT>
__global__ void __launch_bounds__(256)
k_conv_first_fused(const imf_slot *__restrict__ tab, uint32_t capmask,
                   const int32_t *__restrict__ coords, long long n, int ts, int ksize, int kvol,
                   const float *__restrict__ in, int cin, const float *__restrict__ w,
                   const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                   float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float wl[];      // [kvol*cin*COUT] weights, then nbr tile
  const int nw = kvol * cin * COUT;
  int *nbr_l = reinterpret_cast<int *>(wl + nw);                   // [kFirstRows][128]
  const int tid = threadIdx.x;
  for (int i = tid; i < nw; i += 256) wl[i] = w[i];
  const long long row0 = (long long)blockIdx.x * kFirstRows;
  const int r = ksize >> 1;
  // 16 probes per thread, issued as one independent batch of 16-byte slot loads (key + row together);
  // only a collision (rare: the level-0 table is <= 25 % full) falls back to the probe loop.
  constexpr int NP = kFirstRows * 128 / 256;
  uint64_t want[NP];
  uint4 got[NP];
  uint32_t hs[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int idx = j * 256 + tid, lr = idx >> 7, k = idx & 127;
    const long long row = row0 + lr;
    want[j] = kEmptyKey;                               // "no probe": resolves to -1 below
    hs[j] = 0;
    if (k < kvol && row < n) {
      const int4 c = reinterpret_cast<const int4 *>(coords)[row];
      const int dx = k % ksize - r, dy = (k / ksize) % ksize - r, dz = k / (ksize * ksize) - r;
      const int x = c.y + dx * ts, y = c.z + dy * ts, z = c.w + dz * ts;
      if (coord_in_range(x, y, z)) {
        want[j] = pack_key(c.x, x, y, z);
        hs[j] = hash_slot(want[j], __builtin_ctz((unsigned)ts), capmask);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NP; ++j) got[j] = *reinterpret_cast<const uint4 *>(tab + hs[j]);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    int found = -1;
    if (want[j] != kEmptyKey) {
      const uint64_t k0 = ((uint64_t)got[j].y << 32) | got[j].x;
      if (k0 == want[j]) found = (int)got[j].z;
      else if (k0 != kEmptyKey) found = hash_find(tab, capmask, want[j], __builtin_ctz((unsigned)ts));   // collision: slow path
    }
    nbr_l[j * 256 + tid] = found;
  }
  __syncthreads();
  constexpr int RPT = kFirstRows * COUT / 256;                     // rows per thread: 4 (cout 32) / 8 (64)
  constexpr int RG = 256 / COUT;                                   // row groups
  const int co = tid % COUT, rg = tid / COUT;
  float acc[RPT];
#pragma unroll
  for (int q = 0; q < RPT; ++q) acc[q] = 0.f;
  for (int k = 0; k < kvol; ++k) {
    int idx[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) idx[q] = nbr_l[(rg + q * RG) * 128 + k];
    for (int ci = 0; ci < cin; ++ci) {
      const float wv = wl[(k * cin + ci) * COUT + co];
#pragma unroll
      for (int q = 0; q < RPT; ++q) {
        if (in) {
          if (idx[q] >= 0) acc[q] = fmaf(in[(long long)idx[q] * cin + ci], wv, acc[q]);
        } else {
          acc[q] += idx[q] >= 0 ? wv : 0.f;                        // x == 1: exact, branch-free
        }
      }
    }
  }
  const float sc = scale ? scale[co] : 1.f, sh = shift ? shift[co] : 0.f;
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const long long row = row0 + rg + q * RG;
    if (row < n) {
      float v = acc[q] * sc + sh;
      if (relu) v = fmaxf(v, 0.f);
      out[row * COUT + co] = v;
    }
  }
}


// ---- first layer on an occupancy bit grid (all-ones input feature) -----------------------------
// util/misc.py:76-79 feeds the network a column of ones, so conv1 is "sum of the weight rows of the
// occupied offsets".  Occupancy of a 5x5x5 neighbourhood is 25 five-bit windows of a dense bit grid
// over the fragment's bounding box (0.7 MB for a 3DMatch fragment, L2-resident) instead of 125
// dependent probes into a multi-MB hash table.  Per workgroup (64 voxels): the windows are expanded
// into 128-bit masks and out = A . W runs on the f16 matrix pipe (the 0 / 1 operand is exact in f16, the weights
// are split into three f16 parts) with the folded BatchNorm epilogue.
// GridDesc, grid_desc_from_bbox, DynGrid, dyn_grid, grid_row: geometry_internal.h (the level-0 compaction kernel fills the grid too)
__global__ void __launch_bounds__(256)
k_bitgrid_fill(const int32_t *__restrict__ coords, long long n, uint32_t *grid, GridDesc g, int ksize,
               const DynGrid dg) {
  if (!dyn_grid(dg, ksize, g, n)) return;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int4 c = reinterpret_cast<const int4 *>(coords)[i];
  const int bit = c.y - g.x0;
  atomicOr(grid + grid_row(g, c.x, c.z, c.w) + (bit >> 5), 1u << (bit & 31));
}

constexpr int kBitsRows = 64;

typedef unsigned int u32x2_b __attribute__((ext_vector_type(2)));

// conv1's weights as f16 B fragments: max |w| (block reduce over 256 threads) -> power-of-two scale -> THREE f16 parts per weight,
// w = p0 + p1 + p2 exactly (3 x 11 significant bits >= fp32's 24; round 3 kept two parts = 22 bits).  conv1's left operand is
// the 0 / 1 occupancy, exact in f16, and the matrix pipe accumulates in fp32: with exact weights conv1 IS fp32 arithmetic --
// in every mode, for 8 more MFMAs per wavefront.  Writes [nkc][CBN][part][64 lanes] float4 (8 halves each) to `W_l` (LDS or
// global) and returns the factor that undoes the scale.
constexpr int kFirstParts = 3;
template <int COUT>
__device__ __forceinline__ float first_kernel_split(const float *__restrict__ w, int kvol, int nkc, float4 *W_l, unsigned *red,
                                                    int tid) {
  constexpr int CBN = COUT / 16;
  const int wave = tid >> 6, lane = tid & 63;
  unsigned amax = 0u;
  for (int i = tid; i < kvol * COUT; i += 256) {
    const unsigned bits = __float_as_uint(fabsf(w[i]));
    if (bits < 0x7F800000u) amax = bits > amax ? bits : amax;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = __shfl_xor(amax, o, 64);
    amax = t > amax ? t : amax;
  }
  if (lane == 0) red[wave] = amax;
  __syncthreads();
  amax = max(max(red[0], red[1]), max(red[2], red[3]));
  int wshift = 0;
  if (amax != 0u) {
    wshift = 13 - ((int)(amax >> 23) - 127);             // the scaled kernel peaks in [2^13, 2^14): lo halves stay normal
    wshift = wshift < -40 ? -40 : (wshift > 100 ? 100 : wshift);
  }
  for (int i = tid; i < nkc * CBN * 64; i += 256) {
    const int ln = i & 63, cb = (i >> 6) % CBN, kc = i / (64 * CBN);
    f16x8 p0, p1, p2;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int k = 32 * kc + 16 * (t >> 2) + 4 * (ln >> 4) + (t & 3);
      const float x = k < kvol ? ldexpf(w[k * COUT + 16 * cb + (ln & 15)], wshift) : 0.f;
      const _Float16 h0 = (_Float16)x;
      const float r1 = x - (float)h0;                  // exact
      const _Float16 h1 = (_Float16)r1;
      p0[t] = h0;
      p1[t] = h1;
      p2[t] = (_Float16)(r1 - (float)h1);              // exact while normal (>= 2^-24 after the scale: |w| >= 2^-17 max |w|)
    }
    W_l[((kc * CBN + cb) * kFirstParts + 0) * 64 + ln] = __builtin_bit_cast(float4, p0);
    W_l[((kc * CBN + cb) * kFirstParts + 1) * 64 + ln] = __builtin_bit_cast(float4, p1);
    W_l[((kc * CBN + cb) * kFirstParts + 2) * 64 + ln] = __builtin_bit_cast(float4, p2);
  }
  return ldexpf(1.f, -wshift);
}

template <int COUT>
__global__ void __launch_bounds__(256) k_pack_first_kernel(const float *__restrict__ w, int kvol, float *__restrict__ image) {
  __shared__ unsigned red[4];
  const int nkc = (kvol + 31) >> 5;
  const float un = first_kernel_split<COUT>(w, kvol, nkc, reinterpret_cast<float4 *>(image), red, threadIdx.x);
  if (threadIdx.x == 0) image[(size_t)nkc * (COUT / 16) * kFirstParts * 64 * 4] = un;
}

// conv1 for the all-ones occupancy feature: out[v] = sum_k occ(v + off_k) * W[k], a [64, kvol] x [kvol, COUT] product per
// workgroup whose left operand is BINARY.  The occupancy window of a voxel is kept as a 128-bit mask (one thread per
// (voxel, 32-offset word): no LDS atomics, no 33 KiB float matrix, no bank conflicts) and expanded to f16 0 / 1 A fragments
// in registers; 0 and 1 are exact in f16, so only the WEIGHTS are split (three f16 parts, pre-scaled by a power of two:
// first_kernel_split): kFirstParts x v_mfma_f32_16x16x32_f16 per 32 offsets and column block instead of
// 8 x v_mfma_f32_16x16x4_f32.  The parts come from the image imf_pack_first_kernel wrote once per model (DynGrid::w_image)
// or, without one, from a split that every workgroup redoes (4 000 values from L2).
template <int COUT, int KS>
__device__ __forceinline__ void conv_first_bits_body(const int32_t *__restrict__ coords, long long n,
                                                     const uint32_t *__restrict__ grid, GridDesc g, int ksize_rt, int kvol,
                                                     const float *__restrict__ w, const float *__restrict__ scale,
                                                     const float *__restrict__ shift, int relu, float *__restrict__ out,
                                                     const DynGrid dg, int out_split, const long long blk) {
  constexpr int CBN = COUT / 16;                         // column blocks; wave w owns row block w
  constexpr int ksize = KS;
  constexpr int kMaxWin = KS == 3 ? 11 : 8;              // windows of KS bits that can touch one 32-offset word
  extern __shared__ __attribute__((aligned(16))) float lds_f[];
  (void)ksize_rt;
  if (!dyn_grid(dg, ksize, g, n)) return;
  if (blk * kBitsRows >= n) return;
  float4 *W_l = reinterpret_cast<float4 *>(lds_f);                          // [4 kc][CBN][3 parts][64 lanes] x 8 halves
  uint32_t *M_l = reinterpret_cast<uint32_t *>(W_l + 4 * CBN * kFirstParts * 64);     // [64 rows][4 words]: occupancy masks
  __shared__ unsigned red[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long v0 = blk * kBitsRows;
  const int nkc = (kvol + 31) >> 5;

  // ---- occupancy masks: thread (v, wd) gathers the windows (dy, dz) whose ksize bits fall into offsets 32 wd .. 32 wd + 31
  const int v = tid >> 2, wd = tid & 3;
  const int r = ksize >> 1;
  const long long row = v0 + v < n ? v0 + v : n - 1;     // clamped: the loads are unconditional
  const int4 c = reinterpret_cast<const int4 *>(coords)[row];
  const int k_lo = 32 * wd, k_hi = min(32 * wd + 31, kvol - 1);
  const int yz_lo = k_lo / ksize;
  const int n_win = k_hi >= k_lo ? k_hi / ksize - yz_lo + 1 : 0;          // <= kMaxWin
  const int bx = c.y - r - g.x0;                         // first bit of every window of this voxel, >= 0 by construction
  const int wi = bx >> 5, sh = bx & 31;
  const __amdgpu_buffer_rsrc_t rs_grid = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(grid), (short)0, 0x7FFFFFFF, 0x00020000);
  uint32_t w0[kMaxWin], w1[kMaxWin];
#pragma unroll
  for (int j = 0; j < kMaxWin; ++j) {
    const int yz = j < n_win ? yz_lo + j : (n_win ? yz_lo : 0);   // unused slots repeat a valid window (the load is unconditional)
    const int dy = yz % ksize - r, dz = yz / ksize - r;
    // both words of the window in ONE 8-byte buffer load (dword-aligned is enough for buffer addressing): a row has
    // nx / 32 + 2 words and a window starts at most ksize bits before its last occupied bit, so word wi + 1 is in the row
    const long long off = (grid_row(g, c.x, c.z + dy, c.w + dz) + wi) * 4;
    const u32x2_b pr = __builtin_amdgcn_raw_buffer_load_b64(rs_grid, (int)off, 0, 0);
    w0[j] = pr[0];
    w1[j] = pr[1];
  }
  // ---- weights: the three-part f16 B fragments in the MFMA's lane order, [kc][cb][part][lane][t]: offset k = 32 kc + 16 (t >> 2) +
  //      4 (lane >> 4) + (t & 3), column 16 cb + (lane & 15).  From the image imf_pack_first_kernel wrote once per model
  //      (16 KiB verbatim: round 4 -- every one of the ~1 600 workgroups of a launch used to redo the 4 096 splits, 1.5 k of its
  //      1.7 k VALU instructions per wavefront), or, without one, split here: max |w| -> power-of-two scale -> three parts.
  float un;
  if (dg.w_image) {
    const float4 *img = reinterpret_cast<const float4 *>(dg.w_image);
    for (int i = tid; i < nkc * CBN * kFirstParts * 64; i += 256) W_l[i] = img[i];
    un = dg.w_image[(size_t)nkc * CBN * kFirstParts * 64 * 4];
  } else {
    un = first_kernel_split<COUT>(w, kvol, nkc, W_l, red, tid);
  }
  // ---- combine the windows into this thread's mask word
  {
    const uint32_t wmask = (1u << ksize) - 1u;
    uint32_t m = 0u;
#pragma unroll
    for (int j = 0; j < kMaxWin; ++j) {
      if (j >= n_win) continue;
      uint32_t bits = w0[j] >> sh;
      if (sh + ksize > 32) bits |= w1[j] << (32 - sh);
      bits &= wmask;
      const int rel = (yz_lo + j) * ksize - k_lo;        // where the window's offset 0 sits in this word (may be < 0)
      m |= rel >= 0 ? bits << rel : bits >> (-rel);
    }
    if (k_hi - k_lo < 31) m &= (1u << (k_hi - k_lo + 1)) - 1u;            // offsets >= kvol do not exist
    M_l[v * 4 + wd] = v0 + v < n ? m : 0u;
  }
  __syncthreads();

  const int r16 = lane & 15, q4 = lane >> 4;
  f32x4 acc[CBN];
#pragma unroll
  for (int cb = 0; cb < CBN; ++cb) acc[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < nkc; ++kc) {
    // A fragment of lane (r16, q4): offsets 32 kc + {4 q4 .. 4 q4 + 3, 16 + 4 q4 .. 16 + 4 q4 + 3} of row 16 wave + r16
    const uint32_t word = M_l[(wave * 16 + r16) * 4 + kc];
    const uint32_t b8 = ((word >> (4 * q4)) & 0xFu) | (((word >> (16 + 4 * q4)) & 0xFu) << 4);
    uint32_t aw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      aw[j] = ((b8 >> (2 * j)) & 1u ? 0x3C00u : 0u) | ((b8 >> (2 * j + 1)) & 1u ? 0x3C000000u : 0u);   // f16 1.0 = 0x3C00
    const f16x8 a = __builtin_bit_cast(f16x8, make_uint4(aw[0], aw[1], aw[2], aw[3]));
#pragma unroll
    for (int cb = 0; cb < CBN; ++cb) {
      const f16x8 b0 = __builtin_bit_cast(f16x8, W_l[((kc * CBN + cb) * kFirstParts + 0) * 64 + lane]);
      const f16x8 b1 = __builtin_bit_cast(f16x8, W_l[((kc * CBN + cb) * kFirstParts + 1) * 64 + lane]);
      const f16x8 b2 = __builtin_bit_cast(f16x8, W_l[((kc * CBN + cb) * kFirstParts + 2) * 64 + lane]);
      acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b2, acc[cb], 0, 0, 0);      // smallest parts first
      acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b1, acc[cb], 0, 0, 0);
      acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b0, acc[cb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int cb = 0; cb < CBN; ++cb) {
    const int col = cb * 16 + r16;
    const float sc = scale ? scale[col] : 1.f, shf = shift ? shift[col] : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long orow = v0 + wave * 16 + q4 * 4 + e;
      if (orow < n) {
        float y = (acc[cb][e] * un) * sc + shf;
        if (relu) y = fmaxf(y, 0.f);
        if (dg.err && out_of_f16_range(y)) atomicOr(dg.err, 32);
        if (out_split) store_split(out, orow, COUT, col, y);   // operand image for block1 (ConvParams::a_split)
        else out[orow * COUT + col] = y;
      }
    }
  }
}

template <int COUT, int KS>
__global__ void __launch_bounds__(256)
k_conv_first_bits(const int32_t *__restrict__ coords, long long n, const uint32_t *__restrict__ grid,
                  GridDesc g, int ksize_rt, int kvol, const float *__restrict__ w,
                  const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                  float *__restrict__ out, const DynGrid dg, int out_split) {
  conv_first_bits_body<COUT, KS>(coords, n, grid, g, ksize_rt, kvol, w, scale, shift, relu, out, dg, out_split, blockIdx.x);
}

// conv1 AND the level-0 3x3x3 neighbour map in one launch (imf_fragment_forward): both need only the level-0 rows (and
// grid / table), block1 needs both, and as two launches one of them has to cross streams -- the hand-over (event record,
// stream wait) costs ~15 us on the critical path.  Even workgroups run conv1's 64-row blocks, odd ones the map's tiles.
struct MapArgs {
  const imf_slot *tab;
  uint32_t capmask;
  const int32_t *n_out_dev;
  int32_t *tile_rows, *nbr;
  uint32_t *tile_mask;
  long long n_slots;
};
template <int COUT, int KS>
__global__ void __launch_bounds__(256)
k_conv_first_and_map(const int32_t *__restrict__ coords, long long n, const uint32_t *__restrict__ grid,
                     GridDesc g, int kvol, const float *__restrict__ w, const float *__restrict__ scale,
                     const float *__restrict__ shift, int relu, float *__restrict__ out, const DynGrid dg, int out_split,
                     const MapArgs m) {
  const long long idx = blockIdx.x >> 1;
  if (blockIdx.x & 1) {
    if (idx < m.n_slots / IMF_TILE_ROWS)
      rulebook_tile<+1, false>(m.tab, m.capmask, coords, n, m.n_out_dev, 1, 3, 27, m.tile_rows, m.nbr, m.tile_mask, m.n_slots, idx);
  } else {
    conv_first_bits_body<COUT, KS>(coords, n, grid, g, KS, kvol, w, scale, shift, relu, out, dg, out_split, idx);
  }
}

}  // namespace imf

using namespace imf;

extern "C" {

int imf_spconv_small_cin(const float *in, int cin, const float *w, int kvol, int cout,
                         const int32_t *nbr, int64_t n_slots, int64_t n_out, const float *scale,
                         const float *shift, int relu, float *out, void *stream) {
  IMF_REQUIRE(in && w && nbr && out, "imf_spconv_small_cin: null pointer");
  IMF_REQUIRE(cin >= 1 && cin <= 4, "imf_spconv_small_cin: cin=%d not in [1,4]", cin);
  IMF_REQUIRE(cout == 32 || cout == 64, "imf_spconv_small_cin: cout=%d not in {32,64}", cout);
  IMF_REQUIRE(kvol >= 1 && kvol <= IMF_MAX_KVOL, "imf_spconv_small_cin: kvol=%d", kvol);
  const size_t lds = (size_t)kvol * cin * cout * sizeof(float);
  IMF_REQUIRE(lds <= 64 * 1024, "imf_spconv_small_cin: kernel does not fit 64 KiB of LDS");
  IMF_REQUIRE(n_out > 0 && n_slots >= n_out, "imf_spconv_small_cin: n_out / n_slots");
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)div_up(n_out, 256);
  if (cout == 32)
    k_spconv_small_cin<32><<<nb, 256, lds, st>>>(in, cin, w, kvol, nbr, n_slots, n_out, scale, shift, relu, out);
  else
    k_spconv_small_cin<64><<<nb, 256, lds, st>>>(in, cin, w, kvol, nbr, n_slots, n_out, scale, shift, relu, out);
  IMF_CHECK_LAUNCH("k_spconv_small_cin");
  return IMF_OK;
}

int imf_conv_first_fused(const imf_slot *table, int64_t capacity,
                         const int32_t *coords, int64_t n, int ts, int ksize, const float *in, int cin,
                         const float *w, int cout, const float *scale, const float *shift, int relu,
                         float *out, void *stream) {
  IMF_REQUIRE(table && coords && w && out, "imf_conv_first_fused: null pointer");
  IMF_REQUIRE(ksize == 3 || ksize == 5, "imf_conv_first_fused: ksize must be 3 or 5");
  IMF_REQUIRE(cin >= 1 && cin <= 4, "imf_conv_first_fused: cin=%d not in [1,4]", cin);
  IMF_REQUIRE(cout == 32 || cout == 64, "imf_conv_first_fused: cout=%d not in {32,64}", cout);
  IMF_REQUIRE(n > 0 && ts >= 1, "imf_conv_first_fused: bad n / ts");
  IMF_REQUIRE((capacity & (capacity - 1)) == 0, "imf_conv_first_fused: capacity not a power of 2");
  const int kvol = ksize * ksize * ksize;
  const size_t lds = (size_t)kvol * cin * cout * sizeof(float) + (size_t)kFirstRows * 128 * sizeof(int);
  IMF_REQUIRE(lds <= 64 * 1024, "imf_conv_first_fused: kernel does not fit 64 KiB of LDS");
  hipStream_t st = (hipStream_t)stream;
  const long long nb = div_up(n, kFirstRows);
  if (cout == 32)
    k_conv_first_fused<32><<<(unsigned)nb, 256, lds, st>>>(table, (uint32_t)(capacity - 1), coords, n, ts,
                                                          ksize, kvol, in, cin, w, scale, shift, relu, out);
  else
    k_conv_first_fused<64><<<(unsigned)nb, 256, lds, st>>>(table, (uint32_t)(capacity - 1), coords, n, ts,
                                                          ksize, kvol, in, cin, w, scale, shift, relu, out);
  IMF_CHECK_LAUNCH("k_conv_first_fused");
  return IMF_OK;
}

size_t imf_bitgrid_words(const int32_t *bbox, int ksize) {
  GridDesc g;
  size_t words = 0;
  if (!bbox || (ksize != 3 && ksize != 5)) return 0;
  return grid_desc_from_bbox(bbox, ksize, g, words) ? words : 0;
}


}  // extern "C"

namespace imf {
// The one launch path of the bit-grid kernels (ConvFirstArgs: spconv_shared.h).
int conv_first_bitgrid(const ConvFirstArgs &a, hipStream_t st) {
  const bool dyn = a.bbox_dev != nullptr;
  const int n_map = !!a.table + !!a.tile_rows + !!a.nbr + !!a.tile_mask;
  IMF_REQUIRE(a.coords && a.grid && a.w && a.out && (dyn ? a.n_dev && a.err && a.grid_words > 0 : a.bbox && !a.n_dev),
              "imf_conv_first_bitgrid: null pointer");
  IMF_REQUIRE(a.ksize == 3 || a.ksize == 5, "imf_conv_first_bitgrid: ksize must be 3 or 5");
  IMF_REQUIRE(a.cout == 32 || a.cout == 64, "imf_conv_first_bitgrid: cout=%d not in {32,64}", a.cout);
  IMF_REQUIRE(a.n > 0, "imf_conv_first_bitgrid: n");
  IMF_REQUIRE(n_map == 0 || (n_map == 4 && dyn && a.grid_filled),
              "imf_conv_first_bitgrid: the level-0 map needs all its outputs, capacity mode and a filled grid");
  IMF_REQUIRE(n_map == 0 || (a.capacity & (a.capacity - 1)) == 0, "imf_conv_first_bitgrid: capacity not a power of 2");
  GridDesc g;
  memset(&g, 0, sizeof(g));
  size_t words = a.grid_words;
  IMF_REQUIRE(dyn || (grid_desc_from_bbox(a.bbox, a.ksize, g, words) && words <= a.grid_words),
              "imf_conv_first_bitgrid: bounding box too large for the provided grid");
  const DynGrid dg{a.n_dev, a.bbox_dev, a.err, (unsigned long long)a.grid_words, a.w_image};
  if (!a.grid_filled) {   // grid_filled: imf_fragment_forward zeroed it and the level-0 compaction kernel set the bits
    IMF_CHECK_HIP(hipMemsetAsync(a.grid, 0, words * sizeof(uint32_t), st));
    k_bitgrid_fill<<<(unsigned)div_up(a.n, 256), 256, 0, st>>>(a.coords, a.n, a.grid, g, a.ksize, dg);
  }
  const int kvol = a.ksize * a.ksize * a.ksize;
  const size_t lds = (size_t)4 * (a.cout / 16) * kFirstParts * 64 * 16 + (size_t)kBitsRows * 4 * sizeof(uint32_t);   // B fragments + masks
  const int64_t n_slots = imf_rulebook_slots(a.n);       // with the map: conv1's 64-row blocks == the map's tiles
  const MapArgs m{a.table, (uint32_t)(a.capacity - 1), a.n_dev, a.tile_rows, a.nbr, a.tile_mask, (long long)n_slots};
  const unsigned nb = n_map ? 2u * (unsigned)(n_slots / IMF_TILE_ROWS) : (unsigned)div_up(a.n, kBitsRows);
#define IMF_FIRST_LAUNCH(C, K)                                                                                                     \
  do {                                                                                                                             \
    if (n_map)                                                                                                                     \
      k_conv_first_and_map<C, K><<<nb, 256, lds, st>>>(a.coords, a.n, a.grid, g, kvol, a.w, a.scale, a.shift, a.relu, a.out, dg,   \
                                                       a.out_split, m);                                                            \
    else                                                                                                                           \
      k_conv_first_bits<C, K><<<nb, 256, lds, st>>>(a.coords, a.n, a.grid, g, a.ksize, kvol, a.w, a.scale, a.shift, a.relu, a.out, \
                                                    dg, a.out_split);                                                              \
  } while (0)
  if (a.cout == 32 && a.ksize == 5) IMF_FIRST_LAUNCH(32, 5);
  else if (a.cout == 32)            IMF_FIRST_LAUNCH(32, 3);
  else if (a.ksize == 5)            IMF_FIRST_LAUNCH(64, 5);
  else                              IMF_FIRST_LAUNCH(64, 3);
#undef IMF_FIRST_LAUNCH
  IMF_CHECK_LAUNCH(n_map ? "k_conv_first_and_map" : "k_conv_first_bits");
  return IMF_OK;
}
}  // namespace imf

extern "C" {

int imf_conv_first_bitgrid_flags(const int32_t *coords, int64_t n, const int32_t *bbox, int ksize,
                                 uint32_t *grid, size_t grid_words, const float *w, int cout, const float *scale,
                                 const float *shift, int relu, float *out, int32_t *flags, void *stream) {
  ConvFirstArgs a{};
  a.coords = coords; a.n = n; a.bbox = bbox; a.err = flags; a.ksize = ksize; a.grid = grid; a.grid_words = grid_words;
  a.w = w; a.cout = cout; a.scale = scale; a.shift = shift; a.relu = relu; a.out = out;
  return conv_first_bitgrid(a, (hipStream_t)stream);
}

int imf_conv_first_bitgrid(const int32_t *coords, int64_t n, const int32_t *bbox, int ksize,
                           uint32_t *grid, size_t grid_words, const float *w, int cout,
                           const float *scale, const float *shift, int relu, float *out, void *stream) {
  return imf_conv_first_bitgrid_flags(coords, n, bbox, ksize, grid, grid_words, w, cout, scale, shift, relu, out, nullptr, stream);
}

int imf_conv_first_bitgrid_dyn(const int32_t *coords, int64_t n_cap, const int32_t *n_dev, const int32_t *bbox_dev,
                               int32_t *err, int ksize, uint32_t *grid, size_t grid_words, const float *w, int cout,
                               const float *scale, const float *shift, int relu, float *out, void *stream) {
  IMF_REQUIRE(n_dev && bbox_dev && err && grid_words > 0, "imf_conv_first_bitgrid_dyn: null pointer");
  ConvFirstArgs a{};
  a.coords = coords; a.n = n_cap; a.n_dev = n_dev; a.bbox_dev = bbox_dev; a.err = err; a.ksize = ksize; a.grid = grid;
  a.grid_words = grid_words; a.w = w; a.cout = cout; a.scale = scale; a.shift = shift; a.relu = relu; a.out = out;
  return conv_first_bitgrid(a, (hipStream_t)stream);
}

/* conv1's three-part f16 weight image (see first_kernel_split): [ceil(kvol / 32)][cout / 16][3 parts][64][8 halves] + the unscale factor. */
int64_t imf_first_kernel_image_floats(int kvol, int cout) { return (int64_t)((kvol + 31) / 32) * (cout / 16) * imf::kFirstParts * 64 * 4 + 4; }

int imf_pack_first_kernel(const float *w, int kvol, int cout, float *image, void *stream) {
  IMF_REQUIRE(w && image, "imf_pack_first_kernel: null pointer");
  IMF_REQUIRE((kvol == 27 || kvol == 125) && (cout == 32 || cout == 64), "imf_pack_first_kernel: kvol=%d cout=%d", kvol, cout);
  IMF_REQUIRE(aligned16(image), "imf_pack_first_kernel: image must be 16-byte aligned");
  if (cout == 32) imf::k_pack_first_kernel<32><<<1, 256, 0, (hipStream_t)stream>>>(w, kvol, image);
  else            imf::k_pack_first_kernel<64><<<1, 256, 0, (hipStream_t)stream>>>(w, kvol, image);
  IMF_CHECK_LAUNCH("k_pack_first_kernel");
  return IMF_OK;
}
}
