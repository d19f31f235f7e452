// Sparse convolution on gfx950: output-stationary gather -> fp32 MFMA small-GEMM per rulebook
// tile, fused BatchNorm / bias / residual / ReLU / L2-norm epilogue.
//
// Work decomposition (one workgroup = 4 wavefronts = one 64-row rulebook tile x one 32/64-wide
// slab of output channels x one partition of the tile's active kernel offsets):
//   wavefront w owns output rows [16w, 16w+16) of the tile and all CO_BLK 16-column blocks of the
//   slab: CO_BLK accumulators of v_mfma_f32_16x16x4_f32 (4 VGPRs each).
//   The K dimension (kernel offset k, input-channel chunk cc) is walked in 16 KiB "macro stages" of
//   packed weights.  Per macro stage:
//     - the weights (already in MFMA B-fragment order in HBM/L2) are prefetched global->VGPR one
//       stage ahead and written to one of two LDS buffers: ONE barrier per stage, loads of stage
//       n+1 in flight under the MFMAs of stage n;
//     - every lane gathers its A fragments straight from the input rows as float4 (lane l holds
//       channels 16j + 4(l>>4) + 0..3 of row nbr[k][l&15]) -- no LDS round trip for A; the tile's
//       slice of the neighbour table is cached in LDS once;
//     - a wavefront whose 16 rows have no input at offset k skips the MFMAs (wave-uniform).
//   Levels with few tiles are latency-bound, so their offsets are split over gridDim.z workgroups
//   that write raw partial sums; k_spconv_reduce adds them in a fixed order and applies the
//   epilogue.  The accumulation order per output element is fixed => bit-reproducible, no atomics.
#include "spconv_shared.h"

namespace imf {

__global__ void __launch_bounds__(256)
k_pack_weights(const float *__restrict__ w, int kvol, int cin, int cout, float *__restrict__ packed) {
  const long long total = (long long)kvol * cin * cout;
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int CI = ci_chunk_of(cin), J = CI / 16, CB = co_blk_of(cout), CW = 16 * CB;
  const int ncc = cin / CI;
  long long r = idx;
  const int t = r & 3; r >>= 2;
  const int lane = r & 63; r >>= 6;
  const int cb = r % CB; r /= CB;
  const int j = r % J; r /= J;
  const int cc = r % ncc; r /= ncc;
  const int k = r % kvol; r /= kvol;
  const int y = (int)r;
  const int ci = cc * CI + 16 * j + 4 * (lane >> 4) + t;
  const int co = y * CW + 16 * cb + (lane & 15);
  packed[idx] = w[((long long)k * cin + ci) * cout + co];
}

// ---- variant 1: simple reference kernel (single LDS buffer, two barriers per stage) -----------
template <int CO_BLK, int J>
__global__ void __launch_bounds__(256)
k_spconv_mfma_simple(const ConvParams p) {
  constexpr int STAGE_F4 = J * CO_BLK * 64;          // float4 per weight stage (<= 1024 = 16 KiB)
  __shared__ float4 wlds[STAGE_F4];

  const int tile = blockIdx.x, y = blockIdx.y;
  if (p.n_out_dev && (long long)tile * IMF_TILE_ROWS >= conv_slots(p, conv_rows(p))) return;   // capacity mode: beyond the rows
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, q4 = lane >> 4;
  const int cin = p.c_a + p.c_b;
  const int ncc = cin / (16 * J);

  uint32_t mask[IMF_MASK_WORDS] = {1u, 0u, 0u, 0u};
  if (p.tile_mask) {
#pragma unroll
    for (int w = 0; w < IMF_MASK_WORDS; ++w) mask[w] = p.tile_mask[tile * IMF_MASK_WORDS + w];
  }
  if ((mask[0] | mask[1] | mask[2] | mask[3]) == 0u) return;   // padding tile

  const long long my_slot = (long long)tile * IMF_TILE_ROWS + wave * 16 + r16;

  f32x4 acc[CO_BLK];
#pragma unroll
  for (int cb = 0; cb < CO_BLK; ++cb) acc[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const float4 *wbase = reinterpret_cast<const float4 *>(p.w_packed) +
                        (long long)y * p.kvol * ncc * STAGE_F4;

#pragma unroll 1
  for (int w = 0; w < IMF_MASK_WORDS; ++w) {
    uint32_t m = mask[w];
#pragma unroll 1
    while (m) {
      const int k = w * 32 + __builtin_ctz(m);
      m &= m - 1;
      const int irow = p.nbr ? p.nbr[(long long)k * p.n_slots + my_slot] : row_of_slot(p, my_slot);
      const bool wave_active = __any(irow >= 0);
#pragma unroll 1
      for (int cc = 0; cc < ncc; ++cc) {
        __syncthreads();                      // previous stage fully consumed
        const float4 *src = wbase + ((long long)k * ncc + cc) * STAGE_F4;
#pragma unroll
        for (int q = 0; q < STAGE_F4 / 256; ++q) wlds[q * 256 + tid] = src[q * 256 + tid];

        float4 a[J];
        if (wave_active) {
#pragma unroll
          for (int j = 0; j < J; ++j) a[j] = gather_a(p, irow, cc * 16 * J + 16 * j + 4 * q4);
        }
        __syncthreads();                      // stage visible
        if (wave_active) {
#pragma unroll
          for (int j = 0; j < J; ++j) {
#pragma unroll
            for (int cb = 0; cb < CO_BLK; ++cb) {
              const float4 b = wlds[(j * CO_BLK + cb) * 64 + lane];
              acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].x, b.x, acc[cb], 0, 0, 0);
              acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].y, b.y, acc[cb], 0, 0, 0);
              acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].z, b.z, acc[cb], 0, 0, 0);
              acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].w, b.w, acc[cb], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  conv_epilogue<CO_BLK>(p, acc, tile, y, wave, r16, q4);
}

// ---- variant 0: pipelined kernel ------------------------------------------------------------

template <int CO_BLK, int J>
__global__ void __launch_bounds__(256)
k_spconv_mfma(const ConvParams p) {
  constexpr int SUB_F4 = J * CO_BLK * 64;            // float4 per (k, cc) sub-stage
  constexpr int KG = 1024 / SUB_F4;                  // sub-stages per 16 KiB macro stage: 1, 2 or 4
  constexpr int QPS = SUB_F4 / 256;                  // float4 per thread per sub-stage: 4, 2 or 1
  __shared__ float4 wlds[2][1024];
  __shared__ int nbr_lds[kKCache][IMF_TILE_ROWS];
  __shared__ int klist[kKCache];

  const int tile = blockIdx.x, y = blockIdx.y, z = blockIdx.z, S = gridDim.z;
  if (p.n_out_dev && (long long)tile * IMF_TILE_ROWS >= conv_slots(p, conv_rows(p))) return;   // capacity mode: beyond the rows
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, q4 = lane >> 4;
  const int cin = p.c_a + p.c_b;
  const int ncc = cin / (16 * J);

  uint32_t mask[IMF_MASK_WORDS] = {1u, 0u, 0u, 0u};
  if (p.tile_mask) {
#pragma unroll
    for (int w = 0; w < IMF_MASK_WORDS; ++w) mask[w] = p.tile_mask[tile * IMF_MASK_WORDS + w];
  }
  const int total = __builtin_popcount(mask[0]) + __builtin_popcount(mask[1]) +
                    __builtin_popcount(mask[2]) + __builtin_popcount(mask[3]);
  if (total == 0 && S == 1) return;                  // padding tile
  const int lo = (int)((long long)z * total / S), hi = (int)((long long)(z + 1) * total / S);
  const int nk = hi - lo;

  if (tid == 0) {
    int ord = 0, n = 0;
#pragma unroll
    for (int w = 0; w < IMF_MASK_WORDS; ++w) {
      uint32_t m = mask[w];
      while (m) {
        const int k = w * 32 + __builtin_ctz(m);
        m &= m - 1;
        if (ord >= lo && ord < hi) klist[n++] = k;
        ++ord;
      }
    }
  }
  __syncthreads();
  const long long tile_slot0 = (long long)tile * IMF_TILE_ROWS;
  for (int j = wave; j < nk; j += 4)
    nbr_lds[j][lane] = p.nbr ? p.nbr[(long long)klist[j] * p.n_slots + tile_slot0 + lane]
                             : row_of_slot(p, tile_slot0 + lane);
  __syncthreads();

  f32x4 acc[CO_BLK];
#pragma unroll
  for (int cb = 0; cb < CO_BLK; ++cb) acc[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const float4 *wbase = reinterpret_cast<const float4 *>(p.w_packed) +
                        (long long)y * p.kvol * ncc * SUB_F4;
  const int n_sub = nk * ncc;
  const int n_macro = (n_sub + KG - 1) / KG;

  // Prefetch registers.  The four weight quads are NAMED scalars on purpose: as an array they are
  // left in scratch memory by hipcc (ROCm 7.2), which serialises the prefetch behind vmcnt waits.
  float4 w0, w1, w2, w3;
  float4 a_next[KG][J];
  const float4 *sp[KG];

  // prefetch of macro stage n: weights -> w0..w3, A fragments -> a_next
#define IMF_PREFETCH(n)                                                                           \
  {                                                                                                \
    _Pragma("unroll") for (int g = 0; g < KG; ++g) {                                              \
      const int t = (n) * KG + g;                                                                  \
      const int tc = t < n_sub ? t : n_sub - 1;   /* tail: reload the last sub-stage, unused */    \
      const int jk = tc / ncc, cc = tc - jk * ncc;                                                 \
      sp[g] = wbase + ((long long)klist[jk] * ncc + cc) * SUB_F4 + tid;                            \
      const int irow = (t < n_sub) ? nbr_lds[jk][wave * 16 + r16] : -1;                            \
      /* a (k, cc) chunk never straddles the two cat sources: c_a % (16 J) == 0 (host-checked) */   \
      const int ch0 = cc * 16 * J;                                                                 \
      const float *rowp = (ch0 < p.c_a) ? p.in_a + (long long)irow * p.c_a + ch0                   \
                                        : p.in_b + (long long)irow * p.c_b + (ch0 - p.c_a);        \
      if (irow >= 0) {                                                                             \
        _Pragma("unroll") for (int j = 0; j < J; ++j)                                              \
            a_next[g][j] = *reinterpret_cast<const float4 *>(rowp + 16 * j + 4 * q4);              \
      } else {                                                                                     \
        _Pragma("unroll") for (int j = 0; j < J; ++j) a_next[g][j] = make_float4(0.f, 0.f, 0.f, 0.f); \
      }                                                                                            \
    }                                                                                              \
    w0 = sp[0 / QPS][(0 % QPS) * 256];                                                             \
    w1 = sp[1 / QPS][(1 % QPS) * 256];                                                             \
    w2 = sp[2 / QPS][(2 % QPS) * 256];                                                             \
    w3 = sp[3 / QPS][(3 % QPS) * 256];                                                             \
  }

  if (n_macro > 0) IMF_PREFETCH(0)
#pragma unroll 1
  for (int n = 0; n < n_macro; ++n) {
    float4 *wbuf = wlds[n & 1];
    wbuf[0 * 256 + tid] = w0;
    wbuf[1 * 256 + tid] = w1;
    wbuf[2 * 256 + tid] = w2;
    wbuf[3 * 256 + tid] = w3;
    float4 a_cur[KG][J];
#pragma unroll
    for (int g = 0; g < KG; ++g) {
#pragma unroll
      for (int j = 0; j < J; ++j) a_cur[g][j] = a_next[g][j];
    }
    __syncthreads();   // stage n visible; every wave is past its reads of this buffer (stage n-2)
    if (n + 1 < n_macro) IMF_PREFETCH(n + 1)
#pragma unroll
    for (int g = 0; g < KG; ++g) {     // unconditional: empty rows carry zeros (a skipped tail adds 0)
#pragma unroll
      for (int j = 0; j < J; ++j) {
#pragma unroll
        for (int cb = 0; cb < CO_BLK; ++cb) {
          const float4 b = wbuf[g * SUB_F4 + (j * CO_BLK + cb) * 64 + lane];
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[g][j].x, b.x, acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[g][j].y, b.y, acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[g][j].z, b.z, acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[g][j].w, b.w, acc[cb], 0, 0, 0);
        }
      }
    }
  }
#undef IMF_PREFETCH

  if (S == 1) {
    conv_epilogue<CO_BLK>(p, acc, tile, y, wave, r16, q4);
  } else {   // raw partial sums, slot-major
    const int CW = 16 * CO_BLK;
#pragma unroll
    for (int cb = 0; cb < CO_BLK; ++cb) {
      const int col = y * CW + cb * 16 + r16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long slot = tile_slot0 + wave * 16 + q4 * 4 + r;
        p.partial[((long long)z * p.n_slots + slot) * p.cout + col] = acc[cb][r];
      }
    }
  }
}


// Adds the split-K partial sums in ascending partition order and applies the epilogue.
// One thread per (slot, 4 output channels).
__global__ void __launch_bounds__(256)
k_spconv_reduce(const ConvParams p, int S) {
  const int c4n = p.cout / 4;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long slot = idx / c4n;
  const int c4 = (int)(idx - slot * c4n);
  const bool in_range = slot < p.n_slots;
  const int orow = in_range ? row_of_slot(p, slot) : -1;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (orow >= 0) {
    for (int zz = 0; zz < S; ++zz) {
      const float4 v = *reinterpret_cast<const float4 *>(
          p.partial + ((long long)zz * p.n_slots + slot) * p.cout + 4 * c4);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float x[4] = {s.x, s.y, s.z, s.w};
    const float un = p.w_unscale ? *p.w_unscale : 1.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = 4 * c4 + e;
      float v = (x[e] * un) * (p.scale ? p.scale[col] : 1.f) + (p.shift ? p.shift[col] : 0.f);
      if (p.residual) v += p.residual[(long long)orow * p.cout + col];
      if (p.relu) v = fmaxf(v, 0.f);
      x[e] = v;
    }
    s = make_float4(x[0], x[1], x[2], x[3]);
    if (range_guard(p) && (out_of_f16_range(s.x) || out_of_f16_range(s.y) || out_of_f16_range(s.z) || out_of_f16_range(s.w)))
      atomicOr(p.err, 32);
  }
  if (p.l2norm) {   // cout in {32, 64}: a row = 8 or 16 consecutive lanes (all lanes take part)
    float ss = s.x * s.x + s.y * s.y + s.z * s.z + s.w * s.w;
    for (int o = 1; o < c4n; o <<= 1) ss += __shfl_xor(ss, o, 64);
    const float nrm = sqrtf(ss);
    s.x /= nrm; s.y /= nrm; s.z /= nrm; s.w /= nrm;
  }
  if (orow >= 0) *reinterpret_cast<float4 *>(p.out + (long long)orow * p.cout + 4 * c4) = s;
}

}  // namespace imf

using namespace imf;

extern "C" {

int64_t imf_packed_weight_floats(int kvol, int cin, int cout) { return (int64_t)kvol * cin * cout; }
int64_t imf_packed_weight_floats_split16(int kvol, int cin, int cout) { return (int64_t)kvol * cin * cout + 64; }

int imf_pack_weights(const float *w, int kvol, int cin, int cout, float *packed, void *stream) {
  IMF_REQUIRE(w && packed, "imf_pack_weights: null pointer");
  IMF_REQUIRE(kvol >= 1 && kvol <= IMF_MAX_KVOL, "imf_pack_weights: kvol=%d", kvol);
  IMF_REQUIRE(cin > 0 && cin % 32 == 0 && cout > 0 && cout % 32 == 0,
              "imf_pack_weights: cin=%d cout=%d must be multiples of 32", cin, cout);
  const long long total = (long long)kvol * cin * cout;
  k_pack_weights<<<(unsigned)div_up(total, 256), 256, 0, (hipStream_t)stream>>>(w, kvol, cin, cout,
                                                                                packed);
  IMF_CHECK_LAUNCH("k_pack_weights");
  return IMF_OK;
}

/* X(K<CO_BLK, J>) for the instantiation of kernel template K that serves a shape (X is variadic: the comma splits its argument). */
#define IMF_CB_J(K, cb, j, X)               \
  do {                                      \
    if (cb == 4 && j == 4) X(K<4, 4>);      \
    else if (cb == 4 && j == 2) X(K<4, 2>); \
    else if (cb == 2 && j == 4) X(K<2, 4>); \
    else X(K<2, 2>);                        \
  } while (0)

constexpr int kSplitMinBlocks = 400;   // measured: 438 unsplit workgroups (a pair's stride-2 level) beat split 2 + reduce by 1.5 % per step
constexpr int kSplitTarget = 768;      // (round-1 values; 512 ... 1536 measured in round 2)

int imf_spconv_auto_split(int64_t n_slots, int cout, int kvol) {
  if (kvol <= 1 || kvol >= 28) return 1;
  const long long blocks = (n_slots / IMF_TILE_ROWS) * (cout / (16 * co_blk_of(cout)));
  if (blocks >= kSplitMinBlocks || blocks <= 0) return 1;
  long long s = (kSplitTarget + blocks - 1) / blocks;
  if (s > 8) s = 8;
  if (s > kvol / 2) s = kvol / 2;
  return s < 1 ? 1 : (int)s;
}

size_t imf_spconv_workspace_bytes(int64_t n_slots, int cout, int split) {
  return split > 1 ? (size_t)split * (size_t)n_slots * (size_t)cout * sizeof(float) : 0;   // unsplit launches need none
}

int imf_spconv_fwd(const imf_conv_args *a, void *stream) {
  IMF_REQUIRE(a, "imf_spconv_fwd: null args");
  IMF_REQUIRE(a->in_a && a->w_packed && a->out, "imf_spconv_fwd: null pointer");
  IMF_REQUIRE(a->kvol >= 1 && a->kvol <= IMF_MAX_KVOL, "imf_spconv_fwd: kvol=%d", a->kvol);
  IMF_REQUIRE((a->nbr && a->tile_mask) || a->kvol == 1,
              "imf_spconv_fwd: nbr / tile_mask may be NULL only when kvol == 1");
  IMF_REQUIRE(a->c_a > 0 && a->c_a % 32 == 0 && a->c_b >= 0 && a->c_b % 32 == 0,
              "imf_spconv_fwd: c_a=%d c_b=%d must be multiples of 32", a->c_a, a->c_b);
  IMF_REQUIRE((a->c_b == 0) == (a->in_b == nullptr), "imf_spconv_fwd: in_b / c_b mismatch");
  IMF_REQUIRE(a->cout > 0 && a->cout % 32 == 0, "imf_spconv_fwd: cout=%d", a->cout);
  IMF_REQUIRE(a->n_slots > 0 && a->n_slots % IMF_TILE_ROWS == 0, "imf_spconv_fwd: n_slots");
  IMF_REQUIRE(a->n_out > 0 && (a->tile_rows || a->n_out <= a->n_slots), "imf_spconv_fwd: n_out");
  const int cin = a->c_a + a->c_b;
  const int J = ci_chunk_of(cin) / 16, CB = co_blk_of(a->cout);
  IMF_REQUIRE(!a->l2norm || a->cout == 16 * CB, "imf_spconv_fwd: l2norm needs cout in {32, 64}");
  IMF_REQUIRE(a->variant == 0 || a->variant == 1 || a->variant == 3 || a->variant == 6,
              "imf_spconv_fwd: variant=%d (0 = fp32 MFMA, 1 = fp32 MFMA without the pipeline, 3 = bf16x3 MFMA, 6 = split-f16 MFMA)", a->variant);
  // ---- the route: which kernel family, how many kernel-offset partitions ----
  const bool regs = (a->kernel_tag & IMF_TAG_REGS) != 0;
  const bool v16 = a->variant == 6 || a->variant == 3;   // the 16-bit matrix pipe: LDS-DMA kernels only
  // variants 0 / 1 without any pipeline: variant 1, maps of 28 offsets or more, a (k, cc) chunk that would straddle the two sources
  const bool simple = !v16 && (a->variant == 1 || a->kvol >= kKCache || (a->c_b > 0 && a->c_a % (16 * J) != 0));
  // Variant 0 (fp32 MFMA) runs on the LDS-DMA kernels too (k_spconv_g / k_spconv_w with AR = kArF32: the fp32 weight image
  // has the split-f16 image's sub-stage addressing) wherever their tables cover the shape; IMF_TAG_REGS keeps the
  // register-staged kernel k_spconv_mfma (A/B, inputs beyond IMF_CONV_ROW_WINDOW: the caller's choice, the library sees no sizes).
  const bool dma0 = a->variant == 0 && !simple && !regs && a->kvol * (cin / 32) < kSubTab && a->c_a <= 1024 && a->c_b <= 1024;
  const bool dma = v16 || dma0;
  // the wave-split kernel (spconv_w.hip): the whole unit of rows in one workgroup, no split-K partitions, no reduce launch
  const bool wsplit = dma && (a->kernel_tag & (IMF_TAG_WAVE8 | IMF_TAG_WAVE4));
  const int split = (simple || wsplit) ? 1 : (a->split_k > 0 ? a->split_k : imf_spconv_auto_split(a->n_slots, a->cout, a->kvol));

  // ---- what the route asks of the arguments ----
  if (v16) {
    IMF_REQUIRE(a->kvol < kKCache, "imf_spconv_fwd: variants 6 / 3 (split-f16 / bf16x3 weights) need kvol <= %d", kKCache - 1);
    IMF_REQUIRE(a->kvol * (cin / 32) < kSubTab && a->c_a <= 1024 && a->c_b <= 1024,
                "imf_spconv_fwd: variants 6 / 3 need kvol * cin / 32 < %d and <= 1024 channels per source (kvol=%d cin=%d): use variant 0",
                kSubTab, a->kvol, cin);
    IMF_REQUIRE(a->variant != 3 || !regs, "imf_spconv_fwd: variant 3 has no register-staged kernel");
  }
  if (wsplit) {
    IMF_REQUIRE(a->cout % 64 == 0 && (a->kvol > 1 || cin >= 256),
                "imf_spconv_fwd: the wave-split kernel needs cout %% 64 == 0 and kvol > 1 or cin >= 256 (kvol=%d cin=%d cout=%d)",
                a->kvol, cin, a->cout);
    IMF_REQUIRE(a->split_k <= 1, "imf_spconv_fwd: the wave-split kernel takes no split_k");
  }
  IMF_REQUIRE(split >= 1 && split <= 32, "imf_spconv_fwd: split_k=%d", split);
  IMF_REQUIRE(!a->n_out_dev || split == 1,
              "imf_spconv_fwd: n_out_dev (capacity mode) needs an unsplit launch (split_k = 1), got split_k=%d", split);
  if (split > 1)
    IMF_REQUIRE(a->workspace && a->workspace_bytes >= imf_spconv_workspace_bytes(a->n_slots, a->cout, split),
                "imf_spconv_fwd: split_k=%d needs %zu workspace bytes", split,
                imf_spconv_workspace_bytes(a->n_slots, a->cout, split));
  IMF_REQUIRE(!a->operand_format || (a->variant == 6 && split == 1 && !regs),
              "imf_spconv_fwd: operand_format needs variant 6 and an unsplit launch (split_k=%d)", split);
  IMF_REQUIRE(!(a->operand_format & IMF_FMT_OUT_SPLIT) || !a->l2norm, "imf_spconv_fwd: IMF_FMT_OUT_SPLIT not with l2norm");
  IMF_REQUIRE(!(a->operand_format & IMF_FMT_RES_SPLIT) || a->residual, "imf_spconv_fwd: IMF_FMT_RES_SPLIT without a residual");
  IMF_REQUIRE(!a->geglu || ((v16 || (a->variant == 0 && !simple)) && !wsplit && a->kvol == 1 && a->cout % 64 == 0 &&
                            split == 1 && !a->scale && !a->residual && !a->relu && !a->l2norm && (dma0 || !regs)),
              "imf_spconv_fwd: geglu needs variant 6 (k_spconv_g) or 0, kvol 1, cout %% 64 == 0, an unsplit launch and no other epilogue");
  if (a->variant == 6 && regs) {
    set_error("imf_spconv_fwd: variant 6 has no register-staged kernel (IMF_TAG_REGS): it belongs to variant 0");
    return IMF_EUNSUPPORTED;
  }

  ConvParams p{a->in_a, a->in_b, a->c_a, a->c_b, a->w_packed, a->kvol, a->cout, a->tile_rows,
               a->nbr, a->tile_mask, (long long)a->n_slots, (long long)a->n_out, a->scale, a->shift,
               a->residual, a->relu, a->l2norm, a->out, (float *)a->workspace};
  p.w_unscale = a->variant == 6 ? a->w_packed + (long long)a->kvol * cin * a->cout + 1 : nullptr;
  p.arith = a->variant == 6 ? kArF16x2 : (a->variant == 3 ? kArBf16x3 : kArF32);
  p.n_out_dev = a->n_out_dev;
  p.slots_extra = a->slots_extra;
  p.err = a->dyn_err;
  p.geglu = a->geglu;
  p.a_split = (a->operand_format & IMF_FMT_A_SPLIT) ? 1 : 0;
  p.res_split = (a->operand_format & IMF_FMT_RES_SPLIT) ? 1 : 0;
  p.out_split = (a->operand_format & IMF_FMT_OUT_SPLIT) ? 1 : 0;
  // XCD-contiguous tile order of k_spconv_g: workgroup b runs on XCD b % 8 and every XCD has its own 4 MiB L2, so XCD x
  // walks ONE range of consecutive tiles (cut from the actual tiles on the device; grid.x padded to a multiple of 8) and its
  // L2 serves ~1/8 of the input rows.  Same sums.  Not for parity-grouped transposed maps, whose consecutive tiles are one
  // parity class spread over the whole level.  Measurements: LAB_NOTES.md 4h-h.
  const bool g_xcd = dma && !wsplit && a->n_slots == imf_rulebook_slots(a->n_out);
  p.no_xcd_swizzle = !g_xcd;
  dim3 grid((unsigned)(a->n_slots / IMF_TILE_ROWS), (unsigned)(a->cout / (16 * CB)), (unsigned)split);
  if (g_xcd) grid.x = (grid.x + 7u) / 8u * 8u;
  hipStream_t st = (hipStream_t)stream;
  if (a->ev_begin) IMF_CHECK_HIP(hipEventRecord((hipEvent_t)a->ev_begin, st));
  if (wsplit) {
    launch_spconv_w(p, grid.x, a->kernel_tag, st);
  } else if (dma) {
    launch_spconv_g(p, grid, CB, st, a->kernel_tag & IMF_TAG_LABEL);
  } else {
#define IMF_LAUNCH(...) __VA_ARGS__<<<grid, 256, 0, st>>>(p)
    if (simple) IMF_CB_J(k_spconv_mfma_simple, CB, J, IMF_LAUNCH);
    else IMF_CB_J(k_spconv_mfma, CB, J, IMF_LAUNCH);
#undef IMF_LAUNCH
  }
  IMF_CHECK_LAUNCH("k_spconv_mfma");
  if (a->ev_end) IMF_CHECK_HIP(hipEventRecord((hipEvent_t)a->ev_end, st));
  if (split > 1) {
    const long long total = (long long)a->n_slots * (a->cout / 4);
    k_spconv_reduce<<<(unsigned)div_up(total, 256), 256, 0, st>>>(p, split);
    IMF_CHECK_LAUNCH("k_spconv_reduce");
  }
  return IMF_OK;
}

}  // extern "C"
