// The descriptor head in TRAINING: forward with saved activations, and the closed-form backward (model/resunet.py
// forward_layers after block2_tr: ME.cat(out, out_s1), conv1_tr 1x1 96 -> 64 without bias, ReLU, final 1x1 64 -> 32 with
// bias, L2 normalisation).  head.hip is the inference path (packed weights, one persistent launch); here the weights
// change every step, so every product reads them in the parameters' own layout -- `kernel` [Cin, Cout], `bias` [1, Cout],
// nothing is packed -- and [U S] is never materialised: the kernels read the two sources and write dU and dS apart.
//
//   H = relu(U W1[:cu] + S W1[cu:])     [N, 64]   saved (doubles as the ReLU mask)
//   Z = H W2 + b                        [N, 32]
//   r = sqrt(sum_c Z[:, c]^2)           [N]       saved
//   Y = Z / r  (normalize)  or  Y = Z   (r is not written)
//
//   dZ = (dY - Y sum_c(dY Y)) / r  (normalize)  or  dZ = dY
//   db = sum_rows dZ      dW2 = H^T dZ      dH = (dZ W2^T) [H > 0]      dW1 = [U S]^T dH
//   dU = dH W1[:cu]^T     dS = dH W1[cu:]^T
// No epsilon: a row with r == 0 gives the non-finite values the division gives, and raises IMF_HT_FLAG_NORM in *meta.
//
// One shape: cu 64, cs 32, ch 64, co 32 (ResUNetBN2C with 32 output channels).  All fp32, no floating-point atomics:
//   k_ht_fwd       one wavefront owns 16 rows: both products on the fp32 MFMA (v_mfma_f32_16x16x4_f32), K ascending, U's
//                  64 channels before S's 32; H goes from the accumulator layout to the operand layout through LDS.
//                  SUMMATION ORDER of r^2, a fixed shuffle tree: lane (row, j) of the 16 lanes that hold a row adds
//                  Z[j]^2 + Z[j + 16]^2, then the 16 lanes are added by the xor butterfly 8, 4, 2, 1.
//   k_ht_bwd_rows  one wavefront owns 16 rows: sum_c(dY Y) is 8 channels per lane in ascending order (4 q .. 4 q + 3, then
//                  16 + 4 q .. 16 + 4 q + 3 for lane quarter q), the four quarters added by the xor butterfly 32, 16; then
//                  dZ, dH, dU, dS on the MFMA.  dZ and dH are left in the workspace for the sums over rows.
//   k_ht_tn        every sum over rows of a product: partial[chunk] = A[chunk rows]^T B[chunk rows] on the MFMA per chunk
//                  of kHtChunk rows, rows ascending (the cut depends on N only); k_ht_colsum the same for db in fp64.
//   k_ht_final     adds the partials in chunk order in fp64 and rounds once -- the norm_train.hip / fusion_train.hip scheme.
// A row's Y, dU and dS depend on that row alone: rows split over two calls equal the rows of one call, bit for bit.
// Rows beyond N are loaded as +0.0 and never stored: padding contributes exactly nothing to any sum.
#include "common.h"

namespace imf {

typedef float ht_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kHtCu = 64;         // U: the decoder output
constexpr int kHtCs = 32;         // S: the stride-1 skip
constexpr int kHtCh = 64;         // hidden (conv1_tr's outputs)
constexpr int kHtCo = 32;         // descriptor channels
constexpr int kHtChunk = 256;     // rows per reduction chunk: part of the summation order, hence of the last bits
constexpr int kHtThreads = 256;
constexpr int kHtLd = kHtCh + 4;  // LDS row stride of a 16 x 64 tile: rows stay 16-byte aligned, quarters on other banks

// acc += A[:, 4 k-slots] B[4 k-slots, :]; lane (r16, q4) supplies k = 4 q4 + j of the 16-wide step in its j-th component
__device__ __forceinline__ void ht_mfma4(ht_f32x4 &acc, const float4 a, const float4 b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

// rows k .. k + 3 of a [K, ld] matrix at column col: the B operand of W[K][N]
__device__ __forceinline__ float4 ht_col4(const float *__restrict__ w, int k, int ld, int col) {
  const float *p = w + k * ld + col;
  return make_float4(p[0], p[ld], p[2 * ld], p[3 * ld]);
}

__device__ __forceinline__ float4 ht_row4(const float *p, bool ok) {
  return ok ? *reinterpret_cast<const float4 *>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void __launch_bounds__(kHtThreads)
k_ht_fwd(const float *__restrict__ U, const float *__restrict__ S, long long n, const float *__restrict__ W1,
         const float *__restrict__ W2, const float *__restrict__ bias, int normalize, float *__restrict__ H,
         float *__restrict__ R, float *__restrict__ Y, int32_t *meta) {
  __shared__ __attribute__((aligned(16))) float sm[4][16][kHtLd];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, q4 = lane >> 4;
  const long long row0 = ((long long)blockIdx.x * 4 + wave) * 16;
  const bool a_ok = row0 + r16 < n;
  ht_f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = (ht_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k0 = 0; k0 < kHtCu; k0 += 16) {
    const float4 a = ht_row4(U + (row0 + r16) * kHtCu + k0 + 4 * q4, a_ok);
#pragma unroll
    for (int c = 0; c < 4; ++c) ht_mfma4(acc[c], a, ht_col4(W1, k0 + 4 * q4, kHtCh, c * 16 + r16));
  }
#pragma unroll
  for (int k0 = 0; k0 < kHtCs; k0 += 16) {
    const float4 a = ht_row4(S + (row0 + r16) * kHtCs + k0 + 4 * q4, a_ok);
#pragma unroll
    for (int c = 0; c < 4; ++c) ht_mfma4(acc[c], a, ht_col4(W1, kHtCu + k0 + 4 * q4, kHtCh, c * 16 + r16));
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float t = acc[c][r];
      const float h = t > 0.f ? t : (t == t ? 0.f : t);
      const long long row = row0 + 4 * q4 + r;
      sm[wave][4 * q4 + r][c * 16 + r16] = h;
      if (row < n) H[row * kHtCh + c * 16 + r16] = h;
    }
  }
  __syncthreads();
  ht_f32x4 z[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) z[c] = (ht_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k0 = 0; k0 < kHtCh; k0 += 16) {
    const float4 a = *reinterpret_cast<const float4 *>(&sm[wave][r16][k0 + 4 * q4]);
#pragma unroll
    for (int c = 0; c < 2; ++c) ht_mfma4(z[c], a, ht_col4(W2, k0 + 4 * q4, kHtCo, c * 16 + r16));
  }
  const float b0 = bias[r16], b1 = bias[16 + r16];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long row = row0 + 4 * q4 + r;
    float y0 = z[0][r] + b0, y1 = z[1][r] + b1;
    if (normalize) {
      float s = fmaf(y1, y1, y0 * y0);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      const float rr = sqrtf(s);
      y0 = y0 / rr;
      y1 = y1 / rr;
      if (row < n && r16 == 0) {
        R[row] = rr;
        if (!(rr > 0.f && rr < __builtin_inff())) atomicOr(meta, IMF_HT_FLAG_NORM);
      }
    }
    if (row < n) {
      Y[row * kHtCo + r16] = y0;
      Y[row * kHtCo + 16 + r16] = y1;
    }
  }
}

// dZ (always) and dH (when wanted) into the workspace, dU and dS when wanted
__global__ void __launch_bounds__(kHtThreads)
k_ht_bwd_rows(const float *__restrict__ dY, const float *__restrict__ Y, const float *__restrict__ R,
              const float *__restrict__ H, const float *__restrict__ W1, const float *__restrict__ W2, long long n,
              int normalize, float *__restrict__ dZ, float *__restrict__ dH, float *__restrict__ dU,
              float *__restrict__ dS, int32_t *meta) {
  __shared__ __attribute__((aligned(16))) float sm[4][16][kHtLd];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, q4 = lane >> 4;
  const long long row0 = ((long long)blockIdx.x * 4 + wave) * 16;
  const long long arow = row0 + r16;
  const bool a_ok = arow < n;
  float4 g[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) g[kk] = ht_row4(dY + arow * kHtCo + kk * 16 + 4 * q4, a_ok);
  if (normalize) {
    float4 y[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) y[kk] = ht_row4(Y + arow * kHtCo + kk * 16 + 4 * q4, a_ok);
    float s = 0.f;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      s = fmaf(g[kk].x, y[kk].x, s);
      s = fmaf(g[kk].y, y[kk].y, s);
      s = fmaf(g[kk].z, y[kk].z, s);
      s = fmaf(g[kk].w, y[kk].w, s);
    }
    s += __shfl_xor(s, 32, 64);
    s += __shfl_xor(s, 16, 64);
    const float rr = a_ok ? R[arow] : 1.f;
    if (a_ok && q4 == 0 && !(rr > 0.f && rr < __builtin_inff())) atomicOr(meta, IMF_HT_FLAG_NORM);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      g[kk].x = (g[kk].x - y[kk].x * s) / rr;
      g[kk].y = (g[kk].y - y[kk].y * s) / rr;
      g[kk].z = (g[kk].z - y[kk].z * s) / rr;
      g[kk].w = (g[kk].w - y[kk].w * s) / rr;
    }
  }
  if (a_ok) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) *reinterpret_cast<float4 *>(dZ + arow * kHtCo + kk * 16 + 4 * q4) = g[kk];
  }
  if (!dH) return;                                                    // uniform: only db / dW2 are wanted
  // dH = (dZ W2^T) [H > 0]: W2 [ch][co] is the B operand's W[N][K]
  ht_f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = (ht_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      ht_mfma4(acc[c], g[kk], *reinterpret_cast<const float4 *>(W2 + (c * 16 + r16) * kHtCo + kk * 16 + 4 * q4));
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long row = row0 + 4 * q4 + r;
      const float h = row < n ? H[row * kHtCh + c * 16 + r16] : 0.f;
      const float v = h > 0.f ? acc[c][r] : 0.f;
      sm[wave][4 * q4 + r][c * 16 + r16] = v;
      if (row < n) dH[row * kHtCh + c * 16 + r16] = v;
    }
  }
  if (!dU && !dS) return;                                             // uniform
  __syncthreads();
  // dU = dH W1[:cu]^T, dS = dH W1[cu:]^T: W1 [cu + cs][ch] is W[N][K]
  ht_f32x4 du[4], ds[2];
#pragma unroll
  for (int c = 0; c < 4; ++c) du[c] = (ht_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 2; ++c) ds[c] = (ht_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k0 = 0; k0 < kHtCh; k0 += 16) {
    const float4 a = *reinterpret_cast<const float4 *>(&sm[wave][r16][k0 + 4 * q4]);
    if (dU) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        ht_mfma4(du[c], a, *reinterpret_cast<const float4 *>(W1 + (c * 16 + r16) * kHtCh + k0 + 4 * q4));
    }
    if (dS) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
        ht_mfma4(ds[c], a, *reinterpret_cast<const float4 *>(W1 + (kHtCu + c * 16 + r16) * kHtCh + k0 + 4 * q4));
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long row = row0 + 4 * q4 + r;
    if (row >= n) continue;
    if (dU) {
#pragma unroll
      for (int c = 0; c < 4; ++c) dU[row * kHtCu + c * 16 + r16] = du[c][r];
    }
    if (dS) {
#pragma unroll
      for (int c = 0; c < 2; ++c) dS[row * kHtCs + c * 16 + r16] = ds[c][r];
    }
  }
}

// partial[chunk][NA0 + NA1][N2] = [A0 A1][chunk rows]^T B[chunk rows]: one wavefront per 16 rows of the result
template <int NA0, int NA1, int N2>
__global__ void __launch_bounds__(kHtThreads)
k_ht_tn(const float *__restrict__ A0, const float *__restrict__ A1, const float *__restrict__ B, long long n,
        float *__restrict__ partial) {
  constexpr int N1 = NA0 + NA1, NB = N2 / 16;
  static_assert(NA0 % 16 == 0 && NA1 % 16 == 0 && N2 % 16 == 0, "whole 16 x 16 tiles");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, q4 = lane >> 4;
  const int unit = blockIdx.x * 4 + wave;
  if (unit >= N1 / 16) return;
  const long long c0 = (long long)blockIdx.y * kHtChunk;
  const long long c1 = c0 + kHtChunk < n ? c0 + kHtChunk : n;
  const int i0 = unit * 16;
  const bool first = i0 < NA0;                                        // wave-uniform: a tile never straddles the sources
  const float *A = first ? A0 + i0 + r16 : A1 + (i0 - NA0) + r16;
  const int lda = first ? NA0 : NA1;
  ht_f32x4 acc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) acc[c] = (ht_f32x4){0.f, 0.f, 0.f, 0.f};
  for (long long k0 = c0; k0 < c1; k0 += 16) {
    float a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long row = k0 + 4 * q4 + j;
      a[j] = row < c1 ? A[row * lda] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      float b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long row = k0 + 4 * q4 + j;
        b[j] = row < c1 ? B[row * N2 + c * 16 + r16] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc[c], 0, 0, 0);
    }
  }
  float *out = partial + (long long)blockIdx.y * (N1 * N2);
#pragma unroll
  for (int c = 0; c < NB; ++c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(i0 + 4 * q4 + r) * N2 + c * 16 + r16] = acc[c][r];
  }
}

// partial[chunk][col] = sum of dZ[chunk rows][col] in fp64, rows ascending
__global__ void __launch_bounds__(64)
k_ht_colsum(const float *__restrict__ dZ, long long n, double *__restrict__ partial) {
  const int col = threadIdx.x;
  if (col >= kHtCo) return;
  const long long c0 = (long long)blockIdx.x * kHtChunk;
  const long long c1 = c0 + kHtChunk < n ? c0 + kHtChunk : n;
  double s = 0.0;
  for (long long r = c0; r < c1; ++r) s += (double)dZ[r * kHtCo + col];
  partial[(long long)blockIdx.x * kHtCo + col] = s;
}

// the three parameter gradients (NULL: not wanted) = fp32(sum of the chunk partials, in chunk order, in fp64)
__global__ void __launch_bounds__(kHtThreads)
k_ht_final(const float *__restrict__ part1, const float *__restrict__ part2, const double *__restrict__ partb,
           long long chunks, float *__restrict__ dW1, float *__restrict__ dW2, float *__restrict__ db) {
  constexpr int E1 = (kHtCu + kHtCs) * kHtCh, E2 = kHtCh * kHtCo;
  const int e = blockIdx.x * kHtThreads + threadIdx.x;
  double s = 0.0;
  if (e < E1) {
    if (!dW1) return;
    for (long long k = 0; k < chunks; ++k) s += (double)part1[k * E1 + e];
    dW1[e] = (float)s;
  } else if (e < E1 + E2) {
    if (!dW2) return;
    for (long long k = 0; k < chunks; ++k) s += (double)part2[k * E2 + (e - E1)];
    dW2[e - E1] = (float)s;
  } else if (e < E1 + E2 + kHtCo) {
    if (!db) return;
    for (long long k = 0; k < chunks; ++k) s += partb[k * kHtCo + (e - E1 - E2)];
    db[e - E1 - E2] = (float)s;
  }
}

// The backward's workspace in bytes from its start (every part 256-byte aligned)
struct HtWork {
  size_t dz, dh, part1, part2, partb, total;
  long long chunks;
};
static HtWork ht_work(int64_t n) {
  HtWork w;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t a = at; at += align256(bytes); return a; };
  w.chunks = div_up(n, kHtChunk);
  w.dz = take((size_t)n * kHtCo * sizeof(float));
  w.dh = take((size_t)n * kHtCh * sizeof(float));
  w.part1 = take((size_t)w.chunks * (kHtCu + kHtCs) * kHtCh * sizeof(float));
  w.part2 = take((size_t)w.chunks * kHtCh * kHtCo * sizeof(float));
  w.partb = take((size_t)w.chunks * kHtCo * sizeof(double));
  w.total = at;
  return w;
}

constexpr int64_t kHtMaxRows = 1 << 22;     // 16384 chunks: far below the grid's 65535 in y

}  // namespace imf

using namespace imf;

extern "C" {

int imf_head_train_chunk_rows(void) { return kHtChunk; }

size_t imf_head_train_workspace_bytes(int64_t n) {
  if (n < 1 || n > kHtMaxRows) return 0;
  return ht_work(n).total;
}

#define HT_REQUIRE_SHAPE(who)                                                                                              \
  IMF_REQUIRE(cu == kHtCu && cs == kHtCs && ch == kHtCh && co == kHtCo,                                                    \
              who ": channels (%d + %d) -> %d -> %d: only (64 + 32) -> 64 -> 32", cu, cs, ch, co);                          \
  IMF_REQUIRE(n >= 0 && n <= kHtMaxRows, who ": n=%lld (0 .. %lld)", (long long)n, (long long)kHtMaxRows)

int imf_head_train_forward(const float *u, int cu, const float *s, int cs, int64_t n, const float *w1, int ch,
                           const float *w2, int co, const float *bias, int normalize, float *h, float *r, float *y,
                           int32_t *meta, void *stream) {
  HT_REQUIRE_SHAPE("imf_head_train_forward");
  if (n == 0) return IMF_OK;                                          // nothing to launch, nothing written
  IMF_REQUIRE(u && s && w1 && w2 && bias && h && y && meta && (r || !normalize), "imf_head_train_forward: null pointer");
  IMF_REQUIRE(aligned16(u) && aligned16(s) && aligned16(w1) && aligned16(w2),
              "imf_head_train_forward: u, s, w1 and w2 must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  IMF_CHECK_HIP(hipMemsetAsync(meta, 0, sizeof(int32_t), st));
  k_ht_fwd<<<(unsigned)div_up(n, 64), kHtThreads, 0, st>>>(u, s, n, w1, w2, bias, normalize != 0, h, r, y, meta);
  IMF_CHECK_LAUNCH("imf_head_train_forward");
  return IMF_OK;
}

int imf_head_train_backward(const float *dy, const float *y, const float *r, const float *h, const float *u, int cu,
                            const float *s, int cs, int64_t n, const float *w1, int ch, const float *w2, int co,
                            int normalize, float *du, float *ds, float *dw1, float *dw2, float *dbias, void *workspace,
                            size_t workspace_bytes, int32_t *meta, void *stream) {
  HT_REQUIRE_SHAPE("imf_head_train_backward");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {                                                       // no rows: the sums over rows are +0.0
    if (dw1) IMF_CHECK_HIP(hipMemsetAsync(dw1, 0, (size_t)(kHtCu + kHtCs) * kHtCh * sizeof(float), st));
    if (dw2) IMF_CHECK_HIP(hipMemsetAsync(dw2, 0, (size_t)kHtCh * kHtCo * sizeof(float), st));
    if (dbias) IMF_CHECK_HIP(hipMemsetAsync(dbias, 0, (size_t)kHtCo * sizeof(float), st));
    return IMF_OK;
  }
  IMF_REQUIRE(dy && h && u && s && w1 && w2 && workspace && meta && ((y && r) || !normalize),
              "imf_head_train_backward: null pointer");
  IMF_REQUIRE(workspace_bytes >= imf_head_train_workspace_bytes(n), "imf_head_train_backward: workspace too small (%zu bytes)",
              imf_head_train_workspace_bytes(n));
  IMF_REQUIRE(aligned16(dy) && aligned16(w1) && aligned16(w2) && aligned16(workspace) && (!normalize || aligned16(y)),
              "imf_head_train_backward: dy, y, w1, w2 and workspace must be 16-byte aligned");
  IMF_CHECK_HIP(hipMemsetAsync(meta, 0, sizeof(int32_t), st));
  if (!du && !ds && !dw1 && !dw2 && !dbias) return IMF_OK;
  const HtWork W = ht_work(n);
  char *ws = (char *)workspace;
  float *dz = (float *)(ws + W.dz), *dh = (float *)(ws + W.dh);
  float *part1 = (float *)(ws + W.part1), *part2 = (float *)(ws + W.part2);
  double *partb = (double *)(ws + W.partb);
  const bool need_dh = du || ds || dw1;
  k_ht_bwd_rows<<<(unsigned)div_up(n, 64), kHtThreads, 0, st>>>(dy, y, r, h, w1, w2, n, normalize != 0, dz,
                                                               need_dh ? dh : nullptr, du, ds, meta);
  const unsigned chunks = (unsigned)W.chunks;
  if (dw1)
    k_ht_tn<kHtCu, kHtCs, kHtCh><<<dim3(2, chunks, 1), kHtThreads, 0, st>>>(u, s, dh, n, part1);
  if (dw2)
    k_ht_tn<kHtCh, 0, kHtCo><<<dim3(1, chunks, 1), kHtThreads, 0, st>>>(h, nullptr, dz, n, part2);
  if (dbias) k_ht_colsum<<<chunks, 64, 0, st>>>(dz, n, partb);
  if (dw1 || dw2 || dbias) {
    constexpr int E = (kHtCu + kHtCs) * kHtCh + kHtCh * kHtCo + kHtCo;
    k_ht_final<<<(unsigned)div_up(E, kHtThreads), kHtThreads, 0, st>>>(part1, part2, partb, W.chunks, dw1, dw2, dbias);
  }
  IMF_CHECK_LAUNCH("imf_head_train_backward");
  return IMF_OK;
}

}  // extern "C"
