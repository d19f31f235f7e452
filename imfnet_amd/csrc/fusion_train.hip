// The bottleneck fusion block in TRAINING: forward with saved activations, and the closed-form backward
// (model/fusion.py AttentionFusion with depth 0, one head, no mask; latent 256, context 128, inner 128, GEGLU hidden 1024,
// at most 320 tokens per image).  fusion.hip is the inference path (packed weights, three launches); here the weights
// change every step, so every product reads them in the parameters' own row-major [out, in] layout -- no packing pass.
//
//   c  = LNc(tok_b)              k, v = c Wkv^T split (K first, V second)          per item b
//   q  = LN1(x) Wq^T             p = softmax(q k^T * 128^-1/2) over that item's T tokens
//   y  = (p v) Wo^T + bo + x
//   h  = LN2(y) W1^T + b1        (a, g) = h split (value first, gate second)
//   z  = (a * gelu_erf(g)) W2^T + b2 + y
//
// Three kinds of kernel, all fp32, no floating-point atomics:
//   k_ft_rows     C[rows, N] = alpha * A[rows, K] . B (+ bias) (+ residual): one wavefront owns 16 rows x 64 columns and
//                 walks K on the fp32 MFMA (v_mfma_f32_16x16x4_f32), fragments straight from memory.  B is either W[N][K]
//                 ("NT": Linear forward, q k^T, dO v^T) or W[K][N] ("NN": every input gradient, p v, ds k).  A row's result
//                 depends on that row alone: rows of a batched call equal the rows of each item run alone, bit for bit.
//   k_ft_tn       every sum over rows (weight gradients, dk / dv per item): partial[chunk] = A[chunk rows, N1]^T .
//                 B[chunk rows, N2] on the MFMA per chunk of kFtChunk rows (the cut depends on the row range only), then
//                 k_ft_tn_final adds the partials in chunk order in fp64 and rounds once -- the norm_train.hip scheme.
//   k_ft_colsum   bias and LayerNorm-parameter gradients: fp64 column sums per chunk, rows in ascending order, then
//                 k_ft_colsum_final in chunk order.
// LayerNorm, softmax and their backwards are one wavefront per row with fixed xor butterflies.
// Rows and tokens beyond a range are loaded as +0.0 and never stored: padding contributes exactly nothing to any sum.
//
// The batch partition is a DEVICE array of n_items + 1 ascending row starts; nothing here waits for the device.  An
// item kernel validates its item's range (0 <= s0 <= s1 <= n, starts[0] == 0, starts[n_items] == n); a bad range raises
// IMF_FT_FLAG_STARTS in *meta and that item's workgroups leave without touching memory.
#include "common.h"

namespace imf {

typedef float ft_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFtD = 256;        // latent dim (the stride-8 rows)
constexpr int kFtC = 128;        // context dim (image tokens)
constexpr int kFtQ = 128;        // attention inner dim
constexpr int kFtH = 1024;       // GEGLU hidden
constexpr int kFtMaxTok = 320;
constexpr int kFtLdP = 320;      // row stride of the probabilities / score gradients; columns >= T are +0.0
constexpr int kFtChunk = 256;    // rows per reduction chunk: part of the summation order, hence of the last bits
constexpr int kFtThreads = 256;

// rows [r0, r1) of item b; false (and the flag) for a range that is not inside [0, n] or breaks the partition
__device__ __forceinline__ bool ft_item_rows(const int32_t *__restrict__ starts, int b, int n_items, long long n,
                                             int32_t *meta, long long &r0, long long &r1) {
  const long long s0 = starts[b], s1 = starts[b + 1];
  bool ok = s0 >= 0 && s0 <= s1 && s1 <= n;
  if (b == 0 && s0 != 0) ok = false;
  if (b == n_items - 1 && s1 != n) ok = false;
  r0 = ok ? s0 : 0;
  r1 = ok ? s1 : 0;
  if (!ok && threadIdx.x == 0) atomicOr(meta, IMF_FT_FLAG_STARTS);
  return ok;
}

struct FtRows {
  const float *A; long long lda;            // [rows, K], K contiguous, lda % 4 == 0
  const float *B; long long ldb;            // NT: W[N][K] (row stride ldb); NN: W[K][N]
  long long b_item;                         // item mode: B of item b = B + b * b_item
  float *C; long long ldc;
  const float *bias;                        // [N] or NULL
  const float *res; long long ldres;        // [rows, N] or NULL
  float alpha;
  int N, K, Kb;                             // K % 16 == 0 is walked; NN: rows k >= Kb of B read as +0.0
  long long n;                              // rows (all items)
  const int32_t *starts; int n_items; int32_t *meta;   // item mode (blockIdx.z = item), else NULL
};

template <bool NT>
__global__ void __launch_bounds__(kFtThreads)
k_ft_rows(const FtRows p) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, q4 = lane >> 4;
  long long r0 = 0, r1 = p.n;
  const float *B = p.B;
  if (p.starts) {
    if (!ft_item_rows(p.starts, blockIdx.z, p.n_items, p.n, p.meta, r0, r1)) return;
    B += (long long)blockIdx.z * p.b_item;
  }
  const int groups = (p.N + 63) / 64;
  const long long unit = (long long)blockIdx.x * 4 + wave;
  const long long row0 = r0 + unit / groups * 16;
  const int n0 = (int)(unit % groups) * 64;
  if (row0 >= r1) return;
  const bool a_ok = row0 + r16 < r1;
  const float *ap = p.A + (row0 + r16) * p.lda + 4 * q4;
  ft_f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = (ft_f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < p.K; k0 += 16) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a_ok) a = *reinterpret_cast<const float4 *>(ap + k0);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (n0 + c * 16 >= p.N) continue;                       // a column block beyond N (wave-uniform)
      const int col = n0 + c * 16 + r16;
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (col < p.N) {
        if constexpr (NT) {
          b = *reinterpret_cast<const float4 *>(B + (long long)col * p.ldb + k0 + 4 * q4);
        } else {
          const int k = k0 + 4 * q4;
          const float *bp = B + (long long)k * p.ldb + col;
          if (k + 0 < p.Kb) b.x = bp[0];
          if (k + 1 < p.Kb) b.y = bp[p.ldb];
          if (k + 2 < p.Kb) b.z = bp[2 * p.ldb];
          if (k + 3 < p.Kb) b.w = bp[3 * p.ldb];
        }
      }
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[c], 0, 0, 0);
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[c], 0, 0, 0);
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[c], 0, 0, 0);
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[c], 0, 0, 0);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = n0 + c * 16 + r16;
    if (col >= p.N) continue;
    const float bias = p.bias ? p.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long row = row0 + 4 * q4 + r;
      if (row >= r1) continue;
      float v = acc[c][r] * p.alpha;
      if (p.bias) v += bias;
      if (p.res) v += p.res[row * p.ldres + col];
      p.C[row * p.ldc + col] = v;
    }
  }
}

struct FtTn {
  const float *A; long long lda; int N1;    // [rows, N1]
  const float *B; long long ldb; int N2;    // [rows, N2]
  float *partial;                           // [items][cmax][N1][N2]
  int cmax;
  long long n;
  const int32_t *starts; int n_items; int32_t *meta;   // item mode (blockIdx.z = item; chunks count from the item's first row)
};

__global__ void __launch_bounds__(kFtThreads)
k_ft_tn(const FtTn p) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, q4 = lane >> 4;
  long long r0 = 0, r1 = p.n;
  if (p.starts && !ft_item_rows(p.starts, blockIdx.z, p.n_items, p.n, p.meta, r0, r1)) return;
  const long long c0 = r0 + (long long)blockIdx.y * kFtChunk;
  if (c0 >= r1) return;
  const long long c1 = c0 + kFtChunk < r1 ? c0 + kFtChunk : r1;
  const int groups = (p.N2 + 63) / 64, tiles = (p.N1 + 15) / 16;
  const long long unit = (long long)blockIdx.x * 4 + wave;
  if (unit >= (long long)tiles * groups) return;
  const int i0 = (int)(unit / groups) * 16, j0 = (int)(unit % groups) * 64;
  const bool a_ok = i0 + r16 < p.N1;
  ft_f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = (ft_f32x4){0.f, 0.f, 0.f, 0.f};
  for (long long k0 = c0; k0 < c1; k0 += 16) {
    float a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long row = k0 + 4 * q4 + j;
      a[j] = (a_ok && row < c1) ? p.A[row * p.lda + i0 + r16] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (j0 + c * 16 >= p.N2) continue;
      const int col = j0 + c * 16 + r16;
      float b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long row = k0 + 4 * q4 + j;
        b[j] = (col < p.N2 && row < c1) ? p.B[row * p.ldb + col] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc[c], 0, 0, 0);
    }
  }
  float *out = p.partial + ((long long)blockIdx.z * p.cmax + blockIdx.y) * ((long long)p.N1 * p.N2);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = j0 + c * 16 + r16;
    if (col >= p.N2) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 4 * q4 + r;
      if (i < p.N1) out[(long long)i * p.N2 + col] = acc[c][r];
    }
  }
}

// out[item][i][j] = fp32(sum over the item's chunks, in chunk order, in fp64); +0.0 for an item without rows
__global__ void __launch_bounds__(kFtThreads)
k_ft_tn_final(const float *__restrict__ partial, int cmax, int N1, int N2, long long n, const int32_t *starts, int n_items,
              int32_t *meta, float *__restrict__ out, long long out_item, long long ldo) {
  long long r0 = 0, r1 = n;
  if (starts) ft_item_rows(starts, blockIdx.y, n_items, n, meta, r0, r1);
  const long long chunks = (r1 - r0 + kFtChunk - 1) / kFtChunk, E = (long long)N1 * N2;
  const long long e = (long long)blockIdx.x * kFtThreads + threadIdx.x;
  if (e >= E) return;
  const float *src = partial + (long long)blockIdx.y * cmax * E + e;
  double s = 0.0;
  for (long long k = 0; k < chunks; ++k) s += (double)src[k * E];
  out[(long long)blockIdx.y * out_item + e / N2 * ldo + e % N2] = (float)s;
}

// partial[chunk][0][col] = sum g, partial[chunk][1][col] = sum g * xh (LN: xh = (x - mean[row]) * rstd[row]); fp64, rows ascending
template <bool LN>
__global__ void __launch_bounds__(kFtThreads)
k_ft_colsum(const float *__restrict__ g, const float *__restrict__ x, const float *__restrict__ stats, long long rows, int C,
            double *__restrict__ partial) {
  const int col = blockIdx.y * kFtThreads + threadIdx.x;
  if (col >= C) return;
  const long long c0 = (long long)blockIdx.x * kFtChunk;
  const long long c1 = c0 + kFtChunk < rows ? c0 + kFtChunk : rows;
  double s1 = 0.0, s2 = 0.0;
  for (long long r = c0; r < c1; ++r) {
    const double gv = (double)g[r * C + col];
    s1 += gv;
    if constexpr (LN) s2 = fma(gv, ((double)x[r * C + col] - (double)stats[2 * r]) * (double)stats[2 * r + 1], s2);
  }
  partial[((long long)blockIdx.x * 2) * C + col] = s1;
  if constexpr (LN) partial[((long long)blockIdx.x * 2 + 1) * C + col] = s2;
}

__global__ void __launch_bounds__(kFtThreads)
k_ft_colsum_final(const double *__restrict__ partial, long long chunks, int C, float *__restrict__ out_sum,
                  float *__restrict__ out_sum_xh) {
  const int col = blockIdx.x * kFtThreads + threadIdx.x;
  if (col >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (long long k = 0; k < chunks; ++k) {
    s1 += partial[(k * 2) * C + col];
    if (out_sum_xh) s2 += partial[(k * 2 + 1) * C + col];
  }
  if (out_sum) out_sum[col] = (float)s1;
  if (out_sum_xh) out_sum_xh[col] = (float)s2;
}

// LayerNorm (eps 1e-5, biased variance) of rows W wide: one wavefront per row, W / 64 values per lane.
// stats[2 row] = mean, stats[2 row + 1] = rstd.
template <int W>
__global__ void __launch_bounds__(kFtThreads)
k_ft_ln(const float *__restrict__ x, long long rows, const float *__restrict__ gamma, const float *__restrict__ beta,
        float *__restrict__ out, float *__restrict__ stats) {
  constexpr int PER = W / 64;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[PER], s = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    v[j] = x[row * W + PER * lane + j];
    s += v[j];
  }
  const float mean = wave_sum(s) * (1.f / W);
  float s2 = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    v[j] -= mean;
    s2 = fmaf(v[j], v[j], s2);
  }
  const float rstd = 1.f / sqrtf(wave_sum(s2) * (1.f / W) + 1e-5f);
#pragma unroll
  for (int j = 0; j < PER; ++j)
    out[row * W + PER * lane + j] = fmaf(v[j] * rstd, gamma[PER * lane + j], beta[PER * lane + j]);
  if (lane == 0) {
    stats[2 * row] = mean;
    stats[2 * row + 1] = rstd;
  }
}

// dx = rstd * (g - mean(g) - xh * mean(g xh)) (+ res), g = dn * gamma, xh = (x - mean) * rstd
template <int W>
__global__ void __launch_bounds__(kFtThreads)
k_ft_ln_bwd(const float *__restrict__ dn, const float *__restrict__ x, const float *__restrict__ stats,
            const float *__restrict__ gamma, const float *__restrict__ res, float *__restrict__ dx, long long rows) {
  constexpr int PER = W / 64;
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float mean = stats[2 * row], rstd = stats[2 * row + 1];
  float g[PER], xh[PER], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const long long at = row * W + PER * lane + j;
    g[j] = dn[at] * gamma[PER * lane + j];
    xh[j] = (x[at] - mean) * rstd;
    s1 += g[j];
    s2 = fmaf(g[j], xh[j], s2);
  }
  const float m1 = wave_sum(s1) * (1.f / W), m2 = wave_sum(s2) * (1.f / W);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const long long at = row * W + PER * lane + j;
    float v = rstd * ((g[j] - m1) - xh[j] * m2);
    if (res) v += res[at];
    dx[at] = v;
  }
}

// in place over P [n][kFtLdP]: scores -> probabilities over columns < T; columns T .. kFtLdP - 1 <- +0.0
__global__ void __launch_bounds__(kFtThreads)
k_ft_softmax(float *__restrict__ P, long long n, int T) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  float *srow = P + row * kFtLdP;
  float v[5], m = -3.0e38f;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < T ? srow[c] : -3.0e38f;
    m = fmaxf(m, v[i]);
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < T ? expf(v[i] - m) : 0.f;
    s += v[i];
  }
  s = wave_sum(s);
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int c = lane + 64 * i;
    srow[c] = c < T ? v[i] / s : 0.f;
  }
}

// in place over dP: ds = p * (dp - sum_t p dp) * scale over columns < T; columns T .. kFtLdP - 1 <- +0.0
__global__ void __launch_bounds__(kFtThreads)
k_ft_softmax_bwd(const float *__restrict__ P, float *__restrict__ dP, long long n, int T, float scale) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const float *prow = P + row * kFtLdP;
  float *drow = dP + row * kFtLdP;
  float pv[5], dv[5], s = 0.f;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int c = lane + 64 * i;
    pv[i] = c < T ? prow[c] : 0.f;
    dv[i] = c < T ? drow[c] : 0.f;
    s = fmaf(pv[i], dv[i], s);
  }
  s = wave_sum(s);
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int c = lane + 64 * i;
    drow[c] = c < T ? pv[i] * (dv[i] - s) * scale : 0.f;
  }
}

// u = a * gelu(g), (a, g) = h[:, :1024], h[:, 1024:]; exact (erf) GELU
__global__ void __launch_bounds__(kFtThreads)
k_ft_geglu(const float *__restrict__ h, float *__restrict__ u, long long total) {
  const long long e = (long long)blockIdx.x * kFtThreads + threadIdx.x;
  if (e >= total) return;
  const long long r = e / kFtH;
  const int c = (int)(e % kFtH);
  const float a = h[r * 2 * kFtH + c], g = h[r * 2 * kFtH + kFtH + c];
  u[e] = a * (g * 0.5f * (1.f + erff(g * 0.70710678118654752440f)));
}

// da = du * gelu(g), dg = du * a * gelu'(g), gelu'(g) = Phi(g) + g phi(g)
__global__ void __launch_bounds__(kFtThreads)
k_ft_geglu_bwd(const float *__restrict__ h, const float *__restrict__ du, float *__restrict__ dh, long long total) {
  const long long e = (long long)blockIdx.x * kFtThreads + threadIdx.x;
  if (e >= total) return;
  const long long r = e / kFtH;
  const int c = (int)(e % kFtH);
  const float a = h[r * 2 * kFtH + c], g = h[r * 2 * kFtH + kFtH + c], d = du[e];
  const float cdf = 0.5f * (1.f + erff(g * 0.70710678118654752440f));
  const float pdf = expf(-0.5f * g * g) * 0.39894228040143267794f;
  dh[r * 2 * kFtH + c] = d * (g * cdf);
  dh[r * 2 * kFtH + kFtH + c] = d * a * fmaf(g, pdf, cdf);
}

// ---- host side ------------------------------------------------------------------------------------------------------

static inline size_t ft_pad4(size_t floats) { return (floats + 3) / 4 * 4; }

// What the forward leaves for the backward, in floats from the start of `saved` (every part 16-byte aligned)
struct FtSaved {
  size_t stat1, stat2, statc, n1, q, p, o, y, n2, h, u, c, kv, total;
};
static FtSaved ft_saved(int64_t n, int items, int T) {
  FtSaved s;
  size_t at = 0;
  const size_t N = (size_t)n, BT = (size_t)items * T;
  auto take = [&](size_t floats) { const size_t a = at; at += ft_pad4(floats); return a; };
  s.stat1 = take(2 * N); s.stat2 = take(2 * N); s.statc = take(2 * BT);
  s.n1 = take(N * kFtD); s.q = take(N * kFtQ); s.p = take(N * kFtLdP); s.o = take(N * kFtQ);
  s.y = take(N * kFtD); s.n2 = take(N * kFtD); s.h = take(N * 2 * kFtH); s.u = take(N * kFtH);
  s.c = take(BT * kFtC); s.kv = take(BT * 2 * kFtQ);
  s.total = at;
  return s;
}

// The backward's scratch, in floats; `colpart` (fp64) is 8-byte aligned because every part is a multiple of 4 floats
struct FtWork {
  size_t du, dh, dn, dy, dO, dP, dq, dkv, dc, part, colpart, total;
  int cm_n, cm_bt;
};
static FtWork ft_work(int64_t n, int items, int T) {
  FtWork w;
  size_t at = 0;
  const size_t N = (size_t)n, BT = (size_t)items * T;
  auto take = [&](size_t floats) { const size_t a = at; at += ft_pad4(floats); return a; };
  w.cm_n = (int)div_up(n, kFtChunk);
  w.cm_bt = (int)div_up((int64_t)BT, kFtChunk);
  w.du = take(N * kFtH); w.dh = take(N * 2 * kFtH); w.dn = take(N * kFtD); w.dy = take(N * kFtD);
  w.dO = take(N * kFtQ); w.dP = take(N * kFtLdP); w.dq = take(N * kFtQ); w.dkv = take(BT * 2 * kFtQ); w.dc = take(BT * kFtC);
  size_t part = (size_t)w.cm_n * 2 * kFtH * kFtD;                                    // dW1, the largest weight
  const size_t part_item = (size_t)items * w.cm_n * T * kFtQ;                        // dk or dv of every item
  const size_t part_kv = (size_t)w.cm_bt * 2 * kFtQ * kFtC;                          // dWkv
  part = part > part_item ? part : part_item;
  part = part > part_kv ? part : part_kv;
  w.part = take(part);
  const size_t cm = w.cm_n > w.cm_bt ? w.cm_n : w.cm_bt;
  w.colpart = take(cm * 2 * 2 * kFtH * 2);                                           // [chunk][2][<= 2048] doubles
  w.total = at;
  return w;
}

static bool ft_sizes_ok(int64_t n, int items, int T) {
  return n >= 0 && n <= (1 << 22) && items >= 1 && items <= 65535 && T >= 1 && T <= kFtMaxTok;
}

static FtRows ft_rows_args(const float *A, long long lda, const float *B, long long ldb, float *C, long long ldc, int N, int K,
                           long long rows) {
  FtRows p;
  p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.b_item = 0; p.C = C; p.ldc = ldc; p.bias = nullptr; p.res = nullptr;
  p.ldres = 0; p.alpha = 1.f; p.N = N; p.K = K; p.Kb = K; p.n = rows; p.starts = nullptr; p.n_items = 1; p.meta = nullptr;
  return p;
}
static void ft_items(FtRows &p, const int32_t *starts, int items, int32_t *meta, long long b_item) {
  p.starts = starts; p.n_items = items; p.meta = meta; p.b_item = b_item;
}
template <bool NT> static void ft_rows_launch(const FtRows &p, hipStream_t st) {
  const long long units = div_up(p.n, 16) * div_up(p.N, 64);      // item mode: every item's grid covers all n rows
  k_ft_rows<NT><<<dim3((unsigned)div_up(units, 4), 1, p.starts ? p.n_items : 1), kFtThreads, 0, st>>>(p);
}

// out[item][N1][N2] (+ out_item per item, row stride ldo) = sum over the rows of A^T B; starts NULL: one range [0, rows)
static void ft_tn_launch(const float *A, long long lda, int N1, const float *B, long long ldb, int N2, long long rows, int cmax,
                         const int32_t *starts, int items, int32_t *meta, float *partial, float *out, long long out_item,
                         long long ldo, hipStream_t st) {
  FtTn p;
  p.A = A; p.lda = lda; p.N1 = N1; p.B = B; p.ldb = ldb; p.N2 = N2; p.partial = partial; p.cmax = cmax; p.n = rows;
  p.starts = starts; p.n_items = items; p.meta = meta;
  const int nz = starts ? items : 1;
  const long long units = div_up(N1, 16) * div_up(N2, 64);
  k_ft_tn<<<dim3((unsigned)div_up(units, 4), (unsigned)cmax, nz), kFtThreads, 0, st>>>(p);
  k_ft_tn_final<<<dim3((unsigned)div_up((long long)N1 * N2, kFtThreads), nz, 1), kFtThreads, 0, st>>>(
      partial, cmax, N1, N2, rows, starts, items, meta, out, out_item, ldo);
}

// out_sum[col] = sum_r g[r][col]; out_sum_xh[col] = sum_r g[r][col] * xh[r][col] (needs x and the rows' LayerNorm stats)
static void ft_colsum_launch(const float *g, const float *x, const float *stats, long long rows, int C, double *partial,
                             float *out_sum, float *out_sum_xh, hipStream_t st) {
  const long long chunks = div_up(rows, kFtChunk);
  const dim3 grid((unsigned)chunks, (unsigned)div_up(C, kFtThreads), 1);
  if (out_sum_xh) {
    k_ft_colsum<true><<<grid, kFtThreads, 0, st>>>(g, x, stats, rows, C, partial);
  } else {
    k_ft_colsum<false><<<grid, kFtThreads, 0, st>>>(g, nullptr, nullptr, rows, C, partial);
  }
  k_ft_colsum_final<<<(unsigned)div_up(C, kFtThreads), kFtThreads, 0, st>>>(partial, chunks, C, out_sum, out_sum_xh);
}

}  // namespace imf

using namespace imf;

extern "C" {

int imf_fusion_train_chunk_rows(void) { return kFtChunk; }

size_t imf_fusion_train_saved_bytes(int64_t n, int n_items, int n_tokens) {
  if (!ft_sizes_ok(n, n_items, n_tokens)) return 0;
  return ft_saved(n, n_items, n_tokens).total * sizeof(float);
}

size_t imf_fusion_train_workspace_bytes(int64_t n, int n_items, int n_tokens) {
  if (!ft_sizes_ok(n, n_items, n_tokens)) return 0;
  return ft_work(n, n_items, n_tokens).total * sizeof(float);
}

#define FT_REQUIRE_COMMON(who)                                                                                              \
  IMF_REQUIRE(latent_dim == kFtD && context_dim == kFtC && inner_dim == kFtQ && hidden_dim == kFtH,                         \
              who ": dims (%d, %d, %d, %d): only latent 256, context 128, inner 128, hidden 1024", latent_dim, context_dim, \
              inner_dim, hidden_dim);                                                                                       \
  IMF_REQUIRE(n_tokens >= 1 && n_tokens <= kFtMaxTok, who ": n_tokens=%d (1 .. %d)", n_tokens, kFtMaxTok);                  \
  IMF_REQUIRE(n >= 0 && n <= (1 << 22) && n_items >= 1 && n_items <= 65535, who ": n=%lld n_items=%d", (long long)n, n_items); \
  if (n == 0) return IMF_OK;                                        /* nothing to launch; x and z may be null */           \
  IMF_REQUIRE(x && item_starts && tokens && weights && saved && meta, who ": null pointer");                                \
  for (int i = 0; i < IMF_FT_NPARAM; ++i) IMF_REQUIRE(weights[i], who ": null pointer (weights[%d])", i);                    \
  IMF_REQUIRE(saved_bytes >= imf_fusion_train_saved_bytes(n, n_items, n_tokens), who ": saved buffer too small (%zu bytes)", \
              imf_fusion_train_saved_bytes(n, n_items, n_tokens));                                                          \
  IMF_REQUIRE(aligned16(x) && aligned16(tokens) && aligned16(saved), who ": x, tokens and saved must be 16-byte aligned"); \
  for (int i = 0; i < IMF_FT_NPARAM; ++i) IMF_REQUIRE(aligned16(weights[i]), who ": weights[%d] must be 16-byte aligned", i)

int imf_fusion_train_forward(const float *x, int64_t n, const int32_t *item_starts, int n_items, const float *tokens,
                             int n_tokens, int latent_dim, int context_dim, int inner_dim, int hidden_dim,
                             const float *const *weights, float *z, float *saved, size_t saved_bytes, int32_t *meta,
                             void *stream) {
  FT_REQUIRE_COMMON("imf_fusion_train_forward");
  IMF_REQUIRE(z, "imf_fusion_train_forward: null pointer (z)");
  IMF_REQUIRE(aligned16(z), "imf_fusion_train_forward: z must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int T = n_tokens, Tp = (int)div_up(T, 16) * 16;
  const long long BT = (long long)n_items * T;
  const FtSaved S = ft_saved(n, n_items, T);
  const float *const *w = weights;
  float *c = saved + S.c, *kv = saved + S.kv, *n1 = saved + S.n1, *q = saved + S.q, *P = saved + S.p, *o = saved + S.o;
  float *y = saved + S.y, *n2 = saved + S.n2, *h = saved + S.h, *u = saved + S.u;
  IMF_CHECK_HIP(hipMemsetAsync(meta, 0, sizeof(int32_t), st));
  // context: c = LNc(tok), kv = c Wkv^T
  k_ft_ln<kFtC><<<(unsigned)div_up(BT, 4), kFtThreads, 0, st>>>(tokens, BT, w[IMF_FT_LNC_G], w[IMF_FT_LNC_B], c, saved + S.statc);
  ft_rows_launch<true>(ft_rows_args(c, kFtC, w[IMF_FT_WKV], kFtC, kv, 2 * kFtQ, 2 * kFtQ, kFtC, BT), st);
  // q = LN1(x) Wq^T
  k_ft_ln<kFtD><<<(unsigned)div_up(n, 4), kFtThreads, 0, st>>>(x, n, w[IMF_FT_LN1_G], w[IMF_FT_LN1_B], n1, saved + S.stat1);
  ft_rows_launch<true>(ft_rows_args(n1, kFtD, w[IMF_FT_WQ], kFtD, q, kFtQ, kFtQ, kFtD, n), st);
  // p = softmax(q k^T * scale) per item
  {
    FtRows p = ft_rows_args(q, kFtQ, kv, 2 * kFtQ, P, kFtLdP, T, kFtQ, n);
    p.alpha = 0.08838834764831845f;                                   // 128^-1/2
    ft_items(p, item_starts, n_items, meta, (long long)T * 2 * kFtQ);
    ft_rows_launch<true>(p, st);
  }
  k_ft_softmax<<<(unsigned)div_up(n, 4), kFtThreads, 0, st>>>(P, n, T);
  // o = p v per item
  {
    FtRows p = ft_rows_args(P, kFtLdP, kv + kFtQ, 2 * kFtQ, o, kFtQ, kFtQ, Tp, n);
    p.Kb = T;
    ft_items(p, item_starts, n_items, meta, (long long)T * 2 * kFtQ);
    ft_rows_launch<false>(p, st);
  }
  // y = o Wo^T + bo + x
  {
    FtRows p = ft_rows_args(o, kFtQ, w[IMF_FT_WO], kFtQ, y, kFtD, kFtD, kFtQ, n);
    p.bias = w[IMF_FT_BO]; p.res = x; p.ldres = kFtD;
    ft_rows_launch<true>(p, st);
  }
  // h = LN2(y) W1^T + b1, u = GEGLU(h), z = u W2^T + b2 + y
  k_ft_ln<kFtD><<<(unsigned)div_up(n, 4), kFtThreads, 0, st>>>(y, n, w[IMF_FT_LN2_G], w[IMF_FT_LN2_B], n2, saved + S.stat2);
  {
    FtRows p = ft_rows_args(n2, kFtD, w[IMF_FT_W1], kFtD, h, 2 * kFtH, 2 * kFtH, kFtD, n);
    p.bias = w[IMF_FT_B1];
    ft_rows_launch<true>(p, st);
  }
  k_ft_geglu<<<(unsigned)div_up(n * kFtH, kFtThreads), kFtThreads, 0, st>>>(h, u, (long long)n * kFtH);
  {
    FtRows p = ft_rows_args(u, kFtH, w[IMF_FT_W2], kFtH, z, kFtD, kFtD, kFtH, n);
    p.bias = w[IMF_FT_B2]; p.res = y; p.ldres = kFtD;
    ft_rows_launch<true>(p, st);
  }
  IMF_CHECK_LAUNCH("imf_fusion_train_forward");
  return IMF_OK;
}

int imf_fusion_train_backward(const float *dz, const float *x, int64_t n, const int32_t *item_starts, int n_items,
                              const float *tokens, int n_tokens, int latent_dim, int context_dim, int inner_dim,
                              int hidden_dim, const float *const *weights, const float *saved, size_t saved_bytes, float *dx,
                              float *dtokens, float *const *grads, int32_t *meta, void *workspace, size_t workspace_bytes,
                              void *stream) {
  FT_REQUIRE_COMMON("imf_fusion_train_backward");
  IMF_REQUIRE(dz && grads && workspace, "imf_fusion_train_backward: null pointer");
  IMF_REQUIRE(workspace_bytes >= imf_fusion_train_workspace_bytes(n, n_items, n_tokens),
              "imf_fusion_train_backward: workspace too small (%zu bytes)", imf_fusion_train_workspace_bytes(n, n_items, n_tokens));
  IMF_REQUIRE(aligned16(dz) && aligned16(workspace) && aligned16(dx) && aligned16(dtokens),
              "imf_fusion_train_backward: dz, dx, dtokens and workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int T = n_tokens, Tp = (int)div_up(T, 16) * 16;
  const long long BT = (long long)n_items * T, kv_item = (long long)T * 2 * kFtQ;
  const FtSaved S = ft_saved(n, n_items, T);
  const FtWork W = ft_work(n, n_items, T);
  const float *const *w = weights;
  float *const *g = grads;
  const float *c = saved + S.c, *kv = saved + S.kv, *n1 = saved + S.n1, *q = saved + S.q, *P = saved + S.p, *o = saved + S.o;
  const float *y = saved + S.y, *n2 = saved + S.n2, *h = saved + S.h, *u = saved + S.u;
  float *ws = (float *)workspace;
  float *du = ws + W.du, *dh = ws + W.dh, *dn = ws + W.dn, *dy = ws + W.dy, *dO = ws + W.dO, *dP = ws + W.dP, *dq = ws + W.dq;
  float *dkv = ws + W.dkv, *dc = ws + W.dc, *part = ws + W.part;
  double *colpart = (double *)(ws + W.colpart);

  const bool need_kv = dtokens || g[IMF_FT_WKV] || g[IMF_FT_LNC_G] || g[IMF_FT_LNC_B];
  const bool need_dn1 = dx || g[IMF_FT_LN1_G] || g[IMF_FT_LN1_B];
  const bool need_q = need_dn1 || g[IMF_FT_WQ];
  const bool need_do = need_kv || need_q;
  const bool need_dy = need_do || g[IMF_FT_WO] || g[IMF_FT_BO];
  const bool need_dn2 = need_dy || g[IMF_FT_LN2_G] || g[IMF_FT_LN2_B];
  const bool need_dh = need_dn2 || g[IMF_FT_W1] || g[IMF_FT_B1];
  IMF_CHECK_HIP(hipMemsetAsync(meta, 0, sizeof(int32_t), st));

  // z = u W2^T + b2 + y
  if (g[IMF_FT_W2]) ft_tn_launch(dz, kFtD, kFtD, u, kFtH, kFtH, n, W.cm_n, nullptr, 1, meta, part, g[IMF_FT_W2], 0, kFtH, st);
  if (g[IMF_FT_B2]) ft_colsum_launch(dz, nullptr, nullptr, n, kFtD, colpart, g[IMF_FT_B2], nullptr, st);
  if (need_dh) {
    ft_rows_launch<false>(ft_rows_args(dz, kFtD, w[IMF_FT_W2], kFtH, du, kFtH, kFtH, kFtD, n), st);
    k_ft_geglu_bwd<<<(unsigned)div_up(n * kFtH, kFtThreads), kFtThreads, 0, st>>>(h, du, dh, (long long)n * kFtH);
    // h = LN2(y) W1^T + b1
    if (g[IMF_FT_W1]) ft_tn_launch(dh, 2 * kFtH, 2 * kFtH, n2, kFtD, kFtD, n, W.cm_n, nullptr, 1, meta, part, g[IMF_FT_W1], 0, kFtD, st);
    if (g[IMF_FT_B1]) ft_colsum_launch(dh, nullptr, nullptr, n, 2 * kFtH, colpart, g[IMF_FT_B1], nullptr, st);
  }
  if (need_dn2) {
    ft_rows_launch<false>(ft_rows_args(dh, 2 * kFtH, w[IMF_FT_W1], kFtD, dn, kFtD, kFtD, 2 * kFtH, n), st);
    if (g[IMF_FT_LN2_G] || g[IMF_FT_LN2_B])
      ft_colsum_launch(dn, y, saved + S.stat2, n, kFtD, colpart, g[IMF_FT_LN2_B], g[IMF_FT_LN2_G], st);
  }
  if (need_dy) {
    // dy = dz + LN2'(dn2); y = o Wo^T + bo + x
    k_ft_ln_bwd<kFtD><<<(unsigned)div_up(n, 4), kFtThreads, 0, st>>>(dn, y, saved + S.stat2, w[IMF_FT_LN2_G], dz, dy, n);
    if (g[IMF_FT_WO]) ft_tn_launch(dy, kFtD, kFtD, o, kFtQ, kFtQ, n, W.cm_n, nullptr, 1, meta, part, g[IMF_FT_WO], 0, kFtQ, st);
    if (g[IMF_FT_BO]) ft_colsum_launch(dy, nullptr, nullptr, n, kFtD, colpart, g[IMF_FT_BO], nullptr, st);
  }
  if (need_do) {
    ft_rows_launch<false>(ft_rows_args(dy, kFtD, w[IMF_FT_WO], kFtQ, dO, kFtQ, kFtQ, kFtD, n), st);
    // o = p v: dv_b = p^T dO over the item's rows, dp = dO v_b^T
    if (need_kv)
      ft_tn_launch(P, kFtLdP, T, dO, kFtQ, kFtQ, n, W.cm_n, item_starts, n_items, meta, part, dkv + kFtQ, kv_item, 2 * kFtQ, st);
    {
      FtRows p = ft_rows_args(dO, kFtQ, kv + kFtQ, 2 * kFtQ, dP, kFtLdP, T, kFtQ, n);
      ft_items(p, item_starts, n_items, meta, kv_item);
      ft_rows_launch<true>(p, st);
    }
    k_ft_softmax_bwd<<<(unsigned)div_up(n, 4), kFtThreads, 0, st>>>(P, dP, n, T, 0.08838834764831845f);
    // sim = q k^T: dk_b = ds^T q over the item's rows, dq = ds k_b
    if (need_kv)
      ft_tn_launch(dP, kFtLdP, T, q, kFtQ, kFtQ, n, W.cm_n, item_starts, n_items, meta, part, dkv, kv_item, 2 * kFtQ, st);
  }
  if (need_q) {
    {
      FtRows p = ft_rows_args(dP, kFtLdP, kv, 2 * kFtQ, dq, kFtQ, kFtQ, Tp, n);
      p.Kb = T;
      ft_items(p, item_starts, n_items, meta, kv_item);
      ft_rows_launch<false>(p, st);
    }
    if (g[IMF_FT_WQ]) ft_tn_launch(dq, kFtQ, kFtQ, n1, kFtD, kFtD, n, W.cm_n, nullptr, 1, meta, part, g[IMF_FT_WQ], 0, kFtD, st);
    if (need_dn1) {
      ft_rows_launch<false>(ft_rows_args(dq, kFtQ, w[IMF_FT_WQ], kFtD, dn, kFtD, kFtD, kFtQ, n), st);
      if (g[IMF_FT_LN1_G] || g[IMF_FT_LN1_B])
        ft_colsum_launch(dn, x, saved + S.stat1, n, kFtD, colpart, g[IMF_FT_LN1_B], g[IMF_FT_LN1_G], st);
      if (dx) k_ft_ln_bwd<kFtD><<<(unsigned)div_up(n, 4), kFtThreads, 0, st>>>(dn, x, saved + S.stat1, w[IMF_FT_LN1_G], dy, dx, n);
    }
  }
  if (need_kv) {
    // kv = LNc(tok) Wkv^T
    if (g[IMF_FT_WKV])
      ft_tn_launch(dkv, 2 * kFtQ, 2 * kFtQ, c, kFtC, kFtC, BT, W.cm_bt, nullptr, 1, meta, part, g[IMF_FT_WKV], 0, kFtC, st);
    if (dtokens || g[IMF_FT_LNC_G] || g[IMF_FT_LNC_B]) {
      ft_rows_launch<false>(ft_rows_args(dkv, 2 * kFtQ, w[IMF_FT_WKV], kFtC, dc, kFtC, kFtC, 2 * kFtQ, BT), st);
      if (g[IMF_FT_LNC_G] || g[IMF_FT_LNC_B])
        ft_colsum_launch(dc, tokens, saved + S.statc, BT, kFtC, colpart, g[IMF_FT_LNC_B], g[IMF_FT_LNC_G], st);
      if (dtokens)
        k_ft_ln_bwd<kFtC><<<(unsigned)div_up(BT, 4), kFtThreads, 0, st>>>(dc, tokens, saved + S.statc, w[IMF_FT_LNC_G], nullptr, dtokens, BT);
    }
  }
  IMF_CHECK_LAUNCH("imf_fusion_train_backward");
  return IMF_OK;
}

}  // extern "C"
