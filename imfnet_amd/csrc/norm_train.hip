// Training-mode BatchNorm of the sparse path (ME.MinkowskiBatchNorm = nn.BatchNorm1d over the rows of a batched sparse
// tensor), forward and backward, with the ReLU and the residual add that follow it in the residual block folded in.
// Features are row-major fp32 [N, C], any C >= 1.
//
// Statistics are fp64 sums in a fixed order, no floating-point atomics:
//   * rows are cut into chunks of kBnChunkRows; the cut depends on N only, never on the grid or the CU count;
//   * one workgroup owns a (chunk, tile of <= 256 channels) cell.  Thread (row lane l, column group g) adds its rows
//     l, l + L, l + 2L, ... of the chunk in ascending order, the L row lanes are then added in lane order through LDS;
//   * a one-workgroup finalize adds the chunk partials in chunk order.
// The forward sums d = x - p and d^2 about the per-channel pivot p = x[0][c] (exact in fp64 for fp32 operands that are
// within 2^29 of each other): mean = (sum d + N p) / N, var = (sum d^2 - (sum d)^2 / N) / N.  On integer data every sum
// is an exact integer and the mean is one correctly rounded division.  What the pivot leaves of the textbook
// cancellation is ((p - mean) / sigma)^2 * N * 2^-53 relative in var: a first row within 10 sigma of the channel's mean
// and N = 10^6 give 1e-8, a tenth of an fp32 ulp of rstd; a first row that is an outlier by k sigma costs k^2 of it.
//
// ROUNDINGS, forward (imf_bn_train_forward), per element -- the test bound k = 4:
//   xh = fp32((double(x) - mean) * rstd)      1 rounding, on |xh|; no |mean| / sigma term: the centring is fp64
//   t  = fmaf(xh, gamma, beta)                1 rounding, on |gamma xh + beta| <= |gamma xh| + |beta|
//   y  = t + residual                         1 rounding, on |y| (only with a residual)
//   ReLU                                      exact
//   |y - y_ref| <= 2^-24 (3 |gamma xh| + 2 |beta| + |residual|) to first order; the fourth unit covers the second-order
//   terms and what fp64 carries (the two sums' own rounding, N 2^-53 relative to sum |d|, and the division, square root
//   and product behind mean and rstd).  k = 4.
// ROUNDINGS, backward (imf_bn_train_backward) -- the test bound k' = 2:
//   everything up to the store is fp64: g = dy or 0 (mask y > 0), xh = (double(x) - mean) * rstd unrounded,
//   dbeta = sum g, dgamma = sum g xh, dx = gamma rstd (g - dbeta / N - xh dgamma / N).  Each fp32 output is ONE rounding
//   of an fp64 value: dx on |dx| <= |gamma| rstd (|g| + |dbeta| / N + |xh dgamma| / N), dgamma on |dgamma| <= sum |g xh|,
//   dbeta on |sum g| (exact on integer data).  The second unit covers what fp64 carries.  dresidual = g, a copy.
//
// Rows are read and written as 16-byte vectors when C % 4 == 0 and every pointer is 16-byte aligned, else as scalars.
//
// The second half of the file is the InstanceNorm of the ResUNetIN2* residual blocks (imf_in_forward / imf_in_backward):
// the same cells, sums and roundings with the statistics cut per batch item over a device-side partition of the rows.
// Its forward bound has one more term, for the fp64 statistics' own rounding times rstd (eps = 1e-8 lets rstd reach
// 1e4): include/imfnet_hip.h states it.
#include "common.h"

namespace imf {

constexpr int kBnChunkRows = 128;    // rows per chunk: part of the summation order, hence of the results' last bits
constexpr int kBnThreads = 256;
constexpr int kBnTileGroups = 64;    // column groups (of VEC channels) per workgroup

template <int VEC> __device__ __forceinline__ void bn_load(const float *p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

template <int VEC> __device__ __forceinline__ void bn_store(float *p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *p = v[0];
  }
}

// Where a thread works: column group `g` (channels g * VEC ..), rows r0 + lane, r0 + lane + lanes, ... below r1.
struct BnCell {
  int width, lanes, col, lane, group;
  long long r0, r1;
  bool active;
};

template <int VEC> __device__ __forceinline__ BnCell bn_cell(long long n, int c) {
  BnCell q;
  const int groups = c / VEC;
  q.width = groups < kBnTileGroups ? groups : kBnTileGroups;
  q.lanes = kBnThreads / q.width;
  q.col = threadIdx.x % q.width;
  q.lane = threadIdx.x / q.width;
  q.group = blockIdx.y * q.width + q.col;
  q.r0 = (long long)blockIdx.x * kBnChunkRows;
  q.r1 = q.r0 + kBnChunkRows < n ? q.r0 + kBnChunkRows : n;
  q.active = q.lane < q.lanes && q.group < groups;
  return q;
}

// The workgroup's two per-channel sums of one chunk: row lanes added in lane order, written to partial[chunk][which][C].
template <int VEC>
__device__ __forceinline__ void bn_block_sums(const BnCell &q, const double (&s1)[VEC], const double (&s2)[VEC], int c,
                                              double *__restrict__ partial, double *sm /* [2][kBnThreads * VEC] */) {
  const int nv = q.width * VEC;                      // channels of this tile
  if (q.lane < q.lanes) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      sm[q.lane * nv + q.col * VEC + j] = s1[j];
      sm[kBnThreads * VEC + q.lane * nv + q.col * VEC + j] = s2[j];
    }
  }
  __syncthreads();
  for (int v = threadIdx.x; v < 2 * nv; v += kBnThreads) {
    const int which = v / nv, cv = v - which * nv;
    const int ch = blockIdx.y * nv + cv;
    if (ch >= c) continue;
    const double *src = sm + which * (kBnThreads * VEC) + cv;
    double s = 0.0;
    for (int l = 0; l < q.lanes; ++l) s += src[l * nv];
    partial[((long long)blockIdx.x * 2 + which) * c + ch] = s;
  }
}

template <int VEC>
__global__ void __launch_bounds__(kBnThreads)
k_bn_stats(const float *__restrict__ x, long long n, int c, double *__restrict__ partial) {
  __shared__ double sm[2 * kBnThreads * VEC];
  const BnCell q = bn_cell<VEC>(n, c);
  double s1[VEC], s2[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s1[j] = s2[j] = 0.0;
  if (q.active) {
    float p[VEC];
    bn_load<VEC>(x + (long long)q.group * VEC, p);                       // the pivot: row 0
#pragma unroll 4
    for (long long r = q.r0 + q.lane; r < q.r1; r += q.lanes) {
      float v[VEC];
      bn_load<VEC>(x + r * c + (long long)q.group * VEC, v);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const double d = (double)v[j] - (double)p[j];
        s1[j] += d;
        s2[j] = fma(d, d, s2[j]);
      }
    }
  }
  bn_block_sums<VEC>(q, s1, s2, c, partial, sm);
}

// One workgroup: chunk partials in chunk order -> stats = (mean [C], rstd [C]) and the running statistics.
__global__ void __launch_bounds__(kBnThreads)
k_bn_finalize(const double *__restrict__ partial, long long chunks, const float *__restrict__ x, long long n, int c,
              double eps, double *__restrict__ stats, float *__restrict__ running_mean, float *__restrict__ running_var,
              double momentum) {
  for (int ch = threadIdx.x; ch < c; ch += kBnThreads) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
    for (long long k = 0; k < chunks; ++k) {
      s1 += partial[(k * 2) * c + ch];
      s2 += partial[(k * 2 + 1) * c + ch];
    }
    const double dn = (double)n;
    const double mean = (s1 + dn * (double)x[ch]) / dn;
    double var = (s2 - s1 * s1 / dn) / dn;
    if (var < 0.0) var = 0.0;
    stats[ch] = mean;
    stats[c + ch] = 1.0 / sqrt(var + eps);
    if (running_mean) running_mean[ch] = (float)((1.0 - momentum) * (double)running_mean[ch] + momentum * mean);
    if (running_var)
      running_var[ch] = (float)((1.0 - momentum) * (double)running_var[ch] + momentum * (var * dn / (dn - 1.0)));
  }
}

template <int VEC>
__global__ void __launch_bounds__(kBnThreads)
k_bn_apply(const float *__restrict__ x, long long n, int c, const double *__restrict__ stats,
           const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ residual, int relu,
           float *__restrict__ y) {
  const BnCell q = bn_cell<VEC>(n, c);
  if (!q.active) return;
  const long long c0 = (long long)q.group * VEC;
  double mean[VEC], rstd[VEC];
  float ga[VEC], be[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    mean[j] = stats[c0 + j];
    rstd[j] = stats[c + c0 + j];
  }
  bn_load<VEC>(gamma + c0, ga);
  bn_load<VEC>(beta + c0, be);
#pragma unroll 4
  for (long long r = q.r0 + q.lane; r < q.r1; r += q.lanes) {
    float v[VEC], res[VEC], o[VEC];
    bn_load<VEC>(x + r * c + c0, v);
    if (residual) bn_load<VEC>(residual + r * c + c0, res);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float xh = (float)(((double)v[j] - mean[j]) * rstd[j]);
      float t = fmaf(xh, ga[j], be[j]);
      if (residual) t = t + res[j];
      if (relu) t = t > 0.f ? t : (t == t ? 0.f : t);
      o[j] = t;
    }
    bn_store<VEC>(y + r * c + c0, o);
  }
}

// Backward, pass 1: g = masked dy (stored as dresidual when wanted), chunk sums of g and g * xh.
template <int VEC>
__global__ void __launch_bounds__(kBnThreads)
k_bn_bwd_sums(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ y /* NULL: no mask */,
              long long n, int c, const double *__restrict__ stats, float *__restrict__ dres, double *__restrict__ partial) {
  __shared__ double sm[2 * kBnThreads * VEC];
  const BnCell q = bn_cell<VEC>(n, c);
  double s1[VEC], s2[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s1[j] = s2[j] = 0.0;
  if (q.active) {
    const long long c0 = (long long)q.group * VEC;
    double mean[VEC], rstd[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      mean[j] = stats[c0 + j];
      rstd[j] = stats[c + c0 + j];
    }
#pragma unroll 4
    for (long long r = q.r0 + q.lane; r < q.r1; r += q.lanes) {
      float g[VEC], v[VEC], m[VEC];
      bn_load<VEC>(dy + r * c + c0, g);
      bn_load<VEC>(x + r * c + c0, v);
      if (y) {
        bn_load<VEC>(y + r * c + c0, m);
#pragma unroll
        for (int j = 0; j < VEC; ++j) g[j] = m[j] > 0.f ? g[j] : 0.f;
      }
      if (dres) bn_store<VEC>(dres + r * c + c0, g);
      if (partial) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const double xh = ((double)v[j] - mean[j]) * rstd[j];
          s1[j] += (double)g[j];
          s2[j] = fma((double)g[j], xh, s2[j]);
        }
      }
    }
  }
  if (partial) bn_block_sums<VEC>(q, s1, s2, c, partial, sm);
}

// One workgroup: chunk partials in chunk order -> sums = (dbeta [C], dgamma [C]) in fp64, and their fp32 roundings.
__global__ void __launch_bounds__(kBnThreads)
k_bn_bwd_finalize(const double *__restrict__ partial, long long chunks, int c, double *__restrict__ sums,
                  float *__restrict__ dgamma, float *__restrict__ dbeta) {
  for (int ch = threadIdx.x; ch < c; ch += kBnThreads) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
    for (long long k = 0; k < chunks; ++k) {
      s1 += partial[(k * 2) * c + ch];
      s2 += partial[(k * 2 + 1) * c + ch];
    }
    sums[ch] = s1;
    sums[c + ch] = s2;
    if (dbeta) dbeta[ch] = (float)s1;
    if (dgamma) dgamma[ch] = (float)s2;
  }
}

// Backward, pass 2: dx = gamma rstd (g - dbeta / N - xh dgamma / N), fp64 up to the store.
template <int VEC>
__global__ void __launch_bounds__(kBnThreads)
k_bn_bwd_dx(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ y, long long n, int c,
            const double *__restrict__ stats, const float *__restrict__ gamma, const double *__restrict__ sums,
            float *__restrict__ dx) {
  const BnCell q = bn_cell<VEC>(n, c);
  if (!q.active) return;
  const long long c0 = (long long)q.group * VEC;
  double mean[VEC], rstd[VEC], a[VEC], b[VEC], d[VEC];
  float ga[VEC];
  bn_load<VEC>(gamma + c0, ga);
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    mean[j] = stats[c0 + j];
    rstd[j] = stats[c + c0 + j];
    a[j] = (double)ga[j] * rstd[j];
    b[j] = sums[c0 + j] / (double)n;
    d[j] = sums[c + c0 + j] / (double)n;
  }
#pragma unroll 4
  for (long long r = q.r0 + q.lane; r < q.r1; r += q.lanes) {
    float g[VEC], v[VEC], m[VEC], o[VEC];
    bn_load<VEC>(dy + r * c + c0, g);
    bn_load<VEC>(x + r * c + c0, v);
    if (y) {
      bn_load<VEC>(y + r * c + c0, m);
#pragma unroll
      for (int j = 0; j < VEC; ++j) g[j] = m[j] > 0.f ? g[j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const double xh = ((double)v[j] - mean[j]) * rstd[j];
      o[j] = (float)(a[j] * ((double)g[j] - b[j] - xh * d[j]));
    }
    bn_store<VEC>(dx + r * c + c0, o);
  }
}

static inline dim3 bn_grid(int64_t chunks, int c, int vec) {
  const int groups = c / vec;
  const int width = groups < kBnTileGroups ? groups : kBnTileGroups;
  return dim3((unsigned)chunks, (unsigned)div_up(groups, width), 1);
}

static inline size_t bn_partial_bytes(int64_t n, int c) {
  return (size_t)div_up(n, kBnChunkRows) * 2 * (size_t)c * sizeof(double);
}

// ---- InstanceNorm: the same kernels with the statistics cut per batch item ---------------------------------------------
// Item b owns rows [starts[b], starts[b + 1]) of the device array `starts`; nothing on the host ever reads it.  An item
// is cut into chunks of kBnChunkRows rows counted from ITS first row, and workgroup `slot` of the grid owns the slot-th
// chunk when the items' chunks are numbered item after item.  The items have at most ceil(n / R) + n_items chunks
// between them, so the grid has that many slots and the ones past the last chunk leave at once.  partial[slot] holds
// a chunk's two sums; one workgroup per item adds that item's slots in slot order.  What item b's rows receive thus
// depends on item b's rows alone -- not on the item's place in the batch, the other items, the grid or the CU count.
// The values of `starts` are made non-decreasing and clamped to [0, n] as they are read, so that no content of the
// array can send a row index or a slot out of bounds.

struct InItem {
  long long first, rows, slot0, chunks;     // first row, row count, first slot, slot count
};

__device__ __forceinline__ long long in_clamp(long long v, long long lo, long long hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// Item b's rows and slots, b < n_items: walks the items before it (n_items <= 8).
__device__ __forceinline__ InItem in_item(const int32_t *__restrict__ starts, int b, long long n) {
  InItem it;
  it.first = in_clamp(starts[0], 0, n);
  it.slot0 = 0;
  for (int i = 0;; ++i) {
    it.rows = in_clamp(starts[i + 1], it.first, n) - it.first;
    it.chunks = (it.rows + kBnChunkRows - 1) / kBnChunkRows;
    if (i >= b) return it;
    it.first += it.rows;
    it.slot0 += it.chunks;
  }
}

struct InChunk {
  int item;                                 // -1: a slot past the last chunk
  long long first, rows, r0, r1;            // the item's first row and row count, this chunk's rows [r0, r1)
};

__device__ __forceinline__ InChunk in_chunk(const int32_t *__restrict__ starts, int n_items, long long n, long long slot) {
  InChunk k;
  k.item = -1;
  k.first = k.rows = k.r0 = k.r1 = 0;
  long long a = in_clamp(starts[0], 0, n), s0 = 0;
  for (int b = 0; b < n_items; ++b) {
    const long long e = in_clamp(starts[b + 1], a, n);
    const long long chunks = (e - a + kBnChunkRows - 1) / kBnChunkRows;
    if (slot < s0 + chunks) {
      k.item = b;
      k.first = a;
      k.rows = e - a;
      k.r0 = a + (slot - s0) * kBnChunkRows;
      k.r1 = k.r0 + kBnChunkRows < e ? k.r0 + kBnChunkRows : e;
      return k;
    }
    s0 += chunks;
    a = e;
  }
  return k;
}

template <int VEC> __device__ __forceinline__ BnCell in_cell(const InChunk &k, long long n, int c) {
  BnCell q = bn_cell<VEC>(n, c);
  q.r0 = k.r0;
  q.r1 = k.r1;
  return q;
}

template <int VEC>
__global__ void __launch_bounds__(kBnThreads)
k_in_stats(const float *__restrict__ x, long long n, int c, const int32_t *__restrict__ starts, int n_items,
           double *__restrict__ partial) {
  __shared__ double sm[2 * kBnThreads * VEC];
  const InChunk k = in_chunk(starts, n_items, n, blockIdx.x);
  if (k.item < 0) return;                                                // the whole workgroup: no barrier is skipped
  const BnCell q = in_cell<VEC>(k, n, c);
  double s1[VEC], s2[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s1[j] = s2[j] = 0.0;
  if (q.active) {
    float p[VEC];
    bn_load<VEC>(x + k.first * c + (long long)q.group * VEC, p);         // the pivot: the item's first row
#pragma unroll 4
    for (long long r = q.r0 + q.lane; r < q.r1; r += q.lanes) {
      float v[VEC];
      bn_load<VEC>(x + r * c + (long long)q.group * VEC, v);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const double d = (double)v[j] - (double)p[j];
        s1[j] += d;
        s2[j] = fma(d, d, s2[j]);
      }
    }
  }
  bn_block_sums<VEC>(q, s1, s2, c, partial, sm);
}

// One workgroup per item: its chunk partials in chunk order -> stats[item] = (mean [C], rstd [C]).  An item without
// rows gets (0, 0): nothing reads them.
__global__ void __launch_bounds__(kBnThreads)
k_in_finalize(const double *__restrict__ partial, const float *__restrict__ x, long long n, int c,
              const int32_t *__restrict__ starts, double eps, double *__restrict__ stats) {
  const InItem it = in_item(starts, blockIdx.x, n);
  double *out = stats + (long long)blockIdx.x * 2 * c;
  for (int ch = threadIdx.x; ch < c; ch += kBnThreads) {
    if (it.rows == 0) {
      out[ch] = out[c + ch] = 0.0;
      continue;
    }
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
    for (long long k = it.slot0; k < it.slot0 + it.chunks; ++k) {
      s1 += partial[(k * 2) * c + ch];
      s2 += partial[(k * 2 + 1) * c + ch];
    }
    const double dn = (double)it.rows;
    const double mean = (s1 + dn * (double)x[it.first * c + ch]) / dn;
    double var = (s2 - s1 * s1 / dn) / dn;
    if (var < 0.0) var = 0.0;
    out[ch] = mean;
    out[c + ch] = 1.0 / sqrt(var + eps);
  }
}

template <int VEC>
__global__ void __launch_bounds__(kBnThreads)
k_in_apply(const float *__restrict__ x, long long n, int c, const int32_t *__restrict__ starts, int n_items,
           const double *__restrict__ stats, const float *__restrict__ gamma, const float *__restrict__ beta,
           const float *__restrict__ residual, int relu, float *__restrict__ y) {
  const InChunk k = in_chunk(starts, n_items, n, blockIdx.x);
  if (k.item < 0) return;
  const BnCell q = in_cell<VEC>(k, n, c);
  if (!q.active) return;
  const long long c0 = (long long)q.group * VEC;
  const double *st = stats + (long long)k.item * 2 * c;
  double mean[VEC], rstd[VEC];
  float ga[VEC], be[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    mean[j] = st[c0 + j];
    rstd[j] = st[c + c0 + j];
  }
  bn_load<VEC>(gamma + c0, ga);
  bn_load<VEC>(beta + c0, be);
#pragma unroll 4
  for (long long r = q.r0 + q.lane; r < q.r1; r += q.lanes) {
    float v[VEC], res[VEC], o[VEC];
    bn_load<VEC>(x + r * c + c0, v);
    if (residual) bn_load<VEC>(residual + r * c + c0, res);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float xh = (float)(((double)v[j] - mean[j]) * rstd[j]);
      float t = fmaf(xh, ga[j], be[j]);
      if (residual) t = t + res[j];
      if (relu) t = t > 0.f ? t : (t == t ? 0.f : t);
      o[j] = t;
    }
    bn_store<VEC>(y + r * c + c0, o);
  }
}

// Backward, pass 1: g = masked dy (stored as dresidual when wanted), chunk sums of g and g * xh.
template <int VEC>
__global__ void __launch_bounds__(kBnThreads)
k_in_bwd_sums(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ y /* NULL: no mask */,
              long long n, int c, const int32_t *__restrict__ starts, int n_items, const double *__restrict__ stats,
              float *__restrict__ dres, double *__restrict__ partial) {
  __shared__ double sm[2 * kBnThreads * VEC];
  const InChunk k = in_chunk(starts, n_items, n, blockIdx.x);
  if (k.item < 0) return;
  const BnCell q = in_cell<VEC>(k, n, c);
  double s1[VEC], s2[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s1[j] = s2[j] = 0.0;
  if (q.active) {
    const long long c0 = (long long)q.group * VEC;
    const double *st = stats + (long long)k.item * 2 * c;
    double mean[VEC], rstd[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      mean[j] = st[c0 + j];
      rstd[j] = st[c + c0 + j];
    }
#pragma unroll 4
    for (long long r = q.r0 + q.lane; r < q.r1; r += q.lanes) {
      float g[VEC], v[VEC], m[VEC];
      bn_load<VEC>(dy + r * c + c0, g);
      bn_load<VEC>(x + r * c + c0, v);
      if (y) {
        bn_load<VEC>(y + r * c + c0, m);
#pragma unroll
        for (int j = 0; j < VEC; ++j) g[j] = m[j] > 0.f ? g[j] : 0.f;
      }
      if (dres) bn_store<VEC>(dres + r * c + c0, g);
      if (partial) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const double xh = ((double)v[j] - mean[j]) * rstd[j];
          s1[j] += (double)g[j];
          s2[j] = fma((double)g[j], xh, s2[j]);
        }
      }
    }
  }
  if (partial) bn_block_sums<VEC>(q, s1, s2, c, partial, sm);
}

// One workgroup: per item its chunk partials in chunk order -> sums[item] = (S1 [C], S2 [C]) in fp64; dbeta and dgamma
// are the items' S1 and S2 added in item order, rounded once.
__global__ void __launch_bounds__(kBnThreads)
k_in_bwd_finalize(const double *__restrict__ partial, long long n, int c, const int32_t *__restrict__ starts, int n_items,
                  double *__restrict__ sums, float *__restrict__ dgamma, float *__restrict__ dbeta) {
  for (int ch = threadIdx.x; ch < c; ch += kBnThreads) {
    double t1 = 0.0, t2 = 0.0;
    long long a = in_clamp(starts[0], 0, n), slot = 0;
    for (int b = 0; b < n_items; ++b) {
      const long long e = in_clamp(starts[b + 1], a, n);
      const long long chunks = (e - a + kBnChunkRows - 1) / kBnChunkRows;
      double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
      for (long long k = slot; k < slot + chunks; ++k) {
        s1 += partial[(k * 2) * c + ch];
        s2 += partial[(k * 2 + 1) * c + ch];
      }
      sums[(long long)b * 2 * c + ch] = s1;
      sums[(long long)b * 2 * c + c + ch] = s2;
      t1 += s1;
      t2 += s2;
      slot += chunks;
      a = e;
    }
    if (dbeta) dbeta[ch] = (float)t1;
    if (dgamma) dgamma[ch] = (float)t2;
  }
}

// Backward, pass 2: dx = gamma rstd_b (g - S1_b / n_b - xh S2_b / n_b), fp64 up to the store.
template <int VEC>
__global__ void __launch_bounds__(kBnThreads)
k_in_bwd_dx(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ y, long long n, int c,
            const int32_t *__restrict__ starts, int n_items, const double *__restrict__ stats,
            const float *__restrict__ gamma, const double *__restrict__ sums, float *__restrict__ dx) {
  const InChunk k = in_chunk(starts, n_items, n, blockIdx.x);
  if (k.item < 0) return;
  const BnCell q = in_cell<VEC>(k, n, c);
  if (!q.active) return;
  const long long c0 = (long long)q.group * VEC;
  const double *st = stats + (long long)k.item * 2 * c;
  const double *su = sums + (long long)k.item * 2 * c;
  double mean[VEC], rstd[VEC], a[VEC], b[VEC], d[VEC];
  float ga[VEC];
  bn_load<VEC>(gamma + c0, ga);
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    mean[j] = st[c0 + j];
    rstd[j] = st[c + c0 + j];
    a[j] = (double)ga[j] * rstd[j];
    b[j] = su[c0 + j] / (double)k.rows;
    d[j] = su[c + c0 + j] / (double)k.rows;
  }
#pragma unroll 4
  for (long long r = q.r0 + q.lane; r < q.r1; r += q.lanes) {
    float g[VEC], v[VEC], m[VEC], o[VEC];
    bn_load<VEC>(dy + r * c + c0, g);
    bn_load<VEC>(x + r * c + c0, v);
    if (y) {
      bn_load<VEC>(y + r * c + c0, m);
#pragma unroll
      for (int j = 0; j < VEC; ++j) g[j] = m[j] > 0.f ? g[j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const double xh = ((double)v[j] - mean[j]) * rstd[j];
      o[j] = (float)(a[j] * ((double)g[j] - b[j] - xh * d[j]));
    }
    bn_store<VEC>(dx + r * c + c0, o);
  }
}

static inline int64_t in_slots(int64_t n, int n_items) { return div_up(n, kBnChunkRows) + n_items; }

static inline size_t in_partial_bytes(int64_t n, int c, int n_items) {
  return (size_t)in_slots(n, n_items) * 2 * (size_t)c * sizeof(double);
}

}  // namespace imf

using namespace imf;

extern "C" {

int imf_bn_train_chunk_rows(void) { return kBnChunkRows; }

size_t imf_bn_train_workspace_bytes(int64_t n, int c) {
  if (n < 1 || c < 1) return 0;
  return bn_partial_bytes(n, c) + 2 * (size_t)c * sizeof(double);      // chunk partials, then the backward's two sums
}

int imf_bn_train_forward(const float *x, int64_t n, int c, const float *gamma, const float *beta, double eps,
                         const float *residual, int relu, float *running_mean, float *running_var, double momentum,
                         float *y, double *stats, void *workspace, size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(x && gamma && beta && y && stats && workspace, "imf_bn_train_forward: null pointer");
  IMF_REQUIRE(c >= 1, "imf_bn_train_forward: c=%d", c);
  IMF_REQUIRE(n >= 2, "imf_bn_train_forward: n=%lld (batch statistics need more than one value per channel)", (long long)n);
  IMF_REQUIRE(workspace_bytes >= imf_bn_train_workspace_bytes(n, c), "imf_bn_train_forward: workspace too small");
  IMF_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, "imf_bn_train_forward: fp64 buffers must be 8-byte aligned");
  const int64_t chunks = div_up(n, kBnChunkRows);
  IMF_REQUIRE(chunks <= 2147483647LL && div_up(c, kBnTileGroups) <= 65535, "imf_bn_train_forward: too many rows or channels");
  const bool vec4 = c % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta) &&
                    (!residual || aligned16(residual));
  hipStream_t st = (hipStream_t)stream;
  double *partial = (double *)workspace;
  if (vec4) {
    k_bn_stats<4><<<bn_grid(chunks, c, 4), kBnThreads, 0, st>>>(x, n, c, partial);
  } else {
    k_bn_stats<1><<<bn_grid(chunks, c, 1), kBnThreads, 0, st>>>(x, n, c, partial);
  }
  k_bn_finalize<<<1, kBnThreads, 0, st>>>(partial, chunks, x, n, c, eps, stats, running_mean, running_var, momentum);
  if (vec4) {
    k_bn_apply<4><<<bn_grid(chunks, c, 4), kBnThreads, 0, st>>>(x, n, c, stats, gamma, beta, residual, relu, y);
  } else {
    k_bn_apply<1><<<bn_grid(chunks, c, 1), kBnThreads, 0, st>>>(x, n, c, stats, gamma, beta, residual, relu, y);
  }
  IMF_CHECK_LAUNCH("k_bn_train_forward");
  return IMF_OK;
}

int imf_bn_train_backward(const float *dy, const float *x, const float *y, int relu, const double *stats,
                          const float *gamma, int64_t n, int c, float *dx, float *dgamma, float *dbeta, float *dresidual,
                          void *workspace, size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(dy && x && stats && gamma && workspace, "imf_bn_train_backward: null pointer");
  IMF_REQUIRE(y || !relu, "imf_bn_train_backward: the ReLU mask needs y");
  IMF_REQUIRE(c >= 1, "imf_bn_train_backward: c=%d", c);
  IMF_REQUIRE(n >= 2, "imf_bn_train_backward: n=%lld", (long long)n);
  IMF_REQUIRE(workspace_bytes >= imf_bn_train_workspace_bytes(n, c), "imf_bn_train_backward: workspace too small");
  IMF_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, "imf_bn_train_backward: fp64 buffers must be 8-byte aligned");
  const int64_t chunks = div_up(n, kBnChunkRows);
  IMF_REQUIRE(chunks <= 2147483647LL && div_up(c, kBnTileGroups) <= 65535, "imf_bn_train_backward: too many rows or channels");
  const bool want_sums = dx || dgamma || dbeta;
  if (!want_sums && !dresidual) return IMF_OK;
  const float *mask = relu ? y : nullptr;
  const bool vec4 = c % 4 == 0 && aligned16(dy) && aligned16(x) && aligned16(gamma) && (!mask || aligned16(mask)) &&
                    (!dx || aligned16(dx)) && (!dresidual || aligned16(dresidual));
  hipStream_t st = (hipStream_t)stream;
  double *partial = want_sums ? (double *)workspace : nullptr;
  double *sums = (double *)((char *)workspace + bn_partial_bytes(n, c));
  if (vec4) {
    k_bn_bwd_sums<4><<<bn_grid(chunks, c, 4), kBnThreads, 0, st>>>(dy, x, mask, n, c, stats, dresidual, partial);
  } else {
    k_bn_bwd_sums<1><<<bn_grid(chunks, c, 1), kBnThreads, 0, st>>>(dy, x, mask, n, c, stats, dresidual, partial);
  }
  if (want_sums) k_bn_bwd_finalize<<<1, kBnThreads, 0, st>>>(partial, chunks, c, sums, dgamma, dbeta);
  if (dx) {
    if (vec4) {
      k_bn_bwd_dx<4><<<bn_grid(chunks, c, 4), kBnThreads, 0, st>>>(dy, x, mask, n, c, stats, gamma, sums, dx);
    } else {
      k_bn_bwd_dx<1><<<bn_grid(chunks, c, 1), kBnThreads, 0, st>>>(dy, x, mask, n, c, stats, gamma, sums, dx);
    }
  }
  IMF_CHECK_LAUNCH("k_bn_train_backward");
  return IMF_OK;
}

size_t imf_in_workspace_bytes(int64_t n, int c, int n_items) {
  if (n < 1 || c < 1 || n_items < 1 || n_items > IMF_MAX_BATCH) return 0;
  return in_partial_bytes(n, c, n_items) + (size_t)n_items * 2 * (size_t)c * sizeof(double);   // chunk partials, then the backward's per-item sums
}

int imf_in_forward(const float *x, int64_t n, int c, const int32_t *item_starts, int n_items, const float *gamma,
                   const float *beta, double eps, const float *residual, int relu, float *y, double *stats,
                   void *workspace, size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(x && item_starts && gamma && beta && y && stats && workspace, "imf_in_forward: null pointer");
  IMF_REQUIRE(c >= 1, "imf_in_forward: c=%d", c);
  IMF_REQUIRE(n >= 1 && n <= 2147483647LL, "imf_in_forward: n=%lld", (long long)n);
  IMF_REQUIRE(n_items >= 1 && n_items <= IMF_MAX_BATCH, "imf_in_forward: n_items=%d (1 .. %d)", n_items, IMF_MAX_BATCH);
  IMF_REQUIRE(eps >= 0.0, "imf_in_forward: eps=%g", eps);
  IMF_REQUIRE(workspace_bytes >= imf_in_workspace_bytes(n, c, n_items), "imf_in_forward: workspace too small");
  IMF_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, "imf_in_forward: fp64 buffers must be 8-byte aligned");
  IMF_REQUIRE(((uintptr_t)item_starts & 3) == 0, "imf_in_forward: item_starts must be 4-byte aligned");
  const int64_t slots = in_slots(n, n_items);
  IMF_REQUIRE(div_up(c, kBnTileGroups) <= 65535, "imf_in_forward: too many channels");
  const bool vec4 = c % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(gamma) && aligned16(beta) &&
                    (!residual || aligned16(residual));
  hipStream_t st = (hipStream_t)stream;
  double *partial = (double *)workspace;
  if (vec4) {
    k_in_stats<4><<<bn_grid(slots, c, 4), kBnThreads, 0, st>>>(x, n, c, item_starts, n_items, partial);
  } else {
    k_in_stats<1><<<bn_grid(slots, c, 1), kBnThreads, 0, st>>>(x, n, c, item_starts, n_items, partial);
  }
  k_in_finalize<<<n_items, kBnThreads, 0, st>>>(partial, x, n, c, item_starts, eps, stats);
  if (vec4) {
    k_in_apply<4><<<bn_grid(slots, c, 4), kBnThreads, 0, st>>>(x, n, c, item_starts, n_items, stats, gamma, beta, residual,
                                                               relu, y);
  } else {
    k_in_apply<1><<<bn_grid(slots, c, 1), kBnThreads, 0, st>>>(x, n, c, item_starts, n_items, stats, gamma, beta, residual,
                                                               relu, y);
  }
  IMF_CHECK_LAUNCH("k_in_forward");
  return IMF_OK;
}

int imf_in_backward(const float *dy, const float *x, const float *y, int relu, const double *stats, const float *gamma,
                    const int32_t *item_starts, int64_t n, int c, int n_items, float *dx, float *dgamma, float *dbeta,
                    float *dresidual, void *workspace, size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(dy && x && stats && gamma && item_starts && workspace, "imf_in_backward: null pointer");
  IMF_REQUIRE(y || !relu, "imf_in_backward: the ReLU mask needs y");
  IMF_REQUIRE(c >= 1, "imf_in_backward: c=%d", c);
  IMF_REQUIRE(n >= 1 && n <= 2147483647LL, "imf_in_backward: n=%lld", (long long)n);
  IMF_REQUIRE(n_items >= 1 && n_items <= IMF_MAX_BATCH, "imf_in_backward: n_items=%d (1 .. %d)", n_items, IMF_MAX_BATCH);
  IMF_REQUIRE(workspace_bytes >= imf_in_workspace_bytes(n, c, n_items), "imf_in_backward: workspace too small");
  IMF_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, "imf_in_backward: fp64 buffers must be 8-byte aligned");
  IMF_REQUIRE(((uintptr_t)item_starts & 3) == 0, "imf_in_backward: item_starts must be 4-byte aligned");
  IMF_REQUIRE(div_up(c, kBnTileGroups) <= 65535, "imf_in_backward: too many channels");
  const int64_t slots = in_slots(n, n_items);
  const bool want_sums = dx || dgamma || dbeta;
  if (!want_sums && !dresidual) return IMF_OK;
  const float *mask = relu ? y : nullptr;
  const bool vec4 = c % 4 == 0 && aligned16(dy) && aligned16(x) && aligned16(gamma) && (!mask || aligned16(mask)) &&
                    (!dx || aligned16(dx)) && (!dresidual || aligned16(dresidual));
  hipStream_t st = (hipStream_t)stream;
  double *partial = want_sums ? (double *)workspace : nullptr;
  double *sums = (double *)((char *)workspace + in_partial_bytes(n, c, n_items));
  if (vec4) {
    k_in_bwd_sums<4><<<bn_grid(slots, c, 4), kBnThreads, 0, st>>>(dy, x, mask, n, c, item_starts, n_items, stats, dresidual,
                                                                  partial);
  } else {
    k_in_bwd_sums<1><<<bn_grid(slots, c, 1), kBnThreads, 0, st>>>(dy, x, mask, n, c, item_starts, n_items, stats, dresidual,
                                                                  partial);
  }
  if (want_sums) k_in_bwd_finalize<<<1, kBnThreads, 0, st>>>(partial, n, c, item_starts, n_items, sums, dgamma, dbeta);
  if (dx) {
    if (vec4) {
      k_in_bwd_dx<4><<<bn_grid(slots, c, 4), kBnThreads, 0, st>>>(dy, x, mask, n, c, item_starts, n_items, stats, gamma, sums,
                                                                  dx);
    } else {
      k_in_bwd_dx<1><<<bn_grid(slots, c, 1), kBnThreads, 0, st>>>(dy, x, mask, n, c, item_starts, n_items, stats, gamma, sums,
                                                                  dx);
    }
  }
  IMF_CHECK_LAUNCH("k_in_backward");
  return IMF_OK;
}

}  // extern "C"
