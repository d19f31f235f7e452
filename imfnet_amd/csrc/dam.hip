// Descriptor Activation Mapping (pytorch_dam/base_dam.py:120-173, pytorch_dam/dam.py:15-21; colouring:
// pytorch_dam/utils/image.py:111-162): for a target row t, how much every voxel's activation in `final` supports that
// row's descriptor.  The reference runs 32 backward passes through the whole network per target and reads only
// final.kernel.grad; `final` is a 1x1x1 convolution followed by a row-wise L2 normalisation and the "loss" is one
// component of one row, so that gradient is an outer product known in closed form:
//   o = h K + b  [n, 32],  r = |o[t]|,  f = o[t] / r,  a_j = 32 - j (the accumulating .grad) or 1 (accumulate == 0)
//   s_c = (a_c - f_c * sum_j a_j f_j) / r,   w_c = mean_k(h[t, k]) * s_c,   heat[n] = max(0, sum_c w_c o[n, c]).
// T targets over n rows in three launches, no autograd, no host loop, no atomics:
//   k_dam_weights  one wavefront per target: r, f, sum a_j f_j, mean(h[t]) as fp64 sums in a fixed order (channels
//                  ascending; the hidden row as 32 strided partial sums, each ascending, added in lane order), w rounded
//                  ONCE to fp32 into weights[T, 32].  A target outside [0, n), r == 0 or a non-finite r sets flags[t] = 1
//                  and w = 0: that target's heat is all zeros.
//   k_dam_heat     one thread per row keeps o[n, 0:32] in registers and walks a tile of kDamTargetTile targets.  The
//                  index of w is the loop counter, the same in every lane, so w arrives by wave-uniform loads through the
//                  constant cache into SGPRs (loads only) and costs no vector memory traffic; 32 fp32 FMAs over ascending
//                  c per target; the 64 lanes of a wavefront store 256 contiguous bytes of heat[t, :].
//   k_dam_minmax   one workgroup per target reads its heat row back and reduces min and max: min and max are
//                  order-free, so two calls give the same bits.
// This is deliberately VALU work.  At K = 32 the launch is bound by the [T, n] store (51 MB for 256 targets x 50 k
// rows against 6.4 MB of inputs and 0.4 GFLOP): the matrix pipe would buy nothing, and its accumulator layout would put
// 4 rows x 16 targets in a lane, which stores 64-byte segments instead of 256-byte ones.
// ROUNDINGS -- the test bound 40 * 2^-24 * sum_c |w_c| |o[n, c]|: one rounding of w (1 unit) and the 32-term FMA chain
// (gamma_32, to first order 32 units); the fp64 phase contributes ~100 * 2^-53.  7 units of margin.
#include <math.h>

#include "common.h"

namespace imf {

constexpr int kDamOut = 32;            // width of `final`: the closed form's a_j = 32 - j is tied to it
constexpr int kDamThreads = 256;
constexpr int kDamTargetTile = 64;     // targets per workgroup of k_dam_heat: o is re-read once per tile (128 B per 256 B stored)

__device__ __forceinline__ long long dam_rows(long long n, const int32_t *n_dev) {
  if (n_dev) {
    const long long nd = *n_dev;
    n = nd < n ? (nd < 0 ? 0 : nd) : n;
  }
  return n;
}

__global__ void __launch_bounds__(64)
k_dam_weights(const float *__restrict__ out, long long n, const int32_t *__restrict__ n_dev,
              const float *__restrict__ hidden, int c_hid, const int32_t *__restrict__ targets, int accumulate,
              float *__restrict__ weights, int32_t *__restrict__ flags) {
  __shared__ double so[kDamOut], sh[kDamOut], sc[3];
  __shared__ int sbad;
  const int t = blockIdx.x, lane = threadIdx.x;
  const long long rows = dam_rows(n, n_dev);
  const long long tg = targets[t];
  const bool inside = tg >= 0 && tg < rows;
  if (lane < kDamOut) {
    so[lane] = inside ? (double)out[tg * kDamOut + lane] : 0.0;
    double s = 0.0;
    if (inside)
      for (int k = lane; k < c_hid; k += kDamOut) s += (double)hidden[tg * c_hid + k];
    sh[lane] = s;
  }
  __syncthreads();
  if (lane == 0) {
    double r2 = 0.0, hs = 0.0;
#pragma unroll 1
    for (int c = 0; c < kDamOut; ++c) r2 += so[c] * so[c];
#pragma unroll 1
    for (int c = 0; c < kDamOut; ++c) hs += sh[c];
    const double r = sqrt(r2);
    const bool bad = !inside || !(r > 0.0 && r < (double)INFINITY);
    double dot = 0.0;                                                  // sum_j a_j f_j
    if (!bad)
#pragma unroll 1
      for (int c = 0; c < kDamOut; ++c) dot += (accumulate ? (double)(kDamOut - c) : 1.0) * (so[c] / r);
    sc[0] = r; sc[1] = dot; sc[2] = hs / (double)c_hid;
    sbad = bad;
    flags[t] = bad ? 1 : 0;
  }
  __syncthreads();
  if (lane < kDamOut) {
    float w = 0.f;
    if (!sbad) {
      const double r = sc[0], a = accumulate ? (double)(kDamOut - lane) : 1.0;
      w = (float)(sc[2] * ((a - (so[lane] / r) * sc[1]) / r));
    }
    weights[(long long)t * kDamOut + lane] = w;
  }
}

__global__ void __launch_bounds__(kDamThreads)
k_dam_heat(const float *__restrict__ out, long long n, const int32_t *__restrict__ n_dev,
           const float *__restrict__ weights, int T, float *__restrict__ heat) {
  const long long rows = dam_rows(n, n_dev);
  const long long row = (long long)blockIdx.x * kDamThreads + threadIdx.x;
  if (row >= rows) return;
  float o[kDamOut];
  const float4 *src = reinterpret_cast<const float4 *>(out + row * kDamOut);
#pragma unroll
  for (int q = 0; q < kDamOut / 4; ++q) {
    const float4 v = src[q];
    o[4 * q] = v.x; o[4 * q + 1] = v.y; o[4 * q + 2] = v.z; o[4 * q + 3] = v.w;
  }
  const int t0 = blockIdx.y * kDamTargetTile;
  const int t1 = t0 + kDamTargetTile < T ? t0 + kDamTargetTile : T;
  // the next target's w is requested before the current one's FMAs: the constant-cache latency hides behind them
  float wn[kDamOut];
  if (t0 < t1) {
#pragma unroll
    for (int c = 0; c < kDamOut; ++c) wn[c] = weights[(long long)t0 * kDamOut + c];   // the same address in every lane
  }
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    float w[kDamOut];
#pragma unroll
    for (int c = 0; c < kDamOut; ++c) w[c] = wn[c];
    if (t + 1 < t1) {
#pragma unroll
      for (int c = 0; c < kDamOut; ++c) wn[c] = weights[(long long)(t + 1) * kDamOut + c];
    }
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < kDamOut; ++c) acc = fmaf(w[c], o[c], acc);
    heat[(long long)t * n + row] = acc > 0.f ? acc : 0.f;               // NaN and -0 become +0
  }
}

// Heat is never negative and never NaN, so the order of the values is the order of their bit patterns.
__global__ void __launch_bounds__(kDamThreads)
k_dam_minmax(const float *__restrict__ heat, long long n, const int32_t *__restrict__ n_dev, float *__restrict__ minmax) {
  __shared__ uint32_t slo[kDamThreads], shi[kDamThreads];
  const long long rows = dam_rows(n, n_dev);
  const float *__restrict__ src = heat + (long long)blockIdx.x * n;
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
  for (long long i = threadIdx.x; i < rows; i += kDamThreads) {
    const uint32_t b = __float_as_uint(src[i]);
    lo = b < lo ? b : lo;
    hi = b > hi ? b : hi;
  }
  slo[threadIdx.x] = lo;
  shi[threadIdx.x] = hi;
  __syncthreads();
  for (int s = kDamThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const uint32_t a = slo[threadIdx.x + s], b = shi[threadIdx.x + s];
      if (a < slo[threadIdx.x]) slo[threadIdx.x] = a;
      if (b > shi[threadIdx.x]) shi[threadIdx.x] = b;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    minmax[2 * blockIdx.x] = rows > 0 ? __uint_as_float(slo[0]) : 0.f;
    minmax[2 * blockIdx.x + 1] = __uint_as_float(shi[0]);
  }
}

}  // namespace imf

using namespace imf;

extern "C" {

int imf_dam_heat(const float *out_prenorm, int64_t n, const int32_t *n_dev, const float *hidden, int c_hid, int c_out,
                 const int32_t *targets, int T, int accumulate, float *weights, float *heat, float *minmax,
                 int32_t *flags, void *stream) {
  IMF_REQUIRE(n >= 0 && T >= 0 && c_hid > 0 && c_out > 0, "imf_dam_heat: n=%lld T=%d c_hid=%d c_out=%d", (long long)n, T,
              c_hid, c_out);
  if (c_out != kDamOut || c_hid % 32 != 0) {
    set_error("imf_dam_heat: c_out=%d c_hid=%d (c_out must be 32, c_hid a positive multiple of 32)", c_out, c_hid);
    return IMF_EUNSUPPORTED;
  }
  if (T == 0) return IMF_OK;
  IMF_REQUIRE(targets && weights && minmax && flags && (n == 0 || (out_prenorm && hidden && heat)),
              "imf_dam_heat: null pointer");
  IMF_REQUIRE(aligned16(out_prenorm), "imf_dam_heat: out_prenorm must be 16-byte aligned");
  const int64_t row_blocks = div_up(n, kDamThreads), tiles = div_up(T, kDamTargetTile);
  IMF_REQUIRE(row_blocks <= 2147483647LL && tiles <= 65535, "imf_dam_heat: too many rows or targets");
  hipStream_t st = (hipStream_t)stream;
  k_dam_weights<<<T, 64, 0, st>>>(out_prenorm, n, n_dev, hidden, c_hid, targets, accumulate, weights, flags);
  if (n > 0)
    k_dam_heat<<<dim3((unsigned)row_blocks, (unsigned)tiles, 1), kDamThreads, 0, st>>>(out_prenorm, n, n_dev, weights, T, heat);
  k_dam_minmax<<<T, kDamThreads, 0, st>>>(heat, n, n_dev, minmax);
  IMF_CHECK_LAUNCH("k_dam_heat");
  return IMF_OK;
}

}  // extern "C"
