// Fast Point Feature Histograms of a point cloud with normals (imf_fpfh_features).
//
// Reference being replaced: nothing upstream computes it; it is the hand-crafted descriptor every registration toolkit
// ships (Rusu, Blodow, Beetz 2009; Open3D's compute_fpfh_feature), here so that the registration and evaluation tools run
// without a trained checkpoint.  What is recalled from Open3D's Feature.cpp is marked [RECALLED]; there is no Open3D to
// check against.  The project's own: the neighbour lists are the ones imf_estimate_normals writes (knn smallest (d^2,
// index) within max_radius, Open3D: a hybrid radius / max_nn KD-tree search, the same set where no tie straddles the
// last place), the integer counts as an output, the order of every sum, zero features for a zero-length pair.
//
// Rules the tests pin (tests/fpfh_restate.py, tests/test_gpu_fpfh.py).  All arithmetic is fp64 WITHOUT fused
// multiply-add: every product and sum rounds one by one, in the order written, so a NumPy restatement forms the same bits.
//   - neighbours of point i: the first counts[i] entries of nbr[i] (the rest is padding, -1) in list order, minus every
//     entry equal to i, minus anything outside [0, n) (a corrupt list reads nothing out of bounds).  m_i is their number;
//   - pair features of (i, j) [RECALLED: ComputePairFeatures]: d = p_j - p_i, d2 = (dx*dx + dy*dy) + dz*dz, L = sqrt(d2).
//     L == 0: all three features are 0.  a1 = (n_i . d) / L, a2 = (n_j . d) / L, every dot product (x + y) + z.
//     |a1| < |a2| swaps the roles: n1 = n_j, n2 = n_i, d = -d, f2 = -a2; otherwise n1 = n_i, n2 = n_j, f2 = a1.
//     v = d x n1 (each component a*b - c*d); |v| = sqrt(v . v) == 0: all three features are 0; otherwise v /= |v|.
//     w = n1 x v, f1 = v . n2, f0 = atan2(w . n2, n1 . n2);
//   - bins [RECALLED: 11 per feature, f0 over [-pi, pi], f1 and f2 over [-1, 1]]: b0 = floor(((11 * (f0 + pi)) / (2 pi))),
//     b1 = 11 + floor((11 * (f1 + 1)) * 0.5), b2 = 22 + floor((11 * (f2 + 1)) * 0.5), each clamped to its 11 bins.  Zero
//     features are binned like any other: 5.5, the middle bin;
//   - SPFH: cnt_i[33], the integer number of pairs per bin (out_hist; every row sums to 3 m_i);
//     spfh_i[b] = (double)cnt_i[b] * (100.0 / m_i), zeros when m_i == 0 [RECALLED: the scale 100 / neighbours];
//   - FPFH [RECALLED: the 1 / d2 weight, the renormalisation to 100 per feature, the point's own SPFH added on top]: over
//     the neighbours j of i in list order, skipping d2 == 0, acc[b] += spfh_j[b] / d2, one after the other.  S[g] = the sum
//     of acc[b] over the 11 bins of group g, ascending b.  out[b] = (S[g] != 0 ? acc[b] * (100.0 / S[g]) : 0.0) + spfh_i[b],
//     rounded once to fp32.  Columns 33 .. width - 1 are +0.0f.
// Two kernels, one wavefront per point in both.  k_spfh: lane l owns list entry l and computes its three bins; 33 ballots
// count them, so the histogram is made of integers and has no summation order.  k_fpfh: lane l first fetches d2 and m_j
// of entry l, then lanes 0..32 own a bin and walk the list in order (the 33 counts of a neighbour are one 132-byte read);
// the group sums come lane by lane in ascending bin order.  No atomics at all, no workgroup waits for another: two calls
// give the same bits.
#include "common.h"

#pragma clang fp contract(off)

namespace imf {
namespace {

constexpr int kFpfhWaves = 4;            // points per workgroup
constexpr int kBins = 33;
constexpr double kPi = 3.14159265358979323846;

struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 ld3(const double *p, int64_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ double dot3(D3 a, D3 b) {
  const double xx = a.x * b.x, yy = a.y * b.y, zz = a.z * b.z;
  const double xy = xx + yy;
  return xy + zz;
}
__device__ __forceinline__ double det2(double a, double b, double c, double d) {
  const double ab = a * b, cd = c * d;
  return ab - cd;
}
__device__ __forceinline__ D3 cross3(D3 a, D3 b) {
  return {det2(a.y, b.z, a.z, b.y), det2(a.z, b.x, a.x, b.z), det2(a.x, b.y, a.y, b.x)};
}
__device__ __forceinline__ int bin11(double t) {         // floor, clamped; NaN goes to 0
  return (int)fmin(fmax(floor(t), 0.0), 10.0);
}
__device__ __forceinline__ bool listed(int j, int64_t i, int64_t n) { return j >= 0 && j < n && j != i; }

__global__ __launch_bounds__(64 * kFpfhWaves) void k_spfh(const double *__restrict__ points,
                                                          const double *__restrict__ normals, int64_t n,
                                                          const int32_t *__restrict__ nbr,
                                                          const int32_t *__restrict__ counts, int knn,
                                                          int32_t *__restrict__ cnt, int32_t *__restrict__ m_out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kFpfhWaves + (threadIdx.x >> 6);
  if (i >= n) return;                                    // the whole wavefront
  const int j = lane < min(knn, counts[i]) ? nbr[i * knn + lane] : -1;
  const bool mine = listed(j, i, n);
  int b0 = 0, b1 = 0, b2 = 0;
  if (mine) {
    const D3 pi = ld3(points, i), pj = ld3(points, j), ni = ld3(normals, i), nj = ld3(normals, j);
    D3 d{pj.x - pi.x, pj.y - pi.y, pj.z - pi.z};
    const double len = sqrt(dot3(d, d));
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    if (len != 0.0) {
      const double a1 = dot3(ni, d) / len, a2 = dot3(nj, d) / len;
      const bool swap = fabs(a1) < fabs(a2);
      const D3 n1 = swap ? nj : ni, n2 = swap ? ni : nj;
      if (swap) d = {-d.x, -d.y, -d.z};
      D3 v = cross3(d, n1);
      const double vl = sqrt(dot3(v, v));
      if (vl != 0.0) {
        v = {v.x / vl, v.y / vl, v.z / vl};
        const D3 w = cross3(n1, v);
        f2 = swap ? -a2 : a1;
        f1 = dot3(v, n2);
        f0 = atan2(dot3(w, n2), dot3(n1, n2));
      }
    }
    b0 = bin11((11.0 * (f0 + kPi)) / (2.0 * kPi));
    b1 = 11 + bin11((11.0 * (f1 + 1.0)) * 0.5);
    b2 = 22 + bin11((11.0 * (f2 + 1.0)) * 0.5);
  }
  int c = 0;
  for (int b = 0; b < kBins; ++b) {
    const int hits = __popcll(__ballot(mine && (b0 == b || b1 == b || b2 == b)));
    if (lane == b) c = hits;
  }
  const int m = __popcll(__ballot(mine));
  if (lane < kBins) cnt[i * kBins + lane] = c;
  if (lane == 0) m_out[i] = m;
}

__global__ __launch_bounds__(64 * kFpfhWaves) void k_fpfh(const double *__restrict__ points, int64_t n,
                                                          const int32_t *__restrict__ nbr,
                                                          const int32_t *__restrict__ counts, int knn,
                                                          const int32_t *__restrict__ cnt,
                                                          const int32_t *__restrict__ m_of, int width,
                                                          float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kFpfhWaves + (threadIdx.x >> 6);
  if (i >= n) return;                                    // the whole wavefront
  // lane l: entry l of the list, its d2 and the scale 100 / m_j of its histogram (0: the entry adds nothing)
  int lj = lane < min(knn, counts[i]) ? nbr[i * knn + lane] : -1;
  double ld2 = 0.0, lscale = 0.0;
  if (listed(lj, i, n)) {
    const D3 pi = ld3(points, i), pj = ld3(points, lj);
    const D3 d{pj.x - pi.x, pj.y - pi.y, pj.z - pi.z};
    ld2 = dot3(d, d);
    const int mj = m_of[lj];
    if (mj > 0) lscale = 100.0 / (double)mj;
  }
  if (!(ld2 > 0.0)) lj = -1;                             // skipped: itself, padding, out of range, a duplicate (NaN too)
  const int bin = lane < kBins ? lane : 0;               // lanes 33.. shadow bin 0 and write zeros
  double acc = 0.0;
  for (int e0 = 0; e0 < knn; e0 += 8) {
    int c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                        // 8 neighbours' counts in flight
      const int j = __shfl(lj, (e0 + k) & 63, 64);
      c[k] = (e0 + k < knn && j >= 0) ? cnt[(int64_t)j * kBins + bin] : 0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int j = __shfl(lj, (e0 + k) & 63, 64);
      const double d2 = __shfl(ld2, (e0 + k) & 63, 64), scale = __shfl(lscale, (e0 + k) & 63, 64);
      if (e0 + k < knn && j >= 0) {                      // wave-uniform
        const double s = (double)c[k] * scale;
        acc += s / d2;
      }
    }
  }
  const int g0 = (bin / 11) * 11;
  double sum = 0.0;
  for (int k = 0; k < 11; ++k) sum += __shfl(acc, g0 + k, 64);
  const int mi = m_of[i];
  const double own = mi > 0 ? (double)cnt[i * kBins + bin] * (100.0 / (double)mi) : 0.0;
  const double val = (sum != 0.0 ? acc * (100.0 / sum) : 0.0) + own;
  if (lane < width) out[i * width + lane] = lane < kBins ? (float)val : 0.0f;
}

size_t fpfh_counts_offset(int64_t n) { return align256((size_t)n * sizeof(int32_t)); }

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

size_t imf_fpfh_workspace_bytes(int64_t n, int knn) {
  if (n <= 0 || n >= (1ll << 30) || knn < 1 || knn > 64) return 0;
  return fpfh_counts_offset(n) + align256((size_t)n * kBins * sizeof(int32_t));       // m [n], then cnt [n, 33]
}

int imf_fpfh_features(const double *points, const double *normals, int64_t n, const int32_t *nbr, const int32_t *counts,
                      int knn, int width, float *out, int32_t *out_hist, void *workspace, size_t workspace_bytes,
                      void *stream) {
  IMF_REQUIRE(points && normals && nbr && counts && out && workspace, "imf_fpfh_features: null pointer");
  IMF_REQUIRE(n >= 1 && n < (1ll << 30), "imf_fpfh_features: n=%lld", (long long)n);
  IMF_REQUIRE(knn >= 1 && knn <= 64, "imf_fpfh_features: knn=%d, expected 1..64", knn);
  IMF_REQUIRE(width == 33 || width == 64, "imf_fpfh_features: width=%d, expected 33 or 64", width);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "imf_fpfh_features: workspace must be 256-byte aligned");
  IMF_REQUIRE(workspace_bytes >= imf_fpfh_workspace_bytes(n, knn), "imf_fpfh_features: workspace %zu < %zu",
              workspace_bytes, imf_fpfh_workspace_bytes(n, knn));
  hipStream_t st = (hipStream_t)stream;
  int32_t *m = (int32_t *)workspace;
  int32_t *cnt = out_hist ? out_hist : (int32_t *)((char *)workspace + fpfh_counts_offset(n));
  const unsigned blocks = (unsigned)div_up(n, kFpfhWaves);
  k_spfh<<<blocks, 64 * kFpfhWaves, 0, st>>>(points, normals, n, nbr, counts, knn, cnt, m);
  IMF_CHECK_LAUNCH("imf_fpfh_features");
  k_fpfh<<<blocks, 64 * kFpfhWaves, 0, st>>>(points, n, nbr, counts, knn, cnt, m, width, out);
  IMF_CHECK_LAUNCH("imf_fpfh_features");
  return IMF_OK;
}

}  // extern "C"
