// Coloured ICP: the colour gradient of a target cloud (imf_color_gradient, here) and the joint geometric + photometric fit
// (imf_icp_colored: the third kind of k_icp_corr in icp.hip).
//
// Reference being replaced: nothing upstream calls it; it is the refinement the reconstruction pipeline of Choi, Zhou,
// Koltun 2015 uses as Open3D ships it -- registration_colored_icp / TransformationEstimationForColoredICP (Park, Zhou,
// Koltun, "Colored Point Cloud Registration Revisited", ICCV 2017), restated ([RECALLED] from Open3D like the other ICP
// rules; no Open3D to check against).
//
// Intensity.  I = (r + g + b) / 765 in fp64 from the uint8 colours: the integer sum first, then ONE division, in [0, 1]
// (imfnet_amd.matching.intensity on the host; the kernels read fp64 intensities).
//
// Colour gradient of the target, once per cloud, one row per point.  Point p has the unit normal n, the intensity I_p and
// the neighbour list j_0 .. j_{m-1} imf_estimate_normals wrote for it ((d^2, index) order, the point itself first, padded
// with -1; m = counts[p], entries beyond knn, below 0 or >= n_points are skipped):
//   for every listed neighbour p':  u = (p' - p) - ((p' - p) . n) n   (the offset in the tangent plane),  b = I_p' - I_p;
//     the point's own entry IS included: its row is exactly zero;
//   one constraint row (m - 1) n with right-hand side 0 pins the gradient into the tangent plane;
//   (sum u u^T + (m - 1)^2 n n^T) g = sum u b  by LDL^T without pivoting under the singular rule of icp.hip: a pivot
//     <= 1e-12 times the largest diagonal entry, or NaN, fails, and then g = 0;  m < 4 gives g = 0.
// fp64 throughout, without fused multiply-add (every product and sum rounds on its own, as a NumPy restatement does).  The
// nine sums (six of u u^T, three of u b) are taken over the list positions by the xor butterfly of normals.hip: the order
// depends on the list only.  No floating-point atomics: two calls give the same bits.
//
// The joint fit.  The loop is point-to-plane's (icp.hip): strict d^2 < r^2 correspondences, ties to the lowest original
// target index, fitness and rmse over point distances, T = update . T applied incrementally, the stop rule, 2
// (max_iteration + 1) launches with no host wait.  Per correspondence, with the current source point p (intensity I_s: it
// belongs to the source ROW and does not move with the point), its target q with normal n, gradient g, intensity I_q, and
// lambda = lambda_geometric:
//   geometric:    r_G = (p - q) . n,                      J_G = [p x n, n]
//   photometric:  pt = p - r_G n,  r_I = I_s - (I_q + g . (pt - q)),  M = -g + (n . g) n,  J_I = [p x M, M]
//   sums: count, sum d^2, the 21 upper entries of lambda J_G^T J_G + (1 - lambda) J_I^T J_I and the 6 of
//         lambda J_G r_G + (1 - lambda) J_I r_I
// (rotation first, the parametrisation of the update [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5]; J_I is the derivative of r_I under
// it, which tests/test_colored_icp_host.py checks by central differences).  lambda = 1 forms exactly point-to-plane's sums.
//
// One wavefront per point: lane l holds list position l (knn <= 64) and gathers that neighbour's xyz and intensity; the
// butterfly leaves every sum in every lane; lane 0 solves the 3x3 system and writes the row.
#include "common.h"
#include "registration.h"

namespace imf {
namespace {

constexpr int kGradWaves = 4;           // points per workgroup

__global__ __launch_bounds__(64 * kGradWaves) void k_color_gradient(const double *__restrict__ points,
                                                                    const double *__restrict__ normals,
                                                                    const double *__restrict__ intensity,
                                                                    const int32_t *__restrict__ nbr,
                                                                    const int32_t *__restrict__ counts, int64_t n, int knn,
                                                                    double *__restrict__ out_grad) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kGradWaves + (threadIdx.x >> 6);
  if (i >= n) return;                                    // the whole wavefront
  const int m = min(max(counts[i], 0), knn);
  const V3 p = load3(points, i), nv = load3(normals, i);
  const int j = lane < m ? nbr[i * knn + lane] : -1;
  const bool mine = j >= 0 && j < n;
  double ux = 0.0, uy = 0.0, uz = 0.0, b = 0.0;
  if (mine) {
    const V3 q = load3(points, j);
    const double ex = q.x - p.x, ey = q.y - p.y, ez = q.z - p.z;
    const double d = (ex * nv.x + ey * nv.y) + ez * nv.z;
    ux = ex - d * nv.x;
    uy = ey - d * nv.y;
    uz = ez - d * nv.z;
    b = intensity[j] - intensity[i];
  }
  double A[3][3], rhs[3];
  A[0][0] = wave_sum(ux * ux);
  A[0][1] = wave_sum(ux * uy);
  A[0][2] = wave_sum(ux * uz);
  A[1][1] = wave_sum(uy * uy);
  A[1][2] = wave_sum(uy * uz);
  A[2][2] = wave_sum(uz * uz);
  rhs[0] = wave_sum(ux * b);
  rhs[1] = wave_sum(uy * b);
  rhs[2] = wave_sum(uz * b);
  if (lane != 0) return;
  double gx = 0.0, gy = 0.0, gz = 0.0;
  if (m >= 4) {
    const double w = (double)(m - 1), w2 = w * w;
    A[0][0] = A[0][0] + w2 * (nv.x * nv.x);
    A[0][1] = A[0][1] + w2 * (nv.x * nv.y);
    A[0][2] = A[0][2] + w2 * (nv.x * nv.z);
    A[1][1] = A[1][1] + w2 * (nv.y * nv.y);
    A[1][2] = A[1][2] + w2 * (nv.y * nv.z);
    A[2][2] = A[2][2] + w2 * (nv.z * nv.z);
    // LDL^T without pivoting, written out: A = L D L^T, L unit lower
    const double big = fmax(A[0][0], fmax(A[1][1], A[2][2]));
    const double d0 = A[0][0];
    if (d0 > 1e-12 * big) {                              // zero, negative, tiny or NaN fails
      const double l10 = A[0][1] / d0, l20 = A[0][2] / d0;
      const double d1 = A[1][1] - l10 * l10 * d0;
      if (d1 > 1e-12 * big) {
        const double l21 = (A[1][2] - l20 * l10 * d0) / d1;
        const double d2 = (A[2][2] - l20 * l20 * d0) - l21 * l21 * d1;
        if (d2 > 1e-12 * big) {
          const double y0 = rhs[0], y1 = rhs[1] - l10 * y0, y2 = (rhs[2] - l20 * y0) - l21 * y1;
          gz = y2 / d2;
          gy = y1 / d1 - l21 * gz;
          gx = (y0 / d0 - l10 * gy) - l20 * gz;
        }
      }
    }
  }
  out_grad[3 * i + 0] = gx;
  out_grad[3 * i + 1] = gy;
  out_grad[3 * i + 2] = gz;
}

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

int imf_color_gradient(const double *points, const double *normals, const double *intensity, const int32_t *neighbors,
                       const int32_t *counts, int64_t n, int knn, double *out_grad, void *stream) {
  IMF_REQUIRE(points, "imf_color_gradient: null pointer (points)");
  IMF_REQUIRE(normals, "imf_color_gradient: null pointer (normals)");
  IMF_REQUIRE(intensity, "imf_color_gradient: null pointer (intensity)");
  IMF_REQUIRE(neighbors, "imf_color_gradient: null pointer (neighbors)");
  IMF_REQUIRE(counts, "imf_color_gradient: null pointer (counts)");
  IMF_REQUIRE(out_grad, "imf_color_gradient: null pointer (out_grad)");
  IMF_REQUIRE(n >= 1 && n < (1ll << 30), "imf_color_gradient: n=%lld", (long long)n);
  IMF_REQUIRE(knn >= 1 && knn <= 64, "imf_color_gradient: knn=%d, expected 1..64", knn);
  k_color_gradient<<<(unsigned)div_up(n, kGradWaves), 64 * kGradWaves, 0, (hipStream_t)stream>>>(
      points, normals, intensity, neighbors, counts, n, knn, out_grad);
  IMF_CHECK_LAUNCH("imf_color_gradient");
  return IMF_OK;
}

}  // extern "C"
