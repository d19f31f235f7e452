// The 6x6 information matrix of a registered pair of point clouds (imf_information_matrix): the quantity a 3DMatch
// gt.info record holds, which evaluate.compute_transform_error reads and the pose graph (imfnet_amd/pose_graph.py) weighs
// an edge with.
//
// Reference being restated: Open3D's GetInformationMatrixFromPointClouds(source, target, max_correspondence_distance,
// transformation) ([RECALLED] from memory of Open3D's Registration.cpp; no Open3D to check against, the reference tree
// only ships the resulting gt.info files).  Recalled: the source is transformed, every transformed source point takes its
// nearest target point within the distance, and each correspondence adds G^T G with G built from the TARGET point,
// rotation columns first.  The rules as this file pins them:
//
// Correspondences.  p = T . src[s] (T row-major, applied as k_icp_start applies ICP's init).  They are k_icp_corr's
// (icp.hip, grid_nearest of point_grid.h) and no others: the nearest target point with d^2 < r^2, STRICT; d^2 = dot(e, e)
// = (ex ex + ey ey) + ez ez in fp64, compiled as in icp.hip; equal d^2 go to the lowest ORIGINAL target index; the grid is
// point_grid.h's with cell edge r, ICP's for the same radius; a source row with a NaN (or beyond the key range) has no
// correspondence; a NaN or out-of-range target point raises out_meta[1], as ICP's out_meta[2].
//
// The matrix.  With q = (x, y, z) = dst[j], the target point in the target's frame,
//   G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]],   G (w, v) = w x q + v  (rotation first)
// and Lambda = sum over the correspondences of G^T G.  Ten sums are formed, every addend in the order written and without
// contraction (each product rounded, then the sum of two products rounded):
//   K = sum 1, Sx = sum x, Sy = sum y, Sz = sum z,
//   A00 = sum (y y + z z), A11 = sum (x x + z z), A22 = sum (x x + y y), Pxy = sum x y, Pxz = sum x z, Pyz = sum y z
// and the 21 upper entries are
//   L00 = A00, L01 = 0 - Pxy, L02 = 0 - Pxz, L04 = 0 - Sz, L05 = Sy,
//   L11 = A11, L12 = 0 - Pyz, L13 = Sz, L15 = 0 - Sx,
//   L22 = A22, L23 = 0 - Sy, L24 = Sx,
//   L33 = L44 = L55 = K, every other one +0.0
// mirrored into the lower triangle: exactly symmetric.  (0 - S is the sum of the negated addends bit for bit, except that
// an empty sum stays +0.0.)  out_meta[0] = K as an integer.  An empty correspondence set gives 36 times +0.0 and K = 0.
//
// Summation order.  One thread per source row, so a thread has one addend; the xor butterfly inside each wavefront, the
// four wavefronts in order through LDS (block_sum), one row of ten doubles per block; then ONE workgroup adds the block
// rows: thread t the rows t, t + 256, ... ascending, then the fixed tree of k_icp_fit.  No floating-point atomics, no
// host wait: two calls give the same bytes.
//
// Resources (make resource-usage, gfx950): see DESIGN.md section 17.
#include "common.h"
#include "registration.h"
#include "point_grid.h"

#pragma clang fp contract(off)

namespace imf {
namespace {

constexpr int kInfoThreads = 256;
constexpr int kInfoSums = 10;          // K, Sx, Sy, Sz, A00, A11, A22, Pxy, Pxz, Pyz
constexpr int kInfoSumThreads = 256;

struct InfoT {
  double T[16];                         // row-major 4x4, by value (a host matrix)
};

__global__ __launch_bounds__(kInfoThreads) void k_info_corr(Grid g, const double *__restrict__ src, int64_t n, InfoT T,
                                                            double r2, double *__restrict__ partial) {
  __shared__ double lds4[4];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double v[kInfoSums];
#pragma unroll
  for (int k = 0; k < kInfoSums; ++k) v[k] = 0.0;
  if (i < n) {
    const V3 p = apply(T.T, load3(src, i));
    double d2;
    const int r = grid_nearest(g, p, r2, d2);
    if (r >= 0) {
      const V3 q = load3(g.xyz, r);
      const double xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z;
      v[0] = 1.0;
      v[1] = q.x; v[2] = q.y; v[3] = q.z;
      v[4] = yy + zz; v[5] = xx + zz; v[6] = xx + yy;
      v[7] = q.x * q.y; v[8] = q.x * q.z; v[9] = q.y * q.z;
    }
  }
#pragma unroll
  for (int k = 0; k < kInfoSums; ++k) {
    const double s = block_sum(v[k], lds4);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * kInfoSums + k] = s;
  }
}

// one workgroup: the block rows in k_icp_fit's fixed order, then the 36 entries and the two integers
__global__ __launch_bounds__(kInfoSumThreads) void k_info_sum(const double *__restrict__ partial, int n_blocks,
                                                              const int32_t *__restrict__ err, double *__restrict__ out_info,
                                                              int32_t *__restrict__ out_meta) {
  __shared__ double lds[kInfoSumThreads];
  __shared__ double sums[kInfoSums];
  const int t = threadIdx.x;
  for (int k = 0; k < kInfoSums; ++k) {
    double a = 0.0;
    for (int b = t; b < n_blocks; b += kInfoSumThreads) a += partial[(int64_t)b * kInfoSums + k];   // ascending per thread
    lds[t] = a;
    __syncthreads();
    for (int o = kInfoSumThreads / 2; o > 0; o >>= 1) {   // fixed tree
      if (t < o) lds[t] += lds[t + o];
      __syncthreads();
    }
    if (t == 0) sums[k] = lds[0];
    __syncthreads();
  }
  if (t != 0) return;
  const double K = sums[0], Sx = sums[1], Sy = sums[2], Sz = sums[3];
  double L[6][6];
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) L[a][b] = 0.0;
  L[0][0] = sums[4]; L[0][1] = 0.0 - sums[7]; L[0][2] = 0.0 - sums[8]; L[0][4] = 0.0 - Sz; L[0][5] = Sy;
  L[1][1] = sums[5]; L[1][2] = 0.0 - sums[9]; L[1][3] = Sz;            L[1][5] = 0.0 - Sx;
  L[2][2] = sums[6]; L[2][3] = 0.0 - Sy;      L[2][4] = Sx;
  L[3][3] = K;       L[4][4] = K;             L[5][5] = K;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) out_info[6 * a + b] = out_info[6 * b + a] = L[a][b];
  out_meta[0] = (int32_t)K;
  out_meta[1] = *err;
}

size_t info_workspace_bytes(int64_t n_src, int64_t n_dst) {
  if (n_src <= 0 || n_dst <= 0 || n_src >= (1ll << 30) || n_dst >= (1ll << 30)) return 0;
  return grid_layout(n_dst).total + align256((size_t)div_up(n_src, kInfoThreads) * kInfoSums * 8);
}

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

size_t imf_information_workspace_bytes(int64_t n_src, int64_t n_dst) { return info_workspace_bytes(n_src, n_dst); }

int imf_information_matrix(const double *src, int64_t n_src, const double *dst, int64_t n_dst, const double *T_host,
                           double max_corr_dist, double *out_info, int32_t *out_meta, void *workspace,
                           size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(src && dst && out_info && out_meta && workspace, "imf_information_matrix: null pointer");
  IMF_REQUIRE(n_src >= 1 && n_dst >= 1 && n_src < (1ll << 30) && n_dst < (1ll << 30),
              "imf_information_matrix: n_src=%lld n_dst=%lld", (long long)n_src, (long long)n_dst);
  IMF_REQUIRE(max_corr_dist > 0.0 && max_corr_dist < 1e6, "imf_information_matrix: max_corr_dist=%g", max_corr_dist);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "imf_information_matrix: workspace must be 256-byte aligned");
  IMF_REQUIRE(workspace_bytes >= info_workspace_bytes(n_src, n_dst), "imf_information_matrix: workspace %zu < %zu",
              workspace_bytes, info_workspace_bytes(n_src, n_dst));
  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  Grid g;
  int32_t *err;
  int rc = build_grid(dst, n_dst, max_corr_dist, ws, g, err, st);
  if (rc) return rc;
  double *partial = (double *)(ws + grid_layout(n_dst).total);
  const int nb = (int)div_up(n_src, kInfoThreads);
  InfoT T;
  for (int k = 0; k < 16; ++k) T.T[k] = T_host ? T_host[k] : (k % 5 == 0 ? 1.0 : 0.0);
  k_info_corr<<<(unsigned)nb, kInfoThreads, 0, st>>>(g, src, n_src, T, max_corr_dist * max_corr_dist, partial);
  k_info_sum<<<1, kInfoSumThreads, 0, st>>>(partial, nb, err, out_info, out_meta);
  IMF_CHECK_LAUNCH("imf_information_matrix");
  return IMF_OK;
}

}  // extern "C"
