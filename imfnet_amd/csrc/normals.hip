// Exact k-NN PCA normals of a point cloud (imf_estimate_normals).
//
// Reference being replaced: data/fuse_fragments_3DMatch.py:89, `pcd.estimate_normals()` after the TSDF extract, Open3D's
// PointCloud.estimate_normals with its default KDTreeSearchParamKNN(knn=30) ([RECALLED]; no Open3D to check against): the
// normal of point i is the eigenvector of the smallest eigenvalue of the covariance of its knn nearest cloud points, the
// point itself among them (the KNN query of a cloud point returns that point first).  A set of fewer than 3 points gives
// (0, 0, 1), Open3D's fallback ([RECALLED]), unsigned.
// The project's own: the radius cap (max_radius), the covariance in two passes (Open3D: cumulants), the Jacobi solver and
// the sign rules below (Open3D leaves the sign to a separate orient_normals_* call; upstream's fragments get theirs from
// the TSDF gradient).
//
// Rules the tests pin (tests/normals_restate.py, tests/test_gpu_normals.py):
//   - neighbour set of point i: the knn smallest of (d^2, original index), lexicographic, among the points with
//     d^2 <= max_radius^2; d^2 = (ex*ex + ey*ey) + ez*ez of e = q - p in fp64 WITHOUT fused multiply-add (the products
//     and sums round one by one, so a NumPy restatement forms the same bits).  A tie goes to the lowest index, the first of
//     exact duplicates wins.  counts[i] = how many were found, nbr[i] lists them in that order, padded with -1;
//   - the grid: csrc/point_grid.h with the rules of icp.hip (cell formula, 18-bit keys, a point beyond cells
//     [-(2^17 - 1), 2^17 - 2] or NaN raises the error flag and is in nobody's list; as a query it finds nothing).  The cell
//     edge is max_radius / 2.  Shells of cells grow around the query's cell: shell s is the cells at Chebyshev distance s.
//     Every point outside shells 0..s is further than s * edge (the hair in inv_cell covers the rounding of x * inv_cell),
//     so the search stops after shell s when the list is full and its last d^2 <= (s * edge)^2, and after shell 2 at the
//     latest (2 * edge = max_radius): at most 125 cells;
//   - the normal: mean m of the set, then C = sum (p - m)(p - m)^T / count, both summed by one xor butterfly over the list
//     positions (the order depends on the list only).  Cyclic Jacobi on C, pairs (0,1), (0,2), (1,2) per sweep, at most 12
//     sweeps, ended when |c01| + |c02| + |c12| <= 2^-70 (|c00| + |c11| + |c22|); a zero off-diagonal entry is skipped, so
//     exact zeros stay exact.  The column of the smallest diagonal entry (the lowest index on a tie), renormalised;
//   - the sign: with a viewpoint v, n . (v - p) >= 0; without one, the component of the largest magnitude is positive
//     (the first one on a tie).
// One wavefront per query: lane l holds the l-th best (d^2, index) so far.  The cells of a shell are probed by the lanes
// in parallel; the rows of a found cell are read 64 at a time, the candidates that beat the list's last entry are
// inserted one by one (a ballot gives the position, a lane shift makes room).  The final list is the knn smallest of a
// strict total order: it does not depend on the order of the candidates, hence not on the grid's scatter.  No
// floating-point atomics, no workgroup waits for another: two calls give the same bits.
#include "common.h"
#include "registration.h"
#include "point_grid.h"

namespace imf {
namespace {

constexpr int kNormalWaves = 4;         // queries per workgroup
constexpr int kMaxShell = 2;            // cell edge = max_radius / 2
constexpr int kNoIndex = 0x7FFFFFFF;

struct Viewpoint {
  double v[3];
  int use;
};

__device__ __forceinline__ double dist2_unfused(V3 a, V3 b) {
#pragma clang fp contract(off)
  const double ex = a.x - b.x, ey = a.y - b.y, ez = a.z - b.z;
  const double xx = ex * ex, yy = ey * ey, zz = ez * ez;
  const double xy = xx + yy;
  return xy + zz;
}

__device__ __forceinline__ bool before(double d, int i, double d2, int i2) { return d < d2 || (d == d2 && i < i2); }

// eigenvector of the smallest eigenvalue of the symmetric a (overwritten), the rule of the file header
__device__ void smallest_eigenvector(double a[3][3], double n[3]) {
  double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    if (off <= 0x1p-70 * (fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]))) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int r = 0; r < 3; ++r) {                    // A J, V J
          const double arp = a[r][p], arq = a[r][q];
          a[r][p] = c * arp - s * arq;
          a[r][q] = s * arp + c * arq;
          const double vrp = v[r][p], vrq = v[r][q];
          v[r][p] = c * vrp - s * vrq;
          v[r][q] = s * vrp + c * vrq;
        }
        for (int r = 0; r < 3; ++r) {                    // J^T (A J)
          const double apr = a[p][r], aqr = a[q][r];
          a[p][r] = c * apr - s * aqr;
          a[q][r] = s * apr + c * aqr;
        }
        a[p][q] = a[q][p] = 0.0;
      }
  }
  int m = 0;
  if (a[1][1] < a[m][m]) m = 1;
  if (a[2][2] < a[m][m]) m = 2;
  const double len = sqrt(v[0][m] * v[0][m] + v[1][m] * v[1][m] + v[2][m] * v[2][m]);
  for (int r = 0; r < 3; ++r) n[r] = v[r][m] / len;
}

__global__ __launch_bounds__(64 * kNormalWaves) void k_normals(Grid g, const double *__restrict__ points, int64_t n,
                                                               int knn, double edge, double r2, Viewpoint vp,
                                                               double *__restrict__ normals, int32_t *__restrict__ counts,
                                                               int32_t *__restrict__ nbr) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * kNormalWaves + (threadIdx.x >> 6);
  if (i >= n) return;                                    // the whole wavefront
  const V3 p = load3(points, i);
  double ld = INFINITY;                                  // this lane's list entry
  int li = kNoIndex;
  int cx, cy, cz;
  const bool in_grid = cell_of_point(p, g.inv_cell, kCoordLim, cx, cy, cz);
  for (int s = 0; in_grid && s <= kMaxShell; ++s) {
    const int side = 2 * s + 1, cells = side * side * side;
    for (int base = 0; base < cells; base += 64) {
      // every lane probes one cell of the cube; the cells inside it belong to earlier shells
      const int c = base + lane;
      int r0 = 0, rn = 0;
      if (c < cells) {
        const int dx = c % side - s, dy = (c / side) % side - s, dz = c / (side * side) - s;
        const int x = cx + dx, y = cy + dy, z = cz + dz;
        if (max(abs(dx), max(abs(dy), abs(dz))) == s && coord_in_range(x, y, z)) {
          const int slot = hash_find_slot(g.tab, g.capmask, pack_key(0, x, y, z));
          if (slot >= 0) {
            const uint4 v = *reinterpret_cast<const uint4 *>(g.tab + slot);
            r0 = (int)v.z;
            rn = (int)v.w;
          }
        }
      }
      unsigned long long found = __ballot(rn > 0);
      while (found) {
        const int src = __ffsll((long long)found) - 1;
        found &= found - 1;
        const int b0 = __shfl(r0, src, 64), b1 = b0 + __shfl(rn, src, 64);
        for (int rb = b0; rb < b1; rb += 64) {
          const int r = rb + lane;
          double d = INFINITY;
          int id = kNoIndex;
          if (r < b1) {
            d = dist2_unfused(load3(g.xyz, r), p);
            id = g.idx[r];
          }
          const double kd = __shfl(ld, knn - 1, 64);
          const int ki = __shfl(li, knn - 1, 64);
          unsigned long long cand = __ballot(r < b1 && d <= r2 && before(d, id, kd, ki));
          while (cand) {
            const int cl = __ffsll((long long)cand) - 1;
            cand &= cand - 1;
            const double nd = __shfl(d, cl, 64);
            const int ni = __shfl(id, cl, 64);
            const int pos = __popcll(__ballot(before(ld, li, nd, ni)));   // entries that stay in front
            const double ud = __shfl_up(ld, 1, 64);
            const int ui = __shfl_up(li, 1, 64);
            if (lane == pos) { ld = nd; li = ni; }
            else if (lane > pos) { ld = ud; li = ui; }
          }
        }
      }
    }
    const double covered = s * edge;
    const double kd = __shfl(ld, knn - 1, 64);
    if (kd <= covered * covered) break;                  // full, and nothing unseen can come before its last entry
  }
  const bool mine = lane < knn && li != kNoIndex;
  const int count = __popcll(__ballot(mine));
  if (nbr && lane < knn) nbr[i * knn + lane] = mine ? li : -1;
  double nv[3] = {0.0, 0.0, 1.0};
  if (count >= 3) {
    const V3 q = mine ? load3(points, li) : V3{0.0, 0.0, 0.0};
    const double inv = 1.0 / (double)count;
    const V3 m{wave_sum(mine ? q.x : 0.0) * inv, wave_sum(mine ? q.y : 0.0) * inv, wave_sum(mine ? q.z : 0.0) * inv};
    const V3 e = mine ? sub(q, m) : V3{0.0, 0.0, 0.0};
    double a[3][3];
    a[0][0] = wave_sum(e.x * e.x) * inv;
    a[0][1] = a[1][0] = wave_sum(e.x * e.y) * inv;
    a[0][2] = a[2][0] = wave_sum(e.x * e.z) * inv;
    a[1][1] = wave_sum(e.y * e.y) * inv;
    a[1][2] = a[2][1] = wave_sum(e.y * e.z) * inv;
    a[2][2] = wave_sum(e.z * e.z) * inv;
    smallest_eigenvector(a, nv);
    bool flip;
    if (vp.use) {
      flip = nv[0] * (vp.v[0] - p.x) + nv[1] * (vp.v[1] - p.y) + nv[2] * (vp.v[2] - p.z) < 0.0;
    } else {
      int k = 0;
      if (fabs(nv[1]) > fabs(nv[k])) k = 1;
      if (fabs(nv[2]) > fabs(nv[k])) k = 2;
      flip = nv[k] < 0.0;
    }
    if (flip) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
  }
  if (lane == 0) {
    counts[i] = count;
    normals[3 * i + 0] = nv[0];
    normals[3 * i + 1] = nv[1];
    normals[3 * i + 2] = nv[2];
  }
}

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

size_t imf_normals_workspace_bytes(int64_t n) {
  if (n <= 0 || n >= (1ll << 30)) return 0;
  return grid_layout(n).total;
}

int imf_estimate_normals(const double *points, int64_t n, int knn, double max_radius, const double *viewpoint_host,
                         double *normals, int32_t *counts, int32_t *nbr, int32_t *out_err, void *workspace,
                         size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(points && normals && counts && out_err && workspace, "imf_estimate_normals: null pointer");
  IMF_REQUIRE(n >= 1 && n < (1ll << 30), "imf_estimate_normals: n=%lld", (long long)n);
  IMF_REQUIRE(knn >= 1 && knn <= 64, "imf_estimate_normals: knn=%d, expected 1..64", knn);
  IMF_REQUIRE(max_radius > 0.0 && max_radius < 1e6, "imf_estimate_normals: max_radius=%g", max_radius);   // NaN too
  if (viewpoint_host)
    for (int k = 0; k < 3; ++k)
      IMF_REQUIRE(viewpoint_host[k] - viewpoint_host[k] == 0.0, "imf_estimate_normals: viewpoint[%d]=%g", k,
                  viewpoint_host[k]);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "imf_estimate_normals: workspace must be 256-byte aligned");
  IMF_REQUIRE(workspace_bytes >= imf_normals_workspace_bytes(n), "imf_estimate_normals: workspace %zu < %zu",
              workspace_bytes, imf_normals_workspace_bytes(n));
  hipStream_t st = (hipStream_t)stream;
  const double edge = 0.5 * max_radius;
  Grid g;
  int32_t *err;
  int rc = build_grid(points, n, edge, (char *)workspace, g, err, st);
  if (rc) return rc;
  Viewpoint vp;
  vp.use = viewpoint_host != nullptr;
  for (int k = 0; k < 3; ++k) vp.v[k] = viewpoint_host ? viewpoint_host[k] : 0.0;
  k_normals<<<(unsigned)div_up(n, kNormalWaves), 64 * kNormalWaves, 0, st>>>(g, points, n, knn, edge,
                                                                             max_radius * max_radius, vp, normals, counts,
                                                                             nbr);
  IMF_CHECK_LAUNCH("imf_estimate_normals");
  IMF_CHECK_HIP(hipMemcpyAsync(out_err, err, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return IMF_OK;
}

}  // extern "C"
