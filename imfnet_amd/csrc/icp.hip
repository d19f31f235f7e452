// Point-to-point ICP and the radius-count overlap test of the KITTI evaluation (imfnet_amd/evaluate_kitti.py).
//
// Reference being replaced (ICP): lib/data_loaders.py:527-556 refines every KITTI ground-truth pose with Open3D 0.12
// `registration_icp(src, dst, max_corr_dist, init, TransformationEstimationPointToPoint(), ICPConvergenceCriteria(
// max_iteration))`, relative_fitness = relative_rmse = 1e-6 (the defaults).  Restated here as pinned ([RECALLED] from
// Open3D's RegistrationICP; no Open3D to check against):
//   pcd = init . src; corr = correspondences(pcd)
//   for i < max_iteration:
//     update = umeyama(corr) (no scaling; identity when corr is empty)
//     T = update . T
//     pcd = update . pcd                 (incremental, as pcd.Transform(update): not recomputed from src)
//     corr = correspondences(pcd)
//     stop when |d fitness| < 1e-6 and |d rmse| < 1e-6
// correspondences: every source point gets its nearest target point with d^2 < r^2 (STRICT: FLANN's hybrid
// search keeps a neighbour whose squared distance is below the squared radius; cKDTree's distance_upper_bound
// excludes the bound too); equal distances go to the lowest target index.  fitness = n_corr / n_src, rmse =
// sqrt(sum d^2 / n_corr), both 0 without correspondences.  Reported: T, fitness, rmse of the last correspondence
// set, the loop iterations run, and n_corr.
//
// Reference being replaced (radius count): util/pointcloud.py:56-69 get_matching_indices(pcd0, pcd1, trans,
// 1.5 voxel), of which the evaluator only uses the length (lib/data_loaders.py:586-588: pairs with fewer than
// 1000 matches are skipped): the number of pairs (i, j) with |T src_i - dst_j| <= r (the radius search's bound,
// d^2 <= r^2), and optionally every source point's count.
//
// Reference being replaced (radius pairs): the same get_matching_indices, whose pairs themselves the training data set
// uses (lib/data_loaders.py:313, positive pairs of the hardest-contrastive loss): every (i, j) with |T src_i - dst_j|
// <= r, the same bound and transform arithmetic as the count.  FLANN lists a row's hits by distance; here row i's j
// ascend (the set is identical, the trainer samples from it at random).  Three steps after the grid: the count pass
// (k_radius_count into a per-point buffer), a one-workgroup int64 scan into CSR offsets, and an emit pass in which
// every source point fills its own segment and insertion-sorts it by j.  The segment contents do not depend on the
// scatter's order once sorted: bit-identical from run to run.
//
// Device design.  The target goes into a uniform grid ONCE per call: cell edge = r, so every point within r of a
// query lies in the 27 cells around the query's cell (a 125-cell probe at r/2 reads fewer candidates per cell but
// pays 98 more hash probes per point; on 5 cm KITTI subsets a 0.2 m cell holds a handful of points, the probes
// dominate).  Cells are keyed through the library's locality-preserving imf_slot hash (common.h): count per cell,
// one exclusive scan over the table, scatter into a cell-CSR copy of the target (fp64 xyz + original index).  The
// order of points inside a cell is whatever the scatter's atomics give, which is harmless: the nearest-neighbour
// choice is (d^2, index)-lexicographic, the count is a count.
// One ICP iteration is two plain launches: k_icp_corr (one thread per source point: apply the previous update to
// its current position, search the 27 cells, write the block's fp64 partial sums -- count, sum d^2, sum s, sum d,
// sum s d^T -- to its own row, no atomics), and k_icp_fit (one workgroup: sums the block rows in a fixed order,
// fitness / rmse / the convergence test / the Umeyama fit / T = update . T, all fp64).  The host enqueues
// 2 (max_iteration + 1) launches and never waits inside the loop; once the device's done flag is up, the remaining
// launches return at once.  No fp64 atomics anywhere: two runs are bit-identical.  No workgroup ever waits for
// another one.
//
// What the tests pin (tests/registration_cases.py, tests/test_gpu_registration_exact.py):
//   - the bound: ICP keeps d^2 < r^2 (a target at exactly r is no correspondence), count and pairs keep d^2 <= r^2;
//   - ties: equal d^2 go to the lowest ORIGINAL target index, whichever cell is probed first and whatever order the
//     scatter gave a cell; of exact duplicates the first occurrence wins;
//   - cells: cell = floor(x * inv_cell) with inv_cell = (1 - 1e-9) / r, so x = k r lies in cell k - 1 for k > 0 and in
//     cell k for k <= 0;
//   - the key range: a TARGET must lie in cells [-(2^17 - 1), 2^17 - 2] on every axis; one in the next cell, or a NaN,
//     raises the error flag (the wrappers raise ImfError).  A QUERY searches from cells [-2^17, 2^17 - 1]; beyond them,
//     or NaN, it finds nothing.  A query in an outermost cell probes a neighbour whose 18-bit key wraps to the other end
//     of the range: that cell is one no target may occupy, so nothing aliases;
//   - the update of a rank-deficient correspondence set is a proper rotation by the rank rule of registration.h: one
//     correspondence, or all on one target point, give R = I and the pure translation md - ms.  The zero must be exact
//     for that: the covariance is formed in one pass, sum s d^T - (sum s) md^T, and on generic coordinates a set whose
//     exact covariance is 0 leaves rounding noise there, whose fit is some proper rotation about the centroids.
//
// Point-to-plane ICP (imf_icp_point_to_plane).  Open3D registration_icp with TransformationEstimationPointToPlane(),
// restated ([RECALLED]; no Open3D to check against).  The loop, the correspondence rule (strict d^2 < r^2, ties -> lowest
// original index), fitness, rmse (over POINT distances, not plane residuals), T = update . T, the stop rule and the launch
// pattern are the point-to-point ones above; only the update differs:
//   r_i = (p_i - q_i) . n_i,  J_i = [p_i x n_i, n_i]  (rotation first),  solve (sum J^T J) x = -(sum J^T r),
//   update = [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5]
// with p the current source point, q its target and n the target's normal.  k_icp_corr<kEstPlane> writes per block the fp64
// partial sums count, sum d^2, the 21 upper entries of J^T J (row-major) and the 6 of J^T r; k_icp_fit<true> adds the block
// rows in the fixed order of the point-to-point fit and solves the 6x6 system by LDL^T without pivoting.
// The singular rule: when a pivot d_k <= 1e-12 * (the largest diagonal entry of sum J^T J), or is NaN, the update is the
// identity (as is the update of an empty correspondence set).  A single-plane target (rank 3) and fewer than 6 independent
// rows end there: the next stage then repeats the statistics and the stop rule ends the loop at iteration 1.
//
// Coloured ICP (imf_icp_colored): the joint fit of csrc/colored_icp.hip, whose head states the rule.  It is the third kind
// of k_icp_corr: the same loop, correspondences, statistics and launches; the 29 sums of the point-to-plane row are those
// of lambda J_G^T J_G + (1 - lambda) J_I^T J_I and lambda J_G r_G + (1 - lambda) J_I r_I, and k_icp_fit<true> serves unchanged.
#include "common.h"
#include "registration.h"
#include "point_grid.h"

namespace imf {
namespace {

constexpr int kIcpThreads = 256;
constexpr int kIcpSums = 17;           // count, sum d^2, sum s[3], sum d[3], sum s d^T [9]
constexpr int kIcpRow = 18;            // doubles per block row (padded)
constexpr int kFitThreads = 256;
constexpr int kPlaneSums = 29;         // point-to-plane: count, sum d^2, upper J^T J [21], J^T r [6]
constexpr int kPlaneRow = 30;          // doubles per block row (padded)

struct IcpInit {
  double T[16];                         // row-major 4x4, by value (a host matrix)
};

struct IcpState {
  double T[16];                         // accumulated transformation, row-major
  double upd[12];                       // the last update [R | t], applied by the next k_icp_corr
  double fitness, rmse;
  int32_t n_corr, iters, done, pad;
};

__global__ __launch_bounds__(256) void k_icp_start(const double *__restrict__ src, int64_t n, IcpInit init,
                                                   double *__restrict__ cur, IcpState *st) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    for (int k = 0; k < 16; ++k) st->T[k] = init.T[k];
    st->fitness = st->rmse = 0.0;
    st->n_corr = st->iters = st->done = st->pad = 0;
  }
  if (i >= n) return;
  const V3 p = apply(init.T, load3(src, i));
  cur[3 * i + 0] = p.x; cur[3 * i + 1] = p.y; cur[3 * i + 2] = p.z;
}

enum Estimation { kEstPoint, kEstPlane, kEstColor };

// what the coloured kind reads besides the normals: intensities of the source rows and of the target, the target's colour
// gradient [n_dst, 3] (target arrays in the ORIGINAL order), and lambda_geometric.  Unused by the other kinds.
struct ColorTerm {
  const double *src_intensity, *dst_intensity, *dst_gradient;
  double lambda;
};

// stage k: k = 0 on the initial points, k = i + 1 after the update of iteration i.  kEstPlane: the point-to-plane sums, with
// normals [n_dst, 3] in the target's ORIGINAL order (unused by kEstPoint); kEstColor: the joint sums in the same layout
template <Estimation kEst>
__global__ __launch_bounds__(kIcpThreads) void k_icp_corr(Grid g, const double *__restrict__ normals,
                                                          double *__restrict__ cur, int64_t n, double r2, int stage,
                                                          const IcpState *__restrict__ st, double *__restrict__ partial,
                                                          ColorTerm ct) {
  if (st->done) return;
  constexpr bool kPlane = kEst != kEstPoint;
  constexpr int kSums = kPlane ? kPlaneSums : kIcpSums, kRow = kPlane ? kPlaneRow : kIcpRow;
  __shared__ double lds4[4];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double v[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) v[k] = 0.0;
  if (i < n) {
    V3 p = load3(cur, i);
    if (stage > 0) {
      p = apply(st->upd, p);
      cur[3 * i + 0] = p.x; cur[3 * i + 1] = p.y; cur[3 * i + 2] = p.z;
    }
    double d2;
    const int r = grid_nearest(g, p, r2, d2);
    if (r >= 0) {
      const V3 q = load3(g.xyz, r);
      v[0] = 1.0;
      v[1] = d2;
      if constexpr (kEst == kEstColor) {
        const int j = g.idx[r];
        const V3 nq = load3(normals, j), gq = load3(ct.dst_gradient, j);
        const V3 c = cross(p, nq);
        const double res = dot(sub(p, q), nq);
        const V3 pt{p.x - res * nq.x, p.y - res * nq.y, p.z - res * nq.z};            // p projected onto q's tangent plane
        const double ri = ct.src_intensity[i] - (ct.dst_intensity[j] + dot(gq, sub(pt, q)));
        const double ng = dot(nq, gq);
        const V3 M{ng * nq.x - gq.x, ng * nq.y - gq.y, ng * nq.z - gq.z};              // -g + (n . g) n
        const V3 cm = cross(p, M);
        const double J[6] = {c.x, c.y, c.z, nq.x, nq.y, nq.z}, K[6] = {cm.x, cm.y, cm.z, M.x, M.y, M.z};
        const double wg = ct.lambda, wi = 1.0 - ct.lambda;
        int k = 2;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) v[k++] = wg * (J[a] * J[b]) + wi * (K[a] * K[b]);
#pragma unroll
        for (int a = 0; a < 6; ++a) v[23 + a] = wg * (J[a] * res) + wi * (K[a] * ri);
      } else if constexpr (kPlane) {
        const V3 nq = load3(normals, g.idx[r]);
        const V3 c = cross(p, nq);
        const double res = dot(sub(p, q), nq);
        const double J[6] = {c.x, c.y, c.z, nq.x, nq.y, nq.z};
        int k = 2;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) v[k++] = J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) v[23 + a] = J[a] * res;
      } else {
        const double sv[3] = {p.x, p.y, p.z}, dv[3] = {q.x, q.y, q.z};
        for (int a = 0; a < 3; ++a) {
          v[2 + a] = sv[a];
          v[5 + a] = dv[a];
          for (int b = 0; b < 3; ++b) v[8 + 3 * a + b] = sv[a] * dv[b];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    const double s = block_sum(v[k], lds4);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * kRow + k] = s;
  }
}

// one workgroup per stage; kPlane selects the sums' layout and the update (point-to-point: Umeyama, point-to-plane: LDL^T)
template <bool kPlane>
__global__ __launch_bounds__(kFitThreads) void k_icp_fit(const double *__restrict__ partial, int n_blocks, int64_t n_src,
                                                         int stage, int max_iteration, IcpState *st, double *out_T,
                                                         double *out_stats, int32_t *out_meta) {
  if (st->done) return;
  __shared__ double lds[kFitThreads];
  constexpr int kSums = kPlane ? kPlaneSums : kIcpSums, kRow = kPlane ? kPlaneRow : kIcpRow;
  __shared__ double sums[kSums];
  const int t = threadIdx.x;
  for (int k = 0; k < kSums; ++k) {
    double a = 0.0;
    for (int b = t; b < n_blocks; b += kFitThreads) a += partial[(int64_t)b * kRow + k];   // ascending per thread
    lds[t] = a;
    __syncthreads();
    for (int o = kFitThreads / 2; o > 0; o >>= 1) {     // fixed tree
      if (t < o) lds[t] += lds[t + o];
      __syncthreads();
    }
    if (t == 0) sums[k] = lds[0];
    __syncthreads();
  }
  if (t != 0) return;
  const double cnt = sums[0];
  const int n_corr = (int)cnt;
  const double fitness = n_corr > 0 ? cnt / (double)n_src : 0.0;
  const double rmse = n_corr > 0 ? sqrt(sums[1] / cnt) : 0.0;
  int done = 0;
  if (stage > 0) {
    st->iters = stage;
    if (fabs(st->fitness - fitness) < 1e-6 && fabs(st->rmse - rmse) < 1e-6) done = 1;
  }
  if (stage >= max_iteration) done = 1;
  st->fitness = fitness;
  st->rmse = rmse;
  st->n_corr = n_corr;
  if (!done) {
    double U[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if constexpr (kPlane) {
      double A[6][6], b[6], x[6];
      int k = 2;
      for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) A[a][c] = A[c][a] = sums[k++];
      for (int a = 0; a < 6; ++a) b[a] = sums[23 + a];
      if (n_corr > 0 && solve_plane_system(A, b, x)) update_from_solution(x, U);   // both in registration.h
    } else if (n_corr > 0) {
      const double inv = 1.0 / cnt;
      const V3 ms{sums[2] * inv, sums[3] * inv, sums[4] * inv}, md{sums[5] * inv, sums[6] * inv, sums[7] * inv};
      const double sv[3] = {sums[2], sums[3], sums[4]}, mdv[3] = {md.x, md.y, md.z};
      double B[3][3];                                   // sum (s - ms)(d - md)^T = sum s d^T - (sum s) md^T
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) B[a][b] = sums[8 + 3 * a + b] - sv[a] * mdv[b];
      rigid_from_cov(ms, md, B, U);
    }
    double Tn[16];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c)
        Tn[4 * r + c] = U[4 * r + 0] * st->T[c] + U[4 * r + 1] * st->T[4 + c] + U[4 * r + 2] * st->T[8 + c] +
                        U[4 * r + 3] * st->T[12 + c];
    for (int c = 0; c < 4; ++c) Tn[12 + c] = st->T[12 + c];
    for (int k = 0; k < 16; ++k) st->T[k] = Tn[k];
    for (int k = 0; k < 12; ++k) st->upd[k] = U[k];
  }
  st->done = done;
  for (int k = 0; k < 16; ++k) out_T[k] = st->T[k];
  out_stats[0] = fitness;
  out_stats[1] = rmse;
  out_meta[0] = st->iters;
  out_meta[1] = n_corr;
}

// radius count: one thread per source point, integer totals (order-free)
__global__ __launch_bounds__(256) void k_radius_count(Grid g, const double *__restrict__ src, int64_t n, IcpInit T, double r2,
                                                      int32_t *__restrict__ per_point, unsigned long long *total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int c = 0;
  if (i < n) {
    const V3 p = apply(T.T, load3(src, i));
    int x, y, z;
    if (cell_of_point(p, g.inv_cell, kCoordLim, x, y, z))
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int s = hash_find_slot(g.tab, g.capmask, pack_key(0, x + dx, y + dy, z + dz));
            if (s < 0) continue;
            const uint4 v = *reinterpret_cast<const uint4 *>(g.tab + s);
            for (int r = (int)v.z, r1 = (int)v.z + (int)v.w; r < r1; ++r) {
              const V3 e = sub(load3(g.xyz, r), p);
              if (dot(e, e) <= r2) ++c;
            }
          }
    if (per_point) per_point[i] = c;
  }
  unsigned long long w = (unsigned long long)c;
  for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
  if ((threadIdx.x & 63) == 0 && w) atomicAdd(total, w);
}

__global__ void k_zero_u64(unsigned long long *p) { *p = 0ull; }

// radius pairs, step 2: one workgroup, exclusive scan of the per-point counts in point order -> offsets[0..n],
// *out_total = offsets[n].  Each thread owns a contiguous run of points; int64 sums, no atomics.
__global__ __launch_bounds__(1024) void k_pairs_scan(const int32_t *__restrict__ cnt, int64_t n,
                                                     int64_t *__restrict__ offsets, int64_t *__restrict__ out_total) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (n + 1023) / 1024, b = t * per, e = min(n, b + per);
  int64_t sum = 0;
  for (int64_t i = b; i < e; ++i) sum += cnt[i];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {                 // Hillis-Steele inclusive scan
    const int64_t v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = part[t] - sum;
  for (int64_t i = b; i < e; ++i) {
    offsets[i] = run;
    run += cnt[i];
  }
  if (t == 1023) {
    offsets[n] = part[1023];
    *out_total = part[1023];
  }
}

// radius pairs, step 3: one thread per source point writes (i, j) for every target within r into its own segment
// [offsets[i], offsets[i+1]), then insertion-sorts the segment by j.  Nothing is written when the total exceeds the
// capacity.  The candidate test is k_radius_count's, so the segment fills exactly; the bound check is a guard.
__global__ __launch_bounds__(256) void k_pairs_emit(Grid g, const double *__restrict__ src, int64_t n, IcpInit T,
                                                    double r2, const int64_t *__restrict__ offsets, int64_t capacity,
                                                    int32_t *__restrict__ pairs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || offsets[n] > capacity) return;
  const int64_t o0 = offsets[i], o1 = offsets[i + 1];
  if (o1 == o0) return;
  int2 *seg = reinterpret_cast<int2 *>(pairs) + o0;
  const int64_t len = o1 - o0;
  const V3 p = apply(T.T, load3(src, i));
  int64_t c = 0;
  int x, y, z;
  if (cell_of_point(p, g.inv_cell, kCoordLim, x, y, z))
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int s = hash_find_slot(g.tab, g.capmask, pack_key(0, x + dx, y + dy, z + dz));
          if (s < 0) continue;
          const uint4 v = *reinterpret_cast<const uint4 *>(g.tab + s);
          for (int r = (int)v.z, r1 = (int)v.z + (int)v.w; r < r1; ++r) {
            const V3 e = sub(load3(g.xyz, r), p);
            if (dot(e, e) <= r2 && c < len) seg[c++] = make_int2((int32_t)i, g.idx[r]);
          }
        }
  for (int64_t a = 1; a < c; ++a) {                    // a few dozen entries at r = 1.5 voxel
    const int2 v = seg[a];
    int64_t b = a - 1;
    while (b >= 0 && seg[b].y > v.y) {
      seg[b + 1] = seg[b];
      --b;
    }
    seg[b + 1] = v;
  }
}

size_t icp_workspace_bytes(int64_t n_src, int64_t n_dst, int row) {
  if (n_src <= 0 || n_dst <= 0) return 0;
  const size_t nb = (size_t)div_up(n_src, kIcpThreads);
  return grid_layout(n_dst).total + align256((size_t)n_src * 24) + align256(nb * row * 8) + align256(sizeof(IcpState));
}

// the ICP entry points: the argument checks, the grid, 2 (max_iteration + 1) launches; normals: point-to-plane and coloured,
// ct: coloured only
template <Estimation kEst>
int icp_run(const char *name, const double *src, int64_t n_src, const double *dst, const double *normals, int64_t n_dst,
            double max_corr_dist, const double *init_host, int max_iteration, double *out_T, double *out_stats,
            int32_t *out_meta, void *workspace, size_t workspace_bytes, void *stream, ColorTerm ct = ColorTerm{}) {
  constexpr bool kPlane = kEst != kEstPoint;
  constexpr int kRow = kPlane ? kPlaneRow : kIcpRow;
  IMF_REQUIRE(src && dst && (normals || !kPlane) && out_T && out_stats && out_meta && workspace, "%s: null pointer", name);
  if constexpr (kEst == kEstColor) {
    IMF_REQUIRE(ct.src_intensity, "%s: null pointer (src_intensity)", name);
    IMF_REQUIRE(ct.dst_intensity, "%s: null pointer (dst_intensity)", name);
    IMF_REQUIRE(ct.dst_gradient, "%s: null pointer (dst_gradient)", name);
    IMF_REQUIRE(ct.lambda >= 0.0 && ct.lambda <= 1.0, "%s: lambda_geometric=%g, expected 0..1", name, ct.lambda);   // NaN too
  }
  IMF_REQUIRE(n_src >= 1 && n_dst >= 1 && n_src < (1ll << 30) && n_dst < (1ll << 30), "%s: n_src=%lld n_dst=%lld", name,
              (long long)n_src, (long long)n_dst);
  IMF_REQUIRE(max_corr_dist > 0.0 && max_corr_dist < 1e6, "%s: max_corr_dist=%g", name, max_corr_dist);
  IMF_REQUIRE(max_iteration >= 0 && max_iteration <= 100000, "%s: max_iteration=%d", name, max_iteration);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", name);
  IMF_REQUIRE(workspace_bytes >= icp_workspace_bytes(n_src, n_dst, kRow), "%s: workspace %zu < %zu", name, workspace_bytes,
              icp_workspace_bytes(n_src, n_dst, kRow));
  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  Grid g;
  int32_t *err;
  int rc = build_grid(dst, n_dst, max_corr_dist, ws, g, err, st);
  if (rc) return rc;
  size_t p = grid_layout(n_dst).total;
  const int nb = (int)div_up(n_src, kIcpThreads);
  double *cur = (double *)(ws + p);     p += align256((size_t)n_src * 24);
  double *partial = (double *)(ws + p); p += align256((size_t)nb * kRow * 8);
  IcpState *state = (IcpState *)(ws + p);
  IcpInit init;
  for (int k = 0; k < 16; ++k) init.T[k] = init_host ? init_host[k] : (k % 5 == 0 ? 1.0 : 0.0);
  k_icp_start<<<(unsigned)nb, 256, 0, st>>>(src, n_src, init, cur, state);
  const double r2 = max_corr_dist * max_corr_dist;
  for (int stage = 0; stage <= max_iteration; ++stage) {
    k_icp_corr<kEst><<<(unsigned)nb, kIcpThreads, 0, st>>>(g, normals, cur, n_src, r2, stage, state, partial, ct);
    k_icp_fit<kPlane><<<1, kFitThreads, 0, st>>>(partial, nb, n_src, stage, max_iteration, state, out_T, out_stats, out_meta);
  }
  IMF_CHECK_LAUNCH(name);
  IMF_CHECK_HIP(hipMemcpyAsync(out_meta + 2, err, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return IMF_OK;
}

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

size_t imf_icp_workspace_bytes(int64_t n_src, int64_t n_dst) { return icp_workspace_bytes(n_src, n_dst, kIcpRow); }

int imf_icp_point_to_point(const double *src, int64_t n_src, const double *dst, int64_t n_dst, double max_corr_dist,
                           const double *init_host, int max_iteration, double *out_T, double *out_stats,
                           int32_t *out_meta, void *workspace, size_t workspace_bytes, void *stream) {
  return icp_run<kEstPoint>("imf_icp_point_to_point", src, n_src, dst, nullptr, n_dst, max_corr_dist, init_host,
                            max_iteration, out_T, out_stats, out_meta, workspace, workspace_bytes, stream);
}

size_t imf_icp_plane_workspace_bytes(int64_t n_src, int64_t n_dst) { return icp_workspace_bytes(n_src, n_dst, kPlaneRow); }

int imf_icp_point_to_plane(const double *src, int64_t n_src, const double *dst, const double *dst_normals, int64_t n_dst,
                           double max_corr_dist, const double *init_host, int max_iteration, double *out_T,
                           double *out_stats, int32_t *out_meta, void *workspace, size_t workspace_bytes, void *stream) {
  return icp_run<kEstPlane>("imf_icp_point_to_plane", src, n_src, dst, dst_normals, n_dst, max_corr_dist, init_host,
                            max_iteration, out_T, out_stats, out_meta, workspace, workspace_bytes, stream);
}

size_t imf_icp_colored_workspace_bytes(int64_t n_src, int64_t n_dst) { return icp_workspace_bytes(n_src, n_dst, kPlaneRow); }

int imf_icp_colored(const double *src, const double *src_intensity, int64_t n_src, const double *dst,
                    const double *dst_normals, const double *dst_intensity, const double *dst_gradient, int64_t n_dst,
                    double max_corr_dist, double lambda_geometric, const double *init_host, int max_iteration, double *out_T,
                    double *out_stats, int32_t *out_meta, void *workspace, size_t workspace_bytes, void *stream) {
  return icp_run<kEstColor>("imf_icp_colored", src, n_src, dst, dst_normals, n_dst, max_corr_dist, init_host, max_iteration,
                            out_T, out_stats, out_meta, workspace, workspace_bytes, stream,
                            ColorTerm{src_intensity, dst_intensity, dst_gradient, lambda_geometric});
}

size_t imf_radius_count_workspace_bytes(int64_t n_dst) {
  if (n_dst <= 0) return 0;
  return grid_layout(n_dst).total;
}

int imf_radius_count(const double *src, int64_t n_src, const double *dst, int64_t n_dst, const double *T_host, double r,
                     int64_t *out_count, int32_t *out_per_point, int32_t *out_err, void *workspace,
                     size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(src && dst && out_count && out_err && workspace, "imf_radius_count: null pointer");
  IMF_REQUIRE(n_src >= 1 && n_dst >= 1 && n_src < (1ll << 30) && n_dst < (1ll << 30),
              "imf_radius_count: n_src=%lld n_dst=%lld", (long long)n_src, (long long)n_dst);
  IMF_REQUIRE(r > 0.0 && r < 1e6, "imf_radius_count: r=%g", r);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "imf_radius_count: workspace must be 256-byte aligned");
  IMF_REQUIRE(workspace_bytes >= imf_radius_count_workspace_bytes(n_dst), "imf_radius_count: workspace %zu < %zu",
              workspace_bytes, imf_radius_count_workspace_bytes(n_dst));
  hipStream_t st = (hipStream_t)stream;
  Grid g;
  int32_t *err;
  int rc = build_grid(dst, n_dst, r, (char *)workspace, g, err, st);
  if (rc) return rc;
  IcpInit T;
  for (int k = 0; k < 16; ++k) T.T[k] = T_host ? T_host[k] : (k % 5 == 0 ? 1.0 : 0.0);
  unsigned long long *total = reinterpret_cast<unsigned long long *>(out_count);
  k_zero_u64<<<1, 1, 0, st>>>(total);
  k_radius_count<<<(unsigned)div_up(n_src, 256), 256, 0, st>>>(g, src, n_src, T, r * r, out_per_point, total);
  IMF_CHECK_LAUNCH("imf_radius_count");
  IMF_CHECK_HIP(hipMemcpyAsync(out_err, err, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return IMF_OK;
}

// radius pairs: workspace = the grid, the per-point counts, the count pass's total
size_t imf_radius_pairs_workspace_bytes(int64_t n_src, int64_t n_dst) {
  if (n_src <= 0 || n_dst <= 0) return 0;
  return grid_layout(n_dst).total + align256((size_t)n_src * 4) + 256;
}

int imf_radius_pairs(const double *src, int64_t n_src, const double *dst, int64_t n_dst, const double *T_host, double r,
                     int64_t *offsets, int32_t *pairs, int64_t capacity, int64_t *out_total, int32_t *out_err,
                     void *workspace, size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(offsets && out_total && out_err, "imf_radius_pairs: null pointer");
  IMF_REQUIRE(n_src >= 0 && n_dst >= 0 && n_src < (1ll << 30) && n_dst < (1ll << 30),
              "imf_radius_pairs: n_src=%lld n_dst=%lld", (long long)n_src, (long long)n_dst);
  IMF_REQUIRE(r > 0.0 && r < 1e6, "imf_radius_pairs: r=%g", r);
  IMF_REQUIRE(capacity >= 0 && (pairs || capacity == 0), "imf_radius_pairs: capacity=%lld with pairs=%p",
              (long long)capacity, (const void *)pairs);
  IMF_REQUIRE(((uintptr_t)pairs & 7) == 0, "imf_radius_pairs: pairs must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (n_src == 0 || n_dst == 0) {                      // no pairs: zero the outputs, launch nothing
    IMF_CHECK_HIP(hipMemsetAsync(offsets, 0, (size_t)(n_src + 1) * sizeof(int64_t), st));
    IMF_CHECK_HIP(hipMemsetAsync(out_total, 0, sizeof(int64_t), st));
    IMF_CHECK_HIP(hipMemsetAsync(out_err, 0, sizeof(int32_t), st));
    return IMF_OK;
  }
  IMF_REQUIRE(src && dst && workspace, "imf_radius_pairs: null pointer");
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "imf_radius_pairs: workspace must be 256-byte aligned");
  IMF_REQUIRE(workspace_bytes >= imf_radius_pairs_workspace_bytes(n_src, n_dst),
              "imf_radius_pairs: workspace %zu < %zu", workspace_bytes, imf_radius_pairs_workspace_bytes(n_src, n_dst));
  char *ws = (char *)workspace;
  Grid g;
  int32_t *err;
  int rc = build_grid(dst, n_dst, r, ws, g, err, st);
  if (rc) return rc;
  size_t p = grid_layout(n_dst).total;
  int32_t *cnt = (int32_t *)(ws + p);                              p += align256((size_t)n_src * 4);
  unsigned long long *count_total = (unsigned long long *)(ws + p);
  IcpInit T;
  for (int k = 0; k < 16; ++k) T.T[k] = T_host ? T_host[k] : (k % 5 == 0 ? 1.0 : 0.0);
  const unsigned nb = (unsigned)div_up(n_src, 256);
  k_zero_u64<<<1, 1, 0, st>>>(count_total);
  k_radius_count<<<nb, 256, 0, st>>>(g, src, n_src, T, r * r, cnt, count_total);
  k_pairs_scan<<<1, 1024, 0, st>>>(cnt, n_src, offsets, out_total);
  k_pairs_emit<<<nb, 256, 0, st>>>(g, src, n_src, T, r * r, offsets, capacity, pairs);
  IMF_CHECK_LAUNCH("imf_radius_pairs");
  IMF_CHECK_HIP(hipMemcpyAsync(out_err, err, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return IMF_OK;
}

}  // extern "C"
