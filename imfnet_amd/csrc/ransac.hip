// RANSAC registration on feature correspondences.
//
// Reference being replaced: scripts/benchmark_util.py:16-34 `run_ransac` = Open3D 0.12
// `registration_ransac_based_on_feature_matching(source, target, feat_s, feat_t,
// max_correspondence_distance = 1.5 voxel, TransformationEstimationPointToPoint(False), ransac_n,
// [CorrespondenceCheckerBasedOnEdgeLength(0.9), CorrespondenceCheckerBasedOnDistance(1.5 voxel)],
// RANSACConvergenceCriteria(50000, 1000), mutual_filter=False)`: correspondences = nearest target
// feature of every source point (imf_nn_search); then max_iteration hypotheses, each from ransac_n
// random correspondences: rigid fit (Umeyama without scale), edge-length and distance checkers, score
// = number of correspondences within max_correspondence_distance (ties: lower RMSE, then the earlier
// hypothesis -- the reference's sequential `IsBetterRANSACThan` keeps the first).  The criteria's second
// argument (1000) is outside Open3D 0.12's confidence range, so the loop never terminates early: all
// max_iteration hypotheses are drawn.  Open3D seeds its generator from std::random_device, so the
// reference's draw sequence cannot be reproduced; this implementation and its oracle restatement share
// a counter-based generator (splitmix64 of seed, iteration, pick) and agree hypothesis by hypothesis.
// Samples are drawn with replacement: a repeated pick passes the edge-length checker (0 against 0) and its fit is rank
// deficient; registration.h's rank rule makes that fit a proper rotation all the same (rank 0: a pure translation).
//
// A correspondence with corres[i] < 0 or corres[i] >= n_dst is "no correspondence" (imf_nn_search writes -1 for a
// query without a neighbour): a hypothesis that draws one fails the checkers without its points being loaded and is not
// counted in meta[2]; scoring reads row 0 in its place and masks the result, so it is never an inlier.  The draws are
// unchanged (r % n_src) and fitness keeps n_src as its denominator, as Open3D's fitness is over source points.  dst is
// never read outside [0, n_dst).
//
// On the GPU the 50 000 hypotheses are independent: one thread fits and checks each (fp64, 3x3
// one-sided Jacobi SVD), one wavefront scores each surviving hypothesis over all correspondences, one
// workgroup picks the winner in a fixed order.
#include "common.h"
#include "registration.h"

namespace imf {
namespace {

constexpr int kMaxSample = 4;   // ransac_n: 3 (3DMatch) or 4 (KITTI)

__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// one thread per hypothesis: sample, fit, checkers; valid[it] = 1 and Ts[it] = [R|t] when it survives
__global__ __launch_bounds__(256) void k_ransac_hypotheses(const double *__restrict__ src, const double *__restrict__ dst,
                                                           const int32_t *__restrict__ corres, int n_corres,
                                                           int n_dst, int ransac_n, double max_dist, double edge_sim,
                                                           uint64_t seed, int max_iter, double *__restrict__ Ts,
                                                           uint8_t *__restrict__ valid) {
  const int it = blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= max_iter) return;
  V3 s[kMaxSample], d[kMaxSample];
  bool ok = true;
  for (int j = 0; j < ransac_n; ++j) {
    const uint64_t r = splitmix64(seed ^ ((uint64_t)it * kMaxSample + j));
    const int ci = (int)(r % (uint64_t)n_corres);
    const int cj = corres[ci];
    if (cj < 0 || cj >= n_dst) {                  // no correspondence: the hypothesis fails, nothing is loaded
      ok = false;
      break;
    }
    s[j] = load3(src, ci);
    d[j] = load3(dst, cj);
  }
  for (int i = 0; i < ransac_n && ok; ++i)      // CorrespondenceCheckerBasedOnEdgeLength
    for (int j = i + 1; j < ransac_n; ++j) {
      const V3 es = sub(s[i], s[j]), ed = sub(d[i], d[j]);
      const double ds = sqrt(dot(es, es)), dd = sqrt(dot(ed, ed));
      if (ds < dd * edge_sim || dd < ds * edge_sim) {
        ok = false;
        break;
      }
    }
  double T[12];
  if (ok) {
    rigid_fit(s, d, ransac_n, T);
    for (int j = 0; j < ransac_n; ++j) {          // CorrespondenceCheckerBasedOnDistance
      const V3 e = sub(apply(T, s[j]), d[j]);
      if (sqrt(dot(e, e)) > max_dist) ok = false;
    }
  }
  valid[it] = ok ? 1 : 0;
  if (ok)
    for (int k = 0; k < 12; ++k) Ts[(long long)it * 12 + k] = T[k];
}

// one wavefront per hypothesis: inlier count and squared error over all correspondences
__global__ __launch_bounds__(256) void k_ransac_score(const double *__restrict__ src, const double *__restrict__ dst,
                                                      const int32_t *__restrict__ corres, int n_corres, int n_dst,
                                                      double max_dist, int max_iter, const double *__restrict__ Ts,
                                                      const uint8_t *__restrict__ valid, int32_t *__restrict__ inliers,
                                                      double *__restrict__ err2) {
  const int it = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (it >= max_iter) return;
  if (!valid[it]) {
    if (lane == 0) {
      inliers[it] = -1;
      err2[it] = 0.0;
    }
    return;
  }
  double T[12];
  for (int k = 0; k < 12; ++k) T[k] = Ts[(long long)it * 12 + k];
  int cnt = 0;
  double e2 = 0.0;
  for (int i = lane; i < n_corres; i += 64) {
    const int ci = corres[i];
    const bool has = (unsigned)ci < (unsigned)n_dst;   // no correspondence: row 0 is read in its place, never an inlier
    const V3 e = sub(apply(T, load3(src, i)), load3(dst, has ? ci : 0));
    const double dis = sqrt(dot(e, e));
    if (has && dis < max_dist) {
      ++cnt;
      e2 += dis * dis;
    }
  }
  // fixed-order reduction (xor butterfly): every lane ends with the same sums
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    e2 += __shfl_xor(e2, o, 64);
  }
  if (lane == 0) {
    inliers[it] = cnt;
    err2[it] = e2;
  }
}

// winner: most inliers, then lowest RMSE, then the earliest hypothesis
__global__ __launch_bounds__(1024) void k_ransac_select(const int32_t *__restrict__ inliers, const double *__restrict__ err2,
                                                        int max_iter, const double *__restrict__ Ts, int n_corres,
                                                        double *__restrict__ out_T, int32_t *__restrict__ meta,
                                                        double *__restrict__ stats) {
  __shared__ int s_cnt[1024], s_it[1024];
  __shared__ double s_rm[1024];
  const int t = threadIdx.x;
  int bc = -1, bi = 0x7fffffff, nvalid = 0;
  double br = 0.0;
  for (int it = t; it < max_iter; it += 1024) {
    const int c = inliers[it];
    if (c < 0) continue;
    ++nvalid;
    const double rm = c > 0 ? sqrt(err2[it] / c) : 0.0;
    if (c > bc || (c == bc && rm < br)) {   // `it` ascends per thread: strict comparisons keep the earliest
      bc = c; br = rm; bi = it;
    }
  }
  s_cnt[t] = bc; s_rm[t] = br; s_it[t] = bi;
  __shared__ int s_nv[1024];
  s_nv[t] = nvalid;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (t < o) {
      const int c = s_cnt[t + o], i2 = s_it[t + o];
      const double r = s_rm[t + o];
      const bool better = c > s_cnt[t] || (c == s_cnt[t] && (r < s_rm[t] || (r == s_rm[t] && i2 < s_it[t])));
      if (better) { s_cnt[t] = c; s_rm[t] = r; s_it[t] = i2; }
      s_nv[t] += s_nv[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    const bool any = s_cnt[0] > 0;       // Open3D starts from fitness 0: a hypothesis must have an inlier
    meta[0] = any ? s_it[0] : -1;
    meta[1] = any ? s_cnt[0] : 0;
    meta[2] = s_nv[0];
    stats[0] = any ? (double)s_cnt[0] / n_corres : 0.0;
    stats[1] = any ? s_rm[0] : 0.0;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) {
        double v = r == c ? 1.0 : 0.0;   // identity when nothing survives (Open3D's default result)
        if (any && r < 3) v = Ts[(long long)s_it[0] * 12 + 4 * r + c];
        out_T[4 * r + c] = v;
      }
  }
}

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

// host only: the fit of registration.h on CPU arrays, any n >= 1 (the sums of rigid_fit, then the same rigid_from_cov)
int imf_host_rigid_fit(const double *src, const double *dst, int n, double *T12) {
  IMF_REQUIRE(src && dst && T12, "imf_host_rigid_fit: null pointer");
  IMF_REQUIRE(n >= 1, "imf_host_rigid_fit: n=%d", n);
  V3 ms{0, 0, 0}, md{0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const V3 s = load3(src, i), d = load3(dst, i);
    ms.x += s.x; ms.y += s.y; ms.z += s.z;
    md.x += d.x; md.y += d.y; md.z += d.z;
  }
  const double inv = 1.0 / n;
  ms = {ms.x * inv, ms.y * inv, ms.z * inv};
  md = {md.x * inv, md.y * inv, md.z * inv};
  double B[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int i = 0; i < n; ++i) {
    const V3 a = sub(load3(src, i), ms), b = sub(load3(dst, i), md);
    const double av[3] = {a.x, a.y, a.z}, bv[3] = {b.x, b.y, b.z};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) B[r][c] += av[r] * bv[c];
  }
  rigid_from_cov(ms, md, B, T12);
  return IMF_OK;
}

size_t imf_ransac_workspace_bytes(int max_iter) {
  if (max_iter <= 0) return 0;
  return (size_t)max_iter * (12 * 8 + 8 + 4 + 1) + 256;
}

int imf_ransac_registration(const double *src, int64_t n_src, const double *dst, int64_t n_dst,
                            const int32_t *corres, int ransac_n, double max_corr_dist, double edge_similarity,
                            int max_iter, uint64_t seed, double *out_T, int32_t *out_meta, double *out_stats,
                            void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  IMF_REQUIRE(src && dst && corres && out_T && out_meta && out_stats && workspace, "imf_ransac_registration: null pointer");
  IMF_REQUIRE(n_src >= 1 && n_dst >= 1 && n_src < (1ll << 30) && n_dst <= 0x7fffffffll,
              "imf_ransac_registration: n_src=%lld n_dst=%lld", (long long)n_src, (long long)n_dst);
  IMF_REQUIRE(ransac_n >= 3 && ransac_n <= kMaxSample, "imf_ransac_registration: ransac_n=%d (3 or 4)", ransac_n);
  IMF_REQUIRE(max_iter >= 1 && max_iter <= (1 << 24), "imf_ransac_registration: max_iter=%d", max_iter);
  IMF_REQUIRE(workspace_bytes >= imf_ransac_workspace_bytes(max_iter), "imf_ransac_registration: workspace %zu < %zu",
              workspace_bytes, imf_ransac_workspace_bytes(max_iter));
  double *Ts = (double *)workspace;
  double *err2 = Ts + (size_t)max_iter * 12;
  int32_t *inl = (int32_t *)(err2 + max_iter);
  uint8_t *valid = (uint8_t *)(inl + max_iter);
  k_ransac_hypotheses<<<(unsigned)div_up(max_iter, 256), 256, 0, stream>>>(src, dst, corres, (int)n_src, (int)n_dst,
                                                                         ransac_n, max_corr_dist, edge_similarity, seed, max_iter,
                                                                         Ts, valid);
  k_ransac_score<<<(unsigned)div_up(max_iter, 4), 256, 0, stream>>>(src, dst, corres, (int)n_src, (int)n_dst, max_corr_dist,
                                                                    max_iter, Ts, valid, inl, err2);
  k_ransac_select<<<1, 1024, 0, stream>>>(inl, err2, max_iter, Ts, (int)n_src, out_T, out_meta, out_stats);
  IMF_CHECK_LAUNCH("imf_ransac_registration");
  return IMF_OK;
}

}  // extern "C"
