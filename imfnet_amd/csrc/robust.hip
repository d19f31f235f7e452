// The robust transform estimator of the trainer's validation (imfnet_amd/train/trainer.py valid_epoch): RTE / RRE /
// success of a pair from its feature correspondences.
//
// Reference being replaced: util/transform_estimation.py:89-116 est_quad_linear_robust(pts0, pts1, weight), 20 rounds
// on the host in float32.  Restated:
//   cur = pts0; T = I; par = 1; w = weight (ones when absent)
//   for i < 20:
//     if i > 0 and i % 5 == 0: par /= 2
//     A = w . J(cur) (3n x 6, J = [-[cur]x | I] per point), b = w . (pts1 - cur)
//     x = (A^T A)^-1 A^T b
//     U = [Rz(x2) Ry(x1) Rx(x0) | x3..5];  cur = U cur;  T = U T
//     w = par / (|cur - pts1| + par)
// Changed on purpose: fp64 throughout (upstream is float32); the normal equations are solved by elimination with
// pivoting on the diagonally equilibrated matrix instead of an explicit inverse; a system that cannot be solved sets
// a flag and returns the identity (upstream raises from torch.inverse).
//
// Device design.  ONE launch of ONE workgroup (512 threads = 8 wavefronts) carries all 20 rounds; the host enqueues
// it and never waits.  Thread t owns rows t, t + 512, ...: up to kRtRows = 10 of them live in registers (current point
// and weight; n <= 5 120 covers the trainer's 5 000-row subsample), beyond that in the caller's workspace, which only
// the owning thread ever touches.  512 threads, not 1024: a 512-thread workgroup may use 256 VGPRs per thread, and the
// ten rows (80), the 16 accumulators (32), U (24) and the inlined solve need 216; at 1024 threads the cap is 128 and
// half of the rows spilled to scratch.  `make resource-usage` on this file: k_robust_transform<true> 216 VGPRs, 0
// spills, 0 bytes of scratch; <false> 104 VGPRs, 0 spills, 0 bytes of scratch.  A is never built: the three rows of a point have known sparsity, so A^T A is
//   [ sum W (|p|^2 I - p p^T)    sum W [p]x ]
//   [ sum W [p]x^T               sum W I    ]        W = w^2
// and its 21 distinct entries come from 10 moments (W, W p, W p p^T); with the 6 entries of A^T b that is 16 sums per
// round.  Each thread adds its rows in ascending order, a wavefront combines by an xor butterfly, the 8 wavefronts'
// partials go through LDS and thread 0 adds them in wavefront order: no atomics, the same order every call, so two
// calls are bit-identical.  Thread 0 solves the 6 x 6 system in LDS and publishes U; every thread then moves its rows
// and computes their new weights in the same pass.
#include "common.h"
#include "registration.h"

namespace imf {
namespace {

constexpr int kRtThreads = 512;
constexpr int kRtWaves = kRtThreads / 64;
constexpr int kRtSums = 16;            // W xx yy zz xy xz yz x y z 1 (10 moments), then A^T b (6)
constexpr int kRtRows = 10;            // register-resident rows per thread
constexpr int kRtRounds = 20;
constexpr double kRtPivotMin = 1e-10;  // smallest pivot of the unit-diagonal (equilibrated) matrix taken as solvable

struct RtShared {
  double part[kRtWaves][kRtSums];
  double M[6][7];                      // equilibrated [A^T A | A^T b], eliminated in place
  double d[6];                         // 1 / sqrt(diag)
  double U[12];                        // this round's [R | t], row-major 3x4
  double T[16];                        // accumulated transform
  int bad;
};

__device__ __forceinline__ void rt_add_row(double (&s)[kRtSums], V3 p, V3 q, double w) {
  const double W = w * w;
  const V3 r = sub(q, p);
  const double Wx = W * p.x, Wy = W * p.y, Wz = W * p.z;
  s[0] += Wx * p.x; s[1] += Wy * p.y; s[2] += Wz * p.z;
  s[3] += Wx * p.y; s[4] += Wx * p.z; s[5] += Wy * p.z;
  s[6] += Wx; s[7] += Wy; s[8] += Wz; s[9] += W;
  s[10] += Wy * r.z - Wz * r.y;        // J^T r: rotation part is p x r
  s[11] += Wz * r.x - Wx * r.z;
  s[12] += Wx * r.y - Wy * r.x;
  s[13] += W * r.x; s[14] += W * r.y; s[15] += W * r.z;
}

// thread 0: the wavefront partials in order, the equilibrated system, elimination with partial pivoting, U and T.
// Inlined on purpose: as a call it forces the caller's rows out of their registers around it.
// Returns false when the system cannot be solved.
__device__ __forceinline__ bool rt_solve_round(RtShared &sh) {
  double S[kRtSums];
#pragma unroll
  for (int k = 0; k < kRtSums; ++k) {
    double a = sh.part[0][k];
    for (int w = 1; w < kRtWaves; ++w) a += sh.part[w][k];
    S[k] = a;
  }
  double(*M)[7] = sh.M;
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 7; ++c) M[r][c] = 0.0;
  M[0][0] = S[1] + S[2]; M[0][1] = -S[3];       M[0][2] = -S[4];       M[0][4] = -S[8]; M[0][5] = S[7];
  M[1][1] = S[0] + S[2]; M[1][2] = -S[5];       M[1][3] = S[8];        M[1][5] = -S[6];
  M[2][2] = S[0] + S[1]; M[2][3] = -S[7];       M[2][4] = S[6];
  M[3][3] = M[4][4] = M[5][5] = S[9];
  for (int r = 0; r < 6; ++r) {
    for (int c = 0; c < r; ++c) M[r][c] = M[c][r];
    M[r][6] = S[10 + r];
  }
  for (int r = 0; r < 6; ++r) {
    const double v = M[r][r];
    if (!(v > 0.0) || !(v < 1.79e308)) return false;              // NaN, inf, no weight at all
    sh.d[r] = 1.0 / sqrt(v);
  }
  for (int r = 0; r < 6; ++r) {
    for (int c = 0; c < 6; ++c) M[r][c] *= sh.d[r] * sh.d[c];
    M[r][6] *= sh.d[r];
  }
  for (int k = 0; k < 6; ++k) {
    int piv = k;
    for (int r = k + 1; r < 6; ++r)
      if (fabs(M[r][k]) > fabs(M[piv][k])) piv = r;
    if (!(fabs(M[piv][k]) >= kRtPivotMin)) return false;           // rank deficient (or NaN)
    if (piv != k)
      for (int c = k; c < 7; ++c) {
        const double t = M[k][c];
        M[k][c] = M[piv][c];
        M[piv][c] = t;
      }
    const double inv = 1.0 / M[k][k];
    for (int r = k + 1; r < 6; ++r) {
      const double f = M[r][k] * inv;
      for (int c = k; c < 7; ++c) M[r][c] -= f * M[k][c];
    }
  }
  for (int k = 5; k >= 0; --k) {
    double v = M[k][6];
    for (int c = k + 1; c < 6; ++c) v -= M[k][c] * M[c][6];
    M[k][6] = v / M[k][k];
  }
  double x[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    x[k] = M[k][6] * sh.d[k];
    if (!(fabs(x[k]) < 1.79e308)) return false;
  }
  const double sa = sin(x[0]), ca = cos(x[0]), sb = sin(x[1]), cb = cos(x[1]), sc = sin(x[2]), cc = cos(x[2]);
  double *U = sh.U;                                                // Rz(x2) Ry(x1) Rx(x0)
  U[0] = cc * cb; U[1] = cc * sb * sa - sc * ca; U[2] = cc * sb * ca + sc * sa;  U[3] = x[3];
  U[4] = sc * cb; U[5] = sc * sb * sa + cc * ca; U[6] = sc * sb * ca - cc * sa;  U[7] = x[4];
  U[8] = -sb;     U[9] = cb * sa;                U[10] = cb * ca;                U[11] = x[5];
  double Tn[12];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      Tn[4 * r + c] = U[4 * r] * sh.T[c] + U[4 * r + 1] * sh.T[4 + c] + U[4 * r + 2] * sh.T[8 + c] +
                      (c == 3 ? U[4 * r + 3] : 0.0);
#pragma unroll
  for (int k = 0; k < 12; ++k) sh.T[k] = Tn[k];
  return true;
}

// kRegs: every thread's rows fit its registers (n <= kRtThreads * kRtRows); otherwise cur [n,3] and wgt [n] are the
// workspace, read and written by the owning thread only.
template <bool kRegs>
__global__ __launch_bounds__(kRtThreads) void k_robust_transform(const double *__restrict__ pts0,
                                                                 const double *__restrict__ pts1,
                                                                 const double *__restrict__ weight, int64_t n,
                                                                 double *__restrict__ cur, double *__restrict__ wgt,
                                                                 double *__restrict__ out_T,
                                                                 int32_t *__restrict__ out_meta) {
  __shared__ RtShared sh;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  V3 p[kRtRows];
  double w[kRtRows];
  if (kRegs) {
#pragma unroll
    for (int k = 0; k < kRtRows; ++k) {
      const int64_t i = t + (int64_t)k * kRtThreads;
      p[k] = i < n ? load3(pts0, i) : V3{0.0, 0.0, 0.0};
      w[k] = i < n ? (weight ? weight[i] : 1.0) : 0.0;
    }
  } else {
    for (int64_t i = t; i < n; i += kRtThreads) {
      cur[3 * i] = pts0[3 * i]; cur[3 * i + 1] = pts0[3 * i + 1]; cur[3 * i + 2] = pts0[3 * i + 2];
      wgt[i] = weight ? weight[i] : 1.0;
    }
  }
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k) sh.T[k] = (k % 5 == 0) ? 1.0 : 0.0;
    sh.bad = 0;
  }
  double par = 1.0;
  for (int round = 0; round < kRtRounds; ++round) {
    if (round > 0 && round % 5 == 0) par *= 0.5;
    double s[kRtSums];
#pragma unroll
    for (int k = 0; k < kRtSums; ++k) s[k] = 0.0;
    if (kRegs) {
#pragma unroll
      for (int k = 0; k < kRtRows; ++k) {
        const int64_t i = t + (int64_t)k * kRtThreads;
        if (i < n) rt_add_row(s, p[k], load3(pts1, i), w[k]);
      }
    } else {
      for (int64_t i = t; i < n; i += kRtThreads) rt_add_row(s, load3(cur, i), load3(pts1, i), wgt[i]);
    }
#pragma unroll
    for (int k = 0; k < kRtSums; ++k) {
      double v = s[k];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) sh.part[wave][k] = v;
    }
    __syncthreads();
    if (t == 0 && !rt_solve_round(sh)) sh.bad = 1;
    __syncthreads();
    if (sh.bad) break;                                             // uniform: every thread reads the same word
    double U[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) U[k] = sh.U[k];
    if (kRegs) {
#pragma unroll
      for (int k = 0; k < kRtRows; ++k) {
        const int64_t i = t + (int64_t)k * kRtThreads;
        if (i < n) {
          p[k] = apply(U, p[k]);
          const V3 e = sub(p[k], load3(pts1, i));
          w[k] = par / (sqrt(dot(e, e)) + par);
        }
      }
    } else {
      for (int64_t i = t; i < n; i += kRtThreads) {
        const V3 q = apply(U, load3(cur, i));
        cur[3 * i] = q.x; cur[3 * i + 1] = q.y; cur[3 * i + 2] = q.z;
        const V3 e = sub(q, load3(pts1, i));
        wgt[i] = par / (sqrt(dot(e, e)) + par);
      }
    }
  }
  if (t < 16) {
    const double ident = (t % 5 == 0) ? 1.0 : 0.0;
    out_T[t] = sh.bad ? ident : (t < 12 ? sh.T[t] : ident);
  }
  if (t == 16) out_meta[0] = sh.bad;
}

const double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
const int32_t kFlagged = 1;

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

size_t imf_robust_transform_workspace_bytes(int64_t n) {
  if (n <= (int64_t)kRtThreads * kRtRows) return 0;
  return align256((size_t)n * 24) + align256((size_t)n * 8);
}

int imf_robust_transform(const double *pts0, const double *pts1, const double *weight, int64_t n, double *out_T,
                         int32_t *out_meta, void *workspace, size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(out_T && out_meta, "imf_robust_transform: null output pointer");
  IMF_REQUIRE(n >= 0 && n < (1ll << 30), "imf_robust_transform: n=%lld", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {                                        // nothing to fit: the flag and the identity, no kernel
    IMF_CHECK_HIP(hipMemcpyAsync(out_T, kIdentity, sizeof(kIdentity), hipMemcpyHostToDevice, st));
    IMF_CHECK_HIP(hipMemcpyAsync(out_meta, &kFlagged, sizeof(kFlagged), hipMemcpyHostToDevice, st));
    return IMF_OK;
  }
  IMF_REQUIRE(pts0 && pts1, "imf_robust_transform: null pointer");
  const size_t need = imf_robust_transform_workspace_bytes(n);
  if (need == 0) {
    k_robust_transform<true><<<1, kRtThreads, 0, st>>>(pts0, pts1, weight, n, nullptr, nullptr, out_T, out_meta);
  } else {
    IMF_REQUIRE(workspace, "imf_robust_transform: n=%lld needs a workspace", (long long)n);
    IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "imf_robust_transform: workspace must be 256-byte aligned");
    IMF_REQUIRE(workspace_bytes >= need, "imf_robust_transform: workspace %zu < %zu", workspace_bytes, need);
    double *cur = (double *)workspace;
    double *wgt = (double *)((char *)workspace + align256((size_t)n * 24));
    k_robust_transform<false><<<1, kRtThreads, 0, st>>>(pts0, pts1, weight, n, cur, wgt, out_T, out_meta);
  }
  IMF_CHECK_LAUNCH("imf_robust_transform");
  return IMF_OK;
}

}  // extern "C"
