// Frame-to-frame RGB-D odometry: the image pyramids of a frame (imf_rgbd_prepare) and the coarse-to-fine hybrid fit of a
// source frame onto a target frame (imf_rgbd_odometry; imf_rgbd_odometry_stage exposes one stage to the tests).
//
// Reference being replaced: nothing upstream calls it; it is the step the reconstruction pipeline of Choi, Zhou, Koltun 2015
// puts in front of everything else, as Open3D ships it -- compute_rgbd_odometry with RGBDOdometryJacobianFromHybridTerm
// (Steinbruecker 2011; Park, Zhou, Koltun, ICCV 2017), restated ([RECALLED] from Open3D like the ICP rules of icp.hip and
// colored_icp.hip; no Open3D to check against).  The rules below are therefore the specification; tests/odometry_restate.py
// states them again in float64 NumPy.
//
// All arithmetic is fp64 without fused multiply-add, every operation in the order written, so the per-pixel quantities equal
// the restatement's bit for bit and only the sums differ by their order.
//
// Frame preparation.  depth uint16 [H, W], colour uint8 [H, W, 3], fx, fy, cx, cy, 1 <= levels <= 5; H and W divisible by
// 2^(levels - 1), the coarsest level at least 3 x 3.
//   I = (r + g + b) / 765            the integer sum first, then ONE division (imfnet_amd.matching.intensity's rule)
//   d = u16 / depth_scale            valid iff u16 > 0 and depth_min < d < depth_max; an invalid depth is stored as NaN
// per level l (level 0 is the input):
//   Is_l = the 3 x 3 Gaussian of I_l, separable: h = ((left + (mid + mid)) + right) / 4 along the row first, then the same
//          down the column of h; the border replicated
//   Sobel gradients of Is_l and of D_l at interior pixels, NaN on the one-pixel border; with the neighbourhood
//          a b c / d . f / g h i:  d/du = (((c - a) + ((f - d) + (f - d))) + (i - g)) / 8,
//                                  d/dv = (((g - a) + ((h - b) + (h - b))) + (i - c)) / 8
//   a depth gradient is NaN unless all nine depths are valid and each differs from the centre by less than depth_edge
//          (without this mask the gradients across a silhouette pull the coarse levels away from the answer)
//   I_{l+1} = ((a + b) + (c + d)) / 4 of the 2 x 2 quad of Is_l (a b the upper row)
//   D_{l+1} = ((a + b) + (c + d)) / count over the VALID pixels of the quad, invalid ones contributing 0; NaN when none is
//          (a quad that needed all four valid would leave 44 usable pixels at 40 x 30 under 2 % holes)
//   fx, fy halve; cx <- (cx - 0.5) / 2, cy likewise (pixel centres)
//
// One stage at a level; T maps source-camera coordinates into the target camera.  A pixel leaves the source through the
// source frame's intrinsics and enters the target through the target frame's (fx, fy, cx, cy below the projection and in the
// rows are the target's; the two are the same camera in a sequence).  For each source pixel (u, v) with valid d:
//   X = (((u - cx) d) / fx, ((v - cy) d) / fy, d),  X' = R X + t with every row ((r0 x + r1 y) + r2 z) + t;  z' > 0
//   ut = floor(((fx x') / z' + cx) + 0.5), vt likewise;  1 <= ut <= W - 2, 1 <= vt <= H - 2
//   the target at (ut, vt) has a valid depth and finite depth gradients;  |D_t - z'| < max_depth_diff (strict)
// Occlusion: a target pixel keeps the candidate of the smallest z' (compared in fp64), ties to the lowest source index
// v W + u: an integer atomic minimum on the bit pattern of the positive double, then one on the index among those that equal
// it -- exact and free of the order of arrival.  Every winner contributes two rows; with iz = 1 / z' and a gradient pair
// (gx, gy):  c0 = (gx fx) iz,  c1 = (gy fy) iz,  c2 = -((c0 x' + c1 y') iz) - own,
//   J = [-(z' c1) + y' c2,  z' c0 - x' c2,  -(y' c0) + x' c1,  c0, c1, c2]
//   photometric: the gradients of Is_t, own = 0, r_I = Is_t(ut, vt) - Is_s(u, v)
//   geometric:   the gradients of D_t,  own = 1, r_G = D_t(ut, vt) - z'
// (rotation first, the parametrisation of the update [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5]; tests/test_odometry_host.py checks the
// rows by central differences).  The 29 sums, each addend formed per winner with lambda = lambda_depth:
//   n;  lambda r_G^2 + (1 - lambda) r_I^2;  the 21 upper entries of lambda J_G^T J_G + (1 - lambda) J_I^T J_I;  the 6 of
//   lambda J_G r_G + (1 - lambda) J_I r_I.
// Solve A x = -b by the LDL^T of registration.h under icp.hip's singular rule; T <- update . T.  A stage with n < min_corr or
// a singular system has the identity update and raises bit 0 of the flags.
//
// The loop: levels from the coarsest to level 0, iterations[k] stages at the k-th coarsest, no early stop; one more stage at
// level 0 reports n, the cost, the 6 x 6 A as the information matrix (written exactly symmetric) and fitness = n / (valid
// source pixels at level 0); flag bit 1 ("lost") when that stage has n < min_corr or a singular A.
//
// Left out: Open3D's intensity normalisation between the two frames, bilinear sampling, loop closures between key frames and a
// per-fragment pose graph.
//
// Device design.  A frame is one device block: a 256-byte header (magic, H, W, levels, the intrinsics of every level) and six
// fp64 planes per level.  The entry points read the two headers back once, before the loop (the block is opaque to the
// caller, and a block prepared for another shape must be refused), then enqueue everything and never wait.  A stage is five
// steps: the winner table is cleared (all ones: the largest key, index -1), k_odo_depth (one thread per source pixel: the
// candidate, atomicMin of its z' bits), k_odo_index (atomicMin of the index where the bits equal the table's), k_odo_rows (the
// winners' addends; wavefront butterfly, then the four wavefronts of a workgroup in a fixed order, one fp64 row per
// workgroup, no atomics) and k_odo_fit (one workgroup: adds the rows in a fixed order, solves, updates T on the device).  The
// only atomics are those two integer minima: two calls give the same bits.
#include "common.h"
#include "registration.h"

namespace imf {
namespace {

constexpr uint64_t kFrameMagic = 0x314d524644424752ull;      // "RGBDFRM1"
constexpr int kMaxLevels = 5;
constexpr int kOdoThreads = 256;
constexpr int kOdoSums = 29;            // n, cost, upper A [21], b [6]
constexpr int kOdoRow = 30;             // + the workgroup's count of valid source pixels

struct FrameHeader {                     // the first 256 bytes of a frame block
  uint64_t magic;
  int32_t h, w, levels, pad;
  double K[kMaxLevels][4];               // fx, fy, cx, cy per level
};
static_assert(sizeof(FrameHeader) <= 256, "frame header");

struct Level {                           // one level of a prepared frame, by value
  const double *Is, *D, *Isx, *Isy, *Dx, *Dy;
  int h, w;
  double fx, fy, cx, cy;
};

bool shape_ok(int h, int w, int levels) {
  if (levels < 1 || levels > kMaxLevels || h < 3 || w < 3 || h > 16384 || w > 16384) return false;
  const int m = (1 << (levels - 1)) - 1;
  return !(h & m) && !(w & m) && (h >> (levels - 1)) >= 3 && (w >> (levels - 1)) >= 3;
}

size_t plane_bytes(int h, int w, int l) { return align256((size_t)(h >> l) * (size_t)(w >> l) * sizeof(double)); }

size_t frame_bytes(int h, int w, int levels) {
  if (!shape_ok(h, w, levels)) return 0;
  size_t p = 256;
  for (int l = 0; l < levels; ++l) p += 6 * plane_bytes(h, w, l);
  return p;
}

Level level_of(const void *frame, const FrameHeader &hd, int l) {
  size_t p = 256;
  for (int k = 0; k < l; ++k) p += 6 * plane_bytes(hd.h, hd.w, k);
  const size_t pb = plane_bytes(hd.h, hd.w, l);
  const char *b = (const char *)frame + p;
  Level L;
  L.Is = (const double *)b;
  L.D = (const double *)(b + pb);
  L.Isx = (const double *)(b + 2 * pb);
  L.Isy = (const double *)(b + 3 * pb);
  L.Dx = (const double *)(b + 4 * pb);
  L.Dy = (const double *)(b + 5 * pb);
  L.h = hd.h >> l;
  L.w = hd.w >> l;
  L.fx = hd.K[l][0]; L.fy = hd.K[l][1]; L.cx = hd.K[l][2]; L.cy = hd.K[l][3];
  return L;
}

__global__ void k_frame_header(FrameHeader hd, FrameHeader *out) { *out = hd; }

// ---- preparation ---------------------------------------------------------------------------------------------------------
// I_l and D_l of a level: level 0 from the input images, a coarser level from the quads of the finer level's Is and D
struct Source {
  const uint16_t *depth;
  const uint8_t *color;
  const double *Is, *D;                  // the finer level (w2 = its width)
  int w2;
  double depth_scale, depth_min, depth_max;
};

template <bool kFirst>
__device__ __forceinline__ double intensity_at(const Source &s, int v, int u, int w) {
#pragma clang fp contract(off)
  if constexpr (kFirst) {
    const uint8_t *c = s.color + 3 * ((size_t)v * w + u);
    return (double)((int)c[0] + (int)c[1] + (int)c[2]) / 765.0;
  } else {
    const double *p = s.Is + (size_t)(2 * v) * s.w2 + 2 * u;
    return ((p[0] + p[1]) + (p[s.w2] + p[s.w2 + 1])) / 4.0;
  }
}

template <bool kFirst>
__device__ __forceinline__ double depth_at(const Source &s, int v, int u, int w) {
#pragma clang fp contract(off)
  if constexpr (kFirst) {
    const uint16_t raw = s.depth[(size_t)v * w + u];
    const double d = (double)raw / s.depth_scale;
    return raw > 0 && s.depth_min < d && d < s.depth_max ? d : __builtin_nan("");
  } else {
    const double *p = s.D + (size_t)(2 * v) * s.w2 + 2 * u;
    const double q[4] = {p[0], p[1], p[s.w2], p[s.w2 + 1]};
    double t[4], cnt = 0.0;
    for (int k = 0; k < 4; ++k) {
      const bool ok = q[k] == q[k];
      t[k] = ok ? q[k] : 0.0;
      cnt += ok ? 1.0 : 0.0;
    }
    return cnt > 0.0 ? ((t[0] + t[1]) + (t[2] + t[3])) / cnt : __builtin_nan("");
  }
}

template <bool kFirst>
__global__ __launch_bounds__(256) void k_prep_smooth(Source s, int h, int w, double *__restrict__ Is, double *__restrict__ D) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)h * w) return;
  const int v = (int)(i / w), u = (int)(i % w);
  const int ul = max(u - 1, 0), ur = min(u + 1, w - 1);
  double hrow[3];
  for (int k = 0; k < 3; ++k) {
    const int vv = min(max(v - 1 + k, 0), h - 1);
    const double m = intensity_at<kFirst>(s, vv, u, w);
    hrow[k] = ((intensity_at<kFirst>(s, vv, ul, w) + (m + m)) + intensity_at<kFirst>(s, vv, ur, w)) / 4.0;
  }
  Is[i] = ((hrow[0] + (hrow[1] + hrow[1])) + hrow[2]) / 4.0;
  D[i] = depth_at<kFirst>(s, v, u, w);
}

__global__ __launch_bounds__(256) void k_prep_grad(const double *__restrict__ Is, const double *__restrict__ D, int h, int w,
                                                   double depth_edge, double *__restrict__ Isx, double *__restrict__ Isy,
                                                   double *__restrict__ Dx, double *__restrict__ Dy) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)h * w) return;
  const int v = (int)(i / w), u = (int)(i % w);
  const double nan = __builtin_nan("");
  double ix = nan, iy = nan, dx = nan, dy = nan;
  if (v >= 1 && v <= h - 2 && u >= 1 && u <= w - 2) {
    double p[9], q[9];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const size_t j = (size_t)(v - 1 + a) * w + (u - 1 + b);
        p[3 * a + b] = Is[j];
        q[3 * a + b] = D[j];
      }
    ix = (((p[2] - p[0]) + ((p[5] - p[3]) + (p[5] - p[3]))) + (p[8] - p[6])) / 8.0;
    iy = (((p[6] - p[0]) + ((p[7] - p[1]) + (p[7] - p[1]))) + (p[8] - p[2])) / 8.0;
    bool ok = true;
    for (int k = 0; k < 9; ++k) ok = ok && fabs(q[k] - q[4]) < depth_edge;       // a NaN fails
    if (ok) {
      dx = (((q[2] - q[0]) + ((q[5] - q[3]) + (q[5] - q[3]))) + (q[8] - q[6])) / 8.0;
      dy = (((q[6] - q[0]) + ((q[7] - q[1]) + (q[7] - q[1]))) + (q[8] - q[2])) / 8.0;
    }
  }
  Isx[i] = ix; Isy[i] = iy; Dx[i] = dx; Dy[i] = dy;
}

// ---- a stage -------------------------------------------------------------------------------------------------------------
struct OdoState {
  double T[16];                          // source camera -> target camera, row-major
  int32_t flags, stages;
};

struct OdoInit {
  double T[16];
};

__global__ void k_odo_start(OdoInit init, OdoState *st) {
  for (int k = 0; k < 16; ++k) st->T[k] = init.T[k];
  st->flags = st->stages = 0;
}

struct Candidate {
  double x, y, z;                        // X'
  int t;                                 // target pixel vt W + ut, or -1
};

// the candidate of source pixel i under T: the rules of the file header up to the depth test.  The three kernels of a stage
// each form it again (three passes of fp64 divisions) instead of storing it: the same code on the same inputs gives the same
// bits, and a stage stays free of per-pixel scratch.
__device__ __forceinline__ Candidate candidate(const Level &s, const Level &t, const double *__restrict__ T, int64_t i,
                                               double max_depth_diff, bool &valid) {
#pragma clang fp contract(off)
  Candidate c{0.0, 0.0, 0.0, -1};
  const double d = s.D[i];
  valid = d == d;
  if (!valid) return c;
  const int v = (int)(i / s.w), u = (int)(i % s.w);
  const double x = (((double)u - s.cx) * d) / s.fx, y = (((double)v - s.cy) * d) / s.fy;
  c.x = ((T[0] * x + T[1] * y) + T[2] * d) + T[3];
  c.y = ((T[4] * x + T[5] * y) + T[6] * d) + T[7];
  c.z = ((T[8] * x + T[9] * y) + T[10] * d) + T[11];
  if (!(c.z > 0.0)) return c;
  const double pu = ((t.fx * c.x) / c.z + t.cx) + 0.5, pv = ((t.fy * c.y) / c.z + t.cy) + 0.5;
  if (!(pu >= 1.0 && pu < (double)(t.w - 1) && pv >= 1.0 && pv < (double)(t.h - 1))) return c;      // a NaN fails
  const int tp = (int)floor(pv) * t.w + (int)floor(pu);
  const double dt = t.D[tp], gx = t.Dx[tp], gy = t.Dy[tp];
  if (!(dt == dt) || !(fabs(gx) <= 1.79769313486231570815e308) || !(fabs(gy) <= 1.79769313486231570815e308)) return c;
  if (!(fabs(dt - c.z) < max_depth_diff)) return c;
  c.t = tp;
  return c;
}

__global__ __launch_bounds__(kOdoThreads) void k_odo_depth(Level s, Level t, const OdoState *__restrict__ st,
                                                           const double *__restrict__ T_fixed, double max_depth_diff,
                                                           unsigned long long *__restrict__ zmin) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)s.h * s.w) return;
  bool valid;
  const Candidate c = candidate(s, t, T_fixed ? T_fixed : st->T, i, max_depth_diff, valid);
  if (c.t >= 0) atomicMin(zmin + c.t, (unsigned long long)__double_as_longlong(c.z));       // z' > 0: the bits order as z'
}

__global__ __launch_bounds__(kOdoThreads) void k_odo_index(Level s, Level t, const OdoState *__restrict__ st,
                                                           const double *__restrict__ T_fixed, double max_depth_diff,
                                                           const unsigned long long *__restrict__ zmin,
                                                           unsigned int *__restrict__ winner) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)s.h * s.w) return;
  bool valid;
  const Candidate c = candidate(s, t, T_fixed ? T_fixed : st->T, i, max_depth_diff, valid);
  if (c.t >= 0 && zmin[c.t] == (unsigned long long)__double_as_longlong(c.z)) atomicMin(winner + c.t, (unsigned int)i);
}

__device__ __forceinline__ void jacobian_row(double gx, double gy, const Level &t, const Candidate &c, double own,
                                             double J[6]) {
#pragma clang fp contract(off)
  const double iz = 1.0 / c.z;
  const double c0 = (gx * t.fx) * iz, c1 = (gy * t.fy) * iz;
  const double c2 = -((c0 * c.x + c1 * c.y) * iz) - own;
  J[0] = -(c.z * c1) + c.y * c2;
  J[1] = c.z * c0 - c.x * c2;
  J[2] = -(c.y * c0) + c.x * c1;
  J[3] = c0; J[4] = c1; J[5] = c2;
}

__global__ __launch_bounds__(kOdoThreads) void k_odo_rows(Level s, Level t, const OdoState *__restrict__ st,
                                                          const double *__restrict__ T_fixed, double max_depth_diff,
                                                          double lambda, const unsigned int *__restrict__ winner,
                                                          double *__restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double lds[kOdoThreads / 64][kOdoRow];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double a[kOdoRow];
#pragma unroll
  for (int k = 0; k < kOdoRow; ++k) a[k] = 0.0;
  if (i < (int64_t)s.h * s.w) {
    bool valid;
    const Candidate c = candidate(s, t, T_fixed ? T_fixed : st->T, i, max_depth_diff, valid);
    a[kOdoSums] = valid ? 1.0 : 0.0;
    if (c.t >= 0 && winner[c.t] == (unsigned int)i) {
      const double rI = t.Is[c.t] - s.Is[i], rG = t.D[c.t] - c.z;
      double JI[6], JG[6];
      jacobian_row(t.Isx[c.t], t.Isy[c.t], t, c, 0.0, JI);
      jacobian_row(t.Dx[c.t], t.Dy[c.t], t, c, 1.0, JG);
      const double wg = lambda, wi = 1.0 - lambda;
      a[0] = 1.0;
      a[1] = wg * (rG * rG) + wi * (rI * rI);
      int k = 2;
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = p; q < 6; ++q) a[k++] = wg * (JG[p] * JG[q]) + wi * (JI[p] * JI[q]);
#pragma unroll
      for (int p = 0; p < 6; ++p) a[23 + p] = wg * (JG[p] * rG) + wi * (JI[p] * rI);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kOdoRow; ++k) {
    const double v = wave_sum(a[k]);
    if (lane == 0) lds[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kOdoRow)
    partial[(int64_t)blockIdx.x * kOdoRow + threadIdx.x] =
        ((lds[0][threadIdx.x] + lds[1][threadIdx.x]) + lds[2][threadIdx.x]) + lds[3][threadIdx.x];
}

// one workgroup per stage.  final: nothing moves, the outputs are written.  out_sums (the test surface): the 29 sums.
__global__ __launch_bounds__(kOdoThreads) void k_odo_fit(const double *__restrict__ partial, int n_blocks, int min_corr,
                                                         int final, OdoState *st, double *out_T, double *out_info,
                                                         double *out_stats, int32_t *out_meta, double *out_sums) {
  __shared__ double lds[kOdoThreads];
  __shared__ double sums[kOdoRow];
  const int t = threadIdx.x;
  for (int k = 0; k < kOdoRow; ++k) {
    double a = 0.0;
    for (int b = t; b < n_blocks; b += kOdoThreads) a += partial[(int64_t)b * kOdoRow + k];   // ascending per thread
    lds[t] = a;
    __syncthreads();
    for (int o = kOdoThreads / 2; o > 0; o >>= 1) {     // fixed tree
      if (t < o) lds[t] += lds[t + o];
      __syncthreads();
    }
    if (t == 0) sums[k] = lds[0];
    __syncthreads();
  }
  if (t != 0) return;
  if (out_sums) {
    for (int k = 0; k < kOdoSums; ++k) out_sums[k] = sums[k];
    return;
  }
  const int n = (int)sums[0];
  double A[6][6], b[6], x[6];
  int k = 2;
  for (int p = 0; p < 6; ++p)
    for (int q = p; q < 6; ++q) A[p][q] = A[q][p] = sums[k++];
  for (int p = 0; p < 6; ++p) b[p] = sums[23 + p];
  const bool ok = n >= min_corr && solve_plane_system(A, b, x);
  st->stages += 1;
  if (!final) {
    if (!ok) {
      st->flags |= 1;
      return;
    }
    double U[12], Tn[12];
    update_from_solution(x, U);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c)
        Tn[4 * r + c] = U[4 * r + 0] * st->T[c] + U[4 * r + 1] * st->T[4 + c] + U[4 * r + 2] * st->T[8 + c] +
                        U[4 * r + 3] * st->T[12 + c];
    for (int j = 0; j < 12; ++j) st->T[j] = Tn[j];
    return;
  }
  for (int j = 0; j < 16; ++j) out_T[j] = st->T[j];
  for (int p = 0; p < 6; ++p)
    for (int q = 0; q < 6; ++q) out_info[6 * p + q] = A[p][q];
  const double n_valid = sums[kOdoSums];
  out_stats[0] = n_valid > 0.0 ? sums[0] / n_valid : 0.0;
  out_stats[1] = sums[1];
  out_meta[0] = n;
  out_meta[1] = st->flags | (ok ? 0 : 2);
  out_meta[2] = st->stages;
  out_meta[3] = (int32_t)n_valid;
}

// workspace: the z' table and the winner table of level 0's size, the workgroup rows, the state
struct OdoLayout {
  size_t zmin, winner, partial, state, total;
};
OdoLayout odo_layout(int h, int w) {
  const size_t px = (size_t)h * w;
  OdoLayout L;
  size_t p = 0;
  L.zmin = p;    p += align256(px * 8);
  L.winner = p;  p += align256(px * 4);
  L.partial = p; p += align256((size_t)div_up((int64_t)px, kOdoThreads) * kOdoRow * 8);
  L.state = p;   p += align256(sizeof(OdoState));
  L.total = p;
  return L;
}

// the two headers, read back once: both prepared, of one shape (each keeps its own intrinsics)
int read_headers(const char *name, const void *src, const void *dst, FrameHeader &hs, FrameHeader &hd, hipStream_t st) {
  IMF_CHECK_HIP(hipMemcpyAsync(&hs, src, sizeof(FrameHeader), hipMemcpyDeviceToHost, st));
  IMF_CHECK_HIP(hipMemcpyAsync(&hd, dst, sizeof(FrameHeader), hipMemcpyDeviceToHost, st));
  IMF_CHECK_HIP(hipStreamSynchronize(st));
  IMF_REQUIRE(hs.magic == kFrameMagic && hd.magic == kFrameMagic && shape_ok(hs.h, hs.w, hs.levels),
              "%s: not a frame block of imf_rgbd_prepare", name);
  IMF_REQUIRE(hs.h == hd.h && hs.w == hd.w && hs.levels == hd.levels,
              "%s: the frames were prepared for different shapes: %d x %d, %d levels and %d x %d, %d levels", name, hs.h,
              hs.w, hs.levels, hd.h, hd.w, hd.levels);
  return IMF_OK;
}

// clear, depth, index, rows of one stage at level views s, t (the fit follows)
int enqueue_stage(const Level &s, const Level &t, const OdoState *state, const double *T_fixed, double max_depth_diff,
                  double lambda, char *ws, const OdoLayout &lay, hipStream_t st) {
  const size_t px = (size_t)s.h * s.w;
  const unsigned nb = (unsigned)div_up((int64_t)px, kOdoThreads);
  unsigned long long *zmin = (unsigned long long *)(ws + lay.zmin);
  unsigned int *winner = (unsigned int *)(ws + lay.winner);
  IMF_CHECK_HIP(hipMemsetAsync(zmin, 0xFF, px * 8, st));
  IMF_CHECK_HIP(hipMemsetAsync(winner, 0xFF, px * 4, st));
  k_odo_depth<<<nb, kOdoThreads, 0, st>>>(s, t, state, T_fixed, max_depth_diff, zmin);
  k_odo_index<<<nb, kOdoThreads, 0, st>>>(s, t, state, T_fixed, max_depth_diff, zmin, winner);
  k_odo_rows<<<nb, kOdoThreads, 0, st>>>(s, t, state, T_fixed, max_depth_diff, lambda, winner,
                                         (double *)(ws + lay.partial));
  return IMF_OK;
}

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

size_t imf_rgbd_frame_bytes(int h, int w, int levels) { return frame_bytes(h, w, levels); }

int imf_rgbd_prepare(const uint16_t *depth_u16, const uint8_t *color_u8, int h, int w, double fx, double fy, double cx,
                     double cy, double depth_scale, double depth_min, double depth_max, double depth_edge, int levels,
                     void *frame, size_t frame_bytes_, void *stream) {
  IMF_REQUIRE(depth_u16, "imf_rgbd_prepare: null pointer (depth_u16)");
  IMF_REQUIRE(color_u8, "imf_rgbd_prepare: null pointer (color_u8)");
  IMF_REQUIRE(frame, "imf_rgbd_prepare: null pointer (frame)");
  IMF_REQUIRE(levels >= 1 && levels <= kMaxLevels, "imf_rgbd_prepare: levels=%d, expected 1..%d", levels, kMaxLevels);
  IMF_REQUIRE(shape_ok(h, w, levels),
              "imf_rgbd_prepare: %d x %d with %d levels: both must be divisible by 2^(levels-1), the coarsest level at least 3 x 3",
              h, w, levels);
  IMF_REQUIRE(fx > 0.0 && fy > 0.0 && fx < 1e9 && fy < 1e9 && fabs(cx) < 1e9 && fabs(cy) < 1e9,
              "imf_rgbd_prepare: intrinsics fx=%g fy=%g cx=%g cy=%g", fx, fy, cx, cy);                      // NaN too
  IMF_REQUIRE(depth_scale > 0.0 && depth_scale < 1e9, "imf_rgbd_prepare: depth_scale=%g", depth_scale);
  IMF_REQUIRE(depth_min >= 0.0 && depth_max > depth_min, "imf_rgbd_prepare: depth_min=%g depth_max=%g", depth_min, depth_max);
  IMF_REQUIRE(depth_edge > 0.0, "imf_rgbd_prepare: depth_edge=%g", depth_edge);
  IMF_REQUIRE(((uintptr_t)frame & 255) == 0, "imf_rgbd_prepare: frame must be 256-byte aligned");
  IMF_REQUIRE(frame_bytes_ >= frame_bytes(h, w, levels), "imf_rgbd_prepare: frame %zu < %zu", frame_bytes_,
              frame_bytes(h, w, levels));
  hipStream_t st = (hipStream_t)stream;
  FrameHeader hd{};
  hd.magic = kFrameMagic;
  hd.h = h; hd.w = w; hd.levels = levels;
  for (int l = 0; l < levels; ++l) {
    hd.K[l][0] = fx; hd.K[l][1] = fy; hd.K[l][2] = cx; hd.K[l][3] = cy;
    fx = fx / 2.0; fy = fy / 2.0; cx = (cx - 0.5) / 2.0; cy = (cy - 0.5) / 2.0;
  }
  k_frame_header<<<1, 1, 0, st>>>(hd, (FrameHeader *)frame);
  Source s{depth_u16, color_u8, nullptr, nullptr, 0, depth_scale, depth_min, depth_max};
  for (int l = 0; l < levels; ++l) {
    const Level L = level_of(frame, hd, l);
    const unsigned nb = (unsigned)div_up((int64_t)L.h * L.w, 256);
    if (l == 0)
      k_prep_smooth<true><<<nb, 256, 0, st>>>(s, L.h, L.w, (double *)L.Is, (double *)L.D);
    else
      k_prep_smooth<false><<<nb, 256, 0, st>>>(s, L.h, L.w, (double *)L.Is, (double *)L.D);
    k_prep_grad<<<nb, 256, 0, st>>>(L.Is, L.D, L.h, L.w, depth_edge, (double *)L.Isx, (double *)L.Isy, (double *)L.Dx,
                                    (double *)L.Dy);
    s.Is = L.Is; s.D = L.D; s.w2 = L.w;
  }
  IMF_CHECK_LAUNCH("imf_rgbd_prepare");
  return IMF_OK;
}

size_t imf_rgbd_odometry_workspace_bytes(int h, int w, int levels) {
  return shape_ok(h, w, levels) ? odo_layout(h, w).total : 0;
}

int imf_rgbd_odometry(const void *src_frame, const void *dst_frame, const double *init_host, const int *iterations,
                      int n_iterations, double max_depth_diff, double lambda_depth, int min_corr, double *out_T,
                      double *out_info, double *out_stats, int32_t *out_meta, void *workspace, size_t workspace_bytes,
                      void *stream) {
  IMF_REQUIRE(src_frame, "imf_rgbd_odometry: null pointer (src_frame)");
  IMF_REQUIRE(dst_frame, "imf_rgbd_odometry: null pointer (dst_frame)");
  IMF_REQUIRE(iterations, "imf_rgbd_odometry: null pointer (iterations)");
  IMF_REQUIRE(out_T && out_info && out_stats && out_meta, "imf_rgbd_odometry: null pointer (outputs)");
  IMF_REQUIRE(workspace, "imf_rgbd_odometry: null pointer (workspace)");
  IMF_REQUIRE(n_iterations >= 1 && n_iterations <= kMaxLevels, "imf_rgbd_odometry: levels=%d, expected 1..%d", n_iterations,
              kMaxLevels);
  for (int k = 0; k < n_iterations; ++k)
    IMF_REQUIRE(iterations[k] >= 1 && iterations[k] <= 10000, "imf_rgbd_odometry: iterations[%d]=%d, expected 1..10000", k,
                iterations[k]);
  IMF_REQUIRE(max_depth_diff > 0.0, "imf_rgbd_odometry: max_depth_diff=%g", max_depth_diff);                  // NaN too
  IMF_REQUIRE(lambda_depth >= 0.0 && lambda_depth <= 1.0, "imf_rgbd_odometry: lambda_depth=%g, expected 0..1", lambda_depth);
  IMF_REQUIRE(min_corr >= 0, "imf_rgbd_odometry: min_corr=%d", min_corr);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "imf_rgbd_odometry: workspace must be 256-byte aligned");
  IMF_REQUIRE(workspace_bytes > 0, "imf_rgbd_odometry: workspace 0 bytes");
  hipStream_t st = (hipStream_t)stream;
  FrameHeader hd, hdst;
  int rc = read_headers("imf_rgbd_odometry", src_frame, dst_frame, hd, hdst, st);
  if (rc) return rc;
  IMF_REQUIRE(n_iterations == hd.levels, "imf_rgbd_odometry: %d iteration counts for frames of %d levels", n_iterations,
              hd.levels);
  const OdoLayout lay = odo_layout(hd.h, hd.w);
  IMF_REQUIRE(workspace_bytes >= lay.total, "imf_rgbd_odometry: workspace %zu < %zu", workspace_bytes, lay.total);
  char *ws = (char *)workspace;
  OdoState *state = (OdoState *)(ws + lay.state);
  OdoInit init;
  for (int k = 0; k < 16; ++k) init.T[k] = init_host ? init_host[k] : (k % 5 == 0 ? 1.0 : 0.0);
  k_odo_start<<<1, 1, 0, st>>>(init, state);
  for (int k = 0; k <= n_iterations; ++k) {              // the last round is the reporting stage at level 0
    const int final = k == n_iterations, l = final ? 0 : hd.levels - 1 - k;
    const Level s = level_of(src_frame, hd, l), t = level_of(dst_frame, hdst, l);
    const int nb = (int)div_up((int64_t)s.h * s.w, kOdoThreads);
    for (int it = 0, n_it = final ? 1 : iterations[k]; it < n_it; ++it) {
      rc = enqueue_stage(s, t, state, nullptr, max_depth_diff, lambda_depth, ws, lay, st);
      if (rc) return rc;
      k_odo_fit<<<1, kOdoThreads, 0, st>>>((const double *)(ws + lay.partial), nb, min_corr, final, state, out_T, out_info,
                                           out_stats, out_meta, nullptr);
    }
  }
  IMF_CHECK_LAUNCH("imf_rgbd_odometry");
  return IMF_OK;
}

int imf_rgbd_odometry_stage(const void *src_frame, const void *dst_frame, int level, const double *T_dev,
                            double max_depth_diff, double lambda_depth, int32_t *out_winner, double *out_sums,
                            void *workspace, size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(src_frame && dst_frame && T_dev && out_winner && out_sums && workspace, "imf_rgbd_odometry_stage: null pointer");
  IMF_REQUIRE(max_depth_diff > 0.0, "imf_rgbd_odometry_stage: max_depth_diff=%g", max_depth_diff);
  IMF_REQUIRE(lambda_depth >= 0.0 && lambda_depth <= 1.0, "imf_rgbd_odometry_stage: lambda_depth=%g, expected 0..1",
              lambda_depth);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "imf_rgbd_odometry_stage: workspace must be 256-byte aligned");
  IMF_REQUIRE(workspace_bytes > 0, "imf_rgbd_odometry_stage: workspace 0 bytes");
  hipStream_t st = (hipStream_t)stream;
  FrameHeader hd, hdst;
  int rc = read_headers("imf_rgbd_odometry_stage", src_frame, dst_frame, hd, hdst, st);
  if (rc) return rc;
  IMF_REQUIRE(level >= 0 && level < hd.levels, "imf_rgbd_odometry_stage: level=%d of %d", level, hd.levels);
  const OdoLayout lay = odo_layout(hd.h, hd.w);
  IMF_REQUIRE(workspace_bytes >= lay.total, "imf_rgbd_odometry_stage: workspace %zu < %zu", workspace_bytes, lay.total);
  char *ws = (char *)workspace;
  const Level s = level_of(src_frame, hd, level), t = level_of(dst_frame, hdst, level);
  const int nb = (int)div_up((int64_t)s.h * s.w, kOdoThreads);
  rc = enqueue_stage(s, t, nullptr, T_dev, max_depth_diff, lambda_depth, ws, lay, st);
  if (rc) return rc;
  k_odo_fit<<<1, kOdoThreads, 0, st>>>((const double *)(ws + lay.partial), nb, 0, 0, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, out_sums);
  IMF_CHECK_LAUNCH("imf_rgbd_odometry_stage");
  IMF_CHECK_HIP(hipMemcpyAsync(out_winner, ws + lay.winner, (size_t)s.h * s.w * 4, hipMemcpyDeviceToDevice, st));
  return IMF_OK;
}

}  // extern "C"
