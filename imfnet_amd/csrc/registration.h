// Rigid registration maths shared by RANSAC (ransac.hip) and ICP (icp.hip): fp64 3-vectors, the
// Umeyama / Kabsch fit without scale, and the application of a row-major 3x4 [R | t].
#pragma once
#include "common.h"

namespace imf {

struct V3 {
  double x, y, z;
};
__host__ __device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__host__ __device__ inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__host__ __device__ inline V3 load3(const double *p, long long i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

// Rotation and translation from the means and the cross-covariance B = H = sum (s - ms)(d - md)^T of a
// correspondence set (B is overwritten).  Shared by RANSAC's per-hypothesis fit and ICP's per-iteration fit, and by
// imf_host_rigid_fit on the CPU.  R is a proper rotation (orthonormal, det +1) for EVERY B: rank 3 and rank 2 are the
// SVD answer; rank 1 and rank 0 follow the rank rule below, a chosen, deterministic completion
// where the residual does not determine R.
__host__ __device__ inline void rigid_from_cov(V3 ms, V3 md, double B[3][3], double *T) {
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 12; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int r = 0; r < 3; ++r) {
          al += B[r][p] * B[r][p];
          be += B[r][q] * B[r][q];
          ga += B[r][p] * B[r][q];
        }
        off = fmax(off, fabs(ga) / (sqrt(al * be) + 1e-300));
        if (fabs(ga) <= 1e-300) continue;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
        for (int r = 0; r < 3; ++r) {
          const double bp = B[r][p], bq = B[r][q];
          B[r][p] = c * bp - sn * bq;
          B[r][q] = sn * bp + c * bq;
          const double vp = V[r][p], vq = V[r][q];
          V[r][p] = c * vp - sn * vq;
          V[r][q] = sn * vp + c * vq;
        }
      }
    if (off < 1e-15) break;
  }
  double sg[3];
  for (int k = 0; k < 3; ++k) sg[k] = sqrt(B[0][k] * B[0][k] + B[1][k] * B[1][k] + B[2][k] * B[2][k]);
  // The rank rule: a column counts as zero when its norm is at most 2^-52 of the largest one (below one rounding of
  // the entries B was formed from); such a column is never divided by its own norm.
  const double tiny = fmax(sg[0], fmax(sg[1], sg[2])) * 0x1p-52;
  const int rank = (sg[0] > tiny) + (sg[1] > tiny) + (sg[2] > tiny);
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};   // rank 0: the fit is the translation md - ms
  if (rank >= 2) {
    int m = 0;
    if (sg[1] < sg[m]) m = 1;
    if (sg[2] < sg[m]) m = 2;
    const int a = (m + 1) % 3, b = (m + 2) % 3;         // (a, b, m) is a cyclic permutation
    V3 ua{B[0][a], B[1][a], B[2][a]}, ub{B[0][b], B[1][b], B[2][b]};
    const double na = 1.0 / sg[a], nb = 1.0 / sg[b];    // both above `tiny`: m is the only column that may be zero
    ua = {ua.x * na, ua.y * na, ua.z * na};
    ub = {ub.x * nb, ub.y * nb, ub.z * nb};
    const V3 um = cross(ua, ub);                        // det[ua ub um] = +1
    const V3 va{V[0][a], V[1][a], V[2][a]}, vb{V[0][b], V[1][b], V[2][b]};
    const V3 vm = cross(va, vb);                        // V is a rotation: equals its third column
    const double U3[3][3] = {{ua.x, ub.x, um.x}, {ua.y, ub.y, um.y}, {ua.z, ub.z, um.z}};
    const double V3m[3][3] = {{va.x, vb.x, vm.x}, {va.y, vb.y, vm.y}, {va.z, vb.z, vm.z}};
    // H = sum a b^T maps the roles: columns of B live in the "d" space? B = H V with H = A^T-like sum over
    // a (rows) x b (cols): B columns are combinations of the a-space (rows index a).  R takes s to d:
    // R = Vd Us^T with Us = left vectors (a-space = source), Vd = right vectors (b-space = destination).
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[r][c] = V3m[r][0] * U3[c][0] + V3m[r][1] * U3[c][1] + V3m[r][2] * U3[c][2];
  } else if (rank == 1) {
    // One direction: u (source) = the live column of B, v (target) = its column of V.  Every rotation that takes u
    // to v has the same residual; the one of the least angle is chosen, written as two half turns, about u and then
    // about the bisector h = u + v: R = (2 h h^T / h.h - I)(2 u u^T / u.u - I).  u = v gives I.  When u and v are
    // opposite (|u + v|^2 <= 2^-40) the bisector is gone and R is the half turn about the coordinate axis e_j of the
    // smallest |u_j| (the lowest j on ties) made perpendicular to u.
    int k = 0;
    if (sg[1] > sg[k]) k = 1;
    if (sg[2] > sg[k]) k = 2;
    const double nk = 1.0 / sg[k];
    const double u[3] = {B[0][k] * nk, B[1][k] * nk, B[2][k] * nk}, v[3] = {V[0][k], V[1][k], V[2][k]};
    const double h[3] = {u[0] + v[0], u[1] + v[1], u[2] + v[2]};
    const double uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2], hh = h[0] * h[0] + h[1] * h[1] + h[2] * h[2];
    if (hh > 0x1p-40) {
      const double hu = h[0] * u[0] + h[1] * u[1] + h[2] * u[2];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
          R[r][c] = (r == c ? 1.0 : 0.0) - 2.0 * u[r] * u[c] / uu - 2.0 * h[r] * h[c] / hh +
                    4.0 * hu * h[r] * u[c] / (hh * uu);
    } else {
      int j = 0;
      if (fabs(u[1]) < fabs(u[j])) j = 1;
      if (fabs(u[2]) < fabs(u[j])) j = 2;
      double ax[3] = {-u[j] / uu * u[0], -u[j] / uu * u[1], -u[j] / uu * u[2]};
      ax[j] += 1.0;
      const double aa = ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = 2.0 * ax[r] * ax[c] / aa - (r == c ? 1.0 : 0.0);
    }
  }
  const double msv[3] = {ms.x, ms.y, ms.z}, mdv[3] = {md.x, md.y, md.z};
  for (int r = 0; r < 3; ++r) {
    T[4 * r + 0] = R[r][0];
    T[4 * r + 1] = R[r][1];
    T[4 * r + 2] = R[r][2];
    T[4 * r + 3] = mdv[r] - (R[r][0] * msv[0] + R[r][1] * msv[1] + R[r][2] * msv[2]);
  }
}

// Rigid fit dst ~ R src + t of n <= 4 pairs (Kabsch / Umeyama without scale): H = sum (s - ms)(d - md)^T
// = U S V^T, R = V diag(1, 1, det(V U^T)) U^T.  One-sided Jacobi on the columns of H; the column of
// the smallest singular value is replaced by the cross product of the other two, which is exactly the
// determinant correction.  T = row-major 3x4 [R | t].
__host__ __device__ inline void rigid_fit(const V3 *s, const V3 *d, int n, double *T) {
  V3 ms{0, 0, 0}, md{0, 0, 0};
  for (int i = 0; i < n; ++i) {
    ms.x += s[i].x; ms.y += s[i].y; ms.z += s[i].z;
    md.x += d[i].x; md.y += d[i].y; md.z += d[i].z;
  }
  const double inv = 1.0 / n;
  ms = {ms.x * inv, ms.y * inv, ms.z * inv};
  md = {md.x * inv, md.y * inv, md.z * inv};
  double B[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // B = H V (starts as H), column k = B[.][k]
  for (int i = 0; i < n; ++i) {
    const V3 a = sub(s[i], ms), b = sub(d[i], md);
    const double av[3] = {a.x, a.y, a.z}, bv[3] = {b.x, b.y, b.z};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) B[r][c] += av[r] * bv[c];
  }
  rigid_from_cov(ms, md, B, T);
}

__host__ __device__ inline V3 apply(const double *T, V3 p) {
  return {T[0] * p.x + T[1] * p.y + T[2] * p.z + T[3], T[4] * p.x + T[5] * p.y + T[6] * p.z + T[7],
          T[8] * p.x + T[9] * p.y + T[10] * p.z + T[11]};
}

// x of A x = -b for the symmetric 6x6 A by LDL^T without pivoting; false under the singular rule of icp.hip's header: a
// pivot <= 1e-12 times the largest diagonal entry, or NaN.  Shared by the point-to-plane / coloured ICP fit (icp.hip) and
// the RGB-D odometry fit (odometry.hip).
__device__ inline bool solve_plane_system(const double A[6][6], const double b[6], double x[6]) {
  double L[6][6], D[6], big = 0.0;
  for (int k = 0; k < 6; ++k) big = fmax(big, A[k][k]);
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
    if (!(d > 1e-12 * big)) return false;               // zero, negative, tiny or NaN
    D[j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k] * D[k];
      L[i][j] = s / d;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {                          // L y = -b
    double s = -b[i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s;
  }
  for (int i = 5; i >= 0; --i) {                         // L^T x = D^-1 y
    double s = y[i] / D[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
    x[i] = s;
  }
  return true;
}

// The update of that solution, row-major 3x4: [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5]
__device__ inline void update_from_solution(const double x[6], double U[12]) {
  const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
  U[0] = cg * cb; U[1] = cg * sb * sa - sg * ca; U[2] = cg * sb * ca + sg * sa;  U[3] = x[3];   // Rz Ry Rx
  U[4] = sg * cb; U[5] = sg * sb * sa + cg * ca; U[6] = sg * sb * ca - cg * sa;  U[7] = x[4];
  U[8] = -sb;     U[9] = cb * sa;                U[10] = cb * ca;                U[11] = x[5];
}

}  // namespace imf
