// Fragment fusion: depth frames -> sparse truncated signed distance volume -> surface points (imfnet_amd/fuse.py,
// python -m imfnet_amd.fuse_fragments).
//
// Reference being replaced: data/fuse_fragments_3DMatch.py:47-96 builds every fragment with Open3D 0.12
// `ScalableTSDFVolume(voxel_length = tsdf_cubic_size / 512, sdf_trunc = 0.04, RGB8)`, `integrate(rgbd, intrinsic,
// inv(pose_cam2world))` per frame with a valid pose, then `extract_point_cloud()`.  Restated here as pinned ([RECALLED]
// from Open3D's ScalableTSDFVolume / UniformTSDFVolume; no Open3D to check against):
//   volume units of 16^3 voxels, unit_length = 16 voxel_length, keyed by floor(point / unit_length)
//   allocate: every 4th depth pixel of every 4th row (d = raw / depth_scale as float32, raw != 0, d <= depth_trunc) is
//     back-projected, p_cam = ((u - cx) d / fx, (v - cy) d / fy, d), p = cam2world . p_cam; the unit of p and its
//     neighbours within reach = ceil(sdf_trunc / unit_length) units per axis are opened
//   integrate, per opened unit, per voxel (sample position p = (16 unit + local + lattice_offset) voxel_length), per frame
//   IN FRAME ORDER:
//     (x, y, z) = world2cam . p;            skip z <= 0
//     uf = fx x / z + cx + 0.5, vf = fy y / z + cy + 0.5;   skip unless 0 <= uf < width and 0 <= vf < height
//     u = (int)uf, v = (int)vf;  raw = depth[v][u];         skip raw == 0
//     d = (float)raw / (float)depth_scale;                  skip d > depth_trunc
//     sdf = (d - z) * || ((u - cx) / fx, (v - cy) / fy, 1) ||;   skip sdf <= -sdf_trunc
//     new = (float)min(1, sdf / sdf_trunc)
//     tsdf = (tsdf * w + new) / (w + 1);  w = w + 1         (float32, as the stored values)
//   extract: every voxel with w != 0, tsdf < 0.98, tsdf != 0 and each of its +x, +y, +z neighbours (in the next unit
//     where the voxel is on the unit's face) with the same conditions and f0 f1 < 0 gives one point on that edge:
//     p0 + voxel_length |f0| / (|f0| + |f1|) along the axis.
// Geometry is fp64, tsdf and weight are float32.  Contraction into fused multiply-adds is switched off for this file
// so that the arithmetic above is the arithmetic that runs (tests/tsdf_restate.py states it in NumPy).
// Colour (imf_tsdf_integrate_rgb / imf_tsdf_extract_rgb; upstream's volume is RGB8 and integrates the colour frame with
// the depth frame), pinned as the depth rule is ([RECALLED] from UniformTSDFVolume; tests/tsdf_color_restate.py in NumPy):
//   a colour image uint8 [H][W][3] = R, G, B comes beside every depth image.  Exactly when a frame updates a voxel's tsdf
//   (every skip above has passed), with the same pixel (u, v) and w = the weight BEFORE this frame's increment, per channel:
//     c[k] = (c[k] * w + (float)rgb[v][u][k]) / (w + 1)          float32 on the 0..255 scale, one __fdiv_rn, no contraction
//   so a constant colour stays exactly that colour, and frames fed in several calls give the bits of one call.
//   extract: the point between the samples lo and hi gets, with t = |f_lo| / (|f_lo| + |f_hi|) as its position uses it,
//     c = c_lo + t * (c_hi - c_lo) per channel in fp64, uint8 = floor(c + 0.5) clamped to [0, 255] (tsdf_shared.h:
//     edge_color).  Both ends have w != 0, so both have a colour.
//   Open3D keeps the colour as three doubles per voxel; here three float32, like the tsdf beside them.
//   The colour state is a buffer of its own, float32 [rows, 3, 4096]: per unit one plane of 4096 per channel, so that a
//   wavefront's voxels read and write consecutive dwords, and `voxels` keeps its [rows, 4096, 2] for every other consumer.
//   Colour is a compile-time switch of k_tsdf_integrate and of k_tsdf_extract's write pass: the depth-only instantiations
//   are the code they were, the coloured ones share every line of the projection and the scans, and leave the same
//   (tsdf, weight) and the same points bit for bit.
// Changed against Open3D, on purpose: a frame is integrated into EVERY opened unit it sees, not only into the units its
// own stride-4 samples opened (one thread owns a voxel and walks the frames; a unit list per frame would add a
// second indirection for a difference of a few free-space voxels); colour as float32; no normals.
//
// Device design.  The unit table is the library's open-addressing table of 16-byte imf_slot entries (common.h: the same
// slot hash and double-hashing step), key = the biased unit coordinate with z in the high field, so that ascending keys
// are ascending (z, y, x).  allocate: one thread per sampled pixel inserts its (2 reach + 1)^3 units (integer atomics
// only); the occupied slots are collected and every unit's place in the sorted list is its rank, counted against all
// other keys through LDS tiles (10^4 units: 10^8 integer compares, no sort passes, no dependence on the collection
// order); the rank is written back as the slot's value.  integrate: one workgroup of 256 threads per unit, 16 voxels
// per thread (x fastest, so a wavefront's voxels project to neighbouring pixels), 8 bytes of state per voxel read and
// written once per call.  Each workgroup first tests its unit's bounding sphere against every frame's frustum
// (behind the camera, beyond depth_trunc + sdf_trunc, outside one of the four side planes) into an LDS bit mask: a
// frame whose bit is clear would have been skipped by every voxel of the unit, so the skip changes no result.  The
// world -> camera matrices are read with wave-uniform addresses.  No floating-point atomics and a fixed frame order:
// two runs are bit-identical, and frames fed in several calls give the bits of one call.
// PRECONDITION of integrate: every world2cam is rigid, or holds a NaN (the frame is then skipped by every voxel).  The cull
// measures the unit's bounding sphere in the camera's frame with the radius it has in the volume's frame, widened by a
// relative 1e-6; that covers a rotation block whose singular values lie within 1e-6 of 1 (float32-rounded poses are at
// about 1e-7) and nothing beyond: under a pose with scale the voxels of partly visible units are silently lost.
// imfnet_amd/fuse.py refuses poses beyond half that margin (RIGID_TOL); a caller of the raw entry points owes the same.
// extract: a count pass per
// unit, one exclusive scan over the units, a write pass that repeats the count with a workgroup scan per 256 voxels,
// so the output order is (unit, voxel = (z * 16 + y) * 16 + x, axis).  No workgroup waits for another one.
#include "common.h"
#include "tsdf_shared.h"

#pragma clang fp contract(off)

namespace imf {
namespace {

__device__ __forceinline__ void unit_of_key(uint64_t k, int &x, int &y, int &z) {
  x = (int)(k & 0x3FFFF) - kCoordLim;
  y = (int)((k >> kCoordBits) & 0x3FFFF) - kCoordLim;
  z = (int)((k >> (2 * kCoordBits)) & 0x3FFFF) - kCoordLim;
}

// hash_insert with an end: at most one pass over the table, and no new key once the unit list is full
__device__ __forceinline__ void unit_insert(imf_slot *tab, uint32_t capmask, uint64_t key, int32_t *meta, int unit_cap) {
  uint32_t s = hash_slot(key, 0, capmask);
  uint32_t step = 0;
  for (uint32_t probes = 0; probes <= capmask; ++probes) {
    unsigned long long cur = __atomic_load_n(reinterpret_cast<unsigned long long *>(&tab[s].key), __ATOMIC_RELAXED);
    if (cur == key) return;
    if (cur == kEmptyKey) {
      if (__atomic_load_n(&meta[0], __ATOMIC_RELAXED) >= unit_cap) break;
      cur = atomicCAS(reinterpret_cast<unsigned long long *>(&tab[s].key), (unsigned long long)kEmptyKey,
                      (unsigned long long)key);
      if (cur == kEmptyKey) {
        atomicAdd(&meta[0], 1);
        return;
      }
      if (cur == key) return;
    }
    if (!step) step = hash_step(key);
    s = (s + step) & capmask;
  }
  atomicOr(&meta[1], kFlagCapacity);
}

__global__ __launch_bounds__(256) void k_tsdf_reset(imf_slot *tab, int64_t cap, int32_t *meta) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) meta[0] = meta[1] = 0;
  if (i < cap) reinterpret_cast<uint4 *>(tab)[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u);
}

// one thread per sampled pixel (frame, row / stride, column / stride)
__global__ __launch_bounds__(256) void k_tsdf_touch(const uint16_t *__restrict__ depth, int F, const double *__restrict__ c2w,
                                                    TsdfP P, int stride, int reach, imf_slot *tab, uint32_t capmask,
                                                    int32_t *meta, int unit_cap) {
  const int sw = (P.W + stride - 1) / stride, sh = (P.H + stride - 1) / stride;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)F * sh * sw) return;
  const int f = (int)(i / ((int64_t)sh * sw)), r = (int)(i % ((int64_t)sh * sw));
  const int v = (r / sw) * stride, u = (r % sw) * stride;
  const uint16_t raw = depth[((int64_t)f * P.H + v) * P.W + u];
  if (raw == 0) return;
  const double d = (double)__fdiv_rn((float)raw, P.scale);
  if (d > P.dtrunc) return;
  const double xc = ((double)u - P.cx) * d / P.fx, yc = ((double)v - P.cy) * d / P.fy;
  const double *M = c2w + 12 * f;
  const double ul = (double)kUnitRes * P.vl;
  const double q[3] = {floor((M[0] * xc + M[1] * yc + M[2] * d + M[3]) / ul), floor((M[4] * xc + M[5] * yc + M[6] * d + M[7]) / ul),
                       floor((M[8] * xc + M[9] * yc + M[10] * d + M[11]) / ul)};
  const double lim = (double)(kCoordLim - 1 - reach);
  if (!(q[0] >= -lim && q[0] < lim && q[1] >= -lim && q[1] < lim && q[2] >= -lim && q[2] < lim)) {   // NaN too
    atomicOr(&meta[1], kFlagRange);
    return;
  }
  const int x = (int)q[0], y = (int)q[1], z = (int)q[2];
  for (int dz = -reach; dz <= reach; ++dz)
    for (int dy = -reach; dy <= reach; ++dy)
      for (int dx = -reach; dx <= reach; ++dx) unit_insert(tab, capmask, unit_key(x + dx, y + dy, z + dz), meta, unit_cap);
}

__global__ __launch_bounds__(256) void k_tsdf_collect(const imf_slot *__restrict__ tab, int64_t cap, int32_t *meta, int unit_cap,
                                                      uint64_t *__restrict__ keys, int32_t *__restrict__ slot_of,
                                                      int32_t *n_listed) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cap) return;
  const uint64_t k = tab[s].key;
  if (k == kEmptyKey) return;
  const int i = atomicAdd(n_listed, 1);
  if (i >= unit_cap) {
    atomicOr(&meta[1], kFlagCapacity);
    return;
  }
  keys[i] = k;
  slot_of[i] = (int32_t)s;
}

// the place of every unit in the ascending list = the number of smaller keys
__global__ __launch_bounds__(256) void k_tsdf_rank(const uint64_t *__restrict__ keys, const int32_t *__restrict__ slot_of,
                                                   const int32_t *__restrict__ n_listed, int unit_cap, imf_slot *tab,
                                                   int32_t *__restrict__ units) {
  __shared__ uint64_t tile[256];
  const int n = min(*n_listed, unit_cap);
  const int i0 = blockIdx.x * 256, t = threadIdx.x, i = i0 + t;
  if (i0 >= n) return;
  const uint64_t mine = i < n ? keys[i] : 0;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    __syncthreads();
    tile[t] = j0 + t < n ? keys[j0 + t] : kEmptyKey;
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < 256; ++j) rank += tile[j] < mine ? 1 : 0;
  }
  if (i >= n) return;
  int x, y, z;
  unit_of_key(mine, x, y, z);
  units[3 * rank + 0] = x; units[3 * rank + 1] = y; units[3 * rank + 2] = z;
  tab[slot_of[i]].val = rank;
}

// true when no voxel of the unit (bounding sphere: centre w, radius r) can pass the per-voxel tests of this frame
__device__ __forceinline__ bool frame_misses_unit(const double *M, const TsdfP &P, double wx, double wy, double wz, double r) {
  const double x = M[0] * wx + M[1] * wy + M[2] * wz + M[3], y = M[4] * wx + M[5] * wy + M[6] * wz + M[7],
               z = M[8] * wx + M[9] * wy + M[10] * wz + M[11];
  if (!(z + r > 0.0)) return true;                       // behind the camera (a NaN pose too: every voxel skips it)
  if (z - r > P.dtrunc + P.trunc) return true;           // sdf <= depth_trunc - z < -sdf_trunc for every voxel
  const double ax0 = (-P.cx - 0.5) / P.fx, ax1 = ((double)P.W - P.cx - 0.5) / P.fx;   // x / z at uf = 0 and uf = W
  const double ay0 = (-P.cy - 0.5) / P.fy, ay1 = ((double)P.H - P.cy - 0.5) / P.fy;
  if ((x - ax0 * z) / sqrt(1.0 + ax0 * ax0) < -r) return true;
  if ((x - ax1 * z) / sqrt(1.0 + ax1 * ax1) > r) return true;
  if ((y - ay0 * z) / sqrt(1.0 + ay0 * ay0) < -r) return true;
  if ((y - ay1 * z) / sqrt(1.0 + ay1 * ay1) > r) return true;
  return false;
}

// COLOR = true also folds the colour frames into the colour planes, at exactly the updates of the tsdf
template <bool COLOR>
__global__ __launch_bounds__(kTsdfThreads) void k_tsdf_integrate(const uint16_t *__restrict__ depth, int F,
                                                                const double *__restrict__ w2c, TsdfP P,
                                                                const int32_t *__restrict__ units,
                                                                const int32_t *__restrict__ n_units,
                                                                float2 *__restrict__ vox,
                                                                const uint8_t *__restrict__ color,
                                                                float *__restrict__ col) {
  const int u = blockIdx.x;
  if (u >= n_units[0]) return;
  __shared__ uint32_t act[kTsdfMaxFrames / 32];
  const int t = threadIdx.x;
  const int ux = units[3 * u], uy = units[3 * u + 1], uz = units[3 * u + 2];
  for (int i = t; i < (F + 31) / 32; i += kTsdfThreads) act[i] = 0u;
  __syncthreads();
  {
    const double mid = 0.5 * (kUnitRes - 1) + P.off;      // the samples span local 0 .. 15
    const double wx = ((double)(kUnitRes * ux) + mid) * P.vl, wy = ((double)(kUnitRes * uy) + mid) * P.vl,
                 wz = ((double)(kUnitRes * uz) + mid) * P.vl;
    const double r = 0.5 * (kUnitRes - 1) * P.vl * 1.7320508075688772 * (1.0 + 1e-6) + 1e-9;
    for (int f = t; f < F; f += kTsdfThreads)
      if (!frame_misses_unit(w2c + 12 * f, P, wx, wy, wz, r)) atomicOr(&act[f >> 5], 1u << (f & 31));
  }
  __syncthreads();
  const int lx = t & 15, ly = t >> 4;
  const double px = ((double)(kUnitRes * ux + lx) + P.off) * P.vl, py = ((double)(kUnitRes * uy + ly) + P.off) * P.vl;
  for (int lz = 0; lz < kUnitRes; ++lz) {
    const double pz = ((double)(kUnitRes * uz + lz) + P.off) * P.vl;
    const int64_t at = (int64_t)u * kUnitVoxels + lz * 256 + t;
    float2 s = vox[at];                                   // x = tsdf, y = weight
    float c[3] = {0.f, 0.f, 0.f};
    if constexpr (COLOR) {
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = col[color_index(u, k, lz * 256 + t)];
    }
    for (int f = 0; f < F; ++f) {
      if (!((act[f >> 5] >> (f & 31)) & 1u)) continue;    // wave-uniform
      const double *M = w2c + 12 * f;
      const double z = M[8] * px + M[9] * py + M[10] * pz + M[11];
      if (!(z > 0.0)) continue;
      const double x = M[0] * px + M[1] * py + M[2] * pz + M[3], y = M[4] * px + M[5] * py + M[6] * pz + M[7];
      const double uf = P.fx * x / z + P.cx + 0.5, vf = P.fy * y / z + P.cy + 0.5;
      if (!(uf >= 0.0 && uf < (double)P.W && vf >= 0.0 && vf < (double)P.H)) continue;
      const int iu = (int)uf, iv = (int)vf;
      const uint16_t raw = depth[((int64_t)f * P.H + iv) * P.W + iu];
      if (raw == 0) continue;
      const double d = (double)__fdiv_rn((float)raw, P.scale);
      if (d > P.dtrunc) continue;
      const double a = ((double)iu - P.cx) / P.fx, b = ((double)iv - P.cy) / P.fy;
      const double sdf = (d - z) * sqrt(a * a + b * b + 1.0);
      if (sdf <= -P.trunc) continue;
      const float nw = (float)fmin(1.0, sdf / P.trunc);
      s.x = __fdiv_rn(s.x * s.y + nw, s.y + 1.0f);
      if constexpr (COLOR) {                                // the same pixel, the weight before its increment
        const uint8_t *px = color + (((int64_t)f * P.H + iv) * P.W + iu) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = __fdiv_rn(c[k] * s.y + (float)px[k], s.y + 1.0f);
      }
      s.y = s.y + 1.0f;
    }
    vox[at] = s;
    if constexpr (COLOR) {
#pragma unroll
      for (int k = 0; k < 3; ++k) col[color_index(u, k, lz * 256 + t)] = c[k];
    }
  }
}

__device__ __forceinline__ bool tsdf_surface_side(float2 s) { return s.y != 0.0f && s.x < 0.98f && s.x != 0.0f; }

// WRITE = false: unit_cnt[u] = points of unit u.  WRITE = true: the points, at offsets[u] + their place in the unit.
// COLOR (with WRITE): row i of out_rgb = the colour of row i of out.
template <bool WRITE, bool COLOR>
__global__ __launch_bounds__(kTsdfThreads) void k_tsdf_extract(const float2 *__restrict__ vox, const int32_t *__restrict__ units,
                                                              const int32_t *__restrict__ n_units, int max_units,
                                                              const imf_slot *__restrict__ tab, uint32_t capmask, TsdfP P,
                                                              int32_t *__restrict__ unit_cnt,
                                                              const int64_t *__restrict__ offsets, int64_t capacity,
                                                              double *__restrict__ out,
                                                              const float *__restrict__ col,
                                                              uint8_t *__restrict__ out_rgb) {
  const int u = blockIdx.x, n = min(n_units[0], max_units);
  if (u >= n) return;
  if (WRITE && offsets[n] > capacity) return;
  __shared__ int nb[3];
  __shared__ int wsum[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int ux = units[3 * u], uy = units[3 * u + 1], uz = units[3 * u + 2];
  if (t < 3) {
    const int r = hash_find(tab, capmask, unit_key(ux + (t == 0), uy + (t == 1), uz + (t == 2)), 0);
    nb[t] = r >= 0 && r < n ? r : -1;
  }
  __syncthreads();
  const float2 *mine = vox + (int64_t)u * kUnitVoxels;
  const int lx = t & 15, ly = t >> 4;
  int64_t run = WRITE ? offsets[u] : 0;
  int total = 0;
  for (int lz = 0; lz < kUnitRes; ++lz) {
    const int l = lz * 256 + t;
    const float2 s0 = mine[l];
    bool cross[3] = {false, false, false};
    float f1[3] = {0.f, 0.f, 0.f};
    if (tsdf_surface_side(s0)) {
      const int in_unit[3] = {lx < 15, ly < 15, lz < 15};
      const int step[3] = {1, 16, 256};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float2 *src = in_unit[a] ? mine : (nb[a] >= 0 ? vox + (int64_t)nb[a] * kUnitVoxels : nullptr);
        if (!src) continue;
        const float2 s1 = src[in_unit[a] ? l + step[a] : l - 15 * step[a]];
        if (tsdf_surface_side(s1) && s0.x * s1.x < 0.0f) {
          cross[a] = true;
          f1[a] = s1.x;
        }
      }
    }
    const int c = (int)cross[0] + (int)cross[1] + (int)cross[2];
    if (!WRITE) {
      total += c;
      continue;
    }
    int incl = c;                                          // workgroup exclusive scan of c, in voxel order
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    __syncthreads();
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wv) before += wsum[w];
      all += wsum[w];
    }
    int64_t row = run + before + incl - c;
    run += all;
    if (c) {
      const double p0[3] = {((double)(kUnitRes * ux + lx) + P.off) * P.vl, ((double)(kUnitRes * uy + ly) + P.off) * P.vl,
                            ((double)(kUnitRes * uz + lz) + P.off) * P.vl};
      const double r0 = fabs((double)s0.x);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (!cross[a] || row >= capacity) continue;
        const double r1 = fabs((double)f1[a]);
        const double tt = r0 / (r0 + r1);
        double p[3] = {p0[0], p0[1], p0[2]};
        p[a] = p0[a] + P.vl * tt;
        out[3 * row + 0] = p[0]; out[3 * row + 1] = p[1]; out[3 * row + 2] = p[2];
        if constexpr (COLOR) {                              // hi: the sample the crossing was found at (above)
          const int step_a = a == 0 ? 1 : (a == 1 ? 16 : 256);
          const bool in_a = a == 0 ? lx < 15 : (a == 1 ? ly < 15 : lz < 15);
          edge_color(col, u, l, in_a ? u : nb[a], in_a ? l + step_a : l - 15 * step_a, tt, out_rgb + 3 * row);
        }
        ++row;
      }
    }
  }
  if (!WRITE) {
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
    if (lane == 0) wsum[wv] = total;
    __syncthreads();
    if (t == 0) unit_cnt[u] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  }
}

}  // namespace
}  // namespace imf

using namespace imf;

// imf_tsdf_integrate and imf_tsdf_integrate_rgb: one set of checks, the kernel with or without the colour planes
static int tsdf_integrate(const char *what, bool rgb, const uint16_t *depth, const uint8_t *color, int n_frames,
                          const double *world2cam, const imf_tsdf_params *params, const int32_t *units,
                          const int32_t *n_units, int64_t max_units, float *voxels, float *colors, void *stream) {
  TsdfP P;
  int rc = tsdf_params(what, params, P);
  if (rc) return rc;
  IMF_REQUIRE(n_frames >= 0 && n_frames <= kTsdfMaxFrames, "%s: n_frames=%d", what, n_frames);
  IMF_REQUIRE(max_units >= 0 && max_units <= kTsdfMaxUnits, "%s: max_units=%lld", what, (long long)max_units);
  if (n_frames == 0 || max_units == 0) return IMF_OK;
  IMF_REQUIRE(depth && world2cam && units && n_units && voxels, "%s: null pointer", what);
  IMF_REQUIRE(((uintptr_t)voxels & 7) == 0, "%s: voxels must be 8-byte aligned", what);
  float2 *vox = reinterpret_cast<float2 *>(voxels);
  if (rgb) {
    IMF_REQUIRE(color, "%s: color is NULL", what);
    IMF_REQUIRE(colors, "%s: colors is NULL", what);
    IMF_REQUIRE(((uintptr_t)colors & 3) == 0, "%s: colors must be 4-byte aligned", what);
    k_tsdf_integrate<true><<<(unsigned)max_units, kTsdfThreads, 0, (hipStream_t)stream>>>(depth, n_frames, world2cam, P, units,
                                                                                         n_units, vox, color, colors);
  } else {
    k_tsdf_integrate<false><<<(unsigned)max_units, kTsdfThreads, 0, (hipStream_t)stream>>>(depth, n_frames, world2cam, P, units,
                                                                                          n_units, vox, nullptr, nullptr);
  }
  IMF_CHECK_LAUNCH(what);
  return IMF_OK;
}

// imf_tsdf_extract and imf_tsdf_extract_rgb: the same count pass and scan, the write pass with or without the colours
static int tsdf_extract(const char *what, bool rgb, const float *voxels, const float *colors, const int32_t *units,
                        const int32_t *n_units, int64_t max_units, const imf_slot *table, int64_t table_capacity,
                        const imf_tsdf_params *params, double *out, uint8_t *out_rgb, int64_t capacity, int64_t *out_n,
                        void *workspace, size_t workspace_bytes, void *stream) {
  TsdfP P;
  int rc = tsdf_params(what, params, P);
  if (rc) return rc;
  IMF_REQUIRE(voxels && units && n_units && table && out_n && workspace, "%s: null pointer", what);
  IMF_REQUIRE(max_units >= 1 && max_units <= kTsdfMaxUnits, "%s: max_units=%lld", what, (long long)max_units);
  IMF_REQUIRE(is_pow2(table_capacity) && table_capacity <= (1ll << 31), "%s: table_capacity=%lld", what,
              (long long)table_capacity);
  IMF_REQUIRE(capacity >= 0 && (out || capacity == 0), "%s: capacity=%lld with out=%p", what, (long long)capacity,
              (const void *)out);
  if (rgb) {
    IMF_REQUIRE(colors, "%s: colors is NULL", what);
    IMF_REQUIRE(out_rgb || capacity == 0, "%s: out_rgb is NULL with capacity=%lld", what, (long long)capacity);
    IMF_REQUIRE(((uintptr_t)colors & 3) == 0, "%s: colors must be 4-byte aligned", what);
  }
  IMF_REQUIRE(((uintptr_t)voxels & 7) == 0, "%s: voxels must be 8-byte aligned", what);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", what);
  IMF_REQUIRE(workspace_bytes >= imf_tsdf_extract_workspace_bytes(max_units), "%s: workspace %zu < %zu", what, workspace_bytes,
              imf_tsdf_extract_workspace_bytes(max_units));
  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  int32_t *cnt = (int32_t *)ws;
  int64_t *offsets = (int64_t *)(ws + align256((size_t)max_units * 4));
  const uint32_t capmask = (uint32_t)(table_capacity - 1);
  const float2 *vox = reinterpret_cast<const float2 *>(voxels);
  const unsigned grid = (unsigned)max_units;
  k_tsdf_extract<false, false><<<grid, kTsdfThreads, 0, st>>>(vox, units, n_units, (int)max_units, table, capmask, P, cnt,
                                                              nullptr, 0, nullptr, nullptr, nullptr);
  k_tsdf_scan<<<1, 1024, 0, st>>>(cnt, n_units, (int)max_units, offsets, out_n);
  if (capacity > 0 && rgb)
    k_tsdf_extract<true, true><<<grid, kTsdfThreads, 0, st>>>(vox, units, n_units, (int)max_units, table, capmask, P, nullptr,
                                                              offsets, capacity, out, colors, out_rgb);
  else if (capacity > 0)
    k_tsdf_extract<true, false><<<grid, kTsdfThreads, 0, st>>>(vox, units, n_units, (int)max_units, table, capmask, P, nullptr,
                                                               offsets, capacity, out, nullptr, nullptr);
  IMF_CHECK_LAUNCH(what);
  return IMF_OK;
}

extern "C" {

size_t imf_tsdf_allocate_workspace_bytes(int64_t unit_capacity) {
  if (unit_capacity < 1 || unit_capacity > kTsdfMaxUnits) return 0;
  return align256((size_t)unit_capacity * 8) + align256((size_t)unit_capacity * 4) + 256;
}

int imf_tsdf_allocate(const uint16_t *depth, int n_frames, const double *cam2world, const imf_tsdf_params *params,
                      int reset, imf_slot *table, int64_t table_capacity, int32_t *units, int64_t unit_capacity,
                      int32_t *n_units, void *workspace, size_t workspace_bytes, void *stream) {
  TsdfP P;
  int rc = tsdf_params("imf_tsdf_allocate", params, P);
  if (rc) return rc;
  IMF_REQUIRE(table && units && n_units && workspace, "imf_tsdf_allocate: null pointer");
  IMF_REQUIRE(n_frames >= 0 && n_frames <= kTsdfMaxFrames && (n_frames == 0 || (depth && cam2world)),
              "imf_tsdf_allocate: n_frames=%d", n_frames);
  IMF_REQUIRE(unit_capacity >= 1 && unit_capacity <= kTsdfMaxUnits, "imf_tsdf_allocate: unit_capacity=%lld",
              (long long)unit_capacity);
  IMF_REQUIRE(is_pow2(table_capacity) && table_capacity >= 2 * unit_capacity && table_capacity <= (1ll << 31),
              "imf_tsdf_allocate: table_capacity=%lld for %lld units (use imf_hash_capacity)", (long long)table_capacity,
              (long long)unit_capacity);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "imf_tsdf_allocate: workspace must be 256-byte aligned");
  IMF_REQUIRE(workspace_bytes >= imf_tsdf_allocate_workspace_bytes(unit_capacity), "imf_tsdf_allocate: workspace %zu < %zu",
              workspace_bytes, imf_tsdf_allocate_workspace_bytes(unit_capacity));
  const double reach_d = ceil(P.trunc / (kUnitRes * P.vl));
  IMF_REQUIRE(reach_d >= 1.0 && reach_d <= (double)kTsdfMaxReach,
              "imf_tsdf_allocate: sdf_trunc=%g reaches %g units of %g m (at most %d)", P.trunc, reach_d, kUnitRes * P.vl,
              kTsdfMaxReach);
  const int reach = (int)reach_d, stride = 4;
  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  uint64_t *keys = (uint64_t *)ws;
  int32_t *slot_of = (int32_t *)(ws + align256((size_t)unit_capacity * 8));
  int32_t *n_listed = (int32_t *)(ws + align256((size_t)unit_capacity * 8) + align256((size_t)unit_capacity * 4));
  const uint32_t capmask = (uint32_t)(table_capacity - 1);
  if (reset) k_tsdf_reset<<<(unsigned)div_up(table_capacity, 256), 256, 0, st>>>(table, table_capacity, n_units);
  const int64_t samples = (int64_t)n_frames * div_up(P.H, stride) * div_up(P.W, stride);
  if (samples > 0)
    k_tsdf_touch<<<(unsigned)div_up(samples, 256), 256, 0, st>>>(depth, n_frames, cam2world, P, stride, reach, table, capmask,
                                                                 n_units, (int)unit_capacity);
  IMF_CHECK_HIP(hipMemsetAsync(n_listed, 0, sizeof(int32_t), st));
  k_tsdf_collect<<<(unsigned)div_up(table_capacity, 256), 256, 0, st>>>(table, table_capacity, n_units, (int)unit_capacity, keys,
                                                                        slot_of, n_listed);
  k_tsdf_rank<<<(unsigned)div_up(unit_capacity, 256), 256, 0, st>>>(keys, slot_of, n_listed, (int)unit_capacity, table, units);
  IMF_CHECK_LAUNCH("imf_tsdf_allocate");
  return IMF_OK;
}

int imf_tsdf_integrate(const uint16_t *depth, int n_frames, const double *world2cam, const imf_tsdf_params *params,
                       const int32_t *units, const int32_t *n_units, int64_t max_units, float *voxels, void *stream) {
  return tsdf_integrate("imf_tsdf_integrate", false, depth, nullptr, n_frames, world2cam, params, units, n_units, max_units,
                        voxels, nullptr, stream);
}

int imf_tsdf_integrate_rgb(const uint16_t *depth, const uint8_t *color, int n_frames, const double *world2cam,
                           const imf_tsdf_params *params, const int32_t *units, const int32_t *n_units, int64_t max_units,
                           float *voxels, float *colors, void *stream) {
  return tsdf_integrate("imf_tsdf_integrate_rgb", true, depth, color, n_frames, world2cam, params, units, n_units, max_units,
                        voxels, colors, stream);
}

size_t imf_tsdf_extract_workspace_bytes(int64_t max_units) {
  if (max_units < 1 || max_units > kTsdfMaxUnits) return 0;
  return align256((size_t)max_units * 4) + align256((size_t)(max_units + 1) * 8);
}

int imf_tsdf_extract(const float *voxels, const int32_t *units, const int32_t *n_units, int64_t max_units,
                     const imf_slot *table, int64_t table_capacity, const imf_tsdf_params *params, double *out,
                     int64_t capacity, int64_t *out_n, void *workspace, size_t workspace_bytes, void *stream) {
  return tsdf_extract("imf_tsdf_extract", false, voxels, nullptr, units, n_units, max_units, table, table_capacity, params, out,
                      nullptr, capacity, out_n, workspace, workspace_bytes, stream);
}

int imf_tsdf_extract_rgb(const float *voxels, const float *colors, const int32_t *units, const int32_t *n_units,
                         int64_t max_units, const imf_slot *table, int64_t table_capacity, const imf_tsdf_params *params,
                         double *out, uint8_t *out_rgb, int64_t capacity, int64_t *out_n, void *workspace,
                         size_t workspace_bytes, void *stream) {
  return tsdf_extract("imf_tsdf_extract_rgb", true, voxels, colors, units, n_units, max_units, table, table_capacity, params,
                      out, out_rgb, capacity, out_n, workspace, workspace_bytes, stream);
}

}  // extern "C"
