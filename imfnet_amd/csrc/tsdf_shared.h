// What the TSDF entry points share (tsdf.hip: allocate / integrate / extract; tsdf_mesh.hip: the triangle mesh): the
// constants of the volume, the kernels' parameter block and its checks, the unit key of the table, and the one-workgroup
// exclusive scan over the units that turns per-unit counts into output offsets.  The rules are documented at the head of
// tsdf.hip.  Everything here has internal linkage: each translation unit that includes it gets its own copy.
#pragma once
#include "common.h"

namespace imf {
namespace {

constexpr int kUnitRes = 16;                      // voxels per unit edge
constexpr int kUnitVoxels = kUnitRes * kUnitRes * kUnitRes;
constexpr int kTsdfThreads = 256;
constexpr int kTsdfMaxFrames = 4096;
constexpr int kTsdfMaxSide = 8192;                // image height / width
constexpr int64_t kTsdfMaxUnits = 1ll << 22;
constexpr int kTsdfMaxReach = 4;
constexpr int kFlagRange = 1, kFlagCapacity = 2;

struct TsdfP {
  double fx, fy, cx, cy, vl, trunc, dtrunc, off;
  float scale;
  int H, W;
};

__device__ __forceinline__ uint64_t unit_key(int x, int y, int z) {
  return ((uint64_t)(uint32_t)(z + kCoordLim) << (2 * kCoordBits)) | ((uint64_t)(uint32_t)(y + kCoordLim) << kCoordBits) |
         (uint64_t)(uint32_t)(x + kCoordLim);
}

// Colour state: float32 [rows, 3, 4096], one plane of 4096 per channel and unit, so that the thread-per-voxel walks read
// and write consecutive dwords per channel.  The index of channel k of a voxel:
__device__ __forceinline__ int64_t color_index(int64_t row, int k, int voxel) {
  return (row * 3 + k) * kUnitVoxels + voxel;
}

// The colour of a surface point between the samples lo and hi (row, voxel), t = |f_lo| / (|f_lo| + |f_hi|) as the position
// uses it: c = c_lo + t (c_hi - c_lo) in fp64 without contraction, uint8 = floor(c + 0.5) clamped to [0, 255] (a NaN: 0).
__device__ __forceinline__ void edge_color(const float *__restrict__ col, int64_t row_lo, int vox_lo, int64_t row_hi, int vox_hi,
                                           double t, uint8_t *__restrict__ out) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double lo = (double)col[color_index(row_lo, k, vox_lo)], hi = (double)col[color_index(row_hi, k, vox_hi)];
    const double q = floor(lo + t * (hi - lo) + 0.5);
    out[k] = (uint8_t)(int)(!(q >= 0.0) ? 0.0 : (q > 255.0 ? 255.0 : q));
  }
}

// one workgroup: exclusive scan of the per-unit counts in unit order -> offsets[0..n], *out_n = offsets[n]
__global__ __launch_bounds__(1024) void k_tsdf_scan(const int32_t *__restrict__ cnt, const int32_t *__restrict__ n_units,
                                                    int max_units, int64_t *__restrict__ offsets, int64_t *__restrict__ out_n) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t n = min(n_units[0], max_units);
  const int64_t per = (n + 1023) / 1024, b = min(n, t * per), e = min(n, b + per);
  int64_t sum = 0;
  for (int64_t i = b; i < e; ++i) sum += cnt[i];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {                   // Hillis-Steele inclusive scan
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
    *out_n = part[1023];
  }
}

// the checks every entry point shares; fills the kernels' parameter block
int tsdf_params(const char *what, const imf_tsdf_params *p, TsdfP &P) {
  IMF_REQUIRE(p, "%s: null parameters", what);
  IMF_REQUIRE(p->height >= 1 && p->height <= kTsdfMaxSide && p->width >= 1 && p->width <= kTsdfMaxSide,
              "%s: image %d x %d", what, p->height, p->width);
  IMF_REQUIRE(p->fx > 0.0 && p->fy > 0.0 && p->fx < 1e9 && p->fy < 1e9 && fabs(p->cx) < 1e9 && fabs(p->cy) < 1e9,
              "%s: intrinsics fx=%g fy=%g cx=%g cy=%g", what, p->fx, p->fy, p->cx, p->cy);
  IMF_REQUIRE(p->voxel_length > 0.0 && p->voxel_length < 1e3 && p->sdf_trunc > 0.0 && p->sdf_trunc < 1e6,
              "%s: voxel_length=%g sdf_trunc=%g", what, p->voxel_length, p->sdf_trunc);
  IMF_REQUIRE(p->depth_scale > 0.0 && p->depth_scale < 1e9 && p->depth_trunc > 0.0 && p->depth_trunc < 1e9,
              "%s: depth_scale=%g depth_trunc=%g", what, p->depth_scale, p->depth_trunc);
  IMF_REQUIRE(p->lattice_offset >= 0.0 && p->lattice_offset < 1.0, "%s: lattice_offset=%g", what, p->lattice_offset);
  P.fx = p->fx; P.fy = p->fy; P.cx = p->cx; P.cy = p->cy;
  P.vl = p->voxel_length; P.trunc = p->sdf_trunc; P.dtrunc = p->depth_trunc; P.off = p->lattice_offset;
  P.scale = (float)p->depth_scale;
  P.H = p->height; P.W = p->width;
  return IMF_OK;
}

bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace
}  // namespace imf
