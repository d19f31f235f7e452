// The cell-CSR grid over a point set that the ICPs, the radius searches (icp.hip) and the k-NN normals (normals.hip)
// search.  The rules are documented at the head of icp.hip: cell = floor(x * inv_cell) with inv_cell = (1 - 1e-9) / edge,
// 18-bit keys per axis, targets one cell inside the key range, an out-of-range or NaN target raises the error flag.
// grid_nearest is the one correspondence rule of the ICPs and of the information matrix (information.hip); block_sum is
// their fixed-order workgroup sum.
// Everything here has internal linkage: each translation unit that includes it gets its own kernels.
#pragma once
#include "common.h"
#include "registration.h"

namespace imf {
namespace {

// cell-CSR grid over the target
struct Grid {
  imf_slot *tab;                        // key -> (val = first sorted row, pad = count) after the scan
  uint32_t capmask;
  int32_t *cnt;                         // [cap] points per slot, then the scatter cursor
  int32_t *cell_of;                     // [n_dst] slot of every target point
  double *xyz;                          // [n_dst, 3] target sorted by cell
  int32_t *idx;                         // [n_dst] original index of every sorted row
  double inv_cell;
};

__device__ __forceinline__ bool cell_of_point(V3 p, double inv_cell, int lim, int &x, int &y, int &z) {
  const double fx = floor(p.x * inv_cell), fy = floor(p.y * inv_cell), fz = floor(p.z * inv_cell);
  if (!(fx >= -lim && fx < lim && fy >= -lim && fy < lim && fz >= -lim && fz < lim)) return false;   // NaN too
  x = (int)fx; y = (int)fy; z = (int)fz;
  return true;
}

__global__ __launch_bounds__(256) void k_grid_init(imf_slot *tab, int32_t *cnt, int64_t cap, int32_t *err) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *err = 0;
  if (i < cap) {
    reinterpret_cast<uint4 *>(tab)[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
    cnt[i] = 0;
  }
}

// target cells are kept one cell inside the key range, so that a query cell's 26 neighbours never wrap
__global__ __launch_bounds__(256) void k_grid_insert(const double *__restrict__ dst, int64_t n, Grid g, int32_t *err) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int x, y, z;
  if (!cell_of_point(load3(dst, j), g.inv_cell, kCoordLim - 1, x, y, z)) {
    atomicOr(err, 1);
    g.cell_of[j] = -1;
    return;
  }
  const uint32_t s = hash_insert(g.tab, g.capmask, pack_key(0, x, y, z), 0);
  g.cell_of[j] = (int32_t)s;
  atomicAdd(&g.cnt[s], 1);
}

// one workgroup: exclusive scan of the per-slot counts in slot order -> tab[s].val = first row, tab[s].pad = count,
// cnt[s] = scatter cursor
__global__ __launch_bounds__(1024) void k_grid_scan(Grid g, int64_t cap) {
  __shared__ int32_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (cap + 1023) / 1024, b = t * per, e = min(cap, b + per);
  int32_t sum = 0;
  for (int64_t s = b; s < e; ++s) sum += g.cnt[s];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {                 // Hillis-Steele inclusive scan
    const int32_t v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int32_t run = part[t] - sum;
  for (int64_t s = b; s < e; ++s) {
    const int32_t c = g.cnt[s];
    g.tab[s].val = run;
    g.tab[s].pad = c;
    g.cnt[s] = run;
    run += c;
  }
}

__global__ __launch_bounds__(256) void k_grid_scatter(const double *__restrict__ dst, int64_t n, Grid g) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t s = g.cell_of[j];
  if (s < 0) return;
  const int32_t r = atomicAdd(&g.cnt[s], 1);
  g.xyz[3 * (int64_t)r + 0] = dst[3 * j + 0];
  g.xyz[3 * (int64_t)r + 1] = dst[3 * j + 1];
  g.xyz[3 * (int64_t)r + 2] = dst[3 * j + 2];
  g.idx[r] = (int32_t)j;
}

// nearest target (d^2 < r2, ties -> lowest original index) of p; returns its sorted row or -1
__device__ __forceinline__ int grid_nearest(const Grid &g, V3 p, double r2, double &best_d2) {
  int x, y, z;
  best_d2 = 0.0;
  if (!cell_of_point(p, g.inv_cell, kCoordLim, x, y, z)) return -1;   // beyond every target cell's neighbourhood
  int best = -1, best_idx = 0x7FFFFFFF;
  double bd = r2;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int s = hash_find_slot(g.tab, g.capmask, pack_key(0, x + dx, y + dy, z + dz));
        if (s < 0) continue;
        const uint4 v = *reinterpret_cast<const uint4 *>(g.tab + s);
        const int r0 = (int)v.z, r1 = r0 + (int)v.w;
        for (int r = r0; r < r1; ++r) {
          const V3 e = sub(load3(g.xyz, r), p);
          const double d2 = dot(e, e);
          const int id = g.idx[r];
          if (d2 < bd || (d2 == bd && best >= 0 && id < best_idx)) {
            bd = d2; best = r; best_idx = id;
          }
        }
      }
  best_d2 = bd;
  return best;
}

// fixed-order sum of a workgroup's per-thread values (xor butterfly per wavefront, then the 4 wavefronts in order)
__device__ __forceinline__ double block_sum(double v, double *lds4) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds4[w] = v;
  __syncthreads();
  return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// workspace layout of the grid (all offsets 256-byte aligned)
struct GridLayout {
  int64_t cap;
  size_t tab, cnt, cell_of, xyz, idx, err, total;
};
GridLayout grid_layout(int64_t n_dst) {
  GridLayout L;
  L.cap = imf_hash_capacity(n_dst);
  size_t p = 0;
  L.tab = p;     p += align256((size_t)L.cap * sizeof(imf_slot));
  L.cnt = p;     p += align256((size_t)L.cap * 4);
  L.cell_of = p; p += align256((size_t)n_dst * 4);
  L.xyz = p;     p += align256((size_t)n_dst * 24);
  L.idx = p;     p += align256((size_t)n_dst * 4);
  L.err = p;     p += 256;
  L.total = p;
  return L;
}

int build_grid(const double *dst, int64_t n_dst, double cell, char *ws, Grid &g, int32_t *&err, hipStream_t st) {
  const GridLayout L = grid_layout(n_dst);
  g.tab = (imf_slot *)(ws + L.tab);
  g.capmask = (uint32_t)(L.cap - 1);
  g.cnt = (int32_t *)(ws + L.cnt);
  g.cell_of = (int32_t *)(ws + L.cell_of);
  g.xyz = (double *)(ws + L.xyz);
  g.idx = (int32_t *)(ws + L.idx);
  g.inv_cell = (1.0 - 1e-9) / cell;   // a hair over r: rounding in p * inv_cell can never put a point within r two cells away
  err = (int32_t *)(ws + L.err);
  k_grid_init<<<(unsigned)div_up(L.cap, 256), 256, 0, st>>>(g.tab, g.cnt, L.cap, err);
  k_grid_insert<<<(unsigned)div_up(n_dst, 256), 256, 0, st>>>(dst, n_dst, g, err);
  k_grid_scan<<<1, 1024, 0, st>>>(g, L.cap);
  k_grid_scatter<<<(unsigned)div_up(n_dst, 256), 256, 0, st>>>(dst, n_dst, g);
  IMF_CHECK_LAUNCH("imf icp grid build");
  return IMF_OK;
}

}  // namespace
}  // namespace imf
