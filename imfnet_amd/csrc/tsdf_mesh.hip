// Triangle mesh of the sparse TSDF volume (imfnet_amd/fuse.py: TSDFVolume.extract_mesh; python -m
// imfnet_amd.integrate_scene): marching tetrahedra on the Kuhn split of every cell.  Not Open3D's marching cubes: the
// 16-case table below is derived by a generator (tests/tsdf_mesh_restate.py: generate_cases) instead of typed in, has no
// ambiguous cases, and gives a closed, consistently oriented manifold wherever the data are complete; it costs about
// twice the triangles.  The rule, restated in NumPy in tests/tsdf_mesh_restate.py:
//   valid:  a sample with w != 0 and tsdf < 0.98.  inside: valid and tsdf < 0 (a stored 0 is outside).  This is not
//     extract's rule, which also skips tsdf == 0: the mesh needs a sign for every valid sample.
//   cell (i, j, k): the eight samples (i + bx, j + by, k + bz), corner number b = bx + 2 by + 4 bz.  A cell belongs to
//     the unit of its corner 0; corners on the unit's far faces are read from the +x, +y, +xy, +z, +xz, +yz, +xyz
//     neighbour units through the table, a missing unit makes them invalid.  A cell is meshed when all 8 are valid.
//   tetrahedra: six per cell, one per permutation (a1, a2, a3) of the axes in lexicographic order, with the corners
//     0, bit(a1), bit(a1) | bit(a2), 7 (local corners 0..3).  Every cell is split alike, so neighbours agree on the
//     diagonal of their common face.
//   edges: lo -> hi for corners with lo a proper subset of hi: 12 axis edges, 6 face diagonals, the body diagonal.  An
//     edge is owned by the voxel at lo, in slot e = 0..6 for the direction hi - lo = (1, 2, 4, 3, 5, 6, 7)[e]; slots
//     0..2 are extract's three axes.
//   vertex: on an owned edge whose ends are valid, exactly one of them inside, and that lies in at least one meshed
//     cell (so no vertex is unreferenced).  t = |f_lo| / (|f_lo| + |f_hi|) in fp64, then per coordinate c:
//     p_lo[c] + voxel_length * t where the direction has bit c, p_lo[c] elsewhere, p_lo built as extract builds p0.
//     On slots 0..2 with both ends non-zero that is extract's point bit for bit.  Contraction is off for this file.
//   triangles per tetrahedron, by the inside corners (local numbers, a < b < c inside, ... < d outside):
//     1 inside a, outside b < c < d: (ab, ac, ad);  3 inside, outside d: (ad, bd, cd);
//     2 inside a < b, outside c < d: the quad (ac, ad, bd, bc) as (ac, ad, bd) and (ac, bd, bc)
//     where xy is the vertex on the edge x-y.  Each is wound counter-clockwise seen from the outside (tsdf >= 0) side by
//     swapping its last two vertices where needed.  Whether to swap is combinatorial: kTriTable holds the wound triangles
//     of an even permutation, an odd one (tetrahedra 1, 2, 5) swaps.  Positions are never consulted, so a vertex that
//     lands on a corner (f = 0) gives a zero-area triangle that is still wound consistently.
//   order: vertices (unit, voxel (z 16 + y) 16 + x, slot); triangles (unit, cell, tetrahedron, triangle); int32 indices.
//   colour (imf_tsdf_mesh_rgb; the state and its rule at the head of tsdf.hip): a vertex gets c_lo + t (c_hi - c_lo) per
//     channel in fp64 with the t above, uint8 = floor(c + 0.5) clamped (tsdf_shared.h: edge_color, the function extract
//     uses): on slots 0..2 with both ends non-zero the vertex colour is extract's point colour bit for bit.  Both ends of
//     a vertex's edge are valid, so both have a colour.  Colour is a compile-time switch of k_mesh_vertices alone; the
//     vertices and triangles of the coloured call are the plain call's.
//
// Device design.  Workspace: 1 byte (the 7-bit vertex mask) + 4 bytes (the index of its first vertex) per voxel, and
// two counts and two offsets per unit.
//   k_mesh_cells, one workgroup per unit: stages valid / inside of the unit's 17^3 samples (its own and the far-face
//     halo) as bytes in LDS, ORs the crossing edges of every meshed cell into a 17^3 LDS mask of their owners (integer
//     atomicOr: order-free), counts the unit's triangles, then ORs the non-zero LDS masks into the global byte masks of
//     this unit and its seven + neighbours.  A set bit IS a vertex: the edge lies in a meshed cell, whose corners are
//     all valid, and one end is inside.
//   k_mesh_vertex_count: vertices of a unit = set bits of its 4096 masks.  k_tsdf_scan (tsdf_shared.h) twice: offsets.
//   k_mesh_vertices: per 256 voxels a workgroup scan of the bit counts -> the voxel's first vertex index, positions.
//   k_mesh_triangles: stages the samples again, a workgroup scan of the cells' triangle counts per 256 cells, and every
//     triangle vertex resolves (owner voxel, slot) to first index + popcount(mask below slot).
// No atomic decides an output position, no floating-point atomics, no workgroup waits for another: two calls give the
// same bytes.  The write passes do nothing when a count exceeds its capacity or the vertices exceed 2^31 - 1.
#include "common.h"
#include "tsdf_shared.h"

#pragma clang fp contract(off)

namespace imf {
namespace {

constexpr int kHalo = kUnitRes + 1;               // samples per axis a unit's cells read
constexpr int kHaloN = kHalo * kHalo * kHalo;     // 4913
constexpr int kFlagValid = 1, kFlagInside = 2;

constexpr uint32_t tri6(int a, int b, int c, int d = 0, int e = 0, int f = 0) {
  return (uint32_t)a | (uint32_t)b << 3 | (uint32_t)c << 6 | (uint32_t)d << 9 | (uint32_t)e << 12 | (uint32_t)f << 15;
}
// case (bit i: local corner i inside) -> up to two triangles of local edge numbers, 3 bits each, for an even tetrahedron.
// Local edges: 0 = 0-1, 1 = 0-2, 2 = 0-3, 3 = 1-2, 4 = 1-3, 5 = 2-3.  From generate_cases (tests/tsdf_mesh_restate.py).
__constant__ uint32_t kTriTable[16] = {
    0,                       tri6(0, 1, 2),           tri6(0, 4, 3),           tri6(1, 2, 4, 1, 4, 3),
    tri6(1, 3, 5),           tri6(0, 5, 2, 0, 3, 5),  tri6(0, 4, 5, 0, 5, 1),  tri6(2, 4, 5),
    tri6(2, 5, 4),           tri6(0, 1, 5, 0, 5, 4),  tri6(0, 5, 3, 0, 2, 5),  tri6(1, 5, 3),
    tri6(1, 3, 4, 1, 4, 2),  tri6(0, 3, 4),           tri6(0, 2, 1),           0};
constexpr uint32_t kEdgeLo = 0u | 0u << 2 | 0u << 4 | 1u << 6 | 1u << 8 | 2u << 10;     // local edge -> local corners
constexpr uint32_t kEdgeHi = 1u | 2u << 2 | 3u << 4 | 2u << 6 | 3u << 8 | 3u << 10;
constexpr uint32_t kTetC1 = 1u | 1u << 3 | 2u << 6 | 2u << 9 | 4u << 12 | 4u << 15;     // tetrahedron -> bit(a1)
constexpr uint32_t kTetC2 = 3u | 5u << 3 | 3u << 6 | 6u << 9 | 5u << 12 | 6u << 15;     //             -> bit(a1) | bit(a2)
constexpr uint32_t kTetOdd = 1u << 1 | 1u << 2 | 1u << 5;                                // odd permutations
constexpr uint32_t kSlotOfDir = 0u << 3 | 1u << 6 | 3u << 9 | 2u << 12 | 4u << 15 | 5u << 18 | 6u << 21;   // 3 bits per direction
constexpr uint32_t kDirOfSlot = 1u | 2u << 3 | 4u << 6 | 3u << 9 | 5u << 12 | 6u << 15 | 7u << 18;

__device__ __forceinline__ int halo_index(int x, int y, int z) { return (z * kHalo + y) * kHalo + x; }
// which of the eight units (this one and its + neighbours) holds the sample at halo coordinate 0..16, and where
__device__ __forceinline__ int halo_unit(int x, int y, int z) { return (x >> 4) | ((y >> 4) << 1) | ((z >> 4) << 2); }
__device__ __forceinline__ int halo_voxel(int x, int y, int z) { return (((z & 15) * kUnitRes) + (y & 15)) * kUnitRes + (x & 15); }

// rows of this unit (nb[0]) and its seven + neighbours, -1 where there is none; threads 0..7
__device__ __forceinline__ void find_neighbours(int *nb, int u, int n, const int32_t *__restrict__ units,
                                                const imf_slot *__restrict__ tab, uint32_t capmask) {
  const int t = threadIdx.x;
  if (t == 0) nb[0] = u;
  else if (t < 8) {
    const int r = hash_find(tab, capmask, unit_key(units[3 * u] + (t & 1), units[3 * u + 1] + ((t >> 1) & 1), units[3 * u + 2] + (t >> 2)), 0);
    nb[t] = r >= 0 && r < n ? r : -1;
  }
}

// valid / inside of the unit's 17^3 samples into LDS
__device__ __forceinline__ void stage_flags(uint8_t *flags, const int *nb, const float2 *__restrict__ vox) {
  for (int i = threadIdx.x; i < kHaloN; i += kTsdfThreads) {
    const int x = i % kHalo, y = (i / kHalo) % kHalo, z = i / (kHalo * kHalo);
    const int r = nb[halo_unit(x, y, z)];
    int f = 0;
    if (r >= 0) {
      const float2 s = vox[(int64_t)r * kUnitVoxels + halo_voxel(x, y, z)];
      if (s.y != 0.0f && s.x < 0.98f) f = kFlagValid | (s.x < 0.0f ? kFlagInside : 0);
    }
    flags[i] = (uint8_t)f;
  }
}

// the inside bits of the cell's eight corners; false when the cell is not meshed
__device__ __forceinline__ bool cell_corners(const uint8_t *flags, int lx, int ly, int lz, int &inside) {
  const int base = halo_index(lx, ly, lz);
  int all = kFlagValid;
  inside = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int f = flags[base + halo_index(b & 1, (b >> 1) & 1, b >> 2)];
    all &= f;
    inside |= ((f >> 1) & 1) << b;
  }
  return all != 0;
}

__device__ __forceinline__ int tet_case(int inside, int q) {
  const int c1 = (kTetC1 >> (3 * q)) & 7, c2 = (kTetC2 >> (3 * q)) & 7;
  return (inside & 1) | (((inside >> c1) & 1) << 1) | (((inside >> c2) & 1) << 2) | (((inside >> 7) & 1) << 3);
}
__device__ __forceinline__ int case_triangles(int c) {
  const int k = __popc(c);
  return k == 2 ? 2 : (k & 1);
}
__device__ __forceinline__ int cell_triangles(int inside) {
  int n = 0;
#pragma unroll
  for (int q = 0; q < 6; ++q) n += case_triangles(tet_case(inside, q));
  return n;
}

// exclusive scan of c over the workgroup's 256 threads in thread order; all = the workgroup's sum
__device__ __forceinline__ int block_scan(int c, int *wsum, int &all) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int incl = c;
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  __syncthreads();
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int before = 0;
  all = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wv) before += wsum[w];
    all += wsum[w];
  }
  return before + incl - c;
}

__global__ __launch_bounds__(kTsdfThreads) void k_mesh_cells(const float2 *__restrict__ vox, const int32_t *__restrict__ units,
                                                            const int32_t *__restrict__ n_units, int max_units,
                                                            const imf_slot *__restrict__ tab, uint32_t capmask,
                                                            uint32_t *mask, int32_t *__restrict__ tri_cnt) {
  const int u = blockIdx.x, n = min(n_units[0], max_units);
  if (u >= n) return;
  __shared__ int nb[8];
  __shared__ int wsum[4];
  __shared__ uint8_t flags[(kHaloN + 3) & ~3];
  __shared__ uint32_t em[kHaloN];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  find_neighbours(nb, u, n, units, tab, capmask);
  for (int i = t; i < kHaloN; i += kTsdfThreads) em[i] = 0u;
  __syncthreads();
  stage_flags(flags, nb, vox);
  __syncthreads();
  const int lx = t & 15, ly = t >> 4;
  int total = 0;
  for (int lz = 0; lz < kUnitRes; ++lz) {
    int inside;
    if (!cell_corners(flags, lx, ly, lz, inside) || inside == 0 || inside == 255) continue;
    total += cell_triangles(inside);
    const int base = halo_index(lx, ly, lz);
#pragma unroll
    for (int lo = 0; lo < 7; ++lo) {
      uint32_t m = 0u;
#pragma unroll
      for (int d = 1; d < 8; ++d) {
        if (lo & d) continue;                                // lo | d is a corner: the edge lo -> lo + d
        if (((inside >> lo) ^ (inside >> (lo | d))) & 1) m |= 1u << ((kSlotOfDir >> (3 * d)) & 7);
      }
      if (m) atomicOr(&em[base + halo_index(lo & 1, (lo >> 1) & 1, lo >> 2)], m);
    }
  }
  for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
  if (lane == 0) wsum[wv] = total;
  __syncthreads();                                           // the LDS masks are complete as well
  if (t == 0) tri_cnt[u] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  for (int i = t; i < kHaloN; i += kTsdfThreads) {
    const uint32_t m = em[i];
    if (!m) continue;
    const int x = i % kHalo, y = (i / kHalo) % kHalo, z = i / (kHalo * kHalo);
    const int r = nb[halo_unit(x, y, z)];
    if (r < 0) continue;                                     // cannot be: a meshed cell has this corner valid
    const int64_t g = (int64_t)r * kUnitVoxels + halo_voxel(x, y, z);
    atomicOr(&mask[g >> 2], m << (8 * (int)(g & 3)));
  }
}

__global__ __launch_bounds__(kTsdfThreads) void k_mesh_vertex_count(const uint32_t *__restrict__ mask,
                                                                   const int32_t *__restrict__ n_units, int max_units,
                                                                   int32_t *__restrict__ vtx_cnt) {
  const int u = blockIdx.x, n = min(n_units[0], max_units);
  if (u >= n) return;
  __shared__ int wsum[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t *mine = mask + (int64_t)u * (kUnitVoxels / 4);
  int total = 0;
  for (int i = t; i < kUnitVoxels / 4; i += kTsdfThreads) total += __popc(mine[i]);
  for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
  if (lane == 0) wsum[wv] = total;
  __syncthreads();
  if (t == 0) vtx_cnt[u] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// true when the write passes must leave the outputs alone
__device__ __forceinline__ bool mesh_refused(const int64_t *v_off, const int64_t *t_off, int n, int64_t v_cap, int64_t t_cap) {
  return v_off[n] > v_cap || t_off[n] > t_cap || v_off[n] > 0x7FFFFFFFll;
}

// COLOR: row i of out_rgb = the colour of vertex row i
template <bool COLOR>
__global__ __launch_bounds__(kTsdfThreads) void k_mesh_vertices(const float2 *__restrict__ vox, const int32_t *__restrict__ units,
                                                               const int32_t *__restrict__ n_units, int max_units,
                                                               const imf_slot *__restrict__ tab, uint32_t capmask, TsdfP P,
                                                               const uint8_t *__restrict__ mask,
                                                               const int64_t *__restrict__ v_off,
                                                               const int64_t *__restrict__ t_off, int64_t v_cap, int64_t t_cap,
                                                               int32_t *__restrict__ v_base, double *__restrict__ out,
                                                               const float *__restrict__ col,
                                                               uint8_t *__restrict__ out_rgb) {
  const int u = blockIdx.x, n = min(n_units[0], max_units);
  if (u >= n) return;
  if (mesh_refused(v_off, t_off, n, v_cap, t_cap)) return;
  __shared__ int nb[8];
  __shared__ int wsum[4];
  const int t = threadIdx.x;
  find_neighbours(nb, u, n, units, tab, capmask);
  __syncthreads();
  const int ux = units[3 * u], uy = units[3 * u + 1], uz = units[3 * u + 2];
  const int lx = t & 15, ly = t >> 4;
  int64_t run = v_off[u];
  for (int lz = 0; lz < kUnitRes; ++lz) {
    const int64_t g = (int64_t)u * kUnitVoxels + lz * 256 + t;
    const uint32_t m = mask[g];
    const int c = __popc(m);
    int all;
    int64_t row = run + block_scan(c, wsum, all);
    run += all;
    v_base[g] = (int32_t)row;
    if (!c) continue;
    const double p0[3] = {((double)(kUnitRes * ux + lx) + P.off) * P.vl, ((double)(kUnitRes * uy + ly) + P.off) * P.vl,
                          ((double)(kUnitRes * uz + lz) + P.off) * P.vl};
    const double r0 = fabs((double)vox[g].x);
#pragma unroll
    for (int e = 0; e < 7; ++e) {
      if (!((m >> e) & 1u)) continue;
      const int d = (kDirOfSlot >> (3 * e)) & 7;
      const int x = lx + (d & 1), y = ly + ((d >> 1) & 1), z = lz + (d >> 2);
      const int r = nb[halo_unit(x, y, z)];
      const double r1 = r >= 0 ? fabs((double)vox[(int64_t)r * kUnitVoxels + halo_voxel(x, y, z)].x) : 0.0;   // r >= 0 always
      const double tt = r0 / (r0 + r1);
      const double step = P.vl * tt;
      out[3 * row + 0] = (d & 1) ? p0[0] + step : p0[0];
      out[3 * row + 1] = (d & 2) ? p0[1] + step : p0[1];
      out[3 * row + 2] = (d & 4) ? p0[2] + step : p0[2];
      if constexpr (COLOR) edge_color(col, u, lz * 256 + t, r >= 0 ? r : u, halo_voxel(x, y, z), tt, out_rgb + 3 * row);
      ++row;
    }
  }
}

__global__ __launch_bounds__(kTsdfThreads) void k_mesh_triangles(const float2 *__restrict__ vox, const int32_t *__restrict__ units,
                                                                const int32_t *__restrict__ n_units, int max_units,
                                                                const imf_slot *__restrict__ tab, uint32_t capmask,
                                                                const uint8_t *__restrict__ mask,
                                                                const int32_t *__restrict__ v_base,
                                                                const int64_t *__restrict__ v_off,
                                                                const int64_t *__restrict__ t_off, int64_t v_cap, int64_t t_cap,
                                                                int32_t *__restrict__ out) {
  const int u = blockIdx.x, n = min(n_units[0], max_units);
  if (u >= n) return;
  if (mesh_refused(v_off, t_off, n, v_cap, t_cap)) return;
  __shared__ int nb[8];
  __shared__ int wsum[4];
  __shared__ uint8_t flags[(kHaloN + 3) & ~3];
  const int t = threadIdx.x;
  find_neighbours(nb, u, n, units, tab, capmask);
  __syncthreads();
  stage_flags(flags, nb, vox);
  __syncthreads();
  const int lx = t & 15, ly = t >> 4;
  int64_t run = t_off[u];
  for (int lz = 0; lz < kUnitRes; ++lz) {
    int inside;
    const bool meshed = cell_corners(flags, lx, ly, lz, inside);
    const int c = meshed ? cell_triangles(inside) : 0;
    int all;
    int64_t row = run + block_scan(c, wsum, all);
    run += all;
    if (!c) continue;
    for (int q = 0; q < 6; ++q) {
      const int cs = tet_case(inside, q), nt = case_triangles(cs);
      if (!nt) continue;
      const uint32_t tri = kTriTable[cs];
      const int c1 = (kTetC1 >> (3 * q)) & 7, c2 = (kTetC2 >> (3 * q)) & 7;
      const bool odd = (kTetOdd >> q) & 1u;
      for (int s = 0; s < nt; ++s) {
        int32_t idx[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int e = (tri >> (3 * (3 * s + k))) & 7;
          const int a = (kEdgeLo >> (2 * e)) & 3, b = (kEdgeHi >> (2 * e)) & 3;      // local corners, a < b
          const int lo = a == 0 ? 0 : (a == 1 ? c1 : c2), hi = b == 1 ? c1 : (b == 2 ? c2 : 7);
          const int slot = (kSlotOfDir >> (3 * (hi - lo))) & 7;
          const int x = lx + (lo & 1), y = ly + ((lo >> 1) & 1), z = lz + (lo >> 2);
          const int r = nb[halo_unit(x, y, z)];                                      // >= 0: the cell is meshed
          const int64_t g = (int64_t)(r >= 0 ? r : u) * kUnitVoxels + halo_voxel(x, y, z);
          idx[k] = v_base[g] + __popc((uint32_t)mask[g] & ((1u << slot) - 1u));
        }
        out[3 * row + 0] = idx[0];
        out[3 * row + 1] = odd ? idx[2] : idx[1];
        out[3 * row + 2] = odd ? idx[1] : idx[2];
        ++row;
      }
    }
  }
}

}  // namespace
}  // namespace imf

using namespace imf;

// imf_tsdf_mesh and imf_tsdf_mesh_rgb: the same passes, the vertex pass with or without the colours
static int tsdf_mesh(const char *what, bool rgb, const float *voxels, const float *colors, const int32_t *units,
                     const int32_t *n_units, int64_t max_units, const imf_slot *table, int64_t table_capacity,
                     const imf_tsdf_params *params, double *out_vertices, uint8_t *out_rgb, int64_t vertex_capacity,
                     int32_t *out_triangles, int64_t triangle_capacity, int64_t *out_n, void *workspace,
                     size_t workspace_bytes, void *stream) {
  TsdfP P;
  int rc = tsdf_params(what, params, P);
  if (rc) return rc;
  IMF_REQUIRE(voxels && units && n_units && table && out_n && workspace, "%s: null pointer", what);
  IMF_REQUIRE(max_units >= 1 && max_units <= kTsdfMaxUnits, "%s: max_units=%lld", what, (long long)max_units);
  IMF_REQUIRE(is_pow2(table_capacity) && table_capacity <= (1ll << 31), "%s: table_capacity=%lld", what,
              (long long)table_capacity);
  IMF_REQUIRE(vertex_capacity >= 0 && (out_vertices || vertex_capacity == 0), "%s: vertex_capacity=%lld with out=%p",
              what, (long long)vertex_capacity, (const void *)out_vertices);
  IMF_REQUIRE(triangle_capacity >= 0 && (out_triangles || triangle_capacity == 0),
              "%s: triangle_capacity=%lld with out=%p", what, (long long)triangle_capacity, (const void *)out_triangles);
  if (rgb) {
    IMF_REQUIRE(colors, "%s: colors is NULL", what);
    IMF_REQUIRE(out_rgb || vertex_capacity == 0, "%s: out_rgb is NULL with vertex_capacity=%lld", what,
                (long long)vertex_capacity);
    IMF_REQUIRE(((uintptr_t)colors & 3) == 0, "%s: colors must be 4-byte aligned", what);
  }
  IMF_REQUIRE(((uintptr_t)voxels & 7) == 0, "%s: voxels must be 8-byte aligned", what);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", what);
  IMF_REQUIRE(workspace_bytes >= imf_tsdf_mesh_workspace_bytes(max_units), "%s: workspace %zu < %zu", what,
              workspace_bytes, imf_tsdf_mesh_workspace_bytes(max_units));
  hipStream_t st = (hipStream_t)stream;
  char *ws = (char *)workspace;
  int32_t *v_cnt = (int32_t *)ws;
  ws += align256((size_t)max_units * 4);
  int32_t *t_cnt = (int32_t *)ws;
  ws += align256((size_t)max_units * 4);
  int64_t *v_off = (int64_t *)ws;
  ws += align256((size_t)(max_units + 1) * 8);
  int64_t *t_off = (int64_t *)ws;
  ws += align256((size_t)(max_units + 1) * 8);
  uint8_t *mask = (uint8_t *)ws;
  ws += align256((size_t)max_units * kUnitVoxels);
  int32_t *v_base = (int32_t *)ws;
  const uint32_t capmask = (uint32_t)(table_capacity - 1);
  const float2 *vox = reinterpret_cast<const float2 *>(voxels);
  const unsigned grid = (unsigned)max_units;
  IMF_CHECK_HIP(hipMemsetAsync(mask, 0, (size_t)max_units * kUnitVoxels, st));
  k_mesh_cells<<<grid, kTsdfThreads, 0, st>>>(vox, units, n_units, (int)max_units, table, capmask,
                                              reinterpret_cast<uint32_t *>(mask), t_cnt);
  k_mesh_vertex_count<<<grid, kTsdfThreads, 0, st>>>(reinterpret_cast<const uint32_t *>(mask), n_units, (int)max_units, v_cnt);
  k_tsdf_scan<<<1, 1024, 0, st>>>(v_cnt, n_units, (int)max_units, v_off, out_n);
  k_tsdf_scan<<<1, 1024, 0, st>>>(t_cnt, n_units, (int)max_units, t_off, out_n + 1);
  if (vertex_capacity > 0 && triangle_capacity > 0) {
    if (rgb)
      k_mesh_vertices<true><<<grid, kTsdfThreads, 0, st>>>(vox, units, n_units, (int)max_units, table, capmask, P, mask, v_off,
                                                           t_off, vertex_capacity, triangle_capacity, v_base, out_vertices,
                                                           colors, out_rgb);
    else
      k_mesh_vertices<false><<<grid, kTsdfThreads, 0, st>>>(vox, units, n_units, (int)max_units, table, capmask, P, mask, v_off,
                                                            t_off, vertex_capacity, triangle_capacity, v_base, out_vertices,
                                                            nullptr, nullptr);
    k_mesh_triangles<<<grid, kTsdfThreads, 0, st>>>(vox, units, n_units, (int)max_units, table, capmask, mask, v_base, v_off,
                                                    t_off, vertex_capacity, triangle_capacity, out_triangles);
  }
  IMF_CHECK_LAUNCH(what);
  return IMF_OK;
}

extern "C" {

size_t imf_tsdf_mesh_workspace_bytes(int64_t max_units) {
  if (max_units < 1 || max_units > kTsdfMaxUnits) return 0;
  return 2 * align256((size_t)max_units * 4) + 2 * align256((size_t)(max_units + 1) * 8) +
         align256((size_t)max_units * kUnitVoxels) + align256((size_t)max_units * kUnitVoxels * 4);
}

int imf_tsdf_mesh(const float *voxels, const int32_t *units, const int32_t *n_units, int64_t max_units,
                  const imf_slot *table, int64_t table_capacity, const imf_tsdf_params *params, double *out_vertices,
                  int64_t vertex_capacity, int32_t *out_triangles, int64_t triangle_capacity, int64_t *out_n,
                  void *workspace, size_t workspace_bytes, void *stream) {
  return tsdf_mesh("imf_tsdf_mesh", false, voxels, nullptr, units, n_units, max_units, table, table_capacity, params,
                   out_vertices, nullptr, vertex_capacity, out_triangles, triangle_capacity, out_n, workspace, workspace_bytes,
                   stream);
}

int imf_tsdf_mesh_rgb(const float *voxels, const float *colors, const int32_t *units, const int32_t *n_units,
                      int64_t max_units, const imf_slot *table, int64_t table_capacity, const imf_tsdf_params *params,
                      double *out_vertices, uint8_t *out_rgb, int64_t vertex_capacity, int32_t *out_triangles,
                      int64_t triangle_capacity, int64_t *out_n, void *workspace, size_t workspace_bytes, void *stream) {
  return tsdf_mesh("imf_tsdf_mesh_rgb", true, voxels, colors, units, n_units, max_units, table, table_capacity, params,
                   out_vertices, out_rgb, vertex_capacity, out_triangles, triangle_capacity, out_n, workspace, workspace_bytes,
                   stream);
}

}  // extern "C"
