// Fragment overlap for the 3DMatch training pairs (imfnet_amd/overlap.py, python -m imfnet_amd.compute_overlap).
//
// Reference being replaced: data/compute_overlap.py:93-141.  For every fragment pair (p, q) of a sequence with
// number(p) < number(q), consecutive numbers left out, a pyflann k-d forest over p's (down-sampled, float32) points is
// asked for the nearest neighbour of every point of q; the rows (nn index in p, index in q) whose sqrt(d^2) <= 0.075
// are the correspondences, ratio = rows / max(n_p, n_q), and a pair below 0.3 writes nothing.  Restated here as pinned
// (tests/overlap_restate.py states it in NumPy):
//   for j in 0 .. n_q - 1 (ascending):
//     for every i: dx = p[i].x - q[j].x, dy, dz likewise              (float32)
//                  d2[i] = (dx * dx + dy * dy) + dz * dz              (float32, every operation rounded, no fma)
//     i* = the lowest i among those of the smallest d2
//     keep the row (i*, j) when sqrtf(d2[i*]) <= (float)thresh         (sqrtf correctly rounded)
//   n = rows kept; rows are int64 and ascend in j
// Changed against upstream, on purpose: the neighbour is the EXACT nearest one (FLANN's forest with trees = 4,
// checks = 32 is approximate), equal distances go to the lowest p index.  Contraction into fused multiply-adds is
// switched off for this file so that the arithmetic above is the arithmetic that runs.
//
// Device design.  A fragment is the search target of dozens of pairs, so its index is built ONCE (imf_overlap_index_build)
// and stays resident: the float32 points sorted by cell (cell-CSR) with their original indices, the cell table (the
// library's open-addressing table of 16-byte imf_slot entries: key = cell, val = first sorted row, pad = points), the
// list of occupied cells, and the list of query chunks (a cell's points in runs of at most 256).  The order of points
// inside a cell is whatever the scatter's integer atomics give; it reaches no output, because the neighbour choice is
// (d2, index)-lexicographic and every result is written by original index.
// The cell edge is a hair over the threshold (the caller passes it; imf_overlap_pair refuses an edge below
// thresh (1 + 2^-20)): a point one whole cell away along an axis has |dx| >= edge, and float32 rounding of dx, dx dx
// and the sums (a few 2^-24 relative) cannot bring sqrtf(d2) down to thresh.  So every neighbour that can be kept lies
// in the 27 cells around the query's cell; a nearest point found there that is farther than thresh is dropped, as
// the true nearest one (at least as far) would be.
// imf_overlap_bound: for every candidate pair, the points of q whose cell has an occupied cell of p among its 27
// neighbours, from the two tables alone -- an upper bound of n, one launch for all pairs of a sequence, integer
// atomics only.  A pair whose bound / max(n_p, n_q) is below the minimum overlap needs no exact pass.
// imf_overlap_pair, the hot kernel: one workgroup of 256 threads per query chunk of q (queries in q's CELL order, so
// the whole workgroup shares one neighbourhood).  27 threads look the neighbour cells up in p's table; the workgroup
// then stages each neighbour cell of p through LDS in tiles of 1024 points (x, y, z, index = 16 bytes, 16 KiB per
// workgroup), and every thread scans the tile for its own query: all lanes read the same LDS address (a broadcast, no
// bank conflict), about ten VALU operations per candidate.  A cell of any size is walked tile by tile, nothing is
// capped.  The result goes to nn_idx[original q index], -1 where nothing is within thresh.
// imf_overlap_emit: the rows in ascending j by a three-step scan (per-block counts, one workgroup over the blocks,
// write); no atomic decides a position, two runs are bit-identical.  No floating-point atomics anywhere, no workgroup
// waits for another one, wave64.
#include "common.h"

#pragma clang fp contract(off)

namespace imf {
namespace {

constexpr int kOvThreads = 256;                    // queries per chunk = threads per workgroup of the exact pass
constexpr int kOvTile = 1024;                      // candidates per LDS tile (float4 each: 16 KiB)
constexpr int kOvFlagRange = 1;                    // a point that is NaN or beyond the cell range was left out
constexpr int kEmitBlock = 1024;                   // rows per block of the emit scan
constexpr int64_t kOvMaxPoints = 1ll << 26;

struct OvLayout {
  int64_t cap;
  size_t tab, xyz, idx, cells, chunks, meta, total;
};
OvLayout ov_layout(int64_t n) {
  OvLayout L;
  L.cap = imf_hash_capacity(n);
  size_t p = 0;
  L.tab = p;    p += align256((size_t)L.cap * sizeof(imf_slot));
  L.xyz = p;    p += align256((size_t)n * 12);
  L.idx = p;    p += align256((size_t)n * 4);
  L.cells = p;  p += align256((size_t)n * 4);
  L.chunks = p; p += align256((size_t)n * 8);
  L.meta = p;   p += 256;
  L.total = p;
  return L;
}

__device__ __forceinline__ void cell_of_key(uint64_t k, int &x, int &y, int &z) {
  x = ((int)((k >> (2 * kCoordBits)) & 0x3FFFF) << 14) >> 14;     // sign-extend the 18-bit fields
  y = ((int)((k >> kCoordBits) & 0x3FFFF) << 14) >> 14;
  z = ((int)(k & 0x3FFFF) << 14) >> 14;
}

__global__ __launch_bounds__(256) void k_ov_init(imf_slot *tab, int64_t cap, int32_t *meta) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4) meta[i] = 0;
  if (i < cap) reinterpret_cast<uint4 *>(tab)[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
}

// cells are kept one cell inside the key range, so that a query cell's 26 neighbours never wrap
__global__ __launch_bounds__(256) void k_ov_insert(const float *__restrict__ pts, int64_t n, double inv_cell, imf_slot *tab,
                                                   uint32_t capmask, int32_t *__restrict__ cell_of, int32_t *meta) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int lim = kCoordLim - 1;
  const double fx = floor((double)pts[3 * j + 0] * inv_cell), fy = floor((double)pts[3 * j + 1] * inv_cell),
               fz = floor((double)pts[3 * j + 2] * inv_cell);
  if (!(fx >= -lim && fx < lim && fy >= -lim && fy < lim && fz >= -lim && fz < lim)) {     // NaN too
    atomicOr(&meta[2], kOvFlagRange);
    cell_of[j] = -1;
    return;
  }
  const uint32_t s = hash_insert(tab, capmask, pack_key(0, (int)fx, (int)fy, (int)fz), 0);
  cell_of[j] = (int32_t)s;
  atomicAdd(&tab[s].pad, 1);
}

// one workgroup: exclusive scans, in slot order, of the points, the occupied cells and the query chunks per slot ->
// tab[s].val = first sorted row, cursor[s] = the same (the scatter's cursor), cells[], chunks[], meta[0..1], meta[3]
__global__ __launch_bounds__(1024) void k_ov_scan(imf_slot *tab, int64_t cap, int32_t *__restrict__ cursor,
                                                  int32_t *__restrict__ cells, int32_t *__restrict__ chunks, int32_t *meta) {
  __shared__ int32_t part[3][1024];
  const int t = threadIdx.x;
  const int64_t per = (cap + 1023) / 1024, b = t * per, e = min(cap, b + per);
  int32_t sum[3] = {0, 0, 0};
  for (int64_t s = b; s < e; ++s) {
    const int32_t c = tab[s].pad;
    sum[0] += c;
    sum[1] += c > 0;
    sum[2] += (c + kOvThreads - 1) / kOvThreads;
  }
  for (int k = 0; k < 3; ++k) part[k][t] = sum[k];
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {                 // Hillis-Steele inclusive scan
    int32_t v[3];
    for (int k = 0; k < 3; ++k) v[k] = t >= o ? part[k][t - o] : 0;
    __syncthreads();
    for (int k = 0; k < 3; ++k) part[k][t] += v[k];
    __syncthreads();
  }
  int32_t row = part[0][t] - sum[0], cell = part[1][t] - sum[1], chunk = part[2][t] - sum[2];
  for (int64_t s = b; s < e; ++s) {
    const int32_t c = tab[s].pad;
    tab[s].val = row;
    cursor[s] = row;
    if (c > 0) cells[cell++] = (int32_t)s;
    for (int32_t o = 0; o < c; o += kOvThreads) {
      chunks[2 * chunk + 0] = (int32_t)s;
      chunks[2 * chunk + 1] = o;
      ++chunk;
    }
    row += c;
  }
  if (t == 1023) {
    meta[0] = part[1][1023];
    meta[1] = part[2][1023];
    meta[3] = part[0][1023];
  }
}

__global__ __launch_bounds__(256) void k_ov_scatter(const float *__restrict__ pts, int64_t n, const int32_t *__restrict__ cell_of,
                                                    int32_t *cursor, float *__restrict__ xyz, int32_t *__restrict__ idx) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t s = cell_of[j];
  if (s < 0) return;
  const int32_t r = atomicAdd(&cursor[s], 1);
  xyz[3 * (int64_t)r + 0] = pts[3 * j + 0];
  xyz[3 * (int64_t)r + 1] = pts[3 * j + 1];
  xyz[3 * (int64_t)r + 2] = pts[3 * j + 2];
  idx[r] = (int32_t)j;
}

// the prefilter: grid (cell blocks of q, pairs).  One thread per occupied cell of q; its points count when p has an
// occupied cell among the 27 around it.
__global__ __launch_bounds__(256) void k_ov_bound(const imf_overlap_index *__restrict__ indices,
                                                  const int32_t *__restrict__ pairs, unsigned long long *__restrict__ bound) {
  const int b = blockIdx.y;
  const imf_overlap_index P = indices[pairs[2 * b + 0]], Q = indices[pairs[2 * b + 1]];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long add = 0;
  if (c < Q.meta[0]) {
    const uint4 v = *reinterpret_cast<const uint4 *>(Q.table + Q.cells[c]);
    int x, y, z;
    cell_of_key(((uint64_t)v.y << 32) | v.x, x, y, z);
    const uint32_t capmask = (uint32_t)(P.capacity - 1);
    bool hit = false;
    for (int dz = -1; dz <= 1 && !hit; ++dz)
      for (int dy = -1; dy <= 1 && !hit; ++dy)
        for (int dx = -1; dx <= 1 && !hit; ++dx) hit = hash_find_slot(P.table, capmask, pack_key(0, x + dx, y + dy, z + dz)) >= 0;
    if (hit) add = (unsigned long long)v.w;
  }
  for (int o = 32; o > 0; o >>= 1) add += __shfl_xor(add, o, 64);
  if ((threadIdx.x & 63) == 0 && add) atomicAdd(&bound[b], add);
}

__global__ __launch_bounds__(256) void k_ov_fill(int32_t *p, int64_t n, int32_t v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// the exact pass: one workgroup per query chunk of q
__global__ __launch_bounds__(kOvThreads) void k_ov_pair(imf_overlap_index P, imf_overlap_index Q, float thresh,
                                                        int32_t *__restrict__ nn_idx) {
  __shared__ float4 tile[kOvTile];
  __shared__ int32_t nb_row[27], nb_cnt[27];
  if ((int)blockIdx.x >= Q.meta[1]) return;            // uniform: the whole workgroup leaves
  const int t = threadIdx.x;
  const int32_t slot = Q.chunks[2 * blockIdx.x + 0], off = Q.chunks[2 * blockIdx.x + 1];
  const uint4 qc = *reinterpret_cast<const uint4 *>(Q.table + slot);
  const int32_t q_row = (int32_t)qc.z + off, q_cnt = min((int32_t)qc.w - off, kOvThreads);
  if (t < 27) {
    int x, y, z;
    cell_of_key(((uint64_t)qc.y << 32) | qc.x, x, y, z);
    const int s = hash_find_slot(P.table, (uint32_t)(P.capacity - 1), pack_key(0, x + t % 3 - 1, y + (t / 3) % 3 - 1, z + t / 9 - 1));
    int32_t row = 0, cnt = 0;
    if (s >= 0) {
      const uint4 v = *reinterpret_cast<const uint4 *>(P.table + s);
      row = (int32_t)v.z;
      cnt = (int32_t)v.w;
    }
    nb_row[t] = row;
    nb_cnt[t] = cnt;
  }
  const bool live = t < q_cnt;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) {
    qx = Q.xyz[3 * (int64_t)(q_row + t) + 0];
    qy = Q.xyz[3 * (int64_t)(q_row + t) + 1];
    qz = Q.xyz[3 * (int64_t)(q_row + t) + 2];
  }
  float best = __builtin_inff();
  int32_t best_id = 0x7FFFFFFF;
  __syncthreads();
  for (int c = 0; c < 27; ++c) {
    const int32_t row = nb_row[c], cnt = nb_cnt[c];
    for (int32_t base = 0; base < cnt; base += kOvTile) {
      const int32_t m = min(cnt - base, kOvTile);
      __syncthreads();                                 // the previous tile has been read by everyone
      for (int32_t k = t; k < m; k += kOvThreads) {
        const int64_t r = (int64_t)row + base + k;
        tile[k] = make_float4(P.xyz[3 * r + 0], P.xyz[3 * r + 1], P.xyz[3 * r + 2], __int_as_float(P.idx[r]));
      }
      __syncthreads();
      if (live) {
#pragma unroll 4
        for (int32_t k = 0; k < m; ++k) {
          const float4 v = tile[k];
          const float dx = v.x - qx, dy = v.y - qy, dz = v.z - qz;
          const float d2 = (dx * dx + dy * dy) + dz * dz;
          const int32_t id = __float_as_int(v.w);
          if (d2 < best || (d2 == best && id < best_id)) {
            best = d2;
            best_id = id;
          }
        }
      }
    }
  }
  if (live) nn_idx[Q.idx[q_row + t]] = (best_id != 0x7FFFFFFF && sqrtf(best) <= thresh) ? best_id : -1;
}

// emit, step 1: kept rows per block of kEmitBlock queries
__global__ __launch_bounds__(256) void k_ov_emit_count(const int32_t *__restrict__ nn_idx, int64_t n, int32_t *__restrict__ block_cnt) {
  __shared__ int32_t w4[4];
  const int64_t b0 = (int64_t)blockIdx.x * kEmitBlock;
  int32_t c = 0;
  for (int k = 0; k < kEmitBlock / 256; ++k) {
    const int64_t j = b0 + k * 256 + threadIdx.x;
    c += j < n && nn_idx[j] >= 0;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) w4[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = w4[0] + w4[1] + w4[2] + w4[3];
}

// emit, step 2: one workgroup, exclusive scan of the block counts in place (int64 total)
__global__ __launch_bounds__(1024) void k_ov_emit_scan(int32_t *__restrict__ block_cnt, int64_t n_blocks, int64_t *out_n) {
  __shared__ int32_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (n_blocks + 1023) / 1024, b = t * per, e = min(n_blocks, b + per);
  int32_t sum = 0;
  for (int64_t i = b; i < e; ++i) sum += block_cnt[i];
  part[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int32_t v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int32_t run = part[t] - sum;
  for (int64_t i = b; i < e; ++i) {
    const int32_t c = block_cnt[i];
    block_cnt[i] = run;
    run += c;
  }
  if (t == 1023) *out_n = (int64_t)part[1023];
}

// emit, step 3: every thread owns 4 consecutive queries; a workgroup scan of the per-thread counts places them
__global__ __launch_bounds__(256) void k_ov_emit_write(const int32_t *__restrict__ nn_idx, int64_t n,
                                                       const int32_t *__restrict__ block_off, int64_t *__restrict__ pairs) {
  __shared__ int32_t part[256];
  const int t = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * kEmitBlock + 4 * t;
  int32_t nn[4], c = 0;
  for (int k = 0; k < 4; ++k) {
    nn[k] = j0 + k < n ? nn_idx[j0 + k] : -1;
    c += nn[k] >= 0;
  }
  part[t] = c;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int32_t v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t pos = (int64_t)block_off[blockIdx.x] + part[t] - c;
  for (int k = 0; k < 4; ++k)
    if (nn[k] >= 0) {
      pairs[2 * pos + 0] = nn[k];
      pairs[2 * pos + 1] = j0 + k;
      ++pos;
    }
}

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

size_t imf_overlap_index_bytes(int64_t n) {
  if (n <= 0 || n > kOvMaxPoints) return 0;
  return ov_layout(n).total;
}

size_t imf_overlap_index_workspace_bytes(int64_t n) {
  if (n <= 0 || n > kOvMaxPoints) return 0;
  return align256((size_t)n * 4) + align256((size_t)imf_hash_capacity(n) * 4);
}

int imf_overlap_index_build(const float *points, int64_t n, double cell, void *storage, size_t storage_bytes,
                            imf_overlap_index *index, void *workspace, size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(points && storage && index && workspace, "imf_overlap_index_build: null pointer");
  IMF_REQUIRE(n >= 1 && n <= kOvMaxPoints, "imf_overlap_index_build: n=%lld", (long long)n);
  IMF_REQUIRE(cell > 0.0 && cell < 1e6, "imf_overlap_index_build: cell=%g", cell);
  IMF_REQUIRE(((uintptr_t)storage & 255) == 0 && ((uintptr_t)workspace & 255) == 0,
              "imf_overlap_index_build: storage and workspace must be 256-byte aligned");
  IMF_REQUIRE(storage_bytes >= imf_overlap_index_bytes(n), "imf_overlap_index_build: storage %zu < %zu", storage_bytes,
              imf_overlap_index_bytes(n));
  IMF_REQUIRE(workspace_bytes >= imf_overlap_index_workspace_bytes(n), "imf_overlap_index_build: workspace %zu < %zu",
              workspace_bytes, imf_overlap_index_workspace_bytes(n));
  hipStream_t st = (hipStream_t)stream;
  const OvLayout L = ov_layout(n);
  char *base = (char *)storage, *ws = (char *)workspace;
  index->table = (imf_slot *)(base + L.tab);
  index->capacity = L.cap;
  index->xyz = (float *)(base + L.xyz);
  index->idx = (int32_t *)(base + L.idx);
  index->cells = (int32_t *)(base + L.cells);
  index->chunks = (int32_t *)(base + L.chunks);
  index->meta = (int32_t *)(base + L.meta);
  index->n = n;
  index->cell = cell;
  int32_t *cell_of = (int32_t *)ws, *cursor = (int32_t *)(ws + align256((size_t)n * 4));
  const unsigned nb = (unsigned)div_up(n, 256);
  k_ov_init<<<(unsigned)div_up(L.cap, 256), 256, 0, st>>>(index->table, L.cap, index->meta);
  k_ov_insert<<<nb, 256, 0, st>>>(points, n, 1.0 / cell, index->table, (uint32_t)(L.cap - 1), cell_of, index->meta);
  k_ov_scan<<<1, 1024, 0, st>>>(index->table, L.cap, cursor, index->cells, index->chunks, index->meta);
  k_ov_scatter<<<nb, 256, 0, st>>>(points, n, cell_of, cursor, index->xyz, index->idx);
  IMF_CHECK_LAUNCH("imf_overlap_index_build");
  return IMF_OK;
}

int imf_overlap_bound(const imf_overlap_index *indices, const int32_t *pairs, int n_pairs, int64_t max_cells,
                      int64_t *bound, void *stream) {
  IMF_REQUIRE(n_pairs >= 0 && n_pairs <= 65535, "imf_overlap_bound: n_pairs=%d", n_pairs);
  if (n_pairs == 0) return IMF_OK;
  IMF_REQUIRE(indices && pairs && bound, "imf_overlap_bound: null pointer");
  IMF_REQUIRE(max_cells >= 1 && max_cells <= kOvMaxPoints, "imf_overlap_bound: max_cells=%lld", (long long)max_cells);
  hipStream_t st = (hipStream_t)stream;
  IMF_CHECK_HIP(hipMemsetAsync(bound, 0, (size_t)n_pairs * sizeof(int64_t), st));
  k_ov_bound<<<dim3((unsigned)div_up(max_cells, 256), (unsigned)n_pairs), 256, 0, st>>>(
      indices, pairs, reinterpret_cast<unsigned long long *>(bound));
  IMF_CHECK_LAUNCH("imf_overlap_bound");
  return IMF_OK;
}

int imf_overlap_pair(const imf_overlap_index *p, const imf_overlap_index *q, float thresh, int64_t max_chunks,
                     int32_t *nn_idx, void *stream) {
  IMF_REQUIRE(p && q && nn_idx, "imf_overlap_pair: null pointer");
  IMF_REQUIRE(p->table && q->table && p->n >= 1 && q->n >= 1, "imf_overlap_pair: an index that was not built");
  IMF_REQUIRE(thresh > 0.f && thresh < 1e6f, "imf_overlap_pair: thresh=%g", (double)thresh);
  IMF_REQUIRE(p->cell == q->cell, "imf_overlap_pair: the indices have cells %g and %g", p->cell, q->cell);
  IMF_REQUIRE(p->cell >= (double)thresh * (1.0 + 1.0 / 1048576.0), "imf_overlap_pair: cell %g is not above thresh %g (1 + 2^-20)",
              p->cell, (double)thresh);
  IMF_REQUIRE(max_chunks >= 0 && max_chunks <= q->n, "imf_overlap_pair: max_chunks=%lld with n_q=%lld", (long long)max_chunks,
              (long long)q->n);
  hipStream_t st = (hipStream_t)stream;
  k_ov_fill<<<(unsigned)div_up(q->n, 256), 256, 0, st>>>(nn_idx, q->n, -1);
  if (max_chunks > 0) k_ov_pair<<<(unsigned)max_chunks, kOvThreads, 0, st>>>(*p, *q, thresh, nn_idx);
  IMF_CHECK_LAUNCH("imf_overlap_pair");
  return IMF_OK;
}

size_t imf_overlap_emit_workspace_bytes(int64_t n_q) {
  if (n_q <= 0 || n_q > kOvMaxPoints) return 0;
  return align256((size_t)div_up(n_q, kEmitBlock) * 4);
}

int imf_overlap_emit(const int32_t *nn_idx, int64_t n_q, int64_t *pairs, int64_t *out_n, void *workspace,
                     size_t workspace_bytes, void *stream) {
  IMF_REQUIRE(nn_idx && pairs && out_n && workspace, "imf_overlap_emit: null pointer");
  IMF_REQUIRE(n_q >= 1 && n_q <= kOvMaxPoints, "imf_overlap_emit: n_q=%lld", (long long)n_q);
  IMF_REQUIRE(((uintptr_t)workspace & 255) == 0, "imf_overlap_emit: workspace must be 256-byte aligned");
  IMF_REQUIRE(workspace_bytes >= imf_overlap_emit_workspace_bytes(n_q), "imf_overlap_emit: workspace %zu < %zu",
              workspace_bytes, imf_overlap_emit_workspace_bytes(n_q));
  hipStream_t st = (hipStream_t)stream;
  int32_t *block_cnt = (int32_t *)workspace;
  const int64_t nb = div_up(n_q, kEmitBlock);
  k_ov_emit_count<<<(unsigned)nb, 256, 0, st>>>(nn_idx, n_q, block_cnt);
  k_ov_emit_scan<<<1, 1024, 0, st>>>(block_cnt, nb, out_n);
  k_ov_emit_write<<<(unsigned)nb, 256, 0, st>>>(nn_idx, n_q, block_cnt, pairs);
  IMF_CHECK_LAUNCH("imf_overlap_emit");
  return IMF_OK;
}

}  // extern "C"
