// The hardest-contrastive loss of training, forward and backward (ops.TRAIN_LOSS == "hip").
//
// Reference being replaced: lib/trainer.py:440-493 `contrastive_hardest_negative_loss` and torch's autograd of it -- some
// sixty small launches around the two nearest-neighbour searches: four row gathers whose backward is an atomic index_put
// (no fixed summation order), two sort-based isin calls and boolean-mask indexing (a host wait for a size).
//
// Sampled pair s: (i_s, j_s) = pairs[pos_sel[s]], a_s = f0[i_s], b_s = f1[j_s].
//   hard01[s] = sel1[k], k = argmin_k |a_s - f1[sel1[k]]|^2;  hard10[s] = sel0[k], k = argmin_k |b_s - f0[sel0[k]]|^2
//               (imf_nn_search itself: fp64 scores of the fp32 rows, a tie goes to the lowest k; its "no neighbour"
//               answer -1 for a non-finite row reads as k = 0 with keep = 0);
//   keep01[s]   = 0 when (i_s, hard01[s]) is one of the n_pairs positive pairs, else 1;  keep10[s]: (hard10[s], j_s).
//               Membership is exact: the injective key i + j * max(n0, n1) in a key-only open-addressing set
//               (common.h hash_insert_key); integer compare-and-swap only, and a set has no order;
//   pos_loss    = mean_s relu(|a_s - b_s|^2 - pos_thresh);
//   D01_s       = sqrt(|a_s - f1[hard01_s]|^2 + 1e-7), D10_s likewise;
//   neg_loss    = (mean_{keep01} relu(neg_thresh - D01)^2 + mean_{keep10} relu(neg_thresh - D10)^2) / 2;  an empty keep set
//               makes its mean 0 / 0 = NaN as torch's mean of nothing, sends no gradient, and raises bit 0 (keep01) or
//               bit 1 (keep10) of meta[2].
//
// FORWARD ARITHMETIC.  Every term is evaluated in fp64 from the fp32 rows (differences exact, squares and sums rounded at
// 2^-53).  The three sums run over s in one fixed shape: thread t of one 1024-thread workgroup adds s = t, t + 1024, ...
// in that order, a butterfly inside each wavefront, the 16 wavefront sums in wavefront order.  Each loss is rounded once
// to fp32: |loss - exact| <= 2^-24 |exact| + O(n_pos 2^-53), all terms being non-negative.
//
// BACKWARD.  With gp = grad[0], gn = grad[1], c01 / c10 the keep counts (meta):
//   cP_s  = gp * 2 / n_pos                                  where |a_s - b_s|^2 > pos_thresh, else 0
//   c01_s = -gn * relu(neg_thresh - D01_s) / (c01 * D01_s)   where keep01[s], else 0;   c10_s likewise
//   df0[i_s]       += cP_s (a_s - b_s) + c01_s (a_s - f1[hard01_s])       df1[j_s]       += cP_s (b_s - a_s) + c10_s (b_s - f0[hard10_s])
//   df0[hard10_s]  += c10_s (f0[hard10_s] - b_s)                          df1[hard01_s]  += c01_s (f1[hard01_s] - a_s)
// (the minimum routes its gradient to the argmin only, as pdist(...).min(1) does).  Term routing: each side has 2 n_pos
// entries (row, e = 2 s + kind); an entry's place in the order of the 64-bit keys row << 32 | e is the number of smaller
// keys, counted through LDS tiles (no sort, no atomics); one wavefront then owns each run of equal rows: its 64 / (c / 4)
// lane groups add the run's entries q = g, g + G, ... in fp64, the groups are combined by a butterfly, and the row is
// rounded once to fp32.  The order depends on the indices (and c) only: two calls give the same bits.  A row without an
// entry is written as +0.0 by the first launch; the call writes all of df0 and df1.
// Per element |got - exact| <= 2^-24 * sum of |addends| + O(2^-53) of it.  No floating-point atomics anywhere.
//
// Launches: forward = one memset (the key set), one gather + set-insert kernel, the two searches, one term kernel, one
// reduction;  backward = coefficients + keys + zero fill, rank, segmented sum.
#include "common.h"

namespace imf {
namespace {

constexpr int64_t kHcMaxPos = 1 << 16;      // 2 n_pos entries per side are ranked by counting: 2^34 compares at the cap
constexpr int64_t kHcMaxPairs = 1ll << 26;  // key set of at most 2^27 slots (1 GiB)
constexpr double kHcEps = 1e-7;
constexpr int kRankTile = 256;

inline uint32_t hc_table_capacity(int64_t n_pairs) {
  uint32_t cap = 1024;
  while ((int64_t)cap < 2 * n_pairs) cap <<= 1;
  return cap;
}

// carve-up of the workspace, the same for the three entry points
struct HcLayout {
  size_t pos0, pos1, sub0, sub1, nn01, nn10, table, search, terms, keys, skeys, coef, total;
  size_t search_bytes;
  uint32_t cap;
};

HcLayout hc_layout(int64_t n_pos, int c, int64_t n_pairs, int64_t n_sel0, int64_t n_sel1) {
  HcLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t at = o;
    o += align256(bytes);
    return at;
  };
  L.cap = hc_table_capacity(n_pairs);
  const size_t s01 = imf_nn_workspace_bytes(n_pos, n_sel1), s10 = imf_nn_workspace_bytes(n_pos, n_sel0);
  L.search_bytes = s01 > s10 ? s01 : s10;
  L.pos0 = take((size_t)n_pos * c * 4);
  L.pos1 = take((size_t)n_pos * c * 4);
  L.sub0 = take((size_t)n_sel0 * c * 4);
  L.sub1 = take((size_t)n_sel1 * c * 4);
  L.nn01 = take((size_t)n_pos * 4);
  L.nn10 = take((size_t)n_pos * 4);
  L.table = take((size_t)L.cap * 8);
  L.search = take(L.search_bytes);
  L.terms = take((size_t)n_pos * 3 * 8);
  L.keys = take((size_t)n_pos * 4 * 8);    // [side][2 n_pos]
  L.skeys = take((size_t)n_pos * 4 * 8);
  L.coef = take((size_t)n_pos * 3 * 8);
  L.total = o;
  return L;
}

__device__ __forceinline__ int64_t hc_pair_row(const int64_t *__restrict__ pos_sel, int64_t s) {
  return pos_sel ? pos_sel[s] : s;
}

// Rows of the two searches, contiguous: pos0[s] = f0[i_s], pos1[s] = f1[j_s], sub0[k] = f0[sel0[k]], sub1[k] = f1[sel1[k]]
// (one float4 per thread), and the n_pairs keys into the set.
__global__ __launch_bounds__(256) void k_hc_gather(const float *__restrict__ f0, const float *__restrict__ f1, int c4,
                                                   const int64_t *__restrict__ pairs, int64_t n_pairs,
                                                   const int64_t *__restrict__ pos_sel, int64_t n_pos,
                                                   const int64_t *__restrict__ sel0, int64_t n_sel0,
                                                   const int64_t *__restrict__ sel1, int64_t n_sel1, int64_t hash_m,
                                                   float4 *__restrict__ pos0, float4 *__restrict__ pos1,
                                                   float4 *__restrict__ sub0, float4 *__restrict__ sub1,
                                                   uint64_t *__restrict__ table, uint32_t capmask) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t rows = 2 * n_pos + n_sel0 + n_sel1;
  const float4 *g0 = reinterpret_cast<const float4 *>(f0), *g1 = reinterpret_cast<const float4 *>(f1);
  for (int64_t e = tid; e < rows * c4; e += nthr) {
    int64_t r = e / c4;
    const int q = (int)(e - r * c4);
    if (r < n_pos) {
      pos0[r * c4 + q] = g0[pairs[2 * hc_pair_row(pos_sel, r)] * c4 + q];
    } else if ((r -= n_pos) < n_pos) {
      pos1[r * c4 + q] = g1[pairs[2 * hc_pair_row(pos_sel, r) + 1] * c4 + q];
    } else if ((r -= n_pos) < n_sel0) {
      sub0[r * c4 + q] = g0[sel0[r] * c4 + q];
    } else {
      r -= n_sel0;
      sub1[r * c4 + q] = g1[sel1[r] * c4 + q];
    }
  }
  for (int64_t p = tid; p < n_pairs; p += nthr)
    hash_insert_key(table, capmask, (uint64_t)(pairs[2 * p] + pairs[2 * p + 1] * hash_m));
}

// |x - y|^2 of two rows, a float4 per lane of a group of LP = C / 4 lanes; every lane of the group gets the sum
template <int LP>
__device__ __forceinline__ double hc_dist2(const float4 x, const float4 y) {
  const double d0 = (double)x.x - (double)y.x, d1 = (double)x.y - (double)y.y;
  const double d2 = (double)x.z - (double)y.z, d3 = (double)x.w - (double)y.w;
  double s = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
#pragma unroll
  for (int off = 1; off < LP; off <<= 1) s += __shfl_xor(s, off);
  return s;
}

struct HcTerm {
  int64_t i, j, h01, h10;
  double d2p, d01, d10;   // |a - b|^2, D01, D10
};

// one lane group per sampled pair: the rows' float4 of this lane and the three distances
template <int LP>
__device__ __forceinline__ HcTerm hc_term(const float *__restrict__ f0, const float *__restrict__ f1,
                                          const int64_t *__restrict__ pairs, const int64_t *__restrict__ pos_sel,
                                          int64_t s, int64_t h01, int64_t h10, int q) {
  HcTerm t;
  const int64_t p = hc_pair_row(pos_sel, s);
  t.i = pairs[2 * p];
  t.j = pairs[2 * p + 1];
  t.h01 = h01;
  t.h10 = h10;
  const float4 a = reinterpret_cast<const float4 *>(f0)[t.i * LP + q];
  const float4 b = reinterpret_cast<const float4 *>(f1)[t.j * LP + q];
  const float4 n1 = reinterpret_cast<const float4 *>(f1)[h01 * LP + q];
  const float4 n0 = reinterpret_cast<const float4 *>(f0)[h10 * LP + q];
  t.d2p = hc_dist2<LP>(a, b);
  t.d01 = sqrt(hc_dist2<LP>(a, n1) + kHcEps);
  t.d10 = sqrt(hc_dist2<LP>(b, n0) + kHcEps);
  return t;
}

template <int LP>
__global__ __launch_bounds__(256) void k_hc_terms(const float *__restrict__ f0, const float *__restrict__ f1,
                                                  const int64_t *__restrict__ pairs, const int64_t *__restrict__ pos_sel,
                                                  int64_t n_pos, const int64_t *__restrict__ sel0,
                                                  const int64_t *__restrict__ sel1, const int32_t *__restrict__ nn01,
                                                  const int32_t *__restrict__ nn10, const uint64_t *__restrict__ table,
                                                  uint32_t capmask, int64_t hash_m, double pos_thresh, double neg_thresh,
                                                  int64_t *__restrict__ hard01, int64_t *__restrict__ hard10,
                                                  uint8_t *__restrict__ keep01, uint8_t *__restrict__ keep10,
                                                  double *__restrict__ terms) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = (int)(gid % LP);
  const int64_t s_raw = gid / LP;
  const bool live = s_raw < n_pos;           // whole groups are live or not; dead groups shadow the last pair
  const int64_t s = live ? s_raw : n_pos - 1;
  // imf_nn_search answers -1 for a row without a neighbour (a non-finite feature row): gather row 0 and keep the pair
  // out of the negative term, as train/loss.py does
  const int k01_nn = nn01[s], k10_nn = nn10[s];
  const int64_t h01 = sel1[max(k01_nn, 0)], h10 = sel0[max(k10_nn, 0)];
  const HcTerm t = hc_term<LP>(f0, f1, pairs, pos_sel, s, h01, h10, q);
  if (!live || q != 0) return;
  const bool k01 = k01_nn >= 0 && !hash_contains_key(table, capmask, (uint64_t)(t.i + h01 * hash_m));
  const bool k10 = k10_nn >= 0 && !hash_contains_key(table, capmask, (uint64_t)(h10 + t.j * hash_m));
  const double r01 = fmax(neg_thresh - t.d01, 0.0), r10 = fmax(neg_thresh - t.d10, 0.0);
  hard01[s] = h01;
  hard10[s] = h10;
  keep01[s] = k01;
  keep10[s] = k10;
  terms[3 * s] = fmax(t.d2p - pos_thresh, 0.0);
  terms[3 * s + 1] = k01 ? r01 * r01 : 0.0;
  terms[3 * s + 2] = k10 ? r10 * r10 : 0.0;
}

// One workgroup: the three sums and the two keep counts in the fixed order of the header comment.
__global__ __launch_bounds__(1024) void k_hc_reduce(const double *__restrict__ terms, const uint8_t *__restrict__ keep01,
                                                    const uint8_t *__restrict__ keep10, int64_t n_pos,
                                                    float *__restrict__ loss, int32_t *__restrict__ meta) {
  __shared__ double part[16][3];
  __shared__ int cnt[16][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  int c0 = 0, c1 = 0;
  for (int64_t s = tid; s < n_pos; s += 1024) {
    a0 += terms[3 * s];
    a1 += terms[3 * s + 1];
    a2 += terms[3 * s + 2];
    c0 += keep01[s];
    c1 += keep10[s];
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    a0 += __shfl_xor(a0, off);
    a1 += __shfl_xor(a1, off);
    a2 += __shfl_xor(a2, off);
    c0 += __shfl_xor(c0, off);
    c1 += __shfl_xor(c1, off);
  }
  if (lane == 0) {
    part[wave][0] = a0;
    part[wave][1] = a1;
    part[wave][2] = a2;
    cnt[wave][0] = c0;
    cnt[wave][1] = c1;
  }
  __syncthreads();
  if (tid == 0) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int n01 = 0, n10 = 0;
    for (int w = 0; w < 16; ++w) {
      s0 += part[w][0];
      s1 += part[w][1];
      s2 += part[w][2];
      n01 += cnt[w][0];
      n10 += cnt[w][1];
    }
    loss[0] = (float)(s0 / (double)n_pos);
    loss[1] = (float)((s1 / (double)n01 + s2 / (double)n10) * 0.5);   // 0 / 0 = NaN: the mean of nothing
    meta[0] = n01;
    meta[1] = n10;
    meta[2] = (n01 == 0 ? 1 : 0) | (n10 == 0 ? 2 : 0);
    meta[3] = 0;
  }
}

// Backward 1: per sampled pair the three coefficients and its two entries on each side; every thread also zeroes its
// share of df0 / df1 (rows with entries are overwritten by k_hc_rows, which runs after this launch on the stream).
template <int LP>
__global__ __launch_bounds__(256) void k_hc_coef(const float *__restrict__ f0, const float *__restrict__ f1,
                                                 const int64_t *__restrict__ pairs, const int64_t *__restrict__ pos_sel,
                                                 int64_t n_pos, const int64_t *__restrict__ hard01,
                                                 const int64_t *__restrict__ hard10, const uint8_t *__restrict__ keep01,
                                                 const uint8_t *__restrict__ keep10, const int32_t *__restrict__ meta,
                                                 const float *__restrict__ grad, double pos_thresh, double neg_thresh,
                                                 double *__restrict__ coef, uint64_t *__restrict__ keys,
                                                 float4 *__restrict__ df0, int64_t n0_vec, float4 *__restrict__ df1,
                                                 int64_t n1_vec) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t e = gid; e < n0_vec; e += nthr) df0[e] = zero;
  for (int64_t e = gid; e < n1_vec; e += nthr) df1[e] = zero;
  const int64_t groups = nthr / LP;
  const int q = (int)(gid % LP);
  const int64_t g = gid / LP;
  const double gp = (double)grad[0], gn = (double)grad[1];
  const double n01 = (double)meta[0], n10 = (double)meta[1];
  // trip count rounded up so that whole groups stay together through the shuffles of hc_term
  for (int64_t s0 = 0; s0 < n_pos; s0 += groups) {
    const int64_t s_raw = s0 + g;
    const bool live = s_raw < n_pos;
    const int64_t s = live ? s_raw : n_pos - 1;
    const int64_t h01 = hard01[s], h10 = hard10[s];
    const HcTerm t = hc_term<LP>(f0, f1, pairs, pos_sel, s, h01, h10, q);
    if (!live || q != 0) continue;
    coef[3 * s] = t.d2p - pos_thresh > 0.0 ? gp * 2.0 / (double)n_pos : 0.0;
    coef[3 * s + 1] = keep01[s] ? -gn * fmax(neg_thresh - t.d01, 0.0) / (n01 * t.d01) : 0.0;
    coef[3 * s + 2] = keep10[s] ? -gn * fmax(neg_thresh - t.d10, 0.0) / (n10 * t.d10) : 0.0;
    const uint64_t e0 = 2 * (uint64_t)s, e1 = e0 + 1;
    keys[e0] = ((uint64_t)t.i << 32) | e0;                      // side 0: the anchor row of f0, the 10 negative
    keys[e1] = ((uint64_t)h10 << 32) | e1;
    keys[2 * n_pos + e0] = ((uint64_t)t.j << 32) | e0;          // side 1: the anchor row of f1, the 01 negative
    keys[2 * n_pos + e1] = ((uint64_t)h01 << 32) | e1;
  }
}

// Backward 2: the place of every entry in the order of its side's keys = the number of smaller keys (they are distinct).
__global__ __launch_bounds__(kRankTile) void k_hc_rank(const uint64_t *__restrict__ keys, int n_ent,
                                                       uint64_t *__restrict__ skeys) {
  __shared__ uint64_t tile[kRankTile];
  const uint64_t *k = keys + (int64_t)blockIdx.y * n_ent;
  const int e = blockIdx.x * kRankTile + threadIdx.x;
  const uint64_t mine = e < n_ent ? k[e] : kEmptyKey;
  int rank = 0;
  for (int t0 = 0; t0 < n_ent; t0 += kRankTile) {
    __syncthreads();
    tile[threadIdx.x] = t0 + threadIdx.x < n_ent ? k[t0 + threadIdx.x] : kEmptyKey;   // the padding is larger than any key
    __syncthreads();
#pragma unroll 16
    for (int u = 0; u < kRankTile; ++u) rank += tile[u] < mine ? 1 : 0;
  }
  if (e < n_ent) skeys[(int64_t)blockIdx.y * n_ent + rank] = mine;
}

// Backward 3: one wavefront per place in the order; the one at the head of a run of equal rows sums the run.
template <int LP>
__global__ __launch_bounds__(256) void k_hc_rows(const float *__restrict__ f0, const float *__restrict__ f1,
                                                 const int64_t *__restrict__ pairs, const int64_t *__restrict__ pos_sel,
                                                 int n_ent, const int64_t *__restrict__ hard01,
                                                 const int64_t *__restrict__ hard10, const double *__restrict__ coef,
                                                 const uint64_t *__restrict__ skeys, float *__restrict__ df0,
                                                 float *__restrict__ df1) {
  constexpr int G = 64 / LP;
  const int side = blockIdx.y;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n_ent) return;
  const uint64_t *sk = skeys + (int64_t)side * n_ent;
  const uint64_t row = sk[p] >> 32;
  if (p > 0 && (sk[p - 1] >> 32) == row) return;
  const int lane = threadIdx.x & 63, q = lane % LP, g = lane / LP;
  const float4 *mine = reinterpret_cast<const float4 *>(side ? f1 : f0);    // the side whose rows receive
  const float4 *other = reinterpret_cast<const float4 *>(side ? f0 : f1);
  const int64_t *hard_other = side ? hard10 : hard01;   // the negative, in `other`, of this side's anchor
  const int cneg_anchor = side ? 2 : 1, cneg_row = side ? 1 : 2;
  const float4 x = mine[(int64_t)row * LP + q];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int r = p + g; r < n_ent; r += G) {
    const uint64_t key = sk[r];
    if ((key >> 32) != row) break;
    const int64_t s = (int64_t)((uint32_t)key >> 1);
    const int64_t pr = hc_pair_row(pos_sel, s);
    const int64_t partner = pairs[2 * pr + (side ? 0 : 1)];    // the other end of the sampled pair, a row of `other`
    const float4 y = other[partner * LP + q];
    if ((key & 1) == 0) {
      // this row is the pair's own end: the positive term, then the hardest-negative term it anchors
      const double cp = coef[3 * s], cn = coef[3 * s + cneg_anchor];
      const float4 h = other[hard_other[s] * LP + q];
      a0 += cp * ((double)x.x - (double)y.x);
      a1 += cp * ((double)x.y - (double)y.y);
      a2 += cp * ((double)x.z - (double)y.z);
      a3 += cp * ((double)x.w - (double)y.w);
      a0 += cn * ((double)x.x - (double)h.x);
      a1 += cn * ((double)x.y - (double)h.y);
      a2 += cn * ((double)x.z - (double)h.z);
      a3 += cn * ((double)x.w - (double)h.w);
    } else {
      // this row is the hardest negative of the pair's other end
      const double cn = coef[3 * s + cneg_row];
      a0 += cn * ((double)x.x - (double)y.x);
      a1 += cn * ((double)x.y - (double)y.y);
      a2 += cn * ((double)x.z - (double)y.z);
      a3 += cn * ((double)x.w - (double)y.w);
    }
  }
#pragma unroll
  for (int off = LP; off < 64; off <<= 1) {
    a0 += __shfl_xor(a0, off);
    a1 += __shfl_xor(a1, off);
    a2 += __shfl_xor(a2, off);
    a3 += __shfl_xor(a3, off);
  }
  if (g == 0)
    reinterpret_cast<float4 *>(side ? df1 : df0)[(int64_t)row * LP + q] = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
}

int hc_check(const char *who, int64_t n0, int64_t n1, int c, int64_t n_pairs, int64_t n_pos, int64_t n_sel0,
             int64_t n_sel1, bool pointers, bool all_pairs, const void *workspace, size_t workspace_bytes) {
  IMF_REQUIRE(c == 16 || c == 32 || c == 64, "%s: c %d not in {16,32,64}", who, c);
  IMF_REQUIRE(n0 >= 1 && n1 >= 1 && n0 < (1ll << 30) && n1 < (1ll << 30), "%s: n0=%lld n1=%lld", who, (long long)n0,
              (long long)n1);
  IMF_REQUIRE(n_pairs >= 1 && n_pos >= 1 && n_sel0 >= 1 && n_sel1 >= 1,
              "%s: n_pairs=%lld n_pos=%lld n_sel0=%lld n_sel1=%lld (each must be at least 1)", who, (long long)n_pairs,
              (long long)n_pos, (long long)n_sel0, (long long)n_sel1);
  IMF_REQUIRE(!all_pairs || n_pos == n_pairs, "%s: pos_sel NULL takes every pair, n_pos=%lld != n_pairs=%lld", who,
              (long long)n_pos, (long long)n_pairs);
  IMF_REQUIRE(pointers && workspace, "%s: null pointer", who);
  if (n_pos > kHcMaxPos || n_pairs > kHcMaxPairs || n_sel0 >= (1ll << 30) || n_sel1 >= (1ll << 30)) {
    set_error("%s: n_pos=%lld (at most %lld) n_pairs=%lld (at most %lld)", who, (long long)n_pos, (long long)kHcMaxPos,
              (long long)n_pairs, (long long)kHcMaxPairs);
    return IMF_EUNSUPPORTED;
  }
  const size_t need = hc_layout(n_pos, c, n_pairs, n_sel0, n_sel1).total;
  IMF_REQUIRE(workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
  IMF_REQUIRE(aligned16(workspace), "%s: the workspace must be 16-byte aligned", who);
  return IMF_OK;
}

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

size_t imf_hc_loss_workspace_bytes(int64_t n0, int64_t n1, int c, int64_t n_pairs, int64_t n_pos, int64_t n_sel0,
                                   int64_t n_sel1) {
  if (n0 < 1 || n1 < 1 || (c != 16 && c != 32 && c != 64) || n_pairs < 1 || n_pos < 1 || n_sel0 < 1 || n_sel1 < 1 ||
      n_pos > kHcMaxPos || n_pairs > kHcMaxPairs || n_sel0 >= (1ll << 30) || n_sel1 >= (1ll << 30))
    return 0;
  return hc_layout(n_pos, c, n_pairs, n_sel0, n_sel1).total;
}

int imf_hc_loss_forward(const float *f0, int64_t n0, const float *f1, int64_t n1, int c, const int64_t *pairs,
                        int64_t n_pairs, const int64_t *pos_sel, int64_t n_pos, const int64_t *sel0, int64_t n_sel0,
                        const int64_t *sel1, int64_t n_sel1, double pos_thresh, double neg_thresh, float *loss,
                        int64_t *hard01, int64_t *hard10, uint8_t *keep01, uint8_t *keep10, int32_t *meta,
                        void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const bool ptrs = f0 && f1 && pairs && sel0 && sel1 && loss && hard01 && hard10 && keep01 && keep10 && meta;
  const int rc = hc_check("imf_hc_loss_forward", n0, n1, c, n_pairs, n_pos, n_sel0, n_sel1, ptrs, pos_sel == nullptr,
                          workspace, workspace_bytes);
  if (rc != IMF_OK) return rc;
  IMF_REQUIRE(aligned16(f0) && aligned16(f1), "imf_hc_loss_forward: f0 and f1 must be 16-byte aligned");
  const HcLayout L = hc_layout(n_pos, c, n_pairs, n_sel0, n_sel1);
  char *ws = (char *)workspace;
  float *pos0 = (float *)(ws + L.pos0), *pos1 = (float *)(ws + L.pos1);
  float *sub0 = (float *)(ws + L.sub0), *sub1 = (float *)(ws + L.sub1);
  int32_t *nn01 = (int32_t *)(ws + L.nn01), *nn10 = (int32_t *)(ws + L.nn10);
  uint64_t *table = (uint64_t *)(ws + L.table);
  double *terms = (double *)(ws + L.terms);
  const int64_t hash_m = n0 > n1 ? n0 : n1;
  const int c4 = c / 4;

  IMF_CHECK_HIP(hipMemsetAsync(table, 0xFF, (size_t)L.cap * 8, stream));
  const int64_t work = (2 * n_pos + n_sel0 + n_sel1) * c4;
  int64_t blocks = div_up(work > n_pairs ? work : n_pairs, 256);
  if (blocks > 2048) blocks = 2048;
  k_hc_gather<<<(unsigned)blocks, 256, 0, stream>>>(f0, f1, c4, pairs, n_pairs, pos_sel, n_pos, sel0, n_sel0, sel1, n_sel1,
                                                   hash_m, (float4 *)pos0, (float4 *)pos1, (float4 *)sub0,
                                                   (float4 *)sub1, table, L.cap - 1);
  IMF_CHECK_LAUNCH("imf_hc_loss_forward");
  int rs = imf_nn_search(pos0, n_pos, sub1, n_sel1, c, nn01, nullptr, ws + L.search, L.search_bytes, stream_);
  if (rs != IMF_OK) return rs;
  rs = imf_nn_search(pos1, n_pos, sub0, n_sel0, c, nn10, nullptr, ws + L.search, L.search_bytes, stream_);
  if (rs != IMF_OK) return rs;
  const unsigned tb = (unsigned)div_up(n_pos * c4, 256);
#define IMF_HC_TERMS(LP)                                                                                              \
  k_hc_terms<LP><<<tb, 256, 0, stream>>>(f0, f1, pairs, pos_sel, n_pos, sel0, sel1, nn01, nn10, table, L.cap - 1,     \
                                         hash_m, pos_thresh, neg_thresh, hard01, hard10, keep01, keep10, terms)
  if (c == 16)
    IMF_HC_TERMS(4);
  else if (c == 32)
    IMF_HC_TERMS(8);
  else
    IMF_HC_TERMS(16);
#undef IMF_HC_TERMS
  k_hc_reduce<<<1, 1024, 0, stream>>>(terms, keep01, keep10, n_pos, loss, meta);
  IMF_CHECK_LAUNCH("imf_hc_loss_forward");
  return IMF_OK;
}

int imf_hc_loss_backward(const float *f0, int64_t n0, const float *f1, int64_t n1, int c, const int64_t *pairs,
                         int64_t n_pairs, const int64_t *pos_sel, int64_t n_pos, const int64_t *sel0, int64_t n_sel0,
                         const int64_t *sel1, int64_t n_sel1, double pos_thresh, double neg_thresh,
                         const int64_t *hard01, const int64_t *hard10, const uint8_t *keep01, const uint8_t *keep10,
                         const int32_t *meta, const float *grad, float *df0, float *df1, void *workspace,
                         size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const bool ptrs = f0 && f1 && pairs && sel0 && sel1 && hard01 && hard10 && keep01 && keep10 && meta && grad && df0 && df1;
  const int rc = hc_check("imf_hc_loss_backward", n0, n1, c, n_pairs, n_pos, n_sel0, n_sel1, ptrs, pos_sel == nullptr,
                          workspace, workspace_bytes);
  if (rc != IMF_OK) return rc;
  IMF_REQUIRE(aligned16(f0) && aligned16(f1) && aligned16(df0) && aligned16(df1),
              "imf_hc_loss_backward: f0, f1, df0 and df1 must be 16-byte aligned");
  const HcLayout L = hc_layout(n_pos, c, n_pairs, n_sel0, n_sel1);
  char *ws = (char *)workspace;
  uint64_t *keys = (uint64_t *)(ws + L.keys), *skeys = (uint64_t *)(ws + L.skeys);
  double *coef = (double *)(ws + L.coef);
  const int c4 = c / 4;
  const int n_ent = (int)(2 * n_pos);
  const int64_t n0_vec = n0 * c4, n1_vec = n1 * c4;
  int64_t big = n0_vec > n1_vec ? n0_vec : n1_vec;
  if (big < n_pos * c4) big = n_pos * c4;
  int64_t blocks = div_up(big, 256);
  if (blocks > 2048) blocks = 2048;
  const dim3 rank_grid((unsigned)div_up(n_ent, kRankTile), 2), rows_grid((unsigned)div_up(n_ent, 4), 2);
#define IMF_HC_BACKWARD(LP)                                                                                           \
  do {                                                                                                                \
    k_hc_coef<LP><<<(unsigned)blocks, 256, 0, stream>>>(f0, f1, pairs, pos_sel, n_pos, hard01, hard10, keep01, keep10, \
                                                        meta, grad, pos_thresh, neg_thresh, coef, keys, (float4 *)df0, \
                                                        n0_vec, (float4 *)df1, n1_vec);                               \
    k_hc_rank<<<rank_grid, kRankTile, 0, stream>>>(keys, n_ent, skeys);                                               \
    k_hc_rows<LP><<<rows_grid, 256, 0, stream>>>(f0, f1, pairs, pos_sel, n_ent, hard01, hard10, coef, skeys, df0, df1); \
  } while (0)
  if (c == 16)
    IMF_HC_BACKWARD(4);
  else if (c == 32)
    IMF_HC_BACKWARD(8);
  else
    IMF_HC_BACKWARD(16);
#undef IMF_HC_BACKWARD
  IMF_CHECK_LAUNCH("imf_hc_loss_backward");
  return IMF_OK;
}

}  // extern "C"
