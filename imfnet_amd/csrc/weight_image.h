// The bf16x3 weight image (variant 3): its layout and the split of a value, shared by the kernel that packs an image from
// a kernel tensor (spconv_pack.hip) and the optimizer step that writes the images of the weights it updates (optim.hip).
//
// Image of a kernel W [kvol, cin, cout] (cin % 32 == 0, cout % 32 == 0): [y][k][cc][q = 3 cb + part][lane][t] in bf16, with
//   ci = 32 cc + 16 (t >> 2) + 4 (lane >> 4) + (t & 3),  co = y CW + 16 cb + (lane & 15),  CB = co_blk_of(cout), CW = 16 CB.
// One ENTRY is the 8 values (t = 0..7, 16 bytes) of one (y, k, cc, cb, lane); its parts 1 and 2 follow 64 and 128 entries
// later.  Entries in forward order e = (((y kvol + k) ncc + cc) CB + cb) 64 + lane enumerate the kernel's elements once.
#pragma once
#include "spconv_shared.h"

namespace imf {

struct B3Entry {
  int y, k, cc, cb, lane;
};

// entry e of the forward order -> its coordinates
__host__ __device__ inline B3Entry b3_entry_of(long long e, int kvol, int cin, int cout) {
  const unsigned CB = co_blk_of(cout), ncc = cin / 32;
  B3Entry n;
  n.lane = (int)(e & 63);
  unsigned r = (unsigned)(e >> 6);   // 32-bit divisions: an image has far fewer than 2^38 entries
  n.cb = (int)(r % CB); r /= CB;
  n.cc = (int)(r % ncc); r /= ncc;
  n.k = (int)(r % (unsigned)kvol); r /= (unsigned)kvol;
  n.y = (int)r;
  return n;
}
__host__ __device__ inline int b3_ci(const B3Entry &n, int t) { return n.cc * 32 + 16 * (t >> 2) + 4 * (n.lane >> 4) + (t & 3); }
__host__ __device__ inline int b3_co(const B3Entry &n, int cout) { return n.y * 16 * co_blk_of(cout) + 16 * n.cb + (n.lane & 15); }

// where part 0 of an entry sits in the image, in entries (x 8 bf16)
__host__ __device__ inline long long b3_entry_index(const B3Entry &n, int kvol, int cin, int cout) {
  const int CB = co_blk_of(cout), ncc = cin / 32;
  return ((((long long)n.y * kvol + n.k) * ncc + n.cc) * (3 * CB) + 3 * n.cb) * 64 + n.lane;
}
constexpr int kB3PartStride = 64 * 8;   // bf16 between the parts of one value

// element (k, ci, co) -> the entry that holds it and its place t inside the entry (the inverse of b3_ci / b3_co)
__host__ __device__ inline B3Entry b3_entry_at(int k, int ci, int co, int cout, int *t) {
  const int CW = 16 * co_blk_of(cout), c32 = ci & 31;
  B3Entry n;
  n.k = k;
  n.y = co / CW;
  n.cb = (co % CW) >> 4;
  n.cc = ci >> 5;
  n.lane = (((c32 & 15) >> 2) << 4) | (co & 15);
  *t = ((c32 >> 4) << 2) | (c32 & 3);
  return n;
}

// v = p0 + p1 + p2 exactly (round-to-nearest-even; the residuals are exact fp32 differences): split_b3 for one value
__device__ __forceinline__ void b3_split(float v, __bf16 &p0, __bf16 &p1, __bf16 &p2) {
  p0 = (__bf16)v;
  const float r1 = v - (float)p0;
  p1 = (__bf16)r1;
  p2 = (__bf16)(r1 - (float)p1);
}

}  // namespace imf
