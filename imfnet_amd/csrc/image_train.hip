// Training of the image trunk (model/resnet.py:195-216 under loss.backward(), lib/trainer.py:495-569): the pieces the
// training path needs beside imf_spconv_fwd / imf_spconv_wgrad / imf_bn_train_*.
//
//   tables    the four static pixel tables of the inference branch (image_shared.h) plus the OPPOSITE direction of the two
//             stride-2 geometries: the input gradient of a convolution is a convolution of the output gradient over the
//             map read backwards (rows = input pixels, neighbours = the output pixels that read them);
//   im2col    the stem's 7x7 / 2 patch matrix as an entry point of its own (the inference kernel, no range flag);
//   max pool  3x3 / 2 / pad 1 on NHWC rows that remembers which tap won, and its backward as a GATHER over the at most
//             four windows a pixel belongs to: fp64 sum in a fixed order, one rounding, no atomics, every element written.
#include <string.h>

#include "common.h"
#include "image_shared.h"

namespace imf {
namespace {

// one thread per (slot, k), slot fastest, rows = INPUT pixels of the convolution out = in * stride + tap - pad:
// nbr[k][i] = o  <=>  the forward table has nbr[k][o] = i.  A pixel no output reads through tap k gets -1.
// force_tap0: mark tap 0 active in every tile that holds a row, neighbour or not.  imf_spconv_fwd skips a tile whose
// mask is empty and leaves its rows unwritten; with the bit set it walks the tile and writes +0.0 to a row without a
// neighbour.  Only the 1x1 stride-2 geometry has such rows (pixels with an odd coordinate).
__global__ void __launch_bounds__(256)
k_img_rulebook_opposite(int B, int Hin, int Win, int Hout, int Wout, int ksize, int stride, int pad, int64_t n_slots,
                        int force_tap0, int32_t *__restrict__ tile_rows, int32_t *__restrict__ nbr,
                        uint32_t *__restrict__ tile_mask) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int kvol = ksize * ksize;
  if (idx >= n_slots * kvol) return;
  const int k = (int)(idx / n_slots);
  const int64_t slot = idx - (int64_t)k * n_slots;
  const int64_t n_rows = (int64_t)B * Hin * Win;
  const int row = slot < n_rows ? (int)slot : -1;
  if (k == 0) tile_rows[slot] = row;
  int found = -1;
  if (row >= 0) {
    const int b = row / (Hin * Win), r = row - b * (Hin * Win);
    const int iy = r / Win, ix = r - iy * Win;
    const int ny = iy + pad - k / ksize, nx = ix + pad - k % ksize;   // = o * stride
    if (ny >= 0 && nx >= 0 && ny % stride == 0 && nx % stride == 0) {
      const int oy = ny / stride, ox = nx / stride;
      if (oy < Hout && ox < Wout) found = (b * Hout + oy) * Wout + ox;
    }
  }
  nbr[idx] = found;
  const unsigned long long any = __ballot(found >= 0 || (force_tap0 && k == 0 && row >= 0));
  if (any != 0ull && (threadIdx.x & 63) == 0)
    atomicOr(tile_mask + (slot >> 6) * IMF_MASK_WORDS + (k >> 5), 1u << (k & 31));
}

// ---- max pool 3x3 / 2 / pad 1 on NHWC rows, 4 channels per thread ----------------------------------------------------------
// torch's rule (aten/native/cpu/MaxPoolKernel.cpp): taps in (ky, kx) row-major order, a later one replaces the current
// one when it is greater or NaN; the winner's tap ky*3+kx is stored per element.
__device__ __forceinline__ void pool_take(float v, int k, float &m, int &t) {
  if (v > m || v != v) { m = v; t = k; }
}

__global__ void __launch_bounds__(256)
k_img_maxpool_fwd(const float *__restrict__ in, int B, int Hin, int Win, int Hout, int Wout, int C,
                  float *__restrict__ out, uint8_t *__restrict__ tap) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4n = C / 4;
  const int64_t total = (int64_t)B * Hout * Wout * c4n;
  if (idx >= total) return;
  const int c4 = (int)(idx % c4n);
  const int64_t row = idx / c4n;
  const int b = (int)(row / (Hout * Wout)), r = (int)(row - (int64_t)b * Hout * Wout);
  const int oy = r / Wout, ox = r - oy * Wout;
  const float ninf = -__builtin_huge_valf();
  float4 m = make_float4(ninf, ninf, ninf, ninf);
  const int first = (oy == 0 ? 3 : 0) + (ox == 0 ? 1 : 0);   // the first tap inside the map: what torch starts from
  int tx = first, ty = first, tz = first, tw = first;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy + ky - 1;
    if (iy < 0 || iy >= Hin) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox + kx - 1;
      if (ix < 0 || ix >= Win) continue;
      const float4 v = *reinterpret_cast<const float4 *>(in + (((int64_t)b * Hin + iy) * Win + ix) * C + 4 * c4);
      const int k = ky * 3 + kx;
      pool_take(v.x, k, m.x, tx); pool_take(v.y, k, m.y, ty); pool_take(v.z, k, m.z, tz); pool_take(v.w, k, m.w, tw);
    }
  }
  *reinterpret_cast<float4 *>(out + row * C + 4 * c4) = m;
  *reinterpret_cast<uchar4 *>(tap + row * C + 4 * c4) = make_uchar4((unsigned char)tx, (unsigned char)ty, (unsigned char)tz,
                                                                    (unsigned char)tw);
}

// one thread per INPUT pixel and 4 channels: the windows (oy, ox) with 2 o + k - 1 = i, ascending (oy, ox)
__global__ void __launch_bounds__(256)
k_img_maxpool_bwd(const float *__restrict__ dout, const uint8_t *__restrict__ tap, int B, int Hin, int Win, int Hout,
                  int Wout, int C, float *__restrict__ din) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4n = C / 4;
  const int64_t total = (int64_t)B * Hin * Win * c4n;
  if (idx >= total) return;
  const int c4 = (int)(idx % c4n);
  const int64_t row = idx / c4n;
  const int b = (int)(row / (Hin * Win)), r = (int)(row - (int64_t)b * Hin * Win);
  const int iy = r / Win, ix = r - iy * Win;
  const int oy_lo = iy / 2, oy_hi = min(Hout - 1, (iy + 1) / 2);
  const int ox_lo = ix / 2, ox_hi = min(Wout - 1, (ix + 1) / 2);
  double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
  for (int oy = oy_lo; oy <= oy_hi; ++oy) {
    const int ky = iy + 1 - 2 * oy;
    for (int ox = ox_lo; ox <= ox_hi; ++ox) {
      const int k = ky * 3 + (ix + 1 - 2 * ox);
      const int64_t o = (((int64_t)b * Hout + oy) * Wout + ox) * C + 4 * c4;
      const uchar4 t = *reinterpret_cast<const uchar4 *>(tap + o);
      const float4 g = *reinterpret_cast<const float4 *>(dout + o);
      if (t.x == k) sx += (double)g.x;
      if (t.y == k) sy += (double)g.y;
      if (t.z == k) sz += (double)g.z;
      if (t.w == k) sw += (double)g.w;
    }
  }
  *reinterpret_cast<float4 *>(din + row * C + 4 * c4) = make_float4((float)sx, (float)sy, (float)sz, (float)sw);
}

struct TrainPlan {
  Table t4, t48, t48T, td, tdT, t8;
  size_t bytes;
};

TrainPlan train_plan_of(const ImgShape &s, void *storage) {
  TrainPlan p;
  int32_t *ip = (int32_t *)storage;
  ip = place_table(p.t4, ip, s.n4, 9);
  ip = place_table(p.t48, ip, s.n8, 9);
  ip = place_table(p.t48T, ip, s.n4, 9);
  ip = place_table(p.td, ip, s.n8, 1);
  ip = place_table(p.tdT, ip, s.n4, 1);
  ip = place_table(p.t8, ip, s.n8, 9);
  p.bytes = align256((size_t)((char *)ip - (char *)storage));
  return p;
}

bool image_shape_ok(int B, int H, int W) {
  return B >= 1 && H >= 8 && W >= 8 && (int64_t)B * H * W < (1ll << 31);
}

imf_image_table public_table(const Table &t) {
  imf_image_table o;
  o.tile_rows = t.tile_rows; o.nbr = t.nbr; o.tile_mask = t.tile_mask;
  o.n_slots = t.n_slots; o.n_out = t.n_out; o.kvol = t.kvol;
  return o;
}

bool pool_args_ok(int B, int Hin, int Win, int C) {
  return B >= 1 && Hin >= 1 && Win >= 1 && C >= 4 && C % 4 == 0 && (int64_t)B * Hin * Win < (1ll << 31);
}

}  // namespace
}  // namespace imf

using namespace imf;

extern "C" {

size_t imf_image_train_tables_bytes(int B, int H, int W) {
  if (!image_shape_ok(B, H, W)) return 0;
  return train_plan_of(shape_of(B, H, W), nullptr).bytes;
}

int imf_image_train_tables_build(int B, int H, int W, void *storage, size_t storage_bytes, imf_image_train_tables *out,
                                 void *stream) {
  IMF_REQUIRE(storage && out, "imf_image_train_tables_build: null pointer");
  IMF_REQUIRE(image_shape_ok(B, H, W), "imf_image_train_tables_build: B=%d H=%d W=%d", B, H, W);
  IMF_REQUIRE(((uintptr_t)storage & 255) == 0, "imf_image_train_tables_build: storage must be 256-byte aligned");
  IMF_REQUIRE(storage_bytes >= imf_image_train_tables_bytes(B, H, W), "imf_image_train_tables_build: storage too small");
  const ImgShape s = shape_of(B, H, W);
  const TrainPlan p = train_plan_of(s, storage);
  hipStream_t st = (hipStream_t)stream;
  IMF_CHECK_HIP(hipMemsetAsync(storage, 0, p.bytes, st));   // the masks are OR-ed together
  auto build = [&](const Table &t, int Hin, int Win, int Hout, int Wout, int ksize, int stride, int pad) {
    k_img_rulebook<<<(unsigned)div_up(t.n_slots * t.kvol, 256), 256, 0, st>>>(
        s.B, Hin, Win, Hout, Wout, ksize, stride, pad, t.n_slots, t.tile_rows, t.nbr, t.tile_mask);
  };
  auto opposite = [&](const Table &t, int Hin, int Win, int Hout, int Wout, int ksize, int stride, int pad, int force) {
    k_img_rulebook_opposite<<<(unsigned)div_up(t.n_slots * t.kvol, 256), 256, 0, st>>>(
        s.B, Hin, Win, Hout, Wout, ksize, stride, pad, t.n_slots, force, t.tile_rows, t.nbr, t.tile_mask);
  };
  build(p.t4, s.H4, s.W4, s.H4, s.W4, 3, 1, 1);
  build(p.t48, s.H4, s.W4, s.H8, s.W8, 3, 2, 1);
  opposite(p.t48T, s.H4, s.W4, s.H8, s.W8, 3, 2, 1, 0);
  build(p.td, s.H4, s.W4, s.H8, s.W8, 1, 2, 0);
  opposite(p.tdT, s.H4, s.W4, s.H8, s.W8, 1, 2, 0, 1);
  build(p.t8, s.H8, s.W8, s.H8, s.W8, 3, 1, 1);
  IMF_CHECK_LAUNCH("k_img_rulebook");
  out->t4 = public_table(p.t4); out->t48 = public_table(p.t48); out->t48T = public_table(p.t48T);
  out->td = public_table(p.td); out->tdT = public_table(p.tdT); out->t8 = public_table(p.t8);
  return IMF_OK;
}

int imf_image_im2col7(const float *image, int B, int H, int W, float *out, void *stream) {
  IMF_REQUIRE(image && out, "imf_image_im2col7: null pointer");
  IMF_REQUIRE(image_shape_ok(B, H, W), "imf_image_im2col7: B=%d H=%d W=%d", B, H, W);
  const ImgShape s = shape_of(B, H, W);
  const int64_t total = s.n2 * kStemK;
  IMF_REQUIRE(div_up(total, 256) < (1ll << 31), "imf_image_im2col7: %lld elements", (long long)total);
  k_img_im2col7<<<(unsigned)div_up(total, 256), 256, 0, (hipStream_t)stream>>>(image, B, H, W, s.H2, s.W2, out, nullptr);
  IMF_CHECK_LAUNCH("k_img_im2col7");
  return IMF_OK;
}

int imf_image_maxpool_forward(const float *in, int B, int Hin, int Win, int C, float *out, uint8_t *tap, void *stream) {
  IMF_REQUIRE(in && out && tap, "imf_image_maxpool_forward: null pointer");
  IMF_REQUIRE(pool_args_ok(B, Hin, Win, C), "imf_image_maxpool_forward: B=%d Hin=%d Win=%d C=%d (C %% 4 == 0)", B, Hin, Win, C);
  IMF_REQUIRE(aligned16(in) && aligned16(out) && ((uintptr_t)tap & 3) == 0,
              "imf_image_maxpool_forward: in / out must be 16-byte aligned, tap 4-byte aligned");
  const int Hout = (Hin - 1) / 2 + 1, Wout = (Win - 1) / 2 + 1;
  const int64_t total = (int64_t)B * Hout * Wout * (C / 4);
  IMF_REQUIRE(div_up(total, 256) < (1ll << 31), "imf_image_maxpool_forward: %lld threads", (long long)total);
  k_img_maxpool_fwd<<<(unsigned)div_up(total, 256), 256, 0, (hipStream_t)stream>>>(in, B, Hin, Win, Hout, Wout, C, out, tap);
  IMF_CHECK_LAUNCH("k_img_maxpool_fwd");
  return IMF_OK;
}

int imf_image_maxpool_backward(const float *dout, const uint8_t *tap, int B, int Hin, int Win, int C, float *din,
                               void *stream) {
  IMF_REQUIRE(dout && tap && din, "imf_image_maxpool_backward: null pointer");
  IMF_REQUIRE(pool_args_ok(B, Hin, Win, C), "imf_image_maxpool_backward: B=%d Hin=%d Win=%d C=%d (C %% 4 == 0)", B, Hin, Win, C);
  IMF_REQUIRE(aligned16(dout) && aligned16(din) && ((uintptr_t)tap & 3) == 0,
              "imf_image_maxpool_backward: dout / din must be 16-byte aligned, tap 4-byte aligned");
  const int Hout = (Hin - 1) / 2 + 1, Wout = (Win - 1) / 2 + 1;
  const int64_t total = (int64_t)B * Hin * Win * (C / 4);
  IMF_REQUIRE(div_up(total, 256) < (1ll << 31), "imf_image_maxpool_backward: %lld threads", (long long)total);
  k_img_maxpool_bwd<<<(unsigned)div_up(total, 256), 256, 0, (hipStream_t)stream>>>(dout, tap, B, Hin, Win, Hout, Wout, C, din);
  IMF_CHECK_LAUNCH("k_img_maxpool_bwd");
  return IMF_OK;
}

}  // extern "C"
