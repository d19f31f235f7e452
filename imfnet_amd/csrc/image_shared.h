// What the inference image branch (image.hip) and the training entry points (image_train.hip) share: the trunk's
// shapes, the layout of a static pixel table, the kernel that fills one and the stem's im2col kernel.
#pragma once
#include "common.h"

namespace imf {
namespace {

struct ImgShape {
  int B, H, W;          // input image
  int H2, W2;           // after the 7x7 stride-2 stem
  int H4, W4;           // after the 3x3 stride-2 max pool (layer1 resolution)
  int H8, W8;           // layer2 resolution; tokens per image = H8 * W8
  int64_t n2, n4, n8;   // rows (B * H * W) at each resolution
};

ImgShape shape_of(int B, int H, int W) {
  ImgShape s;
  s.B = B; s.H = H; s.W = W;
  s.H2 = (H + 6 - 7) / 2 + 1; s.W2 = (W + 6 - 7) / 2 + 1;
  s.H4 = (s.H2 + 2 - 3) / 2 + 1; s.W4 = (s.W2 + 2 - 3) / 2 + 1;
  s.H8 = (s.H4 + 2 - 3) / 2 + 1; s.W8 = (s.W4 + 2 - 3) / 2 + 1;
  s.n2 = (int64_t)B * s.H2 * s.W2; s.n4 = (int64_t)B * s.H4 * s.W4; s.n8 = (int64_t)B * s.H8 * s.W8;
  return s;
}

constexpr int kStemK = 160;     // 7*7*3 = 147 im2col columns, zero-padded to a multiple of 32

struct Table {   // static rulebook of one dense convolution geometry
  int32_t *tile_rows, *nbr;
  uint32_t *tile_mask;
  int64_t n_slots, n_out;
  int kvol;
};

size_t table_words(int64_t n_out, int kvol) {
  const int64_t n_slots = imf_rulebook_slots(n_out);
  return (size_t)n_slots * (1 + kvol) + (size_t)(n_slots / IMF_TILE_ROWS) * IMF_MASK_WORDS;
}

int32_t *place_table(Table &t, int32_t *p, int64_t n_out, int kvol) {
  t.n_out = n_out; t.kvol = kvol; t.n_slots = imf_rulebook_slots(n_out);
  t.tile_rows = p; p += t.n_slots;
  t.nbr = p; p += (size_t)kvol * t.n_slots;
  t.tile_mask = (uint32_t *)p; p += (size_t)(t.n_slots / IMF_TILE_ROWS) * IMF_MASK_WORDS;
  return p;
}

// ---- static tables ------------------------------------------------------------------------------------
// one thread per (slot, k), slot fastest (the layout of geometry.hip's k_rulebook): in = out * stride + tap - pad
__global__ void __launch_bounds__(256)
k_img_rulebook(int B, int Hin, int Win, int Hout, int Wout, int ksize, int stride, int pad, int64_t n_slots,
               int32_t *__restrict__ tile_rows, int32_t *__restrict__ nbr, uint32_t *__restrict__ tile_mask) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int kvol = ksize * ksize;
  if (idx >= n_slots * kvol) return;
  const int k = (int)(idx / n_slots);
  const int64_t slot = idx - (int64_t)k * n_slots;
  const int64_t n_out = (int64_t)B * Hout * Wout;
  const int row = slot < n_out ? (int)slot : -1;
  if (k == 0) tile_rows[slot] = row;
  int found = -1;
  if (row >= 0) {
    const int b = row / (Hout * Wout), r = row - b * (Hout * Wout);
    const int oy = r / Wout, ox = r - oy * Wout;
    const int iy = oy * stride + k / ksize - pad, ix = ox * stride + k % ksize - pad;
    if (iy >= 0 && iy < Hin && ix >= 0 && ix < Win) found = (b * Hin + iy) * Win + ix;
  }
  nbr[idx] = found;
  const unsigned long long any = __ballot(found >= 0);
  if (any != 0ull && (threadIdx.x & 63) == 0)
    atomicOr(tile_mask + (slot >> 6) * IMF_MASK_WORDS + (k >> 5), 1u << (k & 31));
}

// ---- stem: im2col of the 7x7 stride-2 pad-3 convolution (model/resnet.py:141,199) ---------------------
// column c = (ky*7 + kx)*3 + ch (the order the host lays the stem weight out in); columns 147..159 = 0
__global__ void __launch_bounds__(256)
k_img_im2col7(const float *__restrict__ img, int B, int H, int W, int Ho, int Wo, float *__restrict__ out,
              int32_t *flags) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)B * Ho * Wo * kStemK;
  if (idx >= total) return;
  const int c = (int)(idx % kStemK);
  const int64_t row = idx / kStemK;
  float v = 0.f;
  if (c < 147) {
    const int tap = c / 3, ch = c - 3 * tap, ky = tap / 7, kx = tap - 7 * ky;
    const int b = (int)(row / (Ho * Wo)), r = (int)(row - (int64_t)b * Ho * Wo);
    const int oy = r / Wo, ox = r - oy * Wo;
    const int iy = 2 * oy + ky - 3, ix = 2 * ox + kx - 3;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = img[(((int64_t)b * 3 + ch) * H + iy) * W + ix];
  }
  if (flags && !(fabsf(v) < 65504.f)) atomicOr(flags, 32);   // pixel values must fit the f16 operands of the stem
  out[idx] = v;
}

}  // namespace
}  // namespace imf
