// The SGD step of training as ONE launch over every parameter (ops.TRAIN_OPTIM == "hip", train/optim.py FusedSGD), which
// also leaves the bf16x3 operand images of the convolution weights it has just written.
//
// torch.optim.SGD with dampening 0, no Nesterov, per element in fp32, every operation rounded once:
//   d  = g + wd p          (wd == 0: d = g, as torch skips the term)
//   b' = mu b + d          (the first step of a tensor: b' = d -- torch clones the gradient; mu == 0: no buffer, b' = d)
//   p' = p - lr b'
// Contraction into fused multiply-adds is off for the file, so the result is defined bit for bit and a NumPy float32
// restatement reproduces it (tests/optim_restate.py).  torch's own kernels may contract a + alpha * b: the two agree within
// the bound of tests/test_gpu_optim.py, not necessarily in every bit.
//
// Work split: a device table of imf_sgd_record (one per tensor) and a device block map of (record, chunk) pairs -- a
// workgroup serves one chunk of IMF_SGD_CHUNK elements of one tensor; nothing is shared between workgroups: no atomics, no
// host wait.  Two kinds of record:
//   plain     element i = chunk base + 256 j + thread: coalesced loads and stores, nothing else;
//   packable  a convolution weight with cin % 32 == 0, cout % 32 == 0, kvol <= 27 in the ME layout [kvol, cin, cout]
//             (2-D when kvol == 1) or torch's [cout, cin, kh, kw]: the elements are walked in the order of the FORWARD
//             image (weight_image.h) -- a thread owns one entry, the 8 values t = 0..7 of one (y, k, cc, cb, lane) --, each
//             is read, updated and written once, and its three bf16 parts go to both images: the forward one of
//             W[k][ci][co] as three 16-byte stores per thread (a wavefront writes 1 KiB runs), the backward one of
//             W'[k'][co][ci] = W[k][ci][co], k' = kvol - 1 - k when the record flips the taps, as 2-byte stores (the
//             transposition scatters an entry's 8 values over 8 entries).  Either image pointer may be null.
// The parameter reads of a packable record run over 16 consecutive co per t (64-byte segments, ME layout) or are strided
// by kvol (torch layout); both are read exactly once and the weights are a few MB, so this stays far below the launch
// overheads it removes.
#include "weight_image.h"

#pragma clang fp contract(off)

namespace imf {

constexpr int kSgdThreads = 256;
constexpr int kSgdPerThread = IMF_SGD_CHUNK / kSgdThreads;
static_assert(kSgdPerThread == 8, "a thread of a packable record owns one 8-value image entry");

__device__ __forceinline__ float sgd_element(float p, float g, float b, bool has_buf, bool first, float lr, float mu, float wd,
                                             float &b_out) {
  float d = g;
  if (wd != 0.f) d = g + wd * p;
  float bn = d;
  if (has_buf && !first) bn = mu * b + d;
  b_out = bn;
  return p - lr * bn;
}

__global__ void __launch_bounds__(kSgdThreads)
k_sgd_step(const imf_sgd_record *__restrict__ records, int n_records, const int32_t *__restrict__ block_map, float lr,
           float mu, float wd) {
  const int r = block_map[2 * blockIdx.x], chunk = block_map[2 * blockIdx.x + 1];
  if (r < 0 || r >= n_records || chunk < 0) return;
  const imf_sgd_record rec = records[r];
  float *const __restrict__ param = rec.param;
  const float *const __restrict__ grad = rec.grad;
  float *const __restrict__ mom = rec.momentum;
  const bool has_buf = mom != nullptr, first = rec.first_step != 0;
  const long long base = (long long)chunk * IMF_SGD_CHUNK;

  if (rec.layout == IMF_SGD_PLAIN) {
#pragma unroll
    for (int j = 0; j < kSgdPerThread; ++j) {
      const long long i = base + j * kSgdThreads + threadIdx.x;
      if (i < rec.numel) {
        float bn;
        const float pn = sgd_element(param[i], grad[i], (has_buf && !first) ? mom[i] : 0.f, has_buf, first, lr, mu, wd, bn);
        if (has_buf) mom[i] = bn;
        param[i] = pn;
      }
    }
    return;
  }

  // packable: entry e of the forward image's order
  const int kvol = rec.kvol, cin = rec.cin, cout = rec.cout;
  const long long e = (long long)chunk * kSgdThreads + threadIdx.x;
  if (e * 8 >= rec.numel) return;
  const B3Entry n = b3_entry_of(e, kvol, cin, cout);
  const int co = b3_co(n, cout);
  const int kb = rec.flip ? kvol - 1 - n.k : n.k;
  __bf16 *const __restrict__ img_f = reinterpret_cast<__bf16 *>(rec.image_fwd);
  __bf16 *const __restrict__ img_b = reinterpret_cast<__bf16 *>(rec.image_bwd);
  bf16x8 p0, p1, p2;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int ci = b3_ci(n, t);
    const long long i = rec.layout == IMF_SGD_ME ? ((long long)n.k * cin + ci) * cout + co
                                                 : ((long long)co * cin + ci) * kvol + n.k;
    float bn;
    const float pn = sgd_element(param[i], grad[i], (has_buf && !first) ? mom[i] : 0.f, has_buf, first, lr, mu, wd, bn);
    if (has_buf) mom[i] = bn;
    param[i] = pn;
    __bf16 h0, h1, h2;
    b3_split(pn, h0, h1, h2);
    p0[t] = h0;
    p1[t] = h1;
    p2[t] = h2;
    if (img_b) {   // the image of W'[kb][co][ci]: cin' = cout, cout' = cin
      int tb;
      const B3Entry nb = b3_entry_at(kb, co, ci, cin, &tb);
      __bf16 *const dst = img_b + b3_entry_index(nb, kvol, cout, cin) * 8 + tb;
      dst[0] = h0;
      dst[kB3PartStride] = h1;
      dst[2 * kB3PartStride] = h2;
    }
  }
  if (img_f) {
    __bf16 *const dst = img_f + b3_entry_index(n, kvol, cin, cout) * 8;
    *reinterpret_cast<bf16x8 *>(dst) = p0;
    *reinterpret_cast<bf16x8 *>(dst + kB3PartStride) = p1;
    *reinterpret_cast<bf16x8 *>(dst + 2 * kB3PartStride) = p2;
  }
}

}  // namespace imf

using namespace imf;

extern "C" int imf_sgd_chunk(void) { return IMF_SGD_CHUNK; }

extern "C" int imf_sgd_record_layout(int field, size_t *offset, size_t *size) {
  IMF_REQUIRE(offset && size, "imf_sgd_record_layout: null pointer");
#define IMF_SGD_FIELD(name) {offsetof(imf_sgd_record, name), sizeof(((imf_sgd_record *)0)->name)}
  static const size_t fields[IMF_SGD_RECORD_FIELDS][2] = {
      IMF_SGD_FIELD(param),     IMF_SGD_FIELD(grad),       IMF_SGD_FIELD(momentum), IMF_SGD_FIELD(image_fwd),
      IMF_SGD_FIELD(image_bwd), IMF_SGD_FIELD(numel),      IMF_SGD_FIELD(first_step), IMF_SGD_FIELD(layout),
      IMF_SGD_FIELD(kvol),      IMF_SGD_FIELD(cin),        IMF_SGD_FIELD(cout),     IMF_SGD_FIELD(flip)};
#undef IMF_SGD_FIELD
  if (field < 0) {
    *offset = 0;
    *size = sizeof(imf_sgd_record);
    return IMF_OK;
  }
  IMF_REQUIRE(field < IMF_SGD_RECORD_FIELDS, "imf_sgd_record_layout: field %d of %d", field, IMF_SGD_RECORD_FIELDS);
  *offset = fields[field][0];
  *size = fields[field][1];
  return IMF_OK;
}

extern "C" int imf_sgd_step(const imf_sgd_record *records, int n_records, const int32_t *block_map, int n_blocks, float lr,
                            float momentum, float weight_decay, void *stream) {
  IMF_REQUIRE(n_records >= 0 && n_blocks >= 0, "imf_sgd_step: n_records=%d n_blocks=%d", n_records, n_blocks);
  if (n_blocks == 0) return IMF_OK;
  IMF_REQUIRE(records && block_map && n_records > 0, "imf_sgd_step: null pointer");
  IMF_REQUIRE(((uintptr_t)records & 7) == 0 && ((uintptr_t)block_map & 3) == 0, "imf_sgd_step: tables must be aligned");
  IMF_REQUIRE(momentum >= 0.f && weight_decay >= 0.f && lr == lr, "imf_sgd_step: lr=%g momentum=%g weight_decay=%g",
              (double)lr, (double)momentum, (double)weight_decay);
  k_sgd_step<<<(unsigned)n_blocks, kSgdThreads, 0, (hipStream_t)stream>>>(records, n_records, block_map, lr, momentum,
                                                                          weight_decay);
  IMF_CHECK_LAUNCH("k_sgd_step");
  return IMF_OK;
}
