// Library-level entry points: version, thread-local error string.
#include <stdarg.h>

#include "common.h"

namespace imf {
static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace imf

extern "C" {
int imf_version(void) { return 101; }   /* 0.1.1: imf_conv_args lost two fields */
const char *imf_last_error(void) { return imf::g_err; }

void *imf_event_create(void) {
  hipEvent_t e = nullptr;
  return hipEventCreate(&e) == hipSuccess ? (void *)e : nullptr;
}
void imf_event_destroy(void *ev) {
  if (ev) (void)hipEventDestroy((hipEvent_t)ev);
}
int imf_event_record(void *ev, void *stream) {
  IMF_REQUIRE(ev, "imf_event_record: null event");
  IMF_CHECK_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
  return IMF_OK;
}
/* Streams owned by the library's callers but created here: a framework's stream pool may hand the same stream out
 * twice (torch.cuda.Stream() wraps around after 32), and imf_fragment_forward needs three DISTINCT ones. */
void *imf_stream_create(void) {
  hipStream_t s = nullptr;
  return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? (void *)s : nullptr;
}
void imf_stream_destroy(void *s) {
  if (s) (void)hipStreamDestroy((hipStream_t)s);
}
/* Do two streams run side by side?  HIP multiplexes streams onto a few hardware queues, and two streams that share one run in
 * issue order however independent their work is (LAB_NOTES.md 4i: an ahead stream that shared the image stream's queue made the
 * pair step 15 % slower, one on a queue of its own 13 % faster).  Which queue a new stream gets depends on the process's
 * history, so the answer is measured: one wavefront idles on `a` for ~0.3 ms (bounded: it ends by itself), an empty launch
 * follows on `b`; concurrent <=> b's launch ends in the first half of a's.  1 / 0, or IMF_E* (< 0).  Synchronises both. */
__global__ void k_stream_probe(long long ticks, int *sink) {
  const long long t0 = wall_clock64();   // 100 MHz
  int spins = 0;
  while (wall_clock64() - t0 < ticks && spins < (1 << 12)) {
    __builtin_amdgcn_s_sleep(32);
    ++spins;
  }
  if (sink && spins < 0) *sink = spins;   // (never: keeps the loop)
}

static int probe_streams(hipStream_t sa, hipStream_t sb, hipEvent_t e0, hipEvent_t ea, hipEvent_t eb) {
  int answer = 0;
  for (int pass = 0; pass < 2; ++pass) {   // (the first pass loads the kernel; the second one answers)
    IMF_CHECK_HIP(hipStreamSynchronize(sa)); IMF_CHECK_HIP(hipStreamSynchronize(sb));
    IMF_CHECK_HIP(hipEventRecord(e0, sa));
    k_stream_probe<<<1, 64, 0, sa>>>(pass ? 30000 : 0, nullptr);
    IMF_CHECK_HIP(hipEventRecord(ea, sa));
    k_stream_probe<<<1, 64, 0, sb>>>(0, nullptr);
    IMF_CHECK_HIP(hipEventRecord(eb, sb));
    IMF_CHECK_HIP(hipStreamSynchronize(sa)); IMF_CHECK_HIP(hipStreamSynchronize(sb));
    float ms_a = 0.f, ms_b = 0.f;
    IMF_CHECK_HIP(hipEventElapsedTime(&ms_a, e0, ea)); IMF_CHECK_HIP(hipEventElapsedTime(&ms_b, e0, eb));
    answer = ms_b < 0.5f * ms_a ? 1 : 0;
  }
  return answer;
}

int imf_streams_concurrent(void *a, void *b) {
  IMF_REQUIRE(a && b && a != b, "imf_streams_concurrent: two distinct streams");
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int rc = IMF_OK;
  for (int i = 0; i < 3 && rc == IMF_OK; ++i)
    if (hipEventCreate(&ev[i]) != hipSuccess) { imf::set_error("imf_streams_concurrent: hipEventCreate failed"); rc = IMF_ELAUNCH; }
  if (rc == IMF_OK) rc = probe_streams((hipStream_t)a, (hipStream_t)b, ev[0], ev[1], ev[2]);   // 1 / 0, or IMF_E*
  for (int i = 0; i < 3; ++i)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  return rc;
}

float imf_event_elapsed_ms(void *b, void *e) {
  float ms = -1.f;
  if (!b || !e || hipEventElapsedTime(&ms, (hipEvent_t)b, (hipEvent_t)e) != hipSuccess) return -1.f;
  return ms;
}
}
