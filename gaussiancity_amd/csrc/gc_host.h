// gc_host.h -- host scaffold shared by the libraries' C ABI files (gcr_api.hip, gcv_points.hip, gce_grid.hip,
// gcs_sparse.hip, gca_attention.hip, gcm_modlinear.hip): the error string behind *_last_error, fail / fail_hip / HIP_TRY, and the stage
// timer behind option "timing" / *_get_stage_ms.  Host code only.  Everything has internal linkage, so include it
// from ONE translation unit per library (in libgcr_hip.so that is gcr_api.hip): a second one would get a second error
// string.  Define GC_ERR_HIP, the library's status code for a HIP runtime error, before including it.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#ifndef GC_ERR_HIP
#error "define GC_ERR_HIP (the library's status code for a HIP runtime error) before including gc_host.h"
#endif

namespace {

thread_local std::string g_err;  // what *_last_error() returns on this thread

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int fail_hip(hipError_t e, const char* where) { return fail((int)GC_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e)); }
#define HIP_TRY(expr, where)                          \
  do {                                                \
    hipError_t e_ = (expr);                           \
    if (e_ != hipSuccess) return fail_hip(e_, where); \
  } while (0)

// Stage timer: pairs of hipEvents per stage recorded on the caller's stream, a ring of STAGE_RING pairs per stage.
// Non-blocking in practice: a pair is resolved when its ring slot comes round again, STAGE_RING frames later, and no
// caller keeps that many frames in flight (one pair per stage made the host wait for the PREVIOUS frame's stage
// before it could enqueue this frame's -- with three frames in flight that wait thinned out the overlap and the
// timed kernels looked a third shorter than a rocprofv3 trace of the uninstrumented loop shows them).
// A library declares one StageSlot per stage -- and with that chooses whose times they are: thread_local slots report
// this thread's stages, process-wide slots every thread's (a stage must then be enqueued by one thread at a time) -- and
// hands StageTimer the stage's slot, or null while its option "timing" is 0.
constexpr int STAGE_RING = 8;
struct StageSlot {
  hipEvent_t a[STAGE_RING] = {}, b[STAGE_RING] = {};
  bool pending[STAGE_RING] = {};
  int next = 0;
  double sum_ms = 0.0;
  long count = 0;
};

void stage_resolve(StageSlot& sl, int i) {
  if (!sl.pending[i]) return;
  float ms = 0;
  if (hipEventSynchronize(sl.b[i]) == hipSuccess && hipEventElapsedTime(&ms, sl.a[i], sl.b[i]) == hipSuccess) {
    sl.sum_ms += ms;
    sl.count += 1;
  }
  sl.pending[i] = false;
}

struct StageTimer {
  hipStream_t s;
  StageSlot* sl;
  int i = 0;
  StageTimer(hipStream_t s_, StageSlot* slot) : s(s_), sl(slot) {
    if (!sl) return;
    i = sl->next;
    sl->next = (i + 1) % STAGE_RING;
    if (!sl->a[i]) {
      (void)hipEventCreate(&sl->a[i]);
      (void)hipEventCreate(&sl->b[i]);
    }
    stage_resolve(*sl, i);
    (void)hipEventRecord(sl->a[i], s);
  }
  ~StageTimer() {
    if (!sl) return;
    (void)hipEventRecord(sl->b[i], s);
    sl->pending[i] = true;
  }
};

// The body of *_get_stage_ms: resolves what is pending and reports the average per stage since the last call.
int stage_report(StageSlot* slots, int count, float* ms_out, int capacity) {
  if (!ms_out) return 0;
  int n = 0;
  for (; n < capacity && n < count; n++) {
    StageSlot& sl = slots[n];
    for (int k = 0; k < STAGE_RING; k++) stage_resolve(sl, k);
    ms_out[n] = sl.count ? (float)(sl.sum_ms / (double)sl.count) : 0.0f;
    sl.sum_ms = 0.0;
    sl.count = 0;
  }
  return n;
}

}  // namespace
