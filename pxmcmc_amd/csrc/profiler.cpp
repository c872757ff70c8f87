// Live profiler: event pairs around GEMM / grouped-DFT launches, owned by a plan.
#include "profiler.h"

namespace pxm {

int profiler_enable(Profiler* pr, int max_launches) {
  profiler_release(pr);
  if (max_launches <= 0) return 0;
  for (Profiler::Pool* p : {&pr->gemm, &pr->dft}) {
    p->ev.resize((size_t)max_launches);
    for (auto& e : p->ev) {
      e.first = e.second = nullptr;
      PXM_HIP(hipEventCreate(&e.first));
      PXM_HIP(hipEventCreate(&e.second));
    }
  }
  pr->on = true;
  return 0;
}
void profiler_release(Profiler* pr) {
  pr->on = false;
  for (Profiler::Pool* p : {&pr->gemm, &pr->dft}) {
    for (auto& e : p->ev) {
      deferred_event_destroy(e.first);
      deferred_event_destroy(e.second);
    }
    p->ev.clear();
    p->used = 0;
    p->bytes = p->flops = 0;
    p->launch_bytes.clear();
    p->launch_wgs.clear();
  }
}
int profiler_read(Profiler::Pool* p, double* ms, int64_t* launches, double* bytes, double* flops, double* per_launch_ms,
                  double* per_launch_bytes, int64_t cap, int32_t* per_launch_wgs) {
  double tot = 0;
  for (size_t i = 0; i < p->used; ++i) {
    PXM_HIP(hipEventSynchronize(p->ev[i].second));
    float t = 0;
    PXM_HIP(hipEventElapsedTime(&t, p->ev[i].first, p->ev[i].second));
    tot += t;
    if ((int64_t)i < cap) {
      if (per_launch_ms) per_launch_ms[i] = t;
      if (per_launch_bytes) per_launch_bytes[i] = p->launch_bytes[i];
      if (per_launch_wgs) per_launch_wgs[i] = p->launch_wgs[i];
    }
  }
  if (ms) *ms = tot;
  if (launches) *launches = (int64_t)p->used;
  if (bytes) *bytes = p->bytes;
  if (flops) *flops = p->flops;
  p->used = 0;
  p->bytes = p->flops = 0;
  p->launch_bytes.clear();
  p->launch_wgs.clear();
  return 0;
}

}  // namespace pxm
