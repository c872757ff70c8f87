// Live kernel timing of one plan (profiler.cpp): event pairs around its GEMM and grouped-DFT launches.
#pragma once
#include "common.h"

namespace pxm {

// Live kernel timing of one plan (bench.py roofline leg): event pairs handed to hipExtLaunchKernelGGL, which
// stamps them with the kernel's own start / end on the stream it runs on.  Owned by the plan -- no process state.
struct Profiler {
  struct Pool {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    size_t used = 0;
    double bytes = 0, flops = 0;
    std::vector<double> launch_bytes;  // algorithmic bytes of every bracketed launch (launch classes of bench.py)
    std::vector<int> launch_wgs;       // workgroups of every bracketed launch (the key rocprofv3 records join on)
  };
  bool on = false;
  Pool gemm, dft;
  void next(Pool& p, hipEvent_t* start, hipEvent_t* stop, double alg_bytes, double flops, int workgroups = 0) {
    *start = *stop = nullptr;
    if (!on || p.used >= p.ev.size()) return;
    *start = p.ev[p.used].first;
    *stop = p.ev[p.used].second;
    p.bytes += alg_bytes;
    p.flops += flops;
    p.launch_bytes.push_back(alg_bytes);
    p.launch_wgs.push_back(workgroups);
    ++p.used;
  }
};
int profiler_enable(Profiler* pr, int max_launches);  // 0 = off (events are released)
int profiler_read(Profiler::Pool* p, double* ms, int64_t* launches, double* bytes, double* flops,
                  double* per_launch_ms = nullptr, double* per_launch_bytes = nullptr, int64_t cap = 0,
                  int32_t* per_launch_wgs = nullptr);
void profiler_release(Profiler* pr);

}  // namespace pxm
