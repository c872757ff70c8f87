// What the SHT plan and the wavelet plan share: status word, sizes, side streams, argument check, image descriptors.
#pragma once
#include "../../include/pxmcmc_amd.h"
#include "sht_rec.h"
#include "tasklist.h"

#include <cstdlib>

namespace pxm {

// Device status word of a plan: kernels OR a bit in when a bounded wait expires (dft_wave.h: d5_pair_sync) instead of
// hanging the GPU; the host reads it wherever it synchronises anyway.
inline int status_alloc(unsigned** d) {
  if (int rc = dev_alloc(d, 4 * sizeof(unsigned), "plan status word")) return rc;
  return dev_zero(*d, 4 * sizeof(unsigned));
}
inline int status_read(unsigned* d, hipStream_t st, int clear) {
  if (!d) return 0;
  unsigned h = 0;
  PXM_HIP(hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, st));
  PXM_HIP(hipStreamSynchronize(st));
  if (clear && h) PXM_HIP(hipMemsetAsync(d, 0, sizeof(unsigned), st));
  return (int)(h & 0x7fffffffu);
}

inline int64_t arr_size(int L, int ncol) { return (int64_t)(2 * L - 1) * round_up(L, 16) * ncol; }

// Does a plan of this size take the table-free ring stage (sht_rec.hip) for its B-table contractions?  PXM_REC=1: wherever the
// column count allows (tests run both paths at small L); PXM_REC=0: never; unset: few-column launches at large L, where the
// table stream feeds a fraction of an MFMA tile.
inline bool rec_wanted(int L, int spin, int max_chains) {
  if (!rec_supported(L, spin, max_chains)) return false;
  if (const char* e = std::getenv("PXM_REC")) return std::atoi(e) != 0 && L >= 3;
  return L >= 128;  // (below, the launches are latency-bound either way and the tables are small)
}

// Side streams and their fork / join events are per-device and live for the whole process: every plan borrows
// them.  (Destroying streams that took part in a HIP-graph capture while the capturing stream lives on
// corrupts the runtime's capture bookkeeping: a loop that builds a sampler, captures its iteration and drops
// the plan crashed in the 32nd hipGraphLaunch.)  Sharing only adds false ordering between plans, never a race:
// a fork makes the side stream wait for the caller's stream, a join the reverse.
struct SidePool {
  static constexpr int N = 3;
  hipStream_t side[N] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[N] = {nullptr, nullptr, nullptr};
};
inline int side_pool(SidePool** out) {
  static SidePool pools[16];
  int dev = 0;
  if (dry_run()) {  // no streams without a GPU: the plan runs nothing in dry-run mode
    static SidePool none;
    *out = &none;
    return 0;
  }
  PXM_HIP(hipGetDevice(&dev));
  SidePool& sp = pools[dev & 15];
  if (!sp.ev_fork) {
    for (int i = 0; i < SidePool::N; ++i) {
      PXM_HIP(hipStreamCreateWithFlags(&sp.side[i], hipStreamNonBlocking));
      PXM_HIP(hipEventCreateWithFlags(&sp.ev_join[i], hipEventDisableTiming));
    }
    PXM_HIP(hipEventCreateWithFlags(&sp.ev_fork, hipEventDisableTiming));
  }
  *out = &sp;
  return 0;
}

// the argument check every transform entry point starts with; `who` names the entry point in the error
template <class Plan>
inline int plan_check(const Plan* p, const void* a, const void* b, int C, const char* who) {
  PXM_REQUIRE(p && a && b, std::string(who) + ": null argument");
  PXM_REQUIRE(C >= 1 && C <= p->Cmax, std::string(who) + ": C outside [1, max_chains]");
  return 0;
}

// an image at bandlimit L as DFT-stage input (with data / invcov: the residual invcov .* (f - data)) / output
inline PxIn image_in(int L, const void* f, const void* data = nullptr, const void* invcov = nullptr, int invcov_complex = 0) {
  PxIn in;
  in.f = (const double*)f;
  in.chain_stride = (int64_t)L * (2 * L - 1);
  in.data = (const double*)data;
  in.invcov = (const double*)invcov;
  in.invcov_complex = invcov_complex;
  return in;
}
inline PxOut image_out(int L, void* f) {
  PxOut out;
  out.f = (double*)f;
  out.chain_stride = (int64_t)L * (2 * L - 1);
  return out;
}

}  // namespace pxm
