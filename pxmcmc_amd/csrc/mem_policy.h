// Cache policy of a global memory stream, as a compile-time fact of the kernel that moves it.
//
// MEM_STREAM marks data that nobody reads again before the caches have turned over: the access is emitted non-temporal
// (global_store ... nt), so that its lines do not displace what the next launches re-read from L2 and the Infinity Cache.
// MEM_DEFAULT is the plain access, and a kernel instantiated with MEM_DEFAULT compiles to the code it had before the policy
// existed.  Addresses, widths and the order of the accesses are the same under either policy: no result bit depends on it.
//
// One stream carries a policy: the X' stores of the stock fused phi-DFT step (update.h: px_stock_update4) -- 39 MB per
// iteration at the headline size, next read one whole iteration (~500 MB of other traffic) later.  Every other stream of
// the ring-space step was measured non-temporal too and stays plain (docs/EXPERIMENTS.md, round 15: the ring tables, the
// GEMM results and the ring stores are SLOWER non-temporal; the X and ring reads and the Gram streams are neutral).
// Build-time switch for A/B libraries (scripts/dev/ab_build.sh "-DPXM_NT_DFT_X_OUT=0"); PXM_MEM_POLICY=0 at plan creation
// keeps the plan on the default-policy instantiation (the identity test, tests/test_gpu_mem_policy.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

namespace pxm {

enum MemPolicy { MEM_DEFAULT = 0, MEM_STREAM = 1 };

typedef double mem_d2 __attribute__((ext_vector_type(2)));  // (the builtins take ext vectors, not HIP's double2 struct)

// streaming store (value first, as in an assignment)
__device__ __forceinline__ void mem_store_stream(double2 v, double2* p) {
  __builtin_nontemporal_store(mem_d2{v.x, v.y}, reinterpret_cast<mem_d2*>(p));
}

// PTR[IDX] = VAL under policy POL.  A statement, not a function: under MEM_DEFAULT it is literally the assignment, so the
// kernels that share a body with a policy-carrying one keep their instruction streams (through a function taking the
// address, the address arithmetic of the phi-DFT bodies was scheduled differently).
#define PXM_MEM_STORE(POL, PTR, IDX, VAL)                                                \
  {                                                                                      \
    if constexpr ((POL) == pxm::MEM_STREAM) pxm::mem_store_stream(VAL, (PTR) + (IDX));   \
    else (PTR)[IDX] = VAL;                                                               \
  }

#ifndef PXM_NT_DFT_X_OUT  // the new state X' of the stock fused phi-DFT step
#define PXM_NT_DFT_X_OUT 1
#endif
constexpr int DFT_X_OUT_POLICY = PXM_NT_DFT_X_OUT ? MEM_STREAM : MEM_DEFAULT;

// PXM_MEM_POLICY=0 at plan creation: every launch of the plan on the default-policy instantiations
inline bool mem_policy_from_env() {
  const char* e = getenv("PXM_MEM_POLICY");
  return !e || atoi(e) != 0;
}

}  // namespace pxm
