// The one summation order of the per-chain sums, and the rules that fix how many slices a chain is summed in.
//
// The sums are deterministic and do not depend on the batch a chain runs in; tests compare them bit for bit between launches
// (a chain alone against the chain in a batch, deferred totals against immediate ones).  All of that rests on one order:
//   1. each thread adds its grid-stride terms one after the other (the kernels' own loops);
//   2. the lanes of a wave are combined by a __shfl_down halving tree, offsets 32 ... 1              (wave_sum);
//   3. the waves of a workgroup are added one after the other by thread 0, from 0.0                  (block_sum);
//   4. a finishing kernel gives lane l the slices l, l + 64, ... and runs the same tree             (slice_add, slice_sum).
// Every kernel that leaves such a sum calls these; none writes the order out again.  (The __shfl_xor butterflies of
// spmv.hip and sht_gemm.hip are a different order with a different purpose.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace pxm {

// The helpers take the components of a sum as a pack of double lvalues, not as an array: an array of accumulators becomes a
// vector value in the compiler, and a component that is constant zero or unused is then summed all the same.

// each v += the v of the lanes above: valid in lane 0
template <class... D>
__device__ __forceinline__ void wave_sum(D&... v) {
  static_assert((std::is_same_v<D, double> && ...), "wave_sum: doubles");
  for (int off = 32; off > 0; off >>= 1) ((v += __shfl_down(v, off)), ...);
}

// each v = its sum over the workgroup, valid in thread 0 (unspecified elsewhere).  The workgroup has `nwaves` <= NW waves; NW
// sizes the LDS array.  REUSE: a barrier before the LDS write, for a kernel that calls the same instantiation more than once
// (the calls share one LDS array; two different instantiations would each get their own).
template <int NW, bool REUSE, class... D>
__device__ __forceinline__ void block_sum_of(int nwaves, D&... v) {
  constexpr int K = sizeof...(D);
  __shared__ __attribute__((aligned(K % 2 ? 8 : 16))) double part[NW][K];
  wave_sum(v...);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (REUSE) __syncthreads();
  if (lane == 0) {
    int k = 0;
    ((part[wave][k++] = v), ...);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ((v = 0.0), ...);
    for (int w = 0; w < nwaves; ++w) {
      int k = 0;
      ((v += part[w][k++]), ...);
    }
  }
}

// for a kernel whose launch bound is its launch, NW waves, and that sums once: the loop over the waves unrolls
template <int NW, class... D>
__device__ __forceinline__ void block_sum(D&... v) {
  block_sum_of<NW, false>(NW, v...);
}

// for the kernels whose wave count is the launch's (up to 16 waves) and that may sum more than once: two components, 256
// bytes of LDS however often it is called
__device__ __forceinline__ void block_sum2(double& a, double& b) { block_sum_of<16, true>(blockDim.x >> 6, a, b); }

// The lane's part of step 4: each v += its column of row [slices][STRIDE] (the first v is column 0, the next column 1, ...)
// over the slices lane, lane + 64, ...  On its own only where the waves of a kernel gather rows of different shapes and then
// share one tree (k_pxmala_accept3); everything else calls slice_sum.
template <int STRIDE, class... D>
__device__ __forceinline__ void slice_add(const double* __restrict__ row, int slices, int lane, D&... v) {
  static_assert(sizeof...(D) <= STRIDE, "slice_add: more components than the row holds");
  for (int sl = lane; sl < slices; sl += 64) {
    const double* p = row + (int64_t)sl * STRIDE;
    ((v += *p++), ...);
  }
}

// each v = the sum of its column over all slices, for the wave that calls it with all 64 lanes, `lane` the lane's number -- a
// single-wave workgroup or one wave among many: lane l adds slices l, l + 64, ..., then the tree.  Valid in lane 0.
template <int STRIDE, class... D>
__device__ __forceinline__ void slice_sum(const double* __restrict__ row, int slices, int lane, D&... v) {
  ((v = 0.0), ...);
  slice_add<STRIDE>(row, slices, lane, v...);
  wave_sum(v...);
}

// ---- slices (workgroups) per chain -----------------------------------------------------------------------------------------
// Both rules are functions of the vector length n only, never of the number of chains C: the terms a slice adds, and the
// order the slices are added in, are then the same whatever batch the chain runs in.

// the two-stage reductions and the PxMALA kernels (reduce.hip, pxmala.hip): >= 2048 elements per slice, 64 ... 1024 slices
constexpr int RED_SLICES_MIN = 64, RED_SLICES_MAX = 1024;
inline int red_slices(int64_t n) {
  return (int)std::min<int64_t>(RED_SLICES_MAX, std::max<int64_t>(RED_SLICES_MIN, (n + 2047) / 2048));
}

// Those reductions run through a CALLER-OWNED scratch of this many doubles (partial sums of every slice, then the per-chain
// totals): no library-owned buffer is shared between calls, streams or plans.  (pxm_pxmala_propose: 4x this)
inline size_t red_scratch_doubles(int C) { return (size_t)(C + 1) * RED_SLICES_MAX * 2; }

// the stepping kernels that leave per-chain sums (fista.hip, sapg.hip): one slice per 256 elements up to `most`, grid-stride
// beyond
inline int chain_slices(int64_t n, int most) {
  const int64_t s = (n + 255) / 256;
  return (int)(s < 1 ? 1 : (s > most ? most : s));
}

}  // namespace pxm
