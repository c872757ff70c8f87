// What the streaming posterior summaries share (moments.hip, tails.hip, acov.hip): the checks and the
// grid of a save, the read-back of the per-chain counts at a read-out, and the reduction of a read-out's per-element values
// to its stats (an extreme and one or two counts).  The numerics of each summary stay in its own file.
#pragma once
#include "common.h"
#include "reduce.h"

#include <cmath>
#include <limits>
#include <string>
#include <vector>

namespace pxm {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// doubles of C chains of `rows` rows of m elements, -1 on overflow
inline int64_t rows_doubles(int64_t m, int C, int64_t rows) {
  if (m < 1 || C < 1 || rows < 1) return -1;
  if (rows > INT64_MAX / m || rows * m > INT64_MAX / 8 / C) return -1;
  return (int64_t)C * rows * m;
}

// ---- a save: pxm_*_update -----------------------------------------------------------------------------------------------------
// What the three entry points check alike, in the name of the one that was called; the stream is reported.  Each checks its
// own buffers and sizes after this.  0, or -1 with the error set.
inline int save_check(const char* fn, int64_t m, int C, int x_stride, hipStream_t st) {
  const std::string f(fn);
  PXM_REQUIRE(C >= 1 && C <= 65535, f + ": need 1 <= C <= 65535");  // grid.y is the chain
  PXM_REQUIRE(m >= 1, f + ": need m >= 1");
  PXM_REQUIRE(x_stride == 1 || x_stride == 2, f + ": x_stride must be 1 (float64) or 2 (real parts of complex128)");
  note_stream(st);
  return 0;
}

// one element per lane: ceil(m / threads) workgroups per chain up to max_blocks (a grid-stride loop covers the rest of a
// row), grid.y the chain
inline dim3 rows_grid(int64_t m, int threads, int max_blocks, int C) {
  const int64_t nb = (m + threads - 1) / threads;
  return dim3((unsigned)(nb < max_blocks ? nb : max_blocks), (unsigned)C);
}

// ---- a read-out: the counts ---------------------------------------------------------------------------------------------------
struct Counts {
  std::vector<int64_t> n;                                    // count[C]
  int n_part = 0;                                            // chains with samples (count > 0), and over those:
  int64_t lo = std::numeric_limits<int64_t>::max(), hi = 0;  // the smallest and the largest count
};

// A read-out is a post-run call and the counts decide what it computes: they are copied back on the stream, which is
// synchronised.
inline int read_counts(const int64_t* count, int C, hipStream_t st, Counts& k) {
  k.n.resize(C);
  PXM_HIP(hipMemcpyAsync(k.n.data(), count, sizeof(int64_t) * C, hipMemcpyDeviceToHost, st));
  PXM_HIP(hipStreamSynchronize(st));
  for (int64_t v : k.n)
    if (v > 0) {
      ++k.n_part;
      k.lo = v < k.lo ? v : k.lo;
      k.hi = v > k.hi ? v : k.hi;
    }
  return 0;
}

// an estimate over chains of one length (`what`, with the entry point's name in front) refuses chains of different lengths;
// `hint` names what the caller can still have
inline int require_common_count(const Counts& k, const char* what, const char* hint) {
  PXM_REQUIRE(k.n_part < 2 || k.lo == k.hi, std::string(what) + " needs one common sample count, the chains hold between " +
                                                std::to_string(k.lo) + " and " + std::to_string(k.hi) + " samples (" + hint + ")");
  return 0;
}

// ---- a read-out: the stats ----------------------------------------------------------------------------------------------------
// stats = (the extreme of the per-element values that are not NaN -- the largest R-hat, the smallest ESS --, or NaN when
// there is none; one or two counts of elements, the NaN among them).  Two stages: every workgroup of the read-out kernel
// leaves its (extreme, counts...) in part[(1 + counts) b] of a caller-owned scratch, and one workgroup of k_summary_stats
// reduces those.  The order of this reduction does not matter, every order gives the same bits:
//   * the extreme is fmax / fmin over values that are never NaN: a NaN element goes to a count before it reaches it, and the
//     start value is -inf / +inf;
//   * it never meets -0.0 and +0.0 together, the one pair fmax / fmin may order either way: R-hat is >= +0, ESS is > 0;
//   * the counts are sums of integers far below 2^53, exact in any order.
// So the counts take the fixed order of reduce.h and the extreme a shuffle tree beside it, and the result is that of any
// other tree.
constexpr int STATS_THREADS = 256;       // lanes of the second stage
constexpr int STATS_MAX_BLOCKS = 1024;   // workgroups of a read-out kernel, i.e. partials; a grid-stride loop covers the rest

// workgroups of a read-out kernel of `threads` lanes, one element per lane, and the doubles of scratch its `comps`
// components per workgroup take (-1: no such m)
inline int stats_blocks(int64_t m, int threads) {
  const int64_t b = (m + threads - 1) / threads;
  return (int)(b < STATS_MAX_BLOCKS ? b : STATS_MAX_BLOCKS);
}
inline int64_t stats_scratch_doubles(int64_t m, int threads, int comps) {
  return m >= 1 ? comps * (int64_t)stats_blocks(m, threads) : -1;
}

template <bool MAX>
__device__ __forceinline__ double extreme(double a, double b) {
  return MAX ? fmax(a, b) : fmin(a, b);
}

// ext and each cnt over the workgroup of NW waves (all of its lanes call), valid in thread 0
template <bool MAX, int NW, class... D>
__device__ __forceinline__ void block_stats(double& ext, D&... cnt) {
  block_sum<NW>(cnt...);
  for (int off = 32; off > 0; off >>= 1) ext = extreme<MAX>(ext, __shfl_down(ext, off));
  if constexpr (NW > 1) {
    __shared__ double s_ext[NW];
    if ((threadIdx.x & 63) == 0) s_ext[threadIdx.x >> 6] = ext;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < NW; ++w) ext = extreme<MAX>(ext, s_ext[w]);
  }
}

// first stage, the tail of a read-out kernel: the lane's (ext, cnt...) -> the workgroup's in part[(1 + counts) blockIdx.x]
template <bool MAX, int NW, class... D>
__device__ __forceinline__ void stats_partial(double* __restrict__ part, double ext, D... cnt) {
  block_stats<MAX, NW>(ext, cnt...);
  if (threadIdx.x == 0) {
    double* p = part + (1 + sizeof...(D)) * blockIdx.x;
    *p++ = ext;
    ((*p++ = cnt), ...);
  }
}

// second stage, one workgroup: the nblocks partials of NC counts each -> stats[1 + NC]
template <bool MAX, int NC>
__global__ __launch_bounds__(STATS_THREADS) void k_summary_stats(const double* __restrict__ part, int nblocks,
                                                                 double* __restrict__ stats) {
  static_assert(NC == 1 || NC == 2, "k_summary_stats: one or two counts");
  const double none = MAX ? -INFINITY : INFINITY;
  double ext = none, c0 = 0.0, c1 = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += STATS_THREADS) {
    const double* p = part + (1 + NC) * b;
    ext = extreme<MAX>(ext, p[0]);
    c0 += p[1];
    if constexpr (NC == 2) c1 += p[2];
  }
  if constexpr (NC == 2) block_stats<MAX, STATS_THREADS / 64>(ext, c0, c1);
  else block_stats<MAX, STATS_THREADS / 64>(ext, c0);
  if (threadIdx.x == 0) {
    stats[0] = ext == none ? __longlong_as_double(0x7ff8000000000000ll) : ext;
    stats[1] = c0;
    if constexpr (NC == 2) stats[2] = c1;
  }
}

}  // namespace pxm
