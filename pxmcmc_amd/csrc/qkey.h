// The total order on doubles that the quantile kernels select by (tails.hip: k_quantile_range, k_tails_quantiles), and numpy's
// interpolation between two order statistics.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace pxm {

// order-preserving 64-bit key of a double: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, one key per bit pattern
__device__ __forceinline__ uint64_t qkey(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double qval(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}
__device__ __forceinline__ double np_lerp(double a, double b, double t) {  // numpy/lib/_function_base_impl.py: _lerp
#pragma clang fp contract(off)  // separately rounded product and sum, as numpy evaluates them (hipcc contracts a + d * t by default)
  const double d = b - a;
  const double up = a + d * t;
  const double dn = b - d * (1.0 - t);
  return t >= 0.5 ? dn : up;
}

// numpy's linear quantiles of the ns values load(0 .. ns - 1) at Q virtual indices idx[q] + g[q] at once: an exact radix select on
// qkey(), two key bits per sweep of the column and every quantile in the same sweep -- 32 sweeps for the order statistics
// idx[q], one more for their upper neighbours idx[q] + 1 (the same value when it is repeated beyond the wanted rank or
// idx[q] + 1 == ns, else the smallest key above) -- then np_lerp.  No sorting, no scratch memory.
template <int Q, class Load>
__device__ __forceinline__ void select_quantiles(Load load, int64_t ns, const int64_t (&idx)[Q],
                                                 const double (&g)[Q], double (&v)[Q]) {
  uint64_t pre[Q];  // key prefixes found so far
  int64_t rank[Q];  // rank of the wanted statistic among the keys that share the prefix
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    pre[q] = 0;
    rank[q] = idx[q];
  }
  for (int shift = 62; shift >= 0; shift -= 2) {
    int64_t c[Q][4];
#pragma unroll
    for (int q = 0; q < Q; ++q) c[q][0] = c[q][1] = c[q][2] = c[q][3] = 0;
    const uint64_t hi_mask = shift == 62 ? 0ull : (~0ull << (shift + 2));
    for (int64_t s_ = 0; s_ < ns; ++s_) {
      const uint64_t k = qkey(load(s_));
      const int d = (int)((k >> shift) & 3);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const bool m = (k & hi_mask) == pre[q];
        c[q][0] += m && d == 0;
        c[q][1] += m && d == 1;
        c[q][2] += m && d == 2;
        c[q][3] += m && d == 3;
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      int d = 0;
      int64_t r_ = rank[q];
      while (d < 3 && r_ >= c[q][d]) r_ -= c[q][d++];
      rank[q] = r_;
      pre[q] |= (uint64_t)d << shift;
    }
  }
  int64_t le[Q];
  uint64_t up[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    le[q] = 0;
    up[q] = ~0ull;
  }
  for (int64_t s_ = 0; s_ < ns; ++s_) {
    const uint64_t k = qkey(load(s_));
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      le[q] += k <= pre[q];
      if (k > pre[q] && k < up[q]) up[q] = k;
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const double a = qval(pre[q]);
    const double b = (le[q] > idx[q] + 1 || idx[q] + 1 >= ns) ? a : qval(up[q]);
    v[q] = np_lerp(a, b, g[q]);
  }
}

// numpy.quantile, method "linear", on n samples: virtual index q (n - 1), the order statistics i = floor and i + 1 (clipped
// to n - 1 by the caller), g the fraction
inline void quantile_split(double q, int64_t n, int64_t* i, double* g) {
  const double vi = q * (double)(n - 1);
  double fl = std::floor(vi);
  if (fl > (double)(n - 1)) fl = (double)(n - 1);
  *i = (int64_t)fl;
  *g = vi - fl;
}

}  // namespace pxm
