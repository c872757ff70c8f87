// Streaming posterior summaries: per-chain Welford moments and the highest-posterior sample of a
// [C, m] float64 batch, accumulated on the device at the samplers' save points, and their reduction over chains (pooled
// moments, Gelman-Rubin R-hat).  Replaces the np.mean / np.std over a saved chain and the argmax(logposterior) look-up of the
// reference's plot scripts, which need the whole chain in host memory.
#include "summary.h"

#include "../../include/pxmcmc_amd.h"

namespace pxm {

constexpr int MOM_THREADS = 256;
constexpr int MOM_UNROLL = 4;         // independent 16-byte loads in flight per array and lane
constexpr int MOM_MAX_BLOCKS = 2048;  // per chain; the rest of a row is covered by the grid-stride loop

// elements j, j + 1 of the sample: XS = 1 a dense float64 row (j even relative to a 16-byte boundary), XS = 2 the real
// parts of a complex128 row (every element its own aligned 16-byte load)
template <int XS>
__device__ __forceinline__ double2 mom_load2(const double* __restrict__ x, int64_t j) {
  if constexpr (XS == 1) return *reinterpret_cast<const double2*>(x + j);
  const double2* z = reinterpret_cast<const double2*>(x);
  return double2{z[j].x, z[j + 1].x};
}
template <int XS>
__device__ __forceinline__ double mom_load1(const double* __restrict__ x, int64_t j) {
  return x[j * XS];
}

__device__ __forceinline__ void welford(double x, double k, double& mean, double& m2) {
  const double d = x - mean;
  mean += d / k;
  m2 += d * (x - mean);
}

// One Welford step of chain c = blockIdx.y: k = count[c] + 1; d = x - mean; mean += d / k; m2 += d (x - mean_new), and,
// with BEST, best_x = x when logpi[c] > best_logpi[c] (NaN never wins, ties keep the first).  count and best_logpi are only
// READ here: k_moments_advance, queued behind this launch, writes them, so every workgroup of a chain sees the same k.
// Rows start at c * m doubles: with m odd every other row is 8 bytes off a 16-byte boundary, so a row is a scalar head (0 or
// 1 element), 16-byte pairs and a scalar tail.  A masked-out chain returns before it touches memory.
template <int XS, bool BEST>
__global__ __launch_bounds__(MOM_THREADS) void k_moments_update(const double* __restrict__ x, int64_t ldx,
                                                                const int64_t* __restrict__ count, double* __restrict__ mean,
                                                                double* __restrict__ m2, const int* __restrict__ mask,
                                                                const double* __restrict__ logpi, int logpi_stride,
                                                                const double* __restrict__ best_logpi,
                                                                double* __restrict__ best_x, int64_t m) {
  const int c = blockIdx.y;
  if (mask && !mask[c]) return;
  const double k = (double)(count[c] + 1);
  bool take = false;
  if constexpr (BEST) take = logpi[(int64_t)c * logpi_stride] > best_logpi[c];
  const int64_t row = (int64_t)c * m;
  const double* xr = x + (int64_t)c * ldx;
  double* mr = mean + row;
  double* sr = m2 + row;
  double* br = BEST ? best_x + row : nullptr;
  const int64_t head = row & 1;
  const int64_t npairs = (m - head) >> 1;
  const int64_t tid = (int64_t)blockIdx.x * MOM_THREADS + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * MOM_THREADS;

  auto one = [&](int64_t j) {
    const double v = mom_load1<XS>(xr, j);
    double a = mr[j], s = sr[j];
    welford(v, k, a, s);
    mr[j] = a;
    sr[j] = s;
    if constexpr (BEST)
      if (take) br[j] = v;
  };
  if (tid == 0 && head) one(0);
  if (tid == 1 && ((m - head) & 1)) one(m - 1);

  int64_t i = tid;
  for (; i + (MOM_UNROLL - 1) * stride < npairs; i += MOM_UNROLL * stride) {
    double2 v[MOM_UNROLL], a[MOM_UNROLL], s[MOM_UNROLL];
#pragma unroll
    for (int u = 0; u < MOM_UNROLL; ++u) {
      const int64_t j = head + 2 * (i + u * stride);
      v[u] = mom_load2<XS>(xr, j);
      a[u] = *reinterpret_cast<const double2*>(mr + j);
      s[u] = *reinterpret_cast<const double2*>(sr + j);
    }
#pragma unroll
    for (int u = 0; u < MOM_UNROLL; ++u) {
      const int64_t j = head + 2 * (i + u * stride);
      welford(v[u].x, k, a[u].x, s[u].x);
      welford(v[u].y, k, a[u].y, s[u].y);
      *reinterpret_cast<double2*>(mr + j) = a[u];
      *reinterpret_cast<double2*>(sr + j) = s[u];
      if constexpr (BEST)
        if (take) *reinterpret_cast<double2*>(br + j) = v[u];
    }
  }
  for (; i < npairs; i += stride) {
    const int64_t j = head + 2 * i;
    const double2 v = mom_load2<XS>(xr, j);
    double2 a = *reinterpret_cast<const double2*>(mr + j);
    double2 s = *reinterpret_cast<const double2*>(sr + j);
    welford(v.x, k, a.x, s.x);
    welford(v.y, k, a.y, s.y);
    *reinterpret_cast<double2*>(mr + j) = a;
    *reinterpret_cast<double2*>(sr + j) = s;
    if constexpr (BEST)
      if (take) *reinterpret_cast<double2*>(br + j) = v;
  }
}

// The late launch of an update: one workgroup, queued behind k_moments_update on the same stream, advances count (and
// best_logpi) of the masked-in chains.
__global__ __launch_bounds__(MOM_THREADS) void k_moments_advance(int64_t* __restrict__ count, const int* __restrict__ mask,
                                                                 const double* __restrict__ logpi, int logpi_stride,
                                                                 double* __restrict__ best_logpi, int C) {
  for (int c = threadIdx.x; c < C; c += MOM_THREADS) {
    if (mask && !mask[c]) continue;
    if (logpi) {
      const double lp = logpi[(int64_t)c * logpi_stride];
      if (lp > best_logpi[c]) best_logpi[c] = lp;
    }
    count[c] += 1;
  }
}

// Reduction over chains, one lane per element, chains in index order (deterministic).  Pooled moments by Chan's pairwise
// merge over the chains with count > 0; R-hat over those chains when they share one count n_common >= 2 (n_common = 0:
// undefined, NaN).  Every product and sum is rounded on its own (no contraction): uncertainty.rhat_np states the same
// sequence of operations.  n_common and n_part come from the host, which has read the counts: n_common = the common count
// when n_part >= 2 chains take part and it is >= 2, else 0.  Each workgroup leaves (max R-hat over its non-NaN elements, its
// NaN count) in part[2 b] (summary.h).
__global__ __launch_bounds__(MOM_THREADS) void k_moments_finalize(const int64_t* __restrict__ count,
                                                                  const double* __restrict__ mean,
                                                                  const double* __restrict__ m2, int C, int64_t m,
                                                                  int64_t n_common, int n_part, double* __restrict__ pooled_mean,
                                                                  double* __restrict__ pooled_var, double* __restrict__ rhat,
                                                                  double* __restrict__ part) {
#pragma clang fp contract(off)
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double rmax = -INFINITY;
  double nnan = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * MOM_THREADS + threadIdx.x; e < m; e += (int64_t)gridDim.x * MOM_THREADS) {
    double na = 0.0, ma = 0.0, sa = 0.0;
    for (int c = 0; c < C; ++c) {
      const double nb = (double)count[c];
      if (nb == 0.0) continue;
      const double mb = mean[(int64_t)c * m + e], sb = m2[(int64_t)c * m + e];
      const double n = na + nb;
      const double d = mb - ma;
      ma = ma + d * (nb / n);
      sa = (sa + sb) + (d * d) * (na * nb / n);
      na = n;
    }
    if (pooled_mean) pooled_mean[e] = na > 0.0 ? ma : nan;
    if (pooled_var) pooled_var[e] = na > 1.0 ? sa / (na - 1.0) : nan;
    if (rhat) {
      double r = nan;
      if (n_common >= 2) {
        const double n = (double)n_common, cp = (double)n_part;
        double sm = 0.0, sw = 0.0;
        for (int c = 0; c < C; ++c)
          if (count[c] > 0) {
            sm += mean[(int64_t)c * m + e];
            sw += m2[(int64_t)c * m + e] / (n - 1.0);
          }
        const double mbar = sm / cp, W = sw / cp;
        double sb = 0.0;
        for (int c = 0; c < C; ++c)
          if (count[c] > 0) {
            const double d = mean[(int64_t)c * m + e] - mbar;
            sb += d * d;
          }
        const double B = n / (cp - 1.0) * sb;
        if (W != 0.0) r = sqrt(((n - 1.0) / n * W + B / n) / W);
      }
      rhat[e] = r;
      if (r != r) nnan += 1.0;
      else rmax = fmax(rmax, r);
    }
  }
  if (part) stats_partial<true, MOM_THREADS / 64>(part, rmax, nnan);
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int64_t pxm_moments_scratch_doubles(int64_t m) { return stats_scratch_doubles(m, MOM_THREADS, 2); }

int pxm_moments_update(const double* x, int x_stride, int64_t* count, double* mean, double* m2, const int* mask,
                       const double* logpi, int logpi_stride, double* best_logpi, double* best_x, int64_t m, int C,
                       pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (save_check("pxm_moments_update", m, C, x_stride, st)) return -1;
  PXM_REQUIRE(x && count && mean && m2, "pxm_moments_update: null buffer");
  const bool best = logpi || best_logpi || best_x;
  PXM_REQUIRE(!best || (logpi && best_logpi && best_x), "pxm_moments_update: logpi, best_logpi and best_x are given together");
  PXM_REQUIRE(!best || logpi_stride == 1 || logpi_stride == 2, "pxm_moments_update: logpi_stride must be 1 or 2");
  PXM_REQUIRE(aligned16(x) && aligned16(mean) && aligned16(m2) && aligned16(best_x),
              "pxm_moments_update: x, mean, m2 and best_x must be 16-byte aligned");
  const int64_t per = (int64_t)MOM_THREADS * MOM_UNROLL;
  // whole unrolled passes only (floor): every lane runs the 4-deep body for the bulk of a row and the first lanes take what
  // is left (fewer than 4 strides) one pair at a time; rows shorter than one pass run on a single workgroup
  int64_t nb = (m / 2) / per;
  nb = nb < 1 ? 1 : (nb > MOM_MAX_BLOCKS ? MOM_MAX_BLOCKS : nb);
  const dim3 grid((unsigned)nb, (unsigned)C);
  const int64_t ldx = m * x_stride;
#define MOM_LAUNCH(XS, BEST)                                                                                                  \
  hipLaunchKernelGGL((k_moments_update<XS, BEST>), grid, dim3(MOM_THREADS), 0, st, x, ldx, count, mean, m2, mask, logpi,       \
                     logpi_stride, best_logpi, best_x, m)
  if (x_stride == 1) {
    if (best) MOM_LAUNCH(1, true);
    else MOM_LAUNCH(1, false);
  } else {
    if (best) MOM_LAUNCH(2, true);
    else MOM_LAUNCH(2, false);
  }
#undef MOM_LAUNCH
  PXM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_moments_advance, dim3(1), dim3(MOM_THREADS), 0, st, count, mask, logpi, logpi_stride, best_logpi, C);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_moments_finalize(const int64_t* count, const double* mean, const double* m2, int64_t m, int C, double* pooled_mean,
                         double* pooled_var, double* rhat, double* stats, double* scratch, pxm_stream_t stream) {
  PXM_REQUIRE(C >= 1, "pxm_moments_finalize: need C >= 1");
  PXM_REQUIRE(m >= 1, "pxm_moments_finalize: need m >= 1");
  PXM_REQUIRE(count && mean && m2, "pxm_moments_finalize: null buffer");
  PXM_REQUIRE(pooled_mean || pooled_var || rhat, "pxm_moments_finalize: no output requested");
  PXM_REQUIRE(!stats || (rhat && scratch), "pxm_moments_finalize: stats needs rhat and scratch");
  hipStream_t st = (hipStream_t)stream;
  note_stream(st);
  Counts k;  // they decide whether R-hat is defined
  if (rhat && (read_counts(count, C, st, k) ||
               require_common_count(k, "pxm_moments_finalize: R-hat", "the pooled moments do not: call without rhat")))
    return -1;
  const int64_t n_common = k.n_part >= 2 && k.lo >= 2 ? k.lo : 0;
  const int nb = stats_blocks(m, MOM_THREADS);
  hipLaunchKernelGGL(k_moments_finalize, dim3(nb), dim3(MOM_THREADS), 0, st, count, mean, m2, C, m, n_common, k.n_part, pooled_mean,
                     pooled_var, rhat, stats ? scratch : nullptr);
  PXM_HIP(hipGetLastError());
  if (stats) {
    hipLaunchKernelGGL((k_summary_stats<true, 1>), dim3(1), dim3(STATS_THREADS), 0, st, scratch, nb, stats);
    PXM_HIP(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
