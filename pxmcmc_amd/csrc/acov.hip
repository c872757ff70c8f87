// Streaming effective sample size: per chain and element the lagged products of the saved samples at
// lags 0 ... K - 1, accumulated on the device at the samplers' save points, and the read-out that turns them into the
// autocovariances about the chain's own mean, Geyer's initial monotone sequence, the effective sample size per chain and
// pooled over the chain batch, and the Monte-Carlo standard error of the pooled mean -- without the chain.
//
// With x_0 ... x_{n-1} the saves of one chain, p = x_0 the pivot and y_t = x_t - p (which makes every sum below independent
// of an offset of the samples), the state is
//   acc  [C][K][m]  acc_l = sum_{t >= l} y_t y_{t-l}, in save order, one product and one addition at a time
//   tot  [C][m]     sum_t y_t, in save order
//   head [C][K][m]  the first K saves, raw (row 0 is the pivot)
//   ring [C][R][m]  save t at row t mod R, raw, R = K - 1 + ACOV_STAGE
// acc and tot hold the saves of the complete blocks of ACOV_STAGE saves only: a save is a row copy into the ring (and into
// head during the first K saves), and the save that completes a block folds the block into acc and tot, reading the K - 1
// saves before the block from the ring.  Folding every save on its own would read and write the K rows of acc per save;
// a block does so once per ACOV_STAGE saves.  The first block starts its sums from zero instead of reading them, so the
// state needs no initialisation.  The read-out folds the saves of the incomplete last block on the fly, in the order a merge
// would use, and writes nothing to the state.
#include "summary.h"

#include "../../include/pxmcmc_amd.h"

namespace pxm {

constexpr int ACOV_THREADS = 256;
constexpr int ACOV_STAGE = 16;         // B: saves of a block
constexpr int ACOV_MAX_LAGS = 64;      // largest K
constexpr int ACOV_MAX_BLOCKS = 4096;  // per chain; the rest of a row is covered by the grid-stride loop
constexpr int ESS_THREADS = 64;        // lanes of a read-out workgroup

__device__ __forceinline__ double acov_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// row r0 + i of a ring of R rows, for -R < i < R and 0 <= r0 < R
__device__ __forceinline__ int ring_row(int r0, int i, int R) {
  const int r = r0 + i;
  return r < 0 ? r + R : (r >= R ? r - R : r);
}

// One save of chain c = blockIdx.y, n = count[c] saves before it (count is only read: the pxm_moments_update queued behind
// this launch advances it).  A masked-out chain returns before it touches memory.  The sample goes to row n mod R of the
// ring and, for n < K, to row n of head.  When it completes a block (n mod B == B - 1, block start n0 = n - (B - 1)) each
// lane loads the window of its element -- the K - 1 saves before the block and the block, oldest first, less the pivot --
// into registers and updates tot and every acc_l, which it reads and writes once.  KMAX >= K is the compiled window length:
// every loop over lags and window slots is unrolled over KMAX with the test against K inside, so that the rotation of the
// ring ends up in the row a load addresses (uniform over the workgroup) and never in a register index.
template <int KMAX>
__global__ __launch_bounds__(ACOV_THREADS) void k_acov_update(const double* __restrict__ x, int64_t ldx, int xs,
                                                              const int64_t* __restrict__ count, double* __restrict__ acc,
                                                              double* __restrict__ tot, double* __restrict__ head,
                                                              double* __restrict__ ring, const int* __restrict__ mask, int64_t m,
                                                              int K) {
#pragma clang fp contract(off)
  const int c = blockIdx.y;
  if (mask && !mask[c]) return;
  const int64_t n = count[c];
  if (n < 0) return;
  constexpr int B = ACOV_STAGE;
  const int R = K - 1 + B;
  const double* xr = x + (int64_t)c * ldx;
  double* ar = acc + (int64_t)c * K * m;
  double* tr = tot + (int64_t)c * m;
  double* hr = head + (int64_t)c * K * m;
  double* rr = ring + (int64_t)c * R * m;
  const int row = (int)(n % R);
  const int64_t tid = (int64_t)blockIdx.x * ACOV_THREADS + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * ACOV_THREADS;

  if (n % B != B - 1) {
    for (int64_t j = tid; j < m; j += stride) {
      const double v = xr[j * xs];
      rr[row * m + j] = v;
      if (n < K) hr[n * m + j] = v;
    }
    return;
  }

  const int64_t n0 = n - (B - 1);
  const int r0 = (int)(n0 % R);
  const bool first = n0 == 0;
  for (int64_t j = tid; j < m; j += stride) {
    const double v = xr[j * xs];
    rr[row * m + j] = v;
    if (n < K) hr[n * m + j] = v;
    const double p = hr[j];
    // w[KMAX - 1 + s]: save n0 + s of the block; w[KMAX - 1 - d]: the save d before the block (unused where there is none)
    double w[KMAX - 1 + B];
#pragma unroll
    for (int d = 1; d < KMAX; ++d) w[KMAX - 1 - d] = (d < K && d <= n0) ? rr[ring_row(r0, -d, R) * m + j] - p : 0.0;
#pragma unroll
    for (int s = 0; s < B - 1; ++s) w[KMAX - 1 + s] = rr[ring_row(r0, s, R) * m + j] - p;
    w[KMAX - 1 + B - 1] = v - p;
    double t = first ? 0.0 : tr[j];
#pragma unroll
    for (int s = 0; s < B; ++s) t = t + w[KMAX - 1 + s];
    tr[j] = t;
#pragma unroll
    for (int l = 0; l < KMAX; ++l) {
      if (l < K) {
        double a = first ? 0.0 : ar[l * m + j];
#pragma unroll
        for (int s = 0; s < B; ++s)
          if (n0 + s >= l) a = a + w[KMAX - 1 + s] * w[KMAX - 1 + s - l];
        ar[l * m + j] = a;
      }
    }
  }
}

// Geyer's initial monotone sequence over P_k = rho_2k + rho_2k+1, fed one lag at a time: stops at the first P_k that is not
// positive (a NaN included), otherwise P_k <- min(P_k, P_k-1) joins the sum.  lag: the even lag 2 k of the stop.
struct Geyer {
  double sum = 0.0, prev = INFINITY, even = 0.0;
  int lag = -1;
  __device__ __forceinline__ void step(int l, double rho) {
    if (lag >= 0) return;
    if (!(l & 1)) {
      even = rho;
      return;
    }
    const double P = even + rho;
    if (!(P > 0.0)) {
      lag = l - 1;
      return;
    }
    prev = fmin(P, prev);
    sum = sum + prev;
  }
  // tau = -1 + 2 sum; ESS = min(N / tau, N log10 N), the cap where tau <= 0.  lmax = min(K, n) lags were fed
  __device__ __forceinline__ double ess(double N, int lmax, int* lag_out) {
    *lag_out = lag >= 0 ? lag : 2 * (lmax / 2);
    const double tau = -1.0 + 2.0 * sum, cap = N * log10(N);
    return tau > 0.0 ? fmin(N / tau, cap) : cap;
  }
};

// tot of chain c at element e with the saves of the incomplete block folded in, and the pivot
__device__ __forceinline__ double acov_total(const double* __restrict__ tr, const double* __restrict__ hr,
                                             const double* __restrict__ rr, int64_t m, int64_t e, int64_t n0, int np, int r0, int R,
                                             double* pivot) {
#pragma clang fp contract(off)
  const double p = hr[e];
  double t = n0 ? tr[e] : 0.0;
#pragma unroll
  for (int s = 0; s < ACOV_STAGE - 1; ++s)
    if (s < np) t = t + (rr[ring_row(r0, s, R) * m + e] - p);
  *pivot = p;
  return t;
}

// The read-out, one lane per element, chains in index order.  Per chain: d = tot / n, gamma_l = (acc_l - d ((tot - head_l) +
// (tot - tail_l)) + (n - l) d^2) / n with head_l (tail_l) the sum of the first (last) l of the y_t, rho_l = gamma_l /
// gamma_0, Geyer's sum, ess [C][m] and ess_lag [C][m] (NaN and -1 for n < 4 or a gamma_0 that is not positive and finite).
// Pooled (ess_pooled non-null; the host has read the counts and checked that the n_part >= 1 chains with samples share the
// count n_common, 0 when no chain has any):
// G_l = sum_c n / (n - 1) gamma_l,c in the registers of the lane, W = G_0 / C', var+ = (n - 1) / n W + sum_c (mean_c -
// mean of means)^2 / (C' - 1) with mean_c = p_c + d_c, rho_l = 1 - (W - G_l / C') / var+, the same Geyer sum,
// ESS = min(C' n / tau, C' n log10(C' n)) and mcse = sqrt(var+ / ESS).  Every product and sum is rounded on its own:
// uncertainty.ess_np / ess_pooled_np state the same sequence of operations.  Each workgroup leaves (min ESS over its non-NaN
// values, NaN count, truncated count) of the per-chain values in part[3 b] (summary.h).  The lag loops run to K at run time
// and the G_l are indexed by the lag, so they live in LDS, one column per lane (a register array indexed so would go to
// scratch memory); the workgroup is one wave to keep that at 32 KiB.
__global__ __launch_bounds__(ESS_THREADS) void k_acov_ess(const int64_t* __restrict__ count, const double* __restrict__ acc,
                                                           const double* __restrict__ tot, const double* __restrict__ head,
                                                           const double* __restrict__ ring, int64_t m, int C, int K,
                                                           int64_t n_common, int n_part, double* __restrict__ ess,
                                                           int* __restrict__ ess_lag, double* __restrict__ ess_pooled,
                                                           double* __restrict__ mcse, double* __restrict__ part) {
#pragma clang fp contract(off)
  constexpr int B = ACOV_STAGE;
  const int R = K - 1 + B;
  const bool pooled = ess_pooled && n_common >= 4;
  __shared__ double G[ACOV_MAX_LAGS][ESS_THREADS];
  double emin = INFINITY, nnan = 0.0, ntrunc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * ESS_THREADS + threadIdx.x; e < m; e += (int64_t)gridDim.x * ESS_THREADS) {
    for (int l = 0; l < K; ++l) G[l][threadIdx.x] = 0.0;
    double sm = 0.0;
    for (int c = 0; c < C; ++c) {
      const int64_t n = count[c];
      if (n < 4) {
        ess[(int64_t)c * m + e] = acov_nan();
        ess_lag[(int64_t)c * m + e] = -1;
        nnan += 1.0;
        continue;
      }
      const double* ar = acc + (int64_t)c * K * m;
      const double* hr = head + (int64_t)c * K * m;
      const double* rr = ring + (int64_t)c * R * m;
      const int np = (int)(n % B);
      const int64_t n0 = n - np;
      const int r0 = (int)(n0 % R);
      double p;
      const double t = acov_total(tot + (int64_t)c * m, hr, rr, m, e, n0, np, r0, R, &p);
      double pend[B - 1];
#pragma unroll
      for (int s = 0; s < B - 1; ++s) pend[s] = s < np ? rr[ring_row(r0, s, R) * m + e] - p : 0.0;
      const double nd = (double)n, d = t / nd, dd = d * d, f = nd / (nd - 1.0);
      const int lmax = K < n ? K : (int)n;
      const int rl = ring_row(r0, np - 1, R);  // row of the last save
      double hc = 0.0, tc = 0.0, g0 = 0.0;
      bool ok = true;
      Geyer gy;
      for (int l = 0; l < lmax && ok; ++l) {
        {
          double a = n0 ? ar[l * m + e] : 0.0;
#pragma unroll
          for (int s = 0; s < B - 1; ++s)
            if (s < np && n0 + s >= l) a = a + pend[s] * (rr[ring_row(r0, s - l, R) * m + e] - p);
          const double g = ((a - d * ((t - hc) + (t - tc))) + (double)(n - l) * dd) / nd;
          if (l == 0) {
            g0 = g;
            ok = g0 > 0.0 && g0 < INFINITY;
          }
          if (ok) {
            gy.step(l, g / g0);
            if (pooled) G[l][threadIdx.x] = G[l][threadIdx.x] + f * g;
            hc = hc + (hr[l * m + e] - p);
            tc = tc + (rr[ring_row(rl, -l, R) * m + e] - p);
          }
        }
      }
      sm = sm + (p + d);
      double v = acov_nan();
      int lag = -1;
      if (ok) {
        v = gy.ess(nd, lmax, &lag);
        emin = fmin(emin, v);
        if (lag == 2 * (lmax / 2)) ntrunc += 1.0;
      } else {
        nnan += 1.0;
        if (pooled) G[0][threadIdx.x] = acov_nan();  // a chain without a variance: no pooled estimate either
      }
      ess[(int64_t)c * m + e] = v;
      ess_lag[(int64_t)c * m + e] = lag;
    }
    if (!ess_pooled) continue;
    double vp = acov_nan(), se = acov_nan();
    if (pooled) {
      const double nd = (double)n_common, cp = (double)n_part;
      const double mbar = sm / cp, W = G[0][threadIdx.x] / cp;
      double ssq = 0.0;
      for (int c = 0; c < C; ++c) {
        const int64_t n = count[c];
        if (n < 4) continue;
        const int np = (int)(n % B);
        const int64_t n0 = n - np;
        double p;
        const double t = acov_total(tot + (int64_t)c * m, head + (int64_t)c * K * m, ring + (int64_t)c * R * m, m, e, n0, np,
                                    (int)(n0 % R), R, &p);
        const double dm = (p + t / nd) - mbar;
        ssq = ssq + dm * dm;
      }
      double varp = (nd - 1.0) / nd * W;
      if (n_part > 1) varp = varp + ssq / (cp - 1.0);
      if (varp > 0.0 && varp < INFINITY) {
        const int lmax = K < n_common ? K : (int)n_common;
        Geyer gy;
        for (int l = 0; l < lmax; ++l) gy.step(l, 1.0 - (W - G[l][threadIdx.x] / cp) / varp);
        int lag;
        vp = gy.ess(cp * nd, lmax, &lag);
        se = sqrt(varp / vp);
      }
    }
    ess_pooled[e] = vp;
    if (mcse) mcse[e] = se;
  }
  if (part) stats_partial<false, ESS_THREADS / 64>(part, emin, nnan, ntrunc);
}

static inline bool acov_lags_ok(int64_t K) { return K >= 2 && K <= ACOV_MAX_LAGS && K % 2 == 0; }

}  // namespace pxm

using namespace pxm;

extern "C" {

int pxm_acov_stage_depth(void) { return ACOV_STAGE; }

int64_t pxm_acov_state_doubles(int64_t m, int C, int K) { return acov_lags_ok(K) ? rows_doubles(m, C, K) : -1; }

int64_t pxm_acov_ring_doubles(int64_t m, int C, int K) { return acov_lags_ok(K) ? rows_doubles(m, C, K - 1 + ACOV_STAGE) : -1; }

int64_t pxm_acov_scratch_doubles(int64_t m) { return stats_scratch_doubles(m, ESS_THREADS, 3); }

int pxm_acov_update(const double* x, int x_stride, const int64_t* count, double* acc, double* tot, double* head, double* ring,
                    const int* mask, int64_t m, int C, int K, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (save_check("pxm_acov_update", m, C, x_stride, st)) return -1;
  PXM_REQUIRE(acov_lags_ok(K), "pxm_acov_update: K must be even with 2 <= K <= 64");
  PXM_REQUIRE(pxm_acov_ring_doubles(m, C, K) > 0, "pxm_acov_update: C (K - 1 + B) m overflows");
  PXM_REQUIRE(x && count && acc && tot && head && ring, "pxm_acov_update: null buffer");
  const dim3 grid = rows_grid(m, ACOV_THREADS, ACOV_MAX_BLOCKS, C);  // 8-byte coalesced accesses
  const int64_t ldx = m * x_stride;
#define ACOV_LAUNCH(KMAX) \
  hipLaunchKernelGGL((k_acov_update<KMAX>), grid, dim3(ACOV_THREADS), 0, st, x, ldx, x_stride, count, acc, tot, head, ring, mask, m, K)
  if (K <= 8) ACOV_LAUNCH(8);
  else if (K <= 16) ACOV_LAUNCH(16);
  else if (K <= 32) ACOV_LAUNCH(32);
  else ACOV_LAUNCH(64);
#undef ACOV_LAUNCH
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_acov_ess(const int64_t* count, const double* acc, const double* tot, const double* head, const double* ring, int64_t m, int C,
                 int K, double* ess, int* ess_lag, double* ess_pooled, double* mcse, double* stats, double* scratch,
                 pxm_stream_t stream) {
  PXM_REQUIRE(C >= 1, "pxm_acov_ess: need C >= 1");
  PXM_REQUIRE(m >= 1, "pxm_acov_ess: need m >= 1");
  PXM_REQUIRE(acov_lags_ok(K), "pxm_acov_ess: K must be even with 2 <= K <= 64");
  PXM_REQUIRE(pxm_acov_ring_doubles(m, C, K) > 0, "pxm_acov_ess: C (K - 1 + B) m overflows");
  PXM_REQUIRE(count && acc && tot && head && ring && ess && ess_lag, "pxm_acov_ess: null buffer");
  PXM_REQUIRE(!mcse || ess_pooled, "pxm_acov_ess: mcse needs ess_pooled");
  PXM_REQUIRE(!stats || scratch, "pxm_acov_ess: stats needs scratch");
  hipStream_t st = (hipStream_t)stream;
  note_stream(st);
  Counts k;  // the pooled estimate is over chains of one length
  if (ess_pooled && (read_counts(count, C, st, k) ||
                     require_common_count(k, "pxm_acov_ess: the pooled ESS", "the per-chain values do not: call without ess_pooled")))
    return -1;
  const int64_t n_common = k.n_part >= 1 ? k.lo : 0;
  const int nb = stats_blocks(m, ESS_THREADS);
  hipLaunchKernelGGL(k_acov_ess, dim3(nb), dim3(ESS_THREADS), 0, st, count, acc, tot, head, ring, m, C, K, n_common, k.n_part, ess, ess_lag,
                     ess_pooled, mcse, stats ? scratch : nullptr);
  PXM_HIP(hipGetLastError());
  if (stats) {
    hipLaunchKernelGGL((k_summary_stats<false, 2>), dim3(1), dim3(STATS_THREADS), 0, st, scratch, nb, stats);
    PXM_HIP(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
