// Exact streaming credible intervals: per chain and element the k smallest and the k largest samples
// seen so far, kept on the device at the samplers' save points.  numpy's linear quantile at alpha / 2 (1 - alpha / 2) of n
// samples needs two order statistics within k(alpha, N) of the bottom (top), so the two tails give np.quantile of the whole
// chain -- the credible_interval_range of pxmcmc/uncertainty.py:7-16 -- without the chain.
//
// Each tail is a binary heap over its k slots, slot-major ([C][k][m]: slot s of every element of a chain is one row, so
// adjacent lanes touch adjacent addresses in every slot): `lo` a max-heap of the k smallest, `hi` a min-heap of the k
// largest, ordered by qkey().  The root (slot 0) is the tail's threshold, the value a new sample has to beat; thr_lo /
// thr_hi [C][m] mirror the roots in the layout of the sample.  A sample beyond a threshold replaces the root and sifts down:
// two reads per level, log2 k levels, in place of a rescan of the k slots.  Saves are staged in a ring of TAIL_STAGE rows
// per chain and merged into the heaps when it is full (k_tails_update says why).  After them: the same select on a whole
// chain that is resident on the device (k_quantile_range).
#include "qkey.h"
#include "summary.h"

#include "../../include/pxmcmc_amd.h"

namespace pxm {

constexpr int TAIL_THREADS = 256;
constexpr int TAIL_STAGE = 16;         // saves staged in the ring between two merges into the heaps (2 bits each in a word)
constexpr int TAIL_MAX_BLOCKS = 4096;  // per chain; the rest of a row is covered by the grid-stride loop

// Both heaps run the same code: with the keys of `hi` complemented (flip = ~0, 0 for `lo`) the entry nearer the root is the
// larger key in either, so lanes that insert into different tails do not diverge.
__device__ __forceinline__ uint64_t tail_flip(bool upper) { return upper ? ~0ull : 0ull; }

// Fill phase: the heap of one element (h: its slot 0, ld doubles between slots) holds n < k values; v goes to slot n and
// sifts up.  The path n -> (n - 1) / 2 -> ... -> 0 is the same for every lane, so every read is a coalesced row access.
// True when v became the root.
__device__ __forceinline__ bool heap_push(double* __restrict__ h, int64_t ld, int64_t n, double v, bool upper) {
  const uint64_t flip = tail_flip(upper), kv = qkey(v) ^ flip;
  int64_t pos = n;
  while (pos > 0) {
    const int64_t par = (pos - 1) >> 1;
    const double pv = h[par * ld];
    if (kv <= (qkey(pv) ^ flip)) break;
    h[pos * ld] = pv;
    pos = par;
  }
  h[pos * ld] = v;
  return pos == 0;
}

// Steady state: v beats the root of a full heap of k slots, takes its place and sifts down.  Returns the new root.  Every
// index formed is < k.
__device__ __forceinline__ double heap_replace_root(double* __restrict__ h, int64_t ld, int64_t k, double v, bool upper) {
  const uint64_t flip = tail_flip(upper), kv = qkey(v) ^ flip;
  int64_t pos = 0;
  double root = v;
  for (;;) {
    int64_t ch = 2 * pos + 1;
    if (ch >= k) break;
    double cv = h[ch * ld];
    uint64_t ck = qkey(cv) ^ flip;
    if (ch + 1 < k) {
      const double rv = h[(ch + 1) * ld];
      const uint64_t rk = qkey(rv) ^ flip;
      if (rk > ck) {
        ++ch;
        cv = rv;
        ck = rk;
      }
    }
    if (ck <= kv) break;
    h[pos * ld] = cv;
    if (pos == 0) root = cv;
    pos = ch;
  }
  h[pos * ld] = v;
  return root;
}

// One save of chain c = blockIdx.y, n = count[c] samples before it (count is only read: the pxm_moments_update queued behind
// this launch advances it).  A masked-out chain returns before it touches memory; so does one with n >= nsamples, more
// saves than the capacity was sized for (the read-out reports it).  n < k: fill phase, slot n of both heaps.  Later the
// sample is staged: save n goes to row (n - k) % TAIL_STAGE of the chain's ring, a coalesced copy, and the save that fills
// the ring merges its TAIL_STAGE samples into the heaps.  An insert moves a 128-byte line per slot it touches, a line that
// holds the slot for 16 neighbouring elements; merging TAIL_STAGE saves at once touches each line at most once per pass
// instead of once per save, and the thresholds are read once per pass.  The read-out takes the samples still in the ring
// into its select, so nothing has to be flushed.
template <int XS>
__global__ __launch_bounds__(TAIL_THREADS) void k_tails_update(const double* __restrict__ x, int64_t ldx,
                                                               const int64_t* __restrict__ count, double* __restrict__ lo,
                                                               double* __restrict__ hi, double* __restrict__ thr_lo,
                                                               double* __restrict__ thr_hi, double* __restrict__ stage,
                                                               const int* __restrict__ mask, int64_t m, int64_t k,
                                                               int64_t nsamples) {
  const int c = blockIdx.y;
  if (mask && !mask[c]) return;
  const int64_t n = count[c];
  if (n < 0 || n >= nsamples) return;
  const int64_t row = (int64_t)c * m;
  const double* xr = x + (int64_t)c * ldx;
  double* tl = thr_lo + row;
  double* th = thr_hi + row;
  double* lor = lo + (int64_t)c * k * m;
  double* hir = hi + (int64_t)c * k * m;
  double* sr = stage + (int64_t)c * TAIL_STAGE * m;
  const int64_t tid = (int64_t)blockIdx.x * TAIL_THREADS + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * TAIL_THREADS;

  if (n < k) {
    for (int64_t j = tid; j < m; j += stride) {
      const double v = xr[j * XS];
      if (heap_push(lor + j, m, n, v, false)) tl[j] = v;
      if (heap_push(hir + j, m, n, v, true)) th[j] = v;
    }
    return;
  }

  const int64_t slot = (n - k) % TAIL_STAGE;
  if (slot < TAIL_STAGE - 1) {
    for (int64_t j = tid; j < m; j += stride) sr[slot * m + j] = xr[j * XS];
    return;
  }

  for (int64_t j = tid; j < m; j += stride) {
    double v[TAIL_STAGE];
#pragma unroll
    for (int s = 0; s < TAIL_STAGE - 1; ++s) v[s] = sr[s * m + j];
    v[TAIL_STAGE - 1] = xr[j * XS];
    double a = tl[j], b = th[j];
    uint64_t ka = qkey(a), kb = qkey(b);
    // candidates by the thresholds before the pass, which only tighten: bit 2 s for `lo`, 2 s + 1 for `hi` (both while the
    // tails overlap)
    unsigned pend = 0;
#pragma unroll
    for (int s = 0; s < TAIL_STAGE; ++s) {
      const uint64_t kv = qkey(v[s]);
      pend |= ((kv < ka ? 1u : 0u) | (kv > kb ? 2u : 0u)) << (2 * s);
    }
    if (!pend) continue;
    // The candidates are drained one per trip: a sift-down is a chain of dependent, divergent loads, and this way a wave runs
    // as many of them as its busiest lane has candidates, not one for every candidate that any of its lanes has.  The sample
    // is read again from the ring (it is in the cache; a register array indexed by the bit would go to scratch memory), so
    // the last one joins the ring as well.
    sr[(TAIL_STAGE - 1) * m + j] = v[TAIL_STAGE - 1];
    const unsigned entered = pend;
    while (pend) {
      const int bit = __ffs(pend) - 1;
      pend &= pend - 1;
      const bool upper = bit & 1;
      const double w = sr[(bit >> 1) * m + j];
      const uint64_t kw = qkey(w);
      if (upper ? kw > kb : kw < ka) {
        const double r = heap_replace_root((upper ? hir : lor) + j, m, k, w, upper);
        if (upper) {
          b = r;
          kb = qkey(r);
        } else {
          a = r;
          ka = qkey(r);
        }
      }
    }
    if (entered & 0x55555555u) tl[j] = a;
    if (entered & 0xaaaaaaaau) th[j] = b;
  }
}

// read-out of one chain, one lane per element: ns = min(k, n) slots of each tail hold samples and np rows of the ring hold
// samples not merged yet; each tail with those rows is viewed as an (ns + np)-sample chain with leading dimension m for the
// select of k_quantile_range, one quantile per tail.  ns == 0: NaN
__global__ __launch_bounds__(TAIL_THREADS) void k_tails_quantiles(const double* __restrict__ lo, const double* __restrict__ hi,
                                                                  const double* __restrict__ stage, int64_t m, int64_t ns,
                                                                  int64_t np, int64_t r_lo, double g_lo, int64_t r_hi, double g_hi,
                                                                  double* __restrict__ q_lo, double* __restrict__ q_hi) {
  const int64_t j = (int64_t)blockIdx.x * TAIL_THREADS + threadIdx.x;
  if (j >= m) return;
  if (ns == 0) {
    q_lo[j] = q_hi[j] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  double v[1];
  select_quantiles<1>([=](int64_t s) { return s < ns ? lo[s * m + j] : stage[(s - ns) * m + j]; }, ns + np, {r_lo}, {g_lo}, v);
  q_lo[j] = v[0];
  select_quantiles<1>([=](int64_t s) { return s < ns ? hi[s * m + j] : stage[(s - ns) * m + j]; }, ns + np, {r_hi}, {g_hi}, v);
  q_hi[j] = v[0];
}

}  // namespace pxm

using namespace pxm;

// ---- quantile credible-interval range of a chain resident on the device (pxmcmc/uncertainty.py:7-16) ------------------------
// out[j] = Q(1 - alpha/2) - Q(alpha/2) of column j of chain[ns][np] (numpy's default "linear" quantile: virtual index q (ns - 1),
// the two order statistics around it, numpy's lerp).  One thread per column -- adjacent threads read adjacent columns, every
// pass over the samples is a fully coalesced sweep of the chain -- and the radix select of qkey.h, both quantiles in the same
// sweep: 33 sweeps of the chain.  (Outside the namespace, as it always was: the kernel's name is an exported symbol.)
__global__ __launch_bounds__(256) void k_quantile_range(const double* __restrict__ chain, int64_t ns, int64_t np, int64_t ld,
                                                        int64_t i_lo, double g_lo, int64_t i_hi, double g_hi, double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= np) return;
  const int64_t idx[2] = {i_lo, i_hi};
  const double g[2] = {g_lo, g_hi};
  double v[2];
  const double* col = chain + j;
  select_quantiles<2>([=](int64_t s_) { return col[s_ * ld]; }, ns, idx, g, v);
  out[j] = v[1] - v[0];
}

extern "C" {

int64_t pxm_tails_buffer_doubles(int64_t m, int C, int64_t k) { return rows_doubles(m, C, k); }

int64_t pxm_tails_stage_doubles(int64_t m, int C) { return pxm_tails_buffer_doubles(m, C, TAIL_STAGE); }

int pxm_tails_update(const double* x, int x_stride, const int64_t* count, double* lo, double* hi, double* thr_lo, double* thr_hi,
                     double* stage, const int* mask, int64_t m, int C, int64_t k, int64_t nsamples, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (save_check("pxm_tails_update", m, C, x_stride, st)) return -1;
  PXM_REQUIRE(k >= 1 && k <= nsamples, "pxm_tails_update: need 1 <= k <= nsamples");
  PXM_REQUIRE(pxm_tails_buffer_doubles(m, C, k) > 0 && pxm_tails_stage_doubles(m, C) > 0, "pxm_tails_update: C k m overflows");
  PXM_REQUIRE(x && count && lo && hi && thr_lo && thr_hi && stage, "pxm_tails_update: null buffer");
  PXM_REQUIRE(aligned16(x) && aligned16(thr_lo) && aligned16(thr_hi), "pxm_tails_update: x, thr_lo and thr_hi must be 16-byte aligned");
  const dim3 grid = rows_grid(m, TAIL_THREADS, TAIL_MAX_BLOCKS, C);  // 8-byte coalesced accesses
  const int64_t ldx = m * x_stride;
  if (x_stride == 1)
    hipLaunchKernelGGL((k_tails_update<1>), grid, dim3(TAIL_THREADS), 0, st, x, ldx, count, lo, hi, thr_lo, thr_hi, stage, mask, m, k, nsamples);
  else
    hipLaunchKernelGGL((k_tails_update<2>), grid, dim3(TAIL_THREADS), 0, st, x, ldx, count, lo, hi, thr_lo, thr_hi, stage, mask, m, k, nsamples);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_tails_quantiles(const int64_t* count, const double* lo, const double* hi, const double* stage, int64_t m, int C, int64_t k, int64_t nsamples,
                        double alpha, double* q_lo, double* q_hi, pxm_stream_t stream) {
  PXM_REQUIRE(C >= 1, "pxm_tails_quantiles: need C >= 1");
  PXM_REQUIRE(m >= 1, "pxm_tails_quantiles: need m >= 1");
  PXM_REQUIRE(k >= 1 && k <= nsamples, "pxm_tails_quantiles: need 1 <= k <= nsamples");
  PXM_REQUIRE(pxm_tails_buffer_doubles(m, C, k) > 0, "pxm_tails_quantiles: C k m overflows");
  PXM_REQUIRE(count && lo && hi && stage && q_lo && q_hi, "pxm_tails_quantiles: null buffer");
  PXM_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "pxm_tails_quantiles: alpha must lie in [0, 1]");
  hipStream_t st = (hipStream_t)stream;
  note_stream(st);
  Counts counts;  // they decide the ranks
  if (read_counts(count, C, st, counts)) return -1;
  struct Ranks {
    int64_t ns, np, r_lo, r_hi;  // filled slots of a tail, rows of the ring not merged yet, ranks in the two together
    double g_lo, g_hi;
  };
  std::vector<Ranks> ranks(C);
  for (int c = 0; c < C; ++c) {
    const int64_t n = counts.n[c];
    if (n < 0 || n > nsamples) {
      set_error("pxm_tails_quantiles: chain " + std::to_string(c) + " holds " + std::to_string(n) + " samples, the tails were sized for " +
                std::to_string(nsamples) + " (the saves beyond were not recorded)");
      return -1;
    }
    Ranks& r = ranks[c];
    r.ns = n < k ? n : k;
    r.np = n > k ? (n - k) % TAIL_STAGE : 0;
    if (n == 0) continue;
    int64_t i_lo, i_hi;
    quantile_split(alpha / 2, n, &i_lo, &r.g_lo);
    quantile_split(1 - alpha / 2, n, &i_hi, &r.g_hi);
    r.r_lo = i_lo;
    r.r_hi = i_hi - (n - r.ns - r.np);
    // both order statistics of each pair inside the tail (the upper one is clipped to n - 1, as numpy clips it)
    const int64_t top_lo = i_lo + 1 < n ? i_lo + 1 : i_lo;
    if (top_lo >= r.ns || i_hi < n - r.ns) {
      set_error("pxm_tails_quantiles: alpha = " + std::to_string(alpha) + " at " + std::to_string(n) + " samples needs order statistics " +
                std::to_string(top_lo) + " and " + std::to_string(i_hi) + ", outside tails of " + std::to_string(k) + " slots");
      return -1;
    }
  }
  const unsigned nb = (unsigned)((m + TAIL_THREADS - 1) / TAIL_THREADS);
  for (int c = 0; c < C; ++c) {
    const Ranks& r = ranks[c];
    hipLaunchKernelGGL(k_tails_quantiles, dim3(nb), dim3(TAIL_THREADS), 0, st, lo + (int64_t)c * k * m, hi + (int64_t)c * k * m,
                       stage + (int64_t)c * TAIL_STAGE * m, m, r.ns, r.np, r.r_lo, r.g_lo, r.r_hi, r.g_hi, q_lo + (int64_t)c * m, q_hi + (int64_t)c * m);
    PXM_HIP(hipGetLastError());
  }
  return 0;
}

int pxm_quantile_range(const double* chain, int64_t nsamples, int64_t nparams, int64_t ld, double alpha, double* out,
                       pxm_stream_t stream) {
  PXM_REQUIRE(chain && out, "pxm_quantile_range: null buffer");
  PXM_REQUIRE(nsamples >= 1 && nparams >= 1 && ld >= nparams, "pxm_quantile_range: bad shape");
  PXM_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "pxm_quantile_range: alpha must lie in [0, 1]");
  int64_t i_lo, i_hi;
  double g_lo, g_hi;
  quantile_split(alpha / 2, nsamples, &i_lo, &g_lo);
  quantile_split(1 - alpha / 2, nsamples, &i_hi, &g_hi);
  hipLaunchKernelGGL(k_quantile_range, dim3((unsigned)((nparams + 255) / 256)), dim3(256), 0, (hipStream_t)stream, chain, nsamples,
                     nparams, ld, i_lo, g_lo, i_hi, g_hi, out);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
