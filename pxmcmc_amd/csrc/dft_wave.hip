// phi-DFT stage, the two Bluestein units that run a ring on whole waves with eight points per lane: the pair unit (below)
// with the grouped launches of a wavelet plan's scales, which also dispatch to the exact-length bodies of n = 511
// (dft_pfa.h), and the quad unit (further down).  (The two share one translation unit: compiled on its own, the quad
// unit's kernels leave the module and the inlining of the shared epilogue helpers into the fused pair kernels changes --
// 37 spilled VGPRs in the grouped rings -> X' -> rings kernel instead of none.)
//
// Pair unit: a pair of waves per ring set, every ring length n = 2L-1 <= 511, i.e. L <= 256.
//
// Bluestein at M = 2 Mh, Mh = max(64, nextpow2(n)) = 64 r0, r0 in {1, 2, 4, 8}.  The chirped input a[j] is zero
// above n <= Mh, so the first radix-2 (DIF) stage of the M-point transform is free: the even bins are the
// Mh-point transform of a[j], the odd bins that of a[j] W_M^j, and after the filter
//     conv[j] = y_even[j] + W_M^(-j) y_odd[j],   j < n <= Mh.
// A PAIR of waves owns a ring set of RPW = 8 / r0 rings (one ring of 512 slots, two of 256, ...): wave 0 runs the
// even-bin convolution, wave 1 the odd-bin one, each with 8 complex points per lane; they exchange their shares
// through LDS (workgroup barrier) and each finishes FOUR of the eight elements a lane holds (epilogue, Philox).
// 84-127 VGPR, no spills: 4 waves per SIMD -- the one-wave M = 1024 kernels of round 1 (dft3.hip, removed) held 16 points per lane at
// 203 VGPR, 2 waves per SIMD, and were bound by VALU issue latency at that occupancy with 1.5x the instructions
// (DESIGN.md section 9).  Inside a wave every transpose of the transform needs wave-local ordering only (dft_wave.h).
#include "dft_unit.h"
#include "dft_wave.h"
#include "update.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace pxm {

constexpr int D5_RMAX = 4;        // most chains (units: ring sets) per workgroup; the launch bound of the kernels

struct Dft5Args {
  int L, n, Rp;
  int lgR;              // log2 of R = chains (units) per workgroup: 1, 2 or 4 (16 R-byte segments of the ring arrays)
  const double2* cE;    // [Mh] chirp c_j = exp(-i pi j^2 / n), zero for j >= n
  const double2* cO;    // [Mh] c_j W_M^j       (input of the odd-bin half)
  const double2* dO;    // [Mh] c_j W_M^(-j)    (output weight of the odd-bin half)
  const double2* tw1;   // [8][64] W_Mh^(lam(lane) k2)
  const double2* wt;    // [8][8]  W_(8 r0)^(a b)
  const double2* bE;    // [r0][64] FFT_M(filter)/M at the even bins, in the order pass 3 leaves them
  const double2* bO;    // [r0][64] the odd bins
  unsigned* err;        // status word of the owning plan (bit PXM_STATUS_PAIR_SYNC: a pair wait expired) or null
  unsigned spin_limit;  // bound of the pair wait (1 << 18; PXM_DEBUG_PAIR_SYNC_LIMIT at plan creation forces an expiry)
  const double* pfa;    // n = 511: table block of the exact-length unit (dft_pfa.h) for the single-scale launches, or null
};

// one scale of a grouped launch
struct Dft5Group {
  Dft5Args a;
  int64_t g_off;  // this scale's ring array inside the workspace (doubles)
  int64_t ring0;  // offset of its coefficient block inside a chain (complex elements)
  int r0;
  int b0, nbx, nby;  // first block of the scale in the grid, its blocks along rings / chain groups
  int xs;            // ring sets (workgroups along the rings) per 128-B line of the ring array: > 1 on narrow arrays
  int64_t tbase;     // the scale's table allocation as an offset (doubles) from the workspace base ...
  int toff[7];       // ... and cE, cO, dO, tw1, wt, bE, bO inside it (doubles)
  int pfa_off;       // r0 == 9 (exact-length body, n = 511): the PFA table block inside the allocation (doubles)
  int pfa_passes;    // ... and the ring pairs a workgroup of that body handles one after the other (1 or 2)
};

// The two waves of a ring set run one half each (half 0: even bins, half 1: odd bins) and leave
// their weighted share t_w[p] of every output element in x; d5_exchange then hands each wave the partner's share
// of the FOUR elements it owns (p in [4 half, 4 half + 4)).
template <int R0>
__device__ __forceinline__ void d5_dft_half(double2 (&x)[8], double2* plane, int lane, const D5Lane& q, int jb, int half,
                                            const Dft5Args& a, const double2* tw) {
  // (the chirp tables are zero-padded to Mh entries: elements j >= n enter and leave as zeros without a test)
  const double2* __restrict__ cin = (half ? a.cO : a.cE) + jb;
  const double2* __restrict__ cout = (half ? a.dO : a.cE) + jb;
#pragma unroll
  for (int p = 0; p < 8; ++p) x[p] = cmul(x[p], cin[8 * R0 * p]);
  d5_conv<R0>(x, plane, lane, q, tw, half ? a.bO : a.bE);
#pragma unroll
  for (int p = 0; p < 8; ++p) x[p] = cmul(x[p], cout[8 * R0 * p]);
}
// The share of the partner's elements -> partner; x[0..4) <- own share + partner's share of the wave's OWN elements
// p = 4 half + u (always kept in x[0..4): register indices stay compile-time).
// SLOT selects one of two disjoint exchange regions of the planes (two exchanges may be in flight).
template <int SLOT>
__device__ __forceinline__ void d5_exchange_sum(double2 (&x)[8], double2* plane, double2* pplane, int lane, int half,
                                                unsigned* pcnt, unsigned& epoch, const D5Sync& sy) {
#pragma unroll
  for (int u = 0; u < 4; ++u) plane[256 * SLOT + 64 * u + lane] = d5_sel(half, x[u], x[4 + u]);
  d5_pair_sync(pcnt, epoch += 2, lane, sy);
#pragma unroll
  for (int u = 0; u < 4; ++u) x[u] = cadd(d5_sel(half, x[4 + u], x[u]), pplane[256 * SLOT + 64 * u + lane]);
}
// own elements x[0..4) -> partner; x <- all 8 elements of the ring in natural order (both waves then hold them)
template <int SLOT>
__device__ __forceinline__ void d5_exchange_fill(double2 (&x)[8], double2* plane, double2* pplane, int lane, int half,
                                                 unsigned* pcnt, unsigned& epoch, const D5Sync& sy) {
#pragma unroll
  for (int u = 0; u < 4; ++u) plane[256 * SLOT + 64 * u + lane] = x[u];
  d5_pair_sync(pcnt, epoch += 2, lane, sy);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const double2 o = pplane[256 * SLOT + 64 * u + lane], own = x[u];
    x[u] = d5_sel(half, o, own);
    x[4 + u] = d5_sel(half, own, o);
  }
}

// the same where the wave's own (updated) elements already stand in exchange region SLOT of its plane (STOCK epilogue)
template <int SLOT>
__device__ __forceinline__ void d5_exchange_fill_parked(double2 (&x)[8], const double2* plane, const double2* pplane, int lane, int half,
                                                        unsigned* pcnt, unsigned& epoch, const D5Sync& sy) {
  d5_pair_sync(pcnt, epoch += 2, lane, sy);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const double2 o = pplane[256 * SLOT + 64 * u + lane], own = plane[256 * SLOT + 64 * u + lane];
    x[u] = d5_sel(half, o, own);
    x[4 + u] = d5_sel(half, own, o);
  }
}

// ---- workgroup geometry ---------------------------------------------------------------------------------------
// Two waves per ring set: wave = 2 * unit + half; unit u = chain u of the workgroup; lane -> ring rho of the unit.  stage: the rings of the workgroup in [ring][k][chain] order (16-B x R
// segments per m in the ring arrays); the chain slot is rotated with k so that the lanes' strided reads
// (consecutive k, one chain) spread over the banks.
#define PXM_D5_GEOMETRY                                                                     \
  constexpr int RPW = 8 / R0;                                                               \
  constexpr int lgR = 2, R = 4;                       /* chains per workgroup (compile-time: index arithmetic folds) */ \
  const int n = a.n;                                                                        \
  /* Mh = 64 r0 is the smallest power of two >= n (r0 > 1): half of a lane's elements, j < 32 r0, need no j < n test */ \
  if (R0 > 1) __builtin_assume(n > 32 * R0 && n <= 64 * R0);                                \
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63; /* wave: a scalar */ \
  const int half = wave & 1, unit = wave >> 1;        /* two waves per ring set */          \
  const D5Lane q{lane & 7, lane >> 3};                                                      \
  const int r = unit;                                 /* chain of the workgroup */          \
  const int rho = q.lo / R0;                          /* ring of the unit this lane works on */ \
  const int jb = (q.lo & (R0 - 1)) + R0 * q.hi;       /* its first element: j = jb + 8 r0 p */ \
  constexpr int TRS = RPW;                            /* rings per workgroup */             \
  const int trs = rho;                                /* own ring within the workgroup */   \
  const int t = bx * TRS + trs;                       /* own ring */                        \
  const int c0 = by * R, ch = c0 + r;                                                       \
  const bool tv = t < a.L;                                                                  \
  const int Cp = ncol >> 1;                                                                 \
  const int rsh = 4 - lgR;                            /* 16 / R: rotation period of the chain slot */ \
  constexpr int P1 = 4;                               /* the wave owns the elements p = pb + u, u < P1, */ \
  const int pb = 4 * half;                            /* and keeps them in x[u] */          \
  double2* stage = lds5;                                                                    \
  double2* plane = lds5 + wave * D5_PLANE;                                                  \
  double2* pplane = lds5 + (wave ^ 1) * D5_PLANE;                                           \
  const double2* tw = lds5 + 2 * R * D5_PLANE;        /* twiddles of the transform passes (LDS copy) */ \
  /* (row a = 0 of the wt copy, tw[448 .. 455], is never read: it holds the pair counters of d5_pair_sync) */ \
  unsigned* pcnt = reinterpret_cast<unsigned*>(lds5 + 2 * R * D5_PLANE + 448) + unit;       \
  unsigned epoch = 0;                                                                       \
  const D5Sync sy{a.err, a.spin_limit};                                                     \
  for (int i = threadIdx.x; i < D5_TW; i += 512)                                     \
    lds5[2 * R * D5_PLANE + i] = i < 448 ? a.tw1[64 + i] : (i < 456 ? double2{0.0, 0.0} : a.wt[i - 448]);
#define PXM_D5_SLOT(RING, K, CH) ((((RING)*n + (K)) << lgR) + (((CH) + ((K) >> rsh)) & (R - 1)))

// stage -> G rows of every ring of the workgroup.  ZFILL (pixels -> rings): chain groups without a live chain do
// not run at all, and the last live group also writes zeros into the padding slots of its (m, ring) lines -- the
// ring arrays keep zero padding columns and every 128-B line is written whole.
#define PXM_D5_STORE_RINGS(ZFILL)                                                                              \
  {                                                                                                            \
    const int rr = threadIdx.x & (R - 1), kq = threadIdx.x >> lgR, kstep = (512 >> lgR) /* workgroups of 512 threads */;                 \
    const int mstride = a.Rp * Cp; /* complex elements between consecutive m */                                \
    double2* Gc = reinterpret_cast<double2*>(G) + c0 + rr;                                                     \
    const bool zf = (ZFILL) && c0 + R >= C;                                                                    \
    if (c0 + rr < Cp) {                                                                                        \
      _Pragma("nounroll") for (int trr = 0; trr < TRS; ++trr) {                                                \
        const int tt = bx * TRS + trr;                                                                         \
        if (tt >= a.L) break;                                                                                  \
        for (int k = kq; k < n; k += kstep) {                                                                  \
          const int mi = (k < a.L) ? k + a.L - 1 : k - a.L; /* m + L - 1 */                                    \
          double2* line = Gc + mi * mstride + tt * Cp;                                                         \
          *line = stage[PXM_D5_SLOT(trr, k, rr)];                                                              \
          if (zf) for (int z = R; c0 + rr + z < Cp; z += R) line[z] = double2{0.0, 0.0};                       \
        }                                                                                                      \
      }                                                                                                        \
    }                                                                                                          \
  }

// the transform of x (all 8 elements in every wave of the ring) -> the wave's own elements of the result in x[0 .. P1)
#define PXM_D5_TRANSFORM(SLOT)                                            \
  d5_dft_half<R0>(x, plane, lane, q, jb, half, a, tw);                    \
  d5_exchange_sum<SLOT>(x, plane, pplane, lane, half, pcnt, epoch, sy);
// own elements of x -> stage (after every plane of the workgroup is dead)
#define PXM_D5_TO_STAGE                                                   \
  d5_barrier();                                                        \
  _Pragma("unroll") for (int u = 0; u < P1; ++u) {                        \
    const int j = jb + 8 * R0 * (pb + u);                                 \
    if (j < n) stage[PXM_D5_SLOT(trs, j, r)] = x[u];                      \
  }                                                                       \
  d5_barrier();

template <int R0>
__device__ __forceinline__ void px2ring_body5(const Dft5Args& a, const PxIn& in, double* __restrict__ G, int ncol, int C,
                                              int bx, int by, double2* lds5) {
  if ((by << 2) >= C) return;  // no live chain in this group: its slots are zero-filled by the last live group
  PXM_D5_GEOMETRY
  // each wave of the pair fetches half of the ring set (its four p) and the two share it through the stage
  {  // the wave's four elements: batched loads (elements past the ring end / dead rings re-read a valid element)
    int64_t ev[4];
    bool ok[4];
    double2 v[4];
    const bool act = ch < C && tv;
    const int64_t e_ring = in.ring0 + (int64_t)(tv ? t : 0) * n;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = jb + 8 * R0 * (pb + u);
      ok[u] = act && j < n;
      ev[u] = e_ring + (j < n ? j : 0);
    }
    if (ch < C) px_in_load_n<4>(in, ch, ev, ok, v);
    else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = double2{0.0, 0.0};
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = jb + 8 * R0 * (pb + u);
      if (j < n) stage[PXM_D5_SLOT(trs, j, r)] = v[u];
    }
  }
  d5_barrier();  // (also: the LDS copy of the twiddles is complete)
  double2 x[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int j = jb + 8 * R0 * p;
    x[p] = j < n ? stage[PXM_D5_SLOT(trs, j, r)] : double2{0.0, 0.0};
  }
  d5_barrier();  // the stage is dead: the planes may be written
  PXM_D5_TRANSFORM(0)
  PXM_D5_TO_STAGE
  PXM_D5_STORE_RINGS(true)
}

// rings -> pixels (inverse DFT by conjugation) with out's epilogue; RING_OUT: the written ring is transformed
// again and its rings go back IN PLACE over G (rings of S X -> X' and the rings of X' in one kernel).
#ifdef PXM_D5_TRACE
__device__ unsigned long long* g_dft_trace = nullptr;
#define PXM_D5_STAMP(K) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); d5_stamp[K] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); }
#else
#define PXM_D5_STAMP(K)
#endif
// N64: the Philox stream's Box-Muller step in double precision (PxOut::noise64; a kernel instantiation of its own: the
// fp64 evaluation holds ~40 registers and the update epilogue sits at the 128-VGPR budget of four waves per SIMD)
// STOCK: the launch is the stock MYULA update (dft_step_is_stock, sht_core.h; fp64 noise): its epilogue is px_stock_update4
// (update.h) on elements parked in the wave's plane, and none of the mode fields of PxOut is read
// XOUT: cache policy of the X' stores (mem_policy.h); STOCK only.
template <int R0, bool RING_OUT, bool N64, bool STOCK = false, int XOUT = MEM_DEFAULT>
__device__ __forceinline__ void ring2px_body5(const Dft5Args& a, double* __restrict__ G, int ncol, const PxOut& out, int C,
                                              int bx, int by, double2* lds5) {
  static_assert(STOCK || XOUT == MEM_DEFAULT, "only the stock instantiation carries a cache policy");
  // chain groups without a live chain do nothing (see run_tasks / GemmAffine::ncol_live: nothing iterates on them)
  if ((by << 2) >= C) return;
#ifdef PXM_D5_TRACE
  unsigned long long d5_stamp[4] = {0, 0, 0, 0};
  const unsigned long long d5_t0 = wall_clock64();
#endif
  PXM_D5_GEOMETRY
  {  // rings of the workgroup -> stage; thread -> (chain rr, k), k advances by threads / R: no integer division
    const int rr = threadIdx.x & (R - 1), kq = threadIdx.x >> lgR, kstep = (512 >> lgR) /* workgroups of 512 threads */;
    const int mstride = a.Rp * Cp;  // complex elements between consecutive m
    const double2* Gc = reinterpret_cast<const double2*>(G) + c0 + rr;
    const bool cv = c0 + rr < Cp;
    // small scales hold several short rings per workgroup: RU of them are gathered together, so that the memory
    // latency is paid once per RU rings (a workgroup of the smallest scale spent 6.4 of its 22 us here, ring by ring)
    constexpr int RU = TRS >= 4 ? 4 : (TRS >= 2 ? 2 : 1);
    constexpr int NB = TRS >= 4 ? 1 : (TRS >= 2 ? 2 : 4);  // batches of independent loads per ring (RU * NB = 4 in flight)
#pragma nounroll
    for (int tr0 = 0; tr0 < TRS; tr0 += RU) {
      for (int kb = kq; kb < n; kb += NB * kstep) {
        double2 v[RU][NB];
#pragma unroll
        for (int ru = 0; ru < RU; ++ru) {
          const int tt = bx * TRS + tr0 + ru;
          const bool rv = cv && tt < a.L;
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            const int k = kb + u * kstep;
            v[ru][u] = double2{0.0, 0.0};
            if (rv && k < n) v[ru][u] = Gc[((k < a.L) ? k + a.L - 1 : k - a.L) * mstride + tt * Cp];
          }
        }
#pragma unroll
        for (int ru = 0; ru < RU; ++ru)
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            const int k = kb + u * kstep;
            if (k < n) stage[PXM_D5_SLOT(tr0 + ru, k, rr)] = double2{v[ru][u].x, -v[ru][u].y};  // inverse DFT by conjugation: y = conj(DFT(conj x))
          }
      }
    }
  }
  d5_barrier();
  PXM_D5_STAMP(0)  // rings staged
  double2 x[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int j = jb + 8 * R0 * p;
    x[p] = j < n ? stage[PXM_D5_SLOT(trs, j, r)] : double2{0.0, 0.0};
  }
  d5_barrier();
  PXM_D5_TRANSFORM(0)
  PXM_D5_STAMP(1)  // inverse transform done
  const bool act = ch < C && tv;
  const int64_t e0 = out.ring0 + (int64_t)t * n + jb + (int64_t)(8 * R0) * pb;  // the wave's first element; u advances by 8 r0
  const int64_t ce0 = (int64_t)ch * out.chain_stride + e0;
  if constexpr (STOCK) {
    static_assert(RING_OUT && N64, "the stock instantiation is the fused step with the fp64 noise stream");
    // The wave's four elements wait in exchange region 1 of its OWN plane -- dead since the transform, and where
    // d5_exchange_fill<1> would put the updated elements for the partner anyway -- while the noise is drawn: the operand
    // loads can then go first and fly across the Philox rounds (as in the exact-length body) without 16 more live registers.
    double2* park = plane + 256 + lane;
#pragma unroll
    for (int u = 0; u < 4; ++u) park[64 * u] = act ? x[u] : double2{0.0, 0.0};
    if (act) {
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) ok[u] = jb + 8 * R0 * (pb + u) < n;
      px_stock_update4<8 * R0, XOUT>(out, ok, e0, ce0, -(jb + 8 * R0 * pb), __builtin_amdgcn_readfirstlane(ch), out.iter + *out.iter_dev, park,
                               reinterpret_cast<const double2*>(&NOISE_LOG_TAB[0][0]), reinterpret_cast<const double2*>(&NOISE_SINCOS_TAB[0][0]));
    }
  } else if (act && out.X) {  // fused prox + MYULA update (pxmcmc/mcmc.py:185-201, prior.py:49-50)
    const uint64_t it_eff = out.iter + (out.iter_dev ? *out.iter_dev : 0);
    // (the chain slot is the same for every lane of a wave: as a scalar, the Philox key -- seed + chain * odd constant,
    // a 64-bit multiply -- is computed once on the scalar unit instead of per lane and per element)
    const int ch_s = __builtin_amdgcn_readfirstlane(ch);
#pragma unroll
    for (int g0 = 0; g0 < P1; g0 += 4) {  // all loads of a group first (independent), then its arithmetic
      // The loads are unconditional (elements past the ring end re-read the ring's element 0 and are dropped below;
      // the threshold vector and the injected noise sit behind ONE uniform branch per group): with a per-element
      // predicate around each load the compiler drained the memory pipe (s_waitcnt vmcnt(0)) once per element and
      // the workgroup paid four memory latencies here instead of one.
      double2 xs[4], wn[4];
      double Ts[4];
      int64_t eo[4];  // element offset from e0 (or to the ring's element 0)
      // The noise of the four elements BEFORE the operand loads, one element at a time: the fp64 Box-Muller keeps ~40
      // registers live, and evaluated between the loads and their use (beside xs / Ts / the addresses) it cost 250
      // spilled registers in this kernel (93 instead of 70 us per launch).  Ahead of the loads: 124 VGPR, no spills,
      // 66.6 us per grouped launch; element by element between the loads and their use: 8 spilled registers, one of
      // them a freshly loaded threshold, i.e. an s_waitcnt vmcnt(0) right behind the loads (68.4 us); behind the loads
      // as a block: 12 spills.
      double2 wph[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        wph[u] = double2{0.0, 0.0};
        if (!out.noise) wph[u] = px_noise_philox_t<N64>(out, ch_s, e0 + (int64_t)(8 * R0) * (g0 + u), it_eff);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = g0 + u;
        const bool ok = jb + 8 * R0 * (pb + p) < n;
        eo[u] = ok ? (int64_t)(8 * R0) * p : -(int64_t)(jb + 8 * R0 * pb);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) xs[u] = reinterpret_cast<const double2*>(out.X)[ce0 + eo[u]];
      if (out.T) {
#pragma unroll
        for (int u = 0; u < 4; ++u) Ts[u] = out.T[e0 + eo[u]];
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) Ts[u] = out.T_scalar;
      }
      if (out.noise) {
#pragma unroll
        for (int u = 0; u < 4; ++u) wn[u] = px_noise_load(out, ch, e0 + eo[u]);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) wn[u] = double2{0.0, 0.0};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = g0 + u;
        if (jb + 8 * R0 * (pb + p) >= n) {
          x[p] = double2{0.0, 0.0};
          continue;
        }
        const int64_t off = (int64_t)(8 * R0) * p;
        const double2 y{x[p].x, -x[p].y};
        double2 w = wn[u];
        if (!out.noise) w = wph[u];
        x[p] = px_update(out, xs[u], Ts[u], y, w);
        reinterpret_cast<double2*>(out.f)[ce0 + off] = x[p];
      }
    }
  } else if (act) {
    // plain / gathered output of the wave's P1 elements, and (RING_OUT) the residual invcov .* (image - data) that
    // goes back to the rings: the loads of all elements first (elements past the ring end re-read the ring's
    // element 0), then the arithmetic -- one memory latency per batch instead of one or two per element
    bool ok[P1];
    int64_t ev[P1];
    double2 yv[P1];
#pragma unroll
    for (int p = 0; p < P1; ++p) {
      ok[p] = jb + 8 * R0 * (pb + p) < n;
      ev[p] = ok[p] ? e0 + (int64_t)(8 * R0) * p : out.ring0 + (int64_t)t * n;
      yv[p] = double2{x[p].x, -x[p].y};
    }
    px_out_store_n<P1>(out, ch, ev, yv, ok);
    if (RING_OUT && out.rdata) {
      double2 rd[P1], rc[P1];
#pragma unroll
      for (int p = 0; p < P1; ++p) rd[p] = reinterpret_cast<const double2*>(out.rdata)[ev[p]];
      if (out.rinvcov_complex) {
#pragma unroll
        for (int p = 0; p < P1; ++p) rc[p] = reinterpret_cast<const double2*>(out.rinvcov)[ev[p]];
      } else {
#pragma unroll
        for (int p = 0; p < P1; ++p) rc[p] = double2{out.rinvcov[ev[p]], 0.0};
      }
#pragma unroll
      for (int p = 0; p < P1; ++p) {
        const double2 d = csub(yv[p], rd[p]);
        yv[p] = out.rinvcov_complex ? cmul(rc[p], d) : double2{rc[p].x * d.x, rc[p].x * d.y};
      }
    }
#pragma unroll
    for (int p = 0; p < P1; ++p) x[p] = ok[p] ? yv[p] : double2{0.0, 0.0};
  } else {
#pragma unroll
    for (int p = 0; p < P1; ++p) x[p] = double2{0.0, 0.0};  // padding chains / rings: their rings are kept at zero
  }
  if (!RING_OUT) return;
  PXM_D5_STAMP(2)  // prox + update + noise done
  // ---- forward transform of the updated ring
  if constexpr (STOCK) d5_exchange_fill_parked<1>(x, plane, pplane, lane, half, pcnt, epoch, sy);  // (its own elements stand there already)
  else d5_exchange_fill<1>(x, plane, pplane, lane, half, pcnt, epoch, sy);  // both waves of the ring set need all 8 elements
  d5_pair_sync(pcnt, epoch += 2, lane, sy);        // ... and every exchange read is done before the planes are reused
  PXM_D5_TRANSFORM(0)
  PXM_D5_STAMP(3)  // forward transform done
  PXM_D5_TO_STAGE
  PXM_D5_STORE_RINGS(false)
#ifdef PXM_D5_TRACE
  d5_barrier();
  if (threadIdx.x == 0 && g_dft_trace) {
    const unsigned long long slot = atomicAdd(g_dft_trace + 1, 1ull);
    unsigned long long* rr_ = g_dft_trace + 8 + 8 * 4096 + 8 * slot;  // phase records behind the workgroup records
    rr_[0] = R0; rr_[1] = d5_stamp[0] - d5_t0; rr_[2] = d5_stamp[1] - d5_t0; rr_[3] = d5_stamp[2] - d5_t0;
    rr_[4] = d5_stamp[3] - d5_t0; rr_[5] = wall_clock64() - d5_t0; rr_[6] = bx; rr_[7] = by;
  }
#endif
}

}  // namespace pxm
#include "dft_pfa.h"
namespace pxm {

template <int R0>
__global__ __launch_bounds__(128 * D5_RMAX, 4) void k_px2ring5(Dft5Args a, PxIn in, double* __restrict__ G,
                                                                                 int ncol, int C) {
  extern __shared__ double2 lds5[];
  if (in.bump && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *in.bump += 1;
  if constexpr (R0 == 8) {
    if (a.pfa && ncol >= 8) {  // exact-length unit (the launch wrapper sized the grid for it: one ring pair per workgroup)
      const PfaTabs pt{reinterpret_cast<const uint16_t*>(a.pfa + PFA_TAB_GAT), reinterpret_cast<const uint16_t*>(a.pfa + PFA_TAB_KIDX),
                       reinterpret_cast<const double2*>(a.pfa + PFA_TAB_B2)};
      px2ring_body_pfa(a, pt, in, G, ncol, C, blockIdx.x, blockIdx.y, 1, lds5);
      return;
    }
  }
  px2ring_body5<R0>(a, in, G, ncol, C, blockIdx.x, blockIdx.y, lds5);
}

template <int R0, bool RING_OUT, bool N64, bool STOCK = false>
__global__ __launch_bounds__(128 * D5_RMAX, 4) void k_ring2px5(Dft5Args a, double* __restrict__ G, int ncol,
                                                                                 PxOut out, int C) {
  extern __shared__ double2 lds5[];
  if constexpr (R0 == 8) {
    if (a.pfa && ncol >= 8) {
      const PfaTabs pt{reinterpret_cast<const uint16_t*>(a.pfa + PFA_TAB_GAT), reinterpret_cast<const uint16_t*>(a.pfa + PFA_TAB_KIDX),
                       reinterpret_cast<const double2*>(a.pfa + PFA_TAB_B2)};
      ring2px_body_pfa<RING_OUT, N64, STOCK>(a, pt, G, ncol, out, C, blockIdx.x, blockIdx.y, 1, lds5);
      return;
    }
  }
  ring2px_body5<R0, RING_OUT, N64, STOCK>(a, G, ncol, out, C, blockIdx.x, blockIdx.y, lds5);
}

// block id -> (scale entry, bx, by).  XCD-aware order inside a scale: the chain groups (by) of one ring set share
// the 128-B lines of the ring arrays (8 chain slots per (m, ring)), so they are given block ids that differ by 8 --
// same XCD (same L2) under the round-robin placement of blocks, dispatched back to back: the second one finds its
// half-lines in L2 and their half-line stores merge there.  (b0 and the per-scale block counts are multiples of 8.)
// The table pointers of a group entry would be LOADED from the descriptor array: the compiler cannot see their
// address space and emits flat_load for every chirp / filter / twiddle access (162 of them in the fused kernel) --
// flat loads count on lgkmcnt as well as vmcnt, so every s_waitcnt lgkmcnt(0) of the LDS transposes also drained
// the table loads in flight.  The entries therefore carry the tables as offsets (doubles) from the workspace base,
// a kernel argument: pointers derived from it are global and the loads are global_load (like the GEMM's tab_off).
#define PXM_D5_GROUP_DECODE                                              \
  int e = 0;                                                             \
  while (e + 1 < nent && (int)blockIdx.x >= ents[e + 1].b0) ++e;         \
  const Dft5Group g = ents[e];                                           \
  const int local = blockIdx.x - g.b0;                                   \
  const int rest = local >> 3;                                           \
  const int by = rest % g.nby;                                           \
  int bx = (rest / g.nby) * 8 + (local & 7);                             \
  /* narrow ring arrays: the xs ring sets that share a 128-B line go to workgroups of ONE XCD (d6_ring_of_block) */ \
  if (g.xs > 1 && bx < (g.nbx & ~(8 * g.xs - 1))) {                      \
    const int q = rest / g.nby;                                          \
    bx = g.xs * (8 * (q / g.xs) + (local & 7)) + q % g.xs;               \
  }                                                                      \
  if (bx >= g.nbx) return;                                               \
  double* G = ws + g.g_off;                                              \
  Dft5Args a = g.a;                                                      \
  {                                                                      \
    const double* tb = ws + g.tbase;                                     \
    a.cE = reinterpret_cast<const double2*>(tb + g.toff[0]);             \
    a.cO = reinterpret_cast<const double2*>(tb + g.toff[1]);             \
    a.dO = reinterpret_cast<const double2*>(tb + g.toff[2]);             \
    a.tw1 = reinterpret_cast<const double2*>(tb + g.toff[3]);            \
    a.wt = reinterpret_cast<const double2*>(tb + g.toff[4]);             \
    a.bE = reinterpret_cast<const double2*>(tb + g.toff[5]);             \
    a.bO = reinterpret_cast<const double2*>(tb + g.toff[6]);             \
  }

// Grouped launch of the ring-space step: the rings -> X' -> rings bodies (RING_OUT) of EVERY scale of a wavelet plan
// in one grid, largest scales first (their workgroups are the long ones; the small scales fill the tail); without
// RING_OUT the plain rings -> pixels transform of every member scale (generic synthesis / adjoint operators).
#ifdef PXM_D5_TRACE
// development build only: per-workgroup timeline of the grouped launches (see sht_gemm.hip: PXM_GEMM_TRACE)
extern "C" int pxm_debug_set_dft_trace(unsigned long long* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_dft_trace), &buf, sizeof(buf)) == hipSuccess ? 0 : -1;
}
#endif
template <bool RING_OUT, bool N64, bool STOCK = false, int XOUT = MEM_DEFAULT>
__global__ __launch_bounds__(128 * D5_RMAX, 4) void k_ring2px_group5(const Dft5Group* __restrict__ ents, int nent,
                                                                                       double* __restrict__ ws, int ncol, PxOut out,
                                                                                       int C) {
  extern __shared__ double2 lds5[];
#ifdef PXM_D5_TRACE
  const unsigned long long trace_t0 = wall_clock64();
#endif
  PXM_D5_GROUP_DECODE
  out.ring0 = g.ring0;
  if (g.r0 == 9) {  // exact-length unit (the entries of 511-point scales on eight-slot lines: workgroups of that unit)
    const double* pb = ws + g.tbase + g.pfa_off;
    const PfaTabs pt{reinterpret_cast<const uint16_t*>(pb + PFA_TAB_GAT), reinterpret_cast<const uint16_t*>(pb + PFA_TAB_KIDX),
                     reinterpret_cast<const double2*>(pb + PFA_TAB_B2)};
    // (pfa_passes = 2: half as many workgroups, each taking two ring pairs in turn -- with one such workgroup per CU the
    // latency-bound workgroups of the small scales are resident from the start instead of forming a second round)
    ring2px_body_pfa<RING_OUT, N64, STOCK, XOUT>(a, pt, G, ncol, out, C, bx, by, g.pfa_passes, lds5);
  }
  switch (g.r0) {
    case 9: break;  // (done above)
    case 8: ring2px_body5<8, RING_OUT, N64, STOCK, XOUT>(a, G, ncol, out, C, bx, by, lds5); break;
    case 4: ring2px_body5<4, RING_OUT, N64, STOCK, XOUT>(a, G, ncol, out, C, bx, by, lds5); break;
    case 2: ring2px_body5<2, RING_OUT, N64, STOCK, XOUT>(a, G, ncol, out, C, bx, by, lds5); break;
    default: ring2px_body5<1, RING_OUT, N64, STOCK, XOUT>(a, G, ncol, out, C, bx, by, lds5); break;
  }
#ifdef PXM_D5_TRACE
  if (threadIdx.x == 0 && g_dft_trace) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const unsigned long long slot = atomicAdd(g_dft_trace, 1ull);
    unsigned long long* r = g_dft_trace + 8 + 8 * slot;
    r[0] = blockIdx.x; r[1] = gridDim.x; r[2] = trace_t0; r[3] = wall_clock64();
    r[4] = ((unsigned long long)(xcc & 0xf) << 32) | hw; r[5] = g.r0; r[6] = e; r[7] = by;
  }
#endif
}

// pixels -> rings of every member scale in one grid
__global__ __launch_bounds__(128 * D5_RMAX, 4) void k_px2ring_group5(const Dft5Group* __restrict__ ents, int nent,
                                                                                       double* __restrict__ ws, int ncol, PxIn in,
                                                                                       int C) {
  extern __shared__ double2 lds5[];
  if (in.bump && blockIdx.x == 0 && threadIdx.x == 0) *in.bump += 1;
  PXM_D5_GROUP_DECODE
  in.ring0 = g.ring0;
  if (g.r0 == 9) {
    const double* pb = ws + g.tbase + g.pfa_off;
    const PfaTabs pt{reinterpret_cast<const uint16_t*>(pb + PFA_TAB_GAT), reinterpret_cast<const uint16_t*>(pb + PFA_TAB_KIDX),
                     reinterpret_cast<const double2*>(pb + PFA_TAB_B2)};
    px2ring_body_pfa(a, pt, in, G, ncol, C, bx, by, g.pfa_passes, lds5);
    return;
  }
  switch (g.r0) {
    case 8: px2ring_body5<8>(a, in, G, ncol, C, bx, by, lds5); break;
    case 4: px2ring_body5<4>(a, in, G, ncol, C, bx, by, lds5); break;
    case 2: px2ring_body5<2>(a, in, G, ncol, C, bx, by, lds5); break;
    default: px2ring_body5<1>(a, in, G, ncol, C, bx, by, lds5); break;
  }
}

// =============================================================================================================
// Quad unit: four waves per ring for 512 < n <= 1023 (256 < L <= 512), Bluestein at M = 2048 = 4 x 512.
// The chirped input is zero above n < 1024 = 2 x 512, so the first radix-4 (DIF) stage needs two inputs per output:
// wave w takes the bins 4k'+w as the 512-point transform of
//     b_w[j'] = (a[j'] + (-i)^w a[j'+512]) W_2048^(j' w),        j' < 512,
// runs the same 8-points-per-lane convolution core as the pair unit on them (dft_wave.h: d5_conv<8>), and
//     conv[j' + 512 q] = sum_w i^(q w) W_2048^(-j' w) y_w[j'],   q = 0, 1.
// The four waves reduce their weighted shares in two pair exchanges through LDS (w <-> w^1, then w <-> w^2); each
// wave finishes 4 of the 16 elements a lane position covers: p in {pb, pb+1}, pb = 4 (w & 1) + 2 (w >> 1), both
// halves q.  Tables (zero-padded, no j < n tests on the transform path): cA_w = c W^(j'w), cB_w = (-i)^w c[.+512]
// W^(j'w) on input, dA_w = c W^(-j'w), dB_w = i^w c[.+512] W^(-j'w) on output.  scripts/proto_dft5.py: dft_quad.
// =============================================================================================================

struct Dft6Args {
  int L, n, Rp;
  int lgR;                           // log2 of the chains per workgroup (4 waves each)
  const double2 *cA, *cB, *dA, *dB;  // [4][512]
  const double2 *tw1, *wt;           // pass twiddles of the 512-point transform ([8][64], [8][8])
  const double2* bQ;                 // [4][8][64] FFT_2048(filter)/2048 at the bins 4k'+w, pass-3 order
};

#define PXM_D6_GEOMETRY                                                                      \
  constexpr int lgR = LGR, R = 1 << LGR;            /* chains per workgroup: compile-time */ \
  const int n = a.n;                                                                         \
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;                                \
  const int w = wave & 3, r = wave >> 2;            /* bin class of the wave, chain of the workgroup */ \
  const D5Lane q{lane & 7, lane >> 3};                                                       \
  const int t = bx, c0 = by * R, ch = c0 + r;                                                \
  const int Cp = ncol >> 1;                                                                  \
  const int rsh = 4 - lgR;                                                                   \
  const int wa = w & 1, wb = w >> 1;                                                         \
  const int pb = 4 * wa + 2 * wb;                   /* the wave finishes p = pb, pb + 1 (both halves) */ \
  double2* stage = lds5;                                                                     \
  double2* plane = lds5 + wave * D5_PLANE;                                                   \
  const double2* pp1 = lds5 + (wave ^ 1) * D5_PLANE;                                         \
  const double2* pp2 = lds5 + (wave ^ 2) * D5_PLANE;                                         \
  const double2* tw = lds5 + 4 * R * D5_PLANE;                                               \
  for (int i = threadIdx.x; i < D5_TW; i += 256 * R) lds5[4 * R * D5_PLANE + i] = i < 448 ? a.tw1[64 + i] : a.wt[i - 448];
#define PXM_D6_SLOT(K, CH) (((K) << lgR) + (((CH) + ((K) >> rsh)) & (R - 1)))

// xl[p] = element lane + 64 p, xh[p] = element lane + 64 p + 512 of the ring (zeros past n) -> fo[ii][q]: the
// transform at j = lane + 64 (pb + ii) + 512 q.  Three workgroup barriers inside.
__device__ __forceinline__ void d6_transform(double2 (&xl)[8], const double2 (&xh)[8], double2 (&fo)[2][2], double2* plane,
                                             const double2* pp1, const double2* pp2, const double2* tw, int lane,
                                             const D5Lane& q, int w, const Dft6Args& a) {
  const int wa = w & 1, wb = w >> 1;
  const double2* __restrict__ cA = a.cA + w * 512 + lane;
  const double2* __restrict__ cB = a.cB + w * 512 + lane;
  const double2* __restrict__ dA = a.dA + w * 512 + lane;
  const double2* __restrict__ dB = a.dB + w * 512 + lane;
#pragma unroll
  for (int p = 0; p < 8; ++p) xl[p] = cadd(cmul(xl[p], cA[64 * p]), cmul(xh[p], cB[64 * p]));
  d5_conv<8>(xl, plane, lane, q, tw, a.bQ + w * 512);
  // ---- pair exchange 1 (w <-> w ^ 1): keep p in [4 wa, 4 wa + 4), send the shares of the other four
  double2 su[4], sv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double2 yk = d5_sel(wa, xl[4 + i], xl[i]), ys = d5_sel(wa, xl[i], xl[4 + i]);
    const int pk = 64 * (4 * wa + i), ps = 64 * (4 * (1 - wa) + i);
    su[i] = cmul(yk, dA[pk]);
    sv[i] = cmul(yk, dB[pk]);
    plane[64 * i + lane] = cmul(ys, dA[ps]);
    plane[256 + 64 * i + lane] = cmul(ys, dB[ps]);
  }
  d5_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    su[i] = cadd(su[i], pp1[64 * i + lane]);
    sv[i] = cadd(sv[i], pp1[256 + 64 * i + lane]);
  }
  d5_barrier();  // every read of exchange 1 is done before the planes take exchange 2
  // ---- pair exchange 2 (w <-> w ^ 2): keep i in {2 wb, 2 wb + 1}
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    plane[64 * ii + lane] = d5_sel(wb, su[ii], su[2 + ii]);
    plane[128 + 64 * ii + lane] = d5_sel(wb, sv[ii], sv[2 + ii]);
  }
  d5_barrier();
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) {
    fo[ii][0] = cadd(d5_sel(wb, su[2 + ii], su[ii]), pp2[64 * ii + lane]);
    fo[ii][1] = cadd(d5_sel(wb, sv[2 + ii], sv[ii]), pp2[128 + 64 * ii + lane]);
  }
}

// Workgroup -> ring.  On the narrow ring arrays (2 or 4 doubles per (m, ring) entry) eight or four neighbouring rings share a
// 128-B line, and a workgroup reads / writes ONE ring of every order: with ring = block id the eight XCDs (block id mod 8 under
// the round-robin placement) each fetch every line of the array -- 8 x the bytes, 8 us of the 24-us launch at L = 512 -- and
// write it in 16-B pieces from eight L2s.  Here the eight rings of a line go to eight workgroups of ONE XCD that are dispatched
// back to back (block ids 8 q + x, q = 8 j .. 8 j + 7): the line is fetched once and its stores merge in that L2.
__device__ __forceinline__ int d6_ring_of_block(int b, int nb) {
  if (b >= (nb & ~63)) return b;
  const int x = b & 7, q = b >> 3;
  return ((((q >> 3) << 3) + x) << 3) + (q & 7);
}

// LGR: log2 of the chains per workgroup -- 1 (two chains, 8 waves) in general, 0 (4 waves) for a single chain, whose second
// half-workgroup would transform zeros on the same SIMDs
template <int LGR>
__global__ __launch_bounds__(256 << LGR, 4) void k_px2ring6(Dft6Args a, PxIn in, double* __restrict__ G, int ncol, int C) {
  extern __shared__ double2 lds5[];
  if (in.bump && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *in.bump += 1;
  const int bx = d6_ring_of_block(blockIdx.x, gridDim.x), by = blockIdx.y;
  if ((by << LGR) >= C) return;  // no live chain in this group: its slots are zero-filled by the last live group
  PXM_D6_GEOMETRY
  // every wave fetches a quarter of the ring (its two p, both halves) and the four share it through the stage
  {  // batched loads of the wave's four elements (elements past the ring end re-read element 0 of the ring)
    int64_t ev[4];
    bool ok[4];
    double2 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = lane + 64 * (2 * w + (u >> 1)) + 512 * (u & 1);
      ok[u] = ch < C && j < n;
      ev[u] = in.ring0 + (int64_t)t * n + (j < n ? j : 0);
    }
    if (ch < C) px_in_load_n<4>(in, ch, ev, ok, v);
    else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = double2{0.0, 0.0};
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = lane + 64 * (2 * w + (u >> 1)) + 512 * (u & 1);
      if (j < n) stage[PXM_D6_SLOT(j, r)] = v[u];
    }
  }
  d5_barrier();  // (also: the LDS copy of the twiddles is complete)
  double2 xl[8], xh[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int j = lane + 64 * p;
    xl[p] = stage[PXM_D6_SLOT(j, r)];
    xh[p] = (j + 512 < n) ? stage[PXM_D6_SLOT(j + 512, r)] : double2{0.0, 0.0};
  }
  d5_barrier();  // the stage is dead: the planes may be written
  double2 fo[2][2];
  d6_transform(xl, xh, fo, plane, pp1, pp2, tw, lane, q, w, a);
  d5_barrier();  // the planes are dead; the same LDS is the [k][chain] layout-transpose stage
#pragma unroll
  for (int ii = 0; ii < 2; ++ii)
#pragma unroll
    for (int hq = 0; hq < 2; ++hq) {
      const int j = lane + 64 * (pb + ii) + 512 * hq;
      if (j < n) stage[PXM_D6_SLOT(j, r)] = fo[ii][hq];
    }
  d5_barrier();
  {
    const int rr = threadIdx.x & (R - 1), kq = threadIdx.x >> lgR, kstep = 256 /* workgroups of 256 R threads */;
    const int mstride = a.Rp * Cp;
    double2* Gc = reinterpret_cast<double2*>(G) + c0 + rr;
    const bool zf = c0 + R >= C;  // last live chain group: the padding slots of the line are zeroed (whole 128-B lines)
    if (c0 + rr < Cp)
      for (int k = kq; k < n; k += kstep) {
        double2* line = Gc + ((k < a.L) ? k + a.L - 1 : k - a.L) * mstride + t * Cp;
        *line = stage[PXM_D6_SLOT(k, rr)];
        if (zf) for (int z = R; c0 + rr + z < Cp; z += R) line[z] = double2{0.0, 0.0};
      }
  }
}

template <bool N64, int LGR>
__global__ __launch_bounds__(256 << LGR, 4) void k_ring2px6(Dft6Args a, const double* __restrict__ G, int ncol, PxOut out, int C) {
  extern __shared__ double2 lds5[];
  const int bx = d6_ring_of_block(blockIdx.x, gridDim.x), by = blockIdx.y;
  if ((by << LGR) >= C) return;
  PXM_D6_GEOMETRY
  {  // the ring of the workgroup's chains -> stage (conjugated: inverse DFT by conjugation)
    const int rr = threadIdx.x & (R - 1), kq = threadIdx.x >> lgR, kstep = 256 /* workgroups of 256 R threads */;
    const int mstride = a.Rp * Cp;
    const double2* Gc = reinterpret_cast<const double2*>(G) + c0 + rr;
    const bool cv = c0 + rr < Cp;
    constexpr int NB = 4;
    for (int kb = kq; kb < n; kb += NB * kstep) {
      double2 v[NB];
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int k = kb + u * kstep;
        v[u] = double2{0.0, 0.0};
        if (cv && k < n) v[u] = Gc[((k < a.L) ? k + a.L - 1 : k - a.L) * mstride + t * Cp];
      }
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int k = kb + u * kstep;
        if (k < n) stage[PXM_D6_SLOT(k, rr)] = double2{v[u].x, -v[u].y};
      }
    }
  }
  d5_barrier();
  double2 xl[8], xh[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int j = lane + 64 * p;
    xl[p] = stage[PXM_D6_SLOT(j, r)];
    xh[p] = (j + 512 < n) ? stage[PXM_D6_SLOT(j + 512, r)] : double2{0.0, 0.0};
  }
  d5_barrier();
  double2 fo[2][2];
  d6_transform(xl, xh, fo, plane, pp1, pp2, tw, lane, q, w, a);
  if (ch >= C) return;
  const uint64_t it_eff = out.iter + (out.iter_dev ? *out.iter_dev : 0);
  const int64_t e0 = out.ring0 + (int64_t)t * n + lane + 64 * pb;
  const int64_t ce0 = (int64_t)ch * out.chain_stride + e0;
  // the four elements of the lane: loads first (independent), then the arithmetic
  // (unconditional loads behind uniform branches, elements past the ring end re-read the lane's first element: see
  // ring2px_body5 -- one memory latency per batch instead of one per element)
  bool ok[4];
  int64_t eo[4];
  double2 yv[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int ii = u >> 1, hq = u & 1;
    ok[u] = lane + 64 * (pb + ii) + 512 * hq < n;
    eo[u] = ok[u] ? 64 * ii + 512 * hq : 0;  // (the lane's first element, lane + 64 pb < 512 < n, always exists)
    yv[u] = double2{fo[ii][hq].x, -fo[ii][hq].y};
  }
  if (out.X) {  // fused prox + MYULA update (pxmcmc/mcmc.py:185-201, prior.py:49-50)
    double2 xs[4], wn[4];
    double Ts[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xs[u] = reinterpret_cast<const double2*>(out.X)[ce0 + eo[u]];
    if (out.T) {
#pragma unroll
      for (int u = 0; u < 4; ++u) Ts[u] = out.T[e0 + eo[u]];
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) Ts[u] = out.T_scalar;
    }
    if (out.noise) {
#pragma unroll
      for (int u = 0; u < 4; ++u) wn[u] = px_noise_load(out, ch, e0 + eo[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!ok[u]) continue;
      const double2 wv = out.noise ? wn[u] : px_noise_philox_t<N64>(out, ch, e0 + eo[u], it_eff);
      reinterpret_cast<double2*>(out.f)[ce0 + eo[u]] = px_update(out, xs[u], Ts[u], yv[u], wv);
    }
  } else {
    int64_t ev[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ev[u] = e0 + eo[u];
    px_out_store_n<4>(out, ch, ev, yv, ok);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
int pair_r0(int n) {  // 0: no pair unit for this ring length
  if (n > 512) return 0;
  int Mh = 64;
  while (Mh < n) Mh <<= 1;
  return Mh / 64;
}

// Host tables of the exact-length unit (n = 511): idx[(64 + 80) * 8] u16 -- rows 0..63: byte offset 16 k of the element
// k = (73 j1 + 7 g^-q) mod 511, q = CRT72(q8, q9), that lane (j1, q9) = (row / 9, row % 9) holds in register q8 of the S1 layout
// (row 63 idle: zeros); rows 64..136: byte offset 16 k of the output k = CRT511(k1, k2) of instance (row - 64), column k1 < 7,
// k2 = g^CRT72(p8, p9) for instance p9 + 9 p8 and k2 = 0 for instance 72 -- and B2[8][9] = FFT2(b) / 72, b[r] = W_73^(g^r),
// the spectrum of Rader's filter on Z_8 x Z_9.  g = 5 generates (Z / 73)^*.  Checked against scripts/dev/proto_pfa511.py
// by the CPU suite (pxm_host_pfa511_tables).
void pfa511_host_tables(uint16_t* idx, double* b2) {
  typedef std::complex<long double> cld;
  const long double PI_L = 3.141592653589793238462643383279502884L;
  const int n = PFA_N, N2 = 73, g = 5;
  auto ang = [&](long double num, long double den) { return cld(cosl(-PI_L * num / den), sinl(-PI_L * num / den)); };
  auto powm = [&](long long b, int e) { long long r_ = 1; for (int i = 0; i < e; ++i) r_ = r_ * b % N2; return (int)r_; };
  const int ginv = powm(g, 71);  // g^-1 = g^(phi - 1)
  auto crt72 = [](int q8, int q9) { return (9 * q8 + 64 * q9) % 72; };
  std::fill(idx, idx + (size_t)(64 + 80) * 8, (uint16_t)0);
  for (int l = 0; l < 63; ++l)
    for (int q8 = 0; q8 < 8; ++q8) idx[(size_t)l * 8 + q8] = (uint16_t)(16 * ((73 * (l / 9) + 7 * powm(ginv, crt72(q8, l % 9))) % n));
  for (int inst = 0; inst < 73; ++inst) {
    const int k2 = inst < 72 ? powm(g, crt72(inst / 9, inst % 9)) : 0;
    for (int k1 = 0; k1 < 7; ++k1) idx[(size_t)(64 + inst) * 8 + k1] = (uint16_t)(16 * ((365 * k1 + 147 * k2) % n));
  }
  for (int k8 = 0; k8 < 8; ++k8)
    for (int k9 = 0; k9 < 9; ++k9) {
      cld acc(0, 0);
      for (int q8 = 0; q8 < 8; ++q8)
        for (int q9 = 0; q9 < 9; ++q9)
          acc += ang(2.0L * powm(g, crt72(q8, q9)), N2) * ang(2.0L * ((q8 * k8) % 8), 8) * ang(2.0L * ((q9 * k9) % 9), 9);
      acc /= 72.0L;
      b2[2 * (k8 * 9 + k9)] = (double)acc.real();
      b2[2 * (k8 * 9 + k9) + 1] = (double)acc.imag();
    }
}

int pair_make_tables(int n, bool pfa, PairTables* t) {
  typedef std::complex<long double> cld;
  const long double PI_L = 3.141592653589793238462643383279502884L;
  const int r0 = pair_r0(n), Mh = 64 * r0, M = 2 * Mh;
  auto ang = [&](long double num, long double den) { return cld(cosl(-PI_L * num / den), sinl(-PI_L * num / den)); };
  std::vector<cld> chirp, bhat;
  bluestein_chirp_spectrum(n, M, true, chirp, bhat);
  std::vector<double> h;
  auto put = [&](const cld& v) {
    h.push_back((double)v.real());
    h.push_back((double)v.imag());
  };
  const cld zero(0, 0);  // the three chirp tables are zero-padded to Mh entries (the kernels read them without a j < n test)
  const size_t o_cE = 0;
  for (int j = 0; j < Mh; ++j) put(j < n ? chirp[j] : zero);
  const size_t o_cO = h.size();
  for (int j = 0; j < Mh; ++j) put(j < n ? chirp[j] * ang(2.0L * j, M) : zero);
  const size_t o_dO = h.size();
  for (int j = 0; j < Mh; ++j) put(j < n ? chirp[j] * std::conj(ang(2.0L * j, M)) : zero);
  const size_t o_tw1 = h.size();
  for (int k = 0; k < 8; ++k)
    for (int lane = 0; lane < 64; ++lane) {
      const int lam = ((lane & 7) % r0) + r0 * (lane >> 3);
      put(ang(2.0L * ((lam * k) % Mh), Mh));
    }
  const size_t o_wt = h.size();
  for (int a = 0; a < 8; ++a)
    for (int b = 0; b < 8; ++b) put(ang(2.0L * ((a * b) % (8 * r0)), 8 * r0));
  size_t o_b[2];
  for (int w = 0; w < 2; ++w) {
    o_b[w] = h.size();
    for (int k0 = 0; k0 < r0; ++k0)
      for (int lane = 0; lane < 64; ++lane) put(bhat[2 * ((lane >> 3) + 8 * (lane & 7) + 64 * k0) + w]);
  }
  // n = 511: the tables of the exact-length unit (dft_pfa.h, scripts/dev/proto_pfa511.py) behind the Bluestein ones
  size_t o_pfa = 0;
  if (n == PFA_N && pfa) {
    o_pfa = h.size();
    h.resize(h.size() + PFA_TAB_DOUBLES);
    pfa511_host_tables(reinterpret_cast<uint16_t*>(h.data() + o_pfa + PFA_TAB_GAT), h.data() + o_pfa + PFA_TAB_B2);
  }
  t->pfa_off = (int)o_pfa;
  if (int rc = dev_table(&t->d_all, h, "phi-DFT tables (8 points per lane)")) return rc;
  t->r0 = r0;
  t->cE = t->d_all + o_cE;
  t->cO = t->d_all + o_cO;
  t->dO = t->d_all + o_dO;
  t->tw1 = t->d_all + o_tw1;
  t->wt = t->d_all + o_wt;
  t->bE = t->d_all + o_b[0];
  t->bO = t->d_all + o_b[1];
  return 0;
}

// Geometry of the pair unit: D5_RMAX = 4 chains per workgroup (64-B segments of the ring arrays, a compile-time constant of
// the kernels: the index arithmetic of the staging folds) and one ring set per workgroup.  (Until round 3 PXM_DFT_R=1|2
// selected smaller workgroups for A/B runs: 79 / 92 us against 72 for the grouped launch -- fewer waves per barrier do not
// pay for 16 / 32-B segments.)  LDS: the planes of the eight waves, aliased by the stage (8 / r0 rings of n <= 64 r0
// slots x 4 chains), and behind them the LDS copy of the pass twiddles: 8 x 9216 + 8192 = 81 920 B -- exactly two
// workgroups (16 waves, 4 per SIMD) in the 160 KiB of a CU.
constexpr size_t D5_LDS = (size_t)2 * D5_RMAX * D5_PLANE * 16 + (size_t)D5_TW * 16;
static_assert((size_t)512 * D5_RMAX * 16 <= (size_t)2 * D5_RMAX * D5_PLANE * 16, "the stage of a ring set fits in the planes");
// the exact-length body in the same workgroups: 8 planes of PFA_PLANE slots (aliased by the stage of 2 rings x 511 x 4
// slots) + the filter spectrum, the fp64 Box-Muller tables and the group counters: 81 056 B
static_assert(((size_t)8 * PFA_PLANE + 72 + NOISE_LOG_N + 256 + 1) * 16 <= D5_LDS, "PFA workgroup LDS");

void pair_workgroup(int n, bool pfa, int* rings, int* threads, size_t* lds, bool* exact) {
  *exact = n == PFA_N && pfa;
  *rings = *exact ? 2 : 8 / pair_r0(n);  // (pair_ring_blocks on ring arrays of whole lines)
  *threads = 128 * D5_RMAX;
  *lds = D5_LDS;
}

static Dft5Args pair_args(const DftPlan& p) {
  const PairTables& t = p.pair;
  auto c = [](const double* x) { return reinterpret_cast<const double2*>(x); };
  return Dft5Args{p.L, p.n, p.Rp, 2 /* log2 D5_RMAX */, c(t.cE), c(t.cO), c(t.dO), c(t.tw1), c(t.wt), c(t.bE), c(t.bO),
                  p.d_status, p.spin_limit, t.pfa_off ? t.d_all + t.pfa_off : nullptr};
}

template <int R0>
static int pair_attr() {
  static std::atomic<uint64_t> done{0};
  return allow_dynamic_lds(done, {reinterpret_cast<const void*>(k_px2ring5<R0>), reinterpret_cast<const void*>(k_ring2px5<R0, false, false>),
                                  reinterpret_cast<const void*>(k_ring2px5<R0, true, false>), reinterpret_cast<const void*>(k_ring2px5<R0, false, true>),
                                  reinterpret_cast<const void*>(k_ring2px5<R0, true, true>),
                                  reinterpret_cast<const void*>(k_ring2px5<R0, true, true, true>)});
}

// ring sets (workgroups) along the rings: one ring set of 8 / r0 rings each, or a ring pair of the exact-length unit
template <int R0>
static int pair_ring_blocks(const Dft5Args& a, int ncol) {
  const int rings = (R0 == 8 && a.pfa && ncol >= 8) ? 2 : 8 / R0;
  return (a.L + rings - 1) / rings;
}

template <int R0>
static int pair_px2ring_r(const DftPlan& p, const PxIn& in, double* G, int ncol, int C, hipStream_t st) {
  if (int rc = pair_attr<R0>()) return rc;
  const Dft5Args da = pair_args(p);
  dim3 grid(pair_ring_blocks<R0>(da, ncol), (ncol / 2 + D5_RMAX - 1) / D5_RMAX), block(128 * D5_RMAX);
  hipLaunchKernelGGL((k_px2ring5<R0>), grid, block, D5_LDS, st, da, in, G, ncol, C);
  PXM_HIP(hipGetLastError());
  return 0;
}

template <int R0>
static int pair_ring2px_r(const DftPlan& p, const double* G, int ncol, const PxOut& out, int C, hipStream_t st, bool ring_out) {
  if (int rc = pair_attr<R0>()) return rc;
  const Dft5Args da = pair_args(p);
  dim3 grid(pair_ring_blocks<R0>(da, ncol), (C + D5_RMAX - 1) / D5_RMAX), block(128 * D5_RMAX);
  double* Gw = const_cast<double*>(G);
  // (the fp64-noise instantiations only where the launch draws Philox noise in double precision)
  const bool n64 = out.X && !out.noise && out.noise64;
  if (ring_out) {
    // (the stock update of the fp64 stream on the instantiation that holds its mode at compile time)
    if (n64 && p.stock && dft_step_is_stock(out)) hipLaunchKernelGGL((k_ring2px5<R0, true, true, true>), grid, block, D5_LDS, st, da, Gw, ncol, out, C);
    else if (n64) hipLaunchKernelGGL((k_ring2px5<R0, true, true>), grid, block, D5_LDS, st, da, Gw, ncol, out, C);
    else hipLaunchKernelGGL((k_ring2px5<R0, true, false>), grid, block, D5_LDS, st, da, Gw, ncol, out, C);
  } else {
    if (n64) hipLaunchKernelGGL((k_ring2px5<R0, false, true>), grid, block, D5_LDS, st, da, Gw, ncol, out, C);
    else hipLaunchKernelGGL((k_ring2px5<R0, false, false>), grid, block, D5_LDS, st, da, Gw, ncol, out, C);
  }
  PXM_HIP(hipGetLastError());
  return 0;
}

#define PXM_D5_DISPATCH(FN, ...)         \
  switch (p.pair.r0) {                   \
    case 8: return FN<8>(__VA_ARGS__);   \
    case 4: return FN<4>(__VA_ARGS__);   \
    case 2: return FN<2>(__VA_ARGS__);   \
    default: return FN<1>(__VA_ARGS__);  \
  }

int pair_px2ring(const DftPlan& p, const PxIn& in, double* G, int ncol, int C, hipStream_t st) {
  PXM_D5_DISPATCH(pair_px2ring_r, p, in, G, ncol, C, st)
}
int pair_ring2px(const DftPlan& p, const double* G, int ncol, const PxOut& out, int C, hipStream_t st, bool ring_out) {
  PXM_D5_DISPATCH(pair_ring2px_r, p, G, ncol, out, C, st, ring_out)
}

// ---- grouped launch (wavelet plan: every scale in one grid) -----------------------------------------------------
int dft_group_create(const std::vector<const DftPlan*>& plans, const std::vector<int64_t>& g_off,
                     const std::vector<int64_t>& ring0, int ncol, const double* ws_base, DftGroupList* out) {
  // members: the scales on the pair unit (the others keep their own launches); longest workgroups first, the smaller
  // scales fill the tail
  std::vector<int> order;
  for (size_t i = 0; i < plans.size(); ++i)
    if (plans[i]->unit == DFT_PAIR) order.push_back((int)i);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return plans[x]->L > plans[y]->L; });
  if (order.size() < 2) return 1;
  std::vector<Dft5Group> v;
  out->member.assign(plans.size(), 0);
  int b0 = 0;
  // address ranges of a grouped launch (host model of the kernels' global accesses): the ring array of every entry
  // -- rows (m, t) with t < L, all ncol columns: loads of dead rings / padding slots are predicated off or clamped
  // INSIDE the array --, the seven table views and the table block of the exact-length body must each lie inside one
  // registered allocation; the coefficient side (X, T, noise, output: caller-owned, chain_stride elements per chain)
  // is checked against chain_stride at launch (ring_end below: the clamped loads of elements past a ring's end re-read
  // the ring's element 0)
  std::string why;
  int64_t nchk = 0;
  for (int s : order) {
    const DftPlan& p = *plans[s];
    const PairTables& t = p.pair;
    const std::string entry = "DFT group entry " + std::to_string(v.size());
    Dft5Group g;
    g.a = pair_args(p);
    g.g_off = g_off[s];
    g.ring0 = ring0[s];
    g.r0 = t.r0;
    g.tbase = t.d_all - ws_base;
    const double* tp[7] = {t.cE, t.cO, t.dO, t.tw1, t.wt, t.bE, t.bO};
    for (int k = 0; k < 7; ++k) g.toff[k] = (int)(tp[k] - t.d_all);
    const int rings = 8 / t.r0;
    g.nbx = (p.L + rings - 1) / rings;
    g.nby = (ncol / 2 + D5_RMAX - 1) / D5_RMAX;
    {
      const int per_line = 16 / ncol;  // rings per 128-B line: 8 for one complex slot per entry, 4 for two, < 2 otherwise
      g.xs = (g.nby == 1 && per_line > rings && per_line % rings == 0) ? per_line / rings : 1;
    }
    g.pfa_off = 0;
    g.pfa_passes = 1;
    // n = 511 takes the exact-length body (one wave per ring unit: two rings x four chain slots per workgroup, half the
    // workgroups) -- on eight-slot lines only: the narrow arrays of one-chain plans keep the Bluestein body
    if (t.pfa_off && ncol >= 8) {
      ++out->n_pfa;
      g.r0 = 9;
      g.pfa_off = t.pfa_off;
      g.pfa_passes = (getenv("PXM_PFA_PASSES") && atoi(getenv("PXM_PFA_PASSES")) == 1) ? 1 : 2;
      g.nbx = ((p.L + 1) / 2 + g.pfa_passes - 1) / g.pfa_passes;
      g.xs = 1;
    }
    g.b0 = b0;
    b0 += round_up(g.nbx, 8) * g.nby;  // (padded so that every scale starts on an XCD-label boundary)
    out->px_elems += (double)p.L * p.n;
    out->member[s] = 1;
    v.push_back(g);

    const int64_t ring_doubles = (int64_t)(2 * p.L - 1) * p.Rp * ncol;
    ++nchk;
    if (!dev_range_ok(ws_base + g.g_off, ws_base + g.g_off + ring_doubles, &why)) {
      set_error(entry + ": ring array outside its buffer: " + why);
      return -1;
    }
    const int Mh = 64 * t.r0;
    const int64_t tsize[7] = {2 * Mh, 2 * Mh, 2 * Mh, 2 * 8 * 64, 2 * 64, 2 * t.r0 * 64, 2 * t.r0 * 64};
    for (int k = 0; k < 7; ++k) {
      ++nchk;
      const double* tb = ws_base + g.tbase + g.toff[k];
      if (!dev_range_ok(tb, tb + tsize[k], &why)) {
        set_error(entry + ": table view " + std::to_string(k) + " outside its buffer: " + why);
        return -1;
      }
    }
    out->ring_end = std::max(out->ring_end, g.ring0 + (int64_t)p.L * p.n);
    if (g.r0 == 9) {
      ++nchk;
      const double* tb = ws_base + g.tbase + g.pfa_off;
      if (!dev_range_ok(tb, tb + PFA_TAB_DOUBLES, &why)) {
        set_error(entry + ": PFA table block outside its buffer: " + why);
        return -1;
      }
    }
  }
  ranges_checked_add(nchk);
  out->n = (int)v.size();
  out->all = v.size() == plans.size();
  out->blocks = b0;
  out->stock = plans[order[0]]->stock;  // (PXM_DFT_STOCK, read by make_dft_plan: the same for every scale of a plan)
  out->mem_policy = mem_policy_from_env();
  if (int rc = dev_table(&out->d, v, "DFT group entries")) return rc;
  static std::atomic<uint64_t> lds_done{0};
  return allow_dynamic_lds(lds_done, {reinterpret_cast<const void*>(k_ring2px_group5<true, false>), reinterpret_cast<const void*>(k_ring2px_group5<true, true>),
                                      reinterpret_cast<const void*>(k_ring2px_group5<true, true, true>),
                                      reinterpret_cast<const void*>(k_ring2px_group5<true, true, true, DFT_X_OUT_POLICY>),
                                      reinterpret_cast<const void*>(k_ring2px_group5<false, false>), reinterpret_cast<const void*>(k_ring2px_group5<false, true>),
                                      reinterpret_cast<const void*>(k_px2ring_group5)});
}

void dft_group_destroy(DftGroupList* g) {
  if (g->d) deferred_free(g->d);
  g->d = nullptr;
  g->n_pfa = 0;
  g->n = 0;
}

int dft_group_launch(const DftGroupList& g, double* ws, int ncol, const PxOut& out, int C, hipStream_t st, Profiler* prof) {
  // algorithmic bytes: rings read + written (16 B per slot and coefficient, every padded slot), state read, new state
  // written (live slots), thresholds read once
  PXM_REQUIRE(g.ring_end <= out.chain_stride, "dft_group_launch: a scale's coefficient block ends past chain_stride");
  const double bytes = g.px_elems * (2.0 * 16 * (ncol / 2) + 2.0 * 16 * C + (out.T ? 8.0 : 0.0));
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (prof) prof->next(prof->dft, &ev0, &ev1, bytes, 0.0);
  const Dft5Group* ents = reinterpret_cast<const Dft5Group*>(g.d);
  if (g.stock && out.noise64 && dft_step_is_stock(out))  // the stock update: its mode is part of the instantiation
    hipExtLaunchKernelGGL((g.mem_policy ? k_ring2px_group5<true, true, true, DFT_X_OUT_POLICY> : k_ring2px_group5<true, true, true>), dim3(g.blocks), dim3(128 * D5_RMAX), D5_LDS, st, ev0, ev1, 0,
                          ents, g.n, ws, ncol, out, C);
  else if (out.X && !out.noise && out.noise64)
    hipExtLaunchKernelGGL((k_ring2px_group5<true, true>), dim3(g.blocks), dim3(128 * D5_RMAX), D5_LDS, st, ev0, ev1, 0,
                          ents, g.n, ws, ncol, out, C);
  else
    hipExtLaunchKernelGGL((k_ring2px_group5<true, false>), dim3(g.blocks), dim3(128 * D5_RMAX), D5_LDS, st, ev0, ev1, 0,
                          ents, g.n, ws, ncol, out, C);
  PXM_HIP(hipGetLastError());
  return 0;
}

int dft_group_px2ring(const DftGroupList& g, double* ws, int ncol, const PxIn& in, int C, hipStream_t st) {
  PXM_REQUIRE(in.gidx || g.ring_end <= in.chain_stride, "dft_group_px2ring: a scale's coefficient block ends past chain_stride");
  hipLaunchKernelGGL(k_px2ring_group5, dim3(g.blocks), dim3(128 * D5_RMAX), D5_LDS, st, reinterpret_cast<const Dft5Group*>(g.d),
                     g.n, ws, ncol, in, C);
  PXM_HIP(hipGetLastError());
  return 0;
}

int dft_group_ring2px(const DftGroupList& g, double* ws, int ncol, const PxOut& out, int C, hipStream_t st) {
  PXM_REQUIRE(out.gidx || g.ring_end <= out.chain_stride, "dft_group_ring2px: a scale's coefficient block ends past chain_stride");
  const Dft5Group* ents = reinterpret_cast<const Dft5Group*>(g.d);
  if (out.X && !out.noise && out.noise64)
    hipLaunchKernelGGL((k_ring2px_group5<false, true>), dim3(g.blocks), dim3(128 * D5_RMAX), D5_LDS, st, ents, g.n, ws, ncol, out, C);
  else
    hipLaunchKernelGGL((k_ring2px_group5<false, false>), dim3(g.blocks), dim3(128 * D5_RMAX), D5_LDS, st, ents, g.n, ws, ncol, out, C);
  PXM_HIP(hipGetLastError());
  return 0;
}

// ---- host side of the quad unit ----------------------------------------------------------------------------------------------------
int quad_make_tables(int n, QuadTables* t) {
  typedef std::complex<long double> cld;
  const long double PI_L = 3.141592653589793238462643383279502884L;
  const int M = 2048;
  auto ang = [&](long double num, long double den) { return cld(cosl(-PI_L * num / den), sinl(-PI_L * num / den)); };
  std::vector<cld> chirp, bhat;
  bluestein_chirp_spectrum(n, M, true, chirp, bhat);
  chirp.resize(1024, cld(0, 0));
  std::vector<double> h;
  auto put = [&](const cld& v) {
    h.push_back((double)v.real());
    h.push_back((double)v.imag());
  };
  const cld mi(0, -1), pi(0, 1);
  auto ipow = [](cld b, int e) { cld r(1, 0); for (int i = 0; i < e; ++i) r *= b; return r; };
  size_t o[4];
  for (int tab = 0; tab < 4; ++tab) {  // cA, cB, dA, dB: [4][512]
    o[tab] = h.size();
    for (int w = 0; w < 4; ++w)
      for (int j = 0; j < 512; ++j) {
        const cld W = ang(2.0L * ((j * w) % M), M);
        if (tab == 0) put(chirp[j] * W);
        else if (tab == 1) put(ipow(mi, w) * chirp[j + 512] * W);
        else if (tab == 2) put(chirp[j] * std::conj(W));
        else put(ipow(pi, w) * chirp[j + 512] * std::conj(W));
      }
  }
  const size_t o_tw1 = h.size();
  for (int k = 0; k < 8; ++k)
    for (int lane = 0; lane < 64; ++lane) put(ang(2.0L * ((lane * k) % 512), 512));
  const size_t o_wt = h.size();
  for (int x = 0; x < 8; ++x)
    for (int y = 0; y < 8; ++y) put(ang(2.0L * ((x * y) % 64), 64));
  const size_t o_bq = h.size();
  for (int w = 0; w < 4; ++w)
    for (int k0 = 0; k0 < 8; ++k0)
      for (int lane = 0; lane < 64; ++lane) put(bhat[4 * ((lane >> 3) + 8 * (lane & 7) + 64 * k0) + w]);
  if (int rc = dev_table(&t->d_all, h, "phi-DFT tables (four waves per ring)")) return rc;
  t->cA = t->d_all + o[0];
  t->cB = t->d_all + o[1];
  t->dA = t->d_all + o[2];
  t->dB = t->d_all + o[3];
  t->tw1 = t->d_all + o_tw1;
  t->wt = t->d_all + o_wt;
  t->bQ = t->d_all + o_bq;
  return 0;
}

static Dft6Args quad_args(const DftPlan& p) {
  const QuadTables& t = p.quad;
  auto c = [](const double* x) { return reinterpret_cast<const double2*>(x); };
  return Dft6Args{p.L, p.n, p.Rp, 1, c(t.cA), c(t.cB), c(t.dA), c(t.dB), c(t.tw1), c(t.wt), c(t.bQ)};
}
// chains per workgroup: 2 (8 waves, 2 workgroups per CU: 4 waves per SIMD); 1 for a single chain
static size_t quad_lds(int R) { return (size_t)4 * R * D5_PLANE * 16 + (size_t)D5_TW * 16; }  // (>= the stage: n R 16 B)
static int quad_attr() {
  static std::atomic<uint64_t> done{0};
  return allow_dynamic_lds(done, {reinterpret_cast<const void*>(k_px2ring6<0>), reinterpret_cast<const void*>(k_px2ring6<1>),
                                  reinterpret_cast<const void*>(k_ring2px6<false, 0>), reinterpret_cast<const void*>(k_ring2px6<true, 0>),
                                  reinterpret_cast<const void*>(k_ring2px6<false, 1>), reinterpret_cast<const void*>(k_ring2px6<true, 1>)});
}
static int quad_chains_per_wg(int C) { return C == 1 ? 1 : 2; }
void quad_workgroup(int* chains, int* threads, size_t* lds) {
  *chains = quad_chains_per_wg(2);
  *threads = 256 * *chains;
  *lds = quad_lds(*chains);
}
int quad_px2ring(const DftPlan& p, const PxIn& in, double* G, int ncol, int C, hipStream_t st) {
  if (int rc = quad_attr()) return rc;
  const int R = quad_chains_per_wg(C);
  dim3 grid(p.L, (ncol / 2 + R - 1) / R), block(256 * R);
  if (R == 1) hipLaunchKernelGGL(k_px2ring6<0>, grid, block, quad_lds(R), st, quad_args(p), in, G, ncol, C);
  else hipLaunchKernelGGL(k_px2ring6<1>, grid, block, quad_lds(R), st, quad_args(p), in, G, ncol, C);
  PXM_HIP(hipGetLastError());
  return 0;
}
int quad_ring2px(const DftPlan& p, const double* G, int ncol, const PxOut& out, int C, hipStream_t st) {
  if (int rc = quad_attr()) return rc;
  const int R = quad_chains_per_wg(C);
  dim3 grid(p.L, (C + R - 1) / R), block(256 * R);
  const bool n64 = out.X && !out.noise && out.noise64;
  const Dft6Args a = quad_args(p);
  if (R == 1) {
    if (n64) hipLaunchKernelGGL((k_ring2px6<true, 0>), grid, block, quad_lds(R), st, a, G, ncol, out, C);
    else hipLaunchKernelGGL((k_ring2px6<false, 0>), grid, block, quad_lds(R), st, a, G, ncol, out, C);
  } else {
    if (n64) hipLaunchKernelGGL((k_ring2px6<true, 1>), grid, block, quad_lds(R), st, a, G, ncol, out, C);
    else hipLaunchKernelGGL((k_ring2px6<false, 1>), grid, block, quad_lds(R), st, a, G, ncol, out, C);
  }
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // namespace pxm
