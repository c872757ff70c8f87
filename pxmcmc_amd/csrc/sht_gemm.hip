// Legendre ("ring") stage of the MW transforms: per-m real-table x complex-batch GEMMs on
// v_mfma_f64_16x16x4_f64, the host model of the addresses the kernel forms, and the launchers.  (The tables are built in
// sht_tables.hip, the task lists in tasklist.hip.)
//
// Table layout: for every stored m and every tile of 16 output rows the
// contraction index runs in chunks of 8; one chunk is 128 doubles = [lane(64)][2], where
// double h of lane l is T[row = 16*rt + (l & 15)][k = k_beg + 8*kk2 + 4*h + (l >> 4)] -- exactly
// the A-operand fragments of two consecutive MFMAs, so a wave streams its table with one
// coalesced 16-B-per-lane load per two MFMA k-steps and the table never touches LDS.
#include "../../include/pxmcmc_amd.h"
#include "sht_core.h"

#include <type_traits>

#include <hip/hip_ext.h>

#include <algorithm>

namespace pxm {

typedef double d4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------
// GEMM kernel.  One workgroup (4 waves) = one GemmTask = up to 8 row tiles of 16 output rows
// (two per wave) x NCT = CT*NSLAB column tiles of 16 columns:
//     Y[row][col] = sum_k T[row][k] * kscale[k] * X[k][col].
// * the table T streams HBM -> registers in its pre-tiled MFMA A-fragment layout, prefetched two
//   16-k chunks ahead (it is read exactly once per launch and never touches LDS);
// * the operand X (shared by every row tile of the task) is staged once per workgroup through
//   double-buffered LDS with 16-B coalesced loads issued one chunk ahead; the row pitch is
//   = 128 B mod 256 B so the ds_read_b64 B-fragment reads of the two k-rows a 32-lane group
//   touches fall on disjoint bank halves;
// * one barrier per 16-k chunk (32 MFMAs per wave between barriers).
// ---------------------------------------------------------------------------------------
constexpr int KC = 16;  // contraction rows per staged chunk
// NW waves per workgroup, RT row tiles of 16 rows per wave: a task covers NW*RT row tiles.
// NSET: register sets of the table AND operand streams, i.e. both run NSET-1 chunks (of 16 k) ahead (the depth each
// launcher instantiates, and why, is at launch_gemm / launch_gemm_packed below).
#define PXM_GEMM_MFMA(ACC, A, B) ACC = __builtin_amdgcn_mfma_f64_16x16x4f64(A, B, ACC, 0, 0, 0);
#ifdef PXM_GEMM_TRACE
// development build only: per-workgroup timeline (start / end clock, placement, task shape) of every launch into a
// caller-provided buffer [8 words per record], records appended through an atomic cursor in word 0
__device__ unsigned long long* g_gemm_trace = nullptr;
extern "C" int pxm_debug_set_gemm_trace(unsigned long long* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_trace), &buf, sizeof(buf)) == hipSuccess ? 0 : -1;
}
#endif
__device__ __forceinline__ double stage_add(double a, double b, bool on) { return a + (on ? b : 0.0); }
__device__ __forceinline__ double2 stage_add(double2 a, double2 b, bool on) { return double2{a.x + (on ? b.x : 0.0), a.y + (on ? b.y : 0.0)}; }
__device__ __forceinline__ double stage_scale(double a, double sc) { return a * sc; }
__device__ __forceinline__ double2 stage_scale(double2 a, double sc) { return double2{a.x * sc, a.y * sc}; }
// TWO: the tasks of the launch sum a second operand in while staging; SK: they scale the operand per contraction row
// (compile-time, so that the launches without them issue no loads for them)
template <int CT, int NSLAB>
struct GemmGeom {
  static constexpr int NCT = CT * NSLAB;
  static constexpr int COLS = 16 * NCT;                       // staged operand columns
  static constexpr int PITCH = COLS + (COLS == 16 ? 0 : 16);  // doubles; PITCH*8 = 128 (mod 256)
};
// Epilogue operands of a task in LDS (the unpacked kernels): the distinct values its epilogue needs -- per output row the
// complex data term of every slab, the output scale and, in the POLE variant, b of the row -- fetched once per workgroup at
// task start, [hd: NSLAB][ROWS][2] [rs: ROWS] [b_own: ROWS] doubles, ROWS = 16 NW RT
template <int NSLAB, int NW, int RT, bool POLE>
struct GemmEpi {
  static constexpr int ROWS = 16 * NW * RT;
  static constexpr int NHD = 2 * NSLAB * ROWS;
  static constexpr int RS_AT = NHD, B_AT = NHD + ROWS;
  static constexpr int SIZE = NHD + ROWS + (POLE ? ROWS : 0);
};
// PK (packed columns, few-chain plans): 0 = off.  PK = 2 C in {2, 4}: ONE column tile whose 16 columns are up to 16 / PK
// slabs of PK live columns each -- slab s = column / PK reads / writes columns col0 .. col0 + PK - 1 of ITS operand / result
// array (x_off[s] / y_off[s]), slabs 2g, 2g + 1 being the +m / -m slabs of transform g of a task that streams one table
// for up to two transforms (the two L-band-limited wavelet scales).  With one chain the unpacked launch spends two MFMA
// column tiles per table fragment on 4 live columns and streams the 512-table once per scale; packed, one tile carries the
// 8 live columns of both scales: half the table bytes and a quarter of the MFMAs.  Instantiated with CT = NSLAB = 1.
// POLE: the launch has tasks with a pole term (GemmTask::pole_n, the order-0 halves of the split Gram list).  A variant of
// its own, so that every other launch runs the code it ran before.
template <int CT, int NSLAB, int NW, int RT, int NSET, bool TWO, bool SK, int PK = 0, bool POLE = false>
__device__ __forceinline__ void sht_gemm_body(const GemmTask* __restrict__ tasks, const int bid,
                                              const double* __restrict__ X, double* __restrict__ Y, int ncol, int col0,
                                              const GemmAffine& aff, double (*xs)[KC][GemmGeom<CT, NSLAB>::PITCH],
                                              double* __restrict__ es) {
  constexpr int NCT = CT * NSLAB;
  typedef GemmEpi<NSLAB, NW, RT, POLE> Epi;
  constexpr bool EARLY = PK == 0;  // the epilogue operands go through es (the packed kernels load them after the loop)
  // all B-fragment LDS reads of a chunk ahead of its MFMAs (one LDS round trip per chunk instead of four): pays in the
  // Gram launch (1.5 workgroups per CU, nothing else to hide the latency: 22.3 -> 21.8 us), costs 6-10 VGPRs and with
  // them the eighth wave per SIMD in the streaming launches (32.0 -> 32.7 us) -- on for the two-operand variants only
  constexpr bool HOIST = TWO;
  constexpr int COLS = GemmGeom<CT, NSLAB>::COLS;
  constexpr int PITCH = GemmGeom<CT, NSLAB>::PITCH;
  constexpr int NT = 64 * NW;                             // threads per workgroup
  // staging unit: a double2 per thread where the chunk has at least one for everybody, otherwise a double (so that
  // every thread of the workgroup stages the same amount and nobody loads twice)
  constexpr int VW = (KC * COLS / 2 >= NT) ? 2 : 1;       // doubles per staging load
  constexpr int NV = KC * COLS / VW;                      // staging units per chunk
  constexpr int IT = (NV + NT - 1) / NT;                  // staging loads per thread per chunk
  const GemmTask t = tasks[bid];
  const int tid = threadIdx.x, lane = tid & 63;
  if (t.n_rt == 0) return;  // padding entry of the XCD-queue order (tasklist.hip: order_tasks)
  // doubles per operand / result row: the task's own in the packed and the two-operand variants (narrow arrays; the parity
  // halves of the split Gram list walk a plane two rows at a time), the launch's in the streaming variants (HOIST below:
  // their register budget is tight)
  const int xn = (PK || TWO) ? t.x_ncol : ncol, yn = (PK || TWO) ? t.y_ncol : ncol;
#ifdef PXM_GEMM_TRACE
  const unsigned long long trace_t0 = wall_clock64();
  unsigned long long trace_t1 = 0, trace_t2 = 0;
  long long trace_c[5] = {0, 0, 0, 0, 0};  // shader-clock stamps inside one steady-state chunk (chunk 8 of tasks that have it)
#define PXM_GEMM_CSTAMP(K) if (ch == 8) trace_c[K] = clock64();
#else
#define PXM_GEMM_CSTAMP(K)
#endif
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: keeps the row-tile tests scalar
  const int kq = lane >> 4, cl = lane & 15;
  const int n_my = min(RT, max(0, t.n_rt - RT * wave));       // row tiles of this wave
  const int nch = (t.k_end - t.k_beg) / KC;

  // ---- operand staging map: thread -> (row kr, column pair) of the chunk.
  // Every thread issues the SAME number of global loads per chunk, unconditionally (threads beyond the staging range
  // re-read element q mod NV and drop it; a missing second operand / scale vector re-reads the first operand and is
  // masked by a select): the compiler can then count the loads in flight exactly -- with loads behind divergent or
  // data-dependent branches it fell back to s_waitcnt vmcnt(0..2) in the loop and every chunk paid two full memory
  // latencies (one steady-state chunk of the Gram launch: 2 650 cycles, of which 1 330 + 1 170 in those waits).
  const double* sp[IT];   // first operand
  const double* sp2[IT];  // second operand summed in while staging (fused wavelet combine)
  const double* skp[IT];  // per-k operand scale of the thread's slab group
  int so[IT];
  bool sv[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int q0 = tid + NT * i;
    const int q = q0 % NV;
    const int kr = (q / (COLS / VW)) % KC, col = VW * (q % (COLS / VW));
    // (packed: columns of slabs the task does not have re-read slab 0; their products are never stored)
    const int slab = PK ? ((col / (PK ? PK : 1)) < tasks[bid].nslab ? col / (PK ? PK : 1) : 0) : col / (16 * CT);
    const int cin = PK ? col % (PK ? PK : 1) : col % (16 * CT);
    sv[i] = q0 < NV;
    // (per-thread slab: read from the task in memory -- a runtime index into the register copy would push
    // the whole struct into scratch)
    const int64_t xo = tasks[bid].x_off[slab];
    sp[i] = X + xo + col0 + cin + (int64_t)(t.k_beg + kr) * xn;
    sp2[i] = sp[i];
    skp[i] = sp[i];
    if (TWO) {  // a task of a TWO launch without a second operand (x2_off = 0) re-reads the first and adds zero
      const int64_t x2o = tasks[bid].x2_off[slab];
      if (x2o) sp2[i] = sp[i] + (x2o - xo);
    }
    if (SK) {
      const int64_t ks = tasks[bid].ks_off[slab >> 1];
      if (ks) skp[i] = X + ks + t.k_beg + kr;
    }
    so[i] = kr * PITCH + col;
  }
  const bool two = TWO && t.x2_off[0] != 0;
  const bool has_sk = SK && t.ks_off[0] != 0;
  typedef typename std::conditional<VW == 2, double2, double>::type stage_t;
  stage_t st[NSET - 1][IT], st2[NSET - 1][IT];  // operand chunks in flight (register sets, compile-time indices)
  double ssc[NSET - 1][IT];
#define PXM_STAGE_LOAD(SET, CH)                                                                     \
  {                                                                                                 \
    const int cs = min((CH), nch - 1);                                                              \
    _Pragma("unroll") for (int i = 0; i < IT; ++i) {                                                \
      st[SET][i] = *reinterpret_cast<const stage_t*>(sp[i] + (int64_t)cs * KC * xn);                \
      if (TWO) st2[SET][i] = *reinterpret_cast<const stage_t*>(sp2[i] + (int64_t)cs * KC * xn);   \
      if (SK) ssc[SET][i] = skp[i][cs * KC];                                                        \
    }                                                                                               \
  }
#define PXM_STAGE_STORE(SET, BUF)                                                                   \
  _Pragma("unroll") for (int i = 0; i < IT; ++i) {                                                  \
    stage_t v = st[SET][i];                                                                         \
    if (TWO) v = stage_add(v, st2[SET][i], two);                                                    \
    if (SK) {                                                                                       \
      v = stage_scale(v, has_sk ? ssc[SET][i] : 1.0);                                               \
    }                                                                                               \
    if (sv[i]) *reinterpret_cast<stage_t*>(&xs[BUF][0][0] + so[i]) = v;                             \
  }

  // ---- table stream: per row tile two double2 per chunk (k-steps {0,1} and {2,3}).
  // rows this wave does not own alias row tile 0 (valid memory, results discarded); chunk indices are
  // clamped so every load is unconditional: plain global_load_dwordx4, no select, no flat access
  const double2* tab[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
    tab[r] = reinterpret_cast<const double2*>(X + t.tab_off + (int64_t)(n_my > r ? RT * wave + r : 0) * t.rt_stride) + lane;
  const bool v0 = n_my > 0;
  // NSET register sets used round-robin with compile-time indices (no register rotation: a copy of an
  // in-flight load would force a full vmcnt(0) drain every chunk); the table runs NSET-1 chunks ahead
  double2 A[NSET][RT][2];
#define PXM_TAB_LOAD(SET, CH)                                                 \
  {                                                                           \
    const int cc = min((CH), nch - 1);                                        \
    _Pragma("unroll") for (int r = 0; r < RT; ++r) {                          \
      A[SET][r][0] = tab[r][(int64_t)(2 * cc) * 64];                          \
      A[SET][r][1] = tab[r][(int64_t)(2 * cc + 1) * 64];                      \
    }                                                                         \
  }

  // ---- epilogue operands: none of them depends on the contraction, so their loads go out here, ahead of every load of
  // the loop (its exact vmcnt counts keep holding: these are older), one value per thread instead of one per output
  // element -- sixteen column lanes used to load the same scale, eight the same data term, in a memory round trip of
  // its own after the last MFMA, with every workgroup of the launch at that point together.  The values wait in
  // registers until iteration 1 has its operand and go to es there; that iteration's barrier publishes them.  As compiled,
  // they have arrived long before: the wait for the per-thread slab offsets of the staging map (iteration 0, a
  // vmcnt(0) ahead of the first table load) covers them, at a time when the memory system has nothing else to do.
  // Without that wait (slab offsets selected from scalars, these loads in flight with the first table chunk) the three
  // launches measured 0.6 - 0.8 us slower each (docs/EXPERIMENTS.md, round 9).
  // Rows past the task's tiles re-read its row 0 (valid memory; nobody reads those entries).
  constexpr int EIT = (Epi::NHD + NT - 1) / NT;
  double e_hd[EIT], e_rs = 1.0;
  if constexpr (EARLY) {
#pragma unroll
    for (int i = 0; i < EIT; ++i) {
      const int e = (tid + NT * i) % Epi::NHD, sl = e / (2 * Epi::ROWS), rl = (e >> 1) % Epi::ROWS;
      int64_t ho = t.hd_off[0];
#pragma unroll
      for (int s2 = 1; s2 < NSLAB; ++s2) ho = sl == s2 ? t.hd_off[s2] : ho;  // (a select, not a run-time index: see x_off above)
      e_hd[i] = 0.0;
      if (aff.on && ho) e_hd[i] = (X + ho)[(int64_t)(t.row0 + (rl < 16 * t.n_rt ? rl : 0)) * t.hd_stride + (e & 1)];
    }
    if (t.rs_off[0] && tid < Epi::ROWS) e_rs = (X + t.rs_off[0])[t.row0 + (tid < 16 * t.n_rt ? tid : 0)];
  }
  // Pole term of an order-0 half (task-uniform branch): acc[row][col] += 1/2 b_own[row] * s[col] with
  // s[col] = sum_r b_other[r] * x_other[r][col] over the half-rows of the other parity.  Both slabs of order 0 stage
  // the same operand, so s is formed once for the 16 CT columns of slab 0.  Fixed summation order: thread (row
  // group rg, column pair cp) sums rows rg, rg + NRG, ...; a butterfly over the row groups of a wave; the eight
  // waves through LDS in wave order.  The thread's own sum is formed HERE, before the loop -- the operand is what the
  // previous launch wrote -- and b of the task's rows goes to es; the butterfly and the exchange need xs and follow the loop.
  double2 part{0.0, 0.0};
  if constexpr (POLE) {
    if (t.pole_n) {
      constexpr int W2 = 8 * CT;    // column pairs of one slab
      constexpr int NRG = NT / W2;  // row groups of the workgroup
      const int cp = tid % W2, rg = tid / W2;
      const double* xo = X + t.x_off[0] + t.pole_dx + col0 + 2 * cp;
      const double* xo2 = two ? X + t.x2_off[0] + t.pole_dx + col0 + 2 * cp : xo;
      const double* bo = X + t.pole_bo_off;
      double b_own = 0.0;  // (in flight with the operand rows below)
      if (tid < Epi::ROWS) b_own = (X + t.pole_b_off)[t.row0 + (tid < 16 * t.n_rt ? tid : 0)];
#pragma unroll 1  // (two rows per thread at L = 256)
      for (int r = rg; r < t.pole_n; r += NRG) {
        const double2 a = *reinterpret_cast<const double2*>(xo + (int64_t)r * xn);
        const double2 a2 = *reinterpret_cast<const double2*>(xo2 + (int64_t)r * xn);
        const double bv = bo[r];
        const double2 v = stage_add(a, a2, two);
        part.x += bv * v.x;
        part.y += bv * v.y;
      }
      if (tid < Epi::ROWS) es[Epi::B_AT + tid] = b_own;
    }
  }

  d4 acc[RT][NCT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int c = 0; c < NCT; ++c) acc[r][c] = d4{0, 0, 0, 0};

  // One loop, no prologue: iteration it stores chunk it - (NSET-1) to LDS (a dummy store of zeros while that is
  // negative), loads chunk it (operand set it % (NSET-1), table set it % NSET; clamped past the end), passes the
  // barrier and multiplies chunk it - (NSET-1).  Up to the barrier the body is straight-line and identical in every
  // iteration, so the steady-state load counts hold on every path into it and the waits are exact: vmcnt(2) before
  // the LDS store (the two table loads may stay in flight), vmcnt(5+) before the MFMAs.
#pragma unroll
  for (int u = 0; u < NSET - 1; ++u)
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      st[u][i] = st2[u][i] = stage_t{};
      ssc[u][i] = 0.0;
    }
  constexpr int PER = NSET * (NSET - 1);
  const int nit = nch + NSET - 1;
  for (int it0 = 0; it0 < nit; it0 += PER) {
#pragma unroll
    for (int pv = 0; pv < PER; ++pv) {
      const int it = it0 + pv;
      const int ch = it - (NSET - 1);                      // the chunk stored / multiplied in this iteration
      constexpr int LAG = NSET - 1;
      const int us = pv % (NSET - 1);                       // operand set: stored, then reloaded with chunk it
      const int ut = pv % NSET;                             // table set loaded with chunk it
      const int um = (pv + NSET - LAG % NSET) % NSET;       // table set of chunk ch
      const int buf = (pv + PER - LAG) & 1;                 // LDS buffer of chunk ch (PER is even)
      PXM_GEMM_CSTAMP(0)
#ifdef PXM_GEMM_TRACE
      if (ch == 9) trace_c[4] = clock64();
#endif
      PXM_STAGE_STORE(us, buf)
      PXM_GEMM_CSTAMP(1)  // operand of this chunk arrived and went to LDS
      if (EARLY && pv == 1 && it0 == 0) {  // iteration 1 (every task has it): the epilogue operands, loaded before the loop
#pragma unroll
        for (int i = 0; i < EIT; ++i)
          if (tid + NT * i < Epi::NHD) es[tid + NT * i] = e_hd[i];
        if (tid < Epi::ROWS) es[Epi::RS_AT + tid] = e_rs;
      }
      PXM_STAGE_LOAD(us, it)
      PXM_TAB_LOAD(ut, it)
      __syncthreads();
#ifdef PXM_GEMM_TRACE
      if (ch == 0) trace_t1 = wall_clock64();  // first chunk staged: task fetch + first operand loads are behind us
#endif
      PXM_GEMM_CSTAMP(2)  // barrier passed
      if (v0 && ch >= 0 && ch < nch) {
#define PXM_MFMA_CHUNK(NC)                                                                                     \
  {                                                                                                            \
    double b[4][NC]; /* all B fragments of the chunk first: one LDS round trip instead of one per k-step */    \
    _Pragma("unroll") for (int h4 = 0; h4 < 4; ++h4)                                                           \
      _Pragma("unroll") for (int c = 0; c < NC; ++c) b[h4][c] = xs[buf][4 * h4 + kq][16 * c + cl];             \
    if (HOIST) __builtin_amdgcn_sched_barrier(0); /* (otherwise the scheduler sinks the reads between the MFMAs) */ \
    _Pragma("unroll") for (int h4 = 0; h4 < 4; ++h4)                                                           \
      _Pragma("unroll") for (int r = 0; r < RT; ++r) {                                                         \
        const double av = (h4 & 1) ? A[um][r][h4 >> 1].y : A[um][r][h4 >> 1].x;                                \
        _Pragma("unroll") for (int c = 0; c < NC; ++c)                                                         \
            PXM_GEMM_MFMA(acc[r][c], av, b[h4][c])                                                             \
      }                                                                                                        \
  }
        PXM_MFMA_CHUNK(NCT)
#undef PXM_MFMA_CHUNK
      }
      PXM_GEMM_CSTAMP(3)  // MFMAs of the chunk issued (table fragment of this chunk had to be there)
    }
  }
#undef PXM_STAGE_LOAD
#undef PXM_STAGE_STORE
#undef PXM_TAB_LOAD
#ifdef PXM_GEMM_TRACE
  trace_t2 = wall_clock64();  // contraction done (the last MFMAs may still be in flight)
#endif

  // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg.
  // Epilogue operands first -- the per-row data term of the Gram step and the per-row scale of the fused combine: LDS
  // reads of what the task fetched at its start (packed kernels: global loads, ALL in flight together), then the
  // arithmetic and the stores.
  constexpr int NGRP = PK ? 2 : 1;  // slab groups (transforms) per task: one, or up to two in packed lists
  double hdv[RT][NSLAB][4], rsv[RT][NGRP][4];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const int rl = 16 * (r < n_my ? RT * wave + r : 0) + kq;  // (a tile this wave does not own: the task's tile 0 -- valid rows, values discarded)
    const int rowb = t.row0 + rl;
    if constexpr (EARLY) {
#pragma unroll
      for (int sl = 0; sl < NSLAB; ++sl)
#pragma unroll
        for (int q = 0; q < 4; ++q) hdv[r][sl][q] = es[2 * (sl * Epi::ROWS + rl + 4 * q) + (cl & 1)];
#pragma unroll
      for (int q = 0; q < 4; ++q) rsv[r][0][q] = es[Epi::RS_AT + rl + 4 * q];
    } else {
#pragma unroll
      for (int g = 0; g < NGRP; ++g)
#pragma unroll
        for (int q = 0; q < 4; ++q) rsv[r][g][q] = t.rs_off[g] ? (X + t.rs_off[g])[rowb + 4 * q] : 1.0;
    }
  }
  if constexpr (POLE) {
    if (t.pole_n) {  // the thread's sum `part` was formed before the loop
      constexpr int W2 = 8 * CT;    // column pairs of one slab
      double bown[RT][4];
#pragma unroll
      for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) bown[r][q] = es[Epi::B_AT + 16 * (r < n_my ? RT * wave + r : 0) + kq + 4 * q];
#pragma unroll
      for (int msk = W2; msk < 64; msk <<= 1) {
        part.x += __shfl_xor(part.x, msk);
        part.y += __shfl_xor(part.y, msk);
      }
      double* red = &xs[0][0][0];  // [NW][2 W2], over the operand buffers: nobody may still be reading the last chunk
      __syncthreads();
      if (lane < W2) *reinterpret_cast<double2*>(red + wave * 2 * W2 + 2 * lane) = part;
      __syncthreads();
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        double sc = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) sc += red[w * 2 * W2 + 16 * ct + cl];
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
          for (int sl = 0; sl < NSLAB; ++sl)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[r][sl * CT + ct][q] += 0.5 * bown[r][q] * sc;
      }
    }
  }
  if constexpr (PK != 0) {
    // packed tile: this lane's column cl belongs to slab cl / PK (dead beyond the task's slabs), column cl % PK of its array
    const int slab = cl / PK, grp = slab >> 1;
    const bool live = slab < t.nslab;
    const double sgn = (slab & 1) ? t.sign1 : 1.0;
    const int64_t yo = tasks[bid].y_off[live ? slab : 0];  // (from memory: a run-time index into the register copy would spill it)
    const int row_lo = grp ? t.row_lo[1] : t.row_lo[0], row_hi = grp ? t.row_hi[1] : t.row_hi[0];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      if (r >= n_my) continue;
      const int rowb = t.row0 + 16 * (RT * wave + r) + kq;
      double* yb = Y + yo + col0 + (cl % PK) + (int64_t)rowb * yn;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = rowb + 4 * q;
        const double rs = grp ? rsv[r][NGRP - 1][q] : rsv[r][0][q];
        if (live && row >= row_lo && row < row_hi) yb[(int64_t)(4 * q) * yn] = sgn * rs * acc[r][0][q];
      }
    }
  } else {
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    if (r >= n_my) continue;
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
      const int slab = c / CT, cin = 16 * (c % CT), grp = slab >> 1;
      const double sgn = (slab & 1) ? t.sign1 : 1.0;
      const int rowb = t.row0 + 16 * (RT * wave + r) + kq;
      double* yb = Y + t.y_off[slab] + col0 + cin + cl + (int64_t)rowb * yn;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = rowb + 4 * q;
        double v = acc[r][c][q];
        if (aff.on) {  // out = w * (ns * acc - hd[row]), complex per chain: (re, im) sit in adjacent lanes
          const double u = aff.ns * v - hdv[r][slab][q];
          int lo = __double2loint(u), hi = __double2hiint(u);
          lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]: partner lane
          hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true);
          const double pu = __hiloint2double(hi, lo);
          v = (cl & 1) ? (aff.wr * u + aff.wi * pu) : (aff.wr * u - aff.wi * pu);
          if (col0 + cin + cl >= aff.ncol_live) v = 0.0;  // padding chains stay at zero (they have no prox / damping)
        }
        if (row >= t.row_lo[grp] && row < t.row_hi[grp]) yb[(int64_t)(4 * q) * yn] = sgn * rsv[r][grp][q] * v;
      }
    }
  }
  }
#ifdef PXM_GEMM_TRACE
  __syncthreads();
  if (tid == 0 && g_gemm_trace) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const unsigned long long slot = atomicAdd(g_gemm_trace, 1ull);
    unsigned long long* r = g_gemm_trace + 8 + 8 * slot;
    r[0] = blockIdx.x; r[1] = gridDim.x; r[2] = trace_t0; r[3] = wall_clock64();
    r[4] = ((unsigned long long)(xcc & 0xf) << 32) | hw; r[5] = (unsigned long long)nch | ((unsigned long long)t.n_rt << 16) | ((unsigned long long)aff.on << 32);
    r[6] = trace_t1; r[7] = trace_t2;
    if (nch > 9) {  // second record: the chunk-8 stamps (cycles): stage store done, barrier passed, MFMAs issued, next chunk's top
      const unsigned long long s2 = atomicAdd(g_gemm_trace + 1, 1ull);
      unsigned long long* q = g_gemm_trace + 8 + 8 * 8192 + 8 * s2;
      q[0] = nch; q[1] = trace_c[1] - trace_c[0]; q[2] = trace_c[2] - trace_c[1]; q[3] = trace_c[3] - trace_c[2];
      q[4] = trace_c[4] - trace_c[3]; q[5] = aff.on; q[6] = gridDim.x; q[7] = 0;
    }
  }
#endif
}

template <int CT, int NSLAB, int NW, int RT, int NSET, bool TWO, bool SK, bool POLE = false>
__global__ __launch_bounds__(64 * NW) void k_sht_gemm(const GemmTask* __restrict__ tasks,
                                                      const double* __restrict__ X, double* __restrict__ Y,
                                                      int ncol, int col0, GemmAffine aff) {
  __shared__ double xs[2][KC][GemmGeom<CT, NSLAB>::PITCH];
  __shared__ double es[GemmEpi<NSLAB, NW, RT, POLE>::SIZE];
  static_assert(!POLE || 2 * KC * GemmGeom<CT, NSLAB>::PITCH >= NW * 16 * CT, "the pole reduction borrows the operand buffers");
  if (aff.bump && blockIdx.x == 0 && threadIdx.x == 0) *aff.bump += 1;  // Philox iteration counter of the ring-space step
  sht_gemm_body<CT, NSLAB, NW, RT, NSET, TWO, SK, 0, POLE>(tasks, blockIdx.x, X, Y, ncol, col0, aff, xs, es);
}
// packed column tile (few-chain plans): PK live columns per slab, up to 16 / PK slabs in the one tile
template <int PK, int NW, int RT, int NSET, bool TWO, bool SK>
__global__ __launch_bounds__(64 * NW) void k_sht_gemm_pk(const GemmTask* __restrict__ tasks, const double* __restrict__ X,
                                                         double* __restrict__ Y, int ncol, int col0, GemmAffine aff) {
  __shared__ double xs[2][KC][GemmGeom<1, 1>::PITCH];
  sht_gemm_body<1, 1, NW, RT, NSET, TWO, SK, PK>(tasks, blockIdx.x, X, Y, ncol, col0, aff, xs, nullptr);
}

// ---------------------------------------------------------------------------------------
// Host model of the addresses k_sht_gemm forms.  KEEP IN STEP WITH THE KERNEL ABOVE: every global load and store of
// the kernel has one line here, including the loads whose values are discarded (clamped chunk indices past the end
// of a task, row tiles a wave does not own aliased to tile 0, a missing second operand / scale aliased to the
// first operand).  Such a load faulted in round 2 (commit 0808422: the batched epilogue read the per-row scale of
// tiles the wave did not own, past the end of the vector); a host check of task SHAPES could not see it, this
// check of address RANGES does, without a GPU.  For every task and every column group run_tasks can launch, each
// range must lie inside ONE registered device allocation (common.h: dev_alloc / dev_range_ok).
// ---------------------------------------------------------------------------------------
int check_gemm_task_ranges(const std::vector<GemmTask>& v, int nslab, int pk, int flags, int ncol, const double* ws_base,
                           const char* list_name) {
  int64_t n = 0;
  std::string why;
  auto bad = [&](size_t ti, const char* what, int col0) {
    set_error(std::string("GEMM task address range outside its buffer: list '") + list_name + "', task " + std::to_string(ti) +
              ", column group " + std::to_string(col0) + ", " + what + ": " + why);
    return -1;
  };
  // [lo, hi] in doubles relative to the workspace base (the kernel's X / Y argument)
  auto ok = [&](int64_t lo, int64_t hi) {
    ++n;
    return lo <= hi && dev_range_ok(ws_base + lo, ws_base + hi + 1, &why);
  };
  const bool TWO = flags & GEMM_LIST_TWO, SK = flags & GEMM_LIST_SCALE;
  for (size_t ti = 0; ti < v.size(); ++ti) {
    const GemmTask& t = v[ti];
    if (t.n_rt == 0) continue;  // padding entry: the workgroup exits before forming any address
    const int nch = (t.k_end - t.k_beg) / KC;
    // table stream: tab[r] + (2 cc + {0, 1}) * 64 double2, cc <= nch - 1, row tile <= n_rt - 1 (others alias tile 0),
    // lane < 64, two doubles each
    if (!ok(t.tab_off, t.tab_off + (int64_t)(t.n_rt - 1) * t.rt_stride + (int64_t)(2 * (nch - 1) + 1) * 128 + 127))
      return bad(ti, "ring-table stream", 0);
    for (int col0 = 0; col0 < ncol && t.pole_n; col0 += GEMM_GROUP_COLS) {
      // pole term: b of the task's own rows (one cooperative load at task start, as the per-row scale below), b of the other parity's pole_n
      // half-rows, and the 16 CT columns of slab 0 of the other parity's operand(s), rows 0 .. pole_n - 1 at the task's pitch
      const int CT = gemm_group_tiles(ncol, col0);
      if (!ok(t.pole_b_off + t.row0, t.pole_b_off + t.row0 + 16 * t.n_rt - 1)) return bad(ti, "pole column of the task's rows", col0);
      if (!ok(t.pole_bo_off, t.pole_bo_off + t.pole_n - 1)) return bad(ti, "pole column of the other parity", col0);
      const int64_t lo = t.pole_dx + col0, hi = t.pole_dx + col0 + 16 * CT - 1 + (int64_t)(t.pole_n - 1) * t.x_ncol;
      if (!ok(t.x_off[0] + lo, t.x_off[0] + hi)) return bad(ti, "pole term operand", col0);
      if (t.x2_off[0] && !ok(t.x2_off[0] + lo, t.x2_off[0] + hi)) return bad(ti, "pole term second operand", col0);
    }
    for (int col0 = 0; col0 < ncol; col0 += GEMM_GROUP_COLS) {
      const int CT = gemm_group_tiles(ncol, col0);
      for (int slab = 0; slab < nslab; ++slab) {
        // operand staging: X + x_off[slab] + col0 + cin + (k_beg + kr + cs KC) xn, cin < 16 CT, kr < KC, cs <= nch - 1
        // (xn, yn: the task's own row pitch in the packed and two-operand kernels, the launch's ncol in the streaming
        // ones -- upload_tasks holds the tasks of a streaming list to the launch's ncol)
        const int xn = ((TWO || pk) && t.x_ncol) ? t.x_ncol : ncol, yn = ((TWO || pk) && t.y_ncol) ? t.y_ncol : ncol;
        const int wx = std::min(16 * CT, xn), wy = std::min(16 * CT, yn);  // (a narrow array has fewer than 16 columns per row)
        const int64_t lo = col0 + (int64_t)t.k_beg * xn, hi = col0 + wx - 1 + (int64_t)(t.k_end - 1) * xn;
        if (!ok(t.x_off[slab] + lo, t.x_off[slab] + hi)) return bad(ti, "operand staging", col0);
        if (TWO && t.x2_off[slab] && !ok(t.x2_off[slab] + lo, t.x2_off[slab] + hi)) return bad(ti, "second operand staging", col0);
        // per-k operand scale: X + ks_off[slab >> 1] + k_beg + kr + cs KC
        if (SK && t.ks_off[slab >> 1] && !ok(t.ks_off[slab >> 1] + t.k_beg, t.ks_off[slab >> 1] + t.k_end - 1))
          return bad(ti, "operand scale vector", col0);
        // epilogue operands.  Unpacked kernels: one cooperative load at task start, thread -> row row0 + rl of the task,
        // rl < 16 n_rt (threads past the task's tiles re-read its row 0) -- every row of the task, contiguous.  Packed
        // kernels: after the loop, rows row0 + 16 tile + kq + 4 q, tile <= n_rt - 1 (a tile the wave does not own: tile 0).
        // The same range either way.
        const int64_t r_lo = t.row0, r_hi = t.row0 + 16 * t.n_rt - 1;
        // affine constants: (X + hd_off[slab])[(row) hd_stride + {0, 1}]
        if (t.hd_off[slab] && !ok(t.hd_off[slab] + r_lo * t.hd_stride, t.hd_off[slab] + r_hi * t.hd_stride + 1))
          return bad(ti, "affine data term", col0);
        if (t.rs_off[slab >> 1] && !ok(t.rs_off[slab >> 1] + r_lo, t.rs_off[slab >> 1] + r_hi))
          return bad(ti, "per-row output scale", col0);
        // stores: Y + y_off[slab] + col0 + cin + cl + row yn for the owned rows inside [row_lo, row_hi)
        const int64_t s_lo = std::max<int64_t>(r_lo, t.row_lo[slab >> 1]), s_hi = std::min<int64_t>(r_hi, (int64_t)t.row_hi[slab >> 1] - 1);
        if (s_lo <= s_hi && !ok(t.y_off[slab] + col0 + s_lo * yn, t.y_off[slab] + col0 + wy - 1 + s_hi * yn))
          return bad(ti, "result rows", col0);
      }
    }
  }
  ranges_checked_add(n);
  return 0;
}

// ---------------------------------------------------------------------------------------
// Launchers.  Workgroup geometry: NW waves x RT row tiles per wave cover the row tiles of a task (sht_core.h).
// ---------------------------------------------------------------------------------------
constexpr int NW = 8, RT = 1;
static_assert(NW * RT == GEMM_TASK_ROW_TILES, "a workgroup covers the row tiles of one task");

// calls f(two, sk): the flags GEMM_LIST_TWO / GEMM_LIST_SCALE of a list as std::bool_constant, i.e. the TWO / SK kernel variant
template <class F>
static void with_gemm_variant(int flags, F f) {
  switch (flags & (GEMM_LIST_TWO | GEMM_LIST_SCALE)) {
    case 0: f(std::false_type(), std::false_type()); break;
    case GEMM_LIST_TWO: f(std::true_type(), std::false_type()); break;
    case GEMM_LIST_SCALE: f(std::false_type(), std::true_type()); break;
    default: f(std::true_type(), std::true_type()); break;
  }
}

// flags: GemmListFlag bits of the list
int launch_gemm(const GemmTask* d_tasks, int n_tasks, int nslab, int flags, const double* X, double* Y, int ncol,
                int col0, int ct, double alg_bytes, double flops, hipStream_t stream, const GemmAffine& aff, Profiler* prof) {
  if (n_tasks == 0) return 0;
  PXM_REQUIRE(nslab == 1 || nslab == 2, "launch_gemm: nslab must be 1 (unpaired tables) or 2 (+-m pairs)");
  dim3 grid(n_tasks), block(64 * NW);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (prof) prof->next(prof->gemm, &ev0, &ev1, alg_bytes, flops, n_tasks);
  // look-ahead NSET = 2 (one chunk ahead) on every launch: occupancy hides the load latency (60 VGPR at 16 columns,
  // 4 workgroups per CU); 3 / 4 sets measured 10-15 % slower on the grouped launches, and 4 % / 16 % slower on the
  // Gram launch too (its short tasks re-read their last chunk in the deeper prologue, its long chains are not what
  // bounds it)
  constexpr int NSET = 2;
  auto go = [&](auto kernel) { hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, ev0, ev1, 0, d_tasks, X, Y, ncol, col0, aff); };
  if (flags & GEMM_LIST_POLE) {
    PXM_REQUIRE(nslab == 2 && (flags & (GEMM_LIST_TWO | GEMM_LIST_SCALE)) == GEMM_LIST_TWO, "launch_gemm: a pole term outside the Gram list");
    if (ct == 1) go(k_sht_gemm<1, 2, NW, RT, NSET, true, false, true>);
    else go(k_sht_gemm<2, 2, NW, RT, NSET, true, false, true>);
  } else {
    with_gemm_variant(flags, [&](auto two, auto sk) {
      constexpr bool TWO = decltype(two)::value, SK = decltype(sk)::value;
      if (nslab == 2) {
        if (ct == 1) go(k_sht_gemm<1, 2, NW, RT, NSET, TWO, SK>);
        else go(k_sht_gemm<2, 2, NW, RT, NSET, TWO, SK>);
      } else {
        if (ct == 1) go(k_sht_gemm<1, 1, NW, RT, NSET, TWO, SK>);
        else go(k_sht_gemm<2, 1, NW, RT, NSET, TWO, SK>);
      }
    });
  }
  PXM_HIP(hipGetLastError());
  return 0;
}

// packed launch (pk = live columns per slab: 2 or 4); tasks carry up to 4 slabs
int launch_gemm_packed(const GemmTask* d_tasks, int n_tasks, int pk, int flags, const double* X, double* Y, int ncol, int col0,
                       double alg_bytes, double flops, hipStream_t stream, Profiler* prof) {
  if (n_tasks == 0) return 0;
  PXM_REQUIRE(pk == 2 || pk == 4, "launch_gemm_packed: 2 or 4 live columns per slab");
  dim3 grid(n_tasks), block(64 * NW);
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (prof) prof->next(prof->gemm, &ev0, &ev1, alg_bytes, flops, n_tasks);
  GemmAffine aff;
  // look-ahead NSET = 3 (two chunks ahead).  The packed launches carry a quarter of the MFMA work per table byte of the
  // 16-columns-per-slab ones and 44 - 54 VGPRs: with one chunk of look-ahead their waves spent half their cycles in
  // s_waitcnt (SQ_WAIT_INST_ANY 425 M of 825 M wave-cycles, 2.5 TB/s)
  constexpr int NSET = 3;
  with_gemm_variant(flags, [&](auto two, auto sk) {
    constexpr bool TWO = decltype(two)::value, SK = decltype(sk)::value;
    auto go = [&](auto kernel) { hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, ev0, ev1, 0, d_tasks, X, Y, ncol, col0, aff); };
    if (pk == 2) go(k_sht_gemm_pk<2, NW, RT, NSET, TWO, SK>);
    else go(k_sht_gemm_pk<4, NW, RT, NSET, TWO, SK>);
  });
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // namespace pxm
