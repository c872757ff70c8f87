// Exact-length phi-DFT for ring length n = 511 = 7 x 73 (bandlimit 256), one wave per ring -- device side: the transform
// core and the ring bodies the pair unit's kernels dispatch to.  Included by dft_wave.hip behind Dft5Args and the trace
// stamps; the in-register radix-2 modules (dft8r) and the wave / group synchronisation come from dft_wave.h.
//
// The Bluestein body of the pair unit pads a ring to M = 1024 and spends a wave PAIR on it (2 x 552 fp64 operations per lane,
// 128 lanes).  511 = 7 x 73 has an exact-length factorisation whose lane / register-exact numpy model, operation count and
// LDS count are scripts/dev/proto_pfa511.py (484 operations per lane on 64 lanes: 0.44 x; LDS pipe cycles 0.74 x):
//
//   511 = 7 x 73   Good-Thomas: input j = (73 j1 + 7 j2) mod 511, output k = CRT(k1, k2) -- a plain 7 x 73 two-dimensional DFT
//   73 points      Rader: j2 = g^-q, k2 = g^p (g = 5) -> 72-point cyclic convolution with b[r] = W_73^(g^r)
//   72 = 8 x 9     Z_72 = Z_8 x Z_9: the convolution is diagonalised by the 8 x 9 two-dimensional DFT (radix-2 8-point and
//                  3 x 3 9-point transforms in registers), filter spectrum B2[k8][k9] = FFT2(b) / 72 (72 constants)
//   7 points       direct symmetric form (pair sums / differences, real 3 x 3 products by FMA)
//
// Layouts of a wave (every transpose through its own LDS plane, 16-B slots):
//   S1  lane (j1, q9) = (lane / 9, lane % 9), lanes < 63, regs q8     FFT8  q8 -> k8
//   T2  plane[j1 * 72 + k8 * 9 + q9]   ->  lane (j1, k8) = (lane / 8, lane % 8), lanes < 56, regs q9
//   S2  DFT9 q9 -> k9, x B2[k8][k9], + x0 at bin (0, 0), inverse DFT9 -> p9;   Y0[j1] = x0[j1] + A[0][0]  (the k2 = 0 output)
//   T3  the same array back          ->  lane (j1, p9), regs k8;   Y0[j1] parked at slot 504 + j1
//   S3  inverse FFT8 k8 -> p8:  Y[j1][k2 = g^CRT72(p8, p9)]
//   T4  plane[(p9 + 9 p8) * 7 + j1]   ->  lane = instance (two passes: instances 0..63, 64..72 on lanes 0..8), regs j1
//   S4  DFT7 j1 -> k1:  y[k], k = CRT511(k1, k2(instance))
// The element j2 = 0 of every j1 (seven per ring) never enters the convolution: lane (j1, k8 = 0) of S2 reads it where it
// gathers its inputs and applies both Rader corrections.
#pragma once
#include "dft_wave.h"

namespace pxm {

constexpr int PFA_N = 511;
constexpr int PFA_PLANE = 576;   // 16-B slots of one wave's plane: 511 (T4 / natural order) + slack; = D5_PLANE
constexpr int PFA_Y0 = 504;      // slots of Y0[j1]: instance 72 of the T4 array, free while the T2 / T3 array [0, 504) is live
constexpr int PFA_TAB_GAT = 0;   // table block (in doubles from its base): gat16 [64][8] u16 ...
constexpr int PFA_TAB_KIDX = 128;  // ... kidx16 [80][8] u16 ...
constexpr int PFA_TAB_B2 = 288;    // ... B2 [8][9] complex
constexpr int PFA_TAB_DOUBLES = 288 + 144;

// X0, X1, X2 of (a, b, c), kernel exp(SGN 2 pi i jk / 3): 12 operations
template <int SGN>
__device__ __forceinline__ void pfa_dft3(double2& a, double2& b, double2& c) {
  constexpr double C3 = 0.86602540378443864676 * (SGN > 0 ? 1.0 : -1.0);
  const double2 s = cadd(b, c), d = csub(b, c);
  const double2 m{fma(s.x, -0.5, a.x), fma(s.y, -0.5, a.y)};
  a = cadd(a, s);
  // X1 = m + SGN i (sqrt3 / 2) d,  X2 = m - SGN i (sqrt3 / 2) d
  b = double2{fma(-C3, d.y, m.x), fma(C3, d.x, m.y)};
  c = double2{fma(C3, d.y, m.x), fma(-C3, d.x, m.y)};
}

// 9-point DFT in registers, natural order in and out: 3 x 3 Cooley-Tukey, j = 3 a + b, k = c + 3 d (6 x 12 + 4 x 4 = 88 operations)
template <int SGN>
__device__ __forceinline__ void pfa_dft9(double2 (&x)[9]) {
  constexpr double S = SGN > 0 ? 1.0 : -1.0;
  constexpr double2 W1{0.76604444311897803520, S * 0.64278760968653932632};    // exp(SGN 2 pi i / 9)
  constexpr double2 W2{0.17364817766693034885, S * 0.98480775301220805937};    // ^2
  constexpr double2 W4{-0.93969262078590838405, S * 0.34202014332566873304};   // ^4
  pfa_dft3<SGN>(x[0], x[3], x[6]);  // over a for b = 0, 1, 2: x[3 c + b] = column b, output c
  pfa_dft3<SGN>(x[1], x[4], x[7]);
  pfa_dft3<SGN>(x[2], x[5], x[8]);
  x[4] = cmul(x[4], W1);
  x[5] = cmul(x[5], W2);
  x[7] = cmul(x[7], W2);
  x[8] = cmul(x[8], W4);
  pfa_dft3<SGN>(x[0], x[1], x[2]);  // over b for c = 0, 1, 2: x[3 c + d] = X[c + 3 d]
  pfa_dft3<SGN>(x[3], x[4], x[5]);
  pfa_dft3<SGN>(x[6], x[7], x[8]);
  d5_swap(x[1], x[3]);              // 3 x 3 transpose (compile-time register renaming)
  d5_swap(x[2], x[6]);
  d5_swap(x[5], x[7]);
}

// 7-point DFT in registers, natural order in and out: 66 operations
template <int SGN>
__device__ __forceinline__ void pfa_dft7(double2 (&x)[7]) {
  constexpr double c1 = 0.62348980185873353053, c2 = -0.22252093395631440429, c3 = -0.90096886790241912624;
  constexpr double s1 = 0.78183148246802980871, s2 = 0.97492791218182360702, s3 = 0.43388373911755812048;
  const double2 p1 = cadd(x[1], x[6]), p2 = cadd(x[2], x[5]), p3 = cadd(x[3], x[4]);
  const double2 m1 = csub(x[1], x[6]), m2 = csub(x[2], x[5]), m3 = csub(x[3], x[4]);
  const double2 x0 = x[0];
  x[0] = cadd(cadd(x0, p1), cadd(p2, p3));
  // a_k = x0 + sum_j cos(2 pi jk / 7) p_j,  b_k = sum_j sin(2 pi jk / 7) m_j,  X_k = a_k + SGN i b_k,  X_(7-k) = a_k - SGN i b_k
  auto comb = [&](double ca, double cb, double cc, double sa, double sb, double sc, double2& lo, double2& hi) {
    const double2 a{fma(p3.x, cc, fma(p2.x, cb, fma(p1.x, ca, x0.x))), fma(p3.y, cc, fma(p2.y, cb, fma(p1.y, ca, x0.y)))};
    double2 b{fma(m3.x, sc, fma(m2.x, sb, m1.x * sa)), fma(m3.y, sc, fma(m2.y, sb, m1.y * sa))};
    if (SGN < 0) b = double2{-b.x, -b.y};          // (folds into the adds below)
    lo = double2{a.x - b.y, a.y + b.x};            // a + i b
    hi = double2{a.x + b.y, a.y - b.x};            // a - i b
  };
  // jk mod 7: k = 1: (1, 2, 3); k = 2: (2, 4, 6) -> cos (c2, c3, c1), sin (s2, -s3, -s1); k = 3: (3, 6, 2) -> cos (c3, c1, c2), sin (s3, -s1, s2)
  comb(c1, c2, c3, s1, s2, s3, x[1], x[6]);
  comb(c2, c3, c1, s2, -s3, -s1, x[2], x[5]);
  comb(c3, c1, c2, s3, -s1, s2, x[3], x[4]);
}

// byte offset k of a packed table row (8 x u16 in a uint4)
__device__ __forceinline__ unsigned pfa_u16(const uint4& v, int k) {
  const unsigned w = k < 2 ? v.x : (k < 4 ? v.y : (k < 6 ? v.z : v.w));
  return (k & 1) ? (w >> 16) : (w & 0xffffu);
}

// Forward 511-point DFT of one ring.  In: z[q8] = the ring in the S1 layout (element gat(lane, q8)), x0 = element (73 j1) mod 511 for
// the lane's S2 role j1 = lane / 8.  Out: o1[k1] = y[k(instance lane, k1)], o2[k1] = y[k(instance 64 + lane, k1)] (lanes < 9).
__device__ __forceinline__ void pfa511_core(double2 (&z)[8], const double2 x0, double2 (&o1)[7], double2 (&o2)[7], double2* plane,
                                            const double2* B2l, int lane) {
  const int j1l = lane / 9, q9l = lane - 9 * j1l;  // S1 / S3 role (lanes < 63)
  const int j1m = lane >> 3, k8m = lane & 7;       // S2 role (lanes < 56)
  dft8r<-1, 0>(z);
  if (lane < 63) {
    double2* w = plane + j1l * 72 + q9l;
#pragma unroll
    for (int k = 0; k < 8; ++k) w[9 * k] = z[k];  // T2
  }
  d5_wave_sync();
  double2 y[9];
  double2* const a2 = plane + (j1m < 7 ? j1m : 6) * 72 + k8m * 9;  // (lanes >= 56 re-read ring 6: in range, unused)
#pragma unroll
  for (int k = 0; k < 9; ++k) y[k] = a2[k];
  d5_wave_sync();
  pfa_dft9<-1>(y);
  const double2 Y0 = cadd(x0, y[0]);  // the k2 = 0 output: x0 + sum of the other 72 elements (lanes k8 = 0)
  const double2* bw = B2l + k8m * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) y[k] = cmul(y[k], bw[k]);
  if (k8m == 0) y[0] = cadd(y[0], x0);  // + x0 on every output of the convolution
  pfa_dft9<+1>(y);
  if (lane < 56) {
#pragma unroll
    for (int k = 0; k < 9; ++k) a2[k] = y[k];  // T3
    if (k8m == 0) plane[PFA_Y0 + j1m] = Y0;
  }
  d5_wave_sync();
  {
    const double2* r3 = plane + (j1l < 7 ? j1l : 6) * 72 + q9l;
#pragma unroll
    for (int k = 0; k < 8; ++k) z[k] = r3[9 * k];
  }
  d5_wave_sync();
  dft8r<+1, 0>(z);
  if (lane < 63) {
    double2* w = plane + q9l * 7 + j1l;
#pragma unroll
    for (int k = 0; k < 8; ++k) w[63 * k] = z[k];  // T4: instance p9 + 9 p8
  }
  d5_wave_sync();
  {
    const double2* r4 = plane + lane * 7;
    const double2* r5 = plane + (64 + (lane < 9 ? lane : 8)) * 7;  // (lanes >= 9 re-read instance 72: unused)
#pragma unroll
    for (int k = 0; k < 7; ++k) o1[k] = r4[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) o2[k] = r5[k];
  }
  d5_wave_sync();
  pfa_dft7<-1>(o1);
  pfa_dft7<-1>(o2);
}


// ---- ring bodies ------------------------------------------------------------------------------------------------------
// ONE wave per ring unit.  Workgroup = 8 waves = two ring groups of four waves (one ring x four chain slots each); a group
// stages its ring in LDS (64-B segments of the ring arrays), every transpose of the transform is local to a wave.  Every
// launch of a 511-point scale on eight-slot lines takes these bodies (fused rings -> X' -> rings, plain rings -> pixels,
// pixels -> rings; grouped and single-scale); PXM_DFT_PFA=0 at plan creation keeps the Bluestein body for A/B runs and the
// unit-against-unit test; the narrow arrays of one-chain plans keep it too.
// The four waves of a ring group synchronise through an LDS counter of their own (d5_pair_sync, as a wave pair of the
// Bluestein body does): the two ring groups of a workgroup share nothing but the read-only tables, so each runs at its own
// pace -- a workgroup barrier made every phase wait for the slowest of eight waves (7-10 us between a unit's last transform
// and the end of its workgroup in the trace build).  Bounded spin; an expiry sets the plan's PXM_STATUS_PAIR_SYNC bit.
struct PfaTabs {
  const uint16_t* gat;   // [64][8]  byte offset (16 k) of element k = gat(lane, q8) of the S1 layout
  const uint16_t* kidx;  // [80][8]  byte offset (16 k) of output k(instance, k1), rows 0..72
  const double2* B2;     // [8][9]
};

// stage of the exact-length body: [chain slot][k] per ring, rows of 514 slots.  The units gather / scatter pseudo-random k of
// ONE chain slot: with the chain innermost (slot 4 k + r, as in the Bluestein bodies) a wave would touch 4 of the 16 bank
// groups only (190 / 329 instead of ~94 / ~157 LDS cycles per gather / scatter, scripts/dev/proto_pfa511.py); 514 = 2 mod 8
// keeps the cooperative fill (thread -> (chain, k): 4 chains x 2 k per group of eight lanes) free of write conflicts.
constexpr int PFA_STAGE_S = 514;
static_assert(4 * PFA_STAGE_S <= 4 * PFA_PLANE, "a ring group's stage fits in its four planes");

// bxw: workgroup index along the rings; the workgroup takes the ring pairs bxw * passes + ps, ps < passes, one after the
// other (passes = 2: half as many workgroups -- with one such workgroup per CU the latency-bound workgroups of the small
// scales are resident from the start of the launch instead of forming a second round).
// STOCK: the launch is the stock MYULA update (dft_step_is_stock, sht_core.h; fp64 noise): its epilogue is
// px_stock_update4 (update.h) and none of the mode fields of PxOut is read.
// XOUT: cache policy of the X' stores (mem_policy.h); STOCK only.
template <bool RING_OUT, bool N64, bool STOCK = false, int XOUT = MEM_DEFAULT>
__device__ __forceinline__ void ring2px_body_pfa(const Dft5Args& a, const PfaTabs& pt, double* __restrict__ G, int ncol,
                                                 const PxOut& out, int C, int bxw, int by, int passes, double2* lds5) {
  static_assert(!STOCK || (RING_OUT && N64), "the stock instantiation is the fused step with the fp64 noise stream");
  static_assert(STOCK || XOUT == MEM_DEFAULT, "only the stock instantiation carries a cache policy");
  if ((by << 2) >= C) return;
#ifdef PXM_D5_TRACE
  unsigned long long d5_stamp[7] = {0, 0, 0, 0, 0, 0, 0};
  unsigned long long d5_t0 = wall_clock64();
#endif
  constexpr int n = PFA_N, R = 4, S = PFA_STAGE_S;
  // Everything derived from the thread id is formed from an OPAQUE copy of it, once in front of the pass loop and again at the top
  // of every pass: hoisted out of the loop as invariants these values (lane roles, LDS and global bases) stay live through the
  // whole pass and cost 65-90 spilled registers at the 128-VGPR budget.
#define PXM_PFA_THREAD_SETUP                                                                                              \
  int tid = threadIdx.x;                                                                                                  \
  asm volatile("" : "+v"(tid));                                                                                           \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;                                             \
  const int r = wave & 3, grp = wave >> 2; /* chain slot of the unit; ring group (waves 0-3 / 4-7: one ring each per pass) */ \
  const int c0 = by * R, ch = c0 + r;                                                                                     \
  const int Cp = ncol >> 1;                                                                                               \
  double2* stage = lds5 + grp * (4 * PFA_PLANE); /* the group's stage aliases the group's own four planes */              \
  double2* plane = lds5 + wave * PFA_PLANE;                                                                               \
  double2* B2l = lds5 + 8 * PFA_PLANE;                                                                                    \
  const double2* const logt = B2l + 72;                                                                                   \
  const double2* const sct = B2l + 72 + NOISE_LOG_N;                                                                      \
  unsigned* const gcnt = reinterpret_cast<unsigned*>(B2l + 72 + NOISE_LOG_N + 256) + grp;                                 \
  const int j1m = lane >> 3;                                                                                              \
  const int x0k = (73 * (j1m < 7 ? j1m : 6)) % n; /* element j2 = 0 of the lane's S2 ring role */                         \
  const int mstride = a.Rp * Cp;                  /* complex elements between consecutive m */                            \
  /* ring <-> stage: thread of the group -> (chain rr, k = kq + 64 i), 64-B segments of the ring arrays */                 \
  const int rr = tid & (R - 1), kq = (tid & 255) >> 2;                                                                    \
  const bool cv = c0 + rr < Cp;                                                                                           \
  double2* const Gc = reinterpret_cast<double2*>(G) + c0 + rr;
#define PXM_PFA_RING_LOAD(TT)                                                                                             \
  { /* all eight loads of the thread in flight together */                                                                \
    const int tt_ = (TT);                                                                                                 \
    const bool rv_ = cv && tt_ < a.L;                                                                                     \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                                       \
      const int k = kq + 64 * i;                                                                                          \
      v[i] = double2{0.0, 0.0};                                                                                           \
      if (rv_ && k < n) v[i] = Gc[((k < a.L) ? k + a.L - 1 : k - a.L) * mstride + tt_ * Cp];                              \
    }                                                                                                                     \
  }
  double2 v[8];
  unsigned epoch = 0;
  const D5Sync sy{a.err, a.spin_limit};
  {
    PXM_PFA_THREAD_SETUP
    (void)ch; (void)stage; (void)plane; (void)logt; (void)sct; (void)gcnt; (void)x0k; (void)lane;
    if (tid < 72) B2l[tid] = pt.B2[tid];
    // fp64 noise: LDS copies of the two Box-Muller tables (129 + 256 entries behind the filter spectrum); behind them the two
    // group counters: 81 056 B per workgroup
#if !defined(PXM_NOISE_F64_POLY)
    if (N64 && (STOCK || (out.X && !out.noise)) && tid < NOISE_LOG_N + 256)  // (385 entries, 512 threads)
      B2l[72 + tid] = tid < NOISE_LOG_N ? reinterpret_cast<const double2*>(&NOISE_LOG_TAB[0][0])[tid]
                                        : reinterpret_cast<const double2*>(&NOISE_SINCOS_TAB[0][0])[tid - NOISE_LOG_N];
#endif
    if (tid < 2) reinterpret_cast<unsigned*>(B2l + 72 + NOISE_LOG_N + 256)[tid] = 0;
    PXM_PFA_RING_LOAD((bxw * passes) * 2 + grp)
  }
  d5_barrier();  // the tables and the counters are in place (the only workgroup barrier of this body)
#pragma nounroll
  for (int ps = 0; ps < passes; ++ps) {
  PXM_PFA_THREAD_SETUP
  const int t = (bxw * passes + ps) * 2 + grp;
  const bool tv = t < a.L;
#pragma unroll
  for (int i = 0; i < 8; ++i) {  // conjugated: inverse DFT by conjugation
    const int k = kq + 64 * i;
    if (k < n) stage[rr * S + k] = double2{v[i].x, -v[i].y};
  }
  d5_pair_sync(gcnt, epoch += 4, lane, sy);
  PXM_D5_STAMP(0)  // ring staged
  double2 z[8], o1[7], o2[7];
  double2 x0;
  {
    const char* sb = reinterpret_cast<const char*>(stage + r * S);
    const uint4 gv = reinterpret_cast<const uint4*>(pt.gat)[lane];
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] = *reinterpret_cast<const double2*>(sb + pfa_u16(gv, q));
    x0 = *reinterpret_cast<const double2*>(sb + 16 * x0k);
  }
  d5_pair_sync(gcnt, epoch += 4, lane, sy);  // the stage is dead: the planes may be written
  PXM_D5_STAMP(1)  // unit gathered
  pfa511_core(z, x0, o1, o2, plane, B2l, lane);
  PXM_D5_STAMP(2)  // inverse transform done
  // natural order in the plane: slot k = y[k]
  {
    char* pb_ = reinterpret_cast<char*>(plane);
    const uint4 kv1 = reinterpret_cast<const uint4*>(pt.kidx)[lane];
    const uint4 kv2 = reinterpret_cast<const uint4*>(pt.kidx)[64 + (lane < 9 ? lane : 8)];
#pragma unroll
    for (int k = 0; k < 7; ++k) *reinterpret_cast<double2*>(pb_ + pfa_u16(kv1, k)) = o1[k];
    if (lane < 9) {
#pragma unroll
      for (int k = 0; k < 7; ++k) *reinterpret_cast<double2*>(pb_ + pfa_u16(kv2, k)) = o2[k];
    }
    d5_wave_sync();
  }
  // The lane's eight elements lane + 64 p go through the epilogue FOUR at a time, from the plane and back into it (the
  // natural-order plane is the input of the second transform's gather): never more than four elements in registers
  // beside the epilogue's operands, as in the Bluestein body.
  const bool act = ch < C && tv;
  const int64_t e0 = out.ring0 + (int64_t)t * n + lane;  // the lane's first element; p advances by 64
  const int64_t ce0 = (int64_t)ch * out.chain_stride + e0;
  const bool last_ok = lane < 63;                        // element lane + 448 exists
  const uint64_t it_eff = out.iter + ((STOCK || out.iter_dev) ? *out.iter_dev : 0);
  const int ch_s = __builtin_amdgcn_readfirstlane(ch);
#pragma unroll
  for (int g0 = 0; g0 < 8; g0 += 4) {
    if constexpr (STOCK) {
      // the stock update (update.h), plane -> X' -> plane four elements at a time
      double2* park = plane + lane + 64 * g0;
      if (act) {
        const bool ok[4] = {true, true, true, g0 + 3 < 7 || last_ok};  // (lane 63, p = 7: slot 511, never an element)
        px_stock_update4<64, XOUT>(out, ok, e0 + 64 * g0, ce0 + 64 * g0, -lane - 64 * g0, ch_s, it_eff, park, logt, sct);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) park[64 * u] = double2{0.0, 0.0};  // padding chains / rings: their rings are kept at zero
      }
#ifdef PXM_D5_TRACE
      if (g0 == 0) PXM_D5_STAMP(3) else PXM_D5_STAMP(4)
#endif
      continue;
    }
    double2 x[4];
    // (lane 63, p = 7: slot 511, never an element.  In the update branch the four elements stay in the plane until the noise
    // has been drawn: 16 registers fewer across the fp64 Box-Muller)
    if (!N64 || !(act && out.X)) {  // (f32 noise: reading early is the allocation without spills)
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = plane[lane + 64 * (g0 + u)];
    }
    if (act && out.X) {  // fused prox + MYULA update (pxmcmc/mcmc.py:185-201, prior.py:49-50); see ring2px_body5
      double2 xs[4], wn[4], wph[4];
      double Ts[4];
      int eo[4];  // element offsets from e0 (32 bits: a ring is 511 elements)
      // operand loads FIRST, the noise of the four elements while they are in flight (this body holds four elements, not
      // eight, beside the epilogue's operands: the fp64 Box-Muller fits between the loads and their use without spills --
      // in ring2px_body5 that order cost 250 spilled registers)
#pragma unroll
      for (int u = 0; u < 4; ++u) eo[u] = (g0 + u < 7 || last_ok) ? 64 * (g0 + u) : -lane;  // (else: the ring's element 0)
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
      __builtin_amdgcn_sched_barrier(0);
#if !defined(PXM_NOISE_F64_POLY)
      // fp64 noise of a chain pair (the benchmarked mode): the Philox bits of the four elements first -- four independent
      // integer chains --, then the fp64 Box-Muller step element by element (its ~40 live registers are why the elements
      // are not interleaved there)
      if (N64 && !out.noise && out.mode == PXM_MODE_REAL_PAIRS && !(out.chain0 & 1)) {
        uint4 pbits[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          pbits[u] = philox_bits(out.seed + PXM_PAIR_TWEAK, (out.chain0 >> 1) + ch_s, (uint64_t)(e0 + 64 * (g0 + u)), it_eff);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const NormalPair q_ = normal_pair_from_bits_tabs(pbits[u], logt, sct);
          wph[u] = double2{q_.z0, q_.z1};
          __builtin_amdgcn_sched_barrier(0);
        }
      } else
#endif
      {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        wph[u] = double2{0.0, 0.0};
#if defined(PXM_NOISE_F64_POLY)
        if (!out.noise) wph[u] = px_noise_philox_t<N64>(out, ch_s, e0 + 64 * (g0 + u), it_eff);
#else
        if (!out.noise) wph[u] = N64 ? px_noise_philox_tabs(out, ch_s, e0 + 64 * (g0 + u), it_eff, logt, sct)
                                     : px_noise_philox_t<false>(out, ch_s, e0 + 64 * (g0 + u), it_eff);
#endif
        __builtin_amdgcn_sched_barrier(0);
      }
      }
      if (N64) {
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = plane[lane + 64 * (g0 + u)];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = g0 + u;
        if (p == 7 && !last_ok) {
          x[u] = double2{0.0, 0.0};
          continue;
        }
        const double2 y{x[u].x, -x[u].y};
        const double2 w = out.noise ? wn[u] : wph[u];
        x[u] = px_update(out, xs[u], Ts[u], y, w);
        reinterpret_cast<double2*>(out.f)[ce0 + 64 * p] = x[u];
      }
    } else if (act) {  // plain / gathered output and the residual that goes back to the rings
      bool ok[4];
      int64_t ev[4];
      double2 yv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ok[u] = g0 + u < 7 || last_ok;
        ev[u] = ok[u] ? e0 + 64 * (g0 + u) : out.ring0 + (int64_t)t * n;
        yv[u] = double2{x[u].x, -x[u].y};
      }
      px_out_store_n<4>(out, ch, ev, yv, ok);
      if (out.rdata) {
        double2 rd[4], rc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) rd[u] = reinterpret_cast<const double2*>(out.rdata)[ev[u]];
        if (out.rinvcov_complex) {
#pragma unroll
          for (int u = 0; u < 4; ++u) rc[u] = reinterpret_cast<const double2*>(out.rinvcov)[ev[u]];
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) rc[u] = double2{out.rinvcov[ev[u]], 0.0};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double2 d = csub(yv[u], rd[u]);
          yv[u] = out.rinvcov_complex ? cmul(rc[u], d) : double2{rc[u].x * d.x, rc[u].x * d.y};
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = ok[u] ? yv[u] : double2{0.0, 0.0};
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = double2{0.0, 0.0};  // padding chains / rings: their rings are kept at zero
    }
    if (RING_OUT) {
#pragma unroll
      for (int u = 0; u < 4; ++u) plane[lane + 64 * (g0 + u)] = x[u];
    }
#ifdef PXM_D5_TRACE
    if (g0 == 0) PXM_D5_STAMP(3) else PXM_D5_STAMP(4)  // first / second half of the epilogue done
#endif
  }
  if (!RING_OUT) {  // plain rings -> pixels: the pass ends here; the next ring may be staged once every plane of the group is dead
    PXM_PFA_RING_LOAD(ps + 1 < passes ? (bxw * passes + ps + 1) * 2 + grp : a.L)
    if (ps + 1 < passes) d5_pair_sync(gcnt, epoch += 4, lane, sy);
    continue;
  }
  // ---- forward transform of the updated ring: natural order -> S1 layout through the plane
  d5_wave_sync();
  {
    const char* pb_ = reinterpret_cast<const char*>(plane);
    const uint4 gv = reinterpret_cast<const uint4*>(pt.gat)[lane];
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] = *reinterpret_cast<const double2*>(pb_ + pfa_u16(gv, q));
    x0 = plane[x0k];
  }
  d5_wave_sync();
  pfa511_core(z, x0, o1, o2, plane, B2l, lane);
  PXM_D5_STAMP(5)  // forward transform done
  d5_pair_sync(gcnt, epoch += 4, lane, sy);  // every plane of the group is dead: its stage may be written
  {
    char* sb = reinterpret_cast<char*>(stage + r * S);
    const uint4 kv1 = reinterpret_cast<const uint4*>(pt.kidx)[lane];
    const uint4 kv2 = reinterpret_cast<const uint4*>(pt.kidx)[64 + (lane < 9 ? lane : 8)];
#pragma unroll
    for (int k = 0; k < 7; ++k) *reinterpret_cast<double2*>(sb + pfa_u16(kv1, k)) = o1[k];
    if (lane < 9) {
#pragma unroll
      for (int k = 0; k < 7; ++k) *reinterpret_cast<double2*>(sb + pfa_u16(kv2, k)) = o2[k];
    }
  }
  // the next ring's loads are in flight across the stores (unconditional assignment -- zeros behind the last pass: a conditional
  // one would keep the eight registers of v live through the whole pass)
  PXM_PFA_RING_LOAD(ps + 1 < passes ? (bxw * passes + ps + 1) * 2 + grp : a.L)
  d5_pair_sync(gcnt, epoch += 4, lane, sy);
  PXM_D5_STAMP(6)  // results in the stage
  if (cv && tv) {  // stage -> G rows of the ring
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = kq + 64 * i;
      if (k < n) Gc[((k < a.L) ? k + a.L - 1 : k - a.L) * mstride + t * Cp] = stage[rr * S + k];
    }
  }
  if (ps + 1 < passes) d5_pair_sync(gcnt, epoch += 4, lane, sy);  // the stage has been read: the next ring may be staged
#ifdef PXM_D5_TRACE
  if (tid == 0 && g_dft_trace) {
    const unsigned long long slot = atomicAdd(g_dft_trace + 1, 1ull);
    unsigned long long* rr_ = g_dft_trace + 8 + 8 * 4096 + 8 * slot;
    rr_[0] = 9;  // six phase stamps + the end of the pass (bx / by are not recorded for this body)
    for (int k = 0; k < 6; ++k) rr_[1 + k] = d5_stamp[k] - d5_t0;
    rr_[7] = wall_clock64() - d5_t0;
    d5_t0 = wall_clock64();
  }
#endif
  }  // passes
#undef PXM_PFA_THREAD_SETUP
#undef PXM_PFA_RING_LOAD
}

// pixels -> rings of the same unit (the plain forward phi-DFT of a 511-point scale: px2ring_body5's job): every wave loads its
// ring in natural order straight into its plane, gathers the S1 layout, transforms, and the four waves of a ring group put the
// result through the group's stage into 64-B segments of the ring array.  ZFILL as in PXM_D5_STORE_RINGS(true): the last live
// chain group also zeroes the padding slots of its (m, ring) lines.
__device__ __forceinline__ void px2ring_body_pfa(const Dft5Args& a, const PfaTabs& pt, const PxIn& in, double* __restrict__ G, int ncol,
                                                 int C, int bxw, int by, int passes, double2* lds5) {
  if ((by << 2) >= C) return;
  constexpr int n = PFA_N, R = 4, S = PFA_STAGE_S;
  unsigned epoch = 0;
  const D5Sync sy{a.err, a.spin_limit};
  {
    const int tid = threadIdx.x;
    double2* B2l = lds5 + 8 * PFA_PLANE;
    if (tid < 72) B2l[tid] = pt.B2[tid];
    if (tid < 2) reinterpret_cast<unsigned*>(B2l + 72 + NOISE_LOG_N + 256)[tid] = 0;
  }
  d5_barrier();
#pragma nounroll
  for (int ps = 0; ps < passes; ++ps) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));  // (see ring2px_body_pfa: nothing derived from the thread id is hoisted out of the pass loop)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int r = wave & 3, grp = wave >> 2;
    const int c0 = by * R, ch = c0 + r;
    const int Cp = ncol >> 1;
    double2* stage = lds5 + grp * (4 * PFA_PLANE);
    double2* plane = lds5 + wave * PFA_PLANE;
    const double2* B2l = lds5 + 8 * PFA_PLANE;
    unsigned* const gcnt = reinterpret_cast<unsigned*>(lds5 + 8 * PFA_PLANE + 72 + NOISE_LOG_N + 256) + grp;
    const int j1m = lane >> 3;
    const int x0k = (73 * (j1m < 7 ? j1m : 6)) % n;
    const int t = (bxw * passes + ps) * 2 + grp;
    const bool tv = t < a.L;
    const bool act = ch < C && tv;
    const int64_t e_ring = in.ring0 + (int64_t)(tv ? t : 0) * n;
#pragma unroll
    for (int g0 = 0; g0 < 8; g0 += 4) {  // the lane's elements lane + 64 p, four at a time (see px2ring_body5)
      int64_t ev[4];
      bool ok[4];
      double2 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = lane + 64 * (g0 + u);
        ok[u] = act && j < n;
        ev[u] = e_ring + (j < n ? j : 0);
      }
      if (ch < C) px_in_load_n<4>(in, ch, ev, ok, v);
      else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = double2{0.0, 0.0};
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) plane[lane + 64 * (g0 + u)] = v[u];  // (lane 63, p = 7: slot 511, a zero)
    }
    d5_wave_sync();
    double2 z[8], o1[7], o2[7];
    double2 x0;
    {
      const char* pb_ = reinterpret_cast<const char*>(plane);
      const uint4 gv = reinterpret_cast<const uint4*>(pt.gat)[lane];
#pragma unroll
      for (int q = 0; q < 8; ++q) z[q] = *reinterpret_cast<const double2*>(pb_ + pfa_u16(gv, q));
      x0 = plane[x0k];
    }
    d5_wave_sync();
    pfa511_core(z, x0, o1, o2, plane, B2l, lane);
    d5_pair_sync(gcnt, epoch += 4, lane, sy);  // every plane of the group is dead: its stage may be written
    {
      char* sb = reinterpret_cast<char*>(stage + r * S);
      const uint4 kv1 = reinterpret_cast<const uint4*>(pt.kidx)[lane];
      const uint4 kv2 = reinterpret_cast<const uint4*>(pt.kidx)[64 + (lane < 9 ? lane : 8)];
#pragma unroll
      for (int k = 0; k < 7; ++k) *reinterpret_cast<double2*>(sb + pfa_u16(kv1, k)) = o1[k];
      if (lane < 9) {
#pragma unroll
        for (int k = 0; k < 7; ++k) *reinterpret_cast<double2*>(sb + pfa_u16(kv2, k)) = o2[k];
      }
    }
    d5_pair_sync(gcnt, epoch += 4, lane, sy);
    {  // stage -> G rows of the ring
      const int rr = tid & (R - 1), kq = (tid & 255) >> 2;
      const int mstride = a.Rp * Cp;
      double2* const Gc = reinterpret_cast<double2*>(G) + c0 + rr;
      const bool zf = c0 + R >= C;
      if (c0 + rr < Cp && tv) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int k = kq + 64 * i;
          if (k < n) {
            double2* line = Gc + ((k < a.L) ? k + a.L - 1 : k - a.L) * mstride + t * Cp;
            *line = stage[rr * S + k];
            if (zf)
              for (int zz = R; c0 + rr + zz < Cp; zz += R) line[zz] = double2{0.0, 0.0};
          }
        }
      }
    }
    if (ps + 1 < passes) d5_pair_sync(gcnt, epoch += 4, lane, sy);  // the stage has been read
  }
}

}  // namespace pxm
