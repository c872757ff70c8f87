// Device helpers shared by the units of the phi-DFT stage that run a ring on whole waves: the Bluestein pair unit
// (dft_wave.hip, L <= 256), the Bluestein quad unit (dft_wave.hip, 256 < L <= 512) and the exact-length unit (dft_pfa.h).
//
// Mh-point transform, j = j0 + r0 j1 + 8 r0 j2 (j0 < r0; j1, j2 < 8), bin k = k2 + 8 k1 + 64 k0 (k0 < r0):
//   lane = g + 8 j1, g = j0 + r0 rho (rho = ring of the wave), registers p = j2: element j = lam + 8 r0 p of ring
//   rho, lam = j0 + r0 j1 -- consecutive lanes hold consecutive elements;
//   pass 1: radix 8 over j2 -> k2, twiddle W_Mh^(lam k2);         T1: lane g + 8 j1, reg k2 -> lane g + 8 k2, reg j1
//   pass 2: radix 8 over j1 -> k1, twiddle W_(8 r0)^(j0 k1);      T2: lane g + 8 k2, reg k1 -> lane k1 + 8 k2, reg g
//   pass 3: radix r0 over j0 -> k0 for every ring;                bin k of ring rho in reg k0 + r0 rho
// and the mirror image back (scripts/proto_dft5.py is the lane- and register-exact numpy model of this file).
// The transposes go through a per-wave LDS plane of 8 x 72 complex: T1 at 72 k2 + 8 j1 + g, T2 at 72 k2 + 9 k1 + g;
// with these pitches every ds_write_b128 (8 contiguous lanes per pass) and ds_read_b128 (the four 16-lane groups
// {0-3,12-15,20-27} ...) of both directions is bank-conflict-free.
#pragma once
#include "elem.h"

namespace pxm {

constexpr int D5_PLANE = 8 * 72;  // complex elements of one wave's transpose plane
constexpr int D5_TW = 512;        // LDS copy of the pass twiddles: tw1 rows k = 1..7 ([7][64]) then wt ([8][8])

// Workgroup barrier of these kernels: every exchange between waves goes through LDS, so only the LDS counter has to
// drain before the barrier.  __syncthreads() is fence + s_barrier = s_waitcnt vmcnt(0) lgkmcnt(0): it also waited
// for every global load AND STORE in flight -- the stores of the updated coefficients sat in front of the exchange
// barrier of the forward transform, the ring stores of a chain group in front of nothing at all.  Global memory needs
// no intra-kernel ordering here: a workgroup only re-reads global data it has not written (the in-place ring stores
// come after every ring load of the workgroup has been consumed into LDS).
__device__ __forceinline__ void d5_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Synchronisation of the TWO waves of a ring set (the even- and odd-bin halves exchange their shares through LDS):
// an LDS counter per wave pair instead of a workgroup barrier.  With s_barrier the four ring sets of a workgroup moved
// in lock-step -- all eight waves hit the LDS in the same phase and the vector ALUs in the next -- although only the
// pairs exchange anything between the staging barriers; decoupled, the pairs drift apart and one pair's transposes
// overlap another's butterflies.  LDS operations of a wave are performed in order, so the ds_add behind the wave's
// ds_writes publishes them.  The spin is bounded (a lost partner would otherwise hang the GPU); a wait that EXPIRES
// sets bit PXM_STATUS_PAIR_SYNC of the owning plan's status word -- the kernel runs on with data its partner has not
// written, and the host finds the bit wherever it already synchronises (pxm_wav_status / pxm_sht_status: the sampler
// raises at its next save point instead of returning a silently corrupted chain).
struct D5Sync {
  unsigned* err;
  unsigned limit;
};
__device__ __forceinline__ void d5_pair_sync(unsigned* cnt, unsigned target, int lane, const D5Sync& sy) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  unsigned spins = 0;
  bool ready;
  while (!(ready = __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) >= (int)target) &&
         ++spins < sy.limit)
    __builtin_amdgcn_s_sleep(1);
  if (!ready && sy.err && lane == 0) __hip_atomic_fetch_or(sy.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ void d5_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// v * exp(SGN i pi k / 4)
template <int SGN>
__device__ __forceinline__ double2 mul_w8(double2 v, int k) {
  constexpr double s = 0.70710678118654752440;
  switch (k & 3) {
    case 0: return v;
    case 1: return SGN < 0 ? double2{s * (v.x + v.y), s * (v.y - v.x)} : double2{s * (v.x - v.y), s * (v.x + v.y)};
    case 2: return SGN < 0 ? double2{v.y, -v.x} : double2{-v.y, v.x};
    default: return SGN < 0 ? double2{s * (v.y - v.x), -s * (v.x + v.y)} : double2{-s * (v.x + v.y), s * (v.x - v.y)};
  }
}
__device__ __forceinline__ void d5_swap(double2& a, double2& b) {
  const double2 t = a;
  a = b;
  b = t;
}

// in-register DFTs over consecutive registers x[B .. B + R), natural order in and out
template <int SGN, int B>
__device__ __forceinline__ void dft8r(double2 (&x)[8]) {
  static_assert(B == 0, "one 8-point transform per lane");
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double2 u = x[i], v = x[i + 4];
    x[i] = cadd(u, v);
    x[i + 4] = mul_w8<SGN>(csub(u, v), i);
  }
#pragma unroll
  for (int h = 0; h < 8; h += 4)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const double2 u = x[h + i], v = x[h + i + 2];
      x[h + i] = cadd(u, v);
      x[h + i + 2] = mul_w8<SGN>(csub(u, v), 2 * i);
    }
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const double2 u = x[i], v = x[i + 1];
    x[i] = cadd(u, v);
    x[i + 1] = csub(u, v);
  }
  d5_swap(x[1], x[4]);  // bit reversal (compile-time register renaming)
  d5_swap(x[3], x[6]);
}
template <int SGN, int B>
__device__ __forceinline__ void dft4r(double2 (&x)[8]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double2 u = x[B + i], v = x[B + i + 2];
    x[B + i] = cadd(u, v);
    x[B + i + 2] = mul_w8<SGN>(csub(u, v), 2 * i);
  }
#pragma unroll
  for (int i = 0; i < 4; i += 2) {
    const double2 u = x[B + i], v = x[B + i + 1];
    x[B + i] = cadd(u, v);
    x[B + i + 1] = csub(u, v);
  }
  d5_swap(x[B + 1], x[B + 2]);
}
template <int B>
__device__ __forceinline__ void dft2r(double2 (&x)[8]) {
  const double2 u = x[B], v = x[B + 1];
  x[B] = cadd(u, v);
  x[B + 1] = csub(u, v);
}
// pass 3 / 3': radix r0 over j0 for each of the 8 / r0 rings of the wave
template <int SGN, int R0>
__device__ __forceinline__ void pass3(double2 (&x)[8]) {
  if (R0 == 8) dft8r<SGN, 0>(x);
  if (R0 == 4) {
    dft4r<SGN, 0>(x);
    dft4r<SGN, 4>(x);
  }
  if (R0 == 2) {
    dft2r<0>(x);
    dft2r<2>(x);
    dft2r<4>(x);
    dft2r<6>(x);
  }
}

// per-lane constants of the transposes and twiddle look-ups
struct D5Lane {
  int lo, hi;  // lane & 7, lane >> 3
};

// forward Mh-point transform of the wave's rings: natural order -> bins (reg k0 + r0 rho, lane k1 + 8 k2)
template <int R0>
__device__ __forceinline__ void d5_fwd(double2 (&z)[8], double2* plane, int lane, const D5Lane& q, const double2* tw) {
  dft8r<-1, 0>(z);
#pragma unroll
  for (int k = 1; k < 8; ++k) z[k] = cmul(z[k], tw[(k - 1) * 64 + lane]);
#pragma unroll
  for (int k = 0; k < 8; ++k) plane[72 * k + lane] = z[k];  // T1
  d5_wave_sync();
#pragma unroll
  for (int k = 0; k < 8; ++k) z[k] = plane[72 * q.hi + 8 * k + q.lo];
  d5_wave_sync();
  dft8r<-1, 0>(z);
  if (R0 > 1) {
#pragma unroll
    for (int k = 1; k < 8; ++k) z[k] = cmul(z[k], tw[448 + k * 8 + (q.lo & (R0 - 1))]);  // W^(j0(g) k1)
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) plane[72 * q.hi + 9 * k + q.lo] = z[k];  // T2
  d5_wave_sync();
#pragma unroll
  for (int k = 0; k < 8; ++k) z[k] = plane[72 * q.hi + 9 * q.lo + k];
  d5_wave_sync();
  pass3<-1, R0>(z);
}

// the mirror image: bins -> natural order (unnormalised inverse transform)
template <int R0>
__device__ __forceinline__ void d5_inv(double2 (&z)[8], double2* plane, int lane, const D5Lane& q, const double2* tw) {
  pass3<+1, R0>(z);
  if (R0 > 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k & (R0 - 1)) z[k] = cmulc(z[k], tw[448 + (k & (R0 - 1)) * 8 + q.lo]);  // W^(-j0(reg) k1)
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) plane[72 * q.hi + 9 * q.lo + k] = z[k];  // T2'
  d5_wave_sync();
#pragma unroll
  for (int k = 0; k < 8; ++k) z[k] = plane[72 * q.hi + 9 * k + q.lo];
  d5_wave_sync();
  dft8r<+1, 0>(z);
#pragma unroll
  for (int k = 0; k < 8; ++k) plane[72 * q.hi + 8 * k + q.lo] = z[k];  // T1'
  d5_wave_sync();
#pragma unroll
  for (int k = 0; k < 8; ++k) z[k] = plane[72 * k + lane];
  d5_wave_sync();
#pragma unroll
  for (int k = 1; k < 8; ++k) z[k] = cmulc(z[k], tw[(k - 1) * 64 + lane]);
  dft8r<+1, 0>(z);
}

// cyclic convolution half: z (chirped input, natural order) -> forward transform -> filter spectrum bw -> back
template <int R0>
__device__ __forceinline__ void d5_conv(double2 (&z)[8], double2* plane, int lane, const D5Lane& q, const double2* tw,
                                        const double2* __restrict__ bw) {
  d5_fwd<R0>(z, plane, lane, q, tw);
#pragma unroll
  for (int k = 0; k < 8; ++k) z[k] = cmul(z[k], bw[(k & (R0 - 1)) * 64 + lane]);
  d5_inv<R0>(z, plane, lane, q, tw);
}

// lane-wise select on the (wave-uniform) half index: registers keep compile-time indices
__device__ __forceinline__ double2 d5_sel(int half, double2 a, double2 b) { return double2{half ? a.x : b.x, half ? a.y : b.y}; }

}  // namespace pxm
