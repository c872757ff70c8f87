// Per-element device functions shared by the elementwise kernels and the DFT stage's fused epilogues.
#pragma once
#include <hip/hip_runtime.h>

#include "philox.h"

namespace pxm {

__device__ inline double2 cmul(double2 a, double2 b) { return double2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ inline double2 cmulc(double2 a, double2 b) {  // a * conj(b)
  return double2{a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y};
}
__device__ inline double2 cadd(double2 a, double2 b) { return double2{a.x + b.x, a.y + b.y}; }
__device__ inline double2 csub(double2 a, double2 b) { return double2{a.x - b.x, a.y - b.y}; }

// utils.soft (pxmcmc/utils.py:55-67,84-88): sign(x) (|x| - T) where |x| > T else 0, in the
// reference's own operation order: (x / |x|) * (|x| - T)
__device__ inline double soft_real(double x, double T) {
  const double a = fabs(x);
  if (a <= T) return 0.0;
  return copysign(a - T, x);  // == (x / a) * (a - T) bit for bit: x / |x| is exactly +-1 for a finite non-zero x
}
// complex: sign(z) (|z| - T) = z (|z| - T) / |z| with ONE division and a plain sqrt (no hypot rescaling: |z|^2 of
// a chain state is far inside the fp64 range); differs from the reference's (z / |z|) * (|z| - T) by at most
// an ulp or two (tests: 1e-13 relative against the golden vectors captured from the reference)
__device__ inline double2 soft_cplx(double2 z, double T) {
  const double a = sqrt(fma(z.x, z.x, z.y * z.y));
  if (a <= T) return double2{0.0, 0.0};
  const double s = (a - T) / a;
  return double2{z.x * s, z.y * s};
}

// MYULA.chain_step (pxmcmc/mcmc.py:196-201), same association order as the reference:
// ((1 - d/l) X + (d/l) proxf - d gradg) + sqrt(2 d) w
__device__ inline double chain_step_real(double X, double px, double g, double w, double delta, double lmda) {
  const double r = delta / lmda;
  return (1 - r) * X + r * px - delta * g + sqrt(2 * delta) * w;
}
// the same step with its two chain-independent factors r = d / l and s = sqrt(2 d) formed by the caller, once for all its
// elements (the division and the square root are ~25 fp64 operations): the same operations on X, px, g and w in the same order
__device__ __forceinline__ double chain_step_real_rs(double X, double px, double g, double w, double delta, double r, double s) {
  return (1 - r) * X + r * px - delta * g + s * w;
}
__device__ inline double2 chain_step_cplx(double2 X, double2 px, double2 g, double2 w, double delta, double lmda) {
  return double2{chain_step_real(X.x, px.x, g.x, w.x, delta, lmda), chain_step_real(X.y, px.y, g.y, w.y, delta, lmda)};
}

// x * x + y * y with both products and the sum rounded (no fma contraction): numpy's re ** 2 + im ** 2
__device__ __forceinline__ double abs2_plain(double x, double y) {
#pragma clang fp contract(off)
  return x * x + y * y;
}

// ---- the noise of the stepping kernels (pxm_myula_step, pxm_chain_step, pxm_randn, pxm_sapg_step): a given [C][n] array
// or the Philox stream keyed (seed, chain0 + c, element, iter + *iter_dev)
struct NoiseSrc {
  const double* noise;
  int noise_complex;
  uint64_t seed, chain0, iter;
  const uint64_t* iter_dev = nullptr;  // optional device-resident addend to iter (caller-owned counter: graph replay)
  int f64 = 0;                         // Box-Muller step in double precision (flag PXM_NOISE_F64 of the entry point)
};
// noise_complex argument of the entry points = (0 | 1) | PXM_NOISE_F64 (include/pxmcmc_amd.h is not included here: its mode
// macros would replace the enumerators of update.h; the callers assert that the two values agree)
constexpr int NOISE_F64_FLAG = 16;
static inline NoiseSrc make_noise_src(const void* noise, int noise_arg, uint64_t seed, uint64_t chain0, uint64_t iter,
                                      const uint64_t* iter_dev = nullptr) {
  return NoiseSrc{(const double*)noise, noise_arg & 1, seed, chain0, iter, iter_dev, (noise_arg & NOISE_F64_FLAG) ? 1 : 0};
}

template <bool CPLX>
__device__ inline double2 draw_noise(const NoiseSrc& ns, int c, int64_t n, int64_t i) {
  if (ns.noise) {
    if (CPLX && ns.noise_complex) return reinterpret_cast<const double2*>(ns.noise)[(int64_t)c * n + i];
    return double2{ns.noise[(int64_t)c * n + i], 0.0};
  }
  const uint64_t it = ns.iter + (ns.iter_dev ? *ns.iter_dev : 0);
  if (CPLX && ns.noise_complex) {
    NormalPair q = philox_normal_pair(ns.seed, ns.chain0 + c, (uint64_t)i, it, ns.f64);
    return double2{q.z0, q.z1};
  }
  return double2{philox_normal_real(ns.seed, ns.chain0 + c, (uint64_t)i, it, ns.f64), 0.0};
}

}  // namespace pxm
