// One stage of the SKROCK Chebyshev recursion (Pereyra, Vargas-Mieles & Zygalakis, SIAM J. Imaging Sci. 13(2), 2020;
// the reference's SKROCK._K_recursion, pxmcmc/mcmc.py:349-368), per element of every chain:
//
//   out = a U + b P + c G + e V + r Z
//
// with grad log pi(U) = -(U - P) / lmda - G (pxmcmc/mcmc.py:84-89) folded into the coefficients by the caller:
//   stage 0 -> Y    U = X                          a = 1,                 r = nu_1 sqrt(2 delta)
//   stage 1 -> K_1  U = Y,       G = g(Y),   V = X  a = -mu_1 delta / lmda,  b = mu_1 delta / lmda,  c = -mu_1 delta,
//                                                   e = 1,                 r = kappa_1 sqrt(2 delta)
//   stage j -> K_j  U = K_{j-1}, G = g(U), V = K_{j-2}
//                                                   a = nu_j - mu_j delta / lmda,  b = mu_j delta / lmda,  c = -mu_j delta,
//                                                   e = kappa_j,           r = 0
// P is soft(U, T) formed here (the stock synthesis L1 prox, pxmcmc/prior.py:49-50) or a given proxf array.  Z is the
// project's Philox stream keyed (seed, chain0 + c, element, iteration) -- the same draws as pxm_myula_step -- or a given
// array; stages 0 and 1 of an iteration regenerate the same Z from the same counters, so no noise buffer is kept.
//
// The noise term is a template switch: stages j >= 2 carry no Philox code and are a pure stream (16-byte loads per
// complex128 element, a grid sized to the chip, no LDS).
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"

#include <algorithm>

namespace pxm {

static_assert(NOISE_F64_FLAG == PXM_NOISE_F64, "elem.h: the noise flag must be the public one");

struct SkCoef {
  double a, b, c, e, r;
};

// PM: 0 no prox term, 1 P = soft(U, T), 2 P given.  HAS_G / HAS_V: gradient / second state present.  NOISE: r Z term.
template <bool CPLX, int PM, bool HAS_G, bool HAS_V, bool NOISE>
__global__ __launch_bounds__(256) void k_skrock_stage(const double* __restrict__ U, const double* __restrict__ P,
                                                      const double* __restrict__ T, double Ts, const double* __restrict__ G,
                                                      const double* __restrict__ V, SkCoef k, NoiseSrc ns,
                                                      double* __restrict__ out, int64_t n) {
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (CPLX) {
      const double2 u = reinterpret_cast<const double2*>(U)[base + i];
      double2 acc{k.a * u.x, k.a * u.y};
      if constexpr (PM != 0) {
        const double2 p = PM == 1 ? soft_cplx(u, T ? T[i] : Ts) : reinterpret_cast<const double2*>(P)[base + i];
        acc = double2{fma(k.b, p.x, acc.x), fma(k.b, p.y, acc.y)};
      }
      if constexpr (HAS_G) {
        const double2 g = reinterpret_cast<const double2*>(G)[base + i];
        acc = double2{fma(k.c, g.x, acc.x), fma(k.c, g.y, acc.y)};
      }
      if constexpr (HAS_V) {
        const double2 v = reinterpret_cast<const double2*>(V)[base + i];
        acc = double2{fma(k.e, v.x, acc.x), fma(k.e, v.y, acc.y)};
      }
      if constexpr (NOISE) {
        const double2 z = draw_noise<true>(ns, c, n, i);
        acc = double2{fma(k.r, z.x, acc.x), fma(k.r, z.y, acc.y)};
      }
      reinterpret_cast<double2*>(out)[base + i] = acc;
    } else {
      const double u = U[base + i];
      double acc = k.a * u;
      if constexpr (PM != 0) acc = fma(k.b, PM == 1 ? soft_real(u, T ? T[i] : Ts) : P[base + i], acc);
      if constexpr (HAS_G) acc = fma(k.c, G[base + i], acc);
      if constexpr (HAS_V) acc = fma(k.e, V[base + i], acc);
      if constexpr (NOISE) acc = fma(k.r, draw_noise<false>(ns, c, n, i).x, acc);
      out[base + i] = acc;
    }
  }
}

// grid sized to the chip: at most 2048 workgroups of 256 threads in all (256 CUs x 8), grid-stride for the rest
static inline dim3 sk_grid(int64_t n, int C) {
  int64_t cap = std::max<int64_t>(1, 2048 / C);
  int64_t bx = std::min<int64_t>((n + 255) / 256, cap);
  return dim3((unsigned)std::max<int64_t>(bx, 1), (unsigned)C);
}

template <bool CPLX, int PM, bool HAS_G, bool HAS_V>
static void sk_launch_noise(bool noise, dim3 g, hipStream_t st, const double* U, const double* P, const double* T, double Ts,
                            const double* G, const double* V, SkCoef k, const NoiseSrc& ns, double* out, int64_t n) {
  if (noise)
    hipLaunchKernelGGL((k_skrock_stage<CPLX, PM, HAS_G, HAS_V, true>), g, dim3(256), 0, st, U, P, T, Ts, G, V, k, ns, out, n);
  else
    hipLaunchKernelGGL((k_skrock_stage<CPLX, PM, HAS_G, HAS_V, false>), g, dim3(256), 0, st, U, P, T, Ts, G, V, k, ns, out, n);
}

template <bool CPLX, int PM>
static void sk_launch_gv(bool noise, dim3 g, hipStream_t st, const double* U, const double* P, const double* T, double Ts,
                         const double* G, const double* V, SkCoef k, const NoiseSrc& ns, double* out, int64_t n) {
  if (G && V) sk_launch_noise<CPLX, PM, true, true>(noise, g, st, U, P, T, Ts, G, V, k, ns, out, n);
  else if (G) sk_launch_noise<CPLX, PM, true, false>(noise, g, st, U, P, T, Ts, G, V, k, ns, out, n);
  else if (V) sk_launch_noise<CPLX, PM, false, true>(noise, g, st, U, P, T, Ts, G, V, k, ns, out, n);
  else sk_launch_noise<CPLX, PM, false, false>(noise, g, st, U, P, T, Ts, G, V, k, ns, out, n);
}

template <bool CPLX>
static void sk_launch(int pm, bool noise, dim3 g, hipStream_t st, const double* U, const double* P, const double* T, double Ts,
                      const double* G, const double* V, SkCoef k, const NoiseSrc& ns, double* out, int64_t n) {
  if (pm == 0) sk_launch_gv<CPLX, 0>(noise, g, st, U, P, T, Ts, G, V, k, ns, out, n);
  else if (pm == 1) sk_launch_gv<CPLX, 1>(noise, g, st, U, P, T, Ts, G, V, k, ns, out, n);
  else sk_launch_gv<CPLX, 2>(noise, g, st, U, P, T, Ts, G, V, k, ns, out, n);
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int pxm_skrock_stage(const void* U, const void* proxf, const double* T, double T_scalar, const void* gradg, const void* V,
                     double a, double b, double c, double e, double r, const void* noise, int noise_complex, uint64_t seed,
                     uint64_t chain0, uint64_t iter, const uint64_t* iter_dev, void* out, int64_t n, int C, int dtype,
                     pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_skrock_stage: bad n / C / dtype");
  if (n == 0) return 0;
  PXM_REQUIRE(U && out, "pxm_skrock_stage: null buffer");
  PXM_REQUIRE(out != U && out != proxf && out != gradg && out != V && out != noise,
              "pxm_skrock_stage: out must not alias an input");
  if (int rc = check_noise_arg("pxm_skrock_stage", noise_complex, dtype)) return rc;
  const int pm = b == 0.0 ? 0 : (proxf ? 2 : 1);
  const bool nz = r != 0.0;
  const NoiseSrc ns = make_noise_src(noise, noise_complex, seed, chain0, iter, iter_dev);
  const SkCoef k{a, b, c, e, r};
  const dim3 g = sk_grid(n, C);
  hipStream_t st = (hipStream_t)stream;
  const double *u = (const double*)U, *p = (const double*)proxf, *gr = (const double*)gradg, *v = (const double*)V;
  if (dtype) sk_launch<true>(pm, nz, g, st, u, p, T, T_scalar, gr, v, k, ns, (double*)out, n);
  else sk_launch<false>(pm, nz, g, st, u, p, T, T_scalar, gr, v, k, ns, (double*)out, n);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
