// One iteration of SAPG, the stochastic-approximation proximal-gradient estimator of the regularisation strength (Vidal,
// De Bortoli, Pereyra & Durmus, SIAM J. Imaging Sci. 13(4), 2020), on the posterior of the samplers with the prior scaled by
// a per-chain theta:
//
//   pi_theta(X) ~ exp(-1/2 Re L2(X) - theta G(X)),   G(X) = (1 / lmda) sum_i T_i |X_i|
//
// Step kernel, per element of chain c -- a MYULA step whose soft threshold is theta_c T_i, theta read from device memory:
//
//   thr = fl(theta_c T_i);   X1 = (1 - delta/lmda) X + (delta/lmda) soft(X, thr) - delta g + sqrt(2 delta) w
//
// with the update arithmetic (elem.h: soft_*, chain_step_*) and the noise (elem.h: draw_noise) of pxm_myula_step.  Every
// workgroup also writes one partial of sum_i T_i |X1_i| (plain products and sums, no contraction); the number of workgroups
// per chain depends on n only (reduce.h: chain_slices), so a chain's sum does not depend on its batch.  A pure stream like
// k_fista_step: 16-byte accesses per complex128 element, one element per lane and pass, no LDS beyond the 32 bytes of the
// workgroup sum, no atomics.
//
// Update kernel (one workgroup): G is 1-homogeneous, so the normaliser of exp(-theta G) is ~ theta^-d and the gradient of the
// marginal log-likelihood in eta = log theta is estimated by d - theta G(X1):
//
//   G_c = (partials of chain c, fixed order) / lmda;   pool: G_c := (G_0 + ... + G_{C-1}) / C for every c
//   eta_c = min(max(eta_c + rho_k (d - theta_c G_c), eta_min), eta_max);   theta_c = exp(eta_c)
//
// rho_k is read from a device table at k = iter + *iter_dev (clamped to the table), so a captured graph replays with the
// step size of its iteration; (theta_c, eta_c, G_c) go to row k of the trace when it has one.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"
#include "reduce.h"

#include <cmath>

namespace pxm {

static_assert(NOISE_F64_FLAG == PXM_NOISE_F64, "elem.h: the noise flag must be the public one");

// NZ selects the noise at compile time, so that draw_noise's run-time switches fold away and with them the scalar registers
// of the paths not taken (with all of them in one kernel the complex128 form runs out of scalar registers):
// 0: the caller's array (no Philox code); else the Philox stream, 1 + (Box-Muller in fp64) + 2 * (complex noise), with the
// iteration number read once
template <bool CPLX, int NZ>
__global__ __launch_bounds__(256) void k_sapg_step(const double* __restrict__ X, const double* __restrict__ G,
                                                   const double* __restrict__ T, double Ts,
                                                   const double* __restrict__ theta, double delta, double lmda, NoiseSrc ns_,
                                                   double* __restrict__ X1, double* __restrict__ part, int64_t n) {
#pragma clang fp contract(off)  // products and sums as written: the threshold theta_c T_i is rounded before the shrink, the
                                // terms of the sum are the ones float64 numpy forms (the shared helpers keep their own mode)
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  const double th = theta[c];
  NoiseSrc ns = ns_;
  if constexpr (NZ == 0) {
    __builtin_assume(ns.noise != nullptr);
    ns.iter_dev = nullptr;
  } else {
    ns.noise = nullptr;
    ns.f64 = (NZ - 1) & 1;
    ns.noise_complex = (NZ - 1) >> 1;
    if (ns.iter_dev) ns.iter += *ns.iter_dev;
    ns.iter_dev = nullptr;
  }
  double acc = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double t = T ? T[i] : Ts;
    const double thr = th * t;
    const double2 w = draw_noise<CPLX>(ns, c, n, i);
    if constexpr (CPLX) {
      const double2 x = reinterpret_cast<const double2*>(X)[base + i];
      const double2 x1 = chain_step_cplx(x, soft_cplx(x, thr), reinterpret_cast<const double2*>(G)[base + i], w, delta, lmda);
      reinterpret_cast<double2*>(X1)[base + i] = x1;
      acc += t * sqrt(abs2_plain(x1.x, x1.y));
    } else {
      const double x = X[base + i];
      const double x1 = chain_step_real(x, soft_real(x, thr), G[base + i], w.x, delta, lmda);
      X1[base + i] = x1;
      acc += t * fabs(x1);
    }
  }
  block_sum<4>(acc);
  if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = acc;
}

struct SapgUpdate {
  double lmda, d, eta_min, eta_max;
  const double* rho_tab;
  int64_t n_rho, n_trace;
  uint64_t iter;
  const uint64_t* iter_dev;
  int pool;
};

// part [C][slices] -> gsum [C] (wave w adds the chains w, w + 16, ... in the fixed order, reduce.h: slice_sum), then one
// thread per chain moves eta and theta
__global__ __launch_bounds__(1024) void k_sapg_update(const double* __restrict__ part, int slices, int C, SapgUpdate u,
                                                      double* __restrict__ gsum, double* __restrict__ theta,
                                                      double* __restrict__ eta, double* __restrict__ trace) {
#pragma clang fp contract(off)  // each operation of the update rounded: the host model reproduces it bit for bit
  __shared__ double pooled;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwave = blockDim.x >> 6;
  for (int c = wave; c < C; c += nwave) {
    double v;
    slice_sum<1>(part + (int64_t)c * slices, slices, lane, v);
    if (lane == 0) gsum[c] = v / u.lmda;
  }
  __syncthreads();
  if (u.pool) {
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int c = 0; c < C; ++c) s += gsum[c];
      pooled = s / (double)C;
    }
    __syncthreads();
  }
  const uint64_t k = u.iter + (u.iter_dev ? *u.iter_dev : 0);
  const double rho = u.rho_tab[k < (uint64_t)u.n_rho ? (int64_t)k : u.n_rho - 1];
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const double g = u.pool ? pooled : gsum[c];
    const double e = fmin(fmax(eta[c] + rho * (u.d - theta[c] * g), u.eta_min), u.eta_max);
    const double th = exp(e);
    eta[c] = e;
    theta[c] = th;
    if (k < (uint64_t)u.n_trace) {
      double* row = trace + ((int64_t)k * C + c) * 3;
      row[0] = th, row[1] = e, row[2] = g;
    }
  }
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int pxm_sapg_step(const void* X, const void* gradg, const double* T, double T_scalar, double delta, double lmda,
                  const void* noise, int noise_complex, uint64_t seed, uint64_t chain0, uint64_t iter,
                  const uint64_t* iter_dev, double* theta, double* eta, double d, const double* rho_table, int64_t n_rho,
                  double eta_min, double eta_max, int pool, double* trace, int64_t n_trace, void* X_out, double* scratch,
                  int64_t n, int C, int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_sapg_step: bad n / C / dtype");
  PXM_REQUIRE(theta && eta && scratch, "pxm_sapg_step: null buffer");
  PXM_REQUIRE(rho_table && n_rho >= 1, "pxm_sapg_step: the step-size table needs at least one entry");
  PXM_REQUIRE(std::isfinite(lmda) && lmda > 0 && std::isfinite(delta) && delta > 0 && std::isfinite(d) && d > 0,
              "pxm_sapg_step: lmda, delta and d must be positive and finite");
  PXM_REQUIRE(eta_min <= eta_max, "pxm_sapg_step: eta_min must not exceed eta_max");  // (false for a NaN bound)
  PXM_REQUIRE(n_trace >= 0 && (trace || n_trace == 0), "pxm_sapg_step: a trace of n_trace > 0 rows needs its array");
  if (int rc = check_noise_arg("pxm_sapg_step", noise_complex, dtype)) return rc;
  if (n > 0) {
    PXM_REQUIRE(X && gradg && X_out, "pxm_sapg_step: null buffer");
    PXM_REQUIRE(X_out != X && X_out != gradg && X_out != noise, "pxm_sapg_step: X_out must not alias an input");
  }
  for (const void* o : {(const void*)theta, (const void*)eta, (const void*)trace, (const void*)scratch}) {
    if (!o) continue;
    PXM_REQUIRE(o != X && o != gradg && o != noise && o != (const void*)T && o != (const void*)rho_table && o != X_out,
                "pxm_sapg_step: an output must not alias an input");
  }
  PXM_REQUIRE(theta != eta && theta != scratch && eta != scratch && trace != theta && trace != eta && trace != scratch,
              "pxm_sapg_step: theta, eta, trace and scratch must be different arrays");
  hipStream_t st = (hipStream_t)stream;
  const int slices = n > 0 ? chain_slices(n, PXM_SAPG_SLICES_MAX) : 0;
  double* gsum = scratch + (int64_t)PXM_SAPG_SLICES_MAX * C;
  if (n > 0) {
    const dim3 g((unsigned)slices, (unsigned)C);
    const NoiseSrc ns = make_noise_src(noise, noise_complex, seed, chain0, iter, iter_dev);
#define PXM_SAPG_LAUNCH(CPLX, NZ)                                                                                           \
  hipLaunchKernelGGL((k_sapg_step<CPLX, NZ>   ), g, dim3(256), 0, st, (const double*)X, (const double*)gradg, T, T_scalar, \
                     (const double*)theta, delta, lmda, ns, (double*)X_out, scratch, n)
    switch (noise ? 0 : 1 + ns.f64 + 2 * ns.noise_complex + (dtype ? 8 : 0)) {  // (complex noise needs a complex state)
      case 0: if (dtype) PXM_SAPG_LAUNCH(true, 0); else PXM_SAPG_LAUNCH(false, 0); break;
      case 1: PXM_SAPG_LAUNCH(false, 1); break;
      case 2: PXM_SAPG_LAUNCH(false, 2); break;
      case 9: PXM_SAPG_LAUNCH(true, 1); break;
      case 10: PXM_SAPG_LAUNCH(true, 2); break;
      case 11: PXM_SAPG_LAUNCH(true, 3); break;
      case 12: PXM_SAPG_LAUNCH(true, 4); break;
      default: PXM_REQUIRE(false, "pxm_sapg_step: complex noise needs a complex state");
    }
#undef PXM_SAPG_LAUNCH
  }
  const SapgUpdate u{lmda, d, eta_min, eta_max, rho_table, n_rho, n_trace, iter, iter_dev, pool ? 1 : 0};
  const int threads = C >= 16 ? 1024 : 64 * C;  // one wave per chain up to 16
  hipLaunchKernelGGL(k_sapg_update, dim3(1), dim3(threads), 0, st, (const double*)scratch, slices, C, u, gsum, theta, eta,
                     trace);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
