// One FISTA iteration (Beck & Teboulle, SIAM J. Imaging Sci. 2(1), 2009) on the posterior of the samplers, per element of
// every chain:
//
//   V       = Y - gamma gradg(Y)
//   X_{k+1} = soft(V, T gamma / lmda)            (or a given proxf(V) array: analysis setting / user prior)
//   Y_{k+1} = X_{k+1} + beta_k (X_{k+1} - X_k)
//
// f(X) = (1 / lmda) sum_i T_i |X_i| is the potential whose prox MYULA's drift uses (pxmcmc/prior.py:49-50 with the
// threshold T = lmda mu w), so prox_{gamma f} is the soft threshold at gamma T / lmda.  beta_k is read on the device from a
// table indexed by iter + *iter_dev (clamped to the table), so a captured graph replays with the right momentum.
//
// Per chain the launch also leaves sum |X_{k+1} - X_k|^2, sum |X_{k+1}|^2 and sum T_i |X_{k+1,i}|: every workgroup writes
// one partial of each (plain products and sums, no contraction: the terms are the ones float64 numpy forms), a second
// kernel adds the partials in a fixed order.  The number of workgroups per chain depends on n only, so a chain's sums do
// not depend on its batch.  The step itself is a pure stream like k_skrock_stage: 16-byte loads per complex128 element,
// one element per lane and pass, no LDS beyond the 96 bytes of the workgroup sum.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"
#include "reduce.h"

#include <algorithm>
#include <cmath>

namespace pxm {

// workgroups (slices) per chain: one per 256 elements up to PXM_FISTA_SLICES_MAX, grid-stride beyond
static inline int fista_slices(int64_t n) { return chain_slices(n, PXM_FISTA_SLICES_MAX); }

struct FistaSums {
  double dx2, x2, tx;
};

// GIVEN: X_{k+1} is the array P (Y, G, T unused); else X_{k+1} = soft(Y - gamma G, tscale T_i), T_i = T[i] or Ts
template <bool CPLX, bool GIVEN>
__global__ __launch_bounds__(256) void k_fista_step(const double* __restrict__ Y, const double* __restrict__ G,
                                                    const double* __restrict__ P, const double* __restrict__ T, double Ts,
                                                    double tscale, const double* __restrict__ X0, double gamma,
                                                    const double* __restrict__ beta_tab, int64_t nbeta, uint64_t iter,
                                                    const uint64_t* __restrict__ iter_dev, double* __restrict__ X1,
                                                    double* __restrict__ Y1, double* __restrict__ part, int64_t n) {
#pragma clang fp contract(off)  // products and sums as written (the explicit fma calls stay): the threshold T_i tscale is
                                // rounded before the shrink, the terms of the sums are the ones float64 numpy forms
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  const uint64_t k = iter + (iter_dev ? *iter_dev : 0);
  const double beta = beta_tab[k < (uint64_t)nbeta ? (int64_t)k : nbeta - 1];
  FistaSums acc{0.0, 0.0, 0.0};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (CPLX) {
      double2 x1;
      if constexpr (GIVEN) {
        x1 = reinterpret_cast<const double2*>(P)[base + i];
      } else {
        const double2 y = reinterpret_cast<const double2*>(Y)[base + i], g = reinterpret_cast<const double2*>(G)[base + i];
        x1 = soft_cplx(double2{fma(-gamma, g.x, y.x), fma(-gamma, g.y, y.y)}, (T ? T[i] : Ts) * tscale);
      }
      const double2 x0 = reinterpret_cast<const double2*>(X0)[base + i];
      const double2 d{x1.x - x0.x, x1.y - x0.y};
      reinterpret_cast<double2*>(X1)[base + i] = x1;
      reinterpret_cast<double2*>(Y1)[base + i] = double2{fma(beta, d.x, x1.x), fma(beta, d.y, x1.y)};
      const double a2 = abs2_plain(x1.x, x1.y);
      acc.dx2 += abs2_plain(d.x, d.y);
      acc.x2 += a2;
      if constexpr (!GIVEN) acc.tx += (T ? T[i] : Ts) * sqrt(a2);
    } else {
      double x1;
      if constexpr (GIVEN) x1 = P[base + i];
      else x1 = soft_real(fma(-gamma, G[base + i], Y[base + i]), (T ? T[i] : Ts) * tscale);
      const double d = x1 - X0[base + i];
      X1[base + i] = x1;
      Y1[base + i] = fma(beta, d, x1);
      acc.dx2 += d * d;
      acc.x2 += x1 * x1;
      if constexpr (!GIVEN) acc.tx += (T ? T[i] : Ts) * fabs(x1);
    }
  }
  block_sum<4>(acc.dx2, acc.x2, acc.tx);
  if (threadIdx.x == 0) {
    double* p = part + ((int64_t)c * gridDim.x + blockIdx.x) * 3;
    p[0] = acc.dx2, p[1] = acc.x2, p[2] = acc.tx;
  }
}

// sums[c][0..2] = the chain's partials added in the fixed order (reduce.h: slice_sum); the third sum is NaN when the launch
// did not form it (given prox)
__global__ __launch_bounds__(64) void k_fista_finish(const double* __restrict__ part, int slices, int has_f,
                                                     double* __restrict__ sums) {
  const int c = blockIdx.x;
  FistaSums v;
  slice_sum<3>(part + (int64_t)c * slices * 3, slices, threadIdx.x, v.dx2, v.x2, v.tx);
  if (threadIdx.x == 0) {
    sums[c * 3 + 0] = v.dx2;
    sums[c * 3 + 1] = v.x2;
    sums[c * 3 + 2] = has_f ? v.tx : __builtin_nan("");
  }
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int pxm_fista_step(const void* Y, const void* gradg, const void* proxf, const double* T, double T_scalar, const void* X_prev,
                   double gamma, double lmda, const double* beta_table, int64_t n_beta, uint64_t iter,
                   const uint64_t* iter_dev, void* X_out, void* Y_out, double* sums, double* scratch, int64_t n, int C,
                   int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_fista_step: bad n / C / dtype");
  PXM_REQUIRE(beta_table && n_beta >= 1, "pxm_fista_step: the momentum table needs at least one entry");
  PXM_REQUIRE(std::isfinite(gamma) && gamma > 0 && std::isfinite(lmda) && lmda > 0, "pxm_fista_step: gamma and lmda must be positive");
  PXM_REQUIRE(sums && scratch, "pxm_fista_step: null buffer");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {  // nothing to step: the sums are zero (NaN for the prior sum of a given prox), never left unwritten
    hipLaunchKernelGGL(k_fista_finish, dim3(C), dim3(64), 0, st, scratch, 0, proxf ? 0 : 1, sums);
    PXM_HIP(hipGetLastError());
    return 0;
  }
  PXM_REQUIRE(X_prev && X_out && Y_out, "pxm_fista_step: null buffer");
  PXM_REQUIRE(proxf || (Y && gradg), "pxm_fista_step: Y and gradg are needed unless proxf is given");
  for (const void* o : {(const void*)X_out, (const void*)Y_out})
    PXM_REQUIRE(o != Y && o != gradg && o != proxf && o != X_prev, "pxm_fista_step: an output must not alias an input");
  PXM_REQUIRE(X_out != Y_out, "pxm_fista_step: X_out and Y_out must be different arrays");
  const int slices = fista_slices(n);
  const dim3 g((unsigned)slices, (unsigned)C);
  const double tscale = gamma / lmda;
  const double *y = (const double*)Y, *gr = (const double*)gradg, *p = (const double*)proxf, *x0 = (const double*)X_prev;
  double *x1 = (double*)X_out, *y1 = (double*)Y_out;
#define PXM_FISTA_LAUNCH(CPLX, GIVEN)                                                                                    \
  hipLaunchKernelGGL((k_fista_step<CPLX, GIVEN>), g, dim3(256), 0, st, y, gr, p, T, T_scalar, tscale, x0, gamma,          \
                     beta_table, n_beta, iter, iter_dev, x1, y1, scratch, n)
  if (dtype && proxf) PXM_FISTA_LAUNCH(true, true);
  else if (dtype) PXM_FISTA_LAUNCH(true, false);
  else if (proxf) PXM_FISTA_LAUNCH(false, true);
  else PXM_FISTA_LAUNCH(false, false);
#undef PXM_FISTA_LAUNCH
  hipLaunchKernelGGL(k_fista_finish, dim3(C), dim3(64), 0, st, scratch, slices, proxf ? 0 : 1, sums);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
