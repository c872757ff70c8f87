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
// one element per lane and pass, no LDS beyond the 96 bytes (128 with restart) of the workgroup sum.
//
// Adaptive (gradient) restart (O'Donoghue & Candes, Found. Comput. Math. 15, 2015), pxm_fista_step_restart: every chain has
// its own momentum index k_c on the device.  The same pass also leaves r_c = sum Re conj(Y_k - X_{k+1}) (X_{k+1} - X_k);
// the finishing kernel sets k_c = 0 when r_c > 0 and k_c + 1 otherwise, so the decision acts on the following step (which
// then runs with beta_0 = 0) and never needs the host.
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
  double dx2, x2, tx, r;
};

// GIVEN: X_{k+1} is the array P (G, T unused; Y only read with RESTART); else X_{k+1} = soft(Y - gamma G, tscale T_i),
// T_i = T[i] or Ts.  RESTART: beta is read at the chain's own momentum index index[c] and a fourth partial,
// r = sum Re conj(Y - X_{k+1}) (X_{k+1} - X_k), is left (4 per slice instead of 3); else at iter + *index (index may be null).
template <bool CPLX, bool GIVEN, bool RESTART>
__global__ __launch_bounds__(256) void k_fista_step(const double* __restrict__ Y, const double* __restrict__ G,
                                                    const double* __restrict__ P, const double* __restrict__ T, double Ts,
                                                    double tscale, const double* __restrict__ X0, double gamma,
                                                    const double* __restrict__ beta_tab, int64_t nbeta, uint64_t iter,
                                                    const uint64_t* __restrict__ index, double* __restrict__ X1,
                                                    double* __restrict__ Y1, double* __restrict__ part, int64_t n) {
#pragma clang fp contract(off)  // products and sums as written (the explicit fma calls stay): the threshold T_i tscale is
                                // rounded before the shrink, the terms of the sums are the ones float64 numpy forms
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  const uint64_t k = RESTART ? index[c] : iter + (index ? *index : 0);
  const double beta = beta_tab[k < (uint64_t)nbeta ? (int64_t)k : nbeta - 1];
  FistaSums acc{0.0, 0.0, 0.0, 0.0};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (CPLX) {
      double2 x1, y;
      if constexpr (!GIVEN || RESTART) y = reinterpret_cast<const double2*>(Y)[base + i];
      if constexpr (GIVEN) {
        x1 = reinterpret_cast<const double2*>(P)[base + i];
      } else {
        const double2 g = reinterpret_cast<const double2*>(G)[base + i];
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
      if constexpr (RESTART) acc.r += (y.x - x1.x) * d.x + (y.y - x1.y) * d.y;
    } else {
      double x1, y;
      if constexpr (!GIVEN || RESTART) y = Y[base + i];
      if constexpr (GIVEN) x1 = P[base + i];
      else x1 = soft_real(fma(-gamma, G[base + i], y), (T ? T[i] : Ts) * tscale);
      const double d = x1 - X0[base + i];
      X1[base + i] = x1;
      Y1[base + i] = fma(beta, d, x1);
      acc.dx2 += d * d;
      acc.x2 += x1 * x1;
      if constexpr (!GIVEN) acc.tx += (T ? T[i] : Ts) * fabs(x1);
      if constexpr (RESTART) acc.r += (y - x1) * d;
    }
  }
  if constexpr (RESTART) block_sum<4>(acc.dx2, acc.x2, acc.tx, acc.r);
  else block_sum<4>(acc.dx2, acc.x2, acc.tx);
  if (threadIdx.x == 0) {
    constexpr int K = RESTART ? 4 : 3;
    double* p = part + ((int64_t)c * gridDim.x + blockIdx.x) * K;
    p[0] = acc.dx2, p[1] = acc.x2, p[2] = acc.tx;
    if constexpr (RESTART) p[3] = acc.r;
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

// The restarted step's finish: sums[c][0..3], then the decision between two steps -- r > 0 (false for 0 and for NaN) sends
// the chain's momentum index back to 0 and counts a restart, anything else advances the index.  One wave per chain, which
// is the only writer of the chain's index; the step kernel that read it ran before in the same stream.
__global__ __launch_bounds__(64) void k_fista_finish_restart(const double* __restrict__ part, int slices, int has_f,
                                                             int restart_on, double* __restrict__ sums,
                                                             uint64_t* __restrict__ index, uint64_t* __restrict__ restarts) {
  const int c = blockIdx.x;
  FistaSums v;
  slice_sum<4>(part + (int64_t)c * slices * 4, slices, threadIdx.x, v.dx2, v.x2, v.tx, v.r);
  if (threadIdx.x == 0) {
    sums[c * 4 + 0] = v.dx2;
    sums[c * 4 + 1] = v.x2;
    sums[c * 4 + 2] = has_f ? v.tx : __builtin_nan("");
    sums[c * 4 + 3] = v.r;
    const bool restart = restart_on && v.r > 0.0;
    index[c] = restart ? 0 : index[c] + 1;
    if (restart && restarts) restarts[c] += 1;
  }
}

}  // namespace pxm

using namespace pxm;

// Both entry points: the checks, the step launch and the finishing launch.  index == the shared counter (may be null) of
// pxm_fista_step with restart_on < 0, or the per-chain momentum indices of pxm_fista_step_restart with restart_on 0 / 1.
static int fista_launch(const void* Y, const void* gradg, const void* proxf, const double* T, double T_scalar,
                        const void* X_prev, double gamma, double lmda, const double* beta_table, int64_t n_beta, uint64_t iter,
                        uint64_t* index, uint64_t* restarts, int restart_on, void* X_out, void* Y_out, double* sums,
                        double* scratch, int64_t n, int C, int dtype, hipStream_t st) {
  const bool rs = restart_on >= 0;
  PXM_REQUIRE(n >= 0 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_fista_step: bad n / C / dtype");
  PXM_REQUIRE(beta_table && n_beta >= 1, "pxm_fista_step: the momentum table needs at least one entry");
  PXM_REQUIRE(std::isfinite(gamma) && gamma > 0 && std::isfinite(lmda) && lmda > 0, "pxm_fista_step: gamma and lmda must be positive");
  PXM_REQUIRE(sums && scratch, "pxm_fista_step: null buffer");
  if (rs) {
    PXM_REQUIRE(index, "pxm_fista_step_restart: null momentum_index");
    PXM_REQUIRE((const void*)index != (const void*)restarts && (const void*)index != (const void*)sums &&
                    (const void*)restarts != (const void*)sums,
                "pxm_fista_step_restart: momentum_index, restarts and sums must be different arrays");
  }
  const int has_f = proxf ? 0 : 1;
  int slices = 0;
  if (n > 0) {
    PXM_REQUIRE(X_prev && X_out && Y_out, "pxm_fista_step: null buffer");
    PXM_REQUIRE(proxf || (Y && gradg), "pxm_fista_step: Y and gradg are needed unless proxf is given");
    PXM_REQUIRE(!rs || Y, "pxm_fista_step_restart: Y is needed with a given proxf too (the restart sum reads it)");
    for (const void* o : {(const void*)X_out, (const void*)Y_out})
      PXM_REQUIRE(o != Y && o != gradg && o != proxf && o != X_prev, "pxm_fista_step: an output must not alias an input");
    PXM_REQUIRE(X_out != Y_out, "pxm_fista_step: X_out and Y_out must be different arrays");
    slices = fista_slices(n);
    const dim3 g((unsigned)slices, (unsigned)C);
    const double tscale = gamma / lmda;
    const double *y = (const double*)Y, *gr = (const double*)gradg, *p = (const double*)proxf, *x0 = (const double*)X_prev;
    double *x1 = (double*)X_out, *y1 = (double*)Y_out;
#define PXM_FISTA_LAUNCH(CPLX, GIVEN, RESTART)                                                                           \
  hipLaunchKernelGGL((k_fista_step<CPLX, GIVEN, RESTART>), g, dim3(256), 0, st, y, gr, p, T, T_scalar, tscale, x0, gamma, \
                     beta_table, n_beta, iter, (const uint64_t*)index, x1, y1, scratch, n)
#define PXM_FISTA_FORMS(RESTART)                                   \
  do {                                                             \
    if (dtype && proxf) PXM_FISTA_LAUNCH(true, true, RESTART);     \
    else if (dtype) PXM_FISTA_LAUNCH(true, false, RESTART);        \
    else if (proxf) PXM_FISTA_LAUNCH(false, true, RESTART);        \
    else PXM_FISTA_LAUNCH(false, false, RESTART);                  \
  } while (0)
    if (rs) PXM_FISTA_FORMS(true);
    else PXM_FISTA_FORMS(false);
#undef PXM_FISTA_FORMS
#undef PXM_FISTA_LAUNCH
  }
  // n == 0: nothing to step, no slices: the sums are zero (NaN for the prior sum of a given prox), never left unwritten, and
  // the momentum indices advance
  if (rs) hipLaunchKernelGGL(k_fista_finish_restart, dim3(C), dim3(64), 0, st, scratch, slices, has_f, restart_on, sums, index, restarts);
  else hipLaunchKernelGGL(k_fista_finish, dim3(C), dim3(64), 0, st, scratch, slices, has_f, sums);
  PXM_HIP(hipGetLastError());
  return 0;
}

extern "C" {

int pxm_fista_step(const void* Y, const void* gradg, const void* proxf, const double* T, double T_scalar, const void* X_prev,
                   double gamma, double lmda, const double* beta_table, int64_t n_beta, uint64_t iter,
                   const uint64_t* iter_dev, void* X_out, void* Y_out, double* sums, double* scratch, int64_t n, int C,
                   int dtype, pxm_stream_t stream) {
  return fista_launch(Y, gradg, proxf, T, T_scalar, X_prev, gamma, lmda, beta_table, n_beta, iter, const_cast<uint64_t*>(iter_dev),
                      nullptr, -1, X_out, Y_out, sums, scratch, n, C, dtype, (hipStream_t)stream);
}

int pxm_fista_step_restart(const void* Y, const void* gradg, const void* proxf, const double* T, double T_scalar,
                           const void* X_prev, double gamma, double lmda, const double* beta_table, int64_t n_beta,
                           uint64_t* momentum_index, uint64_t* restarts, int restart_on, void* X_out, void* Y_out, double* sums,
                           double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream) {
  return fista_launch(Y, gradg, proxf, T, T_scalar, X_prev, gamma, lmda, beta_table, n_beta, 0, momentum_index, restarts,
                      restart_on ? 1 : 0, X_out, Y_out, sums, scratch, n, C, dtype, (hipStream_t)stream);
}

}  // extern "C"
