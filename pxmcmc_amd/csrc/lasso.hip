// The conditional draw of the prior precisions given the field for the L1 (Laplace) prior: the second half of a Gibbs sweep on
// the sparse posterior (Park & Casella 2008; Kyung et al. 2010 for the group form).  The Laplace prior is a
// Gaussian scale mixture, exp(-t |x|) ~ int N(x; 0, v I_m) Gamma(v; (m + 1) / 2, t^2 / 2) dv (m = 1 real, 2 complex), and given
// the field every precision D_i = 1 / v_i is an independent inverse-Gaussian variate,
//
//   D_i | x  ~  IG(mean = t_i / |x_i|, shape = t_i^2),   t_i = tscale T_i,
//
// drawn by the transformation of Michael, Schucany & Haas (1976) written so that nothing cancels and nothing divides by |x|:
//
//   a = |x| / t,  g = z^2 / (2 t^2),  D1 = 1 / (a + g + sqrt(g (g + 2 a))),   D = D1 if u (1 + a D1) <= 1 else 1 / (a^2 D1)
//
// (x = 0: the Levy limit t^2 / z^2, always the first branch).  z is component 0 of the fp64 complex-stream Philox pair at
// counter (i, iter) -- the real part of element i of pxm_randn(n, dtype 1 | PXM_NOISE_F64) -- and u the exact 52-bit uniform
// of the block at counter (i, iter + 1) (philox.h: uniform52_from_bits), for real and complex states alike.
//
// k_lasso_draw is one streaming pass in the style of k_cg_update: one element per lane and pass, one workgroup per 256 elements
// up to PXM_FISTA_SLICES_MAX and grid-stride beyond.  The Philox bits of both blocks are formed first, the Box-Muller step
// runs after them (philox.h).  It reads the state once (16 bytes per complex element, plus 8 of T) and writes D, sqrt(D) and
// M^-1 = 1 / (D + h_c), 24 bytes, with the default cache policy of mem_policy.h: the CG launches read them back at once.
// With sums: per-slice partials of sum t |x| and of the clamped count through block_sum, then k_lasso_finish, one wave per
// chain (slice_sum: a chain's sums depend on n only).  No atomics, no host read, no data-dependent loop.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"
#include "reduce.h"

#include <cmath>

namespace pxm {

static inline int lasso_slices(int64_t n) { return chain_slices(n, PXM_FISTA_SLICES_MAX); }

template <bool CPLX, bool SUMS>
__global__ __launch_bounds__(256) void k_lasso_draw(const double* __restrict__ X, const double* __restrict__ T, double Ts,
                                                    double tscale, const double* __restrict__ H, double Hs, double d_lo,
                                                    double d_hi, uint64_t seed, uint64_t chain0, uint64_t iter,
                                                    double* __restrict__ D, double* __restrict__ sqrtD,
                                                    double* __restrict__ Minv, double* __restrict__ part, int64_t n) {
#pragma clang fp contract(off)  // sums and products as written
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  const uint64_t chain = chain0 + (uint64_t)c;
  const double h = H ? H[c] : Hs;
  double pri = 0.0, ncl = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint4 bz = philox_bits(seed, chain, (uint64_t)i, iter);
    const uint4 bu = philox_bits(seed, chain, (uint64_t)i, iter + 1);
    double ax;
    if constexpr (CPLX) {
      const double2 x = reinterpret_cast<const double2*>(X)[base + i];
      ax = sqrt(abs2_plain(x.x, x.y));
    } else {
      ax = fabs(X[base + i]);
    }
    const double t = tscale * (T ? T[i] : Ts);
    const double z = normal_pair_from_bits(bz).z0;
    const double u = uniform52_from_bits(bu);
    const double rt = 1.0 / t;
    const double a = ax * rt, zt = z * rt;
    const double g = 0.5 * (zt * zt);
    const double d1 = 1.0 / ((a + g) + sqrt(g * (g + 2.0 * a)));
    // (x = 0 and z = 0: d1 = inf and the test is NaN -- the first branch, which the clamp turns into d_hi)
    const double raw = !(u * (1.0 + a * d1) > 1.0) ? d1 : 1.0 / (a * (a * d1));
    const double d = fmin(fmax(raw, d_lo), d_hi);
    D[base + i] = d;
    sqrtD[base + i] = sqrt(d);
    Minv[base + i] = 1.0 / (d + h);
    if constexpr (SUMS) {
      pri += t * ax;
      ncl += d != raw ? 1.0 : 0.0;
    }
  }
  if constexpr (SUMS) {
    block_sum<4>(pri, ncl);
    if (threadIdx.x == 0) {
      double* p = part + ((int64_t)c * gridDim.x + blockIdx.x) * 2;
      p[0] = pri, p[1] = ncl;
    }
  }
}

// One wave per chain, the only writer of the chain's row of sums.
__global__ __launch_bounds__(64) void k_lasso_finish(const double* __restrict__ part, int slices, double* __restrict__ sums) {
#pragma clang fp contract(off)
  const int c = blockIdx.x;
  double pri, ncl;
  slice_sum<2>(part + (int64_t)c * slices * 2, slices, threadIdx.x, pri, ncl);
  if (threadIdx.x == 0) sums[2 * c] = pri, sums[2 * c + 1] = ncl;
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int pxm_lasso_precision_draw(const void* X, const double* T, double T_scalar, double tscale, const double* h, double h_scalar,
                             double d_lo, double d_hi, uint64_t seed, uint64_t chain0, uint64_t iter, double* D, double* sqrtD,
                             double* Minv, double* sums, double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 1 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_lasso_precision_draw: bad n / C / dtype");
  PXM_REQUIRE(X && D && sqrtD && Minv, "pxm_lasso_precision_draw: null buffer");
  PXM_REQUIRE(std::isfinite(tscale) && tscale > 0 && (T || (std::isfinite(T_scalar) && T_scalar > 0)),
              "pxm_lasso_precision_draw: tscale and T must be finite and positive");
  PXM_REQUIRE(std::isfinite(d_lo) && std::isfinite(d_hi) && d_lo > 0 && d_lo <= d_hi,
              "pxm_lasso_precision_draw: the clamp needs finite 0 < d_lo <= d_hi");
  PXM_REQUIRE(h || (std::isfinite(h_scalar) && h_scalar >= 0), "pxm_lasso_precision_draw: h must be finite and not negative");
  PXM_REQUIRE(!sums || scratch, "pxm_lasso_precision_draw: sums need scratch");
  const void* outs[] = {D, sqrtD, Minv, sums, sums ? scratch : nullptr};
  const void* ins[] = {X, T, h};
  for (int a = 0; a < 5; ++a) {
    if (!outs[a]) continue;
    for (int b = a + 1; b < 5; ++b) PXM_REQUIRE(outs[a] != outs[b], "pxm_lasso_precision_draw: the outputs must all be different");
    for (int b = 0; b < 3; ++b) PXM_REQUIRE(outs[a] != ins[b], "pxm_lasso_precision_draw: an output must not alias an input");
  }
  hipStream_t st = (hipStream_t)stream;
  const int slices = lasso_slices(n);
  const dim3 g((unsigned)slices, (unsigned)C);
  const double* x = (const double*)X;
#define PXM_LASSO_LAUNCH(CPLX, SUMS)                                                                                          \
  hipLaunchKernelGGL((k_lasso_draw<CPLX, SUMS>), g, dim3(256), 0, st, x, T, T_scalar, tscale, h, h_scalar, d_lo, d_hi, seed, \
                     chain0, iter, D, sqrtD, Minv, scratch, n)
  if (sums) {
    if (dtype) PXM_LASSO_LAUNCH(true, true);
    else PXM_LASSO_LAUNCH(false, true);
    hipLaunchKernelGGL(k_lasso_finish, dim3(C), dim3(64), 0, st, scratch, slices, sums);
  } else {
    if (dtype) PXM_LASSO_LAUNCH(true, false);
    else PXM_LASSO_LAUNCH(false, false);
  }
#undef PXM_LASSO_LAUNCH
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
