// The two elementwise steps of the forward-backward primal-dual iteration (Condat, J. Optim. Theory Appl. 158, 2013; Vu, Adv.
// Comput. Math. 38, 2013) on the analysis-setting posterior g(x) + h(A x), g = 1/2 Re L2, h(u) = (1 / lmda) sum_i T_i |u_i|:
//
//   x1   = x - tau (gradg(x) + A^H v)                      pxm_pd_primal_step, G = gradg(x), U = A^H v
//   xbar = 2 x1 - x
//   v1   = proj_{|v_i| <= T_i / lmda}(v + sigma A xbar)    pxm_pd_dual_step, W = A xbar, rscale = 1 / lmda
//
// The projection is the prox of sigma h^* whatever sigma is (h^* is the indicator of the box / of the discs).  With
// rscale = 1 the dual step is also the projection of the exact analysis prox's dual iteration (optim.analysis_prox).
//
// Both follow fista.hip: no contraction besides the explicit fma calls, one double2 per lane and pass, one workgroup per
// 256 elements up to PXM_FISTA_SLICES_MAX and grid-stride beyond, per-chain sums through block_sum partials and a one-wave
// finishing kernel (reduce.h), so a chain's sums depend on n only.  No atomics, no host read: a HIP graph replays them.
// Pure streams: per complex element the primal step moves 80 bytes (X, G, U in; X1, Xbar out), the dual step 56 (V, W in;
// V1 out) plus 8 of a vector T.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"
#include "reduce.h"

#include <cmath>

namespace pxm {

static inline int pd_slices(int64_t n) { return chain_slices(n, PXM_FISTA_SLICES_MAX); }

template <bool CPLX>
__global__ __launch_bounds__(256) void k_pd_primal(const double* __restrict__ X, const double* __restrict__ G,
                                                   const double* __restrict__ U, double tau, double* __restrict__ X1,
                                                   double* __restrict__ Xbar, double* __restrict__ part, int64_t n) {
#pragma clang fp contract(off)  // sums and products as written; the fma calls stay
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  double dx2 = 0.0, x2 = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (CPLX) {
      const double2 x = reinterpret_cast<const double2*>(X)[base + i];
      const double2 g = reinterpret_cast<const double2*>(G)[base + i];
      const double2 u = reinterpret_cast<const double2*>(U)[base + i];
      const double2 x1{fma(-tau, g.x + u.x, x.x), fma(-tau, g.y + u.y, x.y)};
      reinterpret_cast<double2*>(X1)[base + i] = x1;
      reinterpret_cast<double2*>(Xbar)[base + i] = double2{fma(2.0, x1.x, -x.x), fma(2.0, x1.y, -x.y)};
      dx2 += abs2_plain(x1.x - x.x, x1.y - x.y);
      x2 += abs2_plain(x1.x, x1.y);
    } else {
      const double x = X[base + i];
      const double x1 = fma(-tau, G[base + i] + U[base + i], x);
      X1[base + i] = x1;
      Xbar[base + i] = fma(2.0, x1, -x);
      const double d = x1 - x;
      dx2 += d * d;
      x2 += x1 * x1;
    }
  }
  block_sum<4>(dx2, x2);
  if (threadIdx.x == 0) {
    double* p = part + ((int64_t)c * gridDim.x + blockIdx.x) * 2;
    p[0] = dx2, p[1] = x2;
  }
}

// T_i = T[i] or Ts; r_i = T_i rscale, rounded once
template <bool CPLX>
__global__ __launch_bounds__(256) void k_pd_dual(const double* __restrict__ V, const double* __restrict__ W,
                                                 const double* __restrict__ T, double Ts, double sigma, double rscale,
                                                 double* __restrict__ V1, double* __restrict__ part, int64_t n) {
#pragma clang fp contract(off)
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  double dv2 = 0.0, v2 = 0.0, tw = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double t = T ? T[i] : Ts;
    const double r = t * rscale;
    if constexpr (CPLX) {
      const double2 v = reinterpret_cast<const double2*>(V)[base + i];
      const double2 wa = reinterpret_cast<const double2*>(W)[base + i];
      const double2 w{fma(sigma, wa.x, v.x), fma(sigma, wa.y, v.y)};
      const double a = sqrt(abs2_plain(w.x, w.y));
      double2 v1 = w;
      if (a > r) {  // a > r >= 0, so a > 0; a == 0 keeps w; r == 0 gives w * 0
        const double s = r / a;
        v1 = double2{w.x * s, w.y * s};
      }
      reinterpret_cast<double2*>(V1)[base + i] = v1;
      dv2 += abs2_plain(v1.x - v.x, v1.y - v.y);
      v2 += abs2_plain(v1.x, v1.y);
      tw += t * sqrt(abs2_plain(wa.x, wa.y));
    } else {
      const double v = V[base + i], wa = W[base + i];
      const double w = fma(sigma, wa, v);
      const double v1 = w > r ? r : (w < -r ? -r : w);
      V1[base + i] = v1;
      const double d = v1 - v;
      dv2 += d * d;
      v2 += v1 * v1;
      tw += t * fabs(wa);
    }
  }
  block_sum<4>(dv2, v2, tw);
  if (threadIdx.x == 0) {
    double* p = part + ((int64_t)c * gridDim.x + blockIdx.x) * 3;
    p[0] = dv2, p[1] = v2, p[2] = tw;
  }
}

// sums[c][0..K-1] = the chain's partials added in the fixed order (reduce.h: slice_sum); no slices (n == 0): zeros
template <int K>
__global__ __launch_bounds__(64) void k_pd_finish(const double* __restrict__ part, int slices, double* __restrict__ sums) {
  const int c = blockIdx.x;
  double a, b, t = 0.0;
  if constexpr (K == 3) slice_sum<3>(part + (int64_t)c * slices * 3, slices, threadIdx.x, a, b, t);
  else slice_sum<2>(part + (int64_t)c * slices * 2, slices, threadIdx.x, a, b);
  if (threadIdx.x == 0) {
    sums[c * K + 0] = a;
    sums[c * K + 1] = b;
    if constexpr (K == 3) sums[c * K + 2] = t;
  }
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int pxm_pd_primal_step(const void* X, const void* G, const void* U, double tau, void* X1_out, void* Xbar_out, double* sums,
                       double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  PXM_REQUIRE(n >= 0 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_pd_primal_step: bad n / C / dtype");
  PXM_REQUIRE(std::isfinite(tau) && tau > 0, "pxm_pd_primal_step: tau must be positive");
  PXM_REQUIRE(sums && scratch, "pxm_pd_primal_step: null buffer");
  int slices = 0;
  if (n > 0) {
    PXM_REQUIRE(X && G && U && X1_out && Xbar_out, "pxm_pd_primal_step: null buffer");
    for (const void* o : {(const void*)X1_out, (const void*)Xbar_out})
      PXM_REQUIRE(o != X && o != G && o != U, "pxm_pd_primal_step: an output must not alias an input");
    PXM_REQUIRE(X1_out != Xbar_out, "pxm_pd_primal_step: X1_out and Xbar_out must be different arrays");
    slices = pd_slices(n);
    const dim3 g((unsigned)slices, (unsigned)C);
    const double *x = (const double*)X, *gr = (const double*)G, *u = (const double*)U;
    if (dtype) hipLaunchKernelGGL(k_pd_primal<true>, g, dim3(256), 0, st, x, gr, u, tau, (double*)X1_out, (double*)Xbar_out, scratch, n);
    else hipLaunchKernelGGL(k_pd_primal<false>, g, dim3(256), 0, st, x, gr, u, tau, (double*)X1_out, (double*)Xbar_out, scratch, n);
  }
  hipLaunchKernelGGL(k_pd_finish<2>, dim3(C), dim3(64), 0, st, scratch, slices, sums);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_pd_dual_step(const void* V, const void* W, const double* T, double T_scalar, double sigma, double rscale, void* V1_out,
                     double* sums, double* scratch, int64_t m, int C, int dtype, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  PXM_REQUIRE(m >= 0 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_pd_dual_step: bad m / C / dtype");
  PXM_REQUIRE(std::isfinite(sigma) && sigma > 0, "pxm_pd_dual_step: sigma must be positive");
  PXM_REQUIRE(rscale > 0 && !(T == nullptr && !(T_scalar >= 0)), "pxm_pd_dual_step: rscale must be positive and T_scalar >= 0");
  PXM_REQUIRE(sums && scratch, "pxm_pd_dual_step: null buffer");
  int slices = 0;
  if (m > 0) {
    PXM_REQUIRE(V && W && V1_out, "pxm_pd_dual_step: null buffer");
    PXM_REQUIRE(V1_out != V && V1_out != W && (const void*)V1_out != (const void*)T,
                "pxm_pd_dual_step: the output must not alias an input");
    slices = pd_slices(m);
    const dim3 g((unsigned)slices, (unsigned)C);
    const double *v = (const double*)V, *w = (const double*)W;
    if (dtype) hipLaunchKernelGGL(k_pd_dual<true>, g, dim3(256), 0, st, v, w, T, T_scalar, sigma, rscale, (double*)V1_out, scratch, m);
    else hipLaunchKernelGGL(k_pd_dual<false>, g, dim3(256), 0, st, v, w, T, T_scalar, sigma, rscale, (double*)V1_out, scratch, m);
  }
  hipLaunchKernelGGL(k_pd_finish<3>, dim3(C), dim3(64), 0, st, scratch, slices, sums);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
