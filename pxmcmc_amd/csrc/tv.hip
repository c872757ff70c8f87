// Total variation on the MW grid: the discrete gradient A and its adjoint, the isotropic TV value, the pair form of the dual
// projection, and the two steps of the primal-dual iteration (primal_dual.hip) with the stencil formed in the kernel
// (DESIGN.md section 14e):
//
//   pxm_tv_grad             out = A x                                    x [C][L n] -> out [C][2][L n]
//   pxm_tv_grad_adjoint     out = A^H v                                  the reverse
//   pxm_tv_value            out[c] = sum_i T_i sqrt(|(A x)[0]_i|^2 + |(A x)[1]_i|^2), no coefficient array
//   pxm_pd_dual_step_pairs  pxm_pd_dual_step on [C][2][m] with the projection onto the pair norm
//   pxm_tv_primal_step      pxm_pd_primal_step with U = A^H V formed in the kernel
//   pxm_tv_dual_step        pxm_pd_dual_step_pairs with W = A Xbar formed in the kernel
//
// The stencil and the projection are the inline functions of tv_core.h in every kernel, and the launches share the slice
// rule of primal_dual.hip, so the fused steps equal the composed ones bit for bit, sums included.  As there: no contraction
// besides the explicit fma calls, one element per lane, one workgroup per 256 pixels up to PXM_FISTA_SLICES_MAX and
// grid-stride beyond, per-chain sums through block_sum partials and a one-wave finishing kernel, no atomics, no LDS tiles,
// no host read: a HIP graph replays them.  The neighbour reads (rows t +- 1, columns p +- 1) are served by the caches: per
// complex pixel the fused dual step moves 80 bytes (Xbar in; V in and V1 out, two planes each) against 144 of A Xbar followed by
// the pair step, the fused primal step 96 (X, G, V two planes in; X1, Xbar out) against 128.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "reduce.h"
#include "tv_core.h"

#include <cmath>

namespace pxm {

static inline int tv_slices(int64_t m) { return chain_slices(m, PXM_FISTA_SLICES_MAX); }

#define TV_PIXEL_LOOP(i, m) \
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < (m); i += (int)(gridDim.x * blockDim.x))

template <bool CPLX>
__global__ __launch_bounds__(256) void k_tv_grad(const double* __restrict__ X, const double* __restrict__ ab,
                                                 double* __restrict__ out, int L) {
  using E = typename TvElem<CPLX>::type;
  const int n = 2 * L - 1, m = L * n;
  const E* x = reinterpret_cast<const E*>(X) + (int64_t)blockIdx.y * m;
  E* o = reinterpret_cast<E*>(out) + (int64_t)blockIdx.y * 2 * m;
  TV_PIXEL_LOOP(i, m) {
    const TvPix q = tv_pix(ab, L, n, i);
    E d0, d1;
    tv_grad_at<CPLX>(x, q, L, n, i, d0, d1);
    o[i] = d0;
    o[m + i] = d1;
  }
}

template <bool CPLX>
__global__ __launch_bounds__(256) void k_tv_adj(const double* __restrict__ V, const double* __restrict__ ab,
                                                double* __restrict__ out, int L) {
  using E = typename TvElem<CPLX>::type;
  const int n = 2 * L - 1, m = L * n;
  const E* v0 = reinterpret_cast<const E*>(V) + (int64_t)blockIdx.y * 2 * m;
  E* o = reinterpret_cast<E*>(out) + (int64_t)blockIdx.y * m;
  TV_PIXEL_LOOP(i, m) {
    const TvPix q = tv_pix(ab, L, n, i);
    o[i] = tv_adj_at<CPLX>(v0, v0 + m, q, n, i);
  }
}

template <bool CPLX>
__global__ __launch_bounds__(256) void k_tv_value(const double* __restrict__ X, const double* __restrict__ ab,
                                                  const double* __restrict__ T, double Ts, double* __restrict__ part, int L) {
#pragma clang fp contract(off)
  using E = typename TvElem<CPLX>::type;
  const int n = 2 * L - 1, m = L * n;
  const E* x = reinterpret_cast<const E*>(X) + (int64_t)blockIdx.y * m;
  double tv = 0.0;
  TV_PIXEL_LOOP(i, m) {
    const TvPix q = tv_pix(ab, L, n, i);
    E d0, d1;
    tv_grad_at<CPLX>(x, q, L, n, i, d0, d1);
    tv += (T ? T[i] : Ts) * sqrt(tv_pair2(d0, d1));
  }
  block_sum<4>(tv);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = tv;
}

// W given (pxm_pd_dual_step_pairs: m pixels, ab and L unused) or W = A Xbar formed here (FUSED: XW is Xbar, m = L n)
template <bool CPLX, bool FUSED>
__global__ __launch_bounds__(256) void k_tv_dual(const double* __restrict__ V, const double* __restrict__ XW,
                                                 const double* __restrict__ ab, const double* __restrict__ T, double Ts,
                                                 double sigma, double rscale, double* __restrict__ V1,
                                                 double* __restrict__ part, int L, int m) {
  using E = typename TvElem<CPLX>::type;
  const int n = 2 * L - 1;
  const int c = blockIdx.y;
  const E* v = reinterpret_cast<const E*>(V) + (int64_t)c * 2 * m;
  const E* xw = reinterpret_cast<const E*>(XW) + (int64_t)c * (FUSED ? 1 : 2) * m;
  E* v1 = reinterpret_cast<E*>(V1) + (int64_t)c * 2 * m;
  double dv2 = 0.0, v2 = 0.0, tw = 0.0;
  TV_PIXEL_LOOP(i, m) {
    E wa, wb;
    if constexpr (FUSED) {
      const TvPix q = tv_pix(ab, L, n, i);
      tv_grad_at<CPLX>(xw, q, L, n, i, wa, wb);
    } else {
      wa = xw[i];
      wb = xw[m + i];
    }
    E oa, ob;
    tv_pair_step(v[i], v[m + i], wa, wb, T ? T[i] : Ts, sigma, rscale, oa, ob, dv2, v2, tw);
    v1[i] = oa;
    v1[m + i] = ob;
  }
  block_sum<4>(dv2, v2, tw);
  if (threadIdx.x == 0) {
    double* p = part + ((int64_t)c * gridDim.x + blockIdx.x) * 3;
    p[0] = dv2, p[1] = v2, p[2] = tw;
  }
}

// pxm_pd_primal_step with U = A^H V formed here; G == nullptr: zero; Xbar == nullptr: not written
template <bool CPLX>
__global__ __launch_bounds__(256) void k_tv_primal(const double* __restrict__ X, const double* __restrict__ G,
                                                   const double* __restrict__ V, const double* __restrict__ ab, double tau,
                                                   double* __restrict__ X1, double* __restrict__ Xbar,
                                                   double* __restrict__ part, int L) {
#pragma clang fp contract(off)
  using E = typename TvElem<CPLX>::type;
  const int n = 2 * L - 1, m = L * n;
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * m;
  const E* x = reinterpret_cast<const E*>(X) + base;
  const E* g = G ? reinterpret_cast<const E*>(G) + base : nullptr;
  const E* v0 = reinterpret_cast<const E*>(V) + 2 * base;
  E* x1 = reinterpret_cast<E*>(X1) + base;
  E* xb = Xbar ? reinterpret_cast<E*>(Xbar) + base : nullptr;
  double dx2 = 0.0, x2 = 0.0;
  TV_PIXEL_LOOP(i, m) {
    const TvPix q = tv_pix(ab, L, n, i);
    const E u = tv_adj_at<CPLX>(v0, v0 + m, q, n, i);
    const E xi = x[i];
    const E r = tv_primal(xi, g ? g[i] : TvElem<CPLX>::zero(), u, tau);
    x1[i] = r;
    if (xb) xb[i] = tv_bar(r, xi);
    dx2 += tv_abs2(tv_sub(r, xi));
    x2 += tv_abs2(r);
  }
  block_sum<4>(dx2, x2);
  if (threadIdx.x == 0) {
    double* p = part + ((int64_t)c * gridDim.x + blockIdx.x) * 2;
    p[0] = dx2, p[1] = x2;
  }
}

// sums[c][0..K-1] = the chain's partials added in the fixed order (reduce.h: slice_sum)
template <int K>
__global__ __launch_bounds__(64) void k_tv_finish(const double* __restrict__ part, int slices, double* __restrict__ sums) {
  const int c = blockIdx.x;
  double a, b = 0.0, t = 0.0;
  if constexpr (K == 3) slice_sum<3>(part + (int64_t)c * slices * 3, slices, threadIdx.x, a, b, t);
  else if constexpr (K == 2) slice_sum<2>(part + (int64_t)c * slices * 2, slices, threadIdx.x, a, b);
  else slice_sum<1>(part + (int64_t)c * slices, slices, threadIdx.x, a);
  if (threadIdx.x == 0) {
    sums[c * K + 0] = a;
    if constexpr (K >= 2) sums[c * K + 1] = b;
    if constexpr (K == 3) sums[c * K + 2] = t;
  }
}

// L n as the kernels index it (int, the grid stride included): L >= 2 and L n <= 2^30
static inline bool tv_size_ok(int L) { return L >= 2 && L <= 16384; }

}  // namespace pxm

using namespace pxm;

#define TV_COMMON(fn)                                                                                        \
  hipStream_t st = (hipStream_t)stream;                                                                      \
  PXM_REQUIRE(tv_size_ok(L), fn ": L must be 2 ... 16384");                                                  \
  PXM_REQUIRE(C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), fn ": bad C / dtype");                     \
  const int m = L * (2 * L - 1);                                                                             \
  const dim3 grid((unsigned)tv_slices(m), (unsigned)C);                                                      \
  (void)st;                                                                                                  \
  (void)m;                                                                                                   \
  (void)grid

#define TV_THRESHOLD(fn) PXM_REQUIRE(!(T == nullptr && !(T_scalar >= 0)), fn ": T_scalar must be >= 0")

extern "C" {

int pxm_tv_grad(const void* x, const double* ab, void* out, int L, int C, int dtype, pxm_stream_t stream) {
  TV_COMMON("pxm_tv_grad");
  PXM_REQUIRE(x && ab && out, "pxm_tv_grad: null buffer");
  PXM_REQUIRE(out != x && (const void*)out != (const void*)ab, "pxm_tv_grad: the output must not alias an input");
  const double* xd = (const double*)x;
  if (dtype) hipLaunchKernelGGL(k_tv_grad<true>, grid, dim3(256), 0, st, xd, ab, (double*)out, L);
  else hipLaunchKernelGGL(k_tv_grad<false>, grid, dim3(256), 0, st, xd, ab, (double*)out, L);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_tv_grad_adjoint(const void* v, const double* ab, void* out, int L, int C, int dtype, pxm_stream_t stream) {
  TV_COMMON("pxm_tv_grad_adjoint");
  PXM_REQUIRE(v && ab && out, "pxm_tv_grad_adjoint: null buffer");
  PXM_REQUIRE(out != v && (const void*)out != (const void*)ab, "pxm_tv_grad_adjoint: the output must not alias an input");
  const double* vd = (const double*)v;
  if (dtype) hipLaunchKernelGGL(k_tv_adj<true>, grid, dim3(256), 0, st, vd, ab, (double*)out, L);
  else hipLaunchKernelGGL(k_tv_adj<false>, grid, dim3(256), 0, st, vd, ab, (double*)out, L);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_tv_value(const void* x, const double* ab, const double* T, double T_scalar, double* out, double* scratch, int L, int C,
                 int dtype, pxm_stream_t stream) {
  TV_COMMON("pxm_tv_value");
  TV_THRESHOLD("pxm_tv_value");
  PXM_REQUIRE(x && ab && out && scratch, "pxm_tv_value: null buffer");
  PXM_REQUIRE((const void*)out != x && out != ab && out != T && (const void*)scratch != x && scratch != ab && scratch != T &&
                  out != scratch,
              "pxm_tv_value: out and scratch must not alias an input or each other");
  const double* xd = (const double*)x;
  if (dtype) hipLaunchKernelGGL(k_tv_value<true>, grid, dim3(256), 0, st, xd, ab, T, T_scalar, scratch, L);
  else hipLaunchKernelGGL(k_tv_value<false>, grid, dim3(256), 0, st, xd, ab, T, T_scalar, scratch, L);
  hipLaunchKernelGGL(k_tv_finish<1>, dim3(C), dim3(64), 0, st, scratch, (int)grid.x, out);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_pd_dual_step_pairs(const void* V, const void* W, const double* T, double T_scalar, double sigma, double rscale,
                           void* V1_out, double* sums, double* scratch, int64_t m, int C, int dtype, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  PXM_REQUIRE(m >= 0 && m <= ((int64_t)1 << 30) && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1),
              "pxm_pd_dual_step_pairs: bad m / C / dtype");
  PXM_REQUIRE(std::isfinite(sigma) && sigma > 0, "pxm_pd_dual_step_pairs: sigma must be positive");
  PXM_REQUIRE(rscale > 0 && !(T == nullptr && !(T_scalar >= 0)),
              "pxm_pd_dual_step_pairs: rscale must be positive and T_scalar >= 0");
  PXM_REQUIRE(sums && scratch, "pxm_pd_dual_step_pairs: null buffer");
  int slices = 0;
  if (m > 0) {
    PXM_REQUIRE(V && W && V1_out, "pxm_pd_dual_step_pairs: null buffer");
    PXM_REQUIRE(V1_out != V && V1_out != W && (const void*)V1_out != (const void*)T,
                "pxm_pd_dual_step_pairs: the output must not alias an input");
    slices = tv_slices(m);
    const dim3 g((unsigned)slices, (unsigned)C);
    const double *v = (const double*)V, *w = (const double*)W;
    const double* none = nullptr;
    if (dtype) hipLaunchKernelGGL((k_tv_dual<true, false>), g, dim3(256), 0, st, v, w, none, T, T_scalar, sigma, rscale, (double*)V1_out, scratch, 1, (int)m);
    else hipLaunchKernelGGL((k_tv_dual<false, false>), g, dim3(256), 0, st, v, w, none, T, T_scalar, sigma, rscale, (double*)V1_out, scratch, 1, (int)m);
  }
  hipLaunchKernelGGL(k_tv_finish<3>, dim3(C), dim3(64), 0, st, scratch, slices, sums);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_tv_primal_step(const void* X, const void* G, const void* V, const double* ab, double tau, void* X1_out, void* Xbar_out,
                       double* sums, double* scratch, int L, int C, int dtype, pxm_stream_t stream) {
  TV_COMMON("pxm_tv_primal_step");
  PXM_REQUIRE(std::isfinite(tau) && tau > 0, "pxm_tv_primal_step: tau must be positive");
  PXM_REQUIRE(X && V && ab && X1_out && sums && scratch, "pxm_tv_primal_step: null buffer");
  for (const void* o : {(const void*)X1_out, (const void*)Xbar_out})
    PXM_REQUIRE(o == nullptr || (o != X && o != G && o != V && o != (const void*)ab),
                "pxm_tv_primal_step: an output must not alias an input");
  PXM_REQUIRE(X1_out != Xbar_out, "pxm_tv_primal_step: X1_out and Xbar_out must be different arrays");
  const double *x = (const double*)X, *g = (const double*)G, *v = (const double*)V;
  if (dtype) hipLaunchKernelGGL(k_tv_primal<true>, grid, dim3(256), 0, st, x, g, v, ab, tau, (double*)X1_out, (double*)Xbar_out, scratch, L);
  else hipLaunchKernelGGL(k_tv_primal<false>, grid, dim3(256), 0, st, x, g, v, ab, tau, (double*)X1_out, (double*)Xbar_out, scratch, L);
  hipLaunchKernelGGL(k_tv_finish<2>, dim3(C), dim3(64), 0, st, scratch, (int)grid.x, sums);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_tv_dual_step(const void* V, const void* Xbar, const double* ab, const double* T, double T_scalar, double sigma,
                     double rscale, void* V1_out, double* sums, double* scratch, int L, int C, int dtype, pxm_stream_t stream) {
  TV_COMMON("pxm_tv_dual_step");
  PXM_REQUIRE(std::isfinite(sigma) && sigma > 0, "pxm_tv_dual_step: sigma must be positive");
  PXM_REQUIRE(rscale > 0 && !(T == nullptr && !(T_scalar >= 0)), "pxm_tv_dual_step: rscale must be positive and T_scalar >= 0");
  PXM_REQUIRE(V && Xbar && ab && V1_out && sums && scratch, "pxm_tv_dual_step: null buffer");
  PXM_REQUIRE(V1_out != V && V1_out != Xbar && (const void*)V1_out != (const void*)T && (const void*)V1_out != (const void*)ab,
              "pxm_tv_dual_step: the output must not alias an input");
  const double *v = (const double*)V, *xb = (const double*)Xbar;
  if (dtype) hipLaunchKernelGGL((k_tv_dual<true, true>), grid, dim3(256), 0, st, v, xb, ab, T, T_scalar, sigma, rscale, (double*)V1_out, scratch, L, m);
  else hipLaunchKernelGGL((k_tv_dual<false, true>), grid, dim3(256), 0, st, v, xb, ab, T, T_scalar, sigma, rscale, (double*)V1_out, scratch, L, m);
  hipLaunchKernelGGL(k_tv_finish<3>, dim3(C), dim3(64), 0, st, scratch, (int)grid.x, sums);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
