// The Gaussian posterior: preconditioned conjugate gradients on H x = b, H = D + A, per chain of a batch.  D = (T / lmda) p is
// the prior precision (a vector shared by the chains, one row per chain, or a scalar) and A the linear part of x -> calc_gradg(forward(x)), which
// the operators apply between the two launches below.  The iteration is the single-reduction PCG of Chronopoulos & Gear (J.
// Comput. Appl. Math. 25, 1989): all three inner products of an iteration are taken in one pass, so one iteration is one
// operator pair and two launches,
//
//   u = M^-1 r;  q = calc_gradg(forward(u))          (q = A u - b0, b0 = -calc_gradg(forward(0)))
//   pxm_cg_apply:   w = D u + (q + b0);  per chain gamma = sum Re conj(r) u,  delta = sum Re conj(u) w,  rho = sum |r|^2,
//                   then one wave per chain decides: frozen, or rho <= tol^2 ||b||^2 -> alpha = beta = 0 and the chain is
//                   frozen; else beta = gamma / gamma_old (0 on the first iteration), denom = delta - beta gamma / alpha_old,
//                   denom not > 0 or gamma, delta not finite -> frozen with the breakdown flag; else alpha = gamma / denom
//   pxm_cg_update:  p = u + beta p;  s = w + beta s;  x_dst = x_src + alpha p;  r -= alpha s;  u = M^-1 r
//
// H is Hermitian positive definite, so every per-chain scalar is real.  The scalars live in coef [C][PXM_CG_COEF] on the
// device; the host reads them only at a check, and a captured graph replays the iteration.  A frozen chain is copied
// x_src -> x_dst and nothing else of it is read or written.
//
// Both launches follow fista.hip: no contraction besides the explicit fma calls, one double2 per lane and pass, one workgroup
// per 256 elements up to PXM_FISTA_SLICES_MAX and grid-stride beyond, per-chain sums through block_sum partials and a one-wave
// finishing kernel (reduce.h), so a chain's sums depend on n only.  No atomics, no host read.  Pure streams: per complex
// element pxm_cg_apply moves 64 bytes (u, q, r in; w out) plus 8 + 16 of D and b0, pxm_cg_update 176 (u, w, p, s, x, r in;
// p, s, x, r, u out) plus 8 of M^-1.  At the sizes the solver runs at every array stays in the
// Infinity Cache between its write and its next read (w: the next launch; the rest: the next iteration), so every stream
// keeps the default cache policy of mem_policy.h.
//
// Also here: the prox of the Gaussian prior (pxm_gauss_prox) and the helper that assembles right-hand sides (pxm_cg_rhs).
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"
#include "reduce.h"

#include <cmath>

namespace pxm {

static inline int cg_slices(int64_t n) { return chain_slices(n, PXM_FISTA_SLICES_MAX); }

// entries of a chain's row of coef
enum CgCoef { CG_ALPHA = 0, CG_BETA, CG_GAMMA_OLD, CG_ALPHA_OLD, CG_RHO, CG_BNORM2, CG_FLAGS, CG_ITERS };
static_assert(CG_ITERS + 1 == PXM_CG_COEF, "coef row");

// w = fma(D_i, u, q + b0) per component (the sum q + b0 rounded first); partials (gamma, delta, rho) per slice.  A frozen
// chain's workgroups return at once: its partials are not written and the finishing kernel does not read them.
template <bool CPLX>
__global__ __launch_bounds__(256) void k_cg_apply(const double* __restrict__ U, const double* __restrict__ Q,
                                                  const double* __restrict__ B0, const double* __restrict__ D, double Ds,
                                                  int64_t Dst, const double* __restrict__ R, double* __restrict__ W,
                                                  const double* __restrict__ coef, double* __restrict__ part, int64_t n) {
#pragma clang fp contract(off)  // sums and products as written; the fma calls stay
  const int c = blockIdx.y;
  if (coef[c * PXM_CG_COEF + CG_FLAGS] != 0.0) return;
  const int64_t base = (int64_t)c * n;
  double gam = 0.0, del = 0.0, rho = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double d = D ? D[c * Dst + i] : Ds;
    if constexpr (CPLX) {
      const double2 u = reinterpret_cast<const double2*>(U)[base + i];
      const double2 q = reinterpret_cast<const double2*>(Q)[base + i];
      const double2 r = reinterpret_cast<const double2*>(R)[base + i];
      const double2 b = B0 ? reinterpret_cast<const double2*>(B0)[i] : double2{0.0, 0.0};
      const double2 w{fma(d, u.x, q.x + b.x), fma(d, u.y, q.y + b.y)};
      reinterpret_cast<double2*>(W)[base + i] = w;
      gam += r.x * u.x + r.y * u.y;
      del += u.x * w.x + u.y * w.y;
      rho += abs2_plain(r.x, r.y);
    } else {
      const double u = U[base + i], r = R[base + i];
      const double w = fma(d, u, Q[base + i] + (B0 ? B0[i] : 0.0));
      W[base + i] = w;
      gam += r * u;
      del += u * w;
      rho += r * r;
    }
  }
  block_sum<4>(gam, del, rho);
  if (threadIdx.x == 0) {
    double* p = part + ((int64_t)c * gridDim.x + blockIdx.x) * 3;
    p[0] = gam, p[1] = del, p[2] = rho;
  }
}

// One wave per chain, the only writer of the chain's row of coef: the sums in the fixed order (reduce.h: slice_sum), then the
// step lengths, the convergence freeze and the breakdown guard.  No slices (n == 0): the sums are zero and the chain freezes.
__global__ __launch_bounds__(64) void k_cg_finish(const double* __restrict__ part, int slices, double tol2,
                                                  double* __restrict__ coef) {
#pragma clang fp contract(off)
  const int c = blockIdx.x;
  double* k = coef + c * PXM_CG_COEF;
  if (k[CG_FLAGS] != 0.0) {  // (uniform over the wave: one word)
    if (threadIdx.x == 0) k[CG_ALPHA] = k[CG_BETA] = 0.0;
    return;
  }
  double gam, del, rho;
  slice_sum<3>(part + (int64_t)c * slices * 3, slices, threadIdx.x, gam, del, rho);
  if (threadIdx.x != 0) return;
  k[CG_RHO] = rho;
  if (rho <= tol2 * k[CG_BNORM2]) {
    k[CG_ALPHA] = k[CG_BETA] = 0.0;
    k[CG_FLAGS] = (double)PXM_CG_FROZEN;
    return;
  }
  const bool first = k[CG_ITERS] == 0.0;
  const double beta = first ? 0.0 : gam / k[CG_GAMMA_OLD];
  const double denom = first ? del : del - beta * gam / k[CG_ALPHA_OLD];
  if (!(denom > 0.0) || !isfinite(gam) || !isfinite(del)) {
    k[CG_ALPHA] = k[CG_BETA] = 0.0;
    k[CG_FLAGS] = (double)(PXM_CG_FROZEN | PXM_CG_BREAKDOWN);
    return;
  }
  const double alpha = gam / denom;
  k[CG_ALPHA] = alpha, k[CG_BETA] = beta;
  k[CG_GAMMA_OLD] = gam, k[CG_ALPHA_OLD] = alpha;
  k[CG_ITERS] += 1.0;
}

// p = fma(beta, p, u); s = fma(beta, s, w); x_dst = fma(alpha, p, x_src); r = fma(-alpha, s, r); u = M^-1_i r, per
// component, every array but x in place (each element is read and written by one lane).  Frozen chain: x_dst = x_src only.
template <bool CPLX>
__global__ __launch_bounds__(256) void k_cg_update(double* __restrict__ U, const double* __restrict__ W, double* __restrict__ P,
                                                   double* __restrict__ S, const double* __restrict__ X0,
                                                   double* __restrict__ X1, double* __restrict__ R,
                                                   const double* __restrict__ Minv, double Ms, int64_t Mst,
                                                   const double* __restrict__ coef, int64_t n) {
#pragma clang fp contract(off)
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  const double* k = coef + c * PXM_CG_COEF;
  const bool frozen = k[CG_FLAGS] != 0.0;
  const double alpha = k[CG_ALPHA], beta = k[CG_BETA];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if constexpr (CPLX) {
      if (frozen) {
        reinterpret_cast<double2*>(X1)[base + i] = reinterpret_cast<const double2*>(X0)[base + i];
        continue;
      }
      const double m = Minv ? Minv[c * Mst + i] : Ms;
      const double2 u = reinterpret_cast<double2*>(U)[base + i];
      const double2 w = reinterpret_cast<const double2*>(W)[base + i];
      double2 p = reinterpret_cast<double2*>(P)[base + i];
      double2 s = reinterpret_cast<double2*>(S)[base + i];
      const double2 x = reinterpret_cast<const double2*>(X0)[base + i];
      double2 r = reinterpret_cast<double2*>(R)[base + i];
      p = double2{fma(beta, p.x, u.x), fma(beta, p.y, u.y)};
      s = double2{fma(beta, s.x, w.x), fma(beta, s.y, w.y)};
      r = double2{fma(-alpha, s.x, r.x), fma(-alpha, s.y, r.y)};
      reinterpret_cast<double2*>(P)[base + i] = p;
      reinterpret_cast<double2*>(S)[base + i] = s;
      reinterpret_cast<double2*>(X1)[base + i] = double2{fma(alpha, p.x, x.x), fma(alpha, p.y, x.y)};
      reinterpret_cast<double2*>(R)[base + i] = r;
      reinterpret_cast<double2*>(U)[base + i] = double2{m * r.x, m * r.y};
    } else {
      if (frozen) {
        X1[base + i] = X0[base + i];
        continue;
      }
      const double m = Minv ? Minv[c * Mst + i] : Ms;
      const double p = fma(beta, P[base + i], U[base + i]);
      const double s = fma(beta, S[base + i], W[base + i]);
      const double r = fma(-alpha, s, R[base + i]);
      P[base + i] = p;
      S[base + i] = s;
      X1[base + i] = fma(alpha, p, X0[base + i]);
      R[base + i] = r;
      U[base + i] = m * r;
    }
  }
}

// out = x / (1 + T p_i) per component: the sum 1 + T p_i rounded (product, then sum), one division per component
template <bool CPLX>
__global__ __launch_bounds__(256) void k_gauss_prox(const double* __restrict__ X, const double* __restrict__ Pv, double Ps,
                                                    double T, double* __restrict__ out, int64_t n) {
#pragma clang fp contract(off)
  const int64_t base = (int64_t)blockIdx.y * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double den = 1.0 + T * (Pv ? Pv[i] : Ps);
    if constexpr (CPLX) {
      const double2 x = reinterpret_cast<const double2*>(X)[base + i];
      reinterpret_cast<double2*>(out)[base + i] = double2{x.x / den, x.y / den};
    } else {
      out[base + i] = X[base + i] / den;
    }
  }
}

// out = B_i + gs G + (zs S_i) Z per component: acc = B_i (0 without B); with G: acc = fma(gs, G, acc); with Z:
// acc = fma(zs S_i (rounded), Z, acc).  B [n] is shared by the chains, G and Z are [C][n], S is [n], [C][n] (chain stride Sst) or the
// scalar Ss.
template <bool CPLX>
__global__ __launch_bounds__(256) void k_cg_rhs(const double* __restrict__ B, const double* __restrict__ G, double gs,
                                                const double* __restrict__ Z, const double* __restrict__ S, double Ss,
                                                int64_t Sst, double zs, double* __restrict__ out, int64_t n) {
#pragma clang fp contract(off)
  const int64_t base = (int64_t)blockIdx.y * n, sbase = (int64_t)blockIdx.y * Sst;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double f = zs * (S ? S[sbase + i] : Ss);
    if constexpr (CPLX) {
      double2 a = B ? reinterpret_cast<const double2*>(B)[i] : double2{0.0, 0.0};
      if (G) {
        const double2 g = reinterpret_cast<const double2*>(G)[base + i];
        a = double2{fma(gs, g.x, a.x), fma(gs, g.y, a.y)};
      }
      if (Z) {
        const double2 z = reinterpret_cast<const double2*>(Z)[base + i];
        a = double2{fma(f, z.x, a.x), fma(f, z.y, a.y)};
      }
      reinterpret_cast<double2*>(out)[base + i] = a;
    } else {
      double a = B ? B[i] : 0.0;
      if (G) a = fma(gs, G[base + i], a);
      if (Z) a = fma(f, Z[base + i], a);
      out[base + i] = a;
    }
  }
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int pxm_cg_apply(const void* U, const void* Q, const void* B0, const double* D, double D_scalar, int64_t D_stride, const void* R,
                 void* W_out, double* coef, double tol, double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_cg_apply: bad n / C / dtype");
  PXM_REQUIRE(coef && scratch, "pxm_cg_apply: null buffer");
  PXM_REQUIRE(std::isfinite(tol) && tol >= 0, "pxm_cg_apply: tol must be finite and not negative");
  PXM_REQUIRE(D_stride == 0 || D_stride == n, "pxm_cg_apply: D_stride is 0 (shared) or n (one row per chain)");
  hipStream_t st = (hipStream_t)stream;
  int slices = 0;
  if (n > 0) {
    PXM_REQUIRE(U && Q && R && W_out, "pxm_cg_apply: null buffer");
    PXM_REQUIRE(W_out != U && W_out != Q && W_out != R && W_out != B0 && W_out != (const void*)D,
                "pxm_cg_apply: W_out must not alias an input");
    slices = cg_slices(n);
    const dim3 g((unsigned)slices, (unsigned)C);
    const double *u = (const double*)U, *q = (const double*)Q, *b = (const double*)B0, *r = (const double*)R;
    if (dtype) hipLaunchKernelGGL(k_cg_apply<true>, g, dim3(256), 0, st, u, q, b, D, D_scalar, D_stride, r, (double*)W_out, coef, scratch, n);
    else hipLaunchKernelGGL(k_cg_apply<false>, g, dim3(256), 0, st, u, q, b, D, D_scalar, D_stride, r, (double*)W_out, coef, scratch, n);
  }
  hipLaunchKernelGGL(k_cg_finish, dim3(C), dim3(64), 0, st, scratch, slices, tol * tol, coef);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_cg_update(void* U, const void* W, void* P, void* S, const void* X_src, void* X_dst, void* R, const double* Minv,
                  double Minv_scalar, int64_t Minv_stride, const double* coef, int64_t n, int C, int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_cg_update: bad n / C / dtype");
  PXM_REQUIRE(coef, "pxm_cg_update: null buffer");
  PXM_REQUIRE(Minv_stride == 0 || Minv_stride == n, "pxm_cg_update: Minv_stride is 0 (shared) or n (one row per chain)");
  if (n == 0) return 0;
  PXM_REQUIRE(U && W && P && S && X_src && X_dst && R, "pxm_cg_update: null buffer");
  const void* arrays[] = {U, W, P, S, X_src, X_dst, R, (const void*)Minv};
  for (int a = 0; a < 8; ++a)
    for (int b = a + 1; b < 8; ++b)
      PXM_REQUIRE(arrays[a] != arrays[b], "pxm_cg_update: the arrays must all be different");
  const dim3 g((unsigned)cg_slices(n), (unsigned)C);
  hipStream_t st = (hipStream_t)stream;
  double *u = (double*)U, *p = (double*)P, *s = (double*)S, *x1 = (double*)X_dst, *r = (double*)R;
  const double *w = (const double*)W, *x0 = (const double*)X_src;
  if (dtype) hipLaunchKernelGGL(k_cg_update<true>, g, dim3(256), 0, st, u, w, p, s, x0, x1, r, Minv, Minv_scalar, Minv_stride, coef, n);
  else hipLaunchKernelGGL(k_cg_update<false>, g, dim3(256), 0, st, u, w, p, s, x0, x1, r, Minv, Minv_scalar, Minv_stride, coef, n);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_gauss_prox(const void* X, const double* precision, double precision_scalar, double T, void* out, int64_t n, int C,
                   int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_gauss_prox: bad n / C / dtype");
  PXM_REQUIRE(std::isfinite(T) && T >= 0, "pxm_gauss_prox: T must be finite and not negative");
  PXM_REQUIRE(precision || (std::isfinite(precision_scalar) && precision_scalar >= 0),
              "pxm_gauss_prox: the precision must be finite and not negative");
  if (n == 0) return 0;
  PXM_REQUIRE(X && out, "pxm_gauss_prox: null buffer");
  PXM_REQUIRE(out != X && out != (const void*)precision, "pxm_gauss_prox: out must not alias an input");
  const dim3 g((unsigned)cg_slices(n), (unsigned)C);
  hipStream_t st = (hipStream_t)stream;
  if (dtype) hipLaunchKernelGGL(k_gauss_prox<true>, g, dim3(256), 0, st, (const double*)X, precision, precision_scalar, T, (double*)out, n);
  else hipLaunchKernelGGL(k_gauss_prox<false>, g, dim3(256), 0, st, (const double*)X, precision, precision_scalar, T, (double*)out, n);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_cg_rhs(const void* B, const void* G, double g_scale, const void* Z, const double* S, double S_scalar, int64_t S_stride,
               double z_scale, void* out, int64_t n, int C, int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_cg_rhs: bad n / C / dtype");
  PXM_REQUIRE(S_stride == 0 || S_stride == n, "pxm_cg_rhs: S_stride is 0 (shared) or n (one row per chain)");
  if (n == 0) return 0;
  PXM_REQUIRE(out, "pxm_cg_rhs: null buffer");
  PXM_REQUIRE(out != B && out != G && out != Z && out != (const void*)S, "pxm_cg_rhs: out must not alias an input");
  const dim3 g((unsigned)cg_slices(n), (unsigned)C);
  hipStream_t st = (hipStream_t)stream;
  const double *b = (const double*)B, *gg = (const double*)G, *z = (const double*)Z;
  if (dtype) hipLaunchKernelGGL(k_cg_rhs<true>, g, dim3(256), 0, st, b, gg, g_scale, z, S, S_scalar, S_stride, z_scale, (double*)out, n);
  else hipLaunchKernelGGL(k_cg_rhs<false>, g, dim3(256), 0, st, b, gg, g_scale, z, S, S_scalar, S_stride, z_scale, (double*)out, n);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
