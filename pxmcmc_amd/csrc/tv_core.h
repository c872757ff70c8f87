// The arithmetic of the discrete gradient on the MW grid, its adjoint and the pair projection of isotropic total variation,
// written once: every kernel of tv.hip calls these, so a fused launch equals the composed launches bit for bit.
//
// Image [L][n], n = 2L - 1, ring t at theta_t = pi (2t + 1) / n; ab = [2][L] float64 (a_t, b_t; a_{L-1} = b_{L-1} = 0):
//   (A x)[0][t][p] = a_t (x[t+1][p] - x[t][p])
//   (A x)[1][t][p] = b_t (x[t][(p+1) mod n] - x[t][p])
//   (A^H v)[t][p]  = a_{t-1} v0[t-1][p] - a_t v0[t][p] + b_t (v1[t][(p-1) mod n] - v1[t][p]),   a_{-1} = 0
// Per real component: a difference and a product, each rounded, for A; the difference, the product and two fma for A^H.
// A neighbour that does not exist (row L of A, row -1 of A^H) is not read: its coefficient is zero and its value is taken as
// the centre's (A) or as zero (A^H), which leaves an exact zero term.
#pragma once
#include <hip/hip_runtime.h>

#include "elem.h"

namespace pxm {

// a pixel's place on the grid and its ring coefficients
struct TvPix {
  int t, p;
  double a, b, am;  // a_t, b_t, a_{t-1} (0 on ring 0)
};

__device__ __forceinline__ TvPix tv_pix(const double* __restrict__ ab, int L, int n, int i) {
  TvPix q;
  q.t = (int)((unsigned)i / (unsigned)n);
  q.p = i - q.t * n;
  q.a = ab[q.t];
  q.b = ab[L + q.t];
  q.am = q.t > 0 ? ab[q.t - 1] : 0.0;
  return q;
}

__device__ __forceinline__ double tv_diff(double coef, double x_next, double x) {
#pragma clang fp contract(off)
  return coef * (x_next - x);
}

__device__ __forceinline__ double tv_adj(double am, double v0_up, double a, double v0, double b, double v1_west, double v1) {
#pragma clang fp contract(off)
  const double s = b * (v1_west - v1);
  return fma(am, v0_up, fma(-a, v0, s));
}

// one real (T = double) or complex (T = double2) element
template <bool CPLX>
struct TvElem;
template <>
struct TvElem<false> {
  using type = double;
  static __device__ __forceinline__ double zero() { return 0.0; }
  static __device__ __forceinline__ double diff(double c, double xn, double x) { return tv_diff(c, xn, x); }
  static __device__ __forceinline__ double adj(double am, double v0u, double a, double v0, double b, double v1w, double v1) {
    return tv_adj(am, v0u, a, v0, b, v1w, v1);
  }
};
template <>
struct TvElem<true> {
  using type = double2;
  static __device__ __forceinline__ double2 zero() { return double2{0.0, 0.0}; }
  static __device__ __forceinline__ double2 diff(double c, double2 xn, double2 x) {
    return double2{tv_diff(c, xn.x, x.x), tv_diff(c, xn.y, x.y)};
  }
  static __device__ __forceinline__ double2 adj(double am, double2 v0u, double a, double2 v0, double b, double2 v1w, double2 v1) {
    return double2{tv_adj(am, v0u.x, a, v0.x, b, v1w.x, v1.x), tv_adj(am, v0u.y, a, v0.y, b, v1w.y, v1.y)};
  }
};

// (A x) at pixel q of the image x (one chain, [L n] elements): d0 along theta, d1 along phi
template <bool CPLX>
__device__ __forceinline__ void tv_grad_at(const typename TvElem<CPLX>::type* __restrict__ x, const TvPix& q, int L, int n, int i,
                                           typename TvElem<CPLX>::type& d0, typename TvElem<CPLX>::type& d1) {
  const auto xc = x[i];
  const auto xs = q.t + 1 < L ? x[i + n] : xc;
  const auto xe = x[q.p + 1 < n ? i + 1 : i + 1 - n];
  d0 = TvElem<CPLX>::diff(q.a, xs, xc);
  d1 = TvElem<CPLX>::diff(q.b, xe, xc);
}

// (A^H v) at pixel q of the coefficients v (one chain: plane 0 at v0, plane 1 at v1, [L n] elements each)
template <bool CPLX>
__device__ __forceinline__ typename TvElem<CPLX>::type tv_adj_at(const typename TvElem<CPLX>::type* __restrict__ v0,
                                                                 const typename TvElem<CPLX>::type* __restrict__ v1,
                                                                 const TvPix& q, int n, int i) {
  const auto up = q.t > 0 ? v0[i - n] : TvElem<CPLX>::zero();
  const auto west = v1[q.p > 0 ? i - 1 : i - 1 + n];
  return TvElem<CPLX>::adj(q.am, up, q.a, v0[i], q.b, west, v1[i]);
}

// sum of the squares of a pair's real components, plane by plane: every product and sum rounded
__device__ __forceinline__ double tv_pair2(double d0, double d1) { return abs2_plain(d0, d1); }
__device__ __forceinline__ double tv_pair2(double2 d0, double2 d1) {
#pragma clang fp contract(off)
  return abs2_plain(d0.x, d0.y) + abs2_plain(d1.x, d1.y);
}

__device__ __forceinline__ double tv_fma1(double s, double w, double v) { return fma(s, w, v); }
__device__ __forceinline__ double2 tv_fma1(double s, double2 w, double2 v) { return double2{fma(s, w.x, v.x), fma(s, w.y, v.y)}; }
__device__ __forceinline__ double tv_scale(double w, double s) {
#pragma clang fp contract(off)
  return w * s;
}
__device__ __forceinline__ double2 tv_scale(double2 w, double s) {
#pragma clang fp contract(off)
  return double2{w.x * s, w.y * s};
}
__device__ __forceinline__ double tv_sub(double x, double y) { return x - y; }
__device__ __forceinline__ double2 tv_sub(double2 x, double2 y) { return double2{x.x - y.x, x.y - y.y}; }

// The dual half of a primal-dual iteration on one pair: w = v + sigma wa per component; the pair is scaled by r / |w| when
// its norm |w| = sqrt(sum of squares) exceeds r = t rscale (|w| == r and |w| == 0 are kept, t == 0 gives 0, r == inf never
// binds).  Adds the pair's terms to dv2 = sum |v1 - v|^2, v2 = sum |v1|^2 and tw = sum t |wa|.
template <class T>
__device__ __forceinline__ void tv_pair_step(T va, T vb, T wa, T wb, double t, double sigma, double rscale, T& oa, T& ob,
                                             double& dv2, double& v2, double& tw) {
#pragma clang fp contract(off)
  const double r = t * rscale;
  oa = tv_fma1(sigma, wa, va);
  ob = tv_fma1(sigma, wb, vb);
  const double nrm = sqrt(tv_pair2(oa, ob));
  if (nrm > r) {  // nrm > r >= 0, so nrm > 0
    const double s = r / nrm;
    oa = tv_scale(oa, s);
    ob = tv_scale(ob, s);
  }
  dv2 += tv_pair2(tv_sub(oa, va), tv_sub(ob, vb));
  v2 += tv_pair2(oa, ob);
  tw += t * sqrt(tv_pair2(wa, wb));
}

// The primal half on one element, the arithmetic of k_pd_primal (primal_dual.hip): x1 = fma(-tau, g + u, x) per component
__device__ __forceinline__ double tv_primal(double x, double g, double u, double tau) {
#pragma clang fp contract(off)
  return fma(-tau, g + u, x);
}
__device__ __forceinline__ double2 tv_primal(double2 x, double2 g, double2 u, double tau) {
  return double2{tv_primal(x.x, g.x, u.x, tau), tv_primal(x.y, g.y, u.y, tau)};
}
__device__ __forceinline__ double tv_bar(double x1, double x) { return fma(2.0, x1, -x); }
__device__ __forceinline__ double2 tv_bar(double2 x1, double2 x) { return double2{fma(2.0, x1.x, -x.x), fma(2.0, x1.y, -x.y)}; }
__device__ __forceinline__ double tv_abs2(double x) {
#pragma clang fp contract(off)
  return x * x;
}
__device__ __forceinline__ double tv_abs2(double2 x) { return abs2_plain(x.x, x.y); }

}  // namespace pxm
