// One slice of the L2 and of the transition sum of PxMALA, as the workgroup (c, bx of nb) forms it.  The kernels of
// pxm_reduce_l2 / pxm_logtransition (reduce.hip) and the merged tail kernel of PxMALA (pxmala.hip) share these bodies, so a
// slice's sum does not depend on which launch computed it.
#pragma once
#include "elem.h"
#include "reduce.h"

namespace pxm {

// L2 = vdot(d, invcov d) = sum conj(d) * (invcov * d), d = data - preds   (pxmcmc/mcmc.py:78-79)
template <bool CPLX, bool ICPLX>
__device__ __forceinline__ void l2_partial_body(const double* __restrict__ preds, const double* __restrict__ data,
                                                const double* __restrict__ invcov, double* __restrict__ part, int64_t n,
                                                int c, int bx, int nb) {
  double2 acc{0.0, 0.0};
  for (int64_t i = bx * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)nb * blockDim.x) {
    if (CPLX) {
      const double2 d = csub(reinterpret_cast<const double2*>(data)[i], reinterpret_cast<const double2*>(preds)[(int64_t)c * n + i]);
      double2 wd;
      if (ICPLX) wd = cmul(reinterpret_cast<const double2*>(invcov)[i], d);
      else wd = double2{invcov[i] * d.x, invcov[i] * d.y};
      // conj(d) * wd
      acc.x += d.x * wd.x + d.y * wd.y;
      acc.y += d.x * wd.y - d.y * wd.x;
    } else {
      const double d = data[i] - preds[(int64_t)c * n + i];
      acc.x += d * (invcov[i] * d);
    }
  }
  block_sum2(acc.x, acc.y);
  if (threadIdx.x == 0) reinterpret_cast<double2*>(part)[(int64_t)c * nb + bx] = acc;
}

// S = sum (X2 - X1 - (d/2) g)^2 with g = -((X1 - proxf)/l) - gradg; complex squares, no abs (literal)
// (P == nullptr: proxf = soft(X1, T) is formed here instead of being read -- the stock L1 prox, prior.py:49-50)
template <bool CPLX>
__device__ __forceinline__ void logtrans_partial_body(const double* __restrict__ X1, const double* __restrict__ X2,
                                                      const double* __restrict__ P, const double* __restrict__ G, double d,
                                                      double lmda, double* __restrict__ part, int64_t n, int c, int bx,
                                                      int nb, const double* __restrict__ T = nullptr, double Ts = 0.0) {
  const int64_t base = (int64_t)c * n;
  double2 acc{0.0, 0.0};
  for (int64_t i = bx * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)nb * blockDim.x) {
    if (CPLX) {
      const double2 x1 = reinterpret_cast<const double2*>(X1)[base + i], x2 = reinterpret_cast<const double2*>(X2)[base + i];
      const double2 g = reinterpret_cast<const double2*>(G)[base + i];
      const double2 p = P ? reinterpret_cast<const double2*>(P)[base + i] : soft_cplx(x1, T ? T[i] : Ts);
      const double2 gl{-((x1.x - p.x) / lmda) - g.x, -((x1.y - p.y) / lmda) - g.y};
      const double2 r{x2.x - x1.x - (d / 2) * gl.x, x2.y - x1.y - (d / 2) * gl.y};
      acc.x += r.x * r.x - r.y * r.y;
      acc.y += 2 * r.x * r.y;
    } else {
      const double x1 = X1[base + i];
      const double p = P ? P[base + i] : soft_real(x1, T ? T[i] : Ts);
      const double gl = -((x1 - p) / lmda) - G[base + i];
      const double r = X2[base + i] - x1 - (d / 2) * gl;
      acc.x += r * r;
    }
  }
  block_sum2(acc.x, acc.y);
  if (threadIdx.x == 0) reinterpret_cast<double2*>(part)[(int64_t)c * nb + bx] = acc;
}

}  // namespace pxm
