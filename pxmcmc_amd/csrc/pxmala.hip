// The PxMALA iteration beyond the forward model: proposal with its sums, the merged tail sums, the Metropolis test, and their
// C-ABI.  Every array is [C][n] (chain-major); T / data / invcov / weights are [n], shared by all chains.  The sums follow the
// fixed order and the slice count of reduce.h.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"
#include "pxmala_sums.h"
#include "reduce.h"

#include <algorithm>

namespace pxm {

static_assert(NOISE_F64_FLAG == PXM_NOISE_F64, "elem.h: the noise flag must be the public one");

// PxMALA, after the forward model and the gradient of the proposal: the reverse transition sum S(X', X) and the L2 of the
// proposal's predictions in ONE grid -- workgroups [0, nb_lt) are the slices of the transition sum, [nb_lt, nb_lt + nb_l2)
// those of the L2 (two short latency-bound launches otherwise)
template <bool CPLX, bool DCPLX, bool ICPLX>
__global__ void k_pxmala_tail_partial(const double* __restrict__ X1, const double* __restrict__ X2,
                                      const double* __restrict__ P, const double* __restrict__ G,
                                      const double* __restrict__ delta_dev, double lmda, double* __restrict__ part_lt,
                                      int64_t n, int nb_lt, const double* __restrict__ preds,
                                      const double* __restrict__ data, const double* __restrict__ invcov,
                                      double* __restrict__ part_l2, int64_t nd, int nb_l2, const double* __restrict__ T,
                                      double Ts) {
  const int c = blockIdx.y;
  if ((int)blockIdx.x < nb_lt) logtrans_partial_body<CPLX>(X1, X2, P, G, delta_dev[c], lmda, part_lt, n, c, blockIdx.x, nb_lt, T, Ts);
  else l2_partial_body<DCPLX, ICPLX>(preds, data, invcov, part_l2, nd, c, blockIdx.x - nb_lt, nb_l2);
}

// ---- PxMALA proposal in one pass (pxmcmc/mcmc.py:231,234,236-238,242 for the proposal) -----------------------
//   X' = chain_step(X, proxf, gradg)                                   (mcmc.py:185-201)
//   P' = soft(X', T)                                                   (prior.py:49-50)
//   S  = sum (X' - X - (d/2) g)^2,  g = -((X - proxf)/l) - gradg       (calc_logtransition(X, X', proxf, gradg), :281-289)
//   A  = sum |w X'|                                                     (prior.prior(X'), prior.py:28-35,83-84)
// partial sums per slice: (S.re, S.im, A, -)
template <bool CPLX>
__global__ void k_pxmala_propose(const double* __restrict__ X, const double* __restrict__ P, const double* __restrict__ G,
                                 const double* __restrict__ T, double Ts, const double* __restrict__ wp,
                                 const double* __restrict__ delta_dev, double lmda, NoiseSrc ns, double* __restrict__ Xp,
                                 double* __restrict__ Pp, double* __restrict__ part, int64_t n) {
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  const double d = delta_dev[c];
  double2 acc{0.0, 0.0};
  double accA = 0.0, none = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double2 w = draw_noise<CPLX>(ns, c, n, i);
    const double t = T ? T[i] : Ts;
    const double wa = wp ? fabs(wp[i]) : 1.0;
    if (CPLX) {
      const double2 x = reinterpret_cast<const double2*>(X)[base + i];
      const double2 p = P ? reinterpret_cast<const double2*>(P)[base + i] : soft_cplx(x, t);
      const double2 g = reinterpret_cast<const double2*>(G)[base + i];
      const double2 xn = chain_step_cplx(x, p, g, w, d, lmda);
      reinterpret_cast<double2*>(Xp)[base + i] = xn;
      if (Pp) reinterpret_cast<double2*>(Pp)[base + i] = soft_cplx(xn, t);
      const double2 gl{-((x.x - p.x) / lmda) - g.x, -((x.y - p.y) / lmda) - g.y};
      const double2 r{xn.x - x.x - (d / 2) * gl.x, xn.y - x.y - (d / 2) * gl.y};
      acc.x += r.x * r.x - r.y * r.y;
      acc.y += 2 * r.x * r.y;
      accA += wa * sqrt(fma(xn.x, xn.x, xn.y * xn.y));
    } else {
      const double x = X[base + i], p = P ? P[base + i] : soft_real(x, t), g = G[base + i];
      const double xn = chain_step_real(x, p, g, w.x, d, lmda);
      Xp[base + i] = xn;
      if (Pp) Pp[base + i] = soft_real(xn, t);
      const double gl = -((x - p) / lmda) - g;
      const double r = xn - x - (d / 2) * gl;
      acc.x += r * r;
      accA += wa * fabs(xn);
    }
  }
  // two sums of the two-component form: they share its one LDS array (a three-component sum would be another instantiation)
  block_sum2(acc.x, acc.y);
  block_sum2(accA, none);
  if (threadIdx.x == 0) {
    double* o = part + ((int64_t)c * gridDim.x + blockIdx.x) * 4;
    o[0] = acc.x;
    o[1] = acc.y;
    o[2] = accA;
    o[3] = 0.0;
  }
}

// lt[c] = -(d/2) S^2 (complex, literal: (1/2*d) == d/2 and the sum is squared again), prior[c] = A
__global__ void k_pxmala_propose_final(const double* __restrict__ part, double* __restrict__ lt, double* __restrict__ prior,
                                       int slices, const double* __restrict__ delta_dev) {
  const int c = blockIdx.x;
  double2 v;
  double a;
  slice_sum<4>(part + (int64_t)c * slices * 4, slices, threadIdx.x, v.x, v.y, a);
  if (threadIdx.x == 0) {
    const double d = delta_dev[c];
    const double2 s2 = cmul(v, v);
    reinterpret_cast<double2*>(lt)[c] = double2{-(1.0 / 2 * d) * s2.x, -(1.0 / 2 * d) * s2.y};
    prior[c] = a;
  }
}

// Metropolis test, state bookkeeping, delta adaptation and traces of one PxMALA iteration for chain c
// (pxmcmc/mcmc.py:244-260,277-279).  logpi' = -mu prior' - L2' (mcmc.py:81); only real parts enter logalpha.
struct AcceptArgs {
  double mu, lmda;
  double2* logpi_c;
  double2* L2_c;
  double* prior_c;
  const double* u;
  uint64_t seed, chain0, iter;
  const uint64_t* iter_dev;
  int32_t* accept;
  double* delta_dev;
  int tune;
  int32_t* acc_trace;
  double* delta_trace;
  int chunk, C;
};
__device__ __forceinline__ void accept_chain(const AcceptArgs& a, int c, double2 lt_pc, double2 lt_cp, double prior_p, double2 L2_p) {
  const uint64_t it = a.iter + (a.iter_dev ? *a.iter_dev : 0);
  const double2 lpp{-a.mu * prior_p - L2_p.x, -L2_p.y};
  const double logalpha = lt_pc.x + lpp.x - lt_cp.x - a.logpi_c[c].x;
  const double uu = a.u ? a.u[c] : philox_uniform(a.seed, a.chain0 + c, it);
  const int acc = log(uu) < logalpha ? 1 : 0;
  a.accept[c] = acc;
  if (acc) {
    a.logpi_c[c] = lpp;
    a.L2_c[c] = L2_p;
    a.prior_c[c] = prior_p;
  }
  double d = a.delta_dev[c];
  if (a.tune) {  // pxmcmc/mcmc.py:277-279
    d = d * (1 + (acc - 0.5) / pow((double)(it + 1), 0.75));
    d = fmin(fmax(d, a.lmda * 1e-8), a.lmda / 2);
    a.delta_dev[c] = d;
  }
  if (a.acc_trace) {
    const int64_t k = (int64_t)(it % (uint64_t)a.chunk);
    a.acc_trace[k * a.C + c] = acc;
    a.delta_trace[k * a.C + c] = d;
  }
}

__global__ void k_pxmala_accept2(const double2* __restrict__ lt_pc, const double2* __restrict__ lt_cp,
                                 const double* __restrict__ prior_p, const double2* __restrict__ L2_p, AcceptArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.C) return;
  accept_chain(a, c, lt_pc[c], lt_cp[c], prior_p[c], L2_p[c]);
}

// The same test fed by the PARTIAL sums of the iteration (pxm_pxmala_propose with deferred totals, k_pxmala_tail_partial):
// ONE workgroup of 16 waves, three waves per chain (five chains in flight): one wave each for the slices of the forward
// transition sum + prior, of the reverse transition sum and of the L2, added in the order of k_reduce_final /
// k_pxmala_propose_final (so the totals are the ones the separate kernels give); the totals meet in LDS and lane 0 of the
// chain's first wave decides.  The totals are also stored for observers.  `bump`: the device-resident iteration counter of a
// captured iteration, advanced here after every chain has read it (one workgroup) -- the last reader of the counter in an
// iteration.  `bump` MAY ALIAS a.iter_dev (PxMALA's captured iteration passes the same counter as both): it is not
// `__restrict__`, and the store sits behind the last barrier.
__global__ __launch_bounds__(1024) void k_pxmala_accept3(const double* __restrict__ part_prop, int slices_prop,
                                                         const double2* __restrict__ part_lt, int slices_lt,
                                                         const double2* __restrict__ part_l2, int slices_l2,
                                                         double2* __restrict__ lt_pc_out, double2* __restrict__ lt_cp_out,
                                                         double* __restrict__ prior_p_out, double2* __restrict__ L2_p_out,
                                                         AcceptArgs a, uint64_t* bump) {
  constexpr int CB = 5;              // chains per round
  __shared__ double tot[CB][8];      // (S_cp.re, S_cp.im, prior, -, S_pc.re, S_pc.im, L2.re, L2.im)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = wave / 3, role = wave % 3;
  for (int c0 = 0; c0 < a.C; c0 += CB) {
    const int c = c0 + slot;
    if (slot < CB && c < a.C) {
      double* o = tot[slot] + (role == 0 ? 0 : (role == 1 ? 4 : 6));
      double re = 0.0, im = 0.0, pr = 0.0;
      if (role == 0) slice_add<4>(part_prop + (int64_t)c * slices_prop * 4, slices_prop, lane, re, im, pr);
      else if (role == 1) slice_add<2>(reinterpret_cast<const double*>(part_lt) + (int64_t)c * slices_lt * 2, slices_lt, lane, re, im);
      else slice_add<2>(reinterpret_cast<const double*>(part_l2) + (int64_t)c * slices_l2 * 2, slices_l2, lane, re, im);
      wave_sum(re, im, pr);
      if (lane == 0) {
        o[0] = re, o[1] = im;
        if (role == 0) o[2] = pr;
      }
    }
    __syncthreads();
    if (slot < CB && c < a.C && role == 0 && lane == 0) {
      const double2 s_cp{tot[slot][0], tot[slot][1]}, s_pc{tot[slot][4], tot[slot][5]}, l2{tot[slot][6], tot[slot][7]};
      const double pr = tot[slot][2];
      const double d = a.delta_dev[c];  // (before its adaptation below: the delta both transitions were proposed with)
      const double2 q_cp = cmul(s_cp, s_cp), q_pc = cmul(s_pc, s_pc);
      const double2 lt_cp{-(1.0 / 2 * d) * q_cp.x, -(1.0 / 2 * d) * q_cp.y}, lt_pc{-(1.0 / 2 * d) * q_pc.x, -(1.0 / 2 * d) * q_pc.y};
      lt_cp_out[c] = lt_cp;
      lt_pc_out[c] = lt_pc;
      prior_p_out[c] = pr;
      L2_p_out[c] = l2;
      accept_chain(a, c, lt_pc, lt_cp, pr, l2);
    }
    __syncthreads();
  }
  if (bump && threadIdx.x == 0) *bump += 1;  // (behind the last barrier: every chain has read the counter)
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int pxm_pxmala_propose(const void* X, const void* proxf, const void* gradg, const double* T, double T_scalar,
                       const double* prior_weights, const double* delta_dev, double lmda, const void* noise,
                       int noise_complex, uint64_t seed, uint64_t chain0, uint64_t iter, const uint64_t* iter_dev,
                       void* X_prop, void* proxf_prop, double* logtrans_out, double* prior_out, double* scratch,
                       int64_t n, int C, int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 1 && C >= 1 && (dtype == 0 || dtype == 1), "pxm_pxmala_propose: bad n / C / dtype");
  PXM_REQUIRE(X && gradg && delta_dev && X_prop && scratch, "pxm_pxmala_propose: null buffer");
  PXM_REQUIRE((proxf == nullptr) == (proxf_prop == nullptr),
              "pxm_pxmala_propose: proxf and proxf_prop are given together, or both null (prox = soft(., T) formed in the kernels)");
  PXM_REQUIRE((logtrans_out == nullptr) == (prior_out == nullptr),
              "pxm_pxmala_propose: logtrans_out and prior_out are given together, or both null (totals deferred to pxm_pxmala_finish)");
  if (int rc = check_noise_arg("pxm_pxmala_propose", noise_complex, dtype)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int RS = red_slices(n);
  dim3 g(RS, C), b(512);  // (8 waves per slice: 25.5 us against 29.8 with 4 and 33.8 with 16 at n = 1.2 M complex, one chain)
  NoiseSrc ns = make_noise_src(noise, noise_complex, seed, chain0, iter, iter_dev);
  if (dtype)
    hipLaunchKernelGGL(k_pxmala_propose<true>, g, b, 0, st, (const double*)X, (const double*)proxf, (const double*)gradg, T,
                       T_scalar, prior_weights, delta_dev, lmda, ns, (double*)X_prop, (double*)proxf_prop, scratch, n);
  else
    hipLaunchKernelGGL(k_pxmala_propose<false>, g, b, 0, st, (const double*)X, (const double*)proxf, (const double*)gradg, T,
                       T_scalar, prior_weights, delta_dev, lmda, ns, (double*)X_prop, (double*)proxf_prop, scratch, n);
  if (logtrans_out)
    hipLaunchKernelGGL(k_pxmala_propose_final, dim3(C), dim3(64), 0, st, scratch, logtrans_out, prior_out, RS, delta_dev);
  PXM_HIP(hipGetLastError());
  return 0;
}

static AcceptArgs make_accept_args(double mu, double lmda, double* logpi_c, double* L2_c, double* prior_c, const double* u,
                                   uint64_t seed, uint64_t chain0, uint64_t iter, const uint64_t* iter_dev, int32_t* accept_out,
                                   double* delta_dev, int tune, int32_t* acc_trace, double* delta_trace, int chunk, int C) {
  AcceptArgs a;
  a.mu = mu, a.lmda = lmda;
  a.logpi_c = (double2*)logpi_c, a.L2_c = (double2*)L2_c, a.prior_c = prior_c;
  a.u = u, a.seed = seed, a.chain0 = chain0, a.iter = iter, a.iter_dev = iter_dev;
  a.accept = accept_out, a.delta_dev = delta_dev, a.tune = tune;
  a.acc_trace = acc_trace, a.delta_trace = delta_trace, a.chunk = chunk, a.C = C;
  return a;
}

int pxm_pxmala_accept(const double* logtrans_pc, const double* logtrans_cp, const double* prior_p, const double* L2_p,
                      double mu, double* logpi_c, double* L2_c, double* prior_c, const double* u, uint64_t seed,
                      uint64_t chain0, uint64_t iter, const uint64_t* iter_dev, int32_t* accept_out, double* delta_dev,
                      int tune, double lmda, int32_t* acc_trace, double* delta_trace, int chunk, int C,
                      pxm_stream_t stream) {
  PXM_REQUIRE(C >= 1 && logtrans_pc && logtrans_cp && prior_p && L2_p && logpi_c && L2_c && prior_c && accept_out && delta_dev,
              "pxm_pxmala_accept: null buffer");
  PXM_REQUIRE((acc_trace == nullptr) == (delta_trace == nullptr) && (!acc_trace || chunk >= 1), "pxm_pxmala_accept: bad trace buffers");
  hipLaunchKernelGGL(k_pxmala_accept2, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const double2*)logtrans_pc,
                     (const double2*)logtrans_cp, prior_p, (const double2*)L2_p,
                     make_accept_args(mu, lmda, logpi_c, L2_c, prior_c, u, seed, chain0, iter, iter_dev, accept_out, delta_dev, tune,
                                      acc_trace, delta_trace, chunk, C));
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_pxmala_finish(const void* X_prop, const void* X_curr, const void* proxf_prop, const double* T, double T_scalar,
                      const void* gradg_prop, int64_t n, int dtype, const void* preds_prop, const void* data, const void* invcov, int invcov_complex,
                      int64_t n_data, int data_dtype, const double* propose_scratch, double mu, double lmda, double* logpi_c,
                      double* L2_c, double* prior_c, const double* u, uint64_t seed, uint64_t chain0, uint64_t iter,
                      const uint64_t* iter_dev, int32_t* accept_out, double* delta_dev, int tune, int32_t* acc_trace,
                      double* delta_trace, int chunk, double* logtrans_pc_out, double* logtrans_cp_out, double* prior_p_out,
                      double* L2_p_out, double* scratch, uint64_t* bump_counter, int C, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 1 && n_data >= 1 && C >= 1 && (dtype == 0 || dtype == 1) && (data_dtype == 0 || data_dtype == 1),
              "pxm_pxmala_finish: bad n / n_data / C / dtype");
  PXM_REQUIRE(X_prop && X_curr && gradg_prop && preds_prop && data && invcov && propose_scratch && scratch,
              "pxm_pxmala_finish: null buffer");
  PXM_REQUIRE(data_dtype == 1 || !invcov_complex, "pxm_pxmala_finish: complex invcov needs complex data");
  PXM_REQUIRE(logpi_c && L2_c && prior_c && accept_out && delta_dev && logtrans_pc_out && logtrans_cp_out && prior_p_out && L2_p_out,
              "pxm_pxmala_finish: null state / output buffer");
  PXM_REQUIRE((acc_trace == nullptr) == (delta_trace == nullptr) && (!acc_trace || chunk >= 1), "pxm_pxmala_finish: bad trace buffers");
  hipStream_t st = (hipStream_t)stream;
  const int RS = red_slices(n), RD = red_slices(n_data);
  double *part_lt = scratch, *part_l2 = scratch + red_scratch_doubles(C);
  const double *x1 = (const double*)X_prop, *x2 = (const double*)X_curr, *px = (const double*)proxf_prop, *g = (const double*)gradg_prop;
  const double *pp = (const double*)preds_prop, *dd = (const double*)data, *ic = (const double*)invcov;
  dim3 grid(RS + RD, C), blk(256);
#define PXM_TAIL(CP, DC, IC_)                                                                                              \
  hipLaunchKernelGGL((k_pxmala_tail_partial<CP, DC, IC_>), grid, blk, 0, st, x1, x2, px, g, delta_dev, lmda, part_lt, n, RS, pp, dd, \
                     ic, part_l2, n_data, RD, T, T_scalar)
  if (dtype) {
    if (data_dtype && invcov_complex) PXM_TAIL(true, true, true);
    else if (data_dtype) PXM_TAIL(true, true, false);
    else PXM_TAIL(true, false, false);
  } else {
    if (data_dtype && invcov_complex) PXM_TAIL(false, true, true);
    else if (data_dtype) PXM_TAIL(false, true, false);
    else PXM_TAIL(false, false, false);
  }
#undef PXM_TAIL
  hipLaunchKernelGGL(k_pxmala_accept3, dim3(1), dim3(64 * std::min(16, 3 * C)), 0, st, propose_scratch, RS, (const double2*)part_lt, RS,
                     (const double2*)part_l2, RD, (double2*)logtrans_pc_out, (double2*)logtrans_cp_out, prior_p_out,
                     (double2*)L2_p_out,
                     make_accept_args(mu, lmda, logpi_c, L2_c, prior_c, u, seed, chain0, iter, iter_dev, accept_out, delta_dev, tune,
                                      acc_trace, delta_trace, chunk, C),
                     bump_counter);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
