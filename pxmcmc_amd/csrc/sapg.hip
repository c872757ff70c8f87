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
//
// pxm_sapg_step_groups: one theta per chain AND per group of the state, for G(X) = sum_k theta_k G_k(X) with G_k the sum over
// the contiguous block [b_k, b_k+1) (a wavelet scale): the normaliser factorises into theta_k^-d_k, so block k moves by
// d_k - theta_ck G_ck.  The same step kernel (template parameter GROUPS), launched with the slices of all groups side by side:
// a workgroup belongs to one group -- it finds it by counting the group slice offsets at or below its number, K - 1 uniform
// compares on kernel arguments -- reads that group's theta and strides over that group's elements only, group k in
// chain_slices(b_k+1 - b_k) slices: the sum of a group is the sum pxm_sapg_step leaves for the sub-vector alone.  Element and
// noise indices stay the global ones.  The update kernel runs one workgroup per group, which handles the group's C chains the
// way k_sapg_update handles the chains (pooling is per group, so the groups are independent); rho is a table [n_rho][K] and
// d a vector [K] on the device.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"
#include "reduce.h"

#include <cmath>
#include <string>

namespace pxm {

static_assert(NOISE_F64_FLAG == PXM_NOISE_F64, "elem.h: the noise flag must be the public one");

// The groups of pxm_sapg_step_groups, passed to both kernels by value: element offsets b[0 .. K] and the offsets s[0 .. K] of
// the groups' slices in the grid (s[k + 1] - s[k] = chain_slices(b[k + 1] - b[k])).  The ungrouped kernel takes the empty form.
template <bool GROUPS>
struct SapgGroups {};
template <>
struct SapgGroups<true> {
  int K;
  int s[PXM_SAPG_GROUPS_MAX + 1];
  int64_t b[PXM_SAPG_GROUPS_MAX + 1];
};

// The body both forms of the step kernel share: the thread steps the elements first, first + stride, ... below last of chain
// c with the threshold scale th and returns its part of sum T_i |X1_i|.  n is the length of the whole chain: the element and
// noise indices are the global ones whatever the slice.
template <bool CPLX>
__device__ __forceinline__ double sapg_step_slice(const double* __restrict__ X, const double* __restrict__ G,
                                                  const double* __restrict__ T, double Ts, double th, double delta, double lmda,
                                                  const NoiseSrc& ns, double* __restrict__ X1, int c, int64_t n, int64_t first,
                                                  int64_t last, int64_t stride) {
#pragma clang fp contract(off)  // products and sums as written: the threshold theta_c T_i is rounded before the shrink, the
                                // terms of the sum are the ones float64 numpy forms (the shared helpers keep their own mode)
  const int64_t base = (int64_t)c * n;
  double acc = 0.0;
  for (int64_t i = first; i < last; i += stride) {
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
  return acc;
}

// One workgroup per slice: 256 threads striding over their elements, then one partial (reduce.h).  Ungrouped: theta [C], part
// [C][gridDim.x].  GROUPS: theta [C][K], part [C][K][PXM_SAPG_SLICES_MAX]; the slices of all groups are numbered side by
// side, gr.s[K] = gridDim.x in all, so a workgroup belongs to exactly one group and reads one theta.
// NZ selects the noise at compile time, so that draw_noise's run-time switches fold away and with them the scalar registers
// of the paths not taken (with all of them in one kernel the complex128 form runs out of scalar registers):
// 0: the caller's array (no Philox code); else the Philox stream, 1 + (Box-Muller in fp64) + 2 * (complex noise), with the
// iteration number read once
template <bool CPLX, int NZ, bool GROUPS>
__global__ __launch_bounds__(256) void k_sapg_step(const double* __restrict__ X, const double* __restrict__ G,
                                                   const double* __restrict__ T, double Ts,
                                                   const double* __restrict__ theta, double delta, double lmda, NoiseSrc ns_,
                                                   double* __restrict__ X1, double* __restrict__ part, int64_t n,
                                                   SapgGroups<GROUPS> gr) {
  const int c = blockIdx.y;
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
  if constexpr (GROUPS) {
    int k = 0;
    for (int j = 1; j < gr.K; ++j) k += gr.s[j] <= (int)blockIdx.x;  // the workgroup's group; uniform: the offsets increase
    const int slice = (int)blockIdx.x - gr.s[k];
    const int64_t pair = (int64_t)c * gr.K + k;
    double acc = sapg_step_slice<CPLX>(X, G, T, Ts, theta[pair], delta, lmda, ns, X1, c, n,
                                       gr.b[k] + slice * (int64_t)blockDim.x + threadIdx.x, gr.b[k + 1],
                                       (int64_t)(gr.s[k + 1] - gr.s[k]) * blockDim.x);
    block_sum<4>(acc);
    if (threadIdx.x == 0) part[pair * PXM_SAPG_SLICES_MAX + slice] = acc;
  } else {
    double acc = sapg_step_slice<CPLX>(X, G, T, Ts, theta[c], delta, lmda, ns, X1, c, n,
                                       blockIdx.x * (int64_t)blockDim.x + threadIdx.x, n, (int64_t)gridDim.x * blockDim.x);
    block_sum<4>(acc);
    if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = acc;
  }
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
// thread per chain moves eta and theta.  GROUPS: workgroup k does the same for the C chains of group k (nothing couples the
// groups: the pooled mean is per group), on the pairs p = c K + k: part [C][K][PXM_SAPG_SLICES_MAX] with the group's own
// number of slices, gsum / theta / eta [C][K], d_k from the device vector dvec and rho from column k of the table
// [n_rho][K]; trace [n_trace][C][K][3].  (One workgroup for all C K pairs took one round of dependent loads per 16 pairs.)
template <bool GROUPS>
__global__ __launch_bounds__(1024) void k_sapg_update(const double* __restrict__ part, int slices, int C, SapgUpdate u,
                                                      double* __restrict__ gsum, double* __restrict__ theta,
                                                      double* __restrict__ eta, double* __restrict__ trace,
                                                      SapgGroups<GROUPS> gr, const double* __restrict__ dvec) {
#pragma clang fp contract(off)  // each operation of the update rounded: the host model reproduces it bit for bit
  __shared__ double pooled;
  int K = 1, k = 0;
  int64_t stride = slices;  // between the partials of one pair and the next
  double d = u.d;
  if constexpr (GROUPS) {
    K = gr.K, k = blockIdx.x;
    slices = gr.s[k + 1] - gr.s[k], stride = PXM_SAPG_SLICES_MAX;
    d = dvec[k];
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwave = blockDim.x >> 6;
  for (int c = wave; c < C; c += nwave) {
    double v;
    slice_sum<1>(part + ((int64_t)c * K + k) * stride, slices, lane, v);
    if (lane == 0) gsum[c * K + k] = v / u.lmda;
  }
  __syncthreads();
  if (u.pool) {
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int c = 0; c < C; ++c) s += gsum[c * K + k];
      pooled = s / (double)C;
    }
    __syncthreads();
  }
  const uint64_t it = u.iter + (u.iter_dev ? *u.iter_dev : 0);
  const double rho = u.rho_tab[(it < (uint64_t)u.n_rho ? (int64_t)it : u.n_rho - 1) * K + k];
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const int64_t p = (int64_t)c * K + k;
    const double g = u.pool ? pooled : gsum[p];
    const double e = fmin(fmax(eta[p] + rho * (d - theta[p] * g), u.eta_min), u.eta_max);
    const double th = exp(e);
    eta[p] = e;
    theta[p] = th;
    if (it < (uint64_t)u.n_trace) {
      double* row = trace + (((int64_t)it * C + c) * K + k) * 3;
      row[0] = th, row[1] = e, row[2] = g;
    }
  }
}

// ---- host side: what the two entry points share ------------------------------------------------------------------------------
struct SapgArgs {
  const void *X, *gradg;
  const double* T;
  double T_scalar, delta, lmda;
  const void* noise;
  int noise_complex;
  uint64_t seed, chain0, iter;
  const uint64_t* iter_dev;
  double *theta, *eta;
  const double* rho_table;
  int64_t n_rho;
  double eta_min, eta_max;
  int pool;
  double* trace;
  int64_t n_trace;
  void* X_out;
  double* scratch;
  int64_t n;
  int C, dtype;
  hipStream_t st;
};

// the null, alias, finiteness and noise checks; dvec: the device vector d of the grouped form (an input like rho_table)
static int sapg_check(const char* fn, const SapgArgs& a, const double* dvec) {
  const std::string f(fn);
  PXM_REQUIRE(a.C >= 1 && a.C <= 65535 && (a.dtype == 0 || a.dtype == 1), f + ": bad n / C / dtype");
  PXM_REQUIRE(a.theta && a.eta && a.scratch, f + ": null buffer");
  PXM_REQUIRE(a.rho_table && a.n_rho >= 1, f + ": the step-size table needs at least one entry");
  PXM_REQUIRE(std::isfinite(a.lmda) && a.lmda > 0 && std::isfinite(a.delta) && a.delta > 0,
              f + ": lmda, delta and d must be positive and finite");
  PXM_REQUIRE(a.eta_min <= a.eta_max, f + ": eta_min must not exceed eta_max");  // (false for a NaN bound)
  PXM_REQUIRE(a.n_trace >= 0 && (a.trace || a.n_trace == 0), f + ": a trace of n_trace > 0 rows needs its array");
  if (int rc = check_noise_arg(fn, a.noise_complex, a.dtype)) return rc;
  if (a.n > 0) {
    PXM_REQUIRE(a.X && a.gradg && a.X_out, f + ": null buffer");
    PXM_REQUIRE(a.X_out != a.X && a.X_out != a.gradg && a.X_out != a.noise, f + ": X_out must not alias an input");
  }
  PXM_REQUIRE(!dvec || a.X_out != (const void*)dvec, f + ": X_out must not alias an input");
  for (const void* o : {(const void*)a.theta, (const void*)a.eta, (const void*)a.trace, (const void*)a.scratch}) {
    if (!o) continue;
    PXM_REQUIRE(o != a.X && o != a.gradg && o != a.noise && o != (const void*)a.T && o != (const void*)a.rho_table &&
                    o != (const void*)dvec && o != a.X_out,
                f + ": an output must not alias an input");
  }
  PXM_REQUIRE(a.theta != a.eta && a.theta != a.scratch && a.eta != a.scratch && a.trace != a.theta && a.trace != a.eta &&
                  a.trace != a.scratch,
              f + ": theta, eta, trace and scratch must be different arrays");
  return 0;
}

// the step kernel on `slices` workgroups per chain (none with n == 0), then the update kernel
template <bool GROUPS>
static int sapg_launch(const char* fn, const SapgArgs& a, int slices, const SapgGroups<GROUPS>& gr, double d, const double* dvec) {
  int K = 1;
  if constexpr (GROUPS) K = gr.K;
  double* gsum = a.scratch + (int64_t)PXM_SAPG_SLICES_MAX * K * a.C;
  if (a.n > 0) {
    const dim3 g((unsigned)slices, (unsigned)a.C);
    const NoiseSrc ns = make_noise_src(a.noise, a.noise_complex, a.seed, a.chain0, a.iter, a.iter_dev);
#define PXM_SAPG_LAUNCH(CPLX, NZ)                                                                                   \
  hipLaunchKernelGGL((k_sapg_step<CPLX, NZ, GROUPS>), g, dim3(256), 0, a.st, (const double*)a.X, (const double*)a.gradg, a.T, \
                     a.T_scalar, (const double*)a.theta, a.delta, a.lmda, ns, (double*)a.X_out, a.scratch, a.n, gr)
    switch (a.noise ? 0 : 1 + ns.f64 + 2 * ns.noise_complex + (a.dtype ? 8 : 0)) {  // (complex noise needs a complex state)
      case 0: if (a.dtype) PXM_SAPG_LAUNCH(true, 0); else PXM_SAPG_LAUNCH(false, 0); break;
      case 1: PXM_SAPG_LAUNCH(false, 1); break;
      case 2: PXM_SAPG_LAUNCH(false, 2); break;
      case 9: PXM_SAPG_LAUNCH(true, 1); break;
      case 10: PXM_SAPG_LAUNCH(true, 2); break;
      case 11: PXM_SAPG_LAUNCH(true, 3); break;
      case 12: PXM_SAPG_LAUNCH(true, 4); break;
      default: PXM_REQUIRE(false, std::string(fn) + ": complex noise needs a complex state");
    }
#undef PXM_SAPG_LAUNCH
  }
  const SapgUpdate u{a.lmda, d, a.eta_min, a.eta_max, a.rho_table, a.n_rho, a.n_trace, a.iter, a.iter_dev, a.pool ? 1 : 0};
  const int threads = a.C >= 16 ? 1024 : 64 * a.C;  // one wave per chain up to 16; one workgroup per group
  hipLaunchKernelGGL(k_sapg_update<GROUPS>, dim3(K), dim3(threads), 0, a.st, (const double*)a.scratch, slices, a.C, u, gsum,
                     a.theta, a.eta, a.trace, gr, dvec);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int pxm_sapg_step(const void* X, const void* gradg, const double* T, double T_scalar, double delta, double lmda,
                  const void* noise, int noise_complex, uint64_t seed, uint64_t chain0, uint64_t iter,
                  const uint64_t* iter_dev, double* theta, double* eta, double d, const double* rho_table, int64_t n_rho,
                  double eta_min, double eta_max, int pool, double* trace, int64_t n_trace, void* X_out, double* scratch,
                  int64_t n, int C, int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0, "pxm_sapg_step: bad n / C / dtype");
  PXM_REQUIRE(std::isfinite(d) && d > 0, "pxm_sapg_step: lmda, delta and d must be positive and finite");
  const SapgArgs a{X, gradg, T, T_scalar, delta, lmda, noise, noise_complex, seed, chain0, iter, iter_dev, theta, eta, rho_table,
                   n_rho, eta_min, eta_max, pool, trace, n_trace, X_out, scratch, n, C, dtype, (hipStream_t)stream};
  if (int rc = sapg_check("pxm_sapg_step", a, nullptr)) return rc;
  const int slices = n > 0 ? chain_slices(n, PXM_SAPG_SLICES_MAX) : 0;
  return sapg_launch<false>("pxm_sapg_step", a, slices, SapgGroups<false>{}, d, nullptr);
}

int pxm_sapg_step_groups(const void* X, const void* gradg, const double* T, double T_scalar, double delta, double lmda,
                         const void* noise, int noise_complex, uint64_t seed, uint64_t chain0, uint64_t iter,
                         const uint64_t* iter_dev, double* theta, double* eta, const int64_t* bounds, int K, const double* d,
                         const double* rho_table, int64_t n_rho, double eta_min, double eta_max, int pool, double* trace,
                         int64_t n_trace, void* X_out, double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream) {
  const char* fn = "pxm_sapg_step_groups";
  PXM_REQUIRE(n >= 1, "pxm_sapg_step_groups: bad n / C / dtype (a group cannot be empty: n >= 1)");
  PXM_REQUIRE(K >= 1 && K <= PXM_SAPG_GROUPS_MAX, "pxm_sapg_step_groups: K must lie in 1 ... PXM_SAPG_GROUPS_MAX");
  PXM_REQUIRE(bounds && d, "pxm_sapg_step_groups: null buffer");
  PXM_REQUIRE(bounds[0] == 0 && bounds[K] == n, "pxm_sapg_step_groups: the group offsets must run from 0 to n");
  SapgGroups<true> gr{};
  gr.K = K;
  for (int k = 0; k < K; ++k) {
    PXM_REQUIRE(bounds[k] < bounds[k + 1], "pxm_sapg_step_groups: the group offsets must increase strictly (no empty group)");
    gr.b[k] = bounds[k];
    gr.s[k + 1] = gr.s[k] + chain_slices(bounds[k + 1] - bounds[k], PXM_SAPG_SLICES_MAX);
  }
  gr.b[K] = n;
  const SapgArgs a{X, gradg, T, T_scalar, delta, lmda, noise, noise_complex, seed, chain0, iter, iter_dev, theta, eta, rho_table,
                   n_rho, eta_min, eta_max, pool, trace, n_trace, X_out, scratch, n, C, dtype, (hipStream_t)stream};
  if (int rc = sapg_check(fn, a, d)) return rc;
  return sapg_launch<true>(fn, a, gr.s[K], gr, 0.0, d);
}

}  // extern "C"
