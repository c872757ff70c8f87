// Local credible intervals from the MAP point.  Per slot c (one region of the image) the objective
// along the surrogate X(xi) = a + xi b is the convex function of one real variable
//
//   F(xi) = q0 + q1 xi + q2 xi^2 + (1 / lmda) P(xi),   P(xi) = sum_k T_k |a_k + xi b_k|
//
// and the interval is {xi : F(xi) <= gamma}.  Three entry points:
//   pxm_lci_data_terms  (q0, q1, q2) of every slot in one pass over the predictions of a and b;
//   pxm_lci_eval        P at 32 values of xi per slot in one pass over a, b and T (and S_a = sum T|a|, S_b = sum T|b|);
//   pxm_lci_search      the whole search: an initialisation kernel, then `rounds` times (eval, finish, refine).
// The number of rounds is a host argument and every device loop runs over n (grid stride), the slices of a slot or the 32
// points: no trip count depends on the data, and nothing waits.  Every sum is a fixed-order sum of reduce.h with a slice
// count that depends on n only, so a slot's numbers do not depend on the batch it runs in.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "reduce.h"

#include <cmath>
#include <utility>

namespace pxm {

constexpr int LCI_NXI = PXM_LCI_POINTS;  // values of xi per slot and pass
constexpr int LCI_NP = LCI_NXI + 2;      // sums per slot and pass: P(xi_0 ... xi_31), S_a, S_b
constexpr int LCI_HALF = LCI_NXI / 2;    // points per end in the split phase
constexpr int LCI_SLICES_MAX = 512;
using LciIdx = std::make_index_sequence<LCI_NXI>;

// workgroups (slices) per slot: one per 1024 elements (four per lane) up to LCI_SLICES_MAX, grid-stride beyond
static inline int lci_slices(int64_t n) {
  const int64_t s = (n + 1023) / 1024;
  return (int)(s < 1 ? 1 : (s > LCI_SLICES_MAX ? LCI_SLICES_MAX : s));
}

// the helpers of reduce.h take their components as a pack of lvalues: the 32 accumulators, then the two prior sums
template <size_t... I>
__device__ __forceinline__ void lci_block_sum(double (&p)[LCI_NXI], double& sa, double& sb, std::index_sequence<I...>) {
  block_sum<4>(p[I]..., sa, sb);
}
template <size_t... I>
__device__ __forceinline__ void lci_slice_sum(const double* __restrict__ row, int slices, int lane, double (&p)[LCI_NXI],
                                              double& sa, double& sb, std::index_sequence<I...>) {
  slice_sum<LCI_NP>(row, slices, lane, p[I]..., sa, sb);
}

// part[c][slice][0 .. 33]: the slice's share of P(xi_cj), S_a, S_b.  The slot's xi are the same for every lane (blockIdx.y
// selects them): uniform loads into scalar registers; the accumulators stay in vector registers.  The modulus is formed
// from (a_re + xi b_re, a_im + xi b_im), each with one rounding: the expanded quadratic |a|^2 + 2 xi Re(conj(a) b) + xi^2
// |b|^2 cancels near a kink a_k + xi b_k = 0, where the shape of F is decided.
template <bool CPLX, bool TVEC>
__global__ __launch_bounds__(256) void k_lci_eval(const double* __restrict__ A, const double* __restrict__ B,
                                                  const double* __restrict__ T, double Ts, const double* __restrict__ xi,
                                                  double* __restrict__ part, int64_t n) {
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  const double* __restrict__ xc = xi + (int64_t)c * LCI_NXI;
  double x[LCI_NXI], p[LCI_NXI];
#pragma unroll
  for (int j = 0; j < LCI_NXI; ++j) x[j] = xc[j], p[j] = 0.0;
  double sa = 0.0, sb = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double t = TVEC ? T[i] : Ts;
    if constexpr (CPLX) {
      const double2 a = reinterpret_cast<const double2*>(A)[base + i], b = reinterpret_cast<const double2*>(B)[base + i];
#pragma unroll
      for (int j = 0; j < LCI_NXI; ++j) {
        const double re = fma(x[j], b.x, a.x), im = fma(x[j], b.y, a.y);
        p[j] += t * sqrt(fma(re, re, im * im));
      }
      sa += t * sqrt(fma(a.x, a.x, a.y * a.y));
      sb += t * sqrt(fma(b.x, b.x, b.y * b.y));
    } else {
      const double a = A[base + i], b = B[base + i];
#pragma unroll
      for (int j = 0; j < LCI_NXI; ++j) p[j] += t * fabs(fma(x[j], b, a));
      sa += t * fabs(a);
      sb += t * fabs(b);
    }
  }
  lci_block_sum(p, sa, sb, LciIdx{});
  if (threadIdx.x == 0) {
    double* o = part + ((int64_t)c * gridDim.x + blockIdx.x) * LCI_NP;
#pragma unroll
    for (int j = 0; j < LCI_NXI; ++j) o[j] = p[j];
    o[LCI_NXI] = sa, o[LCI_NXI + 1] = sb;
  }
}

// P[c][0 .. 33] = the slot's partials added in the fixed order (reduce.h: slice_sum)
__global__ __launch_bounds__(64) void k_lci_finish(const double* __restrict__ part, int slices, double* __restrict__ P) {
  const int c = blockIdx.x;
  double p[LCI_NXI], sa, sb;
  lci_slice_sum(part + (int64_t)c * slices * LCI_NP, slices, threadIdx.x, p, sa, sb, LciIdx{});
  if (threadIdx.x == 0) {
    double* o = P + (int64_t)c * LCI_NP;
#pragma unroll
    for (int j = 0; j < LCI_NXI; ++j) o[j] = p[j];
    o[LCI_NXI] = sa, o[LCI_NXI + 1] = sb;
  }
}

// part[c][slice][0 .. 2]: sum w |r|^2, sum w Re(conj(r) s), sum w |s|^2 with r = preds_a - data, s = preds_b
template <bool CPLX>
__global__ __launch_bounds__(256) void k_lci_data(const double* __restrict__ PA, const double* __restrict__ PB,
                                                  const double* __restrict__ D, const double* __restrict__ W,
                                                  double* __restrict__ part, int64_t n) {
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  double q0 = 0.0, q1 = 0.0, q2 = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double w = W[i];
    if constexpr (CPLX) {
      const double2 pa = reinterpret_cast<const double2*>(PA)[base + i], s = reinterpret_cast<const double2*>(PB)[base + i];
      const double2 d = reinterpret_cast<const double2*>(D)[i];
      const double rx = pa.x - d.x, ry = pa.y - d.y;
      q0 += w * fma(rx, rx, ry * ry);
      q1 += w * fma(rx, s.x, ry * s.y);
      q2 += w * fma(s.x, s.x, s.y * s.y);
    } else {
      const double r = PA[base + i] - D[i], s = PB[base + i];
      q0 += w * (r * r);
      q1 += w * (r * s);
      q2 += w * (s * s);
    }
  }
  block_sum<4>(q0, q1, q2);
  if (threadIdx.x == 0) {
    double* o = part + ((int64_t)c * gridDim.x + blockIdx.x) * 3;
    o[0] = q0, o[1] = q1, o[2] = q2;
  }
}

// quad[c] = (q0, q1, q2) = (1/2 sum w |r|^2, sum w Re(conj(r) s), 1/2 sum w |s|^2); the halvings are exact
__global__ __launch_bounds__(64) void k_lci_data_finish(const double* __restrict__ part, int slices, double* __restrict__ quad) {
  const int c = blockIdx.x;
  double q0, q1, q2;
  slice_sum<3>(part + (int64_t)c * slices * 3, slices, threadIdx.x, q0, q1, q2);
  if (threadIdx.x == 0) quad[c * 3 + 0] = 0.5 * q0, quad[c * 3 + 1] = q1, quad[c * 3 + 2] = 0.5 * q2;
}

// ---- the search ------------------------------------------------------------------------------------------------------------
// A slot's state between two rounds.  joint: the sublevel set lies in [lo, hi].  split: its lower end lies in [lo, lo_in],
// its upper end in [hi_in, hi], and F <= gamma was seen at lo_in and hi_in.  pending: q2 == 0, the bracket waits for S_a and
// S_b of the first pass.  done: nothing is left to evaluate.
enum LciMode : int { LCI_JOINT = 0, LCI_SPLIT = 1, LCI_DONE = 2, LCI_PENDING = 3 };
struct LciState {
  double lo, lo_in, hi_in, hi, fmin, ximin, outer_lo, outer_hi;
  int mode, status;
};
constexpr int LCI_STATE_DOUBLES = (sizeof(LciState) + 7) / 8;

__device__ __forceinline__ void lci_done(LciState& s, int status, double lower, double upper) {
  s.mode = LCI_DONE, s.status |= status;
  s.lo = s.lo_in = lower, s.hi = s.hi_in = upper;
}

// the 32 points of the next pass: joint, evenly over [lo, hi] with both ends; split, the 16 interior points j / 17 of each
// end's bracket (the ends of those brackets are known); otherwise zeros, whose sums nobody reads.  lo + (width * j) / 31: the
// product first, so that a bracket such as [-31, 31] has exactly the grid points -31, -29, ..., 31
__device__ __forceinline__ void lci_points(const LciState& s, double* __restrict__ xi) {
  for (int j = 0; j < LCI_NXI; ++j) {
    double v = 0.0;
    if (s.mode == LCI_JOINT) {
      v = j == LCI_NXI - 1 ? s.hi : fmin(s.lo + (s.hi - s.lo) * j / (LCI_NXI - 1), s.hi);
    } else if (s.mode == LCI_SPLIT) {
      if (j < LCI_HALF) v = fmin(s.lo + (s.lo_in - s.lo) * (j + 1) / (LCI_HALF + 1), s.lo_in);
      else v = fmin(s.hi_in + (s.hi - s.hi_in) * (j - LCI_HALF + 1) / (LCI_HALF + 1), s.hi);
    }
    xi[j] = v;
  }
}

// out[c] = (lower, upper, width of the lower bracket, of the upper bracket, smallest F seen, its xi, outer bracket lo, hi).
// A slot that is still joint has seen no point with F <= gamma: empty, with the bracket of the minimiser.
__device__ __forceinline__ void lci_result(const LciState& s, double* __restrict__ o, int* __restrict__ status) {
  const double nan = __builtin_nan("");
  int st = s.status;
  double lower = s.lo_in, upper = s.hi_in, wlo = s.lo_in - s.lo, whi = s.hi - s.hi_in, fmin = s.fmin, ximin = s.ximin;
  if (s.mode == LCI_JOINT) st |= PXM_LCI_EMPTY, lower = s.lo, upper = s.hi, wlo = whi = s.hi - s.lo;
  if (s.mode == LCI_PENDING) st |= PXM_LCI_EMPTY, lower = upper = wlo = whi = nan;
  if (s.mode == LCI_DONE) wlo = whi = (st & (PXM_LCI_EMPTY | PXM_LCI_NONFINITE)) ? nan : 0.0;
  if (st & PXM_LCI_NONFINITE) lower = upper = fmin = ximin = nan;
  o[0] = lower, o[1] = upper, o[2] = wlo, o[3] = whi, o[4] = fmin, o[5] = ximin, o[6] = s.outer_lo, o[7] = s.outer_hi;
  *status = st;
}

// The outer bracket.  F >= the quadratic (the prior term is >= 0), so with q2 > 0 the set lies between the roots of
// q(xi) = gamma, taken in the form that does not cancel; a negative discriminant: empty.
__global__ __launch_bounds__(64) void k_lci_init(const double* __restrict__ quad, const double* __restrict__ gamma,
                                                 LciState* __restrict__ state, double* __restrict__ xi,
                                                 double* __restrict__ out, int* __restrict__ status, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double q0 = quad[c * 3], q1 = quad[c * 3 + 1], q2 = quad[c * 3 + 2], g = gamma[c];
  const double nan = __builtin_nan("");
  LciState s;
  s.lo = s.lo_in = s.hi_in = s.hi = s.ximin = s.outer_lo = s.outer_hi = nan;
  s.fmin = __builtin_inf();
  s.mode = LCI_PENDING, s.status = 0;
  if (!(isfinite(q0) && isfinite(q1) && isfinite(q2) && isfinite(g))) {
    lci_done(s, PXM_LCI_NONFINITE, nan, nan);
  } else if (q2 > 0.0) {
    const double cc = q0 - g;
    const double disc = fma(q1, q1, -4.0 * q2 * cc);
    if (disc < 0.0) {
      lci_done(s, PXM_LCI_EMPTY, nan, nan);
    } else {
      const double t = -0.5 * (q1 + copysign(sqrt(disc), q1));
      const double r1 = t == 0.0 ? 0.0 : t / q2, r2 = t == 0.0 ? 0.0 : cc / t;
      s.lo = s.outer_lo = fmin(r1, r2), s.hi = s.outer_hi = fmax(r1, r2);
      s.mode = LCI_JOINT;
    }
  }
  lci_points(s, xi + (int64_t)c * LCI_NXI);
  state[c] = s;
  lci_result(s, out + (int64_t)c * 8, status + c);
}

// One round: F at the 32 points from the sums of the pass, then the new bracket(s) and the points of the next pass.
__global__ __launch_bounds__(64) void k_lci_refine(const double* __restrict__ quad, const double* __restrict__ gamma,
                                                   double lmda, const double* __restrict__ P, LciState* __restrict__ state,
                                                   double* __restrict__ xi, double* __restrict__ out,
                                                   int* __restrict__ status, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  LciState s = state[c];
  const double q0 = quad[c * 3], q1 = quad[c * 3 + 1], q2 = quad[c * 3 + 2], g = gamma[c];
  const double* __restrict__ Pc = P + (int64_t)c * LCI_NP;
  double* __restrict__ x = xi + (int64_t)c * LCI_NXI;
  const double nan = __builtin_nan("");
  bool finite = true;
  for (int j = 0; j < LCI_NP; ++j) finite = finite && isfinite(Pc[j]);
  if (!finite) {  // also for a slot the initialisation finished (its points are zeros: the sums still see a and b)
    s.status = 0;
    lci_done(s, PXM_LCI_NONFINITE, nan, nan);
  } else if (s.mode == LCI_DONE) {
    return;  // (its result and its points stand)
  } else if (s.mode == LCI_PENDING) {
    // q2 == 0: F >= q0 - |q1| |xi| + (|xi| S_b - S_a) / lmda.  (s = 0 gives q1 = 0; a q2 that underflowed may leave q1 != 0.)
    const double Sa = Pc[LCI_NXI], Sb = Pc[LCI_NXI + 1];
    const double D = Sb - lmda * fabs(q1);
    s.fmin = q0 + Pc[0] / lmda, s.ximin = 0.0;  // (the points of a pending slot are zeros)
    if (D > 0.0) {
      const double R = (lmda * (g - q0) + Sa) / D;
      if (R < 0.0) {
        lci_done(s, PXM_LCI_EMPTY, nan, nan);
      } else {
        s.lo = s.outer_lo = -R, s.hi = s.outer_hi = R;
        s.mode = LCI_JOINT;
      }
    } else if (q1 != 0.0 || s.fmin <= g) {  // F is constant, or falls without end on one side
      lci_done(s, PXM_LCI_UNCONSTRAINED, -__builtin_inf(), __builtin_inf());
    } else {
      lci_done(s, PXM_LCI_EMPTY, nan, nan);
    }
  } else {
    int first[2] = {-1, -1}, last[2] = {-1, -1}, jmin = 0;  // per half of the points: first / last with F <= gamma
    double fbest = __builtin_inf();
    for (int j = 0; j < LCI_NXI; ++j) {
      const double F = fma(fma(q2, x[j], q1), x[j], q0) + Pc[j] / lmda;
      const int h = j / LCI_HALF;
      if (F <= g) {
        if (first[h] < 0) first[h] = j;
        last[h] = j;
      }
      if (F < fbest) fbest = F, jmin = j;
    }
    if (fbest < s.fmin) s.fmin = fbest, s.ximin = x[jmin];
    if (s.mode == LCI_JOINT) {
      const int j0 = first[0] >= 0 ? first[0] : first[1], j1 = last[1] >= 0 ? last[1] : last[0];
      if (j0 >= 0) {  // the points inside form one run (convexity): each end lies between the run and its neighbour
        const double lo = x[j0 > 0 ? j0 - 1 : 0], hi = x[j1 < LCI_NXI - 1 ? j1 + 1 : LCI_NXI - 1];
        s.lo_in = x[j0], s.hi_in = x[j1];
        s.lo = lo, s.hi = hi;
        s.mode = LCI_SPLIT;
      } else {  // nothing inside: the set, if any, lies in a cell next to the grid's smallest value
        const double lo = x[jmin > 0 ? jmin - 1 : 0], hi = x[jmin < LCI_NXI - 1 ? jmin + 1 : LCI_NXI - 1];
        s.lo = lo, s.hi = hi;
      }
    } else {
      // lower end: the first interior point inside becomes the inner point, its left neighbour the outer one
      if (first[0] >= 0) {
        if (first[0] > 0) s.lo = x[first[0] - 1];
        s.lo_in = x[first[0]];
      } else {
        s.lo = x[LCI_HALF - 1];
      }
      // upper end: the last interior point inside, and its right neighbour
      if (last[1] >= 0) {
        if (last[1] < LCI_NXI - 1) s.hi = x[last[1] + 1];
        s.hi_in = x[last[1]];
      } else {
        s.hi = x[LCI_HALF];
      }
    }
  }
  lci_points(s, x);
  state[c] = s;
  lci_result(s, out + (int64_t)c * 8, status + c);
}

static inline size_t lci_part_doubles(int64_t n, int C) { return (size_t)C * lci_slices(n) * LCI_NP; }

static void lci_launch_eval(int dtype, dim3 g, hipStream_t st, const double* a, const double* b, const double* T, double Ts,
                            const double* xi, double* part, int64_t n) {
#define PXM_LCI_EVAL(CPLX, TVEC) hipLaunchKernelGGL((k_lci_eval<CPLX, TVEC>), g, dim3(256), 0, st, a, b, T, Ts, xi, part, n)
  if (dtype && T) PXM_LCI_EVAL(true, true);
  else if (dtype) PXM_LCI_EVAL(true, false);
  else if (T) PXM_LCI_EVAL(false, true);
  else PXM_LCI_EVAL(false, false);
#undef PXM_LCI_EVAL
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int64_t pxm_lci_scratch_doubles(int64_t n, int C) {
  if (n < 1 || C < 1) return -1;
  return (int64_t)(lci_part_doubles(n, C) + (size_t)C * (LCI_NXI + LCI_NP + LCI_STATE_DOUBLES));
}

int pxm_lci_data_terms(const void* preds_a, const void* preds_b, const void* data, const double* w, double* quad,
                       double* scratch, int64_t ndata, int C, int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(ndata >= 1 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_lci_data_terms: bad ndata / C / dtype");
  PXM_REQUIRE(preds_a && preds_b && data && w && quad && scratch, "pxm_lci_data_terms: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const int slices = lci_slices(ndata);
  const dim3 g((unsigned)slices, (unsigned)C);
  const double *pa = (const double*)preds_a, *pb = (const double*)preds_b, *d = (const double*)data;
  if (dtype) hipLaunchKernelGGL(k_lci_data<true>, g, dim3(256), 0, st, pa, pb, d, w, scratch, ndata);
  else hipLaunchKernelGGL(k_lci_data<false>, g, dim3(256), 0, st, pa, pb, d, w, scratch, ndata);
  hipLaunchKernelGGL(k_lci_data_finish, dim3(C), dim3(64), 0, st, scratch, slices, quad);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_lci_eval(const void* a, const void* b, const double* T, double T_scalar, const double* xi, double* P,
                 double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 1 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_lci_eval: bad n / C / dtype");
  PXM_REQUIRE(a && b && xi && P && scratch, "pxm_lci_eval: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const int slices = lci_slices(n);
  lci_launch_eval(dtype, dim3((unsigned)slices, (unsigned)C), st, (const double*)a, (const double*)b, T, T_scalar, xi,
                  scratch, n);
  hipLaunchKernelGGL(k_lci_finish, dim3(C), dim3(64), 0, st, scratch, slices, P);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_lci_search(const void* a, const void* b, const double* T, double T_scalar, const double* quad, double lmda,
                   const double* gamma, int rounds, double* out, int* status, double* scratch, int64_t n, int C, int dtype,
                   pxm_stream_t stream) {
  PXM_REQUIRE(n >= 1 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_lci_search: bad n / C / dtype");
  PXM_REQUIRE(rounds >= 1 && rounds <= PXM_LCI_ROUNDS_MAX, "pxm_lci_search: rounds must lie in 1 ... PXM_LCI_ROUNDS_MAX");
  PXM_REQUIRE(std::isfinite(lmda) && lmda > 0, "pxm_lci_search: lmda must be positive");
  PXM_REQUIRE(a && b && quad && gamma && out && status && scratch, "pxm_lci_search: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const int slices = lci_slices(n);
  double* part = scratch;
  double* xi = part + lci_part_doubles(n, C);
  double* P = xi + (size_t)C * LCI_NXI;
  LciState* state = reinterpret_cast<LciState*>(P + (size_t)C * LCI_NP);
  const dim3 gs((unsigned)((C + 63) / 64)), ge((unsigned)slices, (unsigned)C);
  hipLaunchKernelGGL(k_lci_init, gs, dim3(64), 0, st, quad, gamma, state, xi, out, status, C);
  for (int r = 0; r < rounds; ++r) {
    lci_launch_eval(dtype, ge, st, (const double*)a, (const double*)b, T, T_scalar, (const double*)xi, part, n);
    hipLaunchKernelGGL(k_lci_finish, dim3(C), dim3(64), 0, st, (const double*)part, slices, P);
    hipLaunchKernelGGL(k_lci_refine, gs, dim3(64), 0, st, quad, gamma, lmda, (const double*)P, state, xi, out, status, C);
  }
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
