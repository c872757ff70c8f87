// The conditional draw of the prior precisions given the field: the second half of a Gibbs sweep on the Gaussian posterior
// (Wandelt, Larson & Lakshminarayanan 2004; Jewell, Levin & Anderson 2004).  The state is cut into K
// contiguous groups with one precision each; given the field x the precision of group k is
//
//   D_k = chi2_nu / sigma_k,   sigma_k = sum_{i in k} |x_i|^2,   nu_k = dof n_k + 2 q - 2
//
// for the hyper-prior p(v) ~ v^-q on the variance v = 1 / D (dof = 2 for a complex state, 1 for a real one).  The chi-square
// deviate is a sum of nu_k squared normals of the Philox stream: deviate t of group k is component t & 1 of the fp64
// complex-stream pair at counter index b_k + k + (t >> 1), so group k owns the indices b_k + k ... b_{k+1} + k -- one more
// pair than it has elements, which covers every nu up to 2 n_k + 2 -- and the index ranges of the groups are disjoint.
//
// pxm_group_variance_draw is three launches:
//   k_gibbs_slices  one workgroup per (slice, chain): the groups are cut into slices of PXM_GIBBS_SLICE elements by a table the
//                   host built, so a workgroup stays inside one group.  A lane takes the elements lo + tid, lo + tid + 256, ...
//                   of its slice and the Philox pairs of the same local indices; the group's last slice also takes the one
//                   pair past n_k.  The Philox bits of a lane's pairs are formed first, the Box-Muller step then runs pair by
//                   pair (philox.h).  Partials of sigma and chi2 through block_sum.
//   k_gibbs_finish  one wave per (group, chain): slice_sum of the group's slices in fixed order (reduce.h), so a group's sums
//                   depend on its length only; the division, the clamp, Dg and the trace row.
//   k_gibbs_expand  one workgroup per (slice, chain): D, sqrt(D) and M^-1 = 1 / (D + h_c) of every element, the [C][n] arrays
//                   the CG launches read in place.
// No atomics, no host read, no data-dependent loop.  Pure streams: the slice pass reads the state once (16 bytes per complex
// element), the expansion writes 24 bytes per element; the draw's cost is the Philox and Box-Muller arithmetic of nu / 2 pairs.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"
#include "reduce.h"

#include <cmath>

namespace pxm {

constexpr int GIBBS_S = PXM_GIBBS_SLICE;
constexpr int GIBBS_PER = GIBBS_S / 256;  // elements (and Philox pairs) per lane of a slice
static_assert(GIBBS_S % 256 == 0 && GIBBS_PER >= 1, "a slice is a whole number of passes of the workgroup");

// What a workgroup or wave needs to know of its group.  `inside`: the offsets lie in the state; `sampled`: and it is drawn.
struct GibbsGroup {
  int64_t b0, nk, nu;
  bool inside, sampled;
};
template <bool CPLX>
__device__ __forceinline__ GibbsGroup gibbs_group(const int64_t* __restrict__ bounds, const int32_t* __restrict__ fixed, int64_t k,
                                                  int K, int two_q, int64_t n) {
  GibbsGroup g{0, 0, 0, false, false};
  if (k < 0 || k >= K) return g;
  const int64_t b0 = bounds[k], b1 = bounds[k + 1];
  if (b0 < 0 || b1 > n || b1 <= b0) return g;
  g.b0 = b0, g.nk = b1 - b0;
  g.nu = (CPLX ? 2 : 1) * g.nk + two_q - 2;
  g.inside = true;
  g.sampled = fixed[k] == 0 && g.nu >= 1;
  return g;
}

template <bool CPLX>
__global__ __launch_bounds__(256) void k_gibbs_slices(const double* __restrict__ X, const int64_t* __restrict__ bounds,
                                                      const int64_t* __restrict__ tab, const int32_t* __restrict__ fixed, int K,
                                                      int two_q, uint64_t seed, uint64_t chain0, uint64_t iter,
                                                      double* __restrict__ part, int64_t n) {
#pragma clang fp contract(off)  // sums and products as written
  const int64_t s = blockIdx.x;
  const int c = blockIdx.y;
  const int64_t k = tab[2 * s], j = tab[2 * s + 1];
  const GibbsGroup g = gibbs_group<CPLX>(bounds, fixed, k, K, two_q, n);
  const int64_t lo = j * GIBBS_S;  // the slice's first element, counted from the group's
  if (!g.sampled || j < 0 || lo >= g.nk) return;  // (uniform over the workgroup; the finishing wave skips the same groups)
  const uint64_t chain = chain0 + (uint64_t)c, idx0 = (uint64_t)(g.b0 + k);
  uint4 bits[GIBBS_PER];
#pragma unroll
  for (int r = 0; r < GIBBS_PER; ++r) {
    const int64_t jl = lo + r * 256 + threadIdx.x;
    bits[r] = (jl < g.nk && 2 * jl < g.nu) ? philox_bits(seed, chain, idx0 + (uint64_t)jl, iter) : uint4{0, 0, 0, 0};
  }
  const int64_t base = (int64_t)c * n + g.b0;
  double sig = 0.0, chi = 0.0;
#pragma unroll
  for (int r = 0; r < GIBBS_PER; ++r) {
    const int64_t jl = lo + r * 256 + threadIdx.x;
    if (jl >= g.nk) continue;
    if constexpr (CPLX) {
      const double2 x = reinterpret_cast<const double2*>(X)[base + jl];
      sig += abs2_plain(x.x, x.y);
    } else {
      const double x = X[base + jl];
      sig += x * x;
    }
    if (2 * jl < g.nu) {
      const NormalPair z = normal_pair_from_bits(bits[r]);
      chi += z.z0 * z.z0;
      if (2 * jl + 1 < g.nu) chi += z.z1 * z.z1;
    }
  }
  // the pair past the group's elements: the last slice's, added by its first lane after that lane's own terms
  if (threadIdx.x == 0 && lo + GIBBS_S >= g.nk && 2 * g.nk < g.nu) {
    const NormalPair z = normal_pair_from_bits(philox_bits(seed, chain, idx0 + (uint64_t)g.nk, iter));
    chi += z.z0 * z.z0;
    if (2 * g.nk + 1 < g.nu) chi += z.z1 * z.z1;
  }
  block_sum<4>(sig, chi);
  if (threadIdx.x == 0) {
    double* p = part + ((int64_t)c * gridDim.x + s) * 2;
    p[0] = sig, p[1] = chi;
  }
}

// One wave per (group, chain), the only writer of Dg[c][k].
template <bool CPLX>
__global__ __launch_bounds__(64) void k_gibbs_finish(const double* __restrict__ part, const int64_t* __restrict__ bounds,
                                                     const int64_t* __restrict__ gs0, const int32_t* __restrict__ fixed, int K,
                                                     int two_q, int64_t nslices, double d_lo, double d_hi, double* __restrict__ Dg,
                                                     double* __restrict__ sums, double* __restrict__ trow, int64_t n) {
#pragma clang fp contract(off)
  const int k = blockIdx.x, c = blockIdx.y;
  const GibbsGroup g = gibbs_group<CPLX>(bounds, fixed, k, K, two_q, n);
  const int64_t at = (int64_t)c * K + k;
  double d = Dg[at];
  if (g.sampled) {  // (uniform over the wave)
    const int64_t s0 = gs0[k], ns = gs0[k + 1] - s0;
    if (s0 < 0 || ns < 1 || s0 + ns > nslices || ns != (g.nk + GIBBS_S - 1) / GIBBS_S) return;  // not the table of these groups
    double sig, chi;
    slice_sum<2>(part + ((int64_t)c * nslices + s0) * 2, (int)ns, threadIdx.x, sig, chi);
    d = sig > 0.0 ? fmin(fmax(chi / sig, d_lo), d_hi) : d_hi;
    if (threadIdx.x == 0) {
      Dg[at] = d;
      if (sums) sums[2 * at] = sig, sums[2 * at + 1] = chi;
    }
  }
  if (threadIdx.x == 0 && trow) trow[at] = d;
}

__global__ __launch_bounds__(256) void k_gibbs_expand(const int64_t* __restrict__ bounds, const int64_t* __restrict__ tab,
                                                      const int32_t* __restrict__ fixed, int K, const double* __restrict__ Dg,
                                                      const double* __restrict__ H, double Hs, double* __restrict__ D,
                                                      double* __restrict__ sqrtD, double* __restrict__ Minv, int64_t n) {
#pragma clang fp contract(off)
  const int64_t s = blockIdx.x;
  const int c = blockIdx.y;
  const int64_t k = tab[2 * s], j = tab[2 * s + 1];
  const GibbsGroup g = gibbs_group<false>(bounds, fixed, k, K, 0, n);  // (nu is not read here)
  const int64_t lo = j * GIBBS_S;
  if (!g.inside || j < 0 || lo >= g.nk) return;
  const double d = Dg[(int64_t)c * K + k];
  const double sd = sqrt(d), mi = 1.0 / (d + (H ? H[c] : Hs));
  const int64_t base = (int64_t)c * n + g.b0;
#pragma unroll
  for (int r = 0; r < GIBBS_PER; ++r) {
    const int64_t jl = lo + r * 256 + threadIdx.x;
    if (jl >= g.nk) continue;
    D[base + jl] = d;
    sqrtD[base + jl] = sd;
    Minv[base + jl] = mi;
  }
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int pxm_group_variance_draw(const void* X, const int64_t* bounds, int K, const int64_t* slice_tab, const int64_t* group_slice0,
                            int64_t nslices, const int32_t* fixed, int two_q, const double* h, double h_scalar, double d_lo,
                            double d_hi, uint64_t seed, uint64_t chain0, uint64_t iter, double* Dg, double* sums, double* trace,
                            int64_t n_trace, int64_t trace_row, double* D, double* sqrtD, double* Minv, double* scratch,
                            int64_t n, int C, int dtype, int expand_only, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 1 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_group_variance_draw: bad n / C / dtype");
  PXM_REQUIRE(K >= 1 && K <= n && nslices >= K && nslices <= n && nslices <= 0x7fffffff,
              "pxm_group_variance_draw: K groups need K <= nslices <= n");
  PXM_REQUIRE(bounds && slice_tab && group_slice0 && fixed && Dg && D && sqrtD && Minv,
              "pxm_group_variance_draw: null buffer");
  PXM_REQUIRE(std::isfinite(d_lo) && std::isfinite(d_hi) && d_lo > 0 && d_lo <= d_hi,
              "pxm_group_variance_draw: the clamp needs finite 0 < d_lo <= d_hi");
  PXM_REQUIRE(h || (std::isfinite(h_scalar) && h_scalar >= 0), "pxm_group_variance_draw: h must be finite and not negative");
  PXM_REQUIRE(two_q >= -(1 << 20) && two_q <= 4, "pxm_group_variance_draw: two_q must be at most 4 (q <= 2)");
  PXM_REQUIRE(n_trace >= 0 && (trace || n_trace == 0) && trace_row >= 0, "pxm_group_variance_draw: bad trace");
  const void* outs[] = {Dg, sums, trace, D, sqrtD, Minv, scratch};
  const void* ins[] = {X, bounds, slice_tab, group_slice0, fixed, h};
  for (int a = 0; a < 7; ++a) {
    if (!outs[a]) continue;
    for (int b = a + 1; b < 7; ++b) PXM_REQUIRE(outs[a] != outs[b], "pxm_group_variance_draw: the outputs must all be different");
    for (int b = 0; b < 6; ++b) PXM_REQUIRE(outs[a] != ins[b], "pxm_group_variance_draw: an output must not alias an input");
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 gs((unsigned)nslices, (unsigned)C), gk((unsigned)K, (unsigned)C);
  if (!expand_only) {
    PXM_REQUIRE(X && scratch, "pxm_group_variance_draw: null buffer");
    double* trow = (trace && trace_row < n_trace) ? trace + trace_row * (int64_t)C * K : nullptr;
    const double* x = (const double*)X;
    if (dtype) {
      hipLaunchKernelGGL(k_gibbs_slices<true>, gs, dim3(256), 0, st, x, bounds, slice_tab, fixed, K, two_q, seed, chain0, iter, scratch, n);
      hipLaunchKernelGGL(k_gibbs_finish<true>, gk, dim3(64), 0, st, scratch, bounds, group_slice0, fixed, K, two_q, nslices, d_lo, d_hi, Dg, sums, trow, n);
    } else {
      hipLaunchKernelGGL(k_gibbs_slices<false>, gs, dim3(256), 0, st, x, bounds, slice_tab, fixed, K, two_q, seed, chain0, iter, scratch, n);
      hipLaunchKernelGGL(k_gibbs_finish<false>, gk, dim3(64), 0, st, scratch, bounds, group_slice0, fixed, K, two_q, nslices, d_lo, d_hi, Dg, sums, trow, n);
    }
  }
  hipLaunchKernelGGL(k_gibbs_expand, gs, dim3(256), 0, st, bounds, slice_tab, fixed, K, Dg, h, h_scalar, D, sqrtD, Minv, n);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
