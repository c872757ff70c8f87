// The per-chain reductions of the samplers (L1, L2, vdot, log transition probability) and their C-ABI: one workgroup per
// (chain, slice) writes a partial, a second kernel adds the partials -- the fixed order and the slice count of reduce.h.
// Every array is [C][n] (chain-major); data / invcov / weights are [n], shared by all chains.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"
#include "pxmala_sums.h"
#include "reduce.h"

namespace pxm {

template <bool CPLX>
__global__ void k_l1_partial(const double* __restrict__ X, const double* __restrict__ w, double* __restrict__ part,
                             int64_t n) {
  const int c = blockIdx.y;
  double acc = 0.0, none = 0.0;  // (the two-component sum of every reduction here; the second stays zero)
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double a;
    if (CPLX) {
      const double2 z = reinterpret_cast<const double2*>(X)[(int64_t)c * n + i];
      a = sqrt(fma(z.x, z.x, z.y * z.y));  // (no overflow guard needed: |z|^2 of a chain state is far inside fp64 range)
    } else a = fabs(X[(int64_t)c * n + i]);
    acc += w ? fabs(w[i]) * a : a;
  }
  block_sum2(acc, none);
  if (threadIdx.x == 0) part[((int64_t)c * gridDim.x + blockIdx.x) * 2] = acc, part[((int64_t)c * gridDim.x + blockIdx.x) * 2 + 1] = 0.0;
}

template <bool CPLX, bool ICPLX>
__global__ void k_l2_partial(const double* __restrict__ preds, const double* __restrict__ data,
                             const double* __restrict__ invcov, double* __restrict__ part, int64_t n) {
  l2_partial_body<CPLX, ICPLX>(preds, data, invcov, part, n, blockIdx.y, blockIdx.x, gridDim.x);
}

// vdot(a, b) = sum conj(a) * b per chain (logpi's L2 with a full inverse covariance: b = invcov @ a)
template <bool CPLX>
__global__ void k_vdot_partial(const double* __restrict__ A, const double* __restrict__ Bv, double* __restrict__ part, int64_t n) {
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  double2 acc{0.0, 0.0};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (CPLX) {
      const double2 a = reinterpret_cast<const double2*>(A)[base + i], b = reinterpret_cast<const double2*>(Bv)[base + i];
      acc.x += a.x * b.x + a.y * b.y;
      acc.y += a.x * b.y - a.y * b.x;
    } else {
      acc.x += A[base + i] * Bv[base + i];
    }
  }
  block_sum2(acc.x, acc.y);
  if (threadIdx.x == 0) reinterpret_cast<double2*>(part)[(int64_t)c * gridDim.x + blockIdx.x] = acc;
}

template <bool CPLX>
__global__ void k_logtrans_partial(const double* __restrict__ X1, const double* __restrict__ X2,
                                   const double* __restrict__ P, const double* __restrict__ G,
                                   const double* __restrict__ delta_dev, double delta, double lmda,
                                   double* __restrict__ part, int64_t n) {
  const int c = blockIdx.y;
  logtrans_partial_body<CPLX>(X1, X2, P, G, delta_dev ? delta_dev[c] : delta, lmda, part, n, c, blockIdx.x, gridDim.x);
}

// mode 0: out[c] = sum of partials; mode 1 (logtransition): out[c] = -(d/2) * S^2 (complex)
__global__ void k_reduce_final(const double* __restrict__ part, double* __restrict__ out, int slices, int mode,
                               const double* __restrict__ delta_dev, double delta) {
  const int c = blockIdx.x;
  double2 v;
  slice_sum<2>(part + (int64_t)c * slices * 2, slices, threadIdx.x, v.x, v.y);
  if (threadIdx.x == 0) {
    if (mode == 1) {
      const double d = delta_dev ? delta_dev[c] : delta;
      const double2 s2 = cmul(v, v);
      v = double2{-(1.0 / 2 * d) * s2.x, -(1.0 / 2 * d) * s2.y};
    }
    reinterpret_cast<double2*>(out)[c] = v;
  }
}

__global__ void k_l1_store(const double* __restrict__ red, double* __restrict__ out, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) out[c] = red[2 * c];
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int64_t pxm_reduce_scratch_doubles(int C) { return C >= 1 ? (int64_t)red_scratch_doubles(C) : -1; }

int pxm_reduce_l1(const void* X, const double* w, double* out, double* scratch, int64_t n, int C, int dtype,
                  pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && (dtype == 0 || dtype == 1), "pxm_reduce_l1: bad n / C / dtype");
  hipStream_t st = (hipStream_t)stream;
  PXM_REQUIRE(X && out && scratch, "pxm_reduce_l1: null buffer");
  double* part = scratch;
  const int RS = red_slices(n);
  dim3 g(RS, C), b(256);
  if (dtype) hipLaunchKernelGGL(k_l1_partial<true>, g, b, 0, st, (const double*)X, w, part, n);
  else hipLaunchKernelGGL(k_l1_partial<false>, g, b, 0, st, (const double*)X, w, part, n);
  double* red = part + (size_t)C * RS * 2;
  // final sums land in the tail of the scratch, then the real parts are compacted to out[C]
  hipLaunchKernelGGL(k_reduce_final, dim3(C), dim3(64), 0, st, part, red, RS, 0, (const double*)nullptr, 0.0);
  hipLaunchKernelGGL(k_l1_store, dim3((C + 63) / 64), dim3(64), 0, st, red, out, C);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_reduce_l2(const void* preds, const void* data, const void* invcov, int invcov_complex, double* out,
                  double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && (dtype == 0 || dtype == 1), "pxm_reduce_l2: bad n / C / dtype");
  PXM_REQUIRE(dtype == 1 || !invcov_complex, "pxm_reduce_l2: complex invcov needs complex data");
  hipStream_t st = (hipStream_t)stream;
  PXM_REQUIRE(preds && data && invcov && out && scratch, "pxm_reduce_l2: null buffer");
  double* part = scratch;
  const int RS = red_slices(n);
  dim3 g(RS, C), b(256);
  const double *p = (const double*)preds, *d = (const double*)data, *ic = (const double*)invcov;
  if (dtype && invcov_complex) hipLaunchKernelGGL((k_l2_partial<true, true>), g, b, 0, st, p, d, ic, part, n);
  else if (dtype) hipLaunchKernelGGL((k_l2_partial<true, false>), g, b, 0, st, p, d, ic, part, n);
  else hipLaunchKernelGGL((k_l2_partial<false, false>), g, b, 0, st, p, d, ic, part, n);
  hipLaunchKernelGGL(k_reduce_final, dim3(C), dim3(64), 0, st, part, out, RS, 0, (const double*)nullptr, 0.0);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_reduce_vdot(const void* a, const void* b, double* out, double* scratch, int64_t n, int C, int dtype,
                    pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && (dtype == 0 || dtype == 1), "pxm_reduce_vdot: bad n / C / dtype");
  PXM_REQUIRE(a && b && out && scratch, "pxm_reduce_vdot: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const int RS = red_slices(n);
  dim3 g(RS, C), blk(256);
  if (dtype) hipLaunchKernelGGL(k_vdot_partial<true>, g, blk, 0, st, (const double*)a, (const double*)b, scratch, n);
  else hipLaunchKernelGGL(k_vdot_partial<false>, g, blk, 0, st, (const double*)a, (const double*)b, scratch, n);
  hipLaunchKernelGGL(k_reduce_final, dim3(C), dim3(64), 0, st, scratch, out, RS, 0, (const double*)nullptr, 0.0);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_logtransition(const void* X1, const void* X2, const void* proxf, const void* gradg, const double* delta_dev,
                      double delta, double lmda, double* out, double* scratch, int64_t n, int C, int dtype,
                      pxm_stream_t stream) {
  PXM_REQUIRE(n >= 0 && C >= 1 && (dtype == 0 || dtype == 1), "pxm_logtransition: bad n / C / dtype");
  hipStream_t st = (hipStream_t)stream;
  PXM_REQUIRE(X1 && X2 && proxf && gradg && out && scratch, "pxm_logtransition: null buffer");
  double* part = scratch;
  const int RS = red_slices(n);
  dim3 g(RS, C), b(256);
  if (dtype)
    hipLaunchKernelGGL(k_logtrans_partial<true>, g, b, 0, st, (const double*)X1, (const double*)X2, (const double*)proxf,
                       (const double*)gradg, delta_dev, delta, lmda, part, n);
  else
    hipLaunchKernelGGL(k_logtrans_partial<false>, g, b, 0, st, (const double*)X1, (const double*)X2,
                       (const double*)proxf, (const double*)gradg, delta_dev, delta, lmda, part, n);
  hipLaunchKernelGGL(k_reduce_final, dim3(C), dim3(64), 0, st, part, out, RS, 1, delta_dev, delta);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
