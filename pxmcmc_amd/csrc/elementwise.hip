// HBM-bound elementwise kernels of the samplers (shrink, residual, chain step, noise, selected copy, the weak-lensing helpers),
// and their C-ABI.  Every array is [C][n] (chain-major); T / data / invcov are [n], shared by all chains.
#include "../../include/pxmcmc_amd.h"
#include "elem.h"
#include "common.h"
#include "sht_core.h"

#include <algorithm>

namespace pxm {

static_assert(NOISE_F64_FLAG == PXM_NOISE_F64, "elem.h: the noise flag must be the public one");

static inline dim3 ew_grid(int64_t n, int C) {
  int64_t bx = (n + 255) / 256;
  if (bx > 2048) bx = 2048;
  if (bx < 1) bx = 1;
  return dim3((unsigned)bx, (unsigned)C);
}

template <bool CPLX>
__global__ void k_soft(const double* __restrict__ X, const double* __restrict__ T, double Ts, double* __restrict__ out,
                       int64_t n) {
  const int64_t base = (int64_t)blockIdx.y * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double t = T ? T[i] : Ts;
    if (CPLX) {
      reinterpret_cast<double2*>(out)[base + i] = soft_cplx(reinterpret_cast<const double2*>(X)[base + i], t);
    } else {
      out[base + i] = soft_real(X[base + i], t);
    }
  }
}

template <bool CPLX, bool ICPLX>
__global__ void k_residual(const double* __restrict__ preds, const double* __restrict__ data,
                           const double* __restrict__ invcov, double* __restrict__ out, int64_t n) {
  const int64_t base = (int64_t)blockIdx.y * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (CPLX) {
      double2 d = csub(reinterpret_cast<const double2*>(preds)[base + i], reinterpret_cast<const double2*>(data)[i]);
      if (ICPLX) d = cmul(reinterpret_cast<const double2*>(invcov)[i], d);
      else {
        const double w = invcov[i];
        d = double2{w * d.x, w * d.y};
      }
      reinterpret_cast<double2*>(out)[base + i] = d;
    } else {
      out[base + i] = invcov[i] * (preds[base + i] - data[i]);
    }
  }
}

// X_out = (1-d/l) X + (d/l) P - d g + sqrt(2d) w, with P = soft(X,T) (FUSED_PROX) or given
template <bool CPLX, bool FUSED_PROX>
__global__ void k_chain_step(const double* __restrict__ X, const double* __restrict__ P, const double* __restrict__ g,
                             const double* __restrict__ T, double Ts, const double* __restrict__ delta_dev,
                             double delta, double lmda, NoiseSrc ns, double* __restrict__ out, int64_t n) {
  const int c = blockIdx.y;
  const int64_t base = (int64_t)c * n;
  const double d = delta_dev ? delta_dev[c] : delta;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double2 w = draw_noise<CPLX>(ns, c, n, i);
    if (CPLX) {
      const double2 x = reinterpret_cast<const double2*>(X)[base + i];
      const double2 px = FUSED_PROX ? soft_cplx(x, T ? T[i] : Ts) : reinterpret_cast<const double2*>(P)[base + i];
      reinterpret_cast<double2*>(out)[base + i] =
          chain_step_cplx(x, px, reinterpret_cast<const double2*>(g)[base + i], w, d, lmda);
    } else {
      const double x = X[base + i];
      const double px = FUSED_PROX ? soft_real(x, T ? T[i] : Ts) : P[base + i];
      out[base + i] = chain_step_real(x, px, g[base + i], w.x, d, lmda);
    }
  }
}

template <bool CPLX>
__global__ void k_randn(double* __restrict__ out, int64_t n, NoiseSrc ns) {
  const int c = blockIdx.y;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double2 w = draw_noise<CPLX>(ns, c, n, i);
    if (CPLX) reinterpret_cast<double2*>(out)[(int64_t)c * n + i] = w;
    else out[(int64_t)c * n + i] = w.x;
  }
}

// the Box-Muller step of the noise stream on given uniforms (test aid: its edge cases cannot be reached through Philox)
__global__ void k_box_muller(const double* __restrict__ u1, const double* __restrict__ u2, double* __restrict__ z0,
                             double* __restrict__ z1, int64_t n, int f64) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const NormalPair q = f64 ? box_muller_f64(u1[i], u2[i]) : box_muller_fast(u1[i], u2[i]);
    z0[i] = q.z0;
    z1[i] = q.z1;
  }
}

struct CopySet {
  const uint64_t* src[4];
  uint64_t* dst[4];
  int64_t nwords[4];
};
__global__ void k_select_copy_many(const int32_t* __restrict__ flag, CopySet cs) {
  const int c = blockIdx.y, a = blockIdx.z;
  if (!flag[c]) return;
  const int64_t nw = cs.nwords[a];
  const uint64_t* s = cs.src[a] + (int64_t)c * nw;
  uint64_t* d = cs.dst[a] + (int64_t)c * nw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nw; i += (int64_t)gridDim.x * blockDim.x) d[i] = s[i];
}

__global__ void k_counter_add(uint64_t* c, uint64_t inc) { *c += inc; }

__global__ void k_wl_mapping(const double2* __restrict__ flm, const double* __restrict__ kernel, double2* __restrict__ out,
                             int64_t n) {
  const int64_t base = (int64_t)blockIdx.y * n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double2 v = flm[base + i];
    const double k = kernel[i];
    v = (i < 4) ? double2{0.0, 0.0} : double2{v.x * k, v.y * k};
    out[base + i] = v;
  }
}

__global__ void k_wl_gather(const double2* __restrict__ f, const int64_t* __restrict__ idx, const double* __restrict__ w,
                            double2* __restrict__ out, int64_t npix, int64_t ndata) {
  const int c = blockIdx.y;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < ndata; k += (int64_t)gridDim.x * blockDim.x) {
    const double2 v = f[(int64_t)c * npix + idx[k]];
    const double ww = w ? w[k] : 1.0;
    out[(int64_t)c * ndata + k] = double2{v.x * ww, v.y * ww};
  }
}

__global__ void k_wl_scatter(const double2* __restrict__ g, const int64_t* __restrict__ idx, const double* __restrict__ w,
                             double2* __restrict__ f, int64_t npix, int64_t ndata) {
  const int c = blockIdx.y;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < ndata; k += (int64_t)gridDim.x * blockDim.x) {
    const double2 v = g[(int64_t)c * ndata + k];
    const double ww = w ? w[k] : 1.0;
    f[(int64_t)c * npix + idx[k]] = double2{v.x * ww, v.y * ww};
  }
}

}  // namespace pxm

using namespace pxm;

#define CHECK_ARGS(name)                                                          \
  PXM_REQUIRE(n >= 0 && C >= 1 && (dtype == 0 || dtype == 1), name ": bad n / C / dtype"); \
  if (n == 0) return 0;                                                           \
  hipStream_t st = (hipStream_t)stream

extern "C" {

int pxm_soft(const void* X, const double* T, double T_scalar, void* out, int64_t n, int C, int dtype,
             pxm_stream_t stream) {
  CHECK_ARGS("pxm_soft");
  PXM_REQUIRE(X && out, "pxm_soft: null buffer");
  dim3 g = ew_grid(n, C), b(256);
  if (dtype) hipLaunchKernelGGL(k_soft<true>, g, b, 0, st, (const double*)X, T, T_scalar, (double*)out, n);
  else hipLaunchKernelGGL(k_soft<false>, g, b, 0, st, (const double*)X, T, T_scalar, (double*)out, n);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_residual_grad(const void* preds, const void* data, const void* invcov, int invcov_complex, void* out,
                      int64_t n, int C, int dtype, pxm_stream_t stream) {
  CHECK_ARGS("pxm_residual_grad");
  PXM_REQUIRE(preds && data && invcov && out, "pxm_residual_grad: null buffer");
  PXM_REQUIRE(dtype == 1 || !invcov_complex, "pxm_residual_grad: complex invcov needs complex data");
  dim3 g = ew_grid(n, C), b(256);
  const double *p = (const double*)preds, *d = (const double*)data, *ic = (const double*)invcov;
  if (dtype && invcov_complex) hipLaunchKernelGGL((k_residual<true, true>), g, b, 0, st, p, d, ic, (double*)out, n);
  else if (dtype) hipLaunchKernelGGL((k_residual<true, false>), g, b, 0, st, p, d, ic, (double*)out, n);
  else hipLaunchKernelGGL((k_residual<false, false>), g, b, 0, st, p, d, ic, (double*)out, n);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_myula_step(const void* X, const void* gradg, const double* T, double T_scalar, const double* delta_dev,
                   double delta, double lmda, const void* noise, int noise_complex, uint64_t seed, uint64_t chain0,
                   uint64_t iter, const uint64_t* iter_dev, void* X_out, int64_t n, int C, int dtype,
                   pxm_stream_t stream) {
  CHECK_ARGS("pxm_myula_step");
  PXM_REQUIRE(X && gradg && X_out, "pxm_myula_step: null buffer");
  if (int rc = check_noise_arg("pxm_myula_step", noise_complex, dtype)) return rc;
  dim3 g = ew_grid(n, C), b(256);
  NoiseSrc ns = make_noise_src(noise, noise_complex, seed, chain0, iter, iter_dev);
  if (dtype)
    hipLaunchKernelGGL((k_chain_step<true, true>), g, b, 0, st, (const double*)X, (const double*)nullptr,
                       (const double*)gradg, T, T_scalar, delta_dev, delta, lmda, ns, (double*)X_out, n);
  else
    hipLaunchKernelGGL((k_chain_step<false, true>), g, b, 0, st, (const double*)X, (const double*)nullptr,
                       (const double*)gradg, T, T_scalar, delta_dev, delta, lmda, ns, (double*)X_out, n);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_chain_step(const void* X, const void* proxf, const void* gradg, const double* delta_dev, double delta,
                   double lmda, const void* noise, int noise_complex, uint64_t seed, uint64_t chain0, uint64_t iter,
                   const uint64_t* iter_dev, void* X_out, int64_t n, int C, int dtype, pxm_stream_t stream) {
  CHECK_ARGS("pxm_chain_step");
  PXM_REQUIRE(X && proxf && gradg && X_out, "pxm_chain_step: null buffer");
  if (int rc = check_noise_arg("pxm_chain_step", noise_complex, dtype)) return rc;
  dim3 g = ew_grid(n, C), b(256);
  NoiseSrc ns = make_noise_src(noise, noise_complex, seed, chain0, iter, iter_dev);
  if (dtype)
    hipLaunchKernelGGL((k_chain_step<true, false>), g, b, 0, st, (const double*)X, (const double*)proxf,
                       (const double*)gradg, (const double*)nullptr, 0.0, delta_dev, delta, lmda, ns, (double*)X_out, n);
  else
    hipLaunchKernelGGL((k_chain_step<false, false>), g, b, 0, st, (const double*)X, (const double*)proxf,
                       (const double*)gradg, (const double*)nullptr, 0.0, delta_dev, delta, lmda, ns, (double*)X_out, n);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_randn(void* out, int64_t n, int C, int dtype, uint64_t seed, uint64_t chain0, uint64_t iter,
              pxm_stream_t stream) {
  const int f64flag = dtype & PXM_NOISE_F64;  // dtype = (0 | 1) | PXM_NOISE_F64
  dtype &= ~PXM_NOISE_F64;
  CHECK_ARGS("pxm_randn");
  PXM_REQUIRE(out, "pxm_randn: null buffer");
  dim3 g = ew_grid(n, C), b(256);
  NoiseSrc ns = make_noise_src(nullptr, dtype | f64flag, seed, chain0, iter);
  if (dtype & 1) hipLaunchKernelGGL(k_randn<true>, g, b, 0, st, (double*)out, n, ns);
  else hipLaunchKernelGGL(k_randn<false>, g, b, 0, st, (double*)out, n, ns);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_box_muller(const double* u1, const double* u2, double* z0, double* z1, int64_t n, int f64, pxm_stream_t stream) {
  PXM_REQUIRE(u1 && u2 && z0 && z1 && n >= 0, "pxm_box_muller: bad arguments");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_box_muller, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream,
                     u1, u2, z0, z1, n, f64);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_select_copy_many(const int32_t* flag, int narrays, const void* const* src, void* const* dst, const int64_t* n,
                         const int* esize, int C, pxm_stream_t stream) {
  PXM_REQUIRE(C >= 1 && flag && narrays >= 1 && narrays <= 4 && src && dst && n && esize, "pxm_select_copy_many: bad arguments");
  CopySet cs;
  int64_t most = 0;
  for (int a = 0; a < 4; ++a) {
    const int k = a < narrays ? a : 0;
    PXM_REQUIRE(src[k] && dst[k] && n[k] >= 0 && esize[k] > 0 && esize[k] % 8 == 0, "pxm_select_copy_many: bad array");
    cs.src[a] = (const uint64_t*)src[k];
    cs.dst[a] = (uint64_t*)dst[k];
    cs.nwords[a] = n[k] * (esize[k] / 8);
    most = std::max(most, cs.nwords[a]);
  }
  if (most == 0) return 0;
  // (workgroups of rejected chains leave at once: the launch then costs its dispatch, so the grid is kept to about one
  // resident round -- 2048 workgroups per chain batch -- and every thread loops)
  dim3 g = ew_grid(most, C);
  g.x = std::min<unsigned>(g.x, std::max(64u, 2048u / (unsigned)(C * narrays)));
  g.z = narrays;
  hipLaunchKernelGGL(k_select_copy_many, g, dim3(256), 0, (hipStream_t)stream, flag, cs);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_counter_add(uint64_t* counter_dev, uint64_t inc, pxm_stream_t stream) {
  PXM_REQUIRE(counter_dev, "pxm_counter_add: null counter");
  hipLaunchKernelGGL(k_counter_add, dim3(1), dim3(1), 0, (hipStream_t)stream, counter_dev, inc);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_wl_harmonic_mapping(const void* flm, const double* kernel, void* out, int64_t n, int C, pxm_stream_t stream) {
  PXM_REQUIRE(C >= 1 && flm && kernel && out && n >= 0, "pxm_wl_harmonic_mapping: bad arguments");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_wl_mapping, ew_grid(n, C), dim3(256), 0, (hipStream_t)stream, (const double2*)flm, kernel,
                     (double2*)out, n);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_wl_mask_gather(const void* f, const int64_t* idx, const double* w, void* out, int64_t npix, int64_t ndata,
                       int C, pxm_stream_t stream) {
  PXM_REQUIRE(C >= 1 && ndata >= 0 && npix >= ndata, "pxm_wl_mask_gather: bad arguments");
  if (ndata == 0) return 0;  // everything masked: nothing to gather
  PXM_REQUIRE(f && idx && out, "pxm_wl_mask_gather: null buffer");
  hipLaunchKernelGGL(k_wl_gather, ew_grid(ndata, C), dim3(256), 0, (hipStream_t)stream, (const double2*)f, idx, w,
                     (double2*)out, npix, ndata);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_wl_mask_scatter(const void* g, const int64_t* idx, const double* w, void* f, int64_t npix, int64_t ndata, int C,
                        pxm_stream_t stream) {
  PXM_REQUIRE(C >= 1 && f && ndata >= 0 && npix >= ndata, "pxm_wl_mask_scatter: bad arguments");
  PXM_HIP(hipMemsetAsync(f, 0, (size_t)C * npix * 16, (hipStream_t)stream));
  if (ndata == 0) return 0;  // everything masked: the image is zero
  PXM_REQUIRE(g && idx, "pxm_wl_mask_scatter: null buffer");
  hipLaunchKernelGGL(k_wl_scatter, ew_grid(ndata, C), dim3(256), 0, (hipStream_t)stream, (const double2*)g, idx, w,
                     (double2*)f, npix, ndata);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
