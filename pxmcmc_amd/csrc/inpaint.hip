// Segment inpainting for the hypothesis test of image structure.  Per slot c (one region of an
// integer label image) one iteration of the surrogate is
//
//   x_next[c][k] = labels[k] == region[c] ? y[c][k] : x_map[k],      y = Psi soft_tau(A x_prev) formed by the caller,
//
// and the slot freezes once |x_next - x_prev|^2 <= tol^2 |x_next|^2; a frozen slot is copied through.  One entry point,
// pxm_inpaint_step: a streaming kernel (the select, and per slice the partial sums of the two squared norms of the slots
// that are not frozen), then a one-wave finishing kernel per slot (the sums, the counter and the flag).  No indicator array
// exists: the label of a pixel is compared with the slot's region.  No trip count depends on the data and nothing waits.
// The sums are fixed-order sums of reduce.h with a slice count that depends on npix only.
//
// The unit of work is 16 bytes of a slot's row: one complex element, or the pair (2p, 2p + 1) of real ones.  Thread t of
// slice s takes the units s * 256 + t, + slices * 256, ... and adds their terms in that order (a pair: 2p, then 2p + 1).
// A real row whose pairs are not 16-byte aligned (odd npix, an offset view) is read with 8-byte accesses instead: the same
// units, terms and order, so the numbers do not depend on the alignment.
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "reduce.h"

#include <cmath>

namespace pxm {

constexpr int INP_SLICES_MAX = 512;

// workgroups (slices) per slot: one per 1024 pixels up to INP_SLICES_MAX, grid-stride beyond
static inline int inpaint_slices(int64_t npix) {
  const int64_t s = (npix + 1023) / 1024;
  return (int)(s < 1 ? 1 : (s > INP_SLICES_MAX ? INP_SLICES_MAX : s));
}

// a pixel of the slot's region takes y, every other pixel (label -1 included, whatever region[c] holds) the MAP image
__device__ __forceinline__ bool inp_inside(int label, int reg) { return label == reg && label >= 0; }

__device__ __forceinline__ void inp_term(double v, double p, double& d2, double& n2) {
  const double d = v - p;
  d2 = fma(d, d, d2);
  n2 = fma(v, v, n2);
}

// part[c][slice] = (d2, n2) of the slice; nothing is written for a frozen slot.  done[c] and region[c] are the same for
// every lane (blockIdx.y selects them): one uniform read each per workgroup.
template <bool CPLX, bool VEC>
__global__ __launch_bounds__(256) void k_inpaint_step(const double* __restrict__ Y, const double* __restrict__ XP,
                                                      const double* __restrict__ XM, const int* __restrict__ labels,
                                                      const int* __restrict__ region, const int* __restrict__ done,
                                                      double* __restrict__ XN, double* __restrict__ part, int64_t n) {
  const int c = blockIdx.y;
  const bool frozen = done[c] != 0;
  const int reg = region[c];
  const int64_t first = blockIdx.x * (int64_t)256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  double d2 = 0.0, n2 = 0.0;
  if constexpr (CPLX) {
    const double2* __restrict__ y = reinterpret_cast<const double2*>(Y) + (int64_t)c * n;
    const double2* __restrict__ xp = reinterpret_cast<const double2*>(XP) + (int64_t)c * n;
    const double2* __restrict__ xm = reinterpret_cast<const double2*>(XM);
    double2* __restrict__ xn = reinterpret_cast<double2*>(XN) + (int64_t)c * n;
    if (frozen) {
      for (int64_t i = first; i < n; i += stride) xn[i] = xp[i];
      return;
    }
    for (int64_t i = first; i < n; i += stride) {
      const double2 p = xp[i];
      const double2 v = inp_inside(labels[i], reg) ? y[i] : xm[i];
      const double dx = v.x - p.x, dy = v.y - p.y;
      d2 += fma(dx, dx, dy * dy);
      n2 += fma(v.x, v.x, v.y * v.y);
      xn[i] = v;
    }
  } else {
    const double* __restrict__ y = Y + (int64_t)c * n;
    const double* __restrict__ xp = XP + (int64_t)c * n;
    double* __restrict__ xn = XN + (int64_t)c * n;
    const int64_t pairs = (n + 1) / 2;
    if constexpr (VEC) {  // n is even and every row starts on 16 bytes (the labels on 8)
      const double2* __restrict__ y2 = reinterpret_cast<const double2*>(y);
      const double2* __restrict__ xp2 = reinterpret_cast<const double2*>(xp);
      const double2* __restrict__ xm2 = reinterpret_cast<const double2*>(XM);
      const int2* __restrict__ l2 = reinterpret_cast<const int2*>(labels);
      double2* __restrict__ xn2 = reinterpret_cast<double2*>(xn);
      if (frozen) {
        for (int64_t q = first; q < pairs; q += stride) xn2[q] = xp2[q];
        return;
      }
      for (int64_t q = first; q < pairs; q += stride) {
        const double2 p = xp2[q];
        const int2 l = l2[q];
        const bool in0 = inp_inside(l.x, reg), in1 = inp_inside(l.y, reg);
        double2 v;
        if (in0 == in1) {  // (the usual case: one 16-byte load)
          v = in0 ? y2[q] : xm2[q];
        } else {
          v.x = in0 ? y[2 * q] : XM[2 * q];
          v.y = in1 ? y[2 * q + 1] : XM[2 * q + 1];
        }
        inp_term(v.x, p.x, d2, n2);
        inp_term(v.y, p.y, d2, n2);
        xn2[q] = v;
      }
    } else {
      if (frozen) {
        for (int64_t q = first; q < pairs; q += stride) {
          xn[2 * q] = xp[2 * q];
          if (2 * q + 1 < n) xn[2 * q + 1] = xp[2 * q + 1];
        }
        return;
      }
      for (int64_t q = first; q < pairs; q += stride) {
        for (int64_t i = 2 * q; i < 2 * q + 2 && i < n; ++i) {
          const double v = inp_inside(labels[i], reg) ? y[i] : XM[i];
          inp_term(v, xp[i], d2, n2);
          xn[i] = v;
        }
      }
    }
  }
  block_sum<4>(d2, n2);
  if (threadIdx.x == 0) {
    double* o = part + ((int64_t)c * gridDim.x + blockIdx.x) * 2;
    o[0] = d2, o[1] = n2;
  }
}

// One wave per slot.  Not frozen: the slot's partials added in the fixed order (reduce.h: slice_sum), one more iteration
// counted, stat[c] = (d2, n2), and the flag from one multiply and one compare (a NaN compares false: it never freezes a
// slot).  Frozen: nothing of the slot changes.
__global__ __launch_bounds__(64) void k_inpaint_finish(const double* __restrict__ part, int slices, double tol2,
                                                       int* __restrict__ done, int* __restrict__ iters,
                                                       double* __restrict__ stat) {
  const int c = blockIdx.x;
  if (done[c] != 0) return;
  double d2, n2;
  slice_sum<2>(part + (int64_t)c * slices * 2, slices, threadIdx.x, d2, n2);
  if (threadIdx.x == 0) {
    const double rhs = tol2 * n2;
    iters[c] += 1;
    stat[2 * c] = d2, stat[2 * c + 1] = n2;
    done[c] = d2 <= rhs ? 1 : 0;
  }
}

static inline bool inp_overlap(const void* a, const void* b, size_t bytes) {
  const char *x = (const char*)a, *y = (const char*)b;
  return x < y + bytes && y < x + bytes;
}

}  // namespace pxm

using namespace pxm;

extern "C" {

int64_t pxm_inpaint_scratch_doubles(int64_t npix, int C) {
  if (npix < 1 || C < 1) return -1;
  return (int64_t)C * inpaint_slices(npix) * 2;
}

int pxm_inpaint_step(const void* y, const void* x_prev, const void* x_map, const int* labels, const int* region, double tol2,
                     void* x_next, int* done, int* iters, double* stat, double* scratch, int64_t npix, int C, int dtype,
                     pxm_stream_t stream) {
  PXM_REQUIRE(npix >= 1 && C >= 1 && C <= 65535 && (dtype == 0 || dtype == 1), "pxm_inpaint_step: bad npix / C / dtype");
  PXM_REQUIRE(tol2 >= 0.0 && std::isfinite(tol2), "pxm_inpaint_step: tol2 must be finite and >= 0");
  PXM_REQUIRE(y && x_prev && x_map && labels && region && x_next && done && iters && stat && scratch,
              "pxm_inpaint_step: null buffer");
  const size_t elem = dtype ? 16 : 8, bytes = (size_t)C * (size_t)npix * elem;
  PXM_REQUIRE(!inp_overlap(x_next, x_prev, bytes) && !inp_overlap(x_next, y, bytes),
              "pxm_inpaint_step: x_next must not overlap x_prev or y");
  const auto at = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
  PXM_REQUIRE(at(y, elem) && at(x_prev, elem) && at(x_map, elem) && at(x_next, elem) && at(labels, 4),
              "pxm_inpaint_step: a buffer is not aligned to its element");
  hipStream_t st = (hipStream_t)stream;
  const int slices = inpaint_slices(npix);
  const dim3 g((unsigned)slices, (unsigned)C);
  const double *Y = (const double*)y, *XP = (const double*)x_prev, *XM = (const double*)x_map;
  double* XN = (double*)x_next;
  const bool vec = npix % 2 == 0 && at(y, 16) && at(x_prev, 16) && at(x_map, 16) && at(x_next, 16) && at(labels, 8);
#define PXM_INP(CPLX, VEC) \
  hipLaunchKernelGGL((k_inpaint_step<CPLX, VEC>), g, dim3(256), 0, st, Y, XP, XM, labels, region, (const int*)done, XN, scratch, npix)
  if (dtype) PXM_INP(true, true);
  else if (vec) PXM_INP(false, true);
  else PXM_INP(false, false);
#undef PXM_INP
  hipLaunchKernelGGL(k_inpaint_finish, dim3(C), dim3(64), 0, st, (const double*)scratch, slices, tol2, done, iters, stat);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
