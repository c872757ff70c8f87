// phi-DFT stage of the MW transforms: length n = 2L-1 (odd) DFTs of every ring of every chain.  This file holds the
// unit selection and launch dispatch of a DftPlan (sht_core.h: DftUnit) and the radix-2 unit: Bluestein's chirp-z
// algorithm on an in-LDS power-of-two FFT (DIF forward, bit-reversed pointwise product with the pre-transformed chirp
// filter, DIT back -- no bit-reversal pass).
// Every unit also transposes between the image layout [c][t][p] and the ring layout [m][t][c] through LDS, and carries
// the fused elementwise prologue/epilogue of the MYULA step (residual on read, prox + Langevin update on write).
#include "dft_unit.h"
#include "elem.h"
#include "update.h"

#include <cstdlib>

namespace pxm {

struct DftArgs {
  int L, n, M, logM, Rp, R;
  const double2* chirp;
  const double2* bhat;
  const double2* tw;
};

// In-LDS Bluestein core on R rows of M complex values; rows hold a_j = x_j * chirp_j (zero padded).
// On return row r holds the circular convolution with the chirp filter; y_k = chirp_k * row[k].
__device__ inline void bluestein_core(double2* buf, const double2* tw, const DftArgs& a) {
  const int M = a.M, half = M >> 1, R = a.R;
  const int total = R * half;
  // forward DIF: natural in, bit-reversed out
  for (int s = half, st = 1; s >= 1; s >>= 1, st <<= 1) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      const int r = idx / half, b = idx - r * half;
      const int g = b / s, p = b - g * s;
      double2* x = buf + r * M + g * 2 * s + p;
      const double2 u = x[0], v = x[s];
      x[0] = cadd(u, v);
      x[s] = cmul(csub(u, v), tw[p * st]);
    }
  }
  __syncthreads();
  // pointwise product with FFT(filter)/M (stored bit-reversed)
  for (int idx = threadIdx.x; idx < R * M; idx += blockDim.x) {
    const int j = idx & (M - 1);
    buf[idx] = cmul(buf[idx], a.bhat[j]);
  }
  // inverse DIT: bit-reversed in, natural out
  for (int s = 1, st = half; s <= half; s <<= 1, st >>= 1) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
      const int r = idx / half, b = idx - r * half;
      const int g = b / s, p = b - g * s;
      double2* x = buf + r * M + g * 2 * s + p;
      const double2 u = x[0], v = cmulc(x[s], tw[p * st]);
      x[0] = cadd(u, v);
      x[s] = csub(u, v);
    }
  }
  __syncthreads();
}

// image -> rings: G[m][t][c] = sum_p f(c,t,p) e^{-i m phi_p}
__global__ void k_px2ring(DftArgs a, PxIn in, double* __restrict__ G, int ncol, int C) {
  extern __shared__ double2 lds[];
  double2* tw = lds;
  double2* buf = lds + (a.M >> 1);
  const int t = blockIdx.x, c0 = blockIdx.y * a.R;
  const int n = a.n, M = a.M, R = a.R;
  if (in.bump && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *in.bump += 1;
  for (int k = threadIdx.x; k < (M >> 1); k += blockDim.x) tw[k] = a.tw[k];
  for (int idx = threadIdx.x; idx < R * M; idx += blockDim.x) {
    const int r = idx / M, j = idx - r * M;
    const int c = c0 + r;
    double2 v{0.0, 0.0};
    if (j < n && c < C) {
      const int64_t e = in.ring0 + (int64_t)t * n + j;
      v = px_in_load(in, c, e);
      v = cmul(v, a.chirp[j]);
    }
    buf[idx] = v;
  }
  bluestein_core(buf, tw, a);
  const int Cp = ncol >> 1;
  for (int idx = threadIdx.x; idx < n * R; idx += blockDim.x) {
    const int k = idx / R, r = idx - k * R;
    const int c = c0 + r;
    if (c >= Cp) continue;
    const double2 y = cmul(buf[r * M + k], a.chirp[k]);
    const int m = (k < a.L) ? k : k - n;
    reinterpret_cast<double2*>(G)[((int64_t)(m + a.L - 1) * a.Rp + t) * Cp + c] = y;
  }
}

// rings -> image: f(c,t,p) = sum_m G[m][t][c] e^{+i m phi_p}   (conjugate trick on the same core)
__global__ void k_ring2px(DftArgs a, const double* __restrict__ G, int ncol, PxOut out, int C) {
  extern __shared__ double2 lds[];
  double2* tw = lds;
  double2* buf = lds + (a.M >> 1);
  const int t = blockIdx.x, c0 = blockIdx.y * a.R;
  const int n = a.n, M = a.M, R = a.R;
  const int Cp = ncol >> 1;
  for (int k = threadIdx.x; k < (M >> 1); k += blockDim.x) tw[k] = a.tw[k];
  for (int idx = threadIdx.x; idx < (M - n) * R; idx += blockDim.x) {
    const int r = idx / (M - n), j = n + idx - r * (M - n);
    buf[r * M + j] = double2{0.0, 0.0};
  }
  for (int idx = threadIdx.x; idx < n * R; idx += blockDim.x) {
    const int k = idx / R, r = idx - k * R;
    const int c = c0 + r;
    double2 v{0.0, 0.0};
    if (c < Cp) {
      const int m = (k < a.L) ? k : k - n;
      v = reinterpret_cast<const double2*>(G)[((int64_t)(m + a.L - 1) * a.Rp + t) * Cp + c];
      v.y = -v.y;
      v = cmul(v, a.chirp[k]);
    }
    buf[r * M + k] = v;
  }
  bluestein_core(buf, tw, a);
  for (int idx = threadIdx.x; idx < R * n; idx += blockDim.x) {
    const int r = idx / n, p = idx - r * n;
    const int c = c0 + r;
    if (c >= C) continue;
    double2 y = cmul(buf[r * M + p], a.chirp[p]);
    y.y = -y.y;
    const int64_t e = out.ring0 + (int64_t)t * n + p;
    const int64_t ce = (int64_t)c * out.chain_stride + e;
    if (out.X) {  // fused prox + MYULA update (pxmcmc/mcmc.py:185-201, prior.py:49-50)
      const uint64_t it_eff = out.iter + (out.iter_dev ? *out.iter_dev : 0);
      const double2 x = reinterpret_cast<const double2*>(out.X)[ce];
      const double T = out.T ? out.T[e] : out.T_scalar;
      const double2 w = out.noise ? px_noise_load(out, c, e) : px_noise_philox(out, c, e, it_eff);
      reinterpret_cast<double2*>(out.f)[ce] = px_update(out, x, T, y, w);
    } else {
      px_out_store(out, c, e, y);
    }
  }
}

int dft_geometry(int L, DftGeometry* g) {
  PXM_REQUIRE(L >= 1 && L <= (1 << 28), "dft_geometry: need 1 <= L <= 2^28");
  const int n = 2 * L - 1;
  // PXM_DFT_NO_W=1: the radix-2 unit for every size; PXM_DFT_PFA=0: the pair unit's Bluestein body for n = 511 as well
  const bool radix2_only = getenv("PXM_DFT_NO_W") != nullptr;
  const char* pfa_env = getenv("PXM_DFT_PFA");
  *g = DftGeometry();
  g->pfa = !(pfa_env && atoi(pfa_env) == 0);
  if (!radix2_only && pair_r0(n)) {
    g->unit = DFT_PAIR;
    g->M = 128 * pair_r0(n);
    pair_workgroup(n, g->pfa, &g->per_wg, &g->threads, &g->lds, &g->exact);
  } else if (!radix2_only && n <= 1023) {
    g->unit = DFT_QUAD;
    g->M = 2048;
    quad_workgroup(&g->per_wg, &g->threads, &g->lds);
  } else {
    g->unit = DFT_RADIX2;
    g->M = bluestein_size(n);
    // chains per workgroup: as many as fit in ~128 KB of LDS, at most 8 (128-B ring-layout segments)
    int R = 8;
    while (R > 1 && (size_t)R * g->M * 16 > 128 * 1024) R >>= 1;
    g->per_wg = R;
    g->lds = ((size_t)R * g->M + g->M / 2) * 16;
    const int64_t th = (int64_t)R * g->M / 2;
    g->threads = th < 64 ? 64 : (th > 1024 ? 1024 : (int)th);
  }
  // (one chain of M = 8192 points and its twiddles: no smaller R to fall back to)
  PXM_REQUIRE(g->lds <= DFT_LDS_MAX, "phi-DFT stage: no unit for bandlimit L = " + std::to_string(L) + ": the radix-2 unit at M = " +
                                         std::to_string(g->M) + " needs " + std::to_string(g->lds) + " B of LDS per workgroup, a CU has " +
                                         std::to_string(DFT_LDS_MAX) + " (the largest bandlimit is L = 1024)");
  return 0;
}

int make_dft_plan(int L, DftPlan* p) {
  DftGeometry g;
  if (int rc = dft_geometry(L, &g)) return rc;
  p->L = L;
  p->n = 2 * L - 1;
  p->Rp = round_up(L, 16);
  p->unit = g.unit;
  if (const char* e = getenv("PXM_DFT_STOCK")) p->stock = atoi(e) != 0;
  if (g.unit == DFT_PAIR) {
    if (const char* e = getenv("PXM_DEBUG_PAIR_SYNC_LIMIT")) p->spin_limit = (unsigned)std::max(0, atoi(e));
    return pair_make_tables(p->n, g.pfa, &p->pair);
  }
  if (g.unit == DFT_QUAD) return quad_make_tables(p->n, &p->quad);
  BluesteinTables b = make_bluestein(p->n, g.M);
  PXM_REQUIRE(b.M == g.M, "make_dft_plan: the Bluestein tables disagree with dft_geometry");
  p->M = b.M;
  p->logM = b.logM;
  p->R = g.per_wg;
  p->lds = g.lds;
  p->threads = g.threads;
  int rc;
  if ((rc = dev_table(&p->d_chirp, b.chirp, "Bluestein chirp"))) return rc;
  if ((rc = dev_table(&p->d_bhat, b.bhat, "Bluestein filter spectrum"))) return rc;
  if ((rc = dev_table(&p->d_tw, b.tw, "radix-2 twiddles"))) return rc;
  static std::atomic<uint64_t> lds_done{0};
  return allow_dynamic_lds(lds_done, {reinterpret_cast<const void*>(k_px2ring), reinterpret_cast<const void*>(k_ring2px)});
}

void free_dft_plan(DftPlan* p) {
  for (double** d : {&p->d_chirp, &p->d_bhat, &p->d_tw, &p->pair.d_all, &p->quad.d_all}) {
    if (*d) deferred_free(*d);
    *d = nullptr;
  }
}

static DftArgs make_args(const DftPlan& p) {
  DftArgs a;
  a.L = p.L;
  a.n = p.n;
  a.M = p.M;
  a.logM = p.logM;
  a.Rp = p.Rp;
  a.R = p.R;
  a.chirp = reinterpret_cast<const double2*>(p.d_chirp);
  a.bhat = reinterpret_cast<const double2*>(p.d_bhat);
  a.tw = reinterpret_cast<const double2*>(p.d_tw);
  return a;
}

int launch_px2ring(const DftPlan& p, const PxIn& in, double* G, int ncol, int C, hipStream_t stream) {
  switch (p.unit) {
    case DFT_PAIR: return pair_px2ring(p, in, G, ncol, C, stream);
    case DFT_QUAD: return quad_px2ring(p, in, G, ncol, C, stream);
    case DFT_RADIX2: break;
  }
  const int Cp = ncol / 2;
  dim3 grid(p.L, (Cp + p.R - 1) / p.R), block(p.threads);
  hipLaunchKernelGGL(k_px2ring, grid, block, p.lds, stream, make_args(p), in, G, ncol, C);
  PXM_HIP(hipGetLastError());
  return 0;
}

int launch_ring2px2ring(const DftPlan& p, double* G, int ncol, const PxOut& out, int C, hipStream_t stream) {
  PXM_REQUIRE(dft_can_fuse(p), "launch_ring2px2ring: the plan's DFT unit has no fused rings -> pixels -> rings kernel");
  return pair_ring2px(p, G, ncol, out, C, stream, true);
}

int launch_ring2px(const DftPlan& p, const double* G, int ncol, const PxOut& out, int C, hipStream_t stream) {
  switch (p.unit) {
    case DFT_PAIR: return pair_ring2px(p, G, ncol, out, C, stream, false);
    case DFT_QUAD: return quad_ring2px(p, G, ncol, out, C, stream);
    case DFT_RADIX2: break;
  }
  dim3 grid(p.L, (C + p.R - 1) / p.R), block(p.threads);
  hipLaunchKernelGGL(k_ring2px, grid, block, p.lds, stream, make_args(p), G, ncol, out, C);
  PXM_HIP(hipGetLastError());
  return 0;
}

// ---- public harmonic layout <-> internal [m][el][c] -----------------------------------------
__global__ void k_lm_to_mel(const double2* __restrict__ flm, double2* __restrict__ H, int L, int Rp, int Cp, int C,
                            int spin) {
  const int64_t total = (int64_t)(2 * L - 1) * Rp * Cp;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cp);
    const int el = (int)((i / Cp) % Rp);
    const int m = (int)(i / ((int64_t)Cp * Rp)) - (L - 1);
    double2 v{0.0, 0.0};
    const int am = m < 0 ? -m : m, as = spin < 0 ? -spin : spin;
    if (c < C && el < L && el >= am && el >= as) v = flm[(int64_t)c * L * L + (int64_t)el * el + el + m];
    H[i] = v;
  }
}

__global__ void k_mel_to_lm(const double2* __restrict__ H, double2* __restrict__ flm, int L, int Rp, int Cp, int C,
                            int spin) {
  const int64_t total = (int64_t)C * L * L;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i / ((int64_t)L * L));
    const int lm = (int)(i - (int64_t)c * L * L);
    int el = (int)sqrt((double)lm);
    while ((el + 1) * (el + 1) <= lm) ++el;
    while (el * el > lm) --el;
    const int m = lm - el * el - el;
    const int as = spin < 0 ? -spin : spin;
    double2 v{0.0, 0.0};
    if (el >= as) v = H[((int64_t)(m + L - 1) * Rp + el) * Cp + c];
    flm[i] = v;
  }
}

int launch_lm_to_mel(const double* flm, double* H, int L, int Rp, int ncol, int C, int spin, hipStream_t stream) {
  const int Cp = ncol / 2;
  const int64_t total = (int64_t)(2 * L - 1) * Rp * Cp;
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_lm_to_mel, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const double2*>(flm),
                     reinterpret_cast<double2*>(H), L, Rp, Cp, C, spin);
  PXM_HIP(hipGetLastError());
  return 0;
}

int launch_mel_to_lm(const double* H, double* flm, int L, int Rp, int ncol, int C, int spin, hipStream_t stream) {
  const int Cp = ncol / 2;
  const int64_t total = (int64_t)C * L * L;
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_mel_to_lm, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const double2*>(H),
                     reinterpret_cast<double2*>(flm), L, Rp, Cp, C, spin);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // namespace pxm
