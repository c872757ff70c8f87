// Directional (N = dirs >= 1) scale-discretised wavelet transforms, spin 0, upsample = 0 (Leistedt et al. 2013;
// McEwen et al. 2015, "Directional spin wavelets on the sphere"): what pys2let.analysis_px2wav / synthesis_wav2px and
// their adjoints compute with N > 1 (pxmcmc/transforms.py:95-98).  Conventions: DESIGN.md section 11.
//
// Per scale j and orientation index n in {-(N-1), -(N-3), .., N-1} the SO(3) transform factors into spin transforms:
//
//   analysis    a^{j,n}_lm = (-1)^n kappa_j(l) conj(s_ln) f_lm / sqrt(2 pi)      harmonic split   (k_dw_split)
//               g_n        = inverse SHT, spin -n, at bl_j                         (pxm_sht_inverse of an inner plan)
//               W^j(gamma_c) = sum_n e^{+i n gamma_c} g_n                         gamma stage      (k_dw_gamma_fwd)
//   synthesis   g_n  = (1/(2N-1)) sum_c e^{-i n gamma_c} W^j(gamma_c)              gamma stage      (k_dw_gamma_back)
//               b    = forward SHT, spin -n, at bl_j
//               f_lm = kappa_0 (scaling) + sum_{j,n} (-1)^n kappa_j(l) s_ln sqrt(2 pi) b_lm   harmonic merge (k_dw_merge)
//
// and the two adjoints run the conjugate-transposed stages in reverse order.  The scaling function rides along as one
// more (block, n = 0) item with weight kappa_0 and a single plane.  Pairs (j, n) with |n| >= bl_j are skipped: s_ln
// vanishes for every l < bl_j there.
//
// Both new kernels are complex128 streams: one 16-byte element per lane, phases and weights from host tables (no device
// trig), one launch per direction for every item and chain (grid.y = chain, grid.x = the items' blocks back to back).
#include "update.h"  // (first: its mode enum precedes the public header's PXM_MODE_* macros of the same values)
#include "../../include/pxmcmc_amd.h"
#include "common.h"
#include "elem.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <vector>

namespace pxm {

constexpr int DW_THREADS = 256;
constexpr int DW_REG_N = 8;  // orientation counts up to this keep the N inputs / outputs of a pixel in registers

struct DwItem {      // one (block, n) operand of the harmonic stages
  int64_t a_off;     // offset of chain 0's bl*bl entries: in the harmonic arena, or in a harmonic coefficient vector
  int64_t cstride;   // chain stride of the operand: bl*bl (arena, [C][bl*bl] per item) or ncoefs ([C][ncoefs] vector)
  int64_t w_off;     // row of the weight tables, L entries
  int bl;
  int blk0;          // first thread block of this item in the split launch
};

struct DwBlock {   // one coefficient block (scaling, or scale j with its planes) of the gamma stage
  int64_t coef_off;  // offset of the block in a chain's coefficient vector
  int64_t goff;      // row of the g-offset table: nn entries, offset of g_n in the pixel arena or -1 (skipped pair)
  int npix, nplanes, nn;
  int blk0;
};

// block -> item of a flattened launch: the last entry with blk0 <= b (uniform per workgroup, scalar loads)
template <class T>
__device__ __forceinline__ int dw_find(const T* __restrict__ d, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].blk0 <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int dw_el(int lm) {
  int el = (int)sqrt((double)lm);
  if ((el + 1) * (el + 1) <= lm) ++el;
  if (el * el > lm) --el;
  return el;
}

__device__ __forceinline__ double2 dw_w(double2 w, bool cj) { return cj ? double2{w.x, -w.y} : w; }

// out_d[c][lm] = w_d(l) f[c][lm]  (w or conj(w)), for every item d and lm < bl_d^2 (out_d[c] at a_off + c cstride)
__global__ __launch_bounds__(DW_THREADS) void k_dw_split(const double2* __restrict__ flm, double2* __restrict__ harm,
                                                         const DwItem* __restrict__ items, int nitems,
                                                         const double2* __restrict__ W, int cj, int L) {
  const int d = dw_find(items, nitems, blockIdx.x);
  const DwItem it = items[d];
  const int lm = (blockIdx.x - it.blk0) * DW_THREADS + threadIdx.x;
  const int nlm = it.bl * it.bl;
  if (lm >= nlm) return;
  const int c = blockIdx.y;
  const double2 w = dw_w(W[it.w_off + dw_el(lm)], cj);
  harm[it.a_off + (int64_t)c * it.cstride + lm] = cmul(w, flm[(int64_t)c * L * L + lm]);
}

// f[c][lm] = sum_d [l < bl_d] w_d(l) b_d[c][lm]
__global__ __launch_bounds__(DW_THREADS) void k_dw_merge(const double2* __restrict__ harm, double2* __restrict__ flm,
                                                         const DwItem* __restrict__ items, int nitems,
                                                         const double2* __restrict__ W, int cj, int L) {
  const int lm = blockIdx.x * DW_THREADS + threadIdx.x;
  if (lm >= L * L) return;
  const int c = blockIdx.y;
  const int el = dw_el(lm);
  double2 acc{0.0, 0.0};
  for (int d = 0; d < nitems; ++d) {
    const DwItem it = items[d];
    if (el >= it.bl) continue;
    const double2 w = dw_w(W[it.w_off + el], cj);
    const double2 b = harm[it.a_off + (int64_t)c * it.cstride + lm];
    acc = cadd(acc, cmul(w, b));
  }
  flm[(int64_t)c * L * L + lm] = acc;
}

// n -> planes: X[c][coef_off + q npix + p] = sc sum_k ph[q][k] g_k[c][p]   (ph[q][k] = e^{i n_k gamma_q})
template <int NK>
__global__ __launch_bounds__(DW_THREADS) void k_dw_gamma_fwd(const double2* __restrict__ pix, double2* __restrict__ X,
                                                             const DwBlock* __restrict__ blocks, int nblocks,
                                                             const int64_t* __restrict__ goff, const double2* __restrict__ ph,
                                                             int N, int64_t ncoefs, int norm) {
  const int bi = dw_find(blocks, nblocks, blockIdx.x);
  const DwBlock bk = blocks[bi];
  const int p = (blockIdx.x - bk.blk0) * DW_THREADS + threadIdx.x;
  if (p >= bk.npix) return;
  const int c = blockIdx.y;
  const int64_t gp = (int64_t)c * bk.npix + p;
  double2* out = X + (int64_t)c * ncoefs + bk.coef_off + p;
  const double sc = (norm && bk.nplanes > 1) ? 1.0 / bk.nplanes : 1.0;
  if (bk.nplanes == 1) {  // scaling function, or N = 1: a copy
    const int64_t o = goff[bk.goff];
    const double2 g = o >= 0 ? pix[o + gp] : double2{0.0, 0.0};
    out[0] = double2{sc * g.x, sc * g.y};
    return;
  }
  if (NK > 0) {
    double2 g[NK > 0 ? NK : 1];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int64_t o = goff[bk.goff + k];
      g[k] = o >= 0 ? pix[o + gp] : double2{0.0, 0.0};
    }
#pragma unroll 1  // (q rolled: NK phases live in SGPRs at a time, not all (2NK - 1) NK of them)
    for (int q = 0; q < 2 * NK - 1; ++q) {
      double2 acc{0.0, 0.0};
#pragma unroll
      for (int k = 0; k < NK; ++k) acc = cadd(acc, cmul(ph[q * NK + k], g[k]));
      out[(int64_t)q * bk.npix] = double2{sc * acc.x, sc * acc.y};
    }
  } else {
    for (int q = 0; q < 2 * N - 1; ++q) {
      double2 acc{0.0, 0.0};
      for (int k = 0; k < N; ++k) {
        const int64_t o = goff[bk.goff + k];
        if (o >= 0) acc = cadd(acc, cmul(ph[q * N + k], pix[o + gp]));
      }
      out[(int64_t)q * bk.npix] = double2{sc * acc.x, sc * acc.y};
    }
  }
}

// planes -> n: g_k[c][p] = sc sum_q conj(ph[q][k]) X[c][coef_off + q npix + p], for the pairs that are not skipped
template <int NK>
__global__ __launch_bounds__(DW_THREADS) void k_dw_gamma_back(const double2* __restrict__ X, double2* __restrict__ pix,
                                                              const DwBlock* __restrict__ blocks, int nblocks,
                                                              const int64_t* __restrict__ goff, const double2* __restrict__ ph,
                                                              int N, int64_t ncoefs, int norm) {
  const int bi = dw_find(blocks, nblocks, blockIdx.x);
  const DwBlock bk = blocks[bi];
  const int p = (blockIdx.x - bk.blk0) * DW_THREADS + threadIdx.x;
  if (p >= bk.npix) return;
  const int c = blockIdx.y;
  const int64_t gp = (int64_t)c * bk.npix + p;
  const double2* in = X + (int64_t)c * ncoefs + bk.coef_off + p;
  const double sc = (norm && bk.nplanes > 1) ? 1.0 / bk.nplanes : 1.0;
  if (bk.nplanes == 1) {
    const int64_t o = goff[bk.goff];
    const double2 x = in[0];
    if (o >= 0) pix[o + gp] = double2{sc * x.x, sc * x.y};
    return;
  }
  if (NK > 0) {
    double2 acc[NK > 0 ? NK : 1];
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] = double2{0.0, 0.0};
#pragma unroll 1
    for (int q = 0; q < 2 * NK - 1; ++q) {
      const double2 x = in[(int64_t)q * bk.npix];
#pragma unroll
      for (int k = 0; k < NK; ++k) acc[k] = cadd(acc[k], cmulc(x, ph[q * NK + k]));
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int64_t o = goff[bk.goff + k];
      if (o >= 0) pix[o + gp] = double2{sc * acc[k].x, sc * acc[k].y};
    }
  } else {
    for (int k = 0; k < N; ++k) {
      const int64_t o = goff[bk.goff + k];
      if (o < 0) continue;
      double2 acc{0.0, 0.0};
      for (int q = 0; q < 2 * N - 1; ++q) acc = cadd(acc, cmulc(in[(int64_t)q * bk.npix], ph[q * N + k]));
      pix[o + gp] = double2{sc * acc.x, sc * acc.y};
    }
  }
}

template <int NK>
static void dw_gamma_launch(bool fwd, dim3 g, hipStream_t st, const double2* in, double2* out, const DwBlock* blocks, int nb,
                            const int64_t* goff, const double2* ph, int N, int64_t ncoefs, int norm) {
  if (fwd) hipLaunchKernelGGL(k_dw_gamma_fwd<NK>, g, dim3(DW_THREADS), 0, st, in, out, blocks, nb, goff, ph, N, ncoefs, norm);
  else hipLaunchKernelGGL(k_dw_gamma_back<NK>, g, dim3(DW_THREADS), 0, st, in, out, blocks, nb, goff, ph, N, ncoefs, norm);
}

// directionality component s_lm [L*L]: nu sqrt(2^-g C(g, (g - m)/2)), m = -g, -g + 2, .., g,
// g = gamma_l = the largest integer <= min(N - 1, l) with the parity of N - 1; nu = 1 (N odd), i (N even)
static std::vector<double2> dir_component(int L, int N) {
  std::vector<double2> s((size_t)L * L, double2{0.0, 0.0});
  for (int el = 0; el < L; ++el) {
    int g = std::min(N - 1, el);
    if ((N - 1 - g) % 2) --g;
    if (g < 0) continue;
    for (int m = -g; m <= g; m += 2) {
      // C(g, k) 2^-g through lgamma: exact enough for g < 1000 (the values are O(1) and below)
      const int k = (g - m) / 2;
      const double v = std::sqrt(std::exp(std::lgamma(g + 1.0) - std::lgamma(k + 1.0) - std::lgamma(g - k + 1.0) - g * std::log(2.0)));
      s[(size_t)el * el + el + m] = (N % 2) ? double2{v, 0.0} : double2{0.0, v};
    }
  }
  return s;
}

// The weights of the harmonic stages, item by item: one row of L entries per (block b, orientation n) for the split (wa)
// and one for the merge (ws).  Block 0 is the scaling function (n = 0): kappa_0(l) in both rows.  Block b > 0 is scale
// J_min + b - 1 with k = kappa_j(l) s_ln:
//   pixel space (DirWavPlan)      wa = (-1)^n conj(k) / sqrt(2 pi)      ws = (-1)^n k sqrt(2 pi)
//   harmonic space (HarmWavPlan)  wa = sqrt(8 pi^2/(2l+1)) conj(k)     ws = sqrt((2l+1)/(8 pi^2)) k
// Spin s (N = 1): every row is zero for l < |s|.
struct DwTiling {
  int L, J_min, spin;
  std::vector<double> k0, kap;
  std::vector<double2> s;
  DwTiling(int L_, double B, int J_min_, int N, int spin_) : L(L_), J_min(J_min_), spin(spin_), s(dir_component(L_, N)) {
    tiling_axisym(L, B, J_min, k0, kap);
  }
  void rows(int b, int n, bool harmonic, std::vector<double2>& wa, std::vector<double2>& ws) const {
    const double ca = 1.0 / std::sqrt(2.0 * M_PI), cs = std::sqrt(2.0 * M_PI);
    const double sgn = (!harmonic && (n % 2)) ? -1.0 : 1.0;
    for (int el = 0; el < L; ++el) {
      if (el < std::abs(spin)) {
        wa.push_back({0.0, 0.0});
        ws.push_back({0.0, 0.0});
        continue;
      }
      if (!b) {
        wa.push_back({k0[el], 0.0});
        ws.push_back({k0[el], 0.0});
        continue;
      }
      const double kj = kap[(size_t)(J_min + b - 1) * L + el];
      const double2 sv = std::abs(n) <= el ? s[(size_t)el * el + el + n] : double2{0.0, 0.0};
      const double fa = harmonic ? std::sqrt(8.0 * M_PI * M_PI / (2 * el + 1)) : ca;
      const double fs = harmonic ? std::sqrt((2 * el + 1) / (8.0 * M_PI * M_PI)) : cs;
      wa.push_back({sgn * kj * sv.x * fa, -sgn * kj * sv.y * fa});
      ws.push_back({sgn * kj * sv.x * fs, sgn * kj * sv.y * fs});
    }
  }
};

}  // namespace pxm

using namespace pxm;

struct pxm_dwav_plan_s {
  int L = 0, N = 0, Cmax = 0;
  std::vector<int> bl;            // [scaling, J_min .. J_max]
  int64_t ncoefs = 0, nscal = 0;
  pxm_sht_plan_t shtL = nullptr;  // spin 0 at L
  std::map<std::pair<int, int>, pxm_sht_plan_t> sht;  // (bl, spin) -> inner plan, shared by the items that need it
  struct Item {
    int block, n, bl;
    int64_t a_off, g_off;
    pxm_sht_plan_t plan;
  };
  std::vector<Item> items;
  double2* ws = nullptr;           // [flm: Cmax L^2 | harmonic arena | pixel arena]
  int64_t off_harm = 0, off_pix = 0;
  DwItem* d_items = nullptr;
  DwBlock* d_blocks = nullptr;
  int64_t* d_goff = nullptr;
  double2* d_wa = nullptr;         // analysis-split weights (-1)^n kappa_j conj(s_ln) / sqrt(2 pi); kappa_0 for the scaling
  double2* d_ws = nullptr;         // synthesis-merge weights (-1)^n kappa_j s_ln sqrt(2 pi); kappa_0 for the scaling
  double2* d_ph = nullptr;         // e^{i n_k gamma_q} [2N-1][N]
  int split_blocks = 0, gamma_blocks = 0;
  int64_t table_bytes = 0;
};

static std::vector<int> dw_sizes(int L, double B, int J_min, int N, int64_t* ncoefs, int64_t* nscal) {
  std::vector<int> bl = wav_bandlimits(L, B, J_min);
  int64_t n = (int64_t)bl[0] * (2 * bl[0] - 1);
  if (nscal) *nscal = n;
  for (size_t i = 1; i < bl.size(); ++i) n += (int64_t)(2 * N - 1) * bl[i] * (2 * bl[i] - 1);
  if (ncoefs) *ncoefs = n;
  return bl;
}

extern "C" {

int64_t pxm_dwav_ncoefs(int L, double B, int J_min, int N, int64_t* nscal_out) {
  PXM_REQUIRE(L >= 1 && B > 1.0 && J_min >= 0, "pxm_dwav_ncoefs: bad (L, B, J_min)");
  PXM_REQUIRE(N >= 1 && N <= L, "pxm_dwav_ncoefs: need 1 <= N <= L");
  int64_t n = 0;
  dw_sizes(L, B, J_min, N, &n, nscal_out);
  return n;
}

int pxm_dwav_plan_destroy(pxm_dwav_plan_t p) {
  if (!p) return 0;
  for (auto& kv : p->sht) pxm_sht_plan_destroy(kv.second);
  pxm_sht_plan_destroy(p->shtL);
  for (void* q : {(void*)p->ws, (void*)p->d_items, (void*)p->d_blocks, (void*)p->d_goff, (void*)p->d_wa, (void*)p->d_ws,
                  (void*)p->d_ph})
    deferred_free(q);
  delete p;
  drain_deferred();
  return 0;
}

int pxm_dwav_plan_create(int L, double B, int J_min, int N, int max_chains, unsigned flags, pxm_dwav_plan_t* plan) {
  (void)flags;
  PXM_REQUIRE(plan, "pxm_dwav_plan_create: null plan pointer");
  PXM_REQUIRE(L >= 2 && B > 1.0 && J_min >= 0, "pxm_dwav_plan_create: bad (L, B, J_min)");
  PXM_REQUIRE(N >= 1 && N <= L, "pxm_dwav_plan_create: need 1 <= N <= L");
  PXM_REQUIRE(max_chains >= 1 && max_chains <= 65535, "pxm_dwav_plan_create: max_chains outside [1, 65535]");
  PXM_REQUIRE(J_min <= j_max(L, B), "pxm_dwav_plan_create: J_min > J_max");
  PXM_REQUIRE(pxm_device_count() > 0, "pxm_dwav_plan_create: no HIP device visible (the HIP path is the only path)");
  std::unique_ptr<pxm_dwav_plan_s, int (*)(pxm_dwav_plan_t)> guard(new pxm_dwav_plan_s(), pxm_dwav_plan_destroy);
  pxm_dwav_plan_s* p = guard.get();
  p->L = L;
  p->N = N;
  p->Cmax = max_chains;
  p->bl = dw_sizes(L, B, J_min, N, &p->ncoefs, &p->nscal);
  const int nb = (int)p->bl.size();
  int rc;
  if ((rc = pxm_sht_plan_create(L, 0, max_chains, 0, &p->shtL))) return rc;

  // items: (scaling, n = 0), then (j, n) for |n| < bl_j; arenas laid out item after item
  const DwTiling tw(L, B, J_min, N, 0);
  std::vector<double2> wa, wsy;
  std::vector<DwItem> hitems;
  std::vector<int64_t> goff((size_t)nb * N, -1);
  int64_t harm = 0, pix = 0;
  int blk = 0;
  for (int b = 0; b < nb; ++b) {
    const int bl = p->bl[b];
    for (int k = 0; k < (b ? N : 1); ++k) {
      const int n = b ? -(N - 1) + 2 * k : 0;
      if (std::abs(n) >= bl) continue;
      pxm_sht_plan_t& sp = p->sht[{bl, -n}];
      if (!sp && (rc = pxm_sht_plan_create(bl, -n, max_chains, 0, &sp))) return rc;
      p->items.push_back({b, n, bl, harm, pix, sp});
      hitems.push_back({harm, (int64_t)bl * bl, (int64_t)wa.size(), bl, blk});
      goff[(size_t)b * N + k] = pix;
      tw.rows(b, n, false, wa, wsy);
      harm += (int64_t)max_chains * bl * bl;
      pix += (int64_t)max_chains * bl * (2 * bl - 1);
      blk += (bl * bl + DW_THREADS - 1) / DW_THREADS;
    }
  }
  p->split_blocks = blk;
  std::vector<DwBlock> hblocks;
  int64_t coef = 0;
  blk = 0;
  for (int b = 0; b < nb; ++b) {
    const int bl = p->bl[b], npix = bl * (2 * bl - 1);
    const int npl = b ? 2 * N - 1 : 1;
    hblocks.push_back({coef, (int64_t)b * N, npix, npl, b ? N : 1, blk});
    coef += (int64_t)npl * npix;
    blk += (npix + DW_THREADS - 1) / DW_THREADS;
  }
  p->gamma_blocks = blk;
  PXM_REQUIRE(p->split_blocks < (1 << 30) && p->gamma_blocks < (1 << 30), "pxm_dwav_plan_create: grid too large");
  std::vector<double2> ph((size_t)(2 * N - 1) * N);
  for (int q = 0; q < 2 * N - 1; ++q)
    for (int k = 0; k < N; ++k) {
      // e^{i n gamma_q}, n gamma_q = 2 pi (n q mod (2N-1)) / (2N-1): the angle reduced exactly before the sincos
      const int n = -(N - 1) + 2 * k;
      const int r = (((n * q) % (2 * N - 1)) + (2 * N - 1)) % (2 * N - 1);
      const double a = 2.0 * M_PI * r / (2 * N - 1);
      ph[(size_t)q * N + k] = double2{std::cos(a), std::sin(a)};
    }

  p->off_harm = (int64_t)max_chains * L * L;
  p->off_pix = p->off_harm + harm;
  const size_t wsb = (size_t)(p->off_pix + pix) * sizeof(double2);
  if ((rc = dev_alloc(&p->ws, wsb, "directional wavelet plan workspace"))) return rc;
  if ((rc = dev_zero(p->ws, wsb))) return rc;
  // (the split writes every item operand in full and the SHT stages every g_n: the zeroing only keeps unused tails clean)
  auto up = [&](auto** d, const auto& v, const char* what) -> int {
    const size_t bytes = v.size() * sizeof(v[0]);
    if (int r = dev_alloc(d, bytes, what)) return r;
    p->table_bytes += (int64_t)bytes;
    return dev_upload(*d, v.data(), bytes);
  };
  if ((rc = up(&p->d_items, hitems, "directional wavelet items"))) return rc;
  if ((rc = up(&p->d_blocks, hblocks, "directional wavelet blocks"))) return rc;
  if ((rc = up(&p->d_goff, goff, "directional wavelet g offsets"))) return rc;
  if ((rc = up(&p->d_wa, wa, "directional wavelet analysis weights"))) return rc;
  if ((rc = up(&p->d_ws, wsy, "directional wavelet synthesis weights"))) return rc;
  if ((rc = up(&p->d_ph, ph, "directional wavelet gamma phases"))) return rc;
  *plan = guard.release();
  return 0;
}

}  // extern "C"

namespace pxm {

static int dw_check(pxm_dwav_plan_t p, const void* a, const void* b, int C, hipStream_t st, const char* who) {
  if (!p || !a || !b) {
    set_error(std::string(who) + ": null argument");
    return -1;
  }
  if (C < 1 || C > p->Cmax) {
    set_error(std::string(who) + ": C outside [1, max_chains]");
    return -1;
  }
  note_stream(st);
  return 0;
}

// weights: 0 analysis (wa), 1 synthesis (ws); cj: conjugate them
static int dw_split(pxm_dwav_plan_t p, int weights, int cj, int C, hipStream_t st) {
  const dim3 g(p->split_blocks, C);
  hipLaunchKernelGGL(k_dw_split, g, dim3(DW_THREADS), 0, st, p->ws, p->ws + p->off_harm, p->d_items, (int)p->items.size(),
                     weights ? p->d_ws : p->d_wa, cj, p->L);
  PXM_HIP(hipGetLastError());
  return 0;
}

static int dw_merge(pxm_dwav_plan_t p, int weights, int cj, int C, hipStream_t st) {
  const dim3 g((p->L * p->L + DW_THREADS - 1) / DW_THREADS, C);
  hipLaunchKernelGGL(k_dw_merge, g, dim3(DW_THREADS), 0, st, p->ws + p->off_harm, p->ws, p->d_items, (int)p->items.size(),
                     weights ? p->d_ws : p->d_wa, cj, p->L);
  PXM_HIP(hipGetLastError());
  return 0;
}

// fwd: arena g_n -> coefficients X; back: X -> arena.  norm: the 1/(2N-1) of the gamma quadrature on wavelet planes
static int dw_gamma(pxm_dwav_plan_t p, bool fwd, const double2* in, double2* out, int norm, int C, hipStream_t st) {
  const dim3 g(p->gamma_blocks, C);
  const int nb = (int)p->bl.size();
  const double2* pin = fwd ? p->ws + p->off_pix : in;
  double2* pout = fwd ? out : p->ws + p->off_pix;
  switch (p->N) {
#define DW_CASE(K) \
  case K: dw_gamma_launch<K>(fwd, g, st, pin, pout, p->d_blocks, nb, p->d_goff, p->d_ph, p->N, p->ncoefs, norm); break;
    DW_CASE(1) DW_CASE(2) DW_CASE(3) DW_CASE(4) DW_CASE(5) DW_CASE(6) DW_CASE(7) DW_CASE(8)
#undef DW_CASE
    default: dw_gamma_launch<0>(fwd, g, st, pin, pout, p->d_blocks, nb, p->d_goff, p->d_ph, p->N, p->ncoefs, norm);
  }
  static_assert(DW_REG_N == 8, "the switch above instantiates 1 .. DW_REG_N");
  PXM_HIP(hipGetLastError());
  return 0;
}

// kind: 0 inverse, 1 forward, 2 inverse_adjoint, 3 forward_adjoint of every item's inner plan, arena to arena
static int dw_items_sht(pxm_dwav_plan_t p, int kind, int C, hipStream_t st) {
  for (const auto& it : p->items) {
    double2* a = p->ws + p->off_harm + it.a_off;
    double2* g = p->ws + p->off_pix + it.g_off;
    int rc = 0;
    switch (kind) {
      case 0: rc = pxm_sht_inverse(it.plan, a, g, C, st); break;
      case 1: rc = pxm_sht_forward(it.plan, g, a, C, st); break;
      case 2: rc = pxm_sht_inverse_adjoint(it.plan, g, a, C, st); break;
      default: rc = pxm_sht_forward_adjoint(it.plan, a, g, C, st); break;
    }
    if (rc) return rc;
  }
  return 0;
}

}  // namespace pxm

extern "C" {

int pxm_dwav_analysis(pxm_dwav_plan_t p, const void* f, void* X, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = dw_check(p, f, X, C, st, "pxm_dwav_analysis");
  if (!rc) rc = pxm_sht_forward(p->shtL, f, p->ws, C, stream);
  if (!rc) rc = dw_split(p, 0, 0, C, st);
  if (!rc) rc = dw_items_sht(p, 0, C, st);
  if (!rc) rc = dw_gamma(p, true, nullptr, (double2*)X, 0, C, st);
  return rc;
}

int pxm_dwav_analysis_adjoint(pxm_dwav_plan_t p, const void* X, void* f, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = dw_check(p, X, f, C, st, "pxm_dwav_analysis_adjoint");
  if (!rc) rc = dw_gamma(p, false, (const double2*)X, nullptr, 0, C, st);
  if (!rc) rc = dw_items_sht(p, 2, C, st);
  if (!rc) rc = dw_merge(p, 0, 1, C, st);
  if (!rc) rc = pxm_sht_forward_adjoint(p->shtL, p->ws, f, C, stream);
  return rc;
}

int pxm_dwav_synthesis(pxm_dwav_plan_t p, const void* X, void* f, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = dw_check(p, X, f, C, st, "pxm_dwav_synthesis");
  if (!rc) rc = dw_gamma(p, false, (const double2*)X, nullptr, 1, C, st);
  if (!rc) rc = dw_items_sht(p, 1, C, st);
  if (!rc) rc = dw_merge(p, 1, 0, C, st);
  if (!rc) rc = pxm_sht_inverse(p->shtL, p->ws, f, C, stream);
  return rc;
}

int pxm_dwav_synthesis_adjoint(pxm_dwav_plan_t p, const void* f, void* X, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = dw_check(p, f, X, C, st, "pxm_dwav_synthesis_adjoint");
  if (!rc) rc = pxm_sht_inverse_adjoint(p->shtL, f, p->ws, C, stream);
  if (!rc) rc = dw_split(p, 1, 1, C, st);
  if (!rc) rc = dw_items_sht(p, 3, C, st);
  if (!rc) rc = dw_gamma(p, true, nullptr, (double2*)X, 1, C, st);
  return rc;
}

int64_t pxm_dwav_table_bytes(pxm_dwav_plan_t p) {
  if (!p) return -1;
  int64_t n = p->table_bytes;
  auto add = [&](pxm_sht_plan_t s) {
    for (int op = 0; op < 4; ++op) n += pxm_sht_table_bytes(s, op);
  };
  add(p->shtL);
  for (auto& kv : p->sht)
    if (kv.first != std::make_pair(p->L, 0)) add(kv.second);  // (the cache shares the tables of one (L, spin))
  return n;
}

int pxm_dwav_status(pxm_dwav_plan_t p, int clear, pxm_stream_t stream) {
  PXM_REQUIRE(p, "pxm_dwav_status: null plan");
  int s = pxm_sht_status(p->shtL, clear, stream);
  if (s < 0) return s;
  for (auto& kv : p->sht) {
    const int t = pxm_sht_status(kv.second, clear, stream);
    if (t < 0) return t;
    s |= t;
  }
  return s;
}

int pxm_dwav_plan_info(pxm_dwav_plan_t p, int* nitems, int* split_blocks, int* gamma_blocks) {
  PXM_REQUIRE(p, "pxm_dwav_plan_info: null plan");
  if (nitems) *nitems = (int)p->items.size();
  if (split_blocks) *split_blocks = p->split_blocks;
  if (gamma_blocks) *gamma_blocks = p->gamma_blocks;
  return 0;
}

}  // extern "C"

// ---- harmonic-space wavelet plan (pxm_hwav_*) ----------------------------------------------------
// The coefficients are the (block, n) operands of the split / merge themselves, stored chain-major in one vector: the four
// operators are one k_dw_split or k_dw_merge launch each, with the items addressing [C][ncoefs] (cstride = ncoefs).
namespace pxm {

// One MYULA iteration, one lane per (chain, lm).  The K items with a non-zero merge weight at this degree (row el of
// act, in item order) keep their coefficients in registers from the merge through the update to the merge of the new
// state; the items with a zero weight have no gradient and are streamed through the update.  K = 0: any count, the
// coefficients re-read instead of held.
template <int K>
__global__ __launch_bounds__(DW_THREADS) void k_hw_myula(const double2* __restrict__ X, const double2* __restrict__ data,
                                                         const double* __restrict__ invcov, int ic_cplx,
                                                         const double* __restrict__ kern, const DwItem* __restrict__ items,
                                                         int nitems, const int* __restrict__ act, int kact,
                                                         const double2* __restrict__ Ws, int L, int64_t ncoefs, PxOut o,
                                                         double2* __restrict__ Xout, double2* __restrict__ preds) {
  const int lm = blockIdx.x * DW_THREADS + threadIdx.x;
  if (lm >= L * L) return;
  const int c = blockIdx.y;
  const int el = dw_el(lm);
  const uint64_t it = o.iter + (o.iter_dev ? *o.iter_dev : 0);
  const double2* xc = X + (int64_t)c * ncoefs;
  double2* xo = Xout + (int64_t)c * ncoefs;
  const int* a = act + (int64_t)el * kact;
  // the measurement at lm: 1 (identity) or k_l with l < 2 zeroed (WeakLensingHarmonic.harmonic_mapping)
  const double kl = kern ? (lm < 4 ? 0.0 : kern[lm]) : 1.0;
  auto update = [&](double2 x, int64_t e, double2 g) {
    return px_update(o, x, o.T ? o.T[e] : o.T_scalar, g, px_noise_philox(o, c, e, it));
  };
  auto residual = [&](double2 f) {  // k invcov (k f - d): the gradient of the data fidelity at lm before the split
    double2 r = csub(double2{kl * f.x, kl * f.y}, data[lm]);
    if (ic_cplx) r = cmul(reinterpret_cast<const double2*>(invcov)[lm], r);
    else r = double2{invcov[lm] * r.x, invcov[lm] * r.y};
    return double2{kl * r.x, kl * r.y};
  };
  double2 fn{0.0, 0.0};
  if constexpr (K > 0) {
    double2 x[K], w[K];
    int64_t e[K];
    double2 f{0.0, 0.0};
#pragma clang loop unroll(full)
    for (int k = 0; k < K; ++k) {
      const int d = k < kact ? a[k] : -1;
      e[k] = -1;
      x[k] = w[k] = double2{0.0, 0.0};
      if (d >= 0) {
        const DwItem itm = items[d];
        e[k] = itm.a_off + lm;
        w[k] = Ws[itm.w_off + el];
        x[k] = xc[e[k]];
      }
      f = cadd(f, cmul(w[k], x[k]));
    }
    const double2 g = residual(f);
#pragma clang loop unroll(full)
    for (int k = 0; k < K; ++k) {
      if (e[k] >= 0) {
        x[k] = update(x[k], e[k], cmul(double2{w[k].x, -w[k].y}, g));
        xo[e[k]] = x[k];
      }
    }
#pragma clang loop unroll(full)
    for (int k = 0; k < K; ++k) fn = cadd(fn, cmul(w[k], x[k]));
  } else {
    double2 f{0.0, 0.0};
    for (int k = 0; k < kact && a[k] >= 0; ++k) {
      const DwItem itm = items[a[k]];
      f = cadd(f, cmul(Ws[itm.w_off + el], xc[itm.a_off + lm]));
    }
    const double2 g = residual(f);
    for (int k = 0; k < kact && a[k] >= 0; ++k) {
      const DwItem itm = items[a[k]];
      const double2 w = Ws[itm.w_off + el];
      const int64_t e = itm.a_off + lm;
      const double2 xn = update(xc[e], e, cmul(double2{w.x, -w.y}, g));
      xo[e] = xn;
      fn = cadd(fn, cmul(w, xn));
    }
  }
  for (int d = 0; d < nitems; ++d) {  // zero weight at this degree (or outside the block): no gradient
    const DwItem itm = items[d];
    if (el >= itm.bl) continue;
    const double2 w = Ws[itm.w_off + el];
    if (w.x != 0.0 || w.y != 0.0) continue;
    const int64_t e = itm.a_off + lm;
    xo[e] = update(xc[e], e, double2{0.0, 0.0});
  }
  preds[(int64_t)c * L * L + lm] = double2{kl * fn.x, kl * fn.y};
}

static std::vector<int> hw_sizes(int L, double B, int J_min, int N, int64_t* ncoefs, int64_t* nscal) {
  std::vector<int> bl = wav_bandlimits(L, B, J_min);
  int64_t n = (int64_t)bl[0] * bl[0];
  if (nscal) *nscal = n;
  for (size_t i = 1; i < bl.size(); ++i) n += (int64_t)N * bl[i] * bl[i];
  if (ncoefs) *ncoefs = n;
  return bl;
}

}  // namespace pxm

struct pxm_hwav_plan_s {
  int L = 0, N = 0, spin = 0, Cmax = 0;
  std::vector<int> bl;  // [scaling, J_min .. J_max]
  int64_t ncoefs = 0, nscal = 0;
  int nitems = 0, split_blocks = 0, kact = 0;
  DwItem* d_items = nullptr;  // (scaling, n = 0), then every (j, n): a_off = offset of the block in a chain's vector
  double2* d_wa = nullptr;    // analysis weights sqrt(8 pi^2/(2l+1)) kappa_j conj(s_ln); kappa_0 for the scaling
  double2* d_ws = nullptr;    // synthesis weights sqrt((2l+1)/(8 pi^2)) kappa_j s_ln; kappa_0 for the scaling
  int* d_act = nullptr;       // [L][kact]: the items with a non-zero synthesis weight at degree l, in item order, -1 padded
};

extern "C" {

int64_t pxm_hwav_ncoefs(int L, double B, int J_min, int N, int64_t* nscal_out) {
  PXM_REQUIRE(L >= 1 && B > 1.0 && J_min >= 0, "pxm_hwav_ncoefs: bad (L, B, J_min)");
  PXM_REQUIRE(N >= 1 && N <= L, "pxm_hwav_ncoefs: need 1 <= N <= L");
  int64_t n = 0;
  hw_sizes(L, B, J_min, N, &n, nscal_out);
  return n;
}

int pxm_hwav_plan_destroy(pxm_hwav_plan_t p) {
  if (!p) return 0;
  for (void* q : {(void*)p->d_items, (void*)p->d_wa, (void*)p->d_ws, (void*)p->d_act}) deferred_free(q);
  delete p;
  drain_deferred();
  return 0;
}

int pxm_hwav_plan_create(int L, double B, int J_min, int N, int spin, int max_chains, unsigned flags, pxm_hwav_plan_t* plan) {
  (void)flags;
  PXM_REQUIRE(plan, "pxm_hwav_plan_create: null plan pointer");
  PXM_REQUIRE(L >= 2 && B > 1.0 && J_min >= 0, "pxm_hwav_plan_create: bad (L, B, J_min)");
  PXM_REQUIRE(N >= 1 && N <= L, "pxm_hwav_plan_create: need 1 <= N <= L");
  PXM_REQUIRE(std::abs(spin) < L, "pxm_hwav_plan_create: |spin| must be < L");
  PXM_REQUIRE(spin == 0 || N == 1, "pxm_hwav_plan_create: spin != 0 needs N = 1 (spin directional wavelets are not supported)");
  PXM_REQUIRE(max_chains >= 1 && max_chains <= 65535, "pxm_hwav_plan_create: max_chains outside [1, 65535]");
  PXM_REQUIRE(J_min <= j_max(L, B), "pxm_hwav_plan_create: J_min > J_max");
  PXM_REQUIRE(pxm_device_count() > 0, "pxm_hwav_plan_create: no HIP device visible (the HIP path is the only path)");
  std::unique_ptr<pxm_hwav_plan_s, int (*)(pxm_hwav_plan_t)> guard(new pxm_hwav_plan_s(), pxm_hwav_plan_destroy);
  pxm_hwav_plan_s* p = guard.get();
  p->L = L;
  p->N = N;
  p->spin = spin;
  p->Cmax = max_chains;
  p->bl = hw_sizes(L, B, J_min, N, &p->ncoefs, &p->nscal);
  const int nb = (int)p->bl.size();
  // items: (scaling, n = 0), then (j, n) for every n -- the layout stores every block, s_ln = 0 ones included
  const DwTiling tw(L, B, J_min, N, spin);
  std::vector<double2> wa, wsy;
  std::vector<DwItem> hitems;
  int64_t off = 0;
  int blk = 0;
  for (int b = 0; b < nb; ++b) {
    const int bl = p->bl[b];
    for (int k = 0; k < (b ? N : 1); ++k) {
      const int n = b ? -(N - 1) + 2 * k : 0;
      hitems.push_back({off, p->ncoefs, (int64_t)wa.size(), bl, blk});
      tw.rows(b, n, true, wa, wsy);
      off += (int64_t)bl * bl;
      blk += (bl * bl + DW_THREADS - 1) / DW_THREADS;
    }
  }
  PXM_REQUIRE(off == p->ncoefs, "pxm_hwav_plan_create: layout mismatch");
  PXM_REQUIRE(blk < (1 << 30), "pxm_hwav_plan_create: grid too large");
  p->nitems = (int)hitems.size();
  p->split_blocks = blk;
  std::vector<std::vector<int>> rows(L);
  for (int d = 0; d < p->nitems; ++d)
    for (int el = 0; el < hitems[d].bl; ++el) {
      const double2 w = wsy[(size_t)hitems[d].w_off + el];
      if (w.x != 0.0 || w.y != 0.0) rows[el].push_back(d);
    }
  for (const auto& r : rows) p->kact = std::max(p->kact, (int)r.size());
  p->kact = std::max(p->kact, 1);
  std::vector<int> act((size_t)L * p->kact, -1);
  for (int el = 0; el < L; ++el) std::copy(rows[el].begin(), rows[el].end(), act.begin() + (size_t)el * p->kact);
  int rc;
  auto up = [&](auto** d, const auto& v, const char* what) -> int {
    const size_t bytes = v.size() * sizeof(v[0]);
    if (int r = dev_alloc(d, bytes, what)) return r;
    return dev_upload(*d, v.data(), bytes);
  };
  if ((rc = up(&p->d_items, hitems, "harmonic wavelet items"))) return rc;
  if ((rc = up(&p->d_wa, wa, "harmonic wavelet analysis weights"))) return rc;
  if ((rc = up(&p->d_ws, wsy, "harmonic wavelet synthesis weights"))) return rc;
  if ((rc = up(&p->d_act, act, "harmonic wavelet active items per degree"))) return rc;
  *plan = guard.release();
  return 0;
}

}  // extern "C"

namespace pxm {

static int hw_check(pxm_hwav_plan_t p, const void* a, const void* b, int C, hipStream_t st, const char* who) {
  if (!p || !a || !b) {
    set_error(std::string(who) + ": null argument");
    return -1;
  }
  if (C < 1 || C > p->Cmax) {
    set_error(std::string(who) + ": C outside [1, max_chains]");
    return -1;
  }
  note_stream(st);
  return 0;
}

static int hw_split(pxm_hwav_plan_t p, const void* flm, void* X, int weights, int cj, int C, hipStream_t st) {
  hipLaunchKernelGGL(k_dw_split, dim3(p->split_blocks, C), dim3(DW_THREADS), 0, st, (const double2*)flm, (double2*)X,
                     p->d_items, p->nitems, weights ? p->d_ws : p->d_wa, cj, p->L);
  PXM_HIP(hipGetLastError());
  return 0;
}

static int hw_merge(pxm_hwav_plan_t p, const void* X, void* flm, int weights, int cj, int C, hipStream_t st) {
  hipLaunchKernelGGL(k_dw_merge, dim3((p->L * p->L + DW_THREADS - 1) / DW_THREADS, C), dim3(DW_THREADS), 0, st,
                     (const double2*)X, (double2*)flm, p->d_items, p->nitems, weights ? p->d_ws : p->d_wa, cj, p->L);
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // namespace pxm

extern "C" {

int pxm_hwav_analysis(pxm_hwav_plan_t p, const void* flm, void* X, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = hw_check(p, flm, X, C, st, "pxm_hwav_analysis");
  return rc ? rc : hw_split(p, flm, X, 0, 0, C, st);
}

int pxm_hwav_analysis_adjoint(pxm_hwav_plan_t p, const void* X, void* flm, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = hw_check(p, X, flm, C, st, "pxm_hwav_analysis_adjoint");
  return rc ? rc : hw_merge(p, X, flm, 0, 1, C, st);
}

int pxm_hwav_synthesis(pxm_hwav_plan_t p, const void* X, void* flm, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = hw_check(p, X, flm, C, st, "pxm_hwav_synthesis");
  return rc ? rc : hw_merge(p, X, flm, 1, 0, C, st);
}

int pxm_hwav_synthesis_adjoint(pxm_hwav_plan_t p, const void* flm, void* X, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = hw_check(p, flm, X, C, st, "pxm_hwav_synthesis_adjoint");
  return rc ? rc : hw_split(p, flm, X, 1, 1, C, st);
}

int pxm_hwav_status(pxm_hwav_plan_t p, int clear, pxm_stream_t stream) {
  (void)clear;
  (void)stream;
  PXM_REQUIRE(p, "pxm_hwav_status: null plan");
  return 0;
}

int pxm_hwav_plan_info(pxm_hwav_plan_t p, int* nitems, int* split_blocks, int* kact) {
  PXM_REQUIRE(p, "pxm_hwav_plan_info: null plan");
  if (nitems) *nitems = p->nitems;
  if (split_blocks) *split_blocks = p->split_blocks;
  if (kact) *kact = p->kact;
  return 0;
}

int pxm_hwav_myula_step(pxm_hwav_plan_t p, const void* X, const void* data, const void* invcov, int invcov_complex,
                        const double* kernel, const double* T, double T_scalar, double delta, double lmda, int mode,
                        uint64_t seed, uint64_t chain0, uint64_t iter, const uint64_t* iter_dev, void* X_out,
                        void* preds_out, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = hw_check(p, X, X_out, C, st, "pxm_hwav_myula_step")) return rc;
  PXM_REQUIRE(data && invcov && preds_out, "pxm_hwav_myula_step: null argument");
  PXM_REQUIRE(X != X_out, "pxm_hwav_myula_step: X_out must not alias X");
  const int m = mode & ~PXM_NOISE_F64;
  PXM_REQUIRE(m == PXM_MODE_REAL_NOISE || m == PXM_MODE_CPLX_NOISE,
              "pxm_hwav_myula_step: mode must be 0 or 1 (two real chains per slot are refused: harmonic coefficients are never real)");
  PxOut o;
  o.T = T;
  o.T_scalar = T_scalar;
  o.delta = delta;
  o.lmda = lmda;
  o.mode = m;
  o.noise64 = (mode & PXM_NOISE_F64) ? 1 : 0;
  o.seed = seed;
  o.chain0 = chain0;
  o.iter = iter;
  o.iter_dev = iter_dev;
  const dim3 g((p->L * p->L + DW_THREADS - 1) / DW_THREADS, C);
  const int K = p->kact <= 2 ? 2 : p->kact <= 3 ? 3 : p->kact <= 5 ? 5 : p->kact <= 9 ? 9 : p->kact <= 17 ? 17 : 0;
  switch (K) {
#define HW_CASE(KK)                                                                                                        \
  case KK:                                                                                                                 \
    hipLaunchKernelGGL(k_hw_myula<KK>, g, dim3(DW_THREADS), 0, st, (const double2*)X, (const double2*)data,              \
                       (const double*)invcov, invcov_complex, kernel, p->d_items, p->nitems, p->d_act, p->kact, p->d_ws,   \
                       p->L, p->ncoefs, o, (double2*)X_out, (double2*)preds_out);                                          \
    break;
    HW_CASE(2) HW_CASE(3) HW_CASE(5) HW_CASE(9) HW_CASE(17)
    default: HW_CASE(0)
#undef HW_CASE
  }
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
