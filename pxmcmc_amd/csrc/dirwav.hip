// Directional (N = dirs >= 1) scale-discretised wavelet transforms, spin 0, upsample = 0 (Leistedt et al. 2013;
// McEwen et al. 2015, "Directional spin wavelets on the sphere"): what pys2let.analysis_px2wav / synthesis_wav2px and
// their adjoints compute with N > 1 (pxmcmc/transforms.py:95-98).  Conventions: DESIGN.md section 11.
//
// Per scale j and orientation index n in {-(N-1), -(N-3), .., N-1} the SO(3) transform factors into spin transforms:
//
//   analysis    a^{j,n}_lm = (-1)^n kappa_j(l) conj(s_ln) f_lm / sqrt(2 pi)      harmonic split   (harm_stage.h: k_dw_split)
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
// The gamma kernels are complex128 streams: one 16-byte element per lane, phases from a host table (no device trig), one
// launch per direction for every block and chain (grid.y = chain, grid.x = the blocks' workgroups back to back).
#include "plan_common.h"
#include "elem.h"
#include "harm_stage.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <vector>

namespace pxm {

constexpr int DW_REG_N = 8;  // orientation counts up to this keep the N inputs / outputs of a pixel in registers

struct DwBlock {   // one coefficient block (scaling, or scale j with its planes) of the gamma stage
  int64_t coef_off;  // offset of the block in a chain's coefficient vector
  int64_t goff;      // row of the g-offset table: nn entries, offset of g_n in the pixel arena or -1 (skipped pair)
  int npix, nplanes, nn;
  int blk0;
};

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
  int64_t off_harm = 0, off_pix = 0, ws_elems = 0;
  std::vector<DwBlock> blocks;     // the host copies of d_blocks and d_goff (pxm_dwav_workspace_layout)
  std::vector<int64_t> goff;
  HarmStage hs;                    // items in the harmonic arena; wa = (-1)^n kappa_j conj(s_ln) / sqrt(2 pi),
                                   // ws = (-1)^n kappa_j s_ln sqrt(2 pi); kappa_0 for the scaling function in both
  DwBlock* d_blocks = nullptr;
  int64_t* d_goff = nullptr;
  double2* d_ph = nullptr;         // e^{i n_k gamma_q} [2N-1][N]
  int gamma_blocks = 0;
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
  harm_release(&p->hs);
  for (void* q : {(void*)p->ws, (void*)p->d_blocks, (void*)p->d_goff, (void*)p->d_ph}) deferred_free(q);
  delete p;
  drain_deferred();
  return 0;
}

int pxm_dwav_plan_create(int L, double B, int J_min, int N, int max_chains, unsigned flags, pxm_dwav_plan_t* plan) {
  (void)flags;
  if (int rc = harm_create_check("pxm_dwav_plan_create", plan, L, B, J_min, N, 0, max_chains)) return rc;
  std::unique_ptr<pxm_dwav_plan_s, int (*)(pxm_dwav_plan_t)> guard(new pxm_dwav_plan_s(), pxm_dwav_plan_destroy);
  pxm_dwav_plan_s* p = guard.get();
  p->L = L;
  p->hs.L = L;
  p->N = N;
  p->Cmax = max_chains;
  p->bl = dw_sizes(L, B, J_min, N, &p->ncoefs, &p->nscal);
  const int nb = (int)p->bl.size();
  int rc;
  if ((rc = pxm_sht_plan_create(L, 0, max_chains, 0, &p->shtL))) return rc;

  // items: (scaling, n = 0), then (j, n) for |n| < bl_j; arenas laid out item after item
  std::vector<double2> wa, wsy;
  const std::vector<HarmRow> wrows = harm_weight_rows(L, B, J_min, N, 0, false, wa, wsy);
  std::vector<DwItem> hitems;
  std::vector<int64_t>& goff = p->goff;
  goff.assign((size_t)nb * N, -1);
  int64_t harm = 0, pix = 0;
  int blk = 0;
  for (size_t d = 0; d < wrows.size(); ++d) {
    const int b = wrows[d].block, n = wrows[d].n, bl = wrows[d].bl;
    PXM_REQUIRE(b < nb && bl == p->bl[b], "pxm_dwav_plan_create: layout mismatch");
    pxm_sht_plan_t& sp = p->sht[{bl, -n}];
    if (!sp && (rc = pxm_sht_plan_create(bl, -n, max_chains, 0, &sp))) return rc;
    p->items.push_back({b, n, bl, harm, pix, sp});
    hitems.push_back({harm, (int64_t)bl * bl, (int64_t)d * L, bl, blk});
    goff[(size_t)b * N + (b ? (n + N - 1) / 2 : 0)] = pix;
    harm += (int64_t)max_chains * bl * bl;
    pix += (int64_t)max_chains * bl * (2 * bl - 1);
    blk += (bl * bl + DW_THREADS - 1) / DW_THREADS;
  }
  p->hs.nitems = (int)hitems.size();
  p->hs.split_blocks = blk;
  std::vector<DwBlock>& hblocks = p->blocks;
  int64_t coef = 0;
  blk = 0;
  for (int b = 0; b < nb; ++b) {
    const int bl = p->bl[b], npix = bl * (2 * bl - 1);
    const int npl = b ? 2 * N - 1 : 1;
    hblocks.push_back({coef, (int64_t)b * N, npix, npl, harm_orients(b, N), blk});
    coef += (int64_t)npl * npix;
    blk += (npix + DW_THREADS - 1) / DW_THREADS;
  }
  p->gamma_blocks = blk;
  PXM_REQUIRE(p->hs.split_blocks < (1 << 30) && p->gamma_blocks < (1 << 30), "pxm_dwav_plan_create: grid too large");
  const std::vector<double2> ph = dw_phases(N);

  p->off_harm = (int64_t)max_chains * L * L;
  p->off_pix = p->off_harm + harm;
  p->ws_elems = p->off_pix + pix;
  const size_t wsb = (size_t)p->ws_elems * sizeof(double2);
  if ((rc = dev_alloc(&p->ws, wsb, "directional wavelet plan workspace"))) return rc;
  if ((rc = dev_zero(p->ws, wsb))) return rc;
  // (the split writes every item operand in full and the SHT stages every g_n: the zeroing only keeps unused tails clean)
  if ((rc = dev_table(&p->hs.d_items, hitems, "directional wavelet items"))) return rc;
  if ((rc = dev_table(&p->d_blocks, hblocks, "directional wavelet blocks"))) return rc;
  if ((rc = dev_table(&p->d_goff, goff, "directional wavelet g offsets"))) return rc;
  if ((rc = dev_table(&p->hs.d_wa, wa, "directional wavelet analysis weights"))) return rc;
  if ((rc = dev_table(&p->hs.d_ws, wsy, "directional wavelet synthesis weights"))) return rc;
  if ((rc = dev_table(&p->d_ph, ph, "directional wavelet gamma phases"))) return rc;
  p->table_bytes = (int64_t)(hitems.size() * sizeof(DwItem) + hblocks.size() * sizeof(DwBlock) + goff.size() * sizeof(int64_t) +
                             (wa.size() + wsy.size() + ph.size()) * sizeof(double2));
  *plan = guard.release();
  return 0;
}

}  // extern "C"

namespace pxm {

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
  if (int rc = plan_check(p, f, X, C, "pxm_dwav_analysis")) return rc;
  note_stream(st);
  int rc = pxm_sht_forward(p->shtL, f, p->ws, C, stream);
  if (!rc) rc = harm_split(p->hs, p->ws, p->ws + p->off_harm, 0, 0, C, st);
  if (!rc) rc = dw_items_sht(p, 0, C, st);
  if (!rc) rc = dw_gamma(p, true, nullptr, (double2*)X, 0, C, st);
  return rc;
}

int pxm_dwav_analysis_adjoint(pxm_dwav_plan_t p, const void* X, void* f, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = plan_check(p, X, f, C, "pxm_dwav_analysis_adjoint")) return rc;
  note_stream(st);
  int rc = dw_gamma(p, false, (const double2*)X, nullptr, 0, C, st);
  if (!rc) rc = dw_items_sht(p, 2, C, st);
  if (!rc) rc = harm_merge(p->hs, p->ws + p->off_harm, p->ws, 0, 1, C, st);
  if (!rc) rc = pxm_sht_forward_adjoint(p->shtL, p->ws, f, C, stream);
  return rc;
}

int pxm_dwav_synthesis(pxm_dwav_plan_t p, const void* X, void* f, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = plan_check(p, X, f, C, "pxm_dwav_synthesis")) return rc;
  note_stream(st);
  int rc = dw_gamma(p, false, (const double2*)X, nullptr, 1, C, st);
  if (!rc) rc = dw_items_sht(p, 1, C, st);
  if (!rc) rc = harm_merge(p->hs, p->ws + p->off_harm, p->ws, 1, 0, C, st);
  if (!rc) rc = pxm_sht_inverse(p->shtL, p->ws, f, C, stream);
  return rc;
}

int pxm_dwav_synthesis_adjoint(pxm_dwav_plan_t p, const void* f, void* X, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = plan_check(p, f, X, C, "pxm_dwav_synthesis_adjoint")) return rc;
  note_stream(st);
  int rc = pxm_sht_inverse_adjoint(p->shtL, f, p->ws, C, stream);
  if (!rc) rc = harm_split(p->hs, p->ws, p->ws + p->off_harm, 1, 1, C, st);
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
  if (split_blocks) *split_blocks = p->hs.split_blocks;
  if (gamma_blocks) *gamma_blocks = p->gamma_blocks;
  return 0;
}

// ---- test hooks: the workspace and one stage of one operator at a time (include/pxmcmc_amd.h) ----
int64_t pxm_dwav_workspace_layout(pxm_dwav_plan_t p, int64_t* out, int64_t cap) {
  PXM_REQUIRE(p, "pxm_dwav_workspace_layout: null plan");
  std::vector<int64_t> w = {p->ws_elems, 0, (int64_t)p->Cmax * p->L * p->L, p->off_harm, p->off_pix, (int64_t)p->items.size(),
                            (int64_t)p->blocks.size(), p->Cmax};
  for (const auto& it : p->items)
    w.insert(w.end(), {it.block, it.n, it.bl, p->off_harm + it.a_off, (int64_t)it.bl * it.bl, p->off_pix + it.g_off,
                       (int64_t)it.bl * (2 * it.bl - 1), 0});
  for (const DwBlock& b : p->blocks) w.insert(w.end(), {b.coef_off, b.npix, b.nplanes, b.nn, b.blk0, b.goff, 0, 0});
  w.insert(w.end(), p->goff.begin(), p->goff.end());  // the table as uploaded
  const int64_t n = (int64_t)w.size();
  if (cap > 0) {
    PXM_REQUIRE(out, "pxm_dwav_workspace_layout: null destination");
    std::copy(w.begin(), w.begin() + std::min(cap, n), out);
  }
  return n;
}

int pxm_dwav_workspace_write(pxm_dwav_plan_t p, int64_t offset, const void* src, int64_t n, pxm_stream_t stream) {
  PXM_REQUIRE(p && src, "pxm_dwav_workspace_write: null argument");
  PXM_REQUIRE(offset >= 0 && n >= 0 && offset <= p->ws_elems && n <= p->ws_elems - offset,
              "pxm_dwav_workspace_write: range outside the workspace");
  note_stream((hipStream_t)stream);
  PXM_HIP(hipMemcpyAsync(p->ws + offset, src, (size_t)n * sizeof(double2), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int pxm_dwav_workspace_read(pxm_dwav_plan_t p, int64_t offset, void* dst, int64_t n, pxm_stream_t stream) {
  PXM_REQUIRE(p && dst, "pxm_dwav_workspace_read: null argument");
  PXM_REQUIRE(offset >= 0 && n >= 0 && offset <= p->ws_elems && n <= p->ws_elems - offset,
              "pxm_dwav_workspace_read: range outside the workspace");
  note_stream((hipStream_t)stream);
  PXM_HIP(hipMemcpyAsync(dst, p->ws + offset, (size_t)n * sizeof(double2), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int pxm_dwav_run_stage(pxm_dwav_plan_t p, int op, int stage, void* x, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  PXM_REQUIRE(p, "pxm_dwav_run_stage: null plan");
  PXM_REQUIRE(op >= 0 && op < 4 && stage >= 0 && stage < 4, "pxm_dwav_run_stage: op and stage must be 0 .. 3");
  PXM_REQUIRE(C >= 1 && C <= p->Cmax, "pxm_dwav_run_stage: C outside [1, max_chains]");
  PXM_REQUIRE(x || stage == 1 || stage == 2, "pxm_dwav_run_stage: the first and the last stage need X or f");
  note_stream(st);
  double2* harm = p->ws + p->off_harm;
  switch (4 * op + stage) {  // (the calls of pxm_dwav_analysis, _analysis_adjoint, _synthesis, _synthesis_adjoint, in their order)
    case 0: return pxm_sht_forward(p->shtL, x, p->ws, C, stream);
    case 1: return harm_split(p->hs, p->ws, harm, 0, 0, C, st);
    case 2: return dw_items_sht(p, 0, C, st);
    case 3: return dw_gamma(p, true, nullptr, (double2*)x, 0, C, st);
    case 4: return dw_gamma(p, false, (const double2*)x, nullptr, 0, C, st);
    case 5: return dw_items_sht(p, 2, C, st);
    case 6: return harm_merge(p->hs, harm, p->ws, 0, 1, C, st);
    case 7: return pxm_sht_forward_adjoint(p->shtL, p->ws, x, C, stream);
    case 8: return dw_gamma(p, false, (const double2*)x, nullptr, 1, C, st);
    case 9: return dw_items_sht(p, 1, C, st);
    case 10: return harm_merge(p->hs, harm, p->ws, 1, 0, C, st);
    case 11: return pxm_sht_inverse(p->shtL, p->ws, x, C, stream);
    case 12: return pxm_sht_inverse_adjoint(p->shtL, x, p->ws, C, stream);
    case 13: return harm_split(p->hs, p->ws, harm, 1, 1, C, st);
    case 14: return dw_items_sht(p, 3, C, st);
    default: return dw_gamma(p, true, nullptr, (double2*)x, 1, C, st);
  }
}

}  // extern "C"
