// Harmonic-space scale-discretised wavelet transforms (pxm_hwav_*): what pys2let's
// analysis_lm2lmn / synthesis_lmn2lm and their adjoints compute, and one fused MYULA iteration on them.
// The coefficients are the (block, n) operands of the split / merge themselves, stored chain-major in one vector: the four
// operators are one k_dw_split or k_dw_merge launch each (harm_stage.h), with the items addressing [C][ncoefs]
// (cstride = ncoefs).
#include "update.h"  // (first: its mode enum precedes the public header's PXM_MODE_* macros of the same values)
#include "plan_common.h"
#include "harm_stage.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

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

using namespace pxm;

struct pxm_hwav_plan_s {
  int L = 0, N = 0, spin = 0, Cmax = 0;
  std::vector<int> bl;  // [scaling, J_min .. J_max]
  int64_t ncoefs = 0, nscal = 0;
  int kact = 0;
  HarmStage hs;          // (scaling, n = 0), then every (j, n): a_off = offset of the block in a chain's vector;
                         // wa = sqrt(8 pi^2/(2l+1)) kappa_j conj(s_ln), ws = sqrt((2l+1)/(8 pi^2)) kappa_j s_ln;
                         // kappa_0 for the scaling function in both
  int* d_act = nullptr;  // [L][kact]: the items with a non-zero synthesis weight at degree l, in item order, -1 padded
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
  harm_release(&p->hs);
  deferred_free(p->d_act);
  delete p;
  drain_deferred();
  return 0;
}

int pxm_hwav_plan_create(int L, double B, int J_min, int N, int spin, int max_chains, unsigned flags, pxm_hwav_plan_t* plan) {
  (void)flags;
  if (int rc = harm_create_check("pxm_hwav_plan_create", plan, L, B, J_min, N, spin, max_chains)) return rc;
  std::unique_ptr<pxm_hwav_plan_s, int (*)(pxm_hwav_plan_t)> guard(new pxm_hwav_plan_s(), pxm_hwav_plan_destroy);
  pxm_hwav_plan_s* p = guard.get();
  p->L = L;
  p->hs.L = L;
  p->N = N;
  p->spin = spin;
  p->Cmax = max_chains;
  p->bl = hw_sizes(L, B, J_min, N, &p->ncoefs, &p->nscal);
  // items: (scaling, n = 0), then (j, n) for every n -- the layout stores every block, s_ln = 0 ones included
  std::vector<double2> wa, wsy;
  const std::vector<HarmRow> wrows = harm_weight_rows(L, B, J_min, N, spin, true, wa, wsy);
  std::vector<DwItem> hitems;
  int64_t off = 0;
  int blk = 0;
  for (size_t d = 0; d < wrows.size(); ++d) {
    const int bl = wrows[d].bl;
    hitems.push_back({off, p->ncoefs, (int64_t)d * L, bl, blk});
    off += (int64_t)bl * bl;
    blk += (bl * bl + DW_THREADS - 1) / DW_THREADS;
  }
  PXM_REQUIRE(off == p->ncoefs, "pxm_hwav_plan_create: layout mismatch");
  PXM_REQUIRE(blk < (1 << 30), "pxm_hwav_plan_create: grid too large");
  p->hs.nitems = (int)hitems.size();
  p->hs.split_blocks = blk;
  std::vector<std::vector<int>> rows(L);
  for (int d = 0; d < p->hs.nitems; ++d)
    for (int el = 0; el < hitems[d].bl; ++el) {
      const double2 w = wsy[(size_t)hitems[d].w_off + el];
      if (w.x != 0.0 || w.y != 0.0) rows[el].push_back(d);
    }
  for (const auto& r : rows) p->kact = std::max(p->kact, (int)r.size());
  p->kact = std::max(p->kact, 1);
  std::vector<int> act((size_t)L * p->kact, -1);
  for (int el = 0; el < L; ++el) std::copy(rows[el].begin(), rows[el].end(), act.begin() + (size_t)el * p->kact);
  int rc;
  if ((rc = dev_table(&p->hs.d_items, hitems, "harmonic wavelet items"))) return rc;
  if ((rc = dev_table(&p->hs.d_wa, wa, "harmonic wavelet analysis weights"))) return rc;
  if ((rc = dev_table(&p->hs.d_ws, wsy, "harmonic wavelet synthesis weights"))) return rc;
  if ((rc = dev_table(&p->d_act, act, "harmonic wavelet active items per degree"))) return rc;
  *plan = guard.release();
  return 0;
}

int pxm_hwav_analysis(pxm_hwav_plan_t p, const void* flm, void* X, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = plan_check(p, flm, X, C, "pxm_hwav_analysis")) return rc;
  note_stream(st);
  return harm_split(p->hs, (const double2*)flm, (double2*)X, 0, 0, C, st);
}

int pxm_hwav_analysis_adjoint(pxm_hwav_plan_t p, const void* X, void* flm, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = plan_check(p, X, flm, C, "pxm_hwav_analysis_adjoint")) return rc;
  note_stream(st);
  return harm_merge(p->hs, (const double2*)X, (double2*)flm, 0, 1, C, st);
}

int pxm_hwav_synthesis(pxm_hwav_plan_t p, const void* X, void* flm, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = plan_check(p, X, flm, C, "pxm_hwav_synthesis")) return rc;
  note_stream(st);
  return harm_merge(p->hs, (const double2*)X, (double2*)flm, 1, 0, C, st);
}

int pxm_hwav_synthesis_adjoint(pxm_hwav_plan_t p, const void* flm, void* X, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = plan_check(p, flm, X, C, "pxm_hwav_synthesis_adjoint")) return rc;
  note_stream(st);
  return harm_split(p->hs, (const double2*)flm, (double2*)X, 1, 1, C, st);
}

int pxm_hwav_status(pxm_hwav_plan_t p, int clear, pxm_stream_t stream) {
  (void)clear;
  (void)stream;
  PXM_REQUIRE(p, "pxm_hwav_status: null plan");
  return 0;
}

int pxm_hwav_plan_info(pxm_hwav_plan_t p, int* nitems, int* split_blocks, int* kact) {
  PXM_REQUIRE(p, "pxm_hwav_plan_info: null plan");
  if (nitems) *nitems = p->hs.nitems;
  if (split_blocks) *split_blocks = p->hs.split_blocks;
  if (kact) *kact = p->kact;
  return 0;
}

int pxm_hwav_myula_step(pxm_hwav_plan_t p, const void* X, const void* data, const void* invcov, int invcov_complex,
                        const double* kernel, const double* T, double T_scalar, double delta, double lmda, int mode,
                        uint64_t seed, uint64_t chain0, uint64_t iter, const uint64_t* iter_dev, void* X_out,
                        void* preds_out, int C, pxm_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int rc = plan_check(p, X, X_out, C, "pxm_hwav_myula_step")) return rc;
  note_stream(st);
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
                       (const double*)invcov, invcov_complex, kernel, p->hs.d_items, p->hs.nitems, p->d_act, p->kact,    \
                       p->hs.d_ws, p->L, p->ncoefs, o, (double2*)X_out, (double2*)preds_out);                              \
    break;
    HW_CASE(2) HW_CASE(3) HW_CASE(5) HW_CASE(9) HW_CASE(17)
    default: HW_CASE(0)
#undef HW_CASE
  }
  PXM_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
