// Weak-lensing measurement fused with the wavelet synthesis (BASELINE config 5): the plan's attachment and pxm_wav_wl_*.
// forward  = WeakLensing.forward(transform.inverse(X))   (pxmcmc/forward.py:63-64, measurements.py:221-230)
//          = mask / weight( SHT2^-1( k_l .* SHT0( SHT0^-1( f_lm ) ) ) ),  f_lm = sum_j c_j kappa_j W^j_lm.
// SHT0 o SHT0^-1 is the identity on band-limited coefficients (MW sampling theorem: exact quadrature), so the
// inverse transform at L of the synthesis and the forward transform of the measurement are never executed: the
// harmonic kernel is applied to f_lm directly while the spin-2 inverse GEMM stages its operand.  The adjoint
// collapses the same way (SHT0^-1 adjoint o SHT0 adjoint = identity).  Results equal the composed operators to
// round-off; 4 ring GEMMs and 4 DFT stages per forward + adjoint pair instead of 8 and 8.
#include "wav_plan.h"

#include <cmath>
#include <memory>

using namespace pxm;

void pxm::wl_release(WlAttach* w) {
  if (!w) return;
  deferred_free(w->d_wlk);
  free_tasks(&w->inv);
  free_tasks(&w->invadj);
  if (w->T2) release_tables(w->T2);
  rec_tables_destroy(w->rec2);
  deferred_free(w->d_twin);
  deferred_free(w->d_g2n);
  deferred_free(w->d_hn);
  deferred_free(w->d_gn);
  dft_group_destroy(&w->dft_group_n);
  free_tasks(&w->syn_fwd);
  free_tasks(&w->adj_fwdadj);
  delete w;
}

// Builds every resource of the attachment into *w, which the plan does not see yet: the plan is only read.
static int wl_build(const pxm_wav_plan_s* p, WlAttach* w) {
  int rc;
  std::vector<double> k((size_t)p->Rp, 0.0);
  for (int el = 2; el < p->L; ++el) k[el] = -std::sqrt(((el + 2.0) * (el - 1.0)) / ((el + 1.0) * el));
  if ((rc = dev_table(&w->d_wlk, k, "weak-lensing harmonic kernel k_l [Rp]"))) return rc;
  // one chain, two top scales of equal bandlimit outside the DFT group (L = 512, B = 2: scales 8 and 9): twin ring array
  if (p->pk == 2 && p->Cmax == 1)
    for (int s = 0; s + 1 < p->nsc && w->twin_s < 0; ++s)
      if (p->bl[s + 1] == p->bl[s] && p->T[s + 1] == p->T[s] && !wav_in_group(p, s) && !wav_in_group(p, s + 1)) w->twin_s = s;
  if (rec_wanted(p->L, 2, p->Cmax)) {
    // few chains: Wigner rows of the two spin-2 contractions by recursion (no 2 x 8 L^3-byte tables, no table build)
    w->ncol_g2 = 2 * p->Cmax;
    if (w->ncol_g2 != p->ncol) {
      const size_t nb = (size_t)(2 * p->L - 1) * p->Rp * w->ncol_g2 * sizeof(double);
      if ((rc = dev_alloc(&w->d_g2n, nb, "narrow spin-2 ring array"))) return rc;
      if ((rc = dev_zero(w->d_g2n, nb))) return rc;
    }
    if (w->twin_s >= 0) {  // narrow harmonic side (the weak-lensing lists of the twin path are this path's own)
      w->ncol_h = 2 * p->Cmax;
      const int64_t sz = (int64_t)(2 * p->L - 1) * p->Rp * w->ncol_h + p->ncol;  // (+ slack for the 16-column address model)
      if ((rc = dev_alloc(&w->d_hn, (size_t)(3 * sz) * sizeof(double), "narrow class buffers and H_L of the weak-lensing path"))) return rc;
      if ((rc = dev_zero(w->d_hn, (size_t)(3 * sz) * sizeof(double)))) return rc;
      w->offHAn = w->d_hn - p->ws;
      w->offHBn = w->offHAn + sz;
      w->offHLn = w->offHAn + 2 * sz;
    }
    if ((rc = rec_tables_create(p->L, 2, p->Cmax, p->Rp, w->ncol_h ? w->ncol_h : p->ncol, &w->rec2, w->ncol_g2))) { w->rec2 = nullptr; return rc; }
  } else {
    if ((rc = get_tables(p->L, 2, (1u << TAB_INV) | (1u << TAB_INV_ADJ), &w->T2))) { w->T2 = nullptr; return rc; }
    retain_tables(w->T2);
    std::vector<GemmTask> v;
    GemmFuse sum2;
    sum2.x2_base = p->offHB;
    append_gemm_tasks(*w->T2, TAB_INV, p->ncol, GemmSide{p->offHA, p->offG2, p->L, p->Rp, p->L, p->Rp, w->d_wlk, 0, sum2}, p->offS, p->ws, v);
    if ((rc = upload_tasks(v, false, &w->inv, {p->L}, p->ncol, p->ws, "weak-lensing spin-2 inverse"))) return rc;
    v.clear();
    GemmFuse rs;
    rs.rscale = w->d_wlk;
    append_gemm_tasks(*w->T2, TAB_INV_ADJ, p->ncol, GemmSide{p->offG2, p->offHL, p->L, p->Rp, p->L, p->Rp, nullptr, 0, rs}, p->offS, p->ws, v);
    if ((rc = upload_tasks(v, false, &w->invadj, {p->L}, p->ncol, p->ws, "weak-lensing spin-2 inverse-adjoint"))) return rc;
  }
  if (w->twin_s < 0) return 0;
  const int s = w->twin_s;
  w->ncol_t = 4;  // narrow: 4 doubles per row (the two slots)
  // (+ one row: the address model of the GEMM stage counts a row's width from a slab's first column, and slot 1 starts at 2)
  const int64_t n = (int64_t)(2 * p->bl[s] - 1) * round_up(p->bl[s], 16) * w->ncol_t + w->ncol_t;
  if ((rc = dev_alloc(&w->d_twin, (size_t)n * sizeof(double), "twin ring array of the two top scales"))) return rc;
  if ((rc = dev_zero(w->d_twin, (size_t)n * sizeof(double)))) return rc;
  w->offGT = w->d_twin - p->ws;
  if (w->ncol_h && p->dft_group.d && p->plain_group) {
    // the member scales of the DFT group on rows of 2 Cmax doubles as well: own arrays, own group descriptors
    w->ncol_gn = 2 * p->Cmax;
    w->offGn = p->offG;
    int64_t tot = 0;
    std::vector<int64_t> rel((size_t)p->nsc, 0);
    for (int k = 0; k < p->nsc; ++k)
      if (p->dft_group.member[k]) {
        rel[k] = tot;
        tot += ((int64_t)(2 * p->bl[k] - 1) * round_up(p->bl[k], 16) * w->ncol_gn + p->ncol + 15) / 16 * 16;  // (+ slack: 16-column address model)
      }
    if ((rc = dev_alloc(&w->d_gn, (size_t)tot * sizeof(double), "narrow ring arrays of the DFT group's scales"))) return rc;
    if ((rc = dev_zero(w->d_gn, (size_t)tot * sizeof(double)))) return rc;
    for (int k = 0; k < p->nsc; ++k)
      if (p->dft_group.member[k]) w->offGn[k] = (w->d_gn - p->ws) + rel[k];
    std::vector<const DftPlan*> dp;
    for (int k = 0; k < p->nsc; ++k) dp.push_back(&p->dft[k]);
    rc = dft_group_create(dp, w->offGn, p->coef_off, w->ncol_gn, p->ws, &w->dft_group_n);
    if (rc < 0) return rc;
    if (rc != 0 || w->dft_group_n.member != p->dft_group.member) dft_group_destroy(&w->dft_group_n);  // -> the plan's arrays
  }
  std::vector<GemmTask> vf, va;
  std::vector<char> shared;
  if ((rc = wav_packed_lists(p, 0, TAB_FWD, w, vf, &shared))) return rc;
  if ((rc = wav_packed_lists(p, 1, TAB_FWD_ADJ, w, va, nullptr))) return rc;
  if ((rc = upload_tasks(vf, true, &w->syn_fwd, p->bl, p->ncol, p->ws, "weak-lensing synthesis forward (twin scales)", p->el_lo_s, p->pk, shared))) return rc;
  return upload_tasks(va, true, &w->adj_fwdadj, p->bl, p->ncol, p->ws, "weak-lensing forward-adjoint (twin scales)", p->el_lo_s, p->pk, shared);
}

// the ring array of the spin-2 stage and its row stride (narrow only with the recursion stage: set together)
static inline double* wl_g2(pxm_wav_plan_t p) { return p->wl->d_g2n ? p->wl->d_g2n : p->ws + p->offG2; }
static inline int wl_g2_ncol(pxm_wav_plan_t p) { return p->wl->d_g2n ? p->wl->ncol_g2 : p->ncol; }

extern "C" {

int pxm_wav_wl_attach(pxm_wav_plan_t p, const int32_t* pix2data, const double* weight, int64_t ndata) {
  PXM_REQUIRE(p, "pxm_wav_wl_attach: null plan");
  PXM_REQUIRE(p->spin == 0, "pxm_wav_wl_attach: the weak-lensing kernel k_l maps a spin-0 field to the shear; this plan has spin " +
                                std::to_string(p->spin));
  PXM_REQUIRE(p->L >= 3, "pxm_wav_wl_attach: Bandlimit must be at least 3 for a spin-2 field");
  const int64_t P = (int64_t)p->L * (2 * p->L - 1);
  PXM_REQUIRE(ndata >= 0 && ndata <= P && (pix2data || ndata == P), "pxm_wav_wl_attach: bad mask description");
  if (!p->wl) {  // (a plan that has its attachment keeps it: a second call only re-points the mask)
    // owned by a guard until it is complete: an error leaves the plan as it was, and the call may be repeated
    std::unique_ptr<WlAttach, void (*)(WlAttach*)> w(new WlAttach(), wl_release);
    if (int rc = wl_build(p, w.get())) return rc;
    p->wl = w.release();
  }
  p->wl->gidx = pix2data;
  p->wl->gw = weight;
  p->wl->ndata = ndata;
  return 0;
}

int pxm_wav_wl_uses_recursion(pxm_wav_plan_t p) {
  PXM_REQUIRE(p, "pxm_wav_wl_uses_recursion: null plan");
  return p->wl && p->wl->rec2 ? p->wl->rec2->R * 16 + p->wl->rec2->NC : 0;
}

int pxm_wav_wl_forward(pxm_wav_plan_t p, const void* X, void* gamma, int C, pxm_stream_t stream) {
  int rc = plan_check(p, X, gamma, C, "pxm_wav_wl_forward");
  if (rc) return rc;
  PXM_REQUIRE(p->wl, "pxm_wav_wl_forward: call pxm_wav_wl_attach first");
  const WlAttach& w = *p->wl;
  PXM_REQUIRE(w.gidx || !w.gw, "pxm_wav_wl_forward: a covariance weight needs the pixel -> data map");
  hipStream_t st = (hipStream_t)stream;
  const bool twin = w.twin_s >= 0 && C == 1;
  if ((rc = wav_blocks_to_rings(p, X, C, st, twin))) return rc;
  if ((rc = wav_run(p, twin ? w.syn_fwd : p->syn_fwd, C, st))) return rc;  // f_lm (class buffers)
  const int64_t hA = w.ncol_h ? w.offHAn : p->offHA, hB = w.ncol_h ? w.offHBn : p->offHB;  // (narrow: Cmax == 1, twin lists)
  if (w.rec2) rc = rec_launch_e2r(*w.rec2, p->ws + hA, p->ws + hB, w.d_wlk, wl_g2(p), C, st, &p->prof);
  else rc = wav_run(p, w.inv, C, st);  // rings of the shear
  if (rc) return rc;
  PxOut out = image_out(p->L, gamma);
  if (w.gidx) out.chain_stride = w.ndata;
  out.gidx = w.gidx;
  out.gw = w.gw;
  return launch_ring2px(p->dftL, wl_g2(p), wl_g2_ncol(p), out, C, st);
}

// X_out = transform.inverse_adjoint(WeakLensing.adjoint(g)),  g = gamma  or, with data / invcov given, the
// residual invcov .* (gamma - data) of ForwardOperator._gradg_analysis (pxmcmc/forward.py:66-72)
int pxm_wav_wl_adjoint(pxm_wav_plan_t p, const void* gamma, const void* data, const void* invcov, int invcov_complex,
                       void* X_out, int C, pxm_stream_t stream) {
  int rc = plan_check(p, gamma, X_out, C, "pxm_wav_wl_adjoint");
  if (rc) return rc;
  PXM_REQUIRE(p->wl, "pxm_wav_wl_adjoint: call pxm_wav_wl_attach first");
  const WlAttach& w = *p->wl;
  PXM_REQUIRE((data == nullptr) == (invcov == nullptr), "pxm_wav_wl_adjoint: data and invcov come together");
  PXM_REQUIRE(w.gidx || !w.gw, "pxm_wav_wl_adjoint: a covariance weight needs the pixel -> data map");
  hipStream_t st = (hipStream_t)stream;
  PxIn in = image_in(p->L, gamma, data, invcov, invcov_complex);
  if (w.gidx) in.chain_stride = w.ndata;
  in.gidx = w.gidx;
  in.gw = w.gw;
  if ((rc = launch_px2ring(p->dftL, in, wl_g2(p), wl_g2_ncol(p), C, st))) return rc;
  if (w.rec2) rc = rec_launch_r2e(*w.rec2, wl_g2(p), w.d_wlk, p->ws + (w.ncol_h ? w.offHLn : p->offHL), C, st, &p->prof);
  else rc = wav_run(p, w.invadj, C, st);  // k_l B2^T -> H_L
  if (rc) return rc;
  const bool twin = w.twin_s >= 0 && C == 1;
  if ((rc = wav_run(p, twin ? w.adj_fwdadj : p->adj_fwdadj, C, st))) return rc;  // -> rings of every scale
  PxOut out;
  out.f = (double*)X_out;
  return wav_rings_to_blocks(p, out, C, st, twin);
}

}  // extern "C"
