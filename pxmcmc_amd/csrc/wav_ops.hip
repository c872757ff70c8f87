// Wavelet plan: the transforms (synthesis / analysis and their adjoints) and the fused MYULA steps, as sequences of stages.
#include "wav_plan.h"

using namespace pxm;

// ---- coefficient blocks <-> rings of every scale -------------------------------------------------------------
// fork: side streams wait for everything already enqueued on the caller's stream
static int wav_fork(pxm_wav_plan_t p, hipStream_t st, bool used[pxm_wav_plan_s::NSIDE]) {
  for (int i = 0; i < pxm_wav_plan_s::NSIDE; ++i) used[i] = false;
  if (!p->ev_fork) return 0;
  PXM_HIP(hipEventRecord(p->ev_fork, st));
  for (int s = 0; s < p->nsc; ++s) {
    const int ln = p->lane_of[s];
    if (ln >= 0 && !used[ln]) {
      used[ln] = true;
      PXM_HIP(hipStreamWaitEvent(p->side[ln], p->ev_fork, 0));
    }
  }
  return 0;
}
// join: the caller's stream waits for every side stream that got work
static int wav_join(pxm_wav_plan_t p, hipStream_t st, const bool used[pxm_wav_plan_s::NSIDE]) {
  for (int i = 0; i < pxm_wav_plan_s::NSIDE; ++i)
    if (used[i]) {
      PXM_HIP(hipEventRecord(p->ev_join[i], p->side[i]));
      PXM_HIP(hipStreamWaitEvent(st, p->ev_join[i], 0));
    }
  return 0;
}
static inline hipStream_t wav_stream(pxm_wav_plan_t p, int s, hipStream_t st) { return p->lane_of[s] >= 0 ? p->side[p->lane_of[s]] : st; }
// side stream 0 (made to wait for the fork event if no scale had claimed it), or the caller's stream without side streams
static inline hipStream_t wav_group_stream(pxm_wav_plan_t p, hipStream_t st, bool used[pxm_wav_plan_s::NSIDE]) {
  if (!p->ev_fork || !p->side[0]) return st;
  if (!used[0]) {
    used[0] = true;
    (void)hipStreamWaitEvent(p->side[0], p->ev_fork, 0);
  }
  return p->side[0];
}

// The member scales of the plan's DFT group go in ONE grid; a scale outside the group (band-limits above 256: four-wave
// kernels) keeps its own launch, on the calling stream while the group runs on a side stream.
// twin (weak-lensing path, C == 1): scales twin_s and twin_s + 1 as the two "chains" of ONE launch on the twin array -- chain
// stride = the distance of their coefficient blocks -- and the member scales on the attachment's narrow arrays, if it has them
int pxm::wav_blocks_to_rings(pxm_wav_plan_s* p, const void* X, int C, hipStream_t st, bool twin) {
  const bool grp = p->dft_group.d && p->plain_group;
  const WlAttach* wl = twin ? p->wl : nullptr;
  PxIn in;
  in.f = (const double*)X;
  in.chain_stride = p->ncoefs;
  if (grp && p->dft_group.all) return dft_group_px2ring(p->dft_group, p->ws, p->ncol, in, C, st);  // no side streams at all
  bool used[pxm_wav_plan_s::NSIDE];
  int rc = wav_fork(p, st, used);
  if (rc) return rc;
  for (int s = p->nsc - 1; s >= 0; --s) {  // largest first
    if (wav_in_group(p, s)) continue;
    if (wl && s == wl->twin_s + 1) continue;  // rides with twin_s
    PxIn ins = in;  // (this scale's block of the coefficient vector)
    ins.ring0 = p->coef_off[s];
    if (wl && s == wl->twin_s) {
      ins.chain_stride = p->coef_off[s + 1] - p->coef_off[s];
      rc = launch_px2ring(p->dft[s], ins, p->ws + wl->offGT, wl->ncol_t, 2, grp ? st : wav_stream(p, s, st));
    } else {
      rc = launch_px2ring(p->dft[s], ins, p->ws + p->offG[s], p->ncol, C, grp ? st : wav_stream(p, s, st));
    }
    if (rc) return rc;
  }
  if (grp) {
    const bool ng = wl && wl->dft_group_n.d;  // the member scales' narrow arrays
    if ((rc = dft_group_px2ring(ng ? wl->dft_group_n : p->dft_group, p->ws, ng ? wl->ncol_gn : p->ncol, in, C, wav_group_stream(p, st, used)))) return rc;
  }
  return wav_join(p, st, used);
}

int pxm::wav_rings_to_blocks(pxm_wav_plan_s* p, PxOut proto, int C, hipStream_t st, bool twin) {
  const bool grp = p->dft_group.d && p->plain_group;
  const WlAttach* wl = twin ? p->wl : nullptr;
  proto.chain_stride = p->ncoefs;
  if (grp && p->dft_group.all) return dft_group_ring2px(p->dft_group, p->ws, p->ncol, proto, C, st);
  bool used[pxm_wav_plan_s::NSIDE];
  int rc = wav_fork(p, st, used);
  if (rc) return rc;
  for (int s = p->nsc - 1; s >= 0; --s) {
    if (wav_in_group(p, s)) continue;
    if (wl && s == wl->twin_s + 1) continue;
    PxOut out = proto;
    out.ring0 = p->coef_off[s];
    if (wl && s == wl->twin_s) {  // (plain output only: the two "chains" are two blocks of one coefficient vector)
      out.chain_stride = p->coef_off[s + 1] - p->coef_off[s];
      rc = launch_ring2px(p->dft[s], p->ws + wl->offGT, wl->ncol_t, out, 2, grp ? st : wav_stream(p, s, st));
    } else {
      rc = launch_ring2px(p->dft[s], p->ws + p->offG[s], p->ncol, out, C, grp ? st : wav_stream(p, s, st));
    }
    if (rc) return rc;
  }
  if (grp) {
    const bool ng = wl && wl->dft_group_n.d;
    if ((rc = dft_group_ring2px(ng ? wl->dft_group_n : p->dft_group, p->ws, ng ? wl->ncol_gn : p->ncol, proto, C, wav_group_stream(p, st, used)))) return rc;
  }
  return wav_join(p, st, used);
}

// G_s -> coefficient blocks (with out's epilogue) and, in the same kernels, the rings of the written blocks
// back into G_s.  Only when every scale has a fused kernel (wav_can_fuse_dft).
static bool wav_can_fuse_dft(pxm_wav_plan_t p) {
  for (int s = 0; s < p->nsc; ++s)
    if (!dft_can_fuse(p->dft[s])) return false;
  return true;
}

static int wav_rings_update_rings(pxm_wav_plan_t p, PxOut proto, int C, hipStream_t st) {
  proto.chain_stride = p->ncoefs;
  if (p->dft_group.d && p->dft_group.all)  // one grid for every scale, small scales first
    return dft_group_launch(p->dft_group, p->ws, p->ncol, proto, C, st, &p->prof);
  bool used[pxm_wav_plan_s::NSIDE];
  int rc = wav_fork(p, st, used);
  if (rc) return rc;
  // side-stream (small) scales are enqueued first: the full-size kernels fill every wave slot of the chip
  // (2 waves per SIMD by registers), so whatever is enqueued behind them only runs in their tail
  for (int pass = 0; pass < 2; ++pass)
    for (int s = p->nsc - 1; s >= 0; --s) {
      const bool side = p->lane_of[s] >= 0;
      if (side != (pass == 0)) continue;
      PxOut out = proto;
      out.ring0 = p->coef_off[s];
      if ((rc = launch_ring2px2ring(p->dft[s], p->ws + p->offG[s], p->ncol, out, C, wav_stream(p, s, st)))) return rc;
    }
  return wav_join(p, st, used);
}

// rings at L -> image ; image (or residual) -> rings at L
static int wav_rings_to_image(pxm_wav_plan_t p, void* f, int C, hipStream_t st) {
  return launch_ring2px(p->dftL, p->ws + p->offGL, p->ncol, image_out(p->L, f), C, st);
}
static int wav_image_to_rings(pxm_wav_plan_t p, const PxIn& in, int C, hipStream_t st) {
  return launch_px2ring(p->dftL, in, p->ws + p->offGL, p->ncol, C, st);
}

static int wav_synthesis_adjoint_impl(pxm_wav_plan_t p, const PxIn& in, const PxOut& out, int C, hipStream_t st) {
  int rc;
  if ((rc = wav_image_to_rings(p, in, C, st))) return rc;
  if ((rc = wav_run(p, p->adj_invadj, C, st))) return rc;
  if ((rc = wav_run(p, p->adj_fwdadj, C, st))) return rc;
  return wav_rings_to_blocks(p, out, C, st);
}

// The MYULA update of the three fused wavelet steps: checks that X_out does not alias X and the mode word (0, 1 or 2,
// | PXM_NOISE_F64) in the name of the entry point `fn`, and fills the update fields of the ring2px output `out`.
static int wav_update_out(pxm_wav_plan_t p, const char* fn, const void* X, const double* T, double T_scalar, double delta,
                          double lmda, const void* noise, int mode, uint64_t seed, uint64_t chain0, uint64_t iter, void* X_out,
                          PxOut* out) {
  PXM_REQUIRE(X != X_out, std::string(fn) + ": X_out must not alias X");
  PXM_REQUIRE((mode & ~PXM_NOISE_F64) >= 0 && (mode & ~PXM_NOISE_F64) <= 2, std::string(fn) + ": mode must be 0, 1 or 2 (| PXM_NOISE_F64)");
  PXM_REQUIRE(p->spin == 0 || (mode & ~PXM_NOISE_F64) != 2,
              std::string(fn) + ": mode 2 (two real chains per complex slot) needs a spin-0 plan: a spin-s image is never real");
  out->f = (double*)X_out;
  out->X = (const double*)X;
  out->T = T;
  out->T_scalar = T_scalar;
  out->delta = delta;
  out->lmda = lmda;
  out->noise = (const double*)noise;
  out->mode = mode & ~PXM_NOISE_F64;
  out->noise64 = (mode & PXM_NOISE_F64) ? 1 : 0;
  out->seed = seed;
  out->chain0 = chain0;
  out->iter = iter;
  out->iter_dev = p->iter_dev;
  return 0;
}

// coefficient blocks -> harmonic class buffers (what the Gram step reads; pxm_wav_ring_preds forms the rings on demand)
static int wav_coeffs_to_rings(pxm_wav_plan_t p, const void* X, int C, hipStream_t st) {
  int rc = wav_blocks_to_rings(p, X, C, st);
  return rc ? rc : wav_run(p, p->syn_fwd, C, st);
}

namespace pxm {
// HDc[(mi Rp + row) 2 + {0, 1}] = H_D[(mi Rp + row) ncol + {0, 1}]: chain 0 of the H-layout data term, without the
// chain padding.  The Gram epilogue reads its per-row constant from here: a wave's four rows are one 64-B segment,
// against four 128-B lines of the [m][row][chain] array for 16 useful bytes each (PMC: the Gram launch fetched 86.9 MB
// for 75.2 MB algorithmic, 1.16x, until round 3)
__global__ void k_pack_data_term(const double2* __restrict__ HD, double2* __restrict__ HDc, int64_t rows, int Cp) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) HDc[i] = HD[i * Cp];
}
}  // namespace pxm

extern "C" {

int pxm_wav_synthesis(pxm_wav_plan_t p, const void* X, void* f, int C, pxm_stream_t stream) {
  int rc = plan_check(p, X, f, C, "pxm_wav_synthesis");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = wav_blocks_to_rings(p, X, C, st))) return rc;
  if ((rc = wav_run(p, p->syn_fwd, C, st))) return rc;
  if ((rc = wav_run(p, p->syn_inv, C, st))) return rc;
  return wav_rings_to_image(p, f, C, st);
}

int pxm_wav_synthesis_adjoint(pxm_wav_plan_t p, const void* f, void* X, int C, pxm_stream_t stream) {
  int rc = plan_check(p, f, X, C, "pxm_wav_synthesis_adjoint");
  if (rc) return rc;
  PxOut out;
  out.f = (double*)X;
  return wav_synthesis_adjoint_impl(p, image_in(p->L, f), out, C, (hipStream_t)stream);
}

int pxm_wav_analysis(pxm_wav_plan_t p, const void* f, void* X, int C, pxm_stream_t stream) {
  int rc = plan_check(p, f, X, C, "pxm_wav_analysis");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = wav_image_to_rings(p, image_in(p->L, f), C, st))) return rc;
  if ((rc = wav_run(p, p->ana_fwd, C, st))) return rc;
  if ((rc = wav_run(p, p->ana_inv, C, st))) return rc;
  PxOut out;
  out.f = (double*)X;
  return wav_rings_to_blocks(p, out, C, st);
}

int pxm_wav_analysis_adjoint(pxm_wav_plan_t p, const void* X, void* f, int C, pxm_stream_t stream) {
  int rc = plan_check(p, X, f, C, "pxm_wav_analysis_adjoint");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = wav_blocks_to_rings(p, X, C, st))) return rc;
  if ((rc = wav_run(p, p->anadj_invadj, C, st))) return rc;
  if ((rc = wav_run(p, p->anadj_fwdadj, C, st))) return rc;
  return wav_rings_to_image(p, f, C, st);
}

int pxm_wav_gradg_step(pxm_wav_plan_t p, const void* X, const void* preds, const void* data, const void* invcov,
                       int invcov_complex, const double* T, double T_scalar, double delta, double lmda,
                       const void* noise, int mode, uint64_t seed, uint64_t chain0, uint64_t iter,
                       void* X_out, int C, pxm_stream_t stream) {
  int rc = plan_check(p, X, X_out, C, "pxm_wav_gradg_step");
  if (rc) return rc;
  PXM_REQUIRE(preds && data && invcov, "pxm_wav_gradg_step: null argument");
  PxOut out;
  if ((rc = wav_update_out(p, "pxm_wav_gradg_step", X, T, T_scalar, delta, lmda, noise, mode, seed, chain0, iter, X_out, &out))) return rc;
  return wav_synthesis_adjoint_impl(p, image_in(p->L, preds, data, invcov, invcov_complex), out, C, (hipStream_t)stream);
}

// Whole MYULA iteration for a DIAGONAL (per-pixel) inverse covariance (pxm_wav_gradg_step + pxm_wav_synthesis
// fused).  The rings of the residual invcov .* (preds - data) are carried inside the plan between calls:
//   pxm_wav_image_init : residual rings <- DFT(invcov .* (preds - data))            (start of a run)
//   pxm_wav_image_step : X_out = MYULA update of X; preds_out = forward(X_out); residual rings of preds_out.
// Per step: inverse-adjoint + forward-adjoint GEMMs, the grouped rings -> X' -> rings launch of every scale,
// forward + inverse GEMMs and ONE rings -> image -> residual -> rings kernel at L.
int pxm_wav_image_init(pxm_wav_plan_t p, const void* preds, const void* data, const void* invcov, int invcov_complex,
                       int C, pxm_stream_t stream) {
  int rc = plan_check(p, preds, preds, C, "pxm_wav_image_init");
  if (rc) return rc;
  PXM_REQUIRE(data && invcov, "pxm_wav_image_init: null argument");
  return wav_image_to_rings(p, image_in(p->L, preds, data, invcov, invcov_complex), C, (hipStream_t)stream);
}

int pxm_wav_image_step(pxm_wav_plan_t p, const void* X, const void* data, const void* invcov, int invcov_complex,
                       const double* T, double T_scalar, double delta, double lmda, const void* noise, int mode,
                       uint64_t seed, uint64_t chain0, uint64_t iter, void* X_out, void* preds_out, int C,
                       pxm_stream_t stream) {
  int rc = plan_check(p, X, X_out, C, "pxm_wav_image_step");
  if (rc) return rc;
  PXM_REQUIRE(data && invcov && preds_out, "pxm_wav_image_step: null argument");
  PxOut out;
  if ((rc = wav_update_out(p, "pxm_wav_image_step", X, T, T_scalar, delta, lmda, noise, mode, seed, chain0, iter, X_out, &out))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = wav_run(p, p->adj_invadj, C, st))) return rc;  // residual rings -> H_L
  if ((rc = wav_run(p, p->adj_fwdadj, C, st))) return rc;  // -> rings of every scale
  if (wav_can_fuse_dft(p)) {
    if ((rc = wav_rings_update_rings(p, out, C, st))) return rc;  // X' and its rings
  } else {
    if ((rc = wav_rings_to_blocks(p, out, C, st))) return rc;
    if ((rc = wav_blocks_to_rings(p, X_out, C, st))) return rc;
  }
  if ((rc = wav_run(p, p->syn_fwd, C, st))) return rc;
  if ((rc = wav_run(p, p->syn_inv, C, st))) return rc;  // rings of S X'
  if (dft_can_fuse(p->dftL)) {  // rings -> preds -> residual -> rings, one kernel (only the pair unit implements the residual epilogue)
    PxOut po = image_out(p->L, preds_out);
    po.rdata = (const double*)data;
    po.rinvcov = (const double*)invcov;
    po.rinvcov_complex = invcov_complex;
    return launch_ring2px2ring(p->dftL, p->ws + p->offGL, p->ncol, po, C, st);
  }
  if ((rc = wav_rings_to_image(p, preds_out, C, st))) return rc;
  return pxm_wav_image_init(p, preds_out, data, invcov, invcov_complex, C, stream);
}

// ---- ring-space MYULA step (identity measurement, uniform inverse covariance) -------------------------
int pxm_wav_ring_set_data(pxm_wav_plan_t p, const void* data, pxm_stream_t stream) {
  PXM_REQUIRE(p && data, "pxm_wav_ring_set_data: null argument");
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = wav_make_gram_lists(p))) return rc;
  if ((rc = launch_px2ring(p->dftL, image_in(p->L, data), p->ws + p->offGD, p->ncol, 1, st))) return rc;  // chain 0 of G_D
  if ((rc = wav_run(p, p->adj_invadj_D, 1, st))) return rc;  // H_D = B^T DFT(data)
  const int64_t rows = (int64_t)(2 * p->L - 1) * p->Rp;
  hipLaunchKernelGGL(k_pack_data_term, dim3((unsigned)std::min<int64_t>((rows + 255) / 256, 2048)), dim3(256), 0, st,
                     reinterpret_cast<const double2*>(p->ws + p->offHD), reinterpret_cast<double2*>(p->ws + p->offHDc), rows,
                     p->ncol / 2);
  PXM_HIP(hipGetLastError());
  p->have_data_rings = true;
  return 0;
}

int pxm_wav_ring_init(pxm_wav_plan_t p, const void* X, int C, pxm_stream_t stream) {
  int rc = plan_check(p, X, X, C, "pxm_wav_ring_init");
  return rc ? rc : wav_coeffs_to_rings(p, X, C, (hipStream_t)stream);
}

int pxm_wav_ring_preds(pxm_wav_plan_t p, void* preds, int C, pxm_stream_t stream) {
  int rc = plan_check(p, preds, preds, C, "pxm_wav_ring_preds");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = wav_run(p, p->syn_inv, C, st))) return rc;  // rings on demand
  return wav_rings_to_image(p, preds, C, st);
}

int pxm_wav_ring_step(pxm_wav_plan_t p, const void* X, double w_re, double w_im, const double* T, double T_scalar,
                      double delta, double lmda, const void* noise, int mode, uint64_t seed, uint64_t chain0,
                      uint64_t iter, void* X_out, int C, pxm_stream_t stream) {
  int rc = plan_check(p, X, X_out, C, "pxm_wav_ring_step");
  if (rc) return rc;
  PXM_REQUIRE(p->have_data_rings, "pxm_wav_ring_step: call pxm_wav_ring_set_data first");
  PxOut out;
  if ((rc = wav_update_out(p, "pxm_wav_ring_step", X, T, T_scalar, delta, lmda, noise, mode, seed, chain0, iter, X_out, &out))) return rc;
  hipStream_t st = (hipStream_t)stream;
  // H' = w ((2L-1) B^T B H - B^T DFT(data)): inverse transform, ring residual and inverse-adjoint in one GEMM
  GemmAffine aff;
  aff.on = 1;
  aff.ns = (double)(2 * p->L - 1);
  aff.wr = w_re;
  aff.wi = w_im;
  aff.bump = p->iter_dev;  // the step's iteration number = counter after this bump
  if ((rc = wav_run(p, p->gram, C, st, aff))) return rc;
  if ((rc = wav_run(p, p->adj_fwdadj, C, st))) return rc;
  // rings -> X_out -> rings of X_out in one kernel per scale where every scale can, then the per-scale forward GEMMs
  if (wav_can_fuse_dft(p)) {
    if ((rc = wav_rings_update_rings(p, out, C, st))) return rc;
    return wav_run(p, p->syn_fwd, C, st);
  }
  if ((rc = wav_rings_to_blocks(p, out, C, st))) return rc;
  return wav_coeffs_to_rings(p, X_out, C, st);
}

}  // extern "C"
