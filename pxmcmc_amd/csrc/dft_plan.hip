// The phi-DFT stage as a plan of its own (one DftPlan and a status word: no ring tables, no task lists, no workspace) and
// the host report of the unit selection.  The entry points run the launches an SHT plan at the same bandlimit runs, on
// the caller's ring array; the _ex pair runs the same launches with the pixel side (residual, pixel -> data map, an image
// inside a longer chain) and the ring array's column count a weak-lensing or wavelet plan gives them.
#include "plan_common.h"

#include <memory>

using namespace pxm;

struct pxm_dft_plan_s {
  int L = 0, Cmax = 0, Cp = 0, ncol = 0, Rp = 0;
  DftPlan dft;
  unsigned* d_status = nullptr;  // device status word of this plan (pxm_dft_status)
};

extern "C" {

int pxm_host_dft_step_is_stock(unsigned fields, int mode, uint64_t chain0) {
  PXM_REQUIRE((fields & ~0xffu) == 0, "pxm_host_dft_step_is_stock: fields has eight bits");
  static const double some = 0;  // (the predicate asks only whether a pointer is set)
  static const uint64_t some_u = 0;
  static const int32_t some_i = 0;
  PxOut o;
  o.X = (fields & 1) ? &some : nullptr;
  o.T = (fields & 2) ? &some : nullptr;
  o.noise = (fields & 4) ? &some : nullptr;
  o.iter_dev = (fields & 8) ? &some_u : nullptr;
  o.rdata = (fields & 16) ? &some : nullptr;
  o.rinvcov = (fields & 32) ? &some : nullptr;
  o.gidx = (fields & 64) ? &some_i : nullptr;
  o.gw = (fields & 128) ? &some : nullptr;
  o.mode = mode;
  o.chain0 = chain0;
  return dft_step_is_stock(o) ? 1 : 0;
}

int pxm_host_dft_geometry(int L, int* out) {
  PXM_REQUIRE(out, "pxm_host_dft_geometry: null output");
  PXM_REQUIRE(L >= 1, "pxm_host_dft_geometry: need L >= 1");
  DftGeometry g;
  if (int rc = dft_geometry(L, &g)) return rc;
  out[0] = g.unit == DFT_RADIX2 ? 0 : (g.unit == DFT_PAIR ? 1 : 2);
  out[1] = g.M;
  out[2] = g.per_wg;
  out[3] = g.threads;
  out[4] = (int)g.lds;
  out[5] = g.exact ? 1 : 0;
  return 0;
}

int pxm_dft_plan_create(int L, int max_chains, pxm_dft_plan_t* plan) {
  PXM_REQUIRE(plan, "pxm_dft_plan_create: null plan pointer");
  PXM_REQUIRE(L >= 1, "pxm_dft_plan_create: Bandlimit must be greater than 0");
  PXM_REQUIRE(max_chains >= 1, "pxm_dft_plan_create: max_chains must be >= 1");
  PXM_REQUIRE(dry_run() || pxm_device_count() > 0, "pxm_dft_plan_create: no HIP device visible (the HIP path is the only path)");
  drain_deferred();
  std::unique_ptr<pxm_dft_plan_s, int (*)(pxm_dft_plan_t)> guard(new pxm_dft_plan_s(), pxm_dft_plan_destroy);
  pxm_dft_plan_s* p = guard.get();
  p->L = L;
  p->Cmax = max_chains;
  p->Cp = round_up(max_chains, 8);
  p->ncol = 2 * p->Cp;
  p->Rp = round_up(L, 16);
  int rc;
  if ((rc = make_dft_plan(L, &p->dft))) return rc;
  if ((rc = status_alloc(&p->d_status))) return rc;
  p->dft.d_status = p->d_status;
  *plan = guard.release();
  return 0;
}

int pxm_dft_plan_destroy(pxm_dft_plan_t p) {
  if (!p) return 0;
  free_dft_plan(&p->dft);
  deferred_free(p->d_status);
  delete p;
  drain_deferred();  // (a no-op while a stream capture is in progress: freed at the next safe point)
  return 0;
}

int pxm_dft_px2ring(pxm_dft_plan_t p, const void* f, void* G, int C, pxm_stream_t s) {
  if (int rc = plan_check(p, f, G, C, "pxm_dft_px2ring")) return rc;
  PXM_REQUIRE(((uintptr_t)G & 15) == 0, "pxm_dft_px2ring: the ring array must be 16-byte aligned");
  note_stream((hipStream_t)s);
  return launch_px2ring(p->dft, image_in(p->L, f), (double*)G, p->ncol, C, (hipStream_t)s);
}

int pxm_dft_ring2px(pxm_dft_plan_t p, const void* G, void* f, int C, pxm_stream_t s) {
  if (int rc = plan_check(p, G, f, C, "pxm_dft_ring2px")) return rc;
  PXM_REQUIRE(((uintptr_t)G & 15) == 0, "pxm_dft_ring2px: the ring array must be 16-byte aligned");
  note_stream((hipStream_t)s);
  return launch_ring2px(p->dft, (const double*)G, p->ncol, image_out(p->L, f), C, (hipStream_t)s);
}

}  // extern "C"

// The pixel side of the _ex entry points and the launch's column count: every refusal, before any launch.  to_rings: the
// call is pxm_dft_px2ring_ex (the residual is fused into the reads of that direction only).
static int px_side_check(pxm_dft_plan_t p, const void* G, int ncol, int C, int64_t chain_stride, int64_t ring0, const void* data,
                         const void* invcov, const int32_t* gidx, const double* gw, int64_t ndata, bool to_rings, const std::string& who) {
  PXM_REQUIRE(ncol == 2 || ncol == 4 || ncol == 6 || ncol == 8 || (ncol >= 16 && ncol % 16 == 0),
              who + ": ncol must be 2, 4, 6, 8 or a multiple of 16 (the ring arrays the plans make)");
  PXM_REQUIRE(C <= ncol / 2, who + ": C chains need ncol >= 2 C");
  PXM_REQUIRE(((uintptr_t)G & 15) == 0, who + ": the ring array must be 16-byte aligned");
  PXM_REQUIRE((data == nullptr) == (invcov == nullptr), who + ": data and invcov come together");
  PXM_REQUIRE(to_rings || !data, who + ": the residual (data, invcov) is fused into pixels -> rings only");
  PXM_REQUIRE(gidx || !gw, who + ": a weight gw needs the pixel -> data map gidx");
  const int64_t P = (int64_t)p->L * (2 * p->L - 1);
  if (gidx) {
    PXM_REQUIRE(ring0 == 0, who + ": a pixel -> data map needs ring0 == 0");
    PXM_REQUIRE(ndata >= 1, who + ": a pixel -> data map needs ndata >= 1");
    PXM_REQUIRE(chain_stride == ndata, who + ": with a pixel -> data map the chains are ndata apart");
  } else {
    PXM_REQUIRE(ring0 >= 0, who + ": ring0 must be >= 0");
    PXM_REQUIRE(ring0 <= chain_stride && P <= chain_stride - ring0, who + ": the image [ring0, ring0 + L (2L-1)) must lie inside a chain");
  }
  return 0;
}

extern "C" {

int pxm_dft_px2ring_ex(pxm_dft_plan_t p, const void* f, int64_t chain_stride, int64_t ring0, const void* data, const void* invcov,
                       int invcov_complex, const int32_t* gidx, const double* gw, int64_t ndata, void* G, int ncol, int C, pxm_stream_t s) {
  if (int rc = plan_check(p, f, G, C, "pxm_dft_px2ring_ex")) return rc;
  if (int rc = px_side_check(p, G, ncol, C, chain_stride, ring0, data, invcov, gidx, gw, ndata, true, "pxm_dft_px2ring_ex")) return rc;
  PxIn in = image_in(p->L, f, data, invcov, invcov_complex);
  in.chain_stride = chain_stride;
  in.ring0 = ring0;
  in.gidx = gidx;
  in.gw = gw;
  note_stream((hipStream_t)s);
  return launch_px2ring(p->dft, in, (double*)G, ncol, C, (hipStream_t)s);
}

int pxm_dft_ring2px_ex(pxm_dft_plan_t p, const void* G, int ncol, void* f, int64_t chain_stride, int64_t ring0, const void* data,
                       const void* invcov, int invcov_complex, const int32_t* gidx, const double* gw, int64_t ndata, int C, pxm_stream_t s) {
  (void)invcov_complex;
  if (int rc = plan_check(p, G, f, C, "pxm_dft_ring2px_ex")) return rc;
  if (int rc = px_side_check(p, G, ncol, C, chain_stride, ring0, data, invcov, gidx, gw, ndata, false, "pxm_dft_ring2px_ex")) return rc;
  PxOut out = image_out(p->L, f);
  out.chain_stride = chain_stride;
  out.ring0 = ring0;
  out.gidx = gidx;
  out.gw = gw;
  note_stream((hipStream_t)s);
  return launch_ring2px(p->dft, (const double*)G, ncol, out, C, (hipStream_t)s);
}

int pxm_dft_status(pxm_dft_plan_t p, int clear, pxm_stream_t stream) {
  PXM_REQUIRE(p, "pxm_dft_status: null plan");
  return status_read(p->d_status, (hipStream_t)stream, clear);
}

}  // extern "C"
