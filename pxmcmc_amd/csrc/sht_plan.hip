// SHT plan (tables + workspace + the four static task lists) and its C-ABI.
#include "plan_common.h"

#include <cmath>
#include <memory>

using namespace pxm;

struct pxm_sht_plan_s {
  int L = 0, spin = 0, Cmax = 0, Cp = 0, ncol = 0, Rp = 0;
  ShtTables* T = nullptr;
  RecTables* rec = nullptr;  // table-free ring stage of inverse / inverse_adjoint (sht_rec.hip), when the plan takes it
  DftPlan dft;
  double* ws = nullptr;  // [G | H | scratch]
  int64_t offG = 0, offH = 0, offS = 0;
  TaskList tl[4];
  unsigned* d_status = nullptr;  // device status word of this plan (pxm_sht_status)
};

extern "C" {

int pxm_sht_plan_create(int L, int spin, int max_chains, unsigned flags, pxm_sht_plan_t* plan) {
  (void)flags;
  PXM_REQUIRE(plan, "pxm_sht_plan_create: null plan pointer");
  PXM_REQUIRE(L >= 1, "pxm_sht_plan_create: Bandlimit must be greater than 0");
  PXM_REQUIRE(std::abs(spin) < L || L == 1, "pxm_sht_plan_create: |spin| must be < L");
  PXM_REQUIRE(max_chains >= 1, "pxm_sht_plan_create: max_chains must be >= 1");
  PXM_REQUIRE(dry_run() || pxm_device_count() > 0, "pxm_sht_plan_create: no HIP device visible (the HIP path is the only path)");
  drain_deferred();
  // (owned by a guard until it is complete: every error return below releases what was built so far)
  std::unique_ptr<pxm_sht_plan_s, int (*)(pxm_sht_plan_t)> guard(new pxm_sht_plan_s(), pxm_sht_plan_destroy);
  pxm_sht_plan_s* p = guard.get();
  p->L = L;
  p->spin = spin;
  p->Cmax = max_chains;
  p->Cp = round_up(max_chains, 8);
  p->ncol = 2 * p->Cp;
  p->Rp = round_up(L, 16);
  {  // a bandlimit the phi-DFT stage has no unit for is refused before the ring tables are built
    DftGeometry g;
    if (int rc = dft_geometry(L, &g)) return rc;
  }
  int rc = get_tables(L, spin, 0xF, &p->T);
  if (rc) { p->T = nullptr; return rc; }
  retain_tables(p->T);
  if ((rc = make_dft_plan(L, &p->dft))) return rc;
  if ((rc = status_alloc(&p->d_status))) return rc;
  p->dft.d_status = p->d_status;
  const int64_t sz = arr_size(L, p->ncol);
  p->offG = 0;
  p->offH = sz;
  p->offS = 2 * sz;
  const size_t bytes = (size_t)(2 * sz + (int64_t)p->Rp * p->ncol) * sizeof(double);
  if ((rc = dev_alloc(&p->ws, bytes, "SHT plan workspace"))) return rc;
  if ((rc = dev_zero(p->ws, bytes))) return rc;
  for (int k = 0; k < 4; ++k) {
    std::vector<GemmTask> v;
    const bool e2r = kind_el_to_ring(k);
    const GemmSide side{e2r ? p->offH : p->offG, e2r ? p->offG : p->offH, L, p->Rp, L, p->Rp, nullptr, 0, GemmFuse()};
    append_gemm_tasks(*p->T, k, p->ncol, side, p->offS, p->ws, v);
    if ((rc = upload_tasks(v, p->T->paired, &p->tl[k], {L}, p->ncol, p->ws, "SHT stage"))) return rc;
  }
  if (rec_wanted(L, spin, max_chains) && (rc = rec_tables_create(L, spin, max_chains, p->Rp, p->ncol, &p->rec))) return rc;
  *plan = guard.release();
  return 0;
}

int pxm_sht_plan_destroy(pxm_sht_plan_t p) {
  if (!p) return 0;
  free_dft_plan(&p->dft);
  deferred_free(p->ws);
  deferred_free(p->d_status);
  for (int k = 0; k < 4; ++k) free_tasks(&p->tl[k]);
  release_tables(p->T);
  rec_tables_destroy(p->rec);
  delete p;
  drain_deferred();  // (a no-op while a stream capture is in progress: freed at the next safe point)
  return 0;
}

static int sht_el_to_ring(pxm_sht_plan_t p, int kind, const void* flm, void* f, int C, hipStream_t st) {
  note_stream(st);
  int rc = launch_lm_to_mel((const double*)flm, p->ws + p->offH, p->L, p->Rp, p->ncol, C, p->spin, st);
  if (rc) return rc;
  if (p->rec && kind == TAB_INV) rc = rec_launch_e2r(*p->rec, p->ws + p->offH, nullptr, nullptr, p->ws + p->offG, C, st);
  else rc = run_tasks(p->tl[kind], p->ws, p->ws, p->ncol, C, st);
  if (rc) return rc;
  return launch_ring2px(p->dft, p->ws + p->offG, p->ncol, image_out(p->L, f), C, st);
}

static int sht_ring_to_el(pxm_sht_plan_t p, int kind, const void* f, void* flm, int C, hipStream_t st) {
  note_stream(st);
  int rc = launch_px2ring(p->dft, image_in(p->L, f), p->ws + p->offG, p->ncol, C, st);
  if (rc) return rc;
  if (p->rec && kind == TAB_INV_ADJ) rc = rec_launch_r2e(*p->rec, p->ws + p->offG, nullptr, p->ws + p->offH, C, st);
  else rc = run_tasks(p->tl[kind], p->ws, p->ws, p->ncol, C, st);
  if (rc) return rc;
  return launch_mel_to_lm(p->ws + p->offH, (double*)flm, p->L, p->Rp, p->ncol, C, p->spin, st);
}

int pxm_sht_inverse(pxm_sht_plan_t p, const void* flm, void* f, int C, pxm_stream_t s) {
  int rc = plan_check(p, flm, f, C, "pxm_sht_inverse");
  return rc ? rc : sht_el_to_ring(p, TAB_INV, flm, f, C, (hipStream_t)s);
}
int pxm_sht_forward_adjoint(pxm_sht_plan_t p, const void* flm, void* f, int C, pxm_stream_t s) {
  int rc = plan_check(p, flm, f, C, "pxm_sht_forward_adjoint");
  return rc ? rc : sht_el_to_ring(p, TAB_FWD_ADJ, flm, f, C, (hipStream_t)s);
}
int pxm_sht_forward(pxm_sht_plan_t p, const void* f, void* flm, int C, pxm_stream_t s) {
  int rc = plan_check(p, f, flm, C, "pxm_sht_forward");
  return rc ? rc : sht_ring_to_el(p, TAB_FWD, f, flm, C, (hipStream_t)s);
}
int pxm_sht_inverse_adjoint(pxm_sht_plan_t p, const void* f, void* flm, int C, pxm_stream_t s) {
  int rc = plan_check(p, f, flm, C, "pxm_sht_inverse_adjoint");
  return rc ? rc : sht_ring_to_el(p, TAB_INV_ADJ, f, flm, C, (hipStream_t)s);
}

int pxm_sht_status(pxm_sht_plan_t p, int clear, pxm_stream_t stream) {
  PXM_REQUIRE(p, "pxm_sht_status: null plan");
  return status_read(p->d_status, (hipStream_t)stream, clear);
}

int pxm_sht_uses_recursion(pxm_sht_plan_t p) {
  PXM_REQUIRE(p, "pxm_sht_uses_recursion: null plan");
  return p->rec ? p->rec->R * 16 + p->rec->NC : 0;
}

int pxm_rec_reduce_selftest(double* out128) {
  PXM_REQUIRE(out128, "pxm_rec_reduce_selftest: null output");
  PXM_REQUIRE(pxm_device_count() > 0, "pxm_rec_reduce_selftest: no HIP device visible");
  return rec_reduce_selftest(out128);
}

int64_t pxm_sht_table_bytes(pxm_sht_plan_t p, int op) {
  if (!p || op < 0 || op > 3) return -1;
  return (int64_t)p->T->bytes[op];
}

}  // extern "C"
