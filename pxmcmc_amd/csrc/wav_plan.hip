// Wavelet plan: tables, workspace and static task lists; create / destroy and the plan's housekeeping entry points.
#include "wav_plan.h"
#include "mem_policy.h"

#include <cmath>
#include <memory>
#include <mutex>

using namespace pxm;

// the four per-scale ring stages as GemmSide descriptors (which: 0 synthesis forward, 1 its adjoint, 2 analysis inverse,
// 3 its adjoint)
struct SideOverride {  // arrays of a weak-lensing attachment that replace the plan's (offsets relative to ws; ncol 0 = the plan's)
  const int64_t* g = nullptr;   // ring array of this scale (a separate allocation: its offset can have either sign)
  int g_ncol = 0;
  const WlAttach* h = nullptr;  // narrow harmonic side: class buffers / H_L of this attachment (offHAn ...)
};
static GemmSide wav_side(const pxm_wav_plan_s* p, int s, int which, const SideOverride& ov = SideOverride()) {
  const int L = p->L, b = p->bl[s], Rb = round_up(b, 16);
  const int64_t G = ov.g ? *ov.g : p->offG[s];
  GemmSide g;
  // (row strides of replaced arrays: the ring side is x for the forward kinds, y for the adjoint ones; the harmonic side the other)
  const bool ring_is_x = which == 0 || which == 3;
  if (ov.g && ov.g_ncol) (ring_is_x ? g.x_ncol : g.y_ncol) = ov.g_ncol;
  if (ov.h) (ring_is_x ? g.y_ncol : g.x_ncol) = ov.h->ncol_h;
  g.el_lo = p->el_lo_s[s];
  g.fuse = GemmFuse();
  g.kscale = nullptr;
  const int cls = (s == 0) ? 1 : ((s - 1) & 1);
  const int64_t hcls = ov.h ? (cls ? ov.h->offHBn : ov.h->offHAn) : (cls ? p->offHB : p->offHA);
  const int64_t hl = ov.h ? ov.h->offHLn : p->offHL;
  switch (which) {
    case 0:  // synthesis: G_s --A_s--> c_s kappa_s(l) * (...) written straight into the class buffer in L layout
      g.x_base = G; g.x_L = b; g.x_Rp = Rb;
      g.fuse.row_lo = p->el_lo_s[s]; g.fuse.row_hi = b;
      g.y_base = hcls; g.y_L = L; g.y_Rp = p->Rp; g.fuse.rscale = p->d_kc_syn + (size_t)s * p->Rp;
      break;
    case 1:  // synthesis adjoint: H_L (scaled by c_s kappa_s per el) --A_s^T--> G_s
      g.x_base = hl; g.x_L = L; g.x_Rp = p->Rp; g.y_base = G; g.y_L = b; g.y_Rp = Rb;
      g.kscale = p->d_kc_syn + (size_t)s * p->Rp;
      break;
    case 2:  // analysis: H_L (scaled by c_a kappa_s) --B_s--> G_s
      g.x_base = hl; g.x_L = L; g.x_Rp = p->Rp; g.y_base = G; g.y_L = b; g.y_Rp = Rb;
      g.kscale = p->d_kc_ana + (size_t)s * p->Rp;
      break;
    default:  // analysis adjoint: G_s --B_s^T--> class buffer
      g.x_base = G; g.x_L = b; g.x_Rp = Rb;
      g.fuse.row_lo = p->el_lo_s[s]; g.fuse.row_hi = b;
      g.y_base = hcls; g.y_L = L; g.y_Rp = p->Rp; g.fuse.rscale = p->d_kc_ana + (size_t)s * p->Rp;
      break;
  }
  return g;
}

int pxm::wav_packed_lists(const pxm_wav_plan_s* p, int which, int kind, const WlAttach* wl, std::vector<GemmTask>& out,
                          std::vector<char>* shared) {
  if (shared) shared->assign(p->nsc, 0);
  const bool narrow_g = wl && wl->dft_group_n.d;  // narrow ring arrays of the DFT group's member scales
  const int64_t ga = wl ? wl->offGT : 0, gb = ga + 2;
  for (int s = 0; s < p->nsc; ++s) {
    const bool pair = s + 1 < p->nsc && p->bl[s + 1] == p->bl[s] && p->T[s + 1] == p->T[s];
    SideOverride oa, ob;
    oa.h = ob.h = (wl && wl->ncol_h) ? wl : nullptr;
    if (wl && s == wl->twin_s) {
      oa.g = &ga;
      ob.g = &gb;
      oa.g_ncol = ob.g_ncol = wl->ncol_t;
    } else if (narrow_g) {
      if (wl->dft_group_n.member[s]) oa.g = &wl->offGn[s], oa.g_ncol = wl->ncol_gn;
      if (pair && wl->dft_group_n.member[s + 1]) ob.g = &wl->offGn[s + 1], ob.g_ncol = wl->ncol_gn;
    }
    const GemmSide a = wav_side(p, s, which, oa);
    if (pair) {
      const GemmSide b = wav_side(p, s + 1, which, ob);
      // a packed pair is ONE task with one pair of row strides (GemmTask::x_ncol / y_ncol, taken from side a): a pair of which
      // only one scale sits on a narrow array must not be packed
      PXM_REQUIRE((a.x_ncol ? a.x_ncol : p->ncol) == (b.x_ncol ? b.x_ncol : p->ncol) &&
                      (a.y_ncol ? a.y_ncol : p->ncol) == (b.y_ncol ? b.y_ncol : p->ncol),
                  "wav_packed_lists: the two scales of a packed pair have arrays of different row strides");
      append_gemm_tasks_packed(*p->T[s], kind, p->ncol, a, &b, p->offS, p->ws, out);
      if (shared) (*shared)[s + 1] = 1;
      ++s;
    } else {
      append_gemm_tasks_packed(*p->T[s], kind, p->ncol, a, nullptr, p->offS, p->ws, out);
    }
  }
  return 0;
}

// one L-level stage (spin 0 pairs +-m on one table, spin s != 0 stores every m: unpaired lists, one slab per task)
static int wav_level_list(pxm_wav_plan_s* p, int kind, int64_t x, int64_t y, const GemmFuse& fuse, TaskList* tl, const char* name) {
  std::vector<GemmTask> v;
  append_gemm_tasks(*p->TL, kind, p->ncol, GemmSide{x, y, p->L, p->Rp, p->L, p->Rp, nullptr, 0, fuse}, p->offS, p->ws, v);
  return upload_tasks(v, p->TL->paired, tl, {p->L}, p->ncol, p->ws, name);
}

// the one implementation behind pxm_wav_plan_create (spin 0) and pxm_wav_plan_create_spin; `who` names the entry point
static int wav_plan_create_impl(const char* who, int L, double B, int J_min, int spin, int max_chains, pxm_wav_plan_t* plan) {
  const std::string fn(who);
  PXM_REQUIRE(plan, fn + ": null plan pointer");
  PXM_REQUIRE(L >= 1 && B > 1.0 && J_min >= 0, fn + ": bad (L, B, J_min)");
  PXM_REQUIRE(std::abs(spin) < L, fn + ": |spin| must be < L");
  PXM_REQUIRE(max_chains >= 1, fn + ": max_chains must be >= 1");
  PXM_REQUIRE(dry_run() || pxm_device_count() > 0, fn + ": no HIP device visible (the HIP path is the only path)");
  drain_deferred();
  // (owned by a guard until it is complete: every error return below releases what was built so far)
  std::unique_ptr<pxm_wav_plan_s, int (*)(pxm_wav_plan_t)> guard(new pxm_wav_plan_s(), pxm_wav_plan_destroy);
  pxm_wav_plan_s* p = guard.get();
  p->L = L;
  p->spin = spin;
  p->B = B;
  p->J_min = J_min;
  p->J_max = j_max(L, B);
  p->Cmax = max_chains;
  p->Cp = round_up(max_chains, 8);
  p->ncol = 2 * p->Cp;
  p->Rp = round_up(L, 16);
  p->bl = wav_bandlimits(L, B, J_min);
  p->nsc = (int)p->bl.size();
  PXM_REQUIRE(p->nsc <= WAV_MAX_SCALES, fn + ": more than 39 wavelet scales are not supported");
  int64_t off = 0;
  for (int b : p->bl) {
    p->coef_off.push_back(off);
    off += (int64_t)b * (2 * b - 1);
  }
  p->ncoefs = off;
  int rc;
  {  // a bandlimit the phi-DFT stage has no unit for is refused before any table is built (no scale has longer rings)
    DftGeometry g;
    if ((rc = dft_geometry(L, &g))) return rc;
  }
  if ((rc = status_alloc(&p->d_status))) return rc;
  p->mem_policy = mem_policy_from_env();  // (read again, to the same effect, by dft_group_create below)
  // tables: every scale needs the forward pair (synthesis: FWD, its adjoint: FWD_ADJ) and, for the
  // analysis setting, the inverse pair at its own bandlimit (spin 0); L needs all four, at the plan's spin.
  p->T.resize(p->nsc);
  p->dft.resize(p->nsc);
  for (int s = 0; s < p->nsc; ++s) {
    if ((rc = get_tables(p->bl[s], 0, 0xF, &p->T[s]))) return rc;
    wav_hold(p, p->T[s]);
    if ((rc = make_dft_plan(p->bl[s], &p->dft[s]))) return rc;
    p->dft[s].d_status = p->d_status;  // (before the DFT group is built: its entries carry a copy)
  }
  if ((rc = get_tables(L, spin, 0xF, &p->TL))) return rc;
  wav_hold(p, p->TL);
  if ((rc = make_dft_plan(L, &p->dftL))) return rc;
  p->dftL.d_status = p->d_status;
  // workspace
  int64_t w = 0;
  p->offGL = w; w += arr_size(L, p->ncol);
  p->offHL = w; w += arr_size(L, p->ncol);
  p->offGD = w; w += arr_size(L, p->ncol);
  p->offHD = w; w += arr_size(L, p->ncol);
  p->offHDc = w; w += (int64_t)(2 * L - 1) * p->Rp * 2;
  p->offHA = w; w += arr_size(L, p->ncol);
  p->offHB = w; w += arr_size(L, p->ncol);
  p->plain_group = !getenv("PXM_NO_PLAIN_DFT_GROUP");
  for (int s = 0; s < p->nsc; ++s) {
    p->offG.push_back(w); w += arr_size(p->bl[s], p->ncol);
  }
  p->offG2 = w; w += arr_size(L, p->ncol);  // (spin-2 rings of the weak-lensing attachment: 1/8 or so of the workspace)
  p->offS = w; w += (int64_t)p->Rp * p->ncol;
  if ((rc = dev_alloc(&p->ws, (size_t)w * sizeof(double), "wavelet plan workspace"))) return rc;
  if ((rc = dev_zero(p->ws, (size_t)w * sizeof(double)))) return rc;
  // wavelet kernels: synthesis f_lm = kappa0 W^phi + sqrt(2pi) sum_j kappa_j W^j; analysis W^j = kappa_j f / sqrt(2pi)
  // (spin s: rows el < |s| zero -- a spin-s field has no harmonics there)
  std::vector<double> k0, kap;
  tiling_axisym(L, B, J_min, k0, kap);
  std::vector<double> kc_syn((size_t)p->nsc * p->Rp, 0.0), kc_ana((size_t)p->nsc * p->Rp, 0.0);
  const double cs = std::sqrt(2.0 * M_PI), ca = 1.0 / std::sqrt(2.0 * M_PI);
  for (int s = 0; s < p->nsc; ++s)
    for (int el = std::abs(spin); el < p->bl[s]; ++el) {
      const double k = (s == 0) ? k0[el] : kap[(size_t)(J_min + s - 1) * L + el];
      kc_syn[(size_t)s * p->Rp + el] = (s == 0) ? k : cs * k;
      kc_ana[(size_t)s * p->Rp + el] = (s == 0) ? k : ca * k;
    }
  if ((rc = dev_table(&p->d_kc_syn, kc_syn, "synthesis kernel rows c kappa [nsc][Rp]"))) return rc;
  if ((rc = dev_table(&p->d_kc_ana, kc_ana, "analysis kernel rows c kappa [nsc][Rp]"))) return rc;
  // support cut per scale: first degree with a non-zero kernel (compact support of kappa_j).  The rows / contraction
  // steps below it are skipped, and it is the row mask of the fused combine (class buffers are shared by scales with
  // disjoint supports).
  std::vector<int>& el_lo = p->el_lo_s;
  el_lo.assign(p->nsc, 0);
  for (int s = 0; s < p->nsc; ++s)
    while (el_lo[s] < p->bl[s] && kc_syn[(size_t)s * p->Rp + el_lo[s]] == 0.0) ++el_lo[s];
  // task lists of the four per-scale stages
  std::vector<GemmTask> v_syn_fwd, v_adj_fwdadj, v_ana_inv, v_anadj_invadj;
  const int kinds[4] = {TAB_FWD, TAB_FWD_ADJ, TAB_INV, TAB_INV_ADJ};
  std::vector<GemmTask>* lists[4] = {&v_syn_fwd, &v_adj_fwdadj, &v_ana_inv, &v_anadj_invadj};
  for (int s = 0; s < p->nsc; ++s) {
    for (int w = 0; w < 4; ++w) {
      append_gemm_tasks(*p->T[s], kinds[w], p->ncol, wav_side(p, s, w), p->offS, p->ws, *lists[w]);
    }
    p->table_bytes[0] += p->T[s]->bytes[TAB_FWD];
    p->table_bytes[1] += p->T[s]->bytes[TAB_FWD_ADJ];
  }
  p->table_bytes[0] += p->TL->bytes[TAB_INV];
  p->table_bytes[1] += p->TL->bytes[TAB_INV_ADJ];
  // Few-chain plans (<= 2 chains): the forward / forward-adjoint group launches in PACKED form -- the 2 C live columns of
  // every slab side by side in one MFMA column tile, and scales of equal bandlimit (the two L-band-limited ones) streaming
  // their table in one pass.
  const int pk = p->pk = max_chains <= 2 ? 2 * max_chains : 0;
  std::vector<char> shared(p->nsc, 0);
  if (pk) {
    v_syn_fwd.clear();
    v_adj_fwdadj.clear();
    if ((rc = wav_packed_lists(p, 0, TAB_FWD, nullptr, v_syn_fwd, &shared))) return rc;
    if ((rc = wav_packed_lists(p, 1, TAB_FWD_ADJ, nullptr, v_adj_fwdadj, nullptr))) return rc;
  }
  if ((rc = upload_tasks(v_syn_fwd, true, &p->syn_fwd, p->bl, p->ncol, p->ws, "synthesis forward (all scales)", el_lo, pk, shared))) return rc;
  if ((rc = upload_tasks(v_adj_fwdadj, true, &p->adj_fwdadj, p->bl, p->ncol, p->ws, "synthesis-adjoint forward-adjoint (all scales)", el_lo, pk, shared))) return rc;
  if ((rc = upload_tasks(v_ana_inv, true, &p->ana_inv, p->bl, p->ncol, p->ws, "analysis inverse (all scales)", el_lo))) return rc;
  if ((rc = upload_tasks(v_anadj_invadj, true, &p->anadj_invadj, p->bl, p->ncol, p->ws, "analysis-adjoint inverse-adjoint (all scales)", el_lo))) return rc;
  // the L-level stages
  GemmFuse sum2;
  sum2.x2_base = p->offHB;
  if ((rc = wav_level_list(p, TAB_INV, p->offHA, p->offGL, sum2, &p->syn_inv, "synthesis inverse at L"))) return rc;
  if ((rc = wav_level_list(p, TAB_INV_ADJ, p->offGL, p->offHL, GemmFuse(), &p->adj_invadj, "inverse-adjoint at L"))) return rc;
  if ((rc = wav_level_list(p, TAB_FWD, p->offGL, p->offHL, GemmFuse(), &p->ana_fwd, "analysis forward at L"))) return rc;
  if ((rc = wav_level_list(p, TAB_FWD_ADJ, p->offHA, p->offGL, sum2, &p->anadj_fwdadj, "analysis-adjoint forward-adjoint at L"))) return rc;
  // scales at the full bandlimit stay on the caller's stream; the rest are dealt over the side streams
  p->lane_of.assign(p->nsc, -1);
  SidePool* sp = nullptr;
  if ((rc = side_pool(&sp))) return rc;
  for (int i = 0; i < p->nside; ++i) {  // borrowed from the per-device pool, never destroyed
    p->side[i] = sp->side[i];
    p->ev_join[i] = sp->ev_join[i];
  }
  p->ev_fork = sp->ev_fork;
  int k = 0;
  for (int s = p->nsc - 1; s >= 0; --s)
    if (p->bl[s] < L) p->lane_of[s] = (k++) % p->nside;
  std::vector<const DftPlan*> dp;
  for (int s = 0; s < p->nsc; ++s) dp.push_back(&p->dft[s]);
  if ((rc = dft_group_create(dp, p->offG, p->coef_off, p->ncol, p->ws, &p->dft_group)) < 0) return rc;  // (1: no group -> per-scale launches)
  *plan = guard.release();
  return 0;
}

int pxm::wav_make_gram_lists(pxm_wav_plan_s* p) {
  if (p->gram.d) return 0;
  int rc;
  // spin 0 and Rp % 32 == 0: the Gram table without its structurally zero half, order 0 included (sht_tables.h:
  // TAB_GRAM_SPLIT0).  The cross-check and A/B switches: PXM_GRAM_SPLIT=1 keeps order 0 dense (TAB_GRAM_SPLIT),
  // PXM_GRAM_SPLIT=0 keeps the dense list
  const char* split_env = getenv("PXM_GRAM_SPLIT");
  const int split = split_env ? atoi(split_env) : 2;
  const int kind = (!gram_can_split(*p->TL) || split == 0) ? TAB_GRAM : (split == 1 ? TAB_GRAM_SPLIT : TAB_GRAM_SPLIT0);
  if ((rc = get_tables(p->L, p->spin, 1u << kind, &p->TL))) return rc;
  wav_hold(p, p->TL);
  std::vector<GemmTask> v;
  GemmFuse fz;
  fz.x2_base = p->offHB;
  fz.hd_base = p->offHDc;
  fz.hd_stride = 2;
  append_gemm_tasks(*p->TL, kind, p->ncol, GemmSide{p->offHA, p->offHL, p->L, p->Rp, p->L, p->Rp, nullptr, 0, fz}, p->offS, p->ws, v);
  if ((rc = upload_tasks(v, p->TL->paired, &p->gram, {p->L}, p->ncol, p->ws, "Gram step"))) return rc;
  tasklist_set_gram(&p->gram, *p->TL, kind);
  return wav_level_list(p, TAB_INV_ADJ, p->offGD, p->offHD, GemmFuse(), &p->adj_invadj_D, "inverse-adjoint of the data rings");
}

namespace pxm {
__global__ void k_iter_add(uint64_t* c, uint64_t inc) { *c += inc; }

__global__ void k_count_nonfinite(const double* __restrict__ x, int64_t n, unsigned long long* cnt) {
  unsigned long long c = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (!isfinite(x[i])) ++c;
  if (c) atomicAdd(cnt, c);
}
}  // namespace pxm

extern "C" {

int pxm_wav_plan_create(int L, double B, int J_min, int max_chains, unsigned flags, pxm_wav_plan_t* plan) {
  (void)flags;
  return wav_plan_create_impl("pxm_wav_plan_create", L, B, J_min, 0, max_chains, plan);
}

int pxm_wav_plan_create_spin(int L, double B, int J_min, int spin, int max_chains, unsigned flags, pxm_wav_plan_t* plan) {
  (void)flags;
  return wav_plan_create_impl("pxm_wav_plan_create_spin", L, B, J_min, spin, max_chains, plan);
}

int pxm_wav_plan_destroy(pxm_wav_plan_t p) {
  if (!p) return 0;
  // Nothing is freed here directly: device memory and events go to the graveyard, which is emptied at once unless
  // a stream capture is in progress (the garbage collector may run this in the middle of one).
  dft_group_destroy(&p->dft_group);
  for (auto& d : p->dft) free_dft_plan(&d);
  free_dft_plan(&p->dftL);
  deferred_free(p->ws);
  deferred_free(p->d_kc_syn);
  deferred_free(p->d_kc_ana);
  deferred_free(p->d_status);
  // (side streams / events belong to the per-device pool)
  TaskList* tls[] = {&p->syn_fwd, &p->syn_inv, &p->adj_invadj, &p->adj_fwdadj, &p->gram, &p->adj_invadj_D,
                     &p->ana_fwd, &p->ana_inv, &p->anadj_invadj, &p->anadj_fwdadj};
  for (TaskList* t : tls) free_tasks(t);
  profiler_release(&p->prof);
  for (ShtTables* T : p->held) release_tables(T);
  wl_release(p->wl);
  delete p;
  drain_deferred();
  return 0;
}

int pxm_wav_set_iter_counter(pxm_wav_plan_t p, uint64_t* counter_dev) {
  PXM_REQUIRE(p, "pxm_wav_set_iter_counter: null plan");
  // one live counter per plan: a second stepping engine on the same plan must not silently redirect the
  // Philox iteration number of the first (graphs captured earlier keep the pointer they were captured with)
  PXM_REQUIRE(!counter_dev || !p->iter_dev || p->iter_dev == counter_dev,
              "pxm_wav_set_iter_counter: this plan already has a live iteration counter (one stepping engine per plan "
              "at a time; release the first with pxm_wav_release_iter_counter)");
  p->iter_dev = counter_dev;
  return 0;
}

int pxm_wav_release_iter_counter(pxm_wav_plan_t p, const uint64_t* counter_dev) {
  PXM_REQUIRE(p, "pxm_wav_release_iter_counter: null plan");
  if (p->iter_dev == counter_dev) p->iter_dev = nullptr;  // somebody else's counter stays registered
  return 0;
}

int pxm_wav_iter_counter_add(pxm_wav_plan_t p, uint64_t inc, pxm_stream_t stream) {
  PXM_REQUIRE(p && p->iter_dev, "pxm_wav_iter_counter_add: no counter registered on this plan");
  hipLaunchKernelGGL(k_iter_add, dim3(1), dim3(1), 0, (hipStream_t)stream, p->iter_dev, inc);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_wav_profile_enable(pxm_wav_plan_t p, int max_launches) {
  PXM_REQUIRE(p, "pxm_wav_profile_enable: null plan");
  return profiler_enable(&p->prof, max_launches);
}
int pxm_wav_profile_read(pxm_wav_plan_t p, double* gemm_ms, int64_t* gemm_launches, double* gemm_alg_bytes,
                         double* gemm_flops) {
  PXM_REQUIRE(p, "pxm_wav_profile_read: null plan");
  return profiler_read(&p->prof.gemm, gemm_ms, gemm_launches, gemm_alg_bytes, gemm_flops);
}
int pxm_wav_profile_read_launches(pxm_wav_plan_t p, double* launch_ms, double* launch_alg_bytes,
                                  int32_t* launch_workgroups, int64_t cap, int64_t* launches) {
  PXM_REQUIRE(p && launch_ms && launch_alg_bytes && cap >= 0, "pxm_wav_profile_read_launches: bad arguments");
  return profiler_read(&p->prof.gemm, nullptr, launches, nullptr, nullptr, launch_ms, launch_alg_bytes, cap, launch_workgroups);
}
int pxm_wav_profile_read_dft(pxm_wav_plan_t p, double* dft_ms, int64_t* dft_launches, double* dft_alg_bytes) {
  PXM_REQUIRE(p, "pxm_wav_profile_read_dft: null plan");
  return profiler_read(&p->prof.dft, dft_ms, dft_launches, dft_alg_bytes, nullptr);
}

int64_t pxm_wav_workspace_nonfinite(pxm_wav_plan_t p, pxm_stream_t stream) {
  PXM_REQUIRE(p, "pxm_wav_workspace_nonfinite: null plan");
  hipStream_t st = (hipStream_t)stream;
  // (the scratch row block at the end of the workspace doubles as the counter: nothing of a finished step lives there)
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(p->ws + p->offS);
  PXM_HIP(hipMemsetAsync(cnt, 0, sizeof(*cnt), st));
  hipLaunchKernelGGL(k_count_nonfinite, dim3(1024), dim3(256), 0, st, p->ws, p->offS, cnt);
  PXM_HIP(hipGetLastError());
  unsigned long long h = 0;
  PXM_HIP(hipMemcpyAsync(&h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
  PXM_HIP(hipStreamSynchronize(st));
  PXM_HIP(hipMemsetAsync(cnt, 0, sizeof(*cnt), st));
  return (int64_t)h;
}

// test aid: the arrays of the workspace (everything in front of the scratch row block) -> out, at most cap doubles
int64_t pxm_wav_workspace_read(pxm_wav_plan_t p, double* out, int64_t cap, pxm_stream_t stream) {
  PXM_REQUIRE(p, "pxm_wav_workspace_read: null plan");
  const int64_t n = std::min<int64_t>(cap, p->offS);
  if (n > 0) {
    PXM_REQUIRE(out, "pxm_wav_workspace_read: null destination");
    PXM_HIP(hipMemcpyAsync(out, p->ws, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  return p->offS;
}

// bit mask of the bounded waits of this plan's kernels that EXPIRED since the last clear (0 = none): bit 1 a wave-pair
// wait of the fused phi-DFT kernels.  Synchronises the stream.
int pxm_wav_status(pxm_wav_plan_t p, int clear, pxm_stream_t stream) {
  PXM_REQUIRE(p, "pxm_wav_status: null plan");
  return status_read(p->d_status, (hipStream_t)stream, clear);
}
// number of scales whose rings the fused rings -> X' -> rings launch of this plan transforms with the exact-length unit
// (csrc/dft_pfa.h: ring length 511), 0 when the launch is not grouped or PXM_DFT_PFA=0
int pxm_wav_exact_dft_scales(pxm_wav_plan_t p) {
  PXM_REQUIRE(p, "pxm_wav_exact_dft_scales: null plan");
  return p->dft_group.d ? p->dft_group.n_pfa : 0;
}

// 1 when the grouped fused launch of this plan takes the STOCK kernel instantiation for stock updates (sht_core.h:
// dft_step_is_stock), 0 when the launch is not grouped or PXM_DFT_STOCK=0 at creation
int pxm_wav_dft_stock(pxm_wav_plan_t p) {
  PXM_REQUIRE(p, "pxm_wav_dft_stock: null plan");
  return (p->dft_group.d && p->dft_group.stock) ? 1 : 0;
}

// mask of the streams this plan's launches access non-temporally (include/pxmcmc_amd.h); 0 with PXM_MEM_POLICY=0 at creation
int pxm_wav_mem_policy(pxm_wav_plan_t p) {
  PXM_REQUIRE(p, "pxm_wav_mem_policy: null plan");
  if (!p->mem_policy) return 0;
  return (p->dft_group.d && p->dft_group.stock && DFT_X_OUT_POLICY == MEM_STREAM) ? 1 : 0;  // bit 0: the X' stores
}

int64_t pxm_wav_table_bytes(pxm_wav_plan_t p, int op) {
  if (!p || op < 0 || op > 1) return -1;
  return p->table_bytes[op];
}

int pxm_tables_trim(void) {
  const int64_t freed = tables_trim();
  return (int)std::min<int64_t>(freed >> 20, 1 << 30);  // MiB released
}

// Host-only check of the address ranges (no GPU): runs the REAL plan builders in dry-run mode -- fake device
// addresses, uploads and table kernels skipped -- so that every GEMM task list and DFT group entry of an SHT plan
// (what & 1: bandlimit L, spin) and / or a wavelet plan (what & 2: (L, B, J_min), its Gram lists, and with what & 4
// its weak-lensing lists; what & 8: the wavelet plan at `spin` instead of spin 0 -- weak-lensing lists only at spin 0)
// goes through check_gemm_task_ranges / the group check.  Returns the number of address ranges verified, < 0
// (and pxm_last_error) if one leaves its buffer.  Test aid: PXM_RANGE_SELFTEST="<text>:<bytes>"
// registers the dry-run allocations whose description contains <text> that much shorter (host_api.cpp) -- e.g. the
// per-row scale vectors one row tile short, the round-2 fault -- and the check must then refuse the plan.
int64_t pxm_host_check_address_ranges(int L, double B, int J_min, int spin, int max_chains, int what) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  PXM_REQUIRE(!capture_in_progress(), "pxm_host_check_address_ranges: not during a stream capture");
  set_dry_run(true);
  ranges_checked_reset();
  int rc = 0;
  if (what & 1) {
    pxm_sht_plan_t sp = nullptr;
    rc = pxm_sht_plan_create(L, spin, max_chains, 0, &sp);
    if (sp) pxm_sht_plan_destroy(sp);
  }
  if (!rc && (what & 2)) {
    pxm_wav_plan_t wp = nullptr;
    const int wspin = (what & 8) ? spin : 0;
    rc = pxm_wav_plan_create_spin(L, B, J_min, wspin, max_chains, 0, &wp);
    if (!rc) rc = wav_make_gram_lists(wp);
    if (!rc && (what & 4) && L >= 3 && wspin == 0) rc = pxm_wav_wl_attach(wp, nullptr, nullptr, (int64_t)L * (2 * L - 1));
    if (wp) pxm_wav_plan_destroy(wp);
  }
  if (!rc && (what & 16)) {
    pxm_dft_plan_t dp = nullptr;
    rc = pxm_dft_plan_create(L, max_chains, &dp);
    if (dp) pxm_dft_plan_destroy(dp);
  }
  tables_trim();  // the dry-run table entries (fake addresses) never outlive the call
  set_dry_run(false);
  return rc ? -1 : ranges_checked();
}

// Bytes of the Gram table the ring-space step of a wavelet plan (L, B, J_min) at `spin` streams per launch, as stored: the
// parity-split table where it applies (spin 0, Rp % 32 == 0, PXM_GRAM_SPLIT not 0; order 0 is stored whole in either split
// form), the dense one otherwise.  Host-only: a
// dry-run plan like the one above.
int64_t pxm_host_gram_table_bytes(int L, double B, int J_min, int spin, int max_chains) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  PXM_REQUIRE(!capture_in_progress(), "pxm_host_gram_table_bytes: not during a stream capture");
  set_dry_run(true);
  pxm_wav_plan_t wp = nullptr;
  int rc = pxm_wav_plan_create_spin(L, B, J_min, spin, max_chains, 0, &wp);
  if (!rc) rc = wav_make_gram_lists(wp);
  const int64_t bytes = rc ? -1 : (int64_t)wp->gram.gram_table_bytes;
  if (wp) pxm_wav_plan_destroy(wp);
  tables_trim();
  set_dry_run(false);
  return bytes;
}

}  // extern "C"
