// Wavelet plan (axisymmetric scale-discretised wavelets, multiresolution): the plan, its weak-lensing attachment and what
// wav_plan.hip (building), wav_ops.hip (transforms and steps) and wav_wl.hip (weak lensing) share.
#pragma once
#include "plan_common.h"

#include <algorithm>

namespace pxm {

constexpr int WAV_MAX_SCALES = 40;  // scaling function + wavelet scales of one plan (B = 1.2 at L = 512: 36)

// Weak-lensing attachment of a wavelet plan (wav_wl.hip: pxm_wav_wl_attach builds one completely, then hands it to the plan).
// It owns everything below except the caller's mask arrays; wl_release gives it all back.
struct WlAttach {
  // the spin-2 ring stage at L: ring tables and their two lists ...
  ShtTables* T2 = nullptr;             // (one reference of the table cache held)
  TaskList inv, invadj;                // class buffers --k_l B2--> G2 ; G2 --B2^T, k_l--> H_L
  RecTables* rec2 = nullptr;           // ... or the table-free stage (sht_rec.hip) when the plan carries few chains
  double* d_wlk = nullptr;             // [Rp] k_l = -sqrt((l+2)(l-1)/((l+1)l)), zero for l < 2 (measurements.py:151-171)
  const int32_t* gidx = nullptr;       // [P] pixel -> data index (caller-owned), null = no mask
  const double* gw = nullptr;          // [ndata] covariance weight (caller-owned) or null
  int64_t ndata = 0;
  // twin top scales (one chain): two scales of equal bandlimit above the DFT group share ONE ring array -- the finer scale
  // sits in chain slot 1 of the coarser one's 128-B lines -- so that their blocks <-> rings transforms are one two-"chain"
  // launch instead of two one-chain launches and the packed GEMM stages both from the same lines
  int twin_s = -1;                     // the coarser scale of the pair, -1 = none
  double* d_twin = nullptr;            // [2 bl - 1][Rp_bl][ncol_t]
  int64_t offGT = 0;                   // d_twin relative to the plan's ws (doubles)
  int ncol_t = 0;                      // doubles per row of the twin array: 4 (narrow: its two slots and nothing else)
  TaskList syn_fwd, adj_fwdadj;        // packed per-scale lists reading / writing the twin array
  // narrow ring array of the spin-2 stage (recursion kernels <-> DFT at L): 2 Cmax doubles per row instead of a 128-B line of
  // eight chain slots -- both its producers and its consumers take the row stride as an argument
  double* d_g2n = nullptr;
  int ncol_g2 = 0;
  // ... and of the harmonic side of the one-chain path: class buffers A / B and H_L as [m][l][2 C] arrays of their own
  // (the plan's eight-slot class buffers stay with the generic synthesis / analysis paths)
  double* d_hn = nullptr;
  int64_t offHAn = 0, offHBn = 0, offHLn = 0;  // relative to ws (doubles)
  int ncol_h = 0;
  // ... and of the scales INSIDE the DFT group on that path: ring arrays of 2 Cmax doubles per (m, ring) entry in one
  // allocation, their own group descriptors (offGn[s] relative to ws; non-members keep offG[s]; dft_group_n.d null = none)
  double* d_gn = nullptr;
  std::vector<int64_t> offGn;
  int ncol_gn = 0;
  DftGroupList dft_group_n;
};
void wl_release(WlAttach* w);  // wav_wl.hip (null is fine)

}  // namespace pxm

struct pxm_wav_plan_s {
  int L = 0, J_min = 0, J_max = 0, Cmax = 0, Cp = 0, ncol = 0, Rp = 0;
  // spin of the images: only the L-level ring stage runs at it -- the coefficients of axisymmetric
  // wavelets are spin-0 functions whatever the spin of f, so every per-scale stage stays the spin-0 one
  int spin = 0;
  double B = 0;
  int nsc = 0;  // scaling + wavelet scales
  std::vector<int> bl;
  std::vector<int64_t> coef_off;  // offset of each block in the coefficient vector (complex elements)
  int64_t ncoefs = 0;
  std::vector<pxm::ShtTables*> T;  // per scale
  pxm::ShtTables* TL = nullptr;
  std::vector<pxm::DftPlan> dft;  // per scale
  pxm::DftPlan dftL;
  double* ws = nullptr;
  std::vector<int64_t> offG;
  int64_t offGL = 0, offHL = 0, offS = 0;
  int64_t offGD = 0, offHD = 0;
  int64_t offHDc = 0;  // chain-less copy of the data term B^T DFT(data): [m + L - 1][row][2] (re, im), what the Gram epilogue reads
  int64_t offG2 = 0;   // spin-2 rings at L of the weak-lensing attachment (eight-slot lines)
  pxm::TaskList gram, adj_invadj_D;   // Gram step of the ring-space MYULA iteration; B^T DFT(data)
  bool have_data_rings = false;
  int64_t offHA = 0, offHB = 0;  // L-layout class buffers of the fused combine (disjoint l-supports per class)
  double* d_kc_syn = nullptr;  // [nsc][Rp]  c_s * kappa   (synthesis and its adjoint)
  double* d_kc_ana = nullptr;  // [nsc][Rp]  c_a * kappa   (analysis and its adjoint)
  pxm::TaskList syn_fwd, syn_inv, adj_invadj, adj_fwdadj;  // synthesis / synthesis-adjoint stages
  pxm::TaskList ana_fwd, ana_inv, anadj_invadj, anadj_fwdadj;  // analysis / analysis-adjoint stages
  int64_t table_bytes[2] = {0, 0};
  // side streams: the DFT launches of the small scales are latency-bound (a few workgroups each);
  // they run beside the large scales' launches instead of in front of them
  static constexpr int NSIDE = 3;  // capacity (the streams of the per-device pool) ...
  static constexpr int nside = 2;  // ... of which a plan uses two
  hipStream_t side[NSIDE] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[NSIDE] = {nullptr, nullptr, nullptr};
  bool plain_group = true;  // blocks <-> rings of the member scales in one grid (PXM_NO_PLAIN_DFT_GROUP=1: per scale)
  std::vector<int> lane_of;  // per scale: -1 = caller's stream, else side stream index
  pxm::DftGroupList dft_group;   // every scale's rings -> X' -> rings kernel in one grid (ring-space step)
  bool mem_policy = true;    // the plan's lists were made with the build's cache policies (mem_policy.h; PXM_MEM_POLICY is not 0)
  int pk = 0;                // live columns per slab of the packed per-scale lists, 0 = unpacked (more than 2 chains)
  std::vector<int> el_lo_s;  // per scale: first degree of the support (rows / contraction steps below it are skipped)
  pxm::WlAttach* wl = nullptr;   // weak-lensing attachment (owned), null = none attached
  std::vector<pxm::ShtTables*> held;  // table-cache entries this plan retains (each once)
  unsigned* d_status = nullptr;  // device status word of THIS plan: bit 1 DFT pair wait (pxm_wav_status)
  uint64_t* iter_dev = nullptr;  // device-resident Philox iteration counter of THIS plan (pxm_wav_set_iter_counter)
  pxm::Profiler prof;            // live kernel timing of THIS plan (pxm_wav_profile_*)
};

namespace pxm {

inline void wav_hold(pxm_wav_plan_s* p, ShtTables* T) {
  if (std::find(p->held.begin(), p->held.end(), T) != p->held.end()) return;
  retain_tables(T);
  p->held.push_back(T);
}

// a task list of the plan on the plan's workspace, column count and profiler
inline int wav_run(pxm_wav_plan_s* p, const TaskList& tl, int C, hipStream_t st, const GemmAffine& aff = GemmAffine()) {
  return run_tasks(tl, p->ws, p->ws, p->ncol, C, st, aff, &p->prof);
}

// is scale s transformed by the grouped blocks <-> rings launches (dft_wave.hip: k_px2ring_group5 / k_ring2px_group5<false>)?
inline bool wav_in_group(const pxm_wav_plan_s* p, int s) { return p->dft_group.d && p->plain_group && p->dft_group.member[s]; }

// packed per-scale lists (sht_gemm.hip: k_sht_gemm_pk) of stage `which` (0 synthesis forward, 1 its adjoint, 2 analysis
// inverse, 3 its adjoint) for every scale; scales of equal bandlimit stream their table in one pass.  wl != null: the lists
// of that weak-lensing attachment (scales twin_s / twin_s + 1 on chain slots 0 / 1 of its twin array, its narrow arrays).
int wav_packed_lists(const pxm_wav_plan_s* p, int which, int kind, const WlAttach* wl, std::vector<GemmTask>& out,
                     std::vector<char>* shared);
// Gram tables + the two extra task lists of the ring-space step (first pxm_wav_ring_set_data of a plan)
int wav_make_gram_lists(pxm_wav_plan_s* p);

// coefficient blocks -> G_s (scales' px2ring) ; G_s -> coefficient blocks (ring2px with out's epilogue).  twin: the one-chain
// weak-lensing path on the arrays of p->wl.
int wav_blocks_to_rings(pxm_wav_plan_s* p, const void* X, int C, hipStream_t st, bool twin = false);
int wav_rings_to_blocks(pxm_wav_plan_s* p, PxOut proto, int C, hipStream_t st, bool twin = false);

}  // namespace pxm
