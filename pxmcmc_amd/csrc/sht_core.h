// Internal C++ interface of the SHT engine: GEMM stage, DFT stage, layout repack (ring tables: sht_tables.h, task-list
// construction: tasklist.h).
//
// Formulation.  Every MW transform is a phi-DFT stage and a
// per-m "Legendre" stage that contracts a REAL table with complex data:
//   inverse         : H[m][el] --(B^m  : ring<-el)--> G[m][t] --iDFT--> f(t,p)
//   forward_adjoint : H[m][el] --(A^mT : ring<-el)--> G[m][t] --iDFT--> f(t,p)
//   forward         : f(t,p) --DFT--> G[m][t] --(A^m  : el<-ring)--> H[m][el]
//   inverse_adjoint : f(t,p) --DFT--> G[m][t] --(B^mT : el<-ring)--> H[m][el]
// with B^m[t][el] = (-1)^s sqrt((2el+1)/4pi) d^el_{m,-s}(theta_t) and
// A^m = (2pi/(2L-1)) B^mT Q^{parity(m+s)} the exact MW quadrature.  The chain batch
// turns each per-m contraction into a real GEMM with 2*C columns (re/im of every
// chain), run on v_mfma_f64_16x16x4_f64 with the table streamed from HBM exactly once.
//
// Internal layouts (row = ring t or degree el, padded to Rp = roundup(L,16)):
//   G, H : [m_idx = m + L - 1][row][ncol]   ncol = 2*Cp doubles, Cp = roundup(C, 8)
#pragma once
#include "common.h"
#include "profiler.h"

namespace pxm {

// Row tiles of 16 output rows per task (= per workgroup): 8 waves x 1 row tile per wave.  (4 waves x 1 and 4 x 2 were
// A/B variants until round 2: 26.1 us and slower for the Gram launch, operand staged twice as often.)
constexpr int GEMM_TASK_ROW_TILES = 8;

// One workgroup's share of a per-m GEMM: up to GEMM_TASK_ROW_TILES row tiles of 16 output rows.
// Column slabs: slab 0 = +m, slab 1 = -m (spin 0 shares one table up to the sign (-1)^m).  A MERGED task
// (nslab = 4) streams the table once for TWO transforms at the same bandlimit (the two full-size wavelet
// scales): slabs 2, 3 are the +m / -m slabs of the second transform; slabs 2g, 2g+1 form group g and share
// the per-k operand scale, the per-row output scale and the row mask of that transform.
struct GemmTask {
  int64_t tab_off;     // tiled table of this (m, first row tile), in doubles relative to the workspace base
                       // (kernel-argument-relative so the loads are global_load, not flat_load)
  int64_t rt_stride;   // doubles between consecutive row tiles
  int64_t x_off[4];    // operand slab offsets (doubles)
  int64_t y_off[4];    // output slab offsets
  int64_t x2_off[4];   // optional second operand (same layout) added to the first while staging; 0 = none
  int64_t hd_off[4];   // affine epilogue: per-row complex constant of each slab: (re, im) at hd_off + row * hd_stride
  int64_t ks_off[2];   // per group: optional per-k scale vector (indexed by absolute k) relative to the base; 0 = none
  int64_t rs_off[2];   // per group: optional per-output-row scale vector (absolute row); 0 = none
  int row_lo[2], row_hi[2];  // per group: only output rows in [row_lo, row_hi) are written
  int k_beg, k_end;    // contraction range, multiples of 16
  int row0;            // first output row of this task
  int n_rt;            // row tiles in this task (1..GEMM_TASK_ROW_TILES)
  int nslab;           // live slabs: 1 (all m stored) or 2 (+-m pair)
  double sign1;        // factor on the -m outputs ((-1)^m)
  int m_unit;          // the order this task belongs to: m (paired tables: m >= 0 serves +-m) or m + L - 1
  int hd_stride;       // doubles between consecutive rows of the affine constants: 2 = the chain-less [m][row] complex
                       // array of the Gram step (whole 64-B segments per wave), ncol = columns 0, 1 of an H-layout array
  int x_ncol, y_ncol;  // doubles per row of THIS task's operand / result arrays.  Read by the packed kernels (a narrow ring
                       // array of a few-chain plan has 2 C or 4 columns per row instead of the plan's 16) and by the
                       // two-operand kernels (the parity halves of the split Gram list step through an H-layout plane two
                       // rows at a time: 2 ncol); the streaming 16-columns-per-slab kernels take the launch's ncol for both
  // pole term of the order-0 halves of the split Gram list (TAB_GRAM_SPLIT0), pole_n = 0: none.  The task adds
  // 1/2 b_own[row] * s[col] to its products, s[col] = sum over the pole_n half-rows r of the OTHER parity of
  // b_other[r] * x[r][col], x being the staged operand (both class buffers) pole_dx doubles away from the task's own
  int pole_n;          // half-rows of the other parity (Rp / 2)
  int pole_dx;         // doubles from this half's operand to the other parity's: + ncol (even half) or - ncol (odd half)
  int64_t pole_b_off;  // b of this half's degrees, indexed by half-row (relative to the workspace base, like tab_off)
  int64_t pole_bo_off; // b of the other parity's degrees
};

// affine epilogue of the Gram launch: out = w * (ns * acc - hd[row]) as a complex product per chain
struct GemmAffine {
  double ns = 0, wr = 0, wi = 0;
  int on = 0;
  int ncol_live = 1 << 30;   // columns >= ncol_live (padding chains) are written as zero: they must not iterate
  uint64_t* bump = nullptr;  // optional: workgroup 0 adds 1 to this counter before anything of this step reads it
};

// start-up and drain of a GEMM task, in contraction steps (the figure the XCD launch order balances with, tasklist.hip)
constexpr int GEMM_TASK_FIXED_STEPS = 32;

// what the tasks of a list carry, i.e. the kernel variant its launches take (TaskList::flags)
enum GemmListFlag {
  GEMM_LIST_TWO = 1,    // a second operand, summed in while staging
  GEMM_LIST_SCALE = 2,  // a per-contraction-row operand scale
  GEMM_LIST_POLE = 4,   // a pole term (the split Gram list with its order-0 halves: two operands, no scale, +-m pairs)
};

// Column groups of an unpacked list: one launch per 32 columns (two column tiles of 16) while 32 remain, one tile after
constexpr int GEMM_GROUP_COLS = 32;
inline int gemm_group_tiles(int ncol, int col0) { return (ncol - col0 >= GEMM_GROUP_COLS) ? 2 : 1; }

// packed launch (pk = live columns per slab: 2 or 4); flags: GemmListFlag bits
int launch_gemm_packed(const GemmTask* d_tasks, int n_tasks, int pk, int flags, const double* X, double* Y, int ncol, int col0,
                       double alg_bytes, double flops, hipStream_t stream, Profiler* prof = nullptr);

// launch: tasks on device; X/Y = workspace base; col0 = first column of this chain group, ct = column
// tiles (1 or 2) of the group
// alg_bytes: algorithmic bytes of this launch (table once + operand + result), for the live profiler
// nslab: 1 (unpaired) or 2 (+-m pairs); flags: GemmListFlag bits
int launch_gemm(const GemmTask* d_tasks, int n_tasks, int nslab, int flags, const double* X, double* Y, int ncol,
                int col0, int ct, double alg_bytes, double flops, hipStream_t stream,
                const GemmAffine& aff = GemmAffine(), Profiler* prof = nullptr);

// algorithmic bytes of one ring-GEMM stage at bandlimit L for C chains:
// ring table 8*L*L*(L+1)/2 [paired] or 8*L*L*L [all m] read once, harmonic side 16*C*L*L,
// ring side 16*C*L*(2L-1)
// With a support cut el_lo only the degrees el >= el_lo count on the table and harmonic sides.
inline double gemm_table_bytes(int L, bool paired, int el_lo = 0) {
  double tab_entries = 0;
  for (int m = paired ? 0 : -(L - 1); m < L; ++m) {
    const int am = m < 0 ? -m : m;
    const int n = L - (am > el_lo ? am : el_lo);
    if (n > 0) tab_entries += n;
  }
  return 8.0 * L * tab_entries;
}
inline double gemm_alg_bytes(int L, bool paired, int C, int el_lo = 0) {
  double tab_entries = 0, lm_entries = 0;  // (m, el) pairs with el >= max(|m|, el_lo)
  for (int m = paired ? 0 : -(L - 1); m < L; ++m) {
    const int am = m < 0 ? -m : m;
    const int n = L - (am > el_lo ? am : el_lo);
    if (n > 0) tab_entries += n;
  }
  for (int m = -(L - 1); m < L; ++m) {
    const int am = m < 0 ? -m : m;
    const int n = L - (am > el_lo ? am : el_lo);
    if (n > 0) lm_entries += n;
  }
  return 8.0 * L * tab_entries + 16.0 * C * (lm_entries + (double)L * (2 * L - 1));
}

// host model of every address k_sht_gemm / k_sht_gemm_pk (pk != 0) forms for a task list (sht_gemm.hip); < 0 + error
// text when a range leaves its allocation
int check_gemm_task_ranges(const std::vector<GemmTask>& v, int nslab, int pk, int flags, int ncol, const double* ws_base,
                           const char* list_name);

// ---- DFT stage ---------------------------------------------------------------
// Three units transform the rings; a plan uses one, chosen at creation by its ring length n = 2L - 1:
//   DFT_PAIR   n <= 511: eight points per lane, a pair of waves per ring set (dft_wave.hip); n = 511 on eight-slot lines
//              runs the exact-length body (dft_pfa.h) unless PXM_DFT_PFA=0
//   DFT_QUAD   511 < n <= 1023: four waves per ring, eight points per lane (dft_wave.hip)
//   DFT_RADIX2 1023 < n <= 2047, and every n <= 2047 with PXM_DFT_NO_W=1: the radix-2 in-LDS unit (dft.hip; an independent
//              implementation, the cross-check of the other two).  Longer rings (L >= 1025) have no unit: dft_geometry
enum DftUnit { DFT_RADIX2, DFT_PAIR, DFT_QUAD };

// device tables of the pair unit: one allocation, typed views into it
struct PairTables {
  double* d_all = nullptr;
  int r0 = 0;  // Mh / 64
  int pfa_off = 0;  // n = 511: the table block of the exact-length unit inside the allocation (doubles), 0 = none
  const double *cE = nullptr, *cO = nullptr, *dO = nullptr, *tw1 = nullptr, *wt = nullptr, *bE = nullptr, *bO = nullptr;
};

// device tables of the quad unit
struct QuadTables {
  double* d_all = nullptr;
  const double *cA = nullptr, *cB = nullptr, *dA = nullptr, *dB = nullptr, *tw1 = nullptr, *wt = nullptr, *bQ = nullptr;
};

struct DftPlan {
  int L = 0, n = 0, Rp = 0;
  DftUnit unit = DFT_RADIX2;
  // radix-2 unit: M-point in-LDS transform, R chains per workgroup of `threads` threads, `lds` bytes of LDS
  int M = 0, logM = 0, R = 0, threads = 0;
  size_t lds = 0;
  double *d_chirp = nullptr, *d_bhat = nullptr, *d_tw = nullptr;
  PairTables pair;
  QuadTables quad;
  // status word of the OWNING plan (set by the owner after make_dft_plan; null: expiries go unrecorded) and the bound
  // of the wave-pair wait of the pair unit (PXM_DEBUG_PAIR_SYNC_LIMIT, read at plan creation: 0 forces an expiry)
  unsigned* d_status = nullptr;
  unsigned spin_limit = 1u << 18;
  // the fused step's stock launches (dft_step_is_stock) take the STOCK kernel instantiations; PXM_DFT_STOCK=0 at plan
  // creation keeps the generic ones (A/B runs, the identity test)
  bool stock = true;
};
// bit of a plan's status word (pxm_wav_status / pxm_sht_status); bit 0 is unused
enum { PXM_STATUS_PAIR_SYNC_BIT = 2 };

// What a plan at bandlimit L runs its rings on: the one selection rule, read by make_dft_plan and reported by
// pxm_host_dft_geometry.  Honours PXM_DFT_NO_W and PXM_DFT_PFA.
struct DftGeometry {
  DftUnit unit = DFT_RADIX2;
  int M = 0;        // length of the Bluestein transform (the exact-length body runs beside the M = 1024 tables of n = 511)
  int per_wg = 0;   // radix-2, quad: chains per workgroup (R; the quad unit takes 1 for a single chain); pair: rings per ring
                    // set, 8 / r0 (a ring pair for the exact-length body)
  int threads = 0;  // threads per workgroup
  size_t lds = 0;   // dynamic LDS per workgroup, bytes
  bool exact = false;  // n = 511 runs the exact-length body (dft_pfa.h)
  bool pfa = true;     // PXM_DFT_PFA is not 0
};
constexpr size_t DFT_LDS_MAX = 160 * 1024;  // what allow_dynamic_lds permits: the LDS of a CU
// < 0 with the error text (L, M and the byte count) where the selected geometry needs more than DFT_LDS_MAX: L >= 1025
int dft_geometry(int L, DftGeometry* g);

int make_dft_plan(int L, DftPlan* p);
void free_dft_plan(DftPlan* p);

// Input / output functors fused into the DFT stage's global reads / writes.
struct PxIn {  // px2ring input: plain image, or residual invcov .* (preds - data)
  const double* f = nullptr;   // [C][chain_stride] complex (image or preds)
  int64_t chain_stride = 0;    // in complex elements
  int64_t ring0 = 0;           // offset of ring 0 inside a chain (complex elements)
  const double* data = nullptr;    // [P] complex, shared (residual mode when non-null)
  const double* invcov = nullptr;  // [P] real or complex
  int invcov_complex = 0;
  uint64_t* bump = nullptr;  // optional: workgroup 0 adds 1 to this counter (the Philox iteration counter)
  // scatter mode (weak-lensing mask, pxmcmc/measurements.py:263-280,295-304): f / data / invcov are DATA-space
  // arrays [ndata]; pixel e reads entry gidx[e] (masked pixels, gidx < 0, read zero) times the weight gw
  const int32_t* gidx = nullptr;  // [P] pixel -> data index, < 0 = masked
  const double* gw = nullptr;     // [ndata] covariance weight or null
};
struct PxOut {  // ring2px output: plain image, or the fused MYULA update of a coefficient block
  double* f = nullptr;
  int64_t chain_stride = 0;
  int64_t ring0 = 0;
  // MYULA mode when X != null: f = (1-d/l) X + (d/l) soft(X,T) - d * value + sqrt(2d) w
  const double* X = nullptr;
  const double* T = nullptr;  // [N] thresholds (offset by ring0 like X) or null -> T_scalar
  double T_scalar = 0, delta = 0, lmda = 0;
  const double* noise = nullptr;  // injected noise or null -> Philox
  int mode = 0;  // update.h: 0 complex state + real noise, 1 + complex noise, 2 two real chains per slot
  int noise64 = 0;  // Box-Muller step of the Philox stream in double precision (flag PXM_NOISE_F64 of the entry points)
  uint64_t seed = 0, chain0 = 0, iter = 0;
  const uint64_t* iter_dev = nullptr;  // optional device-resident addend to iter (graph replay)
  // residual mode of the fused rings -> image -> rings kernel (X == null): the image is written to f and the rings
  // of rinvcov .* (image - rdata) go back in place (pxmcmc/forward.py:66-69 between forward() and calc_gradg())
  const double* rdata = nullptr;    // [P] complex, shared by all chains
  const double* rinvcov = nullptr;  // [P] real or complex
  int rinvcov_complex = 0;
  // gather mode (weak-lensing mask, pxmcmc/measurements.py:242-261,295-304; plain output only): f is a DATA-space
  // array [C][chain_stride = ndata]; pixel e is written to entry gidx[e] times the weight gw, masked pixels are dropped
  const int32_t* gidx = nullptr;
  const double* gw = nullptr;
};

// The stock MYULA update of the fused rings -> X' -> rings step: state and thresholds in place (X, vector T), Philox noise,
// two real chains per slot from an even first chain (one Philox pair per slot), the device-resident iteration addend of
// graph replay, and neither residual nor gather.  The fused launchers of the pair unit (dft_wave.hip) run such a launch on
// kernel instantiations that hold all of this as compile-time facts (template parameter STOCK); every other launch takes
// the generic instantiations.  mode 2: PXM_MODE_REAL_PAIRS (update.h).
inline bool dft_step_is_stock(const PxOut& o) {
  return o.X && o.T && !o.noise && o.mode == 2 && !(o.chain0 & 1) && o.iter_dev && !o.rdata && !o.rinvcov && !o.gidx && !o.gw;
}

// grouped launches of a wavelet plan's member scales (dft_wave.hip): one grid for every scale on the pair unit
struct DftGroupList {
  void* d = nullptr;  // device array of per-scale descriptors
  int n = 0, blocks = 0;
  int n_pfa = 0;  // member scales that take the exact-length body (n = 511: two rings per workgroup, own block counts)
  double px_elems = 0;  // sum over scales of bl (2 bl - 1): coefficients per chain slot
  int64_t ring_end = 0; // largest ring0 + L n over the entries: the launches require it <= chain_stride
  std::vector<char> member;  // per scale: its rings <-> pixels launches are part of this group
  bool all = false;          // every scale is a member (needed by the fused rings -> X' -> rings step)
  bool stock = true;         // stock launches take the STOCK instantiation (PXM_DFT_STOCK is not 0 at creation)
  bool mem_policy = true;    // ... with the build's cache policy of the X' stores (mem_policy.h; PXM_MEM_POLICY is not 0 at creation)
};
int dft_group_create(const std::vector<const DftPlan*>& plans, const std::vector<int64_t>& g_off,
                     const std::vector<int64_t>& ring0, int ncol, const double* ws_base,
                     DftGroupList* out);  // 1 = not available
void dft_group_destroy(DftGroupList* g);
// the fused rings -> X' -> rings step of every member scale in one grid
int dft_group_launch(const DftGroupList& g, double* ws, int ncol, const PxOut& out, int C, hipStream_t st,
                     Profiler* prof = nullptr);
// the plain transforms of every member scale in one grid each (blocks <-> rings of the generic wavelet operators)
int dft_group_px2ring(const DftGroupList& g, double* ws, int ncol, const PxIn& in, int C, hipStream_t st);
int dft_group_ring2px(const DftGroupList& g, double* ws, int ncol, const PxOut& out, int C, hipStream_t st);

// f(t,p) -> G[m][t][c]  (unnormalised, e^{-i m phi});  G -> f (e^{+i m phi})
int launch_px2ring(const DftPlan& p, const PxIn& in, double* G, int ncol, int C, hipStream_t stream);
int launch_ring2px(const DftPlan& p, const double* G, int ncol, const PxOut& out, int C, hipStream_t stream);
// fused: rings -> out.f (with out's epilogue) and the rings of what was written, in place over G -- only where
// dft_can_fuse (an error otherwise)
int launch_ring2px2ring(const DftPlan& p, double* G, int ncol, const PxOut& out, int C, hipStream_t stream);
inline bool dft_can_fuse(const DftPlan& p) { return p.unit == DFT_PAIR; }

// ---- layout repack (public harmonic layout el^2+el+m <-> internal [m][el][c]) ----------
int launch_lm_to_mel(const double* flm, double* H, int L, int Rp, int ncol, int C, int spin, hipStream_t stream);
int launch_mel_to_lm(const double* H, double* flm, int L, int Rp, int ncol, int C, int spin, hipStream_t stream);

}  // namespace pxm
