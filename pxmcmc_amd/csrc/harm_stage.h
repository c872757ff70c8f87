// The harmonic split / merge stage of the wavelet plans with orientations (harm_stage.hip): the directional plan
// (dirwav.hip) runs it between its SHTs, the harmonic-space plan (harmwav.hip, section 13) is it.
//
//   split   out_d[c][lm] = w_d(l) f[c][lm]                for every (block, n) item d and lm < bl_d^2   (k_dw_split)
//   merge   f[c][lm]     = sum_d [l < bl_d] w_d(l) b_d[c][lm]                                            (k_dw_merge)
//
// Both kernels are complex128 streams: one 16-byte element per lane, weights from host tables, one launch for every item
// and chain (grid.y = chain; the split's grid.x = the items' blocks back to back).
#pragma once
#include "common.h"

#include <vector>

namespace pxm {

constexpr int DW_THREADS = 256;

struct DwItem {      // one (block, n) operand of the harmonic stages
  int64_t a_off;     // offset of chain 0's bl*bl entries: in the harmonic arena, or in a harmonic coefficient vector
  int64_t cstride;   // chain stride of the operand: bl*bl (arena, [C][bl*bl] per item) or ncoefs ([C][ncoefs] vector)
  int64_t w_off;     // row of the weight tables, L entries
  int bl;
  int blk0;          // first thread block of this item in the split launch
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

// The stage as a plan holds it: the items and the two weight tables (one row of L entries per item) on the device.
struct HarmStage {
  int L = 0, nitems = 0, split_blocks = 0;  // split_blocks: grid.x of the split launch
  DwItem* d_items = nullptr;
  double2* d_wa = nullptr;  // analysis weights
  double2* d_ws = nullptr;  // synthesis weights
};
// weights: 0 analysis (wa), 1 synthesis (ws); cj: conjugate them.  flm [C][L*L]; harm: what the items' a_off address
int harm_split(const HarmStage& s, const double2* flm, double2* harm, int weights, int cj, int C, hipStream_t st);
int harm_merge(const HarmStage& s, const double2* harm, double2* flm, int weights, int cj, int C, hipStream_t st);
void harm_release(HarmStage* s);

// The items of a plan are (block b, orientation n) pairs, blocks in order: block 0 is the scaling function with the one
// n = 0, block b > 0 is scale J_min + b - 1 with n_k = -(N-1), -(N-3), .., N-1 for k < N.
inline int harm_orients(int b, int N) { return b ? N : 1; }
inline int harm_n(int b, int k, int N) { return b ? -(N - 1) + 2 * k : 0; }

// The create-time argument checks of both plans, in the name of the entry point `who` (the directional plan is spin 0).
int harm_create_check(const char* who, const void* plan, int L, double B, int J_min, int N, int spin, int max_chains);

// The weights of the harmonic stages, item by item: one row of L entries per (block b, orientation n) for the split (wa)
// and one for the merge (ws).  Block 0 is the scaling function (n = 0): kappa_0(l) in both rows.  Block b > 0 is scale
// J_min + b - 1 with k = kappa_j(l) s_ln:
//   pixel space (DirWavPlan)      wa = (-1)^n conj(k) / sqrt(2 pi)      ws = (-1)^n k sqrt(2 pi)
//   harmonic space (HarmWavPlan)  wa = sqrt(8 pi^2/(2l+1)) conj(k)     ws = sqrt((2l+1)/(8 pi^2)) k
// Spin s (N = 1): every row is zero for l < |s|.
struct DwTiling {
  int L, J_min, spin;
  std::vector<double> k0, kap;
  std::vector<double2> s;  // directionality component s_lm [L*L]
  DwTiling(int L, double B, int J_min, int N, int spin);
  void rows(int b, int n, bool harmonic, std::vector<double2>& wa, std::vector<double2>& ws) const;
};

// The weight tables of a plan as it uploads them: one row of L entries per item, appended to wa / ws in plan order, with
// the (block, n, bl) of every row returned.  Pixel space (harmonic = false) skips the pairs |n| >= bl_j, whose s_ln
// vanishes for every l < bl_j; harmonic space stores every pair.  Both plans and pxm_host_harm_weights build from this.
struct HarmRow {
  int block, n, bl;
};
std::vector<HarmRow> harm_weight_rows(int L, double B, int J_min, int N, int spin, bool harmonic, std::vector<double2>& wa,
                                      std::vector<double2>& ws);

// The phases of the gamma stage, ph[q][k] = e^{i n_k gamma_q} with gamma_q = 2 pi q / (2N-1): [2N-1][N], what the
// directional plan uploads and pxm_host_dwav_phases exports.
std::vector<double2> dw_phases(int N);

}  // namespace pxm
