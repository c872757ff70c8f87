// Static GEMM task lists of the transform plans (tasklist.hip): construction, ordering, range check, upload and launch.
#pragma once
#include "sht_core.h"
#include "sht_tables.h"

namespace pxm {

// extras of a GemmSide for the fused wavelet combine
struct GemmFuse {
  int64_t x2_base = -1;           // second operand array (same L / Rp as x), -1 = none
  const double* rscale = nullptr;  // per-output-row scale
  int row_lo = 0, row_hi = 1 << 30;
  int64_t hd_base = -1;            // array holding the affine constants, -1 = none ...
  int hd_stride = 0;               // ... and its row stride in doubles (0: H layout, ncol doubles per row, chain 0)
};
// One transform's GEMM stage.  x_base / y_base are offsets (doubles) of the [2L-1][Rp][ncol] operand / output arrays
// inside the workspace; x rows may belong to a larger array (x_Rp, x_L give the operand array's row padding and
// bandlimit for the m_idx mapping).
struct GemmSide {
  int64_t x_base, y_base;
  int x_L, x_Rp, y_L, y_Rp;
  const double* kscale;
  int el_lo;
  GemmFuse fuse;
  int x_ncol = 0, y_ncol = 0;  // 0 = the launch's ncol
};
// append the tasks of one transform's GEMM stage
void append_gemm_tasks(const ShtTables& T, int kind, int ncol, const GemmSide& side, int64_t scratch_off,
                       const double* ws_base, std::vector<GemmTask>& tasks);
// the same for up to TWO transforms that share the table T (same bandlimit): one pass over the table, 4 slabs
void append_gemm_tasks_packed(const ShtTables& T, int kind, int ncol, const GemmSide& side_a, const GemmSide* side_b,
                              int64_t scratch_off, const double* ws_base, std::vector<GemmTask>& tasks);

struct TaskList {
  GemmTask* d = nullptr;
  int n = 0;
  bool paired = false;
  int nslab = 2;         // kernel variant: 1 unpaired, 2 +-m pairs
  std::vector<int> bls;  // bandlimits of the transforms grouped in this launch (roofline accounting)
  std::vector<int> los;  // their support cuts el_lo (0 = none)
  double mfma_units = 0; // sum over tasks of row tiles x k-steps x slabs: MFMAs per column tile
  bool gram = false;     // Gram launch: the stored Gram tiles, TWO harmonic operand arrays read, one written, the data term
  double gram_table_bytes = 0;  // bytes of the Gram table as stored (dense: 16-row / 16-k tiles from round_down(m, 16); or
                                // the parity-split table of sht_tables.h)
  bool gram_pole = false;        // the list has the order-0 halves with their pole term (TAB_GRAM_SPLIT0) ...
  double gram_stream_bytes = 0;  // ... and streams this much of the stored table (the off-diagonal blocks of order 0 are not read)
  int flags = 0;         // GemmListFlag bits: GEMM_LIST_TWO tasks sum a second operand in while staging, GEMM_LIST_SCALE
                         // per-row operand scale, GEMM_LIST_POLE pole term (kernel variant)
  int pk = 0;            // packed column tile (few-chain plans, sht_gemm.hip: k_sht_gemm_pk): live columns per slab, 0 = off
  std::vector<char> tab_shared;  // packed lists: transform i streams its table together with transform i - 1 (one pass)
};

// launch order of a list: "xcd" (one queue per XCD), "bins" (one bin per CU) or anything else (descending work)
void order_tasks(std::vector<GemmTask>& v, const std::string& order);
// orders the tasks (PXM_GEMM_ORDER or by size), checks every address range their launches can form and uploads them
// (ordered: where given, receives the list in launch order, padding entries included -- what the GEMM-only plan reports)
int upload_tasks(std::vector<GemmTask> v, bool paired, TaskList* out, std::vector<int> bls, int ncol, const double* ws_base,
                 const char* name, std::vector<int> los = {}, int pk = 0, std::vector<char> tab_shared = {},
                 std::vector<GemmTask>* ordered = nullptr);
// algorithmic bytes of one launch of a list for cg live chain slots
double tasklist_bytes(const TaskList& tl, int cg);
// marks an uploaded list as the Gram launch of table T.d_tab[kind]: the four gram* fields tasklist_bytes accounts with
void tasklist_set_gram(TaskList* tl, const ShtTables& T, int kind);
// run a task list over all chain groups (16 chains = 32 columns per launch)
int run_tasks(const TaskList& tl, const double* X, double* Y, int ncol, int C, hipStream_t st,
              const GemmAffine& aff = GemmAffine(), Profiler* prof = nullptr);
void free_tasks(TaskList* t);

}  // namespace pxm
