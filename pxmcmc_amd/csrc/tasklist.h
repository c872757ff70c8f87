// Static GEMM task lists of the transform plans (tasklist.hip): ordering, range check, upload and launch.
#pragma once
#include "sht_core.h"

namespace pxm {

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
                                // the parity-split table of sht_core.h)
  bool gram_pole = false;        // the list has the order-0 halves with their pole term (TAB_GRAM_SPLIT0) ...
  double gram_stream_bytes = 0;  // ... and streams this much of the stored table (the off-diagonal blocks of order 0 are not read)
  int flags = 0;         // bit 0: tasks sum a second operand in while staging; bit 1: per-row operand scale; bit 2: pole term
                         // (kernel variant)
  int pk = 0;            // packed column tile (few-chain plans, sht_gemm.hip: k_sht_gemm_pk): live columns per slab, 0 = off
  std::vector<char> tab_shared;  // packed lists: transform i streams its table together with transform i - 1 (one pass)
};

// launch order of a list: "xcd" (one queue per XCD), "bins" (one bin per CU) or anything else (descending work)
void order_tasks(std::vector<GemmTask>& v, const std::string& order);
// orders the tasks (PXM_GEMM_ORDER or by size), checks every address range their launches can form and uploads them
int upload_tasks(std::vector<GemmTask> v, bool paired, TaskList* out, std::vector<int> bls, int ncol, const double* ws_base,
                 const char* name, std::vector<int> los = {}, int pk = 0, std::vector<char> tab_shared = {});
// algorithmic bytes of one launch of a list for cg live chain slots
double tasklist_bytes(const TaskList& tl, int cg);
// run a task list over all chain groups (16 chains = 32 columns per launch)
int run_tasks(const TaskList& tl, const double* X, double* Y, int ncol, int C, hipStream_t st,
              const GemmAffine& aff = GemmAffine(), Profiler* prof = nullptr);
void free_tasks(TaskList* t);

}  // namespace pxm
