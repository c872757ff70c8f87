// GEMM task lists: static launch order, invariants, address-range check, upload and launch.
#include "tasklist.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>

namespace pxm {

// Static balance and operand locality.  The dispatcher deals workgroup i to XCD i % 8 and, inside an XCD,
// to whichever CU has a free slot, in id order: the ids congruent to x (mod 8) are XCD x's queue, served
// longest-first if the queue is in descending order (greedy LPT over its 32 CUs x 4 slots).
// Which of the two orders applies depends on the regime: up to ~2 workgroups per slot (256 CUs x 4) the launch is
// (almost) resident at once and the per-CU bins win (L=256: 24.5 vs 26.5 us Gram, 31.4 vs 32.1 us groups); with
// many rounds per slot the queues win (L=512: 200 vs 218 us, 218 vs 231 us).
// `fixed`: start-up / drain of a task in contraction steps
static int64_t task_work(const GemmTask& a, int64_t fixed) { return (int64_t)(a.k_end - a.k_beg + fixed) * a.n_rt; }

// "xcd".  Tasks that read the same operand slab (same x_off: the row groups of one m, and for the harmonic-side lists
// every scale of that m) form a unit that stays together in ONE queue, back to back, so the slab is fetched into that
// XCD's L2 once (PMC at L=512: 1.27x -> see DESIGN.md section 9).  Units go to the lightest queue, longest first;
// queues are padded to equal length with empty tasks (n_rt = 0: the workgroup exits at once).
static void order_xcd(std::vector<GemmTask>& v, int64_t fixed) {
  constexpr int NQ = 8;  // XCDs of gfx950
  std::map<int64_t, int> unit_of;
  std::vector<std::vector<GemmTask>> units;
  for (const GemmTask& t : v) {  // (v is in descending order: so is every unit)
    auto it = unit_of.find(t.x_off[0]);
    if (it == unit_of.end()) {
      it = unit_of.emplace(t.x_off[0], (int)units.size()).first;
      units.emplace_back();
    }
    units[it->second].push_back(t);
  }
  std::vector<int64_t> uw(units.size(), 0);
  std::vector<int> idx(units.size());
  for (size_t u = 0; u < units.size(); ++u) {
    idx[u] = (int)u;
    for (const GemmTask& t : units[u]) uw[u] += task_work(t, fixed);
  }
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return uw[a] > uw[b]; });
  std::vector<std::vector<GemmTask>> q(NQ);
  int64_t load[NQ] = {0};
  for (int u : idx) {
    int best = 0;
    for (int x = 1; x < NQ; ++x)
      if (load[x] < load[best] || (load[x] == load[best] && q[x].size() < q[best].size())) best = x;
    q[best].insert(q[best].end(), units[u].begin(), units[u].end());
    load[best] += uw[u];
  }
  size_t len = 0;
  for (int x = 0; x < NQ; ++x) len = std::max(len, q[x].size());
  GemmTask empty;
  memset(&empty, 0, sizeof(empty));
  std::vector<GemmTask> ordered;
  ordered.reserve(len * NQ);
  for (size_t r = 0; r < len; ++r)
    for (int x = 0; x < NQ; ++x) ordered.push_back(r < q[x].size() ? q[x][r] : empty);
  while (!ordered.empty() && ordered.back().n_rt == 0) ordered.pop_back();  // (trailing padding is not needed)
  v.swap(ordered);
}

// "bins": LPT over one bin per CU, emitted round by round -- workgroup r*256 + b lands on XCD b % 8, CU (b / 8) % 32
static void order_bins(std::vector<GemmTask>& v, int64_t fixed) {
  int nbins = 256;
  hipDeviceProp_t prop;
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
    nbins = prop.multiProcessorCount;
  std::vector<std::vector<GemmTask>> bins(nbins);
  std::vector<int64_t> load(nbins, 0);
  for (const GemmTask& t : v) {
    int best = 0;
    for (int b = 1; b < nbins; ++b)
      if (load[b] < load[best] || (load[b] == load[best] && bins[b].size() < bins[best].size())) best = b;
    bins[best].push_back(t);
    load[best] += task_work(t, fixed);
  }
  std::vector<GemmTask> ordered;
  ordered.reserve(v.size());
  for (size_t r = 0;; ++r) {
    bool any = false;
    for (int b = 0; b < nbins; ++b)
      if (r < bins[b].size()) {
        ordered.push_back(bins[b][r]);
        any = true;
      }
    if (!any) break;
  }
  v.swap(ordered);
}

// fixed cost the orders balance with, in contraction steps.  The per-CU bins ran on work alone (0) until the longest chain of
// the Gram list was halved; with it the headline iteration is 1.3 - 2.5 us shorter (docs/EXPERIMENTS.md, Round 8).  A
// build-time knob for A/B runs.
#ifndef PXM_BINS_FIXED_STEPS
#define PXM_BINS_FIXED_STEPS GEMM_TASK_FIXED_STEPS
#endif
void order_tasks(std::vector<GemmTask>& v, const std::string& order) {
  const int64_t fixed = order == "xcd" ? GEMM_TASK_FIXED_STEPS : PXM_BINS_FIXED_STEPS;
  std::stable_sort(v.begin(), v.end(), [&](const GemmTask& a, const GemmTask& b) { return task_work(a, fixed) > task_work(b, fixed); });
  if (order == "xcd" && !v.empty()) order_xcd(v, fixed);
  else if (order == "bins" && (int)v.size() > 256) order_bins(v, fixed);  // (any other word, e.g. plain: descending)
}

int upload_tasks(std::vector<GemmTask> v, bool paired, TaskList* out, std::vector<int> bls, int ncol, const double* ws_base,
                 const char* name, std::vector<int> los, int pk, std::vector<char> tab_shared) {
  tab_shared.resize(bls.size(), 0);
  los.resize(bls.size(), 0);
  out->pk = pk;
  out->tab_shared = tab_shared;
  out->bls = bls;
  out->los = los;
  const char* order_env = getenv("PXM_GEMM_ORDER");  // xcd | bins | plain forces one order
  order_tasks(v, order_env ? order_env : (v.size() > 2048 ? "xcd" : "bins"));
  out->n = (int)v.size();
  out->paired = paired;
  out->nslab = pk ? 4 : (paired ? 2 : 1);
  for (const GemmTask& t : v) {
    // shape invariants the kernel relies on (its clamped prefetches stay inside the task's own rows and chunks)
    PXM_REQUIRE(t.n_rt >= 0 && t.n_rt <= 8 && t.row0 >= 0 && t.row0 % 16 == 0 && t.k_beg >= 0 && t.k_beg % 16 == 0 &&
                    (t.n_rt == 0 || (t.k_end > t.k_beg && (t.k_end - t.k_beg) % 16 == 0)),
                "upload_tasks: malformed GEMM task");
    out->mfma_units += (double)t.n_rt * ((t.k_end - t.k_beg) / 4) * (pk ? 1 : t.nslab);  // (packed: one column tile per task)
    for (int sl = 0; sl < 4; ++sl)
      if (t.x2_off[sl]) out->flags |= 1;
    if (t.ks_off[0] || t.ks_off[1]) out->flags |= 2;
    if (t.pole_n) out->flags |= 4;
  }
  // only the packed and the two-operand kernels take a task's own row pitch (sht_gemm.hip: xn / yn)
  if (!pk && !(out->flags & 1))
    for (const GemmTask& t : v)
      PXM_REQUIRE(t.n_rt == 0 || (t.x_ncol == ncol && t.y_ncol == ncol), "upload_tasks: a streaming list with a row pitch of its own");
  if (v.empty()) return 0;
  // address ranges of every load / store the launches of this list can form (sht_gemm.hip: check_gemm_task_ranges)
  if (int rc = check_gemm_task_ranges(v, out->nslab, out->flags, ncol, ws_base, name)) return rc;
  if (int rc = dev_alloc(&out->d, v.size() * sizeof(GemmTask), "GEMM task list")) return rc;
  return dev_upload(out->d, v.data(), v.size() * sizeof(GemmTask));
}

double tasklist_bytes(const TaskList& tl, int cg) {
  double bytes = 0;
  for (size_t i = 0; i < tl.bls.size(); ++i) {
    const double Ld = tl.bls[i];
    // Gram launch: the table as stored; the operand is the sum of the TWO class buffers (both read), one result
    // array, (l, m) entries with l >= |m| only (16 B each: L^2 per array and chain slot), and the data term of chain 0
    // (gram_stream_bytes: what the launch reads of the stored table, plus the operand rows and pole columns that the
    // order-0 halves read for their pole term -- 2 L rows of both class buffers, 2 L entries of b twice)
    if (tl.gram) bytes += (tl.gram_pole ? tl.gram_stream_bytes + 2 * 2 * 16.0 * cg * Ld + 2 * 2 * 8.0 * Ld : tl.gram_table_bytes) +
                          3 * 16.0 * cg * Ld * Ld + 16.0 * Ld * Ld;
    else bytes += gemm_alg_bytes(tl.bls[i], tl.paired, cg, tl.los[i]);
    // a transform that rides on the previous one's pass over the table (packed pair: the support cut of the pass is the
    // smaller of the two, i.e. the previous entry's -- scales are listed coarse to fine)
    if (!tl.gram && tl.pk && tl.tab_shared[i]) bytes -= gemm_table_bytes(tl.bls[i], tl.paired, tl.los[i]);
  }
  return bytes;
}

int run_tasks(const TaskList& tl, const double* X, double* Y, int ncol, int C, hipStream_t st, const GemmAffine& aff,
              Profiler* prof) {
  note_stream(st);
  if (tl.pk)  // few-chain plan: one launch, the live columns of every slab packed into one column tile
    return launch_gemm_packed(tl.d, tl.n, tl.pk, tl.flags, X, Y, ncol, 0, tasklist_bytes(tl, C), tl.mfma_units * 2048.0, st, prof);
  for (int col0 = 0; col0 < ncol; col0 += 32) {
    const int ct = (ncol - col0 >= 32) ? 2 : 1;
    const int cg = std::max(0, std::min(C - col0 / 2, 8 * ct));  // live chains in this column group
    if (cg == 0) break;  // column groups of padding chains only: nothing reads them
    const double bytes = tasklist_bytes(tl, cg);
    GemmAffine a = aff;
    if (col0) a.bump = nullptr;  // the iteration counter advances once per call, not once per column group
    a.ncol_live = 2 * C;
    int rc = launch_gemm(tl.d, tl.n, tl.nslab, tl.flags, X, Y, ncol, col0, ct, bytes, tl.mfma_units * ct * 2048.0, st, a, prof);
    if (rc) return rc;
  }
  return 0;
}

void free_tasks(TaskList* t) {
  if (t->d) deferred_free(t->d);
  t->d = nullptr;
}

}  // namespace pxm
