// GEMM task lists: construction, static launch order, invariants, address-range check, upload and launch.
#include "tasklist.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>

namespace pxm {

// ---- construction ----------------------------------------------------------------------
// slabs 2g, 2g+1 of task g <- one transform (side): operand / output slab offsets for +m / -m, scales, row mask
static void fill_side(GemmTask& g, int grp, const ShtTables& T, int m, int ncol, const GemmSide& sd,
                      int64_t scratch_off, const double* ws_base) {
  const int s0 = 2 * grp, s1 = 2 * grp + 1;
  const int xn = sd.x_ncol ? sd.x_ncol : ncol, yn = sd.y_ncol ? sd.y_ncol : ncol;  // doubles per row of the two arrays
  g.x_off[s0] = sd.x_base + (int64_t)(m + sd.x_L - 1) * sd.x_Rp * xn;
  g.y_off[s0] = sd.y_base + (int64_t)(m + sd.y_L - 1) * sd.y_Rp * yn;
  if (T.paired) {
    if (m == 0) {
      g.x_off[s1] = g.x_off[s0];
      g.y_off[s1] = scratch_off;
    } else {
      g.x_off[s1] = sd.x_base + (int64_t)(-m + sd.x_L - 1) * sd.x_Rp * xn;
      g.y_off[s1] = sd.y_base + (int64_t)(-m + sd.y_L - 1) * sd.y_Rp * yn;
    }
  } else {
    g.x_off[s1] = g.x_off[s0];
    g.y_off[s1] = g.y_off[s0];
  }
  g.ks_off[grp] = sd.kscale ? (sd.kscale - ws_base) : 0;
  g.rs_off[grp] = sd.fuse.rscale ? (sd.fuse.rscale - ws_base) : 0;
  g.row_lo[grp] = sd.fuse.row_lo;
  g.row_hi[grp] = sd.fuse.row_hi;
  g.x2_off[s0] = g.x2_off[s1] = 0;
  if (sd.fuse.x2_base >= 0) {
    g.x2_off[s0] = sd.fuse.x2_base + (int64_t)(m + sd.x_L - 1) * sd.x_Rp * xn;
    g.x2_off[s1] = (T.paired && m != 0) ? sd.fuse.x2_base + (int64_t)(-m + sd.x_L - 1) * sd.x_Rp * xn : g.x2_off[s0];
  }
  g.hd_off[s0] = g.hd_off[s1] = 0;
  g.hd_stride = sd.fuse.hd_stride > 0 ? sd.fuse.hd_stride : ncol;
  if (sd.fuse.hd_base >= 0) {
    g.hd_off[s0] = sd.fuse.hd_base + (int64_t)(m + sd.y_L - 1) * sd.y_Rp * g.hd_stride;
    g.hd_off[s1] = (T.paired && m != 0) ? sd.fuse.hd_base + (int64_t)(-m + sd.y_L - 1) * sd.y_Rp * g.hd_stride : g.hd_off[s0];
  }
}

// The tasks of one table block of order m: `tab` its tiled table, kb its start along the el dimension(s), n the extent of
// its row and contraction dimensions.  par < 0: the block spans the order (n = Rp).  par = 0 / 1: a parity half of the
// split Gram table (n = Rp / 2) -- an ordinary task on a strided view of the H-layout arrays: a plane [Rp][ncol] of one
// order is also [Rp / 2][2 ncol], half-row r holding degree 2 r in columns 0 .. ncol - 1 and degree 2 r + 1 in columns
// ncol .. 2 ncol - 1, so the half of parity par has row pitch 2 ncol and starts par * ncol into the plane; rows,
// contraction steps and the row mask of the task count half-rows.  (Sides with a support cut or a row mask of their own
// have no such view: the Gram step has neither.)
static void append_block_tasks(const ShtTables& T, int kind, int ncol, const GemmSide& side, int64_t scratch_off,
                               const double* ws_base, std::vector<GemmTask>& tasks, int m, const double* tab, int kb, int n,
                               int par, int64_t rt_stride_stored = 0, const double* pole = nullptr) {
  // el_lo: harmonic degrees below it carry no signal for the transform (compact support of a wavelet kernel): the
  // rows (ring->el kinds) or contraction steps (el->ring kinds) below it are skipped.
  const bool rows_el = kind_rows_are_el(kind), k_el = kind_k_is_el(kind);
  const int lo16 = round_down(std::max(side.el_lo, 0), 16);
  const int rpt = GEMM_TASK_ROW_TILES;  // row tiles per task
  const int start = std::max(kb, lo16);
  if (start >= n) return;
  // table of this block: [row tiles from (rows_el ? kb : 0)][k chunks of 8 from (k_el ? kb : 0)]
  // (rt_stride_stored: the block is part of a wider stored matrix -- a diagonal block of the permuted order-0 table)
  const int64_t rt_stride = rt_stride_stored ? rt_stride_stored : (int64_t)((k_el ? n - kb : n) / 8) * 128;
  const int k_beg = k_el ? start : 0, k_end = n, row_beg = rows_el ? start : 0;
  const int64_t tab_skip = (rows_el ? (int64_t)((start - kb) / 16) * rt_stride : 0) + (k_el ? (int64_t)((start - kb) / 8) * 128 : 0);
  const int n_rt_total = (n - row_beg) / 16;
  for (int rt = 0; rt < n_rt_total; rt += rpt) {
    GemmTask g;
    g.m_unit = T.paired ? m : m + T.L - 1;
    g.tab_off = (tab + tab_skip + (int64_t)rt * rt_stride) - ws_base;
    g.rt_stride = rt_stride;
    for (int s = 0; s < 2; ++s) fill_side(g, s, T, m, ncol, side, scratch_off, ws_base);  // (slab groups 0 and 1 alike)
    g.nslab = T.paired ? 2 : 1;
    g.k_beg = k_beg;
    g.k_end = k_end;
    g.row0 = row_beg + 16 * rt;
    g.n_rt = std::min(rpt, n_rt_total - rt);
    g.sign1 = kind_is_gram(kind) ? 1.0 : ((m & 1) ? -1.0 : 1.0);  // the Gram table is even in m
    g.x_ncol = side.x_ncol ? side.x_ncol : ncol;
    g.y_ncol = side.y_ncol ? side.y_ncol : ncol;
    g.pole_n = g.pole_dx = 0;
    g.pole_b_off = g.pole_bo_off = 0;
    if (pole) {  // order-0 half: pole = [n even degrees | n odd degrees] of b
      g.pole_n = n;
      g.pole_dx = par ? -g.x_ncol : g.x_ncol;
      g.pole_b_off = (pole + par * n) - ws_base;
      g.pole_bo_off = (pole + (1 - par) * n) - ws_base;
    }
    if (par >= 0) {
      for (int s = 0; s < 4; ++s) {
        g.x_off[s] += par * g.x_ncol;
        g.y_off[s] += par * g.y_ncol;
        if (g.x2_off[s]) g.x2_off[s] += par * g.x_ncol;
        if (g.hd_off[s]) g.hd_off[s] += par * g.hd_stride;
      }
      g.x_ncol *= 2;
      g.y_ncol *= 2;
      g.hd_stride *= 2;
      // written rows: the degrees l >= round_down(m, 16) the dense list writes, no others (kb can start lower)
      for (int grp = 0; grp < 2; ++grp) g.row_lo[grp] = round_down(m, 16) / 2;
    }
    tasks.push_back(g);
  }
}

void append_gemm_tasks(const ShtTables& T, int kind, int ncol, const GemmSide& side, int64_t scratch_off,
                       const double* ws_base, std::vector<GemmTask>& tasks) {
  for (int i = 0; i < T.n_m; ++i) {
    const int m = T.m_of(i);
    const double* tab = T.d_tab[kind] + T.m_off[kind][i];
    const int kb = T.k_beg[kind][i];  // table start of this m along its el dimension(s): multiple of 16
    if (kind == TAB_GRAM_SPLIT0 && m == 0) {  // the diagonal blocks of [[ee, eo], [oe, oo]], each with its pole term
      const int Rh = T.Rp / 2;
      const int64_t rs = (int64_t)(T.Rp / 8) * 128;
      append_block_tasks(T, kind, ncol, side, scratch_off, ws_base, tasks, m, tab, 0, Rh, 0, rs, T.d_pole);
      append_block_tasks(T, kind, ncol, side, scratch_off, ws_base, tasks, m, tab + (Rh / 16) * rs + (int64_t)(Rh / 8) * 128, 0, Rh, 1, rs, T.d_pole);
    } else if (kind_is_gram_split(kind) && T.odd_off[i] >= 0) {  // even-degree half, odd-degree half
      append_block_tasks(T, kind, ncol, side, scratch_off, ws_base, tasks, m, tab, kb, T.Rp / 2, 0);
      append_block_tasks(T, kind, ncol, side, scratch_off, ws_base, tasks, m, T.d_tab[kind] + T.odd_off[i], T.odd_k_beg[i], T.Rp / 2, 1);
    } else {
      append_block_tasks(T, kind, ncol, side, scratch_off, ws_base, tasks, m, tab, kb, T.Rp, -1);
    }
  }
}

// Packed lists: the tasks of one transform (side_b == nullptr) or of TWO transforms at the same bandlimit that stream the table
// once (slabs 0, 1 = +-m of side_a, slabs 2, 3 = +-m of side_b).  The support cut of a pair is the smaller of the two: the
// row masks (ring->el kinds) / zero scale rows (el->ring kinds) of the transform with the narrower support do the rest.
void append_gemm_tasks_packed(const ShtTables& T, int kind, int ncol, const GemmSide& side_a, const GemmSide* side_b,
                              int64_t scratch_off, const double* ws_base, std::vector<GemmTask>& tasks) {
  GemmSide sa = side_a;
  if (side_b) sa.el_lo = std::min(side_a.el_lo, side_b->el_lo);
  const size_t first = tasks.size();
  append_gemm_tasks(T, kind, ncol, sa, scratch_off, ws_base, tasks);
  for (size_t i = first; i < tasks.size(); ++i) {
    GemmTask& g = tasks[i];
    const int m = T.paired ? g.m_unit : g.m_unit - (T.L - 1);
    fill_side(g, 0, T, m, ncol, side_a, scratch_off, ws_base);
    fill_side(g, 1, T, m, ncol, side_b ? *side_b : side_a, scratch_off, ws_base);
    g.nslab = side_b ? 4 : 2;
    g.x_ncol = side_a.x_ncol ? side_a.x_ncol : ncol;  // (the two transforms of a pair share the strides of their arrays)
    g.y_ncol = side_a.y_ncol ? side_a.y_ncol : ncol;
    if (!T.paired) {  // all m stored: one slab per transform -- slabs 0 (a) and 1 (b); the kernel's group index is slab >> 1,
      // so an unpaired packed list carries ONE transform per task
      g.nslab = 1;
    }
  }
}

// ---- launch order ----------------------------------------------------------------------
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
                 const char* name, std::vector<int> los, int pk, std::vector<char> tab_shared, std::vector<GemmTask>* ordered) {
  tab_shared.resize(bls.size(), 0);
  los.resize(bls.size(), 0);
  out->pk = pk;
  out->tab_shared = tab_shared;
  out->bls = bls;
  out->los = los;
  const char* order_env = getenv("PXM_GEMM_ORDER");  // xcd | bins | plain forces one order
  order_tasks(v, order_env ? order_env : (v.size() > 2048 ? "xcd" : "bins"));
  if (ordered) *ordered = v;
  out->n = (int)v.size();
  out->paired = paired;
  out->nslab = pk ? 4 : (paired ? 2 : 1);
  for (const GemmTask& t : v) {
    // shape invariants the kernel relies on (its clamped prefetches stay inside the task's own rows and chunks)
    PXM_REQUIRE(t.n_rt >= 0 && t.n_rt <= GEMM_TASK_ROW_TILES && t.row0 >= 0 && t.row0 % 16 == 0 && t.k_beg >= 0 && t.k_beg % 16 == 0 &&
                    (t.n_rt == 0 || (t.k_end > t.k_beg && (t.k_end - t.k_beg) % 16 == 0)),
                "upload_tasks: malformed GEMM task");
    out->mfma_units += (double)t.n_rt * ((t.k_end - t.k_beg) / 4) * (pk ? 1 : t.nslab);  // (packed: one column tile per task)
    for (int sl = 0; sl < 4; ++sl)
      if (t.x2_off[sl]) out->flags |= GEMM_LIST_TWO;
    if (t.ks_off[0] || t.ks_off[1]) out->flags |= GEMM_LIST_SCALE;
    if (t.pole_n) out->flags |= GEMM_LIST_POLE;
  }
  // only the packed and the two-operand kernels take a task's own row pitch (sht_gemm.hip: xn / yn)
  if (!pk && !(out->flags & GEMM_LIST_TWO))
    for (const GemmTask& t : v)
      PXM_REQUIRE(t.n_rt == 0 || (t.x_ncol == ncol && t.y_ncol == ncol), "upload_tasks: a streaming list with a row pitch of its own");
  if (v.empty()) return 0;
  // address ranges of every load / store the launches of this list can form (sht_gemm.hip: check_gemm_task_ranges)
  if (int rc = check_gemm_task_ranges(v, out->nslab, pk, out->flags, ncol, ws_base, name)) return rc;
  return dev_table(&out->d, v, "GEMM task list");
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

void tasklist_set_gram(TaskList* tl, const ShtTables& T, int kind) {
  tl->gram = true;
  tl->gram_table_bytes = (double)T.bytes[kind];
  tl->gram_pole = kind == TAB_GRAM_SPLIT0;
  tl->gram_stream_bytes = tl->gram_table_bytes - (tl->gram_pole ? 4.0 * T.Rp * T.Rp : 0.0);  // (two Rp/2 x Rp/2 blocks of doubles)
}

int run_tasks(const TaskList& tl, const double* X, double* Y, int ncol, int C, hipStream_t st, const GemmAffine& aff,
              Profiler* prof) {
  note_stream(st);
  if (tl.pk)  // few-chain plan: one launch, the live columns of every slab packed into one column tile
    return launch_gemm_packed(tl.d, tl.n, tl.pk, tl.flags, X, Y, ncol, 0, tasklist_bytes(tl, C), tl.mfma_units * 2048.0, st, prof);
  for (int col0 = 0; col0 < ncol; col0 += GEMM_GROUP_COLS) {
    const int ct = gemm_group_tiles(ncol, col0);
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
