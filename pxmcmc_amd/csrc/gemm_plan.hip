// The ring-GEMM stage as a plan of its own (ring tables, one workspace and ONE task list: no DFT stage, no wavelet kernels,
// no samplers).  The list is built by append_gemm_tasks / append_gemm_tasks_packed, uploaded by upload_tasks and run by
// run_tasks -- the code every other plan uses -- on arrays the caller fills and reads through the plan, so that the
// kernels of sht_gemm.hip can be held to a model of the contraction alone (tests/test_gemm_host.py, tests/test_gpu_gemm.py).
#include "plan_common.h"

#include <algorithm>
#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

using namespace pxm;

namespace {
constexpr int SIDE_INTS = PXM_GEMM_SIDE_INTS;

struct Side {  // one transform's stage as the caller described it, and where its arrays sit in the workspace
  int kind = 0, bl = 0, Lh = 0, two = 0, ks = 0, rs = 0, row_lo = 0, row_hi = 0, el_lo = 0, hd = 0, x_ncol = 0, y_ncol = 0;
  int x_share = -1, y_share = -1;
  ShtTables* T = nullptr;
  int xL = 0, xRp = 0, xn = 0, yL = 0, yRp = 0, yn = 0;
  int64_t off_x = -1, off_x2 = -1, off_y = -1, off_ks = -1, off_rs = -1, off_hd = -1, n_x = 0, n_y = 0;
};
}  // namespace

struct pxm_gemm_plan_s {
  int spin = 0, Cmax = 0, Cp = 0, ncol = 0, pk = 0;
  std::vector<Side> sides;
  std::vector<ShtTables*> held;
  double* ws = nullptr;
  int64_t ws_doubles = 0, off_counter = 0, off_scratch = 0, scratch_doubles = 0;
  TaskList tl;
  std::vector<GemmTask> ordered;             // the list in launch order, padding entries included
  std::vector<std::array<int, 2>> task_side;  // per ordered task: its side (group 0), the second side of a packed pair or -1
};

static GemmSide gemm_side(const pxm_gemm_plan_s* p, const Side& s) {
  GemmSide g;
  g.x_base = s.off_x; g.y_base = s.off_y;
  g.x_L = s.xL; g.x_Rp = s.xRp; g.y_L = s.yL; g.y_Rp = s.yRp;
  g.kscale = s.ks ? p->ws + s.off_ks : nullptr;
  g.el_lo = s.el_lo;
  g.fuse = GemmFuse();
  if (s.two) g.fuse.x2_base = s.off_x2;
  if (s.rs) g.fuse.rscale = p->ws + s.off_rs;
  if (s.row_hi > 0) { g.fuse.row_lo = s.row_lo; g.fuse.row_hi = s.row_hi; }
  if (s.hd) { g.fuse.hd_base = s.off_hd; g.fuse.hd_stride = 2; }
  g.x_ncol = s.x_ncol; g.y_ncol = s.y_ncol;
  return g;
}

static int gemm_plan_create_impl(int spin, int max_chains, int pk, const int* desc, int n_sides, pxm_gemm_plan_t* plan) {
  const std::string fn("pxm_gemm_plan_create");
  PXM_REQUIRE(plan && desc, fn + ": null argument");
  PXM_REQUIRE(max_chains >= 1, fn + ": max_chains must be >= 1");
  PXM_REQUIRE(n_sides >= 1 && n_sides <= 64, fn + ": between 1 and 64 sides");
  PXM_REQUIRE(pk == 0 || pk == 2 || pk == 4, fn + ": pk must be 0 (unpacked), 2 or 4");
  PXM_REQUIRE(!pk || n_sides <= 2, fn + ": a packed list is one side or a pair of sides");
  PXM_REQUIRE(dry_run() || pxm_device_count() > 0, fn + ": no HIP device visible (the HIP path is the only path)");
  drain_deferred();
  std::unique_ptr<pxm_gemm_plan_s, int (*)(pxm_gemm_plan_t)> guard(new pxm_gemm_plan_s(), pxm_gemm_plan_destroy);
  pxm_gemm_plan_s* p = guard.get();
  p->spin = spin;
  p->Cmax = max_chains;
  p->Cp = round_up(max_chains, 8);
  p->ncol = 2 * p->Cp;
  p->pk = pk;
  PXM_REQUIRE(!pk || pk >= 2 * max_chains, fn + ": a packed list carries pk / 2 chains at the most");
  p->sides.resize(n_sides);
  int rc;
  // offset 0 is "none" for every optional array of a task: the counter block sits there
  int64_t w = 16;
  p->off_counter = 0;
  int rp_max = 16;
  for (int i = 0; i < n_sides; ++i) {
    Side& s = p->sides[i];
    const int* d = desc + (size_t)i * SIDE_INTS;
    s.kind = d[0]; s.bl = d[1]; s.Lh = d[2] ? d[2] : d[1];
    s.two = d[3] != 0; s.ks = d[4] != 0; s.rs = d[5] != 0;
    s.row_lo = d[6]; s.row_hi = d[7]; s.el_lo = d[8]; s.hd = d[9] != 0;
    s.x_ncol = d[10]; s.y_ncol = d[11]; s.x_share = d[12]; s.y_share = d[13];
    PXM_REQUIRE(s.kind >= 0 && s.kind < TAB_KINDS, fn + ": table kind outside [0, 7)");
    PXM_REQUIRE(s.bl >= 1 && std::abs(spin) < std::max(s.bl, 2) && s.Lh >= s.bl, fn + ": need |spin| < bl <= bandlimit of the harmonic side");
    PXM_REQUIRE(s.el_lo >= 0 && s.row_lo >= 0, fn + ": negative support cut or row mask");
    PXM_REQUIRE(s.x_share < i && s.y_share < i && s.x_share >= -1 && s.y_share >= -1, fn + ": a side shares arrays of an earlier side only");
    for (int nc : {s.x_ncol, s.y_ncol})
      PXM_REQUIRE(nc == 0 || (pk && nc >= pk && nc <= p->ncol && nc % 2 == 0), fn + ": a row pitch of its own needs a packed list and pk <= pitch <= ncol");
    {
      DftGeometry g;  // (the bandlimits every other plan refuses are refused here too)
      if ((rc = dft_geometry(s.Lh, &g))) return rc;
    }
    if ((rc = get_tables(s.bl, spin, 1u << s.kind, &s.T))) return rc;
    if (std::find(p->held.begin(), p->held.end(), s.T) == p->held.end()) {
      retain_tables(s.T);
      p->held.push_back(s.T);
    }
    const int Rb = round_up(s.bl, 16), Rh = round_up(s.Lh, 16);
    rp_max = std::max(rp_max, Rh);
    const bool x_harm = kind_k_is_el(s.kind), y_harm = kind_rows_are_el(s.kind);
    s.xL = x_harm ? s.Lh : s.bl; s.xRp = x_harm ? Rh : Rb;
    s.yL = y_harm ? s.Lh : s.bl; s.yRp = y_harm ? Rh : Rb;
    s.xn = s.x_ncol ? s.x_ncol : p->ncol;
    s.yn = s.y_ncol ? s.y_ncol : p->ncol;
    s.n_x = (int64_t)(2 * s.xL - 1) * s.xRp * s.xn;
    s.n_y = (int64_t)(2 * s.yL - 1) * s.yRp * s.yn;
    if (s.x_share >= 0) {
      const Side& o = p->sides[s.x_share];
      PXM_REQUIRE(o.xL == s.xL && o.xn == s.xn && o.two == s.two, fn + ": a shared operand array of another shape");
      s.off_x = o.off_x; s.off_x2 = o.off_x2;
    } else {
      s.off_x = w; w += s.n_x;
      if (s.two) { s.off_x2 = w; w += s.n_x; }
    }
    if (s.y_share >= 0) {
      const Side& o = p->sides[s.y_share];
      PXM_REQUIRE(o.yL == s.yL && o.yn == s.yn && o.hd == s.hd, fn + ": a shared result array of another shape");
      s.off_y = o.off_y; s.off_hd = o.off_hd;
    } else {
      s.off_y = w; w += s.n_y;
      if (s.hd) { s.off_hd = w; w += (int64_t)(2 * s.yL - 1) * s.yRp * 2; }
    }
    if (s.ks) { s.off_ks = w; w += s.xRp; }
    if (s.rs) { s.off_rs = w; w += s.yRp; }
  }
  p->off_scratch = w;
  p->scratch_doubles = (int64_t)rp_max * p->ncol;
  w += p->scratch_doubles;
  p->ws_doubles = w;
  if ((rc = dev_alloc(&p->ws, (size_t)w * sizeof(double), "GEMM plan workspace"))) return rc;
  if ((rc = dev_zero(p->ws, (size_t)w * sizeof(double)))) return rc;
  // the list: the sides appended in order (all-scales lists of the wavelet plan), or one packed side / pair
  std::vector<GemmTask> v;
  std::vector<int> bls, los;
  std::vector<char> shared(n_sides, 0);
  std::map<std::tuple<int64_t, int64_t, int64_t, int>, std::array<int, 2>> side_of;
  auto tag = [&](size_t first, int a, int b) {
    for (size_t t = first; t < v.size(); ++t) side_of[std::make_tuple(v[t].tab_off, v[t].x_off[0], v[t].y_off[0], v[t].row0)] = {a, b};
  };
  for (const Side& s : p->sides) {
    bls.push_back(s.bl);
    los.push_back(s.el_lo);
  }
  if (pk) {
    const Side& a = p->sides[0];
    const GemmSide ga = gemm_side(p, a);
    if (n_sides == 2) {
      const Side& b = p->sides[1];
      PXM_REQUIRE(a.T == b.T && a.kind == b.kind, fn + ": the two sides of a packed pair share one table");
      PXM_REQUIRE(a.xn == b.xn && a.yn == b.yn, fn + ": the two sides of a packed pair have arrays of different row strides");
      const GemmSide gb = gemm_side(p, b);
      append_gemm_tasks_packed(*a.T, a.kind, p->ncol, ga, &gb, p->off_scratch, p->ws, v);
      shared[1] = 1;
      tag(0, 0, 1);
    } else {
      append_gemm_tasks_packed(*a.T, a.kind, p->ncol, ga, nullptr, p->off_scratch, p->ws, v);
      tag(0, 0, -1);
    }
  } else {
    for (int i = 0; i < n_sides; ++i) {
      const size_t first = v.size();
      append_gemm_tasks(*p->sides[i].T, p->sides[i].kind, p->ncol, gemm_side(p, p->sides[i]), p->off_scratch, p->ws, v);
      tag(first, i, -1);
    }
  }
  if ((rc = upload_tasks(v, spin == 0, &p->tl, bls, p->ncol, p->ws, "GEMM plan", los, pk, shared, &p->ordered))) return rc;
  if (n_sides == 1 && kind_is_gram(p->sides[0].kind)) tasklist_set_gram(&p->tl, *p->sides[0].T, p->sides[0].kind);
  for (const GemmTask& t : p->ordered) {
    auto it = side_of.find(std::make_tuple(t.tab_off, t.x_off[0], t.y_off[0], t.row0));
    p->task_side.push_back(t.n_rt && it != side_of.end() ? it->second : std::array<int, 2>{-1, -1});
  }
  *plan = guard.release();
  return 0;
}

// what: 0 the layout, 1 the uploaded list, 2 the table bookkeeping of `side`.  Returns the number of words of the report;
// writes them where cap allows it
static int64_t gemm_plan_report(const pxm_gemm_plan_s* p, int what, int side, int64_t* out, int64_t cap) {
  std::vector<int64_t> r;
  if (what == 0) {
    r = {p->ncol, (int64_t)p->sides.size(), (int64_t)p->ordered.size(), p->tl.flags, p->tl.nslab, p->pk, p->ws_doubles, p->off_scratch,
         p->scratch_doubles, p->off_counter, p->Cmax, p->spin == 0, 0, 0, 0, 0};
    for (const Side& s : p->sides)
      for (int64_t x : {s.off_x, s.off_x2, s.off_y, s.off_ks, s.off_rs, s.off_hd, (int64_t)s.xL, (int64_t)s.xRp, (int64_t)s.xn, (int64_t)s.yL,
                        (int64_t)s.yRp, (int64_t)s.yn, s.n_x, s.n_y, (int64_t)(s.T->bytes[s.kind] / sizeof(double)),
                        (int64_t)(s.kind == TAB_GRAM_SPLIT0 ? s.T->Rp : 0)})
        r.push_back(x);
  } else if (what == 1) {
    for (size_t i = 0; i < p->ordered.size(); ++i) {
      const GemmTask& t = p->ordered[i];
      const int sd = p->task_side[i][0];
      int par = -1, m = 0;
      if (sd >= 0) {
        const Side& s = p->sides[sd];
        m = s.T->paired ? t.m_unit : t.m_unit - (s.T->L - 1);
        // a parity half of the split Gram list walks its planes two rows at a time: which half, from where it starts
        if (t.x_ncol == 2 * s.xn) par = (int)(((t.x_off[0] - s.off_x) / s.xn) & 1);
      }
      for (int64_t x : {(int64_t)t.m_unit, (int64_t)t.row0, (int64_t)t.n_rt, (int64_t)t.k_beg, (int64_t)t.k_end, (int64_t)t.pole_n,
                        (int64_t)t.nslab, (int64_t)sd, (int64_t)par, (int64_t)t.row_lo[0], (int64_t)t.row_hi[0], (int64_t)t.row_lo[1],
                        (int64_t)t.row_hi[1], (int64_t)t.sign1, (int64_t)p->task_side[i][1], (int64_t)m})
        r.push_back(x);
    }
  } else {
    const Side& s = p->sides[side];
    const ShtTables& T = *s.T;
    r = {T.n_m, T.Rp, T.paired, (int64_t)(T.bytes[s.kind] / sizeof(double)), s.kind == TAB_GRAM_SPLIT0 ? T.Rp : 0, T.L, T.spin, s.kind};
    for (int i = 0; i < T.n_m; ++i) {
      const bool split = kind_is_gram_split(s.kind);
      for (int64_t x : {(int64_t)T.m_of(i), T.m_off[s.kind][i], (int64_t)T.k_beg[s.kind][i], split ? T.odd_off[i] : (int64_t)-1,
                        split ? (int64_t)T.odd_k_beg[i] : (int64_t)0})
        r.push_back(x);
    }
  }
  if (out)
    for (int64_t i = 0; i < std::min<int64_t>(cap, (int64_t)r.size()); ++i) out[i] = r[i];
  return (int64_t)r.size();
}

extern "C" {

int pxm_gemm_plan_create(int spin, int max_chains, int pk, const int* sides, int n_sides, pxm_gemm_plan_t* plan) {
  return gemm_plan_create_impl(spin, max_chains, pk, sides, n_sides, plan);
}

int pxm_gemm_plan_destroy(pxm_gemm_plan_t p) {
  if (!p) return 0;
  deferred_free(p->ws);
  free_tasks(&p->tl);
  for (ShtTables* T : p->held) release_tables(T);
  delete p;
  drain_deferred();  // (a no-op while a stream capture is in progress: freed at the next safe point)
  return 0;
}

int64_t pxm_gemm_plan_report(pxm_gemm_plan_t p, int what, int side, int64_t* out, int64_t cap) {
  PXM_REQUIRE(p, "pxm_gemm_plan_report: null plan");
  PXM_REQUIRE(what >= 0 && what <= 2, "pxm_gemm_plan_report: what must be 0 (layout), 1 (list) or 2 (table)");
  PXM_REQUIRE(what != 2 || (side >= 0 && side < (int)p->sides.size()), "pxm_gemm_plan_report: no such side");
  PXM_REQUIRE(cap >= 0 && (out || cap == 0), "pxm_gemm_plan_report: null output");
  return gemm_plan_report(p, what, side, out, cap);
}

int64_t pxm_host_gemm_plan_report(int spin, int max_chains, int pk, const int* sides, int n_sides, int what, int side,
                                  int64_t* out, int64_t cap) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  PXM_REQUIRE(!capture_in_progress(), "pxm_host_gemm_plan_report: not during a stream capture");
  set_dry_run(true);
  pxm_gemm_plan_t p = nullptr;
  int64_t rc = pxm_gemm_plan_create(spin, max_chains, pk, sides, n_sides, &p);
  if (!rc) rc = pxm_gemm_plan_report(p, what, side, out, cap);
  if (p) pxm_gemm_plan_destroy(p);
  tables_trim();  // the dry-run table entries (fake addresses) never outlive the call
  set_dry_run(false);
  return rc;
}

int pxm_gemm_plan_write(pxm_gemm_plan_t p, int64_t offset, const double* src, int64_t n, pxm_stream_t s) {
  PXM_REQUIRE(p && src, "pxm_gemm_plan_write: null argument");
  PXM_REQUIRE(offset >= 0 && n >= 0 && offset <= p->ws_doubles && n <= p->ws_doubles - offset, "pxm_gemm_plan_write: range outside the workspace");
  note_stream((hipStream_t)s);
  PXM_HIP(hipMemcpyAsync(p->ws + offset, src, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)s));
  return 0;
}

int pxm_gemm_plan_read(pxm_gemm_plan_t p, int64_t offset, double* dst, int64_t n, pxm_stream_t s) {
  PXM_REQUIRE(p && dst, "pxm_gemm_plan_read: null argument");
  PXM_REQUIRE(offset >= 0 && n >= 0 && offset <= p->ws_doubles && n <= p->ws_doubles - offset, "pxm_gemm_plan_read: range outside the workspace");
  note_stream((hipStream_t)s);
  PXM_HIP(hipMemcpyAsync(dst, p->ws + offset, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)s));
  return 0;
}

int pxm_gemm_plan_table_read(pxm_gemm_plan_t p, int side, int which, double* dst, int64_t n, pxm_stream_t s) {
  PXM_REQUIRE(p && dst, "pxm_gemm_plan_table_read: null argument");
  PXM_REQUIRE(side >= 0 && side < (int)p->sides.size(), "pxm_gemm_plan_table_read: no such side");
  PXM_REQUIRE(which == 0 || which == 1, "pxm_gemm_plan_table_read: which must be 0 (the tiled table) or 1 (the pole column)");
  const Side& sd = p->sides[side];
  const double* src = which ? sd.T->d_pole : sd.T->d_tab[sd.kind];
  const int64_t have = which ? (sd.kind == TAB_GRAM_SPLIT0 ? sd.T->Rp : 0) : (int64_t)(sd.T->bytes[sd.kind] / sizeof(double));
  PXM_REQUIRE(src && n >= 0 && n <= have, "pxm_gemm_plan_table_read: more doubles than the table has");
  note_stream((hipStream_t)s);
  PXM_HIP(hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)s));
  return 0;
}

int pxm_gemm_plan_run(pxm_gemm_plan_t p, int C, int affine, double ns, double wr, double wi, int bump, pxm_stream_t s) {
  PXM_REQUIRE(p, "pxm_gemm_plan_run: null plan");
  PXM_REQUIRE(C >= 1 && C <= p->Cmax, "pxm_gemm_plan_run: C outside [1, max_chains]");
  PXM_REQUIRE(!p->pk || !(affine || bump), "pxm_gemm_plan_run: the packed kernels have no affine epilogue and no counter");
  GemmAffine aff;
  if (affine) {
    aff.on = 1;
    aff.ns = ns;
    aff.wr = wr;
    aff.wi = wi;
  }
  if (bump) aff.bump = reinterpret_cast<uint64_t*>(p->ws + p->off_counter);
  return run_tasks(p->tl, p->ws, p->ws, p->ncol, C, (hipStream_t)s, aff);
}

}  // extern "C"
