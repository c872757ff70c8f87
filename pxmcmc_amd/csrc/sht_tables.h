// Ring tables of the Legendre stage (sht_tables.hip): kinds, layout bookkeeping and the per-device cache.
#pragma once
#include "sht_core.h"

namespace pxm {

// TAB_GRAM: (B^m)^T B^m, el <- el: the inverse transform followed by its adjoint in one contraction
// (normal equations of the ring-space MYULA step)
// TAB_GRAM_SPLIT: the same matrix for spin 0 and Rp % 32 == 0, stored without its structurally zero half.  For m >= 1
// the entries G^m[l][l'] with l + l' odd vanish, so order m is kept as two half-size dense
// matrices G_p[i][j] = G^m[2i + p][2j + p], p = 0 (even degrees) and 1 (odd degrees), each tiled like any other table
// from kb_p = round_down(ceil((m - p) / 2), 16).  m = 0 has a real odd-parity part (the pole ring) and stays dense.
// An order stays one dense block where the two halves would not be cheaper (gram_order_splits below): the halves cannot
// go below one 16 x 16 tile, and each is a workgroup with a start-up and a drain of its own.
// TAB_GRAM_SPLIT0: TAB_GRAM_SPLIT with order 0 split as well.  The odd-parity part of G^0 is the pole ring alone and has
// rank one: G^0[l][l'] = 1/2 b_l b_l' for l + l' odd, b_l = B^0[theta = pi][l].  Order 0 is stored as
// the parity-permuted matrix [[ee, eo], [oe, oo]] (Rp^2 doubles, as before); its two half tasks stream the diagonal blocks
// and add 1/2 b_row (b_other . x_other) in their epilogue (GemmTask::pole_n), the off-diagonal blocks are never read.
enum TableKind { TAB_INV = 0, TAB_FWD = 1, TAB_INV_ADJ = 2, TAB_FWD_ADJ = 3, TAB_GRAM = 4, TAB_GRAM_SPLIT = 5, TAB_GRAM_SPLIT0 = 6, TAB_KINDS = 7 };
inline bool kind_el_to_ring(int kind) { return kind == TAB_INV || kind == TAB_FWD_ADJ; }
inline bool kind_is_gram_split(int kind) { return kind == TAB_GRAM_SPLIT || kind == TAB_GRAM_SPLIT0; }
inline bool kind_is_gram(int kind) { return kind == TAB_GRAM || kind_is_gram_split(kind); }
inline bool kind_rows_are_el(int kind) { return kind == TAB_FWD || kind == TAB_INV_ADJ || kind_is_gram(kind); }
inline bool kind_k_is_el(int kind) { return kind == TAB_INV || kind == TAB_FWD_ADJ || kind_is_gram(kind); }

struct ShtTables {
  int L = 0, spin = 0, Rp = 0;
  bool paired = false;           // spin 0: only m >= 0 stored, -m served with sign (-1)^m
  int n_m = 0;                   // stored m count
  double* d_tab[TAB_KINDS] = {};
  size_t bytes[TAB_KINDS] = {};
  std::vector<int64_t> m_off[TAB_KINDS];  // per stored-m offset (doubles) into d_tab[kind]
  std::vector<int> k_beg[TAB_KINDS];      // per stored-m contraction start (el->ring kinds) / first row tile*16 (ring->el)
  // TAB_GRAM_SPLIT, orders stored as halves: the odd-degree half (m_off / k_beg above describe the even-degree half, in
  // half-row units); odd_off < 0: the order is stored dense (m = 0, and the orders gram_order_splits turns down)
  std::vector<int64_t> odd_off;
  std::vector<int> odd_k_beg;
  // TAB_GRAM_SPLIT0: b_l = B^0[theta = pi][l] by parity, [Rp / 2 even degrees | Rp / 2 odd degrees], zero for l >= L
  double* d_pole = nullptr;
  int refs = 0;                           // plans holding this entry of the per-device cache
  int m_of(int i) const { return paired ? i : i - (L - 1); }
};

// can the Gram matrix of these tables be stored split by degree parity (TAB_GRAM_SPLIT, TAB_GRAM_SPLIT0)?
inline bool gram_can_split(const ShtTables& T) { return T.paired && T.Rp % 32 == 0; }
// first half-row of the parity-par half of order m, down to a tile: the first i with 2 i + par >= m
inline int gram_half_k_beg(int m, int par) { return round_down((m - par + 1) / 2, 16); }
// Is order m >= 1 cheaper as two halves than as one dense block?  Modelled work of a block of extent n from kb on: row
// tiles x (contraction steps + the fixed cost of a task).  The halves win wherever they halve the block; they lose in
// the last 16 orders (a one-tile block would become two) and where two tiles per half replace a 3 x 3 tile block.
inline bool gram_order_splits(int Rp, int m) {
  auto work = [](int n, int kb) { return (n - kb) / 16 * (n - kb + GEMM_TASK_FIXED_STEPS); };
  return work(Rp / 2, gram_half_k_beg(m, 0)) + work(Rp / 2, gram_half_k_beg(m, 1)) < work(Rp, round_down(m, 16));
}

// builds (or returns cached) tables for (L, spin); kinds_mask selects which kinds to build.  The cache is
// per device and shared by plans: a plan retains every entry it uses once and releases it at teardown;
// tables_trim() frees the entries nobody holds (pxm_tables_trim).
int get_tables(int L, int spin, unsigned kinds_mask, ShtTables** out);
void retain_tables(ShtTables* T);
void release_tables(ShtTables* T);
int64_t tables_trim();  // returns the bytes released

}  // namespace pxm
