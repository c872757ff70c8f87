// Ring tables of the Legendre stage: device-side construction in the tiled layout the GEMM kernel streams (sht_gemm.hip,
// DESIGN.md section 4) and the per-device table cache.  Setup time only.
#include "sht_tables.h"

#include <cstdlib>
#include <map>
#include <mutex>

namespace pxm {

// Ad[i][el][t] = scale * sum_t' Bd[i][t'][el] * Q[par(i)][t'][t]
__global__ void k_build_fwd(const double* __restrict__ Bd, const double* __restrict__ Qd, double* __restrict__ Ad,
                            int Rp, int L, double scale, int m0, int spin) {
  const int i = blockIdx.z;
  const int el = blockIdx.x * 16 + threadIdx.x, t = blockIdx.y * 16 + threadIdx.y;
  const int m = m0 + i;
  const int par = ((m + spin) & 1) ? 1 : 0;  // index 0 = even parity (+1), 1 = odd (-1)
  const double* B = Bd + (int64_t)i * Rp * Rp;
  const double* Q = Qd + (int64_t)par * Rp * Rp;
  double acc = 0;
  for (int tp = 0; tp < L; ++tp) acc += B[(int64_t)tp * Rp + el] * Q[(int64_t)tp * Rp + t];
  Ad[(int64_t)i * Rp * Rp + (int64_t)el * Rp + t] = scale * acc;
}

// Gd[i][r][c] = sum_t Bd[i][t][r] * Bd[i][t][c]   (the per-m Gram matrix of the inverse transform)
__global__ void k_build_gram(const double* __restrict__ Bd, double* __restrict__ Gd, int Rp, int L) {
  const int i = blockIdx.z;
  const int r = blockIdx.x * 16 + threadIdx.x, c = blockIdx.y * 16 + threadIdx.y;
  const double* B = Bd + (int64_t)i * Rp * Rp;
  double acc = 0;
  for (int t = 0; t < L; ++t) acc += B[(int64_t)t * Rp + r] * B[(int64_t)t * Rp + c];
  Gd[(int64_t)i * Rp * Rp + (int64_t)r * Rp + c] = acc;
}

// tiled[(rt, kk2, lane, h)] = D[row][k] (transposed = 0) or D[k][row] (transposed = 1), D = dense Rp x Rp.
// par = 0 / 1: the tiled matrix is the n = Rp / 2 parity half of D, entry [row][k] = D[2 row + par][2 k + par]
// par = 2: the whole of D with rows and columns permuted by parity, even degrees first: [[ee, eo], [oe, oo]]
__global__ void k_tile_table(const double* __restrict__ D, double* __restrict__ out, int Rp, int n, int row_beg,
                             int k_beg, int transposed, int par) {
  const int nk2 = (n - k_beg) / 8;
  const int rt = blockIdx.y;
  const int kk2 = blockIdx.x;
  const int lane = threadIdx.x >> 1, h = threadIdx.x & 1;
  int row = row_beg + 16 * rt + (lane & 15);
  int k = k_beg + 8 * kk2 + 4 * h + (lane >> 4);
  if (par == 2) {
    row = row < n / 2 ? 2 * row : 2 * (row - n / 2) + 1;
    k = k < n / 2 ? 2 * k : 2 * (k - n / 2) + 1;
  } else if (par >= 0) {
    row = 2 * row + par;
    k = 2 * k + par;
  }
  const double v = transposed ? D[(int64_t)k * Rp + row] : D[(int64_t)row * Rp + k];
  out[((int64_t)rt * nk2 + kk2) * 128 + threadIdx.x] = v;
}

static std::mutex g_tab_mutex;
static std::map<std::pair<int, int>, ShtTables*> g_tab_cache;

// TAB_GRAM_SPLIT: order 0 dense, the orders m >= 1 as their even-degree and odd-degree halves where that is the cheaper
// form (sht_tables.h), gathered from the dense Gram matrices d_G: the kept entries are the doubles the dense table holds.
// TAB_GRAM_SPLIT0: the same with order 0 permuted by parity (the same Rp^2 doubles in the same space) and the pole column b
static int build_gram_split(ShtTables& T, int kind, const double* d_G) {
  const int Rp = T.Rp, Rh = Rp / 2;
  PXM_REQUIRE(gram_can_split(T), "build_gram_split: the parity split needs spin-0 tables and Rp % 32 == 0");
  T.m_off[kind].assign(T.n_m, 0);
  T.k_beg[kind].assign(T.n_m, 0);
  T.odd_off.assign(T.n_m, -1);
  T.odd_k_beg.assign(T.n_m, 0);
  int64_t total = 0;
  for (int m = 0; m < T.n_m; ++m) {
    if (m == 0 || !gram_order_splits(Rp, m)) {  // dense block, as in TAB_GRAM
      const int kb = round_down(m, 16);
      T.k_beg[kind][m] = kb;
      T.m_off[kind][m] = total;
      total += (int64_t)((Rp - kb) / 16) * ((Rp - kb) / 8) * 128;
      continue;
    }
    for (int par = 0; par < 2; ++par) {
      const int kb = gram_half_k_beg(m, par);
      (par ? T.odd_k_beg[m] : T.k_beg[kind][m]) = kb;
      (par ? T.odd_off[m] : T.m_off[kind][m]) = total;
      total += (int64_t)((Rh - kb) / 16) * ((Rh - kb) / 8) * 128;
    }
  }
  T.bytes[kind] = (size_t)total * sizeof(double);
  if (int rc = dev_alloc(&T.d_tab[kind], T.bytes[kind], "ring table")) return rc;
  if (kind == TAB_GRAM_SPLIT0 && !T.d_pole) {
    if (int rc = dev_alloc(&T.d_pole, (size_t)Rp * sizeof(double), "pole column of the order-0 Gram block")) return rc;
    if (!dry_run()) {
      std::vector<double> B0((size_t)Rp * Rp, 0.0), b(Rp, 0.0);
      wigner_ring_table(T.L, 0, 0, B0.data(), Rp);  // the last ring is theta = pi
      for (int l = 0; l < T.L; ++l) b[(l & 1) * Rh + l / 2] = B0[(size_t)(T.L - 1) * Rp + l];
      if (int rc = dev_upload(T.d_pole, b.data(), b.size() * sizeof(double))) return rc;
    }
  }
  if (dry_run()) return 0;  // layout only: no GPU to tile the tables on
  for (int m = 0; m < T.n_m; ++m) {
    const double* src = d_G + (int64_t)m * Rp * Rp;
    if (T.odd_off[m] < 0) {
      const int kb = T.k_beg[kind][m];
      hipLaunchKernelGGL(k_tile_table, dim3((Rp - kb) / 8, (Rp - kb) / 16), dim3(128), 0, 0, src, T.d_tab[kind] + T.m_off[kind][m],
                         Rp, Rp, kb, kb, 0, (kind == TAB_GRAM_SPLIT0 && m == 0) ? 2 : -1);
      continue;
    }
    for (int par = 0; par < 2; ++par) {
      const int kb = par ? T.odd_k_beg[m] : T.k_beg[kind][m];
      hipLaunchKernelGGL(k_tile_table, dim3((Rh - kb) / 8, (Rh - kb) / 16), dim3(128), 0, 0, src,
                         T.d_tab[kind] + (par ? T.odd_off[m] : T.m_off[kind][m]), Rp, Rh, kb, kb, 0, par);
    }
  }
  PXM_HIP(hipGetLastError());
  return 0;
}

static int build_kind(ShtTables& T, int kind, const double* d_B, const double* d_A, const double* d_G) {
  if (kind_is_gram_split(kind)) return build_gram_split(T, kind, d_G);
  const int Rp = T.Rp;
  const bool rows_el = kind_rows_are_el(kind), k_el = kind_k_is_el(kind);
  T.m_off[kind].resize(T.n_m);
  T.k_beg[kind].resize(T.n_m);
  int64_t total = 0;
  for (int i = 0; i < T.n_m; ++i) {
    const int elmin = std::max(std::abs(T.m_of(i)), std::abs(T.spin));
    const int kb = round_down(elmin, 16);  // contraction runs in 16-k chunks, output row tiles are 16 rows
    T.k_beg[kind][i] = kb;
    T.m_off[kind][i] = total;
    total += (int64_t)((rows_el ? Rp - kb : Rp) / 16) * ((k_el ? Rp - kb : Rp) / 8) * 128;
  }
  T.bytes[kind] = (size_t)total * sizeof(double);
  if (int rc = dev_alloc(&T.d_tab[kind], T.bytes[kind], "ring table")) return rc;
  if (dry_run()) return 0;  // layout only: no GPU to tile the tables on
  for (int i = 0; i < T.n_m; ++i) {
    const int kb = T.k_beg[kind][i];
    const double* src;
    int transposed;
    // dense arrays: B[t][el], A[el][t], G[el][el].  el->ring kinds want D[row = t][k = el].
    if (kind == TAB_INV) { src = d_B; transposed = 0; }
    else if (kind == TAB_FWD_ADJ) { src = d_A; transposed = 1; }
    else if (kind == TAB_FWD) { src = d_A; transposed = 0; }
    else if (kind == TAB_INV_ADJ) { src = d_B; transposed = 1; }
    else { src = d_G; transposed = 0; }
    src += (int64_t)i * Rp * Rp;
    const int row_beg = rows_el ? kb : 0, k_beg = k_el ? kb : 0;
    dim3 grid((Rp - k_beg) / 8, (Rp - row_beg) / 16), block(128);
    if (grid.x == 0 || grid.y == 0) continue;
    hipLaunchKernelGGL(k_tile_table, grid, block, 0, 0, src, T.d_tab[kind] + T.m_off[kind][i], Rp, Rp, row_beg, k_beg,
                       transposed, -1);
  }
  PXM_HIP(hipGetLastError());
  return 0;
}

int get_tables(int L, int spin, unsigned kinds_mask, ShtTables** out) {
  std::lock_guard<std::mutex> lock(g_tab_mutex);
  int dev = 15;  // (dry-run entries -- fake addresses -- live under a device id no node has: never handed to a real plan)
  if (!dry_run()) {
    PXM_HIP(hipGetDevice(&dev));
    PXM_REQUIRE(dev >= 0 && dev < 15, "get_tables: device index outside [0, 15)");
  }
  auto key = std::make_pair(L * 16 + dev, spin);
  ShtTables* T = nullptr;
  auto it = g_tab_cache.find(key);
  if (it != g_tab_cache.end()) T = it->second;
  else {
    T = new ShtTables();
    T->L = L;
    T->spin = spin;
    T->Rp = round_up(L, 16);
    T->paired = (spin == 0);
    T->n_m = T->paired ? L : 2 * L - 1;
    g_tab_cache[key] = T;
  }
  unsigned missing = 0;
  for (int k = 0; k < TAB_KINDS; ++k)
    if ((kinds_mask >> k & 1u) && !T->d_tab[k]) missing |= 1u << k;
  if (missing && dry_run()) {
    for (int k = 0; k < TAB_KINDS; ++k)
      if (missing >> k & 1u) {
        int rc = build_kind(*T, k, nullptr, nullptr, nullptr);
        if (rc) return rc;
      }
  } else if (missing) {
    const int Rp = T->Rp;
    const size_t dense = (size_t)T->n_m * Rp * Rp;
    std::vector<double> hB(dense, 0.0);
    const int m0 = T->paired ? 0 : -(L - 1);
    for (int i = 0; i < T->n_m; ++i) wigner_ring_table(L, spin, m0 + i, hB.data() + (size_t)i * Rp * Rp, Rp);
    double *d_B = nullptr, *d_A = nullptr, *d_Q = nullptr, *d_G = nullptr;
    PXM_HIP(hipMalloc(&d_B, dense * sizeof(double)));
    PXM_HIP(hipMemcpy(d_B, hB.data(), dense * sizeof(double), hipMemcpyHostToDevice));
    hB.clear();
    hB.shrink_to_fit();
    if (missing & ((1u << TAB_FWD) | (1u << TAB_FWD_ADJ))) {
      std::vector<double> hQ((size_t)2 * Rp * Rp, 0.0);
      quadrature_gram(L, +1, hQ.data(), Rp);
      quadrature_gram(L, -1, hQ.data() + (size_t)Rp * Rp, Rp);
      PXM_HIP(hipMalloc(&d_Q, hQ.size() * sizeof(double)));
      PXM_HIP(hipMemcpy(d_Q, hQ.data(), hQ.size() * sizeof(double), hipMemcpyHostToDevice));
      PXM_HIP(hipMalloc(&d_A, dense * sizeof(double)));
      dim3 grid(Rp / 16, Rp / 16, T->n_m), block(16, 16);
      hipLaunchKernelGGL(k_build_fwd, grid, block, 0, 0, d_B, d_Q, d_A, Rp, L, 2.0 * M_PI / (2 * L - 1), m0, spin);
      PXM_HIP(hipGetLastError());
    }
    if (missing & ((1u << TAB_GRAM) | (1u << TAB_GRAM_SPLIT) | (1u << TAB_GRAM_SPLIT0))) {
      PXM_HIP(hipMalloc(&d_G, dense * sizeof(double)));
      dim3 grid(Rp / 16, Rp / 16, T->n_m), block(16, 16);
      hipLaunchKernelGGL(k_build_gram, grid, block, 0, 0, d_B, d_G, Rp, L);
      PXM_HIP(hipGetLastError());
    }
    for (int k = 0; k < TAB_KINDS; ++k)
      if (missing >> k & 1u) {
        int rc = build_kind(*T, k, d_B, d_A, d_G);
        if (rc) return rc;
      }
    PXM_HIP(hipDeviceSynchronize());
    PXM_HIP(hipFree(d_B));
    if (d_A) PXM_HIP(hipFree(d_A));
    if (d_Q) PXM_HIP(hipFree(d_Q));
    if (d_G) PXM_HIP(hipFree(d_G));
  }
  *out = T;
  return 0;
}

void retain_tables(ShtTables* T) {
  std::lock_guard<std::mutex> lock(g_tab_mutex);
  if (T) ++T->refs;
}
void release_tables(ShtTables* T) {
  std::lock_guard<std::mutex> lock(g_tab_mutex);
  if (T && T->refs > 0) --T->refs;
}
int64_t tables_trim() {
  std::lock_guard<std::mutex> lock(g_tab_mutex);
  int64_t freed = 0;
  for (auto it = g_tab_cache.begin(); it != g_tab_cache.end();) {
    ShtTables* T = it->second;
    // (a dry-run pass only drops its own entries -- device id 15 -- and leaves the real cache alone)
    if (T->refs > 0 || (dry_run() && it->first.first % 16 != 15)) {
      ++it;
      continue;
    }
    for (int k = 0; k < TAB_KINDS; ++k) {
      if (T->d_tab[k]) deferred_free(T->d_tab[k]);
      freed += (int64_t)T->bytes[k];
    }
    if (T->d_pole) deferred_free(T->d_pole);
    delete T;
    it = g_tab_cache.erase(it);
  }
  drain_deferred();
  return freed;
}

}  // namespace pxm
