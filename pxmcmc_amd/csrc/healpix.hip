// HEALPix ring synthesis and its adjoint (RING order): band-limited f_lm -> values at the 12 nside^2 pixel centres,
//   v_p = sum_lm sY_lm(theta_p, phi_p) f_lm,      f_lm = sum_p conj(sY_lm(theta_p, phi_p)) v_p   (no quadrature weight),
// sY_lm = lam_lm(theta) exp(i m phi), lam_lm = (-1)^s sqrt((2l+1)/4pi) d^l_{m,-s}  (DESIGN.md section 22).
//
// synthesis = Legendre stage, then phi stage; the adjoint runs the transposed stages in reverse order.
//   G    [C][R][2L-1] c128   ring array of the plan: chain, ring (north to south), order m = -(L-1) .. L-1 contiguous
//   lam  [MI][L][Rp]  f64    MI = L orders m >= 0 at spin 0 (lam_{l,-m} = (-1)^m lam_lm), else all 2L-1; ring minor,
//                            Rp = roundup(R, 64) with zero padding, so that lanes = rings read it coalesced
//   tw   per q = 1 .. nside: exp(i pi t / (4q)), t < 8q, at offset 4 q (q - 1): the azimuth offset phi0 = pi / nphi of the
//                            shifted rings (exp(i m phi0) = tw[m mod 2 nphi]) and every DFT twiddle of a ring of nphi = 4q
// Legendre forward  k_hpx_leg_fwd: one order (spin 0: the pair +-m) and 256 rings per workgroup, a lane per ring; the f_lm
//   of HPX_NC chains go through LDS in tiles of HPX_LT degrees and are read back as broadcasts.
// Legendre adjoint  k_hpx_leg_adj: one order and 64 degrees per workgroup, a lane per degree; 64 x 64 table tiles are
//   transposed through LDS, each of the four waves owns two of the HPX_NC chains and sums the rings 0 .. R-1 in order.
// phi stage         k_hpx_phi_fwd / k_hpx_phi_adj: one ring of one chain per workgroup, in LDS: fold the orders onto
//   k = m mod nphi with the phase of the ring, then one radix-4 split of the nphi = 4q point DFT (k = 4 k1 + k2,
//   j = j1 + q j2): four direct length-q DFTs, the twiddles w^{j1 k2}, a 4-point butterfly.  One path for every ring.
// No kernel uses atomics: a chain's result does not depend on the batch it runs in.
#include "plan_common.h"

#include <cmath>
#include <memory>

using namespace pxm;

namespace {

constexpr int HPX_NC = 8;         // chains per pass over the table
constexpr int HPX_LT = 32;        // degrees per LDS tile of the forward Legendre kernel
constexpr int HPX_LU = 8;         // of which a lane loads this many table entries before it uses the first
constexpr int HPX_THREADS = 256;  // every kernel of this file
constexpr size_t HPX_LDS_MAX = 160 * 1024;
const long double HPX_PI = 3.141592653589793238462643383279502884L;

// bytes of LDS of a phi-stage workgroup: two arrays of the longest ring (4 nside points) and nside twiddles, c128
inline size_t hpx_phi_lds(int nside) { return (size_t)9 * nside * 16; }
inline int hpx_nside_max() { return (int)(HPX_LDS_MAX / (9 * 16)); }

// ring r = 0 .. 4 nside - 2, north to south
struct HpxRing {
  int nphi, shifted;
  long double z;  // cos(theta)
};
HpxRing hpx_ring(int nside, int r) {
  const int i = r + 1, ip = std::min(i, 4 * nside - i);
  HpxRing g;
  const long double ns = nside;
  if (ip < nside) {
    g.nphi = 4 * ip;
    g.z = 1.0L - (long double)ip * ip / (3.0L * ns * ns);
    g.shifted = 1;
  } else {
    g.nphi = 4 * nside;
    g.z = 4.0L / 3.0L - 2.0L * ip / (3.0L * ns);
    g.shifted = ((ip - nside) % 2 == 0) ? 1 : 0;
  }
  if (i > 2 * nside) g.z = -g.z;
  return g;
}

int hpx_check(int L, int nside, int spin, const std::string& who) {
  PXM_REQUIRE(L >= 1, who + ": Bandlimit must be greater than 0");
  PXM_REQUIRE(L <= 1024, who + ": no kernels for bandlimit L = " + std::to_string(L) + " (the largest bandlimit is L = 1024)");
  PXM_REQUIRE(std::abs(spin) < L, who + ": need |spin| < L");
  PXM_REQUIRE(nside >= 1, who + ": need nside >= 1");
  PXM_REQUIRE(nside <= hpx_nside_max(), who + ": nside = " + std::to_string(nside) + ": the longest ring (" + std::to_string(4 * (int64_t)nside) +
                                            " points) needs " + std::to_string(hpx_phi_lds(std::min(nside, 1 << 20))) +
                                            " B of LDS per workgroup, a CU has " + std::to_string(HPX_LDS_MAX) + " (the largest nside is " +
                                            std::to_string(hpx_nside_max()) + ")");
  return 0;
}

__device__ inline double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline double2 cmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a conj(b)
__device__ inline void cfma(double2& acc, double t, double2 x) {
  acc.x = fma(t, x.x, acc.x);
  acc.y = fma(t, x.y, acc.y);
}

// G[c][r][m] = sum_l lam_lm(theta_r) f[c][l^2 + l + m]; PAIR (spin 0): the orders +m and -m from the table row of m >= 0
template <bool PAIR>
__global__ __launch_bounds__(HPX_THREADS) void k_hpx_leg_fwd(const double* __restrict__ lam, const double2* __restrict__ f,
                                                              double2* __restrict__ G, int L, int R, int Rp, int spin, int C) {
  constexpr int S = PAIR ? 2 : 1;
  __shared__ double2 sf[S][HPX_LT][HPX_NC];
  const int tid = threadIdx.x, mi = blockIdx.y, m = PAIR ? mi : mi - (L - 1);
  const int r = blockIdx.x * HPX_THREADS + tid;
  const bool live = r < Rp;  // (the padding rings r >= R of the table are zero)
  const int el0 = max(abs(m), abs(spin)), M = 2 * L - 1;
  const double* tab = lam + (int64_t)mi * L * Rp + r;
  const int64_t nlm = (int64_t)L * L;
  const double sgn = (m & 1) ? -1.0 : 1.0;
  for (int c0 = 0; c0 < C; c0 += HPX_NC) {
    double2 acc[S][HPX_NC];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int k = 0; k < HPX_NC; ++k) acc[s][k] = make_double2(0.0, 0.0);
    for (int l0 = el0; l0 < L; l0 += HPX_LT) {
      __syncthreads();
      for (int e = tid; e < S * HPX_LT * HPX_NC; e += HPX_THREADS) {
        const int k = e % HPX_NC, j = (e / HPX_NC) % HPX_LT, s = e / (HPX_NC * HPX_LT);
        const int l = l0 + j, c = c0 + k;
        double2 x = make_double2(0.0, 0.0);
        if (l < L && c < C) x = f[c * nlm + (int64_t)l * l + l + (s ? -m : m)];
        sf[s][j][k] = x;
      }
      __syncthreads();
      const int nj = min(HPX_LT, L - l0);
      for (int j0 = 0; j0 < nj; j0 += HPX_LU) {  // HPX_LU table loads in flight per lane (sf is zero beyond nj)
        double t[HPX_LU];
#pragma unroll
        for (int u = 0; u < HPX_LU; ++u) t[u] = (live && j0 + u < nj) ? tab[(int64_t)(l0 + j0 + u) * Rp] : 0.0;
#pragma unroll
        for (int u = 0; u < HPX_LU; ++u)
#pragma unroll
          for (int s = 0; s < S; ++s)
#pragma unroll
            for (int k = 0; k < HPX_NC; ++k) cfma(acc[s][k], t[u], sf[s][j0 + u][k]);
      }
    }
    if (r < R) {
#pragma unroll
      for (int k = 0; k < HPX_NC; ++k) {
        const int c = c0 + k;
        if (c >= C) break;
        double2* g = G + ((int64_t)c * R + r) * M + (L - 1);
        g[m] = acc[0][k];
        if (PAIR && m > 0) g[-m] = make_double2(sgn * acc[S - 1][k].x, sgn * acc[S - 1][k].y);
      }
    }
  }
}

// f[c][l^2 + l + m] = sum_r lam_lm(theta_r) Gt[c][r][m], the rings in the order r = 0 .. R-1
template <bool PAIR>
__global__ __launch_bounds__(HPX_THREADS) void k_hpx_leg_adj(const double* __restrict__ lam, const double2* __restrict__ Gt,
                                                              double2* __restrict__ f, int L, int R, int Rp, int spin, int C) {
  constexpr int S = PAIR ? 2 : 1;
  __shared__ double tl[64][65];  // table tile [degree][ring], one column of padding: the column reads are conflict-free
  __shared__ double2 sg[S][64][HPX_NC];
  const int tid = threadIdx.x, w = tid >> 6, lj = tid & 63;
  const int mi = blockIdx.y, m = PAIR ? mi : mi - (L - 1);
  const int l0 = blockIdx.x * 64, l = l0 + lj, M = 2 * L - 1;
  if (l0 + 63 < abs(m)) return;  // (the whole workgroup: no coefficient (l, m) in this tile)
  const double* tab = lam + (int64_t)mi * L * Rp;
  const int64_t nlm = (int64_t)L * L;
  const double sgn = (m & 1) ? -1.0 : 1.0;
  for (int c0 = 0; c0 < C; c0 += HPX_NC) {
    double2 acc[S][2];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s][0] = acc[s][1] = make_double2(0.0, 0.0);
    for (int r0 = 0; r0 < Rp; r0 += 64) {
      __syncthreads();
      for (int jj = 0; jj < 16; ++jj) {
        const int j = w * 16 + jj, ll = l0 + j;
        tl[j][lj] = ll < L ? tab[(int64_t)ll * Rp + r0 + lj] : 0.0;
      }
      for (int e = tid; e < S * 64 * HPX_NC; e += HPX_THREADS) {
        const int k = e % HPX_NC, i = (e / HPX_NC) % 64, s = e / (HPX_NC * 64);
        const int r = r0 + i, c = c0 + k;
        double2 x = make_double2(0.0, 0.0);
        if (r < R && c < C) x = Gt[((int64_t)c * R + r) * M + (L - 1) + (s ? -m : m)];
        sg[s][i][k] = x;
      }
      __syncthreads();
      for (int i = 0; i < 64; ++i) {
        const double t = tl[lj][i];
#pragma unroll
        for (int s = 0; s < S; ++s) {
          cfma(acc[s][0], t, sg[s][i][2 * w]);
          cfma(acc[s][1], t, sg[s][i][2 * w + 1]);
        }
      }
    }
    if (l < L && l >= abs(m)) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int c = c0 + 2 * w + kk;
        if (c < C) {
          double2* o = f + c * nlm + (int64_t)l * l + l;
          o[m] = acc[0][kk];
          if (PAIR && m > 0) o[-m] = make_double2(sgn * acc[S - 1][kk].x, sgn * acc[S - 1][kk].y);
        }
      }
    }
  }
}

// v[c][start_r + j] = sum_m G[c][r][m] exp(i m (phi0_r + 2 pi j / nphi_r))
__global__ __launch_bounds__(HPX_THREADS) void k_hpx_phi_fwd(const double2* __restrict__ G, const double2* __restrict__ tw,
                                                              const int* __restrict__ nphi, const int* __restrict__ shifted,
                                                              const int64_t* __restrict__ start, double2* __restrict__ v, int L, int R,
                                                              int64_t npix) {
  extern __shared__ double2 hpx_sm[];
  const int r = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int N = nphi[r], q = N >> 2, M = 2 * L - 1;
  const bool sh = shifted[r] != 0;
  const double2* twq = tw + 4 * (int64_t)q * (q - 1);
  double2 *H = hpx_sm, *A = hpx_sm + N, *wq = hpx_sm + 2 * N;
  const double2* g = G + ((int64_t)c * R + r) * M + (L - 1);
  // fold: H[k] = sum_{m = k mod N} G_m exp(i m phi0)
  for (int k = tid; k < N; k += HPX_THREADS) {
    double2 acc = make_double2(0.0, 0.0);
    for (int m = k - N * ((k + L - 1) / N); m <= L - 1; m += N) {  // the first m >= -(L-1) congruent to k
      double2 x = g[m];
      if (sh) {
        int t = m % (2 * N);
        if (t < 0) t += 2 * N;
        x = cmul(x, twq[t]);
      }
      acc.x += x.x;
      acc.y += x.y;
    }
    H[k] = acc;
  }
  for (int t = tid; t < q; t += HPX_THREADS) wq[t] = twq[8 * t];  // exp(2 pi i t / q)
  __syncthreads();
  // A[k2][j1] = sum_k1 H[4 k1 + k2] exp(2 pi i j1 k1 / q)
  for (int o = tid; o < N; o += HPX_THREADS) {
    const int k2 = o / q, j1 = o - k2 * q;
    double2 acc = make_double2(0.0, 0.0);
    int t = 0;
    for (int k1 = 0; k1 < q; ++k1) {
      const double2 p = cmul(H[4 * k1 + k2], wq[t]);
      acc.x += p.x;
      acc.y += p.y;
      t += j1;
      if (t >= q) t -= q;
    }
    A[o] = acc;
  }
  __syncthreads();
  // out[j1 + q j2] = sum_k2 i^{j2 k2} w_N^{j1 k2} A[k2][j1]
  double2* out = v + c * npix + start[r];
  for (int j1 = tid; j1 < q; j1 += HPX_THREADS) {
    const double2 b0 = A[j1], b1 = cmul(A[q + j1], twq[2 * j1]), b2 = cmul(A[2 * q + j1], twq[4 * j1]),
                  b3 = cmul(A[3 * q + j1], twq[6 * j1]);
    const double2 s02 = make_double2(b0.x + b2.x, b0.y + b2.y), d02 = make_double2(b0.x - b2.x, b0.y - b2.y);
    const double2 s13 = make_double2(b1.x + b3.x, b1.y + b3.y), d13 = make_double2(b1.x - b3.x, b1.y - b3.y);
    out[j1] = make_double2(s02.x + s13.x, s02.y + s13.y);
    out[j1 + q] = make_double2(d02.x - d13.y, d02.y + d13.x);  // d02 + i d13
    out[j1 + 2 * q] = make_double2(s02.x - s13.x, s02.y - s13.y);
    out[j1 + 3 * q] = make_double2(d02.x + d13.y, d02.y - d13.x);  // d02 - i d13
  }
}

// Gt[c][r][m] = exp(-i m phi0_r) sum_j v[c][start_r + j] exp(-2 pi i j m / nphi_r): every order of the ring is written
__global__ __launch_bounds__(HPX_THREADS) void k_hpx_phi_adj(const double2* __restrict__ v, const double2* __restrict__ tw,
                                                              const int* __restrict__ nphi, const int* __restrict__ shifted,
                                                              const int64_t* __restrict__ start, double2* __restrict__ Gt, int L, int R,
                                                              int64_t npix) {
  extern __shared__ double2 hpx_sm[];
  const int r = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int N = nphi[r], q = N >> 2, M = 2 * L - 1;
  const bool sh = shifted[r] != 0;
  const double2* twq = tw + 4 * (int64_t)q * (q - 1);
  double2 *B = hpx_sm, *H = hpx_sm + N, *wq = hpx_sm + 2 * N;
  const double2* x = v + c * npix + start[r];
  // B[k2][j1] = conj(w_N^{j1 k2}) sum_j2 (-i)^{j2 k2} x[j1 + q j2]
  for (int j1 = tid; j1 < q; j1 += HPX_THREADS) {
    const double2 x0 = x[j1], x1 = x[j1 + q], x2 = x[j1 + 2 * q], x3 = x[j1 + 3 * q];
    const double2 s02 = make_double2(x0.x + x2.x, x0.y + x2.y), d02 = make_double2(x0.x - x2.x, x0.y - x2.y);
    const double2 s13 = make_double2(x1.x + x3.x, x1.y + x3.y), d13 = make_double2(x1.x - x3.x, x1.y - x3.y);
    B[j1] = make_double2(s02.x + s13.x, s02.y + s13.y);
    B[q + j1] = cmulc(make_double2(d02.x + d13.y, d02.y - d13.x), twq[2 * j1]);  // d02 - i d13
    B[2 * q + j1] = cmulc(make_double2(s02.x - s13.x, s02.y - s13.y), twq[4 * j1]);
    B[3 * q + j1] = cmulc(make_double2(d02.x - d13.y, d02.y + d13.x), twq[6 * j1]);  // d02 + i d13
  }
  for (int t = tid; t < q; t += HPX_THREADS) wq[t] = twq[8 * t];
  __syncthreads();
  // H[4 k1 + k2] = sum_j1 B[k2][j1] exp(-2 pi i j1 k1 / q)
  for (int o = tid; o < N; o += HPX_THREADS) {
    const int k2 = o / q, k1 = o - k2 * q;
    double2 acc = make_double2(0.0, 0.0);
    int t = 0;
    for (int j1 = 0; j1 < q; ++j1) {
      const double2 p = cmulc(B[k2 * q + j1], wq[t]);
      acc.x += p.x;
      acc.y += p.y;
      t += k1;
      if (t >= q) t -= q;
    }
    H[4 * k1 + k2] = acc;
  }
  __syncthreads();
  // unfold: periodic in m, with the conjugate phase of the ring
  double2* g = Gt + ((int64_t)c * R + r) * M + (L - 1);
  for (int mo = tid; mo < M; mo += HPX_THREADS) {
    const int m = mo - (L - 1);
    int t = m % (2 * N);
    if (t < 0) t += 2 * N;
    double2 y = H[t >= N ? t - N : t];
    if (sh) y = cmulc(y, twq[t]);
    g[m] = y;
  }
}

std::atomic<uint64_t> g_hpx_lds_done{0};

}  // namespace

struct pxm_hpx_plan_s {
  int L = 0, nside = 0, spin = 0, Cmax = 0, R = 0, Rp = 0, MI = 0;
  int64_t npix = 0;
  size_t lds = 0, table_bytes = 0;
  double* d_lam = nullptr;
  double2* d_tw = nullptr;
  int *d_nphi = nullptr, *d_shifted = nullptr;
  int64_t* d_start = nullptr;
  double2* d_G = nullptr;
  unsigned* d_status = nullptr;
};

extern "C" {

int pxm_host_hpx_geometry(int L, int nside, int64_t* out) {
  PXM_REQUIRE(out, "pxm_host_hpx_geometry: null output");
  if (int rc = hpx_check(L, nside, 0, "pxm_host_hpx_geometry")) return rc;
  out[0] = 4 * (int64_t)nside - 1;
  out[1] = 12 * (int64_t)nside * nside;
  out[2] = (int64_t)hpx_phi_lds(nside);
  out[3] = hpx_nside_max();
  out[4] = HPX_THREADS;
  out[5] = round_up(4 * nside - 1, 64);
  return 0;
}

int pxm_host_hpx_rings(int nside, int* nphi, double* theta, double* phi0, int64_t* start) {
  PXM_REQUIRE(nphi && theta && phi0 && start, "pxm_host_hpx_rings: null output");
  PXM_REQUIRE(nside >= 1 && nside <= (1 << 20), "pxm_host_hpx_rings: need 1 <= nside <= 2^20");
  int64_t s = 0;
  for (int r = 0; r < 4 * nside - 1; ++r) {
    const HpxRing g = hpx_ring(nside, r);
    nphi[r] = g.nphi;
    theta[r] = (double)acosl(g.z);
    phi0[r] = g.shifted ? (double)(HPX_PI / g.nphi) : 0.0;
    start[r] = s;
    s += g.nphi;
  }
  return 0;
}

int pxm_host_hpx_lambda(int L, int spin, int m, const double* theta, int nt, double* out) {
  PXM_REQUIRE(theta && out, "pxm_host_hpx_lambda: null argument");
  PXM_REQUIRE(L >= 1 && nt >= 1 && std::abs(spin) < L && std::abs(m) < L, "pxm_host_hpx_lambda: need L >= 1, nt >= 1, |spin| < L, |m| < L");
  std::vector<long double> th(theta, theta + nt);
  for (int64_t i = 0; i < (int64_t)nt * L; ++i) out[i] = 0.0;
  wigner_colat_table(L, spin, m, th.data(), nt, out, L, 1);
  return 0;
}

int pxm_hpx_plan_create(int L, int nside, int spin, int max_chains, pxm_hpx_plan_t* plan) {
  PXM_REQUIRE(plan, "pxm_hpx_plan_create: null plan pointer");
  if (int rc = hpx_check(L, nside, spin, "pxm_hpx_plan_create")) return rc;
  PXM_REQUIRE(max_chains >= 1, "pxm_hpx_plan_create: max_chains must be >= 1");
  PXM_REQUIRE(dry_run() || pxm_device_count() > 0, "pxm_hpx_plan_create: no HIP device visible (the HIP path is the only path)");
  drain_deferred();
  std::unique_ptr<pxm_hpx_plan_s, int (*)(pxm_hpx_plan_t)> guard(new pxm_hpx_plan_s(), pxm_hpx_plan_destroy);
  pxm_hpx_plan_s* p = guard.get();
  p->L = L;
  p->nside = nside;
  p->spin = spin;
  p->Cmax = max_chains;
  p->R = 4 * nside - 1;
  p->Rp = round_up(p->R, 64);
  p->MI = spin == 0 ? L : 2 * L - 1;
  p->npix = 12 * (int64_t)nside * nside;
  p->lds = hpx_phi_lds(nside);
  int rc;
  // ring geometry
  std::vector<int> nphi(p->R), shifted(p->R);
  std::vector<int64_t> start(p->R);
  std::vector<long double> theta(p->R);
  int64_t s = 0;
  for (int r = 0; r < p->R; ++r) {
    const HpxRing g = hpx_ring(nside, r);
    nphi[r] = g.nphi;
    shifted[r] = g.shifted;
    theta[r] = acosl(g.z);
    start[r] = s;
    s += g.nphi;
  }
  PXM_REQUIRE(s == p->npix, "pxm_hpx_plan_create: internal error: the rings do not add up to 12 nside^2 pixels");
  if ((rc = dev_table(&p->d_nphi, nphi, "HEALPix ring lengths"))) return rc;
  if ((rc = dev_table(&p->d_shifted, shifted, "HEALPix ring shifts"))) return rc;
  if ((rc = dev_table(&p->d_start, start, "HEALPix ring starts"))) return rc;
  // twiddles and ring phases: exp(i pi t / (4q)), t < 8q, q = 1 .. nside
  {
    std::vector<double> tw((size_t)8 * nside * (nside + 1));
    for (int q = 1; q <= nside; ++q) {
      double* row = tw.data() + 8 * (size_t)q * (q - 1);
      for (int t = 0; t < 8 * q; ++t) {
        const long double a = HPX_PI * t / (4.0L * q);
        row[2 * t] = (double)cosl(a);
        row[2 * t + 1] = (double)sinl(a);
      }
    }
    if ((rc = dev_table((double**)&p->d_tw, tw, "HEALPix twiddles"))) return rc;
    p->table_bytes += tw.size() * sizeof(double);
  }
  // Legendre table [MI][L][Rp]
  {
    std::vector<double> lam((size_t)p->MI * L * p->Rp, 0.0);
    for (int mi = 0; mi < p->MI; ++mi)
      wigner_colat_table(L, spin, spin == 0 ? mi : mi - (L - 1), theta.data(), p->R, lam.data() + (size_t)mi * L * p->Rp, 1, p->Rp);
    if ((rc = dev_table(&p->d_lam, lam, "HEALPix Legendre table"))) return rc;
    p->table_bytes += lam.size() * sizeof(double);
  }
  if ((rc = dev_alloc(&p->d_G, (size_t)max_chains * p->R * (2 * L - 1) * sizeof(double2), "HEALPix ring array"))) return rc;
  if ((rc = status_alloc(&p->d_status))) return rc;
  if ((rc = allow_dynamic_lds(g_hpx_lds_done, {(const void*)k_hpx_phi_fwd, (const void*)k_hpx_phi_adj}))) return rc;
  *plan = guard.release();
  return 0;
}

int pxm_hpx_plan_destroy(pxm_hpx_plan_t p) {
  if (!p) return 0;
  deferred_free(p->d_lam);
  deferred_free(p->d_tw);
  deferred_free(p->d_nphi);
  deferred_free(p->d_shifted);
  deferred_free(p->d_start);
  deferred_free(p->d_G);
  deferred_free(p->d_status);
  delete p;
  drain_deferred();  // (a no-op while a stream capture is in progress: freed at the next safe point)
  return 0;
}

int pxm_hpx_synthesis(pxm_hpx_plan_t p, const void* flm, void* v, int C, pxm_stream_t s) {
  if (int rc = plan_check(p, flm, v, C, "pxm_hpx_synthesis")) return rc;
  PXM_REQUIRE((((uintptr_t)flm | (uintptr_t)v) & 15) == 0, "pxm_hpx_synthesis: the arrays must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  note_stream(st);
  if (dry_run()) return 0;
  const dim3 grid((p->Rp + HPX_THREADS - 1) / HPX_THREADS, p->MI);
  if (p->spin == 0)
    hipLaunchKernelGGL(k_hpx_leg_fwd<true>, grid, dim3(HPX_THREADS), 0, st, p->d_lam, (const double2*)flm, p->d_G, p->L, p->R, p->Rp, p->spin, C);
  else
    hipLaunchKernelGGL(k_hpx_leg_fwd<false>, grid, dim3(HPX_THREADS), 0, st, p->d_lam, (const double2*)flm, p->d_G, p->L, p->R, p->Rp, p->spin, C);
  hipLaunchKernelGGL(k_hpx_phi_fwd, dim3(p->R, C), dim3(HPX_THREADS), p->lds, st, p->d_G, p->d_tw, p->d_nphi, p->d_shifted, p->d_start,
                     (double2*)v, p->L, p->R, p->npix);
  PXM_HIP(hipGetLastError());
  return 0;
}

int pxm_hpx_synthesis_adjoint(pxm_hpx_plan_t p, const void* v, void* flm, int C, pxm_stream_t s) {
  if (int rc = plan_check(p, v, flm, C, "pxm_hpx_synthesis_adjoint")) return rc;
  PXM_REQUIRE((((uintptr_t)flm | (uintptr_t)v) & 15) == 0, "pxm_hpx_synthesis_adjoint: the arrays must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  note_stream(st);
  if (dry_run()) return 0;
  hipLaunchKernelGGL(k_hpx_phi_adj, dim3(p->R, C), dim3(HPX_THREADS), p->lds, st, (const double2*)v, p->d_tw, p->d_nphi, p->d_shifted,
                     p->d_start, p->d_G, p->L, p->R, p->npix);
  const dim3 grid((p->L + 63) / 64, p->MI);
  if (p->spin == 0)
    hipLaunchKernelGGL(k_hpx_leg_adj<true>, grid, dim3(HPX_THREADS), 0, st, p->d_lam, p->d_G, (double2*)flm, p->L, p->R, p->Rp, p->spin, C);
  else
    hipLaunchKernelGGL(k_hpx_leg_adj<false>, grid, dim3(HPX_THREADS), 0, st, p->d_lam, p->d_G, (double2*)flm, p->L, p->R, p->Rp, p->spin, C);
  PXM_HIP(hipGetLastError());
  return 0;
}

int64_t pxm_hpx_table_bytes(pxm_hpx_plan_t p) { return p ? (int64_t)p->table_bytes : -1; }

int pxm_hpx_status(pxm_hpx_plan_t p, int clear, pxm_stream_t stream) {
  PXM_REQUIRE(p, "pxm_hpx_status: null plan");
  return status_read(p->d_status, (hipStream_t)stream, clear);
}

}  // extern "C"
