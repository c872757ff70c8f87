// The harmonic split / merge stage (harm_stage.h): its two kernels, their launches, and the host tables of its weights.
#include "../../include/pxmcmc_amd.h"
#include "elem.h"
#include "harm_stage.h"

#include <algorithm>
#include <cmath>

namespace pxm {

__device__ __forceinline__ double2 dw_w(double2 w, bool cj) { return cj ? double2{w.x, -w.y} : w; }

// out_d[c][lm] = w_d(l) f[c][lm]  (w or conj(w)), for every item d and lm < bl_d^2 (out_d[c] at a_off + c cstride)
__global__ __launch_bounds__(DW_THREADS) void k_dw_split(const double2* __restrict__ flm, double2* __restrict__ harm,
                                                         const DwItem* __restrict__ items, int nitems,
                                                         const double2* __restrict__ W, int cj, int L) {
  const int d = dw_find(items, nitems, blockIdx.x);
  const DwItem it = items[d];
  const int lm = (blockIdx.x - it.blk0) * DW_THREADS + threadIdx.x;
  const int nlm = it.bl * it.bl;
  if (lm >= nlm) return;
  const int c = blockIdx.y;
  const double2 w = dw_w(W[it.w_off + dw_el(lm)], cj);
  harm[it.a_off + (int64_t)c * it.cstride + lm] = cmul(w, flm[(int64_t)c * L * L + lm]);
}

// f[c][lm] = sum_d [l < bl_d] w_d(l) b_d[c][lm]
__global__ __launch_bounds__(DW_THREADS) void k_dw_merge(const double2* __restrict__ harm, double2* __restrict__ flm,
                                                         const DwItem* __restrict__ items, int nitems,
                                                         const double2* __restrict__ W, int cj, int L) {
  const int lm = blockIdx.x * DW_THREADS + threadIdx.x;
  if (lm >= L * L) return;
  const int c = blockIdx.y;
  const int el = dw_el(lm);
  double2 acc{0.0, 0.0};
  for (int d = 0; d < nitems; ++d) {
    const DwItem it = items[d];
    if (el >= it.bl) continue;
    const double2 w = dw_w(W[it.w_off + el], cj);
    const double2 b = harm[it.a_off + (int64_t)c * it.cstride + lm];
    acc = cadd(acc, cmul(w, b));
  }
  flm[(int64_t)c * L * L + lm] = acc;
}

int harm_split(const HarmStage& s, const double2* flm, double2* harm, int weights, int cj, int C, hipStream_t st) {
  hipLaunchKernelGGL(k_dw_split, dim3(s.split_blocks, C), dim3(DW_THREADS), 0, st, flm, harm, s.d_items, s.nitems,
                     weights ? s.d_ws : s.d_wa, cj, s.L);
  PXM_HIP(hipGetLastError());
  return 0;
}

int harm_merge(const HarmStage& s, const double2* harm, double2* flm, int weights, int cj, int C, hipStream_t st) {
  hipLaunchKernelGGL(k_dw_merge, dim3((s.L * s.L + DW_THREADS - 1) / DW_THREADS, C), dim3(DW_THREADS), 0, st, harm, flm,
                     s.d_items, s.nitems, weights ? s.d_ws : s.d_wa, cj, s.L);
  PXM_HIP(hipGetLastError());
  return 0;
}

void harm_release(HarmStage* s) {
  for (void* q : {(void*)s->d_items, (void*)s->d_wa, (void*)s->d_ws}) deferred_free(q);
}

int harm_create_check(const char* who, const void* plan, int L, double B, int J_min, int N, int spin, int max_chains) {
  const std::string fn(who);
  PXM_REQUIRE(plan, fn + ": null plan pointer");
  PXM_REQUIRE(L >= 2 && B > 1.0 && J_min >= 0, fn + ": bad (L, B, J_min)");
  PXM_REQUIRE(N >= 1 && N <= L, fn + ": need 1 <= N <= L");
  PXM_REQUIRE(std::abs(spin) < L, fn + ": |spin| must be < L");
  PXM_REQUIRE(spin == 0 || N == 1, fn + ": spin != 0 needs N = 1 (spin directional wavelets are not supported)");
  PXM_REQUIRE(max_chains >= 1 && max_chains <= 65535, fn + ": max_chains outside [1, 65535]");
  PXM_REQUIRE(J_min <= j_max(L, B), fn + ": J_min > J_max");
  PXM_REQUIRE(pxm_device_count() > 0, fn + ": no HIP device visible (the HIP path is the only path)");
  return 0;
}

// directionality component s_lm [L*L]: nu sqrt(2^-g C(g, (g - m)/2)), m = -g, -g + 2, .., g,
// g = gamma_l = the largest integer <= min(N - 1, l) with the parity of N - 1; nu = 1 (N odd), i (N even)
static std::vector<double2> dir_component(int L, int N) {
  std::vector<double2> s((size_t)L * L, double2{0.0, 0.0});
  for (int el = 0; el < L; ++el) {
    int g = std::min(N - 1, el);
    if ((N - 1 - g) % 2) --g;
    if (g < 0) continue;
    // C(g, k) by the recurrence C(g, k + 1) = C(g, k) (g - k) / (k + 1) in long double (64-bit mantissa: exact while the
    // binomial fits, within a few 2^-64 per step beyond, g <= 1023 steps at most), scaled by 2^-g exactly, one square root:
    // within 1 ulp of the exact value after the rounding to double
    long double c = 1.0L;
    for (int k = 0; k <= g; ++k) {
      const int m = g - 2 * k;
      const double v = (double)sqrtl(ldexpl(c, -g));
      s[(size_t)el * el + el + m] = (N % 2) ? double2{v, 0.0} : double2{0.0, v};
      c = c * (long double)(g - k) / (long double)(k + 1);
    }
  }
  return s;
}

DwTiling::DwTiling(int L_, double B, int J_min_, int N, int spin_) : L(L_), J_min(J_min_), spin(spin_), s(dir_component(L_, N)) {
  tiling_axisym(L, B, J_min, k0, kap);
}

void DwTiling::rows(int b, int n, bool harmonic, std::vector<double2>& wa, std::vector<double2>& ws) const {
  const double ca = 1.0 / std::sqrt(2.0 * M_PI), cs = std::sqrt(2.0 * M_PI);
  const double sgn = (!harmonic && (n % 2)) ? -1.0 : 1.0;
  for (int el = 0; el < L; ++el) {
    if (el < std::abs(spin)) {
      wa.push_back({0.0, 0.0});
      ws.push_back({0.0, 0.0});
      continue;
    }
    if (!b) {
      wa.push_back({k0[el], 0.0});
      ws.push_back({k0[el], 0.0});
      continue;
    }
    const double kj = kap[(size_t)(J_min + b - 1) * L + el];
    const double2 sv = std::abs(n) <= el ? s[(size_t)el * el + el + n] : double2{0.0, 0.0};
    const double fa = harmonic ? std::sqrt(8.0 * M_PI * M_PI / (2 * el + 1)) : ca;
    const double fs = harmonic ? std::sqrt((2 * el + 1) / (8.0 * M_PI * M_PI)) : cs;
    wa.push_back({sgn * kj * sv.x * fa, -sgn * kj * sv.y * fa});
    ws.push_back({sgn * kj * sv.x * fs, sgn * kj * sv.y * fs});
  }
}

std::vector<HarmRow> harm_weight_rows(int L, double B, int J_min, int N, int spin, bool harmonic, std::vector<double2>& wa,
                                      std::vector<double2>& ws) {
  const std::vector<int> bls = wav_bandlimits(L, B, J_min);
  const DwTiling tw(L, B, J_min, N, spin);
  std::vector<HarmRow> out;
  for (int b = 0; b < (int)bls.size(); ++b)
    for (int k = 0; k < harm_orients(b, N); ++k) {
      const int n = harm_n(b, k, N);
      if (!harmonic && std::abs(n) >= bls[b]) continue;
      out.push_back({b, n, bls[b]});
      tw.rows(b, n, harmonic, wa, ws);
    }
  return out;
}

std::vector<double2> dw_phases(int N) {
  std::vector<double2> ph((size_t)(2 * N - 1) * N);
  for (int q = 0; q < 2 * N - 1; ++q)
    for (int k = 0; k < N; ++k) {
      // e^{i n gamma_q}, n gamma_q = 2 pi (n q mod (2N-1)) / (2N-1): the angle reduced exactly, then formed and its
      // cosine and sine taken in long double (a double angle alone is off by several 2^-52), rounded to double once
      const int n = harm_n(1, k, N);
      const int r = (((n * q) % (2 * N - 1)) + (2 * N - 1)) % (2 * N - 1);
      const long double a = 2.0L * 3.141592653589793238462643383279502884L * (long double)r / (long double)(2 * N - 1);
      ph[(size_t)q * N + k] = double2{(double)cosl(a), (double)sinl(a)};
    }
  return ph;
}

}  // namespace pxm

extern "C" {

int64_t pxm_host_harm_weights(int L, double B, int J_min, int N, int spin, int harmonic, double* wa, double* ws, int* rows,
                              int64_t cap) {
  PXM_REQUIRE(L >= 1 && B > 1.0 && J_min >= 0 && J_min <= pxm::j_max(L, B), "pxm_host_harm_weights: bad (L, B, J_min)");
  PXM_REQUIRE(N >= 1 && N <= L, "pxm_host_harm_weights: need 1 <= N <= L");
  PXM_REQUIRE(std::abs(spin) < L && (spin == 0 || N == 1), "pxm_host_harm_weights: need |spin| < L, and N = 1 with a spin");
  std::vector<double2> a, s;
  const std::vector<pxm::HarmRow> r = pxm::harm_weight_rows(L, B, J_min, N, spin, harmonic != 0, a, s);
  const int64_t n = (int64_t)r.size();
  if (cap < n) return n;
  PXM_REQUIRE(wa && ws && rows, "pxm_host_harm_weights: null destination");
  for (size_t i = 0; i < a.size(); ++i) {
    wa[2 * i] = a[i].x, wa[2 * i + 1] = a[i].y;
    ws[2 * i] = s[i].x, ws[2 * i + 1] = s[i].y;
  }
  for (int64_t i = 0; i < n; ++i) rows[3 * i] = r[i].block, rows[3 * i + 1] = r[i].n, rows[3 * i + 2] = r[i].bl;
  return n;
}

int pxm_host_dir_component(int L, int N, double* s) {
  PXM_REQUIRE(L >= 1 && L <= 1024 && N >= 1 && N <= L && s, "pxm_host_dir_component: need 1 <= N <= L <= 1024 and a destination");
  const std::vector<double2> v = pxm::dir_component(L, N);
  for (size_t i = 0; i < v.size(); ++i) s[2 * i] = v[i].x, s[2 * i + 1] = v[i].y;
  return 0;
}

int pxm_host_dwav_phases(int N, double* ph) {
  PXM_REQUIRE(N >= 1 && N <= 1024 && ph, "pxm_host_dwav_phases: need 1 <= N <= 1024 and a destination");
  const std::vector<double2> p = pxm::dw_phases(N);
  for (size_t i = 0; i < p.size(); ++i) ph[2 * i] = p[i].x, ph[2 * i + 1] = p[i].y;
  return 0;
}

}  // extern "C"
