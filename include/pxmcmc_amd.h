/*
 * pxmcmc_amd.h -- C-ABI of the MI355X (gfx950) implementation of pxmcmc's
 * proximal-Langevin hot path (MYULA / PxMALA iteration).
 *
 * The reference (auggiemarignier/pxmcmc v1.0.1) has no FFI of its own: its hot
 * path is a duck-typed Python protocol whose O(L^3) work is
 * done by the pyssht / pys2let wheels.  These entry points are what a binding
 * for that path replaces; each cites the reference interface (file:line in
 * /root/reference) it stands in for.  Conventions:
 *
 *   - every function returns 0 on success, <0 on error (pxm_last_error() gives text);
 *   - device buffers are caller-owned; nothing is allocated after plan creation;
 *   - all device work is enqueued on the caller-supplied HIP stream (hipStream_t
 *     passed as void*); plans are not shared across threads or devices;
 *   - all mutable state lives in a plan (workspace, carried rings, Philox iteration counter, profiler); the
 *     only process-wide objects are the read-only per-device table cache (pxm_tables_trim), the borrowed side
 *     streams and the graveyard of deferred frees below;
 *   - arrays carry a leading chain-batch dimension C (independent chains); inside
 *     a chain the reference's own 1-D orders are kept: harmonic index el^2+el+m,
 *     MW images theta-major (L, 2L-1) C-order, wavelet coefficient vectors
 *     [scaling | j=J_min | ... | j=J_max] each block theta-major
 *     (pxmcmc/utils.py:11-22,49-51);
 *   - complex128 values are interleaved (re, im) doubles.
 */
#ifndef PXMCMC_AMD_H
#define PXMCMC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pxm_sht_plan_s* pxm_sht_plan_t;
typedef struct pxm_wav_plan_s* pxm_wav_plan_t;
typedef struct pxm_dwav_plan_s* pxm_dwav_plan_t;
typedef struct pxm_hwav_plan_s* pxm_hwav_plan_t;
typedef struct pxm_dft_plan_s* pxm_dft_plan_t;
typedef struct pxm_gemm_plan_s* pxm_gemm_plan_t;
typedef struct pxm_hpx_plan_s* pxm_hpx_plan_t;
typedef void* pxm_stream_t; /* hipStream_t */

/* ---- library ------------------------------------------------------------ */
int pxm_version(void);
/* Precision of the Box-Muller step of the Philox noise stream (pxmcmc/mcmc.py:193-195 draws fp64 randn).  Every
 * entry point that can draw noise takes the flag PXM_NOISE_F64, OR-ed into its `mode` (pxm_wav_*_step), `noise_complex`
 * (pxm_myula_step, pxm_chain_step, pxm_skrock_stage, pxm_pxmala_propose, pxm_sapg_step) or `dtype` (pxm_randn) argument:
 *   absent   Box-Muller on the f32 transcendental units (v_log_f32 / v_sin_f32 / v_cos_f32 with the exact fp64 exponent:
 *            deviates ~1e-6 relative, tail to 8.5 sigma) -- the default, pxm_noise_bits() == 32;
 *   present  log / sqrt / sincos evaluated in double precision (branch-free polynomials, csrc/philox.h): deviates equal
 *            numpy's float64 evaluation of the same formulae to ~1e-15.
 * Both read the same Philox4x32-10 counter stream and the same uniforms: the two streams agree to ~1e-6. */
#ifdef PXM_NOISE_F64
#error "the -DPXM_NOISE_F64 build switch was removed: pass the flag PXM_NOISE_F64 per call (one library serves both precisions)"
#endif
#define PXM_NOISE_F64 16
int pxm_noise_bits(void);
/* Host-only (no GPU) check that every global address a launch of the plans' GEMM task lists and DFT groups can form
 * -- including the clamped / aliased loads whose values are discarded -- lies inside its buffer.  Builds the plans
 * named by `what` (1: SHT plan (L, spin); 2: wavelet plan (L, B, J_min) + Gram lists; 4: + weak-lensing lists; 8: the
 * wavelet plan of bit 2 at `spin` instead of spin 0, without weak-lensing lists unless spin == 0; 16: the phi-DFT plan
 * (L, max_chains), which has no ranges to count: 0 when it can be created) in
 * dry-run mode and returns the number of address ranges verified, < 0 on a violation (pxm_last_error names the task).
 * The same check runs at every real plan creation.  The dry-run switch is per thread (plans created concurrently on
 * other threads are real); not to be called during a stream capture. */
int64_t pxm_host_check_address_ranges(int L, double B, int J_min, int spin, int max_chains, int what);
/* Host-only: bytes of the Gram table, as stored, of the ring-space step of the wavelet plan (L, B, J_min) at `spin` -- the
 * parity-split table for spin 0 and roundup(L, 16) % 32 == 0 unless PXM_GRAM_SPLIT=0 (read when a plan's Gram lists are
 * made), the dense one otherwise; < 0 on error.  (Order 0 takes Rp^2 doubles in either split form; with its two halves --
 * the default, PXM_GRAM_SPLIT=1 keeps it dense -- the launch streams the two diagonal blocks of them.) */
int64_t pxm_host_gram_table_bytes(int L, double B, int J_min, int spin, int max_chains);
const char* pxm_last_error(void);
/* number of visible HIP devices (0 when none; never fails) */
int pxm_device_count(void);

/* ---- teardown during stream capture ---------------------------------------------------------
 * hipFree is illegal while a stream capture is in progress, and the host language may tear a plan down at any
 * moment (Python's garbage collector).  The destroy calls therefore never free directly: device memory goes to
 * a graveyard that is emptied at safe points (plan creation, pxm_capture_end, a destroy outside any capture).
 * Bracket a capture with pxm_capture_begin / pxm_capture_end; a capture started elsewhere is also recognised
 * as soon as one entry point has been called on its stream.  pxm_deferred_pending: entries still queued. */
int pxm_capture_begin(void);
int pxm_capture_end(void);
int pxm_deferred_pending(void);
/* The Wigner ring tables are cached per device and shared by plans; this frees every cache entry no live plan
 * holds (returns the MiB released). */
int pxm_tables_trim(void);

/* ---- host-side setup helpers (no GPU needed) ------------------------------ */
/* pys2let.pys2let_j_max(B, L, J_min)            (pxmcmc/transforms.py:75) */
int pxm_j_max(int L, double B);
/* multiresolution bandlimits [scaling, j=J_min..J_max] (pxmcmc/utils.py:116-125);
 * writes at most cap entries, returns the count or <0 */
int pxm_wav_bandlimits(int L, double B, int J_min, int* bl_out, int cap);
/* number of wavelet+scaling coefficients  (pxmcmc/transforms.py:156-166) */
int64_t pxm_wav_ncoefs(int L, double B, int J_min, int64_t* nscal_out);
/* axisymmetric tiling: kappa0[L], kappa[(J_max+1)*L]  (pys2let.wavelet_tiling,
 * pxmcmc/utils.py:117; prior.py:121,132) */
int pxm_tiling_axisym(int L, double B, int J_min, double* kappa0, double* kappa);
/* MW quadrature weight per ring q[L] (pxmcmc/utils.py:262-283: mw_map_weights = outer(q, 1)) */
int pxm_mw_ring_weights(int L, double* q);
/* dense per-m ring tables for tests (small L): Binv[t*L+el] = (-1)^s N_el d^el_{m,-s}(theta_t),
 * Afwd[el*L+t] = exact-quadrature forward matrix; either pointer may be NULL */
int pxm_host_sht_tables(int L, int spin, int m, double* Binv, double* Afwd);
/* the same Binv[t*L+el] as the table-free recursion kernels generate it (csrc/rec_core.h: three-term recursion in el in
 * double precision on a per-ring scaled state; host emulation, operation for operation): what pyssht.inverse /
 * inverse_adjoint (pxmcmc/measurements.py:225,237) multiply by when a plan takes the recursion path */
int pxm_host_rec_table(int L, int spin, int m, double* Brec);
/* the launch geometry the recursion kernels of a plan (L, spin, C chains) would take, PXM_REC_R included: out[4] = {ring
 * blocks per wavefront R, complex columns per stored order NC, wavefronts per workgroup, LDS bytes of the ring -> el
 * kernel}; -1 (pxm_last_error) when the size has none and the plan stays on the ring tables.  No GPU needed. */
int pxm_host_rec_geometry(int L, int spin, int C, int* out);
/* tables of the exact-length phi-DFT unit for ring length 511 = 7 x 73 (csrc/dft_pfa.h; the phi stage of
 * pys2let.synthesis_wav2px / synthesis_adjoint_px2wav at bandlimit 256, pxmcmc/transforms.py:126,138): idx[(64 + 80) * 8]
 * uint16 gather / scatter offsets, b2[8 * 9 * 2] the spectrum of Rader's filter; for the CPU test against
 * scripts/dev/proto_pfa511.py */
int pxm_host_pfa511_tables(uint16_t* idx, double* b2);
/* what the phi-DFT stage of a plan at bandlimit L (ring length n = 2L-1) runs on, PXM_DFT_NO_W and PXM_DFT_PFA included:
 * out[6] = {unit (0 radix-2, 1 pair, 2 quad), length M of the Bluestein transform, chains per workgroup (radix-2: R; quad: 2,
 * and 1 for a single chain) or rings per workgroup (pair: 8 / r0 with M = 128 r0; 2 for the exact-length body), threads per
 * workgroup, LDS bytes per workgroup, 1 when n = 511 takes the exact-length body}.  It is the function every plan's creation
 * calls.  -1 (pxm_last_error names L, M and the bytes) where the unit needs more LDS than a CU has: L >= 1025, which every
 * plan constructor refuses with the same text.  No GPU needed. */
int pxm_host_dft_geometry(int L, int* out);
/* whether a fused rings -> X' -> rings launch of the phi-DFT stage is the STOCK MYULA update, which the pair unit runs on
 * kernels that hold the update's mode at compile time (csrc/sht_core.h: dft_step_is_stock -- the predicate the launchers
 * call): fields = which optional operands the launch carries, bit 0 the state X (fused update), 1 the threshold vector T,
 * 2 injected noise, 3 the device-resident iteration addend, 4 / 5 residual data / inverse covariance, 6 / 7 gather index /
 * weight; mode one of PXM_MODE_*; chain0 the id of the first chain.  1: stock -- X, T and the addend present, none of the
 * others, PXM_MODE_REAL_PAIRS and an even chain0; 0 otherwise.  PXM_DFT_STOCK=0 at plan creation keeps every launch on the
 * generic kernels.  No GPU needed. */
int pxm_host_dft_step_is_stock(unsigned fields, int mode, uint64_t chain0);

/* ---- spin spherical-harmonic transforms on the MW grid ---------------------- */
/* replaces pyssht.forward / inverse / inverse_adjoint / forward_adjoint
 * (pxmcmc/measurements.py:223,225,237,239).  flm: [C][L*L] c128, f: [C][L*(2L-1)] c128. */
int pxm_sht_plan_create(int L, int spin, int max_chains, unsigned flags, pxm_sht_plan_t* plan);
int pxm_sht_plan_destroy(pxm_sht_plan_t plan);
/* Non-zero when the plan's inverse / inverse_adjoint (pyssht.inverse / inverse_adjoint, pxmcmc/measurements.py:225,237) run the
 * table-free ring stage -- Wigner rows by three-term recursion in el on the vector pipe, csrc/sht_rec.hip -- instead of the
 * ring-table GEMM: 16 * (ring blocks per wavefront) + (complex columns per order).  Chosen at plan creation: few-column
 * plans at large L; PXM_REC=1 / 0 forces it on (where the column count allows) / off. */
int pxm_sht_uses_recursion(pxm_sht_plan_t plan);
/* self-test of the wavefront transpose-reduce of the ring -> el recursion kernel: out128[lane] = the sum the lane holds for
 * 16 known per-lane values, out128[64 + lane] = the id of the value it claims to hold (test aid) */
int pxm_rec_reduce_selftest(double* out128);
int pxm_sht_inverse(pxm_sht_plan_t plan, const void* flm, void* f, int C, pxm_stream_t stream);
int pxm_sht_forward(pxm_sht_plan_t plan, const void* f, void* flm, int C, pxm_stream_t stream);
int pxm_sht_inverse_adjoint(pxm_sht_plan_t plan, const void* f, void* flm, int C, pxm_stream_t stream);
int pxm_sht_forward_adjoint(pxm_sht_plan_t plan, const void* flm, void* f, int C, pxm_stream_t stream);
/* bytes of Legendre/Wigner ring table one transform launch streams (roofline accounting) */
int64_t pxm_sht_table_bytes(pxm_sht_plan_t plan, int op /*0 inv,1 fwd,2 inv_adj,3 fwd_adj*/);

/* ---- the phi-DFT stage on its own ---------------------------------------------------------------------------------
 * The stage of every transform above between the image and the rings (the FFTs over phi inside pyssht.forward / inverse,
 * pxmcmc/measurements.py:223,225), as a plan without ring tables, task lists or workspace: the same unit selection
 * (pxm_host_dft_geometry; PXM_DFT_NO_W and PXM_DFT_PFA are read at creation) and the same launches as an SHT plan at L.
 *   f : [C][L][2L-1] c128, the image of a chain
 *   G : [2L-1][Rp][Cp] c128, caller-owned, 16-byte aligned: order m = -(L-1) .. L-1, ring t, chain c, with
 *       Rp = roundup(L, 16) rows and Cp = roundup(max_chains, 8) columns (the internal ring layout, not repacked)
 *   pxm_dft_px2ring  G[m][t][c] = sum_p f[c][t][p] exp(-i m phi_p), phi_p = 2 pi p / (2L-1); for t < L every column is written:
 *                    c >= C with zeros; rows t >= L are left as they are
 *   pxm_dft_ring2px  f[c][t][p] = sum_m G[m][t][c] exp(+i m phi_p); rows t >= L and columns c >= C of G never enter a result
 * pxm_dft_status reads the plan's status word as pxm_sht_status does.
 * The _ex pair runs the same launches with the pixel side and the ring array a weak-lensing or wavelet plan gives them:
 *   G      : [2L-1][Rp][ncol / 2] c128 with ncol one of 2, 4, 6, 8 or a multiple of 16 doubles per row, C <= ncol / 2
 *   f      : [C][chain_stride] c128; the image of a chain is its elements [ring0, ring0 + L (2L-1))
 *   data, invcov (px2ring only, together): G <- rings of invcov .* (f - data); [chain_stride] each, read at the image's
 *            own offsets, invcov real or (invcov_complex) complex
 *   gidx   : int32 [L (2L-1)], pixel -> entry of the data vector, < 0 masked; then f (and data, invcov) are data-space
 *            arrays with chain_stride == ndata >= 1 and ring0 == 0: px2ring reads pixel e from entry gidx[e] (masked: zero),
 *            ring2px writes pixel e to entry gidx[e] (masked: dropped; entries no pixel maps to are left as they are).
 *            Every entry must be < ndata: the caller's duty (ops.DftPlan checks it on the device)
 *   gw     : float64 [ndata] weight of the entry a pixel maps to, or null (needs gidx)
 * Every other combination is refused before a launch. */
int pxm_dft_plan_create(int L, int max_chains, pxm_dft_plan_t* plan);
int pxm_dft_plan_destroy(pxm_dft_plan_t plan);
int pxm_dft_px2ring(pxm_dft_plan_t plan, const void* f, void* G, int C, pxm_stream_t stream);
int pxm_dft_ring2px(pxm_dft_plan_t plan, const void* G, void* f, int C, pxm_stream_t stream);
int pxm_dft_px2ring_ex(pxm_dft_plan_t plan, const void* f, int64_t chain_stride, int64_t ring0, const void* data, const void* invcov,
                       int invcov_complex, const int32_t* gidx, const double* gw, int64_t ndata, void* G, int ncol, int C,
                       pxm_stream_t stream);
int pxm_dft_ring2px_ex(pxm_dft_plan_t plan, const void* G, int ncol, void* f, int64_t chain_stride, int64_t ring0, const void* data,
                       const void* invcov, int invcov_complex, const int32_t* gidx, const double* gw, int64_t ndata, int C,
                       pxm_stream_t stream);
int pxm_dft_status(pxm_dft_plan_t plan, int clear, pxm_stream_t stream);

/* ---- HEALPix ring synthesis (csrc/healpix.hip) ---------------------------------------------------
 * The measurement "band-limited signal -> values at the HEALPix pixel centres" and its exact adjoint, RING order (what the
 * reference prepares with healpy.map2alm, experiments/weaklensing/main.py:23-37, without the inexact analysis):
 *   pxm_hpx_synthesis          v[c][p]   = sum_lm sY_lm(theta_p, phi_p) flm[c][l^2 + l + m]
 *   pxm_hpx_synthesis_adjoint  flm[c][.] = sum_p conj(sY_lm(theta_p, phi_p)) v[c][p]          (no quadrature weight)
 *   flm : [C][L*L] c128,  v : [C][12 nside^2] c128, both 16-byte aligned; every element of the output is written.
 * There are R = 4 nside - 1 rings, north to south, i = 1 .. R with i' = min(i, 4 nside - i): polar caps (i' < nside) have
 * nphi = 4 i', z = 1 - i'^2 / (3 nside^2), phi_j = (pi / (2 i')) (j + 1/2); the belt has nphi = 4 nside,
 * z = 4/3 - 2 i' / (3 nside), phi_j = (pi / (2 nside)) (j + 1/2) for even i' - nside and (pi / (2 nside)) j for odd; the
 * southern rings change the sign of z.  Refused: L > 1024, |spin| >= L, nside < 1, nside above out[3] of
 * pxm_host_hpx_geometry (the longest ring must fit the LDS of a phi-stage workgroup).
 *   pxm_host_hpx_geometry  out[6] = rings, pixels, LDS bytes of a phi-stage workgroup, largest nside, threads, padded rings
 *   pxm_host_hpx_rings     per ring: nphi, theta, phi of the first pixel, index of the first pixel     (arrays of 4 nside - 1)
 *   pxm_host_hpx_lambda    out[t][l] = (-1)^s sqrt((2l+1)/4pi) d^l_{m,-s}(theta[t]), l < L: the table recursion the plan uses
 *   pxm_hpx_table_bytes    device bytes of the Legendre table and twiddles the plan holds
 *   pxm_hpx_status         the plan's status word, as pxm_sht_status (no kernel of this plan has a bounded wait: always 0) */
int pxm_host_hpx_geometry(int L, int nside, int64_t* out);
int pxm_host_hpx_rings(int nside, int* nphi, double* theta, double* phi0, int64_t* start);
int pxm_host_hpx_lambda(int L, int spin, int m, const double* theta, int nt, double* out);
int pxm_hpx_plan_create(int L, int nside, int spin, int max_chains, pxm_hpx_plan_t* plan);
int pxm_hpx_plan_destroy(pxm_hpx_plan_t plan);
int pxm_hpx_synthesis(pxm_hpx_plan_t plan, const void* flm, void* v, int C, pxm_stream_t stream);
int pxm_hpx_synthesis_adjoint(pxm_hpx_plan_t plan, const void* v, void* flm, int C, pxm_stream_t stream);
int64_t pxm_hpx_table_bytes(pxm_hpx_plan_t plan);
int pxm_hpx_status(pxm_hpx_plan_t plan, int clear, pxm_stream_t stream);

/* ---- the ring-GEMM stage on its own -------------------------------------------------------------------------------
 * The Legendre stage of every transform above (csrc/sht_gemm.hip) as a plan without DFT stage, wavelet kernels or samplers:
 * ring tables from the shared cache, one workspace and ONE task list, built, ordered (PXM_GEMM_ORDER is read at creation),
 * range-checked, uploaded and launched by the code every other plan uses.  How the test suite holds each kernel variant to
 * a long-double model of the contraction ("Error model and tests of the ring GEMM").
 * A list is n_sides sides appended in order (pk = 0), or one side / a pair of sides sharing a table in packed form (pk = 2,
 * 4: live columns per slab; 2 * max_chains <= pk).  Side i is sides[PXM_GEMM_SIDE_INTS * i + ..]:
 *   0 table kind (0 inverse, 1 forward, 2 inverse adjoint, 3 forward adjoint, 4 Gram, 5 parity-split Gram, 6 the same with
 *     order 0 split and its pole term)            1 bandlimit of the tables and the ring side
 *   2 bandlimit of the harmonic-side array, 0 = the same     3 second operand   4 per-k operand scale   5 per-row result scale
 *   6, 7 row mask [row_lo, row_hi), row_hi <= 0 = none       8 support cut el_lo    9 data term (complex per row, stride 2)
 *   10, 11 doubles per row of the operand / result array, 0 = 2 * roundup(max_chains, 8) (packed lists only)
 *   12, 13 index of the earlier side whose operand(s) / result and data term this side shares, -1 = arrays of its own
 *   14, 15 zero
 * Arrays are [2 L' - 1][roundup(L', 16)][doubles per row] at the bandlimit L' of their side of the table.
 * pxm_gemm_plan_report writes min(cap, n) of its n int64 words to out and returns n:
 *   what 0: {ncol, sides, tasks, list flags (1 second operand, 2 scale, 4 pole), kernel slabs, pk, workspace doubles, offset and
 *           doubles of the scratch row block, offset of the 8-byte counter, max_chains, +-m pairs, 0 x 4}, then 16 per side:
 *           offsets of operand, second operand, result, k scale, row scale, data term (-1 = none), then L', rows, doubles
 *           per row of the operand and of the result array, doubles of both, doubles of the tiled table and of the pole column
 *   what 1: 16 per task in launch order, padding entries (n_rt = 0) included: {m_unit, row0, n_rt, k_beg, k_end, pole_n, nslab,
 *           side, parity half (-1 none), row_lo, row_hi of slab group 0 and of group 1, sign1, second side of a packed pair
 *           (-1 none), order m}
 *   what 2: the tiled table of `side` (layout: top of csrc/sht_gemm.hip): {stored orders, Rp, +-m pairs, doubles, doubles of
 *           the pole column, L, spin, kind, then per stored order: m, m_off, k_beg, odd_off (-1: stored dense), odd_k_beg}
 * pxm_host_gemm_plan_report: the same report of a plan created in dry-run mode (no GPU; address ranges checked as at every
 * creation), < 0 where the creation refuses.
 * pxm_gemm_plan_write / _read copy n doubles device-to-device into / out of the workspace at `offset` (refused outside it);
 * pxm_gemm_plan_table_read copies the first n doubles of the tiled table (which = 0) or the pole column (1) of a side.
 * pxm_gemm_plan_run launches the list once for C chains over every column group with a live chain; affine != 0: the epilogue
 * out = w (ns acc - data term) with w = wr + i wi per chain, columns >= 2 C zero; bump != 0: the counter advances by one. */
#define PXM_GEMM_SIDE_INTS 16
int pxm_gemm_plan_create(int spin, int max_chains, int pk, const int* sides, int n_sides, pxm_gemm_plan_t* plan);
int pxm_gemm_plan_destroy(pxm_gemm_plan_t plan);
int64_t pxm_gemm_plan_report(pxm_gemm_plan_t plan, int what, int side, int64_t* out, int64_t cap);
int64_t pxm_host_gemm_plan_report(int spin, int max_chains, int pk, const int* sides, int n_sides, int what, int side,
                                  int64_t* out, int64_t cap);
int pxm_gemm_plan_write(pxm_gemm_plan_t plan, int64_t offset, const double* src, int64_t n, pxm_stream_t stream);
int pxm_gemm_plan_read(pxm_gemm_plan_t plan, int64_t offset, double* dst, int64_t n, pxm_stream_t stream);
int pxm_gemm_plan_table_read(pxm_gemm_plan_t plan, int side, int which, double* dst, int64_t n, pxm_stream_t stream);
int pxm_gemm_plan_run(pxm_gemm_plan_t plan, int C, int affine, double ns, double wr, double wi, int bump, pxm_stream_t stream);

/* ---- scale-discretised wavelet transform (N=1, upsample=0) -------------------- */
/* replaces pys2let.synthesis_wav2px / synthesis_adjoint_px2wav / analysis_px2wav /
 * analysis_adjoint_wav2px (pxmcmc/transforms.py:95-98).  X: [C][ncoefs] c128, f: [C][L*(2L-1)] c128.
 * pxm_wav_plan_create is the spin-0 plan; pxm_wav_plan_create_spin takes the spin s of the images (|s| < L): the
 * coefficients stay spin-0 functions in the same layout, only the ring stage at L runs at spin s.
 * A spin-s plan (s != 0) refuses pxm_wav_wl_attach and mode 2 (two real chains per slot) of the fused steps. */
int pxm_wav_plan_create(int L, double B, int J_min, int max_chains, unsigned flags, pxm_wav_plan_t* plan);
int pxm_wav_plan_create_spin(int L, double B, int J_min, int spin, int max_chains, unsigned flags, pxm_wav_plan_t* plan);
int pxm_wav_plan_destroy(pxm_wav_plan_t plan);
int pxm_wav_synthesis(pxm_wav_plan_t plan, const void* X, void* f, int C, pxm_stream_t stream);
int pxm_wav_synthesis_adjoint(pxm_wav_plan_t plan, const void* f, void* X, int C, pxm_stream_t stream);
int pxm_wav_analysis(pxm_wav_plan_t plan, const void* f, void* X, int C, pxm_stream_t stream);
int pxm_wav_analysis_adjoint(pxm_wav_plan_t plan, const void* X, void* f, int C, pxm_stream_t stream);
int64_t pxm_wav_table_bytes(pxm_wav_plan_t plan, int op /*0 synthesis,1 synthesis_adjoint*/);

/* ---- directional scale-discretised wavelet transform (N = dirs >= 1, spin 0, upsample=0) ------------------------
 * replaces pys2let.synthesis_wav2px / synthesis_adjoint_px2wav / analysis_px2wav / analysis_adjoint_wav2px with
 * N > 1 (pxmcmc/transforms.py:95-98).  X: [C][ncoefs] c128, f: [C][L*(2L-1)] c128.  Layout
 * [scaling | j = J_min .. J_max]: the scaling block is the MW grid at bl_scal; block j holds 2N-1 MW grids at bl_j,
 * orientation-major [c][theta][phi] with gamma_c = 2 pi c / (2N-1).  With N = 1 the layout and the values are those of
 * the pxm_wav_* plan.  The plan owns its inner SHT plans (one per (bl_j, -n)), the spin-0 plan at L and all scratch:
 * nothing is allocated after creation; every call is enqueued on the given stream (graph-capturable). */
int pxm_dwav_plan_create(int L, double B, int J_min, int N, int max_chains, unsigned flags, pxm_dwav_plan_t* plan);
int pxm_dwav_plan_destroy(pxm_dwav_plan_t plan);
int pxm_dwav_synthesis(pxm_dwav_plan_t plan, const void* X, void* f, int C, pxm_stream_t stream);
int pxm_dwav_synthesis_adjoint(pxm_dwav_plan_t plan, const void* f, void* X, int C, pxm_stream_t stream);
int pxm_dwav_analysis(pxm_dwav_plan_t plan, const void* f, void* X, int C, pxm_stream_t stream);
int pxm_dwav_analysis_adjoint(pxm_dwav_plan_t plan, const void* X, void* f, int C, pxm_stream_t stream);
/* host-only: number of coefficients of the directional layout (pxmcmc/transforms.py:156-166), scaling block in *nscal_out */
int64_t pxm_dwav_ncoefs(int L, double B, int J_min, int N, int64_t* nscal_out);
/* device bytes of the tables the plan reads: its inner plans' Wigner tables (shared per (L, spin)) + its own weights and
 * phases */
int64_t pxm_dwav_table_bytes(pxm_dwav_plan_t plan);
/* OR of the status words of the inner SHT plans (as pxm_sht_status); synchronises */
int pxm_dwav_status(pxm_dwav_plan_t plan, int clear, pxm_stream_t stream);
/* launch shapes (test / timing aid): (block, n) items, workgroups per chain of the harmonic-split and gamma launches */
int pxm_dwav_plan_info(pxm_dwav_plan_t plan, int* nitems, int* split_blocks, int* gamma_blocks);
/* Test hooks of the directional plan: its workspace and one stage of one operator at a time ("Error model and
 * tests of the orientation stages").  The workspace is one complex128 array; offsets and sizes count complex elements.
 * pxm_dwav_workspace_layout writes min(cap, n) of its n int64 words to out and returns n:
 *   {workspace elements, offset and elements of the flm region [max_chains][L*L], offset of the harmonic arena, of the pixel
 *    arena, items, blocks, max_chains}, then 8 per item in plan order: {block, n, bl, offset of chain 0 of the harmonic
 *    operand, its elements per chain (bl^2), offset of chain 0 of the pixel operand, its elements per chain (bl (2 bl - 1)),
 *    0}; chain c of an operand follows chain c - 1; then 8 per block of the gamma stage: {offset in a chain's coefficient
 *    vector, pixels per plane, planes, orientations, first workgroup, first entry of its row of the g-offset table, 0, 0};
 *    then the g-offset table as uploaded, blocks * N entries: per orientation of a block the offset of g_n in the pixel
 *    arena, or -1 for a skipped pair.
 * pxm_dwav_workspace_write / _read copy n elements device-to-device into / out of the workspace at `offset` (refused
 * outside it).  pxm_dwav_run_stage enqueues stage 0 .. 3 of operator op (0 analysis, 1 analysis_adjoint, 2 synthesis,
 * 3 synthesis_adjoint) alone, through the calls the operator makes, in the operator's order: the SHT at L (reads or writes
 * f = x, [C][L (2L-1)]), the harmonic split or merge, the inner SHTs of every item, the gamma stage (reads or writes
 * X = x, [C][ncoefs]); x may be null for the two inner stages. */
int64_t pxm_dwav_workspace_layout(pxm_dwav_plan_t plan, int64_t* out, int64_t cap);
int pxm_dwav_workspace_write(pxm_dwav_plan_t plan, int64_t offset, const void* src, int64_t n, pxm_stream_t stream);
int pxm_dwav_workspace_read(pxm_dwav_plan_t plan, int64_t offset, void* dst, int64_t n, pxm_stream_t stream);
int pxm_dwav_run_stage(pxm_dwav_plan_t plan, int op, int stage, void* x, int C, pxm_stream_t stream);
/* host-only: the tables the harmonic and gamma stages read, as the plans upload them.
 *   pxm_host_harm_weights  the rows of the split (wa) and merge (ws) weights, [rows][L] complex each, item by item in plan
 *                          order: harmonic = 0 the directional plan (spin 0; the pairs |n| >= bl_j are skipped), 1 the
 *                          harmonic plan; rows[3 i ..] = (block, n, bl) of row i.  Returns the number of rows; writes only
 *                          when cap >= that number.
 *   pxm_host_dir_component the directionality component s_lm [L*L] complex that the rows are built from
 *   pxm_host_dwav_phases   ph[q][k] = e^{i n_k gamma_q}, [2N-1][N] complex, n_k = -(N-1) + 2k, gamma_q = 2 pi q / (2N-1) */
int64_t pxm_host_harm_weights(int L, double B, int J_min, int N, int spin, int harmonic, double* wa, double* ws, int* rows,
                              int64_t cap);
int pxm_host_dir_component(int L, int N, double* s);
int pxm_host_dwav_phases(int N, double* ph);

/* Harmonic-space wavelet transforms (pys2let analysis_lm2lmn / synthesis_lmn2lm and their adjoints):
 * inputs and outputs are spherical-harmonic coefficients.  f_lm [C][L*L] (ssht index l^2 + l + m, spin-s coefficients);
 * X [C][ncoefs] = [scaling: bl_0^2 | j = J_min .. J_max: n = -(N-1), -(N-3), .., N-1: bl_j^2 each], every block
 * ssht-indexed.
 *   analysis   W^{j,n}_lm = sqrt(8 pi^2/(2l+1)) kappa_j(l) conj(s_ln) f_lm,   S_lm = kappa_0(l) f_lm
 *   synthesis  f_lm = kappa_0(l) S_lm + sum_{j,n} sqrt((2l+1)/(8 pi^2)) kappa_j(l) s_ln W^{j,n}_lm
 * and the two conjugate transposes.  Entries with l < max(|n|, |spin|) are zero after analysis and ignored by synthesis.
 * N >= 1 at spin 0, N = 1 at any |spin| < L.  No SHT plan; nothing is allocated after creation; every call runs on the
 * given stream (graph-capturable).  Outputs must not alias inputs. */
int pxm_hwav_plan_create(int L, double B, int J_min, int N, int spin, int max_chains, unsigned flags, pxm_hwav_plan_t* plan);
int pxm_hwav_plan_destroy(pxm_hwav_plan_t plan);
int pxm_hwav_synthesis(pxm_hwav_plan_t plan, const void* X, void* flm, int C, pxm_stream_t stream);
int pxm_hwav_synthesis_adjoint(pxm_hwav_plan_t plan, const void* flm, void* X, int C, pxm_stream_t stream);
int pxm_hwav_analysis(pxm_hwav_plan_t plan, const void* flm, void* X, int C, pxm_stream_t stream);
int pxm_hwav_analysis_adjoint(pxm_hwav_plan_t plan, const void* X, void* flm, int C, pxm_stream_t stream);
/* host-only: number of coefficients of the harmonic layout, scaling block (bl_0^2) in *nscal_out */
int64_t pxm_hwav_ncoefs(int L, double B, int J_min, int N, int64_t* nscal_out);
/* no bounded waits: 0 for a valid plan */
int pxm_hwav_status(pxm_hwav_plan_t plan, int clear, pxm_stream_t stream);
/* One MYULA iteration of the synthesis setting with a harmonic plan, a measurement diagonal in (l, m) and a diagonal
 * inverse covariance, in one kernel (one lane per (chain, lm)):
 *   preds = k .* synthesis(X);  g = k .* invcov .* (preds - data);  X_out = MYULA update of X with the gradient
 *   synthesis_adjoint(g) (soft threshold T / T_scalar, Philox noise keyed (seed, chain0 + c, coefficient, iter + *iter_dev)
 *   as pxm_myula_step);  preds_out = k .* synthesis(X_out).
 * kernel: null (identity measurement) or the weak-lensing kernel k_l [L*L], applied with l < 2 zeroed.  data [L*L]
 * complex; invcov [L*L] real or complex (invcov_complex).  mode: PXM_MODE_REAL_NOISE or PXM_MODE_CPLX_NOISE, optionally
 * OR PXM_NOISE_F64 (PXM_MODE_REAL_PAIRS is refused: harmonic coefficients are never real).  iter_dev may be null. */
int pxm_hwav_myula_step(pxm_hwav_plan_t plan, const void* X, const void* data, const void* invcov, int invcov_complex,
                        const double* kernel, const double* T, double T_scalar, double delta, double lmda, int mode,
                        uint64_t seed, uint64_t chain0, uint64_t iter, const uint64_t* iter_dev, void* X_out,
                        void* preds_out, int C, pxm_stream_t stream);
/* launch shape (test / timing aid): items, workgroups per chain of the split launch, most items with a non-zero weight at
 * one degree (the register count of the fused step) */
int pxm_hwav_plan_info(pxm_hwav_plan_t plan, int* nitems, int* split_blocks, int* kact);

/* Device-resident Philox iteration counter OF ONE PLAN (HIP-graph replay of the MYULA step): when registered,
 * the plan's fused steps use iteration = iter + *counter, read on the device at execution time, so a captured
 * graph draws fresh noise at every replay.  Two plans (two samplers) in one process never share a counter.
 * pxm_wav_iter_counter_add enqueues "*counter += inc" on the stream.  A plan holds ONE live counter: registering
 * a different one while another is live is an error (two stepping engines on one plan would redirect each other's
 * noise stream); NULL unregisters unconditionally, pxm_wav_release_iter_counter only if `counter_dev` is still the
 * registered one (the owner's teardown call: never drops somebody else's counter). */
int pxm_wav_set_iter_counter(pxm_wav_plan_t plan, uint64_t* counter_dev);
int pxm_wav_release_iter_counter(pxm_wav_plan_t plan, const uint64_t* counter_dev);
int pxm_wav_iter_counter_add(pxm_wav_plan_t plan, uint64_t inc, pxm_stream_t stream);
/* Device status of a plan.  The wave pairs of the fused phi-DFT kernels (csrc/dft_wave.h, d5_pair_sync: an LDS counter
 * per pair) wait on each other with BOUNDED spins instead of barriers.  A wait that expires does not hang the GPU -- the
 * kernel runs on with data its partner has not written -- and ORs a bit into the plan's status word; the results of
 * that launch are invalid.  The reference fails loudly on bad state (pxmcmc/mcmc.py:104-109); so does the sampler here:
 * it reads the word wherever it already synchronises (saved samples, progress prints, end of run) and raises.
 *   pxm_wav_status / pxm_sht_status : bit mask since the last clear, 0 = every wait was satisfied; `clear` != 0 resets
 *                                     it after reading.  Synchronises the stream.  < 0: error.  Bit 0 is unused.
 * PXM_DEBUG_PAIR_SYNC_LIMIT=<n> (read at plan creation) sets the bound of the pair wait; 0 forces every wait to
 * expire -- the test of this report path. */
#define PXM_STATUS_PAIR_SYNC 2
int pxm_wav_status(pxm_wav_plan_t plan, int clear, pxm_stream_t stream);
int pxm_sht_status(pxm_sht_plan_t plan, int clear, pxm_stream_t stream);
/* scales whose 511-point rings the fused rings -> X' -> rings launch takes through the exact-length phi-DFT unit (0: Bluestein) */
int pxm_wav_exact_dft_scales(pxm_wav_plan_t plan);
/* 1 when that launch runs stock MYULA updates (pxm_host_dft_step_is_stock) on the STOCK kernel instantiation; 0 with
 * PXM_DFT_STOCK=0 at plan creation or without a grouped launch: every update on the generic kernels */
int pxm_wav_dft_stock(pxm_wav_plan_t plan);
/* Cache policies of the plan's ring-space step (csrc/mem_policy.h): a mask of the streams whose accesses the plan's launches
 * issue non-temporal -- bit 0: the X' stores of the fused phi-DFT step (its STOCK kernel instantiation).
 * 0 with PXM_MEM_POLICY=0 at plan creation, or without that instantiation (pxm_wav_dft_stock): every launch on the
 * default-policy kernels (the identity test). */
int pxm_wav_mem_policy(pxm_wav_plan_t plan);

/* Live kernel timing of one plan (bench.py roofline leg).  pxm_wav_profile_enable(plan, n) with n > 0 creates
 * n event pairs per kernel class; while enabled every SHT ring-GEMM launch and every grouped phi-DFT launch of
 * this plan is bracketed by a pair on the stream it is launched on (kernel start / stop, as rocprofv3 reports
 * them).  The read calls synchronise the events and return the summed kernel time (ms), the number of
 * launches, the algorithmic bytes moved and the MFMA flops (any pointer may be NULL), then reset.
 * n = 0 disables and releases the events. */
int pxm_wav_profile_enable(pxm_wav_plan_t plan, int max_launches);
int pxm_wav_profile_read(pxm_wav_plan_t plan, double* gemm_ms, int64_t* gemm_launches, double* gemm_alg_bytes,
                         double* gemm_flops);
int pxm_wav_profile_read_dft(pxm_wav_plan_t plan, double* dft_ms, int64_t* dft_launches, double* dft_alg_bytes);
/* per-launch form of pxm_wav_profile_read (instead of it): kernel time (ms), algorithmic bytes and (optional, may be
 * NULL) workgroup count of each of the first `cap` ring-GEMM launches, in launch order -- the workgroup count is the
 * key a rocprofv3 record of the same launch carries; *launches = how many were bracketed; then resets */
int pxm_wav_profile_read_launches(pxm_wav_plan_t plan, double* launch_ms, double* launch_alg_bytes,
                                  int32_t* launch_workgroups, int64_t cap, int64_t* launches);
/* test aid: number of non-finite doubles in the plan's workspace (ring / harmonic arrays incl. the padding
 * chains' columns); synchronises the stream */
int64_t pxm_wav_workspace_nonfinite(pxm_wav_plan_t plan, pxm_stream_t stream);
/* test aid: the plan's workspace -- every ring and harmonic array of its stages, padding columns included -- copied to the
 * device array out (at most cap doubles); returns the number of doubles the workspace holds, < 0 on error */
int64_t pxm_wav_workspace_read(pxm_wav_plan_t plan, double* out, int64_t cap, pxm_stream_t stream);

/* Fused MYULA half-steps (pxmcmc/mcmc.py:158-161 with forward.py:66-72, prior.py:49-50):
 *   pxm_wav_gradg_step: X_out = (1-d/l) X + (d/l) soft(X,T) - d * S^H( invcov .* (preds - data) ) + sqrt(2 d) w
 * i.e. calc_gradg + proxf + chain_step in one pass over the coefficient vector, with the
 * residual folded into the transform's input read and the update into its output write.
 * data/invcov: [P] shared by all chains (invcov complex iff invcov_complex); T: [N] or NULL
 * (then T_scalar); noise: [C][N] injected N(0,1) or NULL for the Philox stream keyed
 * (seed, chain0 + c, iter).  mode (how a complex128 slot of the state is read):
 *   PXM_MODE_REAL_NOISE 0  complex state, real noise (float64 [C][N] when injected): params.complex = False
 *   PXM_MODE_CPLX_NOISE 1  complex state, complex noise (c128 [C][N]):                params.complex = True
 *   PXM_MODE_REAL_PAIRS 2  real data and real state: slot c carries the two REAL chains 2c (real part) and
 *                          2c+1 (imaginary part) through the complex-linear transforms; soft threshold and
 *                          noise are applied per component (injected noise: float64 [2C][N]; Philox keys
 *                          chain0 + 2c and chain0 + 2c + 1); data must then be passed as d + i d.
 * | PXM_NOISE_F64: the Philox stream's Box-Muller step in double precision (see pxm_noise_bits above). */
#define PXM_MODE_REAL_NOISE 0
#define PXM_MODE_CPLX_NOISE 1
#define PXM_MODE_REAL_PAIRS 2
int pxm_wav_gradg_step(pxm_wav_plan_t plan, const void* X, const void* preds, const void* data,
                       const void* invcov, int invcov_complex, const double* T, double T_scalar,
                       double delta, double lmda, const void* noise, int mode,
                       uint64_t seed, uint64_t chain0, uint64_t iter, void* X_out, int C,
                       pxm_stream_t stream);

/* The whole loop body pxmcmc/mcmc.py:158-161 for the identity measurement and a DIAGONAL (per-pixel) inverse
 * covariance: pxm_wav_gradg_step followed by pxm_wav_synthesis of the new state, fused.  The rings of the
 * residual invcov .* (preds - data) (pxmcmc/forward.py:66-69) are carried inside the plan between calls:
 *   pxm_wav_image_init : residual rings of the start state's preds                      (start of a run)
 *   pxm_wav_image_step : X_out = MYULA update of X (as pxm_wav_gradg_step); preds_out = forward(X_out);
 *                        residual rings <- those of preds_out.  Any other call on the plan invalidates the
 *                        carried rings (call pxm_wav_image_init again). */
int pxm_wav_image_init(pxm_wav_plan_t plan, const void* preds, const void* data, const void* invcov,
                       int invcov_complex, int C, pxm_stream_t stream);
int pxm_wav_image_step(pxm_wav_plan_t plan, const void* X, const void* data, const void* invcov,
                       int invcov_complex, const double* T, double T_scalar, double delta, double lmda,
                       const void* noise, int mode, uint64_t seed, uint64_t chain0, uint64_t iter,
                       void* X_out, void* preds_out, int C, pxm_stream_t stream);

/* Ring-space MYULA iteration: identity measurement + UNIFORM inverse covariance w (complex scalar), i.e.
 * ForwardOperator(data, scalar sig_d, "synthesis", SphericalWaveletTransform, Identity).  Between
 * forward() and calc_gradg() the reference forms the image-space residual w (preds - data)
 * (pxmcmc/forward.py:63-72).  On every ring DFT o iDFT = (2L-1) I, so DFT(residual) =
 * w ((2L-1) G - DFT(data)) with G the rings of S X: the L-level iDFT / DFT pair is never executed and
 * the image `preds` is produced only on demand (saved iterations).  Results equal pxm_wav_gradg_step +
 * pxm_wav_synthesis to round-off.  The rings of the current state are carried inside the plan:
 *   pxm_wav_ring_set_data : rings of the data image (once per data set)
 *   pxm_wav_ring_init     : rings <- S X                           (start of a run)
 *   pxm_wav_ring_step     : X_out = MYULA update of X (as pxm_wav_gradg_step); rings <- S X_out.
 *                           The plan's iteration counter, if registered, is advanced by 1 at the START of the step
 *                           (the step's Philox iteration = iter + counter after the increment).
 *   pxm_wav_ring_preds    : preds = forward(X) of the carried state, [C][L(2L-1)] */
int pxm_wav_ring_set_data(pxm_wav_plan_t plan, const void* data, pxm_stream_t stream);
int pxm_wav_ring_init(pxm_wav_plan_t plan, const void* X, int C, pxm_stream_t stream);
int pxm_wav_ring_step(pxm_wav_plan_t plan, const void* X, double w_re, double w_im, const double* T,
                      double T_scalar, double delta, double lmda, const void* noise, int mode,
                      uint64_t seed, uint64_t chain0, uint64_t iter, void* X_out, int C, pxm_stream_t stream);
int pxm_wav_ring_preds(pxm_wav_plan_t plan, void* preds, int C, pxm_stream_t stream);

/* Weak-lensing measurement fused with the wavelet synthesis (BASELINE config 5; pxmcmc/forward.py:63-72 with
 * transform = SphericalWaveletTransform (transforms.py:114-139) and measurement = WeakLensing
 * (measurements.py:209-304)).  Between the synthesis and the measurement the reference runs an inverse SHT and
 * a forward SHT of the same band-limited field at the same bandlimit -- the identity on harmonic coefficients
 * (exact MW quadrature) -- so the harmonic kernel k_l is applied to the synthesised coefficients directly:
 *   pxm_wav_wl_attach  : spin-2 tables; pix2data [L(2L-1)] maps a pixel to its index in the masked data vector
 *                        (< 0 = masked; NULL = no mask, ndata = L(2L-1)); weight [ndata] = WeakLensing.inv_cov or
 *                        NULL.  Both stay caller-owned and must outlive the plan's use of them.  A failed attach
 *                        leaves the plan untouched and the call may be repeated; on a plan that has its attachment
 *                        a further call only re-points pix2data / weight / ndata.
 *   pxm_wav_wl_forward : gamma [C][ndata] = WeakLensing.forward(transform.inverse(X))
 *   pxm_wav_wl_adjoint : X_out [C][ncoefs] = transform.inverse_adjoint(WeakLensing.adjoint(g)), g = gamma, or the
 *                        residual invcov .* (gamma - data) when data / invcov ([ndata]) are given (calc_gradg). */
int pxm_wav_wl_attach(pxm_wav_plan_t plan, const int32_t* pix2data, const double* weight, int64_t ndata);
/* non-zero (as pxm_sht_uses_recursion) when the attached spin-2 stage of pxm_wav_wl_forward / _adjoint -- pyssht.inverse /
 * inverse_adjoint with Spin=2, pxmcmc/measurements.py:225,237 -- runs the table-free recursion kernels */
int pxm_wav_wl_uses_recursion(pxm_wav_plan_t plan);
int pxm_wav_wl_forward(pxm_wav_plan_t plan, const void* X, void* gamma, int C, pxm_stream_t stream);
int pxm_wav_wl_adjoint(pxm_wav_plan_t plan, const void* gamma, const void* data, const void* invcov,
                       int invcov_complex, void* X_out, int C, pxm_stream_t stream);

/* ---- elementwise / reductions ---------------------------------------------------- */
/* dtype: 0 = float64, 1 = complex128.  n = elements per chain. */
/* utils.soft (pxmcmc/utils.py:55-67,84-88): T vector [n] (shared by chains) or NULL -> T_scalar */
int pxm_soft(const void* X, const double* T, double T_scalar, void* out, int64_t n, int C, int dtype,
             pxm_stream_t stream);
/* ForwardOperator._gradg_analysis residual (pxmcmc/forward.py:66-69) with a diagonal invcov:
 * out = invcov .* (preds - data); data, invcov are [n] shared by all chains */
int pxm_residual_grad(const void* preds, const void* data, const void* invcov, int invcov_complex,
                      void* out, int64_t n, int C, int dtype, pxm_stream_t stream);
/* MYULA.chain_step fused with L1 prox (pxmcmc/mcmc.py:185-201 + prior.py:49-50).
 * delta_dev: per-chain step sizes [C] on the device or NULL -> delta.
 * iter_dev: caller-owned device iteration counter or NULL: the Philox iteration is iter + *iter_dev, read when the kernel
 * runs, so a HIP graph of an iteration replays with fresh noise once the captured sequence ends with pxm_counter_add
 * (MYULA's generic-operator stepping engine, pxmcmc/mcmc.py:157-164). */
int pxm_myula_step(const void* X, const void* gradg, const double* T, double T_scalar,
                   const double* delta_dev, double delta, double lmda, const void* noise,
                   int noise_complex, uint64_t seed, uint64_t chain0, uint64_t iter,
                   const uint64_t* iter_dev, void* X_out, int64_t n, int C, int dtype,
                   pxm_stream_t stream);
/* chain_step with proxf given (PxMALA keeps proxf of the current state, mcmc.py:231); iter_dev as pxm_myula_step */
int pxm_chain_step(const void* X, const void* proxf, const void* gradg, const double* delta_dev,
                   double delta, double lmda, const void* noise, int noise_complex, uint64_t seed,
                   uint64_t chain0, uint64_t iter, const uint64_t* iter_dev, void* X_out, int64_t n,
                   int C, int dtype, pxm_stream_t stream);
/* One stage of the SKROCK Chebyshev recursion (pxmcmc/mcmc.py:349-368 with the recursion coefficients of Pereyra,
 * Vargas-Mieles & Zygalakis 2020, not mcmc.py:370-383; the gradient of pxmcmc/mcmc.py:84-89 folded into a, b, c):
 *   out = a U + b P + c gradg + e V + r Z        (every array [C][n]; T [n] shared by chains)
 * P: b == 0 -> no term; proxf given -> P = proxf (analysis setting / user prior); proxf NULL -> P = soft(U, T or T_scalar)
 * as pxm_myula_step.  gradg, V: NULL -> no term.  Z: r == 0 -> no term (no noise code runs); noise given -> that array
 * (real, or complex with noise_complex); NULL -> the Philox stream of pxm_myula_step keyed (seed, chain0 + c, element,
 * iter [+ *iter_dev]), noise_complex = (0 | 1) | PXM_NOISE_F64 -- SKROCK.chain_step's randn [+ 1j randn]
 * (pxmcmc/mcmc.py:338-347).  out must not alias an input. */
int pxm_skrock_stage(const void* U, const void* proxf, const double* T, double T_scalar, const void* gradg,
                     const void* V, double a, double b, double c, double e, double r, const void* noise,
                     int noise_complex, uint64_t seed, uint64_t chain0, uint64_t iter, const uint64_t* iter_dev,
                     void* out, int64_t n, int C, int dtype, pxm_stream_t stream);
/* One FISTA iteration on the samplers' posterior (Beck & Teboulle 2009), every array [C][n]:
 *   V = Y - gamma gradg;  X_out = soft(V, T gamma / lmda) as pxm_myula_step forms it (T [n] shared by chains, or T_scalar)
 *   -- or proxf when given (analysis setting / user prior: Y, gradg, T are then not read);
 *   Y_out = X_out + beta (X_out - X_prev),  beta = beta_table[min(iter + *iter_dev, n_beta - 1)] read when the kernel runs
 *   (iter_dev: caller-owned device iteration counter or NULL, as pxm_myula_step), so a HIP graph replays with the momentum
 *   of its iteration.  sums [C][3] receives per chain sum |X_out - X_prev|^2, sum |X_out|^2 and sum T_i |X_out_i| (NaN with
 *   proxf given), added in a fixed order that depends on n only: a chain's sums do not depend on its batch.
 *   With n == 0 the sums are written as zeros (NaN for the third with proxf given).
 * scratch: caller-owned, 3 * PXM_FISTA_SLICES_MAX * C doubles.  X_out and Y_out must not overlap an input or each other
 * (only equal base pointers are detected and refused). */
#define PXM_FISTA_SLICES_MAX 256
int pxm_fista_step(const void* Y, const void* gradg, const void* proxf, const double* T, double T_scalar,
                   const void* X_prev, double gamma, double lmda, const double* beta_table, int64_t n_beta,
                   uint64_t iter, const uint64_t* iter_dev, void* X_out, void* Y_out, double* sums, double* scratch,
                   int64_t n, int C, int dtype, pxm_stream_t stream);
/* pxm_fista_step with adaptive (gradient) restart decided per chain on the device (O'Donoghue & Candes 2015; DESIGN.md
 * section 14).  The arguments and the arithmetic of X_out, Y_out and the first three sums are those of pxm_fista_step, except:
 *   beta = beta_table[min(momentum_index[c], n_beta - 1)]: momentum_index [C] is the chain's own index on the device, read
 *   by the step and then updated by the finishing kernel;
 *   sums is [C][4]: the three sums of pxm_fista_step, then r_c = sum_i Re conj(Y_i - X_out_i) (X_out_i - X_prev_i), its
 *   terms (y.re - x.re) d.re + (y.im - x.im) d.im formed without contraction and added in the same fixed order;
 *   after the step: restart_on != 0 and r_c > 0 (false for 0 and for NaN) -> momentum_index[c] = 0 and, with restarts [C]
 *   given (NULL: not counted), restarts[c] += 1; otherwise momentum_index[c] += 1.  Y_out keeps the momentum of the step that
 *   decided: the reset acts on the following step, which runs with beta_table[0].
 *   Y is needed with proxf given too (r_c reads it); gradg and T are still not read then.
 *   With n == 0 the sums are zeros (NaN for the third with proxf given) and the indices advance.
 * scratch: caller-owned, 4 * PXM_FISTA_SLICES_MAX * C doubles.  momentum_index, restarts and sums must be different arrays.
 * No atomics and no host read: a HIP graph replays it. */
int pxm_fista_step_restart(const void* Y, const void* gradg, const void* proxf, const double* T, double T_scalar,
                           const void* X_prev, double gamma, double lmda, const double* beta_table, int64_t n_beta,
                           uint64_t* momentum_index, uint64_t* restarts, int restart_on, void* X_out, void* Y_out,
                           double* sums, double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream);
/* The two elementwise steps of the forward-backward primal-dual iteration (Condat 2013; Vu 2013) on
 * g(x) + h(A x), h(u) = (1 / lmda) sum_i T_i |u_i|; every state array [C][n] (dual arrays [C][m]), float64 or complex128.
 * pxm_pd_primal_step, with G = gradg(X) and U = A^H v:
 *   s = G + U (rounded);  X1_out = fma(-tau, s, X);  Xbar_out = fma(2, X1_out, -X), per component;
 *   sums [C][2] = per chain sum |X1_out - X|^2, sum |X1_out|^2.
 *   scratch: caller-owned, 2 * PXM_FISTA_SLICES_MAX * C doubles.
 * pxm_pd_dual_step, with W = A xbar (T [m] shared by chains, or T_scalar; rscale = 1 / lmda in the iteration):
 *   w = fma(sigma, W, V) per component;  r_i = T_i rscale (rounded once);
 *   complex: a = sqrt(re(w)^2 + im(w)^2) (plain products and sum, no hypot), V1_out = a > r_i ? w (r_i / a) : w, one division
 *   per element (a == 0 keeps w, T_i == 0 gives 0);  real: V1_out = min(max(w, -r_i), r_i)
 *   -- the projection onto |v_i| <= r_i, which is the prox of sigma h^* for every sigma;
 *   sums [C][3] = per chain sum |V1_out - V|^2, sum |V1_out|^2 and sum T_i |W_i| (the prior sum of the point W analyses).
 *   scratch: caller-owned, 3 * PXM_FISTA_SLICES_MAX * C doubles.
 * The sums are added in a fixed order that depends on n (m) only: a chain's sums do not depend on its batch; with n == 0
 * (m == 0) they are written as zeros.  An output must not overlap an input or the other output (only equal base pointers
 * are detected and refused).  No atomics and no host read: a HIP graph replays both. */
int pxm_pd_primal_step(const void* X, const void* G, const void* U, double tau, void* X1_out, void* Xbar_out,
                       double* sums, double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream);
int pxm_pd_dual_step(const void* V, const void* W, const double* T, double T_scalar, double sigma, double rscale,
                     void* V1_out, double* sums, double* scratch, int64_t m, int C, int dtype, pxm_stream_t stream);
/* Total variation on the MW grid.  Images are spin-0 MW maps [C][L n], n = 2L - 1, float64 or
 * complex128; coefficients are plane-major per chain, [C][2][L n].  ab: float64 [2][L] on the device, the ring coefficients
 * a_t = q_t / D, b_t = q_t / (D sin theta_t) for t < L - 1 and a_{L-1} = b_{L-1} = 0, with q_t the ring weights of
 * pxm_mw_ring_weights, D = 2 pi / n and theta_t = pi (2t + 1) / n (the quadrature weight is folded into the operator).
 *   (A x)[0][t][p] = a_t (x[t+1][p] - x[t][p])                 (A x)[1][t][p] = b_t (x[t][(p+1) mod n] - x[t][p])
 *   (A^H v)[t][p]  = a_{t-1} v0[t-1][p] - a_t v0[t][p] + b_t (v1[t][(p-1) mod n] - v1[t][p]),   a_{-1} = 0
 * Per real component A rounds the difference and the product; A^H is fma(a_{t-1}, v0[t-1], fma(-a_t, v0[t], s)) with
 * s = b_t (v1[t][p-1] - v1[t][p]), difference and product rounded.  A row that does not exist is not read.
 * pxm_tv_grad: out = A x.   pxm_tv_grad_adjoint: out = A^H v.
 * pxm_tv_value: out[c] = sum_i T_i sqrt(|(A x)[0]_i|^2 + |(A x)[1]_i|^2) (squares and sums rounded one by one; T [L n]
 *   shared by chains, or T_scalar), formed from the image with no coefficient array.  scratch: PXM_FISTA_SLICES_MAX * C.
 * pxm_pd_dual_step_pairs: pxm_pd_dual_step on V, W, V1_out [C][2][m] with the projection onto the pair norm:
 *   w = fma(sigma, W, V) per component;  r_i = T_i rscale;  a = sqrt(sum of the squares of the pair's 2 (real) or 4 (complex)
 *   components);  V1_out = a > r_i ? w (r_i / a) : w on both planes (a == r_i and a == 0 keep w, T_i == 0 gives 0, r_i = inf
 *   never binds);  T is [m] or T_scalar;  sums [C][3] = sum |V1_out - V|^2, sum |V1_out|^2 (both planes), sum_i T_i ||W_i||.
 *   m <= 2^30.  scratch: 3 * PXM_FISTA_SLICES_MAX * C doubles.
 * pxm_tv_primal_step: pxm_pd_primal_step with U = A^H V formed in the kernel (same arithmetic, same sums [C][2]).  G may be
 *   NULL (zero) and Xbar_out may be NULL (not written): with both and tau = 1 it is X - A^H V.
 * pxm_tv_dual_step: pxm_pd_dual_step_pairs with W = A Xbar formed in the kernel, m = L n.
 * The fused steps equal the composed ones bit for bit, sums included.  2 <= L <= 16384, C <= 65535, positive finite steps; an
 * output must not overlap an input or the other output (only equal base pointers are detected and refused).  The sums are
 * added in a fixed order that depends on L (m) only.  No atomics and no host read: a HIP graph replays all of them. */
int pxm_tv_grad(const void* x, const double* ab, void* out, int L, int C, int dtype, pxm_stream_t stream);
int pxm_tv_grad_adjoint(const void* v, const double* ab, void* out, int L, int C, int dtype, pxm_stream_t stream);
int pxm_tv_value(const void* x, const double* ab, const double* T, double T_scalar, double* out, double* scratch, int L,
                 int C, int dtype, pxm_stream_t stream);
int pxm_pd_dual_step_pairs(const void* V, const void* W, const double* T, double T_scalar, double sigma, double rscale,
                           void* V1_out, double* sums, double* scratch, int64_t m, int C, int dtype, pxm_stream_t stream);
int pxm_tv_primal_step(const void* X, const void* G, const void* V, const double* ab, double tau, void* X1_out,
                       void* Xbar_out, double* sums, double* scratch, int L, int C, int dtype, pxm_stream_t stream);
int pxm_tv_dual_step(const void* V, const void* Xbar, const double* ab, const double* T, double T_scalar, double sigma,
                     double rscale, void* V1_out, double* sums, double* scratch, int L, int C, int dtype,
                     pxm_stream_t stream);
/* The Gaussian posterior: preconditioned conjugate gradients on H x = b per chain, H = D + A Hermitian
 * positive definite, D the prior precision ([n] shared by chains, or D_scalar) and A the linear part of
 * x -> calc_gradg(forward(x)).  The single-reduction recurrences of Chronopoulos & Gear (1989): one iteration is the
 * operator pair q = calc_gradg(forward(U)) and the two entry points below.  Every state array is [C][n], float64 or
 * complex128; every per-chain scalar is real.
 * coef [C][PXM_CG_COEF] float64 on the device, a chain's row: alpha, beta, gamma_old, alpha_old, rho = sum |r|^2 of the last
 *   pxm_cg_apply, ||b||^2 (set by the caller), flags (0, PXM_CG_FROZEN, or PXM_CG_FROZEN | PXM_CG_BREAKDOWN, as a double) and
 *   the iterations taken (as a double).  A solve starts from a row that is zero but for ||b||^2.
 * pxm_cg_apply, with Q = q, B0 = -calc_gradg(forward(0)) ([n] shared by chains; NULL: zero) and R the residual:
 *   W_out = fma(D_i, U, Q + B0) per component (the sum rounded first);
 *   per chain gamma = sum Re conj(R) U, delta = sum Re conj(U) W_out, rho = sum |R|^2: plain products and sums without
 *   contraction, added in a fixed order that depends on n only (a chain's sums do not depend on its batch);
 *   then, per chain, on the device: flags != 0 -> alpha = beta = 0, the rest of the row as it was (the sums are not formed);
 *   rho <= tol^2 ||b||^2 -> alpha = beta = 0, flags = PXM_CG_FROZEN;
 *   else beta = gamma / gamma_old (0 when iterations == 0), denom = delta - beta gamma / alpha_old (delta when iterations
 *   == 0); denom not > 0, or gamma or delta not finite -> alpha = beta = 0, flags = PXM_CG_FROZEN | PXM_CG_BREAKDOWN;
 *   else alpha = gamma / denom, gamma_old = gamma, alpha_old = alpha, iterations += 1.
 *   With n == 0 the sums are zero, so every chain freezes.  W_out of a frozen chain is not written.
 *   scratch: caller-owned, 3 * PXM_FISTA_SLICES_MAX * C doubles.
 * pxm_cg_update, per component and in place but for X (Minv [n] shared by chains, or Minv_scalar):
 *   P = fma(beta, P, U);  S = fma(beta, S, W);  X_dst = fma(alpha, P, X_src);  R = fma(-alpha, S, R);  U = Minv_i R;
 *   a chain with flags != 0: X_dst = X_src, and none of its other arrays is read or written.
 *   The eight arrays must all be different (only equal base pointers are detected and refused).
 * pxm_gauss_prox: out = X / (1 + T p_i) per component, p [n] shared by chains or precision_scalar; the sum 1 + T p_i is
 *   rounded (product, then sum), one division per component: the prox of T 1/2 sum_i p_i |x_i|^2.  out must not alias X.
 * pxm_cg_rhs: out = B_i + g_scale G + (z_scale S_i) Z, per component acc = B_i; acc = fma(g_scale, G, acc); acc =
 *   fma(z_scale S_i (rounded), Z, acc).  B [n] shared by chains, G and Z [C][n], S [n] or S_scalar; B, G, Z may each be NULL
 *   (no term).  out must not alias an input.
 * D_stride, Minv_stride, S_stride: the chain stride of the vector in doubles -- 0: one [n] vector shared by the chains; n: one
 *   row per chain ([C][n], the arrays pxm_group_variance_draw writes); chain c reads element c * stride + i.  Any other
 *   value is refused.
 * No atomics and no host read: a HIP graph replays all of them. */
#define PXM_CG_COEF 8
#define PXM_CG_FROZEN 1
#define PXM_CG_BREAKDOWN 2
int pxm_cg_apply(const void* U, const void* Q, const void* B0, const double* D, double D_scalar, int64_t D_stride, const void* R,
                 void* W_out, double* coef, double tol, double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream);
int pxm_cg_update(void* U, const void* W, void* P, void* S, const void* X_src, void* X_dst, void* R, const double* Minv,
                  double Minv_scalar, int64_t Minv_stride, const double* coef, int64_t n, int C, int dtype, pxm_stream_t stream);
int pxm_gauss_prox(const void* X, const double* precision, double precision_scalar, double T, void* out, int64_t n, int C,
                   int dtype, pxm_stream_t stream);
int pxm_cg_rhs(const void* B, const void* G, double g_scale, const void* Z, const double* S, double S_scalar, int64_t S_stride,
               double z_scale, void* out, int64_t n, int C, int dtype, pxm_stream_t stream);
/* The conditional draw of the prior precisions given the field, the second half of a Gibbs sweep on the Gaussian posterior
 * (Wandelt, Larson & Lakshminarayanan 2004).  The state X [C][n] (float64 or complex128) is cut into K
 * contiguous groups by the device offsets bounds [K + 1], 0 = b_0 < ... < b_K = n; group k has n_k = b_{k+1} - b_k elements.
 *   nu_k = dof n_k + two_q - 2, dof = 2 for complex128 and 1 for float64, two_q = 2 q of the hyper-prior p(v) ~ v^-q;
 *   sigma_k = sum_{i in k} |X_i|^2 (products and sums rounded, no contraction);
 *   chi2_k = sum_{t < nu_k} z_t^2, z_t component t & 1 of the fp64 complex-stream Philox pair keyed (seed, chain0 + c) at
 *     counter (b_k + k + (t >> 1), iter): element b_k + k + (t >> 1) of pxm_randn(n + K + 1, dtype 1 | PXM_NOISE_F64);
 *   Dg[c][k] = min(max(chi2_k / sigma_k, d_lo), d_hi), and d_hi when sigma_k is not > 0.
 *   A group with fixed[k] != 0 or nu_k < 1 keeps Dg[c][k]; nothing of it is summed or drawn.
 * Both sums are added in a fixed order that depends on n_k only.  The groups are cut into slices of PXM_GIBBS_SLICE elements,
 * one workgroup each: slice_tab [nslices][2] int64 on the device holds (k, j) of every slice -- elements b_k + j S ... of
 * group k, S = PXM_GIBBS_SLICE -- ordered by k, then j, and group_slice0 [K + 1] the index of every group's first slice
 * (group_slice0[K] = nslices = sum_k ceil(n_k / S)).  A slice whose (k, j) lies outside the groups is skipped.
 * Then, for every element i of group k:  D[c][i] = Dg[c][k], sqrtD[c][i] = sqrt(Dg[c][k]), Minv[c][i] = 1 / (Dg[c][k] + h_c)
 * (h [C] on the device, or h_scalar; the sum rounded, then one division): the arrays pxm_cg_apply, pxm_cg_rhs and
 * pxm_cg_update read with chain stride n.  expand_only != 0: only this last launch (Dg as given).
 *   sums [C][K][2] (or NULL): receives (sigma_k, chi2_k) of every sampled group.
 *   trace [n_trace][C][K] (or NULL with n_trace 0): row trace_row, when there is one, receives Dg after the draw.
 *   scratch: caller-owned, 2 * nslices * C doubles.
 * d_lo, d_hi finite, 0 < d_lo <= d_hi.  Three launches at most, no atomics and no host read: a HIP graph replays the call.
 * The outputs must not overlap an input or each other (only equal base pointers are detected and refused). */
#define PXM_GIBBS_SLICE 1024
int pxm_group_variance_draw(const void* X, const int64_t* bounds, int K, const int64_t* slice_tab, const int64_t* group_slice0,
                            int64_t nslices, const int32_t* fixed, int two_q, const double* h, double h_scalar, double d_lo,
                            double d_hi, uint64_t seed, uint64_t chain0, uint64_t iter, double* Dg, double* sums, double* trace,
                            int64_t n_trace, int64_t trace_row, double* D, double* sqrtD, double* Minv, double* scratch,
                            int64_t n, int C, int dtype, int expand_only, pxm_stream_t stream);
/* The conditional draw of the prior precisions given the field for the L1 prior (1 / lmda) sum_i T_i |X_i|, the second half of
 * a Gibbs sweep on the sparse posterior (Park & Casella 2008): the Laplace prior as a Gaussian scale
 * mixture, under which every precision is an inverse-Gaussian variate given the field.  One pass over X [C][n] (float64 or
 * complex128); per element i of chain c, with plain products and sums and no contraction:
 *   t = tscale T_i (T [n] on the device, shared by the chains, or T_scalar; every t must be positive -- only tscale and
 *     T_scalar can be checked here -- and a t that is not leaves an unspecified value inside the clamp);
 *   |x| = sqrt(re^2 + im^2) for complex128, fabs for float64;
 *   z = component 0 of the fp64 complex-stream Philox pair keyed (seed, chain0 + c) at counter (i, iter): the real part of
 *     element i of pxm_randn(n, dtype 1 | PXM_NOISE_F64) at that iteration, for either dtype;
 *   u = (a + 1/2) 2^-52, a the first 52 bits of the Philox block at counter (i, iter + 1) (words 1 and 0 as one 64-bit number,
 *     shifted right by 12): exact, in (0, 1).  The call owns the iterations iter and iter + 1;
 *   rt = 1 / t;  a = |x| rt;  zt = z rt;  g = 0.5 (zt zt);  D1 = 1 / ((a + g) + sqrt(g (g + 2 a)));
 *   raw = D1 unless u (1 + a D1) > 1, then 1 / (a (a D1))   (Michael, Schucany & Haas 1976: IG(mean t / |x|, shape t^2));
 *   D[c][i] = min(max(raw, d_lo), d_hi) (NaN or overflow: d_hi from the first branch), sqrtD[c][i] = sqrt(D[c][i]),
 *   Minv[c][i] = 1 / (D[c][i] + h_c) (h [C] on the device, or h_scalar): the arrays pxm_cg_apply, pxm_cg_rhs and pxm_cg_update
 *   read with chain stride n.
 *   sums [C][2] (or NULL): receives sum_i t |x_i| -- the prior term of the objective at X -- and the number of elements whose
 *     raw value the clamp changed, as a double; added in a fixed order that depends on n only.
 *   scratch: caller-owned, 2 * PXM_FISTA_SLICES_MAX * C doubles; NULL without sums.
 * d_lo, d_hi finite, 0 < d_lo <= d_hi.  One launch, two with sums; no atomics and no host read: a HIP graph replays the call.
 * The outputs must not overlap an input or each other (only equal base pointers are detected and refused). */
int pxm_lasso_precision_draw(const void* X, const double* T, double T_scalar, double tscale, const double* h, double h_scalar,
                             double d_lo, double d_hi, uint64_t seed, uint64_t chain0, uint64_t iter, double* D, double* sqrtD,
                             double* Minv, double* sums, double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream);
/* One SAPG iteration (Vidal, De Bortoli, Pereyra & Durmus 2020): a MYULA step of every chain on the
 * posterior whose prior is scaled by the chain's theta, then the move of theta towards the marginal maximum-likelihood
 * value of the regularisation strength.  Every state array [C][n]; theta, eta [C] float64 on the device, updated in place.
 *   thr_i = theta[c] T_i (rounded; T [n] shared by chains, or T_scalar);
 *   X_out = (1 - delta/lmda) X + (delta/lmda) soft(X, thr) - delta gradg + sqrt(2 delta) w, the arithmetic and the noise of
 *   pxm_myula_step (noise given, or the Philox stream keyed (seed, chain0 + c, element, iter + *iter_dev); noise_complex =
 *   (0 | 1) | PXM_NOISE_F64; iter_dev: caller-owned device iteration counter or NULL);
 *   G_c = (1 / lmda) sum_i T_i |X_out_i|, added in a fixed order that depends on n only (a chain's sum does not depend on its
 *   batch); pool != 0: every chain takes the chain-order mean of the G_c;
 *   eta[c] = min(max(eta[c] + rho (d - theta[c] G_c), eta_min), eta_max), rho = rho_table[min(iter + *iter_dev, n_rho - 1)]
 *   read when the kernel runs;  theta[c] = exp(eta[c]);
 *   trace [n_trace][C][3] (or NULL with n_trace 0): row iter + *iter_dev, when there is one, receives (theta, eta, G_c).
 * d: the dimension of the state (the degree of the normaliser theta^-d of exp(-theta G)).  With n == 0 only the update runs,
 * with G = 0.  scratch: caller-owned, (PXM_SAPG_SLICES_MAX + 1) * C doubles.  X_out, theta, eta, trace and scratch must not
 * overlap an input or each other (only equal base pointers are detected and refused). */
#define PXM_SAPG_SLICES_MAX 256
int pxm_sapg_step(const void* X, const void* gradg, const double* T, double T_scalar, double delta, double lmda,
                  const void* noise, int noise_complex, uint64_t seed, uint64_t chain0, uint64_t iter,
                  const uint64_t* iter_dev, double* theta, double* eta, double d, const double* rho_table, int64_t n_rho,
                  double eta_min, double eta_max, int pool, double* trace, int64_t n_trace, void* X_out, double* scratch,
                  int64_t n, int C, int dtype, pxm_stream_t stream);
/* pxm_sapg_step with one theta per chain and per group of the state ("One theta per group"): the prior
 * is sum_k theta_k G_k(X), G_k(X) = (1 / lmda) sum_{b_k <= i < b_k+1} T_i |X_i| on K contiguous, non-empty blocks -- the scales
 * of a wavelet prior.  bounds: HOST array of the K + 1 offsets 0 = b_0 < b_1 < ... < b_K = n, 1 <= K <= PXM_SAPG_GROUPS_MAX,
 * read during the call only (the kernels receive them by value).  theta, eta [C][K] float64 on the device, updated in place.
 *   thr_i = theta[c][k(i)] T_i (rounded), k(i) the group of element i;  X_out as pxm_sapg_step's, the noise keyed by the
 *   element's index i in the whole state: X_out is pxm_myula_step on T'_i = theta[c][k(i)] T_i;
 *   G[c][k] = (1 / lmda) sum over group k of T_i |X_out_i|, added in the order pxm_sapg_step adds a state of b_k+1 - b_k
 *   elements: it depends on the group's length only, not on the batch or the other groups;  pool != 0: every chain takes the
 *   chain-order mean of the G[c][k], group by group;
 *   eta[c][k] = min(max(eta[c][k] + rho[j][k] (d[k] - theta[c][k] G[c][k]), eta_min), eta_max), j = min(iter + *iter_dev,
 *   n_rho - 1);  theta[c][k] = exp(eta[c][k]);
 *   trace [n_trace][C][K][3] (or NULL with n_trace 0): row iter + *iter_dev, when there is one, receives (theta, eta, G).
 * d [K] (the dimensions of the groups) and rho_table [n_rho][K]: float64 on the device.  n == 0 is refused: a group cannot be
 * empty.  With K == 1 the results are pxm_sapg_step's with d = d[0], bit for bit.
 * scratch: caller-owned, (PXM_SAPG_SLICES_MAX + 1) * K * C doubles.  Aliasing rules as for pxm_sapg_step; no allocation, copy
 * or host read per call: a HIP graph replays it. */
#define PXM_SAPG_GROUPS_MAX 32
int pxm_sapg_step_groups(const void* X, const void* gradg, const double* T, double T_scalar, double delta, double lmda,
                         const void* noise, int noise_complex, uint64_t seed, uint64_t chain0, uint64_t iter,
                         const uint64_t* iter_dev, double* theta, double* eta, const int64_t* bounds, int K, const double* d,
                         const double* rho_table, int64_t n_rho, double eta_min, double eta_max, int pool, double* trace,
                         int64_t n_trace, void* X_out, double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream);
/* Local credible intervals from the MAP point (Cai, Pereyra & McEwen 2018).  Slot c of a batch is one
 * region of the image; along the surrogate X(xi) = a_c + xi b_c (xi real) the objective of pxm_fista_step's posterior is
 *   F_c(xi) = q0 + q1 xi + q2 xi^2 + (1 / lmda) sum_k T_k |a_ck + xi b_ck|,
 * convex in xi, and the interval of the slot is {xi : F_c(xi) <= gamma_c}.  a, b [C][n] (f64 or c128), T [n] shared by the
 * slots or T_scalar.  Every sum is added in a fixed order that depends on the vector length only: a slot's numbers do not
 * depend on its batch.  scratch: caller-owned, pxm_lci_scratch_doubles(n, C) doubles, n the longer of the vectors summed.
 *
 * pxm_lci_data_terms: quad[c] = (q0, q1, q2) = (1/2 sum w |r|^2, sum w Re(conj(r) s), 1/2 sum w |s|^2) with r = preds_a[c] -
 *   data and s = preds_b[c] (the predictions of a_c and b_c, [C][ndata]; data [ndata] of the same dtype and w [ndata], real,
 *   are shared by the slots).
 * pxm_lci_eval: P[c][j] = sum_k T_k |a_ck + xi[c][j] b_ck| for the PXM_LCI_POINTS values xi[c][.], in one pass over a, b, T,
 *   the modulus formed from (a_re + xi b_re, a_im + xi b_im); P[c][32] = sum T|a_c|, P[c][33] = sum T|b_c|  (P [C][34]).
 * pxm_lci_search: the whole search, enqueued on the stream: an initialisation kernel, then `rounds` times (pxm_lci_eval's
 *   two kernels, a refinement kernel).  `rounds` (1 ... PXM_LCI_ROUNDS_MAX) is fixed here, on the host; no device loop has
 *   a trip count that depends on data, and nothing waits.  gamma [C] on the device.  Outer bracket: the roots of the
 *   quadratic = gamma (q2 > 0; F >= the quadratic), or |xi| <= (lmda (gamma - q0) + S_a) / (S_b - lmda |q1|) (q2 == 0 and
 *   a positive denominator; found in the first round; q1 = 0 whenever s = 0).  While no point has F <= gamma the 32 points span the bracket and the bracket becomes the
 *   smallest point with its two neighbours; from then on each end has a bracket of its own, cut by 16 interior points per
 *   round.  The brackets shrink by at least 2/31 per round (1/17 once split).
 *   out[c] = (lower, upper, width of the lower end's bracket, of the upper end's, smallest F seen, its xi, outer bracket
 *   lo, hi): lower and upper are the inner points of the final brackets, where F <= gamma was evaluated.  status[c]: 0, or
 *   PXM_LCI_EMPTY (no point with F <= gamma was found: negative discriminant -- NaN ends --, or still none after the last
 *   round -- lower, upper are then the bracket of the minimiser), PXM_LCI_UNCONSTRAINED (b = 0 and s = 0 with F <= gamma, or q2 == 0
 *   with |q1| >= S_b / lmda, F not coercive: -inf, +inf), PXM_LCI_NONFINITE (a non-finite input, whatever else holds: NaN). */
#define PXM_LCI_POINTS 32
#define PXM_LCI_ROUNDS_MAX 64
#define PXM_LCI_EMPTY 1
#define PXM_LCI_UNCONSTRAINED 2
#define PXM_LCI_NONFINITE 4
int64_t pxm_lci_scratch_doubles(int64_t n, int C);
int pxm_lci_data_terms(const void* preds_a, const void* preds_b, const void* data, const double* w, double* quad,
                       double* scratch, int64_t ndata, int C, int dtype, pxm_stream_t stream);
int pxm_lci_eval(const void* a, const void* b, const double* T, double T_scalar, const double* xi, double* P,
                 double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream);
int pxm_lci_search(const void* a, const void* b, const double* T, double T_scalar, const double* quad, double lmda,
                   const double* gamma, int rounds, double* out, int* status, double* scratch, int64_t n, int C, int dtype,
                   pxm_stream_t stream);
/* One iteration of segment inpainting for the hypothesis test of image structure (Cai, Pereyra & McEwen 2018 II section 4.2;
 * DESIGN.md section 14c).  Slot c of a batch is one region of an integer label image:
 *   x_next[c][k] = done[c] ? x_prev[c][k] : (labels[k] == region[c] && labels[k] >= 0 ? y[c][k] : x_map[k])
 * (a select: bit-exact), y = Psi soft_tau(A x_prev) formed by the caller.  y, x_prev, x_next [C][npix] (f64 or c128), x_map
 * [npix] of the same dtype and labels int32 [npix] shared by the slots, region int32 [C]; done, iters int32 [C] and stat
 * float64 [C][2] are read and updated.  For a slot that is not done: d2 = sum |x_next - x_prev|^2 and n2 = sum |x_next|^2
 * over the whole image, added in a fixed order that depends on npix only (a slot's numbers do not depend on its batch);
 * then iters[c] += 1, stat[c] = (d2, n2), done[c] = (d2 <= tol2 * n2): one multiply and one compare, tol2 = tol^2 formed by
 * the caller; a NaN compares false and never freezes a slot.  Of a slot that is done only x_next[c] is written.  Two
 * kernels, no trip count that depends on data, nothing waits: capturable.  x_next must not overlap x_prev or y.  scratch:
 * caller-owned, pxm_inpaint_scratch_doubles(npix, C) doubles. */
int64_t pxm_inpaint_scratch_doubles(int64_t npix, int C);
int pxm_inpaint_step(const void* y, const void* x_prev, const void* x_map, const int* labels, const int* region, double tol2,
                     void* x_next, int* done, int* iters, double* stat, double* scratch, int64_t npix, int C, int dtype,
                     pxm_stream_t stream);
/* N(0,1) draws of the Philox4x32-10 stream keyed (seed, chain0+c, iter): out [C][n] (f64 or c128) */
int pxm_randn(void* out, int64_t n, int C, int dtype, uint64_t seed, uint64_t chain0, uint64_t iter,
              pxm_stream_t stream);
/* The Box-Muller step of that stream on GIVEN uniforms u1, u2 in (0, 1] (device arrays [n]): z0 = r cos(2 pi u2),
 * z1 = r sin(2 pi u2), r = sqrt(-2 ln u1); f64 != 0 selects the double-precision evaluation.  Test aid: the edge cases
 * (u1 rounding to 1, the smallest u1, quadrant boundaries of u2) have probability ~2^-53 under Philox. */
int pxm_box_muller(const double* u1, const double* u2, double* z0, double* z1, int64_t n, int f64, pxm_stream_t stream);
/* The reductions below are deterministic two-stage sums; `scratch` is a caller-owned device buffer of
 * pxm_reduce_scratch_doubles(C) doubles (no library-owned buffer is shared between calls or streams). */
int64_t pxm_reduce_scratch_doubles(int C);
/* L1.prior / S2_Wavelets_L1.prior (pxmcmc/prior.py:28-35,83-84): out[c] = sum_i |w_i X_ci| */
int pxm_reduce_l1(const void* X, const double* w, double* out, double* scratch, int64_t n, int C, int dtype,
                  pxm_stream_t stream);
/* logpi's L2 = vdot(d, invcov d), d = data - preds (pxmcmc/mcmc.py:78-79): out[c] = (re, im) */
int pxm_reduce_l2(const void* preds, const void* data, const void* invcov, int invcov_complex,
                  double* out, double* scratch, int64_t n, int C, int dtype, pxm_stream_t stream);
/* np.vdot(a, b) per chain: out[c] = sum conj(a) b as (re, im) -- logpi's L2 = vdot(d, invcov @ d) when invcov is a
 * full (sparse) matrix applied with pxm_csr_matvec (pxmcmc/forward.py:75-78, mcmc.py:78-79) */
int pxm_reduce_vdot(const void* a, const void* b, double* out, double* scratch, int64_t n, int C, int dtype,
                    pxm_stream_t stream);
/* uncertainty.credible_interval_range (pxmcmc/uncertainty.py:7-16) of a chain resident on the device: out[j] = Q(1 - alpha/2) -
 * Q(alpha/2) over the nsamples rows of column j of chain[nsamples][ld >= nparams] (float64), numpy.quantile's default "linear"
 * method reproduced (exact order statistics by radix select + numpy's lerp) */
int pxm_quantile_range(const double* chain, int64_t nsamples, int64_t nparams, int64_t ld, double alpha, double* out,
                       pxm_stream_t stream);
/* PxMALA.calc_logtransition, literal (pxmcmc/mcmc.py:281-289): out[c] = (re, im) */
int pxm_logtransition(const void* X1, const void* X2, const void* proxf, const void* gradg,
                      const double* delta_dev, double delta, double lmda, double* out, double* scratch,
                      int64_t n, int C, int dtype, pxm_stream_t stream);
/* One PxMALA iteration with every per-iteration quantity on the device (pxmcmc/mcmc.py:230-260).
 *   pxm_pxmala_propose : X' = chain_step(X, proxf, gradg) with per-chain delta_dev [C]; proxf' = soft(X', T);
 *                        logtrans_out[c] = calc_logtransition(X, X', proxf, gradg) as (re, im);
 *                        prior_out[c] = sum |w X'| (w = prior_weights [n] or NULL) -- ONE pass over the state.
 *                        iter_dev: optional caller-owned device counter added to iter (HIP-graph replay).
 *                        scratch: 4 * pxm_reduce_scratch_doubles(C) doubles.  logtrans_out == prior_out == NULL: the
 *                        totals are DEFERRED -- the per-slice sums stay in `scratch` for pxm_pxmala_finish.
 *                        proxf == proxf_prop == NULL: the prox arrays are neither read nor written -- proxf = soft(X, T)
 *                        (the stock L1 prox, pxmcmc/prior.py:49-50) is formed in the kernel, and pxm_pxmala_finish forms
 *                        soft(X', T) the same way: 40 % fewer bytes in the pass and one array less in the conditional copy.
 *   pxm_pxmala_accept  : logalpha = Re(logtrans_pc + logpi' - logtrans_cp - logpi), logpi' = -mu prior' - L2';
 *                        accept iff log(u) < logalpha (u injected [C] or the Philox uniform of (seed, chain, iteration));
 *                        accepted chains take (logpi', L2', prior') into their state scalars (logpi_c, L2_c as (re, im),
 *                        prior_c); delta_dev adapted when tune (:277-279) with the iteration number iter + *iter_dev;
 *                        acc_trace / delta_trace: optional [chunk][C] ring buffers written at row iteration % chunk.
 *   pxm_pxmala_finish  : everything between the proposal's gradient and the conditional copy in TWO launches instead of
 *                        seven: (i) ONE grid with the slices of the reverse transition sum of
 *                        calc_logtransition(X', X, proxf', gradg') [n, dtype; proxf_prop == NULL: proxf' = soft(X', T)
 *                        with T [n] or T_scalar] and of L2' = vdot(d, invcov d),
 *                        d = data - preds' [n_data, data_dtype; invcov as for pxm_reduce_l2]; (ii) ONE workgroup that
 *                        totals those and the deferred sums of pxm_pxmala_propose (`propose_scratch`: that call's scratch) in
 *                        the order of the separate reductions, stores logtrans_pc / logtrans_cp / L2' as (re, im) [C] and
 *                        prior' [C] for observers, and runs the test of pxm_pxmala_accept.  bump_counter: optional
 *                        device counter advanced by one AFTER every chain has read iter_dev (replaces pxm_counter_add
 *                        in a captured iteration).  scratch: 2 * pxm_reduce_scratch_doubles(C) doubles.
 *   pxm_select_copy_many : up to 4 arrays per call, dst_a[c] = src_a[c] for accepted chains.
 *   pxm_counter_add    : *counter += inc on the stream (after every reader of the iteration). */
int pxm_pxmala_propose(const void* X, const void* proxf, const void* gradg, const double* T, double T_scalar,
                       const double* prior_weights, const double* delta_dev, double lmda, const void* noise,
                       int noise_complex, uint64_t seed, uint64_t chain0, uint64_t iter, const uint64_t* iter_dev,
                       void* X_prop, void* proxf_prop, double* logtrans_out, double* prior_out, double* scratch,
                       int64_t n, int C, int dtype, pxm_stream_t stream);
int pxm_pxmala_accept(const double* logtrans_pc, const double* logtrans_cp, const double* prior_p, const double* L2_p,
                      double mu, double* logpi_c, double* L2_c, double* prior_c, const double* u, uint64_t seed,
                      uint64_t chain0, uint64_t iter, const uint64_t* iter_dev, int32_t* accept_out, double* delta_dev,
                      int tune, double lmda, int32_t* acc_trace, double* delta_trace, int chunk, int C,
                      pxm_stream_t stream);
int pxm_pxmala_finish(const void* X_prop, const void* X_curr, const void* proxf_prop, const double* T, double T_scalar,
                      const void* gradg_prop, int64_t n, int dtype, const void* preds_prop, const void* data, const void* invcov, int invcov_complex,
                      int64_t n_data, int data_dtype, const double* propose_scratch, double mu, double lmda, double* logpi_c,
                      double* L2_c, double* prior_c, const double* u, uint64_t seed, uint64_t chain0, uint64_t iter,
                      const uint64_t* iter_dev, int32_t* accept_out, double* delta_dev, int tune, int32_t* acc_trace,
                      double* delta_trace, int chunk, double* logtrans_pc_out, double* logtrans_cp_out, double* prior_p_out,
                      double* L2_p_out, double* scratch, uint64_t* bump_counter, int C, pxm_stream_t stream);
int pxm_select_copy_many(const int32_t* flag, int narrays, const void* const* src, void* const* dst, const int64_t* n,
                         const int* esize, int C, pxm_stream_t stream);
int pxm_counter_add(uint64_t* counter_dev, uint64_t inc, pxm_stream_t stream);

/* ---- streaming posterior summaries --------------------------------------------------------
 * pxm_moments_update replaces the chain-wide np.mean of experiments/earthtopography/plot.py:105-122 (and the same lines
 * of the phasevel / weaklensing plot scripts) and the highest-posterior look-up of plot.py:75-76 (MAP_idx / MAP_X), which
 * need every saved sample in host memory: one Welford step per chain, k = count[c] + 1; d = x - mean; mean += d / k;
 * m2 += d (x - mean_new), in one pass over a [C][m] float64 batch.  x_stride 1: x is [C][m] float64; 2: x is [C][m]
 * complex128 and its REAL parts are accumulated (a complex state accumulated per component is passed as float64
 * [C][2 n]).  count int64 [C]; mean, m2 float64 [C][m]; mask int32 [C] or NULL (every chain): a masked-out chain's
 * count, mean, m2 and best fields are not written.  Best sample (all three NULL: not tracked): logpi float64 with
 * element stride logpi_stride (1, or 2 for the real parts of complex128 [C]); a masked-in chain with
 * logpi[c] > best_logpi[c] copies x to best_x [C][m] (ties keep the first, NaN never wins; start best_logpi at -inf).
 * Two launches on the given stream: the streaming pass, which only reads count and best_logpi, then one workgroup that
 * advances them.  No allocation, no synchronisation: graph-capturable.  x, mean, m2 and best_x must be 16-byte aligned. */
int pxm_moments_update(const double* x, int x_stride, int64_t* count, double* mean, double* m2, const int* mask,
                       const double* logpi, int logpi_stride, double* best_logpi, double* best_x, int64_t m, int C,
                       pxm_stream_t stream);
/* doubles of caller-owned scratch pxm_moments_finalize needs for `stats` */
int64_t pxm_moments_scratch_doubles(int64_t m);
/* pxm_moments_finalize reduces the accumulators over chains, in chain order (deterministic), per element: pooled_mean [m]
 * and pooled_var [m] (unbiased) over every sample of every chain with count > 0 by Chan's pairwise merge -- np.mean
 * (plot.py:122) and the np.std maps of a run whose chains were concatenated -- and the Gelman-Rubin rhat [m] of the chains
 * with count > 0, which the reference does not have.  With n their common count and C' their number:
 * W = mean_c m2_c / (n - 1), B = n / (C' - 1) sum_c (mean_c - mean of means)^2, rhat = sqrt(((n - 1) / n W + B / n) / W).
 * NaN where an output is undefined (no sample; variance of one sample; R-hat with C' < 2, n < 2 or W == 0).  stats [2]
 * (optional; needs rhat and scratch): max rhat over the non-NaN elements (NaN if none) and the number of NaN elements, by
 * a two-stage reduction.  Any output may be NULL.  With rhat requested the counts are read back (the call synchronises
 * the stream) and chains with different counts are an error; the pooled moments alone take any counts. */
int pxm_moments_finalize(const int64_t* count, const double* mean, const double* m2, int64_t m, int C, double* pooled_mean,
                         double* pooled_var, double* rhat, double* stats, double* scratch, pxm_stream_t stream);

/* ---- exact streaming credible intervals -----------------------------------------------------
 * Replace np.quantile(chain, (alpha / 2, 1 - alpha / 2), axis=0) of credible_interval_range (pxmcmc/uncertainty.py:7-16),
 * which needs every saved sample, by the k smallest and the k largest samples per chain and element, kept on the device.
 * With N the number of saves declared before the run and (i, g) = split(q, n) the arithmetic of pxm_quantile_range,
 * k = min(N, max(i_lo(N) + 2, N - i_hi(N))) slots per tail hold the order statistics numpy's linear quantile needs at
 * every sample count n <= N and every alpha' <= alpha.  State, caller-owned: lo, hi float64 [C][k][m] (slot-major; each a
 * binary heap over its slots, ordered by the 64-bit key of pxm_quantile_range, slot 0 the threshold: the largest of lo,
 * the smallest of hi), thr_lo, thr_hi float64 [C][m], copies of the thresholds, and stage float64 [C][B][m], a ring of
 * the last saves: they are merged into the heaps B at a time, which touches each cache line of a tail once per B saves.
 * No initialisation is needed.  pxm_tails_buffer_doubles: doubles of each of lo and hi; pxm_tails_stage_doubles: doubles
 * of stage (-1: bad arguments or overflow). */
int64_t pxm_tails_buffer_doubles(int64_t m, int C, int64_t k);
int64_t pxm_tails_stage_doubles(int64_t m, int C);
/* One save: x as for pxm_moments_update (x_stride 1: float64 [C][m]; 2: the real parts of complex128 [C][m]).  count int64
 * [C] is the number of samples BEFORE this one and is only read: queue the call before the pxm_moments_update of the same
 * sample, which advances it.  count[c] < k: the sample goes to slot count[c] of both heaps.  Later it goes to row
 * (count[c] - k) % B of the ring, and the save that fills the ring merges it: a sample between the two thresholds costs
 * no store, one beyond a threshold replaces it and sifts down.  A masked-out chain (mask int32 [C], NULL: every chain)
 * and a chain with count[c] >= nsamples are not touched.  One launch, no allocation, no synchronisation:
 * graph-capturable.  x, thr_lo and thr_hi must be 16-byte aligned. */
int pxm_tails_update(const double* x, int x_stride, const int64_t* count, double* lo, double* hi, double* thr_lo, double* thr_hi,
                     double* stage, const int* mask, int64_t m, int C, int64_t k, int64_t nsamples, pxm_stream_t stream);
/* Read-out after the run: q_lo, q_hi float64 [C][m], numpy's linear quantiles at alpha / 2 and 1 - alpha / 2 of the
 * count[c] samples of every chain and element, bit for bit (exact order statistics of each tail together with the rows
 * of the ring not merged yet, by radix select, numpy's lerp); NaN for a chain without samples.  Nothing is written to the
 * state.  alpha may be any value whose order statistics lie inside the tails (every alpha up to the one k was sized for).
 * The counts are read back (the call synchronises the stream); an alpha the tails do not cover, or a chain with
 * count[c] > nsamples, is an error. */
int pxm_tails_quantiles(const int64_t* count, const double* lo, const double* hi, const double* stage, int64_t m, int C, int64_t k,
                        int64_t nsamples, double alpha, double* q_lo, double* q_hi, pxm_stream_t stream);

/* ---- streaming effective sample size -------------------------------------------------------
 * The lagged autocovariances of every chain and element at lags 0 ... K - 1 (K even, 2 <= K <= 64), accumulated at the
 * save points, without the chain.  With x_0 ... x_{n-1} the saves of a chain, p = x_0 and y_t = x_t - p, the caller-owned
 * float64 state is acc [C][K][m] (acc_l = sum_{t >= l} y_t y_{t-l}) and tot [C][m] (sum_t y_t), both summed in save order
 * with every product and sum rounded on its own, head [C][K][m], the first K saves as they came (row 0 is the pivot), and
 * ring [C][K - 1 + B][m], save t at row t mod (K - 1 + B), B = pxm_acov_stage_depth().  acc and tot cover the complete
 * blocks of B saves; the saves after them wait in the ring.  No initialisation is needed: the first block starts from zero.
 * pxm_acov_state_doubles: doubles of each of acc and head; pxm_acov_ring_doubles: doubles of ring; pxm_acov_scratch_doubles:
 * doubles of the scratch pxm_acov_ess needs for `stats` (-1: bad arguments or overflow). */
int pxm_acov_stage_depth(void);
int64_t pxm_acov_state_doubles(int64_t m, int C, int K);
int64_t pxm_acov_ring_doubles(int64_t m, int C, int K);
int64_t pxm_acov_scratch_doubles(int64_t m);
/* One save: x as for pxm_moments_update (x_stride 1: float64 [C][m]; 2: the real parts of complex128 [C][m]).  count int64
 * [C] is the number of samples BEFORE this one and is only read: queue the call before the pxm_moments_update of the same
 * sample, which advances it.  The sample is copied to row count[c] mod (K - 1 + B) of the ring (and to row count[c] of head
 * while count[c] < K); the save with count[c] mod B == B - 1 also folds its block into acc and tot.  Every chain has its own
 * phase.  A masked-out chain (mask int32 [C], NULL: every chain) is not touched.  One launch, no allocation, no
 * synchronisation: graph-capturable. */
int pxm_acov_update(const double* x, int x_stride, const int64_t* count, double* acc, double* tot, double* head, double* ring,
                    const int* mask, int64_t m, int C, int K, pxm_stream_t stream);
/* Read-out; writes nothing to the state and folds the count[c] mod B saves that wait in the ring on the fly, in the order
 * a merge would.  Per chain, d = tot / n, head_l (tail_l) the sum of the first (last) l of the y_t:
 * gamma_l = (acc_l - d ((tot - head_l) + (tot - tail_l)) + (n - l) d^2) / n, rho_l = gamma_l / gamma_0, Geyer's initial
 * monotone sequence over P_k = rho_2k + rho_2k+1 for 2 k + 1 < min(K, n) (stop at the first P_k that is not positive,
 * else P_k <- min(P_k, P_k-1)), tau = -1 + 2 sum P_k, ess [C][m] = min(n / tau, n log10 n) (the cap where tau <= 0) and
 * ess_lag int32 [C][m], the even lag of the stop, 2 floor(min(K, n) / 2) when the sequence never stopped (the estimate is
 * then truncated: an upper bound).  NaN and -1 for n < 4 or a gamma_0 that is not positive and finite.  ess_pooled [m] and
 * mcse [m] (optional): over the C' chains with samples, W = mean_c n / (n - 1) gamma_0,c, var+ = (n - 1) / n W + the
 * variance of the chain means p_c + d_c, rho_l = 1 - (W - mean_c n / (n - 1) gamma_l,c) / var+, the same sum,
 * ess_pooled = min(C' n / tau, C' n log10(C' n)), mcse = sqrt(var+ / ess_pooled); they make the call read the counts back
 * (it synchronises the stream), and chains with different counts are then an error.  stats [3] (optional, needs scratch):
 * the minimum of ess over its non-NaN values (NaN if none), its NaN count and its truncated count. */
int pxm_acov_ess(const int64_t* count, const double* acc, const double* tot, const double* head, const double* ring, int64_t m, int C,
                 int K, double* ess, int* ess_lag, double* ess_pooled, double* mcse, double* stats, double* scratch,
                 pxm_stream_t stream);

/* ---- weak-lensing measurement helpers (pxmcmc/measurements.py:151-171, 242-304) --------- */
/* out = flm .* kernel with entries [0,4) zeroed: harmonic_mapping (:162-171). kernel: [L*L] */
int pxm_wl_harmonic_mapping(const void* flm, const double* kernel, void* out, int64_t n, int C,
                            pxm_stream_t stream);
/* gather unmasked pixels and weight: out[c][k] = f[c][idx[k]] * w[k]   (mask_forward + cov_weight) */
int pxm_wl_mask_gather(const void* f, const int64_t* idx, const double* w, void* out, int64_t npix,
                       int64_t ndata, int C, pxm_stream_t stream);
/* weight and scatter into zeros: f[c][idx[k]] = g[c][k] * w[k]          (cov_weight + mask_adjoint) */
int pxm_wl_mask_scatter(const void* g, const int64_t* idx, const double* w, void* f, int64_t npix,
                        int64_t ndata, int C, pxm_stream_t stream);

/* ---- sparse path-integral measurement (pxmcmc/measurements.py:59-83) ---------------------- */
/* y[c][row] = sum_k vals[k] x[c][indices[k]], k in [indptr[row], indptr[row+1]): PathIntegral.forward with
 * the CSR of path_matrix, PathIntegral.adjoint with the CSR of path_matrix.getH().  vals: float64, or
 * complex128 iff vals_complex; x: [C][ncols], y: [C][nrows], float64 (dtype 0) or complex128 (dtype 1).
 * scratch: NULL, or a caller-owned buffer of ncols * C elements of x's type through which a chain batch is first copied
 * chain-minor ([ncols][C]), so that a gathered non-zero reads its C chains from one contiguous segment instead of C
 * cache lines.  Identical sums in identical order either way (bit-equal results). */
int pxm_csr_matvec(const int64_t* indptr, const int32_t* indices, const void* vals, int vals_complex,
                   int64_t nrows, int64_t ncols, const void* x, void* y, int C, int dtype, void* scratch,
                   pxm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
