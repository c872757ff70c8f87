"""Host side of the grid-cap tests of the generic kernels (tests/test_gpu_generic_caps.py) -- no GPU needed.

The generic layer (csrc/elementwise.hip, skrock.hip, spmv.hip and the slice rule of reduce.h) launches a capped grid and loops
over the rest.  This file reads the caps out of the sources, derives from them the shapes at which the loops take a second trip,
states every operation per element in long double, and fixes the error bounds the device results are held to.

The bounds (u = 2^-53, one rounding of a float64 operation), derived and not measured:

* real soft, weak-lensing mapping, gather, scatter: ONE rounded operation per component (|x| - T; v k; v w), in the order numpy
  takes, so the device must give numpy's float64 result bit for bit; the long-double model then differs from it by one rounding,
  |f64 - model| <= u |model|.
* complex soft, z (a - T) / a with a = sqrt(fma(x, x, y y)): a carries at most 1.5 u a (fma, sqrt); a - T adds one rounding
  relative to a - T <= a on top of the 1.5 u a it inherits; the quotient s = (a - T) / a <= 1 then has an ABSOLUTE error of at
  most 1.5 u + u + 1.5 u s + u s <= 5 u, and z s one more rounding: 6 u |z| per component pair, 8 u |z| held.  The cancellation
  of a - T next to the threshold leaves this absolute error where it is (the result itself is then tiny), and a threshold
  decision that falls the other way than the model's changes the result by no more than the 1.5 u |z| the modulus is off.
* residual w (p - d): one rounding of the difference, relative to |p - d| <= |p| + |d|, and the product -- one rounding for a real
  w, (1 + sqrt 2) u for the four products and two sums of a complex one: below 4 u |w| (|p| + |d|) in moduli, 6 u held.
* chain step, MYULA step, SKROCK stage: sums of four or five terms, each a product of a coefficient (itself one or two roundings
  off its long-double value) and an element; every partial sum is bounded by the sum of the moduli of the terms, so the error is
  a small multiple of u times that sum.  Held: 1e-14 (90 u) times the sum, plus 1e-300 -- the bound tests/test_gpu_skrock.py uses.
  (The MYULA prox soft(X, T) enters with its 8 u |X| times d / l = 1 / 2, next to the term (1 - d / l) |X| = |X| / 2 of the sum.)
* CSR row sum_k a_k x_k with S = sum_k |a_k| |x_k|: a sum of m terms in ANY order is within (m - 1) u S of the exact sum to first
  order (the device adds lane by lane, then a 64-lane butterfly: 6 more additions on top of the lane's own), and a complex
  product adds (1 + sqrt 2) u of its own modulus: (nnz_row + 8) u S per row covers both, second-order terms included.
"""
import functools
import os
import re

import numpy as np
import pytest

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pxmcmc_amd", "csrc")


# ---- the caps, read from the sources ------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    """the groups of the one place ``pattern`` matches (re.S) -- a source that no longer reads like this fails here, loudly"""
    found = re.findall(pattern, text, re.S)
    assert len(found) == 1, f"{what}: expected one match of {pattern!r} in the source, found {len(found)}"
    g = found[0]
    return tuple(int(v) for v in (g if isinstance(g, tuple) else (g,)))


def read_caps():
    ew, sk, sp, red = _src("elementwise.hip"), _src("skrock.hip"), _src("spmv.hip"), _src("reduce.h")
    caps = {}
    # dim3 ew_grid(n, C): bx = (n + 255) / 256, capped
    (body,) = re.findall(r"static inline dim3 ew_grid\(int64_t n, int C\) \{(.*?)\n\}", ew, re.S)
    r0, block = _one(r"int64_t bx = \(n \+ (\d+)\) / (\d+);", body, "ew_grid block")
    hi, to = _one(r"if \(bx > (\d+)\) bx = (\d+);", body, "ew_grid cap")
    assert r0 == block - 1 and hi == to
    caps["ew_block"], caps["ew_cap"] = block, hi
    # every launch on ew_grid runs workgroups of that many threads
    for call in re.findall(r"hipLaunchKernelGGL\([^;]*?ew_grid\(\w+, C\), dim3\((\d+)\)", ew):
        assert int(call) == block
    assert set(re.findall(r"dim3 g = ew_grid\(\w+, C\), b\((\d+)\);", ew)) == {str(block)}
    # dim3 sk_grid(n, C): min((n + 255) / 256, max(1, 2048 / C))
    (body,) = re.findall(r"static inline dim3 sk_grid\(int64_t n, int C\) \{(.*?)\n\}", sk, re.S)
    (caps["sk_total"],) = _one(r"int64_t cap = std::max<int64_t>\(1, (\d+) / C\);", body, "sk_grid cap")
    r0, caps["sk_block"] = _one(r"std::min<int64_t>\(\(n \+ (\d+)\) / (\d+), cap\)", body, "sk_grid block")
    assert r0 == caps["sk_block"] - 1
    assert set(re.findall(r"k_skrock_stage<[^>]*>\), g, dim3\((\d+)\)", sk)) == {str(caps["sk_block"])}
    # pxm_csr_matvec: one wave per row, waves_per_block waves per workgroup, capped workgroups
    (body,) = re.findall(r'extern "C" int pxm_csr_matvec\(.*?\n\}', sp, re.S)
    (caps["csr_waves"],) = _one(r"const int waves_per_block = (\d+);", body, "csr waves per block")
    hi, to = _one(r"if \(blocks > (\d+)\) blocks = (\d+);", body, "csr block cap")
    assert hi == to
    caps["csr_cap"] = hi
    (blk,) = _one(r"const dim3 grid\(\(unsigned\)blocks, \(unsigned\)ysplit\), blk\((\d+)\);", body, "csr block size")
    assert blk == 64 * caps["csr_waves"]  # wave64: the kernel counts its waves as blockDim.x >> 6
    assert "(blockDim.x >> 6)" in sp
    # the chain-minor transpose and the operand size from which it is taken
    caps["minor_cap"], r0, caps["minor_block"] = _one(
        r"const unsigned tb = \(unsigned\)std::min<int64_t>\((\d+), \(ncols \+ (\d+)\) / (\d+)\);", body, "k_chains_to_minor cap")
    assert r0 == caps["minor_block"] - 1
    assert set(re.findall(r"k_chains_to_minor<\w+>, dim3\(tb\), dim3\((\d+)\)", body)) == {str(caps["minor_block"])}
    (shift,) = _one(r"\(int64_t\)C \* ncols \* \(dtype \? 16 : 8\) >= \(1 << (\d+)\)", body, "chain-minor threshold")
    caps["minor_bytes"] = 1 << shift
    # reduce.h
    caps["red_min"], caps["red_max"] = _one(r"constexpr int RED_SLICES_MIN = (\d+), RED_SLICES_MAX = (\d+);", red, "RED_SLICES")
    r0, caps["red_per_slice"] = _one(r"std::max<int64_t>\(RED_SLICES_MIN, \(n \+ (\d+)\) / (\d+)\)\)", red, "red_slices rule")
    assert r0 == caps["red_per_slice"] - 1
    return caps


CAPS = read_caps()
EW_CAP, EW_BLOCK = CAPS["ew_cap"], CAPS["ew_block"]
EW_PASS = EW_CAP * EW_BLOCK                    # elements of one chain that one pass of the capped grid covers
EW_N, EW_C = EW_PASS + EW_BLOCK + 1, 2          # one full pass, a whole second workgroup's worth and one more thread; odd
WL_NPIX = EW_PASS + 1500                       # the pixel array the gather / scatter index into (ndata = EW_N)
SK_TOTAL, SK_BLOCK, SK_C = CAPS["sk_total"], CAPS["sk_block"], 64
SK_CAP = max(1, SK_TOTAL // SK_C)              # workgroups per chain at SK_C chains
SK_N = 2 * SK_CAP * SK_BLOCK + SK_BLOCK + 1     # three passes
CSR_CAP, CSR_WAVES = CAPS["csr_cap"], CAPS["csr_waves"]
CSR_PASS = CSR_CAP * CSR_WAVES                 # rows of one pass
CSR_ROWS, CSR_COLS = CSR_PASS + 261, 70001
CSR_EMPTY, CSR_LONG, CSR_LONG_NNZ = (5, CSR_PASS + 7), (9, CSR_PASS + 3), 200
MINOR_CAP, MINOR_BLOCK, MINOR_BYTES = CAPS["minor_cap"], CAPS["minor_block"], CAPS["minor_bytes"]
MINOR_PASS = MINOR_CAP * MINOR_BLOCK           # columns of one pass of the transpose
CSR_E_ROWS, CSR_E_COLS = 64, MINOR_PASS + 3
CSR_E_SPECIAL = (0, MINOR_PASS - 1, MINOR_PASS, MINOR_PASS + 2)
RED_SLICES_MAX, RED_PER_SLICE = CAPS["red_max"], CAPS["red_per_slice"]
RED_N = RED_SLICES_MAX * RED_PER_SLICE + RED_PER_SLICE + 1


def test_caps_are_the_ones_the_gpu_shapes_are_built_from():
    """a changed cap fails here instead of quietly moving a loop's second trip out of the tested shapes"""
    assert (EW_CAP, EW_BLOCK, EW_PASS, EW_N) == (2048, 256, 524288, 524545)
    assert (SK_TOTAL, SK_BLOCK, SK_CAP, SK_N) == (2048, 256, 32, 16641)
    assert (CSR_CAP, CSR_WAVES, CSR_PASS, CSR_ROWS) == (16384, 4, 65536, 65797)
    assert (MINOR_CAP, MINOR_BLOCK, MINOR_PASS, CSR_E_COLS, MINOR_BYTES) == (4096, 256, 1048576, 1048579, 1 << 20)
    assert (CAPS["red_min"], RED_SLICES_MAX, RED_PER_SLICE, RED_N) == (64, 1024, 2048, 2099201)
    # what the shapes are for
    assert EW_N % 2 == 1 and EW_N > EW_PASS + EW_BLOCK               # odd: chain 1 of a real array starts 8 bytes off 16
    assert -(-SK_N // (SK_CAP * SK_BLOCK)) == 3                      # three passes
    assert CSR_ROWS > CSR_PASS and CSR_COLS > CSR_PASS               # the adjoint (CSR_COLS rows) strides too
    for C_, minor in ((1, False), (2, True), (3, True)):             # chain-minor operand from C = 2 on (real vectors)
        assert (C_ > 1 and C_ * CSR_COLS * 8 >= MINOR_BYTES) == minor
        assert (C_ > 1 and C_ * CSR_ROWS * 8 >= MINOR_BYTES) == minor  # and so for the adjoint, whose operand is CSR_ROWS long
    assert 2 * CSR_E_COLS * 8 >= MINOR_BYTES and CSR_E_COLS > MINOR_PASS
    assert (RED_N + RED_PER_SLICE - 1) // RED_PER_SLICE == 1026 > RED_SLICES_MAX  # uncapped it would be 1026 slices


# ---- the models: long double, per element -------------------------------------------------------------------------------------
def ld(x):
    x = np.asarray(x)
    return x.astype(CLD if np.iscomplexobj(x) else LD)


def scale(k, x):
    """real k (a scalar, or an array that broadcasts against x) times the real or complex x, in long double; a complex x is
    scaled component by component (the same two products a complex multiplication by k + 0j keeps, at a quarter of its cost)"""
    x = ld(x)
    if x.dtype != CLD:
        return ld(k) * x
    parts = np.ascontiguousarray(x).view(LD).reshape(x.shape + (2,))
    return np.ascontiguousarray(ld(k)[..., None] * parts).view(CLD).reshape(np.broadcast_shapes(np.shape(k), x.shape))


def soft_model(X, T):
    """sign(X) (|X| - T) where |X| > T, else 0"""
    x, t = ld(X), ld(T)
    a = np.abs(x)
    return scale(np.where(a > t, (a - t) / np.where(a > 0, a, 1), 0), x)


def soft_f64(X, T):
    """numpy's float64 evaluation in the reference's order (x / |x|) (|x| - T): what the real kernel gives bit for bit"""
    a = np.abs(X)
    return np.where(a > T, X / np.where(a > 0, a, 1) * (a - T), 0)


def soft_cplx_bound(X):
    return 8 * U * np.abs(ld(X))


def residual_model(preds, data, invcov):
    d = ld(preds) - ld(data)
    return ld(invcov) * d if np.iscomplexobj(invcov) else scale(invcov, d)


def residual_bound(preds, data, invcov):
    return 6 * U * np.abs(ld(invcov)) * (np.abs(ld(preds)) + np.abs(ld(data)))


def _sum_terms(terms):
    return sum(terms), 1e-14 * sum(np.abs(t) for t in terms) + 1e-300


def chain_step_model(X, P, g, w, delta, lmda):
    """(1 - d/l) X + (d/l) P - d g + sqrt(2 d) w -> (model, bound); ``delta``: a float or one value per chain"""
    d = ld(delta).reshape(-1, 1) if np.ndim(delta) else LD(delta)
    r = d / LD(lmda)
    return _sum_terms([scale(1 - r, X), scale(r, P), scale(-d, g), scale(np.sqrt(2 * d), w)])


def myula_step_model(X, g, T, w, delta, lmda):
    return chain_step_model(X, soft_model(X, T), g, w, delta, lmda)


def skrock_stage_model(U_, a, b=0.0, c=0.0, e=0.0, r=0.0, P=None, G=None, V=None, Z=None):
    """a U + b P + c G + e V + r Z -> (model, bound); a term whose coefficient is zero is left out, as the kernel leaves it out"""
    terms = [scale(a, U_)]
    for k, t in ((b, P), (c, G), (e, V), (r, Z)):
        if k != 0:
            terms.append(scale(k, t))
    return _sum_terms(terms)


def wl_mapping_model(flm, kernel):
    out = scale(kernel, flm)
    out[..., :4] = 0
    return out


def wl_mapping_f64(flm, kernel):
    out = flm * kernel
    out[..., :4] = 0
    return out


def wl_gather_model(f, idx, w=None):
    return scale(1 if w is None else w, ld(f)[..., idx])


def wl_gather_f64(f, idx, w=None):
    return f[..., idx] * (1.0 if w is None else w)


def wl_scatter_model(g, idx, npix, w=None, dtype=CLD):
    out = np.zeros(g.shape[:-1] + (npix,), dtype=dtype)
    out[..., idx] = g * (1.0 if w is None else w) if dtype is not CLD else scale(1 if w is None else w, g)
    return out


def wl_scatter_f64(g, idx, npix, w=None):
    return wl_scatter_model(g, idx, npix, w, dtype=np.complex128)


def csr_model(indptr, indices, vals, x):
    """y[c][row] = sum_k vals[k] x[c][indices[k]] over the row, as ONE np.add.reduceat over the long-double products, empty rows
    set to zero -> (y, S) with the per-row scale S = sum_k |a_k| |x_k|; x is [ncols] or [C, ncols]"""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    x2 = np.atleast_2d(x)
    cplx = np.iscomplexobj(vals) or np.iscomplexobj(x2)
    nrows, nnz = indptr.size - 1, indices.size
    y = np.zeros((x2.shape[0], nrows), dtype=CLD if cplx else LD)
    S = np.zeros((x2.shape[0], nrows), dtype=LD)
    if nnz:
        # reduceat over the starts of the non-empty rows only: a segment then runs to the start of the next non-empty row, which
        # is the end of its own (at an empty row's start reduceat would return the element there, and a start equal to nnz is
        # refused); the empty rows keep their zeros
        full = np.diff(indptr) > 0
        start = indptr[:-1][full]
        a, aa = ld(vals), np.abs(ld(vals))
        for c in range(x2.shape[0]):
            xc = ld(x2[c])[indices]
            y[c, full] = np.add.reduceat(a * xc, start)
            S[c, full] = np.add.reduceat(aa * np.abs(xc), start)
    return (y[0], S[0]) if np.ndim(x) == 1 else (y, S)


def csr_bound(indptr, S):
    return (np.diff(np.asarray(indptr, dtype=np.int64)) + 8) * U * S


# ---- the inputs of the GPU cases (made once, shared with the CPU checks below; treat as read-only) -----------------------------
def _normal(rng, shape, cplx):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape) if cplx else rng.normal(size=shape)


@functools.lru_cache(maxsize=None)
def ew_inputs(cplx):
    """case a: state X, prox P, gradient g, real and complex noise [EW_C][EW_N]; thresholds T, data d and inverse covariances
    [EW_N]"""
    rng = np.random.default_rng(524545 + int(cplx))
    sh = (EW_C, EW_N)
    out = dict(X=_normal(rng, sh, cplx), P=_normal(rng, sh, cplx), g=_normal(rng, sh, cplx), w_real=rng.normal(size=sh),
               w_cplx=_normal(rng, sh, True), T=np.abs(rng.normal(size=EW_N)) * 0.3, d=_normal(rng, EW_N, cplx),
               ic_real=1.0 + rng.random(EW_N), ic_cplx=_normal(rng, EW_N, True))
    for v in out.values():
        v.setflags(write=False)
    return out


EW_TS, EW_LMDA, EW_DELTA, EW_DELTAS = 0.4, 2e-3, 1e-3, (1e-3, 7e-4)  # scalar threshold; d / l = 1 / 2 and 0.35


@functools.lru_cache(maxsize=None)
def wl_inputs():
    """case a, weak lensing: field f [EW_C][WL_NPIX], data g [EW_C][EW_N], the sorted index set without repeats, weights, and
    the harmonic kernel [EW_N]"""
    rng = np.random.default_rng(77)
    idx = np.sort(rng.permutation(WL_NPIX)[:EW_N]).astype(np.int64)
    out = dict(f=_normal(rng, (EW_C, WL_NPIX), True), g=_normal(rng, (EW_C, EW_N), True), idx=idx, w=0.5 + rng.random(EW_N),
               flm=_normal(rng, (EW_C, EW_N), True), kernel=-np.sqrt(1.0 + rng.random(EW_N)))
    for v in out.values():
        v.setflags(write=False)
    return out


SK_COEFS = {"stage0": (1.0, 0.0, 0.0, 0.0, 0.37), "stage1": (-0.8, 0.8, -1e-3, 1.0, 0.21), "stagej": (1.3, 0.5, -2e-3, -0.3, 0.0)}
SK_TS = 0.4


@functools.lru_cache(maxsize=None)
def sk_inputs(cplx):
    rng = np.random.default_rng(16641 + int(cplx))
    sh = (SK_C, SK_N)
    out = dict(U=_normal(rng, sh, cplx), P=_normal(rng, sh, cplx), G=_normal(rng, sh, cplx), V=_normal(rng, sh, cplx),
               T=np.abs(rng.normal(size=SK_N)))
    for v in out.values():
        v.setflags(write=False)
    return out


def _rows_to_csr(rng, cnt, ncols, cplx, max_gap):
    """rows of cnt[row] non-zeros at increasing columns without repeats (a random start, random gaps of 1 .. max_gap)"""
    nrows, nnz = cnt.size, int(cnt.sum())
    indptr = np.concatenate(([0], np.cumsum(cnt))).astype(np.int64)
    gaps = rng.integers(1, max_gap + 1, size=nnz)
    csum = np.concatenate(([0], np.cumsum(gaps)))
    off = csum[1:] - np.repeat(csum[indptr[:-1]], cnt)   # 1 .. span within the row, increasing
    span = csum[indptr[1:]] - csum[indptr[:-1]]
    assert span.max() < ncols
    base = np.floor(rng.random(nrows) * (ncols - span)).astype(np.int64) - 1  # -1 .. ncols - 1 - span
    indices = np.repeat(base, cnt) + off
    assert indices.min() >= 0 and indices.max() < ncols
    vals = _normal(rng, nnz, cplx)
    return indptr, indices.astype(np.int32), vals


@functools.lru_cache(maxsize=None)
def csr_rows_case(cplx_mat, adjoint=False):
    """case d: (indptr, indices, vals, shape) of the CSR_ROWS x CSR_COLS matrix -- 1 to 5 non-zeros a row, rows CSR_EMPTY empty,
    rows CSR_LONG of 200 (four lane strides of the wave) -- or of its conjugate transpose as a CSR of its own"""
    rng = np.random.default_rng(65797 + int(cplx_mat))
    cnt = rng.integers(1, 6, size=CSR_ROWS)
    cnt[list(CSR_EMPTY)] = 0
    cnt[list(CSR_LONG)] = CSR_LONG_NNZ
    assert cnt[-1] >= 1
    indptr, indices, vals = _rows_to_csr(rng, cnt, CSR_COLS, cplx_mat, 300)
    shape = (CSR_ROWS, CSR_COLS)
    if adjoint:  # as PathIntegral builds it: path_matrix.conj().T.tocsr()
        import scipy.sparse as sp

        m = sp.csr_matrix((vals, indices, indptr), shape=shape).conj().T.tocsr()
        m.sort_indices()
        indptr, indices, vals, shape = m.indptr.astype(np.int64), m.indices.astype(np.int32), np.array(m.data), m.shape
    for v in (indptr, indices, vals):
        v.setflags(write=False)
    return indptr, indices, vals, shape


@functools.lru_cache(maxsize=None)
def csr_rows_vectors(cplx_vec, adjoint=False):
    """three chains of operands for case d"""
    rng = np.random.default_rng(70001 + int(cplx_vec) + 2 * int(adjoint))
    x = _normal(rng, (3, CSR_ROWS if adjoint else CSR_COLS), cplx_vec)
    x.setflags(write=False)
    return x


CSR_KINDS = [(False, False), (False, True), (True, True)]  # (matrix complex, vector complex)


@functools.lru_cache(maxsize=None)
def csr_rows_model(cplx_mat, cplx_vec, adjoint=False):
    """(y, S, bound) of case d for the three chains"""
    indptr, indices, vals, _ = csr_rows_case(cplx_mat, adjoint)
    y, S = csr_model(indptr, indices, vals, csr_rows_vectors(cplx_vec, adjoint))
    return y, S, csr_bound(indptr, S)


@functools.lru_cache(maxsize=None)
def csr_cols_case():
    """case e: CSR_E_ROWS x CSR_E_COLS real, non-zeros at random columns and at CSR_E_SPECIAL (the last column of the transpose
    kernel's first pass, the first of its second, and the last of all); two chains of operands"""
    rng = np.random.default_rng(1048579)
    rows = []
    for r in range(CSR_E_ROWS):
        cols = rng.integers(0, CSR_E_COLS, size=6)
        special = CSR_E_SPECIAL if r in (0, 17, CSR_E_ROWS - 1) else (CSR_E_SPECIAL[r % 4],)
        tail = rng.integers(MINOR_PASS - 3, CSR_E_COLS, size=1)  # and one more around the end of the first pass
        rows.append(np.unique(np.concatenate((cols, special, tail))))
    indptr = np.concatenate(([0], np.cumsum([c.size for c in rows]))).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    vals = rng.normal(size=indices.size)
    x = rng.normal(size=(2, CSR_E_COLS))
    for v in (indptr, indices, vals, x):
        v.setflags(write=False)
    return indptr, indices, vals, (CSR_E_ROWS, CSR_E_COLS), x


# ---- the comparison every GPU case runs ----------------------------------------------------------------------------------------
def worst(got, model, bound):
    """(number of elements whose error exceeds the bound or is NaN, index of the worst, its error / bound)"""
    err = np.abs(np.asarray(got) - model)
    bound = np.broadcast_to(bound, err.shape)
    ok = err <= bound  # (False for a NaN)
    ratio = np.where(np.isnan(err), np.inf, np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0).astype(LD), where=bound > 0))
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    return int(ratio.size - ok.sum()), tuple(int(i) for i in k), float(ratio[k]) if ratio.size else 0.0


def assert_within(got, model, bound, what):
    """every element of ``got`` within ``bound`` of ``model``; the message names the worst element"""
    nbad, k, ratio = worst(got, model, bound)
    print(f"RATIO {what}: worst error / bound = {ratio:.3g} at index {k}")
    assert nbad == 0, (f"{what}: {nbad} of {np.size(got)} elements outside the bound; worst at index {k}: got {np.asarray(got)[k]!r}, "
                       f"model {model[k]!r}, error / bound = {ratio:.3g}")
    return ratio


def assert_same(got, want, what):
    """every element of ``got`` equal to ``want`` (as numpy's array_equal has it: a NaN is unequal); names the first that is not"""
    got, want = np.asarray(got), np.broadcast_to(want, np.shape(got))
    bad = ~(got == want)
    if bad.any():
        k = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} elements differ; first at index {k}: got {got[k]!r}, want {want[k]!r}")


# ---- CPU tests: the models against the oracle and scipy at small n --------------------------------------------------------------
def _close(model, f64, ulps):
    model = np.asarray(model)
    return np.all(np.abs(model - f64) <= ulps * U * np.abs(model) + 1e-300)


@pytest.mark.parametrize("cplx", [False, True])
def test_models_agree_with_the_oracle(cplx):
    from oracle import pxmcmc_np as ref

    rng = np.random.default_rng(3)
    n = 301
    X, P, g, w = (_normal(rng, n, cplx) for _ in range(4))
    T = np.abs(rng.normal(size=n)) * 0.5
    for t in (0.4, T):
        got, want = soft_model(X, t), ref.soft(X, t)
        assert np.array_equal(got == 0, want == 0)
        assert np.all(np.abs(got - want) <= 8 * U * np.abs(X))
        if not cplx:
            assert np.array_equal(soft_f64(X, t), want)
    m, bound = chain_step_model(X, P, g, w, 1e-3, 2e-3)
    assert np.all(np.abs(m - ref.chain_step(X, P, g, 1e-3, 2e-3, w)) <= bound)
    m, bound = myula_step_model(X, g, T, w, 1e-3, 2e-3)
    assert np.all(np.abs(m - ref.chain_step(X, ref.soft(X, T), g, 1e-3, 2e-3, w)) <= bound)
    # per-chain delta: row c is the step with delta[c]
    X2, P2, g2, w2 = (np.stack([v, -v]) for v in (X, P, g, w))
    m2, _ = chain_step_model(X2, P2, g2, w2, np.array([1e-3, 7e-4]), 2e-3)
    for c, d in enumerate((1e-3, 7e-4)):
        m1, _ = chain_step_model(X2[c], P2[c], g2[c], w2[c], d, 2e-3)
        assert np.array_equal(m2[c], m1)
    # residual: the oracle's apply_invcov(invcov, preds - data)
    d = _normal(rng, n, cplx)
    for ic in ([1 + rng.random(n)] + ([_normal(rng, n, True)] if cplx else [])):
        want = ref.apply_invcov(ic, X - d)
        assert np.all(np.abs(residual_model(X, d, ic) - want) <= residual_bound(X, d, ic))
    # SKROCK stage: the sum of tests/test_gpu_skrock.py
    for a, b, c, e, r in SK_COEFS.values():
        m, bound = skrock_stage_model(X, a, b, c, e, r, P=P, G=g, V=w, Z=X[::-1])
        want = a * X + b * P + c * g + e * w + r * X[::-1]
        assert np.all(np.abs(m - want) <= bound)


def test_weaklensing_models_agree_with_the_oracle():
    from oracle import pxmcmc_np as ref

    L = 9
    rng = np.random.default_rng(4)
    flm = _normal(rng, L * L, True)
    k = ref.wl_harmonic_kernel(L)
    want = ref.wl_harmonic_mapping(flm.copy(), k)
    assert np.array_equal(wl_mapping_f64(flm, k), want) and _close(wl_mapping_model(flm, k), want, 1)
    assert np.all(wl_mapping_model(flm, k)[:4] == 0)
    mask = rng.random((L, 2 * L - 1)) < 0.6
    ngal = rng.integers(1, 30, size=mask.shape)
    wl = ref.WeakLensing(L, mask=mask, ngal=ngal)
    idx = np.flatnonzero(mask.reshape(-1))
    f = _normal(rng, wl.npix, True)
    want = (f.reshape(wl.shape)[wl.mask] * wl.inv_cov).flatten()  # WeakLensing.forward's last line
    assert np.array_equal(wl_gather_f64(f, idx, wl.inv_cov), want) and _close(wl_gather_model(f, idx, wl.inv_cov), want, 1)
    assert np.array_equal(wl_gather_f64(f, idx), f[idx])
    gam = _normal(rng, wl.ndata, True)
    full = np.zeros(wl.shape, dtype=complex)
    full[wl.mask] = gam * wl.inv_cov  # WeakLensing.adjoint's first lines
    assert np.array_equal(wl_scatter_f64(gam, idx, wl.npix, wl.inv_cov), full.reshape(-1))
    assert _close(wl_scatter_model(gam, idx, wl.npix, wl.inv_cov), full.reshape(-1), 1)
    assert np.all(wl_scatter_model(gam, idx, wl.npix)[~mask.reshape(-1)] == 0)


@pytest.mark.parametrize("cplx_mat,cplx_vec", CSR_KINDS)
def test_csr_model_agrees_with_scipy_and_the_oracle(cplx_mat, cplx_vec):
    import scipy.sparse as sp
    from oracle import pxmcmc_np as ref

    rng = np.random.default_rng(5)
    A = sp.random(40, 57, density=0.15, random_state=np.random.RandomState(1), format="csr")
    if cplx_mat:
        A = (A + 1j * sp.random(40, 57, density=0.15, random_state=np.random.RandomState(2), format="csr")).tocsr()
    A = sp.vstack([A, sp.csr_matrix((3, 57))]).tolil()  # trailing empty rows
    A[7] = 0                                            # and one in the middle
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    assert (np.diff(A.indptr) == 0).sum() >= 4
    pi = ref.PathIntegral(A)
    x = _normal(rng, (3, 57), cplx_vec)
    y, S = csr_model(A.indptr, A.indices, A.data, x)
    for c in range(3):
        want = pi.forward(x[c])
        assert np.all(np.abs(y[c] - want) <= csr_bound(A.indptr, S[c]))
        assert np.all(y[c][np.diff(A.indptr) == 0] == 0) and np.all(S[c][np.diff(A.indptr) == 0] == 0)
        np.testing.assert_allclose(S[c].astype(float), abs(A).dot(np.abs(x[c])), rtol=1e-14)
    y1, S1 = csr_model(A.indptr, A.indices, A.data, x[1])
    assert np.array_equal(y1, y[1]) and np.array_equal(S1, S[1])
    # the adjoint, as a CSR of its own
    Ah = pi.path_matrix_adj
    Ah.sort_indices()
    v = _normal(rng, 43, cplx_vec)
    ya, Sa = csr_model(Ah.indptr, Ah.indices, Ah.data, v)
    assert np.all(np.abs(ya - pi.adjoint(v)) <= csr_bound(Ah.indptr, Sa))


# ---- CPU tests: numpy's / scipy's float64 evaluation stays inside each bound at the shapes of the GPU cases --------------------
@pytest.mark.parametrize("cplx", [False, True])
def test_float64_elementwise_meets_the_bounds_at_the_gpu_shape(cplx):
    from oracle import pxmcmc_np as ref

    v = ew_inputs(cplx)
    X, P, g, T = v["X"], v["P"], v["g"], v["T"]
    assert X.shape == (EW_C, EW_N)
    for t in (EW_TS, T):
        f64 = ref.soft(X, t)
        if cplx:
            assert_within(f64, soft_model(X, t), soft_cplx_bound(X), "float64 complex soft")
        else:
            assert_same(soft_f64(X, t), f64, "float64 real soft, two ways")
            assert_within(f64, soft_model(X, t), U * np.abs(soft_model(X, t)), "float64 real soft")
    for ic in ([v["ic_real"]] + ([v["ic_cplx"]] if cplx else [])):
        assert_within(ic * (X - v["d"]), residual_model(X, v["d"], ic), residual_bound(X, v["d"], ic), "float64 residual")
    for w in ([v["w_real"]] + ([v["w_cplx"]] if cplx else [])):
        for delta in (EW_DELTA, np.array(EW_DELTAS)):
            d = delta if np.ndim(delta) == 0 else delta[:, None]
            m, bound = chain_step_model(X, P, g, w, delta, EW_LMDA)
            assert_within(ref.chain_step(X, P, g, d, EW_LMDA, w), m, bound, "float64 chain step")
            m, bound = myula_step_model(X, g, T, w, delta, EW_LMDA)
            assert_within(ref.chain_step(X, ref.soft(X, T), g, d, EW_LMDA, w), m, bound, "float64 MYULA step")


def test_float64_weaklensing_pieces_are_one_rounding_from_the_model():
    v = wl_inputs()
    idx = v["idx"]
    assert idx.size == EW_N and np.all(np.diff(idx) > 0) and idx[-1] < WL_NPIX
    m = wl_mapping_model(v["flm"], v["kernel"])
    assert_within(wl_mapping_f64(v["flm"], v["kernel"]), m, U * np.abs(m), "float64 mapping")
    for w in (None, v["w"]):
        m = wl_gather_model(v["f"], idx, w)
        assert_within(wl_gather_f64(v["f"], idx, w), m, U * np.abs(m), "float64 gather")
        m = wl_scatter_model(v["g"], idx, WL_NPIX, w)
        assert_within(wl_scatter_f64(v["g"], idx, WL_NPIX, w), m, U * np.abs(m), "float64 scatter")


@pytest.mark.parametrize("cplx", [False, True])
def test_float64_skrock_stage_meets_the_bound_at_the_gpu_shape(cplx):
    v = sk_inputs(cplx)
    Uv, P, G, V = v["U"], v["P"], v["G"], v["V"]
    assert Uv.shape == (SK_C, SK_N)
    Z = V[::-1]
    for name, (a, b, c, e, r) in SK_COEFS.items():
        # the prox term: a given array, or the soft threshold (float64 next to its long-double model)
        for P64, Pld in (((P, P), (soft_f64(Uv, SK_TS), soft_model(Uv, SK_TS))) if b else ((None, None),)):
            m, bound = skrock_stage_model(Uv, a, b, c, e, r, P=Pld, G=G, V=V, Z=Z)
            f64 = a * Uv + (b * P64 if b else 0) + c * G + e * V + r * Z
            assert_within(f64, m, bound, f"float64 SKROCK {name}")


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("cplx_mat,cplx_vec", CSR_KINDS)
def test_float64_csr_meets_the_bound_at_the_gpu_shape(cplx_mat, cplx_vec, adjoint):
    import scipy.sparse as sp

    indptr, indices, vals, shape = csr_rows_case(cplx_mat, adjoint)
    cnt = np.diff(indptr)
    if not adjoint:
        assert shape == (CSR_ROWS, CSR_COLS) and cnt[-1] >= 1 and cnt.max() == CSR_LONG_NNZ
        assert all(cnt[r] == 0 for r in CSR_EMPTY) and all(cnt[r] == CSR_LONG_NNZ for r in CSR_LONG)
        others = np.delete(cnt, CSR_EMPTY + CSR_LONG)
        assert others.min() == 1 and others.max() == 5
    else:
        assert shape == (CSR_COLS, CSR_ROWS)
    for r in range(0, shape[0], 997):  # increasing columns without repeats
        assert np.all(np.diff(indices[indptr[r]:indptr[r + 1]]) > 0)
    A = sp.csr_matrix((vals, indices, indptr), shape=shape)
    x = csr_rows_vectors(cplx_vec, adjoint)
    y, S, bound = csr_rows_model(cplx_mat, cplx_vec, adjoint)
    for c in range(3):
        assert_within(A.dot(x[c]), y[c], bound[c], f"scipy float64 CSR product, chain {c}")
        assert np.all(y[c][cnt == 0] == 0)


def test_float64_csr_columns_case():
    import scipy.sparse as sp

    indptr, indices, vals, shape, x = csr_cols_case()
    assert shape == (CSR_E_ROWS, CSR_E_COLS) and set(CSR_E_SPECIAL) <= set(indices.tolist())
    assert (indices >= MINOR_PASS).sum() >= CSR_E_ROWS // 2  # columns past the transpose kernel's first pass are gathered
    for r in range(CSR_E_ROWS):
        assert np.all(np.diff(indices[indptr[r]:indptr[r + 1]]) > 0)
    y, S = csr_model(indptr, indices, vals, x)
    A = sp.csr_matrix((vals, indices, indptr), shape=shape)
    for c in range(2):
        assert_within(A.dot(x[c]), y[c], csr_bound(indptr, S[c]), f"scipy float64 CSR product (columns case), chain {c}")


def test_worst_and_the_assertions_catch_what_they_are_for():
    """a NaN (an element never written) and an element just past its bound both fail, and the message names the index"""
    model = ld(np.arange(1.0, 7.0).reshape(2, 3))
    got = np.arange(1.0, 7.0).reshape(2, 3)
    assert worst(got, model, 0.0) == (0, (0, 0), 0.0)
    for bad in (np.nan, 5.0 + 1e-9):
        g2 = got.copy()
        g2[1, 1] = bad
        nbad, k, _ = worst(g2, model, 1e-12)
        assert (nbad, k) == (1, (1, 1))
        with pytest.raises(AssertionError, match=r"index \(1, 1\)"):
            assert_within(g2, model, 1e-12, "x")
        with pytest.raises(AssertionError, match=r"index \(1, 1\)"):
            assert_same(g2, got, "x")
    assert_same(np.array([0.0, -0.0]), 0.0, "zeros")
