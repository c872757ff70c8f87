"""The phi-DFT stage without a GPU: a long-double model of the stage and its own error, the unit selection
(csrc/dft.hip: dft_geometry through pxm_host_dft_geometry) and the refusal of bandlimits the stage has no unit for.

The model and the case table are shared with tests/test_gpu_dft.py, which holds every unit to them on the device:
  dft_ld       the direct O(n^2) DFT in long double, angles reduced in integers: the reference
  bluestein64  Bluestein's algorithm in float64 at the unit's transform length M with the tables of csrc/tables.cpp (chirp
               and filter spectrum computed in long double and rounded): what a correct unit computes up to the order of
               its sums.  Its error against dft_ld, in units of eps ||x||_2 of the ring, is the measure the device is held
               to (4 x, the rule of test_rec_host.model_tol) and is itself capped at MODEL_CAP here.
"""
import ctypes as C
import functools

import numpy as np
import pytest

LD, CLD = np.longdouble, np.clongdouble
EPS = float(np.finfo(np.float64).eps)
MODEL_CAP = 16.0  # max |bluestein64 - dft_ld| / (eps ||x||_2): measured 4.4 .. 6.8 on dense rings, 6.7 on impulses
LDS_MAX = 160 * 1024

# ---- the cases of the GPU suite: (unit, L, environment at plan creation) ---------------------------------------------------
NO_W = {"PXM_DFT_NO_W": "1"}
CASES = (
    [("pair1", L, {}) for L in (1, 2, 5, 32)]
    + [("pair2", L, {}) for L in (33, 35, 64)]
    + [("pair4", L, {}) for L in (65, 67, 128)]
    + [("pair8", 129, {}), ("pair8", 255, {}), ("pair8", 256, {"PXM_DFT_PFA": "0"})]
    + [("exact", 256, {})]
    + [("quad", L, {}) for L in (257, 300, 512)]
    + [("radix2", L, NO_W) for L in (2, 9, 256, 257, 512)]
    + [("radix2", 513, {}), ("radix2", 1024, {})]
)


def case_id(case):
    unit, L, env = case
    return f"{unit}-L{L}" + ("-" + "-".join(k[4:].lower() + v for k, v in env.items()) if env else "")


def expected_geometry(L, env=None):
    """(unit, M, per_workgroup, threads, lds, exact) as the sources document it (csrc/sht_core.h: DftUnit; dft_wave.hip)"""
    env = env or {}
    n = 2 * L - 1
    if "PXM_DFT_NO_W" not in env and n <= 1023:
        if n <= 511:
            r0 = max(1, (1 << (n - 1).bit_length()) // 64)
            exact = n == 511 and env.get("PXM_DFT_PFA") != "0"
            return ("pair", 128 * r0, 2 if exact else 8 // r0, 512, 81920, exact)
        return ("quad", 2048, 2, 512, 81920, False)
    M = max(16, 1 << (2 * n - 2).bit_length())
    R = 8 if M <= 1024 else (4 if M == 2048 else (2 if M == 4096 else 1))
    return ("radix2", M, R, min(1024, max(64, R * M // 2)), (R * M + M // 2) * 16, False)


def model_M(case):
    """the transform length the model runs a case at (the exact-length unit is held to the model at M = 1024)"""
    _, L, env = case
    return expected_geometry(L, env)[1]


# ---- the model -----------------------------------------------------------------------------------------------------------------
def pi_ld():
    return 4 * np.arctan(LD(1))


@functools.lru_cache(maxsize=None)
def root_table(n):
    """exp(-2 pi i r / n), r < n, in long double"""
    ang = -2 * pi_ld() * np.arange(n, dtype=LD) / LD(n)
    t = np.empty(n, dtype=CLD)
    t.real, t.imag = np.cos(ang), np.sin(ang)
    return t


@functools.lru_cache(maxsize=1)
def dft_matrix_ld(n):
    """W[j, k] = exp(-2 pi i (j k mod n) / n) in long double"""
    j = np.arange(n, dtype=np.int64)
    return root_table(n)[(j[:, None] * j[None, :]) % n]


def dft_ld(x, sign=-1):
    """X[.., k] = sum_j x[.., j] exp(sign 2 pi i j k / n) in long double, term by term"""
    x = np.asarray(x)
    W = dft_matrix_ld(x.shape[-1])
    return x.astype(CLD) @ (W if sign < 0 else np.conj(W))


def _fft_pow2_rows(a, tw):
    """radix-2 transform along the FIRST axis of a [M, rows] (whole rows move: the strides stay short)"""
    if a.shape[0] == 1:
        return a
    e, o = _fft_pow2_rows(a[0::2], tw[::2]), _fft_pow2_rows(a[1::2], tw[::2]) * tw[:, None]
    return np.concatenate([e + o, e - o], axis=0)


def _fft_pow2(a, tw):
    """radix-2 transform along the last axis in a's own precision; tw = exp(-2 pi i k / M), k < M / 2"""
    M = a.shape[-1]
    rows = a.reshape(-1, M)
    out = np.empty_like(rows)
    step = max(1, (1 << 20) // M)  # (16 MB of rows at a time: the passes stay in the cache)
    for r in range(0, len(rows), step):
        out[r:r + step] = _fft_pow2_rows(np.ascontiguousarray(rows[r:r + step].T), tw).T
    return out.reshape(a.shape)


@functools.lru_cache(maxsize=None)
def bluestein_tables(n, M):
    """(chirp[n], bhat[M], tw[M/2]) in float64, each computed in long double and rounded (csrc/tables.cpp):
    c_j = exp(-i pi (j^2 mod 2n) / n), bhat = FFT_M(h) / M of h_j = conj(c_|j|) (j mod M), tw = exp(-2 pi i k / M)"""
    assert M >= 2 * n - 1 and M & (M - 1) == 0
    j = np.arange(n, dtype=np.int64)
    chirp = root_table(2 * n)[(j * j) % (2 * n)]
    h = np.zeros(M, dtype=CLD)
    h[:n] = np.conj(chirp)
    h[M - n + 1:] = np.conj(chirp[1:][::-1])
    tw = root_table(M)[:M // 2] if M > 1 else np.ones(0, dtype=CLD)
    bhat = _fft_pow2(h, tw) / LD(M)
    return chirp.astype(np.complex128), bhat.astype(np.complex128), tw.astype(np.complex128)


def bluestein64(x, M, sign=-1):
    """the DFT of the rows of x by Bluestein's algorithm in float64 at transform length M, as the units run it: chirp, M-point
    transform, product with the filter spectrum, inverse transform (by conjugation), chirp.  sign = +1: the inverse DFT by
    conjugation of input and output, as the rings -> pixels kernels do it."""
    x = np.asarray(x, dtype=np.complex128)
    n = x.shape[-1]
    chirp, bhat, tw = bluestein_tables(n, M)
    if sign > 0:
        x = np.conj(x)
    a = np.zeros(x.shape[:-1] + (M,), dtype=np.complex128)
    a[..., :n] = x * chirp
    A = _fft_pow2(a, tw) * bhat
    conv = np.conj(_fft_pow2(np.conj(A), tw))  # (1 / M is folded into bhat)
    y = conv[..., :n] * chirp
    return np.conj(y) if sign > 0 else y


def model_ratio(x, M, sign=-1, ref=None):
    """max over rows and bins of |bluestein64 - dft_ld| / (eps ||row||_2) -- rows of zeros must come out as zeros"""
    x = np.asarray(x, dtype=np.complex128)
    ref = dft_ld(x, sign) if ref is None else ref
    err = np.abs(bluestein64(x, M, sign).astype(CLD) - ref).astype(float).max(axis=-1)
    norm = np.linalg.norm(x, axis=-1)
    assert not err[norm == 0].any()
    return float((err[norm > 0] / (EPS * norm[norm > 0])).max())


def impulse_spectrum(n, p, sign=-1):
    """the DFT of the unit impulse at p (any shape of p): [.., k] = exp(sign 2 pi i p k / n), from the long-double table"""
    p = np.asarray(p, dtype=np.int64)
    t = root_table(n)[(p[..., None] * np.arange(n, dtype=np.int64)) % n]
    return t if sign < 0 else np.conj(t)


def dense(seed, *shape):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- the pixel side of the stage (tests/test_gpu_dft_px.py): masks, pixel -> data maps and integer-exact residual inputs ---------
# one case per kernel body, at the smallest L where the body's edge cases exist
PX_CASES = [("pair1", 5, {}), ("pair2", 35, {}), ("pair4", 67, {}), ("pair8", 129, {}), ("exact", 256, {}),
            ("pair8", 256, {"PXM_DFT_PFA": "0"}), ("quad", 257, {}), ("quad", 300, {}), ("radix2", 9, NO_W), ("radix2", 513, {})]
assert all(c in CASES for c in PX_CASES)
PX_EXTRA = 7  # entries of the longer data vector that no pixel maps to


@functools.lru_cache(maxsize=None)
def px_mask(L):
    """keep[t, p]: about 30 % of the pixels masked; ring 0 entirely masked (so is the image's first pixel: the entry a masked
    element re-reads is not its own), ring L - 1 entirely kept, ring 1 masked at its first pixel and kept at its last, ring 2
    the reverse"""
    n = 2 * L - 1
    keep = np.random.default_rng(9000 + L).random((L, n)) >= 0.3
    keep[0, :], keep[L - 1, :] = False, True
    keep[1, 0], keep[1, n - 1] = False, True
    keep[2, 0], keep[2, n - 1] = True, False
    keep.setflags(write=False)
    return keep


@functools.lru_cache(maxsize=None)
def px_index_map(L, extra):
    """(gidx int32 [L (2L-1)], ndata): the kept pixels onto [0, ndata) injectively through a random permutation -- not the
    monotone map of a mask --, masked pixels -1; ndata = kept pixels + extra, so `extra` entries stay unreferenced"""
    keep = px_mask(L).reshape(-1)
    ndata = int(keep.sum()) + extra
    gidx = np.full(keep.size, -1, dtype=np.int32)
    gidx[keep] = np.random.default_rng(9100 + 8 * L + extra).permutation(ndata)[:int(keep.sum())]
    gidx.setflags(write=False)
    return gidx, ndata


def px_integer_inputs(seed, C, N):
    """f [C, N], data [N], invcov [N] complex and gw [N] real with integer components: f, data in [-2^10, 2^10], invcov in
    [-2^8, 2^8] without a zero component, gw in {1, 2, 3, 5, 8}.  |f - data| <= 2^11 per component, a component of
    invcov (f - data) is a sum of two products <= 2^19, times gw <= 2^23: every intermediate is an integer below 2^24, exact in
    float64 in any order and with or without a fused multiply-add."""
    rng = np.random.default_rng(seed)
    ints = lambda lo, hi, *shape: rng.integers(lo, hi + 1, size=shape).astype(float)
    nz = lambda *shape: ints(1, 256, *shape) * rng.choice([-1.0, 1.0], size=shape)
    f = ints(-1024, 1024, C, N) + 1j * ints(-1024, 1024, C, N)
    data = ints(-1024, 1024, N) + 1j * ints(-1024, 1024, N)
    invcov = nz(N) + 1j * nz(N)
    gw = rng.choice([1.0, 2.0, 3.0, 5.0, 8.0], size=N)
    return f, data, invcov, gw


PX_CHAINS = 5


def px_integer_inputs_of(L, extra):
    """the integer inputs of the pixel-side tests at bandlimit L: in pixel space (extra None) or in the data space of
    px_index_map(L, extra)"""
    N = L * (2 * L - 1) if extra is None else px_index_map(L, extra)[1]
    return px_integer_inputs(9200 + 16 * L + (0 if extra is None else 1 + extra), PX_CHAINS, N)


@pytest.mark.parametrize("case", PX_CASES, ids=case_id)
def test_integer_residual_inputs_are_exact_in_float64(case):
    """What the bit comparison of the complex residual rests on: for the inputs of every L of the pixel-side tests, pixel
    space and both data vectors, gw (invcov (f - data)) evaluated in float64 equals the evaluation in Python integers, with
    every intermediate below 2^24 -- so no order of the products and no contraction can change a bit."""
    _, L, _ = case
    for extra in (None, 0, PX_EXTRA):
        f, data, invcov, gw = px_integer_inputs_of(L, extra)
        assert f.shape == (PX_CHAINS, L * (2 * L - 1) if extra is None else px_index_map(L, extra)[1])
        for a in (f, data, invcov):
            assert (a.real == np.rint(a.real)).all() and (a.imag == np.rint(a.imag)).all()
        assert (invcov.real != 0).all() and (invcov.imag != 0).all() and set(np.unique(gw)) <= {1.0, 2.0, 3.0, 5.0, 8.0}
        assert max(np.abs(f.real).max(), np.abs(f.imag).max(), np.abs(data.real).max(), np.abs(data.imag).max()) <= 2 ** 10
        assert max(np.abs(invcov.real).max(), np.abs(invcov.imag).max()) <= 2 ** 8
        got = gw * (invcov * (f - data))  # float64, every chain

        def evaluate(as_int):
            fr, fi, dr, di = as_int(f.real), as_int(f.imag), as_int(data.real), as_int(data.imag)
            wr, wi, g = as_int(invcov.real), as_int(invcov.imag), as_int(gw)
            rr, ri = fr - dr, fi - di
            terms = [wr * rr, wi * ri, wr * ri, wi * rr]
            want = [g * (terms[0] - terms[1]), g * (terms[2] + terms[3])]
            assert max(int(np.abs(t).max()) for t in terms + want) < 2 ** 24
            assert (as_int(got.real) == want[0]).all() and (as_int(got.imag) == want[1]).all(), (case_id(case), extra)

        evaluate(lambda a: a.astype(np.int64))  # every chain, in 64-bit integers (nothing near their range)
        evaluate(lambda a: np.array([int(v) for v in a[..., :4096].reshape(-1)], dtype=object).reshape(a[..., :4096].shape))  # Python integers


def test_pixel_masks_have_their_edge_cases():
    for _, L, _ in PX_CASES:
        keep, n = px_mask(L), 2 * L - 1
        assert not keep[0].any() and keep[L - 1].all() and (L < 35 or 0.65 <= keep.mean() <= 0.75)
        assert (keep[1, 0], keep[1, n - 1], keep[2, 0], keep[2, n - 1]) == (False, True, True, False)
        for extra in (0, PX_EXTRA):
            gidx, ndata = px_index_map(L, extra)
            live = gidx[keep.reshape(-1)]
            assert ndata == keep.sum() + extra and (gidx[~keep.reshape(-1)] == -1).all()
            assert live.min() >= 0 and live.max() < ndata and len(np.unique(live)) == len(live)  # injective, in range
            assert (np.diff(live) < 0).any()  # not the monotone map


# ---- the model against numpy and the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 17, 63, 129, 511, 1025])
def test_dft_ld_equals_numpy_fft(n):
    x = dense(n, 4, n)
    for sign, ref in ((-1, np.fft.fft(x, axis=-1)), (+1, np.fft.ifft(x, axis=-1) * n)):
        err = np.abs(dft_ld(x, sign) - ref).astype(float).max(axis=-1)
        assert (err <= 1e-13 * np.linalg.norm(x, axis=-1)).all(), (n, sign, err.max())
    if n <= 129:  # the impulses' closed form
        for sign, ref in ((-1, np.fft.fft(np.eye(n), axis=-1)), (+1, np.fft.ifft(np.eye(n), axis=-1) * n)):
            assert np.abs(impulse_spectrum(n, np.arange(n), sign) - ref).astype(float).max() <= 1e-13


@pytest.mark.parametrize("L", [1, 2, 9, 20])
def test_oracle_phi_stage_equals_dft_ld(L):
    """oracle.ssht.MWTransform: G[m, t] = sum_p f[t, p] e^{-i m phi_p} and back, order m = -(L-1) .. L-1 at index m + L - 1"""
    from oracle.ssht import MWTransform

    n, T = 2 * L - 1, MWTransform(L)
    ms = np.arange(-(L - 1), L)
    f = dense(L, L, n)
    G = T._px_to_rings(f)  # [m, t]
    ref = dft_ld(f)[:, ms % n].T
    assert (np.abs(G - ref).astype(float) <= 1e-13 * np.linalg.norm(f, axis=1)[None, :]).all()
    g = dense(L + 1, n, L)
    spec = np.zeros((L, n), dtype=complex)
    spec[:, ms % n] = g.T
    back = dft_ld(spec, +1)
    assert (np.abs(T._rings_to_px(g) - back).astype(float) <= 1e-13 * np.linalg.norm(g, axis=0)[:, None]).all()


# ---- the model's own error, pinned ------------------------------------------------------------------------------------------------
MODEL_SIZES = sorted({(2 * c[1] - 1, model_M(c)) for c in CASES})


def test_model_sizes_are_those_of_the_units():
    sizes = set(MODEL_SIZES)
    assert {(63, 128), (129, 512), (511, 1024), (513, 2048), (1023, 2048), (1025, 4096), (2047, 4096), (3, 16), (1, 128)} <= sizes
    assert len(sizes) == 20


@pytest.mark.parametrize("n,M", MODEL_SIZES, ids=[f"n{n}-M{M}" for n, M in MODEL_SIZES])
def test_model_error_is_a_few_eps_of_the_ring_norm(n, M):
    """dense normal rings (16; 4 at n = 2047, where the reference costs n^2 long-double products per ring) and EVERY unit
    impulse, both directions: the model stays within MODEL_CAP eps ||x||_2 per element"""
    x = dense(n + M, 4 if n > 1100 else 16, n)
    p = np.arange(n)
    for sign in (-1, +1):
        rd = model_ratio(x, M, sign)
        ri = model_ratio(np.eye(n), M, sign, ref=impulse_spectrum(n, p, sign))
        print(f"n={n} M={M} sign={sign:+d}: dense {rd:.2f}, impulses {ri:.2f} eps ||x||_2")
        assert rd <= MODEL_CAP and ri <= MODEL_CAP, (n, M, sign, rd, ri)
        assert n == 1 or rd > 0  # a float64 algorithm: an error of nothing means the model compared itself


def test_model_error_scales_with_each_ring():
    """rings 2^40 apart in scale: the error of each stays relative to its own norm"""
    n, M = 129, 512
    x = dense(7, 8, n) * (2.0 ** (40 * (np.arange(8) % 2)))[:, None]
    err = np.abs(bluestein64(x, M).astype(CLD) - dft_ld(x)).astype(float).max(axis=-1)
    assert (err <= MODEL_CAP * EPS * np.linalg.norm(x, axis=-1)).all()


# ---- the unit selection -------------------------------------------------------------------------------------------------------
def _env(monkeypatch, env):
    for k in ("PXM_DFT_NO_W", "PXM_DFT_PFA"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _geometry(L):
    from pxmcmc_amd import ops

    return ops.dft_geometry(L)


def test_geometry_table(monkeypatch):
    _env(monkeypatch, {})
    # pair unit: r0 = M / 128 doubles at L = 32/33, 64/65, 128/129; 8 / r0 rings per workgroup
    for L, M, rings in ((1, 128, 8), (32, 128, 8), (33, 256, 4), (64, 256, 4), (65, 512, 2), (128, 512, 2), (129, 1024, 1),
                        (255, 1024, 1)):
        assert _geometry(L) == ("pair", M, rings, 512, 81920, False), L
    assert _geometry(256) == ("pair", 1024, 2, 512, 81920, True)  # the exact-length body: a ring pair per workgroup
    # quad unit: 257 .. 512
    for L in (257, 300, 512):
        assert _geometry(L) == ("quad", 2048, 2, 512, 81920, False), L
    # radix-2 above: M = 4096, two chains and exactly the LDS of a CU, up to L = 1024
    for L in (513, 700, 1024):
        assert _geometry(L) == ("radix2", 4096, 2, 1024, 163840, False), L
    assert 163840 == LDS_MAX
    for L in range(1, 1025):
        assert _geometry(L) == expected_geometry(L), L
    _env(monkeypatch, {"PXM_DFT_PFA": "0"})
    assert _geometry(256) == ("pair", 1024, 1, 512, 81920, False)
    assert _geometry(255) == ("pair", 1024, 1, 512, 81920, False) and _geometry(257)[0] == "quad"
    _env(monkeypatch, NO_W)
    for L, M, R, threads in ((1, 16, 8, 64), (4, 16, 8, 64), (5, 32, 8, 128), (9, 64, 8, 256), (256, 1024, 8, 1024),
                             (257, 2048, 4, 1024), (512, 2048, 4, 1024), (513, 4096, 2, 1024), (1024, 4096, 2, 1024)):
        assert _geometry(L) == ("radix2", M, R, threads, (R * M + M // 2) * 16, False), L
    for L in range(1, 1025):
        g = _geometry(L)
        assert g == expected_geometry(L, NO_W) and g[4] <= LDS_MAX, L


REFUSAL = r"phi-DFT stage: no unit for bandlimit L = %d: the radix-2 unit at M = %d needs %d B of LDS per workgroup"


@pytest.mark.parametrize("env", [{}, NO_W], ids=["default", "no_w"])
def test_geometry_refuses_rings_without_lds(env, monkeypatch):
    """L >= 1025: M = 8192, one chain of 8192 points and its twiddles are 196 608 B, more than the 160 KiB of a CU"""
    import re

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError, lib

    _env(monkeypatch, env)
    for L, M, lds in ((1025, 8192, 196608), (2048, 8192, 196608), (2049, 16384, 393216)):
        with pytest.raises(PxmError, match=re.escape(REFUSAL % (L, M, lds))):
            ops.dft_geometry(L)
        out = (C.c_int * 6)()
        assert lib.pxm_host_dft_geometry(L, out) < 0
    out = (C.c_int * 6)()
    assert lib.pxm_host_dft_geometry(0, out) < 0 and lib.pxm_host_dft_geometry(8, None) < 0
    assert b"pxm_host_dft_geometry" in lib.pxm_last_error()


def _dry(L, what, chains=2):
    from pxmcmc_amd._lib import lib

    rc = lib.pxm_host_check_address_ranges(L, 2.0, 2, 0, chains, what)
    return rc, lib.pxm_last_error().decode()


@pytest.mark.parametrize("env", [{}, NO_W, {"PXM_DFT_PFA": "0"}], ids=["default", "no_w", "pfa0"])
def test_dry_run_dft_plan_creation(env, monkeypatch):
    _env(monkeypatch, env)
    for L in (1, 256, 512, 1024):
        rc, msg = _dry(L, 16, chains=5)
        assert rc == 0, (L, msg)  # (a plan without task lists: no address ranges to count)
    rc, msg = _dry(1025, 16)
    assert rc < 0 and msg.startswith(REFUSAL % (1025, 8192, 196608)), msg


def test_every_plan_constructor_inherits_the_refusal(monkeypatch):
    """the SHT plan (and with it the directional plan, whose first act is its SHT plan at L) and the wavelet plan refuse
    L = 1025 in the same words, before a ring table is built"""
    _env(monkeypatch, {})
    for what in (1, 2):
        rc, msg = _dry(1025, what, chains=1)
        assert rc < 0 and msg.startswith(REFUSAL % (1025, 8192, 196608)), (what, msg)
