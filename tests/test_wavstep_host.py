"""Host model of ONE fused wavelet step (WavPlan.ring_step / image_step / gradg_step: the rings -> pixels -> X' -> rings kernels
of csrc/dft_wave.hip, csrc/dft_pfa.h and csrc/dft.hip, whose shared epilogue is csrc/update.h + csrc/elem.h): the
extended-precision yardstick that tests/test_gpu_wavstep.py holds every noise and update branch of the epilogue to,
element by element.  No GPU needed.

The step, per slot c and element e of the [scaling | j = J_min .. J_max] coefficient vector (r = d/l):

    X' = ((1 - r) X + r soft(X, T) - d g) + sqrt(2 d) w                 (association order of csrc/elem.h chain_step_real)

in the three interpretations of the complex128 slot (csrc/update.h):

    MODE_REAL_NOISE (0)  complex state, complex soft threshold z (|z| - T)/|z|, the deviate in the real part only
    MODE_CPLX_NOISE (1)  complex state, complex soft threshold, a deviate in both parts
    MODE_REAL_PAIRS (2)  two REAL chains per slot (chain 2c in .real, chain 2c + 1 in .imag): a real soft threshold and one
                         deviate per component

The gradient g is an INPUT of the model (the GPU test passes the device's own unfused gradient); so are the deviates w.
``deviates`` says which deviate each (slot, component) must receive from the Philox stream of oracle/philox.py, keyed
(seed, GLOBAL chain id, element index in the whole coefficient vector, it + it_dev):

    MODE_CPLX_NOISE   slot c: the pair (z0, z1) of key (seed, chain0 + c)
    MODE_REAL_NOISE   slot c: chain k = chain0 + c takes member k & 1 of the pair keyed (seed + tweak, k >> 1); .imag gets 0
    MODE_REAL_PAIRS   component comp of slot c: chain k = chain0 + 2 c + comp, member k & 1 of the pair keyed (seed + tweak, k >> 1)
                      (even chain0: one pair serves the slot; odd chain0: the slot straddles two pairs, z1 of the first and z0
                      of the second)

The bound.  Per element (pair mode: per component, each component being one real chain's element; complex modes: moduli)

    |got - model| <= d E_g + sqrt(2 d) E_w max(1, |w|) + K eps (|(1 - r) X| + |r soft| + |d g| + |sqrt(2 d) w|)

E_g = 1e-11 max|g| is the documented agreement of the transforms, E_w = 1e-13 the documented agreement
of the fp64 stream with its numpy restatement (0 for injected noise and for the f32-unit stream, whose model deviate is
ops.randn's own draw), eps = 2^-52.

K = 11, by counting the roundings on the longest path from the inputs to X' (each rounding is at most 2^-53 relative to its
own result, and every result below is at most the sum S of the four moduli of the bound):

    soft_cplx        z.y z.y (1), fma(z.x, z.x, .) (2), sqrt (3), a - T (4), (a - T) / a (5), z.x s (6)
    chain_step_real  r = d / l (7), r px (8), (1 - r) X + r px (9; 1 - r and its product with X lie on the shorter branch:
                     3 roundings), . - d g (10; d g itself: 1 rounding on its branch), sqrt(2 d) w: 2 d exact, sqrt and the
                     product (2 roundings on its branch), the last sum (11)

(a fused multiply-add only removes roundings).  K eps = 22 x 2^-53: twice the first-order count.  The factor covers the one
place where a counted rounding is NOT relative to its result: the three roundings of a = |z| are relative to a, and reach the
prox as 2 x 2^-53 r a (a / (a - T) times larger than counted); with r <= 1/2 that is at most 2^-52 |(1 - r) X|.  The same holds
where the kernel and the model take different sides of a <= T: the prox is continuous there.  It needs d <= l / 2
(``step_bound`` asserts it), the range the samplers keep (tune_delta).  Elements of the complex modes with |X| within
EXCLUDE_ULPS ulp of T are left out nevertheless (``excluded``): the documented cancellation zone; the share may not exceed
EXCLUDE_CAP = 1e-4 and is zero for the inputs of ``step_inputs``.  In pair mode nothing is excluded (the real soft threshold
compares exactly and subtracts once).

Measured on the host (test_fp64_numpy_route_is_inside_the_bound): the fp64 numpy route (oracle.pxmcmc_np soft + chain_step)
against the model with E_g = E_w = 0 reaches 0.10 / 0.10 / 0.12 of the bound (real noise / complex noise / pairs)."""
import functools

import numpy as np
import pytest

from oracle import philox, pxmcmc_np, s2let

LD, CLD = np.longdouble, np.clongdouble
HAVE_LD = np.finfo(np.longdouble).eps < 1.1e-19  # x87 80-bit extended precision
EPS = 2.0 ** -52
K_ROUNDINGS = 11
E_G_REL = 1e-11   # transforms against the oracle, of the data scale
E_W_F64 = 1e-13   # fp64 device stream against oracle/philox.py
EXCLUDE_ULPS = 4
EXCLUDE_CAP = 1e-4
MODE_REAL_NOISE, MODE_CPLX_NOISE, MODE_REAL_PAIRS = 0, 1, 2
MODES = (MODE_REAL_NOISE, MODE_CPLX_NOISE, MODE_REAL_PAIRS)
MODE_IDS = {MODE_REAL_NOISE: "realnoise", MODE_CPLX_NOISE: "cplxnoise", MODE_REAL_PAIRS: "pairs"}
M64 = (1 << 64) - 1


# ---- layout --------------------------------------------------------------------------------------------------------------
def block_layout(L, B, J_min):
    """[(offset, bandlimit)] of the blocks [scaling | j = J_min .. J_max]; block = MW grid bl x (2 bl - 1), ring-major"""
    out, off = [], 0
    for bl in s2let.bandlimits(B, L, J_min):
        out.append((off, bl))
        off += bl * (2 * bl - 1)
    return out, off


def ring_length(L, B, J_min):
    """ring length 2 bl - 1 of the block each element lies in: int64 [ncoefs]"""
    blocks, n = block_layout(L, B, J_min)
    out = np.zeros(n, dtype=np.int64)
    for off, bl in blocks:
        out[off: off + bl * (2 * bl - 1)] = 2 * bl - 1
    return out


# ---- the deviates ----------------------------------------------------------------------------------------------------------
def _pair_member(seed, k, e, t, bits):
    """deviate of REAL chain k: member k & 1 of the pair keyed (seed + tweak, k >> 1)"""
    z = philox.normal_pairs((int(seed) + philox.REAL_TWEAK) & M64, int(k) >> 1, e, t, bits)
    return z[int(k) & 1]


def deviates(mode, seed, chain0, slots, elements, it, it_dev=0, bits=64):
    """complex [slots, len(elements)]: what component 0 (.real) and component 1 (.imag) of every slot must receive"""
    e = np.asarray(elements, dtype=np.uint64)
    t = (int(it) + int(it_dev)) & M64
    out = np.zeros((slots, e.size), dtype=np.complex128)
    for c in range(slots):
        if mode == MODE_CPLX_NOISE:
            z0, z1 = philox.normal_pairs(int(seed), int(chain0) + c, e, t, bits)
            out[c] = z0 + 1j * z1
        elif mode == MODE_REAL_NOISE:
            out[c] = _pair_member(seed, int(chain0) + c, e, t, bits)
        else:
            out[c] = _pair_member(seed, int(chain0) + 2 * c, e, t, bits) + 1j * _pair_member(seed, int(chain0) + 2 * c + 1, e, t, bits)
    return out


# ---- extended-precision model ------------------------------------------------------------------------------------------------
def _Tld(T, shape):
    return np.broadcast_to(np.asarray(T, dtype=np.float64).astype(LD), shape)


def _soft_real_ext(x, T):
    a = np.abs(x)
    return np.where(a > T, np.sign(x) * (a - T), LD(0))


def soft_model(X, T, mode):
    """prox of the step in extended precision: clongdouble, shape of X"""
    x = np.asarray(X).astype(CLD)
    T = _Tld(T, x.shape)
    if mode == MODE_REAL_PAIRS:
        return _soft_real_ext(x.real, T) + 1j * _soft_real_ext(x.imag, T)
    a = np.sqrt(x.real * x.real + x.imag * x.imag)
    s = np.where(a > T, (a - T) / np.where(a > 0, a, LD(1)), LD(0))
    return x * s


def noise_model(w, mode):
    """the deviates as the step adds them: real noise on a complex state has no imaginary part"""
    w = np.asarray(w).astype(CLD)
    return w.real + 0j if mode == MODE_REAL_NOISE else w


def step_terms(X, T, delta, lmda, g, w, mode):
    """the four addends (1 - r) X, r soft, d g, sqrt(2 d) w in extended precision"""
    x, g_ = np.asarray(X).astype(CLD), np.asarray(g).astype(CLD)
    d, l = LD(np.float64(delta)), LD(np.float64(lmda))
    r = d / l
    return (1 - r) * x, r * soft_model(X, T, mode), d * g_, np.sqrt(2 * d) * noise_model(w, mode)


def step_model(X, T, delta, lmda, g, w, mode):
    """X' of one fused wavelet step, clongdouble [slots, N].  X, g: complex [slots, N]; T: [N] or scalar; w: complex [slots, N]
    (pair mode: component deviates in .real / .imag)"""
    a, b, c, n = step_terms(X, T, delta, lmda, g, w, mode)
    return ((a + b) - c) + n


def _mag(z, mode):
    """moduli the bound adds: per component in pair mode (returned as complex: .real / .imag), the modulus otherwise"""
    if mode == MODE_REAL_PAIRS:
        return np.abs(z.real).astype(np.float64) + 1j * np.abs(z.imag).astype(np.float64)
    return np.sqrt(z.real * z.real + z.imag * z.imag).astype(np.float64)


def step_bound(X, T, delta, lmda, g, w, mode, E_g, E_w):
    """the per-element bound of the module docstring: float [slots, N], or complex (bound of .real, bound of .imag) in pair mode"""
    assert 0 < delta <= lmda / 2, "the bound is derived for d <= l / 2"
    a, b, c, n = step_terms(X, T, delta, lmda, g, w, mode)
    S = _mag(a, mode) + _mag(b, mode) + _mag(c, mode) + _mag(n, mode)
    wm = _mag(noise_model(w, mode), mode)
    if mode == MODE_REAL_PAIRS:
        wmax = np.maximum(1.0, wm.real) + 1j * np.maximum(1.0, wm.imag)
        flat = delta * E_g * (1 + 1j)
    else:
        wmax, flat = np.maximum(1.0, wm), delta * E_g
    return flat + np.sqrt(2 * delta) * E_w * wmax + K_ROUNDINGS * EPS * S


def excluded(X, T, mode):
    """bool [slots, N]: complex-mode elements with |X| within EXCLUDE_ULPS ulp of T (soft-threshold cancellation)"""
    X = np.asarray(X)
    if mode == MODE_REAL_PAIRS:
        return np.zeros(X.shape, dtype=bool)
    a = np.abs(X)
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), X.shape)
    return np.abs(a - T) <= EXCLUDE_ULPS * EPS * np.maximum(a, T)


def ratios(got, model, bound, mode, skip=None):
    """|got - model| / bound per element (pair mode: the larger of the two components); excluded elements give 0"""
    d = np.asarray(got).astype(CLD) - model
    if mode == MODE_REAL_PAIRS:
        q = np.maximum(np.abs(d.real).astype(np.float64) / bound.real, np.abs(d.imag).astype(np.float64) / bound.imag)
    else:
        q = _mag(d, mode) / bound
    return q if skip is None else np.where(skip, 0.0, q)


# ---- input builders (shared with the GPU tests) --------------------------------------------------------------------------------
X_SCALE, T_SCALAR = 1e-2, 1e-4
G_MAX = 20.0  # largest |g| of the GPU cases (asserted there; measured 0.6 ... 11.5): the scale at which the rejections are shown


def thresholds(rng, N):
    """vector T: around T_SCALAR, zero (no shrink) at ::97, above every |x| (prox = 0) at 5::89"""
    T = T_SCALAR * (0.5 + rng.random(N))
    T[::97] = 0.0
    T[5::89] = 1.0
    return T


def states(rng, slots, N, mode, T):
    """X ~ X_SCALE N(0, 1) in both parts; pair mode: components exactly at +-T (prox exactly 0) at 3::101"""
    X = X_SCALE * (rng.normal(size=(slots, N)) + 1j * rng.normal(size=(slots, N)))
    if mode == MODE_REAL_PAIRS:
        Te = np.broadcast_to(np.asarray(T, dtype=np.float64), (N,))[3::101]
        X[:, 3::101] = Te * (1 - 2 * (np.arange(Te.size) % 2)) - 1j * Te
    return X


def injected(rng, slots, N, mode):
    """complex [slots, N] carrier of the injected deviates (what ``step_model`` takes) for the mode"""
    w = rng.normal(size=(slots, N)) + 1j * rng.normal(size=(slots, N))
    return w.real + 0j if mode == MODE_REAL_NOISE else w


def step_inputs(rng, slots, N, mode, vecT):
    T = thresholds(rng, N) if vecT else T_SCALAR
    X = states(rng, slots, N, mode, T)
    g = 4.0 * (rng.normal(size=(slots, N)) + 1j * rng.normal(size=(slots, N)))
    return X, T, g, injected(rng, slots, N, mode)


DELTA, LMDA = 1e-4, 2e-3
HOST_LAYOUT = (16, 2.0, 2)  # bandlimits 4, 8, 16, 16: 1140 coefficients


# ---- fp64 numpy route ------------------------------------------------------------------------------------------------------------
def step_np(X, T, delta, lmda, g, w, mode):
    """the step through oracle.pxmcmc_np (soft, chain_step) in fp64; pair mode: the two real chains of a slot separately"""
    if mode == MODE_REAL_PAIRS:
        parts = [pxmcmc_np.chain_step(x, pxmcmc_np.soft(x, T), g_, delta, lmda, w_)
                 for x, g_, w_ in ((X.real, g.real, w.real), (X.imag, g.imag, w.imag))]
        return parts[0] + 1j * parts[1]
    w = w.real + 0j if mode == MODE_REAL_NOISE else w
    return pxmcmc_np.chain_step(X, pxmcmc_np.soft(X, T), g, delta, lmda, w)


# ---- tests -----------------------------------------------------------------------------------------------------------------------
def test_extended_precision_is_available():
    assert HAVE_LD, "the model needs numpy's 80-bit long double"


def test_layout_against_the_oracle():
    for L, B, J_min in ((16, 2.0, 2), (128, 2.0, 2), (256, 2.0, 2), (260, 2.0, 2)):
        blocks, n = block_layout(L, B, J_min)
        T = s2let.WaveletTransform(L, B, J_min) if L <= 16 else None
        if T is not None:
            assert n == T.ncoefs and blocks[1][0] == T.nscal
        rl = ring_length(L, B, J_min)
        assert rl[0] == 2 * blocks[0][1] - 1 and rl[-1] == 2 * L - 1 and rl.size == n
    assert [bl for _, bl in block_layout(128, 2.0, 2)[0]] == [4, 8, 16, 32, 64, 128, 128]
    assert [bl for _, bl in block_layout(256, 2.0, 2)[0]][-2:] == [256, 256]  # the two 511-point scales


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS.get)
@pytest.mark.parametrize("vecT", [1, 0], ids=["Tvec", "Tscalar"])
def test_fp64_numpy_route_is_inside_the_bound(mode, vecT):
    """the model against oracle.pxmcmc_np.chain_step and soft in every mode, under the bound with E_g = E_w = 0, and the
    inputs of the GPU test leave nothing out"""
    rng = np.random.default_rng(10 + 2 * mode + vecT)
    N = block_layout(*HOST_LAYOUT)[1]
    X, T, g, w = step_inputs(rng, 3, N, mode, vecT)
    model = step_model(X, T, DELTA, LMDA, g, w, mode)
    skip = excluded(X, T, mode)
    assert skip.mean() <= EXCLUDE_CAP and not skip.any()
    q = ratios(step_np(X, T, DELTA, LMDA, g, w, mode), model, step_bound(X, T, DELTA, LMDA, g, w, mode, 0.0, 0.0), mode, skip)
    print(f"fp64 numpy route / bound: {q.max():.3f}")
    assert q.max() <= 1.0
    p = soft_model(X, T, mode)
    zero = (p.real == 0) & (p.imag == 0) if mode != MODE_REAL_PAIRS else (p.real == 0)
    assert not zero.all() and (zero.any() or not (vecT or mode == MODE_REAL_PAIRS))  # both sides of the threshold are met
    if mode == MODE_REAL_PAIRS:
        assert np.all(p[:, 3::101] == 0) and np.all(np.abs(X[:, 3::101].real) == np.broadcast_to(T, (N,))[3::101])
    elif mode == MODE_REAL_NOISE:  # real noise on a complex state: nothing reaches the imaginary part
        junk = w + 1j * rng.normal(size=w.shape)
        assert np.array_equal(step_model(X, T, DELTA, LMDA, g, junk, mode), model)


@pytest.mark.parametrize("chain0", [6, 7], ids=["even", "odd"])
@pytest.mark.parametrize("bits", [64, 32])
def test_deviate_assignment_against_the_stream_oracle(chain0, bits):
    """``deviates`` against oracle/philox.py's own chain-level functions for an even and an odd first chain"""
    seed, it, it_dev, slots, n = 11, 5, 3, 3, 300
    e = np.arange(n)
    w = deviates(MODE_REAL_PAIRS, seed, chain0, slots, e, it, it_dev, bits)
    for c in range(slots):
        assert np.array_equal(w[c].real, philox.randn_real(n, seed, chain0 + 2 * c, it + it_dev, bits))
        assert np.array_equal(w[c].imag, philox.randn_real(n, seed, chain0 + 2 * c + 1, it + it_dev, bits))
    z0, z1 = philox.normal_pairs((seed + philox.REAL_TWEAK) & M64, (chain0 + 1) >> 1, e.astype(np.uint64), it + it_dev, bits)
    if chain0 & 1:  # the slot straddles two pairs: z1 of pair (chain0 >> 1), z0 of the next
        assert np.array_equal(w[0].imag, z0) and not np.array_equal(w[0].real, z1)
    else:           # one pair serves the slot
        assert np.array_equal(w[0].real, z0) and np.array_equal(w[0].imag, z1)
    w = deviates(MODE_REAL_NOISE, seed, chain0, slots, e, it, it_dev, bits)
    for c in range(slots):
        assert np.array_equal(w[c].real, philox.randn_real(n, seed, chain0 + c, it + it_dev, bits)) and np.all(w[c].imag == 0)
    w = deviates(MODE_CPLX_NOISE, seed, chain0, slots, e, it, it_dev, bits)
    for c in range(slots):
        assert np.array_equal(w[c], philox.randn_complex(n, seed, chain0 + c, it + it_dev, bits))
    # a sub-range of elements is the same stream: the counter is the element's index in the whole vector
    sub = deviates(MODE_REAL_PAIRS, seed, chain0, slots, e[100:], it, it_dev, bits)
    assert np.array_equal(sub, deviates(MODE_REAL_PAIRS, seed, chain0, slots, e, it, it_dev, bits)[:, 100:])


@functools.lru_cache(maxsize=None)
def _rejection_case(mode, chain0):
    rng = np.random.default_rng(77 + mode)
    N = block_layout(*HOST_LAYOUT)[1]
    X, T, g, _ = step_inputs(rng, 2, N, mode, 1)
    seed, it, it_dev = 11, 5, 3
    w = deviates(mode, seed, chain0, 2, np.arange(N), it, it_dev)
    assert np.abs(g).max() <= G_MAX
    E_g = E_G_REL * G_MAX  # (not max|g| of this draw: the loosest bound any GPU case is given)
    return dict(N=N, X=X, T=T, g=g, w=w, seed=seed, it=it, it_dev=it_dev, E_g=E_g,
                bound=step_bound(X, T, DELTA, LMDA, g, w, mode, E_g, E_W_F64), skip=excluded(X, T, mode))


def _chain_ids(mode, chain0, slots):
    """global chain ids [slots][components that draw from the real stream]"""
    if mode == MODE_REAL_PAIRS:
        return [[chain0 + 2 * c, chain0 + 2 * c + 1] for c in range(slots)]
    return [[chain0 + c] for c in range(slots)]


def _from_real_stream(mode, ids, member):
    """complex carrier [slots, N] with component deviates member(k) for the chain ids of _chain_ids"""
    rows = [[member(k) for k in slot] for slot in ids]
    return np.stack([r[0] + (1j * r[1] if len(r) == 2 else 0j) for r in rows])


def _wrong_outputs(mode, chain0, k):
    """name -> X' of a model with one deliberate error.  On the real stream (real noise, pairs) chain k ^ 1 IS the other
    member of chain k's pair, so the first two errors give the same deviates there, each stated in its own terms; with complex
    noise they differ (another key / the two parts exchanged)"""
    X, T, g, w, N, seed, it, it_dev = (k[n] for n in ("X", "T", "g", "w", "N", "seed", "it", "it_dev"))
    e = np.arange(N, dtype=np.uint64)
    t = it + it_dev
    step = lambda w_: step_model(X, T, DELTA, LMDA, g, w_, mode)  # noqa: E731
    out = {}
    if mode == MODE_CPLX_NOISE:
        nb = [philox.normal_pairs(seed, (chain0 + c) ^ 1, e, t, 64) for c in range(2)]
        out["neighbour_chain"] = step(np.stack([z0 + 1j * z1 for z0, z1 in nb]))
        out["z0_z1_swapped"] = step(w.imag + 1j * w.real)
    else:
        ids = _chain_ids(mode, chain0, 2)
        out["neighbour_chain"] = step(_from_real_stream(mode, ids, lambda c: _pair_member(seed, c ^ 1, e, t, 64)))
        other = lambda c: philox.normal_pairs((seed + philox.REAL_TWEAK) & M64, c >> 1, e, t, 64)[(c & 1) ^ 1]  # noqa: E731
        out["z0_z1_swapped"] = step(_from_real_stream(mode, ids, other))
    ring = ring_length(*HOST_LAYOUT).astype(np.uint64)
    out["element_off_by_one_ring"] = step(deviates(mode, seed, chain0, 2, e + ring, it, it_dev))
    out["it_without_it_dev"] = step(deviates(mode, seed, chain0, 2, e, it, 0))
    a, b, c, n = step_terms(X, T, DELTA, LMDA, g, w, mode)
    r = LD(DELTA) / LD(LMDA)
    r_bad = r * (1 + LD(1e-9))  # d / l wrong by 1e-9 relative, d and l themselves right
    out["ratio_off_by_1e-9"] = (((1 - r_bad) * np.asarray(X).astype(CLD) + b * (r_bad / r)) - c) + n
    s = np.sqrt(2 * LD(DELTA))
    out["sqrt2d_float32"] = ((a + b) - c) + n * (LD(np.float32(np.float64(s))) / s)  # sqrt(2 d) rounded to float32
    return out


ERRORS = ["neighbour_chain", "z0_z1_swapped", "element_off_by_one_ring", "it_without_it_dev", "ratio_off_by_1e-9", "sqrt2d_float32",
          "T_vector_for_T_scalar"]


@pytest.mark.parametrize("error", ERRORS)
def test_bound_rejects_deliberate_errors(error):
    """the bound of the GPU test (E_w = 1e-13, E_g = 1e-11 G_MAX: the gradient scale no GPU case exceeds) passes the fp64 route and
    fails each deliberate error, in every mode and for an even and an odd first chain.  On the real stream (real noise, pairs) the
    first two errors are one and the same set of deviates; they are two checks with complex noise only.  ``ratio_off_by_1e-9`` is
    seen only at the elements whose T lies above |x| (vector T, 5::89): 1e-9 r |x| there, 1e-9 r T = 5e-15 elsewhere, under d E_g"""
    for mode in MODES:
        for chain0 in (6, 7):
            k = _rejection_case(mode, chain0)
            X, T, g, w = k["X"], k["T"], k["g"], k["w"]
            model = step_model(X, T, DELTA, LMDA, g, w, mode)
            good = ratios(step_np(X, T, DELTA, LMDA, g, w, mode), model, k["bound"], mode, k["skip"])
            assert good.max() <= 1.0
            if error == "T_vector_for_T_scalar":  # the scalar is meant; the kernel read the vector
                model = step_model(X, T_SCALAR, DELTA, LMDA, g, w, mode)
                bound = step_bound(X, T_SCALAR, DELTA, LMDA, g, w, mode, k["E_g"], E_W_F64)
                bad = ratios(step_model(X, T, DELTA, LMDA, g, w, mode), model, bound, mode, excluded(X, T_SCALAR, mode))
            else:
                bad = ratios(_wrong_outputs(mode, chain0, k)[error], model, k["bound"], mode, k["skip"])
            assert bad.max() > 1.0, (error, MODE_IDS[mode], chain0, bad.max())
            if error == "ratio_off_by_1e-9":
                assert bad.max() > 10.0 and not (bad > 1.0)[:, np.broadcast_to(T, (k["N"],)) < 1.0].any()
            if error in ("neighbour_chain", "z0_z1_swapped", "element_off_by_one_ring", "it_without_it_dev", "sqrt2d_float32"):
                assert np.mean(bad > 1.0) > 0.9  # a wrong deviate is wrong everywhere
