"""The fused harmonic MYULA step (pxm_hwav_myula_step) on the host: HarmStepModelLD, a second and
independent statement of the step in extended precision, with a per-element error scale; the count of active items per
degree (kact) that selects the kernel instantiation; and the case list of tests/test_gpu_harmwav_step.py, whose kact
values are pinned here so that the GPU cases provably span the instantiations before a GPU is touched.  No GPU needed.

The step, per (l, m) and per coefficient e = (item, lm) (items = scaling block + every (scale j, n) with l < bl_j):

    f_lm   = sum_items w_item(l) x_item,lm
    g_lm   = k_l invcov_lm (k_l f_lm - d_lm)          k_l = 1, or the weak-lensing kernel with lm < 4 zeroed
    x'_e   = (1 - d/lam) x_e + (d/lam) soft(x_e, T_e) - d conj(w_e) g_lm + sqrt(2 d) xi_e
    preds  = k_l sum_items w_item(l) x'_item,lm

and its error scales

    S_e    = |x_e| + d |w_e| |k_l| |invcov_lm| (|k_l| sum |w| |x| + |d_lm|) + sqrt(2 d) |xi_e|
    SP_lm  = |k_l| sum_items |w| (|x'| + S)

HarmStepModelLD never calls HarmWavModel or oracle.pxmcmc_np.chain_step / soft: it builds its own weights from the
tiling arrays (fp64 inputs) in extended precision and applies the formulas above element by element.

K = 3 is reachable through the public API: J_min = J_max with N = 2 (the scaling block and the two orientations of the
one scale), and N = L = 3; the scan of test_kact_scan finds 20 such configurations and the case list holds two.

C0_MEASURED: the largest |fp64 route - LD| / (2^-52 S_e) over the whole case list and both outputs, as printed by
test_fp64_route_within_c0_of_ld (measured 2026-10-16: X' 1.542, preds 1.029).  The GPU tests bound the kernel by 4 C0_MEASURED."""
import itertools
from math import comb

import numpy as np

from oracle import pxmcmc_np, s2let
from test_harmwav_host import HarmWavModel

HAVE_LD = np.finfo(np.longdouble).eps < 1.1e-19  # x87 80-bit (eps 1.08e-19); otherwise mpmath at 40 digits, never a skip

C0_MEASURED = 1.55  # 2026-10-16: largest ratio 1.542 (X'), 1.029 (preds) over CASES x FACTORS x 2 chains, rounded up
EPS64 = 2.0 ** -52


# ---- extended-precision arithmetic: numpy long double, or object arrays of mpmath numbers -----------------------------
class _LongDouble:
    name = "longdouble"
    pi = np.longdouble("3.14159265358979323846264338327950288")

    @staticmethod
    def real(a):
        return np.asarray(a, dtype=np.float64).astype(np.longdouble)

    @staticmethod
    def cplx(a):
        return np.asarray(a).astype(np.clongdouble)

    @staticmethod
    def scalar(v):
        return np.longdouble(v)

    sqrt = staticmethod(np.sqrt)
    conj = staticmethod(np.conj)

    @staticmethod
    def abs(a):
        """|a|; complex: sqrt(re^2 + im^2) (the values of a chain are far inside the range, and hypotl is three times slower)"""
        a = np.asarray(a)
        return np.sqrt(a.real * a.real + a.imag * a.imag) if np.iscomplexobj(a) else np.abs(a)

    @staticmethod
    def f64(a):
        return np.asarray(a).astype(np.float64)

    @staticmethod
    def c128(a):
        return np.asarray(a).astype(np.complex128)


class _MpMath:
    name = "mpmath"

    def __init__(self):
        import mpmath

        self.mp = mpmath.mp.clone()
        self.mp.dps = 40
        self.pi = +self.mp.pi

    def real(self, a):
        a = np.asarray(a, dtype=np.float64)
        out = np.empty(a.shape, dtype=object)
        out.ravel()[:] = [self.mp.mpf(float(v)) for v in a.ravel()]
        return out

    def cplx(self, a):
        a = np.asarray(a, dtype=np.complex128)
        out = np.empty(a.shape, dtype=object)
        out.ravel()[:] = [self.mp.mpc(float(v.real), float(v.imag)) for v in a.ravel()]
        return out

    def scalar(self, v):
        return self.mp.mpf(v)

    def _map(self, fn, a):
        if not isinstance(a, np.ndarray):
            return fn(a)
        out = np.empty(a.shape, dtype=object)
        out.ravel()[:] = [fn(v) for v in a.ravel()]
        return out

    def sqrt(self, a):
        return self._map(self.mp.sqrt, a)

    def abs(self, a):
        return self._map(abs, a)

    def conj(self, a):
        return self._map(self.mp.conj, a)

    @staticmethod
    def f64(a):
        return np.array([float(v) for v in np.asarray(a, dtype=object).ravel()]).reshape(np.shape(a))

    @staticmethod
    def c128(a):
        return np.array([complex(v) for v in np.asarray(a, dtype=object).ravel()]).reshape(np.shape(a))


def backend(force_mpmath=False):
    return _LongDouble if HAVE_LD and not force_mpmath else _MpMath()


# ---- the model --------------------------------------------------------------------------------------------------------
class HarmStepModelLD:
    """one fused harmonic MYULA step of one chain in extended precision, with its per-element error scales"""

    def __init__(self, L, B, J_min, N=1, spin=0, tiling=None, force_mpmath=False):
        """tiling: (kappa_0 [L], kappa [J_max + 1, L]) in fp64 (oracle.s2let's by default, the library's for a device run)"""
        A = self.A = backend(force_mpmath)
        self.L, self.N, self.spin = L, N, spin
        k0, kap = s2let.tiling_axisym(B, L, J_min) if tiling is None else tiling
        self.bls = [int(b) for b in s2let.bandlimits(B, L, J_min)]
        self.el = np.repeat(np.arange(L), 2 * np.arange(L) + 1)  # degree of lm
        nu = (1.0 if N % 2 else 1j) + 0j
        ns = list(range(-(N - 1), N, 2))
        l = np.arange(L)
        g = np.minimum(N - 1, l)
        g = g - (N - 1 - g) % 2  # gamma_l: the largest g <= min(N - 1, l) of the parity of N - 1 (-1: none)
        fac = A.sqrt(A.real(2 * l + 1) / (8 * A.pi * A.pi))
        s_abs = A.real(np.zeros((N + 1, N)))  # |s_ln| = sqrt(2^-g C(g, (g - n) / 2)) at row g + 1, column of n
        for gg in range((N - 1) % 2, N, 2):
            for i, n in enumerate(ns):
                if abs(n) <= gg:
                    s_abs[gg + 1, i] = A.sqrt(A.scalar(comb(gg, (gg - n) // 2)) / A.scalar(2 ** gg))
        self.items = []  # (offset of the block, bl, n, weight per degree [bl] complex)
        off = 0
        for b, bl in enumerate(self.bls):
            for i, n in enumerate(ns) if b else ((0, 0),):
                if b:
                    w = nu * (fac[:bl] * A.real(kap[J_min + b - 1][:bl]) * s_abs[g[:bl] + 1, i])
                else:
                    w = (1.0 + 0j) * A.real(k0[:bl])
                w[: abs(spin)] = w[: abs(spin)] * 0
                self.items.append((off, bl, n, w))
                off += bl * bl
        self._wide = [(w[self.el[: bl * bl]], A.abs(w)[self.el[: bl * bl]]) for _, bl, _, w in self.items]  # per lm: w, |w|
        self.ncoefs = off
        self.nscal = self.bls[0] ** 2

    def active_counts(self):
        """per degree, the number of items with a non-zero weight: the kernel's kact is the largest (at least 1)"""
        cnt = np.zeros(self.L, dtype=int)
        for _, bl, _, w in self.items:
            cnt[:bl] += np.array([complex(v) != 0 for v in w])
        return cnt

    def kact(self):
        return max(int(self.active_counts().max()), 1)

    def zero_weight_mask(self):
        """[ncoefs] True where the element's weight is zero at its degree: prox and noise only, no gradient"""
        m = np.zeros(self.ncoefs, dtype=bool)
        for off, bl, _, w in self.items:
            m[off : off + bl * bl] = np.array([complex(v) == 0 for v in w])[self.el[: bl * bl]]
        return m

    def step(self, X, data, invcov, kernel, T, delta, lmda, xi):
        """X [ncoefs], data [L^2], invcov [L^2] real or complex, kernel None or [L^2] (lm < 4 is zeroed here), T scalar or
        [ncoefs], xi [ncoefs] real or complex, all fp64 -> (X' [ncoefs], preds [L^2], S [ncoefs], SP [L^2]) in the backend's
        precision"""
        A, L2 = self.A, self.L * self.L
        x, d, ic, w_n = A.cplx(X), A.cplx(data), A.cplx(invcov), A.cplx(xi)
        kl = A.real(np.ones(L2) if kernel is None else kernel)
        if kernel is not None:
            kl[:4] = A.scalar(0)
        Tv = A.real(np.broadcast_to(np.asarray(T, dtype=np.float64), (self.ncoefs,)))
        dl, lm_ = A.scalar(float(delta)), A.scalar(float(lmda))
        r, sq = dl / lm_, A.sqrt(2 * dl)
        ax, an = A.abs(x), A.abs(w_n)
        f, fa = A.cplx(np.zeros(L2)), A.real(np.zeros(L2))
        for (off, bl, _, _), (wl, wa) in zip(self.items, self._wide):
            n = bl * bl
            f[:n] = f[:n] + wl * x[off : off + n]
            fa[:n] = fa[:n] + wa * ax[off : off + n]
        akl = A.abs(kl)
        g = kl * (ic * (kl * f - d))
        ga = akl * A.abs(ic) * (akl * fa + A.abs(d))
        keep = ax > Tv
        soft = x * np.where(keep, (ax - Tv) / np.where(keep, ax, ax + 1), ax * 0)  # sign(x)(|x| - T) where |x| > T, else 0
        xn = (1 - r) * x + r * soft + sq * w_n
        S = ax + sq * an
        p, pa = A.cplx(np.zeros(L2)), A.real(np.zeros(L2))
        for (off, bl, _, _), (wl, wa) in zip(self.items, self._wide):
            n = bl * bl
            xo = xn[off : off + n] - dl * (A.conj(wl) * g[:n])
            so = S[off : off + n] + dl * wa * ga[:n]
            xn[off : off + n], S[off : off + n] = xo, so
            p[:n] = p[:n] + wl * xo
            pa[:n] = pa[:n] + wa * (A.abs(xo) + so)
        return xn, kl * p, S, A.abs(kl) * pa

    def ratios(self, got_X, got_P, ref):
        """(|got_X - X'| / (2^-52 S), |got_P - preds| / (2^-52 SP)) per element in fp64; a zero scale asks for an exact zero
        difference (ratio 0 if so, inf if not)"""
        A = self.A
        out = []
        for got, want, scale in ((got_X, ref[0], ref[2]), (got_P, ref[1], ref[3])):
            err, s = A.f64(A.abs(A.cplx(got) - want)), A.f64(scale) * EPS64
            out.append(np.where(s > 0, err / np.where(s > 0, s, 1), np.where(err == 0, 0.0, np.inf)))
        return out


# ---- the case list shared with tests/test_gpu_harmwav_step.py ---------------------------------------------------------
def K_of(kact):
    """the instantiation of k_hw_myula the launcher picks for a plan's kact (pxm_hwav_myula_step)"""
    return 2 if kact <= 2 else 3 if kact <= 3 else 5 if kact <= 5 else 9 if kact <= 9 else 17 if kact <= 17 else 0


# (L, B, J_min, N, spin) -> kact expected from the library's tiling
CASES = {
    (32, 2.0, 2, 1, 0): 2, (33, 1.5, 1, 1, 0): 2, (16, 2.0, 2, 1, 2): 2, (8, 2.0, 0, 1, -7): 2,
    (8, 2.0, 3, 2, 0): 3,
    (32, 2.0, 2, 2, 0): 4, (13, 1.7, 2, 2, 0): 4,
    (32, 2.0, 2, 3, 0): 6, (32, 2.0, 2, 4, 0): 8,
    (32, 2.0, 2, 5, 0): 10, (32, 2.0, 2, 8, 0): 16, (33, 1.5, 1, 5, 0): 10,
    (32, 2.0, 2, 9, 0): 18, (32, 3.0, 1, 9, 0): 18, (32, 2.0, 0, 12, 0): 24,
    (2, 2.0, 0, 1, 0): 1,   # smallest plan
    (3, 2.0, 0, 3, 0): 3,   # N = L
    (8, 2.0, 3, 8, 0): 9,   # J_min = J_max with N = L
}
FULL_SIZE = {(256, 2.0, 2, 1, 0): 2, (256, 2.0, 2, 4, 0): 8, (256, 2.0, 2, 2, 0): 4}
FACTOR_NAMES = ("wl", "vecT", "icplx", "ncplx", "n64")
# orthogonal array OA(8, 2^5) of strength 2: every pair of levels of every two factors occurs (twice) in each case
FACTORS = [(a, b, c, a ^ b, a ^ c) for a, b, c in itertools.product((0, 1), repeat=3)]


def case_id(case, kact):
    L, B, J_min, N, spin = case
    return f"K{K_of(kact)}-L{L}-B{B:g}-J{J_min}-N{N}-s{spin}"


def factor_id(fc):
    return "-".join(n + str(v) for n, v in zip(FACTOR_NAMES, fc))


def step_inputs(rng, M, C, wl, vecT, icplx):
    """(X [C, ncoefs], data, invcov, kernel or None, T) of a case, fp64; complex invcov: unequal real and imaginary parts"""
    L2 = M.L * M.L
    X = (rng.normal(size=(C, M.ncoefs)) + 1j * rng.normal(size=(C, M.ncoefs))) * 0.1
    data = rng.normal(size=L2) + 1j * rng.normal(size=L2)
    invcov = 1.0 / np.linspace(0.5, 1.5, L2) ** 2
    if icplx:
        invcov = invcov * (1.0 + 0.37j * np.cos(np.arange(L2)))
    kernel = pxmcmc_np.wl_harmonic_kernel(M.L) if wl else None
    T = np.abs(rng.normal(size=M.ncoefs)) * 0.05 if vecT else 0.05
    return X, data, invcov, kernel, T


def _library_tiling(L, B, J_min):
    from pxmcmc_amd import ops

    return ops.tiling_axisym(L, B, J_min)


# ---- kact -------------------------------------------------------------------------------------------------------------
def test_kact_table_matches_host_count(capsys):
    """the expected-variant table of the GPU cases equals the host count, on the library's tiling and on the oracle's;
    every instantiation K = 2, 3, 5, 9, 17, 0 is reached by at least two cases"""
    seen = {}
    lines = []
    for case, want in {**CASES, **FULL_SIZE}.items():
        L, B, J_min, N, spin = case
        M = HarmStepModelLD(L, B, J_min, N, spin, tiling=_library_tiling(L, B, J_min))
        assert M.kact() == want, case
        assert M.ncoefs == M.bls[0] ** 2 + N * sum(b * b for b in M.bls[1:])
        if L <= 33:
            assert HarmStepModelLD(L, B, J_min, N, spin).kact() == want, case
            seen.setdefault(K_of(want), []).append(case)
        lines.append(f"  {case_id(case, want):28s} kact = {want:2d}  zero-weight elements = {int(M.zero_weight_mask().sum())} of {M.ncoefs}")
    assert sorted(seen) == [0, 2, 3, 5, 9, 17] and all(len(v) >= 2 for v in seen.values()), seen
    with capsys.disabled():
        print("\nkact table (library tiling):\n" + "\n".join(lines))


def test_kact_scan():
    """B in {1.3, 1.5, 1.7, 2, 3}, every J_min, N = 1 .. 12, L in {8, 16, 32, 33} at spin 0: kact = 2N wherever two scales
    (or the scaling block and one scale) overlap at a degree l >= N - 1, and N + 1 where only the scaling block and the top scale are left (J_min = J_max,
    or J_max - 1 when the last scale is empty below L); so kact = 3 exists (N = 2 there) and K = 3 is reachable"""
    found = {}
    for B, L in itertools.product((1.3, 1.5, 1.7, 2.0, 3.0), (8, 16, 32, 33)):
        for J_min in range(s2let.j_max(B, L) + 1):
            til = _library_tiling(L, B, J_min)
            for N in range(1, min(12, L) + 1):
                found.setdefault(HarmStepModelLD(L, B, J_min, N, 0, tiling=til).kact(), []).append((L, B, J_min, N))
    assert len(found[3]) == 20 and all(N == 2 and J >= s2let.j_max(B, L) - 1 for L, B, J, N in found[3])
    assert {K_of(k) for k in found} == {0, 2, 3, 5, 9, 17}
    assert max(found) == 24


# ---- the model against the existing fp64 route ------------------------------------------------------------------------
def _fp64_route(H, X, data, invcov, kernel, T, delta, lmda, xi):
    meas = (lambda v: pxmcmc_np.wl_harmonic_mapping(v, kernel)) if kernel is not None else (lambda v: v)
    g = H.synthesis_adjoint(meas(invcov * (meas(H.synthesis(X)) - data)))
    Xn = pxmcmc_np.chain_step(X, pxmcmc_np.soft(X, T), g, delta, lmda, xi)
    return Xn, meas(H.synthesis(Xn))


def test_fp64_route_within_c0_of_ld(capsys):
    """HarmWavModel + oracle soft / chain_step in fp64 against HarmStepModelLD, every case and factor row, per element:
    |fp64 - LD| <= C0_MEASURED 2^-52 S_e.  Prints the measured c0 per output."""
    delta, lmda = 5e-4, 2e-3
    worst = [0.0, 0.0]
    for i, (case, _) in enumerate(CASES.items()):
        L, B, J_min, N, spin = case
        M = HarmStepModelLD(L, B, J_min, N, spin)
        H = HarmWavModel(L, B, J_min, N, spin)
        assert (M.ncoefs, M.nscal) == (H.ncoefs, H.nscal)
        for j, (wl, vecT, icplx, ncplx, _) in enumerate(FACTORS):
            rng = np.random.default_rng(100 * i + j)
            X, data, invcov, kernel, T = step_inputs(rng, M, 2, wl, vecT, icplx)
            for c in range(2):
                xi = rng.normal(size=M.ncoefs) + (1j * rng.normal(size=M.ncoefs) if ncplx else 0)
                ref = M.step(X[c], data, invcov, kernel, T, delta, lmda, xi)
                rx, rp = M.ratios(*_fp64_route(H, X[c], data, invcov, kernel, T, delta, lmda, xi), ref)
                worst = [max(worst[0], rx.max()), max(worst[1], rp.max())]
                assert rx.max() <= C0_MEASURED and rp.max() <= C0_MEASURED, (case, FACTORS[j], rx.max(), rp.max())
    with capsys.disabled():
        print(f"\nc0 measured ({backend().name}): X' {worst[0]:.3f}, preds {worst[1]:.3f}; C0_MEASURED = {C0_MEASURED}")


def test_model_catches_a_confined_error():
    """what a global max-norm misses: a dropped conjugate on the weights of one direction (N even: imaginary weights)
    moves X' by 2 delta |w g|, far under 1e-11 of the largest coefficient for some elements, and far over the bound"""
    L, B, J_min, N = 16, 2.0, 2, 2
    M = HarmStepModelLD(L, B, J_min, N)
    rng = np.random.default_rng(5)
    X, data, invcov, kernel, T = step_inputs(rng, M, 1, 0, 0, 0)
    xi = rng.normal(size=M.ncoefs)
    ref = M.step(X[0], data, invcov, kernel, T, 5e-4, 2e-3, xi)
    bad = M.A.c128(ref[0])
    off, bl, _, w = M.items[1]
    wl = np.array([complex(v) for v in w])[M.el[: bl * bl]]
    f = sum(np.pad(np.array([complex(v) for v in wi])[M.el[: b * b]] * X[0][o : o + b * b], (0, L * L - b * b)) for o, b, _, wi in M.items)
    g = invcov * (f - data)
    bad[off : off + bl * bl] += 5e-4 * (np.conj(wl) - wl) * g[: bl * bl]
    rx, _ = M.ratios(bad, M.A.c128(ref[1]), ref)
    hit = np.zeros(M.ncoefs, dtype=bool)
    hit[off : off + bl * bl] = wl != 0
    assert rx[hit].min() > 1e6 and rx[~hit].max() <= 1.0


def test_zero_weight_elements_have_no_gradient():
    """l < |n|, l < |spin| and l outside a scale's support: S_e holds no gradient term and X' is prox + noise"""
    for case in ((16, 2.0, 2, 1, 2), (8, 2.0, 3, 8, 0), (32, 2.0, 0, 12, 0)):
        M = HarmStepModelLD(*case)
        z = M.zero_weight_mask()
        assert z.any() and not z.all()
        rng = np.random.default_rng(1)
        X, data, invcov, kernel, T = step_inputs(rng, M, 1, 0, 1, 1)
        xi = rng.normal(size=M.ncoefs)
        xn, _, S, _ = M.step(X[0], data, invcov, kernel, T, 5e-4, 2e-3, xi)
        want = pxmcmc_np.chain_step(X[0], pxmcmc_np.soft(X[0], T), 0, 5e-4, 2e-3, xi)
        s0 = np.abs(X[0]) + np.sqrt(1e-3) * np.abs(xi)
        assert np.abs(M.A.f64(S)[z] - s0[z]).max() <= 1e-15 * s0.max()
        assert (M.A.f64(M.A.abs(xn - M.A.cplx(want)))[z] <= C0_MEASURED * EPS64 * s0[z]).all()
        assert (M.A.f64(S)[~z] > s0[~z]).all()


def test_mpmath_backend_agrees_with_longdouble():
    """the fallback arithmetic (mpmath, 40 digits) gives the long-double model's step to long-double rounding"""
    case = (8, 2.0, 0, 1, -7)
    Mp = HarmStepModelLD(*case, force_mpmath=True)
    assert Mp.A.name == "mpmath"
    M = HarmStepModelLD(*case)
    rng = np.random.default_rng(2)
    X, data, invcov, kernel, T = step_inputs(rng, M, 1, 1, 1, 1)
    xi = rng.normal(size=M.ncoefs) + 1j * rng.normal(size=M.ncoefs)
    a = M.step(X[0], data, invcov, kernel, T, 5e-4, 2e-3, xi)
    b = Mp.step(X[0], data, invcov, kernel, T, 5e-4, 2e-3, xi)
    assert Mp.kact() == M.kact() == 2
    for u, v, s in ((a[0], b[0], b[2]), (a[1], b[1], b[3])):
        u = Mp.A.cplx(M.A.c128(u))
        assert (Mp.A.f64(Mp.A.abs(u - v)) <= 4 * EPS64 * Mp.A.f64(s)).all()
    for u, v in ((a[2], b[2]), (a[3], b[3])):
        assert np.allclose(M.A.f64(u), Mp.A.f64(v), rtol=1e-14, atol=0)
