"""The tables and the stage statements of the orientation layer on the host ("Error model and tests of the
orientation stages"): the directionality component, the weight rows of the harmonic split / merge and the phases of the
gamma stage, as the library exports them, against long-double statements built from exact integers; and the float64 numpy
statement of each stage against its long-double statement at the bounds the GPU tests hold the kernels to.  No GPU needed.

u = 2^-53 is the unit roundoff of float64 and gamma(k) = k u / (1 - k u) (Higham).  The long-double statements
(``*_ld``), ``worst_ratio`` and ``Stages`` are shared with tests/test_gpu_dirwav_stages.py."""
from math import comb

import numpy as np
import pytest

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "these tests need an extended-precision long double"
U = 2.0 ** -53
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)  # pi to 2^-64: its float64 value plus the remainder

SHAPES = [(16, 2.0, 1), (16, 2.0, 0), (13, 1.5, 1), (33, 2.0, 2)]  # (L, B, J_min) of the stage tests
NS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12]  # every unrolled instantiation of the gamma kernels and the generic one
TABLE_NS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 33, 64]


def gam(k):
    return k * U / (1 - k * U)


def ld_int(c):
    """the integer 0 <= c < 2^64 as a long double, exactly"""
    assert 0 <= c < 1 << 64
    hi, lo = divmod(int(c), 1 << 32)
    return LD(hi) * LD(2.0 ** 32) + LD(lo)


def gamma_l(N, el):
    g = min(N - 1, el)
    return g - 1 if (N - 1 - g) % 2 else g


def s_exact(L, N):
    """|s_lm| [L*L] in long double: sqrt(C(g, (g - m) / 2) / 2^g) from the exact binomial (one division by a power of two
    and one square root, both within 2^-64)"""
    s = np.zeros(L * L, dtype=LD)
    for el in range(L):
        g = gamma_l(N, el)
        for m in range(-g, g + 1, 2):
            s[el * el + el + m] = np.sqrt(np.ldexp(ld_int(comb(g, (g - m) // 2)), -g))
    return s


def _rel_ulps(got, ref):
    """max |got - ref| / |ref| in units of 2^-52 over the non-zero entries of ref; the zero patterns must agree"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(got == 0, ref == 0)
    nz = ref != 0
    if not nz.any():
        return 0.0
    return float((np.abs(LD(got[nz]) - ref[nz]) / np.abs(ref[nz])).max() / LD(2.0 ** -52))


# ---- the tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", TABLE_NS)
def test_s_ln_within_one_ulp(N):
    """the library's directionality component at L = N (every g = gamma_l up to N - 1) within 1 ulp = 2^-52 relative of
    the exact binomial, on the component nu selects; the other component is exactly zero"""
    from pxmcmc_amd import ops

    s, ref = ops.dir_component(N, N), s_exact(N, N)
    mag, other = (s.real, s.imag) if N % 2 else (s.imag, s.real)
    assert np.all(other == 0)
    r = _rel_ulps(mag, ref)
    print(f"DW-RATIO s_ln N={N} L={N} ratio={r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("N", TABLE_NS)
def test_python_dir_component_within_one_ulp(N):
    from pxmcmc_amd import utils

    s, ref = utils.dir_component(N, N), s_exact(N, N)
    mag, other = (s.real, s.imag) if N % 2 else (s.imag, s.real)
    assert np.all(other == 0)
    assert _rel_ulps(mag, ref) <= 1.0


def _row_refs(L, B, J_min, N, spin, harmonic, rows):
    """the long-double rows (|wa|-side magnitude with sign, [rows, L]) of the analysis and synthesis weights and the
    roundoff counts (ka, ks) of the library's expression"""
    from pxmcmc_amd import ops

    k0, kap = ops.tiling_axisym(L, B, J_min)
    s = s_exact(L, N)
    el = np.arange(L)
    if harmonic:
        fa = np.sqrt(LD(8) * PI_LD * PI_LD / (2 * el + 1).astype(LD))
        fs = np.sqrt((2 * el + 1).astype(LD) / (LD(8) * PI_LD * PI_LD))
    else:
        fa = np.full(L, LD(1) / np.sqrt(LD(2) * PI_LD))
        fs = np.full(L, np.sqrt(LD(2) * PI_LD))
    ra, rs = np.zeros((len(rows), L), dtype=LD), np.zeros((len(rows), L), dtype=LD)
    for i, (b, n, bl) in enumerate(rows):
        if b == 0:
            ra[i] = rs[i] = LD(k0)
        else:
            sln = np.array([s[l * l + l + n] if abs(n) <= l else LD(0) for l in range(L)], dtype=LD)
            sgn = -1.0 if (not harmonic and n % 2) else 1.0
            ra[i] = sgn * LD(kap[J_min + b - 1]) * sln * fa
            rs[i] = sgn * LD(kap[J_min + b - 1]) * sln * fs
        ra[i, : abs(spin)] = 0
        rs[i, : abs(spin)] = 0
    return ra, rs


ROW_CASES = ([(L, B, J, N, 0, h) for (L, B, J) in SHAPES for N in (1, 2, 3, 4, 5, 9, 12, L) for h in (False, True)]
             + [(16, 2.0, 1, 1, 2, True), (13, 1.5, 1, 1, -3, True), (64, 2.0, 2, 64, 0, False), (64, 2.0, 2, 64, 0, True)])


@pytest.mark.parametrize("L,B,J_min,N,spin,harmonic", ROW_CASES)
def test_weight_rows_match_long_double(L, B, J_min, N, spin, harmonic):
    """every entry of the exported wa / ws rows against kappa (the library's, taken as given) * exact s_ln * the
    long-double constant.  Roundings of the expression as written, in units of u = 2^-53, with pi_d = M_PI (|pi_d - pi| <
    0.4 u pi, counted as u):

      pixel     wa = ((sgn kappa) s) fa, fa = 1 / sqrt(2 pi_d): s_ln 2 u (1 ulp), the two products 1 u each,
                fa: sqrt halves the u of pi_d and rounds (1.5 u), the division rounds (1 u)              -> 6.5 u, gamma(7)
                ws = ((sgn kappa) s) fs, fs = sqrt(2 pi_d): 2 + 1 + 1 + 1.5                                -> 5.5 u, gamma(6)
      harmonic  fa = sqrt(8 pi_d pi_d / (2l+1)): pi_d twice (2 u), the product pi_d pi_d and the division (1 u each; 8 pi_d
                and 2l+1 are exact), halved by the sqrt (2 u) plus its rounding (1 u) = 3 u; with 2 + 1 + 1  -> 7 u, gamma(7)
                fs = sqrt((2l+1) / (8 pi_d pi_d)): the same count                                          -> 7 u, gamma(7)

    The scaling rows are kappa_0 itself, the rows l < |spin| exact zeros, and the rows come in plan order with the pairs
    |n| >= bl skipped in pixel space only."""
    from pxmcmc_amd import ops

    wa, ws, rows = ops.harm_weights(L, B, J_min, N, spin, harmonic)
    bls = ops.wav_bandlimits(L, B, J_min)
    want = [(0, 0, bls[0])] + [(b, n, bls[b]) for b in range(1, len(bls)) for n in range(-(N - 1), N, 2)
                                if harmonic or abs(n) < bls[b]]
    assert [tuple(int(v) for v in r) for r in rows] == want
    ra, rs = _row_refs(L, B, J_min, N, spin, harmonic, want)
    ka, ks = (7, 7) if harmonic else (7, 6)
    k0, _ = ops.tiling_axisym(L, B, J_min)
    worst = 0.0
    for i, (b, n, bl) in enumerate(want):
        if b == 0:
            expect = k0.copy()
            expect[: abs(spin)] = 0
            assert np.array_equal(wa[i], expect.astype(complex)) and np.array_equal(ws[i], expect.astype(complex))
            continue
        if N % 2:  # nu = 1: real rows
            ga, gs = wa[i].real, ws[i].real
            assert np.all(wa[i].imag == 0) and np.all(ws[i].imag == 0)
        else:  # nu = i: wa = conj(.) = -i |.|, ws = +i |.|
            ga, gs = -wa[i].imag, ws[i].imag
            assert np.all(wa[i].real == 0) and np.all(ws[i].real == 0)
        for got, ref, k in ((ga, ra[i], ka), (gs, rs[i], ks)):
            assert np.array_equal(got == 0, ref == 0), (b, n)
            err, bound = np.abs(LD(got) - ref), gam(k) * np.abs(ref)
            assert np.all(err <= bound), (b, n, float((err[ref != 0] / bound[ref != 0]).max()))
            if (ref != 0).any():
                worst = max(worst, float((err[ref != 0] / bound[ref != 0]).max()))
    print(f"DW-RATIO rows L={L} B={B} J_min={J_min} N={N} spin={spin} harmonic={int(harmonic)} ratio={worst:.3f}")


@pytest.mark.parametrize("N", TABLE_NS + [100, 511])
def test_phases_match_long_double(N):
    """ph[q][k] against exp(2 pi i (n_k q mod (2N-1)) / (2N-1)) in long double, |error| <= 2^-52 per component"""
    from pxmcmc_amd import ops

    ph = ops.dwav_phases(N)
    npl = 2 * N - 1
    q, n = np.arange(npl)[:, None], np.arange(-(N - 1), N, 2)[None, :]
    a = LD(2) * PI_LD * ((n * q) % npl).astype(LD) / LD(npl)
    er = float(np.abs(LD(ph.real) - np.cos(a)).max() / LD(2.0 ** -52))
    ei = float(np.abs(LD(ph.imag) - np.sin(a)).max() / LD(2.0 ** -52))
    print(f"DW-RATIO phases N={N} ratio={max(er, ei):.3f}")
    assert max(er, ei) <= 1.0
    assert np.array_equal(ph[0], np.ones(N, dtype=complex))  # gamma_0 = 0
    # and without a reference from the same libm: e^{i n gamma_{npl - q}} = conj(e^{i n gamma_q}), each component within 2^-53
    # of its value, so the two agree within 2^-52; | |ph|^2 - 1 | <= 2 (|c| + |s|) 2^-53 <= 2 sqrt(2) 2^-53 < 2^-51
    if N > 1:
        back = ph[np.arange(npl - 1, 0, -1)]
        assert np.abs(ph[1:].real - back.real).max() <= 2.0 ** -52 and np.abs(ph[1:].imag + back.imag).max() <= 2.0 ** -52
    assert float(np.abs(LD(ph.real) ** 2 + LD(ph.imag) ** 2 - 1).max()) <= 2.0 ** -51
    if N == 2:  # third roots of unity: the real part is -1/2 exactly
        assert np.all(ph[1:].real == -0.5)


@pytest.mark.parametrize("L,B,J_min", SHAPES)
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 12])
def test_python_tiling_matches_library_rows(L, B, J_min, N):
    """utils.wavelet_tiling (the prior's weights): psi^j_ln = sqrt((2l+1)/(8 pi^2)) kappa_j(l) s_ln, the expression of the
    library's harmonic synthesis row, with the same count of roundings (pi^2, its product with 8, the division, the sqrt
    halving them and rounding, the product with kappa, s_ln and the product with it: 7 u): within gamma(7) of the
    long-double row, hence within 2 gamma(7) of the library's"""
    from pxmcmc_amd import ops, utils

    phi, psi = utils.wavelet_tiling(B, L, N, J_min, 0)
    wa, ws, rows = ops.harm_weights(L, B, J_min, N, 0, True)
    rows = [tuple(int(v) for v in r) for r in rows]
    ra, rs = _row_refs(L, B, J_min, N, 0, True, rows)
    k0, _ = ops.tiling_axisym(L, B, J_min)
    el = np.arange(L)
    phi_ld = np.sqrt((2 * el + 1).astype(LD) / (LD(4) * PI_LD)) * LD(k0)  # (pi, the division, the sqrt, the product: 3 u)
    assert np.all(np.abs(LD(phi) - phi_ld) <= gam(4) * np.abs(phi_ld))
    for i, (b, n, bl) in enumerate(rows):
        if b == 0:
            continue
        col = np.where(abs(n) <= el, psi[el * el + el + n, b - 1], 0)  # (el^2 + el + n with |n| > el is another degree's entry)
        got = col.real if N % 2 else col.imag
        assert np.array_equal(got == 0, rs[i] == 0)
        assert np.all(np.abs(LD(got) - rs[i]) <= gam(7) * np.abs(rs[i]))
        lib = ws[i].real if N % 2 else ws[i].imag
        assert np.all(np.abs(LD(got) - LD(lib)) <= 2 * gam(7) * np.abs(rs[i]))


# ---- the stages: long-double statements with their magnitude sums ---------------------------------------------------------
def _parts(z):
    z = np.asarray(z)
    return LD(z.real), LD(z.imag)


def cmul_ld(a, b, conj_b=False):
    """a b (or a conj(b)) in long double -> (re, im, |re terms|, |im terms|): the magnitude sums of the rounding bounds"""
    ar, ai = _parts(a)
    br, bi = _parts(b)
    if conj_b:
        bi = -bi
    return ar * br - ai * bi, ar * bi + ai * br, np.abs(ar * br) + np.abs(ai * bi), np.abs(ar * bi) + np.abs(ai * br)


def gamma_fwd_ld(ph, G, sc):
    """X[q] = sc sum_k ph[q, k] G[k]; ph [npl, N], G [N, ...] (zeros for a skipped pair) -> (re, im, bre, bim) [npl, ...]"""
    pr, pi = _parts(ph)
    gr, gi = _parts(G)
    sc = LD(sc)
    t = lambda a, b: np.tensordot(a, b, axes=(1, 0))
    return (sc * (t(pr, gr) - t(pi, gi)), sc * (t(pr, gi) + t(pi, gr)),
            sc * (t(np.abs(pr), np.abs(gr)) + t(np.abs(pi), np.abs(gi))), sc * (t(np.abs(pr), np.abs(gi)) + t(np.abs(pi), np.abs(gr))))


def gamma_back_ld(ph, W, sc):
    """g[k] = sc sum_q W[q] conj(ph[q, k]); W [npl, ...] -> (re, im, bre, bim) [N, ...]"""
    pr, pi = _parts(ph)
    wr, wi = _parts(W)
    sc = LD(sc)
    t = lambda a, b: np.tensordot(a.T, b, axes=(1, 0))
    return (sc * (t(pr, wr) + t(pi, wi)), sc * (t(pr, wi) - t(pi, wr)),
            sc * (t(np.abs(pr), np.abs(wr)) + t(np.abs(pi), np.abs(wi))), sc * (t(np.abs(pr), np.abs(wi)) + t(np.abs(pi), np.abs(wr))))


def merge_ld(ws, bs, L):
    """f[c, lm] = sum_d [lm < bl_d^2] w_d[lm] b_d[c, lm]; ws: [bl_d^2] each, bs: [C, bl_d^2] each -> (re, im, bre, bim) [C, L^2]
    and t [L^2], the number of items that contribute to an entry"""
    C = bs[0].shape[0]
    out = [np.zeros((C, L * L), dtype=LD) for _ in range(4)]
    t = np.zeros(L * L, dtype=int)
    for w, b in zip(ws, bs):
        n = w.size
        for o, v in zip(out, cmul_ld(w[None, :], b)):
            o[:, :n] += v
        t[:n] += 1
    return (*out, t)


def worst_ratio(got, re, im, bre, bim, k):
    """max over the components of |got - ref| / (gamma(k) magnitude sum), k a number or an array that broadcasts; where the
    magnitude sum is zero the result must be exactly zero.  NaN if ``got`` holds one."""
    got = np.asarray(got)
    g = np.broadcast_to(gam(np.asarray(k, dtype=float)), got.shape)
    r = 0.0
    for e, m in ((np.abs(LD(got.real) - re), bre), (np.abs(LD(got.imag) - im), bim)):
        z = m == 0
        assert np.all(e[z] == 0), "a non-zero result where every term is zero"
        if (~z).any():
            r = np.maximum(r, float((e[~z] / (LD(g[~z]) * m[~z])).max()))
    return float(r)


# ---- the stages: float64 numpy statements -----------------------------------------------------------------------------------
def gamma_fwd_np(ph, G, sc):
    acc = np.zeros((ph.shape[0],) + G.shape[1:], dtype=complex)
    for k in range(ph.shape[1]):
        acc = acc + ph[:, k].reshape((-1,) + (1,) * (G.ndim - 1)) * G[k][None]
    return sc * acc


def gamma_back_np(ph, W, sc):
    acc = np.zeros((ph.shape[1],) + W.shape[1:], dtype=complex)
    for q in range(ph.shape[0]):
        acc = acc + np.conj(ph[q]).reshape((-1,) + (1,) * (W.ndim - 1)) * W[q][None]
    return sc * acc


def merge_np(ws, bs, L):
    f = np.zeros((bs[0].shape[0], L * L), dtype=complex)
    for w, b in zip(ws, bs):
        f[:, : w.size] = f[:, : w.size] + w[None, :] * b
    return f


class Stages:
    """what the stages of ``ops.DirWavPlan(L, B, J_min, N)`` read, from the library's host exports: the items in plan order,
    their weight rows spread over (l, m), the phases and the block layout of a coefficient vector"""

    def __init__(self, L, B, J_min, N):
        from pxmcmc_amd import ops

        self.L, self.N, self.npl = L, N, 2 * N - 1
        wa, ws, rows = ops.harm_weights(L, B, J_min, N)
        self.items = [tuple(int(v) for v in r) for r in rows]  # (block, n, bl)
        self.bls = ops.wav_bandlimits(L, B, J_min)
        el = np.repeat(np.arange(L), 2 * np.arange(L) + 1)
        self.wa = [wa[d][el[: bl * bl]] for d, (_, _, bl) in enumerate(self.items)]
        self.ws = [ws[d][el[: bl * bl]] for d, (_, _, bl) in enumerate(self.items)]
        self.ph = ops.dwav_phases(N)
        self.npix = [bl * (2 * bl - 1) for bl in self.bls]
        self.nplanes = [1] + [self.npl] * (len(self.bls) - 1)
        self.coef_off = np.concatenate([[0], np.cumsum([p * n for p, n in zip(self.nplanes, self.npix)])]).astype(int)
        self.ncoefs = int(self.coef_off[-1])

    def weights(self, which, cj):
        """the rows a stage multiplies with: which 0 analysis / 1 synthesis, conjugated with cj (harm_split / harm_merge)"""
        w = self.ws if which else self.wa
        return [np.conj(v) for v in w] if cj else w

    def block_items(self, b):
        """[(item index, orientation index k)] of block b"""
        return [(d, (n + self.N - 1) // 2 if blk else 0) for d, (blk, n, _) in enumerate(self.items) if blk == b]

    def stack(self, b, pix):
        """G [nn, C, npix] of block b from the items' pixel operands ``pix[d]`` [C, npix], zeros for the skipped pairs"""
        its = self.block_items(b)
        G = np.zeros((self.N if b else 1,) + pix[its[0][0]].shape, dtype=complex)
        for d, k in its:
            G[k] = pix[d]
        return G

    def planes(self, b, X):
        """W [nplanes, C, npix] of block b from coefficient vectors X [C, ncoefs]"""
        a, n = self.coef_off[b], self.npix[b]
        return np.moveaxis(X[:, a : a + self.nplanes[b] * n].reshape(X.shape[0], self.nplanes[b], n), 1, 0)

    def scale(self, b, norm):
        return 1.0 / self.nplanes[b] if norm and self.nplanes[b] > 1 else 1.0


def _cplx(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


@pytest.mark.parametrize("L,B,J_min,N", [(L, B, J, N) for (L, B, J) in SHAPES for N in NS if N <= L] + [(16, 2.0, 1, 16)])
def test_numpy_stage_statements_meet_the_stage_bounds(L, B, J_min, N):
    """the float64 numpy statements of the four stages within the bounds of the GPU tests of their long-double statements
    on the same tables and operands: gamma(N + 2) for the gamma stage in both directions (a product pair and a subtraction
    per term, N - 1 additions, the scale), gamma(2) for the split, gamma(t + 1) for a merge of t items"""
    S = Stages(L, B, J_min, N)
    rng = np.random.default_rng(100 * L + N)
    C = 2
    worst = dict(fwd=0.0, back=0.0, split=0.0, merge=0.0)
    pix = {d: _cplx(rng, C, bl * (2 * bl - 1)) for d, (_, _, bl) in enumerate(S.items)}
    X = _cplx(rng, C, S.ncoefs)
    for norm in (0, 1):
        for b in range(len(S.bls)):
            G, W, sc = S.stack(b, pix), S.planes(b, X), S.scale(b, norm)
            if S.nplanes[b] == 1:
                assert np.array_equal(gamma_fwd_np(np.ones((1, 1), dtype=complex), G, sc)[0], G[0])
                continue
            worst["fwd"] = max(worst["fwd"], worst_ratio(gamma_fwd_np(S.ph, G, sc), *gamma_fwd_ld(S.ph, G, sc), N + 2))
            worst["back"] = max(worst["back"], worst_ratio(gamma_back_np(S.ph, W, sc), *gamma_back_ld(S.ph, W, sc), N + 2))
    f = _cplx(rng, C, L * L)
    harm = [_cplx(rng, C, bl * bl) for (_, _, bl) in S.items]
    for which, cj in ((0, 0), (1, 1)):
        for w in S.weights(which, cj):
            worst["split"] = max(worst["split"], worst_ratio(w[None, :] * f[:, : w.size], *cmul_ld(w[None, :], f[:, : w.size]), 2))
    for which, cj in ((0, 1), (1, 0)):
        ws = S.weights(which, cj)
        *ref, t = merge_ld(ws, harm, L)
        worst["merge"] = max(worst["merge"], worst_ratio(merge_np(ws, harm, L), *ref, t[None, :] + 1))
    print(f"DW-RATIO numpy L={L} B={B} J_min={J_min} N={N} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0
