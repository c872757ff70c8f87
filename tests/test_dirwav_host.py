"""Directional (N = dirs > 1) scale-discretised wavelets on the host: the directionality component, admissibility,
``wavelet_tiling``, coefficient sizes, the prior's weights and a numpy model of the four transforms checked against the
literal SO(3) sum.  No GPU needed.

The numpy model below is written from the published construction (Leistedt et al. 2013; McEwen et al. 2015,
"Directional spin wavelets on the sphere") on top of ``oracle.ssht`` (any spin) and is shared with
tests/test_gpu_dirwav.py.  Conventions are those of DESIGN.md section 11."""
import numpy as np
import pytest
from math import comb

from oracle import s2let, ssht, wigner


# ---- numpy model ------------------------------------------------------------------------------------------------------
def dir_component(L, N):
    """s_lm [L*L]: nu sqrt(2^-g C(g, (g - m) / 2)) for m = -g, -g + 2, .., g, g = gamma_l the largest integer <= min(N - 1, l)
    of the parity of N - 1; nu = 1 (N odd) or i (N even)"""
    s = np.zeros(L * L, dtype=complex)
    nu = 1.0 if N % 2 else 1j
    for el in range(L):
        g = min(N - 1, el)
        if (N - 1 - g) % 2:
            g -= 1
        if g < 0:
            continue
        for m in range(-g, g + 1, 2):
            s[el * el + el + m] = nu * np.sqrt(2.0 ** -g * comb(g, (g - m) // 2))
    return s


class DirWavModel:
    """the four directional wavelet transforms of one (L, B, J_min, N), chain by chain, on oracle.ssht"""

    def __init__(self, L, B, J_min, N):
        self.L, self.B, self.J_min, self.N = L, B, J_min, N
        self.bls = s2let.bandlimits(B, L, J_min)
        self.kappa0, kap = s2let.tiling_axisym(B, L, J_min)
        self.kappa = kap[J_min:]
        self.s = dir_component(L, N)
        self.ns = list(range(-(N - 1), N, 2))
        self.npl = 2 * N - 1
        sizes = [s2let.mw_size(self.bls[0])] + [self.npl * s2let.mw_size(bl) for bl in self.bls[1:]]
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        self.nscal = sizes[0]
        self.ncoefs = int(self.offsets[-1])
        self.gammas = 2 * np.pi * np.arange(self.npl) / self.npl

    def _w(self, j, n, bl):
        """(-1)^n kappa_j(l) s_ln for l < bl, as a [bl*bl] vector over the (l, m) index"""
        el = np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)
        sln = np.array([self.s[l * l + l + n] if abs(n) <= l else 0.0 for l in range(bl)])
        return (-1.0) ** n * self.kappa[j][el] * sln[el]

    def _pairs(self, j):
        bl = self.bls[j + 1]
        return [(k, n) for k, n in enumerate(self.ns) if abs(n) < bl]

    def _scal_w(self):
        bl = self.bls[0]
        return self.kappa0[np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)]

    def _planes(self, X, j):
        bl = self.bls[j + 1]
        return X[self.offsets[j + 1] : self.offsets[j + 2]].reshape(self.npl, bl * (2 * bl - 1))

    def analysis(self, f):
        L = self.L
        flm = ssht.forward(np.asarray(f).reshape(L, 2 * L - 1), L, 0)
        X = np.zeros(self.ncoefs, dtype=complex)
        b0 = self.bls[0]
        X[: self.nscal] = ssht.inverse(self._scal_w() * flm[: b0 * b0], b0, 0).ravel()
        for j, bl in enumerate(self.bls[1:]):
            W = np.zeros((self.npl, bl * (2 * bl - 1)), dtype=complex)
            for k, n in self._pairs(j):
                a = np.conj(self._w(j, n, bl)) * flm[: bl * bl] / np.sqrt(2 * np.pi)
                g = ssht.inverse(a, bl, -n).ravel()
                W += np.exp(1j * n * self.gammas)[:, None] * g[None, :]
            X[self.offsets[j + 1] : self.offsets[j + 2]] = W.ravel()
        return X

    def analysis_adjoint(self, X):
        L = self.L
        flm = np.zeros(L * L, dtype=complex)
        b0 = self.bls[0]
        flm[: b0 * b0] += self._scal_w() * ssht.inverse_adjoint(X[: self.nscal].reshape(b0, 2 * b0 - 1), b0, 0)
        for j, bl in enumerate(self.bls[1:]):
            W = self._planes(X, j)
            for k, n in self._pairs(j):
                g = (np.exp(-1j * n * self.gammas)[:, None] * W).sum(0)
                b = ssht.inverse_adjoint(g.reshape(bl, 2 * bl - 1), bl, -n)
                flm[: bl * bl] += self._w(j, n, bl) * b / np.sqrt(2 * np.pi)
        return ssht.forward_adjoint(flm, L, 0).ravel()

    def synthesis(self, X):
        L = self.L
        flm = np.zeros(L * L, dtype=complex)
        b0 = self.bls[0]
        flm[: b0 * b0] += self._scal_w() * ssht.forward(X[: self.nscal].reshape(b0, 2 * b0 - 1), b0, 0)
        for j, bl in enumerate(self.bls[1:]):
            W = self._planes(X, j)
            for k, n in self._pairs(j):
                g = (np.exp(-1j * n * self.gammas)[:, None] * W).sum(0) / self.npl
                b = ssht.forward(g.reshape(bl, 2 * bl - 1), bl, -n)
                flm[: bl * bl] += self._w(j, n, bl) * b * np.sqrt(2 * np.pi)
        return ssht.inverse(flm, L, 0).ravel()

    def synthesis_adjoint(self, f):
        L = self.L
        flm = ssht.inverse_adjoint(np.asarray(f).reshape(L, 2 * L - 1), L, 0)
        X = np.zeros(self.ncoefs, dtype=complex)
        b0 = self.bls[0]
        X[: self.nscal] = ssht.forward_adjoint(self._scal_w() * flm[: b0 * b0], b0, 0).ravel()
        for j, bl in enumerate(self.bls[1:]):
            W = np.zeros((self.npl, bl * (2 * bl - 1)), dtype=complex)
            for k, n in self._pairs(j):
                a = np.conj(self._w(j, n, bl)) * flm[: bl * bl] * np.sqrt(2 * np.pi)
                g = ssht.forward_adjoint(a, bl, -n).ravel()
                W += np.exp(1j * n * self.gammas)[:, None] * g[None, :] / self.npl
            X[self.offsets[j + 1] : self.offsets[j + 2]] = W.ravel()
        return X

    def analysis_literal(self, f):
        """W^j(alpha_a, beta_b, gamma_c) = sum_lmn f_lm conj(psi^j_ln) D^l_mn(rho)*, D^l_mn = e^{-im alpha} d^l_mn(beta)
        e^{-in gamma}, d^l from the eigen route (no SHT, no spin transform)"""
        L = self.L
        flm = ssht.forward(np.asarray(f).reshape(L, 2 * L - 1), L, 0)
        X = np.zeros(self.ncoefs, dtype=complex)
        X[: self.nscal] = self.analysis(f)[: self.nscal]
        for j, bl in enumerate(self.bls[1:]):
            beta, alpha = ssht.sample_positions(bl)
            W = np.zeros((self.npl, bl, 2 * bl - 1), dtype=complex)
            for el in range(bl):
                d = wigner.wigner_d_eig(el, beta)  # [b, m + el, n + el]
                psi = np.sqrt((2 * el + 1) / (8 * np.pi ** 2)) * self.kappa[j][el] * self.s[el * el : (el + 1) ** 2]
                for m in range(-el, el + 1):
                    fm = flm[el * el + el + m]
                    if fm == 0:
                        continue
                    for n in range(-el, el + 1):
                        c = fm * np.conj(psi[n + el])
                        if c == 0:
                            continue
                        W += c * (np.exp(1j * n * self.gammas)[:, None, None] * d[None, :, m + el, n + el][:, :, None]
                                  * np.exp(1j * m * alpha)[None, None, :])
            X[self.offsets[j + 1] : self.offsets[j + 2]] = W.ravel()
        return X


def bandlimited_image(L, rng, real=False):
    flm = rng.normal(size=L * L) + 1j * rng.normal(size=L * L)
    if real:
        for el in range(L):
            flm[el * el + el] = flm[el * el + el].real
            for m in range(1, el + 1):
                flm[el * el + el - m] = (-1.0) ** m * np.conj(flm[el * el + el + m])
    f = ssht.inverse(flm, L, 0).ravel()
    return f.real.astype(complex) if real else f


# ---- directionality component and admissibility ------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6])
def test_directionality_component(N):
    L = 12
    s = dir_component(L, N)
    for el in range(L):
        row = s[el * el : (el + 1) ** 2]
        if N % 2 == 0 and el == 0:
            assert np.all(row == 0)
            continue
        assert abs(np.sum(np.abs(row) ** 2) - 1) < 1e-14
        for m in range(-el, el + 1):
            assert abs(row[-m + el] - (-1.0) ** m * np.conj(row[m + el])) < 1e-15  # s_{l,-m} = (-1)^m conj(s_lm)
            if (m - (N - 1)) % 2 or abs(m) > min(N - 1, el):
                assert row[m + el] == 0
    if N == 1:
        assert np.all(s[np.arange(L) ** 2 + np.arange(L)] == 1)
    if N == 2:  # gamma_l = 1 for l >= 1: s_{l,+-1} = i / sqrt(2)
        assert abs(s[1 * 1 + 1 + 1] - 1j / np.sqrt(2)) < 1e-15


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("L,B,J_min", [(16, 2.0, 1), (32, 1.5, 2)])
def test_admissibility(L, B, J_min, N):
    """kappa_0^2 + sum_j kappa_j^2 sum_m |s_lm|^2 = 1 for every l < L (where s_l. is not empty)"""
    from pxmcmc_amd import ops

    k0, k = ops.tiling_axisym(L, B, J_min)
    s = dir_component(L, N)
    for el in range(L):
        ss = np.sum(np.abs(s[el * el : (el + 1) ** 2]) ** 2)
        tot = k0[el] ** 2 + np.sum(k[J_min:, el] ** 2) * ss
        if ss == 0:  # l = 0 with N even: only the scaling function carries it (kappa_0(0) = 1)
            assert abs(k0[el] - 1) < 1e-14
        else:
            assert abs(tot - 1) < 1e-12, (el, tot)


# ---- wavelet_tiling, sizes, prior weights ------------------------------------------------------------------------------
def test_wavelet_tiling_n1_unchanged_and_directional():
    from pxmcmc_amd import utils

    L, B, J_min = 16, 2.0, 2
    phi, psi = utils.wavelet_tiling(B, L, 1, J_min, 0)
    ophi, opsi = s2let.wavelet_tiling(B, L, 1, J_min)
    assert np.abs(phi - ophi).max() < 1e-14 and np.abs(psi - opsi).max() < 1e-14
    for N in (2, 3, 4):
        phiN, psiN = utils.wavelet_tiling(B, L, N, J_min, 0)
        assert np.array_equal(phiN, phi) and psiN.shape == psi.shape
        s = dir_component(L, N)
        el = np.repeat(np.arange(L), 2 * np.arange(L) + 1)
        for col in range(psi.shape[1]):
            # psi^j_lm = psi^j_l0(N = 1) s_lm; the power per l is unchanged
            assert np.abs(psiN[:, col] - psi[el * el + el, col] * s).max() < 1e-15
            assert abs(np.vdot(psiN[:, col], psiN[:, col]) - np.vdot(psi[:, col], psi[:, col]) + (
                0 if N % 2 else abs(psi[0, col]) ** 2)) < 1e-13
    with pytest.raises(NotImplementedError):
        utils.wavelet_tiling(B, L, 2, J_min, 2)


@pytest.mark.parametrize("L,B,J_min", [(16, 2.0, 1), (64, 1.5, 2), (256, 2.0, 2)])
@pytest.mark.parametrize("N", [1, 2, 4, 5])
def test_dwav_ncoefs_layout(L, B, J_min, N):
    import ctypes as C

    from pxmcmc_amd._lib import check, lib

    nscal = C.c_int64()
    n = check(lib.pxm_dwav_ncoefs(L, B, J_min, N, C.byref(nscal)))
    bls = s2let.bandlimits(B, L, J_min)
    assert nscal.value == s2let.mw_size(bls[0])
    assert n == s2let.mw_size(bls[0]) + sum((2 * N - 1) * s2let.mw_size(bl) for bl in bls[1:])
    if N == 1:
        assert n == check(lib.pxm_wav_ncoefs(L, B, J_min, None))
    with pytest.raises(Exception):
        check(lib.pxm_dwav_ncoefs(L, B, J_min, 0, None))


@pytest.mark.parametrize("N", [1, 2, 3])
def test_prior_weights_per_plane(N, monkeypatch):
    from pxmcmc_amd import prior
    from pxmcmc_amd.prior import S2_Wavelets_L1, S2_Wavelets_L1_Power_Weights
    from pxmcmc_amd.utils import mw_map_weights

    monkeypatch.setattr(prior.ops, "as_device", lambda x, dtype=None: x)  # (the device copy of the weights: no GPU here)

    L, B, J_min = 16, 2.0, 2
    pr = S2_Wavelets_L1("synthesis", None, None, 0.5, L, B, J_min, dirs=N)
    bls = s2let.bandlimits(B, L, J_min)
    model = DirWavModel(L, B, J_min, N)
    assert len(pr.map_weights) == model.ncoefs
    assert np.array_equal(pr.map_weights[: model.nscal], mw_map_weights(bls[0]))
    for j, bl in enumerate(bls[1:]):
        blk = pr.map_weights[model.offsets[j + 1] : model.offsets[j + 2]].reshape(2 * N - 1, -1)
        for c in range(2 * N - 1):
            assert np.array_equal(blk[c], mw_map_weights(bl))
    assert np.allclose(pr.T, 0.5 * pr.map_weights)
    if N > 1:
        with pytest.raises(NotImplementedError):
            S2_Wavelets_L1_Power_Weights("synthesis", None, None, 0.5, L, B, J_min, dirs=N)


# ---- the numpy model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B,J_min,N", [(8, 2.0, 1, 2), (12, 2.0, 1, 3), (10, 1.5, 2, 4)])
def test_model_analysis_equals_literal_so3_sum(L, B, J_min, N):
    rng = np.random.default_rng(L * 10 + N)
    f = bandlimited_image(L, rng)
    M = DirWavModel(L, B, J_min, N)
    a, b = M.analysis(f), M.analysis_literal(f)
    assert np.abs(a - b).max() < 1e-12 * np.abs(b).max()


# the tilings test_gpu_dirwav.py adds to the dyadic ones: non-dyadic B, odd L, J_min = 0 (a scaling band-limit of 1), N = L
OTHER_TILINGS = [(13, 1.5, 1), (33, 1.7, 2), (16, 2.0, 0), (13, 3.0, 1)]


@pytest.mark.parametrize("L,B,J_min", OTHER_TILINGS)
@pytest.mark.parametrize("N", [2, 5, "L"])
def test_model_on_other_tilings(L, B, J_min, N):
    """the model on the cases the device is held to it at: exact left inverse, both adjoint pairs, and at L = 13 the
    literal SO(3) sum"""
    N = L if N == "L" else N
    rng = np.random.default_rng(100 * L + 10 * J_min + N)
    M = DirWavModel(L, B, J_min, N)
    assert M.bls[0] >= 1 and M.ncoefs == M.offsets[-1]
    if J_min == 0:
        assert M.bls[0] == 1  # the scaling function is the l = 0 term alone
    f = bandlimited_image(L, rng)
    X = M.analysis(f)
    assert np.abs(M.synthesis(X) - f).max() < 1e-12 * np.abs(f).max()
    Y = rng.normal(size=M.ncoefs) + 1j * rng.normal(size=M.ncoefs)
    g = rng.normal(size=f.size) + 1j * rng.normal(size=f.size)
    assert abs(np.vdot(Y, M.analysis(g)) - np.vdot(M.analysis_adjoint(Y), g)) < 1e-11 * abs(np.vdot(Y, M.analysis(g)))
    assert abs(np.vdot(g, M.synthesis(Y)) - np.vdot(M.synthesis_adjoint(g), Y)) < 1e-11 * abs(np.vdot(g, M.synthesis(Y)))
    if L == 13:
        b = M.analysis_literal(f)
        assert np.abs(X - b).max() < 1e-12 * np.abs(b).max()
        for i in range(len(M.bls)):  # and block by block, against the block's own largest entry
            sl = slice(M.offsets[i], M.offsets[i + 1])
            assert np.abs(X[sl] - b[sl]).max() <= 1e-12 * np.abs(b[sl]).max(), i


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5])
def test_model_properties(N):
    L, B, J_min = 12, 2.0, 1
    rng = np.random.default_rng(N)
    M = DirWavModel(L, B, J_min, N)
    f = bandlimited_image(L, rng)
    X = M.analysis(f)
    assert np.abs(M.synthesis(X) - f).max() < 1e-12 * np.abs(f).max()  # exact left inverse
    Y = rng.normal(size=M.ncoefs) + 1j * rng.normal(size=M.ncoefs)
    g = rng.normal(size=f.size) + 1j * rng.normal(size=f.size)
    assert abs(np.vdot(Y, M.analysis(g)) - np.vdot(M.analysis_adjoint(Y), g)) < 1e-11 * abs(np.vdot(Y, M.analysis(g)))
    assert abs(np.vdot(g, M.synthesis(Y)) - np.vdot(M.synthesis_adjoint(g), Y)) < 1e-11 * abs(np.vdot(g, M.synthesis(Y)))
    fr = bandlimited_image(L, rng, real=True)
    Xr = M.analysis(fr)
    assert np.abs(Xr.imag).max() < 1e-12 * np.abs(Xr.real).max()
    if N == 1:  # the axisymmetric transform (oracle.s2let) with c_a = 1/sqrt(2 pi), c_s = sqrt(2 pi)
        W = s2let.WaveletTransform(L, B, J_min)
        assert np.abs(X - W.analysis(f)).max() < 1e-13 * np.abs(X).max()
        assert np.abs(M.synthesis(Y) - W.synthesis(Y)).max() < 1e-12 * np.abs(W.synthesis(Y)).max()
