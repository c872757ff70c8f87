"""Harmonic-space wavelet transforms (SphericalWaveletTransform(harmonic=True)) on the host: a numpy model of the four
operators, their properties, their links to the pixel-space models, the coefficient count, the gates and the
Kaiser-Squires estimate.  No GPU needed.

The model follows DESIGN.md section 13 (s2let's lm2lmn / lmn2lm): per (scale j, orientation n) block
W^{j,n}_lm = sqrt(8 pi^2/(2l+1)) kappa_j(l) conj(s_ln) f_lm and S_lm = kappa_0(l) f_lm; synthesis is
f_lm = kappa_0 S_lm + sum_{j,n} sqrt((2l+1)/(8 pi^2)) kappa_j(l) s_ln W^{j,n}_lm; the adjoints are the conjugate
transposes.  It is shared with tests/test_gpu_harmwav.py."""
import numpy as np
import pytest

from oracle import pxmcmc_np, s2let, ssht
from test_dirwav_host import DirWavModel, bandlimited_image, dir_component
from test_spinwav_host import SpinWavModel, spin_bandlimited_image

CASES = [(1, 0), (2, 0), (4, 0), (5, 0), (1, 2), (1, -3)]  # (N, spin)


# ---- numpy model ------------------------------------------------------------------------------------------------------
class HarmWavModel:
    """the four harmonic-space wavelet transforms of one (L, B, J_min, N, spin), chain by chain"""

    def __init__(self, L, B, J_min, N=1, spin=0, tiling=None):
        """tiling: (kappa_0 [L], kappa [J_max + 1, L]) to use instead of oracle.s2let's (the library's own, so that a
        device comparison at large L sees the kernels and not two quadratures of the tiling)"""
        self.L, self.B, self.J_min, self.N, self.spin = L, B, J_min, N, spin
        self.bls = s2let.bandlimits(B, L, J_min)
        k0, kap = s2let.tiling_axisym(B, L, J_min) if tiling is None else tiling
        k0, kap = k0.copy(), kap[J_min:].copy()
        k0[: abs(spin)] = 0.0
        kap[:, : abs(spin)] = 0.0
        s = dir_component(L, N)
        self.blocks = []  # (bl, analysis weights [bl^2], synthesis weights [bl^2])
        el0 = np.repeat(np.arange(L), 2 * np.arange(L) + 1)
        w0 = k0[el0[: self.bls[0] ** 2]].astype(complex)
        self.blocks.append((self.bls[0], w0, w0))
        for j, bl in enumerate(self.bls[1:]):
            el = el0[: bl * bl]
            for n in range(-(N - 1), N, 2):
                sln = np.array([s[l * l + l + n] if abs(n) <= l else 0.0 for l in range(bl)])[el]
                wa = np.sqrt(8 * np.pi ** 2 / (2 * el + 1)) * kap[j][el] * np.conj(sln)
                ws = np.sqrt((2 * el + 1) / (8 * np.pi ** 2)) * kap[j][el] * sln
                self.blocks.append((bl, wa, ws))
        sizes = [bl * bl for bl, _, _ in self.blocks]
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        self.nscal = sizes[0]
        self.ncoefs = int(self.offsets[-1])

    def analysis(self, flm):
        X = np.zeros(self.ncoefs, dtype=complex)
        for i, (bl, wa, _) in enumerate(self.blocks):
            X[self.offsets[i] : self.offsets[i + 1]] = wa * flm[: bl * bl]
        return X

    def analysis_adjoint(self, X):
        flm = np.zeros(self.L ** 2, dtype=complex)
        for i, (bl, wa, _) in enumerate(self.blocks):
            flm[: bl * bl] += np.conj(wa) * X[self.offsets[i] : self.offsets[i + 1]]
        return flm

    def synthesis(self, X):
        flm = np.zeros(self.L ** 2, dtype=complex)
        for i, (bl, _, ws) in enumerate(self.blocks):
            flm[: bl * bl] += ws * X[self.offsets[i] : self.offsets[i + 1]]
        return flm

    def synthesis_adjoint(self, flm):
        X = np.zeros(self.ncoefs, dtype=complex)
        for i, (bl, _, ws) in enumerate(self.blocks):
            X[self.offsets[i] : self.offsets[i + 1]] = np.conj(ws) * flm[: bl * bl]
        return X


class HarmWavOracleTransform:
    """the model behind the oracle's transform interface (oracle.pxmcmc_np.ForwardOperator): inverse = synthesis"""

    def __init__(self, model):
        self.w = model
        self.ncoefs = model.ncoefs

    def forward(self, f):
        return self.w.analysis(np.asarray(f).astype(complex))

    def inverse(self, X):
        return self.w.synthesis(np.asarray(X).astype(complex))

    def inverse_adjoint(self, f):
        return self.w.synthesis_adjoint(np.asarray(f).astype(complex))

    def forward_adjoint(self, X):
        return self.w.analysis_adjoint(np.asarray(X).astype(complex))


class WeakLensingHarmonicOracle:
    """pxmcmc/measurements.py:86-182 in numpy (the kernel of oracle.pxmcmc_np)"""

    def __init__(self, L):
        self.L = L
        self.k = pxmcmc_np.wl_harmonic_kernel(L)

    def forward(self, klm):
        return pxmcmc_np.wl_harmonic_mapping(klm, self.k)

    adjoint = forward

    def sks_estimate(self, glm):
        out = glm / self.k
        out[:4] = 0
        return out


def band_limited_flm(rng, L, spin=0):
    """random f_lm of bandlimit L with the degrees l < |spin| zero"""
    flm = rng.normal(size=L * L) + 1j * rng.normal(size=L * L)
    flm[: spin * spin] = 0
    return flm


def cplx(rng, n):
    return rng.normal(size=n) + 1j * rng.normal(size=n)


# ---- model properties -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,spin", CASES)
@pytest.mark.parametrize("L,B,J_min", [(8, 2.0, 1), (13, 1.7, 2)])
def test_model_synthesis_inverts_analysis(L, B, J_min, N, spin):
    rng = np.random.default_rng(L + 10 * N + spin)
    M = HarmWavModel(L, B, J_min, N, spin)
    flm = band_limited_flm(rng, L, spin)
    assert np.abs(M.synthesis(M.analysis(flm)) - flm).max() < 1e-12 * np.abs(flm).max()


@pytest.mark.parametrize("N,spin", CASES)
def test_model_adjoints(N, spin):
    L, B, J_min = 12, 2.0, 1
    rng = np.random.default_rng(7 + N + spin)
    M = HarmWavModel(L, B, J_min, N, spin)
    f, X = cplx(rng, L * L), cplx(rng, M.ncoefs)
    for fwd, adj in ((M.analysis, M.analysis_adjoint), (M.synthesis_adjoint, M.synthesis)):
        a, b = np.vdot(fwd(f), X), np.vdot(f, adj(X))
        assert abs(a - b) < 1e-12 * abs(a)


@pytest.mark.parametrize("N,spin", CASES)
def test_model_zero_below_max_n_spin(N, spin):
    """entries with l < max(|n|, |spin|) are zero after analysis"""
    L, B, J_min = 12, 2.0, 1
    M = HarmWavModel(L, B, J_min, N, spin)
    X = M.analysis(cplx(np.random.default_rng(3), L * L))
    i = 1
    for j, bl in enumerate(M.bls[1:]):
        el = np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)
        for n in range(-(N - 1), N, 2):
            blk = X[M.offsets[i] : M.offsets[i + 1]]
            assert np.all(blk[el < max(abs(n), abs(spin))] == 0)
            i += 1


# ---- links to the pixel-space models -----------------------------------------------------------
@pytest.mark.parametrize("spin", [0, 2, -3])
def test_link_n1_to_pixel_blocks(spin):
    """N = 1: harmonic block j = sqrt(2 pi) sqrt(8 pi^2/(2l+1)) SHT_{bl_j}(pixel block j); the scaling blocks are SHTs"""
    L, B, J_min = 10, 2.0, 1
    rng = np.random.default_rng(11)
    P = SpinWavModel(L, B, J_min, spin)
    H = HarmWavModel(L, B, J_min, 1, spin)
    f = spin_bandlimited_image(rng, L, spin)
    Xp, Xh = P.analysis(f), H.analysis(ssht.forward(f.reshape(L, 2 * L - 1), L, spin))
    for i, bl in enumerate(H.bls):
        blk = ssht.forward(Xp[P.offsets[i] : P.offsets[i + 1]].reshape(bl, 2 * bl - 1), bl, 0)
        el = np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)
        if i:
            blk = np.sqrt(2 * np.pi) * np.sqrt(8 * np.pi ** 2 / (2 * el + 1)) * blk
        assert np.abs(blk - Xh[H.offsets[i] : H.offsets[i + 1]]).max() < 1e-11


@pytest.mark.parametrize("N", [2, 3, 4])
def test_link_directional_to_pixel_planes(N):
    """W^{j,n} = (-1)^n sqrt(2 pi) sqrt(8 pi^2/(2l+1)) a^{j,n}, a^{j,n} = spin -n SHT of g_n = (1/(2N-1)) sum_c
    e^{-i n gamma_c} W^j(gamma_c)"""
    L, B, J_min = 10, 2.0, 1
    rng = np.random.default_rng(N)
    P = DirWavModel(L, B, J_min, N)
    H = HarmWavModel(L, B, J_min, N, 0)
    f = bandlimited_image(L, rng)
    Xp, Xh = P.analysis(f), H.analysis(ssht.forward(f.reshape(L, 2 * L - 1), L, 0))
    b0 = H.bls[0]
    assert np.abs(ssht.forward(Xp[: P.nscal].reshape(b0, 2 * b0 - 1), b0, 0) - Xh[: H.nscal]).max() < 1e-11
    i = 1
    for j, bl in enumerate(H.bls[1:]):
        W = P._planes(Xp, j)
        el = np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)
        for n in range(-(N - 1), N, 2):
            blk = Xh[H.offsets[i] : H.offsets[i + 1]]
            if abs(n) < bl:
                g = (np.exp(-1j * n * P.gammas)[:, None] * W).sum(0) / P.npl
                a = ssht.forward(g.reshape(bl, 2 * bl - 1), bl, -n)
                ref = (-1.0) ** n * np.sqrt(2 * np.pi) * np.sqrt(8 * np.pi ** 2 / (2 * el + 1)) * a
                ref[el < abs(n)] = 0
            else:
                ref = np.zeros(bl * bl)
            assert np.abs(ref - blk).max() < 1e-11, (j, n)
            i += 1


# ---- sizes and gates --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B,J_min", [(16, 2.0, 1), (64, 1.5, 2), (256, 2.0, 2)])
@pytest.mark.parametrize("N", [1, 2, 4, 5])
def test_hwav_ncoefs_layout(L, B, J_min, N):
    import ctypes as C

    from pxmcmc_amd._lib import check, lib

    nscal = C.c_int64()
    n = check(lib.pxm_hwav_ncoefs(L, B, J_min, N, C.byref(nscal)))
    bls = s2let.bandlimits(B, L, J_min)
    assert nscal.value == bls[0] ** 2
    assert n == bls[0] ** 2 + N * sum(bl * bl for bl in bls[1:])
    if L <= 16:
        assert n == HarmWavModel(L, B, J_min, N).ncoefs
    if (L, B, J_min) == (256, 2.0, 2):
        assert n == {1: 152912, 4: 611600}.get(N, n)
    with pytest.raises(Exception):
        check(lib.pxm_hwav_ncoefs(L, B, J_min, 0, None))


def test_hwav_plan_gates_host():
    """the argument checks of plan creation run before the device is touched"""
    import ctypes

    from pxmcmc_amd import _lib

    lib = _lib.lib
    h = ctypes.c_void_p()
    assert lib.pxm_hwav_plan_create(8, 2.0, 1, 1, 8, 1, 0, ctypes.byref(h)) < 0
    assert b"|spin| must be < L" in lib.pxm_last_error()
    assert lib.pxm_hwav_plan_create(8, 2.0, 1, 2, 2, 1, 0, ctypes.byref(h)) < 0
    assert b"spin != 0 needs N = 1" in lib.pxm_last_error()
    assert lib.pxm_hwav_plan_create(8, 2.0, 1, 9, 0, 1, 0, ctypes.byref(h)) < 0
    assert lib.pxm_hwav_plan_create(8, 2.0, 1, 1, 0, 0, 0, ctypes.byref(h)) < 0
    assert lib.pxm_hwav_plan_create(8, 2.0, 9, 1, 0, 1, 0, ctypes.byref(h)) < 0
    assert lib.pxm_hwav_analysis(None, None, None, 1, None) < 0


def test_transform_harmonic_gates():
    from pxmcmc_amd.transforms import SphericalWaveletTransform

    with pytest.raises(NotImplementedError):
        SphericalWaveletTransform(16, 2.0, 2, dirs=2, spin=2, harmonic=True)
    with pytest.raises(ValueError):
        SphericalWaveletTransform(16, 2.0, 2, spin=16, harmonic=True)
    with pytest.raises(ValueError):
        SphericalWaveletTransform(16, 2.0, 2, spin=-17, harmonic=True)


# ---- Kaiser-Squires estimate ------------------------------------------------------------------------------------------
def test_sks_oracle_is_the_reference_division():
    """measurements.py:173-182: glm / k with the first four entries zeroed, and the inverse of the mapping for l >= 2"""
    L = 12
    rng = np.random.default_rng(5)
    W = WeakLensingHarmonicOracle(L)
    klm = cplx(rng, L * L)
    back = W.sks_estimate(W.forward(klm))
    assert np.all(back[:4] == 0)
    assert np.abs(back[4:] - klm[4:]).max() < 1e-14 * np.abs(klm).max() * 10
    glm = cplx(rng, L * L)
    est = W.sks_estimate(glm)
    k = pxmcmc_np.wl_harmonic_kernel(L)
    assert np.array_equal(est[4:], glm[4:] / k[4:])
