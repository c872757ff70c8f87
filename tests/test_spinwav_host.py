"""Spin wavelets (spin s != 0, dirs = 1) on the host: a numpy model of the four transforms, its properties,
``wavelet_tiling`` at spin s, the prior's power weights and the dry-run address check of the spin-s plan.  No GPU needed.

The model follows the convention of DESIGN.md section 12 on top of ``oracle.ssht`` (any spin) and ``oracle.s2let`` (the
spin-0 scale stages): f_lm = spin-s forward SHT at L; every block (scaling included) is the spin-0 inverse SHT at its own
bandlimit of c kappa_j(l) f_lm; synthesis is the left inverse and the adjoints are the conjugate transposes.  It is shared
with tests/test_gpu_spinwav.py."""
import numpy as np
import pytest

from oracle import s2let, ssht

SPINS = [1, 2, -2, 3]


# ---- numpy model ------------------------------------------------------------------------------------------------------
class SpinWavModel(s2let.WaveletTransform):
    """the four axisymmetric wavelet transforms of spin-s images, chain by chain: s2let.WaveletTransform with the L-level
    transform at spin s and the kernels zeroed for l < |s|"""

    def __init__(self, L, B, J_min, spin):
        super().__init__(L, B, J_min)
        self.spin = spin
        self.kappa0 = self.kappa0.copy()
        self.kappa = self.kappa.copy()
        self.kappa0[: abs(spin)] = 0.0
        self.kappa[:, : abs(spin)] = 0.0

    def synthesis(self, X):
        L = self.L
        flm = np.zeros(L * L, dtype=complex)
        for i, bl, kap, _, cs in self._filters():
            wlm = ssht.forward(self._block(X, i).reshape(bl, 2 * bl - 1), bl, 0)
            el = np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)
            flm[: bl * bl] += cs * kap[el] * wlm
        return ssht.inverse(flm, L, self.spin).reshape(-1)

    def synthesis_adjoint(self, f):
        L = self.L
        flm = ssht.inverse_adjoint(np.asarray(f).reshape(L, 2 * L - 1), L, self.spin)
        X = np.zeros(self.ncoefs, dtype=complex)
        for i, bl, kap, _, cs in self._filters():
            el = np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)
            X[self.offsets[i] : self.offsets[i + 1]] = ssht.forward_adjoint(cs * kap[el] * flm[: bl * bl], bl, 0).reshape(-1)
        return X

    def analysis(self, f):
        L = self.L
        flm = ssht.forward(np.asarray(f).reshape(L, 2 * L - 1), L, self.spin)
        X = np.zeros(self.ncoefs, dtype=complex)
        for i, bl, kap, ca, _ in self._filters():
            el = np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)
            X[self.offsets[i] : self.offsets[i + 1]] = ssht.inverse(ca * kap[el] * flm[: bl * bl], bl, 0).reshape(-1)
        return X

    def analysis_adjoint(self, X):
        L = self.L
        flm = np.zeros(L * L, dtype=complex)
        for i, bl, kap, ca, _ in self._filters():
            wlm = ssht.inverse_adjoint(self._block(X, i).reshape(bl, 2 * bl - 1), bl, 0)
            el = np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)
            flm[: bl * bl] += ca * kap[el] * wlm
        return ssht.forward_adjoint(flm, L, self.spin).reshape(-1)


def spin_bandlimited_image(rng, L, spin):
    """a random spin-s MW map of bandlimit L (f_lm = 0 for l < |s|)"""
    flm = rng.normal(size=L * L) + 1j * rng.normal(size=L * L)
    flm[: spin * spin] = 0
    return ssht.inverse(flm, L, spin).reshape(-1)


def _cplx(rng, n):
    return rng.normal(size=n) + 1j * rng.normal(size=n)


# ---- model properties -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin", SPINS)
@pytest.mark.parametrize("L,B,J_min", [(8, 2.0, 1), (13, 1.7, 2)])
def test_model_synthesis_inverts_analysis(L, B, J_min, spin):
    rng = np.random.default_rng(L + 10 * spin + 100)
    M = SpinWavModel(L, B, J_min, spin)
    f = spin_bandlimited_image(rng, L, spin)
    assert np.abs(M.synthesis(M.analysis(f)) - f).max() < 1e-12 * np.abs(f).max()


@pytest.mark.parametrize("spin", SPINS)
def test_model_adjoints(spin):
    L, B, J_min = 12, 2.0, 2
    rng = np.random.default_rng(7 + spin)
    M = SpinWavModel(L, B, J_min, spin)
    X, Y = _cplx(rng, M.ncoefs), _cplx(rng, M.ncoefs)
    f, g = _cplx(rng, L * (2 * L - 1)), _cplx(rng, L * (2 * L - 1))
    for fwd, adj, a, b in ((M.synthesis, M.synthesis_adjoint, X, g), (M.analysis, M.analysis_adjoint, f, Y)):
        lhs, rhs = np.vdot(b, fwd(a)), np.vdot(adj(b), a)
        assert abs(lhs - rhs) < 1e-12 * abs(lhs), (fwd.__name__, lhs, rhs)


def test_model_spin0_is_the_s2let_oracle():
    L, B, J_min = 12, 2.0, 2
    rng = np.random.default_rng(5)
    M, O = SpinWavModel(L, B, J_min, 0), s2let.WaveletTransform(L, B, J_min)
    X, f = _cplx(rng, M.ncoefs), _cplx(rng, L * (2 * L - 1))
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        a, b = getattr(M, name)(arg), getattr(O, name)(arg)
        assert np.abs(a - b).max() < 1e-13 * np.abs(b).max(), name


@pytest.mark.parametrize("spin", [1, 2, 3])
def test_ssht_conjugation_sign(spin):
    """oracle.ssht: the spin -s coefficients of conj(f) are (-1)^(s+m) conj(f_{l,-m}) of the spin-s ones"""
    L = 10
    rng = np.random.default_rng(spin)
    f = spin_bandlimited_image(rng, L, spin)
    a = ssht.forward(f.reshape(L, 2 * L - 1), L, spin)
    b = ssht.forward(np.conj(f).reshape(L, 2 * L - 1), L, -spin)
    for el in range(abs(spin), L):
        for m in range(-el, el + 1):
            want = (-1.0) ** (spin + m) * np.conj(a[el * el + el - m])
            assert abs(b[el * el + el + m] - want) < 1e-12 * np.abs(a).max()


@pytest.mark.parametrize("spin", SPINS)
def test_model_conjugation(spin):
    """analysis_{-s}(conj f) = (-1)^s conj(analysis_s(f)) block by block: with the ssht relation above and the spin-0 one
    (-1)^m conj(W_{l,-m}) for the coefficients of conj(W), the m-dependent signs cancel and (-1)^s is left"""
    L, B, J_min = 11, 2.0, 2
    rng = np.random.default_rng(40 + spin)
    f = spin_bandlimited_image(rng, L, spin)
    Ms, Mn = SpinWavModel(L, B, J_min, spin), SpinWavModel(L, B, J_min, -spin)
    a, b = Ms.analysis(f), Mn.analysis(np.conj(f))
    for i in range(len(Ms.bls)):
        blk = slice(Ms.offsets[i], Ms.offsets[i + 1])
        assert np.abs(b[blk] - (-1.0) ** spin * np.conj(a[blk])).max() < 1e-12 * np.abs(a).max(), i


# ---- wavelet_tiling and the prior ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin", SPINS)
def test_wavelet_tiling_spin(spin):
    from pxmcmc_amd import utils

    L, B, J_min = 32, 2.0, 2
    phi0, psi0 = utils.wavelet_tiling(B, L, 1, J_min, 0)
    phi, psi = utils.wavelet_tiling(B, L, 1, J_min, spin)
    s = abs(spin)
    assert phi.shape == phi0.shape and psi.shape == psi0.shape
    assert not phi[:s].any() and not psi[: s * s].any()
    np.testing.assert_array_equal(phi[s:], phi0[s:])
    np.testing.assert_array_equal(psi[s * s :], psi0[s * s :])
    with pytest.raises(NotImplementedError):
        utils.wavelet_tiling(B, L, 3, J_min, spin)


@pytest.mark.parametrize("spin", [2, -3])
def test_power_weights_follow_the_spin_tiling(spin):
    from pxmcmc_amd import utils
    from pxmcmc_amd.prior import S2_Wavelets_L1_Power_Weights

    L, B, J_min = 16, 2.0, 2
    P = S2_Wavelets_L1_Power_Weights.__new__(S2_Wavelets_L1_Power_Weights)
    P.L, P.B, P.J_min, P.dirs, P.eta, P.spin = L, B, J_min, 1, 1, spin
    w = P._power_weight_map()
    # the scaling block's weight is 2 pi^2 / (power nsamples) sin(theta): its power is that of the spin-s phi_l
    phi, _ = utils.wavelet_tiling(B, L, 1, J_min, spin)
    bl0 = int(utils._multires_bandlimits(L, B, J_min)[0])
    thetas, _ = utils.sample_positions(bl0)
    want = np.repeat(2 * np.pi ** 2 / (np.vdot(phi, phi).real * bl0 * (2 * bl0 - 1)) * np.sin(thetas), 2 * bl0 - 1)
    np.testing.assert_allclose(w[: want.size], want, rtol=1e-14)
    P.spin = 0
    w0 = P._power_weight_map()
    assert w.shape == w0.shape and not np.array_equal(w[: want.size], w0[: want.size])


# ---- dry-run address check of the spin-s plan -----------------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 256])
@pytest.mark.parametrize("C", [1, 3, 16])
def test_spin_plan_address_ranges(L, C):
    from pxmcmc_amd import _lib

    lib = _lib.lib
    n0 = lib.pxm_host_check_address_ranges(L, 2.0, 2, 2, C, 2)  # bit 2 alone: the spin-0 plan
    n2 = lib.pxm_host_check_address_ranges(L, 2.0, 2, 2, C, 2 | 8)  # bit 8: the same plan at spin 2
    assert n0 > 0 and n2 > 0, lib.pxm_last_error()
    # the four L-level lists and the two of the ring step are unpaired at spin 2: one task per m instead of per +-m pair
    assert n2 > n0
    # bit 4 (weak-lensing lists) is skipped for a spin-s plan, not refused
    assert lib.pxm_host_check_address_ranges(L, 2.0, 2, 2, C, 2 | 4 | 8) == n2


def test_spin_plan_bad_spin_refused():
    import ctypes

    from pxmcmc_amd import _lib

    lib = _lib.lib
    h = ctypes.c_void_p()
    assert lib.pxm_wav_plan_create_spin(8, 2.0, 1, 8, 1, 0, ctypes.byref(h)) < 0
    assert b"|spin| must be < L" in lib.pxm_last_error()


def test_transform_spin_gates():
    from pxmcmc_amd.transforms import SphericalWaveletTransform

    with pytest.raises(NotImplementedError):
        SphericalWaveletTransform(16, 2.0, 2, dirs=2, spin=2)
    with pytest.raises(ValueError):
        SphericalWaveletTransform(16, 2.0, 2, spin=16)
