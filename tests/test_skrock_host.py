"""SKROCK on the host: recursion coefficients, the stability polynomial, a numpy model of the sampler against the
reference's own s = 1 trajectory (G16), and construction.  No GPU needed.

The numpy model below is written from the published method (Pereyra, Vargas-Mieles & Zygalakis, SIAM J. Imaging Sci.
13(2), 2020) and is shared with tests/test_gpu_skrock.py."""
import numpy as np
import pytest

from conftest import golden

ETA = 0.05


# ---- numpy model ------------------------------------------------------------------------------------------------------
def model_coefs(s, eta=ETA):
    """(w0, w1, mu, nu, kappa), arrays indexed 0..s (entry 0 unused)"""
    w0 = 1 + eta / s**2
    T = np.ones(s + 1)
    dT = np.zeros(s + 1)  # T_j'(w0) by differentiating the recurrence
    T[1], dT[1] = w0, 1.0
    for j in range(2, s + 1):
        T[j] = 2 * w0 * T[j - 1] - T[j - 2]
        dT[j] = 2 * T[j - 1] + 2 * w0 * dT[j - 1] - dT[j - 2]
    w1 = T[s] / dT[s]
    mu, nu, ka = np.zeros(s + 1), np.zeros(s + 1), np.zeros(s + 1)
    mu[1], nu[1], ka[1] = w1 / w0, s * w1 / 2, s * w1 / w0
    for j in range(2, s + 1):
        mu[j] = 2 * w1 * T[j - 1] / T[j]
        nu[j] = 2 * w0 * T[j - 1] / T[j]
        ka[j] = 1 - nu[j]
    return w0, w1, mu, nu, ka


def model_step(X, Z, s, delta, grad):
    """one SKROCK iteration X -> K_s with noise Z; grad(U) = grad log pi(U)"""
    _, _, mu, nu, ka = model_coefs(s)
    sq = np.sqrt(2 * delta)
    Km2, Km1 = X, X + mu[1] * delta * grad(X + nu[1] * sq * Z) + ka[1] * sq * Z
    for j in range(2, s + 1):
        Km2, Km1 = Km1, mu[j] * delta * grad(Km1) + nu[j] * Km1 + ka[j] * Km2
    return Km1


def soft(x, T):
    a = np.abs(x)
    return np.where(a > T, x / np.where(a > 0, a, 1) * (a - T), 0)


def toy_grad(data, invcov, lmda, T, setting="synthesis"):
    """grad log pi of the identity toy with an L1 prior (soft threshold T; the analysis prox of an identity transform
    is the same soft threshold)"""
    return lambda U: -(U - soft(U, T)) / lmda - invcov * (U - data)


def model_run(X0, data, invcov, lmda, delta, mu, s, nsamples, nburn, ngap, draw, T=None):
    """the reference's run loop (pxmcmc/mcmc.py:308-336) on the identity toy; draw(i) -> Z of iteration i"""
    T = lmda * mu if T is None else T
    grad = toy_grad(data, invcov, lmda, T)
    X = X0
    out = {"chain": [], "logPi": [], "L2s": [], "priors": [], "preds": []}
    i = j = 0
    while j < nsamples:
        X = model_step(X, draw(i), s, delta, grad)
        if i >= nburn and (ngap == 0 or (i - nburn) % ngap == 0):
            d = data - X
            L2 = np.vdot(d, invcov * d)
            prior = np.abs(X).sum()
            out["chain"].append(X)
            out["logPi"].append(-mu * prior - L2)
            out["L2s"].append(L2)
            out["priors"].append(prior)
            out["preds"].append(X)
            j += 1
        i += 1
    return {k: np.array(v) for k, v in out.items()}


def stability_R(s, ldelta):
    """K_s / X of the noise-free recursion on grad log pi(x) = -l x, as a function of l delta"""
    _, _, mu, nu, ka = model_coefs(s)
    Km2, Km1 = 1.0, 1.0 - mu[1] * ldelta
    for j in range(2, s + 1):
        Km2, Km1 = Km1, -mu[j] * ldelta * Km1 + nu[j] * Km1 + ka[j] * Km2
    return Km1


# ---- tests ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3, 5, 10, 30])
def test_coefficients(s):
    from pxmcmc_amd.mcmc import skrock_coefficients

    w0, w1, mu, nu, ka = skrock_coefficients(s, ETA)
    m = model_coefs(s)
    np.testing.assert_allclose([w0, w1], m[:2], rtol=1e-13)
    for a, b in zip((mu, nu, ka), m[2:]):
        np.testing.assert_allclose(a[1:], b[1:], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(nu[2:] + ka[2:], 1.0, rtol=0, atol=1e-15)
    # T_j(w0) by the recurrence equals cosh(j arccosh w0)
    T = [1.0, w0]
    for j in range(2, s + 1):
        T.append(2 * w0 * T[-1] - T[-2])
    np.testing.assert_allclose(T, np.cosh(np.arange(s + 1) * np.arccosh(w0)), rtol=1e-12)
    # T_s'(w0) = s U_{s-1}(w0) = s sinh(s t) / sinh(t), t = arccosh w0
    t = np.arccosh(w0)
    np.testing.assert_allclose(w1, np.cosh(s * t) / (s * np.sinh(s * t) / np.sinh(t)), rtol=1e-12)


def test_s1_coefficients_equal_the_reference():
    """s = 1: the published method and the reference agree (G16 stores the reference's values)"""
    from pxmcmc_amd.mcmc import skrock_coefficients

    g = golden("g16_skrock.npz")
    w0, w1, mu, nu, ka = skrock_coefficients(1, ETA)
    np.testing.assert_allclose([w0, w1, mu[1], nu[1], ka[1]], g["real_coefs"], rtol=1e-15)
    np.testing.assert_allclose([w0, w1, mu[1], nu[1], ka[1]], [1.05, 1.05, 1.0, 0.525, 1.0], rtol=1e-15)


@pytest.mark.parametrize("s", [1, 2, 5, 10, 30])
def test_stability_polynomial(s):
    """zero noise, grad log pi(x) = -l x: K_s = T_s(w0 - w1 l delta) / T_s(w0) X, and |K_s / X| <= 1 on
    l delta in [0, (2 - 4 eta / 3) s^2]"""
    w0, w1, _, _, _ = model_coefs(s)
    ld = np.linspace(0, (2 - 4 * ETA / 3) * s * s, 4001)
    R = np.array([stability_R(s, x) for x in ld])
    expect = np.polynomial.chebyshev.chebval(w0 - w1 * ld, [0] * s + [1]) / np.cosh(s * np.arccosh(w0))
    np.testing.assert_allclose(R, expect, rtol=1e-9, atol=1e-12)
    assert np.abs(R).max() <= 1 + 1e-12


@pytest.mark.parametrize("tag", ["real", "cplx"])
def test_model_reproduces_g16(tag):
    g = golden("g16_skrock.npz")
    lmda, delta, mu, nsamples, nburn, ngap = g["params"]
    data = g["data"]
    N = data.size
    cplx = tag == "cplx"
    rs = np.random.RandomState(int(g[f"{tag}_seed"]))
    draw = (lambda i: rs.randn(N) + rs.randn(N) * 1j) if cplx else (lambda i: rs.randn(N))
    out = model_run(g[f"{tag}_X0"], data, 100.0, lmda, delta, mu, 1, int(nsamples), int(nburn), int(ngap), draw)
    chain = out["chain"] if cplx else out["chain"].real
    np.testing.assert_allclose(chain, g[f"{tag}_chain"], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(out["logPi"].real, g[f"{tag}_logPi"], rtol=1e-11)
    np.testing.assert_allclose(out["L2s"].real, g[f"{tag}_L2s"], rtol=1e-11)
    np.testing.assert_allclose(out["priors"], g[f"{tag}_priors"], rtol=1e-11)
    np.testing.assert_allclose(out["preds"].real, g[f"{tag}_preds"], rtol=1e-11, atol=1e-13)


class _HostToy:
    """the attributes a sampler reads at construction (no device work)"""

    def __init__(self, n):
        self.data = np.zeros(n)
        self.nparams = n


def test_construction():
    from pxmcmc_amd.mcmc import SKROCK, MYULA, PxMALA, PxMCMC, PxMCMCParams  # noqa: F401  (the reference's import line)

    for s in (1, 4):
        sk = SKROCK(_HostToy(8), None, PxMCMCParams(s=s, nsamples=3), nchains=2, rng="numpy", seed=3, chain_offset=1,
                    use_graph=False, noise_bits=32, real_pairs=True)
        assert isinstance(sk, PxMCMC)
        assert sk.eta == 0.05 and sk.s == s
        w0, w1, mu, nu, ka = model_coefs(s)
        assert sk.omega_0 == pytest.approx(w0, rel=1e-15) and sk.omega_1 == pytest.approx(w1, rel=1e-13)
        for a in (sk.mus, sk.nus, sk.ks):
            assert a.shape == (s + 1,)
        assert sk.chain.shape == (2, 3, 8)
    for bad in (0, -1, 2.5, "3", True):
        with pytest.raises(ValueError):
            SKROCK(_HostToy(8), None, PxMCMCParams(s=bad))
