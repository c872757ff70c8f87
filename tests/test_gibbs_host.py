"""The Gibbs sampler on the Gaussian posterior, on the host (pxmcmc_amd/gibbs_np.py): the nu rule, the
assignment of the Philox deviates to the groups, what construction refuses, and the distribution of the numpy sampler
against the identity model's marginal posterior by quadrature."""
import numpy as np
import pytest

from pxmcmc_amd import gibbs_np as G

# ---- the identity model of the distribution tests (tests/test_gpu_gibbs.py runs the GPU sampler on the same inputs) -----------
IDENTITY_SIZES, IDENTITY_VARIANCES, IDENTITY_NOISE_VAR = (3, 8, 16, 37), (4.0, 1.0, 0.25, 2.0), 0.25
IDENTITY_CHAINS, IDENTITY_SWEEPS, IDENTITY_BURN = 16, 400, 50


def identity_model(seed=20241):
    """-> (data [64], bounds [5]): d = x + noise, x_i ~ N(0, v_k) in group k, noise variance 0.25"""
    rng = np.random.default_rng(seed)
    bounds = np.concatenate([[0], np.cumsum(IDENTITY_SIZES)])
    x = rng.standard_normal(bounds[-1]) * np.sqrt(np.repeat(IDENTITY_VARIANCES, IDENTITY_SIZES))
    return x + np.sqrt(IDENTITY_NOISE_VAR) * rng.standard_normal(bounds[-1]), bounds


def identity_expected_log_variance(data, bounds):
    """the quadrature mean of log v of every group at q = 0"""
    S = np.add.reduceat(data * data, bounds[:-1])
    return np.array([G.identity_log_variance_moments(S[k], n, IDENTITY_NOISE_VAR, q=0.0)[0] for k, n in enumerate(np.diff(bounds))])


def z_scores(log_v, expected):
    """``log_v`` [nsweeps, C, K] after burn-in -> per group (mean of the chain means - expected) / (standard error of the
    chain means)"""
    means = log_v.mean(axis=0)  # [C, K]
    se = means.std(axis=0, ddof=1) / np.sqrt(means.shape[0])
    return (means.mean(axis=0) - expected) / se


@pytest.mark.parametrize("dof", [1, 2])
@pytest.mark.parametrize("q", [0.0, 0.5, 1.0, 2.0])
def test_nu_rule(dof, q):
    nk = np.array([1, 2, 3, 17, 1024])
    nu = G.nu_rule(nk, dof, q)
    assert nu.dtype.kind == "i"
    assert np.array_equal(nu, dof * nk + int(2 * q) - 2)
    if dof == 2:  # the complex harmonic state and degree groups: n_l = 2 l + 1 -> nu_l = 4 l + 2 q
        ell = np.arange(12)
        assert np.array_equal(G.nu_rule(2 * ell + 1, 2, q), 4 * ell + int(2 * q))


def test_q_is_half_integer_and_at_most_two():
    for q in (0.25, np.nan, np.inf, 2.5, 3.0):
        with pytest.raises(ValueError):
            G.check_q(q)
    assert [G.check_q(q) for q in (-1.0, 0.0, 0.5, 2.0)] == [-2, 0, 1, 4]


@pytest.mark.parametrize("dof", [1, 2])
def test_deviate_indices_are_disjoint_and_suffice(dof):
    rng = np.random.default_rng(5)
    for _ in range(20):
        sizes = rng.integers(1, 9, size=rng.integers(1, 12))
        b = np.concatenate([[0], np.cumsum(sizes)])
        n, K = b[-1], sizes.size
        seen = np.zeros(n + K + 1, dtype=int)
        for q in (0.0, 0.5, 1.0, 2.0):
            nu = G.nu_rule(sizes, dof, q)
            seen[:] = 0
            for k in range(K):
                if nu[k] < 1:
                    continue
                idx, comp = G.deviate_index(b, k, np.arange(nu[k]))
                pairs = np.unique(idx)
                assert pairs.size <= sizes[k] + 1  # a sampled group needs at most n_k + 1 pairs: q <= 2 is the rule
                assert pairs.min() == b[k] + k and pairs.max() <= b[k + 1] + k
                assert np.array_equal(comp, np.arange(nu[k]) & 1)
                seen[pairs] += 1
            assert seen.max() <= 1  # no pair belongs to two groups
        # the ranges the groups own are disjoint for any offsets, whatever nu
        own = [np.arange(b[k] + k, b[k + 1] + k + 1) for k in range(K)]
        assert np.unique(np.concatenate(own)).size == n + K


def test_slice_table():
    S = 4
    b = np.array([0, 1, 5, 14, 14 + 2 * S + 3])
    tab, g0 = G.slice_table(b, S)
    assert g0.tolist() == [0, 1, 2, 5, 8] and tab.shape == (8, 2)
    covered = np.concatenate([np.arange(b[k] + j * S, min(b[k] + (j + 1) * S, b[k + 1])) for k, j in tab])
    assert np.array_equal(covered, np.arange(b[-1]))


def test_refusals():
    n = 12
    ok = dict(n=n, dof=1, bounds=[0, 3, 12], q=0.0, fixed=(), D=1.0, precision_bounds=(1e-6, 1e6))
    G.check_setup(**ok)
    for bad in ([0, 3, 11], [1, 3, 12], [0, 3, 3, 12], [0, 5, 3, 12], [0.0, 3.0, 12.0], [12], [[0, 12]]):
        with pytest.raises(ValueError):
            G.check_setup(**dict(ok, bounds=bad))
    # an unsampled group that is not marked fixed: real n_k = 2 at q = 0 has nu = 0; the complex monopole at q = 0 too
    with pytest.raises(ValueError, match="fixed"):
        G.check_setup(**dict(ok, bounds=[0, 2, 12]))
    assert G.check_setup(**dict(ok, bounds=[0, 2, 12], fixed=[0]))["sampled"].tolist() == [False, True]
    with pytest.raises(ValueError, match="fixed"):
        G.check_setup(**dict(ok, dof=2, bounds=[0, 1, 4, 12]))
    assert G.check_setup(**dict(ok, dof=2, bounds=[0, 1, 4, 12], q=1.0))["nu"].tolist() == [2, 6, 16]
    with pytest.raises(ValueError):
        G.check_setup(**dict(ok, fixed=[2]))
    # an initial precision that is not constant inside a group
    D = np.repeat([2.0, 3.0], [3, 9])
    assert G.check_setup(**dict(ok, D=D))["D_groups"].tolist() == [2.0, 3.0]
    D[7] = 3.5
    with pytest.raises(ValueError, match="constant"):
        G.check_setup(**dict(ok, D=D))
    # clamp limits
    for pb in ((0.0, 1.0), (1.0, np.inf), (np.nan, 1.0), (-1.0, 1.0), (2.0, 1.0), (1.0,)):
        with pytest.raises(ValueError):
            G.check_setup(**dict(ok, precision_bounds=pb))
    for q in (0.25, 2.5):
        with pytest.raises(ValueError):
            G.check_setup(**dict(ok, q=q))


def test_conditional_draw_models_agree():
    """the float64 draw lies within the bound of the extended-precision one; fixed groups and a zero field"""
    rng = np.random.default_rng(2)
    b = np.array([0, 1, 3, 40, 41 + 60])
    for cplx in (False, True):
        x = rng.standard_normal(b[-1]) + (1j * rng.standard_normal(b[-1]) if cplx else 0)
        om = rng.standard_normal(b[-1] + 5) + 1j * rng.standard_normal(b[-1] + 5)
        for q in (0.0, 1.0, 2.0):
            nu = G.nu_rule(np.diff(b), 2 if cplx else 1, q)
            sampled = nu >= 1
            old = np.array([7.0, 8.0, 9.0, 10.0])
            got = G.variance_draw_np(x, b, q, sampled, old, om, 1e-30, 1e30)
            ld = G.variance_draw_ld(x, b, q, sampled, old, om, 1e-30, 1e30)
            assert np.all(np.abs(got - ld["D"]) <= ld["D_bound"])
            assert np.array_equal(got[~sampled], old[~sampled])
            assert np.all(ld["D_bound"][sampled] < 1e-13 * ld["D"][sampled])
        assert np.array_equal(G.variance_draw_np(0 * x, b, 2.0, np.ones(4, bool), old, om, 1e-3, 1e3), np.full(4, 1e3))


def test_identity_sampler_is_the_dense_sampler():
    """``identity_gibbs_np`` (vectorised, chi-square deviates from the generator) and ``gibbs_run_np`` with ``Phi = I`` fed the
    same deviates, placed in the variance stream by ``deviate_index``, give the same chain: 4 sweeps of 3 chains.  Both
    are float64 evaluations of one formula on a diagonal system (condition number below 10): 1e-12 relative per sweep."""
    data, b = identity_model()
    n, K, C, nsweeps, seed = data.size, 4, 3, 4, 5
    _, nu = G.sampled_groups(b, 1, 0.0)
    rng = np.random.default_rng(seed)
    streams = []
    for _ in range(nsweeps):  # the order in which identity_gibbs_np draws
        w1, w2 = rng.standard_normal((C, n)), rng.standard_normal((C, n))
        wv = np.zeros((C, n + K + 1), dtype=complex)
        for k in range(K):
            z = rng.standard_normal((C, int(nu[k])))
            idx, comp = G.deviate_index(b, k, np.arange(nu[k]))
            wv[:, idx[comp == 0]] += z[:, comp == 0]
            wv[:, idx[comp == 1]] += 1j * z[:, comp == 1]
        streams.append((w1, w2, wv))
    Dg0 = np.array([0.5, 1.0, 2.0, 4.0])
    w = np.full(n, 1 / IDENTITY_NOISE_VAR)
    _, dense = G.gibbs_run_np(np.eye(n), w, data, b, 0.0, (), Dg0, nsweeps, C, lambda t, c: tuple(a[c] for a in streams[t]))
    fast = G.identity_gibbs_np(data, IDENTITY_NOISE_VAR, b, 0.0, Dg0, nsweeps, C, np.random.default_rng(seed))
    assert dense.shape == fast.shape == (nsweeps, C, K)
    for t in range(nsweeps):
        assert np.allclose(fast[t], dense[t], rtol=(t + 1) * 1e-12, atol=0), np.abs(fast[t] / dense[t] - 1).max()
    assert np.all(fast[1:] != fast[:-1]) and np.all(fast[:, 0] != fast[:, 1])


def test_dense_sweep_on_the_identity_against_its_formula():
    """``gibbs_sweep_np`` with ``Phi = I`` against the closed form of the identity model written out here"""
    data, b = identity_model()
    n = data.size
    rng = np.random.default_rng(0)
    w1, w2 = rng.standard_normal(n), rng.standard_normal(n)
    wv = rng.standard_normal(n + 5) + 1j * rng.standard_normal(n + 5)
    w = np.full(n, 1 / IDENTITY_NOISE_VAR)
    Dg = np.array([0.5, 1.0, 2.0, 4.0])
    x, Dn = G.gibbs_sweep_np(np.eye(n), w, data, b, 0.0, np.ones(4, bool), Dg, w1, w2, wv, 1e-30, 1e30)
    D = np.repeat(Dg, np.diff(b))
    want = (w * data + np.sqrt(w) * w1 + np.sqrt(D) * w2) / (w + D)
    assert np.allclose(x, want, rtol=1e-13, atol=0)
    sig = np.add.reduceat(x * x, b[:-1])
    chi = np.array([np.sum(G.group_deviates(wv, b, k, G.nu_rule(b[k + 1] - b[k], 1, 0.0)) ** 2) for k in range(4)])
    assert np.allclose(Dn, chi / sig, rtol=1e-13, atol=0)


def test_numpy_sampler_distribution():
    """identity model, q = 0, 16 chains, 400 sweeps of which 50 burn-in: the mean of log v of every group within 5 standard
    errors (of the 16 chain means) of the quadrature value"""
    data, b = identity_model()
    expected = identity_expected_log_variance(data, b)
    Dg = G.identity_gibbs_np(data, IDENTITY_NOISE_VAR, b, 0.0, np.ones(4), IDENTITY_SWEEPS, IDENTITY_CHAINS,
                             np.random.default_rng(77))
    z = z_scores(-np.log(Dg[IDENTITY_BURN:]), expected)
    print("numpy sampler: expected log v", expected, "z", z)
    assert np.all(np.abs(z) <= 5.0), z
