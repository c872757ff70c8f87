"""Host model of SAPG with one theta per group (pxm_sapg_step_groups, SAPG(groups=...)): the numpy statement of the grouped sum
and update in the kernels' operation order, the offsets of the wavelet scales, the arithmetic of SAPG.apply with groups, and the
statistical yardstick -- a Laplace denoising problem of two blocks whose block-wise marginal MLEs differ by more than a factor
two, so that one theta for all elements cannot pass.

    thr_i = fl(theta[c][k(i)] T_i);   X1 as in test_sapg_host.py
    G[c][k] = (1 / lmda) sum_{b_k <= i < b_k+1} T_i |X1_i|   (sapg_sum_np of the group's sub-vector)
    eta[c][k] = clip(eta[c][k] + rho[k] (d[k] - theta[c][k] G[c][k]));   theta[c][k] = exp(eta[c][k])

The models of tests/test_sapg_host.py are imported, not restated."""
import ctypes

import numpy as np
import pytest

from test_sapg_host import EPS, closed_form_mle, rho_table, sapg_step_np, sapg_sum_np, sapg_update_np

# Largest relative deviation of the host loop's theta_hat[k] from the block's closed-form MLE on two_block_problem(), over the
# seeds 0 ... 7 (test_host_loop_finds_the_block_mles measures them and holds them to these values).  As in test_sapg_host.py
# the deviation is MYULA's bias, not noise: the seeds lie within 0.07 % (block 1) and 0.22 % (block 2) of each other.
# Observed (block MLEs 4.8033 and 11.4995; single-theta MLE 5.8343):
# block 1: -1.065 %, -1.061 %, -1.048 %, -1.080 %, -1.093 %, -1.084 %, -1.113 %, -1.112 %
# block 2: -7.235 %, -7.368 %, -7.243 %, -7.446 %, -7.381 %, -7.396 %, -7.344 %, -7.391 %
# from theta_0 = 25 (seed 0): -1.065 %, -7.235 %.
GROUP_REL_DEV = (0.0113, 0.0750)

TWO_BLOCK_BOUNDS = (0, 700, 1024)


# ---- numpy model ---------------------------------------------------------------------------------------------------------
def element_theta(theta, bounds):
    """theta [C, K] -> [C, n]: the value of every element's group"""
    return np.repeat(np.asarray(theta, dtype=float), np.diff(bounds), axis=1)


def sapg_groups_step_np(X, g, T, theta, bounds, delta, lmda, w):
    """the X update with a threshold per element: theta [C, K]"""
    n = X.shape[1]
    thr = element_theta(theta, bounds) * np.broadcast_to(np.asarray(T, dtype=float), (n,))  # rounded before the shrink
    from oracle import pxmcmc_np

    return pxmcmc_np.chain_step(X, pxmcmc_np.soft(X, thr), g, delta, lmda, w)


def sapg_groups_sum_np(X1, T, bounds):
    """S [K] of one chain: every group is summed as a state of its own length (its own number of slices)"""
    Tv = np.broadcast_to(np.asarray(T, dtype=float), X1.shape)
    return np.array([sapg_sum_np(X1[a:b], Tv[a:b]) for a, b in zip(bounds[:-1], bounds[1:])])


def sapg_groups_update_np(S, theta, eta, d, rho, lmda, eta_min, eta_max, pool=False):
    """one update from the sums S [C, K] -> (theta, eta, G), each [C, K]; d and rho [K]; every operation rounded as written;
    pooling takes the chain-order mean group by group"""
    G = np.asarray(S, dtype=float) / lmda
    if pool:
        s = np.zeros(G.shape[1])
        for gc in G:
            s = s + gc
        G = np.broadcast_to(s / G.shape[0], G.shape).copy()
    eta = np.minimum(np.maximum(eta + rho * (d - theta * G), eta_min), eta_max)
    return np.exp(eta), eta, G


# ---- the statistical yardstick -------------------------------------------------------------------------------------------
def two_block_problem(n=1024, bounds=TWO_BLOCK_BOUNDS, theta_star=(5.0, 12.0), sigma=0.05, seed=2020):
    """laplace_problem() with x drawn block by block, block k ~ Laplace(1 / theta*_k), then the noise"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.laplace(scale=1.0 / t, size=b - a) for t, a, b in zip(theta_star, bounds[:-1], bounds[1:])])
    y = x + sigma * rng.normal(size=n)
    lmda = sigma ** 2
    return dict(n=n, bounds=tuple(bounds), y=y, sigma=sigma, lmda=lmda, T=lmda, delta=0.98 / (1 / sigma ** 2 + 1 / lmda),
                warmup=200, niter=1500, burn=500, theta0=1.0, theta_min=1e-3, theta_max=1e3)


def block_mles(prob):
    return np.array([closed_form_mle(prob["y"][a:b], prob["sigma"]) for a, b in zip(prob["bounds"][:-1], prob["bounds"][1:])])


def sapg_groups_np(prob, seed, theta0=None):
    """the host loop for one chain with one theta per block, numpy noise -> (theta_hat [K], theta trace [iterations, K]);
    the step size of block k is normalised by the block's own dimension"""
    rng = np.random.default_rng([seed, 77])
    y, sigma, lmda, delta, n, bounds = prob["y"], prob["sigma"], prob["lmda"], prob["delta"], prob["n"], prob["bounds"]
    d = np.diff(bounds).astype(float)
    rho = np.stack([rho_table(prob["warmup"], prob["niter"], dk) for dk in d], axis=1)
    lo, hi = np.log(prob["theta_min"]), np.log(prob["theta_max"])
    eta = np.log(np.full((1, len(d)), prob["theta0"] if theta0 is None else theta0, dtype=float))
    theta = np.exp(eta)
    X = y[None, :].copy()
    trace = np.empty((len(rho), len(d)))
    for k in range(len(rho)):
        g = (X - y) / sigma ** 2
        X = sapg_groups_step_np(X, g, prob["T"], theta, bounds, delta, lmda, rng.normal(size=(1, n)))
        theta, eta, _ = sapg_groups_update_np(sapg_groups_sum_np(X[0], prob["T"], bounds)[None], theta, eta, d, rho[k], lmda, lo, hi)
        trace[k] = theta[0]
    return trace[prob["warmup"] + prob["burn"]:].mean(axis=0), trace


# ---- tests ---------------------------------------------------------------------------------------------------------------
def test_grouped_update_is_the_projected_step_per_group():
    """eta[c][k] moves by rho_k theta (d_k / theta - G), the paper's projected step of block k on the log scale; the clip
    holds; pooling is per group; a row of zeros in rho leaves eta alone; one group is the ungrouped update"""
    theta = np.array([[2.0, 0.5, 1.5], [0.25, 4.0, 1.0]])
    eta = np.log(theta)
    S, lmda = np.array([[3.0, 9.0, 0.5], [7.0, 0.125, 2.0]]), 0.5
    d, rho = np.array([10.0, 3.0, 16.0]), np.array([0.01, 0.02, 0.005])
    th, e, G = sapg_groups_update_np(S, theta, eta, d, rho, lmda, -5.0, 5.0)
    assert np.array_equal(G, S / lmda)
    assert np.allclose(e, eta + rho * theta * (d / theta - G), rtol=4 * EPS, atol=4 * EPS) and np.allclose(th, np.exp(e), rtol=2 * EPS)
    for k in range(3):  # group k alone through the ungrouped model
        th1, e1, G1 = sapg_update_np(S[:, k], theta[:, k], eta[:, k], d[k], rho[k], lmda, -5.0, 5.0)
        assert np.array_equal(th[:, k], th1) and np.array_equal(e[:, k], e1) and np.array_equal(G[:, k], G1)
    th, e, G = sapg_groups_update_np(S, theta, eta, d, rho, lmda, -5.0, 5.0, pool=True)
    assert np.array_equal(G, np.broadcast_to((S[0] / lmda + S[1] / lmda) / 2, (2, 3)))
    th, e, _ = sapg_groups_update_np(S, theta, eta, d, 10.0 * np.ones(3), lmda, -0.25, 0.75)
    assert set(e.ravel()) <= {-0.25, 0.75} and np.array_equal(th, np.exp(e))
    th, e, _ = sapg_groups_update_np(S, theta, eta, d, np.zeros(3), lmda, -5.0, 5.0)  # the warm-up: nothing moves
    assert np.array_equal(e, eta)
    th, e, _ = sapg_groups_update_np(S, theta, eta, d, np.array([0.0, 0.02, 0.0]), lmda, -5.0, 5.0)
    assert np.array_equal(e[:, [0, 2]], eta[:, [0, 2]]) and np.all(e[:, 1] != eta[:, 1])


def test_grouped_sum_is_the_sum_of_each_sub_vector():
    """every group in its own slices: a one-element group, a boundary inside a 256-block, a group on the grid-stride path"""
    import math

    rng = np.random.default_rng(4)
    bounds = (0, 3, 65544, 65600)
    X1 = rng.normal(size=bounds[-1]) + 1j * rng.normal(size=bounds[-1])
    T = np.abs(rng.normal(size=bounds[-1]))
    S = sapg_groups_sum_np(X1, T, bounds)
    for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        want = math.fsum(T[a:b] * np.sqrt(X1.real[a:b] ** 2 + X1.imag[a:b] ** 2))
        assert abs(S[k] - want) <= (b - a) * EPS * want
    assert np.array_equal(sapg_groups_sum_np(X1, T, (0, bounds[-1])), [sapg_sum_np(X1, T)])
    assert sapg_groups_sum_np(X1.real, 0.5, (0, 1, 258, 300))[0] == 0.5 * abs(X1.real[0])


def test_grouped_step_is_the_ungrouped_step_per_block():
    rng = np.random.default_rng(8)
    C, bounds = 2, (0, 5, 12, 40)
    X, g, w = (rng.normal(size=(C, 40)) + 1j * rng.normal(size=(C, 40)) for _ in range(3))
    T = np.abs(rng.normal(size=40))
    theta = np.array([[0.7, 1.0, 2.3], [1.9, 0.4, 1.0]])
    X1 = sapg_groups_step_np(X, g, T, theta, bounds, 0.9e-2, 2.5e-2, w)
    for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        assert np.array_equal(X1[:, a:b], sapg_step_np(X[:, a:b], g[:, a:b], T[a:b], theta[:, k], 0.9e-2, 2.5e-2, w[:, a:b]))


# ---- the offsets of the wavelet scales -----------------------------------------------------------------------------------
def _ncoefs(L, B, J_min, dirs, harmonic):
    """the coefficient count the plans report, from the library's host-only functions (no device)"""
    from pxmcmc_amd import _lib

    nscal = ctypes.c_int64(0)
    if harmonic:
        n = _lib.lib.pxm_hwav_ncoefs(L, B, J_min, dirs, ctypes.byref(nscal))
    elif dirs == 1:
        n = _lib.lib.pxm_wav_ncoefs(L, B, J_min, ctypes.byref(nscal))
    else:
        n = _lib.lib.pxm_dwav_ncoefs(L, B, J_min, dirs, ctypes.byref(nscal))
    assert n > 0
    return int(n), int(nscal.value)


@pytest.mark.parametrize("harmonic", [False, True], ids=["pixel", "harmonic"])
@pytest.mark.parametrize("dirs,spin", [(1, 0), (3, 0), (1, 2)])
@pytest.mark.parametrize("L,B,J_min", [(16, 2, 2), (32, 2, 0), (24, 3, 1)])
def test_wavelet_scale_bounds(L, B, J_min, dirs, spin, harmonic):
    from pxmcmc_amd import ops
    from pxmcmc_amd.utils import _multires_bandlimits, mw_size, wavelet_scale_bounds

    b = wavelet_scale_bounds(L, B, J_min, dirs=dirs, spin=spin, harmonic=harmonic)
    bls = _multires_bandlimits(L, B, J_min)
    K = ops.j_max(L, B) - J_min + 2
    assert b.dtype == np.int64 and len(b) == K + 1 == len(bls) + 1 and b[0] == 0 and np.all(np.diff(b) > 0)
    per_plane = [int(bl) ** 2 if harmonic else mw_size(int(bl)) for bl in bls]
    planes = dirs if harmonic else 2 * dirs - 1  # harmonic space: one bl_j^2 block per n = -(N - 1), -(N - 3), ..., N - 1
    assert np.diff(b).tolist() == [per_plane[0]] + [planes * s for s in per_plane[1:]]
    ncoefs, nscal = _ncoefs(L, B, J_min, dirs, harmonic)
    assert b[-1] == ncoefs and b[1] == nscal


def test_flagship_plan_fits_the_group_limit():
    from pxmcmc_amd import ops
    from pxmcmc_amd.utils import wavelet_scale_bounds

    assert len(wavelet_scale_bounds(512, 2, 0)) - 1 == 11 <= ops.SAPG_GROUPS_MAX
    assert ops.SAPG_GROUPS_MAX == 32


def test_group_bounds_rule():
    """the wrapper's rule for ``bounds``, the one the C-ABI applies"""
    from pxmcmc_amd import ops

    assert ops.sapg_group_bounds([0, 3, 10], 10).tolist() == [0, 3, 10]
    assert ops.sapg_group_bounds(np.array([0, 10], dtype=np.int32), 10).dtype == np.int64
    for bad in ([0, 3, 9], [1, 3, 10], [0, 3, 3, 10], [0, 5, 3, 10], [10], [], [0.0, 10.0], [[0, 10]], "scale",
                list(range(0, 34)), None):
        with pytest.raises(ValueError, match="bounds"):
            ops.sapg_group_bounds(bad, 33 if isinstance(bad, list) and len(bad) == 34 else 10)
    assert len(ops.sapg_group_bounds(list(range(0, 33)), 32)) == 33  # K = 32 is allowed


# ---- apply() with groups -------------------------------------------------------------------------------------------------
class _FakePrior:
    def __init__(self, T, map_weights=None):
        self.T = T
        self._T_dev = "stale"
        self.map_weights = map_weights
        self._weights_dev = None


class _FakeWeights:
    """what apply() needs of a device tensor"""

    def __init__(self, a):
        self.a = np.asarray(a, dtype=float)

    def cpu(self):
        return self

    def numpy(self):
        return self.a


@pytest.mark.parametrize("shape", ["K", "CK"])
def test_apply_arithmetic_on_a_fake_trace(shape, monkeypatch):
    """apply() with groups needs no run and no device: T and the weights scaled per block by the chain mean of theta_hat, mu
    untouched, inputs untouched (the upload of the new weights is replaced by the identity here)"""
    from pxmcmc_amd import sapg
    from pxmcmc_amd.mcmc import PxMCMCParams

    monkeypatch.setattr(sapg.ops, "as_device", lambda a, dtype=None: np.asarray(a))
    est = object.__new__(sapg.SAPG)
    est.group_bounds = np.array([0, 2, 3, 7], dtype=np.int64)
    hat = np.array([[2.0, 0.5, 3.0], [4.0, 1.5, 1.0]])
    est.theta_hat = hat[0] if shape == "K" else hat
    s = hat[0] if shape == "K" else (hat[0] + hat[1]) / 2
    per = np.repeat(s, [2, 1, 4])
    p = PxMCMCParams(lmda=1e-2, delta=1e-3, mu=3.0, verbosity=0)
    # scalar T, no weights (plain L1)
    reg = _FakePrior(0.25)
    reg2, p2 = est.apply(reg, p)
    assert reg2 is not reg and p2 is not p and reg.T == 0.25 and reg._weights_dev is None and reg._T_dev == "stale"
    assert np.array_equal(reg2.T, 0.25 * per) and reg2._T_dev is None and np.array_equal(reg2._weights_dev, per)
    assert p2.mu == 3.0 and p.mu == 3.0
    # vector T with weights (S2_Wavelets_L1)
    w = np.linspace(0.5, 2.0, 7)
    reg = _FakePrior(1e-2 * w, map_weights=w.copy())
    reg._weights_dev = _FakeWeights(w)
    T_before = reg.T.copy()
    reg2, p2 = est.apply(reg, p)
    assert np.array_equal(reg.T, T_before) and np.array_equal(reg.map_weights, w) and np.array_equal(reg._weights_dev.a, w)
    assert np.array_equal(reg2.T, T_before * per) and np.array_equal(reg2.map_weights, w * per)
    assert np.array_equal(reg2._weights_dev, w * per) and p2.mu == 3.0
    # consistency: mu prior'(X) = (1 / lmda) sum T'_i |X_i| when T = lmda mu w
    X = np.random.default_rng(0).normal(size=7)
    T = p.lmda * p.mu * w
    assert p.mu * np.sum(w * per * np.abs(X)) == pytest.approx(np.sum(T * per * np.abs(X)) / p.lmda, rel=8 * EPS)


def test_theta0_forms():
    from pxmcmc_amd.sapg import SAPG

    f = SAPG._group_theta0
    assert np.array_equal(f(2.0, 3, 2), np.full((3, 2), 2.0))
    assert np.array_equal(f([1.0, 2.0], 3, 2), [[1.0, 2.0]] * 3)
    assert np.array_equal(f([[1.0], [2.0], [3.0]], 3, 2), [[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]])
    assert np.array_equal(f(np.arange(6.0).reshape(3, 2), 3, 2), np.arange(6.0).reshape(3, 2))
    assert np.array_equal(f([5.0], 1, 1), [[5.0]])
    with pytest.raises(ValueError, match="ambiguous"):
        f([1.0, 2.0, 3.0], 3, 3)
    assert np.array_equal(f([[1.0], [2.0], [3.0]], 3, 3), np.repeat([[1.0], [2.0], [3.0]], 3, axis=1))
    for bad in ([1.0, 2.0, 3.0], np.ones((2, 2)), np.ones((3, 2, 1))):  # [C] with C != K, wrong C, three axes
        with pytest.raises(ValueError, match="theta0"):
            f(bad, 3, 2)


# ---- the statistical yardstick -------------------------------------------------------------------------------------------
def test_two_block_problem_separates_the_blocks():
    """a condition on the problem, not a measurement: the block MLEs differ by at least a factor 2 and the single-theta MLE is
    outside both caps, so a kernel that applies one theta to all elements cannot pass"""
    prob = two_block_problem()
    mles = block_mles(prob)
    single = closed_form_mle(prob["y"], prob["sigma"])
    print("block MLEs", mles, "single-theta MLE", single)
    assert mles[1] >= 2 * mles[0]
    for k in range(2):
        assert abs(single - mles[k]) / mles[k] > 2 * GROUP_REL_DEV[k]  # (2 x: the margin the device test gets)
        assert abs(mles[k] - (5.0, 12.0)[k]) <= 4 * (5.0, 12.0)[k] / np.sqrt(np.diff(prob["bounds"])[k])


def test_host_loop_finds_the_block_mles():
    """the host loop over 8 seeds from theta_0 = 1 and, once, from theta_0 = 25: the largest relative deviation of block k
    from its closed-form MLE is GROUP_REL_DEV[k]"""
    prob = two_block_problem()
    mles = block_mles(prob)
    devs = []
    for seed in range(8):
        hat, trace = sapg_groups_np(prob, seed)
        assert np.all(trace[:prob["warmup"]] == prob["theta0"])  # the warm-up leaves theta alone
        devs.append((hat - mles) / mles)
    devs = np.array(devs)
    for k in range(2):
        print(f"block {k + 1}: MLE {mles[k]:.4f}; relative deviations:", ", ".join(f"{100 * d:+.3f} %" for d in devs[:, k]))
        worst = np.max(np.abs(devs[:, k]))
        assert worst <= GROUP_REL_DEV[k]
        assert worst >= GROUP_REL_DEV[k] / 2  # the pinned value is the measured one, not a loose cap
        assert devs[:, k].max() - devs[:, k].min() <= 4e-3  # bias, not noise
    far, _ = sapg_groups_np(prob, 0, theta0=25.0)
    print("from theta_0 = 25:", ", ".join(f"{100 * d:+.3f} %" for d in (far - mles) / mles))
    assert np.all(np.abs(far - mles) / mles <= GROUP_REL_DEV)
