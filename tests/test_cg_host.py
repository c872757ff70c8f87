"""The numpy statement of the Gaussian posterior's solver (pxmcmc_amd/cg_np.py) on dense systems, without a GPU: the
two-launch recurrences against numpy.linalg.solve, the freeze and the breakdown guard, the construction of the exact draws,
the assignment of the Philox deviates, the prior, and the sharpness of the extended-precision model's bounds."""
import numpy as np
import pytest

from pxmcmc_amd import cg_np

N = 64


def _system(cplx, seed=0, ndata=96):
    """random Hermitian positive-definite H = D + Phi^H W Phi, n = 64: a third of W is zero, D spans 1 to 1e6"""
    rng = np.random.default_rng(seed)
    Phi = rng.normal(size=(ndata, N)) + (1j * rng.normal(size=(ndata, N)) if cplx else 0)
    w = rng.uniform(0.5, 2.0, size=ndata)
    w[rng.permutation(ndata)[: ndata // 3]] = 0.0
    D = 10.0 ** rng.uniform(0, 6, size=N)
    A = Phi.conj().T @ (w[:, None] * Phi)
    b = rng.normal(size=N) + (1j * rng.normal(size=N) if cplx else 0)
    return Phi, w, D, A, b


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("precond", [False, True], ids=["plain", "diag"])
def test_recurrences_against_dense_solve(cplx, precond):
    """pcg_np reaches tol = 1e-10: the true residual within 2 tol and the solution within cond(M^-1/2 H M^-1/2) 2 tol"""
    Phi, w, D, A, b = _system(cplx)
    H = np.diag(D) + A
    minv = 1.0 / (D + np.trace(A).real / N) if precond else 1.0
    tol = 1e-10
    x, info = cg_np.pcg_np(A, D, b, minv=minv, tol=tol, max_iter=2000)
    assert info["frozen"] and not info["breakdown"], info
    if precond:
        assert info["niter"] <= 40, info["niter"]  # (D spans six decades: without M the count is in the hundreds)
    xs = np.linalg.solve(H, b)
    assert np.linalg.norm(b - H @ x) <= 2 * tol * np.linalg.norm(b)
    assert np.linalg.norm(x - xs) <= np.linalg.cond(H) * 2 * tol * np.linalg.norm(xs)
    assert x.dtype == b.dtype


def test_converged_start_freezes_at_once():
    Phi, w, D, A, b = _system(True, seed=1)
    H = np.diag(D) + A
    x0 = np.linalg.solve(H, b)
    x, info = cg_np.pcg_np(A, D, H @ x0, x0=x0, minv=1.0 / D, tol=1e-8)
    assert info["frozen"] and not info["breakdown"] and info["niter"] == 0
    assert np.array_equal(x, x0)


def test_indefinite_system_breaks_down_without_nan():
    Phi, w, D, A, b = _system(False, seed=2)
    D = -D  # H = A - |D|: indefinite
    x, info = cg_np.pcg_np(A, D, b, tol=1e-12, max_iter=500)
    assert info["frozen"] and info["breakdown"], info
    assert np.all(np.isfinite(x))


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_draw_factor_covariance(cplx):
    """G = [Phi^H sqrt(W), sqrt(D)]: G G^H = H to round-off, masked rows included; and the right-hand side the solver forms
    through calc_gradg(data + s o omega_1) is b0 + G omega"""
    Phi, w, D, A, b0 = _system(cplx, seed=3)
    H = np.diag(D) + A
    G = cg_np.draw_factor_np(Phi, w, D)
    assert (w == 0).sum() >= len(w) // 3
    assert np.abs(G @ G.conj().T - H).max() <= 64 * 2.0 ** -52 * np.abs(H).max()
    rng = np.random.default_rng(4)
    o1 = rng.normal(size=len(w)) + (1j * rng.normal(size=len(w)) if cplx else 0)
    o2 = rng.normal(size=N) + (1j * rng.normal(size=N) if cplx else 0)
    rhs = cg_np.draw_rhs_np(Phi, w, D, b0, o1, o2)
    want = b0 + G @ np.concatenate([o1, o2])
    assert np.abs(rhs - want).max() <= 256 * 2.0 ** -52 * np.abs(want).max()


def test_deviate_assignment():
    """draw k of chain c: omega_1 from iteration 2 k, omega_2 from 2 k + 1 of the stream (seed, chain_offset + c); distinct
    draws and chains get distinct deviates"""
    from oracle import philox

    assert [cg_np.draw_iterations(k) for k in range(3)] == [(0, 1), (2, 3), (4, 5)]
    seed, off = 7, 3
    seen = []
    for k in range(2):
        for c in range(2):
            it1, it2 = cg_np.draw_iterations(k)
            o1 = philox.randn_complex(5, seed, off + c, it1, bits=64)
            o2 = philox.randn_complex(9, seed, off + c, it2, bits=64)
            assert np.array_equal(o1, philox.randn_complex(5, seed, off + c, 2 * k, bits=64))
            assert np.array_equal(o2, philox.randn_complex(9, seed, off + c, 2 * k + 1, bits=64))
            assert not np.array_equal(o1, o2[:5])
            seen.append(o1)
    for i in range(len(seen)):
        for j in range(i):
            assert not np.array_equal(seen[i], seen[j])


def test_gaussian_prox_and_power_spectrum():
    from pxmcmc_amd.prior import Gaussian

    rng = np.random.default_rng(5)
    z, p, T = rng.normal(size=8), rng.uniform(0, 3, size=8), 0.7
    x = cg_np.gauss_prox_np(z, p, T)
    f = lambda v: 0.5 * (v - z) ** 2 + T * 0.5 * p * v ** 2  # noqa: E731
    for h in (1e-3, -1e-3):
        assert np.all(f(x) <= f(x + h))
    assert np.allclose((x - z) + T * p * x, 0.0, atol=1e-15)  # the stationarity condition
    L = 4
    cl = np.array([2.0, 4.0, 8.0, 16.0])
    g = Gaussian.from_power_spectrum(cl, L, 0.5)
    assert g.T == 0.5 and g.precision.shape == (L * L,)
    for el in range(L):
        for m in range(-el, el + 1):
            assert g.precision[el * el + el + m] == 1.0 / cl[el]
    assert np.array_equal(g.precision, cg_np.power_spectrum_precision_np(cl, L))
    with pytest.raises(ValueError, match="C_l must be positive"):
        Gaussian.from_power_spectrum([1.0, 0.0, 1.0, 1.0], L, 0.5)
    with pytest.raises(ValueError):
        Gaussian(-1.0, 0.5)
    with pytest.raises(ValueError):
        Gaussian(np.array([1.0, -2.0]), 0.5)


def _iteration_state(cplx):
    """arrays in the middle of a solve (after three iterations), one chain"""
    Phi, w, D, A, b = _system(cplx, seed=6)
    minv = 1.0 / (D + 1.0)
    x = np.zeros_like(b)
    r, u = b.copy(), minv * b
    p, s = np.zeros_like(b), np.zeros_like(b)
    row = cg_np.new_coef(float(np.sum(np.abs(b) ** 2)))
    b0 = 0.1 * b
    for _ in range(3):
        q = A @ u - b0
        wv, sums = cg_np.cg_apply_np(u, q, b0, D, r)
        row = cg_np.cg_decide_np(row, sums, 1e-12)
        p, s, x, r, u = cg_np.cg_update_np(u, wv, p, s, x, r, minv, row)
    return A, D, b0, minv, u, p, s, x, r, row


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_model_accepts_float64_and_rejects_wrong_recurrences(cplx):
    """the float64 statement is within the extended-precision model's bounds; each deliberate error is outside them"""
    A, D, b0, minv, u, p, s, x, r, row = _iteration_state(cplx)
    q = A @ u - b0
    w, sums = cg_np.cg_apply_np(u, q, b0, D, r)
    w_ld, w_bound = cg_np.cg_apply_ld(u, q, b0, D, r)
    assert cg_np.within(w, w_ld, w_bound)
    assert not cg_np.within(D * u + q, w_ld, w_bound)  # w without b0
    sums_ld, sums_bound = cg_np.cg_sums_ld(u, w, r)
    assert all(abs(a - b) <= c for a, b, c in zip(sums, sums_ld, sums_bound))
    new = cg_np.cg_decide_np(row, sums, 1e-12)
    new_ld, coef_bound = cg_np.cg_decide_ld(row, sums, 1e-12)
    assert np.all(np.abs(new - new_ld) <= coef_bound)
    assert abs(row[cg_np.ALPHA] - new_ld[cg_np.ALPHA]) > coef_bound[cg_np.ALPHA]  # alpha taken from the previous iteration
    outs = cg_np.cg_update_np(u, w, p, s, x, r, minv, new)
    outs_ld, bounds = cg_np.cg_update_ld(u, w, p, s, x, r, minv, new)
    for got, want, bound in zip(outs, outs_ld, bounds):
        assert cg_np.within(got, want, bound)
    no_beta = np.array(new)
    no_beta[cg_np.BETA] = 0.0  # a dropped beta term
    bad = cg_np.cg_update_np(u, w, p, s, x, r, minv, no_beta)
    assert not cg_np.within(bad[0], outs_ld[0], bounds[0]) and not cg_np.within(bad[2], outs_ld[2], bounds[2])
    stale = np.array(new)
    stale[cg_np.ALPHA] = row[cg_np.ALPHA]
    bad = cg_np.cg_update_np(u, w, p, s, x, r, minv, stale)
    assert not cg_np.within(bad[2], outs_ld[2], bounds[2]) and not cg_np.within(bad[3], outs_ld[3], bounds[3])
    # a converged chain must freeze: the model returns it as it is with zero bounds, an update that moves it is outside
    done = cg_np.cg_decide_np(row, (sums[0], sums[1], 0.0), 1e-12)
    assert done[cg_np.FLAGS] == cg_np.FROZEN and done[cg_np.ALPHA] == 0 and done[cg_np.BETA] == 0
    kept, zero = cg_np.cg_update_ld(u, w, p, s, x, r, minv, done)
    unfrozen = np.array(done)
    unfrozen[cg_np.FLAGS] = 0
    moved = cg_np.cg_update_np(u, w, p, s, x, r, minv, unfrozen)  # alpha = beta = 0 but not frozen: p <- u, s <- w
    assert cg_np.within(x, kept[2], zero[2]) and cg_np.within(p, kept[0], zero[0])
    assert not cg_np.within(moved[0], kept[0], zero[0])
