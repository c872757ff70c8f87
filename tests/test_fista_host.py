"""Host model of the FISTA MAP estimator (pxmcmc_amd/optim.py, csrc/fista.hip): the numpy restatement of the iteration,
its closed forms, and the extended-precision yardstick of one step that tests/test_gpu_fista.py holds the kernel to.

    V = Y - gamma g;   X1 = soft(V, gamma T / lmda);   Y1 = X1 + beta (X1 - X0)

The numpy route below uses ``oracle.pxmcmc_np.soft``; nothing here runs the code under test except the momentum table
and the credible-region formula, which are host arithmetic."""
import numpy as np
import pytest

from oracle import pxmcmc_np

EPS = 2.0 ** -52
HAVE_LD = np.finfo(np.longdouble).eps < 1.1e-19  # x87 80-bit; otherwise mpmath at 40 digits, never a skip

# Largest error of the fp64 numpy route of one step against the extended-precision model, over every element of
# step_cases(), in units of 2^-52 S_e (test_numpy_route_against_extended_model measures it and holds it to this value).
# Observed: 1.3694 (complex128), 1.2622 (float64).
C0_MEASURED = 1.37


# ---- numpy model -------------------------------------------------------------------------------------------------
def beta_table(n, momentum=True):
    t = np.ones(n + 1)
    for k in range(n):
        t[k + 1] = (1 + np.sqrt(1 + 4 * t[k] ** 2)) / 2
    return (t[:-1] - 1) / t[1:] if momentum else np.zeros(n)


def fista_step_np(Y, g, X0, gamma, T, lmda, beta):
    """one step, fp64 numpy -> (X1, Y1)"""
    X1 = pxmcmc_np.soft(Y - gamma * g, gamma * T / lmda)
    return X1, X1 + beta * (X1 - X0)


def step_sums_np(X1, X0, T):
    """the three per-chain sums of the kernel, formed as it forms their terms: re^2 + im^2 with every product and sum
    rounded, |x| = sqrt(re^2 + im^2) (not hypot)"""
    abs2 = lambda z: np.real(z) ** 2 + np.imag(z) ** 2  # noqa: E731
    a2 = abs2(X1)
    return np.array([abs2(X1 - X0).sum(), a2.sum(), (T * np.sqrt(a2)).sum()])


def fista_np(grad, X0, gamma, T, lmda, tol, max_iter, momentum=True, objective=None):
    """the estimator's loop with a check at every iteration -> (X, iterations, objective trace, last two step lengths)"""
    beta = beta_table(max_iter, momentum)
    X, Y, trace, steps = X0, X0, [], [0.0, 0.0]
    for k in range(max_iter):
        X1, Y = fista_step_np(Y, grad(Y), X, gamma, T, lmda, beta[k])
        steps = [np.linalg.norm(X1 - X), steps[0]]
        X = X1
        if objective is not None:
            trace.append(objective(X))
        if steps[0] <= tol * np.linalg.norm(X):
            break
    return X, k + 1, np.array(trace), steps


# ---- extended-precision model of one step --------------------------------------------------------------------------
def fista_step_ext(Y, g, X0, gamma, T, lmda, beta):
    """(X1, Y1) of one step in extended precision, returned as (re, im) long double pairs (mpmath without an 80-bit type)"""
    if HAVE_LD:
        ld = np.longdouble
        f = lambda a: np.asarray(a, dtype=np.float64).astype(ld)  # noqa: E731
        yr, yi, gr, gi, xr, xi = (f(np.real(Y)), f(np.imag(Y)), f(np.real(g)), f(np.imag(g)), f(np.real(X0)), f(np.imag(X0)))
        vr, vi = yr - ld(gamma) * gr, yi - ld(gamma) * gi
        thr = ld(gamma) * f(T) / ld(lmda) + 0 * vr
        a = np.sqrt(vr * vr + vi * vi)
        s = np.where(a > thr, (a - thr) / np.where(a > 0, a, 1), 0)
        x1r, x1i = vr * s, vi * s
        return (x1r, x1i), (x1r + ld(beta) * (x1r - xr), x1i + ld(beta) * (x1i - xi))
    import mpmath

    mpmath.mp.dps = 40
    m = mpmath.mpf
    Tv = np.broadcast_to(np.asarray(T, dtype=float), np.shape(Y))
    out = [[], [], [], []]
    for y, gg, x0, t in zip(np.ravel(Y), np.ravel(g), np.ravel(X0), np.ravel(Tv)):
        vr, vi = m(float(np.real(y))) - m(gamma) * m(float(np.real(gg))), m(float(np.imag(y))) - m(gamma) * m(float(np.imag(gg)))
        thr = m(gamma) * m(float(t)) / m(lmda)
        a = mpmath.sqrt(vr * vr + vi * vi)
        s = (a - thr) / a if a > thr else m(0)
        x1r, x1i = vr * s, vi * s
        for o, v in zip(out, (x1r, x1i, x1r + m(beta) * (x1r - m(float(np.real(x0)))), x1i + m(beta) * (x1i - m(float(np.imag(x0)))))):
            o.append(v)
    arr = [np.array(o, dtype=object).reshape(np.shape(Y)) for o in out]
    return (arr[0], arr[1]), (arr[2], arr[3])


def error_scale(Y, g, X0, X1, gamma, T, lmda, beta):
    """S_e = |Y_e| + gamma |g_e| + gamma T_e / lmda + |beta| (|X1_e| + |X0_e|)"""
    return np.abs(Y) + gamma * np.abs(g) + gamma * T / lmda + abs(beta) * (np.abs(X1) + np.abs(X0))


def ratio_to_ext(got, ext, S):
    """largest |got - ext| over the elements in units of 2^-52 S_e (complex: the modulus of the difference)"""
    dr = np.array(np.real(got).astype(np.longdouble) - ext[0] if HAVE_LD else [float(a - b) for a, b in zip(np.ravel(np.real(got)), np.ravel(ext[0]))], dtype=float)
    di = np.array(np.imag(got).astype(np.longdouble) - ext[1] if HAVE_LD else [float(a - b) for a, b in zip(np.ravel(np.imag(got)), np.ravel(ext[1]))], dtype=float)
    return float(np.max(np.hypot(dr, di).reshape(-1) / (EPS * np.ravel(S))))


def step_inputs(n, C, cplx, vecT, seed):
    """inputs of one step for C chains of n elements: T has zeros (no shrink) and entries above every |V| (zero output);
    values near the threshold on both sides are included (the branch of the shrink)"""
    rng = np.random.default_rng(seed)
    draw = (lambda: rng.normal(size=(C, n)) + 1j * rng.normal(size=(C, n))) if cplx else (lambda: rng.normal(size=(C, n)))
    Y, g, X0 = draw(), draw() * 3.0, draw()
    gamma, lmda, beta = 0.37, 2.5e-2, 0.83
    if vecT:
        T = np.abs(rng.normal(size=n)) * lmda
        T[::5] = 0.0
        T[2::7] = 1e3
    else:
        T = 0.9 * lmda
    return Y, g, X0, gamma, T, lmda, beta


def step_cases():
    for cplx in (False, True):
        for vecT in (False, True):
            yield cplx, vecT, step_inputs(257, 3, cplx, vecT, seed=11 + 2 * cplx + vecT)


# ---- tests ---------------------------------------------------------------------------------------------------------------
def test_momentum_table_matches_the_recurrence():
    from pxmcmc_amd.optim import fista_momentum

    n = 200
    beta = beta_table(n)
    t = np.ones(n + 1)
    for k in range(n):
        t[k + 1] = (1 + np.sqrt(1 + 4 * t[k] ** 2)) / 2
    assert np.allclose(t[1:] * (t[1:] - 1), t[:-1] ** 2, rtol=8 * EPS, atol=0)  # t_{k+1}^2 - t_{k+1} = t_k^2
    assert beta[0] == 0.0 and np.all(np.diff(beta) > 0) and beta[-1] < 1.0
    assert np.all(t >= (np.arange(n + 1) + 2) / 2)  # Beck & Teboulle, lemma 4.3
    assert np.allclose(beta * t[1:], t[:-1] - 1, rtol=4 * EPS, atol=4 * EPS)
    assert np.array_equal(fista_momentum(n), beta)
    assert np.array_equal(beta_table(n, momentum=False), np.zeros(n))
    assert np.array_equal(fista_momentum(n, momentum=False), np.zeros(n))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("vecT", [False, True], ids=["scalarT", "vectorT"])
def test_identity_operator_closed_form(cplx, vecT):
    """identity operator, data d, variance sigma^2: L_g = 1 / sigma^2, and one step with gamma = sigma^2 from any start is
    soft(d, sigma^2 T / lmda); the next step does not move"""
    rng = np.random.default_rng(5)
    n, sigma, lmda = 64, 0.3, 1e-2
    draw = (lambda: rng.normal(size=n) + 1j * rng.normal(size=n)) if cplx else (lambda: rng.normal(size=n))
    d, X0 = draw(), draw() * 10
    T = np.abs(rng.normal(size=n)) * lmda if vecT else 0.5 * lmda
    grad = lambda X: (X - d) / sigma ** 2  # noqa: E731
    gamma = sigma ** 2
    beta = beta_table(2)
    X1, Y1 = fista_step_np(X0, grad(X0), X0, gamma, T, lmda, beta[0])
    want = pxmcmc_np.soft(d, sigma ** 2 * T / lmda)
    # V = Y - gamma ((Y - d) / sigma^2) = d up to four roundings of size eps (|Y| + |d|); the shrink is 1-Lipschitz and
    # adds three roundings of |V|
    bound = 8 * EPS * np.max(np.abs(X0) + np.abs(d))
    assert np.max(np.abs(X1 - want)) <= bound
    assert np.array_equal(Y1, X1)  # beta_0 = 0
    X2, _ = fista_step_np(Y1, grad(Y1), X1, gamma, T, lmda, beta[1])
    assert np.linalg.norm(X2 - X1) <= 2 * bound * np.sqrt(n)
    assert np.linalg.norm(X2 - X1) / np.linalg.norm(X2) <= 16 * EPS * np.sqrt(n) * np.max(np.abs(X0) + np.abs(d)) / np.linalg.norm(X2)


def _dense_problem(cplx):
    rng = np.random.default_rng(9)
    m, n, lmda = 40, 60, 1e-2
    draw = (lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)) if cplx else (lambda *s: rng.normal(size=s))
    A, d = draw(m, n), draw(m)
    w = 1 / (0.5 + rng.random(m)) ** 2  # diagonal inverse covariance
    T = lmda * (0.5 + rng.random(n)) * 5
    H = A.conj().T @ (w[:, None] * A)
    Lg = np.linalg.eigvalsh(H)[-1]
    grad = lambda X: A.conj().T @ (w * (A @ X - d))  # noqa: E731
    F = lambda X: 0.5 * np.real(np.vdot(A @ X - d, w * (A @ X - d))) + np.sum(T * np.abs(X)) / lmda  # noqa: E731
    return n, lmda, T, Lg, grad, F, draw


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_forward_backward_decreases_the_objective(cplx):
    n, lmda, T, Lg, grad, F, draw = _dense_problem(cplx)
    X0 = draw(n)
    _, _, trace, _ = fista_np(grad, X0, 1 / Lg, T, lmda, tol=0.0, max_iter=150, momentum=False, objective=F)
    full = np.concatenate([[F(X0)], trace])
    # monotone up to the rounding of F itself (a few hundred terms of size <= F: 1e3 eps F is generous and far below any step's decrease
    # that matters)
    assert np.all(np.diff(full) <= 1e3 * EPS * np.abs(full[:-1])), np.diff(full).max()
    assert full[-1] < full[0]


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_fista_fixed_point(cplx):
    """X* = soft(X* - gamma grad g(X*), gamma T / lmda) to the residual the stopping rule implies: the step map P is
    nonexpansive for gamma <= 1 / L_g and X_K = P(Y_{K-1}), Y_{K-1} = X_{K-1} + beta (X_{K-1} - X_{K-2}), so
    ||X_K - P(X_K)|| <= ||X_K - X_{K-1}|| + beta ||X_{K-1} - X_{K-2}|| <= tol ||X_K|| + ||X_{K-1} - X_{K-2}||"""
    n, lmda, T, Lg, grad, F, draw = _dense_problem(cplx)
    tol, gamma = 1e-9, 1 / Lg
    X, k, _, steps = fista_np(grad, draw(n), gamma, T, lmda, tol=tol, max_iter=20000)
    assert k < 20000 and steps[0] <= tol * np.linalg.norm(X)
    res = np.linalg.norm(X - pxmcmc_np.soft(X - gamma * grad(X), gamma * T / lmda))
    roundoff = 64 * EPS * (np.linalg.norm(X) + gamma * np.linalg.norm(grad(X)))
    assert res <= tol * np.linalg.norm(X) + steps[1] + roundoff, (res, steps)
    # and the point is a minimiser: forward-backward from it does not lower F beyond rounding
    X_fb, _, tr, _ = fista_np(grad, X, gamma, T, lmda, tol=0.0, max_iter=5, momentum=False, objective=F)
    assert F(X) - tr[-1] <= 1e-12 * abs(F(X))


def test_approx_credible_region_threshold():
    from pxmcmc_amd.uncertainty import approx_credible_region_threshold as thr

    for ndim, alpha, obj in ((100, 0.05, 12.5), (2 * 4096, 0.01, -3.0)):
        want = obj + ndim * (np.sqrt(16 * np.log(3 / alpha) / ndim) + 1)
        assert thr(obj, ndim, alpha) == pytest.approx(want, rel=4 * EPS)
    vals = [thr(0.0, 1000, a) for a in (0.01, 0.05, 0.2, 0.9)]
    assert np.all(np.diff(vals) < 0)  # a larger alpha is a smaller region
    assert thr(0.0, 1000) == thr(0.0, 1000, 0.05)
    lo = 4 * np.exp(-30 / 3)
    with pytest.raises(ValueError):
        thr(0.0, 30, lo * 0.99)
    with pytest.raises(ValueError):
        thr(0.0, 30, 1.0)
    assert np.isfinite(thr(0.0, 30, lo * 1.01))
    assert np.array_equal(thr(np.array([1.0, 2.0]), 100, 0.05), np.array([1.0, 2.0]) + (thr(0.0, 100, 0.05)))


def test_numpy_route_against_extended_model():
    """the yardstick of the GPU test: how far the fp64 numpy route of one step is from the extended-precision model, per
    element, in units of 2^-52 S_e -- measured here, pinned as C0_MEASURED"""
    worst = {}
    for cplx, vecT, (Y, g, X0, gamma, T, lmda, beta) in step_cases():
        X1, Y1 = fista_step_np(Y, g, X0, gamma, T, lmda, beta)
        eX, eY = fista_step_ext(Y, g, X0, gamma, T, lmda, beta)
        S = error_scale(Y, g, X0, X1, gamma, T, lmda, beta)
        r = max(ratio_to_ext(X1, eX, S), ratio_to_ext(Y1, eY, S))
        worst[cplx] = max(worst.get(cplx, 0.0), r)
        if vecT:  # the cases have what they are meant to have
            assert np.any(X1 == 0) and np.any(X1 != 0) and np.all(X1[:, 2::7] == 0)
    print("fp64 numpy route vs extended model, units of 2^-52 S_e:", worst)
    assert max(worst.values()) <= C0_MEASURED
    assert max(worst.values()) >= C0_MEASURED / 4  # the pinned value is the measured one, not a loose cap
