"""Host model of FISTA with adaptive (gradient) restart (O'Donoghue & Candes, Found. Comput. Math. 15, 2015) as
pxm_fista_step_restart and ``FISTA(restart="gradient")`` define it: the numpy restatement of the loop, with the delayed
decision of the device, and the properties the device is held to in tests/test_gpu_fista_restart.py.

Per chain, with momentum index k_c (from 0) and restart count R_c:

    beta = beta_table[min(k_c, n_beta - 1)]
    X1   = soft(Y - gamma grad g(Y), gamma T / lmda);   Y1 = X1 + beta (X1 - X0)
    r    = sum_i Re(conj(Y_i - X1_i) (X1_i - X0_i))
    restart enabled and r > 0:  k_c <- 0, R_c <- R_c + 1     else:  k_c <- k_c + 1

The decision is known only after the pass that wrote Y1, so Y1 keeps its momentum and the reset acts on the following step,
which runs with beta_0 = 0."""
import numpy as np
import pytest

from oracle import pxmcmc_np
from test_fista_host import EPS, _dense_problem, beta_table, fista_np, fista_step_np


def restart_terms_np(Y, X1, X0):
    """the terms of r as the kernel forms them: (y.re - x1.re) d.re + (y.im - x1.im) d.im with d = x1 - x0, every operation
    rounded (real input: the first product alone)"""
    d = X1 - X0
    if np.iscomplexobj(d):
        return (np.real(Y) - np.real(X1)) * np.real(d) + (np.imag(Y) - np.imag(X1)) * np.imag(d)
    return (Y - X1) * d


def fista_restart_np(grad, X0, gamma, T, lmda, tol, max_iter, restart=True, objective=None):
    """the estimator's loop with a check at every iteration -> (X, iterations, objective trace, last two step lengths, log);
    ``log`` has one row per iteration: (momentum index used, beta used, restarted after it, max |Y - X| of the point it
    started from)"""
    beta = beta_table(max_iter)
    X, Y, trace, steps, log = X0, X0, [], [0.0, 0.0], []
    k_c = 0
    for it in range(max_iter):
        b = beta[min(k_c, len(beta) - 1)]
        gap = float(np.max(np.abs(Y - X)))
        X1, Y1 = fista_step_np(Y, grad(Y), X, gamma, T, lmda, b)
        r = restart_terms_np(Y, X1, X).sum()
        restarted = bool(restart and r > 0)  # False for r == 0 and for NaN
        log.append((k_c, b, restarted, gap))
        k_c = 0 if restarted else k_c + 1
        steps = [np.linalg.norm(X1 - X), steps[0]]
        X, Y = X1, Y1
        if objective is not None:
            trace.append(objective(X))
        if steps[0] <= tol * np.linalg.norm(X):
            break
    return X, it + 1, np.array(trace), steps, log


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_disabled_restart_is_plain_fista(cplx):
    n, lmda, T, Lg, grad, F, draw = _dense_problem(cplx)
    X0 = draw(n)
    want = fista_np(grad, X0, 1 / Lg, T, lmda, tol=1e-6, max_iter=3000, objective=F)
    got = fista_restart_np(grad, X0, 1 / Lg, T, lmda, tol=1e-6, max_iter=3000, restart=False, objective=F)
    assert got[1] == want[1] and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and got[3] == want[3]
    assert [row[0] for row in got[4]] == list(range(got[1])) and not any(row[2] for row in got[4])


@pytest.fixture(scope="module", params=[False, True], ids=["real", "complex"])
def dense_runs(request):
    """the plain and the restarted run of the dense problem at tol = 1e-9, computed once"""
    n, lmda, T, Lg, grad, F, draw = _dense_problem(request.param)
    X0 = draw(n)
    tol, gamma = 1e-9, 1 / Lg
    plain = fista_np(grad, X0, gamma, T, lmda, tol=tol, max_iter=20000)
    fast = fista_restart_np(grad, X0, gamma, T, lmda, tol=tol, max_iter=20000)
    return dict(problem=(n, lmda, T, Lg, grad, F, draw), tol=tol, gamma=gamma, plain=plain, fast=fast)


def test_restart_halves_the_iterations_at_least(dense_runs):
    r = dense_runs
    n, lmda, T, Lg, grad, F, draw = r["problem"]
    Xp, kp, _, _ = r["plain"]
    Xr, kr, _, steps, log = r["fast"]
    nrestarts = sum(row[2] for row in log)
    print(f"tol {r['tol']}: plain {kp} iterations, restarted {kr} ({kr / kp:.3f}), {nrestarts} restarts; "
          f"F plain {F(Xp):.12e}, restarted {F(Xr):.12e}")
    assert kp < 20000 and kr < 20000
    assert steps[0] <= r["tol"] * np.linalg.norm(Xr)  # the rule is met
    assert 2 * kr <= kp
    assert nrestarts > 0
    assert abs(F(Xr) - F(Xp)) <= 1e-12 * abs(F(Xp))


def test_restarted_point_is_a_fixed_point(dense_runs):
    """the assertion of test_fista_host.test_fista_fixed_point on the restarted run's point: beta <= 1 holds with restart too"""
    r = dense_runs
    n, lmda, T, Lg, grad, F, draw = r["problem"]
    tol, gamma = r["tol"], r["gamma"]
    X, k, _, steps, _ = r["fast"]
    assert k < 20000 and steps[0] <= tol * np.linalg.norm(X)
    res = np.linalg.norm(X - pxmcmc_np.soft(X - gamma * grad(X), gamma * T / lmda))
    roundoff = 64 * EPS * (np.linalg.norm(X) + gamma * np.linalg.norm(grad(X)))
    assert res <= tol * np.linalg.norm(X) + steps[1] + roundoff, (res, steps)
    X_fb, _, tr, _ = fista_np(grad, X, gamma, T, lmda, tol=0.0, max_iter=5, momentum=False, objective=F)
    assert F(X) - tr[-1] <= 1e-12 * abs(F(X))


def test_step_after_a_restart_has_no_momentum_and_the_step_after_that_never_restarts(dense_runs):
    """A restart decided at step k makes step k + 1 run with beta_0 = 0, so Y_{k+2} = X_{k+2}, and step k + 2 then has
    r = <X_{k+2} - X_{k+3}, X_{k+3} - X_{k+2}> = -sum |X_{k+3} - X_{k+2}|^2 <= 0: a step that starts from Y = X never
    restarts.  Step k + 1 itself still starts from the Y_{k+1} that kept its momentum, so its r can be positive: with the
    delayed decision the restarts of this problem come in pairs (k, k + 1) -- 7 pairs are the 14 restarts of both runs --
    and never three in a row.  The second of a pair only repeats the reset (the index is 0 already and stays 0)."""
    log = dense_runs["fast"][4]
    rs = [i for i, row in enumerate(log) if row[2]]
    assert rs, "no restart to look at"
    for i in rs:
        if i + 1 < len(log):
            k_c, b, _, _ = log[i + 1]
            assert k_c == 0 and b == 0.0  # the step after a restart runs with beta_0
        if i + 2 < len(log):
            assert log[i + 2][3] == 0.0  # and leaves Y = X: the step after that one starts from it
    for prev, row in zip(log[:-1], log[1:]):
        if prev[1] == 0.0:  # after a step with beta = 0 (the first step of the run included)
            assert row[3] == 0.0 and not row[2]
    assert not any(i + 1 in rs and i + 2 in rs for i in rs)
    print("restarts at iterations", rs)


def test_decision_is_false_for_zero_and_nan():
    """r > 0 as the loop takes it: the index advances at r == 0 and at NaN"""
    for r in (0.0, -0.0, float("nan"), -1.0):
        assert not (r > 0)
    assert 2.0 ** -1000 > 0
