"""The analysis-setting solvers on the host (numpy only): pxmcmc_amd.optim_np -- the primal-dual iteration, the exact analysis
prox and the duality gap -- against optimality conditions, closed forms and the synthesis-setting forward-backward iteration
of tests/test_fista_host.py; and the long-double element models and planted inputs that tests/test_gpu_pd.py holds the two
HIP step kernels to."""
import numpy as np
import pytest

from pxmcmc_amd.optim_np import analysis_prox_np, duality_gap_np, pd_dual_np, pd_primal_np, primal_dual_np
from test_fista_host import fista_np

EPS = 2.0 ** -52
LD = np.longdouble
assert np.finfo(LD).eps < 1.1e-19, "the element models need an extended long double"


def soft_np(x, t):
    a = np.abs(x)
    return np.where(a > t, x * (1 - t / np.where(a > 0, a, 1)), 0)


# ---- long-double element models of the two kernels (tests/test_gpu_pd.py) ------------------------------------------------------
def _parts(a):
    """the real components of an array as long doubles (complex: re, im interleaved along the last axis)"""
    a = np.ascontiguousarray(a)
    return (a.view(np.float64) if np.iscomplexobj(a) else a).astype(LD)


def pd_primal_ext(X, G, U, tau):
    """(X1, Xbar) per real component in long double: x1 = x - tau (g + u), xbar = 2 x1 - x"""
    x, g, u = _parts(X), _parts(G), _parts(U)
    x1 = x - LD(tau) * (g + u)
    return x1, 2 * x1 - x


def pd_dual_ext(V, W, T, sigma, rscale):
    """the projection of v + sigma w onto |.| <= T rscale in long double -> (re, im, |w|, r); im is None for real input"""
    T = np.broadcast_to(np.asarray(T, dtype=float), np.shape(V)).astype(LD)
    r = T * LD(rscale)
    if not np.iscomplexobj(V):
        w = np.asarray(V).astype(LD) + LD(sigma) * np.asarray(W).astype(LD)
        return np.minimum(np.maximum(w, -r), r), None, np.abs(w), r
    wr = V.real.astype(LD) + LD(sigma) * W.real.astype(LD)
    wi = V.imag.astype(LD) + LD(sigma) * W.imag.astype(LD)
    a = np.sqrt(wr * wr + wi * wi)
    s = np.where(a > r, r / np.where(a > 0, a, 1), LD(1))
    return wr * s, wi * s, a, r


# sigma and rscale of the planted dual inputs: powers of two, so the planted elements are exact
PD_SIGMA, PD_RSCALE, PD_TSCALAR = 0.5, 0.5, 10.0


def pd_dual_inputs(n, C, cplx, vecT, seed):
    """(V, W, T) with |v + sigma w| spread around r = T rscale (~ 5), and, for n >= 8, planted elements by position i mod 8:
    1: on the disc exactly (w = (3, 4), r = 5; real: w = 5), 2: w = 0, 3: T_i = 0 (vector T only), 4: far outside,
    5: well inside"""
    rng = np.random.default_rng(seed)
    draw = (lambda: rng.normal(size=(C, n)) + 1j * rng.normal(size=(C, n))) if cplx else (lambda: rng.normal(size=(C, n)))
    V, W = 3.0 * draw(), 6.0 * draw()
    T = PD_TSCALAR * (0.5 + rng.random(n)) if vecT else PD_TSCALAR
    if n >= 8:
        i = np.arange(n) % 8
        V[:, i == 1], W[:, i == 1] = 0, (6 + 8j if cplx else 10)
        V[:, i == 2], W[:, i == 2] = 0, 0
        V[:, i == 4] *= 100
        V[:, i == 5] *= 1e-3
        W[:, i == 5] *= 1e-3
        if vecT:
            T[i == 1] = PD_TSCALAR
            T[i == 3] = 0
    return V, W, T


# ---- pd_dual_np: the edge elements ----------------------------------------------------------------------------------------------
def test_dual_step_edge_elements():
    """|w| = r exactly and w = 0 are kept, T_i = 0 gives 0, r = inf never binds; a point outside lands on the disc"""
    v = np.zeros(5, dtype=complex)
    w = np.array([6 + 8j, 0, 1 - 2j, 1e150 + 1e150j, 30 + 40j])
    T = np.array([10.0, 10.0, 0.0, np.inf, 10.0])
    out = pd_dual_np(v, w, T, 0.5, 0.5)
    assert out[0] == 3 + 4j and out[1] == 0 and out[2] == 0 and out[3] == 0.5 * w[3]
    assert abs(abs(out[4]) - 5) <= 4 * EPS * 5 and abs(out[4] / abs(out[4]) - (0.6 + 0.8j)) <= 4 * EPS
    outr = pd_dual_np(np.zeros(5), np.array([10.0, 0.0, -3.0, -1e150, -70.0]), T, 0.5, 0.5)
    assert np.array_equal(outr, [5.0, 0.0, 0.0, -5e149, -5.0])
    x1, xbar = pd_primal_np(np.array([1.0, 2.0]), np.array([0.5, -1.0]), np.array([0.5, 3.0]), 0.25)
    assert np.array_equal(x1, [0.75, 1.5]) and np.array_equal(xbar, [0.5, 1.0])


# ---- primal_dual_np on a dense complex problem --------------------------------------------------------------------------------
def _dense_problem(ndata=30, unitary=False, seed=7):
    """n = 48 unknowns, m = 120 analysis coefficients (48 with a unitary A), ndata complex data with a diagonal real inverse
    covariance"""
    rng = np.random.default_rng(seed)
    n, m = 48, 120
    cn = lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)  # noqa: E731
    Phi = cn(ndata, n) / np.sqrt(n)
    A = np.linalg.qr(cn(n, n))[0] if unitary else cn(m, n) / np.sqrt(n)
    ic = 1.0 / (0.1 * (1 + rng.random(ndata))) ** 2
    x_true = np.where(rng.random(n) < 0.3, cn(n), 0)
    d = Phi @ x_true + cn(ndata) * 0.05
    lmda = 1e-2
    T = lmda * 2.0 * (0.5 + rng.random(A.shape[0]))
    H = Phi.conj().T @ (ic[:, None] * Phi)
    b = Phi.conj().T @ (ic * d)
    L_g = np.linalg.eigvalsh(H)[-1]
    A2 = np.linalg.norm(A, 2) ** 2
    sigma = 0.5 * L_g / A2  # balance = 1
    tau = 1.0 / (0.5 * L_g + sigma * A2)
    return dict(n=n, Phi=Phi, A=A, ic=ic, d=d, lmda=lmda, T=T, H=H, b=b, L_g=L_g, A2=A2, sigma=sigma, tau=tau,
                grad=lambda x: H @ x - b, Af=lambda x: A @ x, AHf=lambda v: A.conj().T @ v)


PD_DENSE_ITERS = 10000  # limit; the run below needs 2472 for 1e-10 (printed)


def test_primal_dual_meets_the_optimality_conditions():
    """At the stopping rule 1e-10: v is feasible; the residual of 0 = gradg(x) + A^H v obeys the bound that follows from
    x1 = x - tau (gradg(x) + A^H v): gradg(x1) + A^H v1 = -dx / tau + (gradg(x1) - gradg(x)) + A^H (v1 - v), so its norm
    is at most (1 / tau + L_g) ||dx|| + ||A|| ||dv||; and where (A x)_i is not zero, v_i sits on its disc in the direction
    of (A x)_i."""
    p = _dense_problem()
    x, v, info = primal_dual_np(p["grad"], p["Af"], p["AHf"], p["T"], p["lmda"], p["tau"], p["sigma"], np.zeros(p["n"], complex),
                                PD_DENSE_ITERS, tol=1e-10)
    print(f"dense problem: {info['niter']} iterations for 1e-10, ||dx|| = {info['dx']:.3e}, ||dv|| = {info['dv']:.3e}")
    assert info["converged"]
    r = p["T"] / p["lmda"]
    assert np.all(np.abs(v) <= r * (1 + 4 * EPS))
    An = np.sqrt(p["A2"])
    bound = (1 / p["tau"] + p["L_g"]) * info["dx"] + An * info["dv"]
    res = np.linalg.norm(p["grad"](x) + p["AHf"](v))
    print(f"||gradg + A^H v|| = {res:.3e}, bound {bound:.3e}")
    assert res <= bound
    u = p["Af"](x)
    on = np.abs(u) > 1e-8 * np.abs(u).max()
    dev = np.linalg.norm(v[on] - r[on] * u[on] / np.abs(u[on]))
    print(f"{on.sum()} of {u.size} coefficients are non-zero; ||v - (T / lmda) sign(A x)|| on them = {dev:.3e}, bound {bound / An:.3e}")
    assert 0 < on.sum() < u.size
    assert dev <= bound / An


def _quadratic_gap(p, x, v):
    """P(x) - D(v) for g(x) = 1/2 x^H H x - Re<b, x> + const with H invertible: g^*(y) = 1/2 (y + b)^H H^-1 (y + b) - const,
    D(v) = -g^*(-A^H v) on the feasible set (v is projected onto it first)"""
    v = pd_dual_np(np.zeros_like(v), v, p["T"], 1.0, 1.0 / p["lmda"])
    const = 0.5 * np.sum(p["ic"] * np.abs(p["d"]) ** 2)
    y = p["b"] - p["AHf"](v)
    dual = const - 0.5 * np.vdot(y, np.linalg.solve(p["H"], y)).real
    primal = 0.5 * np.vdot(x, p["H"] @ x).real - np.vdot(p["b"], x).real + const + np.sum(p["T"] * np.abs(p["Af"](x))) / p["lmda"]
    return primal - dual


def test_unitary_analysis_equals_synthesis():
    """With A unitary, c = A x turns the problem into the synthesis problem on Phi A^H, which forward-backward splitting
    solves.  64 data make H = Phi^H C^-1 Phi positive definite (smallest eigenvalue mu), so P is mu-strongly convex and each
    point is within sqrt(2 gap / mu) of the minimiser, gap the duality gap with any feasible dual: v of the primal-dual run,
    and -A gradg(x) (projected) for the forward-backward point."""
    p = _dense_problem(ndata=64, unitary=True)
    A, n = p["A"], p["n"]
    x, v, info = primal_dual_np(p["grad"], p["Af"], p["AHf"], p["T"], p["lmda"], p["tau"], p["sigma"], np.zeros(n, complex), 20000,
                                tol=1e-13)
    c = fista_np(lambda c: A @ p["grad"](A.conj().T @ c), np.zeros(n, complex), 1.0 / p["L_g"], p["T"], p["lmda"], 1e-13, 20000,
                    momentum=False)[0]
    xs = A.conj().T @ c
    mu = np.linalg.eigvalsh(p["H"])[0]
    gaps = _quadratic_gap(p, x, v), _quadratic_gap(p, xs, -(A @ p["grad"](xs)))
    # the gaps are differences of values of size P: their own rounding, 64 eps P, is added
    P = abs(0.5 * np.sum(p["ic"] * np.abs(p["d"]) ** 2))
    bound = sum(np.sqrt(2 * (max(g, 0) + 64 * EPS * P) / mu) for g in gaps)
    dist = np.linalg.norm(x - xs)
    print(f"unitary A: {info['niter']} primal-dual iterations, gaps {gaps[0]:.3e} {gaps[1]:.3e}, mu = {mu:.3e}, "
          f"||x_pd - A^H c_fb|| = {dist:.3e}, bound {bound:.3e}, ||x|| = {np.linalg.norm(x):.3e}")
    assert info["converged"] and mu > 0
    assert dist <= bound and bound <= 1e-5 * np.linalg.norm(x)


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_identity_case_against_the_closed_form(cplx):
    """A = I, identity measurement: the minimiser is soft(d, T sigma_d^2 / lmda), and the iterate is within sqrt(2 gap / ic)
    of it (the problem is ic-strongly convex)"""
    rng = np.random.default_rng(3)
    n, ic, lmda = 190, 1 / 0.2 ** 2, 1e-2
    d = rng.normal(size=n) + (1j * rng.normal(size=n) if cplx else 0)
    T = lmda * 10.0 * rng.random(n)
    ident = lambda a: a  # noqa: E731
    sigma = 0.5 * ic
    tau = 1.0 / (0.5 * ic + sigma)
    x, v, info = primal_dual_np(lambda x: ic * (x - d), ident, ident, T, lmda, tau, sigma, np.zeros_like(d), 5000, tol=1e-10)
    want = soft_np(d, T / (lmda * ic))
    gap = duality_gap_np(x, v, d, np.full(n, ic), ident, ident, T, lmda)
    P = 0.5 * ic * np.sum(np.abs(d) ** 2)
    bound = np.sqrt(2 * (max(gap, 0) + 64 * EPS * P) / ic)
    print(f"identity case: {info['niter']} iterations, gap {gap:.3e}, ||x - soft|| = {np.linalg.norm(x - want):.3e}, bound {bound:.3e}")
    assert info["converged"] and gap >= -64 * EPS * P
    assert np.linalg.norm(x - want) <= bound <= 1e-6 * np.linalg.norm(want)
    assert 0 < np.count_nonzero(want) < n


# ---- analysis_prox_np -----------------------------------------------------------------------------------------------------------
def _prox_objective(A, T, Z, p):
    return 0.5 * np.linalg.norm(p - Z) ** 2 + np.sum(T * np.abs(A @ p))


def test_analysis_prox_identity_is_the_soft_threshold():
    rng = np.random.default_rng(4)
    Z = rng.normal(size=64) + 1j * rng.normal(size=64)
    T = rng.random(64)
    ident = lambda a: a  # noqa: E731
    p = analysis_prox_np(ident, ident, T, Z, 1, 1.0)
    assert np.abs(p - soft_np(Z, T)).max() <= 4 * EPS * np.abs(Z).max()
    assert np.abs(analysis_prox_np(ident, ident, T, Z, 7, 1.0) - p).max() <= 4 * EPS * np.abs(Z).max()  # already the fixed point


def test_analysis_prox_on_a_dense_operator():
    """||Z - A^H v_k|| does not increase with k (projected gradient on the dual objective 1/2 ||Z - A^H v||^2 with a step
    1 / ||A||^2 is a descent method), and after 2000 iterations the prox objective is below that of Z itself and of the
    tight-frame formula Z + A^H (soft(A Z) - A Z), which is not the prox for this A"""
    pr = _dense_problem()
    A = pr["A"]
    rng = np.random.default_rng(5)
    Z = rng.normal(size=pr["n"]) + 1j * rng.normal(size=pr["n"])
    T = 0.05 * (0.5 + rng.random(A.shape[0]))
    sigma = 1.0 / (pr["A2"] * (1 + 1e-4))
    norms = []
    for k in (0, 1, 2, 4, 8, 16, 32, 64, 2000):
        p, v = analysis_prox_np(pr["Af"], pr["AHf"], T, Z, k, sigma, return_dual=True)
        assert np.all(np.abs(v) <= T * (1 + 4 * EPS))
        norms.append(np.linalg.norm(p))
    print("||Z - A^H v_k||:", norms)
    assert np.all(np.diff(norms) <= 8 * EPS * norms[0]) and norms[-1] < norms[0]
    a = A @ Z
    tight = Z + A.conj().T @ (soft_np(a, T) - a)
    F = [_prox_objective(A, T, Z, q) for q in (Z, tight, p)]
    print(f"prox objective: Z {F[0]:.6f}, tight-frame formula {F[1]:.6f}, 2000 dual iterations {F[2]:.6f}")
    assert F[2] < F[0] and F[2] < F[1]
    # p is the minimiser: its objective equals the dual value 1/2 ||Z||^2 - 1/2 ||Z - A^H v||^2 up to the remaining gap
    dual = 0.5 * np.linalg.norm(Z) ** 2 - 0.5 * np.linalg.norm(p) ** 2
    assert 0 <= F[2] - dual + 64 * EPS * F[0] and F[2] - dual <= 1e-6 * F[2]
