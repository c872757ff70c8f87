"""Total variation on the MW grid on the host (numpy only): pxmcmc_amd.tv_np -- the discrete gradient and its adjoint, the TV
value, the pair projection and the pair forms of the primal-dual iteration, the exact prox and the duality gap -- against
adjointness, closed forms and optimality conditions; and the problems, long-double models and planted inputs that
tests/test_gpu_tv.py holds the HIP kernels of csrc/tv.hip to.  Ring weights come from oracle.pxmcmc_np.mw_map_weights."""
import numpy as np
import pytest

from oracle import pxmcmc_np as ref
from pxmcmc_amd.tv_np import (analysis_prox_pairs_np, duality_gap_pairs_np, pair_norm_np, pd_dual_pairs_np, primal_dual_pairs_np,
                              tv_grad_adjoint_np, tv_grad_np, tv_ring_coefs_np, tv_value_np)

EPS = 2.0 ** -52
U = 2.0 ** -53  # the unit roundoff
LD = np.longdouble
assert np.finfo(LD).eps < 1.1e-19, "the element models need an extended long double"


def gamma(k):
    """gamma_k = k u / (1 - k u) of Higham: the relative error bound of k roundings"""
    return k * U / (1 - k * U)


def ring_weights(L):
    return ref.mw_map_weights(L)[:: 2 * L - 1].copy()


def ring_coefs(L):
    return tv_ring_coefs_np(ring_weights(L), L)


def thetas(L):
    return np.pi * (2 * np.arange(L) + 1) / (2 * L - 1)


def dense_gradient(L, ab=None):
    ab = ring_coefs(L) if ab is None else ab
    return np.stack([tv_grad_np(e, ab, L) for e in np.eye(L * (2 * L - 1))], axis=1)


def _cn(rng, cplx, *shape):
    return rng.normal(size=shape) + (1j * rng.normal(size=shape) if cplx else 0)


# ---- the polar-cap denoising problem (shared with tests/test_gpu_tv.py) ---------------------------------------------------------
CAP_SIG, CAP_T, CAP_LMDA, CAP_TOL = 0.3, 40.0, 1.0, 1e-6


def polar_cap_problem(L, cplx=False, seed=1):
    """the indicator of the cap theta < pi / 3 plus N(0, 0.3^2) noise, T = 40, lmda = 1; the steps are those of
    optim.PrimalDual with balance 1 from the exact ||A||^2 (dense SVD) and L_g = 1 / sig^2"""
    n = 2 * L - 1
    ab = ring_coefs(L)
    cap = np.repeat((thetas(L) < np.pi / 3).astype(float), n)
    rng = np.random.default_rng(seed)
    d = cap + CAP_SIG * rng.normal(size=L * n)
    if cplx:
        d = d + 1j * CAP_SIG * rng.normal(size=L * n)
    ic = 1.0 / CAP_SIG ** 2
    a2 = np.linalg.norm(dense_gradient(L, ab), 2) ** 2
    sigma = 0.5 * ic / a2
    tau = 1.0 / (0.5 * ic + sigma * a2)
    return dict(L=L, n=n, ab=ab, cap=cap, d=d, ic=ic, a2=a2, sigma=sigma, tau=tau, T=CAP_T, lmda=CAP_LMDA, sig=CAP_SIG,
                A=lambda x: tv_grad_np(x, ab, L), AH=lambda v: tv_grad_adjoint_np(v, ab, L), grad=lambda x: ic * (x - d))


def cap_objective(p, x):
    return 0.5 * p["ic"] * np.sum(np.abs(x - p["d"]) ** 2) + np.sum(p["T"] * pair_norm_np(p["A"](x))) / p["lmda"]


def cap_relative_gap(p, x, v):
    return duality_gap_pairs_np(x, v, p["d"], np.full(x.size, p["ic"]), p["A"], p["AH"], p["T"], p["lmda"]) / cap_objective(p, x)


# ---- long-double statements and planted inputs of the pair step (tests/test_gpu_tv.py) ---------------------------------------------
PAIR_SIGMA, PAIR_RSCALE, PAIR_TSCALAR = 0.5, 0.5, 10.0  # powers of two, so the planted elements are exact


def pair_inputs(m, C, cplx, vecT, seed):
    """(V, W, T) [C, 2 m] with ||v + sigma w|| spread around r = T rscale (= 5), and, for m >= 8, planted pairs by pixel i mod 8:
    1: on the ball exactly (real: w = (3, 4); complex: w = (1 + 2i, 2 + 4i); r = 5), 2: w = 0, 3: T_i = 0 (vector T only),
    4: far outside, 5: well inside.  No other pair lies within 2^-40 relative of its radius (checked in long double; a pair
    that did would be moved out by doubling its v)."""
    rng = np.random.default_rng(seed)
    V, W = 2.0 * _cn(rng, cplx, C, 2, m), 4.0 * _cn(rng, cplx, C, 2, m)
    T = PAIR_TSCALAR * (0.5 + rng.random(m)) if vecT else PAIR_TSCALAR
    planted = np.zeros(m, dtype=bool)
    if m >= 8:
        i = np.arange(m) % 8
        V[:, :, i == 1] = 0
        W[:, 0, i == 1], W[:, 1, i == 1] = (2 + 4j, 4 + 8j) if cplx else (6, 8)
        V[:, :, i == 2], W[:, :, i == 2] = 0, 0
        V[:, :, i == 4] *= 100
        V[:, :, i == 5] *= 1e-3
        W[:, :, i == 5] *= 1e-3
        planted = (i == 1) | (i == 2)
        if vecT:
            T[i == 1] = PAIR_TSCALAR
            T[i == 3] = 0
            planted |= i == 3
    V, W = V.reshape(C, 2 * m), W.reshape(C, 2 * m)
    for _ in range(3):
        _, a, r = pair_step_ext(V, W, T, PAIR_SIGMA, PAIR_RSCALE)
        close = (np.abs(a - r) <= 2.0 ** -40 * r) & ~planted
        if not close.any():
            break
        V.reshape(C, 2, m)[:, :, close.any(axis=0)] *= 2
    assert not close.any()
    return V, W, T


def parts(a):
    """the real components of an array as long doubles (complex: re, im as a trailing axis of 2; real: of 1)"""
    a = np.ascontiguousarray(a)
    return (a.view(np.float64).reshape(a.shape + (2,)) if np.iscomplexobj(a) else a.reshape(a.shape + (1,))).astype(LD)


def pair_step_ext(V, W, T, sigma, rscale):
    """the pair projection of v + sigma w in long double -> (components [C, 2, m, 1 or 2], ||w|| [C, m], r [C, m])"""
    C, m = V.shape[0], V.shape[1] // 2
    w = parts(V.reshape(C, 2, m)) + LD(sigma) * parts(W.reshape(C, 2, m))
    a = np.sqrt((w * w).sum(axis=(1, 3)))
    r = np.broadcast_to(np.asarray(T, dtype=float), (C, m)).astype(LD) * LD(rscale)
    s = np.where(a > r, r / np.where(a > 0, a, 1), LD(1))
    return w * s[:, None, :, None], a, r


# ---- the operator -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3, 5, 8])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_adjointness(L, cplx):
    """<A x, v> = <x, A^H v> to 1e-14 relative (of ||A x|| ||v||)"""
    ab = ring_coefs(L)
    rng = np.random.default_rng(10 * L + cplx)
    n = L * (2 * L - 1)
    x, v = _cn(rng, cplx, n), _cn(rng, cplx, 2 * n)
    lhs, rhs = np.vdot(tv_grad_np(x, ab, L), v), np.vdot(x, tv_grad_adjoint_np(v, ab, L))
    scale = np.linalg.norm(tv_grad_np(x, ab, L)) * np.linalg.norm(v)
    print(f"L={L} cplx={cplx}: |<Ax, v> - <x, A^H v>| / (||Ax|| ||v||) = {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 1e-14 * scale
    # batches and long double go through the same code
    xb = np.stack([x, 2 * x])
    assert np.array_equal(tv_grad_np(xb, ab, L)[1], tv_grad_np(2 * x, ab, L))
    assert np.array_equal(tv_grad_adjoint_np(np.stack([v, v]), ab, L)[0], tv_grad_adjoint_np(v, ab, L))
    assert tv_grad_np(x.real.astype(LD), ab.astype(LD), L).dtype == LD


@pytest.mark.parametrize("L", [2, 3, 5, 8])
def test_constants_and_the_pole_ring(L):
    """A const = 0; the ring theta = pi (n copies of one point) has zero rows in both planes, and every weight is positive"""
    ab = ring_coefs(L)
    n = 2 * L - 1
    assert np.all(ring_weights(L) > 0) and np.all(ab[:, : L - 1] > 0) and np.all(ab[:, L - 1] == 0)
    assert np.all(tv_grad_np(np.full(L * n, 3.7 - 1.2j), ab, L) == 0)
    D = dense_gradient(L, ab).reshape(2, L, n, L * n)
    assert np.all(D[:, L - 1] == 0) and np.any(D[0, L - 2] != 0) and np.any(D[1, L - 2] != 0)
    with pytest.raises(ValueError):
        tv_ring_coefs_np(ring_weights(L), L + 1)
    with pytest.raises(ValueError):
        tv_grad_np(np.zeros(L * n + 1), ab, L)
    with pytest.raises(ValueError):
        tv_grad_adjoint_np(np.zeros(L * n), ab, L)


def test_operator_norm_at_L8():
    """||A||^2 (dense SVD) lies below 4 max a_t^2 + 4 max b_t^2 (each plane is a difference of two entries scaled by its
    coefficient), and the weight folded in keeps it O(1): 1.258 at L = 8"""
    L = 8
    ab = ring_coefs(L)
    a2 = np.linalg.norm(dense_gradient(L, ab), 2) ** 2
    bound = 4 * ab[0].max() ** 2 + 4 * ab[1].max() ** 2
    print(f"L = 8: ||A||^2 = {a2:.4f}, bound {bound:.4f}")
    assert a2 < bound and a2 == pytest.approx(1.258, abs(5e-4))


def test_tv_of_Y10_converges_to_the_integral():
    """TV(Y_10) = sqrt(3 / 4 pi) int |sin theta| dOmega = sqrt(3 / 4 pi) pi^2, approached monotonically over L = 8 ... 64 and
    to 1e-3 relative at L = 64"""
    exact = np.sqrt(3 / (4 * np.pi)) * np.pi ** 2
    vals = []
    for L in (8, 16, 32, 64):
        y10 = np.repeat(np.sqrt(3 / (4 * np.pi)) * np.cos(thetas(L)), 2 * L - 1)
        vals.append(tv_value_np(y10, ring_coefs(L), L))
    print("TV(Y_10) at L = 8, 16, 32, 64:", vals, "exact", exact)
    err = np.abs(np.array(vals) - exact)
    assert np.all(np.diff(err) < 0) and np.all(np.diff(vals) > 0) and err[-1] <= 1e-3 * exact
    assert tv_value_np(y10, ring_coefs(64), 64, T=np.full(y10.size, 2.0)) == pytest.approx(2 * vals[-1], rel=1e-14)


# ---- the pair projection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_pair_projection(cplx):
    """the result lies in the ball, is the identity inside it, keeps ||w|| = r and w = 0, gives 0 for T = 0 and never binds
    for r = inf; a pair outside lands on the sphere in its own direction"""
    V, W, T = pair_inputs(64, 2, cplx, True, seed=3 + cplx)
    out = pd_dual_pairs_np(V, W, T, PAIR_SIGMA, PAIR_RSCALE)
    y = V + PAIR_SIGMA * W
    a, b, r = pair_norm_np(y), pair_norm_np(out), np.broadcast_to(T * PAIR_RSCALE, (2, 64))
    assert out.shape == V.shape and np.all(b <= r * (1 + 4 * EPS))
    inside = a <= r
    assert inside.any() and (~inside).any()
    keep = np.concatenate([inside, inside], axis=1)
    assert np.array_equal(out[keep], y[keep])
    assert np.all(np.abs(b[~inside] - r[~inside]) <= 4 * EPS * r[~inside])
    yo, oo = y.reshape(2, 2, 64), out.reshape(2, 2, 64)
    assert np.all(np.abs(oo * a[:, None] - yo * b[:, None]) <= 8 * EPS * (a * b)[:, None])  # same direction
    i = np.arange(64) % 8
    assert np.all(a[:, i == 1] == 5) and np.array_equal(oo[:, :, i == 1], yo[:, :, i == 1])  # on the ball: kept
    assert np.all(oo[:, :, i == 2] == 0) and np.all(oo[:, :, i == 3] == 0) and np.any(yo[:, :, i == 3] != 0)
    big = np.array([1e150, -1e150, 1e150, 1e150]) * (1 + 1j if cplx else 1)
    assert np.array_equal(pd_dual_pairs_np(np.zeros(4), big, np.array([np.inf, 1.0]), 1.0, 1.0)[[0, 2]], big[[0, 2]])
    # one chain without the batch axis, scalar T
    assert np.array_equal(pd_dual_pairs_np(V[0], W[0], 10.0, 0.5, 0.5), pd_dual_pairs_np(V, W, 10.0, 0.5, 0.5)[0])


# ---- the exact prox and the iteration ---------------------------------------------------------------------------------------------
def test_prox_meets_its_optimality_conditions():
    """L = 5, 20000 dual iterations: p = z - A^H v with ||v_i|| <= T_i, and where (A p)_i != 0 the dual sits on its sphere in
    the direction of (A p)_i; the prox objective equals the dual value 1/2 ||z||^2 - 1/2 ||p||^2 (zero duality gap)"""
    L = 5
    pr = polar_cap_problem(L, seed=1)
    A, AH, z = pr["A"], pr["AH"], pr["d"]
    T = 0.05 * (0.5 + np.random.default_rng(2).random(z.size))
    sigma = 1.0 / (pr["a2"] * (1 + 1e-4))
    p, v = analysis_prox_pairs_np(A, AH, T, z, 20000, sigma, return_dual=True)
    assert np.array_equal(p, z - AH(v)) and np.all(pair_norm_np(v) <= T * (1 + 4 * EPS))
    u = A(p)
    un = pair_norm_np(u)
    on = un > 1e-6 * un.max()
    want = (T / np.where(on, un, 1))[None, :] * u.reshape(2, -1)
    dev = np.abs(v.reshape(2, -1) - want)[:, on].max()
    F = 0.5 * np.linalg.norm(p - z) ** 2 + np.sum(T * un)
    dual = 0.5 * np.linalg.norm(z) ** 2 - 0.5 * np.linalg.norm(p) ** 2
    print(f"{on.sum()} of {on.size} pixels have a gradient; |v - T u / ||u||| on them {dev:.3e}; prox objective {F:.8f}, dual {dual:.8f}")
    assert 0 < on.sum() < on.size and dev <= 1e-6 * T.max()
    assert -64 * EPS * F <= F - dual <= 1e-9 * F
    assert F < np.sum(T * pair_norm_np(A(z)))  # better than staying at z
    norms = [np.linalg.norm(analysis_prox_pairs_np(A, AH, T, z, k, sigma)) for k in (0, 1, 2, 4, 8, 16, 32)]
    assert np.all(np.diff(norms) <= 8 * EPS * norms[0])  # descent of the dual objective


def test_polar_cap_map_at_L5():
    """the polar-cap problem at L = 5 stops within 2000 iterations at tolerance 1e-6 with a relative duality gap below 2e-4
    (this run: 535 iterations, 5.7e-5), and the objective there is below its value at the data and at the start"""
    p = polar_cap_problem(5)
    x, v, info = primal_dual_pairs_np(p["grad"], p["A"], p["AH"], p["T"], p["lmda"], p["tau"], p["sigma"], np.zeros_like(p["d"]),
                                      2000, tol=CAP_TOL)
    gap = cap_relative_gap(p, x, v)
    print(f"L = 5: {info['niter']} iterations, relative duality gap {gap:.3e}, ||A||^2 = {p['a2']:.4f}")
    assert info["converged"] and info["niter"] <= 2000 and 0 <= gap < 2e-4
    assert np.all(pair_norm_np(v) <= p["T"] / p["lmda"] * (1 + 4 * EPS))
    assert cap_objective(p, x) < min(cap_objective(p, p["d"]), cap_objective(p, np.zeros_like(x)))
