"""Host model of the local credible intervals (pxmcmc_amd/uncertainty/lci.py, csrc/lci.hip): the superpixel
labels, the construction X(xi) = a + xi b on the oracle's wavelet transform, and the numpy statement of the search held to a
long-double bisection on random convex instances and on one designed case per status.  tests/test_gpu_lci.py holds the
kernels to the same instances, cases and properties."""
import numpy as np
import pytest

from pxmcmc_amd.uncertainty import (LCI_EMPTY, LCI_NONFINITE, LCI_OK, LCI_UNCONSTRAINED, lci_eval_np, lci_search_np,
                                    lci_shrink_factor, lci_terms_np, superpixel_regions)

LD = np.longdouble
U = 2.0 ** -53  # unit round-off of float64
ROUNDS = 10
# roundings of one term T |a + xi b| beyond the sum: the two fma of the components (1 each), the product and the fma of the
# squared modulus (2), the square root (halves what precedes, adds up to 2 for a device sqrt of 1 ulp), the product with T (1)
TERM_ROUNDINGS = 6


# ---- the long-double model and the tolerance of an evaluation of F -------------------------------------------------------------
def F_ld(inst, xi):
    """F(xi) in long double from the instance's exact-as-given float64 inputs"""
    q = [LD(v) for v in inst["q"]]
    x = LD(xi)
    return q[0] + q[1] * x + q[2] * x * x + lci_eval_np(inst["a"], inst["b"], inst["T"], [xi])[0] / LD(inst["lmda"])


def f_tol(inst, xi, depth):
    """bound on |F evaluated in float64 - F| at xi: the sum of n non-negative terms through a chain of ``depth`` additions,
    each term with TERM_ROUNDINGS roundings, costs (depth + TERM_ROUNDINGS) U P; the division by lmda and the last addition
    one more each; Horner's form of the quadratic at most 5 U (|q0| + |q1 xi| + |q2| xi^2)"""
    q0, q1, q2 = (abs(float(v)) for v in inst["q"])
    P = float(lci_eval_np(inst["a"], inst["b"], inst["T"], [xi])[0])
    x = abs(float(xi))
    return U * ((depth + TERM_ROUNDINGS + 2) * P / inst["lmda"] + 5.0 * (q0 + q1 * x + q2 * x * x))


def bisect_end(inst, level, outside, inside, iters=200):
    """the end of {F <= level} between ``outside`` (F > level) and ``inside`` (F <= level), by long-double bisection"""
    lo, hi = LD(outside), LD(inside)
    for _ in range(iters):
        mid = (lo + hi) / 2
        if F_ld(inst, mid) <= level:
            hi = mid
        else:
            lo = mid
    return hi


def check_ok_result(inst, res, depth, rounds=ROUNDS):
    """the three end-point properties of a result with status ok.  ``depth``: the chain of additions of the sums that
    evaluated F (numpy: n; the device: lci_sum_depth(n)).  Returns the largest width relative to the outer bracket."""
    lower, upper, wlo, whi = res["lower"], res["upper"], res["width_lower"], res["width_upper"]
    olo, ohi = res["outer"]
    gamma = LD(inst["gamma"])
    assert np.isfinite([lower, upper, wlo, whi, olo, ohi]).all() and olo <= lower <= upper <= ohi and wlo >= 0 and whi >= 0
    # 1. F <= gamma at the returned ends, to the rounding of the evaluation that accepted them
    for x in (lower, upper):
        assert F_ld(inst, x) <= gamma + f_tol(inst, x, depth), (x, float(F_ld(inst, x) - gamma))
    # 2. F >= gamma one final width outside, or the bracket's outer point is still the outer bracket's end (F >= gamma holds
    #    there by construction: the quadratic, or the L1 bound, equals gamma)
    for x, end in ((lower - wlo, olo), (upper + whi, ohi)):
        if x != end:
            assert F_ld(inst, x) >= gamma - f_tol(inst, x, depth), (x, float(F_ld(inst, x) - gamma))
    # 3. the widths: the guaranteed factor per round, plus the rounding of the points (a few ulps of the bracket's scale)
    bound = lci_shrink_factor(rounds, inst["q"][2] > 0) * (ohi - olo) + 64 * U * max(abs(olo), abs(ohi))
    assert wlo <= bound and whi <= bound, (wlo, whi, bound)
    # the same against the bisected ends: the end of the set at the level gamma + tol is not right of `lower`, the end at
    # gamma - tol not left of lower - width (and mirrored)
    xin = res["xi_min"]
    if F_ld(inst, xin) <= gamma:
        for inner, outer_pt, end, sign in ((lower, lower - wlo, olo, 1), (upper, upper + whi, ohi, -1)):
            tol = max(f_tol(inst, inner, depth), f_tol(inst, outer_pt, depth))
            far = end - sign * (abs(end) + 1.0)  # a point outside the outer bracket: F > gamma + tol there or F is flat
            if F_ld(inst, far) > gamma + tol:
                assert sign * (bisect_end(inst, gamma + tol, far, xin) - LD(inner)) <= 0
            if outer_pt != end and F_ld(inst, xin) <= gamma - tol and F_ld(inst, far) > gamma - tol:
                assert sign * (bisect_end(inst, gamma - tol, far, xin) - LD(outer_pt)) >= 0
    return max(wlo, whi) / (ohi - olo) if ohi > olo else 0.0


# ---- instances -----------------------------------------------------------------------------------------------------------------
def make_instance(seed):
    """a random convex instance: n from 1 to 200, 30 % non-zero b, q2 = 0 (s = 0) in a fifth of them, complex in half; gamma is
    F at a random point plus a margin, so the set is not empty.  q is the float64 rounding of the long-double sums: the
    search and the model take the same numbers."""
    rng = np.random.default_rng(1000 + seed)
    n, m = int(rng.integers(1, 201)), int(rng.integers(1, 40))
    cplx = bool(seed % 2)
    vec = (lambda k: rng.normal(size=k) + 1j * rng.normal(size=k)) if cplx else (lambda k: rng.normal(size=k))
    a, b = vec(n), vec(n) * (rng.random(n) < 0.3)
    if not np.any(b):
        b[int(rng.integers(n))] = 1.0
    T = rng.random(n) * 2.0 if seed % 3 else float(rng.random() + 0.1)
    r, s = vec(m), (np.zeros(m, dtype=a.dtype) if seed % 5 == 0 else vec(m))
    w = rng.random(m) + 0.5
    q, Sa, Sb = lci_terms_np(a, b, r, s, w, T)
    inst = dict(a=a, b=b, T=T, r=r, s=s, w=w, q=np.array(q, dtype=np.float64), lmda=float(10.0 ** rng.uniform(-2, 0.5)), n=n)
    inst["gamma"] = float(F_ld(inst, rng.normal()) + LD(10.0 ** rng.uniform(-3, 1)))
    return inst


def status_cases():
    """one designed instance per status -> list of (name, instance, expected status)"""
    rng = np.random.default_rng(7)
    n = 40
    a, b = rng.normal(size=n) + 1j * rng.normal(size=n), (rng.normal(size=n) + 1j * rng.normal(size=n)) * (rng.random(n) < 0.3)
    T = rng.random(n) + 0.1
    base = dict(a=a, b=b, T=T, lmda=0.5, n=n, q=np.array([3.0, -1.0, 2.0]))
    xs = np.linspace(-3, 3, 20001)
    Fg = np.array([float(F_ld(base, x)) for x in xs[::50]])
    x0 = xs[::50][int(np.argmin(Fg))]
    fine = np.linspace(x0 - 0.05, x0 + 0.05, 2001)
    Fmin = min(float(F_ld(base, x)) for x in fine)  # min F to ~1e-9 (F is piecewise smooth with curvature ~ 4)
    qmin = 3.0 - 1.0 / 8.0  # min of the quadratic
    cases = [
        ("negative discriminant", dict(base, gamma=qmin - 0.5), LCI_EMPTY),
        ("gamma just below min F", dict(base, gamma=Fmin - 1e-6 * abs(Fmin)), LCI_EMPTY),
        ("gamma just above min F", dict(base, gamma=Fmin + 1e-6 * abs(Fmin)), LCI_OK),
        ("b = 0 with s = 0", dict(base, b=np.zeros(n, dtype=complex), q=np.array([3.0, 0.0, 0.0]), gamma=1e3), LCI_UNCONSTRAINED),
    ]
    # a kink exactly on a grid point: q(xi) = xi^2 + q0 with gamma - q0 = 31^2 gives the outer bracket [-31, 31] and the
    # first-round points -31, -29, ..., 31 exactly; a_k + xi b_k = -9 + xi vanishes at the point j = 20
    ak, bk = np.array([-9.0, 0.5, 2.0]), np.array([1.0, 0.0, -0.25])
    cases.append(("kink on a grid point", dict(a=ak, b=bk, T=np.array([4.0, 1.0, 2.0]), lmda=0.25, n=3,
                                               q=np.array([5.0, 0.0, 1.0]), gamma=5.0 + 961.0), LCI_OK))
    # q2 = 0 with q1 != 0 (a q2 that underflowed): the L1 bracket carries |q1| |xi|
    cases.append(("q2 = 0 with q1 != 0", dict(base, q=np.array([3.0, 0.3, 0.0]), gamma=Fmin + 5.0), LCI_OK))
    cases.append(("q2 = 0, not coercive", dict(base, q=np.array([3.0, 1e3, 0.0]), gamma=Fmin + 5.0), LCI_UNCONSTRAINED))
    nan_a = a.copy()
    nan_a[3] = np.nan
    cases.append(("NaN in a", dict(base, a=nan_a, gamma=Fmin + 1.0), LCI_NONFINITE))
    cases.append(("NaN in a, negative discriminant", dict(base, a=nan_a, gamma=qmin - 0.5), LCI_NONFINITE))
    return cases


def check_status_case(name, inst, want, res, depth):
    assert res["status"] == want, (name, res)
    if want == LCI_OK:
        check_ok_result(inst, res, depth)
        if name == "gamma just above min F":  # narrower than one cell of the first round: found all the same
            assert res["upper"] - res["lower"] < (res["outer"][1] - res["outer"][0]) / 31
        if name == "kink on a grid point":
            assert res["outer"] == (-31.0, 31.0)
    elif want == LCI_UNCONSTRAINED:
        assert res["lower"] == -np.inf and res["upper"] == np.inf
        assert res["f_min"] <= inst["gamma"] or inst["q"][1] != 0
    elif want == LCI_NONFINITE:
        assert np.isnan([res["lower"], res["upper"], res["f_min"], res["xi_min"]]).all()
    elif name == "negative discriminant":
        assert np.isnan(res["lower"]) and np.isnan(res["upper"])
    else:  # no point with F <= gamma: the bracket of the minimiser comes back
        # (near its minimum F is flat to rounding over ~sqrt(U) of the scale, so the last brackets follow rounding noise: the
        # smallest F seen lies within that distance of the final bracket, not necessarily inside it)
        assert np.isfinite([res["lower"], res["upper"]]).all() and res["lower"] <= res["upper"]
        assert abs(res["xi_min"] - res["lower"]) <= 1e-6 * (res["outer"][1] - res["outer"][0])
        assert res["f_min"] > inst["gamma"]
        assert res["upper"] - res["lower"] <= lci_shrink_factor(ROUNDS) * (res["outer"][1] - res["outer"][0]) + 64 * U * 3


# ---- tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [8, 16])
@pytest.mark.parametrize("size", [1, 3, 4, "L"])
def test_superpixel_regions_partition(L, size):
    size = L if size == "L" else size
    lab = superpixel_regions(L, size)
    assert lab.shape == (L, 2 * L - 1) and lab.dtype == np.int32
    nt, nphi = -(-L // size), -(-(2 * L - 1) // size)
    assert np.array_equal(np.unique(lab), np.arange(nt * nphi))  # every pixel in exactly one of the nt x nphi regions
    for it in range(nt):
        for ip in range(nphi):
            rows, cols = np.nonzero(lab == it * nphi + ip)
            h = min(size, L - it * size)  # the last blocks are smaller
            wd = min(size, 2 * L - 1 - ip * size)
            assert rows.size == h * wd
            assert rows.min() == it * size and rows.max() == it * size + h - 1
            assert cols.min() == ip * size and cols.max() == ip * size + wd - 1
    with pytest.raises(ValueError):
        superpixel_regions(L, 0)


@pytest.fixture(scope="module")
def wav16():
    from oracle import s2let

    W = s2let.WaveletTransform(16, 2, 0)
    assert W.ncoefs == 1147
    return W


def test_surrogate_sets_the_region_of_the_bandlimited_image(wav16):
    """synthesis(a + xi b) = x* + synthesis(analysis((xi - x*) zeta)) to round-off"""
    W = wav16
    rng = np.random.default_rng(3)
    X = (rng.normal(size=W.ncoefs) + 1j * rng.normal(size=W.ncoefs)) * 0.3
    x = W.synthesis(X)
    zeta = (superpixel_regions(16, 4).reshape(-1) == 13).astype(float)
    a, b = X - W.analysis(x * zeta), W.analysis(zeta)
    scale = np.abs(x).max()
    for xi in (-2.5, 0.0, 0.7):
        want = x + W.synthesis(W.analysis((xi - x) * zeta))
        err = np.abs(W.synthesis(a + xi * b) - want).max()
        print(f"xi = {xi}: max difference {err:.3e} (image scale {scale:.3f})")
        assert err <= 1e-12 * scale


def test_objective_at_the_regions_own_constant(wav16):
    """where x* is constant c on the region, X(c) = X*: F(c) from (q, P) equals F(X*) formed directly"""
    W = wav16
    rng = np.random.default_rng(4)
    c, lmda = 0.8, 0.05
    X = W.analysis(np.full(W.L * (2 * W.L - 1), c))
    x = W.synthesis(X)
    assert np.abs(x - c).max() < 1e-12
    zeta = (superpixel_regions(16, 4).reshape(-1) == 6).astype(float)
    a, b = X - W.analysis(x * zeta), W.analysis(zeta)
    data = rng.normal(size=x.size)
    w = rng.random(x.size) + 0.5
    T = rng.random(W.ncoefs) * 0.01
    q, Sa, Sb = lci_terms_np(a, b, W.synthesis(a) - data, W.synthesis(b), w, T)
    F_c = q[0] + q[1] * LD(c) + q[2] * LD(c) ** 2 + lci_eval_np(a, b, T, [c])[0] / LD(lmda)
    F_map = 0.5 * np.sum(w * np.abs(x - data) ** 2) + np.sum(T * np.abs(X)) / lmda
    print(f"F(c) = {float(F_c):.12e}, F(X*) = {F_map:.12e}")
    assert abs(float(F_c) - F_map) <= 1e-11 * abs(F_map)
    assert Sb > 0 and q[2] > 0


def test_search_against_long_double_bisection():
    worst = 0.0
    for seed in range(200):
        inst = make_instance(seed)
        res = lci_search_np(inst["q"], inst["a"], inst["b"], inst["T"], inst["lmda"], inst["gamma"], rounds=ROUNDS)
        assert res["status"] == LCI_OK, (seed, res)
        worst = max(worst, check_ok_result(inst, res, inst["n"]) / lci_shrink_factor(ROUNDS, inst["q"][2] > 0))
    print(f"largest final width / (guaranteed factor x outer bracket): {worst:.3e}")


@pytest.mark.parametrize("case", status_cases(), ids=lambda c: c[0])
def test_status_cases(case):
    name, inst, want = case
    res = lci_search_np(inst["q"], inst["a"], inst["b"], inst["T"], inst["lmda"], inst["gamma"], rounds=ROUNDS)
    check_status_case(name, inst, want, res, inst["n"])
