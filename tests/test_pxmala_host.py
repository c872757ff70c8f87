"""Host model of one PxMALA iteration (pxmcmc_amd/mcmc/pxmala.py PxMALA.run, csrc/pxmala.hip): the extended-precision
yardstick that tests/test_gpu_pxmala.py holds the proposal, tail and accept kernels to.

    p  = proxf (given) or soft(X, T)
    X' = (1 - d/l) X + (d/l) p - d g + sqrt(2 d) w,   P' = soft(X', T)
    r  = X' - X - (d/2) (-((X - p)/l) - g)            (the transition term of calc_logtransition(X, X'))
    S  = sum r^2 (complex square, no abs),  A = sum |wt X'|,  L2 = sum conj(e) (ic e), e = data - preds
    lt = -(d/2) S^2

The fp64 numpy route below goes through ``oracle.pxmcmc_np`` (soft, chain_step, calc_logtransition, tune_delta, logpi);
nothing here runs the code under test.

Bounds.  Per element the GPU test allows 4 x C0_MEASURED x 2^-52 x S_e, S_e the sum of the moduli of everything that is
added to form the element (error_scale / trans_scale); C0_MEASURED is the constant of the numpy route against the model,
measured here, and 4 is the margin the project gives device sqrt and division (tests/test_gpu_fista.py).

Sums.  A sum of n terms t_k, each known to within b_k, added in fp64 in any order, differs from the exact sum of the exact
terms by at most  sum_k b_k + n 2^-52 sum_k |t_k|  (every partial sum is at most sum |t_k| and there are n - 1 additions,
each with relative error 2^-53; the factor two absorbs the second-order terms).  For the complex transition sum the term is
r^2 = (re^2 - im^2, 2 re im), whose modulus is |r|^2: sum_k |t_k| = sum |r_k|^2 and NOT |S|, because re^2 - im^2 cancels
(|S| can be far below the sum of the moduli).  b_k for r^2 with r known to within e_k: 2 |r_k| e_k + e_k^2, plus 2 x 2^-52
|r_k|^2 for the two products and the subtraction that form the term.  For A: |wt| (e_k + 2 x 2^-52 |X'_k|) (fma, sqrt,
product).  For the L2 the inputs are exact: 8 x 2^-52 |ic_k| |e_k|^2 (one subtraction, the product with ic, the conjugate
product: fewer than eight roundings, each relative to |ic| |e|^2).  lt = -(d/2) S^2 with S known to within b:
(d/2) (2 |S| b + b^2) + 4 x 2^-52 |lt|."""
import numpy as np
import pytest

from conftest import golden
from oracle import philox, pxmcmc_np

EPS = 2.0 ** -52
LD = np.longdouble
CLD = np.clongdouble
HAVE_LD = np.finfo(np.longdouble).eps < 1.1e-19  # x87 80-bit extended precision

# Largest error of the fp64 numpy route (oracle.pxmcmc_np) against the extended-precision model over every element of
# propose_cases() and of two tail inputs, in units of 2^-52 S_e (test_numpy_route_against_extended_model measures it and
# holds it to this value).  Observed: X' 0.9517 / P' 1.4084 / r 0.3999 (complex128), X' 0.9664 / P' 0.9664 / r 0.4557
# (float64), reverse r 0.5614 / 0.4485.
C0_MEASURED = 1.41


# ---- extended-precision model ----------------------------------------------------------------------------------------
def _ld(a):
    a = np.asarray(a)
    return a.astype(CLD) if np.iscomplexobj(a) else a.astype(LD)


def _abs(z):
    """modulus as the kernels form it (sqrt of the sum of squares), in the precision of z"""
    return np.sqrt(z.real * z.real + z.imag * z.imag) if np.iscomplexobj(z) else np.abs(z)


def soft_ext(z, T):
    a = _abs(z)
    T = _ld(T) + 0 * a
    s = np.where(a > T, (a - T) / np.where(a > 0, a, 1), 0)
    return z * s


def _col(delta):
    return _ld(np.atleast_1d(delta))[:, None]


def transition_term_ext(X1, X2, P, G, delta, lmda, T=None):
    """r of calc_logtransition(X1, X2, P, G) per element; P = None: soft(X1, T).  delta: one value per chain"""
    x1, x2, g, d = _ld(X1), _ld(X2), _ld(G), _col(delta)
    p = soft_ext(x1, T) if P is None else _ld(P)
    gl = -((x1 - p) / LD(lmda)) - g
    return x2 - x1 - (d / 2) * gl


def propose_ext(X, P, G, W, T, delta, lmda):
    """(X', P', r) of the proposal pass; P = None: the prox is soft(X, T); W real on a complex state: a real draw"""
    x, g, w, d = _ld(X), _ld(G), _ld(W), _col(delta)
    p = soft_ext(x, T) if P is None else _ld(P)
    r_ = d / LD(lmda)
    xp = (1 - r_) * x + r_ * p - d * g + np.sqrt(2 * d) * w
    gl = -((x - p) / LD(lmda)) - g
    return xp, soft_ext(xp, T), xp - x - (d / 2) * gl


def sum_sq_ext(r):
    """S = sum r^2 per chain (complex square)"""
    return np.sum(r * r, axis=1)


def sum_l1_ext(Xp, wts=None):
    a = _abs(Xp)
    return np.sum(a if wts is None else np.abs(_ld(wts)) * a, axis=1)


def l2_ext(preds, data, invcov):
    e = _ld(data)[None, :] - _ld(preds)
    return np.sum(np.conj(e) * (_ld(invcov)[None, :] * e), axis=1)


def logtrans_ext(S, delta):
    d = _ld(np.atleast_1d(delta))
    return -(d / 2) * S * S


def logalpha_ext(lt_pc, lt_cp, prior_p, L2_p, mu, logpi_c):
    """log acceptance ratio: real parts only (pxmcmc/mcmc.py:244 compares a real uniform)"""
    f = lambda a: _ld(np.real(a))  # noqa: E731
    return f(lt_pc) + (-LD(mu) * f(prior_p) - f(L2_p)) - f(lt_cp) - f(logpi_c)


def tune_delta_ext(delta, acc, it, lmda):
    d = _ld(delta) * (1 + (_ld(acc) - LD(0.5)) / (LD(it) + 1) ** LD(0.75))
    return np.minimum(np.maximum(d, np.float64(lmda) * 1e-8), np.float64(lmda) / 2)


def accept_chain_model(lt_pc, lt_cp, prior_p, L2_p, mu, lmda, logpi_c, L2_c, prior_c, u, delta, it, tune, chunk=None):
    """accept_chain for every chain -> dict(logalpha, accept, logpi, L2, prior, delta, row): ``it`` is the iteration the
    kernel sees (argument + device counter); the state of a rejected chain is the input object's own values; NaN rejects"""
    la = logalpha_ext(lt_pc, lt_cp, prior_p, L2_p, mu, logpi_c)
    acc = (np.log(_ld(u)) < la).astype(np.int32)  # (NaN compares false)
    lpp = (-LD(mu) * _ld(prior_p) - _ld(np.real(L2_p))).astype(np.float64) + 1j * (-np.imag(L2_p))
    out = dict(logalpha=la, accept=acc, logpi=np.where(acc, lpp, logpi_c), L2=np.where(acc, L2_p, L2_c),
               prior=np.where(acc, prior_p, prior_c))
    out["delta"] = tune_delta_ext(delta, acc, it, lmda) if tune else _ld(delta)
    out["row"] = None if chunk is None else int(it) % int(chunk)
    return out


# ---- scales and ratios -------------------------------------------------------------------------------------------------
def _f64abs(a):
    return np.abs(np.asarray(a).astype(np.complex128 if np.iscomplexobj(a) else np.float64))


def error_scale(X, P, G, W, delta, lmda):
    """S_e of X' and P': |X| + (d/l) (|X| + |p|) + d |g| + sqrt(2 d) |w|"""
    d = np.asarray(np.atleast_1d(delta), dtype=float)[:, None]
    return _f64abs(X) + d / lmda * (_f64abs(X) + _f64abs(P)) + d * _f64abs(G) + np.sqrt(2 * d) * _f64abs(W)


def trans_scale(X1, X2, P, G, delta, lmda):
    """S_e of the transition term: |X2| + |X1| + (d/2) ((|X1| + |p|)/l + |g|)"""
    d = np.asarray(np.atleast_1d(delta), dtype=float)[:, None]
    return _f64abs(X2) + _f64abs(X1) + d / 2 * ((_f64abs(X1) + _f64abs(P)) / lmda + _f64abs(G))


def ratio_to_ext(got, ext, S):
    """largest |got - ext| over the elements in units of 2^-52 S_e (complex: the modulus of the difference)"""
    diff = _f64abs(_ld(got) - ext)
    return float(np.max(diff / (EPS * np.where(S > 0, S, 1))))


def sq_sum_bound(r_ext, e, n):
    """bound of the fp64 sum of r^2 per chain, r known to within e per element (see the module docstring)"""
    a = _f64abs(r_ext)
    return np.sum(2 * a * e + e * e + 2 * EPS * a * a, axis=1) + n * EPS * np.sum(a * a, axis=1)


def l1_sum_bound(Xp_ext, e, wts, n):
    a = _f64abs(Xp_ext)
    w = 1.0 if wts is None else np.abs(wts)
    return np.sum(w * (e + 2 * EPS * a), axis=1) + n * EPS * np.sum(w * a, axis=1)


def l2_sum_bound(preds, data, invcov, n):
    t = np.abs(invcov)[None, :] * np.abs(data[None, :] - preds) ** 2
    return (8 * EPS + n * EPS) * np.sum(t, axis=1)


def logtrans_bound(S_ext, bS, delta):
    d = np.asarray(np.atleast_1d(delta), dtype=float)
    s = _f64abs(S_ext)
    return d / 2 * (2 * s * bS + bS * bS) + 4 * EPS * d / 2 * s * s


# ---- input builders ------------------------------------------------------------------------------------------------------
LMDA = 2.5e-2
T_EXACT = 0.625  # 5 / 8: |(3/8, 4/8)| exactly, in fp64 and in the model


def _draw(rng, shape, cplx):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape) if cplx else rng.normal(size=shape)


def propose_inputs(n, C, cplx, vecT, seed, noise_cplx=None):
    """X, G, W [C, n], T ([n] or scalar), weights [n], delta [C], lmda.  Vector T: zeros (no shrink) at ::5, entries above
    every |x| at 2::7; at 3::11 the state sits exactly at |x| = T (both signs / all four quadrants) -- for a scalar T too"""
    rng = np.random.default_rng(seed)
    X, G = _draw(rng, (C, n), cplx), _draw(rng, (C, n), cplx) * 3.0
    W = _draw(rng, (C, n), cplx if noise_cplx is None else (cplx and noise_cplx))
    if vecT:
        T = np.abs(rng.normal(size=n)) * 0.5
        T[::5] = 0.0
        T[2::7] = 1e3
        T[3::11] = T_EXACT
    else:
        T = T_EXACT
    k = X[:, 3::11].shape[1]
    sg = np.where(rng.random((C, k)) < 0.5, -1.0, 1.0)
    X[:, 3::11] = sg * (0.375 + 0.5j * np.where(rng.random((C, k)) < 0.5, -1.0, 1.0)) if cplx else sg * T_EXACT
    wts = rng.normal(size=n)  # (signed: the kernels take |w|)
    delta = LMDA * (0.2 + 0.25 * rng.random(C))  # below lmda / 2, one per chain
    return dict(X=X, G=G, W=W, T=T, wts=wts, delta=delta, lmda=LMDA)


def tail_inputs(n, nd, C, cplx, dcplx, icplx, vecT, seed):
    """X1 (the proposal), X2 (the current state), G (the proposal's gradient) [C, n], T, preds [C, nd], data / invcov [nd]"""
    rng = np.random.default_rng(seed)
    inp = propose_inputs(n, C, cplx, vecT, seed)
    out = dict(X1=inp["X"], X2=_draw(rng, (C, n), cplx), G=inp["G"], T=inp["T"], delta=inp["delta"], lmda=LMDA)
    out["preds"], out["data"] = _draw(rng, (C, nd), dcplx), _draw(rng, nd, dcplx)
    ic = 1 / (0.5 + rng.random(nd)) ** 2
    out["invcov"] = ic * np.exp(1j * rng.normal(size=nd)) if icplx else ic
    return out


def propose_cases():
    for cplx in (False, True):
        for vecT in (False, True):
            for ncplx in ((False, True) if cplx else (False,)):
                yield cplx, propose_inputs(257, 3, cplx, vecT, seed=21 + 4 * cplx + 2 * vecT + ncplx, noise_cplx=ncplx)


# ---- fp64 numpy route ------------------------------------------------------------------------------------------------------
def propose_np(X, P, G, W, T, delta, lmda):
    d = np.asarray(delta)[:, None]
    p = pxmcmc_np.soft(X, T) if P is None else P
    Xp = pxmcmc_np.chain_step(X, p, G, d, lmda, W)
    r = Xp - X - (d / 2) * (-((X - p) / lmda) - G)
    return Xp, pxmcmc_np.soft(Xp, T), r, p


# ---- tests ---------------------------------------------------------------------------------------------------------------
def test_extended_precision_is_available():
    assert HAVE_LD, "the model needs numpy's 80-bit long double"


def test_builders_place_the_edges():
    for cplx, inp in propose_cases():
        X, T = inp["X"], inp["T"]
        p = pxmcmc_np.soft(X, T)
        assert np.all(np.abs(X[:, 3::11]) == T_EXACT) and np.all(p[:, 3::11] == 0)  # exactly at the threshold: zero
        if np.ndim(T):
            assert T[5] == 0 and T[10] == 0 and T[9] == 1e3 and T[16] == 1e3 and T[3] == T_EXACT and T[25] == T_EXACT
            assert np.all(p[:, [9, 16]] == 0) and np.all(np.abs(X) < 1e3)  # T above every |x|: zero
            assert np.allclose(p[:, 5], X[:, 5], rtol=4 * EPS, atol=0)  # T = 0 keeps the state ((z / |z|) |z| in the oracle)
        assert np.all(inp["delta"] < inp["lmda"] / 2) and np.all(inp["delta"] > 0)
        assert np.array_equal(_f64abs(soft_ext(X, T)) == 0, p == 0)  # the model takes the same branch at the edges


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_model_against_the_oracle(cplx):
    """the model of the proposal, the transition sums, lt, the L2 and logpi against oracle.pxmcmc_np at fp64 accuracy"""
    inp = propose_inputs(63, 2, cplx, True, seed=3 + cplx)
    X, G, W, T, wts, delta, lmda = (inp[k] for k in ("X", "G", "W", "T", "wts", "delta", "lmda"))
    eXp, ePp, er = propose_ext(X, None, G, W, T, delta, lmda)
    S, A = sum_sq_ext(er), sum_l1_ext(eXp, wts)
    t = tail_inputs(63, 9, 2, cplx, cplx, cplx, True, seed=5 + cplx)
    for c in range(2):
        p = pxmcmc_np.soft(X[c], T)
        Xp = pxmcmc_np.chain_step(X[c], p, G[c], delta[c], lmda, W[c])
        np.testing.assert_allclose(eXp[c].astype(Xp.dtype), Xp, rtol=0, atol=16 * EPS * np.abs(X[c]).max() * 4)
        np.testing.assert_allclose(ePp[c].astype(Xp.dtype), pxmcmc_np.soft(Xp, T), rtol=0, atol=64 * EPS)
        lt = pxmcmc_np.calc_logtransition(X[c], Xp, p, G[c], delta[c], lmda)
        lt_model = logtrans_ext(S, delta)[c]
        # (numpy's Xp in place of the model's: r changes by ~eps |X'|, the sum by ~eps sum |r| |X'|: 1e-11 of |lt| is ample)
        assert abs(complex(lt_model) - lt) <= 1e-11 * abs(lt)
        assert abs(float(A[c]) - np.sum(np.abs(wts * Xp))) <= 1e-13 * float(A[c])
        rev = sum_sq_ext(transition_term_ext(t["X1"], t["X2"], None, t["G"], t["delta"], lmda, T=t["T"]))
        lt_rev = pxmcmc_np.calc_logtransition(t["X1"][c], t["X2"][c], pxmcmc_np.soft(t["X1"][c], t["T"]), t["G"][c], t["delta"][c], lmda)
        assert abs(complex(logtrans_ext(rev, t["delta"])[c]) - lt_rev) <= 1e-12 * abs(lt_rev)
        lp, L2, pr = pxmcmc_np.logpi(X[c], t["preds"][c], t["data"], t["invcov"], lambda x: np.sum(np.abs(wts * x)), 1.3)
        assert abs(complex(l2_ext(t["preds"], t["data"], t["invcov"])[c]) - L2) <= 1e-13 * abs(L2)
        m = accept_chain_model(np.array([lt]), np.array([lt_rev]), np.array([pr]), np.array([L2]), 1.3, lmda, np.array([0j]),
                               np.array([0j]), np.array([0.0]), np.array([0.5]), delta[c:c + 1], 4, True)
        assert abs(float(m["logalpha"][0]) - np.real(lt + lp - lt_rev)) <= 1e-13 * (abs(lt) + abs(lp) + abs(lt_rev))


def test_model_against_the_reference_vectors():
    """g4_pxmala.npz, captured from the reference: logpi, both calc_logtransition values and the delta sequence"""
    g = golden("g4_pxmala.npz")
    lmda, delta, mu = (float(v) for v in g["params"][:3])
    data, X, X2 = g["data"], g["X"], g["X2"]
    ic = np.full(data.size, 1 / 0.1 ** 2)
    L2 = l2_ext(X[None], data, ic)[0]
    pr = sum_l1_ext(_ld(X[None]))[0]
    np.testing.assert_allclose(np.array([-mu * pr - L2, L2, pr], dtype=float), g["logpi"], rtol=1e-14)
    r = transition_term_ext(X[None], X2[None], pxmcmc_np.soft(X, lmda * mu)[None], (ic * (X - data))[None], [delta], lmda)
    np.testing.assert_allclose(float(logtrans_ext(sum_sq_ext(r), [delta])[0]), g["logtrans"], rtol=1e-13)
    Xc, X2c = g["Xc"], g["X2c"]
    rc = transition_term_ext(Xc[None], X2c[None], None, (0.5 * Xc)[None], [delta], lmda, T=3e-3)
    np.testing.assert_allclose(complex(logtrans_ext(sum_sq_ext(rc), [delta])[0]), g["logtrans_c"], rtol=1e-13)
    d = delta
    for i, a in enumerate(g["tune_acc"]):
        want = pxmcmc_np.tune_delta(d, int(a), i, lmda)
        got = float(tune_delta_ext(np.array([d]), np.array([int(a)]), i, lmda)[0])
        assert abs(got - want) <= 2 * EPS * want and want == g["tune_seq"][i]
        d = want


def test_accept_model_state_clamps_and_trace_row():
    lmda = LMDA
    z = np.zeros(4)
    lt_pc = np.array([-1.0, -1.0, np.nan, -1.0]) + 0j
    u = np.exp(np.array([-1.0 * (1 + 1e-9), -1.0 * (1 - 1e-9), -5.0, -1.0 * (1 + 1e-9)]))  # accept, reject, NaN, accept
    logpi_c, L2_c, prior_c = np.array([1 + 2j, 3 + 4j, 5 + 6j, 7 + 8j]) * 0, np.arange(4) + 1j, np.arange(4) + 10.0
    delta = np.array([lmda / 2, lmda * 1e-8, 1e-3, 1e-3])
    m = accept_chain_model(lt_pc, z + 0j, z, z + 0j, 1.0, lmda, logpi_c, L2_c, prior_c, u, delta, 6, True, chunk=4)
    assert list(m["accept"]) == [1, 0, 0, 1] and m["row"] == 2
    assert np.array_equal(m["L2"][[1, 2]], L2_c[[1, 2]]) and np.all(m["L2"][[0, 3]] == 0) and np.array_equal(m["prior"][[1, 2]], prior_c[[1, 2]])
    assert float(m["delta"][0]) == lmda / 2 and float(m["delta"][1]) == lmda * 1e-8  # both clamps
    assert float(m["delta"][3]) == pytest.approx(pxmcmc_np.tune_delta(1e-3, 1, 6, lmda), rel=2 * EPS)
    m0 = accept_chain_model(lt_pc, z + 0j, z, z + 0j, 1.0, lmda, logpi_c, L2_c, prior_c, u, delta, 6, False)
    assert np.array_equal(m0["delta"].astype(float), delta)


def test_numpy_route_against_extended_model():
    """the yardstick of the GPU tests: how far the fp64 numpy route is from the extended-precision model, per element, in
    units of 2^-52 S_e -- measured here, pinned as C0_MEASURED"""
    worst = {}
    for cplx, inp in propose_cases():
        X, G, W, T, delta, lmda = (inp[k] for k in ("X", "G", "W", "T", "delta", "lmda"))
        Xp, Pp, r, p = propose_np(X, None, G, W, T, delta, lmda)
        eXp, ePp, er = propose_ext(X, None, G, W, T, delta, lmda)
        S = error_scale(X, p, G, W, delta, lmda)
        Sr = S + trans_scale(X, Xp, p, G, delta, lmda)
        for name, got, ext, sc in (("X'", Xp, eXp, S), ("P'", Pp, ePp, S), ("r", r, er, Sr)):
            worst[(cplx, name)] = max(worst.get((cplx, name), 0.0), ratio_to_ext(got, ext, sc))
        assert np.any(Pp == 0) and np.any(Pp != 0)
    for cplx in (False, True):
        t = tail_inputs(257, 9, 3, cplx, False, False, True, seed=40 + cplx)
        p = pxmcmc_np.soft(t["X1"], t["T"])
        d = t["delta"][:, None]
        r = t["X2"] - t["X1"] - (d / 2) * (-((t["X1"] - p) / t["lmda"]) - t["G"])
        er = transition_term_ext(t["X1"], t["X2"], None, t["G"], t["delta"], t["lmda"], T=t["T"])
        worst[(cplx, "reverse r")] = ratio_to_ext(r, er, trans_scale(t["X1"], t["X2"], p, t["G"], t["delta"], t["lmda"]))
    print("fp64 numpy route vs extended model, units of 2^-52 S_e:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= C0_MEASURED
    assert max(worst.values()) >= C0_MEASURED / 4  # the pinned value is the measured one, not a loose cap


def test_sum_bounds_hold_for_the_numpy_route():
    """the sum bounds of the module docstring, exercised on numpy's own fp64 sums with e = C0_MEASURED 2^-52 S_e"""
    for cplx, inp in propose_cases():
        X, G, W, T, wts, delta, lmda = (inp[k] for k in ("X", "G", "W", "T", "wts", "delta", "lmda"))
        n = X.shape[1]
        Xp, Pp, r, p = propose_np(X, None, G, W, T, delta, lmda)
        eXp, _, er = propose_ext(X, None, G, W, T, delta, lmda)
        S = error_scale(X, p, G, W, delta, lmda)
        e, er_b = C0_MEASURED * EPS * S, C0_MEASURED * EPS * (S + trans_scale(X, Xp, p, G, delta, lmda))
        assert np.all(_f64abs(_ld(np.sum(r ** 2, axis=1)) - sum_sq_ext(er)) <= sq_sum_bound(er, er_b, n))
        assert np.all(_f64abs(_ld(np.sum(np.abs(wts * Xp), axis=1)) - sum_l1_ext(eXp, wts)) <= l1_sum_bound(eXp, e, wts, n))
    t = tail_inputs(63, 300, 3, True, True, True, True, seed=8)
    got = np.array([np.vdot(t["data"] - t["preds"][c], t["invcov"] * (t["data"] - t["preds"][c])) for c in range(3)])
    assert np.all(_f64abs(_ld(got) - l2_ext(t["preds"], t["data"], t["invcov"])) <= l2_sum_bound(t["preds"], t["data"], t["invcov"], 300))
    # the cancellation the docstring speaks of: |S| of a complex transition sum is far below sum |r|^2
    r = _draw(np.random.default_rng(0), (1, 4096), True)
    assert abs(np.sum(r ** 2)) < 0.1 * np.sum(np.abs(r) ** 2)


def test_uniform_oracle():
    """values in (0, 1); a function of (seed, chain, it) only; different across chains, iterations and seeds; the first
    draw of the Philox block at counter index 2^63 (the noise stream's complex pair at that index shares its u1)"""
    vals = {}
    for seed in (0, 7, 2 ** 63 + 11):
        for chain in range(0, 24):
            for it in (0, 1, 6, 2 ** 32 + 3):
                u = philox.uniform(seed, chain, it)
                assert 0.0 < u < 1.0 and u == philox.uniform(seed, chain, it)
                vals[(seed, chain, it)] = u
    assert len(set(vals.values())) == len(vals)
    assert abs(np.mean(list(vals.values())) - 0.5) < 4 / np.sqrt(12 * len(vals))
    # the same block through the oracle's normal_pairs: z0^2 + z1^2 = -2 ln u1
    z0, z1 = philox.normal_pairs(7, 3, np.array([philox.UNIFORM_INDEX], dtype=np.uint64), 6, bits=64)
    assert np.exp(-(z0[0] ** 2 + z1[0] ** 2) / 2) == pytest.approx(philox.uniform(7, 3, 6), rel=1e-13)
    # pinned values (Philox4x32-10 of Salmon et al. with this key / counter layout)
    assert philox.uniform(1, 0, 0) == 0.20334244314712474 and philox.uniform(1, 1, 0) == 0.7599873033460003
    assert philox.uniform(1, 0, 1) == 0.6981913764182652
