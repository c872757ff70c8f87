"""The analysis-setting solvers on the GPU: the two primal-dual step kernels (pxm_pd_primal_step, pxm_pd_dual_step) against
the long-double element models of tests/test_pd_host.py on every element of every chain, their per-chain sums and refusals;
optim.PrimalDual on the identity problem (closed form) and on L = 16 wavelets (optimality conditions through the transforms,
FISTA's point, graph replay); optim.analysis_prox against its numpy statement; MYULA with the exact analysis prox."""
import contextlib
import ctypes
import io
import warnings

import numpy as np
import pytest

from test_pd_host import (EPS, LD, PD_RSCALE, PD_SIGMA, _parts, pd_dual_ext, pd_dual_inputs, pd_primal_ext, soft_np)

pytestmark = pytest.mark.gpu

SLICES_MAX = 256  # PXM_FISTA_SLICES_MAX (asserted below)
N_STRIDE = 256 * SLICES_MAX + 3  # more elements than one pass of the largest grid: the grid-stride loop
C_MAX = 4  # chains the buffers are allocated for: nothing may be written past the launch's C


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _dev(a):
    """a [C, n] numpy array in a NaN-filled device buffer of C_MAX chains"""
    import torch

    from pxmcmc_amd import ops

    dt = torch.complex128 if np.iscomplexobj(a) else torch.float64
    t = torch.full((C_MAX, a.shape[1]), float("nan"), dtype=dt, device=ops.device())
    t[: a.shape[0]] = ops.as_device(a, dt)
    return t


def _nan_like(t, k=None):
    import torch

    shape = t.shape if k is None else (t.shape[0], k)
    return torch.full(shape, float("nan"), dtype=t.dtype if k is None else torch.float64, device=t.device)


def _primal_inputs(n, C, cplx, seed):
    rng = np.random.default_rng(seed)
    draw = (lambda: rng.normal(size=(C, n)) + 1j * rng.normal(size=(C, n))) if cplx else (lambda: rng.normal(size=(C, n)))
    return draw(), 30.0 * draw(), 10.0 * draw(), 0.037


def _run_primal(X, G, U, tau, chains=None):
    """the kernel on chains [0, C) in one launch (or the listed ones, one launch each) -> (X1, Xbar, sums) as numpy"""
    import torch

    from pxmcmc_amd import ops

    C = X.shape[0]
    bX, bG, bU = _dev(X), _dev(G), _dev(U)
    b1, bb, sums = _nan_like(bX), _nan_like(bX), _nan_like(bX, 2)
    for sl in ([slice(0, C)] if chains is None else [slice(c, c + 1) for c in chains]):
        ops.pd_primal_step(bX[sl], bG[sl], bU[sl], tau, out=(b1[sl], bb[sl]), sums=sums[sl])
    torch.cuda.synchronize()
    assert torch.isnan(b1[C:].real).all() and torch.isnan(bb[C:].real).all() and torch.isnan(sums[C:]).all()
    return b1[:C].cpu().numpy(), bb[:C].cpu().numpy(), sums[:C].cpu().numpy()


def _run_dual(V, W, T, chains=None):
    import torch

    from pxmcmc_amd import ops

    C = V.shape[0]
    bV, bW = _dev(V), _dev(W)
    b1, sums = _nan_like(bV), _nan_like(bV, 3)
    Td = ops.as_device(T, torch.float64) if np.ndim(T) else float(T)
    for sl in ([slice(0, C)] if chains is None else [slice(c, c + 1) for c in chains]):
        ops.pd_dual_step(bV[sl], bW[sl], Td, PD_SIGMA, PD_RSCALE, out=b1[sl], sums=sums[sl])
    torch.cuda.synchronize()
    assert torch.isnan(b1[C:].real).all() and torch.isnan(sums[C:]).all()
    return b1[:C].cpu().numpy(), sums[:C].cpu().numpy()


# ---- the two kernels, element by element ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, N_STRIDE])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_primal_step_against_the_long_double_model(n, C, cplx):
    """Per real component, with eps = 2^-52 (two units of rounding):
    s = fl(g + u) is off by at most eps/2 (|g| + |u|), and X1 = fma(-tau, s, x) rounds once more, by eps/2 |X1| <=
    eps/2 (|x| + tau (|g| + |u|)) (1 + eps): together at most eps (|x| + tau (|g| + |u|)), and the bound is twice that.
    Xbar = fma(2, X1, -x) rounds once (eps/2 |Xbar|) on top of twice X1's own error."""
    from pxmcmc_amd._lib import FISTA_SLICES_MAX

    assert FISTA_SLICES_MAX == SLICES_MAX
    X, G, U, tau = _primal_inputs(n, C, cplx, seed=500 + n % 1000 + 7 * C + cplx)
    X1, Xbar, _ = _run_primal(X, G, U, tau)
    e1, eb = pd_primal_ext(X, G, U, tau)
    b1 = 2 * EPS * (np.abs(_parts(X)) + tau * (np.abs(_parts(G)) + np.abs(_parts(U))))
    err1, errb = np.abs(_parts(X1) - e1), np.abs(_parts(Xbar) - eb)
    bb = EPS * np.abs(_parts(Xbar)) + 2 * b1
    print(f"n={n} C={C} cplx={cplx}: worst X1 error / bound {float((err1 / b1).max()):.3f}, Xbar {float((errb / bb).max()):.3f}")
    assert np.isfinite(_parts(X1).astype(float)).all() and np.all(err1 <= b1) and np.all(errb <= bb)


@pytest.mark.parametrize("n", [1, 255, 256, 257, N_STRIDE])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("vecT", [False, True], ids=["scalarT", "vectorT"])
def test_dual_step_against_the_long_double_model(n, C, cplx, vecT):
    """|V1 - exact| <= 4 eps max(|w|, r) on every element, none left out near |w| = r (the projection is continuous: taking
    the other branch there changes the result by the distance to the disc, itself a rounding error of |w|).  In units of
    eps/2: w = fma(sigma, W, V) 1, r = T rscale 1, a = sqrt(re^2 + im^2) 2 (three roundings under the root, halved, and the
    root's own), r / a 1, the product 1 -- at most 6, i.e. 3 eps, relative to max(|w|, r); real input only rounds w.
    The planted elements (test_pd_host.pd_dual_inputs) put some element on every branch."""
    V, W, T = pd_dual_inputs(n, C, cplx, vecT, seed=700 + n % 1000 + 7 * C + 2 * cplx + vecT)
    V1, _ = _run_dual(V, W, T)
    er, ei, a, r = pd_dual_ext(V, W, T, PD_SIGMA, PD_RSCALE)
    err = np.abs(V1.real - er) if ei is None else np.sqrt((V1.real - er) ** 2 + (V1.imag - ei) ** 2)
    bound = 4 * EPS * np.maximum(a, r)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0, np.inf))
    print(f"n={n} C={C} cplx={cplx} vecT={vecT}: worst error / bound {float(ratio.max()):.3f}")
    assert np.isfinite(V1.view(float)).all() and np.all(err <= bound)
    if n >= 255:
        hit = {"inside": (a < r) & (a > 0), "outside": (a > r) & (r > 0), "on": (a == r) & (r > 0), "zero": a == 0}
        if vecT:
            hit["T0"] = (r == 0) & (a > 0)
            assert np.all(V1[hit["T0"]] == 0)
        for name, where in hit.items():
            assert where.any(), name
        assert np.all(V1[hit["on"]] == (3 + 4j if cplx else 5)) and np.all(V1[hit["zero"]] == 0)
        exact_in = V[hit["inside"]] + PD_SIGMA * W[hit["inside"]]
        assert np.abs(V1[hit["inside"]] - exact_in).max() <= EPS * np.abs(exact_in).max()  # kept, not scaled


# ---- the per-chain sums ------------------------------------------------------------------------------------------------------
def _abs2(z):
    return np.real(z) ** 2 + np.imag(z) ** 2  # float64, every product and the sum rounded: the kernel's abs2_plain


def _ld_sum(terms):
    return np.array([t.astype(LD).sum() for t in terms])


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", [1, 257, N_STRIDE])
def test_per_chain_sums(n, cplx):
    """The sums against long-double sums of the terms of the kernel's own outputs, formed in float64 as the kernel forms them
    (differences, plain squares, T |W| with sqrt of the plain square sum): what is left is the error of adding n
    non-negative float64 terms in any order, at most (n - 1) eps/2 of their sum <= n eps sum |terms|.  And every chain of a
    batch of 3 -- outputs and sums -- is bit-identical to its solo launch."""
    C = 3
    X, G, U, tau = _primal_inputs(n, C, cplx, seed=900 + n % 1000 + cplx)
    X1, Xbar, ps = _run_primal(X, G, U, tau)
    V, W, T = pd_dual_inputs(n, C, cplx, True, seed=950 + n % 1000 + cplx)
    V1, ds = _run_dual(V, W, T)
    for c in range(C):
        want_p = _ld_sum([_abs2(X1[c] - X[c]), _abs2(X1[c])])
        want_d = _ld_sum([_abs2(V1[c] - V[c]), _abs2(V1[c]), T * np.sqrt(_abs2(W[c]))])
        for got, want in ((ps[c], want_p), (ds[c], want_d)):
            diff = np.abs(got.astype(LD) - want)
            print(f"n={n} cplx={cplx} chain {c}: |sum - long-double sum| / sum {(diff / np.where(want == 0, 1, want)).astype(float)} (bound {n * EPS:.3e})")
            assert np.all(diff <= n * EPS * want)
    sX1, sXbar, sps = _run_primal(X, G, U, tau, chains=range(C))
    sV1, sds = _run_dual(V, W, T, chains=range(C))
    assert np.array_equal(sX1, X1) and np.array_equal(sXbar, Xbar) and np.array_equal(sps, ps)
    assert np.array_equal(sV1, V1) and np.array_equal(sds, ds)


def test_empty_state_writes_zero_sums():
    import torch

    from pxmcmc_amd import ops

    for dt in (torch.float64, torch.complex128):
        x = torch.zeros((2, 0), dtype=dt, device=ops.device())
        ps = torch.full((2, 2), float("nan"), dtype=torch.float64, device=x.device)
        ds = torch.full((2, 3), float("nan"), dtype=torch.float64, device=x.device)
        ops.pd_primal_step(x, x.clone(), x.clone(), 0.1, out=(x.clone(), x.clone()), sums=ps)
        ops.pd_dual_step(x, x.clone(), 0.1, 0.5, 1.0, out=x.clone(), sums=ds)
        assert torch.equal(ps, torch.zeros_like(ps)) and torch.equal(ds, torch.zeros_like(ds))


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_launched():
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError, lib

    dev = ops.device()
    x = torch.ones((2, 8), dtype=torch.float64, device=dev)
    g, u = x.clone(), x.clone()
    o1, o2 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    ps = torch.full((2, 2), float("nan"), dtype=torch.float64, device=dev)
    ds = torch.full((2, 3), float("nan"), dtype=torch.float64, device=dev)
    scratch = ops.pd_scratch(2, dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731

    def primal(X=x, G=g, U=u, tau=0.1, X1=o1, Xb=o2, sums=ps, scr=scratch, n=8, C=2, dtype=0):
        return lib.pxm_pd_primal_step(p(X), p(G), p(U), tau, p(X1), p(Xb), p(sums), p(scr), n, C, dtype, st)

    def dual(V=x, W=g, T=None, Ts=0.1, sigma=0.5, rscale=1.0, V1=o1, sums=ds, scr=scratch, m=8, C=2, dtype=0):
        return lib.pxm_pd_dual_step(p(V), p(W), p(T), Ts, sigma, rscale, p(V1), p(sums), p(scr), m, C, dtype, st)

    refused = {
        "primal: X1 aliases X": lambda: primal(X1=x), "primal: Xbar aliases G": lambda: primal(Xb=g),
        "primal: X1 is Xbar": lambda: primal(Xb=o1), "primal: null X": lambda: primal(X=None),
        "primal: null sums": lambda: primal(sums=None), "primal: null scratch": lambda: primal(scr=None),
        "primal: null output": lambda: primal(X1=None), "primal: tau = 0": lambda: primal(tau=0.0),
        "primal: tau < 0": lambda: primal(tau=-0.1), "primal: tau nan": lambda: primal(tau=float("nan")),
        "primal: C > 65535": lambda: primal(C=65536), "primal: C = 0": lambda: primal(C=0), "primal: dtype": lambda: primal(dtype=2),
        "primal: n < 0": lambda: primal(n=-1),
        "dual: V1 aliases V": lambda: dual(V1=x), "dual: V1 aliases W": lambda: dual(V1=g), "dual: null W": lambda: dual(W=None),
        "dual: null sums": lambda: dual(sums=None), "dual: null scratch": lambda: dual(scr=None),
        "dual: null output": lambda: dual(V1=None), "dual: sigma = 0": lambda: dual(sigma=0.0),
        "dual: rscale < 0": lambda: dual(rscale=-1.0), "dual: T_scalar < 0": lambda: dual(Ts=-0.1),
        "dual: C > 65535": lambda: dual(C=65536), "dual: dtype": lambda: dual(dtype=-1),
    }
    for what, call in refused.items():
        assert call() < 0, what
        msg = lib.pxm_last_error().decode()
        assert msg.startswith("pxm_pd_primal_step" if what.startswith("primal") else "pxm_pd_dual_step"), (what, msg)
    torch.cuda.synchronize()
    for t in (o1, o2, ps, ds):
        assert torch.isnan(t).all()  # nothing ran
    assert torch.equal(x, torch.ones_like(x)) and torch.equal(g, x) and torch.equal(u, x)
    # through the wrappers: the library's refusal arrives as PxmError, the wrappers' own checks as ValueError / TypeError
    with pytest.raises(PxmError, match="alias"):
        ops.pd_primal_step(x, g, u, 0.1, out=(x, o2))
    with pytest.raises(PxmError, match="tau"):
        ops.pd_primal_step(x, g, u, 0.0)
    with pytest.raises(PxmError, match="alias"):
        ops.pd_dual_step(x, g, 0.1, 0.5, 1.0, out=x)
    with pytest.raises(ValueError):  # a result buffer of another dtype
        ops.pd_primal_step(x, g, u, 0.1, out=(o1.to(torch.complex128), o2.to(torch.complex128)))
    with pytest.raises(ValueError):
        ops.pd_dual_step(x, g, 0.1, 0.5, 1.0, out=o1.to(torch.complex128))
    with pytest.raises(ValueError):
        ops.pd_primal_step(x, g[:, :4], u, 0.1)
    with pytest.raises(ValueError):
        ops.pd_dual_step(x, g, None, 0.5, 1.0)
    with pytest.raises(ValueError):
        ops.pd_dual_step(x, g, torch.ones(5, dtype=torch.float64, device=dev), 0.5, 1.0)
    with pytest.raises(ValueError):
        ops.pd_dual_step(x, g, 0.1, 0.5, 1.0, sums=ps)  # [C, 2] instead of [C, 3]
    # and the valid calls go through
    assert primal() == 0 and dual(V1=o2) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(o1).all() and torch.isfinite(o2).all() and torch.isfinite(ps).all() and torch.isfinite(ds).all()


# ---- PrimalDual, identity case ----------------------------------------------------------------------------------------------
ID_NP_ITERS = 67  # iterations primal_dual_np needs for 1e-10 on the identity problem below (the slowest of the three starts)


@pytest.fixture(scope="module")
def ident():
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.transforms import IdentityTransform

    P, C, sig, lmda = 190, 3, 0.2, 1e-2
    rng = np.random.default_rng(31)
    d = rng.normal(size=P)
    T = lmda * 10.0 * rng.random(P)
    op = ForwardOperator(d, sig, "analysis", IdentityTransform(), Identity(P, P), nparams=P)
    reg = L1("analysis", None, None, T)
    X0 = np.stack([np.zeros(P), d.copy(), rng.normal(size=P) * 3])
    return dict(op=op, reg=reg, p=PxMCMCParams(lmda=lmda, mu=1.0, verbosity=0), d=d, T=T, ic=1 / sig ** 2, lmda=lmda, X0=X0, C=C, P=P)


def test_identity_case_iterates_equal_the_numpy_statement(ident):
    """40 iterations from three starts against primal_dual_np with the estimator's own steps.  One iteration is a few
    roundings of quantities of size `scale` in either route (numpy rounds the product and the sum where the kernel has one
    fma), and the iteration map is nonexpansive, so the differences add up: 40 x 8 eps x scale."""
    from pxmcmc_amd.optim import PrimalDual
    from pxmcmc_amd.optim_np import primal_dual_np

    w = ident
    est = PrimalDual(w["op"], w["reg"], w["p"], nchains=w["C"], tol=0.0, max_iter=40, check_every=40)
    assert est.A_norm2 == 1.0 and est.L_g == pytest.approx(w["ic"] * (1 + 1e-4), rel=1e-12)
    assert est.sigma == pytest.approx(0.5 * est.L_g) and est.tau == pytest.approx(1.0 / est.L_g)
    X = est.run(start_point=w["X0"])
    assert X.dtype == np.float64 and est.used_graph, est.graph_error
    ident_map = lambda a: a  # noqa: E731
    V = est.V_map.cpu().numpy()
    rmax = (w["T"] / w["lmda"]).max()
    for c in range(w["C"]):
        x, v, _ = primal_dual_np(lambda x: w["ic"] * (x - w["d"]), ident_map, ident_map, w["T"], w["lmda"], est.tau, est.sigma,
                                 w["X0"][c], 40)
        sx = np.abs(w["X0"][c]).max() + np.abs(w["d"]).max() + est.tau * rmax
        sv = rmax + est.sigma * sx
        ex, ev = np.abs(X[c] - x).max(), np.abs(V[c] - v).max()
        print(f"chain {c}: |x - numpy| {ex:.3e} (bound {320 * EPS * sx:.3e}), |v - numpy| {ev:.3e} (bound {320 * EPS * sv:.3e})")
        assert ex <= 40 * 8 * EPS * sx and ev <= 40 * 8 * EPS * sv


def test_identity_case_reaches_the_closed_form(ident):
    """tol = 1e-10: within sqrt(2 gap / ic) of soft(d, T sigma_d^2 / lmda) (the problem is ic-strongly convex; the gap is
    optim_np.duality_gap_np at the returned pair, plus its own rounding 64 eps P), and converged within twice the iterations
    the numpy statement needs"""
    from pxmcmc_amd.optim import PrimalDual
    from pxmcmc_amd.optim_np import duality_gap_np, primal_dual_np

    w = ident
    ident_map = lambda a: a  # noqa: E731
    est = PrimalDual(w["op"], w["reg"], w["p"], nchains=w["C"], tol=1e-10, max_iter=2 * ID_NP_ITERS, check_every=4)
    X = est.run(start_point=w["X0"])
    V = est.V_map.cpu().numpy()
    want = soft_np(w["d"], w["T"] / (w["lmda"] * w["ic"]))
    need = [primal_dual_np(lambda x: w["ic"] * (x - w["d"]), ident_map, ident_map, w["T"], w["lmda"], est.tau, est.sigma, x0, 1000,
                           tol=1e-10)[2]["niter"] for x0 in w["X0"]]
    print(f"numpy needs {need} iterations, the estimator stopped at {est.niter} (checks every 4)")
    assert est.converged.all() and np.all(est.niter <= 2 * ID_NP_ITERS) and np.all(est.niter <= 2 * max(need))
    Pval = 0.5 * w["ic"] * np.sum(w["d"] ** 2)
    for c in range(w["C"]):
        gap = duality_gap_np(X[c], V[c], w["d"], np.full(w["P"], w["ic"]), ident_map, ident_map, w["T"], w["lmda"])
        bound = np.sqrt(2 * (max(gap, 0) + 64 * EPS * Pval) / w["ic"])
        dist = np.linalg.norm(X[c] - want)
        print(f"chain {c}: gap {gap:.3e}, ||x - soft|| {dist:.3e}, bound {bound:.3e}")
        assert gap >= -64 * EPS * Pval and dist <= bound <= 1e-5 * np.linalg.norm(want)
    # the traces are what they say
    assert np.allclose(est.objective, est.data_term + est.prior_term, rtol=4 * EPS, atol=0)
    F = 0.5 * w["ic"] * np.sum((X - w["d"]) ** 2, axis=1) + np.sum(w["T"] * np.abs(X), axis=1) / w["lmda"]
    assert np.allclose(est.objective_map, F, rtol=w["P"] * EPS, atol=0)


# ---- PrimalDual, wavelet case -------------------------------------------------------------------------------------------------
WAV_NP_ITERS = 656  # iterations primal_dual_np needs for 1e-9 on oracle.pxmcmc_np transforms with the data of `wav` (both starts)
WAV_BALANCE = 10.0  # on this problem the dual is the slow variable: balance = 1 needs ~5600 iterations, 10 needs ~630


def _wav_problem():
    from oracle import pxmcmc_np as ref

    L, sig, lmda, mu = 16, 0.05, 1e-3, 10.0
    tr = ref.SphericalWaveletTransform(L, 2, 2)
    n = L * (2 * L - 1)
    rng = np.random.default_rng(11)
    m = tr.inverse_adjoint(np.zeros(n, complex)).size
    coef = np.where(rng.random(m) < 0.05, rng.normal(size=m), 0) + 0j
    data = tr.inverse(coef).real + sig * rng.normal(size=n)
    T = lmda * mu * (0.5 + rng.random(m))
    X0 = np.stack([np.zeros(n, complex), data + 0j])
    return dict(L=L, sig=sig, lmda=lmda, mu=mu, ref_tr=tr, n=n, m=m, data=data, T=T, X0=X0, ic=1 / sig ** 2)


@pytest.fixture(scope="module")
def wav():
    """the L = 16 denoising problem, its operators, and one converged run shared by the tests below (read only)"""
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.optim import PrimalDual
    from pxmcmc_amd.prior import L1

    w = _wav_problem()
    op = SphericalWaveletTransformOperator(w["data"], w["sig"], "analysis", w["L"], 2, 2, max_chains=2)
    tr = op.transform
    reg = L1("analysis", tr.inverse, tr.inverse_adjoint, w["T"])
    p = PxMCMCParams(lmda=w["lmda"], mu=w["mu"], verbosity=0)
    est = PrimalDual(op, reg, p, nchains=2, balance=WAV_BALANCE, tol=1e-9, max_iter=2 * WAV_NP_ITERS, check_every=10)
    X = est.run(start_point=w["X0"])
    w.update(op=op, tr=tr, reg=reg, p=p, est=est, X=X)
    return w


def _objective_dev(w, X):
    """F per chain through the device transforms and reductions, independently of the estimator's traces"""
    import torch

    from pxmcmc_amd import ops

    x = ops.as_device(X, torch.complex128)
    x = x if x.dim() == 2 else x[None]
    d = ops.as_device(w["data"], torch.complex128)
    g = 0.5 * w["ic"] * (x - d).abs().pow(2).sum(dim=1)
    u = ops.as_device(w["tr"].inverse_adjoint(x))
    h = (ops.as_device(w["T"], torch.float64) * u.abs()).sum(dim=1) / w["lmda"]
    return (g + h).cpu().numpy()


def test_wavelet_case_meets_the_optimality_conditions(wav):
    """converged within twice the numpy count; V is feasible; the residual gradg(X) + A^H V, formed through the transforms, is
    within (1 / tau + L_g) ||dX|| + ||A|| ||dV|| (the identity of tests/test_pd_host.py) plus 64 eps (||gradg|| + ||A^H V||) for
    forming it; the stationarity trace is sqrt(dx2) / tau; the objective is the sum of its two terms and equals F evaluated
    through the device transforms and through the oracle's"""
    import torch

    from pxmcmc_amd import ops

    w, est = wav, wav["est"]
    print(f"L = 16 wavelets: niter {est.niter}, objective {est.objective_map}, stationarity {est.stationarity[-1]}, "
          f"tau {est.tau:.4e} sigma {est.sigma:.4e} ||A||^2 {est.A_norm2:.4f} L_g {est.L_g:.4f}")
    assert est.used_graph, est.graph_error
    assert est.converged.all() and np.all(est.niter <= 2 * WAV_NP_ITERS)
    assert 1.0 / est.tau - est.sigma * est.A_norm2 >= 0.5 * est.L_g * (1 - 1e-12)
    X, V = est.X_map, est.V_map
    r = w["T"] / w["lmda"]
    assert V.shape == (2, w["m"]) and np.all(np.abs(V.cpu().numpy()) <= r * (1 + 4 * EPS))
    g = ops.as_device(w["op"].calc_gradg(ops.as_device(w["op"].forward(X))), X.dtype)
    aHv = ops.as_device(w["tr"].inverse(V), X.dtype)
    res = torch.linalg.norm(g + aHv, dim=1).cpu().numpy()
    scale = (torch.linalg.norm(g, dim=1) + torch.linalg.norm(aHv, dim=1)).cpu().numpy()
    bound = (1 / est.tau + est.L_g) * est.last_steps[:, 0] + np.sqrt(est.A_norm2) * est.last_steps[:, 1] + 64 * EPS * scale
    print(f"||gradg + A^H V|| {res}, bound {bound}, ||gradg|| + ||A^H V|| {scale}")
    assert np.all(res <= bound) and np.all(bound <= 1e-6 * scale)
    assert np.allclose(est.stationarity[-1], est.last_steps[:, 0] / est.tau, rtol=2 * EPS, atol=0)
    assert np.allclose(est.objective, est.data_term + est.prior_term, rtol=4 * EPS, atol=0)
    assert est.objective.shape == (len(est.checks), 2) == est.rel_change_dual.shape
    # F through the device transforms: sums of n and m terms against the two-stage reductions
    assert np.allclose(est.objective_map, _objective_dev(w, X), rtol=(w["n"] + w["m"]) * EPS, atol=0)
    # and through the oracle's transforms, which the device transforms match to 1e-12 relative
    x = X.cpu().numpy()
    A = w["ref_tr"].inverse_adjoint
    F_np = [0.5 * w["ic"] * np.sum(np.abs(xc - w["data"]) ** 2) + np.sum(w["T"] * np.abs(A(xc))) / w["lmda"] for xc in x]
    assert np.allclose(est.objective_map, F_np, rtol=1e-11, atol=0)
    # both starts reach the same minimum value (F is convex); the minimiser is unique (g is strongly convex)
    assert abs(est.objective_map[0] - est.objective_map[1]) <= 1e-9 * est.objective_map[0]
    assert np.linalg.norm(x[0] - x[1]) <= 1e-6 * np.linalg.norm(x[0])


def test_wavelet_case_numpy_count(wav):
    """the recorded count: primal_dual_np on the oracle's transforms with the same data and the estimator's steps"""
    from pxmcmc_amd.optim_np import primal_dual_np

    w, est = wav, wav["est"]
    tr = w["ref_tr"]
    x, v, info = primal_dual_np(lambda x: w["ic"] * (x - w["data"]), tr.inverse_adjoint, tr.inverse, w["T"], w["lmda"], est.tau,
                                est.sigma, w["X0"][0], 2 * WAV_NP_ITERS, tol=1e-9)
    print(f"numpy: {info['niter']} iterations (recorded {WAV_NP_ITERS}), device: {est.niter}")
    assert info["converged"] and info["niter"] <= WAV_NP_ITERS
    assert np.linalg.norm(x - w["X"][0]) <= 1e-6 * np.linalg.norm(x)


def test_wavelet_case_beats_fista_and_nearby_points(wav):
    """F at the returned point is no larger than at the point FISTA returns for the same operators under its warning (the
    tight-frame prox: a different fixed point), and F(x) <= F(x + delta) + ||residual|| ||delta|| for 8 random perturbations
    of relative size 1e-3 (convexity, with residual = gradg + A^H V)"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.optim import FISTA

    w, est = wav, wav["est"]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fi = FISTA(w["op"], w["reg"], w["p"], nchains=2, tol=1e-6, max_iter=400, check_every=20)
    assert any("not the stock synthesis L1" in str(c.message) for c in caught)
    Xf = fi.run(start_point=w["X0"])
    F_pd, F_fi = est.objective_map, _objective_dev(w, Xf)
    print(f"F at the primal-dual point {F_pd}, at FISTA's point {F_fi} ({fi.niter} iterations), at the data {_objective_dev(w, w['X0'][1])}")
    assert np.all(F_pd <= F_fi)
    X, V = est.X_map, est.V_map
    g = ops.as_device(w["op"].calc_gradg(ops.as_device(w["op"].forward(X))), X.dtype)
    res = torch.linalg.norm(g + ops.as_device(w["tr"].inverse(V), X.dtype), dim=1).cpu().numpy()
    rng = np.random.default_rng(12)
    x = X.cpu().numpy()
    for k in range(8):
        delta = rng.normal(size=x.shape) + 1j * rng.normal(size=x.shape)
        delta *= 1e-3 * np.linalg.norm(x, axis=1, keepdims=True) / np.linalg.norm(delta, axis=1, keepdims=True)
        assert np.all(F_pd <= _objective_dev(w, x + delta) + res * np.linalg.norm(delta, axis=1)), k


def test_wavelet_case_graph_replay_equals_eager(wav):
    from pxmcmc_amd.optim import PrimalDual

    w = wav
    runs = {}
    for graph in (True, False):
        est = PrimalDual(w["op"], w["reg"], w["p"], nchains=2, balance=WAV_BALANCE, tol=0.0, max_iter=45, check_every=15,
                         use_graph=graph)
        X = est.run(start_point=w["X0"])
        assert est.used_graph == graph, est.graph_error
        runs[graph] = (X, est)
    (X, a), (Xe, b) = runs[True], runs[False]
    assert np.array_equal(X, Xe) and np.array_equal(a.V_map.cpu().numpy(), b.V_map.cpu().numpy())
    for k in ("objective", "data_term", "prior_term", "rel_change", "rel_change_dual", "stationarity", "last_steps"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.checks == [15, 30, 45] and not a.converged.any()
    # one chain, a tensor start: the caller's kind and shape back
    import torch

    one = PrimalDual(w["op"], w["reg"], w["p"], balance=WAV_BALANCE, tol=1e-3, max_iter=200)
    x1 = one.run(start_point=torch.zeros(w["n"], dtype=torch.complex128))
    assert isinstance(x1, torch.Tensor) and x1.is_cuda and x1.shape == (w["n"],)


def test_operator_norm2_against_the_dense_value(wav):
    """within the power iteration's tolerance of the largest eigenvalue of A^H A, A dense from the oracle's inverse_adjoint,
    and never above it"""
    import torch

    from pxmcmc_amd.optim import operator_norm2

    w = wav
    A = np.stack([w["ref_tr"].inverse_adjoint(e) for e in np.eye(w["n"], dtype=complex)], axis=1)
    dense = np.linalg.norm(A, 2) ** 2
    tol = 1e-4
    got = operator_norm2(w["tr"].inverse, w["tr"].inverse_adjoint, w["n"], torch.complex128, iters=1000, tol=tol)
    print(f"||A||^2: power iteration {got:.8f}, dense {dense:.8f}, relative gap {(dense - got) / dense:.3e}")
    assert isinstance(got, float) and got <= dense * (1 + 1e-10) and dense - got <= tol * dense
    assert w["est"].A_norm2 == pytest.approx(got * (1 + tol), rel=1e-12)
    assert operator_norm2(None, None, 5) == 1.0
    with pytest.warns(UserWarning, match="operator_norm2.*did not reach"):
        assert operator_norm2(w["tr"].inverse, w["tr"].inverse_adjoint, w["n"], torch.complex128, iters=4, tol=1e-12) <= got


# ---- refusals of the estimator ------------------------------------------------------------------------------------------------
def test_primal_dual_refuses_what_it_cannot_solve(wav, ident):
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.optim import PrimalDual
    from pxmcmc_amd.prior import L1

    w = wav
    syn = SphericalWaveletTransformOperator(w["data"], w["sig"], "synthesis", 16, 2, 2)
    with pytest.raises(ValueError, match="analysis-setting operator"):
        PrimalDual(syn, w["reg"], w["p"])

    class NoT:
        fwd = adj = None

        def proxf(self, X):
            return X

    with pytest.raises(ValueError, match="threshold T"):
        PrimalDual(w["op"], NoT(), w["p"])
    with pytest.raises(ValueError, match="entries"):
        PrimalDual(w["op"], L1("analysis", w["tr"].inverse, w["tr"].inverse_adjoint, w["T"][:-1]), w["p"])
    est = w["est"]
    with pytest.raises(ValueError, match="1 / tau - sigma"):
        PrimalDual(w["op"], w["reg"], w["p"], tau=est.tau * 1.01, sigma=est.sigma)
    with pytest.raises(ValueError, match="1 / tau - sigma"):
        PrimalDual(w["op"], w["reg"], w["p"], tau=4.0 / est.L_g)  # 1 / tau < L_g / 2: no positive sigma
    with pytest.raises(ValueError, match="1 / tau - sigma"):
        PrimalDual(ident["op"], ident["reg"], ident["p"], sigma=-1.0)
    ok = PrimalDual(w["op"], w["reg"], w["p"], tau=est.tau * 0.5, sigma=est.sigma)  # inside the condition
    assert ok.tau == est.tau * 0.5 and ok.sigma == est.sigma
    one = PrimalDual(w["op"], w["reg"], w["p"], tau=est.tau)  # sigma from the condition with equality: the one est.tau came from
    assert one.sigma == pytest.approx(est.sigma, rel=1e-9)


# ---- the exact analysis prox ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_analysis_prox_identity_equals_soft(cplx):
    """A = I: the dual iteration is at its fixed point after one step (sigma = 1, exactly), Z - proj(Z) = soft(Z, T), to
    2 eps |Z| per element (the two routes round the same value differently: z - z (T / |z|) against z (|z| - T) / |z|)"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.optim import analysis_prox
    from pxmcmc_amd.prior import L1, L1_Analysis

    rng = np.random.default_rng(41 + cplx)
    Z = rng.normal(size=(2, 333)) + (1j * rng.normal(size=(2, 333)) if cplx else 0)
    T = rng.random(333)
    T[::9] = 0
    want = ops.soft(ops.as_device(Z), ops.as_device(T, torch.float64)).cpu().numpy()
    for iters in (1, 5):
        got = analysis_prox(L1("analysis", None, None, T), Z, iters)
        assert isinstance(got, np.ndarray) and got.shape == Z.shape
        ratio = (np.abs(got - want) / (2 * EPS * np.abs(Z))).max()
        print(f"cplx={cplx} iters={iters}: worst |prox - soft| / (2 eps |Z|) = {ratio:.3f}")
        assert ratio <= 1
    reg = L1_Analysis(None, None, T, prox_iters=3)
    assert np.array_equal(reg.proxf(Z), analysis_prox(reg, Z, 3))
    z1 = ops.as_device(Z[0])
    p1 = reg.proxf(z1)
    assert isinstance(p1, torch.Tensor) and p1.shape == z1.shape and np.array_equal(p1.cpu().numpy(), reg.proxf(Z)[0])
    pr = reg.prior(Z)
    assert isinstance(pr, torch.Tensor) and np.allclose(pr.cpu().numpy(), (T * np.abs(Z)).sum(axis=1), rtol=333 * EPS)
    assert isinstance(reg.prior(Z[0]), float)


def test_analysis_prox_on_wavelets(wav):
    """L = 16: 16 iterations equal analysis_prox_np on the oracle's transforms (33 transform pairs that agree to 1e-12
    relative, amplified by at most sigma ||A||^2 < 1 per iteration: 1e-10 of max |Z|); ||Z - A^H v_k|| does not increase over
    k = 1 ... 32 (descent of the dual objective; 8 eps ||Z|| for the rounding of the norms); after 64 iterations the prox
    objective is below that of Z and of the tight-frame formula L1.proxf(Z)"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.optim import analysis_prox
    from pxmcmc_amd.optim_np import analysis_prox_np
    from pxmcmc_amd.prior import L1

    w = wav
    rng = np.random.default_rng(43)
    Z = w["data"] + 0.05 * (rng.normal(size=(2, w["n"])) + 1j * rng.normal(size=(2, w["n"])))
    T = 20.0 * w["T"]  # lmda mu weights with lmda = 2e-2: a prox that moves the point
    reg = L1("analysis", w["tr"].inverse, w["tr"].inverse_adjoint, T)
    A, AH = w["ref_tr"].inverse_adjoint, w["ref_tr"].inverse
    p16, v16 = analysis_prox(reg, Z, 16, return_dual=True)
    sigma = reg._prox_sigma[(w["n"], torch.complex128)]
    assert sigma == pytest.approx(1.0 / w["est"].A_norm2, rel=1e-12)
    assert np.all(np.abs(v16.cpu().numpy()) <= T * (1 + 4 * EPS))
    for c in range(2):
        want = analysis_prox_np(A, AH, T, Z[c], 16, sigma)
        err = np.abs(p16[c] - want).max()
        print(f"chain {c}: |prox - numpy| {err:.3e}, max |Z| {np.abs(Z[c]).max():.3f}, moved {np.abs(want - Z[c]).max():.3e}")
        assert err <= 1e-10 * np.abs(Z[c]).max() and np.abs(want - Z[c]).max() > 1e-3
    assert np.array_equal(analysis_prox(reg, Z, 16), p16)  # a pure function of Z
    norms = np.array([np.linalg.norm(analysis_prox(reg, Z, k), axis=1) for k in (1, 2, 4, 8, 16, 32)])
    print("||Z - A^H v_k||, k = 1 ... 32:", norms.T)
    assert np.all(np.diff(norms, axis=0) <= 8 * EPS * np.linalg.norm(Z, axis=1))

    def F(P):
        return 0.5 * np.linalg.norm(P - Z, axis=1) ** 2 + np.array([np.sum(T * np.abs(A(q))) for q in P])

    tight = reg.proxf(Z)
    F_z, F_tight, F_64 = F(Z), F(tight), F(analysis_prox(reg, Z, 64))
    print(f"prox objective: Z {F_z}, tight-frame formula {F_tight}, 64 dual iterations {F_64}")
    assert np.all(F_64 < F_z) and np.all(F_64 < F_tight)


def test_myula_with_the_exact_analysis_prox():
    """L = 10, 2 chains, 20 iterations with L1_Analysis(prox_iters=4): the replayed chain equals the eager one bit for bit
    (the prox is a pure function on fixed launches) and the state stays finite"""
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams
    from pxmcmc_amd.prior import L1_Analysis

    L, C = 10, 2
    rng = np.random.default_rng(51)
    P = L * (2 * L - 1)
    data = rng.normal(size=P)
    lmda, mu, sig = 1e-2, 1.0, 0.5
    delta = 0.8 / (1 / sig ** 2 + 1 / lmda)
    op = SphericalWaveletTransformOperator(data, sig, "analysis", L, 2, 2, max_chains=C)
    reg = L1_Analysis(op.transform.inverse, op.transform.inverse_adjoint, lmda * mu, prox_iters=4)
    assert reg.setting == "analysis" and reg.prox_iters == 4
    p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, nsamples=20, nburn=0, ngap=1, verbosity=0)
    runs = {}
    for graph in (True, False):
        s = MYULA(op, reg, p, nchains=C, seed=6, use_graph=graph)
        _quiet(s.run, start_point=0.1 * data)
        assert s.used_graph == graph, s.graph_error
        runs[graph] = (np.asarray(s.chain).copy(), s.X_curr.cpu().numpy().copy(), np.asarray(s.logPi).copy())
    for a, b in zip(runs[True], runs[False]):
        assert np.isfinite(a.view(float)).all() and np.array_equal(a, b)
    assert np.abs(runs[True][0]).max() < 1e3
