"""The FISTA MAP estimator on the GPU: the fused step kernel (pxm_fista_step) against the extended-precision model of
tests/test_fista_host.py on every element of every chain, its per-chain sums, ForwardOperator.gradient_lipschitz against
dense eigenvalues, FISTA.run (fixed point, graph replay, monotone forward-backward, every operator family) and the MAP
point as a sampler's start."""
import contextlib
import io

import numpy as np
import pytest

from conftest import golden
from test_fista_host import (C0_MEASURED, EPS, error_scale, fista_step_ext, ratio_to_ext, step_inputs, step_sums_np)

pytestmark = pytest.mark.gpu

C_BOUND = 4 * C0_MEASURED  # the margin tests/test_gpu_harmwav_step.py gives its kernel over its numpy route: device sqrt / division
C_MAX = 5  # chains the buffers are allocated for
# stopping tolerance of the FISTA runs: the steps of plain FISTA shrink like 1 / k only, so a rule
# that a few thousand iterations of these small problems can meet
TOL = 1e-3


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _run_step(inp, C, beta_tab, it, it_dev, proxf=None, chains=None):
    """the kernel on chains [0, C) (or the listed ones, one launch each) of buffers allocated for C_MAX, outputs prefilled
    with NaN -> (X1, Y1, sums) as numpy"""
    import torch

    from pxmcmc_amd import ops

    Y, g, X0, gamma, T, lmda, _ = inp
    n = Y.shape[1]
    dev = ops.device()
    dt = torch.complex128 if np.iscomplexobj(Y) else torch.float64

    def buf(a=None):
        t = torch.full((C_MAX, n), float("nan"), dtype=dt, device=dev)
        if a is not None:
            t[: a.shape[0]] = ops.as_device(a, dt)
        return t

    bY, bg, bX0, bX1, bY1 = buf(Y), buf(g), buf(X0), buf(), buf()
    bP = buf(proxf) if proxf is not None else None
    sums = torch.full((C_MAX, 3), float("nan"), dtype=torch.float64, device=dev)
    beta = ops.as_device(np.asarray(beta_tab, dtype=float), torch.float64)
    cnt = torch.full((1,), int(it_dev), dtype=torch.int64, device=dev)
    Tdev = ops.as_device(T, torch.float64) if np.ndim(T) else float(T)
    for sl in ([slice(0, C)] if chains is None else [slice(c, c + 1) for c in chains]):
        kw = dict(it=it, iter_dev=cnt, out=(bX1[sl], bY1[sl]), sums=sums[sl])
        if proxf is None:
            ops.fista_step(bY[sl], bg[sl], bX0[sl], gamma, lmda, beta, T=Tdev, **kw)
        else:
            ops.fista_step(None, None, bX0[sl], gamma, lmda, beta, proxf=bP[sl], **kw)
    torch.cuda.synchronize()
    assert torch.isnan(bX1[C:].real).all() and torch.isnan(bY1[C:].real).all() and torch.isnan(sums[C:]).all()  # nothing past C
    return bX1[:C].cpu().numpy(), bY1[:C].cpu().numpy(), sums[:C].cpu().numpy()


BETA_LONG = np.linspace(0.05, 0.95, 12)  # it + iter_dev = 7 -> 0.05 + 7 * 0.9 / 11
BETA_SHORT = np.array([0.1, 0.2, 0.3, 0.4, 0.61])  # shorter than it + iter_dev: the last entry


@pytest.mark.parametrize("n", [1, 255, 257, 4097])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("vecT", [False, True], ids=["scalarT", "vectorT"])
def test_one_step_against_extended_model(n, C, cplx, vecT):
    """every element of every chain within 4 x C0_MEASURED x 2^-52 S_e of the extended-precision model; non-zero it and
    iter_dev, with a table longer and a table shorter than it + iter_dev (the clamp)"""
    inp = step_inputs(n, C, cplx, vecT, seed=100 + n + 7 * C + 2 * cplx + vecT)
    Y, g, X0, gamma, T, lmda, _ = inp
    worst = 0.0
    for tab, beta in ((BETA_LONG, BETA_LONG[7]), (BETA_SHORT, BETA_SHORT[-1])):
        X1, Y1, _ = _run_step(inp, C, tab, it=3, it_dev=4)
        assert np.isfinite(X1.view(float)).all() and np.isfinite(Y1.view(float)).all()
        eX, eY = fista_step_ext(Y, g, X0, gamma, T, lmda, beta)
        S = error_scale(Y, g, X0, X1, gamma, T, lmda, beta)
        worst = max(worst, ratio_to_ext(X1, eX, S), ratio_to_ext(Y1, eY, S))
        if vecT and n >= 8:
            assert np.all(X1[:, 2::7] == 0) and np.all(X1[:, 5::35] != 0)  # thresholds above every |V|; T = 0 keeps V
    print(f"n={n} C={C} cplx={cplx} vecT={vecT}: worst ratio {worst:.3f} (bound {C_BOUND:.2f})")
    assert worst <= C_BOUND


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", [1, 257, 4097, 70001])
def test_per_chain_sums(n, cplx):
    """the three sums against float64 numpy sums of the kernel's own outputs: at most n additions of non-negative terms
    that the kernel and numpy form identically -> n 2^-52 relative; and every chain bit-equal to the same chain run alone
    (70001: more than PXM_FISTA_SLICES_MAX workgroups' worth, the grid-stride path)"""
    C = 3
    inp = step_inputs(n, C, cplx, True, seed=300 + n + cplx)
    Y, g, X0, gamma, T, lmda, _ = inp
    X1, Y1, sums = _run_step(inp, C, BETA_LONG, it=0, it_dev=2)
    Tn = T if n > 1 else float(T[0])
    for c in range(C):
        want = step_sums_np(X1[c], X0[c], Tn)
        rel = np.abs(sums[c] - want) / np.where(want == 0, 1, want)
        print(f"n={n} cplx={cplx} chain {c}: relative difference of the sums {rel} (bound {n * EPS:.3e})")
        assert np.all(rel <= n * EPS)
    aX1, aY1, asums = _run_step(inp, C, BETA_LONG, it=0, it_dev=2, chains=range(C))
    assert np.array_equal(aX1, X1) and np.array_equal(aY1, Y1) and np.array_equal(asums, sums)


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_given_prox_equals_stock_form(cplx):
    """proxf = ops.soft(Y - gamma g, gamma T / lmda), with V formed by the stage kernel's fma, gives the stock form's X1 and
    Y1 bit for bit and its first two sums; the prior sum is NaN"""
    import torch

    from pxmcmc_amd import ops

    n, C = 1031, 2
    inp = step_inputs(n, C, cplx, True, seed=17 + cplx)
    Y, g, X0, gamma, T, lmda, _ = inp
    X1, Y1, sums = _run_step(inp, C, BETA_LONG, it=5, it_dev=0)
    V = ops.skrock_stage(ops.as_device(Y), 1.0, c=-gamma, gradg=ops.as_device(g))
    P = ops.soft(V, ops.as_device(T, torch.float64) * (gamma / lmda)).cpu().numpy()
    pX1, pY1, psums = _run_step(inp, C, BETA_LONG, it=5, it_dev=0, proxf=P)
    assert np.array_equal(pX1, X1) and np.array_equal(pY1, Y1)
    assert np.array_equal(psums[:, :2], sums[:, :2]) and np.isnan(psums[:, 2]).all() and np.isfinite(sums).all()


def test_bad_arguments_are_refused():
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError

    x = torch.zeros((2, 8), dtype=torch.float64, device=ops.device())
    with pytest.raises(PxmError):
        ops.fista_step(x, x.clone(), x.clone(), 0.1, 0.1, [0.0], T=0.1, out=(x, x.clone()))  # X_out aliases Y
    with pytest.raises(ValueError):
        ops.fista_step(x, x.clone(), x.clone(), 0.1, 0.1, [0.0])  # neither T nor proxf


# ---- gradient_lipschitz -------------------------------------------------------------------------------------------------
def _dense_gradient_matrix(op, dt):
    """A = the linear part of x -> calc_gradg(forward(x)), column by column through the operator's own calls"""
    import torch

    from pxmcmc_amd import ops

    n = op.nparams
    call = lambda v: ops.as_device(op.calc_gradg(ops.as_device(op.forward(v))), dt)  # noqa: E731
    e = torch.zeros(n, dtype=dt, device=ops.device())
    g0 = call(e)
    A = np.empty((n, n), dtype=complex if dt == torch.complex128 else float)
    for i in range(n):
        e[i] = 1
        A[:, i] = (call(e) - g0).cpu().numpy()
        e[i] = 0
    return A


def _lipschitz_cases():
    import scipy.sparse as sp
    import torch

    from pxmcmc_amd.forward import ForwardOperator, PathIntegralOperator, SphericalWaveletTransformOperator
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.transforms import IdentityTransform

    rng = np.random.default_rng(2)
    yield "wavelets", SphericalWaveletTransformOperator(rng.normal(size=16 * 31), 0.05, "synthesis", 16, 2, 2), torch.complex128
    A = sp.random(60, 190, density=0.1, random_state=np.random.RandomState(2), format="csr")
    yield "path", PathIntegralOperator(A, rng.normal(size=60), 0.2, "synthesis", 10, 2, 2), torch.complex128
    g = golden("g12_full_covariance.npz")
    P = g["cov"].shape[0]
    yield "fullcov", ForwardOperator(g["data_r"], g["cov"], "synthesis", IdentityTransform(), Identity(P, P), nparams=P), torch.float64


@pytest.mark.parametrize("which", ["wavelets", "path", "fullcov"])
def test_gradient_lipschitz_against_dense_eigenvalue(which):
    """within the iteration's tolerance of the largest eigenvalue of the dense matrix, and never above it (the estimates
    approach it from below)"""
    name, op, dt = next(c for c in _lipschitz_cases() if c[0] == which)
    tol = 1e-4
    Lg = op.gradient_lipschitz(iters=1000, tol=tol)
    A = _dense_gradient_matrix(op, dt)
    assert np.abs(A - A.conj().T).max() <= 1e-9 * np.abs(A).max()
    lam = np.linalg.eigvalsh((A + A.conj().T) / 2)[-1]
    print(f"{name}: n = {op.nparams}, L_g = {Lg:.10e}, largest eigenvalue {lam:.10e}, relative gap {(lam - Lg) / lam:.3e}")
    assert isinstance(Lg, float)
    assert Lg <= lam * (1 + 1e-10) and lam - Lg <= tol * lam
    assert op.gradient_lipschitz(iters=1000, tol=tol) == Lg and op.gradient_lipschitz(iters=1000, tol=tol, seed=1) != Lg  # seeded start
    with pytest.warns(UserWarning, match="did not reach"):
        assert op.gradient_lipschitz(iters=4, tol=1e-12) <= Lg


# ---- FISTA.run ----------------------------------------------------------------------------------------------------------
def _fixed_point_residual(est, X):
    """||X - P(X)|| per chain with the estimator's own operators, P the step map"""
    import torch

    from pxmcmc_amd import ops

    x = ops.as_device(X, est.X_map.dtype)
    x = x if x.dim() == 2 else x[None]
    f = est.gradient_op
    g = ops.as_device(f.calc_gradg(ops.as_device(f.forward(x))), x.dtype)
    V = x - est.gamma * g
    if est._stock_prox:
        T = est.prior.T_dev
        P = ops.soft(V, (T if isinstance(T, float) else T.to(torch.float64)) * (est.gamma / est.lmda))
    else:
        P = ops.as_device(est.prior.proxf(V), x.dtype)
    scale = torch.linalg.norm(x, dim=1) + est.gamma * torch.linalg.norm(g, dim=1)
    return torch.linalg.norm(x - P, dim=1).cpu().numpy(), torch.linalg.norm(x, dim=1).cpu().numpy(), scale.cpu().numpy()


def _assert_fixed_point(est, X, what):
    """The step map P is nonexpansive for gamma <= 1 / L_g and X_K = P(X_{K-1} + beta (X_{K-1} - X_{K-2})), beta < 1, so
    ||X_K - P(X_K)|| <= ||X_K - X_{K-1}|| + ||X_{K-1} - X_{K-2}||, where the stopping rule gives the first term
    <= tol ||X_K||; both step lengths are the kernel's own sums.  64 eps (||X|| + gamma ||grad||) covers the rounding of
    evaluating P once more."""
    res, nx, scale = _fixed_point_residual(est, X)
    steps = est.last_steps
    bound = steps[:, 0] + steps[:, 1] + 64 * EPS * scale
    print(f"{what}: niter {est.niter}, residual / ||X|| {res / nx}, bound / ||X|| {bound / nx}, rel_change {est.rel_change[-1]}")
    assert est.converged.all(), (what, est.rel_change[-1])
    assert np.all(steps[:, 0] <= est.tol * nx * (1 + 4 * EPS))
    assert np.all(res <= bound), (what, res, bound)


@pytest.fixture(scope="module")
def wav16():
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.prior import S2_Wavelets_L1

    L, B, J_min, C = 16, 2, 2, 3
    rng = np.random.default_rng(5)
    data = rng.normal(size=L * (2 * L - 1))
    lmda, mu = 1e-3, 1.0
    op = SphericalWaveletTransformOperator(data, 0.05, "synthesis", L, B, J_min, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, lmda * mu, L=L, B=B, J_min=J_min)
    p = PxMCMCParams(lmda=lmda, mu=mu, verbosity=0)
    n = op.nparams
    X0 = np.stack([np.zeros(n, dtype=complex), (rng.normal(size=n) + 1j * rng.normal(size=n)) * 0.1, rng.normal(size=n) * 0.5 + 0j])
    gamma = 1.0 / (op.gradient_lipschitz(iters=1000, tol=1e-4) * (1 + 1e-4))
    return dict(op=op, reg=reg, p=p, X0=X0, C=C, gamma=gamma)


def test_run_converges_to_a_fixed_point_and_graph_equals_eager(wav16):
    from pxmcmc_amd.optim import FISTA

    w = wav16
    runs = {}
    for graph in (True, False):
        est = FISTA(w["op"], w["reg"], w["p"], nchains=w["C"], gamma=w["gamma"], tol=TOL, max_iter=5000, check_every=10,
                    use_graph=graph)
        X = est.run(start_point=w["X0"])
        assert isinstance(X, np.ndarray) and X.shape == w["X0"].shape
        assert est.used_graph == graph, est.graph_error
        runs[graph] = (X, est)
    X, est = runs[True]
    _assert_fixed_point(est, X, "L = 16 wavelets, 3 chains")
    Xe, este = runs[False]
    assert np.array_equal(X, Xe) and np.array_equal(est.niter, este.niter)
    for k in ("objective", "data_term", "prior_term", "rel_change", "last_steps"):
        assert np.array_equal(getattr(est, k), getattr(este, k)), k
    # the three start points reach the same minimum value (F is convex) and the traces are what they say
    assert np.allclose(est.objective, est.data_term + est.prior_term, rtol=4 * EPS, atol=0)
    print("objective at the three MAP points:", est.objective_map)
    # the gamma = None path takes the same step
    assert FISTA(w["op"], w["reg"], w["p"], nchains=1).gamma == pytest.approx(w["gamma"], rel=1e-12)
    # one chain, a tensor start: the caller's kind and shape back
    import torch

    one = FISTA(w["op"], w["reg"], w["p"], gamma=w["gamma"], tol=TOL, max_iter=5000)
    x1 = one.run(start_point=torch.zeros(w["op"].nparams, dtype=torch.complex128))
    assert isinstance(x1, torch.Tensor) and x1.is_cuda and x1.shape == (w["op"].nparams,) and one.converged.all()


def test_forward_backward_objective_never_increases(wav16):
    from pxmcmc_amd.optim import FISTA

    w = wav16
    est = FISTA(w["op"], w["reg"], w["p"], nchains=w["C"], gamma=w["gamma"], momentum=False, tol=0.0, max_iter=60, check_every=1)
    est.run(start_point=w["X0"])
    F = est.objective
    assert F.shape == (60, w["C"]) and not est.converged.any()
    # monotone up to the rounding of the two values compared: each a sum of at most n terms, n eps F
    slack = 2 * w["op"].nparams * EPS * np.abs(F[:-1])
    print("forward-backward: largest increase of F relative to F:", (np.diff(F, axis=0) / np.abs(F[:-1])).max())
    assert np.all(np.diff(F, axis=0) <= slack)
    assert np.all(F[-1] < F[0])


def _small_case(which):
    from pxmcmc_amd.forward import ForwardOperator, SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.measurements import WeakLensingHarmonic
    from pxmcmc_amd.prior import L1, S2_Wavelets_L1
    from pxmcmc_amd.transforms import SphericalWaveletTransform

    rng = np.random.default_rng(21)
    cplx = lambda n: rng.normal(size=n) + 1j * rng.normal(size=n)  # noqa: E731
    lmda, mu = 2e-3, 1.0
    # complex data with a real sig_d, as the examples build them: the complex-variance rule (pxmcmc/forward.py:81-82) makes
    # the inverse covariance complex, and FISTA takes its gradient on the operator with Re(invcov)
    sig = 0.1
    if which in ("harmonic", "analysis"):
        L = 16 if which == "analysis" else 8
        tr = SphericalWaveletTransform(L, 2.0, 2, harmonic=True)
        data = cplx(L * L)
        data[:4] = 0
        if which == "harmonic":
            op = ForwardOperator(data, sig, "synthesis", transform=tr, measurement=WeakLensingHarmonic(L), nparams=tr.ncoefs)
            reg = L1("synthesis", None, None, lmda * mu * 0.5)
        else:  # analysis prox X + S (soft - 1) S^H X: nonexpansive since ||S|| <= 1 for the harmonic tiling
            op = ForwardOperator(data, sig, "analysis", transform=tr, measurement=WeakLensingHarmonic(L), nparams=L * L)
            reg = L1("analysis", tr.inverse, tr.inverse_adjoint, lmda * mu * 0.5)
    elif which == "weaklensing":  # examples/weaklensing_synthetic.py in miniature: masked shear data, per-pixel sig_d
        from pxmcmc_amd.measurements import WeakLensing
        from pxmcmc_amd.utils import build_mask

        L = 10
        mask = build_mask(L, size=20.0)
        wl = WeakLensing(L, mask, ngal=np.full_like(mask, 30))
        tr = SphericalWaveletTransform(L, 2, 2)
        op = ForwardOperator(cplx(wl.ndata) * 0.05, 1 / wl.inv_cov, "synthesis", transform=tr, measurement=wl, nparams=tr.ncoefs)
        reg = S2_Wavelets_L1("synthesis", None, None, lmda * mu, L=L, B=2, J_min=2)
    elif which == "dirs2":
        L = 8
        op = SphericalWaveletTransformOperator(rng.normal(size=L * (2 * L - 1)), 0.1, "synthesis", L, 2, 2, dirs=2)
        reg = S2_Wavelets_L1("synthesis", None, None, lmda * mu, L=L, B=2, J_min=2, dirs=2)
    else:  # spin 2
        L = 8
        op = SphericalWaveletTransformOperator(cplx(L * (2 * L - 1)), sig, "synthesis", L, 2, 2, spin=2)
        reg = S2_Wavelets_L1("synthesis", None, None, lmda * mu, L=L, B=2, J_min=2, spin=2)
    p = PxMCMCParams(lmda=lmda, mu=mu, complex=which not in ("dirs2", "weaklensing"), verbosity=0)
    return op, reg, p, cplx(op.nparams) * 0.1


@pytest.mark.parametrize("which", ["analysis", "dirs2", "spin2", "harmonic", "weaklensing"])
def test_fixed_point_on_every_operator_family(which):
    import warnings

    from pxmcmc_amd.optim import FISTA

    op, reg, p, X0 = _small_case(which)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        est = FISTA(op, reg, p, tol=TOL, max_iter=5000, check_every=10)
    # a prior applied through its own proxf is announced: the point returned is not the posterior's MAP
    assert any("not the stock synthesis L1" in str(w.message) for w in caught) == (which == "analysis")
    # complex data with a real sig_d: the gradient is taken on the operator with Re(invcov)
    assert (est.gradient_op is not op) == (which != "dirs2")
    assert not bool((est.gradient_op.invcov.diag.imag != 0).any()) if est.gradient_op.invcov.diag.is_complex() else True
    X = est.run(start_point=X0)
    assert est._stock_prox == (which != "analysis") and est.used_graph, est.graph_error
    assert X.shape == (op.nparams,)
    _assert_fixed_point(est, X, which)
    assert np.isnan(est.objective).all() == (which == "analysis")


def test_map_start_for_myula(wav16):
    """the first recorded logposterior of a MYULA chain started at the MAP point is no lower than the one recorded after
    nburn iterations from a zero start with the same seed.  delta is 0.8 of MYULA's bound 1 / (L_g + 1 / lmda), at which the
    oracle's numpy MYULA on this problem is stable for the 50 iterations of the burn-in (checked on the host model)."""
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams
    from pxmcmc_amd.optim import FISTA

    w = wav16
    op, reg = w["op"], w["reg"]
    lmda = w["p"].lmda
    x_map = FISTA(op, reg, w["p"], gamma=w["gamma"], tol=TOL, max_iter=5000).run()
    delta = 0.8 / (1.0 / w["gamma"] + 1.0 / lmda)
    nburn = 50
    cold = MYULA(op, reg, PxMCMCParams(lmda=lmda, delta=delta, mu=1.0, nsamples=1, nburn=nburn, ngap=1, verbosity=0), seed=4)
    _quiet(cold.run, start_point=np.zeros(op.nparams))
    warm = MYULA(op, reg, PxMCMCParams(lmda=lmda, delta=delta, mu=1.0, nsamples=1, nburn=0, ngap=1, verbosity=0), seed=4)
    _quiet(warm.run, start_point=x_map)
    print(f"logposterior: first sample from the MAP start {warm.logPi[0]:.6e}, after {nburn} iterations from zero {cold.logPi[0]:.6e}")
    assert np.isfinite(cold.logPi[0]) and np.isfinite(warm.logPi[0])
    assert warm.logPi[0] >= cold.logPi[0]


def test_gradient_operator_of_a_complex_inverse_covariance():
    """complex data with a real sig_d: invcov = e^{-i pi/4} / sigma^2, so calc_gradg of the operator FISTA steps on is
    cos(pi/4) e^{i pi/4} times the rotated field of the original -- the gradient of 1/2 Re L2, checked against a central
    difference of the data term along a random direction -- and the recorded data term is that function"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.optim import FISTA, gradient_operator

    op, reg, p, X0 = _small_case("spin2")
    assert bool((op.invcov.diag.imag != 0).all())
    gop = gradient_operator(op)
    assert gop is not op and gop.transform is op.transform and gradient_operator(gop) is gop
    x = ops.as_device(X0)
    g_rot = ops.as_device(op.calc_gradg(ops.as_device(op.forward(x))))
    g = ops.as_device(gop.calc_gradg(ops.as_device(gop.forward(x))))
    want = g_rot * (np.cos(np.pi / 4) * np.exp(1j * np.pi / 4))
    assert float(torch.linalg.norm(g - want) / torch.linalg.norm(want)) <= 1e-12
    host = FISTA(op, reg, p, gamma=1.0)
    gfun = lambda v: 0.5 * float(host._l2_dev(ops.as_device(op.forward(v))[None])[0].real)  # noqa: E731
    rng = np.random.default_rng(3)
    u = ops.as_device(rng.normal(size=op.nparams) + 1j * rng.normal(size=op.nparams))
    h = 1e-4  # g is quadratic: the central difference is exact up to the rounding of two sums of ndata terms, over 2 h
    slope = (gfun(x + h * u) - gfun(x - h * u)) / (2 * h)
    want_slope = float(torch.vdot(g, u).real)  # d/dt g(x + t u) = Re <grad, u>
    print(f"directional derivative: central difference {slope:.10e}, Re<grad, u> {want_slope:.10e}")
    assert abs(slope - want_slope) <= 4 * len(op.data) * EPS * gfun(x) / h
    # the rotated field fails the same check (the reason FISTA does not step on it)
    assert abs(slope - float(torch.vdot(g_rot, u).real)) > 1e-3 * abs(want_slope)


def test_empty_state_writes_its_sums():
    import torch

    from pxmcmc_amd import ops

    x = torch.zeros((2, 0), dtype=torch.float64, device=ops.device())
    sums = torch.full((2, 3), float("nan"), dtype=torch.float64, device=x.device)
    ops.fista_step(x, x.clone(), x.clone(), 0.1, 0.1, [0.0], T=0.1, out=(x.clone(), x.clone()), sums=sums)
    assert torch.equal(sums, torch.zeros_like(sums))
