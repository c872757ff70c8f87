"""The Gibbs sampler on the sparse posterior, on the GPU (csrc/lasso.hip, optim.LassoGibbs): the draw
element by element against the extended-precision model of pxmcmc_amd/lasso_np.py, its bit-for-bit properties, the sampler
against the numpy statement fed the same deviates, and its distribution against the identity model's posterior by quadrature."""
import numpy as np
import pytest
from test_gpu_cg import _dev, _params
from test_lasso_host import (DRAW_CHAIN0, DRAW_CLAMP, DRAW_SEED, DRAW_SIZES, DRAW_SWEEP, IDENTITY_BURN, IDENTITY_CHAINS, IDENTITY_RHAT,
                             IDENTITY_SWEEPS, IDENTITY_T, draw_case, draw_model, draw_uniforms, identity_expected, z_scores)

from pxmcmc_amd import lasso_np as LN

pytestmark = pytest.mark.gpu

IT_Z = LN.draw_iterations(DRAW_SWEEP)[0]


def _launch(case, cplx, sums=True, it=IT_Z, seed=DRAW_SEED, chain0=DRAW_CHAIN0, X=None):
    """the draw of a case of tests/test_lasso_host.py -> (D, sqrtD, Minv, sums) as numpy arrays"""
    import torch

    from pxmcmc_amd import ops

    C, n = case["x"].shape
    dev = ops.device()
    out = [torch.full((C, n), float("nan"), dtype=torch.float64, device=dev) for _ in range(3)]
    sm = torch.full((C, 2), float("nan"), dtype=torch.float64, device=dev) if sums else None
    T = case["T"] if np.ndim(case["T"]) == 0 else _dev(case["T"])
    h = case["h"] if np.ndim(case["h"]) == 0 else _dev(case["h"])
    ops.lasso_precision_draw(_dev(case["x"], cplx) if X is None else X, T, *out, tscale=case["tscale"], h=h, d_lo=DRAW_CLAMP[0],
                             d_hi=DRAW_CLAMP[1], seed=seed, chain0=chain0, it=it, sums=sm)
    return tuple(t.cpu().numpy() for t in out) + ((sm.cpu().numpy(),) if sums else (None,))


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", DRAW_SIZES)
def test_draw_against_model(n, cplx):
    """D, sqrt(D) and M^-1 of EVERY element within the bound of the extended-precision model fed the normals of ops.randn and
    the uniforms rebuilt from the Philox bits (tests/test_lasso_host.py shows that no element of these cases is ambiguous);
    the prior term within the summation bound and the clamped count exact; both clamp limits bind (n >= 255); rows and
    elements of X that are exactly zero; scalar and vector T, float and per-chain h, chain0 = 5; without sums the same bits;
    two calls give the same bits"""
    from pxmcmc_amd import ops

    case = draw_case(n, cplx)
    C = case["C"]
    D, sD, Mi, sums = _launch(case, cplx)
    z = ops.randn(n, C, complex_=True, seed=DRAW_SEED, chain0=DRAW_CHAIN0, it=IT_Z, noise64=True).cpu().numpy().real
    u = draw_uniforms(n, C)
    lo, hi = DRAW_CLAMP
    for c, ld in enumerate(draw_model(case, z, u)):
        assert not ld["ambiguous"].any() and not ld["clamp_open"].any()
        for got, key in ((D[c], "D"), (sD[c], "sqrtD"), (Mi[c], "Minv")):
            err = np.abs(got - ld[key])
            assert np.all(err <= ld[key + "_bound"]), (c, key, int(np.argmax(err - ld[key + "_bound"])), err.max())
        assert np.all((D[c] >= lo) & (D[c] <= hi))
        total, bound, count, slack = LN.sums_ld(ld)
        assert slack == 0 and abs(sums[c, 0] - total) <= bound and sums[c, 1] == count, (c, sums[c], total, bound, count)
        assert count == np.sum((D[c] == lo) | (D[c] == hi))
    if n >= 255:
        assert (D == lo).any() and (D == hi).any() and ((D > lo) & (D < hi)).any()
    if C == 3:  # the deviates differ from chain to chain
        free = (D[0] > lo) & (D[0] < hi) & (D[2] > lo) & (D[2] < hi)
        assert np.all(D[0][free] != D[2][free]) and (free.any() or n == 1)
    for a, b in zip(_launch(case, cplx), (D, sD, Mi, sums)):
        assert np.array_equal(a, b)
    for a, b in zip(_launch(case, cplx, sums=False)[:3], (D, sD, Mi)):
        assert np.array_equal(a, b)


def test_draw_is_disjoint_from_the_field_streams():
    """the draw of sweep t owns the iterations 2^60 + 2 t and 2^60 + 2 t + 1: ops.randn at the field iterations 2 t, 2 t + 1 is
    what it was before the launch, another sweep, seed or chain offset gives other precisions, and chain c of a launch at
    chain0 is chain 0 of a launch at chain0 + c"""
    from pxmcmc_amd import ops

    n, cplx = 257, True
    case = draw_case(n, cplx)
    kw = dict(complex_=True, seed=DRAW_SEED, chain0=DRAW_CHAIN0, noise64=True)
    before = [ops.randn(n, 3, it=it, **kw).cpu().numpy() for it in (2 * DRAW_SWEEP, 2 * DRAW_SWEEP + 1)]
    D = _launch(case, cplx)[0]
    after = [ops.randn(n, 3, it=it, **kw).cpu().numpy() for it in (2 * DRAW_SWEEP, 2 * DRAW_SWEEP + 1)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    free = (D > DRAW_CLAMP[0]) & (D < DRAW_CLAMP[1])
    for other in (dict(it=LN.draw_iterations(DRAW_SWEEP + 1)[0]), dict(seed=DRAW_SEED + 1), dict(chain0=DRAW_CHAIN0 + 3)):
        assert np.all(_launch(case, cplx, **other)[0][free] != D[free])
    one = dict(case, C=1, x=case["x"][2:3], h=case["h"] if np.ndim(case["h"]) == 0 else case["h"][2:3])
    assert np.array_equal(_launch(one, cplx, chain0=DRAW_CHAIN0 + 2)[0][0], D[2])


def test_draw_graph_replay_equals_eager():
    """the two launches captured into a HIP graph and replayed equal the eager call bit for bit"""
    import torch

    from pxmcmc_amd import ops

    n, cplx = 256 * 256 + 3, True
    case = draw_case(n, cplx)
    C = case["C"]
    dev = ops.device()
    X, h = _dev(case["x"], cplx), _dev(np.broadcast_to(case["h"], (C,)).copy())
    T = case["T"] if np.ndim(case["T"]) == 0 else _dev(case["T"])
    new = lambda: ([torch.full((C, n), float("nan"), dtype=torch.float64, device=dev) for _ in range(3)]  # noqa: E731
                   + [torch.full((C, 2), float("nan"), dtype=torch.float64, device=dev)])
    scratch = ops.lasso_scratch(C, dev)
    run = lambda D, sD, Mi, sm: ops.lasso_precision_draw(X, T, D, sD, Mi, tscale=case["tscale"], h=h, d_lo=DRAW_CLAMP[0],  # noqa: E731
                                                         d_hi=DRAW_CLAMP[1], seed=1, chain0=2, it=IT_Z, sums=sm, scratch=scratch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*new())  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    got = new()
    g = torch.cuda.CUDAGraph()
    with ops.capture_scope(), torch.cuda.graph(g):
        run(*got)
    assert torch.isnan(got[0]).all()  # capture does not execute
    g.replay()
    torch.cuda.synchronize()
    want = new()
    run(*want)
    torch.cuda.synchronize()
    for a, e in zip(got, want):
        assert not torch.isnan(a).any() and torch.equal(a.view(torch.int64), e.view(torch.int64))


def test_wrapper_refuses():
    import torch

    from pxmcmc_amd import ops

    dev = ops.device()
    X = torch.zeros((2, 5), dtype=torch.float64, device=dev)
    new = lambda shape=(2, 5), dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    ok = dict(X=X, T=1.0, D=new(), sqrtD=new(), Minv=new())
    ops.lasso_precision_draw(**ok)
    for bad in (dict(T=0.0), dict(T=-1.0), dict(T=np.array([1.0, 1.0, 0.0, 1.0, 1.0])), dict(T=np.ones(4)), dict(tscale=0.0),
                dict(tscale=np.inf), dict(D=new((2, 4))), dict(sqrtD=new(dt=torch.float32)), dict(Minv=new((5, 2)).t()),
                dict(d_lo=0.0), dict(d_lo=2.0, d_hi=1.0), dict(d_hi=np.inf), dict(h=new((3,))), dict(sums=new((2, 3))),
                dict(sums=new((2, 2)), scratch=new((8,)))):
        with pytest.raises(ValueError):
            ops.lasso_precision_draw(**dict(ok, **bad))
    with pytest.raises(ops.PxmError, match="different"):
        ops.lasso_precision_draw(**dict(ok, sqrtD=ok["D"]))
    with pytest.raises(ops.PxmError, match="alias"):
        ops.lasso_precision_draw(**dict(ok, Minv=X))
    with pytest.raises(ops.PxmError, match="h must be"):
        ops.lasso_precision_draw(**dict(ok, h=-1.0))


# ---- the sampler -----------------------------------------------------------------------------------------------------------
DENSE_T = np.r_[np.full(20, 0.8), np.full(20, 2.5), np.linspace(0.5, 4.0, 24)]
DENSE_SWEEPS, DENSE_TOL = 4, 1e-10
DENSE = {}


def _dense_problem():
    """a dense real Phi [96, 64] as a path-integral measurement of a sparse truth -> (Phi, w, data, sigma)"""
    rng = np.random.default_rng(31)
    m, n = 96, 64
    Phi = rng.normal(size=(m, n)) / np.sqrt(m)
    sig = 0.3
    truth = np.where(rng.uniform(size=n) < 0.3, 2 * rng.normal(size=n), 0.0)
    return Phi, np.full(m, 1 / sig ** 2), Phi @ truth + sig * rng.normal(size=m), sig


def _dense_lasso(use_graph=True):
    """the sampler on the dense problem: C = 2, 4 sweeps -> (sampler, X [4, 2, 64])"""
    if use_graph not in DENSE:
        from pxmcmc_amd.forward import ForwardOperator
        from pxmcmc_amd.measurements import PathIntegral
        from pxmcmc_amd.optim import LassoGibbs
        from pxmcmc_amd.prior import L1

        Phi, w, data, sig = _dense_problem()
        op = ForwardOperator(data, sig, "analysis", measurement=PathIntegral(Phi), nparams=Phi.shape[1])
        las = LassoGibbs(op, L1("synthesis", None, None, 2.0 * DENSE_T), _params(lmda=2.0), nchains=2, tol=DENSE_TOL, seed=4,
                         chain_offset=3, use_graph=use_graph)
        DENSE[use_graph] = (las, las.run(DENSE_SWEEPS))
    return DENSE[use_graph]


def test_sampler_follows_the_numpy_statement():
    """dense Phi (n = 64), vector T, lmda = 2, C = 2, 4 sweeps: the field of every sweep is the dense solve of lasso_np's sweep
    fed the same deviates and the precisions the draw gives at the chain's own field of the sweep before, within tol cond(H)
    -- the solver stops at a recurrence residual of tol ||b_data|| <= tol ||b||, and the condition number of that sweep's H is
    computed here from the dense matrix -- and prior_term_chain and clamped_chain are the sums of that field."""
    from pxmcmc_amd import ops

    las, X = _dense_lasso()
    Phi, w, data, _ = _dense_problem()
    n, C = 64, 2
    assert las.solve_converged.all() and las.used_graph and X.shape == (DENSE_SWEEPS, C, n) and X.dtype == np.float64
    assert las.solve_iterations.shape == (DENSE_SWEEPS, C) and las.prior_term_chain.shape == las.clamped_chain.shape == (DENSE_SWEEPS, C)
    kw = dict(seed=las.seed, chain0=las.chain_offset, noise64=True)
    D = np.tile(LN.initial_precision(DENSE_T, False), (C, 1))
    for s in range(DENSE_SWEEPS):
        w1 = ops.randn(len(data), C, it=2 * s, **kw).cpu().numpy()
        w2 = ops.randn(n, C, it=2 * s + 1, **kw).cpu().numpy()
        it_z = LN.draw_iterations(s)[0]
        z = ops.randn(n, C, complex_=True, it=it_z, **kw).cpu().numpy().real
        u = draw_uniforms(n, C, las.seed, las.chain_offset, it_z)
        for c in range(C):
            x, _, H = LN.lasso_sweep_np(Phi, w, data, DENSE_T, D[c], w1[c], w2[c], z[c], u[c], *las.precision_bounds)
            cond = np.linalg.cond(H)
            ex = np.linalg.norm(X[s, c] - x) / np.linalg.norm(x)
            print(f"sweep {s} chain {c}: cond {cond:.3g}, D from {D[c].min():.3g} to {D[c].max():.3g}, field error {ex:.2e} "
                  f"(<= {DENSE_TOL * cond:.2e}), {las.solve_iterations[s, c]} iterations")
            assert ex <= DENSE_TOL * cond
            # the precisions of the next sweep: the draw at the GPU chain's own field
            new = LN.precision_draw_np(X[s, c], DENSE_T, z[c], u[c], 0.0, *las.precision_bounds)
            D[c] = new["D"]
            assert np.isclose(las.prior_term_chain[s, c], new["terms"].sum(), rtol=1e-13, atol=0)
            assert las.clamped_chain[s, c] == new["clamped"].sum()


def test_graph_flag_and_seed_give_the_same_bits():
    las, X = _dense_lasso()
    eager, Xe = _dense_lasso(use_graph=False)
    assert las.used_graph and not eager.used_graph
    assert np.array_equal(X, Xe) and np.array_equal(las.prior_term_chain, eager.prior_term_chain)
    assert np.array_equal(las.solve_iterations, eager.solve_iterations)
    again = las.run(DENSE_SWEEPS)
    assert np.array_equal(again, X)
    # a start point: the precisions are drawn from it, exact zeros included; burn-in drops sweeps; as_torch
    start = X[-1, 0].copy()
    start[::3] = 0.0
    Y = las.run(3, nburn=1, start_point=start, as_torch=True)
    assert tuple(Y.shape) == (2, 2, 64) and las.prior_term_chain.shape == (2, 2) and las.solve_iterations.shape == (3, 2)
    assert np.array_equal(las.run(3, nburn=1, start_point=start), Y.cpu().numpy()) and not np.array_equal(Y.cpu().numpy(), X[1:3])
    with pytest.raises(ValueError, match="start point"):
        las.run(2, start_point=np.zeros(63))


def test_distribution_on_the_identity_model():
    """the real identity model of tests/test_lasso_host.py at noise variance 0.25 (12 elements, 16 chains, 400 sweeps of which
    50 burn-in): the posterior mean and E x^2 of every element within 5 standard errors (of the 16 chain means) of the
    quadrature values, and R-hat from the returned PosteriorSummary below the numpy sampler's largest over ten seeds plus
    its spread there (1.0065 + 0.0014, measured by test_lasso_host.py::test_numpy_sampler_rhat)"""
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.optim import LassoGibbs
    from pxmcmc_amd.prior import L1

    noise_var = 0.25
    d, mean, second = identity_expected(noise_var, False)
    n = d.size
    op = ForwardOperator(d, np.sqrt(noise_var), "analysis", measurement=Identity(n, n), nparams=n)
    las = LassoGibbs(op, L1("synthesis", None, None, IDENTITY_T), _params(), nchains=IDENTITY_CHAINS, tol=1e-10, seed=77)
    X = las.run(IDENTITY_SWEEPS, nburn=IDENTITY_BURN)
    assert las.solve_converged.all() and X.shape == (IDENTITY_SWEEPS - IDENTITY_BURN, IDENTITY_CHAINS, n)
    z1, z2 = z_scores(X, mean), z_scores(X * X, second)
    post = las.run(IDENTITY_SWEEPS, nburn=IDENTITY_BURN, summary="state")
    rhat = post.rhat().cpu().numpy()
    print("GPU sampler: z of the mean", z1, "z of E x^2", z2, "R-hat", rhat, "iterations", las.solve_iterations.max(),
          "clamped", las.clamped_chain.sum())
    assert np.all(np.abs(z1) <= 5.0) and np.all(np.abs(z2) <= 5.0), (z1, z2)
    assert rhat.shape == (n,) and np.all(rhat < IDENTITY_RHAT[0] + IDENTITY_RHAT[1]), rhat
    assert np.allclose(post.mean().cpu().numpy(), X.mean(axis=0), rtol=0, atol=1e-12)
    assert np.allclose(las.prior_term_chain, (IDENTITY_T * np.abs(X)).sum(axis=2), rtol=1e-13, atol=0)


def test_wavelet_state():
    """the wavelet synthesis operator at L = 8 with the identity measurement, S2_Wavelets_L1 (a vector T), C = 2, 3 sweeps:
    complex draws of the operator's size, the records of every solve, the image summary of the image's size, and the prior
    term (1 / lmda) sum T |X| of the draws.  Whether a solve on the redundant frame converges inside max_iter is reported
    (a warning, solve_converged), not asserted here: its iteration count is a measurement of DESIGN.md section 25 -- the dense
    and the identity model above hold the solves to their references."""
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.optim import LassoGibbs
    from pxmcmc_amd.prior import S2_Wavelets_L1

    L, B, J_min, C = 8, 2, 2, 2
    rng = np.random.default_rng(5)
    op = SphericalWaveletTransformOperator(rng.normal(size=L * (2 * L - 1)), 1.0, "synthesis", L, B, J_min, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", op.transform.inverse, op.transform.inverse_adjoint, 2.0, L=L, B=B, J_min=J_min)
    las = LassoGibbs(op, reg, _params(lmda=0.25), nchains=C, tol=1e-6, max_iter=400, check_every=50, seed=3)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        X = las.run(3)
        post = las.run(3, nburn=1, summary="image")
    print("iterations", las.solve_iterations.tolist(), "converged", las.solve_converged.tolist())
    assert X.shape == (3, C, op.nparams) and np.iscomplexobj(X) and np.all(np.isfinite(X))
    assert las.solve_converged.shape == las.solve_iterations.shape == (3, C) and (las.solve_iterations >= 1).all()
    assert np.all(X[1:] != X[:-1]) and np.all(X[:, 0] != X[:, 1])
    assert np.allclose(las.prior_term_chain, (np.asarray(reg.T) * np.abs(X[1:])).sum(axis=2) / 0.25, rtol=1e-12, atol=0)
    assert tuple(post.mean().shape) == (C, L * (2 * L - 1))


def test_construction_refuses():
    """LassoGibbs itself refuses a threshold with an entry that is not positive, the analysis setting, TV, a prior with a prox
    of its own, a Gaussian prior, a full inverse covariance and clamp limits that are not finite and positive -- each with a
    message that says why"""
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.optim import LassoGibbs
    from pxmcmc_amd.prior import L1, TV_S2, Gaussian, L1_Analysis

    n = 12
    op = ForwardOperator(np.ones(n), 0.5, "analysis", measurement=Identity(n, n), nparams=n)
    make = lambda prior, **kw: LassoGibbs(kw.pop("op", op), prior, _params(), nchains=2, **kw)  # noqa: E731
    l1 = lambda T: L1("synthesis", None, None, T)  # noqa: E731
    make(l1(1.0))
    T = np.ones(n)
    T[4] = 0.0
    for bad in (0.0, -1.0, T, -np.ones(n)):
        with pytest.raises(ValueError, match="positive"):
            make(l1(bad))
    with pytest.raises(ValueError, match="one value per parameter"):
        make(l1(np.ones(n - 1)))
    ident = lambda x: x  # noqa: E731
    with pytest.raises(ValueError, match="analysis"):
        make(L1("analysis", ident, ident, 1.0))
    with pytest.raises(ValueError, match="analysis"):
        make(L1_Analysis(ident, ident, 1.0))
    with pytest.raises(ValueError, match="total-variation"):
        make(TV_S2(2, 1.0))

    class Own(L1):
        def proxf(self, X):
            return X

    with pytest.raises(ValueError, match="stock"):
        make(Own("synthesis", None, None, 1.0))
    with pytest.raises(ValueError, match="stock"):
        make(Gaussian(1.0, 1.0))
    full = ForwardOperator(np.ones(n), 0.25 * np.eye(n), "analysis", measurement=Identity(n, n), nparams=n)  # a 2-D covariance
    with pytest.raises(ValueError, match="diagonal inverse covariance"):
        make(l1(1.0), op=full)
    for pb in ((0.0, 1.0), (1.0, np.inf), (np.nan, 1.0), (-1.0, 1.0), (2.0, 1.0)):
        with pytest.raises(ValueError, match="precision_bounds"):
            make(l1(1.0), precision_bounds=pb)
    for kw in (dict(tol=-1.0), dict(max_iter=0), dict(check_every=0)):
        with pytest.raises(ValueError, match="LassoGibbs"):
            make(l1(1.0), **kw)
