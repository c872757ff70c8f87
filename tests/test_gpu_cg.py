"""The Gaussian posterior on the GPU (csrc/cg.hip, optim.GaussianPosterior, prior.Gaussian): the
kernels element by element against the extended-precision model of pxmcmc_amd/cg_np.py, the bit-for-bit properties, the
solver and its exact draws against dense solves, the streaming summary of the draws, the prior inside MYULA, and the
refusals."""
import contextlib
import io

import numpy as np
import pytest

from pxmcmc_amd import cg_np

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 256 * 256 + 1]  # the last: the first size past the slice cap (the grid-stride loop runs)
C3 = 3


def _rand(rng, shape, cplx):
    return rng.normal(size=shape) + (1j * rng.normal(size=shape) if cplx else 0)


def _dev(a, cplx=None):
    import torch

    from pxmcmc_amd import ops

    dt = torch.complex128 if (np.iscomplexobj(a) if cplx is None else cplx) else torch.float64
    return ops.as_device(np.ascontiguousarray(a), dt)


def _rows(C, bnorm2):
    """coefficient rows of three kinds: chain 0 in the middle of a solve, chain 1 at its first iteration, chain 2 frozen"""
    rows = np.zeros((C, 8))
    rows[:, cg_np.BNORM2] = bnorm2
    rows[0, [cg_np.ALPHA, cg_np.BETA, cg_np.GAMMA_OLD, cg_np.ALPHA_OLD, cg_np.ITERS]] = [0.3, 0.2, 1.7, 0.3, 2]
    if C > 2:
        rows[2, [cg_np.ALPHA, cg_np.BETA, cg_np.RHO, cg_np.FLAGS, cg_np.ITERS]] = [0.4, 0.1, 1e-30, cg_np.FROZEN, 5]
    return rows


@pytest.mark.parametrize("vec", [True, False], ids=["vecD", "scalarD"])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", SIZES)
def test_apply_against_model(n, cplx, vec):
    """W element by element within the bound of its operation sequence (2 roundings); gamma, rho (kept in the row) and delta
    (re-summed from the partials) within the bound of a sum of n such terms; alpha and beta within the bound of the
    decision's operations; the frozen chain's row and W untouched; every chain alone bit-equal to the chain in the batch"""
    import torch

    from pxmcmc_amd import ops

    rng = np.random.default_rng(100 + n + 7 * cplx + 13 * vec)
    r = _rand(rng, (C3, n), cplx)
    # a positive definite system in effect, so that the decision takes its regular branch: u = M^-1 r with M^-1 > 0
    # (gamma > 0), q = A u - b0 with A = 2 I (delta > 0), and chain 0's gamma_old, alpha_old put beta gamma / alpha_old at
    # delta / 4
    u = rng.uniform(0.3, 0.7, size=(C3, n)) * r
    b0 = _rand(rng, n, cplx)
    q = 2.0 * u - b0
    D = rng.uniform(0.5, 3.0, size=n) if vec else 1.25
    rows = _rows(C3, np.sum(np.abs(r) ** 2, axis=1) * 4.0 + 1.0)
    if n:
        gam0, dlt0 = np.sum((np.conj(r[0]) * u[0]).real), np.sum((D + 2.0) * np.abs(u[0]) ** 2)
        rows[0, [cg_np.GAMMA_OLD, cg_np.ALPHA_OLD]] = [4.0 * gam0, gam0 / dlt0]
    tol = 1e-3
    du, dq, dr, db0 = _dev(u, cplx), _dev(q, cplx), _dev(r, cplx), _dev(b0, cplx)
    dD = _dev(D) if vec else D
    W = torch.full_like(du, float("nan"))
    coef = _dev(rows)
    scratch = torch.zeros(3 * ops.FISTA_SLICES_MAX * C3, dtype=torch.float64, device=du.device)
    ops.cg_apply(du, dq, db0, dD, dr, coef, tol, out=W, scratch=scratch)
    Wh, got = W.cpu().numpy(), coef.cpu().numpy()
    slices = max(1, min(256, -(-n // 256)))
    part = scratch.cpu().numpy()[: C3 * slices * 3].reshape(C3, slices, 3)
    for c in range(C3):
        if rows[c, cg_np.FLAGS] != 0:  # frozen: alpha = beta = 0, nothing else moves, W is not written
            want = rows[c].copy()
            want[[cg_np.ALPHA, cg_np.BETA]] = 0.0
            assert np.array_equal(got[c], want)
            assert np.isnan(Wh[c].real).all()
            continue
        if n == 0:  # no terms: rho = 0 <= tol^2 ||b||^2, the chain freezes
            assert got[c, cg_np.FLAGS] == cg_np.FROZEN and got[c, cg_np.ALPHA] == 0 and got[c, cg_np.RHO] == 0
            continue
        w_ld, w_bound = cg_np.cg_apply_ld(u[c], q[c], b0, D, r[c])
        assert cg_np.within(Wh[c], w_ld, w_bound), np.abs(Wh[c] - w_ld).max()
        (gam, dlt, rho), (bg, bd, br) = cg_np.cg_sums_ld(u[c], Wh[c], r[c])
        delta_dev = float(np.sum(part[c, :, 1].astype(np.longdouble)))
        assert abs(got[c, cg_np.GAMMA_OLD] - gam) <= bg and abs(got[c, cg_np.RHO] - rho) <= br and abs(delta_dev - dlt) <= bd
        # the decision from the device's own gamma and rho and the model's delta (whose distance to the device's is <= bd)
        want, bound = cg_np.cg_decide_ld(rows[c], (got[c, cg_np.GAMMA_OLD], dlt, got[c, cg_np.RHO]), tol, delta_bound=bd)
        assert want[cg_np.FLAGS] == 0 and got[c, cg_np.FLAGS] == 0
        assert got[c, cg_np.ITERS] == rows[c, cg_np.ITERS] + 1 and got[c, cg_np.BNORM2] == rows[c, cg_np.BNORM2]
        for k in (cg_np.ALPHA, cg_np.BETA, cg_np.ALPHA_OLD):
            assert abs(got[c, k] - want[k]) <= bound[k], (k, got[c, k], want[k], bound[k])
        assert got[c, cg_np.ALPHA_OLD] == got[c, cg_np.ALPHA]
        # the chain alone: the same bits
        W1 = torch.full_like(du[c:c + 1], float("nan"))
        coef1 = _dev(rows[c:c + 1])
        ops.cg_apply(du[c:c + 1], dq[c:c + 1], db0, dD, dr[c:c + 1], coef1, tol, out=W1)
        assert np.array_equal(W1.cpu().numpy()[0], Wh[c]) and np.array_equal(coef1.cpu().numpy()[0], got[c])


@pytest.mark.parametrize("vec", [True, False], ids=["vecM", "scalarM"])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", SIZES)
def test_update_against_model(n, cplx, vec):
    """the five outputs element by element within the bounds of their operation sequences; the frozen chain copied
    x_src -> x_dst and its other arrays bit for bit as they were; every chain alone bit-equal to the chain in the batch"""
    import torch

    from pxmcmc_amd import ops

    rng = np.random.default_rng(200 + n + 7 * cplx + 13 * vec)
    u, w, p, s, x, r = (_rand(rng, (C3, n), cplx) for _ in range(6))
    minv = rng.uniform(0.2, 2.0, size=n) if vec else 0.75
    rows = _rows(C3, 1.0)
    rows[1, [cg_np.ALPHA, cg_np.BETA, cg_np.ITERS]] = [0.9, 0.0, 1]
    d = {k: _dev(v, cplx) for k, v in dict(u=u, w=w, p=p, s=s, x=x, r=r).items()}
    dM = _dev(minv) if vec else minv
    coef = _dev(rows)
    x1 = torch.full_like(d["x"], float("nan"))
    ops.cg_update(d["u"], d["w"], d["p"], d["s"], d["x"], d["r"], dM, coef, out=x1)
    got = [t.cpu().numpy() for t in (d["p"], d["s"], x1, d["r"], d["u"])]
    assert np.array_equal(coef.cpu().numpy(), rows) and np.array_equal(d["w"].cpu().numpy(), w)
    for c in range(C3):
        outs, bounds = cg_np.cg_update_ld(u[c], w[c], p[c], s[c], x[c], r[c], minv, rows[c])
        if rows[c, cg_np.FLAGS] != 0:
            for g, keep in zip(got, (p, s, x, r, u)):
                assert np.array_equal(g[c], keep[c])
        else:
            for name, g, want, bound in zip("psxru", got, outs, bounds):
                assert cg_np.within(g[c], want, bound), name
        one = {k: _dev(v[c:c + 1], cplx) for k, v in dict(u=u, w=w, p=p, s=s, x=x, r=r).items()}
        y1 = torch.full_like(one["x"], float("nan"))
        ops.cg_update(one["u"], one["w"], one["p"], one["s"], one["x"], one["r"], dM, _dev(rows[c:c + 1]), out=y1)
        for g, t in zip(got, (one["p"], one["s"], y1, one["r"], one["u"])):
            assert np.array_equal(t.cpu().numpy()[0], g[c])


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", [1, 257, 256 * 256 + 1])
def test_prox_and_rhs_kernels(n, cplx):
    """pxm_gauss_prox: one division on a denominator of two roundings -> 4 2^-53 relative per component; pxm_cg_rhs: the
    float64 statement of its three operations, two fma roundings apart at most"""
    from pxmcmc_amd import ops

    rng = np.random.default_rng(300 + n + cplx)
    x, g, z = (_rand(rng, (2, n), cplx) for _ in range(3))
    b, pv, T = _rand(rng, n, cplx), rng.uniform(0.0, 4.0, size=n), 0.37
    for prec in (pv, 1.5):
        got = ops.gauss_prox(_dev(x, cplx), _dev(prec) if np.ndim(prec) else prec, T).cpu().numpy()
        want = x / (1.0 + T * np.asarray(prec, dtype=np.longdouble))
        assert np.abs(got - want).max() <= 4 * cg_np.EPS * np.abs(want).max()
        assert np.all(np.abs(got - want) <= 4 * cg_np.EPS * np.abs(want))
    S = rng.uniform(0.5, 2.0, size=n)
    got = ops.cg_rhs(_dev(x, cplx), B=_dev(b, cplx), G=_dev(g, cplx), g_scale=-0.5, Z=_dev(z, cplx), S=_dev(S), z_scale=2.0).cpu().numpy()
    LD = np.clongdouble if cplx else np.longdouble
    want = b.astype(LD) - 0.5 * g.astype(LD) + (2.0 * S) * z.astype(LD)
    mag = lambda part: np.abs(part(b)) + 0.5 * np.abs(part(g)) + 2.0 * S * np.abs(part(z))  # noqa: E731
    bound = 3 * cg_np.EPS * (mag(np.real) + (1j * mag(np.imag) if cplx else 0))  # two fma roundings (2 S_i is exact), + 1
    assert cg_np.within(got, want, bound)
    assert np.array_equal(ops.cg_rhs(_dev(x, cplx), B=_dev(b, cplx)).cpu().numpy(), np.broadcast_to(b, (2, n)))
    assert np.array_equal(ops.cg_rhs(_dev(x, cplx), Z=_dev(z, cplx), S=1.0).cpu().numpy(), z)


# ---- the solver end to end on three small operators ------------------------------------------------------------------------------
def _params(**kw):
    from pxmcmc_amd.mcmc import PxMCMCParams

    base = dict(lmda=1.0, delta=1e-3, mu=1.0, nsamples=1, nburn=0, ngap=1, verbosity=0)
    base.update(kw)
    return PxMCMCParams(**base)


def _problem(which, C):
    """(forward, prior, params) of a small, well-conditioned Gaussian posterior"""
    import scipy.sparse as sp

    from pxmcmc_amd.forward import ForwardOperator, PathIntegralOperator, SphericalWaveletTransformOperator
    from pxmcmc_amd.measurements import WeakLensing
    from pxmcmc_amd.prior import Gaussian
    from pxmcmc_amd.transforms import SphericalHarmonicTransform

    rng = np.random.default_rng(11)
    L = 8
    P = L * (2 * L - 1)
    if which == "wavelets":  # vector sig_d, a masked cap (sig_d = inf: weight 0)
        sig = rng.uniform(0.5, 2.0, size=P)
        sig[: 3 * (2 * L - 1)] = np.inf
        op = SphericalWaveletTransformOperator(rng.normal(size=P), sig, "synthesis", L, 2, 0, max_chains=C)
        prior = Gaussian(rng.uniform(0.5, 4.0, size=op.nparams), 1.0)
        return op, prior, _params()
    if which == "harmonic":  # the Wiener setting: harmonic state, 1 / C_l prior, masked shear data
        mask = np.ones((L, 2 * L - 1), dtype=bool)
        mask[:2] = False
        wl = WeakLensing(L, mask, ngal=np.full(mask.shape, 30.0), max_chains=C)
        tr = SphericalHarmonicTransform(L, max_chains=C)
        data = (rng.normal(size=wl.ndata) + 1j * rng.normal(size=wl.ndata)) * 0.05
        op = ForwardOperator(data, 1 / wl.inv_cov, "synthesis", transform=tr, measurement=wl, nparams=L * L)
        cl = 1e-3 / (1.0 + np.arange(L)) ** 2
        return op, Gaussian.from_power_spectrum(cl, L, 1.0), _params(complex=True)
    A = sp.random(60, P, density=0.1, random_state=np.random.RandomState(2), format="csr")  # path integrals, real state
    op = PathIntegralOperator(A, rng.normal(size=60), 0.2, "analysis", L, 2, 0, max_chains=C)
    return op, Gaussian(2.0, 1.0), _params()


def _dense(post):
    """(H, b0) of the solver's system as dense host matrices: the operator applied to the basis vectors, C at a time"""
    import torch

    from pxmcmc_amd import ops

    n, C = post._n, post.nchains
    b0 = post._b0.cpu().numpy()
    H = np.zeros((n, n), dtype=b0.dtype)
    for j0 in range(0, n, C):
        E = torch.zeros((C, n), dtype=post._dt, device=ops.device())
        idx = np.arange(j0, min(j0 + C, n))
        E[torch.arange(len(idx)), torch.as_tensor(idx)] = 1.0
        H[:, idx] = (post._linear(E).cpu().numpy() + b0).T[:, : len(idx)]
    D = post._D if isinstance(post._D, float) else post._D.cpu().numpy()
    return H + np.diag(np.broadcast_to(D, (n,))), b0


_CACHE = {}


def _solved(which):
    """one solver, its dense system and its MAP run per operator, shared by the tests below"""
    if which not in _CACHE:
        from pxmcmc_amd.optim import GaussianPosterior

        C = 3
        op, prior, params = _problem(which, C)
        post = GaussianPosterior(op, prior, params, nchains=C, tol=1e-8, seed=5, chain_offset=2)
        H, b0 = _dense(post)
        rng = np.random.default_rng(12)
        start = np.stack([np.zeros(post._n), *(_rand(rng, post._n, post._dt.is_complex) for _ in range(C - 1))])
        X = post.run(start.astype(b0.dtype))
        record = dict(niter=post.niter.copy(), converged=post.converged.copy(), breakdown=post.breakdown.copy(),
                      used_graph=post.used_graph, objective=post.objective_map.copy(), rel=post.rel_residual.copy())
        _CACHE[which] = (post, H, b0, X, record)
    return _CACHE[which]


def _assert_solves(H, b, x, tol, cond):
    xs = np.linalg.solve(H, b)
    res = np.linalg.norm(b - H @ x) / np.linalg.norm(b)
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print(f"true relative residual {res:.3e} (<= {2 * tol:.1e}), relative error {err:.3e} (<= {cond * 2 * tol:.3e})")
    assert res <= 2 * tol
    assert err <= cond * 2 * tol


@pytest.mark.parametrize("which", ["wavelets", "harmonic", "paths"])
def test_solver_against_dense_solve(which):
    """H is Hermitian to round-off; cg_np on the same dense H stays within the two bounds (which bounds the drift of the
    recurrence residual); the solver's MAP point, from a zero and from random starts, meets them"""
    import torch

    post, H, b0, X, rec = _solved(which)
    n = post._n
    assert post._dt == (torch.float64 if which == "paths" else torch.complex128)
    # an entry of H is a sum of at most n ndata products through two transforms: 64 n roundings of the largest entry
    assert np.abs(H - H.conj().T).max() <= 64 * n * 2.0 ** -52 * np.abs(H).max()
    H = 0.5 * (H + H.conj().T)
    cond = np.linalg.cond(H)
    assert np.linalg.eigvalsh(H).min() > 0 and cond < 1e6
    tol = 1e-8
    D = np.real(np.diag(H)) * 0.0
    minv = post._minv if isinstance(post._minv, float) else post._minv.cpu().numpy()
    x_np, info = cg_np.pcg_np(H, D, b0, minv=minv, tol=tol)
    assert info["frozen"] and not info["breakdown"]
    _assert_solves(H, b0, x_np, tol, cond)
    assert rec["converged"].all() and not rec["breakdown"].any() and rec["used_graph"], rec
    assert (rec["niter"] > 0).all() and (rec["niter"] <= 200).all() and np.all(rec["rel"][-1] <= tol)
    for c in range(post.nchains):
        _assert_solves(H, b0, X[c], tol, cond)
    # the objective at the MAP point: 1/2 sum w |preds - data|^2 + (T / lmda) 1/2 sum p |x|^2 from the solver's own arrays
    # (sums of a few hundred non-negative terms: 1e-12 relative)
    from pxmcmc_amd import ops

    f = post.gradient_op
    w = ops.as_device(f.invcov.diag).real.cpu().numpy()
    resid = post.preds_map.cpu().numpy() - f.data_dev.cpu().numpy()
    want = 0.5 * np.sum(w * np.abs(resid) ** 2, axis=1) + 0.5 * np.sum(post.prior.precision * np.abs(X) ** 2, axis=1) * (post.prior.T / post.lmda)
    assert np.all(np.abs(rec["objective"] - want) <= 1e-12 * np.abs(want))


def test_graph_replay_equals_eager():
    """20 iterations (tol = 0: no chain freezes) from the captured graph and one by one: the same bits"""
    from pxmcmc_amd.optim import GaussianPosterior

    op, prior, params = _problem("harmonic", 2)
    outs = []
    for graph in (True, False):
        post = GaussianPosterior(op, prior, params, nchains=2, tol=0.0, max_iter=20, check_every=7, use_graph=graph)
        outs.append((post.run(), post.niter.copy(), post.rel_residual.copy(), post.used_graph))
    assert outs[0][3] and not outs[1][3]
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][2], outs[1][2])
    assert np.array_equal(outs[0][1], outs[1][1]) and (outs[0][1] <= 20).all() and (outs[0][1] > 0).all()
    assert np.array_equal(outs[0][0][0], outs[0][0][1])  # two chains of one system: the same bits


def _deviates(post, k, ndata):
    """omega_1 [C, ndata] and omega_2 [C, N] of draw k from the oracle's Philox stream"""
    from oracle import philox

    draw = philox.randn_complex if post._dt.is_complex else philox.randn_real
    chains = [post.chain_offset + c for c in range(post.nchains)]
    it1, it2 = cg_np.draw_iterations(k)
    return (np.stack([draw(ndata, post.seed, ch, it1, bits=64) for ch in chains]),
            np.stack([draw(post._n, post.seed, ch, it2, bits=64) for ch in chains]))


@pytest.mark.parametrize("which", ["harmonic", "paths"])
def test_draws_against_dense_solves(which):
    """every draw of two solves (C = 3) is the dense solve of its own right-hand side b0 + Phi^H W (s o omega_1) +
    sqrt(D) o omega_2, the deviates recomputed by oracle.philox; two calls agree bit for bit; chain_offset shifts the streams"""
    from pxmcmc_amd import ops
    from pxmcmc_amd.optim import GaussianPosterior

    post, H, b0, _, _ = _solved(which)
    H = 0.5 * (H + H.conj().T)
    cond, tol, C, n = np.linalg.cond(H), 1e-8, post.nchains, post._n
    draws = post.sample(2 * C)
    assert draws.shape == (2 * C, n) and post.solve_iterations.shape == (2, C)
    assert np.array_equal(draws, post.sample(2 * C))
    f = post.gradient_op
    w = ops.as_device(f.invcov.diag).real.cpu().numpy()
    with np.errstate(divide="ignore"):
        s = np.where(w > 0, 1.0 / np.sqrt(w), 0.0)
    D = np.broadcast_to(post._D if isinstance(post._D, float) else post._D.cpu().numpy(), (n,))
    data = f.data_dev.cpu().numpy()
    for k in range(2):
        o1, o2 = _deviates(post, k, len(w))
        # Phi^H W (s o omega_1) through the operator itself (linear, checked dense above): calc_gradg(data + s o omega_1)
        a_data = ops.as_device(f.calc_gradg(ops.as_device(data + s * o1)), post._dt).cpu().numpy()
        B = b0 + a_data + np.sqrt(D) * o2
        got_B = post.draw_rhs(k).cpu().numpy()
        # the device's Box-Muller differs from numpy's by a few ulps of each deviate
        assert np.abs(got_B - B).max() <= 1e-12 * np.abs(B).max()
        for c in range(C):
            _assert_solves(H, got_B[c], draws[k * C + c], tol, cond)
    # chain_offset + 1: chain c of the shifted solver draws what chain c + 1 drew
    op, prior, params = _problem(which, C)
    # (the same right-hand side solved at another place of the batch: both within cond 2 tol of the one exact solution)
    shifted = GaussianPosterior(op, prior, params, nchains=C, tol=tol, seed=post.seed, chain_offset=post.chain_offset + 1)
    moved = shifted.sample(C)
    B_here, B_there = shifted.draw_rhs(0).cpu().numpy()[: C - 1], post.draw_rhs(0).cpu().numpy()[1:]
    assert np.abs(B_here - B_there).max() <= 1e-12 * np.abs(B_there).max()
    for c in range(C - 1):
        assert np.linalg.norm(moved[c] - draws[c + 1]) <= cond * 4 * tol * np.linalg.norm(draws[c + 1])
    assert np.linalg.norm(moved[0] - draws[0]) > cond * 4 * tol * np.linalg.norm(draws[0])


def test_summary_of_draws():
    """C = 8, 64 solves at the L = 8 harmonic problem: the streaming mean and variance equal numpy's over the draws of the
    same stream (the tolerance of tests/test_gpu_moments.py: 1e-12 relative to the largest entry), and the pooled effective
    sample size of independent draws is not flagged truncated"""
    from pxmcmc_amd.optim import GaussianPosterior

    C, K = 8, 64
    op, prior, params = _problem("harmonic", C)
    post = GaussianPosterior(op, prior, params, nchains=C, tol=1e-8, seed=3)
    draws = post.sample(C * K).reshape(K, C, -1)
    summ = post.sample(C * K, summary="state", summary_ess=64)
    assert int(summ.counts.min()) == K and int(summ.counts.max()) == K
    mean, var = summ.mean().cpu().numpy(), summ.variance().cpu().numpy()
    want_mean = draws.mean(axis=0)
    want_var = draws.real.var(axis=0, ddof=1) + draws.imag.var(axis=0, ddof=1)
    assert np.abs(mean - want_mean).max() <= 1e-12 * np.abs(want_mean).max()
    assert np.abs(var - want_var).max() <= 1e-12 * np.abs(want_var).max()
    ess = summ.ess_readout(pooled=True)  # stats: (min ESS, undefined count, truncated count)
    pooled, stats = ess["ess_pooled"].cpu().numpy(), ess["stats"].cpu().numpy()
    assert np.isfinite(pooled).all() and (pooled > 0).all() and stats[1] == 0 and stats[2] == 0, stats


def test_gaussian_prior_in_myula():
    """one MYULA iteration with prior.Gaussian equals the oracle's chain step with proxf = X / (1 + T p) to 1e-12"""
    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import MYULA
    from pxmcmc_amd.prior import Gaussian

    L, B, J_min, C = 8, 2, 0, 2
    rng = np.random.default_rng(0)
    P = L * (2 * L - 1)
    data = rng.normal(size=P)
    lmda, delta, mu = 1e-3, 5e-4, 1.0
    op = SphericalWaveletTransformOperator(data, 0.1, "synthesis", L, B, J_min, max_chains=C)
    N = op.nparams
    prec = rng.uniform(0.0, 5.0, size=N)
    reg = Gaussian(prec, lmda * mu)

    class OraclePrior:
        def proxf(self, X):
            return X / (1 + lmda * mu * prec)

        def prior(self, X):
            return 0.5 * np.sum(prec * np.abs(X) ** 2)

    s = MYULA(op, reg, _params(lmda=lmda, delta=delta, mu=mu), nchains=C, rng="numpy")
    X0 = rng.normal(size=N) * 0.1
    np.random.seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        s.run(start_point=X0)
    T = ref.SphericalWaveletTransform(L, B, J_min)
    oop = ref.ForwardOperator(data, 0.1, "synthesis", T, ref.Identity(P, P), T.ncoefs)
    np.random.seed(1)
    noise = [np.random.randn(N) for _ in range(C)]
    for c in range(C):
        out = ref.myula_run(oop, OraclePrior(), lmda, delta, mu, 1, 0, 1, X0.astype(complex), lambda i: noise[c])
        assert np.abs(s.chain[c] - out["chain"]).max() <= 1e-12
    x = rng.normal(size=(C, N)) + 1j * rng.normal(size=(C, N))
    assert np.allclose(reg.proxf(x), x / (1 + lmda * mu * prec), rtol=1e-14, atol=0)  # (the kernel's own bound: above)
    assert np.allclose(reg.prior(x).cpu().numpy(), 0.5 * np.sum(prec * np.abs(x) ** 2, axis=1), rtol=1e-13)
    assert isinstance(reg.prior(x[0]), float) and isinstance(reg.proxf(x[0]), np.ndarray)


def test_refusals():
    import scipy.sparse as sp
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.optim import GaussianPosterior
    from pxmcmc_amd.prior import Gaussian
    from pxmcmc_amd.transforms import IdentityTransform

    rng = np.random.default_rng(3)
    P = 12
    M = rng.normal(size=(P, P))
    cov = M @ M.T + P * np.eye(P)
    full = ForwardOperator(rng.normal(size=P), sp.csr_matrix(cov), "synthesis", IdentityTransform(), Identity(P, P), nparams=P)
    post = GaussianPosterior(full, Gaussian(1.0, 1.0), _params())
    x = post.run()  # run accepts the full covariance ...
    H = np.linalg.inv(cov) + np.eye(P)
    assert np.linalg.norm(H @ x - post._b0.cpu().numpy()) <= 2e-8 * np.linalg.norm(post._b0.cpu().numpy())
    with pytest.raises(ValueError, match="diagonal inverse covariance"):
        post.sample(1)  # ... sample does not
    with pytest.raises(ValueError):
        Gaussian(np.array([1.0, -1.0]), 1.0)
    diag = ForwardOperator(rng.normal(size=P), 0.5, "synthesis", IdentityTransform(), Identity(P, P), nparams=P)
    with pytest.raises(ValueError, match="state's length"):
        GaussianPosterior(diag, Gaussian(1.0, 1.0), _params(), precond=np.ones(P + 1))
    with pytest.raises(ValueError):
        GaussianPosterior(diag, Gaussian(1.0, 1.0), _params(), precond=-np.ones(P))
    with pytest.raises(ValueError):
        GaussianPosterior(diag, Gaussian(np.ones(P + 1), 1.0), _params())
    with pytest.raises(ValueError):
        GaussianPosterior(diag, Gaussian(1.0, 1.0), _params(), precond="jacobi")
    z = torch.zeros((2, 8), dtype=torch.float64, device=ops.device())
    coef = ops.cg_coef(torch.ones(2, dtype=torch.float64, device=z.device))
    with pytest.raises(PxmError):
        ops.cg_apply(z, z.clone(), None, 1.0, z.clone(), coef, 1e-8, out=z)  # W aliases U
    with pytest.raises(PxmError):
        ops.cg_update(z, z.clone(), z.clone(), z.clone(), z.clone(), z, 1.0, coef)  # R is U
    with pytest.raises(ValueError):
        ops.cg_apply(z, z.clone(), None, 1.0, z.clone(), coef[:1], 1e-8)
