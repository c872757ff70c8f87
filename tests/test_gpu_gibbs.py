"""The Gibbs sampler on the Gaussian posterior, on the GPU (csrc/gibbs.hip, the per-chain diagonals of csrc/cg.hip,
optim.GaussianGibbs): the launches element by element against the extended-precision models of
pxmcmc_amd/cg_np.py and pxmcmc_amd/gibbs_np.py, the bit-for-bit properties, the sampler against the numpy statement fed the
same deviates and against dense solves, and its distribution against the identity model's marginal by quadrature."""
import numpy as np
import pytest
from test_gibbs_host import (IDENTITY_BURN, IDENTITY_CHAINS, IDENTITY_NOISE_VAR, IDENTITY_SWEEPS, identity_expected_log_variance,
                             identity_model, z_scores)
from test_gpu_cg import _assert_solves, _dev, _params, _rand, _rows

from pxmcmc_amd import cg_np
from pxmcmc_amd import gibbs_np as G

pytestmark = pytest.mark.gpu

C3 = 3
VAR_ITER = 1 << 61


# ---- per-chain diagonals in the CG launches --------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", [1, 257, 256 * 256 + 1])
def test_cg_launches_with_per_chain_diagonals(n, cplx):
    """cg_apply, cg_update and cg_rhs with one row of D, M^-1 and S per chain: every element within the bound of cg_np's
    extended-precision model run chain by chain with that chain's row; with three identical rows the bits of the
    shared-vector call.  In the cg_apply part chain 2 is frozen by the rows of test_gpu_cg.py (its W is not written), so
    chains 0 and 1, whose rows differ, carry the comparison there; cg_update and cg_rhs check all three rows.  cg_np has no
    model of cg_rhs: it is held to the extended-precision statement of its three operations, as test_gpu_cg.py holds it."""
    import torch

    from pxmcmc_amd import ops

    rng = np.random.default_rng(400 + n + 7 * cplx)
    r = _rand(rng, (C3, n), cplx)
    u = rng.uniform(0.3, 0.7, size=(C3, n)) * r
    b0 = _rand(rng, n, cplx)
    q = 2.0 * u - b0
    tol = 1e-3

    def apply(D):
        rows = _rows(C3, np.sum(np.abs(r) ** 2, axis=1) * 4.0 + 1.0)
        gam0 = np.sum((np.conj(r[0]) * u[0]).real)
        rows[0, [cg_np.GAMMA_OLD, cg_np.ALPHA_OLD]] = [4.0 * gam0, gam0 / np.sum((3.0 + 2.0) * np.abs(u[0]) ** 2)]
        W, coef = torch.full((C3, n), float("nan"), dtype=_dev(u, cplx).dtype, device=ops.device()), _dev(rows)
        ops.cg_apply(_dev(u, cplx), _dev(q, cplx), _dev(b0, cplx), _dev(D), _dev(r, cplx), coef, tol, out=W)
        return rows, W.cpu().numpy(), coef.cpu().numpy()

    D = rng.uniform(0.5, 3.0, size=(C3, n))
    rows, Wh, got = apply(D)
    for c in range(2):  # (chain 2 is frozen: test_gpu_cg.py covers it)
        w_ld, w_bound = cg_np.cg_apply_ld(u[c], q[c], b0, D[c], r[c])
        assert cg_np.within(Wh[c], w_ld, w_bound), np.abs(Wh[c] - w_ld).max()
        (gam, _, rho), (bg, _, br) = cg_np.cg_sums_ld(u[c], Wh[c], r[c])
        assert abs(got[c, cg_np.GAMMA_OLD] - gam) <= bg and abs(got[c, cg_np.RHO] - rho) <= br
        assert got[c, cg_np.FLAGS] == 0 and got[c, cg_np.ITERS] == rows[c, cg_np.ITERS] + 1
    assert np.isnan(Wh[2].real).all()
    _, W_same, coef_same = apply(np.tile(D[1], (C3, 1)))
    _, W_shared, coef_shared = apply(D[1])
    assert np.array_equal(W_same[:2], W_shared[:2]) and np.array_equal(coef_same, coef_shared)

    uu, w, p, s, x = (_rand(rng, (C3, n), cplx) for _ in range(5))
    urows = _rows(C3, 1.0)
    urows[1, [cg_np.ALPHA, cg_np.BETA, cg_np.ITERS]] = [0.9, 0.0, 1]

    def update(minv):
        d = {k: _dev(v, cplx) for k, v in dict(u=uu, w=w, p=p, s=s, x=x, r=r).items()}
        x1 = torch.full_like(d["x"], float("nan"))
        ops.cg_update(d["u"], d["w"], d["p"], d["s"], d["x"], d["r"], _dev(minv), _dev(urows), out=x1)
        return [t.cpu().numpy() for t in (d["p"], d["s"], x1, d["r"], d["u"])]

    minv = rng.uniform(0.2, 2.0, size=(C3, n))
    got = update(minv)
    for c in range(C3):
        outs, bounds = cg_np.cg_update_ld(uu[c], w[c], p[c], s[c], x[c], r[c], minv[c], urows[c])
        if urows[c, cg_np.FLAGS] != 0:
            for g, keep in zip(got, (p, s, x, r, uu)):
                assert np.array_equal(g[c], keep[c])
        else:
            for name, g, want, bound in zip("psxru", got, outs, bounds):
                assert cg_np.within(g[c], want, bound), name
    for a, b in zip(update(np.tile(minv[0], (C3, 1))), update(minv[0])):
        assert np.array_equal(a, b)

    g, z, bb = _rand(rng, (C3, n), cplx), _rand(rng, (C3, n), cplx), _rand(rng, n, cplx)
    S = rng.uniform(0.5, 2.0, size=(C3, n))
    rhs = lambda Sv: ops.cg_rhs(_dev(x, cplx), B=_dev(bb, cplx), G=_dev(g, cplx), g_scale=-0.5, Z=_dev(z, cplx), S=_dev(Sv),  # noqa: E731
                                z_scale=2.0).cpu().numpy()
    got = rhs(S)
    LD = np.clongdouble if cplx else np.longdouble
    for c in range(C3):
        want = bb.astype(LD) - 0.5 * g[c].astype(LD) + (2.0 * S[c]) * z[c].astype(LD)
        mag = lambda part: np.abs(part(bb)) + 0.5 * np.abs(part(g[c])) + 2.0 * S[c] * np.abs(part(z[c]))  # noqa: E731
        bound = 3 * cg_np.EPS * (mag(np.real) + (1j * mag(np.imag) if cplx else 0))  # two fma roundings (2 S_i is exact), + 1
        assert cg_np.within(got[c], want, bound)
    assert np.array_equal(rhs(np.tile(S[2], (C3, 1))), rhs(S[2]))


# ---- the variance draw -----------------------------------------------------------------------------------------------------
def _draw_case(cplx, q):
    from pxmcmc_amd import ops

    S = ops.GIBBS_SLICE
    sizes = np.array([1, 2, 255, 256, 257, S, S + 1, 2 * S + 3])
    b = np.concatenate([[0], np.cumsum(sizes)])
    nu = G.nu_rule(sizes, 2 if cplx else 1, q)
    fixed = np.nonzero(nu < 1)[0]
    assert set(fixed) <= {0, 1}  # only the 1- and 2-element groups, wherever their nu < 1
    return b, nu, fixed, ops.GibbsGroups(b, b[-1], fixed)


def _draw(groups, X, Dg0, h, q, d_lo, d_hi, seed, chain0, it, n_trace=4, row=2):
    import torch

    from pxmcmc_amd import ops

    C, n, K = Dg0.shape[0], groups.n, groups.K
    dev = ops.device()
    Dg = _dev(Dg0)
    D, sD, Mi = (torch.full((C, n), float("nan"), dtype=torch.float64, device=dev) for _ in range(3))
    sums = torch.full((C, K, 2), float("nan"), dtype=torch.float64, device=dev)
    trace = torch.zeros((n_trace, C, K), dtype=torch.float64, device=dev)
    ops.group_variance_draw(X, groups, Dg, D, sD, Mi, q=q, h=h, d_lo=d_lo, d_hi=d_hi, seed=seed, chain0=chain0, it=it, sums=sums,
                            trace=trace, trace_row=row)
    return tuple(t.cpu().numpy() for t in (Dg, D, sD, Mi, sums, trace))


@pytest.mark.parametrize("q", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_variance_draw_against_model(cplx, q):
    """sigma_k, chi2_k and D_k of every sampled group within the derived bounds of the extended-precision model fed the
    deviates of ops.randn; the expanded D (a copy), sqrt(D) and M^-1 element by element; the trace row; a fixed group keeps
    its bits; X = 0 gives d_hi; two calls give the same bits"""
    from pxmcmc_amd import ops

    b, nu, fixed, groups = _draw_case(cplx, q)
    n, K = int(b[-1]), b.size - 1
    rng = np.random.default_rng(500 + 3 * cplx + int(2 * q))
    x = _rand(rng, (C3, n), cplx) * rng.uniform(0.1, 3.0, size=(C3, 1))
    Dg0 = rng.uniform(0.5, 2.0, size=(C3, K))
    seed, chain0, it, d_lo, d_hi = 9, 5, VAR_ITER + 3, 1e-3, 1e3
    hv = rng.uniform(0.1, 1.0, size=C3)
    h = _dev(hv) if cplx else float(hv[0])
    X = _dev(x, cplx)
    Dg, D, sD, Mi, sums, trace = _draw(groups, X, Dg0, h, q, d_lo, d_hi, seed, chain0, it)
    omega = ops.randn(n + K + 1, C3, complex_=True, seed=seed, chain0=chain0, it=it, noise64=True).cpu().numpy()
    sampled = ~groups.fixed
    assert np.array_equal(np.nonzero(~sampled)[0], fixed)
    for c in range(C3):
        ld = G.variance_draw_ld(x[c], b, q, sampled, Dg0[c], omega[c], d_lo, d_hi)
        for k in range(K):
            if not sampled[k]:
                assert Dg[c, k] == Dg0[c, k] and np.isnan(sums[c, k]).all()
                continue
            assert abs(sums[c, k, 0] - ld["sigma"][k]) <= ld["sigma_bound"][k], (c, k, sums[c, k, 0], ld["sigma"][k])
            assert abs(sums[c, k, 1] - ld["chi2"][k]) <= ld["chi2_bound"][k], (c, k, sums[c, k, 1], ld["chi2"][k])
            assert abs(Dg[c, k] - ld["D"][k]) <= ld["D_bound"][k], (c, k, Dg[c, k], ld["D"][k], ld["D_bound"][k])
            assert d_lo <= Dg[c, k] <= d_hi
        (eD, esD, eMi), (_, bsD, bMi) = G.expand_ld(Dg[c], b, hv[c] if cplx else hv[0])
        assert np.array_equal(D[c], eD)
        assert np.all(np.abs(sD[c] - esD) <= bsD) and np.all(np.abs(Mi[c] - eMi) <= bMi)
    assert np.array_equal(trace[2], Dg) and not trace[[0, 1, 3]].any()
    # the deviates matter: the draw differs from chain to chain and from the start values
    assert np.all(Dg[:, sampled] != Dg0[:, sampled]) and np.all(Dg[0, sampled] != Dg[1, sampled])
    again = _draw(groups, X, Dg0, h, q, d_lo, d_hi, seed, chain0, it)
    for a, g in zip(again, (Dg, D, sD, Mi, sums, trace)):
        assert np.array_equal(a, g, equal_nan=True)
    zero = _draw(groups, 0 * X, Dg0, h, q, d_lo, d_hi, seed, chain0, it)[0]
    assert np.all(zero[:, sampled] == d_hi) and np.array_equal(zero[:, ~sampled], Dg0[:, ~sampled])
    # a clamp that binds from below
    low = _draw(groups, 1e3 * X, Dg0, h, q, d_lo, d_hi, seed, chain0, it)[0]
    assert np.all(low[:, 2:] == d_lo)  # the groups of 255 elements and more: chi2 / sigma ~ 1 / |1e3 x|^2 <= 1e-4


def test_variance_draw_graph_replay_equals_eager():
    """the three launches captured into a HIP graph and replayed equal the eager call bit for bit"""
    import torch

    from pxmcmc_amd import ops

    b, nu, fixed, groups = _draw_case(True, 0.0)
    n, K = int(b[-1]), b.size - 1
    rng = np.random.default_rng(6)
    X = _dev(_rand(rng, (C3, n), True), True)
    Dg0 = rng.uniform(0.5, 2.0, size=(C3, K))
    dev = ops.device()
    new = lambda: (_dev(Dg0), *(torch.full((C3, n), float("nan"), dtype=torch.float64, device=dev) for _ in range(3)))  # noqa: E731
    scratch = groups.scratch(C3)
    run = lambda Dg, D, sD, Mi: ops.group_variance_draw(X, groups, Dg, D, sD, Mi, q=0.0, h=0.25, seed=1, chain0=2, it=VAR_ITER,  # noqa: E731
                                                        scratch=scratch)
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
    assert torch.isnan(got[1]).all()  # capture does not execute
    g.replay()
    torch.cuda.synchronize()
    want = new()
    run(*want)
    torch.cuda.synchronize()
    for a, e in zip(got, want):
        assert torch.equal(a.view(torch.int64), e.view(torch.int64))


# ---- the sampler -----------------------------------------------------------------------------------------------------------
DENSE_BOUNDS = np.array([0, 5, 20, 41, 64])
DENSE = {}


def _dense_problem():
    """a dense real Phi [96, 64] as a path-integral measurement, four groups; -> (Phi, w, data, prior precision [64])"""
    rng = np.random.default_rng(31)
    m, n = 96, 64
    Phi = rng.normal(size=(m, n)) / np.sqrt(m)
    sig = 0.3
    truth = rng.normal(size=n) * np.sqrt(np.repeat([2.0, 0.5, 1.0, 4.0], np.diff(DENSE_BOUNDS)))
    data = Phi @ truth + sig * rng.normal(size=m)
    return Phi, np.full(m, 1 / sig ** 2), data, np.repeat([1.0, 2.0, 0.5, 1.5], np.diff(DENSE_BOUNDS)), sig


def _dense_gibbs(use_graph=True):
    """the sampler on the dense problem: C = 2, 3 sweeps, tol = 1e-12 -> (sampler, X [3, 2, 64])"""
    if use_graph not in DENSE:
        from pxmcmc_amd.forward import ForwardOperator
        from pxmcmc_amd.measurements import PathIntegral
        from pxmcmc_amd.optim import GaussianGibbs
        from pxmcmc_amd.prior import Gaussian

        Phi, w, data, p0, sig = _dense_problem()
        op = ForwardOperator(data, sig, "analysis", measurement=PathIntegral(Phi), nparams=Phi.shape[1])
        gib = GaussianGibbs(op, Gaussian(p0, 1.0), _params(), nchains=2, groups=DENSE_BOUNDS, hyper_q=0.0, tol=1e-12, seed=4,
                            chain_offset=3, use_graph=use_graph)
        DENSE[use_graph] = (gib, gib.run(3))
    return DENSE[use_graph]


def _stream(gib, m, t):
    """the deviates of sweep t from the device's own stream: omega_1 [C, m], omega_2 [C, n], the variance stream [C, n + K + 1]"""
    from pxmcmc_amd import ops

    kw = dict(seed=gib.seed, chain0=gib.chain_offset, noise64=True)
    C, cplx = gib.nchains, gib._dt.is_complex
    return (ops.randn(m, C, complex_=cplx, it=2 * t, **kw).cpu().numpy(), ops.randn(gib._n, C, complex_=cplx, it=2 * t + 1, **kw).cpu().numpy(),
            ops.randn(gib._n + gib.K + 1, C, complex_=True, it=VAR_ITER + t, **kw).cpu().numpy())


def test_sampler_follows_the_numpy_statement():
    """dense Phi (n = 64), four groups, C = 2, 3 sweeps: every sweep of the GPU chain is the sweep of gibbs_np fed the same
    deviates and the chain's own precisions of the sweep before -- the field within tol cond(H) (the solver stops at a
    recurrence residual of tol ||b||, and the condition number is computed here from the dense matrix), the precisions
    within what that allows (sigma is quadratic in the field) plus the bound of the draw's own roundings.  The free-running numpy chain is
    followed within the same bounds compounded: an error e of the precisions moves the next field by at most cond(H) e."""
    gib, X = _dense_gibbs()
    Phi, w, data, p0, _ = _dense_problem()
    b, tol, C = DENSE_BOUNDS, 1e-12, 2
    assert gib.solve_converged.all() and gib.used_graph and X.shape == (3, C, 64)
    assert gib.precision_chain.shape == (3, C, 4) and np.array_equal(gib.variance_chain, 1 / gib.precision_chain)
    sampled = np.ones(4, dtype=bool)
    start = np.array([1.0, 2.0, 0.5, 1.5])
    free = np.tile(start, (C, 1))
    free_err = 0.0  # bound of the relative distance of the GPU's precisions to the free-running chain's
    # the draw's own roundings, on both sides: sigma of at most 23 terms, chi2 of at most 21 (gibbs_np.variance_draw_ld), a division
    draw = 2 * (24 + 22 + 2) * cg_np.EPS
    for t in range(3):
        w1, w2, wv = _stream(gib, len(data), t)
        worst = 0.0
        for c in range(C):
            prev = start if t == 0 else gib.precision_chain[t - 1, c]
            H = Phi.T @ (w[:, None] * Phi) + np.diag(np.repeat(prev, np.diff(b)))
            cond = np.linalg.cond(H)
            x, Dn = G.gibbs_sweep_np(Phi, w, data, b, 0.0, sampled, prev, w1[c], w2[c], wv[c], *gib.precision_bounds)
            # a relative error e of the field is at most e ||x|| / ||x_k|| of group k, and sigma_k is quadratic in it
            amp = np.linalg.norm(x) / np.sqrt(np.add.reduceat(x * x, b[:-1]))
            ex = np.linalg.norm(X[t, c] - x) / np.linalg.norm(x)
            eD = np.abs(gib.precision_chain[t, c] / Dn - 1)
            print(f"sweep {t} chain {c}: cond {cond:.1f}, field error {ex:.2e} (<= {tol * cond:.2e}), precision errors {eD}")
            assert ex <= tol * cond
            assert np.all(eD <= 2.5 * (tol * cond) * amp + draw)  # (1 + e)^2 - 1 <= 2.5 e
            # the free-running chain
            xf, free[c] = G.gibbs_sweep_np(Phi, w, data, b, 0.0, sampled, free[c], w1[c], w2[c], wv[c], *gib.precision_bounds)
            bound = tol * cond + 1.01 * cond * free_err
            ampf = np.linalg.norm(xf) / np.sqrt(np.add.reduceat(xf * xf, b[:-1]))
            assert np.linalg.norm(X[t, c] - xf) <= bound * np.linalg.norm(xf)
            assert np.all(np.abs(gib.precision_chain[t, c] / free[c] - 1) <= 2.5 * bound * ampf + draw)
            worst = max(worst, float(np.max(2.5 * bound * ampf + draw)))
        free_err = worst


def test_graph_flag_gives_the_same_bits():
    gib, X = _dense_gibbs()
    eager, Xe = _dense_gibbs(use_graph=False)
    assert gib.used_graph and not eager.used_graph
    assert np.array_equal(X, Xe) and np.array_equal(gib.precision_chain, eager.precision_chain)
    assert np.array_equal(gib.solve_iterations, eager.solve_iterations)


def test_sphere_degree_groups():
    """harmonic state with the identity measurement at L = 8, one group per degree, lmin = 2, C = 4, 5 sweeps: every solve
    converges; each chain's field draw is the dense solve of its own right-hand side with that chain's own D; cl_chain has
    shape [5, 4, 8] and degrees 0 and 1 never move"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.optim import GaussianGibbs
    from pxmcmc_amd.prior import Gaussian
    from pxmcmc_amd.transforms import SphericalHarmonicTransform

    L, C, nsweeps, tol = 8, 4, 5, 1e-8
    P, n = L * (2 * L - 1), L * L
    rng = np.random.default_rng(8)
    tr = SphericalHarmonicTransform(L, max_chains=C)
    op = ForwardOperator(rng.normal(size=P), 0.5, "synthesis", transform=tr, measurement=Identity(P, P), nparams=n)
    cl = 1.0 / (1.0 + np.arange(L)) ** 2
    gib = GaussianGibbs(op, Gaussian.from_power_spectrum(cl, L, 1.0), _params(complex=True), nchains=C, groups="degree", lmin=2,
                        tol=tol, seed=2, chain_offset=1)
    assert gib.group_bounds.tolist() == [l * l for l in range(L + 1)] and gib.sampled.tolist() == [False, False] + [True] * 6
    assert gib.nu.tolist() == [4 * l for l in range(L)]
    X = gib.run(nsweeps)
    assert gib.solve_converged.shape == (nsweeps, C) and gib.solve_converged.all() and (gib.solve_iterations > 0).all()
    assert gib.cl_chain.shape == (nsweeps, C, L) and gib.cl_chain is gib.variance_chain
    assert np.all(gib.cl_chain[:, :, :2] == gib.cl_chain[0, 0, :2]) and np.allclose(gib.cl_chain[0, 0, :2], cl[:2], rtol=1e-15)
    assert np.all(gib.cl_chain[1:, :, 2:] != gib.cl_chain[:-1, :, 2:])
    # the linear part A of the operator as a dense matrix, the basis vectors C at a time
    b0 = gib._b0.cpu().numpy()
    A = np.zeros((n, n), dtype=complex)
    for j0 in range(0, n, C):
        E = torch.zeros((C, n), dtype=gib._dt, device=ops.device())
        E[torch.arange(C), torch.arange(j0, j0 + C)] = 1.0
        A[:, j0:j0 + C] = (gib._linear(E).cpu().numpy() + b0).T
    A = 0.5 * (A + A.conj().T)
    start = np.repeat(1.0 / cl, 2 * np.arange(L) + 1)
    for t in range(nsweeps):
        # the right-hand sides of sweep t: formed with the precisions the sweep before left
        gib._Dg.copy_(ops.as_device(np.tile(1.0 / cl, (C, 1)) if t == 0 else gib.precision_chain[t - 1]))
        gib._expand()
        B = gib.draw_rhs(t).cpu().numpy()
        for c in range(C):
            D = start if t == 0 else np.repeat(gib.precision_chain[t - 1, c], 2 * np.arange(L) + 1)
            H = A + np.diag(D)
            _assert_solves(H, B[c], X[t, c], tol, np.linalg.cond(H))


def test_construction_refuses_and_scales():
    """GaussianGibbs itself refuses bad offsets, an unsampled group that is not fixed, a precision that is not constant inside
    a group, clamp limits that are not finite and positive, an exponent that is not a half-integer <= 2, a preconditioner
    other than "diag" and lmin without degree groups; lmin maps to the fixed degrees; the precision enters as p T / lmda and
    is reported back in the prior's units"""
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.optim import GaussianGibbs
    from pxmcmc_amd.prior import Gaussian
    from pxmcmc_amd.transforms import SphericalHarmonicTransform

    data, b = identity_model()
    n = data.size
    op = ForwardOperator(data, 0.5, "analysis", measurement=Identity(n, n), nparams=n)
    prior, params = Gaussian(2.0, 3.0), _params(lmda=1.5)
    make = lambda **kw: GaussianGibbs(op, kw.pop("prior", prior), params, nchains=2, **{"groups": b, **kw})  # noqa: E731
    for bad in ([0, 3, 63], [1, 3, 64], [0, 3, 3, 64], [0, 5, 3, 64], [0.0, 3.0, 64.0], [64]):
        with pytest.raises(ValueError):
            make(groups=bad)
    with pytest.raises(ValueError, match="fixed"):
        make(groups=[0, 2, 64])  # real, n_k = 2, q = 0: nu = 0
    with pytest.raises(ValueError, match="fixed"):
        make(groups=[0, 1, 64], hyper_q=0.5)  # nu = 0
    with pytest.raises(ValueError):
        make(fixed=[4])
    uneven = np.repeat([1.0, 2.0, 3.0, 4.0], np.diff(b))
    assert make(prior=Gaussian(uneven, 3.0))._Dg0[0].tolist() == [2.0, 4.0, 6.0, 8.0]
    uneven[5] = 2.5
    with pytest.raises(ValueError, match="constant"):
        make(prior=Gaussian(uneven, 3.0))
    for pb in ((0.0, 1.0), (1.0, np.inf), (np.nan, 1.0), (-1.0, 1.0), (2.0, 1.0)):
        with pytest.raises(ValueError):
            make(precision_bounds=pb)
    for q in (0.25, 2.5, np.nan):
        with pytest.raises(ValueError):
            make(hyper_q=q)
    for precond in (None, np.ones(n)):
        with pytest.raises(ValueError, match="diag"):
            make(precond=precond)
    with pytest.raises(ValueError, match="lmin"):
        make(lmin=2)
    for groups in ("degree", "scale", "rings"):  # (no transform of that kind on this operator)
        with pytest.raises(ValueError):
            make(groups=groups)
    # D = p T / lmda = 4 inside the solver, reported as p = 2; a fixed group keeps it
    gib = make(fixed=[0, 2], seed=1)
    assert gib._Dg0.cpu().numpy().tolist() == [[4.0] * 4] * 2 and gib.sampled.tolist() == [False, True, False, True]
    gib.run(2)
    assert np.all(gib.precision_chain[:, :, [0, 2]] == 2.0) and np.all(gib.variance_chain[:, :, [0, 2]] == 0.5)
    assert np.all(gib.precision_chain[:, :, [1, 3]] != 2.0)
    assert np.array_equal(gib._Dg.cpu().numpy(), gib.precision_chain[-1] * 2.0)
    # lmin -> the fixed degrees, together with fixed=
    L = 4
    P = L * (2 * L - 1)
    sph = ForwardOperator(np.zeros(P), 0.5, "synthesis", transform=SphericalHarmonicTransform(L, max_chains=2),
                          measurement=Identity(P, P), nparams=L * L)
    cl = Gaussian.from_power_spectrum(np.ones(L), L, 1.0)
    with pytest.raises(ValueError, match="fixed"):
        GaussianGibbs(sph, cl, _params(complex=True), nchains=2, groups="degree")  # the monopole at q = 0: nu = 0
    assert GaussianGibbs(sph, cl, _params(complex=True), nchains=2, groups="degree", lmin=1).sampled.tolist() == [False, True, True, True]
    assert GaussianGibbs(sph, cl, _params(complex=True), nchains=2, groups="degree", lmin=2, fixed=[3]).sampled.tolist() == [False, False, True, False]
    assert GaussianGibbs(sph, cl, _params(complex=True), nchains=2, groups="degree", hyper_q=1.0).sampled.all()  # nu_0 = 2


def test_distribution_on_the_identity_model():
    """the identity model of tests/test_gibbs_host.py on the same inputs: the mean of log v of every group within 5 standard
    errors (of the 16 chain means) of the quadrature value, and hyper_summary reads out R-hat < 1.1"""
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.optim import GaussianGibbs
    from pxmcmc_amd.prior import Gaussian

    data, b = identity_model()
    expected = identity_expected_log_variance(data, b)
    n = data.size
    op = ForwardOperator(data, np.sqrt(IDENTITY_NOISE_VAR), "analysis", measurement=Identity(n, n), nparams=n)
    gib = GaussianGibbs(op, Gaussian(1.0, 1.0), _params(), nchains=IDENTITY_CHAINS, groups=b, hyper_q=0.0, tol=1e-10, seed=77)
    post = gib.run(IDENTITY_SWEEPS, nburn=IDENTITY_BURN, summary="state")
    assert gib.solve_converged.all() and gib.variance_chain.shape == (IDENTITY_SWEEPS - IDENTITY_BURN, IDENTITY_CHAINS, 4)
    z = z_scores(np.log(gib.variance_chain), expected)
    rhat = gib.hyper_summary.rhat().cpu().numpy()
    print("GPU sampler: expected log v", expected, "z", z, "R-hat", rhat, "iterations", gib.solve_iterations.max())
    assert np.all(np.abs(z) <= 5.0), z
    assert rhat.shape == (4,) and np.all(rhat < 1.1), rhat
    # hyper_summary is the streaming summary of log v over the kept sweeps
    mean = gib.hyper_summary.mean().cpu().numpy()
    assert np.allclose(mean, np.log(gib.variance_chain).mean(axis=0), rtol=0, atol=1e-12 * np.abs(expected).max())
    assert post.mean().shape == (IDENTITY_CHAINS, n)
