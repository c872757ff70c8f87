"""The HEALPix ring synthesis kernels (ops.HpxPlan, csrc/healpix.hip), the measurements built on them and the samplers on
those measurements, on the GPU.

Kernel bound, the rule of tests/test_harmwav_step_host.py: per element |device - long-double model| <= 4 C0_MEASURED 2^-52 S,
with C0_MEASURED the constant the float64 numpy route needs against the same model (tests/test_healpix_host.py) and S the
scale sum |lam| |f| (synthesis, per pixel) or sum |lam| |v| (adjoint, per coefficient); the factor 4 covers the other
summation order of the device.  Each case prints its largest ratio |device - model| / (2^-52 S) as ``HPX-RATIO``.
"""
import contextlib
import io

import numpy as np
import pytest
from test_healpix_host import C0_MEASURED, EPS64, draw, model

pytestmark = pytest.mark.gpu

# (L, nside, spin): the smallest sizes at which each mechanism can fail
CASES = [
    (4, 1, 0),     # every ring nphi = 4 < 2L-1 = 7: the fold; shifted against unshifted rings
    (12, 2, 0),    # a several-fold alias, 23 orders onto 8
    (3, 4, 0),     # 2L-1 = 5 < nphi: no alias, zero-padded orders
    (9, 3, 2),     # nside not a power of two, q = 3 in the belt; spin 2 with the rows l < 2 zero
    (16, 4, 2),    # cap rings q = 1, 2, 3 beside belt rings
    (8, 256, 0),   # long rings and many workgroups, 786 432 pixels
    (64, 32, 2),   # the Legendre kernels past one tile in l, m and rings
    (2, 512, 0),   # (beyond the list of the issue) the largest nside that must work: a phi stage with more than 64 KB of LDS
]


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _dev(x):
    from pxmcmc_amd import ops

    return ops.as_device(np.ascontiguousarray(x))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_plan_against_the_long_double_model(case, capsys):
    import torch

    from pxmcmc_amd import ops

    L, nside, spin = case
    C = 3 if nside < 512 else 1
    M = model(*case, np.longdouble)
    f, v = draw(*case, seed=11, chains=C)
    plan, alone = ops.HpxPlan(L, nside, spin, max_chains=5), ops.HpxPlan(L, nside, spin, max_chains=1)
    assert plan.npix == 12 * nside * nside and plan.nlm == L * L and plan.table_bytes() > 0
    assert plan in ops.live_plans() and plan.status() == 0
    nan = complex(np.nan, np.nan)
    fd, vd = _dev(f), _dev(v)
    got_v = plan.synthesis(fd, out=torch.full((C, plan.npix), nan, dtype=torch.complex128, device=fd.device))
    got_f = plan.synthesis_adjoint(vd, out=torch.full((C, plan.nlm), nan, dtype=torch.complex128, device=fd.device))
    worst = [0.0, 0.0]
    for c in range(C):
        # the same chain alone, on a plan of one chain: bit-equal
        one_v = alone.synthesis(fd[c:c + 1], out=torch.full((1, plan.npix), nan, dtype=torch.complex128, device=fd.device))
        one_f = alone.synthesis_adjoint(vd[c:c + 1], out=torch.full((1, plan.nlm), nan, dtype=torch.complex128, device=fd.device))
        assert torch.equal(one_v[0], got_v[c]) and torch.equal(one_f[0], got_f[c]), c
        for k, (got, want, S) in enumerate(((got_v[c], M.synthesis(f[c]), M.synthesis_scale(f[c])),
                                            (got_f[c], M.synthesis_adjoint(v[c]), M.adjoint_scale(v[c])))):
            got = got.cpu().numpy()
            assert np.isfinite(got).all()
            err = np.abs(got - want).astype(np.float64)
            ok = S > 0
            assert (got[~ok] == 0).all()  # (rows l < |spin|: exact zeros)
            worst[k] = max(worst[k], float((err[ok] / (EPS64 * S[ok])).max()))
    with capsys.disabled():
        print(f"\nHPX-RATIO {case}: synthesis {worst[0]:.3f}, adjoint {worst[1]:.3f} (bound {4 * C0_MEASURED:.2f})")
    assert worst[0] <= 4 * C0_MEASURED and worst[1] <= 4 * C0_MEASURED, worst
    assert plan.status() == 0


def _adjointness(A, AH, n_in, n_out, seed):
    """|<A x, w> - <x, A^H w>| <= 1e-12 ||A x|| ||w|| on device vectors"""
    rng = np.random.default_rng(seed)
    x = _dev(rng.normal(size=n_in) + 1j * rng.normal(size=n_in))
    w = _dev(rng.normal(size=n_out) + 1j * rng.normal(size=n_out))
    Ax, AHw = A(x).cpu().numpy(), AH(w).cpu().numpy()
    x, w = x.cpu().numpy(), w.cpu().numpy()
    assert abs(np.vdot(w, Ax) - np.vdot(AHw, x)) <= 1e-12 * np.linalg.norm(Ax) * np.linalg.norm(w)
    assert np.linalg.norm(Ax) > 0


@pytest.mark.parametrize("case", [(12, 2, 0), (9, 3, 2), (64, 32, 2)], ids=str)
def test_plan_adjointness_on_the_device(case):
    from pxmcmc_amd import ops

    L, nside, spin = case
    plan = ops.HpxPlan(L, nside, spin)
    rng = np.random.default_rng(2)
    x = rng.normal(size=L * L) + 1j * rng.normal(size=L * L)
    x[: spin * spin] = 0
    w = rng.normal(size=plan.npix) + 1j * rng.normal(size=plan.npix)
    Ax, AHw = plan.synthesis(_dev(x)).cpu().numpy(), plan.synthesis_adjoint(_dev(w)).cpu().numpy()
    assert abs(np.vdot(w, Ax) - np.vdot(AHw, x)) <= 1e-12 * np.linalg.norm(Ax) * np.linalg.norm(w)


def _mask_and_ngal(nside, seed=5):
    rng = np.random.default_rng(seed)
    npix = 12 * nside * nside
    return rng.random(npix) > 0.3, rng.integers(5, 40, size=npix).astype(float)


@pytest.mark.parametrize("harmonic", [False, True], ids=["pixel", "harmonic"])
@pytest.mark.parametrize("masked", [False, True], ids=["full", "masked"])
def test_measurement_adjointness_on_the_device(harmonic, masked):
    from pxmcmc_amd.measurements import HealpixSampling, WeakLensingHealpix

    L, nside = 10, 3
    mask, ngal = _mask_and_ngal(nside)
    kernel = 1.0 / (1.0 + np.arange(L))
    w = np.sqrt(ngal[mask]) if masked else None
    hs = HealpixSampling(L, nside, spin=0, kernel=kernel if masked else None, mask=mask if masked else None, harmonic=harmonic, weights=w)
    wl = WeakLensingHealpix(L, nside, mask=mask if masked else None, ngal=ngal if masked else None, harmonic=harmonic)
    for k, m in enumerate((hs, wl)):
        assert m.ndata == (int(mask.sum()) if masked else 12 * nside * nside)
        _adjointness(m.forward, m.adjoint, m.npix, m.ndata, seed=20 + k)


def test_measurements_match_the_numpy_statement():
    from pxmcmc_amd.healpix_np import HealpixSamplingNp, WeakLensingHealpixNp
    from pxmcmc_amd.measurements import HealpixSampling, WeakLensingHealpix

    L, nside = 8, 4
    mask, ngal = _mask_and_ngal(nside)
    kernel = 1.0 / (1.0 + np.arange(L))
    rng = np.random.default_rng(9)
    for harmonic in (False, True):
        pairs = [(HealpixSampling(L, nside, kernel=kernel, mask=mask, harmonic=harmonic, max_chains=2),
                  HealpixSamplingNp(L, nside, kernel=kernel, mask=mask, harmonic=harmonic)),
                 (WeakLensingHealpix(L, nside, mask=mask, ngal=ngal, harmonic=harmonic, max_chains=2),
                  WeakLensingHealpixNp(L, nside, mask=mask, ngal=ngal, harmonic=harmonic))]
        for dev, ref in pairs:
            x = rng.normal(size=(2, dev.npix)) + 1j * rng.normal(size=(2, dev.npix))
            y = rng.normal(size=(2, dev.ndata)) + 1j * rng.normal(size=(2, dev.ndata))
            fx, ay = dev.forward(x), dev.adjoint(y)  # (numpy in, numpy out)
            for c in range(2):
                want = ref.forward(x[c])
                assert np.abs(fx[c] - want).max() <= 1e-11 * np.abs(want).max()
                want = ref.adjoint(y[c])
                assert np.abs(ay[c] - want).max() <= 1e-11 * np.abs(want).max()
            est = dev.approx_analysis(y[0])
            assert np.abs(est - 4 * np.pi / (12 * nside * nside) * ay[0]).max() <= 1e-15 * np.abs(ay[0]).max()


def test_against_the_mw_path():
    """forward of a band-limited MW image = synthesis of its ShtPlan.forward; the harmonic forward of f_lm = the pixel forward
    of the MW image of f_lm, to the tolerance of the SHT round trip (tests/test_gpu_spinwav.py: 1e-12 relative)"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.measurements import HealpixSampling

    L, nside = 12, 4
    rng = np.random.default_rng(3)
    flm = _dev(rng.normal(size=(2, L * L)) + 1j * rng.normal(size=(2, L * L)))
    sht, hpx = ops.ShtPlan(L, 0, max_chains=2), ops.HpxPlan(L, nside, 0, max_chains=2)
    image = sht.inverse(flm)
    px, hm = HealpixSampling(L, nside, max_chains=2), HealpixSampling(L, nside, harmonic=True, max_chains=2)
    assert torch.equal(px.forward(image), hpx.synthesis(sht.forward(image)))
    a, b = hm.forward(flm), px.forward(image)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    assert torch.equal(a, hpx.synthesis(flm))


# ---- samplers on WeakLensingHealpix ----------------------------------------------------------------------------------------
def _sampler_problem(C=3):
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.measurements import WeakLensingHealpix
    from pxmcmc_amd.prior import S2_Wavelets_L1
    from pxmcmc_amd.transforms import SphericalWaveletTransform

    L, nside, B, J_min = 8, 4, 2, 0
    mask, ngal = _mask_and_ngal(nside)
    rng = np.random.default_rng(12)
    wl = WeakLensingHealpix(L, nside, mask=mask, ngal=ngal, max_chains=C)
    tr = SphericalWaveletTransform(L, B, J_min, max_chains=C)
    data = rng.normal(size=wl.ndata) + 1j * rng.normal(size=wl.ndata)
    op = ForwardOperator(data, 1 / wl.inv_cov, "synthesis", transform=tr, measurement=wl, nparams=tr.ncoefs)
    assert op._wl_plan() is None  # no fused attachment: the generic engine
    make_prior = lambda T: S2_Wavelets_L1("synthesis", tr.inverse, tr.inverse_adjoint, T, L=L, B=B, J_min=J_min)  # noqa: E731
    return dict(L=L, nside=nside, B=B, J_min=J_min, mask=mask, ngal=ngal, data=data, op=op, tr=tr, wl=wl, prior=make_prior, C=C)


def test_myula_graph_replay_equals_eager_stepping():
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams

    P = _sampler_problem()
    p = PxMCMCParams(lmda=1e-4, delta=5e-5, nsamples=5, nburn=0, ngap=1, verbosity=0)
    runs = []
    for use_graph in (True, False):
        s = MYULA(P["op"], P["prior"](p.lmda * p.mu), p, nchains=P["C"], seed=5, use_graph=use_graph)
        _quiet(s.run, start_point=np.zeros(P["op"].nparams))
        assert s.used_graph is use_graph, s.graph_error
        assert not getattr(s, "_fused_wav", False)
        runs.append(s)
    assert runs[0].chain.shape == (P["C"], 5, P["op"].nparams) and np.isfinite(runs[0].chain).all()
    np.testing.assert_array_equal(runs[0].chain, runs[1].chain)
    np.testing.assert_array_equal(runs[0].logPi, runs[1].logPi)
    assert np.abs(runs[0].chain[0] - runs[0].chain[1]).max() > 0


def test_myula_matches_the_oracle_loop():
    """five iterations with numpy noise against oracle.pxmcmc_np.myula_run over the numpy operators; tolerance 1e-10 of the
    chain's scale, that of the weak-lensing sampler checks (tests/test_gpu_g15.py)"""
    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.healpix_np import WeakLensingHealpixNp
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams

    P = _sampler_problem()
    C, N = P["C"], P["op"].nparams
    lmda, delta, mu = 1e-4, 5e-5, 1.0
    p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, nsamples=5, nburn=0, ngap=1, verbosity=0)
    rng = np.random.default_rng(1)
    X0 = rng.normal(size=N) * 0.01
    s = MYULA(P["op"], P["prior"](lmda * mu), p, nchains=C, rng="numpy")
    np.random.seed(1)
    _quiet(s.run, start_point=X0)
    T = ref.SphericalWaveletTransform(P["L"], P["B"], P["J_min"])
    owl = WeakLensingHealpixNp(P["L"], P["nside"], mask=P["mask"], ngal=P["ngal"])
    oop = ref.ForwardOperator(P["data"], 1 / owl.inv_cov, "synthesis", T, owl, T.ncoefs)
    oreg = ref.S2_Wavelets_L1("synthesis", None, None, lmda * mu, P["L"], P["B"], P["J_min"])
    np.random.seed(1)
    noise = np.stack([[np.random.randn(N) for _ in range(C)] for _ in range(5)])
    for c in range(C):
        out = ref.myula_run(oop, oreg, lmda, delta, mu, 5, 0, 1, X0.astype(complex), lambda i: noise[i][c])
        assert np.abs(s.chain[c] - out["chain"]).max() <= 1e-10 * np.abs(out["chain"]).max(), c


def test_pxmala_iteration_runs():
    from pxmcmc_amd.mcmc import PxMALA, PxMCMCParams

    P = _sampler_problem()
    p = PxMCMCParams(lmda=1e-4, delta=5e-5, nsamples=1, nburn=0, ngap=1, verbosity=0)
    s = PxMALA(P["op"], P["prior"](p.lmda * p.mu), p, tune_delta=True, nchains=P["C"], seed=2)
    _quiet(s.run, start_point=np.zeros(P["op"].nparams))
    assert s.chain.shape[0] == P["C"] and s.chain.shape[2] == P["op"].nparams and np.isfinite(s.chain).all()
    assert s.acceptance_trace.shape[1] == P["C"]


def test_fista_decreases_the_objective(capsys):
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.optim import FISTA

    P = _sampler_problem()
    p = PxMCMCParams(lmda=1e-4, mu=1.0, complex=False, verbosity=0)
    L_g = P["op"].gradient_lipschitz()
    assert np.isfinite(L_g) and L_g > 0
    est = FISTA(P["op"], P["prior"](p.lmda * p.mu), p, nchains=P["C"], gamma=1 / L_g, tol=0.0, max_iter=20, check_every=1)
    _quiet(est.run, start_point=None)
    obj = est.objective
    with capsys.disabled():
        print(f"\nFISTA on WeakLensingHealpix: L_g = {L_g:.6e}, objective of chain 0: {obj[0, 0]:.6e} -> {obj[-1, 0]:.6e}")
    assert obj.shape == (20, P["C"]) and np.isfinite(obj).all()
    assert (np.diff(obj, axis=0) <= 0).all()
