"""Harmonic-space wavelet transforms on the GPU (HarmWavPlan, SphericalWaveletTransform(harmonic=True)): the four
operators against the numpy model of tests/test_harmwav_host.py, the links to the pixel plans, the fused harmonic MYULA
step (pxm_hwav_myula_step) against the model, the samplers against the numpy samplers, graph replay, the Kaiser-Squires
estimate, the refusals, the pys2let shim and the weak-lensing example."""
import contextlib
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from test_harmwav_host import CASES, HarmWavModel, HarmWavOracleTransform, WeakLensingHarmonicOracle, band_limited_flm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _cplx(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _model(L, B, J_min, N=1, spin=0):
    """the numpy model on the library's tiling"""
    from pxmcmc_amd import ops

    return HarmWavModel(L, B, J_min, N, spin, tiling=ops.tiling_axisym(L, B, J_min))


# ---- the four operators ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("N,spin", CASES)
@pytest.mark.parametrize("L", [8, 16, 64, 256])
def test_four_ops_match_model(L, N, spin, C):
    from pxmcmc_amd import ops

    B, J_min = 2.0, 2
    rng = np.random.default_rng(1000 * L + 10 * N + spin + C)
    plan = ops.HarmWavPlan(L, B, J_min, N, spin=spin, max_chains=C)
    M = _model(L, B, J_min, N, spin)
    assert (plan.ncoefs, plan.nscal) == (M.ncoefs, M.nscal)
    X, f = _cplx(rng, C, M.ncoefs), _cplx(rng, C, L * L)
    rows = range(C) if L < 256 else (0, C - 1)
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        got = getattr(plan, name)(arg).cpu().numpy()
        ref = np.stack([getattr(M, name)(arg[c]) for c in rows])
        assert _rel(got[list(rows)], ref) <= 1e-12, name


@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("B,J_min", [(1.5, 1), (1.7, 2), (3.0, 1), (2.0, 0)])
@pytest.mark.parametrize("L", [13, 33])
def test_four_ops_match_model_other_tilings(L, B, J_min, N):
    """non-dyadic B, J_min = 0 and odd L (a partial last workgroup), and per block: every (scale, n) block of the split
    operators to 1e-12 of its own largest entry, so that the top scale cannot hide the others"""
    from pxmcmc_amd import ops

    C = 2
    rng = np.random.default_rng(1000 * L + 100 * J_min + 10 * N + int(10 * B))
    plan = ops.HarmWavPlan(L, B, J_min, N, max_chains=C)
    M = _model(L, B, J_min, N)
    assert (plan.ncoefs, plan.nscal) == (M.ncoefs, M.nscal)
    X, f = _cplx(rng, C, M.ncoefs), _cplx(rng, C, L * L)
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        got = getattr(plan, name)(arg).cpu().numpy()
        ref = np.stack([getattr(M, name)(arg[c]) for c in range(C)])
        assert _rel(got, ref) <= 1e-12, name
        if ref.shape[1] == M.ncoefs:
            for i in range(len(M.blocks)):
                a, b = M.offsets[i], M.offsets[i + 1]
                scale = np.abs(ref[:, a:b]).max()
                assert np.abs(got[:, a:b] - ref[:, a:b]).max() <= 1e-12 * scale, (name, i)


def test_transform_interface():
    """numpy in -> numpy out, torch in -> torch out, 1-D or [C, n], sizes, chain growth, round trip"""
    import torch

    from pxmcmc_amd.transforms import SphericalWaveletTransform

    L, B, J_min = 16, 2.0, 2
    T = SphericalWaveletTransform(L, B, J_min, dirs=2, harmonic=True)
    M = _model(L, B, J_min, 2, 0)
    assert (T.ncoefs, T.nscal, T.nwav) == (M.ncoefs, M.nscal, M.ncoefs - M.nscal)
    rng = np.random.default_rng(2)
    flm = band_limited_flm(rng, L)
    X = T.forward(flm)
    assert isinstance(X, np.ndarray) and X.shape == (M.ncoefs,)
    assert _rel(T.inverse(X), flm) < 1e-12
    T.ensure_chains(4)
    Xt = T.inverse_adjoint(torch.as_tensor(np.stack([flm] * 4)).cuda())
    assert isinstance(Xt, torch.Tensor) and Xt.shape == (4, M.ncoefs)
    assert _rel(Xt[3].cpu().numpy(), M.synthesis_adjoint(flm)) < 1e-12
    assert _rel(T.forward_adjoint(X), M.analysis_adjoint(X)) < 1e-12


# ---- links to the pixel plans -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin", [0, 2])
def test_link_n1_to_wavplan(spin):
    from pxmcmc_amd import ops
    from pxmcmc_amd.transforms import SphericalWaveletTransform

    L, B, J_min = 32, 2.0, 2
    rng = np.random.default_rng(9)
    flm = band_limited_flm(rng, L, spin)
    f = ops.ShtPlan(L, spin).inverse(flm)
    Xp = SphericalWaveletTransform(L, B, J_min, spin=spin).forward(f).cpu().numpy()
    Xh = SphericalWaveletTransform(L, B, J_min, spin=spin, harmonic=True).forward(flm)
    bls = ops.wav_bandlimits(L, B, J_min)
    po = np.concatenate([[0], np.cumsum([b * (2 * b - 1) for b in bls])])
    ho = np.concatenate([[0], np.cumsum([b * b for b in bls])])
    for i, bl in enumerate(bls):
        blk = ops.ShtPlan(bl, 0).forward(Xp[po[i] : po[i + 1]]).cpu().numpy()
        el = np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)
        if i:
            blk = np.sqrt(2 * np.pi) * np.sqrt(8 * np.pi ** 2 / (2 * el + 1)) * blk
        assert _rel(Xh[ho[i] : ho[i + 1]], blk) < 1e-11, i


def test_link_directional_to_dirwavplan():
    from pxmcmc_amd import ops

    L, B, J_min, N = 16, 2.0, 2, 4
    rng = np.random.default_rng(10)
    flm = band_limited_flm(rng, L)
    f = ops.ShtPlan(L, 0).inverse(flm)
    P = ops.DirWavPlan(L, B, J_min, N)
    Xp = P.analysis(f).cpu().numpy()
    Xh = ops.HarmWavPlan(L, B, J_min, N).analysis(flm).cpu().numpy()
    bls = ops.wav_bandlimits(L, B, J_min)
    b0 = bls[0]
    assert _rel(Xh[: b0 * b0], ops.ShtPlan(b0, 0).forward(Xp[: b0 * (2 * b0 - 1)]).cpu().numpy()) < 1e-11
    npl, gam = 2 * N - 1, 2 * np.pi * np.arange(2 * N - 1) / (2 * N - 1)
    po, ho = b0 * (2 * b0 - 1), b0 * b0
    for bl in bls[1:]:
        W = Xp[po : po + npl * bl * (2 * bl - 1)].reshape(npl, -1)
        el = np.repeat(np.arange(bl), 2 * np.arange(bl) + 1)
        for n in range(-(N - 1), N, 2):
            blk = Xh[ho : ho + bl * bl]
            if abs(n) < bl:
                g = (np.exp(-1j * n * gam)[:, None] * W).sum(0) / npl
                a = ops.ShtPlan(bl, -n).forward(g).cpu().numpy()
                ref = (-1.0) ** n * np.sqrt(2 * np.pi) * np.sqrt(8 * np.pi ** 2 / (2 * el + 1)) * a
                ref[el < abs(n)] = 0
                assert np.abs(blk - ref).max() < 1e-11 * np.abs(Xh).max(), (bl, n)
            else:
                assert np.all(blk == 0)
            ho += bl * bl
        po += npl * bl * (2 * bl - 1)


# ---- the fused step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("vector_sig", [False, True])
@pytest.mark.parametrize("wl", [False, True])
@pytest.mark.parametrize("N,spin", [(1, 0), (4, 0), (1, 2)])
def test_fused_step_matches_model(N, spin, wl, vector_sig, mode):
    import torch

    from oracle import pxmcmc_np as ref
    from pxmcmc_amd import ops

    L, B, J_min, C = 32, 2.0, 2, 3
    lmda, delta, seed, chain0, it = 2e-3, 5e-4, 5, 7, 11
    rng = np.random.default_rng(N + 10 * spin + 100 * wl + 1000 * vector_sig + mode)
    plan = ops.HarmWavPlan(L, B, J_min, N, spin=spin, max_chains=C)
    M = _model(L, B, J_min, N, spin)
    k = ref.wl_harmonic_kernel(L) if wl else None
    meas = (lambda v: ref.wl_harmonic_mapping(v, k)) if wl else (lambda v: v)
    X, data = _cplx(rng, C, M.ncoefs) * 0.1, _cplx(rng, L * L)
    invcov = 1.0 / np.linspace(0.5, 1.5, L * L) ** 2 if vector_sig else np.full(L * L, 4.0)
    T = np.abs(rng.normal(size=M.ncoefs)) * 0.05 if vector_sig else 0.05
    it_dev = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    Xn, Pn = plan.myula_step(X, data, invcov, k, T, delta, lmda, noise_complex=bool(mode), seed=seed, chain0=chain0, it=it,
                             iter_dev=it_dev, noise64=True)
    w = ops.randn(M.ncoefs, C, complex_=bool(mode), seed=seed, chain0=chain0, it=it + 3, noise64=True).cpu().numpy()
    for c in range(C):
        g = M.synthesis_adjoint(meas(invcov * (meas(M.synthesis(X[c])) - data)))
        want = ref.chain_step(X[c], ref.soft(X[c], T), g, delta, lmda, w[c])
        assert _rel(Xn[c].cpu().numpy(), want) <= 1e-11, c
        assert _rel(Pn[c].cpu().numpy(), meas(M.synthesis(want))) <= 1e-11, c


# ---- the samplers -----------------------------------------------------------------------------------------------------------
def _problem(wl=False, sig=0.1, C=1, L=16, N=1, spin=0, subclass=False):
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.measurements import Identity, WeakLensingHarmonic
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.transforms import SphericalWaveletTransform

    B, J_min = 2.0, 2
    rng = np.random.default_rng(L + N + wl)
    tr = SphericalWaveletTransform(L, B, J_min, dirs=N, spin=spin, harmonic=True, max_chains=C)
    if wl:
        ms = (type("WLSub", (WeakLensingHarmonic,), {}) if subclass else WeakLensingHarmonic)(L)
    else:
        ms = (type("IdSub", (Identity,), {}) if subclass else Identity)(L * L, L * L)
    data = _cplx(rng, L * L)
    data[:4] = 0
    lmda, mu = 2e-3, 1.0
    op = ForwardOperator(data, sig, "synthesis", transform=tr, measurement=ms, nparams=tr.ncoefs)
    reg = L1("synthesis", None, None, lmda * mu * 0.5)
    return op, reg, data, lmda, mu, rng


@pytest.mark.parametrize("wl", [False, True])
def test_myula_numpy_rng_matches_numpy_sampler(wl):
    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams

    L, C = 16, 2
    sig = np.linspace(0.08, 0.12, L * L)
    op, reg, data, lmda, mu, rng = _problem(wl, sig, C, L)
    delta = 5e-4
    p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, nsamples=4, nburn=2, ngap=2, verbosity=0)
    s = MYULA(op, reg, p, nchains=C, rng="numpy")
    X0 = _cplx(rng, op.nparams) * 0.1
    np.random.seed(3)
    _quiet(s.run, start_point=X0)
    assert s._fused_harm and s._eager_only and not s._fused_wav
    M = _model(L, 2.0, 2)
    oms = WeakLensingHarmonicOracle(L) if wl else ref.Identity(L * L, L * L)
    oop = ref.ForwardOperator(data, sig, "synthesis", HarmWavOracleTransform(M), oms, M.ncoefs)
    oreg = ref.L1("synthesis", None, None, lmda * mu * 0.5)
    np.random.seed(3)
    noise = np.stack([[np.random.randn(op.nparams) for _ in range(C)] for _ in range(s.niter)])
    for c in range(C):
        out = ref.myula_run(oop, oreg, lmda, delta, mu, 4, 2, 2, X0.astype(complex), lambda i: noise[i][c])
        assert np.abs(s.chain[c] - out["chain"]).max() < 1e-10 * np.abs(out["chain"]).max()
        np.testing.assert_allclose(s.logPi[c], out["logPi"].real, rtol=1e-9)


def _fused_vs_generic(wl, complex_, N, kact):
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams

    L, C = 16, 3
    runs = {}
    for name, subclass, use_graph in (("fused", False, True), ("fused_eager", False, False), ("generic", True, True)):
        op, reg, data, lmda, mu, rng = _problem(wl, np.linspace(0.08, 0.12, L * L), C, L, N=N, subclass=subclass)
        assert op.transform._plan.info()[2] == kact
        X0 = _cplx(rng, op.nparams) * 0.1
        p = PxMCMCParams(lmda=lmda, delta=5e-4, mu=mu, nsamples=5, nburn=9, ngap=10, verbosity=0, complex=complex_)
        s = MYULA(op, reg, p, nchains=C, seed=4, use_graph=use_graph)
        _quiet(s.run, start_point=X0)
        assert s._fused_harm == (not subclass) and not s._fused_wav
        assert s.niter == 50 and getattr(s, "used_graph", False) == use_graph, getattr(s, "graph_error", None)
        runs[name] = s
    f, e, g = runs["fused"], runs["fused_eager"], runs["generic"]
    np.testing.assert_array_equal(f.chain, e.chain)
    np.testing.assert_array_equal(f.logPi, e.logPi)
    assert np.abs(f.chain - g.chain).max() < 1e-10 * np.abs(g.chain).max()
    np.testing.assert_allclose(f.logPi, g.logPi, rtol=1e-9)
    assert np.isfinite(f.chain).all()


@pytest.mark.parametrize("wl", [False, True])
@pytest.mark.parametrize("complex_", [False, True])
def test_myula_fused_matches_generic_engine(wl, complex_):
    """the fused harmonic step and the generic engine (reached through a measurement subclass) on one Philox stream, 50
    iterations; and graph replay against eager stepping"""
    _fused_vs_generic(wl, complex_, 1, 2)


@pytest.mark.parametrize("wl", [False, True])
@pytest.mark.parametrize("complex_", [False, True])
@pytest.mark.parametrize("N,kact", [(2, 4), (5, 10), (9, 18)], ids=["N2-K5", "N5-K17", "N9-K0"])
def test_myula_fused_matches_generic_engine_dirs(wl, complex_, N, kact):
    """the same with dirs = N > 1: the samplers take the fused step for every N, and N selects the instantiation of its
    kernel through kact, the most items with a non-zero weight at one degree (K = 5, 17 and the re-reading K = 0)"""
    _fused_vs_generic(wl, complex_, N, kact)


def test_myula_gates():
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams
    from pxmcmc_amd.prior import L1

    p = PxMCMCParams(lmda=2e-3, delta=5e-4, nsamples=1, nburn=0, ngap=1, verbosity=0)
    op, reg, *_ = _problem()
    s = MYULA(op, reg, p)
    s._prepare()
    assert s._fused_harm and not s._fused_wav and op._wl_plan() is None
    s = MYULA(op, type("MyL1", (L1,), {"proxf": lambda self, X: L1.proxf(self, X)})("synthesis", None, None, 1e-3), p)
    s._prepare()
    assert not s._fused_harm
    op, reg, *_ = _problem(subclass=True)
    s = MYULA(op, reg, p)
    s._prepare()
    assert not s._fused_harm and not s._fused_wav


def test_pxmala_matches_numpy_sampler():
    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.mcmc import PxMALA, PxMCMCParams

    L, C = 16, 2
    op, reg, data, lmda, mu, rng = _problem(True, 0.1, C, L)
    N = op.nparams
    delta0 = 1e-5
    X0 = _cplx(rng, C, N) * 0.1
    p = PxMCMCParams(lmda=lmda, delta=delta0, mu=mu, nsamples=1, nburn=3, ngap=1, verbosity=0)
    s = PxMALA(op, reg, p, tune_delta=True, nchains=C, rng="numpy", max_iter=8)
    np.random.seed(21)
    _quiet(s.run, start_point=X0)
    niter = s.niter
    np.random.seed(21)
    nz, un = np.zeros((niter, C, N)), np.zeros((niter, C))
    for i in range(niter):
        for c in range(C):
            nz[i, c] = np.random.randn(N)
        for c in range(C):
            un[i, c] = np.random.rand()
    M = _model(L, 2.0, 2)
    oop = ref.ForwardOperator(data, 0.1, "synthesis", HarmWavOracleTransform(M), WeakLensingHarmonicOracle(L), N)
    oreg = ref.L1("synthesis", None, None, lmda * mu * 0.5)
    acc = np.asarray(s.acceptance_trace)
    for c in range(C):
        out = ref.pxmala_run(oop, oreg, lmda, delta0, mu, 10 ** 6, 3, 1, X0[c], lambda i: nz[i, c], lambda i: un[i, c],
                             tune=True, max_iter=niter)
        assert list(acc[:, c]) == list(out["acceptance_trace"])
        if len(out["chain"]):
            np.testing.assert_allclose(s.chain[c, 0], out["chain"][0], rtol=0, atol=1e-9 * np.abs(out["chain"][0]).max())


def test_skrock_and_analysis_setting_run_finite():
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import SKROCK, MYULA, PxMCMCParams
    from pxmcmc_amd.measurements import WeakLensingHarmonic
    from pxmcmc_amd.prior import L1

    C = 2
    op, reg, data, lmda, mu, rng = _problem(True, 0.1, C)
    X0 = _cplx(rng, op.nparams) * 0.1
    p = PxMCMCParams(lmda=lmda, delta=1e-3, mu=mu, s=3, nsamples=3, nburn=2, ngap=2, verbosity=0)
    k = SKROCK(op, reg, p, nchains=C)
    _quiet(k.run, start_point=X0)
    assert np.isfinite(k.chain).all() and np.isfinite(k.logPi).all()
    tr = op.transform
    aop = ForwardOperator(data, 0.1, "analysis", transform=tr, measurement=WeakLensingHarmonic(16), nparams=256)
    areg = L1("analysis", tr.inverse, tr.inverse_adjoint, lmda * mu * 0.5)
    p = PxMCMCParams(lmda=lmda, delta=5e-4, mu=mu, nsamples=3, nburn=2, ngap=2, verbosity=0)
    m = MYULA(aop, areg, p, nchains=C)
    _quiet(m.run, start_point=_cplx(rng, 256) * 0.1)
    assert not m._fused_harm and np.isfinite(m.chain).all() and np.isfinite(m.logPi).all()


def test_sks_estimate_on_device():
    import torch

    from pxmcmc_amd.measurements import WeakLensingHarmonic

    L = 32
    rng = np.random.default_rng(4)
    glm = _cplx(rng, 3, L * L)
    W, O = WeakLensingHarmonic(L), WeakLensingHarmonicOracle(L)
    got = W.sks_estimate(glm)
    assert isinstance(got, np.ndarray)
    for c in range(3):
        assert _rel(got[c], O.sks_estimate(glm[c])) < 1e-15
    t = W.harmonic_inverse_mapping(torch.as_tensor(glm[0]).cuda())
    assert isinstance(t, torch.Tensor) and _rel(t.cpu().numpy(), O.sks_estimate(glm[0])) < 1e-15


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError, lib

    L = 16
    plan = ops.HarmWavPlan(L, 2.0, 2, max_chains=2)
    x = torch.zeros((3, plan.ncoefs), dtype=torch.complex128, device="cuda")
    f = torch.zeros((3, L * L), dtype=torch.complex128, device="cuda")
    vp = ctypes.c_void_p
    assert lib.pxm_hwav_synthesis(plan._h, vp(x.data_ptr()), vp(f.data_ptr()), 3, None) < 0
    assert b"C outside" in lib.pxm_last_error()
    assert lib.pxm_hwav_analysis(plan._h, None, vp(x.data_ptr()), 1, None) < 0
    assert b"null" in lib.pxm_last_error()
    data = torch.zeros(L * L, dtype=torch.complex128, device="cuda")
    ic = torch.ones(L * L, dtype=torch.float64, device="cuda")
    rc = lib.pxm_hwav_myula_step(plan._h, vp(x.data_ptr()), vp(data.data_ptr()), vp(ic.data_ptr()), 0, None, None, 0.1, 1e-4,
                                 1e-3, 2, 0, 0, 0, None, vp(f.data_ptr()), vp(f.data_ptr()), 1, None)
    assert rc < 0 and b"mode must be 0 or 1" in lib.pxm_last_error()
    step = lambda X, out, C_: lib.pxm_hwav_myula_step(plan._h, vp(X.data_ptr()), vp(data.data_ptr()), vp(ic.data_ptr()), 0, None,
                                                      None, 0.1, 1e-4, 1e-3, 0, 0, 0, 0, None, vp(out.data_ptr()),
                                                      vp(f.data_ptr()), C_, None)
    y = torch.zeros_like(x)
    assert step(x, y, 3) < 0 and b"pxm_hwav_myula_step: C outside [1, max_chains]" in lib.pxm_last_error()
    assert step(x, x, 2) < 0 and b"X_out must not alias X" in lib.pxm_last_error()
    assert step(x, y, 2) == 0
    with pytest.raises(AssertionError, match="shape mismatch"):
        plan.myula_step(x, data, ic, None, 0.1, 1e-4, 1e-3)
    with pytest.raises(ValueError, match="more chains"):
        plan.synthesis(x)
    with pytest.raises(ValueError, match="distinct"):
        plan.myula_step(x[:1], data, ic, None, 0.1, 1e-4, 1e-3, out=x[:1])
    with pytest.raises(PxmError, match="spin != 0 needs N = 1"):
        ops.HarmWavPlan(L, 2.0, 2, 2, spin=1)


# ---- drop-in surface --------------------------------------------------------------------------------------------------------
def test_pys2let_shim_harmonic_functions():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import pys2let_shim as shim
    finally:
        sys.path.pop(0)
    L, B, J_min = 16, 2.0, 2
    rng = np.random.default_rng(12)
    for N, spin in ((1, 0), (3, 0), (1, 2)):
        M = _model(L, B, J_min, N, spin)
        flm = band_limited_flm(rng, L, spin)
        f_wav, f_scal = shim.analysis_lm2lmn(flm, B, L, J_min, N, spin)
        X = M.analysis(flm)
        assert _rel(np.concatenate((f_scal, f_wav)), X) < 1e-12
        assert _rel(shim.synthesis_lmn2lm(f_wav, f_scal, B, L, J_min, N, spin), M.synthesis(X)) < 1e-12
        a_wav, a_scal = shim.synthesis_adjoint_lm2lmn(flm, B, L, J_min, N, spin)
        assert _rel(np.concatenate((a_scal, a_wav)), M.synthesis_adjoint(flm)) < 1e-12
        assert _rel(shim.analysis_adjoint_lmn2lm(f_wav, f_scal, B, L, J_min, N, spin), M.analysis_adjoint(X)) < 1e-12


def test_weaklensing_example_harmonic(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "weaklensing_synthetic.py"), "--harmonic", "--L", "16",
           "--nsamples", "4", "--ngap", "5", "--nburn", "10", "--outdir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "harmonic" in r.stdout
