"""SKROCK on the GPU: the fused stage kernel (pxm_skrock_stage) against numpy, the sampler against the reference's s = 1
trajectory (G16) and against the numpy model of tests/test_skrock_host.py on the identity toy and on the wavelet, path
integral and weak-lensing operators, graph replay against eager stepping, chain sharding, and the stationary statistics
of the discrete chain at a step 25 times past MYULA's stability limit."""
import contextlib
import io

import numpy as np
import pytest

from conftest import golden
from test_skrock_host import model_run, model_step, stability_R

pytestmark = pytest.mark.gpu


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _toy(data, lmda, mu, setting="synthesis", sig_d=0.1):
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.transforms import IdentityTransform

    N = data.size
    op = ForwardOperator(data, sig_d, setting, IdentityTransform(), Identity(N, N), nparams=N)
    reg = L1(setting, op.transform.inverse, op.transform.inverse_adjoint, lmda * mu)
    return op, reg


def _soft(x, T):
    a = np.abs(x)
    return np.where(a > T, x / np.where(a > 0, a, 1) * (a - T), 0)


def _oracle_grad(oop, oreg, lmda):
    return lambda U: -(U - oreg.proxf(U)) / lmda - oop.calc_gradg(oop.forward(U))


def _host_draws(seed, n_iter, C, N, cplx=False):
    """the reference's np.random order: per iteration, per chain randn(N) [+ 1j randn(N)]"""
    rs = np.random.RandomState(seed)
    return np.array([[rs.randn(N) + (rs.randn(N) * 1j if cplx else 0) for _ in range(C)] for _ in range(n_iter)])


# ---- 1. the stage kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx_state", [False, True])
def test_stage_kernel_matches_numpy(cplx_state):
    import torch

    from pxmcmc_amd import ops

    C, n = 3, 1000
    rng = np.random.default_rng(1)
    rnd = (lambda: rng.normal(size=(C, n)) + 1j * rng.normal(size=(C, n))) if cplx_state else (lambda: rng.normal(size=(C, n)))
    U, P, G, V = rnd(), rnd(), rnd(), rnd()
    Tvec = np.abs(rng.normal(size=n))
    seed, chain0, it = 7, 5, 11
    coefs = {"stage0": (1.0, 0.0, 0.0, 0.0, 0.37), "stage1": (-0.8, 0.8, -1e-3, 1.0, 0.21), "stagej": (1.3, 0.5, -2e-3, -0.3, 0.0)}
    for noise_cplx in ([False, True] if cplx_state else [False]):
        for noise64 in (True, False):
            Zr = ops.randn(n, C, complex_=noise_cplx, seed=seed, chain0=chain0, it=it, noise64=noise64).cpu().numpy()
            Z = Zr if noise_cplx else Zr.real
            # Philox Z of the stage kernel, bit for bit (a = b = c = e = 0, r = 1)
            z = ops.skrock_stage(U, 0.0, r=1.0, noise_complex=noise_cplx, seed=seed, chain0=chain0, it=it, noise64=noise64)
            np.testing.assert_array_equal(z.cpu().numpy().real if cplx_state else z.cpu().numpy(), Z.real)
            if cplx_state:
                np.testing.assert_array_equal(z.cpu().numpy().imag, Z.imag if noise_cplx else 0.0)
            # the same through the device counter: it = 4 + *iter_dev (7)
            cnt = torch.full((1,), it - 4, dtype=torch.int64, device=ops.device())
            z2 = ops.skrock_stage(U, 0.0, r=1.0, noise_complex=noise_cplx, seed=seed, chain0=chain0, it=4, iter_dev=cnt,
                                  noise64=noise64)
            np.testing.assert_array_equal(z2.cpu().numpy(), z.cpu().numpy())
            for name, (a, b, c, e, r) in coefs.items():
                for prox in ("scalarT", "vectorT", "given"):
                    T = {"scalarT": 0.4, "vectorT": Tvec, "given": None}[prox]
                    Pm = P if prox == "given" else _soft(U, T)
                    kw = dict(b=b, c=c, e=e, r=r, T=T, proxf=P if prox == "given" else None,
                              gradg=G if c else None, V=V if e else None, noise_complex=noise_cplx, seed=seed,
                              chain0=chain0, it=it, noise64=noise64)
                    got = ops.skrock_stage(U, a, **kw).cpu().numpy()
                    terms = [a * U, b * Pm, c * G, e * V, r * Z]
                    want = sum(terms)
                    scale = sum(np.abs(t) for t in terms)
                    assert np.all(np.abs(got - want) <= 1e-14 * scale + 1e-300), (name, prox, noise_cplx, noise64)
                    # host-drawn noise (rng="numpy")
                    kw["noise"] = Z
                    got = ops.skrock_stage(U, a, **kw).cpu().numpy()
                    assert np.all(np.abs(got - want) <= 1e-14 * scale + 1e-300)
                    # out= buffer and a one-chain (1-D) call
                    out = torch.empty((C, n), dtype=torch.complex128 if cplx_state else torch.float64, device=ops.device())
                    ops.skrock_stage(U, a, out=out, **kw)
                    np.testing.assert_array_equal(out.cpu().numpy(), got)
                    kw1 = dict(kw, proxf=None if kw["proxf"] is None else P[1], gradg=None if kw["gradg"] is None else G[1],
                               V=None if kw["V"] is None else V[1], noise=Z[1])
                    np.testing.assert_array_equal(ops.skrock_stage(U[1], a, **kw1).cpu().numpy(), got[1])
    with pytest.raises(Exception):
        x = ops.as_device(U)
        ops.skrock_stage(x, 1.0, e=1.0, V=x, out=x)  # out aliases an input


# ---- 2. G16: the reference's s = 1 trajectory ----------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["real", "cplx"])
def test_g16_reference_trajectory(tag):
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams

    g = golden("g16_skrock.npz")
    lmda, delta, mu, nsamples, nburn, ngap = g["params"]
    op, reg = _toy(g["data"], lmda, mu)
    p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, s=1, nsamples=int(nsamples), nburn=int(nburn), ngap=int(ngap),
                     complex=tag == "cplx", verbosity=0, track=["logposterior", "L2", "prior", "chain", "predictions"])
    s = SKROCK(op, reg, p, rng="numpy")
    np.random.seed(int(g[f"{tag}_seed"]))
    _quiet(s.run, start_point=g[f"{tag}_X0"])
    np.testing.assert_allclose(s.chain, g[f"{tag}_chain"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(s.logPi, g[f"{tag}_logPi"], rtol=1e-10)
    np.testing.assert_allclose(s.L2s, g[f"{tag}_L2s"], rtol=1e-10)
    np.testing.assert_allclose(s.priors, g[f"{tag}_priors"], rtol=1e-10)
    np.testing.assert_allclose(s.preds, g[f"{tag}_preds"], rtol=1e-10, atol=1e-12)
    assert s.niter == int(nburn) + (int(nsamples) - 1) * int(ngap) + 1 and not s.used_graph


# ---- 3. s >= 2 against the numpy model on the identity toy -------------------------------------------------------------
@pytest.mark.parametrize("s_", [2, 5, 10])
@pytest.mark.parametrize("setting", ["synthesis", "analysis"])
@pytest.mark.parametrize("sig", ["scalar", "vector"])
def test_identity_toy_matches_model(s_, setting, sig):
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams

    N = 200
    rng = np.random.default_rng(s_)
    data = rng.normal(size=N)
    sig_d = 0.1 if sig == "scalar" else 0.1 * (1 + 0.5 * rng.random(N))
    invcov = 1 / np.asarray(sig_d) ** 2 * np.ones(N)
    lmda, mu = 2e-3, 1.0
    delta = s_ * s_ / 1500  # curvature <= 100 (data) + 1 / lmda (inside the threshold): l delta <= 0.4 s^2
    op, reg = _toy(data, lmda, mu, setting, sig_d)
    nsamples, nburn, ngap = 6, 3, 2
    p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, s=s_, nsamples=nsamples, nburn=nburn, ngap=ngap, verbosity=0,
                     track=["logposterior", "L2", "prior", "chain", "predictions"])
    sk = SKROCK(op, reg, p, rng="numpy")
    X0 = rng.normal(size=N) * 0.1
    np.random.seed(4)
    _quiet(sk.run, start_point=X0)
    rs = np.random.RandomState(4)
    out = model_run(X0, data, invcov, lmda, delta, mu, s_, nsamples, nburn, ngap, lambda i: rs.randn(N))
    sc = np.abs(out["chain"]).max()
    assert np.abs(sk.chain - out["chain"]).max() <= 1e-10 * sc
    np.testing.assert_allclose(sk.logPi, out["logPi"].real, rtol=1e-9)
    np.testing.assert_allclose(sk.priors, out["priors"], rtol=1e-10)
    assert np.abs(sk.preds - out["preds"]).max() <= 1e-10 * sc


@pytest.mark.parametrize("setting", ["analysis", "synthesis"])
@pytest.mark.parametrize("sig", ["scalar", "vector"])
def test_algorithm_runs_reference_smoke(setting, sig):
    """reference tests/test_mcmc.py at s = 5: run(), run(start_point), a wrong-size start raises; the chain is finite"""
    from oracle import ssht
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams

    L = 10
    rng = np.random.default_rng(0)
    flm = np.zeros(L * L, complex)
    for el in range(L):
        for m in range(el + 1):
            r = rng.random()
            flm[el * el + el - m] = (-1.0) ** m * r
            flm[el * el + el + m] = r
    data = ssht.inverse(flm, L).real.reshape(-1)
    n = data.size
    op, reg = _toy(data, 1.0, 1.0, setting, 0.1 if sig == "scalar" else np.full(n, 0.1))
    p = PxMCMCParams(nsamples=100, nburn=10, ngap=5, verbosity=0, s=5)
    _quiet(SKROCK(op, reg, p).run)
    s = SKROCK(op, reg, p)
    _quiet(s.run, data)
    assert s.chain.shape == (100, n) and np.isfinite(s.chain).all()
    with pytest.raises(Exception):
        _quiet(SKROCK(op, reg, p).run, data[:5])
    with pytest.raises(TypeError):
        _quiet(SKROCK(op, reg, p).run, list(data))


# ---- 4. operators: wavelet (L = 16 and L = 256), path integral, weak lensing ---------------------------------------
def test_wavelet_operator_matches_model_L16():
    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams
    from pxmcmc_amd.prior import S2_Wavelets_L1

    L, B, J_min, s_ = 16, 2, 2, 3
    P = L * (2 * L - 1)
    rng = np.random.default_rng(16)
    data = rng.normal(size=P)
    lmda, delta, mu = 1e-3, 2e-3, 2.0
    op = SphericalWaveletTransformOperator(data, 0.05, "synthesis", L, B, J_min)
    reg = S2_Wavelets_L1("synthesis", op.transform.inverse, op.transform.inverse_adjoint, lmda * mu, L=L, B=B, J_min=J_min)
    p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, s=s_, nsamples=4, nburn=1, ngap=2, verbosity=0)
    sk = SKROCK(op, reg, p, rng="numpy")
    N = op.nparams
    X0 = rng.normal(size=N) * 0.1
    np.random.seed(8)
    _quiet(sk.run, start_point=X0)
    T = ref.SphericalWaveletTransform(L, B, J_min)
    oop = ref.ForwardOperator(data, 0.05, "synthesis", T, ref.Identity(P, P), T.ncoefs)
    oreg = ref.S2_Wavelets_L1("synthesis", None, None, lmda * mu, L, B, J_min)
    grad = _oracle_grad(oop, oreg, lmda)
    rs = np.random.RandomState(8)
    X = X0.astype(complex)
    saved = []
    for i in range(1 + 3 * 2 + 1):
        X = model_step(X, rs.randn(N), s_, delta, grad)
        if i >= 1 and (i - 1) % 2 == 0:
            saved.append(X)
    np.testing.assert_allclose(sk.chain, np.array(saved).real, rtol=1e-10, atol=1e-10 * np.abs(saved).max())
    np.testing.assert_allclose(sk.X_curr[0].cpu().numpy(), X, rtol=1e-10, atol=1e-10 * np.abs(X).max())


def _bandlimited_real_field(L, seed):
    from oracle import ssht

    rng = np.random.default_rng(seed)
    flm = np.zeros(L * L, dtype=complex)
    for el in range(L):
        amp = 1.0 / (1.0 + el)
        flm[el * el + el] = amp * rng.normal()
        m = np.arange(1, el + 1)
        v = amp * (rng.normal(size=el) + 1j * rng.normal(size=el)) / np.sqrt(2)
        flm[el * el + el + m] = v
        flm[el * el + el - m] = (-1.0) ** m * np.conj(v)
    f = ssht.inverse(flm, L, 0).real.reshape(-1)
    return f / np.sqrt(np.mean(f**2)), rng


def test_wavelet_operator_matches_model_L256_16chains():
    """BASELINE configs[2] size: L = 256, B = 2, J_min = 2, 16 chains, s = 2, three iterations on the reference's noise
    stream, against the model over the oracle for chains 0 and 15"""
    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams
    from pxmcmc_amd.prior import S2_Wavelets_L1

    L, B, J_min, C, s_, K = 256, 2, 2, 16, 2, 3
    P = L * (2 * L - 1)
    truth, rng = _bandlimited_real_field(L, seed=2)
    sig = 0.05
    data = truth + sig * rng.normal(size=P)
    lmda, delta, mu = 1e-6, 4e-7, 1.0
    op = SphericalWaveletTransformOperator(data, sig, "synthesis", L, B, J_min, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, lmda * mu, L=L, B=B, J_min=J_min)
    N = op.nparams
    X0 = rng.normal(size=(C, N)) * 1e-3
    p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, s=s_, nsamples=1, nburn=K - 1, ngap=1, verbosity=0, track=["chain"])
    sk = SKROCK(op, reg, p, nchains=C, rng="numpy")
    np.random.seed(21)
    _quiet(sk.run, start_point=X0)
    Xk = sk.X_curr.cpu().numpy()
    noise = _host_draws(21, K, C, N)
    T = ref.SphericalWaveletTransform(L, B, J_min)
    oop = ref.ForwardOperator(data, sig, "synthesis", T, ref.Identity(P, P), T.ncoefs)
    oreg = ref.S2_Wavelets_L1("synthesis", None, None, lmda * mu, L, B, J_min)
    grad = _oracle_grad(oop, oreg, lmda)
    for c in (0, 15):
        X = X0[c].astype(complex)
        for i in range(K):
            X = model_step(X, noise[i][c], s_, delta, grad)
        assert np.abs(Xk[c] - X).max() <= 1e-11 * np.abs(X).max()


def test_pathintegral_and_weaklensing_match_model():
    import scipy.sparse as sp
    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.forward import ForwardOperator, PathIntegralOperator
    from pxmcmc_amd.measurements import WeakLensing
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams
    from pxmcmc_amd.prior import S2_Wavelets_L1
    from pxmcmc_amd.transforms import SphericalWaveletTransform

    L, B, J_min, s_ = 10, 2, 2, 3
    P = L * (2 * L - 1)
    rng = np.random.default_rng(3)
    T = ref.SphericalWaveletTransform(L, B, J_min)
    lmda, delta, mu = 1e-3, 1e-3, 1.5
    # path integral (experiments/phasevel in miniature)
    A = sp.random(60, P, density=0.1, random_state=np.random.RandomState(2), format="csr")
    data = rng.normal(size=60)
    op = PathIntegralOperator(A, data, 0.2, "synthesis", L, B, J_min)
    oop = ref.ForwardOperator(data, 0.2, "synthesis", T, ref.PathIntegral(A), op.nparams)
    cases = [(op, oop, False)]
    # weak lensing (experiments/weaklensing in miniature): complex data
    wl = WeakLensing(L)
    tr = SphericalWaveletTransform(L, B, J_min)
    wdata = rng.normal(size=wl.ndata) + 1j * rng.normal(size=wl.ndata)
    wop = ForwardOperator(wdata, 0.3, "synthesis", transform=tr, measurement=wl, nparams=tr.ncoefs)
    woop = ref.ForwardOperator(wdata, 0.3, "synthesis", T, ref.WeakLensing(L), T.ncoefs)
    cases.append((wop, woop, True))
    for fop, foop, cplx in cases:
        reg = S2_Wavelets_L1("synthesis", None, None, lmda * mu, L=L, B=B, J_min=J_min)
        oreg = ref.S2_Wavelets_L1("synthesis", None, None, lmda * mu, L, B, J_min)
        n = fop.nparams
        p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, s=s_, nsamples=3, nburn=1, ngap=1, verbosity=0, complex=cplx)
        sk = SKROCK(fop, reg, p, rng="numpy")
        X0 = rng.normal(size=n) * 0.1 + (1j * rng.normal(size=n) * 0.1 if cplx else 0)
        np.random.seed(9)
        _quiet(sk.run, start_point=X0)
        noise = _host_draws(9, 4, 1, n, cplx)
        grad = _oracle_grad(foop, oreg, lmda)
        X = X0.astype(complex)
        saved = []
        for i in range(4):
            X = model_step(X, noise[i][0], s_, delta, grad)
            if i >= 1:
                saved.append(X)
        saved = np.array(saved) if cplx else np.array(saved).real
        np.testing.assert_allclose(sk.chain, saved, rtol=1e-10, atol=1e-10 * np.abs(saved).max())


# ---- 5. graph replay equals eager stepping; 6. sharding ------------------------------------------------------------
def _wavelet_problem(C, L=16):
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.prior import S2_Wavelets_L1

    B, J_min = 2, 2
    rng = np.random.default_rng(5)
    data = rng.normal(size=L * (2 * L - 1))
    lmda, mu = 1e-3, 1.0
    op = SphericalWaveletTransformOperator(data, 0.05, "synthesis", L, B, J_min, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, lmda * mu, L=L, B=B, J_min=J_min)
    return op, reg, lmda, mu, rng.normal(size=op.nparams) * 0.1


def test_graph_replay_equals_eager():
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams

    C = 3
    wop, wreg, lmda, mu, wX0 = _wavelet_problem(C)
    rng = np.random.default_rng(6)
    tdata = rng.normal(size=300)
    top, treg = _toy(tdata, lmda, mu, "analysis")  # generic prox path (proxf array)
    for op, reg, X0, s_ in ((wop, wreg, wX0, 4), (top, treg, rng.normal(size=300) * 0.1, 3)):
        runs = []
        for use_graph in (True, False):
            p = PxMCMCParams(lmda=lmda, delta=1e-3, mu=mu, s=s_, nsamples=4, nburn=5, ngap=7, verbosity=0,
                             track=["chain", "logposterior", "predictions"])
            sk = SKROCK(op, reg, p, nchains=C, seed=12, use_graph=use_graph)
            _quiet(sk.run, start_point=X0)
            assert sk.used_graph == use_graph, getattr(sk, "graph_error", None)
            runs.append(sk)
        np.testing.assert_array_equal(runs[0].chain, runs[1].chain)
        np.testing.assert_array_equal(runs[0].logPi, runs[1].logPi)
        np.testing.assert_array_equal(runs[0].preds, runs[1].preds)
        np.testing.assert_array_equal(runs[0].X_curr.cpu().numpy(), runs[1].X_curr.cpu().numpy())
        assert np.isfinite(runs[0].chain).all()


def test_chain_sharding():
    """chain c of a C-chain run equals a one-chain run with chain_offset = c: bit for bit on the identity toy (every
    operation elementwise), to rounding on the wavelet operator (its transforms tile the chain batch differently)"""
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams

    C = 4
    wop, wreg, lmda, mu, wX0 = _wavelet_problem(C)
    rng = np.random.default_rng(8)
    top, treg = _toy(rng.normal(size=100), lmda, mu)
    for op, reg, X0, cplx, exact in ((top, treg, rng.normal(size=100) * 0.1, False, True), (wop, wreg, wX0, True, False)):
        p = PxMCMCParams(lmda=lmda, delta=1e-3, mu=mu, s=3, nsamples=2, nburn=3, ngap=2, verbosity=0, complex=cplx,
                         track=["chain"])
        full = SKROCK(op, reg, p, nchains=C, seed=4)
        _quiet(full.run, start_point=X0)
        for c in (0, 3):
            one = SKROCK(op, reg, p, nchains=1, seed=4, chain_offset=c)
            _quiet(one.run, start_point=X0)
            if exact:
                np.testing.assert_array_equal(one.chain, full.chain[c])
            else:
                np.testing.assert_allclose(one.chain, full.chain[c], rtol=1e-12, atol=1e-14)
        assert np.abs(full.chain[0] - full.chain[1]).max() > 1e-6


def test_chain_step_public_and_subclass():
    """chain_step(X) as the reference exposes it; a subclass overriding it steps eagerly through it"""
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams

    N = 50
    rng = np.random.default_rng(2)
    data = rng.normal(size=N)
    op, reg = _toy(data, 2e-3, 1.0)
    p = PxMCMCParams(lmda=2e-3, delta=5e-3, mu=1.0, s=4, nsamples=3, nburn=0, ngap=1, verbosity=0)
    sk = SKROCK(op, reg, p, rng="numpy")
    X = rng.normal(size=N)
    np.random.seed(3)
    got = sk.chain_step(X)
    assert isinstance(got, np.ndarray) and got.shape == (N,)
    rs = np.random.RandomState(3)
    want = model_step(X, rs.randn(N), 4, 5e-3, lambda U: -(U - _soft(U, 2e-3)) / 2e-3 - 100 * (U - data))
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-12)

    calls = []

    class Mine(SKROCK):
        def chain_step(self, X):
            calls.append(1)
            return super().chain_step(X)

    m = Mine(op, reg, p)
    _quiet(m.run, start_point=X)
    assert len(calls) == 3 and not m.used_graph and np.isfinite(m.chain).all()


# ---- 7. statistics ------------------------------------------------------------------------------------------------------
def test_gaussian_stationary_variance_of_the_discrete_chain():
    """T = 0 (Gaussian target, sigma = 0.1): N = 64 coordinates, C = 4096 chains, s = 10, l delta = 50 -- 25 times
    MYULA's stability limit of 2.  The chain X' = R X + Q Z + (1 - R) d has the stationary variance Q^2 / (1 - R^2)."""
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams

    N, C, sigma, s_ = 64, 4096, 0.1, 10
    ell = 1 / sigma**2
    delta = 50 / ell
    rng = np.random.default_rng(7)
    d = rng.normal(size=N)
    op, reg = _toy(d, 1.0, 0.0, sig_d=sigma)  # mu = 0: threshold 0, the prox term vanishes
    p = PxMCMCParams(lmda=1.0, delta=delta, mu=0.0, s=s_, nsamples=1, nburn=50, ngap=1, verbosity=0, track=["chain"])
    sk = SKROCK(op, reg, p, nchains=C, seed=31)
    _quiet(sk.run, start_point=np.zeros(N))
    assert sk.used_graph
    X = sk.X_curr.cpu().numpy().real
    R = stability_R(s_, ell * delta)
    Q = model_step(np.zeros(1), np.ones(1), s_, delta, lambda U: -ell * U)[0]
    var = Q**2 / (1 - R**2)
    assert abs(R) < 1 and -0.4 < R < -0.25 and 0.006 < var < 0.008, (R, var)
    se = np.sqrt(var / C)
    assert np.abs(X.mean(axis=0) - d).max() < 5 * se
    ratio = X.var(axis=0) / var
    assert abs(ratio.mean() - 1) < 0.01, ratio.mean()
    assert np.abs(ratio - 1).max() < 0.10, ratio


def test_philox_l1_toy_stationary_moments():
    """the identity toy with an L1 prior at s = 5: the ensemble of 4096 chains after burn-in against the numpy model run
    on the same problem with its own noise (the two ensembles sample the same discrete chain)"""
    from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams

    N, C, s_ = 64, 4096, 5
    rng = np.random.default_rng(5)
    d = rng.normal(size=N) * 0.3
    d[:8] = np.linspace(-0.02, 0.02, 8)
    sigma, lmda, mu = 0.1, 2e-3, 20.0
    delta = 0.02  # l delta = 2 on the data term (MYULA's limit), 12 inside the threshold (1 / lmda): stable at s = 5
    op, reg = _toy(d, lmda, mu)
    nburn = 100
    p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, s=s_, nsamples=1, nburn=nburn, ngap=1, verbosity=0, track=["chain"])
    sk = SKROCK(op, reg, p, nchains=C, seed=17)
    _quiet(sk.run, start_point=np.zeros(N))
    X = sk.X_curr.cpu().numpy().real
    rs = np.random.default_rng(99)
    grad = lambda U: -(U - _soft(U, lmda * mu)) / lmda - (U - d) / sigma**2
    Y = np.zeros((C, N))
    for _ in range(nburn + 1):
        Y = model_step(Y, rs.normal(size=(C, N)), s_, delta, grad)
    se = np.sqrt((X.var(axis=0) + Y.var(axis=0)) / C)
    assert np.abs(X.mean(axis=0) - Y.mean(axis=0)).max() < 5 * se.max()
    ratio = X.var(axis=0) / Y.var(axis=0)
    assert abs(ratio.mean() - 1) < 0.02, ratio.mean()  # ~0.4 % pooled statistical error (two ensembles)
    assert np.abs(ratio - 1).max() < 0.2, ratio
