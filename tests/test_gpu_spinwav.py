"""Spin wavelets (spin s != 0, dirs = 1) on the GPU: the four WavPlan operators at spin s against the numpy model of
tests/test_spinwav_host.py, the analysis-setting prox, the spin-0 plan through the spin-taking creator, the fused MYULA
steps at spin 2 against the numpy sampler, graph replay, PxMALA / SKROCK and the refusals of a spin-s plan
(DESIGN.md section 12)."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

from test_spinwav_host import SpinWavModel, spin_bandlimited_image

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _cplx(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _four_ops(L, B, J_min, spin, C, tol, rows=None):
    from pxmcmc_amd import ops

    rng = np.random.default_rng(100 * L + 10 * C + spin + 7)
    plan = ops.WavPlan(L, B, J_min, max_chains=C, spin=spin)
    M = SpinWavModel(L, B, J_min, spin)
    assert (plan.ncoefs, plan.nscal, plan.spin) == (M.ncoefs, M.nscal, spin)
    # dense complex inputs: the images carry harmonics below |s| too (every operator must drop them alike)
    X = _cplx(rng, C, M.ncoefs)
    f = _cplx(rng, C, L * (2 * L - 1))
    rows = list(range(C)) if rows is None else rows
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        got = getattr(plan, name)(arg).cpu().numpy()
        ref = np.stack([getattr(M, name)(arg[c]) for c in rows])
        err = _rel(got[rows], ref)
        assert err < tol, (name, L, spin, C, err)
    return plan, M


@pytest.mark.parametrize("spin", [1, 2, -2, 3])
@pytest.mark.parametrize("L", [16, 33, 64])
def test_spin_wavplan_matches_model(L, spin):
    _four_ops(L, 2.0, 2, spin, 3, 1e-11)


def test_spin2_wavplan_L256_16_chains():
    plan, M = _four_ops(256, 2.0, 2, 2, 16, 1e-11, rows=[0, 9, 15])
    # every per-scale stage is the spin-0 one; only the L-level tables are stored for all m
    from pxmcmc_amd import ops

    p0 = ops.WavPlan(256, 2.0, 2, max_chains=16)
    assert plan.table_bytes(0) > p0.table_bytes(0) and plan.table_bytes(1) > p0.table_bytes(1)


def test_spin_round_trip_on_device():
    """synthesis o analysis = identity on band-limited spin-s images, with the plan alone"""
    from pxmcmc_amd import ops

    L, spin = 33, -2
    rng = np.random.default_rng(3)
    plan = ops.WavPlan(L, 2.0, 2, max_chains=2, spin=spin)
    f = np.stack([spin_bandlimited_image(rng, L, spin) for _ in range(2)])
    back = plan.synthesis(plan.analysis(f)).cpu().numpy()
    assert _rel(back, f) < 1e-12


def test_spin_analysis_setting_prox():
    """the analysis-setting L1 prox x + analysis_adjoint(soft(analysis x) - analysis x) at spin 2"""
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.transforms import SphericalWaveletTransform
    from pxmcmc_amd.utils import soft

    L, B, J_min, spin, C = 16, 2.0, 2, 2, 2
    rng = np.random.default_rng(11)
    tr = SphericalWaveletTransform(L, B, J_min, spin=spin, max_chains=C)
    M = SpinWavModel(L, B, J_min, spin)
    reg = L1("analysis", tr.forward_adjoint, tr.forward, 0.05)
    x = np.stack([spin_bandlimited_image(rng, L, spin) for _ in range(C)])
    got = reg.proxf(x)
    for c in range(C):
        a = M.analysis(x[c])
        want = x[c] + M.analysis_adjoint(soft(a, 0.05) - a)
        assert _rel(got[c], want) < 1e-11


def test_spin0_creator_is_bit_identical():
    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import lib

    L, B, J_min, C = 64, 2.0, 2, 3

    class OldWavPlan(ops.WavPlan):
        def __init__(self):
            ops.require_gpu()
            self.L, self.B, self.J_min, self.max_chains, self.spin = L, B, J_min, C, 0
            self.npix = L * (2 * L - 1)
            nscal = ctypes.c_int64()
            self.ncoefs = int(ops.check(lib.pxm_wav_ncoefs(L, B, J_min, ctypes.byref(nscal))))
            self.nscal = int(nscal.value)
            ops._Plan.__init__(self, lib.pxm_wav_plan_create, (L, B, J_min, C, 0), lib.pxm_wav_plan_destroy,
                               lib.pxm_wav_status, "old")

    rng = np.random.default_rng(2)
    new, old = ops.WavPlan(L, B, J_min, max_chains=C, spin=0), OldWavPlan()
    X, f = _cplx(rng, C, new.ncoefs), _cplx(rng, C, new.npix)
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        a, b = getattr(new, name)(arg).cpu().numpy(), getattr(old, name)(arg).cpu().numpy()
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("spin", [2, -3])
def test_spin_fused_steps_match_model(spin):
    """one MYULA update of each fused step (gradg_step, image_step, ring_step) with injected complex noise:
    X' = (1 - d/l) X + (d/l) soft(X, T) - d S^H (w (S X - data)) + sqrt(2 d) W"""
    import torch

    from oracle import pxmcmc_np as ref
    from pxmcmc_amd import ops

    L, B, J_min, C = 33, 2.0, 2, 3
    rng = np.random.default_rng(50 + spin)
    plan = ops.WavPlan(L, B, J_min, max_chains=C, spin=spin)
    M = SpinWavModel(L, B, J_min, spin)
    P = L * (2 * L - 1)
    X = _cplx(rng, C, M.ncoefs) * 0.1
    data = spin_bandlimited_image(rng, L, spin)
    W = _cplx(rng, C, M.ncoefs)
    T = np.abs(rng.normal(size=M.ncoefs)) * 0.05
    delta, lmda, w = 1e-3, 2e-3, complex(3.0, 1.5)
    T_dev = torch.as_tensor(T, device="cuda")
    d_dev = torch.as_tensor(data, device="cuda")
    ic_vec = np.linspace(2.0, 4.0, P) + 0.5j
    want = {}
    for name, ic in (("uniform", np.full(P, w)), ("vector", ic_vec)):
        rows = []
        for c in range(C):
            g = M.synthesis_adjoint(ic * (M.synthesis(X[c]) - data))
            rows.append(ref.chain_step(X[c], ref.soft(X[c], T), g, delta, lmda, W[c]))
        want[name] = np.stack(rows)
    preds = plan.synthesis(X)
    ic_dev = torch.as_tensor(ic_vec, device="cuda")
    got = plan.gradg_step(X, preds, d_dev, ic_dev, T_dev, delta, lmda, noise=W, noise_complex=True).cpu().numpy()
    assert _rel(got, want["vector"]) < 1e-11, "gradg_step"
    plan.image_init(preds, d_dev, ic_dev)
    Xn, Pn = plan.image_step(X, d_dev, ic_dev, T_dev, delta, lmda, noise=W, noise_complex=True)
    assert _rel(Xn.cpu().numpy(), want["vector"]) < 1e-11, "image_step"
    assert _rel(Pn.cpu().numpy(), np.stack([M.synthesis(x) for x in want["vector"]])) < 1e-11, "image_step preds"
    plan.ring_set_data(d_dev)
    plan.ring_init(X)
    Xr = plan.ring_step(X, w, T_dev, delta, lmda, noise=W, noise_complex=True)
    assert _rel(Xr.cpu().numpy(), want["uniform"]) < 1e-11, "ring_step"
    Pr = plan.ring_preds(C).cpu().numpy()
    assert _rel(Pr, np.stack([M.synthesis(x) for x in want["uniform"]])) < 1e-11, "ring_preds"


# ---- samplers ---------------------------------------------------------------------------------------------------------------
def _spin_problem(sig_d=0.1, C=1, spin=2, seed=5):
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.prior import S2_Wavelets_L1

    L, B, J_min = 16, 2, 2
    rng = np.random.default_rng(seed)
    data = spin_bandlimited_image(rng, L, spin)
    lmda, mu = 1e-3, 1.0
    op = SphericalWaveletTransformOperator(data, sig_d, "synthesis", L, B, J_min, spin=spin, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", op.transform.inverse, op.transform.inverse_adjoint, lmda * mu, L=L, B=B, J_min=J_min,
                         spin=spin)
    return op, reg, data, lmda, mu, rng


@pytest.mark.parametrize("vector_sig", [False, True])
def test_myula_spin2_fused_matches_numpy_model(vector_sig):
    """scalar sig_d: the ring-space step (pxm_wav_ring_step); vector sig_d: the image step (pxm_wav_image_step)"""
    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams

    L, B, J_min, spin = 16, 2.0, 2, 2
    P = L * (2 * L - 1)
    sig = np.linspace(0.08, 0.12, P) if vector_sig else 0.1
    op, reg, data, lmda, mu, rng = _spin_problem(sig)
    delta = 5e-4
    p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, nsamples=4, nburn=2, ngap=2, verbosity=0, complex=True)
    s = MYULA(op, reg, p, rng="numpy")
    X0 = _cplx(rng, op.nparams) * 0.1
    np.random.seed(3)
    _quiet(s.run, start_point=X0)
    assert s._fused_wav and not s._pairs
    M = SpinWavModel(L, B, J_min, spin)

    class _T:
        inverse = staticmethod(M.synthesis)
        inverse_adjoint = staticmethod(M.synthesis_adjoint)

    oop = ref.ForwardOperator(data, sig, "synthesis", _T, ref.Identity(P, P), M.ncoefs)
    oreg = ref.L1("synthesis", None, None, lmda * mu * reg.map_weights)
    oreg.prior = lambda X: np.sum(np.abs(reg.map_weights * X))
    np.random.seed(3)
    noise = [np.random.randn(op.nparams) + 1j * np.random.randn(op.nparams) for _ in range(s.niter)]
    out = ref.myula_run(oop, oreg, lmda, delta, mu, 4, 2, 2, X0, lambda i: noise[i], cplx=True)
    scale = np.abs(out["chain"]).max()
    assert np.abs(s.chain - out["chain"]).max() < 1e-9 * scale
    np.testing.assert_allclose(s.logPi, out["logPi"].real, rtol=1e-9)


@pytest.mark.parametrize("vector_sig", [False, True])
def test_myula_spin2_graph_equals_eager(vector_sig):
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams

    C = 3
    P = 16 * 31
    op, reg, data, lmda, mu, rng = _spin_problem(np.linspace(0.08, 0.12, P) if vector_sig else 0.1, C)
    X0 = _cplx(rng, op.nparams) * 0.1
    runs = []
    for use_graph in (True, False):
        p = PxMCMCParams(lmda=lmda, delta=5e-4, mu=mu, nsamples=3, nburn=4, ngap=5, verbosity=0, complex=True)
        s = MYULA(op, reg, p, nchains=C, seed=4, use_graph=use_graph)
        _quiet(s.run, start_point=X0)
        assert s._fused_wav and not s._pairs
        assert getattr(s, "used_graph", False) == use_graph, getattr(s, "graph_error", None)
        runs.append(s)
    np.testing.assert_array_equal(runs[0].chain, runs[1].chain)
    np.testing.assert_array_equal(runs[0].logPi, runs[1].logPi)
    assert np.isfinite(runs[0].chain).all()


def test_myula_spin2_real_start_takes_no_pair_mode():
    """real data values are impossible for a spin-s map, but a real start point with params.complex False must still
    not select the two-real-chains-per-slot mode"""
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams

    C = 2
    op, reg, data, lmda, mu, rng = _spin_problem(0.1, C)
    p = PxMCMCParams(lmda=lmda, delta=5e-4, mu=mu, nsamples=2, nburn=0, ngap=1, verbosity=0)
    s = MYULA(op, reg, p, nchains=C, seed=2)
    _quiet(s.run, start_point=rng.normal(size=op.nparams) * 0.1)
    assert s._fused_wav and not s._pairs
    assert np.isfinite(s.chain).all()


def test_pxmala_and_skrock_spin2_run_finite():
    from pxmcmc_amd.mcmc import SKROCK, PxMALA, PxMCMCParams

    C = 2
    op, reg, data, lmda, mu, rng = _spin_problem(0.1, C)
    X0 = _cplx(rng, op.nparams) * 0.1
    p = PxMCMCParams(lmda=lmda, delta=1e-4, mu=mu, nsamples=3, nburn=2, ngap=2, verbosity=0, complex=True)
    m = PxMALA(op, reg, p, nchains=C, tune_delta=True)
    _quiet(m.run, start_point=X0)
    assert np.isfinite(m.chain).all() and np.isfinite(m.logPi).all()
    p = PxMCMCParams(lmda=lmda, delta=1e-3, mu=mu, s=3, nsamples=3, nburn=2, ngap=2, verbosity=0, complex=True)
    k = SKROCK(op, reg, p, nchains=C)
    _quiet(k.run, start_point=X0)
    assert np.isfinite(k.chain).all() and np.isfinite(k.logPi).all()


def test_spin_plan_refusals():
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError

    L = 16
    plan = ops.WavPlan(L, 2.0, 2, max_chains=2, spin=2)
    with pytest.raises(PxmError, match="spin"):
        plan.wl_attach(None, None, plan.npix)
    x = torch.zeros((1, plan.ncoefs), dtype=torch.complex128, device="cuda")
    preds = torch.zeros((1, plan.npix), dtype=torch.complex128, device="cuda")
    data = torch.zeros(plan.npix, dtype=torch.complex128, device="cuda")
    ic = torch.ones(plan.npix, dtype=torch.float64, device="cuda")
    with pytest.raises(PxmError, match="spin-0 plan"):
        plan.gradg_step(x, preds, data, ic, 0.01, 1e-4, 1e-3, pairs=True)
    plan.ring_set_data(data)
    plan.ring_init(x)
    with pytest.raises(PxmError, match="spin-0 plan"):
        plan.ring_step(x, 1.0, 0.01, 1e-4, 1e-3, pairs=True)
    # the same calls in the complex layout are accepted
    out = plan.gradg_step(x, preds, data, ic, 0.01, 1e-4, 1e-3)
    assert torch.isfinite(torch.view_as_real(out)).all()


# ---- examples ---------------------------------------------------------------------------------------------------------------
def test_pys2let_shim_passes_spin_through():
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    try:
        import pys2let_shim as shim
    finally:
        sys.path.pop(0)
    L, B, J_min, spin = 16, 2.0, 2, 2
    rng = np.random.default_rng(8)
    M = SpinWavModel(L, B, J_min, spin)
    f = spin_bandlimited_image(rng, L, spin)
    f_wav, f_scal = shim.analysis_px2wav(f, B, L, J_min, 1, spin)
    X = M.analysis(f)
    assert _rel(np.concatenate((f_scal, f_wav)), X) < 1e-11
    assert _rel(shim.synthesis_wav2px(f_wav, f_scal, B, L, J_min, 1, spin), f) < 1e-11
    with pytest.raises(NotImplementedError):
        shim.analysis_px2wav(f, B, L, J_min, 2, spin)


def test_topography_example_spin2(tmp_path):
    import os
    import runpy

    from pxmcmc_amd.saving import load_mcmc

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mod = runpy.run_path(os.path.join(root, "examples", "topography_synthetic.py"))
    path, rel, ci = _quiet(mod["main"], ["--L", "16", "--nsamples", "8", "--ngap", "50", "--chains", "2", "--spin", "2",
                                         "--outdir", str(tmp_path)])
    data, attrs = load_mcmc(path)
    assert data["chain"].shape[:2] == (2, 8) and attrs["spin"] == 2 and attrs["complex"]
    assert np.iscomplexobj(data["chain"]) and np.isfinite(data["logposterior"]).all() and (ci >= 0).all()
    assert rel < 1.0
