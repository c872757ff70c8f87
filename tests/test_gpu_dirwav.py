"""Directional wavelets (dirs = N > 1) on the GPU: the odd-spin SHT plans they are built on, the four DirWavPlan
operators against the numpy model of tests/test_dirwav_host.py, operator properties, and the samplers on a directional
wavelet operator."""
import contextlib
import io

import numpy as np
import pytest

from test_dirwav_host import OTHER_TILINGS, DirWavModel, bandlimited_image

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _cplx(rng, *shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


# ---- odd spins of the SHT plan ------------------------------------------------------------------------------------------
def _sht_four_ops(L, spin, C, tol, rows=None):
    from oracle import ssht
    from pxmcmc_amd import ops

    rng = np.random.default_rng(1000 * L + 10 * C + spin + 3)
    plan = ops.ShtPlan(L, spin, max_chains=C)
    flm = _cplx(rng, C, L * L)
    flm[:, : spin * spin] = 0
    f = _cplx(rng, C, L * (2 * L - 1))
    T = ssht.get_transform(L, spin)
    rows = range(C) if rows is None else rows
    for name, arg, fn in (
        ("inverse", flm, lambda x: T.inverse(x).ravel()),
        ("forward_adjoint", flm, lambda x: T.forward_adjoint(x).ravel()),
        ("forward", f, T.forward),
        ("inverse_adjoint", f, T.inverse_adjoint),
    ):
        got = getattr(plan, name)(arg).cpu().numpy()
        ref = np.stack([fn(arg[c]) for c in rows])
        assert _rel(got[list(rows)], ref) < tol, (name, L, spin, C, _rel(got[list(rows)], ref))
    return plan


@pytest.mark.parametrize("L", [4, 9, 16, 33])
@pytest.mark.parametrize("spin", [1, -1, 3, -3])
def test_sht_odd_spins_small(L, spin):
    _sht_four_ops(L, spin, 3, 1e-12)


@pytest.mark.parametrize("spin", [1, -1, 3, -3])
@pytest.mark.parametrize("C", [1, 16])
def test_sht_odd_spins_L256(spin, C):
    """1 chain: the table-free recursion path where the plan takes it; 16 chains: the ring-table GEMM"""
    plan = _sht_four_ops(256, spin, C, 1e-11, rows=None if C == 1 else [0, 7, 15])
    if C == 16:
        assert plan.uses_recursion() == 0


# ---- N = 1: the directional plan computes what WavPlan computes -----------------------------------------------------------
@pytest.mark.parametrize("L", [16, 64, 256])
def test_dirwav_n1_equals_wavplan(L):
    from pxmcmc_amd import ops

    B, J_min, C = 2.0, 2, 2
    rng = np.random.default_rng(L)
    w = ops.WavPlan(L, B, J_min, max_chains=C)
    d = ops.DirWavPlan(L, B, J_min, 1, max_chains=C)
    assert (d.ncoefs, d.nscal) == (w.ncoefs, w.nscal)
    X = _cplx(rng, C, w.ncoefs)
    f = _cplx(rng, C, w.npix)
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        a = getattr(d, name)(arg).cpu().numpy()
        b = getattr(w, name)(arg).cpu().numpy()
        assert _rel(a, b) < 1e-12, (name, _rel(a, b))


# ---- the four operators against the numpy model ------------------------------------------------------------------------
def _four_ops_vs_model(L, B, J_min, N, C, rows, tol):
    from pxmcmc_amd import ops

    rng = np.random.default_rng(7 * L + N)
    M = DirWavModel(L, B, J_min, N)
    plan = ops.DirWavPlan(L, B, J_min, N, max_chains=C)
    assert (plan.ncoefs, plan.nscal) == (M.ncoefs, M.nscal)
    X = _cplx(rng, C, M.ncoefs)
    f = _cplx(rng, C, L * (2 * L - 1))
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        got = getattr(plan, name)(arg).cpu().numpy()
        for c in rows:
            ref = getattr(M, name)(arg[c])
            assert _rel(got[c], ref) < tol, (name, L, B, J_min, N, c, _rel(got[c], ref))


@pytest.mark.parametrize("L", [8, 16, 32])
@pytest.mark.parametrize("N", [2, 3, 4])
@pytest.mark.parametrize("B", [1.5, 2.0])
@pytest.mark.parametrize("J_min", [1, 2])
def test_dirwav_four_ops_match_model(L, N, B, J_min):
    _four_ops_vs_model(L, B, J_min, N, 2, [0, 1], 1e-12)


@pytest.mark.parametrize("N", [5, 6, 8, 12])
@pytest.mark.parametrize("J_min", [1, 2])
def test_dirwav_four_ops_match_model_gamma_variants(N, J_min):
    """with N = 2, 3, 4 above and 7, 9 below: every instantiation of the gamma stage (N = 1 .. 8 unrolled, the generic one
    beyond) runs against the model"""
    _four_ops_vs_model(16, 2.0, J_min, N, 2, [0, 1], 1e-12)


@pytest.mark.parametrize("L,B,J_min", OTHER_TILINGS)
@pytest.mark.parametrize("N", [2, 5, "L"])
@pytest.mark.parametrize("C", [1, 3])
def test_dirwav_four_ops_match_model_other_tilings(L, B, J_min, N, C):
    """non-dyadic B, odd L (partial last workgroups), J_min = 0 and N = L, with C = 1 and 3 chains on a plan of 5 and
    outputs of 5 rows (the rows past C stay as they were); and per block: every (scale, plane) block of the coefficient
    vector to 1e-12 of its own largest entry, so that the top scale cannot hide the others"""
    import ctypes

    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import check, lib

    N = L if N == "L" else N
    CMAX = 5
    rng = np.random.default_rng(1000 * L + 100 * J_min + 10 * N + C)
    M = DirWavModel(L, B, J_min, N)
    plan = ops.DirWavPlan(L, B, J_min, N, max_chains=CMAX)
    assert (plan.ncoefs, plan.nscal) == (M.ncoefs, M.nscal)
    X = _cplx(rng, C, M.ncoefs)
    f = _cplx(rng, C, L * (2 * L - 1))
    vp = ctypes.c_void_p
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        ref = np.stack([getattr(M, name)(arg[c]) for c in range(C)])
        src = torch.as_tensor(arg).cuda()
        out = torch.full((CMAX, ref.shape[1]), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
        check(getattr(lib, "pxm_dwav_" + name)(plan._h, vp(src.data_ptr()), vp(out.data_ptr()), C, None))
        out = out.cpu().numpy()
        assert np.isnan(out[C:].real).all() and np.isnan(out[C:].imag).all(), name
        got = out[:C]
        assert _rel(got, ref) < 1e-12, (name, _rel(got, ref))
        if ref.shape[1] == M.ncoefs:
            for i in range(len(M.bls)):
                npl = 1 if i == 0 else M.npl
                a, b = M.offsets[i], M.offsets[i + 1]
                gb, rb = got[:, a:b].reshape(C, npl, -1), ref[:, a:b].reshape(C, npl, -1)
                for q in range(npl):
                    scale = np.abs(rb[:, q]).max()
                    assert np.abs(gb[:, q] - rb[:, q]).max() <= 1e-12 * scale, (name, i, q)


def test_dirwav_skipped_pairs_match_model():
    """L = 16, B = 2, J_min = 1, N = 5: the scales at bl_j = 2, 4 skip the pairs with |n| >= bl_j"""
    M = DirWavModel(16, 2.0, 1, 5)
    assert any(len(M._pairs(j)) < 5 for j in range(len(M.bls) - 1))
    _four_ops_vs_model(16, 2.0, 1, 5, 2, [0, 1], 1e-12)


def test_dirwav_four_ops_match_model_L256_16chains():
    _four_ops_vs_model(256, 2.0, 2, 4, 16, [0, 15], 1e-11)


def test_dirwav_refusals_leave_plan_usable():
    """every transform entry point refuses too many chains and a null input on the host, in its own name, and the plan
    computes the same afterwards"""
    import ctypes

    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import lib

    L = 8
    plan = ops.DirWavPlan(L, 2.0, 1, 2, max_chains=2)
    X0 = _cplx(np.random.default_rng(5), 2, plan.ncoefs)
    before = plan.synthesis(X0).clone()
    x = torch.zeros((3, plan.ncoefs), dtype=torch.complex128, device="cuda")
    f = torch.zeros((3, plan.npix), dtype=torch.complex128, device="cuda")
    vp = ctypes.c_void_p
    for name, out in (("synthesis", f), ("synthesis_adjoint", x), ("analysis", x), ("analysis_adjoint", f)):
        fn = getattr(lib, "pxm_dwav_" + name)
        src = x if out is f else f
        assert fn(plan._h, vp(src.data_ptr()), vp(out.data_ptr()), 3, None) < 0
        assert b"pxm_dwav_" + name.encode() + b": C outside [1, max_chains]" in lib.pxm_last_error()
        assert fn(plan._h, None, vp(out.data_ptr()), 1, None) < 0
        assert b"pxm_dwav_" + name.encode() + b": null argument" in lib.pxm_last_error()
    assert torch.equal(plan.synthesis(X0), before)


# ---- operator properties -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B,J_min,N", [(16, 2.0, 1, 2), (32, 1.5, 2, 3), (32, 2.0, 2, 4), (64, 2.0, 2, 7), (24, 2.0, 1, 9)])
def test_dirwav_properties(L, B, J_min, N):
    from pxmcmc_amd import ops

    C = 2
    rng = np.random.default_rng(L + N)
    plan = ops.DirWavPlan(L, B, J_min, N, max_chains=C)
    f = np.stack([bandlimited_image(L, rng) for _ in range(C)])
    X = plan.analysis(f)
    assert _rel(plan.synthesis(X).cpu().numpy(), f) < 1e-10  # exact left inverse
    Y = _cplx(rng, C, plan.ncoefs)
    g = _cplx(rng, C, plan.npix)
    for c in range(C):
        lhs = np.vdot(Y[c], plan.analysis(g[c]).cpu().numpy())
        rhs = np.vdot(plan.analysis_adjoint(Y[c]).cpu().numpy(), g[c])
        assert abs(lhs - rhs) < 1e-11 * abs(lhs)
        lhs = np.vdot(g[c], plan.synthesis(Y[c]).cpu().numpy())
        rhs = np.vdot(plan.synthesis_adjoint(g[c]).cpu().numpy(), Y[c])
        assert abs(lhs - rhs) < 1e-11 * abs(lhs)
    fr = bandlimited_image(L, rng, real=True)
    Xr = plan.analysis(fr).cpu().numpy()
    assert np.abs(Xr.imag).max() < 1e-12 * np.abs(Xr.real).max()


@pytest.mark.parametrize("N", [2, 3])
def test_dirwav_rotation_about_z_shifts_alpha(N):
    """f(theta, phi - 2 pi k / (2 bl_j - 1)) -> every plane of scale j shifted by k samples in alpha"""
    from oracle import ssht
    from pxmcmc_amd import ops

    L, B, J_min = 16, 2.0, 1
    rng = np.random.default_rng(N)
    M = DirWavModel(L, B, J_min, N)
    plan = ops.DirWavPlan(L, B, J_min, N)
    flm = _cplx(rng, L * L)
    X = plan.analysis(ssht.inverse(flm, L, 0).ravel()).cpu().numpy()
    m = np.concatenate([np.arange(-el, el + 1) for el in range(L)])
    for j, bl in enumerate(M.bls[1:]):
        k = 1 + j % 3
        phi0 = 2 * np.pi * k / (2 * bl - 1)
        Xr = plan.analysis(ssht.inverse(flm * np.exp(-1j * m * phi0), L, 0).ravel()).cpu().numpy()
        a = M._planes(X, j).reshape(2 * N - 1, bl, 2 * bl - 1)
        b = M._planes(Xr, j).reshape(2 * N - 1, bl, 2 * bl - 1)
        assert _rel(b, np.roll(a, k, axis=2)) < 1e-11, (j, bl)


# ---- samplers on a directional operator ---------------------------------------------------------------------------------
def _dir_problem(C=1, N=3, seed=5):
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.prior import S2_Wavelets_L1

    L, B, J_min = 16, 2, 2
    rng = np.random.default_rng(seed)
    data = rng.normal(size=L * (2 * L - 1))
    lmda, mu = 1e-3, 1.0
    op = SphericalWaveletTransformOperator(data, 0.1, "synthesis", L, B, J_min, dirs=N, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", op.transform.inverse, op.transform.inverse_adjoint, lmda * mu, L=L, B=B, J_min=J_min,
                         dirs=N)
    return op, reg, data, lmda, mu, rng


def test_myula_directional_matches_numpy_model():
    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams

    op, reg, data, lmda, mu, rng = _dir_problem()
    L, B, J_min, N = 16, 2.0, 2, 3
    delta = 5e-4
    p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, nsamples=4, nburn=2, ngap=2, verbosity=0)
    s = MYULA(op, reg, p, rng="numpy")
    X0 = rng.normal(size=op.nparams) * 0.1
    np.random.seed(3)
    _quiet(s.run, start_point=X0)
    assert not s._fused_wav
    M = DirWavModel(L, B, J_min, N)

    class _T:
        inverse = staticmethod(M.synthesis)
        inverse_adjoint = staticmethod(M.synthesis_adjoint)

    P = L * (2 * L - 1)
    oop = ref.ForwardOperator(data, 0.1, "synthesis", _T, ref.Identity(P, P), M.ncoefs)
    oreg = ref.L1("synthesis", None, None, lmda * mu * reg.map_weights)
    oreg.prior = lambda X: np.sum(np.abs(reg.map_weights * X))
    np.random.seed(3)
    noise = [np.random.randn(op.nparams) for _ in range(s.niter)]
    out = ref.myula_run(oop, oreg, lmda, delta, mu, 4, 2, 2, X0.astype(complex), lambda i: noise[i])
    scale = np.abs(out["chain"]).max()
    assert np.abs(s.chain - out["chain"]).max() < 1e-9 * scale
    np.testing.assert_allclose(s.logPi, out["logPi"].real, rtol=1e-9)


def test_myula_directional_graph_equals_eager_and_fused_gate():
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams
    from pxmcmc_amd.prior import S2_Wavelets_L1

    C = 2
    op, reg, data, lmda, mu, rng = _dir_problem(C)
    X0 = rng.normal(size=op.nparams) * 0.1
    runs = []
    for use_graph in (True, False):
        p = PxMCMCParams(lmda=lmda, delta=5e-4, mu=mu, nsamples=3, nburn=4, ngap=5, verbosity=0)
        s = MYULA(op, reg, p, nchains=C, seed=4, use_graph=use_graph)
        _quiet(s.run, start_point=X0)
        assert not s._fused_wav
        # (use_graph=False: the engine's eager-only form, the reference's calls iteration by iteration)
        assert getattr(s, "used_graph", False) == use_graph, getattr(s, "graph_error", None)
        runs.append(s)
    np.testing.assert_array_equal(runs[0].chain, runs[1].chain)
    np.testing.assert_array_equal(runs[0].logPi, runs[1].logPi)
    assert np.isfinite(runs[0].chain).all()
    # dirs = 1 keeps the fused WavPlan path
    L, B, J_min = 16, 2, 2
    op1 = SphericalWaveletTransformOperator(data, 0.1, "synthesis", L, B, J_min, max_chains=C)
    reg1 = S2_Wavelets_L1("synthesis", op1.transform.inverse, op1.transform.inverse_adjoint, lmda * mu, L=L, B=B, J_min=J_min)
    s1 = MYULA(op1, reg1, PxMCMCParams(lmda=lmda, delta=5e-4, mu=mu, nsamples=2, nburn=0, ngap=1, verbosity=0), nchains=C)
    _quiet(s1.run, start_point=rng.normal(size=op1.nparams) * 0.1)
    assert s1._fused_wav


def test_pxmala_and_skrock_directional_run_finite():
    from pxmcmc_amd.mcmc import SKROCK, PxMALA, PxMCMCParams

    C = 2
    op, reg, data, lmda, mu, rng = _dir_problem(C, N=2)
    X0 = rng.normal(size=op.nparams) * 0.1
    p = PxMCMCParams(lmda=lmda, delta=1e-4, mu=mu, nsamples=3, nburn=2, ngap=2, verbosity=0)
    m = PxMALA(op, reg, p, nchains=C, tune_delta=True)
    _quiet(m.run, start_point=X0)
    assert np.isfinite(m.chain).all() and np.isfinite(m.logPi).all()
    p = PxMCMCParams(lmda=lmda, delta=1e-3, mu=mu, s=3, nsamples=3, nburn=2, ngap=2, verbosity=0)
    k = SKROCK(op, reg, p, nchains=C)
    _quiet(k.run, start_point=X0)
    assert np.isfinite(k.chain).all() and np.isfinite(k.logPi).all()
    assert k.used_graph, getattr(k, "graph_error", None)
