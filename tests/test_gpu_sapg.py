"""SAPG on the GPU: the step kernel of pxm_sapg_step against the extended-precision model of tests/test_sapg_host.py on every
element of every chain and, bit for bit, against pxm_myula_step; its per-chain sum; the update kernel from its own trace;
SAPG.run (graph replay against eager stepping, the marginal MLE of the Laplace problem) and the refusals."""
import ctypes

import numpy as np
import pytest

from test_sapg_host import (C0_MEASURED, EPS, SAPG_REL_DEV, closed_form_mle, error_scale, laplace_problem, ratio_to_ext,
                            sapg_step_ext, sapg_sum_np, step_inputs)

pytestmark = pytest.mark.gpu

C_BOUND = 4 * C0_MEASURED  # the margin tests/test_gpu_fista.py gives its kernel over its numpy route: device sqrt / division
C_MAX = 5  # chains the state buffers are allocated for


def _step(X, g, T, theta, eta, delta, lmda, C=None, chains=None, noise=None, rho=(0.0,), d=1.0, lo=-50.0, hi=50.0, pool=False,
          n_trace=1, it=0, it_dev=0, **kw):
    """the kernel on chains [0, C) (or the listed ones, one launch each) of state buffers allocated for C_MAX and prefilled
    with NaN -> (X1, theta, eta, trace) as numpy; theta / eta / trace hold the launched chains only"""
    import torch

    from pxmcmc_amd import ops

    C = X.shape[0] if C is None else C
    n = X.shape[1]
    dev = ops.device()
    dt = torch.complex128 if np.iscomplexobj(X) else torch.float64

    def buf(a=None, dtype=dt):
        t = torch.full((C_MAX, n), float("nan"), dtype=dtype, device=dev)
        if a is not None:
            t[: a.shape[0]] = ops.as_device(a, dtype)
        return t

    bX, bg, bX1 = buf(X), buf(g), buf()
    bw = None if noise is None else buf(noise, torch.complex128 if np.iscomplexobj(noise) else torch.float64)
    Tdev = ops.as_device(T, torch.float64) if np.ndim(T) and np.size(T) > 1 else float(np.ravel(T)[0])
    rho_dev = ops.as_device(np.asarray(rho, dtype=float), torch.float64)
    cnt = torch.full((1,), int(it_dev), dtype=torch.int64, device=dev)
    th_out, eta_out, tr_out = [], [], []
    for sl in ([slice(0, C)] if chains is None else [slice(c, c + 1) for c in chains]):
        th = ops.as_device(np.asarray(theta, dtype=float)[sl], torch.float64).clone()
        et = ops.as_device(np.asarray(eta, dtype=float)[sl], torch.float64).clone()
        tr = torch.full((n_trace, th.numel(), 3), float("nan"), dtype=torch.float64, device=dev)
        ops.sapg_step(bX[sl], bg[sl], Tdev, delta, lmda, th, et, d, rho_dev, lo, hi, pool=pool, trace=tr,
                      noise=None if bw is None else bw[sl], it=it, iter_dev=cnt, out=bX1[sl],
                      chain0=kw.get("chain0", 0) + (sl.start if chains is not None else 0),
                      **{k: v for k, v in kw.items() if k != "chain0"})
        th_out.append(th.cpu().numpy()), eta_out.append(et.cpu().numpy()), tr_out.append(tr.cpu().numpy())
    torch.cuda.synchronize()
    assert torch.isnan(bX1[C:].real).all()  # nothing past the launched chains
    return bX1[:C].cpu().numpy(), np.concatenate(th_out), np.concatenate(eta_out), np.concatenate(tr_out, axis=1)


# ---- 1. one step, element by element ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 65541])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("vecT", [False, True], ids=["scalarT", "vectorT"])
def test_one_step_against_extended_model(n, C, cplx, vecT):
    """every element of every chain within 4 x C0_MEASURED x 2^-52 S_e of the extended-precision model: one slice, two slices
    and the grid-stride case; theta differs per chain; the noise is injected; rho = 0 leaves theta alone"""
    inp = step_inputs(n, C, cplx, vecT, seed=500 + n + 7 * C + 2 * cplx + vecT)
    X, g, T, theta, delta, lmda, w = inp
    X1, th, et, tr = _step(X, g, T, theta, np.log(theta), delta, lmda, noise=w, it=1, it_dev=2, n_trace=4)
    assert np.isfinite(X1.view(float)).all()
    worst = ratio_to_ext(X1, sapg_step_ext(*inp), error_scale(*inp))
    print(f"n={n} C={C} cplx={cplx} vecT={vecT}: worst ratio {worst:.3f} (bound {C_BOUND:.2f})")
    assert worst <= C_BOUND
    want = np.exp(np.log(theta))
    assert np.array_equal(et, np.log(theta)) and np.all(np.abs(th - want) <= 2 * np.spacing(want))
    assert np.isnan(tr[[0, 1, 2]]).all() and np.array_equal(tr[3, :, 1], et)  # row it + iter_dev = 3 and no other


# ---- 2. the arithmetic and the noise of pxm_myula_step ------------------------------------------------------------------
@pytest.mark.parametrize("cplx,noise_complex", [(False, False), (True, False), (True, True)], ids=["f64", "c128-real", "c128-cplx"])
@pytest.mark.parametrize("noise64", [False, True], ids=["bm32", "bm64"])
@pytest.mark.parametrize("vecT", [False, True], ids=["scalarT", "vectorT"])
def test_same_arithmetic_as_myula(cplx, noise_complex, noise64, vecT):
    """Philox noise: with theta = 1 the step equals ops.myula_step bit for bit; with theta != 1 it equals myula_step on
    T' = theta_c T formed in fp64 numpy, chain by chain"""
    import torch

    from pxmcmc_amd import ops

    n, C = 1031, 3
    X, g, T, theta, delta, lmda, _ = step_inputs(n, C, cplx, vecT, seed=40 + 2 * cplx + vecT)
    kw = dict(noise_complex=noise_complex, seed=9, chain0=5, noise64=noise64)
    cnt = torch.full((1,), 4, dtype=torch.int64, device=ops.device())
    myula = lambda x, gg, t, c0: ops.myula_step(ops.as_device(x), ops.as_device(gg), ops.as_device(t, torch.float64) if np.ndim(t) else  # noqa: E731
                                                float(t), delta, lmda, it=3, iter_dev=cnt, **dict(kw, chain0=c0)).cpu().numpy()
    ones = np.ones(C)
    X1, *_ = _step(X, g, T, ones, np.zeros(C), delta, lmda, it=3, it_dev=4, **kw)
    assert np.array_equal(X1, myula(X, g, T, 5))
    X1, *_ = _step(X, g, T, theta, np.log(theta), delta, lmda, it=3, it_dev=4, **kw)
    for c in range(C):
        assert np.array_equal(X1[c:c + 1], myula(X[c:c + 1], g[c:c + 1], theta[c] * T, 5 + c)), c
    assert not np.array_equal(X1[0], myula(X, g, T, 5)[0])  # (theta_0 = 0.7 does change the step)


# ---- 3. the sum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", [1, 257, 4097, 70001])
def test_per_chain_sum(n, cplx):
    """G_c of the trace against the host model's fixed-order sum of the kernel's own output -- at most n additions of
    non-negative terms that the kernel and numpy form identically: n 2^-52 relative -- and bit-equal to the same chain run alone"""
    C = 3
    X, g, T, theta, delta, lmda, w = step_inputs(n, C, cplx, True, seed=700 + n + cplx)
    X1, _, _, tr = _step(X, g, T, theta, np.log(theta), delta, lmda, noise=w)
    for c in range(C):
        want = sapg_sum_np(X1[c], T) / lmda
        rel = abs(tr[0, c, 2] - want) / (want if want else 1.0)
        print(f"n={n} cplx={cplx} chain {c}: G {tr[0, c, 2]:.17e}, host {want:.17e}, relative difference {rel:.3e} (bound {n * EPS:.3e})")
        assert rel <= n * EPS
    aX1, _, _, atr = _step(X, g, T, theta, np.log(theta), delta, lmda, noise=w, chains=range(C))
    assert np.array_equal(aX1, X1) and np.array_equal(atr, tr)


# ---- 4. the update, from the trace alone --------------------------------------------------------------------------------
RHO_12 = np.array([0.0, 0.0, 1e-4, 1e-4, 0.0, 2e-4, 1e-4, 5e-5])  # shorter than the 12 iterations: the last entry stays


def _twelve(pool):
    import torch

    from pxmcmc_amd import ops

    n, C, K = 300, 3, 12
    X, g, T, _, delta, lmda, _ = step_inputs(n, C, False, False, seed=3)
    theta0 = np.array([1.0, 1.0, 1.0]) if pool else np.array([0.7, 1.0, 2.3])
    lo, hi, d = float(np.log(0.5)), 5.0, float(n)  # (d - theta G < 0 here: eta falls until the clip holds it)
    dev = ops.device()
    th, et = ops.as_device(theta0, torch.float64), ops.as_device(np.log(theta0), torch.float64)
    tr = torch.full((K, C, 3), float("nan"), dtype=torch.float64, device=dev)
    rho = ops.as_device(RHO_12, torch.float64)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    x, gd, states = ops.as_device(X), ops.as_device(0.1 * g), []
    for k in range(K):
        x, _, _ = ops.sapg_step(x, gd, T, delta, lmda, th, et, d, rho, lo, hi, pool=pool, trace=tr, seed=2, iter_dev=cnt)
        ops.counter_add(cnt, 1)
        states.append(x.cpu().numpy())
    return dict(tr=tr.cpu().numpy(), theta0=theta0, lo=lo, hi=hi, d=d, states=states, T=T, lmda=lmda, th=th.cpu().numpy(), n=n)


def test_update_from_the_trace():
    """eta[k+1] = clip(eta[k] + rho_k (d - theta[k] G[k+1])) bit for bit with the trace's own theta and G; theta within 2 ulp
    of exp(eta) (the device exp is the only transcendental); zeros of the table leave eta alone; the clip is hit"""
    r = _twelve(pool=False)
    tr = r["tr"]
    theta, eta = r["theta0"], np.log(r["theta0"])
    for k in range(12):
        rho = RHO_12[min(k, len(RHO_12) - 1)]
        want = np.minimum(np.maximum(eta + rho * (r["d"] - theta * tr[k, :, 2]), r["lo"]), r["hi"])
        assert np.array_equal(tr[k, :, 1], want), (k, tr[k, :, 1], want)
        assert np.all(np.abs(tr[k, :, 0] - np.exp(want)) <= 2 * np.spacing(np.exp(want))), k
        if rho == 0.0:
            assert np.array_equal(want, eta)
        for c in range(3):  # G is the sum of the state the step left
            G = sapg_sum_np(r["states"][k][c], r["T"]) / r["lmda"]
            assert abs(tr[k, c, 2] - G) <= r["n"] * EPS * G
        theta, eta = tr[k, :, 0], tr[k, :, 1]
    print("eta trace:", tr[:, :, 1].tolist())
    assert np.any(tr[:, :, 1] == r["lo"]) and np.any(tr[:, :, 1] != r["lo"])
    assert np.array_equal(r["th"], tr[-1, :, 0])  # the caller's arrays hold the last row


def test_pooled_update():
    """pool: every chain carries the same theta, and its G is the chain-order mean of the chains' own sums"""
    r = _twelve(pool=True)
    tr = r["tr"]
    assert np.all(tr[:, :, 0] == tr[:, :1, 0]) and np.all(tr[:, :, 1] == tr[:, :1, 1]) and np.all(tr[:, :, 2] == tr[:, :1, 2])
    assert np.any(tr[:, 0, 1] == r["lo"])
    # the first step from the same state without pooling leaves each chain's own G (theta is 1 for all: the same X1)
    X, g, T, _, delta, lmda, _ = step_inputs(r["n"], 3, False, False, seed=3)
    kw = dict(rho=RHO_12, d=r["d"], lo=r["lo"], hi=r["hi"], seed=2)
    _, _, _, single = _step(X, 0.1 * g, T, np.ones(3), np.zeros(3), delta, lmda, **kw)
    _, _, _, pooled = _step(X, 0.1 * g, T, np.ones(3), np.zeros(3), delta, lmda, pool=True, **kw)
    G = single[0, :, 2]
    assert len(set(G)) == 3
    assert np.all(pooled[0, :, 2] == ((G[0] + G[1]) + G[2]) / 3.0)
    assert np.array_equal(pooled[0, :, 2], tr[0, :, 2])


# ---- 5. graph replay equals eager ---------------------------------------------------------------------------------------
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
    Lg = op.gradient_lipschitz(iters=1000, tol=1e-4) * (1 + 1e-4)
    p = PxMCMCParams(lmda=lmda, delta=0.8 / (Lg + 1 / lmda), mu=mu, verbosity=0)
    n = op.nparams
    X0 = np.stack([np.zeros(n, dtype=complex), (rng.normal(size=n) + 1j * rng.normal(size=n)) * 0.1, rng.normal(size=n) * 0.5 + 0j])
    return dict(op=op, reg=reg, p=p, X0=X0, C=C)


def test_graph_replay_equals_eager(wav16):
    from pxmcmc_amd.sapg import SAPG

    w = wav16
    runs = {}
    for graph in (True, False):
        est = SAPG(w["op"], w["reg"], w["p"], nchains=w["C"], theta0=[0.5, 1.0, 2.0], warmup=5, niter=35, burn=10, seed=3,
                   use_graph=graph)
        hat = est.run(start_point=w["X0"])
        assert est.used_graph == graph, est.graph_error
        assert est._eng["cnt"] is None and est._eng["one"] is None  # the engine is stopped
        assert hat.shape == (w["C"],) and est.theta_trace.shape == (40, w["C"]) and np.isfinite(est.theta_trace).all()
        assert np.array_equal(hat, est.theta_trace[15:].mean(axis=0)) and np.array_equal(est.mu_hat, w["p"].mu * hat)
        runs[graph] = est
    a, b = runs[True], runs[False]
    for k in ("theta_trace", "eta_trace", "g_trace"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.X_curr.cpu().numpy(), b.X_curr.cpu().numpy())
    assert np.all(a.theta_trace[:5] == a.theta_trace[0]) and np.allclose(a.theta_trace[0], [0.5, 1.0, 2.0], rtol=4 * EPS, atol=0)
    assert np.all(a.theta_trace[5] != a.theta_trace[4])
    print("theta after 35 moving iterations:", a.theta_trace[-1])


# ---- 6. statistical -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def laplace():
    prob = laplace_problem()
    return prob, closed_form_mle(prob["y"], prob["sigma"])


def _laplace_sapg(prob, vecT, theta0, **kw):
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.sapg import SAPG
    from pxmcmc_amd.transforms import IdentityTransform

    n = prob["n"]
    op = ForwardOperator(prob["y"], prob["sigma"], "synthesis", IdentityTransform(), Identity(n, n), nparams=n)
    reg = L1("synthesis", None, None, np.full(n, prob["T"]) if vecT else prob["T"])
    p = PxMCMCParams(lmda=prob["lmda"], delta=prob["delta"], mu=1.0, verbosity=0)
    est = SAPG(op, reg, p, nchains=4, theta0=theta0, theta_min=prob["theta_min"], theta_max=prob["theta_max"],
               warmup=prob["warmup"], niter=prob["niter"], burn=prob["burn"], **kw)
    return est, reg, p


@pytest.mark.parametrize("vecT,theta0", [(False, 1.0), (True, 25.0)], ids=["scalarT-from-1", "vectorT-from-25"])
def test_finds_the_marginal_mle(laplace, vecT, theta0):
    """the Laplace problem of the host file on the device, 4 chains: |mean(theta_hat) - MLE| / MLE <= 2 SAPG_REL_DEV (the
    factor 2 covers the Philox against the numpy stream; a wrong d, a missing 1 / lmda, a wrong sign or G of the old state
    are far outside)"""
    prob, mle = laplace
    est, reg, p = _laplace_sapg(prob, vecT, theta0, seed=1)
    hat = est.run(start_point=prob["y"])
    dev = (np.mean(hat) - mle) / mle
    print(f"MLE {mle:.4f}, theta_hat {hat}, relative deviation of the mean {100 * dev:+.3f} % (bound {200 * SAPG_REL_DEV:.2f} %)")
    assert est.used_graph, est.graph_error
    assert hat.shape == (4,) and abs(dev) <= 2 * SAPG_REL_DEV
    first = est.theta_trace[0]
    assert np.all(est.theta_trace[: prob["warmup"]] == first) and np.all(np.abs(first - theta0) <= 4 * np.spacing(theta0))
    # apply(): copies with T and mu scaled; the inputs stay as they are
    T_before, mu_before = np.copy(reg.T), p.mu
    reg2, p2 = est.apply(reg, p)
    s = float(np.mean(hat))
    assert reg2 is not reg and p2 is not p and np.array_equal(reg.T, T_before) and p.mu == mu_before
    assert np.array_equal(reg2.T, T_before * s) and p2.mu == mu_before * s
    Td = reg2.T_dev
    assert (Td == prob["T"] * s) if not vecT else np.array_equal(Td.cpu().numpy(), T_before * s)


def test_pooled_run_returns_one_theta(laplace):
    prob, mle = laplace
    est, _, _ = _laplace_sapg(prob, False, 1.0, seed=2, pool=True)
    hat = est.run(start_point=prob["y"])
    assert isinstance(hat, float) and np.all(est.theta_trace == est.theta_trace[:, :1])
    print(f"pooled: theta_hat {hat:.4f}, MLE {mle:.4f}")
    assert abs(hat - mle) / mle <= 2 * SAPG_REL_DEV


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_at_the_abi():
    """every refusal returns an error before anything is launched: the outputs keep their NaN"""
    import torch

    from pxmcmc_amd import _lib, ops

    dev = ops.device()
    n, C = 8, 2
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
    x, g, out = torch.zeros((C, n), dtype=torch.float64, device=dev), torch.zeros((C, n), dtype=torch.float64, device=dev), nan(C, n)
    theta, eta, trace, scratch = nan(C), nan(C), nan(2, C, 3), nan(257 * C)
    rho = torch.zeros(3, dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)  # noqa: E731
    good = dict(X=x, gradg=g, T=None, Ts=0.1, delta=0.01, lmda=0.02, noise=None, nc=0, theta=theta, eta=eta, d=8.0, rho=rho, n_rho=3,
                lo=-1.0, hi=1.0, pool=0, trace=trace, n_trace=2, out=out, scratch=scratch, n=n, C=C, dtype=0)

    def call(**kw):
        a = dict(good, **kw)
        return _lib.lib.pxm_sapg_step(p(a["X"]), p(a["gradg"]), p(a["T"]), a["Ts"], a["delta"], a["lmda"], p(a["noise"]), a["nc"], 0, 0, 0,
                                      ctypes.c_void_p(0), p(a["theta"]), p(a["eta"]), a["d"], p(a["rho"]), a["n_rho"], a["lo"], a["hi"],
                                      a["pool"], p(a["trace"]), a["n_trace"], p(a["out"]), p(a["scratch"]), a["n"], a["C"], a["dtype"],
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [dict(n=-1), dict(C=0), dict(dtype=2), dict(X=None), dict(gradg=None), dict(out=None), dict(theta=None), dict(eta=None),
           dict(scratch=None), dict(rho=None), dict(n_rho=0), dict(out=x), dict(out=g), dict(theta=rho), dict(eta=theta),
           dict(trace=None), dict(trace=theta), dict(lmda=0.0), dict(lmda=float("inf")), dict(delta=-1.0), dict(delta=float("nan")),
           dict(d=0.0), dict(d=float("inf")), dict(lo=1.0, hi=-1.0), dict(lo=float("nan")), dict(nc=1), dict(nc=2)]
    for kw in bad:
        assert call(**kw) < 0, kw
        assert b"pxm_sapg_step" in _lib.lib.pxm_last_error(), kw
    torch.cuda.synchronize()
    for t in (out, theta, eta, trace, scratch):
        assert torch.isnan(t).all()
    theta.fill_(1.0), eta.fill_(0.0)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(trace[0]).all() and torch.isnan(trace[1]).all()


def test_empty_state_still_updates():
    """n == 0: no step, G = 0, so eta moves by rho d"""
    import torch

    from pxmcmc_amd import ops

    x = torch.zeros((2, 0), dtype=torch.float64, device=ops.device())
    theta, eta = torch.ones(2, dtype=torch.float64, device=x.device), torch.zeros(2, dtype=torch.float64, device=x.device)
    trace = torch.full((1, 2, 3), float("nan"), dtype=torch.float64, device=x.device)
    ops.sapg_step(x, x.clone(), 0.1, 0.01, 0.02, theta, eta, 4.0, [0.125], -5.0, 5.0, trace=trace)
    assert torch.equal(eta, torch.full_like(eta, 0.5)) and torch.equal(trace[0, :, 2], torch.zeros(2, dtype=torch.float64, device=x.device))
    assert np.all(np.abs(theta.cpu().numpy() - np.exp(0.5)) <= 2 * np.spacing(np.exp(0.5)))


def test_driver_refusals():
    import torch

    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.sapg import SAPG
    from pxmcmc_amd.transforms import IdentityTransform

    n = 16
    op = ForwardOperator(np.zeros(n), 0.1, "synthesis", IdentityTransform(), Identity(n, n), nparams=n)
    ident = lambda x: x  # noqa: E731
    with pytest.raises(ValueError, match="stock synthesis L1"):
        SAPG(op, L1("analysis", ident, ident, 0.1), PxMCMCParams(lmda=1e-2, delta=1e-3, verbosity=0))
    with pytest.raises(ValueError, match="float delta"):
        SAPG(op, L1("synthesis", None, None, 0.1), PxMCMCParams(lmda=1e-2, delta=torch.full((1,), 1e-3), verbosity=0))
    with pytest.raises(ValueError):
        SAPG(op, L1("synthesis", None, None, 0.1), PxMCMCParams(lmda=1e-2, delta=1e-3, verbosity=0), theta0=1e4)
    with pytest.raises(ValueError):
        SAPG(op, L1("synthesis", None, None, 0.1), PxMCMCParams(lmda=1e-2, delta=1e-3, verbosity=0), niter=10, burn=10)
