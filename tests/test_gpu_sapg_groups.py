"""SAPG with one theta per group on the GPU (pxm_sapg_step_groups, SAPG(groups=...)): the step kernel against the extended-
precision model of tests/test_sapg_host.py with a threshold per element and, bit for bit, against pxm_myula_step and (one group)
pxm_sapg_step; the per-group sums; the update from its own trace; SAPG.run with groups="scale" (graph replay against eager
stepping), the block-wise marginal MLEs of the two-block Laplace problem, apply(), and the refusals."""
import ctypes

import numpy as np
import pytest

from test_gpu_sapg import wav16  # noqa: F401  (the L = 16 wavelet operator, as a fixture of this module too)
from test_sapg_groups_host import (GROUP_REL_DEV, block_mles, element_theta, sapg_groups_sum_np, two_block_problem)
from test_sapg_host import C0_MEASURED, EPS, error_scale, ratio_to_ext, sapg_step_ext, sapg_sum_np, step_inputs

pytestmark = pytest.mark.gpu

C_BOUND = 4 * C0_MEASURED  # the margin tests/test_gpu_sapg.py gives the ungrouped kernel
C_MAX = 5  # chains the state buffers are allocated for
BOUNDS = {
    "one": (0, 257),
    "tiny": (0, 1, 258, 300),  # a one-element group and a boundary inside a 256-block
    "stride": (0, 3, 65544, 65600),  # 65 541 elements: more than 256 slices of 256, the grid-stride path
}
CHAIN_THETA = np.array([0.7, 1.0, 2.3])
GROUP_FACTOR = np.array([1.0, 1.9, 0.45])


def _thetas(C, K):
    """[C, K], different per chain and per group"""
    return CHAIN_THETA[:C, None] * GROUP_FACTOR[None, :K]


def _step(X, g, T, theta, eta, bounds, delta, lmda, chains=None, noise=None, rho=None, d=None, lo=-50.0, hi=50.0, pool=False,
          n_trace=1, it=0, it_dev=0, **kw):
    """the kernel on all chains (or the listed ones, one launch each) of state buffers allocated for C_MAX and prefilled with
    NaN -> (X1, theta, eta, trace) as numpy; theta, eta [C, K], trace [n_trace, C, K, 3]"""
    import torch

    from pxmcmc_amd import ops

    C, n = X.shape
    K = len(bounds) - 1
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
    rho_dev = ops.as_device(np.zeros((1, K)) if rho is None else np.asarray(rho, dtype=float), torch.float64)
    d_dev = ops.as_device(np.ones(K) if d is None else np.asarray(d, dtype=float), torch.float64)
    cnt = torch.full((1,), int(it_dev), dtype=torch.int64, device=dev)
    th_out, eta_out, tr_out = [], [], []
    for sl in ([slice(0, C)] if chains is None else [slice(c, c + 1) for c in chains]):
        th = ops.as_device(np.asarray(theta, dtype=float)[sl], torch.float64).clone()
        et = ops.as_device(np.asarray(eta, dtype=float)[sl], torch.float64).clone()
        tr = torch.full((n_trace, th.shape[0], K, 3), float("nan"), dtype=torch.float64, device=dev)
        ops.sapg_step_groups(bX[sl], bg[sl], Tdev, delta, lmda, th, et, bounds, d_dev, rho_dev, lo, hi, pool=pool, trace=tr,
                             noise=None if bw is None else bw[sl], it=it, iter_dev=cnt, out=bX1[sl],
                             chain0=kw.get("chain0", 0) + (sl.start if chains is not None else 0),
                             **{k: v for k, v in kw.items() if k != "chain0"})
        th_out.append(th.cpu().numpy()), eta_out.append(et.cpu().numpy()), tr_out.append(tr.cpu().numpy())
    torch.cuda.synchronize()
    assert torch.isnan(bX1[C:].real).all()  # nothing past the launched chains
    return bX1[:C].cpu().numpy(), np.concatenate(th_out), np.concatenate(eta_out), np.concatenate(tr_out, axis=1)


# ---- 1. one step, element by element ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(BOUNDS))
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("vecT", [False, True], ids=["scalarT", "vectorT"])
def test_one_step_against_extended_model(which, C, cplx, vecT):
    """every element of every chain within 4 x C0_MEASURED x 2^-52 S_e of the extended-precision model whose threshold is
    fl(theta[c][k(i)] T_i); the noise is injected; rho = 0 leaves theta alone"""
    bounds = BOUNDS[which]
    n, K = bounds[-1], len(bounds) - 1
    X, g, T, _, delta, lmda, w = step_inputs(n, C, cplx, vecT, seed=900 + n + 7 * C + 2 * cplx + vecT)
    theta = _thetas(C, K)
    X1, th, et, tr = _step(X, g, T, theta, np.log(theta), bounds, delta, lmda, noise=w, it=1, it_dev=2, n_trace=4)
    assert np.isfinite(X1.view(float)).all()
    Tel = element_theta(theta, bounds) * np.broadcast_to(np.asarray(T, dtype=float), (n,))  # fl(theta T) per element, [C, n]
    inp = (X, g, Tel, np.ones(C), delta, lmda, w)
    worst = ratio_to_ext(X1, sapg_step_ext(*inp), error_scale(*inp))
    print(f"{which} C={C} cplx={cplx} vecT={vecT}: worst ratio {worst:.3f} (bound {C_BOUND:.2f})")
    assert worst <= C_BOUND
    want = np.exp(np.log(theta))
    assert np.array_equal(et, np.log(theta)) and np.all(np.abs(th - want) <= 2 * np.spacing(want))
    assert np.isnan(tr[[0, 1, 2]]).all() and np.array_equal(tr[3, :, :, 1], et)  # row it + iter_dev = 3 and no other


# ---- 2. the arithmetic and the noise of pxm_myula_step; one group is pxm_sapg_step ---------------------------------------
@pytest.mark.parametrize("cplx,noise_complex", [(False, False), (True, False), (True, True)], ids=["f64", "c128-real", "c128-cplx"])
@pytest.mark.parametrize("noise64", [False, True], ids=["bm32", "bm64"])
def test_same_arithmetic_as_myula(cplx, noise_complex, noise64):
    """Philox noise, keyed by the element's index in the whole state: chain by chain the step equals ops.myula_step on
    T'_i = theta[c][k(i)] T_i formed in fp64 numpy, bit for bit (scalar and vector T)"""
    import torch

    from pxmcmc_amd import ops

    bounds, C = (0, 1, 258, 300, 1031), 3
    n, K = bounds[-1], len(bounds) - 1
    theta = CHAIN_THETA[:, None] * np.array([1.0, 1.9, 0.45, 1.3])[None, :]
    kw = dict(noise_complex=noise_complex, seed=9, chain0=5, noise64=noise64)
    cnt = torch.full((1,), 4, dtype=torch.int64, device=ops.device())
    for vecT in (False, True):
        X, g, T, _, delta, lmda, _ = step_inputs(n, C, cplx, vecT, seed=60 + 2 * cplx + vecT)
        X1, *_ = _step(X, g, T, theta, np.log(theta), bounds, delta, lmda, it=3, it_dev=4, **kw)
        Tel = element_theta(theta, bounds) * np.broadcast_to(np.asarray(T, dtype=float), (n,))
        for c in range(C):
            want = ops.myula_step(ops.as_device(X[c:c + 1]), ops.as_device(g[c:c + 1]), ops.as_device(Tel[c], torch.float64), delta,
                                  lmda, it=3, iter_dev=cnt, **dict(kw, chain0=5 + c)).cpu().numpy()
            assert np.array_equal(X1[c:c + 1], want), (vecT, c)
        plain, *_ = _step(X, g, T, np.ones((C, K)), np.zeros((C, K)), bounds, delta, lmda, it=3, it_dev=4, **kw)
        assert not np.array_equal(plain, X1)  # (the thetas do change the step)


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("pool", [False, True], ids=["own", "pooled"])
def test_one_group_is_sapg_step(cplx, pool):
    """K = 1, bounds (0, n): X1, theta, eta and the trace equal ops.sapg_step with d = d[0], rho = rho[:, 0], bit for bit"""
    import torch

    from pxmcmc_amd import ops

    n, C = 70001, 3
    X, g, T, theta, delta, lmda, _ = step_inputs(n, C, cplx, True, seed=77 + cplx)
    rho, d, lo, hi = np.array([0.0, 3e-6, 1e-6]), float(n), float(np.log(0.5)), 5.0
    dev = ops.device()
    x, gd, Td = ops.as_device(X), ops.as_device(0.1 * g), ops.as_device(T, torch.float64)
    res = []
    for grouped in (False, True):
        shape = (C, 1) if grouped else (C,)
        th, et = ops.as_device(theta.reshape(shape), torch.float64), ops.as_device(np.log(theta).reshape(shape), torch.float64)
        tr = torch.full((2, *shape, 3), float("nan"), dtype=torch.float64, device=dev)
        kw = dict(pool=pool, trace=tr, seed=4, it=1, noise_complex=cplx, noise64=True)
        if grouped:
            x1, _, _ = ops.sapg_step_groups(x, gd, Td, delta, lmda, th, et, (0, n), [d], rho[:, None], lo, hi, **kw)
        else:
            x1, _, _ = ops.sapg_step(x, gd, Td, delta, lmda, th, et, d, rho, lo, hi, **kw)
        res.append([t.cpu().numpy().reshape(-1) for t in (x1, th, et, tr)])
    for a, b in zip(*res):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.isfinite(res[0][3][3 * C:]).all() and not np.array_equal(res[0][2], np.log(theta))  # row 1 written, eta moved


# ---- 3. the sums --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("which", ["tiny", "stride"])
def test_group_sums(which, cplx):
    """G[c][k] of the trace against the host model's fixed-order sum of the group's slice of the kernel's own output (at most
    n_k additions of non-negative terms formed identically: n_k 2^-52 relative); bit-equal to the same chain run alone; and
    bit-equal to what ops.sapg_step leaves for the group's sub-vector run alone as a state of length n_k"""
    import torch

    from pxmcmc_amd import ops

    bounds, C = BOUNDS[which], 3
    n, K = bounds[-1], len(bounds) - 1
    X, g, T, _, delta, lmda, w = step_inputs(n, C, cplx, True, seed=800 + n + cplx)
    theta = _thetas(C, K)
    X1, _, _, tr = _step(X, g, T, theta, np.log(theta), bounds, delta, lmda, noise=w)
    for c in range(C):
        want = sapg_groups_sum_np(X1[c], T, bounds) / lmda
        for k in range(K):
            nk = bounds[k + 1] - bounds[k]
            rel = abs(tr[0, c, k, 2] - want[k]) / (want[k] if want[k] else 1.0)
            print(f"{which} cplx={cplx} chain {c} group {k}: G {tr[0, c, k, 2]:.17e}, host {want[k]:.17e}, relative difference "
                  f"{rel:.3e} (bound {nk * EPS:.3e})")
            assert rel <= nk * EPS
    aX1, _, _, atr = _step(X, g, T, theta, np.log(theta), bounds, delta, lmda, noise=w, chains=range(C))
    assert np.array_equal(aX1, X1) and np.array_equal(atr, tr)
    for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        th = ops.as_device(theta[:, k].copy(), torch.float64)
        sub_tr = torch.full((1, C, 3), float("nan"), dtype=torch.float64, device=th.device)
        sub, _, _ = ops.sapg_step(ops.as_device(X[:, a:b].copy()), ops.as_device(g[:, a:b].copy()), ops.as_device(T[a:b].copy(), torch.float64),
                                  delta, lmda, th, torch.log(th), 1.0, [0.0], -50.0, 50.0, trace=sub_tr,
                                  noise=ops.as_device(w[:, a:b].copy()))
        assert np.array_equal(sub.cpu().numpy(), X1[:, a:b]), k  # the same X1 rows ...
        assert np.array_equal(sub_tr.cpu().numpy()[0, :, 2], tr[0, :, k, 2]), k  # ... and the same sum, bit for bit


# ---- 4. the update, from the trace alone --------------------------------------------------------------------------------
RHO_12 = np.array([0.0, 0.0, 1e-4, 1e-4, 0.0, 2e-4, 1e-4, 5e-5])[:, None] * np.array([1.0, 8.0, 3.0])  # 8 rows for 12 iterations
BOUNDS_12 = (0, 40, 90, 300)


def _twelve(pool):
    import torch

    from pxmcmc_amd import ops

    n, C, K, N = 300, 3, 3, 12
    X, g, T, _, delta, lmda, _ = step_inputs(n, C, False, False, seed=3)
    theta0 = np.ones((C, K)) * GROUP_FACTOR if pool else _thetas(C, K)
    # every theta0 (the smallest is 0.7 * 0.45) lies inside the interval; d - theta G < 0 here: eta falls until the clip holds it
    lo, hi, d = float(np.log(0.3)), 5.0, np.diff(BOUNDS_12).astype(float)
    dev = ops.device()
    th, et = ops.as_device(theta0, torch.float64), ops.as_device(np.log(theta0), torch.float64)
    tr = torch.full((N, C, K, 3), float("nan"), dtype=torch.float64, device=dev)
    rho, dd = ops.as_device(RHO_12, torch.float64), ops.as_device(d, torch.float64)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = ops.sapg_groups_scratch(C, K, dev)
    x, gd, states = ops.as_device(X), ops.as_device(0.1 * g), []
    for k in range(N):
        x, _, _ = ops.sapg_step_groups(x, gd, T, delta, lmda, th, et, BOUNDS_12, dd, rho, lo, hi, pool=pool, trace=tr, seed=2,
                                       iter_dev=cnt, scratch=scratch)
        ops.counter_add(cnt, 1)
        states.append(x.cpu().numpy())
    return dict(tr=tr.cpu().numpy(), theta0=theta0, lo=lo, hi=hi, d=d, states=states, T=T, lmda=lmda, th=th.cpu().numpy())


@pytest.mark.parametrize("pool", [False, True], ids=["own", "pooled"])
def test_update_from_the_trace(pool):
    """eta[j+1] = clip(eta[j] + rho[j][k] (d[k] - theta[j] G[j+1])) bit for bit with the trace's own theta and G, per group;
    theta within 2 ulp of exp(eta); the table's last row stays after it ends; zeros leave eta alone; the clip is hit.
    pool: G[:, k] is the chain-order mean of the chains' own sums, group by group"""
    r = _twelve(pool)
    tr = r["tr"]
    theta, eta = r["theta0"], np.log(r["theta0"])
    for j in range(12):
        rho = RHO_12[min(j, len(RHO_12) - 1)]
        want = np.minimum(np.maximum(eta + rho * (r["d"] - theta * tr[j, :, :, 2]), r["lo"]), r["hi"])
        assert np.array_equal(tr[j, :, :, 1], want), (j, tr[j, :, :, 1], want)
        assert np.all(np.abs(tr[j, :, :, 0] - np.exp(want)) <= 2 * np.spacing(np.exp(want))), j
        if not rho.any():
            assert np.array_equal(want, eta)
        own = np.array([sapg_groups_sum_np(r["states"][j][c], r["T"], BOUNDS_12) / r["lmda"] for c in range(3)])
        if pool:  # the chain-order mean of the host model's sums: the bound of the sums holds for their mean
            own = np.broadcast_to(((own[0] + own[1]) + own[2]) / 3.0, own.shape)
        assert np.all(np.abs(tr[j, :, :, 2] - own) <= r["d"] * EPS * own)
        theta, eta = tr[j, :, :, 0], tr[j, :, :, 1]
    print("eta trace, chain 0:", tr[:, 0, :, 1].tolist())
    assert np.any(tr[..., 1] == r["lo"]) and np.any(tr[..., 1] != r["lo"])
    assert np.array_equal(r["th"], tr[-1, :, :, 0])  # the caller's arrays hold the last row
    if pool:
        assert np.all(tr == tr[:, :1]) and len({tuple(row) for row in tr[-1, 0]}) == 3  # one theta per group, not one in all


def test_pooled_mean_is_in_chain_order():
    """one pooled step against the same step without pooling: G[:, k] = ((G_0k + G_1k) + G_2k) / 3 of the chains' own sums"""
    X, g, T, _, delta, lmda, _ = step_inputs(300, 3, False, False, seed=3)
    ones = np.ones((3, 3))
    kw = dict(rho=RHO_12, d=np.diff(BOUNDS_12), lo=-1.0, hi=5.0, seed=2)
    _, _, _, single = _step(X, 0.1 * g, T, ones, 0 * ones, BOUNDS_12, delta, lmda, **kw)
    _, _, _, pooled = _step(X, 0.1 * g, T, ones, 0 * ones, BOUNDS_12, delta, lmda, pool=True, **kw)
    G = single[0, :, :, 2]
    assert len(set(G.ravel())) == 9
    assert np.array_equal(pooled[0, :, :, 2], np.broadcast_to(((G[0] + G[1]) + G[2]) / 3.0, (3, 3)))


# ---- 5. graph replay equals eager ---------------------------------------------------------------------------------------
def test_graph_replay_equals_eager(wav16):  # noqa: F811
    from pxmcmc_amd.sapg import SAPG
    from pxmcmc_amd.utils import wavelet_scale_bounds

    w = wav16
    bounds = wavelet_scale_bounds(16, 2, 2)
    K = len(bounds) - 1
    assert bounds[-1] == w["op"].nparams and K == 4
    runs = {}
    for graph in (True, False):
        est = SAPG(w["op"], w["reg"], w["p"], nchains=w["C"], theta0=[[0.5], [1.0], [2.0]], warmup=5, niter=35, burn=10, seed=3,
                   use_graph=graph, groups="scale")
        hat = est.run(start_point=w["X0"])
        assert est.used_graph == graph, est.graph_error
        assert est._eng["cnt"] is None and est._eng["one"] is None  # the engine is stopped
        assert np.array_equal(est.group_bounds, bounds)
        assert hat.shape == (w["C"], K) and est.theta_hat.shape == (3, K)
        assert est.theta_trace.shape == est.eta_trace.shape == est.g_trace.shape == (40, w["C"], K) and np.isfinite(est.theta_trace).all()
        assert np.array_equal(hat, est.theta_trace[15:].mean(axis=0)) and np.array_equal(est.mu_hat, w["p"].mu * hat)
        runs[graph] = est
    a, b = runs[True], runs[False]
    for k in ("theta_trace", "eta_trace", "g_trace"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.X_curr.cpu().numpy(), b.X_curr.cpu().numpy())
    first = np.repeat([[0.5], [1.0], [2.0]], K, axis=1)
    assert np.all(a.theta_trace[:5] == a.theta_trace[0]) and np.allclose(a.theta_trace[0], first, rtol=4 * EPS, atol=0)
    assert np.all(a.theta_trace[5] != a.theta_trace[4])
    assert len(set(a.theta_trace[-1, 0])) == K  # the scales went their own ways
    print("theta after 35 moving iterations:", a.theta_trace[-1].tolist())


# ---- 6. statistics ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_block():
    prob = two_block_problem()
    return prob, block_mles(prob)


@pytest.mark.parametrize("theta0", [1.0, 25.0], ids=["from-1", "from-25"])
def test_finds_the_block_mles(two_block, theta0):
    """the two-block Laplace problem of the host file on the device, 4 Philox chains: the chain mean of theta_hat[:, k] within
    2 GROUP_REL_DEV[k] of block k's MLE (the factor the ungrouped device test gives the Philox stream over numpy's); then
    apply(): T and the weights scaled per block, mu unchanged, mu prior'(X) = (1 / lmda) sum T'_i |X_i|"""
    from pxmcmc_amd import ops
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.sapg import SAPG
    from pxmcmc_amd.transforms import IdentityTransform

    prob, mles = two_block
    n, bounds = prob["n"], prob["bounds"]
    op = ForwardOperator(prob["y"], prob["sigma"], "synthesis", IdentityTransform(), Identity(n, n), nparams=n)
    reg = L1("synthesis", None, None, prob["T"])
    p = PxMCMCParams(lmda=prob["lmda"], delta=prob["delta"], mu=1.0, verbosity=0)
    est = SAPG(op, reg, p, nchains=4, theta0=theta0, theta_min=prob["theta_min"], theta_max=prob["theta_max"],
               warmup=prob["warmup"], niter=prob["niter"], burn=prob["burn"], seed=1, groups=bounds)
    hat = est.run(start_point=prob["y"])
    assert est.used_graph, est.graph_error
    assert hat.shape == (4, 2) and np.array_equal(est.group_bounds, bounds)
    dev = (hat.mean(axis=0) - mles) / mles
    for k in range(2):
        print(f"block {k + 1}: MLE {mles[k]:.4f}, theta_hat {hat[:, k]}, relative deviation of the mean {100 * dev[k]:+.3f} % "
              f"(bound {200 * GROUP_REL_DEV[k]:.2f} %)")
    assert np.all(np.abs(dev) <= 2 * np.array(GROUP_REL_DEV))
    first = est.theta_trace[0]
    assert np.all(est.theta_trace[: prob["warmup"]] == first) and np.all(np.abs(first - theta0) <= 4 * np.spacing(theta0))
    # apply()
    reg2, p2 = est.apply(reg, p)
    s = np.repeat(hat.mean(axis=0), np.diff(bounds))
    assert reg2 is not reg and p2 is not p and reg.T == prob["T"] and reg._weights_dev is None
    assert p2.mu == p.mu == 1.0
    assert np.array_equal(reg2.T, prob["T"] * s) and np.array_equal(reg2._weights_dev.cpu().numpy(), s)
    assert np.array_equal(reg2.T_dev.cpu().numpy(), prob["T"] * s)
    X = np.random.default_rng(11).normal(size=n)
    want = np.sum(reg2.T * np.abs(X)) / prob["lmda"]
    assert p2.mu * reg2.prior(ops.as_device(X)) == pytest.approx(want, rel=n * EPS)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_at_the_abi():
    """every refusal returns an error before anything is launched: the outputs keep their NaN"""
    import torch

    from pxmcmc_amd import _lib, ops

    dev = ops.device()
    n, C, K = 8, 2, 2
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
    x, g, out = torch.zeros((C, n), dtype=torch.float64, device=dev), torch.zeros((C, n), dtype=torch.float64, device=dev), nan(C, n)
    theta, eta, trace, scratch = nan(C, K), nan(C, K), nan(2, C, K, 3), nan(257 * K * C)
    rho, d = torch.zeros((3, K), dtype=torch.float64, device=dev), torch.full((K,), 4.0, dtype=torch.float64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)  # noqa: E731
    good = dict(X=x, gradg=g, T=None, Ts=0.1, delta=0.01, lmda=0.02, noise=None, nc=0, theta=theta, eta=eta, bounds=(0, 3, 8), K=K, d=d,
                rho=rho, n_rho=3, lo=-1.0, hi=1.0, pool=0, trace=trace, n_trace=2, out=out, scratch=scratch, n=n, C=C, dtype=0)

    def call(**kw):
        a = dict(good, **kw)
        b = None if a["bounds"] is None else (ctypes.c_int64 * len(a["bounds"]))(*a["bounds"])
        return _lib.lib.pxm_sapg_step_groups(p(a["X"]), p(a["gradg"]), p(a["T"]), a["Ts"], a["delta"], a["lmda"], p(a["noise"]), a["nc"],
                                             0, 0, 0, ctypes.c_void_p(0), p(a["theta"]), p(a["eta"]),
                                             ctypes.cast(b, ctypes.c_void_p) if b is not None else ctypes.c_void_p(0), a["K"], p(a["d"]),
                                             p(a["rho"]), a["n_rho"], a["lo"], a["hi"], a["pool"], p(a["trace"]), a["n_trace"],
                                             p(a["out"]), p(a["scratch"]), a["n"], a["C"], a["dtype"],
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    bad = [dict(K=0), dict(K=33, bounds=tuple(range(34)), n=33), dict(K=-1), dict(bounds=None), dict(bounds=(0, 5, 3)),  # unsorted
           dict(bounds=(0, 3, 3)), dict(bounds=(0, 0, 8)), dict(bounds=(0, 8, 8)),  # empty groups
           dict(bounds=(0, 3, 7)), dict(bounds=(1, 3, 8)), dict(bounds=(0, 8, 9)),  # short, not from 0, past n
           dict(n=0, bounds=(0, 0), K=1), dict(n=-1), dict(C=0), dict(dtype=2),
           dict(X=None), dict(gradg=None), dict(out=None), dict(theta=None), dict(eta=None), dict(scratch=None), dict(rho=None),
           dict(d=None), dict(n_rho=0), dict(out=x), dict(out=g), dict(out=d), dict(theta=rho), dict(theta=d), dict(eta=theta),
           dict(trace=None), dict(trace=theta), dict(scratch=d), dict(lmda=0.0), dict(lmda=float("inf")), dict(delta=-1.0),
           dict(delta=float("nan")), dict(lo=1.0, hi=-1.0), dict(lo=float("nan")), dict(nc=1), dict(nc=2)]
    for kw in bad:
        assert call(**kw) < 0, kw
        assert b"pxm_sapg_step_groups" in _lib.lib.pxm_last_error(), kw
    torch.cuda.synchronize()
    for t in (out, theta, eta, trace, scratch):
        assert torch.isnan(t).all()
    theta.fill_(1.0), eta.fill_(0.0)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(trace[0]).all() and torch.isnan(trace[1]).all()


def test_wrapper_refusals():
    """each shape has its own message"""
    import torch

    from pxmcmc_amd import ops

    dev = ops.device()
    n, C, K = 8, 2, 2
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
    good = dict(X=z(C, n), gradg=z(C, n), T=0.1, delta=0.01, lmda=0.02, theta=z(C, K) + 1, eta=z(C, K), bounds=(0, 3, 8), d=[3.0, 5.0],
                rho=z(3, K), eta_min=-1.0, eta_max=1.0, trace=z(2, C, K, 3), scratch=ops.sapg_groups_scratch(C, K, dev))
    assert good["scratch"].numel() == (ops.SAPG_SLICES_MAX + 1) * K * C
    cases = [(dict(theta=z(C)), r"theta must be a contiguous float64 \[C, K\]"), (dict(eta=z(K, C + 1)), r"eta must be a contiguous float64 \[C, K\]"),
             (dict(theta=z(C, 2 * K)[:, ::2]), r"theta must be"), (dict(d=[3.0]), r"d must be a contiguous float64 \[K\]"),
             (dict(d=z(K).to(torch.float32)), r"d must be"), (dict(rho=z(3)), r"rho must be a non-empty contiguous float64 \[n_rho, K\]"),
             (dict(rho=z(0, K)), r"rho must be"), (dict(rho=z(3, K + 1)), r"rho must be"),
             (dict(trace=z(2, C, 3)), r"trace must be a contiguous float64 \[n_trace, C, K, 3\]"), (dict(trace=z(2, K, C + 1, 3)), r"trace must be"),
             (dict(scratch=z(257 * K * C - 1)), r"scratch is too small \(sapg_groups_scratch\)"),
             (dict(bounds=(0, 3, 7)), r"bounds must increase strictly from 0 to n = 8"), (dict(bounds=(0, 8, 3)), r"bounds must increase"),
             (dict(bounds=(0.0, 3.0, 8.0)), r"bounds must be a sequence of integers"), (dict(bounds=(0,)), r"bounds must hold K \+ 1 offsets"),
             (dict(gradg=z(C, n + 1)), r"gradg shape mismatch"), (dict(delta=z(C)), r"delta must be a float")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match="sapg_step_groups: " + msg):
            ops.sapg_step_groups(**dict(good, **kw))
    x1, th, et = ops.sapg_step_groups(**good)
    assert x1.shape == (C, n) and th is good["theta"] and et is good["eta"] and torch.isfinite(good["trace"][0]).all()


def test_driver_refusals(wav16):  # noqa: F811
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.sapg import SAPG
    from pxmcmc_amd.transforms import IdentityTransform

    n = 16
    op = ForwardOperator(np.zeros(n), 0.1, "synthesis", IdentityTransform(), Identity(n, n), nparams=n)
    reg, p = L1("synthesis", None, None, 0.1), PxMCMCParams(lmda=1e-2, delta=1e-3, verbosity=0)
    with pytest.raises(ValueError, match="SphericalWaveletTransform"):
        SAPG(op, reg, p, groups="scale")
    with pytest.raises(ValueError, match="SphericalWaveletTransform"):
        SAPG(wav16["op"], wav16["reg"], wav16["p"], groups="scales")  # an unknown name
    for bad in ((0, 4, 15), (0, 4, 17), (1, 4, 16), (0, 4, 4, 16)):
        with pytest.raises(ValueError, match="groups"):
            SAPG(op, reg, p, groups=bad)
    with pytest.raises(ValueError, match="ambiguous"):
        SAPG(op, reg, p, nchains=2, groups=(0, 4, 16), theta0=[1.0, 2.0])
    with pytest.raises(ValueError, match="theta0"):
        SAPG(op, reg, p, nchains=3, groups=(0, 4, 16), theta0=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        SAPG(op, reg, p, nchains=2, groups=(0, 4, 16), theta0=[[1.0, 1e4]])  # outside [theta_min, theta_max]
    est = SAPG(op, reg, p, nchains=2, groups=(0, 4, 16), theta0=[[1.0], [2.0]], warmup=0, niter=3, burn=0)
    assert est.theta0.shape == (2, 2) and est.rho.shape == (3, 2) and np.array_equal(est.ndim, [4.0, 12.0])
    assert np.array_equal(est.rho[0], 10.0 / est.ndim)  # every group by its own dimension
