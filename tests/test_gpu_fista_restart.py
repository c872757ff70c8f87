"""FISTA with adaptive restart on the GPU: pxm_fista_step_restart against pxm_fista_step bit for bit (restart off), its
fourth sum against the numpy model of the summation order, the decision per chain at its edges (r < 0, r == 0, the smallest
r > 0, NaN), the per-chain momentum, batch independence, and ``FISTA(restart="gradient")`` (graph replay, reset hook, fixed
point, iteration count against the plain run) and the examples' --map-restart.  Semantics: tests/test_fista_restart_host.py."""
import numpy as np
import pytest

from test_fista_host import C0_MEASURED, EPS, error_scale, fista_step_ext, ratio_to_ext, step_inputs
from test_fista_restart_host import restart_terms_np
from test_gpu_fista import (BETA_LONG, BETA_SHORT, C_BOUND, C_MAX, TOL, _assert_fixed_point, _run_step, _small_case,
                            wav16)  # noqa: F401  (wav16: the module's fixture, used here as one)
from test_gpu_sum_order import _same_bits, chain_slices, fixed_order_sum

pytestmark = pytest.mark.gpu

assert C_BOUND == 4 * C0_MEASURED


def _run_restart(inp, C, beta_tab, index, restart_on, proxf=None, chains=None, restarts0=0):
    """pxm_fista_step_restart on chains [0, C) (or the listed ones, one launch each) of buffers allocated for C_MAX, outputs
    prefilled with NaN, momentum indices preset to ``index`` and the restart counts to ``restarts0``
    -> (X1, Y1, sums, index, restarts) as numpy"""
    import torch

    from pxmcmc_amd import ops

    Y, g, X0, gamma, T, lmda, _ = inp
    n = Y.shape[1]
    dev = ops.device()
    dt = torch.complex128 if np.iscomplexobj(Y) else torch.float64

    def buf(a=None):
        t = torch.full((C_MAX, n), float("nan"), dtype=dt, device=dev)
        if a is not None:
            t[: a.shape[0]] = ops.as_device(a, dt)
        return t

    bY, bg, bX0, bX1, bY1 = buf(Y), buf(g), buf(X0), buf(), buf()
    bP = buf(proxf) if proxf is not None else None
    sums = torch.full((C_MAX, 4), float("nan"), dtype=torch.float64, device=dev)
    beta = ops.as_device(np.asarray(beta_tab, dtype=float), torch.float64)
    SENTINEL = 12345
    idx = torch.full((C_MAX,), SENTINEL, dtype=torch.int64, device=dev)
    idx[:C] = torch.as_tensor(np.broadcast_to(np.asarray(index, dtype=np.int64), (C,)).copy(), device=dev)
    rst = torch.full((C_MAX,), SENTINEL, dtype=torch.int64, device=dev)
    rst[:C] = int(restarts0)
    Tdev = ops.as_device(T, torch.float64) if np.ndim(T) else float(T)
    for sl in ([slice(0, C)] if chains is None else [slice(c, c + 1) for c in chains]):
        kw = dict(restarts=rst[sl], restart=restart_on, out=(bX1[sl], bY1[sl]), sums=sums[sl])
        if proxf is None:
            ops.fista_step_restart(bY[sl], bg[sl], bX0[sl], gamma, lmda, beta, idx[sl], T=Tdev, **kw)
        else:
            ops.fista_step_restart(bY[sl], None, bX0[sl], gamma, lmda, beta, idx[sl], proxf=bP[sl], **kw)
    torch.cuda.synchronize()
    assert torch.isnan(bX1[C:].real).all() and torch.isnan(bY1[C:].real).all() and torch.isnan(sums[C:]).all()  # nothing past C
    assert bool((idx[C:] == SENTINEL).all()) and bool((rst[C:] == SENTINEL).all())
    return bX1[:C].cpu().numpy(), bY1[:C].cpu().numpy(), sums[:C].cpu().numpy(), idx[:C].cpu().numpy(), rst[:C].cpu().numpy()


def _given_prox(inp):
    """a proxf array for the given-prox form: the stock shrink of V formed in numpy (any array would do: the kernel takes it
    as X1)"""
    from oracle import pxmcmc_np

    Y, g, X0, gamma, T, lmda, _ = inp
    return pxmcmc_np.soft(Y - gamma * g, gamma * T / lmda)


# ---- 1. restart off: the parent kernel bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 4097])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("vecT", [False, True], ids=["scalarT", "vectorT"])
@pytest.mark.parametrize("given", [False, True], ids=["stock", "given"])
def test_restart_off_equals_the_plain_step(n, C, cplx, vecT, given):
    """momentum_index[c] preset to the plain call's it + iter_dev (7), on a table that holds it and on one that ends before
    it (the clamp): X1, Y1 and the first three sums are those of ops.fista_step, the indices advance, nothing is counted"""
    inp = step_inputs(n, C, cplx, vecT, seed=500 + n + 7 * C + 2 * cplx + vecT)
    P = _given_prox(inp) if given else None
    for tab in (BETA_LONG, BETA_SHORT):
        X1, Y1, sums = _run_step(inp, C, tab, it=3, it_dev=4, proxf=P)
        rX1, rY1, rsums, idx, rst = _run_restart(inp, C, tab, 7, False, proxf=P)
        assert np.isfinite(X1.view(float)).all() and np.isfinite(Y1.view(float)).all()
        assert np.array_equal(rX1.view(np.int64), X1.view(np.int64)) and np.array_equal(rY1.view(np.int64), Y1.view(np.int64))
        assert np.array_equal(rsums[:, :2].view(np.int64), np.ascontiguousarray(sums[:, :2]).view(np.int64))
        if given:
            assert np.isnan(rsums[:, 2]).all() and np.isnan(sums[:, 2]).all()
        else:
            assert np.array_equal(rsums[:, 2], sums[:, 2])
        assert np.isfinite(rsums[:, 3]).all()
        assert np.array_equal(idx, np.full(C, 8)) and np.array_equal(rst, np.zeros(C, dtype=np.int64))


# ---- 2. the fourth sum, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 70001])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("given", [False, True], ids=["stock", "given"])
def test_restart_sum_bit_for_bit(n, cplx, given):
    """terms (y.re - x1.re) d.re + (y.im - x1.im) d.im from the kernel's own X1 and the inputs, the same rounded operations
    (contraction off), added in the order of csrc/reduce.h.  The terms are signed: a thread past the end still adds nothing,
    and x + 0.0 is x for every x but -0.0, so the padding of the model holds up to the sign of a zero sum"""
    C = 2
    assert chain_slices(n) == (256 if n == 70001 else 2)
    inp = step_inputs(n, C, cplx, True, seed=700 + n + cplx)
    Y, g, X0 = inp[:3]
    X1, _, sums, _, _ = _run_restart(inp, C, BETA_LONG, 2, True, proxf=_given_prox(inp) if given else None)
    want = [fixed_order_sum(restart_terms_np(Y[c], X1[c], X0[c]), chain_slices(n)) for c in range(C)]
    assert all(w != 0.0 for w in want)
    assert _same_bits(sums[:, 3], want)


# ---- 3., 4. the decision at its edges, then the momentum chain by chain -------------------------------------------------
def _edge_inputs():
    """given prox, n = 257, three chains: r < 0; r == 0 exactly (one term whose product underflows to 0, every other term
    0 * 0); r = 2^-1000 from the single element of the second slice"""
    n, C = 257, 3
    rng = np.random.default_rng(41)
    P = rng.normal(size=(C, n))
    Y, X0 = P.copy(), P.copy()  # y - x1 = 0 and d = 0 everywhere, then:
    e = rng.normal(size=n)
    Y[0], X0[0] = P[0] - 0.5 * e, P[0] - e  # chain 0: y - x1 = -e / 2, d = e (both rounded) -> every term <= 0
    P[1, 3], Y[1, 3], X0[1, 3] = 0.0, 2.0 ** -600, -(2.0 ** -600)  # chain 1: 2^-600 * 2^-600 underflows to 0
    P[2, 256], Y[2, 256], X0[2, 256] = 0.0, 2.0 ** -500, -(2.0 ** -500)  # chain 2: 2^-500 * 2^-500 = 2^-1000 exactly
    inp = (Y, np.zeros_like(Y), X0, 0.37, 0.0, 2.5e-2, None)
    return inp, P


def test_decision_edges_per_chain():
    inp, P = _edge_inputs()
    Y, _, X0 = inp[:3]
    terms = restart_terms_np(Y, P, X0)
    assert np.all(terms[0] <= 0) and terms[0].sum() < 0 and not terms[1].any() and terms[2, 256] == 2.0 ** -1000
    X1, Y1, sums, idx, rst = _run_restart(inp, 3, BETA_LONG, 7, True, proxf=P)
    print("r per chain:", [float(x).hex() for x in sums[:, 3]], "indices", idx, "restarts", rst)
    assert np.array_equal(X1, P)
    assert sums[0, 3] < 0 and sums[1, 3] == 0.0 and sums[2, 3] == 2.0 ** -1000
    assert np.array_equal(idx, [8, 8, 0]) and np.array_equal(rst, [0, 0, 1])
    # the step that decided keeps its momentum: Y1 = fma(beta_7, d, x1), one rounding away from the exact value
    d = P - X0
    assert np.all(np.abs(Y1 - (P + BETA_LONG[7] * d)) <= 2 * EPS * (np.abs(P) + BETA_LONG[7] * np.abs(d)))
    assert np.any(Y1[2] != P[2])
    # restart off: all three advance, nothing is counted; the sums are the same
    _, _, sums_off, idx, rst = _run_restart(inp, 3, BETA_LONG, 7, False, proxf=P)
    assert np.array_equal(idx, [8, 8, 8]) and np.array_equal(rst, [0, 0, 0]) and np.array_equal(sums_off, sums, equal_nan=True)
    # a restart count that is not wanted: a null pointer
    import torch

    from pxmcmc_amd import ops

    i2 = torch.full((3,), 7, dtype=torch.int64, device=ops.device())
    ops.fista_step_restart(ops.as_device(Y), None, ops.as_device(X0), 0.37, 2.5e-2, BETA_LONG, i2, proxf=ops.as_device(P))
    assert i2.cpu().tolist() == [8, 8, 0]
    # a NaN input: r is NaN, the chain advances and does not restart
    Yn = Y[2:3].copy()
    Yn[0, 100] = np.nan
    _, _, s, idx, rst = _run_restart((Yn, inp[1][2:3], X0[2:3]) + inp[3:], 1, BETA_LONG, 7, True, proxf=P[2:3])
    assert np.isnan(s[0, 3]) and np.array_equal(idx, [8]) and np.array_equal(rst, [0])


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_momentum_is_read_chain_by_chain(cplx):
    """the indices the edge case leaves, [8, 8, 0], taken from the device, then a stock step: every element of every chain
    within 4 x C0_MEASURED x 2^-52 S_e of the extended-precision model evaluated with that chain's beta"""
    inp, P = _edge_inputs()
    _, _, _, idx, _ = _run_restart(inp, 3, BETA_LONG, 7, True, proxf=P)
    assert np.array_equal(idx, [8, 8, 0])
    step = step_inputs(257, 3, cplx, True, seed=900 + cplx)
    Y, g, X0, gamma, T, lmda, _ = step
    X1, Y1, _, idx2, _ = _run_restart(step, 3, BETA_LONG, idx, True)
    worst = 0.0
    for c in range(3):
        beta = BETA_LONG[idx[c]]
        eX, eY = fista_step_ext(Y[c:c + 1], g[c:c + 1], X0[c:c + 1], gamma, T, lmda, beta)
        S = error_scale(Y[c:c + 1], g[c:c + 1], X0[c:c + 1], X1[c:c + 1], gamma, T, lmda, beta)
        worst = max(worst, ratio_to_ext(X1[c:c + 1], eX, S), ratio_to_ext(Y1[c:c + 1], eY, S))
        # and the other chain's beta would not pass: the momenta differ by far more than the bound
        other = BETA_LONG[0 if idx[c] else 8]
        assert ratio_to_ext(Y1[c:c + 1], fista_step_ext(Y[c:c + 1], g[c:c + 1], X0[c:c + 1], gamma, T, lmda, other)[1], S) > C_BOUND
    print(f"cplx={cplx}: worst ratio {worst:.3f} (bound {C_BOUND:.2f}); indices after the step {idx2}")
    assert worst <= C_BOUND


# ---- 5. batch independence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 70001])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_chain_alone_equals_chain_in_batch(n, cplx):
    C = 3
    inp = step_inputs(n, C, cplx, True, seed=1100 + n + cplx)
    index = [0, 5, 40]
    batch = _run_restart(inp, C, BETA_LONG, index, True, restarts0=2)
    alone = _run_restart(inp, C, BETA_LONG, index, True, restarts0=2, chains=range(C))
    for a, b in zip(batch, alone):
        assert np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))
    print("r", batch[2][:, 3], "indices", batch[3], "restarts", batch[4])
    assert np.array_equal(batch[3], np.where(batch[2][:, 3] > 0, 0, np.array(index) + 1))
    assert np.array_equal(batch[4], 2 + (batch[2][:, 3] > 0))


def test_empty_state_writes_its_sums_and_advances():
    import torch

    from pxmcmc_amd import ops

    x = torch.zeros((2, 0), dtype=torch.float64, device=ops.device())
    sums = torch.full((2, 4), float("nan"), dtype=torch.float64, device=x.device)
    idx = torch.tensor([3, 0], dtype=torch.int64, device=x.device)
    rst = torch.zeros(2, dtype=torch.int64, device=x.device)
    ops.fista_step_restart(x, x.clone(), x.clone(), 0.1, 0.1, [0.0], idx, T=0.1, restarts=rst, out=(x.clone(), x.clone()), sums=sums)
    assert torch.equal(sums, torch.zeros_like(sums)) and idx.cpu().tolist() == [4, 1] and rst.cpu().tolist() == [0, 0]
    # (the given-prox form of an empty state cannot be reached from torch: an empty tensor's data pointer is null, which is
    # how the library tells the two forms apart)


# ---- 6. FISTA.run(restart="gradient") -----------------------------------------------------------------------------------
def test_run_with_restart_on_wavelets(wav16):  # noqa: F811
    """graph replay equals eager stepping bit for bit, a second run on the same object reproduces the first (the reset hook
    rewinds the indices and the counts), the point is a fixed point, restarts happen, and at tol = 1e-4 the restarted run
    needs no more iterations than the plain one (restart=None: the path without this feature) from the same start.

    Measured on an MI355X (L = 16, 3 chains, tol = 1e-4, check_every = 10): plain 7850 / 8110 / 10000 (the third start does
    not meet the rule in 10000) iterations, restarted 40 / 40 / 40 with 4 counted restarts each.  The rule measures the step,
    and the steps after a restart are short: the restarted runs stop at F = 39769.78 / 39772.00 / 39779.67, the plain ones
    at 39767.82 / 39767.82 / 39767.84 (DESIGN.md section 14 has the iterations to equal objective)."""
    from pxmcmc_amd.optim import FISTA

    w = wav16
    kw = dict(nchains=w["C"], gamma=w["gamma"], tol=1e-4, max_iter=10000, check_every=10)
    keys = ("objective", "data_term", "prior_term", "rel_change", "last_steps", "restarts", "nrestarts", "niter", "checks")
    runs = {}
    for graph in (True, False):
        est = FISTA(w["op"], w["reg"], w["p"], use_graph=graph, restart="gradient", **kw)
        X = est.run(start_point=w["X0"])
        assert est.used_graph == graph, est.graph_error
        runs[graph] = (X, est, {k: np.copy(getattr(est, k)) for k in keys})
    X, est, first = runs[True]
    Xe, _, eager = runs[False]
    assert np.array_equal(X, Xe)
    for k in keys:
        assert np.array_equal(first[k], eager[k]), k
    assert est.restarts.shape == (len(est.checks), w["C"]) and est.nrestarts.shape == (w["C"],)
    assert np.all(np.diff(est.restarts, axis=0) >= 0) and np.array_equal(est.nrestarts, est.restarts[-1])
    X2 = est.run(start_point=w["X0"])  # the same object again: the reset hook
    assert np.array_equal(X2, X)
    for k in keys:
        assert np.array_equal(getattr(est, k), first[k]), k
    _assert_fixed_point(est, X, "L = 16 wavelets, 3 chains, gradient restart")
    plain = FISTA(w["op"], w["reg"], w["p"], restart=None, **kw)
    plain.run(start_point=w["X0"])
    print(f"iterations to tol = 1e-4: plain {plain.niter} (converged {plain.converged}), restarted {est.niter} with "
          f"{est.nrestarts} restarts")
    print(f"objective: plain {plain.objective_map}, restarted {est.objective_map}")
    assert not hasattr(plain, "restarts")
    assert np.all(est.nrestarts > 0)
    assert np.all(est.niter <= plain.niter)


# ---- 7. a complex inverse covariance ---------------------------------------------------------------------------------
def test_restart_on_the_weak_lensing_operator():
    """the weak-lensing operator at the smallest L tests/test_gpu_fista.py uses (complex data, real sig_d: the gradient is
    taken on gradient_operator(forward)), at that file's tolerance"""
    from pxmcmc_amd.optim import FISTA

    op, reg, p, X0 = _small_case("weaklensing")
    est = FISTA(op, reg, p, tol=TOL, max_iter=5000, check_every=10, restart="gradient")
    assert est.gradient_op is not op
    X = est.run(start_point=X0)
    assert est.used_graph, est.graph_error
    print(f"weak lensing: {est.niter} iterations, {est.nrestarts} restarts")
    _assert_fixed_point(est, X, "weaklensing, gradient restart")
    assert np.isfinite(est.objective).all()


# ---- 8. error reporting ---------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(wav16):  # noqa: F811
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError
    from pxmcmc_amd.optim import FISTA

    w = wav16
    with pytest.raises(ValueError):
        FISTA(w["op"], w["reg"], w["p"], gamma=w["gamma"], momentum=False, restart="gradient")
    with pytest.raises(ValueError):
        FISTA(w["op"], w["reg"], w["p"], gamma=w["gamma"], restart="function")
    x = torch.zeros((2, 8), dtype=torch.float64, device=ops.device())
    idx = torch.zeros(2, dtype=torch.int64, device=x.device)
    args = (0.1, 0.1, [0.0])
    with pytest.raises(PxmError, match="momentum_index"):  # a null momentum_index: the library's error path, not a fault
        ops.fista_step_restart(x, x.clone(), x.clone(), *args, None, T=0.1)
    with pytest.raises(PxmError):  # restarts is momentum_index
        ops.fista_step_restart(x, x.clone(), x.clone(), *args, idx, T=0.1, restarts=idx)
    with pytest.raises(PxmError):  # X_out aliases Y
        ops.fista_step_restart(x, x.clone(), x.clone(), *args, idx, T=0.1, out=(x, x.clone()))
    with pytest.raises(PxmError):  # a given prox without Y
        ops.fista_step_restart(None, None, x.clone(), *args, idx, proxf=x.clone())
    with pytest.raises(ValueError):  # neither T nor proxf
        ops.fista_step_restart(x, x.clone(), x.clone(), *args, idx)
    assert idx.cpu().tolist() == [0, 0]  # a refused call changes nothing


# ---- the examples' --map-restart --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["topography_synthetic", "weaklensing_synthetic"])
def test_examples_take_map_restart(name, tmp_path, capsys):
    """--map-start --map-restart at L = 16: the MAP start is found with restart and its count is printed beside the
    iterations; --map-restart alone is refused"""
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    small = ["--L", "16", "--nsamples", "2", "--ngap", "2", "--outdir", str(tmp_path)]
    mod.main(small + ["--map-start", "--map-restart"])
    out = capsys.readouterr().out
    line = next(ln for ln in out.splitlines() if ln.startswith("MAP start: FISTA stopped after"))
    assert " iterations, " in line and " restarts (converged: " in line, line
    with pytest.raises(SystemExit):
        mod.main(small + ["--map-restart"])
