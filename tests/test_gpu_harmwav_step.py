"""The fused harmonic MYULA step (k_hw_myula, pxm_hwav_myula_step) on the GPU, instantiation by instantiation, against the
extended-precision model of tests/test_harmwav_step_host.py -- per chain and per element, no element left out:

    |X_out[e] - LD[e]| <= C 2^-52 S_e        |preds[lm] - LD[lm]| <= C 2^-52 SP_lm        C = 4 C0_MEASURED

(S, SP: the error scales of the model; C0_MEASURED: the fp64 numpy route against the same model, measured on the host; the
factor 4 is for FMA contraction and another summation order over <= 18 items.)  Every test id carries the K of the
instantiation it ran, asserted from plan.info() against the host count of active items per degree.  The noise is the
device stream (ops.randn, pinned to oracle/philox.py elsewhere) and enters the model as data.

Largest observed ratio |got - LD| / (2^-52 S) on the MI355X (bound 6.2), X' / preds, per K, small and full-size cases together:
    K = 2: 1.40 / 1.17    K = 3: 1.05 / 0.54    K = 5: 1.47 / 1.24    K = 9: 1.45 / 1.12    K = 17: 1.28 / 1.41    K = 0: 1.29 / 1.93
"""
import numpy as np
import pytest

from test_harmwav_step_host import (C0_MEASURED, CASES, FACTORS, FULL_SIZE, HarmStepModelLD, K_of, case_id, factor_id,
                                    step_inputs)

pytestmark = pytest.mark.gpu

C_BOUND = 4 * C0_MEASURED
LMDA, DELTA, SEED, CHAIN0, IT, IT_DEV = 2e-3, 5e-4, 5, 7, 11, 3


def _plan_and_model(case, kact, max_chains):
    from pxmcmc_amd import ops

    L, B, J_min, N, spin = case
    plan = ops.HarmWavPlan(L, B, J_min, N, spin=spin, max_chains=max_chains)
    M = HarmStepModelLD(L, B, J_min, N, spin, tiling=ops.tiling_axisym(L, B, J_min))
    assert (plan.ncoefs, plan.nscal) == (M.ncoefs, M.nscal)
    assert plan.info()[0] == len(M.items)
    assert plan.info()[2] == M.kact() == kact, "the plan's kact differs from the host count: another instantiation would run"
    return plan, M


def _run(plan, X, data, invcov, kernel, T, ncplx, n64, chain0=CHAIN0):
    """one step into NaN-filled buffers -> (X_out, preds) as numpy"""
    import torch

    x = torch.as_tensor(np.ascontiguousarray(X)).cuda()
    out = torch.full_like(x, complex(np.nan, np.nan))
    preds = torch.full((x.shape[0], plan.nlm), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
    it_dev = torch.full((1,), IT_DEV, dtype=torch.int64, device="cuda")
    Xn, Pn = plan.myula_step(x, data, invcov, kernel, T, DELTA, LMDA, noise_complex=bool(ncplx), seed=SEED, chain0=chain0, it=IT,
                             iter_dev=it_dev, out=out, preds_out=preds, noise64=bool(n64))
    assert Xn.data_ptr() == out.data_ptr() and Pn.data_ptr() == preds.data_ptr()
    return Xn.cpu().numpy(), Pn.cpu().numpy()


def _check(plan, M, C, wl, vecT, icplx, ncplx, n64, rng, independence=True):
    """the assertions of one (case, factor row); returns the largest ratios (X', preds)"""
    import torch

    from pxmcmc_amd import ops

    X, data, invcov, kernel, T = step_inputs(rng, M, C, wl, vecT, icplx)
    Xn, Pn = _run(plan, X, data, invcov, kernel, T, ncplx, n64)
    assert not np.isnan(Xn.view(np.float64)).any(), "an element of X_out was not written"
    assert not np.isnan(Pn.view(np.float64)).any(), "an element of preds was not written"
    xi = ops.randn(M.ncoefs, C, complex_=bool(ncplx), seed=SEED, chain0=CHAIN0, it=IT + IT_DEV, noise64=bool(n64)).cpu().numpy()
    # zero-weight elements: the plain update on a zero gradient, same stream
    zero = M.zero_weight_mask()
    it_dev = torch.full((1,), IT_DEV, dtype=torch.int64, device="cuda")
    plain = ops.myula_step(X, np.zeros_like(X), T, DELTA, LMDA, noise_complex=bool(ncplx), seed=SEED, chain0=CHAIN0, it=IT,
                           iter_dev=it_dev, noise64=bool(n64)).cpu().numpy()
    worst = [0.0, 0.0]
    for c in range(C):
        ref = M.step(X[c], data, invcov, kernel, T, DELTA, LMDA, xi[c])
        rx, rp = M.ratios(Xn[c], Pn[c], ref)
        e, lm = int(rx.argmax()), int(rp.argmax())
        print(f"chain {c}: max ratio X' {rx[e]:.3f} at e = {e}, preds {rp[lm]:.3f} at lm = {lm} (bound {C_BOUND})")
        assert rx[e] <= C_BOUND, (c, e, rx[e])
        assert rp[lm] <= C_BOUND, (c, lm, rp[lm])
        if wl:
            assert np.all(Pn[c][:4] == 0), "preds at lm < 4 under the weak-lensing kernel"
        if zero.any():
            s0 = np.abs(X[c]) + np.sqrt(2 * DELTA) * np.abs(xi[c])
            assert (np.abs(Xn[c] - plain[c])[zero] <= C_BOUND * 2.0 ** -52 * s0[zero]).all(), c
        worst = [max(worst[0], rx[e]), max(worst[1], rp[lm])]
    if independence:
        for c in range(C):
            Xa, Pa = _run(plan, X[c : c + 1], data, invcov, kernel, T, ncplx, n64, chain0=CHAIN0 + c)
            assert np.array_equal(Xa[0].view(np.float64), Xn[c].view(np.float64)), c
            assert np.array_equal(Pa[0].view(np.float64), Pn[c].view(np.float64)), c
    return worst


@pytest.mark.parametrize("fc", FACTORS, ids=factor_id)
@pytest.mark.parametrize("case", list(CASES), ids=[case_id(c, k) for c, k in CASES.items()])
def test_fused_step_per_element(case, fc):
    """C = 3 chains on a plan of max_chains = 5, non-zero chain0 / it / iter_dev; factor rows: an orthogonal array, so every
    level of (weak-lensing kernel, vector T, complex invcov, complex noise, fp64 Box-Muller) meets every K and every level
    of every other factor"""
    plan, M = _plan_and_model(case, CASES[case], 5)
    rng = np.random.default_rng(1000 * list(CASES).index(case) + FACTORS.index(fc))
    wx, wp = _check(plan, M, 3, *fc, rng)
    print(f"K = {K_of(CASES[case])}: largest ratio X' {wx:.3f}, preds {wp:.3f}")


@pytest.mark.parametrize("wl", [0, 1], ids=["identity", "wl"])
@pytest.mark.parametrize("case,C", [((256, 2.0, 2, 1, 0), 16), ((256, 2.0, 2, 4, 0), 16), ((256, 2.0, 2, 2, 0), 3)],
                         ids=lambda v: case_id(v, FULL_SIZE[v]) if isinstance(v, tuple) else f"C{v}")
def test_fused_step_per_element_full_size(case, C, wl):
    """L = 256 (16 chains at N = 1: the configuration the README quotes a time for): the grid (blockIdx.y = chain, L^2 / 256
    workgroups), the tail and the 64-bit offsets; vector T, vector invcov, fp64 Box-Muller; every chain, every element"""
    plan, M = _plan_and_model(case, FULL_SIZE[case], C)
    rng = np.random.default_rng(case[3] + 10 * wl)
    wx, wp = _check(plan, M, C, wl, 1, 0, 0, 1, rng, independence=False)
    print(f"K = {K_of(FULL_SIZE[case])}: largest ratio X' {wx:.3f}, preds {wp:.3f}")


def test_cases_span_every_instantiation():
    """the ids above name K = 2, 3, 5, 9, 17 and 0, each at least twice"""
    ks = [K_of(k) for k in CASES.values()]
    assert all(ks.count(K) >= 2 for K in (0, 2, 3, 5, 9, 17))
