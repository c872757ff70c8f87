"""The STOCK instantiations of the fused rings -> X' -> rings kernels of the phi-DFT pair unit (csrc/dft_wave.hip, dft_pfa.h,
update.h: px_stock_update4) against the generic ones, to the bit.

STOCK removes branches the stock MYULA update never takes and reorders work on independent elements; the operations on one
element and their order are the same, so the two must agree exactly.  A plan created with PXM_DFT_STOCK=0 keeps every launch
on the generic kernels (``dft_stock()`` is False): the same steps on both plans must give equal X' and equal predictions.

plan (B = 2, J_min = 2)   bodies of the grouped launch
L = 128                   Bluestein, 8 / 4 / 2 rings per wave pair (r0 = 1, 2, 4)
L = 192                   the same plus one ring per wave pair (r0 = 8) on the two 383-point scales
L = 256                   the same plus the exact-length body on the two 511-point scales

Five real-pair slots: the second chain group of every body has one live slot of four.  chain0 = 6, vector T, fp64 noise,
a registered device iteration counter -- the stock conjunction of tests/test_dft_stock_host.py.  That the generic kernels
compute the right thing in every mode is tests/test_gpu_wavstep.py."""
import contextlib
import io

import numpy as np
import pytest

from test_wavstep_host import DELTA, LMDA, MODE_REAL_PAIRS, states, thresholds

pytestmark = pytest.mark.gpu

SLOTS, SEED, CHAIN0, IT, W_IC = 5, 11, 6, 5, 0.04


def _plan(L, stock):
    from pxmcmc_amd import ops

    with pytest.MonkeyPatch.context() as mp:
        for k in ("PXM_DFT_NO_W", "PXM_DFT_PFA", "PXM_PFA_PASSES", "PXM_DFT_STOCK"):
            mp.delenv(k, raising=False)
        if not stock:
            mp.setenv("PXM_DFT_STOCK", "0")
        plan = ops.WavPlan(L, 2.0, 2, max_chains=SLOTS)
    assert plan.dft_stock() == stock
    return plan


@pytest.mark.parametrize("L", [128, 192, 256])
def test_three_ring_steps_equal_the_generic_kernels(L):
    import torch

    from pxmcmc_amd import ops

    assert ops.dft_step_is_stock(("X", "T", "iter_dev"), MODE_REAL_PAIRS, CHAIN0)
    plans = [_plan(L, True), _plan(L, False)]
    assert plans[0].exact_dft_scales() == (2 if L == 256 else 0)
    N, P = plans[0].ncoefs, plans[0].npix
    rng = np.random.default_rng(L)
    T = thresholds(rng, N)
    Td = ops.as_device(T, torch.float64)
    X0 = ops.as_device(states(rng, SLOTS, N, MODE_REAL_PAIRS, T), torch.complex128)
    d = 1e-2 * rng.normal(size=P)
    data = ops.as_device(d + 1j * d, torch.complex128)  # (both chains of a slot see the same real data)
    cnts = [ops.IterCounter(p, 3) for p in plans]
    try:
        X = [X0, X0.clone()]
        for p in plans:
            p.ring_set_data(data)
        for p, x in zip(plans, X):
            p.ring_init(x)
        for step in range(3):
            out = [torch.full_like(X0, complex(np.nan, np.nan)) for _ in plans]
            for p, x, o in zip(plans, X, out):
                p.ring_step(x, W_IC, Td, DELTA, LMDA, out=o, seed=SEED, chain0=CHAIN0, it=IT, pairs=True, noise64=True)
            preds = [p.ring_preds(SLOTS) for p in plans]
            for p in plans:
                assert p.status() == 0
            assert not torch.isnan(out[0].real).any() and not torch.isnan(out[0].imag).any(), "an element of X' was not written"
            assert not torch.equal(out[0], X[0])
            assert torch.equal(out[0], out[1]), f"X' differs after step {step + 1}"
            assert torch.equal(preds[0], preds[1]), f"predictions differ after step {step + 1}"
            X = out
        assert [int(c.t.item()) for c in cnts] == [6, 6]
    finally:
        for c in cnts:
            c.close()


def _engine(L, stock, use_graph):
    """a MYULA sampler of 2 SLOTS real chains from chain 6, its engine started at iteration 0"""
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams
    from pxmcmc_amd.prior import S2_Wavelets_L1

    lmda, sigma, C = 1e-3, 0.05, 2 * SLOTS
    rng = np.random.default_rng(7)
    data = rng.normal(size=L * (2 * L - 1))
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("PXM_DFT_STOCK", raising=False)
        if not stock:
            mp.setenv("PXM_DFT_STOCK", "0")
        op = SphericalWaveletTransformOperator(data, sigma, "synthesis", L, 2.0, 2, max_chains=C)
        reg = S2_Wavelets_L1("synthesis", op.transform.inverse, op.transform.inverse_adjoint, lmda, L=L, B=2.0, J_min=2)
        params = PxMCMCParams(lmda=lmda, delta=1e-6, mu=1.0, nsamples=1, nburn=0, ngap=1, verbosity=0)
        s = MYULA(op, reg, params, nchains=C, rng="philox", seed=2, chain_offset=CHAIN0, use_graph=use_graph, noise_bits=64)
        s._prepare()
        assert s._fused_wav
        with contextlib.redirect_stdout(io.StringIO()):
            X, preds = s._initial_sample(1e-3 * rng.normal(size=op.nparams))
        assert s._pairs_ok(X)
        s._pairs_start()
        s._engine_start(X, preds, 0)
    assert s._pair_plan.dft_stock() == stock
    assert (s._eng["graph"] is not None) == use_graph, s._eng["graph_error"]
    return s


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_engine_steps_equal_the_generic_kernels(use_graph):
    """the samplers' stepping engine at L = 256, launched eagerly and replayed from its captured graphs"""
    import torch

    pair = [_engine(256, True, use_graph), _engine(256, False, use_graph)]
    try:
        for k in (2, 1, 3):
            got = []
            for s in pair:
                s._engine_advance(k)
                X, preds = s._engine_state()
                got.append((X.clone(), preds.clone()))
            assert bool(torch.isfinite(got[0][0].real).all())
            assert torch.equal(got[0][0], got[1][0]), "X differs"
            assert torch.equal(got[0][1], got[1][1]), "predictions differ"
    finally:
        for s in pair:
            s._engine_stop()
