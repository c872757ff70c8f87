"""The cache policies of the ring-space MYULA step (csrc/mem_policy.h) change no result bit.

The kernels of the step issue the accesses of their once-used streams non-temporally; addresses, widths, arithmetic and
order are those of the default-policy instantiations.  A plan created with PXM_MEM_POLICY=0 launches the default-policy
instantiations (``mem_policy()`` is 0): the same steps on both plans must leave equal X', equal predictions and equal
workspaces -- every ring and harmonic array of the step, padding columns included.

plan (B = 2, J_min = 2)   what runs
L = 32                    the unpacked two-slab GEMM variants, the order-0 pole tasks of the Gram list, the r0 = 1 DFT body
L = 256                   the same plus the exact-length 511-point body and the 8-chunk Gram halves

Eight real-pair slots (16 real chains), vector T, fp64 Philox noise, a registered device iteration counter: the stock
update, i.e. the launch whose DFT kernel carries the policies."""
import contextlib
import io

import numpy as np
import pytest

from test_wavstep_host import DELTA, LMDA, MODE_REAL_PAIRS, states, thresholds

pytestmark = pytest.mark.gpu

SLOTS, SEED, CHAIN0, IT, W_IC = 8, 11, 6, 5, 0.04
DFT_BITS = 0xF  # bits of mem_policy() that belong to the fused phi-DFT step


def _plan(L, policy):
    from pxmcmc_amd import ops

    with pytest.MonkeyPatch.context() as mp:
        for k in ("PXM_DFT_NO_W", "PXM_DFT_PFA", "PXM_PFA_PASSES", "PXM_DFT_STOCK", "PXM_MEM_POLICY"):
            mp.delenv(k, raising=False)
        if not policy:
            mp.setenv("PXM_MEM_POLICY", "0")
        plan = ops.WavPlan(L, 2.0, 2, max_chains=SLOTS)
    return plan


def test_override_is_reported_and_selects_the_default_kernels():
    on, off = _plan(32, True), _plan(32, False)
    assert on.dft_stock() and off.dft_stock()
    assert off.mem_policy() == 0 and off.info()["mem_policy"] == 0
    m = on.mem_policy()
    assert m != 0, "this build gives no stream a policy: nothing for the override to select"
    assert m & ~0xFF == 0
    assert on.info() == {"exact_dft_scales": 0, "dft_stock": True, "mem_policy": m}
    # without the STOCK instantiation the DFT step has no policy kernel: its bits are not reported
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PXM_DFT_STOCK", "0")
        mp.delenv("PXM_MEM_POLICY", raising=False)
        from pxmcmc_amd import ops

        generic = ops.WavPlan(32, 2.0, 2, max_chains=SLOTS)
    assert not generic.dft_stock()
    assert generic.mem_policy() == m & ~DFT_BITS


@pytest.mark.parametrize("L,steps", [(32, 3), (256, 1)])
def test_ring_steps_equal_the_default_policy_kernels(L, steps):
    import torch

    from pxmcmc_amd import ops

    assert ops.dft_step_is_stock(("X", "T", "iter_dev"), MODE_REAL_PAIRS, CHAIN0)
    plans = [_plan(L, True), _plan(L, False)]
    assert plans[0].mem_policy() != 0 and plans[1].mem_policy() == 0
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
        for step in range(steps):
            out = [torch.full_like(X0, complex(np.nan, np.nan)) for _ in plans]
            for p, x, o in zip(plans, X, out):
                p.ring_step(x, W_IC, Td, DELTA, LMDA, out=o, seed=SEED, chain0=CHAIN0, it=IT, pairs=True, noise64=True)
            ws = [p.workspace_read() for p in plans]  # (before ring_preds: the arrays as the step left them)
            preds = [p.ring_preds(SLOTS) for p in plans]
            for p in plans:
                assert p.status() == 0
            assert not torch.isnan(out[0].real).any() and not torch.isnan(out[0].imag).any(), "an element of X' was not written"
            assert not torch.equal(out[0], X[0])
            assert torch.equal(out[0], out[1]), f"X' differs after step {step + 1}"
            assert torch.equal(preds[0], preds[1]), f"predictions differ after step {step + 1}"
            assert ws[0].numel() > 2 * SLOTS * P and bool(torch.isfinite(ws[0]).all())
            # (bit patterns: equal compares -0.0 and 0.0 as equal)
            assert torch.equal(ws[0].view(torch.int64), ws[1].view(torch.int64)), f"ring / harmonic arrays differ after step {step + 1}"
            X = out
        assert [int(c.t.item()) for c in cnts] == [3 + steps, 3 + steps]
    finally:
        for c in cnts:
            c.close()


def _engine(L, use_graph):
    """a MYULA sampler of 2 SLOTS real chains from chain 6, its engine started at iteration 0, the policies on"""
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams
    from pxmcmc_amd.prior import S2_Wavelets_L1

    lmda, sigma, C = 1e-3, 0.05, 2 * SLOTS
    rng = np.random.default_rng(7)
    data = rng.normal(size=L * (2 * L - 1))
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("PXM_DFT_STOCK", raising=False)
        mp.delenv("PXM_MEM_POLICY", raising=False)
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
    assert s._pair_plan.dft_stock() and s._pair_plan.mem_policy() != 0
    assert (s._eng["graph"] is not None) == use_graph, s._eng["graph_error"]
    return s


def test_graph_replay_equals_eager_stepping():
    """the samplers' stepping engine at L = 32 with the policies on: replayed from its captured graphs and launched eagerly"""
    import torch

    pair = [_engine(32, True), _engine(32, False)]
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
