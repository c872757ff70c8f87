"""One fused wavelet step (WavPlan.ring_step / image_step / gradg_step) on the GPU against the extended-precision model of
tests/test_wavstep_host.py, element by element, through every noise and update branch of the shared epilogue
(csrc/update.h) in every phi-DFT unit that carries it:

    |got - model| <= d E_g + sqrt(2 d) E_w max(1, |w|) + K eps (|(1 - r) X| + |r soft| + |d g| + |sqrt(2 d) w|),   K = 11

g: the device's own UNFUSED gradient, synthesis_adjoint(residual_grad(preds, data, invcov)) of the same plan (ring_step:
preds = synthesis(X), invcov = the uniform weight); E_g = 1e-11 max|g|; data and preds have the scale of X, and max|g| <= G_MAX
is asserted: the scale at which tests/test_wavstep_host.py shows which errors the bound rejects.  w and E_w per noise source:

    injected   the injected array, E_w = 0
    philox32   ops.randn(..., noise64=False) at the same (seed, global chain, it + it_dev), E_w = 0
    philox64   oracle/philox.py through ``deviates`` (which chain, which member of the pair, which element index), E_w = 1e-13

plan                        unit reached by the grouped rings -> X' -> rings launch
L = 128, B = 2, J_min = 2   Bluestein pair unit at band-limits 4 ... 128 (ring lengths 7 ... 255): the instantiations with 8, 4 and 2
                            rings per wave pair (R0 = 1, 2, 4)
L = 192, B = 2, J_min = 2   the same plus its 1-ring-per-wave-pair instantiation (R0 = 8) on the two 383-point scales: the default
                            body of every plan with 128 < L < 256
L = 256, B = 2, J_min = 2   the same plus the exact-length unit on the two 511-point scales (exact_dft_scales() == 2): the
                            bits-first LDS-table form (pairs, even chain0, philox64), px_noise_philox_tabs (every other
                            philox64 case) and the f32 form
L = 260, B = 2, J_min = 2   the four-wave unit on the 519-point scales
L = 16, PXM_DFT_NO_W=1      the radix-2 unit's epilogue

Every case: two-slot plan, chain0 6 or 7, it = 5 and a registered device counter of 3 (ring_step advances the counter before it
reads it: it sees 5 + 4), vector T or T_scalar, NaN-filled output, plan.status() == 0 afterwards.  Complex-mode elements with
|X| within a few ulp of T would be left out; the inputs leave out none, and the cap of 1e-4 is asserted.

Largest |got - model| / bound observed on the MI355X, per plan: DESIGN.md section 16b."""
import functools
import zlib

import numpy as np
import pytest

from test_wavstep_host import (DELTA, E_G_REL, E_W_F64, EXCLUDE_CAP, G_MAX, LMDA, MODE_CPLX_NOISE, MODE_IDS, MODE_REAL_NOISE,
                               MODE_REAL_PAIRS, MODES, T_SCALAR, X_SCALE, deviates, excluded, injected, ratios, states, step_bound,
                               step_model, thresholds)

pytestmark = pytest.mark.gpu

SEED, IT, IT_DEV = 11, 5, 3
PLANS = {"L128": (128, 2.0, 2, {}), "L192": (192, 2.0, 2, {}), "L256": (256, 2.0, 2, {}), "L260": (260, 2.0, 2, {}), "L16radix2": (16, 2.0, 2, {"PXM_DFT_NO_W": "1"})}
STEPS = ("ring", "image", "gradg")
NOISES = ("injected", "philox32", "philox64")


@pytest.fixture(scope="module")
def plans():
    """name -> (plan, its registered iteration counter, fixed data / preds / invcov on the device), made on first use"""
    import torch

    from pxmcmc_amd import ops

    made = {}

    def get(name):
        if name not in made:
            L, B, J_min, env = PLANS[name]
            with pytest.MonkeyPatch.context() as mp:
                for k in ("PXM_DFT_NO_W", "PXM_DFT_PFA", "PXM_PFA_PASSES"):
                    mp.delenv(k, raising=False)
                for k, v in env.items():
                    mp.setenv(k, v)
                plan = ops.WavPlan(L, B, J_min, max_chains=2)
            rng = np.random.default_rng(L)
            P = plan.npix
            fixed = dict(
                # (the scale of the states: the gradient stays within G_MAX, where the host tests show what the bound rejects)
                data=ops.as_device(X_SCALE * (rng.normal(size=P) + 1j * rng.normal(size=P)), torch.complex128),
                preds=ops.as_device(X_SCALE * (rng.normal(size=(2, P)) + 1j * rng.normal(size=(2, P))), torch.complex128),
                invcov=ops.as_device(4.0 * (1 + 0.3 * np.cos(np.arange(P) * 0.01)), torch.float64),
            )
            made[name] = (plan, ops.IterCounter(plan, 0), fixed)
        return made[name]

    yield get
    for _, cnt, _ in made.values():
        cnt.close()


@functools.lru_cache(maxsize=8)
def _oracle_deviates(mode, chain0, N, it_eff):
    return deviates(mode, SEED, chain0, 2, np.arange(N), it_eff, 0, 64)


def _device_f32_deviates(mode, chain0, live, N, it_eff):
    from pxmcmc_amd import ops

    if mode == MODE_REAL_PAIRS:
        r = ops.randn(N, C_=2 * live, seed=SEED, chain0=chain0, it=it_eff, noise64=False).cpu().numpy()
        return r[0::2] + 1j * r[1::2]
    r = ops.randn(N, C_=live, complex_=mode == MODE_CPLX_NOISE, seed=SEED, chain0=chain0, it=it_eff, noise64=False).cpu().numpy()
    return r.reshape(live, N) + 0j


def _run_case(plans, name, step, mode, noise, chain0, vecT, live=2, odd=False):
    """one step against the model; returns the largest |got - model| / bound"""
    import torch

    from pxmcmc_amd import ops

    plan, cnt, fx = plans(name)
    N, P, pairs = plan.ncoefs, plan.npix, mode == MODE_REAL_PAIRS
    rng = np.random.default_rng(zlib.crc32(repr((name, step, mode, noise, chain0, vecT, live, odd)).encode()))
    T = thresholds(rng, N) if vecT else T_SCALAR
    X = states(rng, live, N, mode, T)
    if odd:  # an odd number of real chains: the last slot's partner is a copy that the samplers discard (MYULA._pack)
        assert pairs
        X[-1] = X[-1].real * (1 + 1j)
    Xd = ops.as_device(X, torch.complex128)
    Td = ops.as_device(T, torch.float64) if vecT else T_SCALAR
    data, preds, invcov = fx["data"], fx["preds"][:live].contiguous(), fx["invcov"]
    # the unfused gradient first: the transforms use the workspace that carries the rings of the fused steps
    if step == "ring":
        w_ic = complex(0.04) if pairs else complex(0.04, -0.0035)  # (a weight that keeps w S^H S X within G_MAX)
        ic = torch.full((P,), w_ic if not pairs else 0.04, dtype=torch.float64 if pairs else torch.complex128, device=Xd.device)
        g = plan.synthesis_adjoint(ops.residual_grad(plan.synthesis(Xd), data, ic))
    else:
        g = plan.synthesis_adjoint(ops.residual_grad(preds, data, invcov))
    g = g.cpu().numpy().reshape(live, N)
    assert 0 < np.abs(g).max() <= G_MAX
    it_eff = IT + IT_DEV + (1 if step == "ring" else 0)
    kw = dict(seed=SEED, chain0=chain0, it=IT, pairs=pairs, noise_complex=mode == MODE_CPLX_NOISE)
    E_w = 0.0
    if noise == "injected":
        w = injected(rng, live, N, mode)
        if pairs:
            kw["noise"] = ops.as_device(np.stack([w.real, w.imag], axis=1).reshape(2 * live, N), torch.float64)
        else:
            kw["noise"] = ops.as_device(w.real, torch.float64) if mode == MODE_REAL_NOISE else ops.as_device(w, torch.complex128)
    elif noise == "philox32":
        w = _device_f32_deviates(mode, chain0, live, N, it_eff)
        kw["noise64"] = False
    else:
        w, E_w = _oracle_deviates(mode, chain0, N, it_eff)[:live], E_W_F64
        kw["noise64"] = True
    cnt.set(IT_DEV)
    out = torch.full_like(Xd, complex(np.nan, np.nan))
    if step == "ring":
        plan.ring_set_data(data)
        plan.ring_init(Xd)
        plan.ring_step(Xd, w_ic, Td, DELTA, LMDA, out=out, **kw)
    elif step == "image":
        plan.image_init(preds, data, invcov)
        plan.image_step(Xd, data, invcov, Td, DELTA, LMDA, out=out, **kw)
    else:
        plan.gradg_step(Xd, preds, data, invcov, Td, DELTA, LMDA, out=out, **kw)
    assert plan.status() == 0
    assert int(cnt.t.item()) == IT_DEV + (1 if step == "ring" else 0)
    got = out.cpu().numpy().reshape(live, N)
    assert not np.isnan(got.view(np.float64)).any(), "an element of X' was not written"
    skip = excluded(X, T, mode)
    assert skip.mean() <= EXCLUDE_CAP
    model = step_model(X, T, DELTA, LMDA, g, w, mode)
    bound = step_bound(X, T, DELTA, LMDA, g, w, mode, E_G_REL * np.abs(g).max(), E_w)
    q = ratios(got, model, bound, mode, skip)
    e = np.unravel_index(int(q.argmax()), q.shape)
    print(f"RATIO {name} {step} {MODE_IDS[mode]} {noise} chain0={chain0} {'Tvec' if vecT else 'Tscalar'} live={live} odd={int(odd)}: "
          f"{q.max():.4f} at slot {e[0]}, element {e[1]}; excluded {int(skip.sum())}; max|g| {np.abs(g).max():.1f}")
    assert q.max() <= 1.0, (e, q.max())
    return float(q.max())


@pytest.mark.parametrize("vecT", [True, False], ids=["Tvec", "Tscalar"])
@pytest.mark.parametrize("chain0", [6, 7], ids=["chain6", "chain7"])
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS.get)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("name", ["L128", "L16radix2"])
def test_step_per_element_full_cross(plans, name, step, mode, noise, chain0, vecT):
    """the Bluestein pair unit (its 8-, 4- and 2-rings-per-wave-pair instantiations in one grouped launch) and the radix-2 unit:
    the whole cross product of step, mode, noise source, chain0 parity and T form"""
    _run_case(plans, name, step, mode, noise, chain0, vecT)


@pytest.mark.parametrize("vecT", [True, False], ids=["Tvec", "Tscalar"])
@pytest.mark.parametrize("chain0", [6, 7], ids=["chain6", "chain7"])
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS.get)
def test_ring_step_per_element_one_ring_per_wave_pair(plans, mode, noise, chain0, vecT):
    """L = 192: the two 383-point scales (256 < n <= 512) go through the pair unit's R0 = 8 instantiation, one ring per wave pair,
    whose element stride 8 R0 and ring tail differ from the smaller instantiations"""
    assert plans("L192")[0].exact_dft_scales() == 0
    _run_case(plans, "L192", "ring", mode, noise, chain0, vecT)


@pytest.mark.parametrize("vecT", [True, False], ids=["Tvec", "Tscalar"])
@pytest.mark.parametrize("chain0", [6, 7], ids=["chain6", "chain7"])
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS.get)
def test_ring_step_per_element_exact_length_unit(plans, mode, noise, chain0, vecT):
    """L = 256: the two 511-point scales go through the exact-length unit; pairs + philox64 + chain0 = 6 is its bits-first LDS-table
    form, every other philox64 case px_noise_philox_tabs (chain0 = 7 in pair mode: the two-trip loop that picks z0 / z1 by chain & 1),
    philox32 the f32 form"""
    assert plans("L256")[0].exact_dft_scales() == 2
    _run_case(plans, "L256", "ring", mode, noise, chain0, vecT)


@pytest.mark.parametrize("vecT", [True, False], ids=["Tvec", "Tscalar"])
@pytest.mark.parametrize("chain0", [6, 7], ids=["chain6", "chain7"])
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS.get)
def test_ring_step_per_element_four_wave_unit(plans, mode, noise, chain0, vecT):
    """L = 260: the 519-point scales go through the four-wave unit, whose epilogue has one noise path per precision"""
    _run_case(plans, "L260", "ring", mode, noise, chain0, vecT)


@pytest.mark.parametrize("chain0", [6, 7], ids=["chain6", "chain7"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS.get)
@pytest.mark.parametrize("step", ["image", "gradg"])
@pytest.mark.parametrize("name", ["L192", "L256", "L260"])
def test_image_and_gradg_step_per_element_large_units(plans, name, step, mode, chain0):
    """the same epilogues entered from the image-space steps: one noise source (philox64), T form alternating"""
    _run_case(plans, name, step, mode, "philox64", chain0, bool((mode + chain0) & 1))


@pytest.mark.parametrize("shape", ["one_slot_pairs", "one_slot_cplx", "odd_real_chains"])
@pytest.mark.parametrize("name", list(PLANS))
def test_fewer_live_chains_than_slots(plans, name, shape):
    """one live slot in the two-slot plan (pairs and complex noise) at chain0 = 7: the second slot's waves must write nothing.
    odd_real_chains: the state as the samplers pack three real chains into two slots (the last partner a discarded copy); the step
    takes no real-chain count, so this runs the two-slot device code on that input -- the odd count itself is the sampler test's"""
    if shape == "one_slot_pairs":
        _run_case(plans, name, "ring", MODE_REAL_PAIRS, "philox64", 7, True, live=1)
    elif shape == "one_slot_cplx":
        _run_case(plans, name, "ring", MODE_CPLX_NOISE, "philox64", 7, False, live=1)
    else:
        _run_case(plans, name, "ring", MODE_REAL_PAIRS, "philox64", 7, False, live=2, odd=True)


def test_sampler_pair_layout_at_an_odd_chain_offset():
    """MYULA in the real-pair layout with 3 chains at chain_offset = 3 -- what rank 1 of a run sharded 3 chains per rank steps:
    odd chain0 in pair mode, an odd number of real chains -- equals chains 3 ... 5 of the 6-chain batch"""
    import contextlib
    import io

    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams
    from pxmcmc_amd.prior import S2_Wavelets_L1

    L, B, J_min = 16, 2, 2
    rng = np.random.default_rng(4)
    data = rng.normal(size=L * (2 * L - 1))
    lmda, delta = 1e-3, 5e-4
    op = SphericalWaveletTransformOperator(data, 0.1, "synthesis", L, B, J_min, max_chains=6)
    reg = S2_Wavelets_L1("synthesis", None, None, lmda, L=L, B=B, J_min=J_min)
    p = PxMCMCParams(lmda=lmda, delta=delta, nsamples=4, nburn=1, ngap=1, verbosity=0)
    X0 = np.zeros(op.nparams)
    runs = []
    for kw in (dict(nchains=6), dict(nchains=3, chain_offset=3)):
        s = MYULA(op, reg, p, seed=7, **kw)
        with contextlib.redirect_stdout(io.StringIO()):
            s.run(start_point=X0)
        assert s._pairs, "the sampler left the real-pair layout"
        runs.append(s.chain)
    assert runs[0].shape == (6, 4, op.nparams) and runs[1].shape == (3, 4, op.nparams)
    np.testing.assert_allclose(runs[1], runs[0][3:6], rtol=1e-12, atol=1e-14)
    assert np.abs(runs[0][3] - runs[0][4]).max() > 1e-6
