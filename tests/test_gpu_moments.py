"""Streaming posterior summaries on the device: k_moments_update element by element against the
long-double model of tests/test_moments_host.py, best-sample tracking, k_moments_finalize against the numpy statements,
graph capture, the samplers' ``summary=`` keyword and a two-rank merge."""
import contextlib
import io
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT, golden
from test_moments_host import C0_MEASURED, error_scales, moment_columns, two_pass_ld

pytestmark = pytest.mark.gpu

BOUND = 4 * C0_MEASURED  # of the per-element scales S_mean / S_m2 (tests/test_moments_host.py)
CMAX = 5  # every buffer of the kernel sweep is allocated for 5 chains
WORST = {"mean": 0.0, "m2": 0.0}  # largest ratios seen by this module's checks (printed by the last test)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _check_against_long_double(mean, m2, samples, what):
    """mean / m2 [m] of one chain against the long-double two-pass values of its samples [n, m], element by element"""
    mean_ld, m2_ld = two_pass_ld(samples)
    s_mean, s_m2 = error_scales(samples)
    for name, got, ext, s in (("mean", mean, mean_ld, s_mean), ("m2", m2, m2_ld, s_m2)):
        err = np.abs(np.asarray(got).astype(np.longdouble) - ext).astype(np.float64)
        assert np.all(err[s == 0] == 0), (what, name)
        r = float(np.max(np.where(s > 0, err / np.where(s > 0, s, 1.0), 0.0)))
        WORST[name] = max(WORST[name], r)
        assert r <= BOUND, (what, name, r, BOUND)


def _samples(T, C, m, cplx, seed, kind0=None):
    """T sample batches [T, C, m] of real components; chain c draws moment_columns with its own seed, its column kinds
    shifted by c (kind0 given: the same kinds in every chain, so that a constant column is constant in all of them)"""
    x = np.stack([moment_columns(T, m, seed + c, kind0) for c in range(C)], axis=1)
    return np.ascontiguousarray(x)


def _batch(x_t, cplx):
    """one batch [C, m] of real components -> the device tensor update() takes ([C, m] float64 or [C, m / 2] complex128)"""
    import torch

    t = _dev(x_t)
    return torch.view_as_complex(t.reshape(t.shape[0], -1, 2)) if cplx else t


# ---- the update kernel, element by element ----------------------------------------------------------------------------------
MODES = ("real", "components", "realparts")


def _sweep_case(m, C, mode, best, nupd):
    """nupd updates of every chain on top of per-chain start counts built by mixed masks, on buffers allocated for CMAX chains
    whose rows beyond C are prefilled with NaN; then an all-off update.  Every element of mean / m2 within 4 C0 of the
    long-double model, best_x / best_logpi bit-equal to the expected sample.  ``mode``: "real" float64 [C, m]; "components" a
    complex128 [C, m] state passed as its 2 m real components; "realparts" complex128 [C, m] whose real parts are
    accumulated (x_stride 2, complex logpi)."""
    import torch

    from pxmcmc_amd import ops

    mm = 2 * m if mode == "components" else m  # accumulated components per chain
    start = [0, 1, 2, 3, 5][:C]  # samples chain c holds before the nupd updates: masked-in for the first start[c] rounds
    T = max(start) + nupd
    x = _samples(T, C, mm, False, seed=m + nupd)
    rng = np.random.default_rng([m, C, nupd])
    lp = rng.normal(size=(T, C))
    if T >= 3:
        lp[T - 1, 0] = lp[T - 3, 0] = 9.0  # a tie at the top of chain 0: the earlier update keeps it
    count = torch.full((CMAX,), -7, dtype=torch.int64, device="cuda")
    mean = torch.full((CMAX, mm), float("nan"), dtype=torch.float64, device="cuda")
    m2, best_x = mean.clone(), mean.clone()
    best_lp = torch.full((CMAX,), float("nan"), dtype=torch.float64, device="cuda")
    count[:C], mean[:C], m2[:C], best_x[:C], best_lp[:C] = 0, 0.0, 0.0, 0.0, -np.inf
    if mode == "realparts":
        xbuf = torch.full((CMAX, m), float("nan"), dtype=torch.complex128, device="cuda")
    else:
        xbuf = torch.full((CMAX, mm), float("nan"), dtype=torch.float64, device="cuda")
    kw = dict(best_logpi=best_lp[:C], best_x=best_x[:C]) if best else {}
    seen = [[] for _ in range(C)]
    want_lp, want_x = [-np.inf] * C, [np.zeros(mm) for _ in range(C)]
    for t in range(T):
        if t < max(start):
            on = [int(t < start[c]) for c in range(C)]
            mask = _dev(np.array(on, dtype=np.int32))
        else:
            on = [1] * C
            mask = None if (t - max(start)) % 2 == 0 else torch.ones(C, dtype=torch.int32, device="cuda")
        if mode == "realparts":
            xbuf[:C] = _dev(x[t] + 1j * rng.normal(size=(C, m)))
            logpi = _dev(lp[t] + 1j * rng.normal(size=C))
        else:
            xbuf[:C] = _dev(x[t])
            logpi = _dev(lp[t])
        ops.moments_update(xbuf[:C], count[:C], mean[:C], m2[:C], mask=mask, logpi=logpi if best else None, **kw)
        for c in range(C):
            if on[c]:
                seen[c].append(x[t, c])
                if lp[t, c] > want_lp[c]:
                    want_lp[c], want_x[c] = lp[t, c], x[t, c]
    state = (count, mean, m2, best_x, best_lp)
    before = [a.clone() for a in state]
    ops.moments_update(xbuf[:C], count[:C], mean[:C], m2[:C], mask=torch.zeros(C, dtype=torch.int32, device="cuda"),
                       logpi=logpi if best else None, **kw)
    for a, b in zip(before, state):  # all-off: nothing is written (NaN rows compared as bits)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    cnt, mean_h, m2_h, bx_h, bl_h = (a.cpu().numpy() for a in state)
    what = (m, C, mode, best, nupd)
    assert list(cnt[:C]) == [start[c] + nupd for c in range(C)] and np.all(cnt[C:] == -7), what
    assert np.isnan(mean_h[C:]).all() and np.isnan(m2_h[C:]).all() and np.isnan(bx_h[C:]).all() and np.isnan(bl_h[C:]).all(), what
    for c in range(C):
        _check_against_long_double(mean_h[c], m2_h[c], np.stack(seen[c]), what + (c,))
        if best:
            assert bl_h[c] == want_lp[c], what + (c,)
            np.testing.assert_array_equal(bx_h[c], want_x[c], err_msg=str(what + (c,)))
        else:
            assert bl_h[c] == -np.inf and not bx_h[c].any(), what + (c,)


@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 257, 1025])
def test_update_kernel_elementwise(m, C):
    """every instantiation <x_stride 1 | 2, best | no best>, 1 / 2 / 7 updates; m = 1025 runs the 4-deep body in the
    "components" mode (2050 components: one workgroup, one unrolled pass and a remainder)"""
    for mode in MODES:
        for best in (False, True):
            for nupd in (1, 2, 7):
                _sweep_case(m, C, mode, best, nupd)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [4099, 8193])
def test_update_kernel_unrolled_body_elementwise(m, mode):
    """rows long enough for the 4-deep grid-stride body on several workgroups (the path that covers all but the last pairs of
    a row at the benchmark size), with a remainder behind it, odd m so that rows 1 of the 3 chains start off a 16-byte
    boundary: m = 4099 is 2 workgroups, one unrolled pass, one remainder pair or none; m = 8193 is 4 workgroups and a scalar
    tail; "components" doubles both"""
    for best in (False, True):
        _sweep_case(m, 3, mode, best, 2)


def test_real_parts_of_a_complex_batch():
    """x_stride 2: a summary of a real-valued quantity fed complex128 samples accumulates their real parts (the samplers'
    real ``chain`` of a complex128 state); bit-equal to the update on the extracted real parts, odd m and odd rows included"""
    import torch

    from pxmcmc_amd.uncertainty import PosteriorSummary

    C, n = 3, 131
    rng = np.random.default_rng(0)
    a, b = PosteriorSummary(C, n, False), PosteriorSummary(C, n, False)
    for t in range(3):
        z = _dev(rng.normal(size=(C, n)) + 1j * rng.normal(size=(C, n)))
        lp = _dev(rng.normal(size=C) + 1j * rng.normal(size=C))
        a.update(z, logpi=lp)
        b.update(z.real.contiguous(), logpi=lp.real.contiguous())
    for k, v in a.to_host().items():
        np.testing.assert_array_equal(v, b.to_host()[k])
    assert a.best_sample().dtype == torch.float64 and a.counts.tolist() == [3, 3, 3]


def test_chains_are_independent():
    """each chain's result is bit-equal to the same chain updated alone"""
    from pxmcmc_amd.uncertainty import PosteriorSummary

    C, m, T = 5, 257, 4
    x = _samples(T, C, m, False, seed=3)
    lp = np.random.default_rng(1).normal(size=(T, C))
    masks = np.array([[1, 0, 1, 1, 0], [1, 1, 1, 0, 0], [0, 1, 1, 1, 1], [1, 1, 0, 1, 1]], dtype=np.int32)
    full = PosteriorSummary(C, m, False)
    for t in range(T):
        full.update(_dev(x[t]), logpi=_dev(lp[t]), mask=masks[t])
    whole = full.to_host()
    for c in range(C):
        alone = PosteriorSummary(1, m, False)
        for t in range(T):
            if masks[t, c]:
                alone.update(_dev(x[t, c : c + 1]), logpi=_dev(lp[t, c : c + 1]))
        for k, v in alone.to_host().items():
            np.testing.assert_array_equal(v[0], whole[k][c], err_msg=f"{k} of chain {c}")


# ---- best sample -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
def test_best_sample_tracking(cplx):
    """best_x is the masked-in sample of largest logpi, bit for bit; ties keep the first; NaN never wins"""
    from pxmcmc_amd.uncertainty import PosteriorSummary

    C, n, T = 4, 65, 9
    rng = np.random.default_rng(5)
    x = rng.normal(size=(T, C, n)) + (1j * rng.normal(size=(T, C, n)) if cplx else 0)
    lp = rng.normal(size=(T, C))
    lp[3, 0] = lp[1, 0] = 7.0  # a tie at the top of chain 0: update 1 keeps it
    lp[2, 1] = np.nan  # NaN in the middle of chain 1 ...
    lp[0, 2] = np.nan  # ... and as the first sample of chain 2
    lp[:, 3] = np.nan  # chain 3 never has a finite logpi: nothing is ever taken
    lp[5, 1] = 50.0  # the largest of chain 1, but masked out below
    masks = np.ones((T, C), dtype=np.int32)
    masks[5, 1] = 0
    masks[4] = [0, 1, 0, 1]
    s = PosteriorSummary(C, n, cplx)
    for t in range(T):
        s.update(_dev(x[t]), logpi=_dev(lp[t]), mask=None if masks[t].all() else masks[t])
    best, best_lp = s.best_sample().cpu().numpy(), s.best_logpi.cpu().numpy()
    for c in range(C):
        cur, arg = -np.inf, None
        for t in range(T):
            if masks[t, c] and lp[t, c] > cur:
                cur, arg = lp[t, c], t
        assert best_lp[c] == cur
        np.testing.assert_array_equal(best[c], x[arg, c] if arg is not None else np.zeros(n))
    assert best_lp[0] == 7.0 and np.array_equal(best[0], x[1, 0]) and best_lp[3] == -np.inf
    np.testing.assert_array_equal(s.counts.cpu().numpy(), masks.sum(axis=0))


def test_best_false_leaves_it_out():
    from pxmcmc_amd.uncertainty import PosteriorSummary

    s, ref = PosteriorSummary(2, 33, False, best=False), PosteriorSummary(2, 33, False)
    x = _samples(3, 2, 33, False, seed=9)
    for t in range(3):
        s.update(_dev(x[t]))
        ref.update(_dev(x[t]), logpi=_dev(np.zeros(2)))
    host = s.to_host()
    assert set(host) == {"count", "mean", "m2"} and s._best_x is None
    np.testing.assert_array_equal(host["mean"], ref.to_host()["mean"])
    np.testing.assert_array_equal(host["m2"], ref.to_host()["m2"])
    with pytest.raises(ValueError):
        s.best_sample()
    with pytest.raises(ValueError):
        ref.update(_dev(x[0]))  # best=True needs logpi


# ---- finalize ----------------------------------------------------------------------------------------------------------------
def _filled(C, m, n, cplx=False, seed=0):
    from pxmcmc_amd.uncertainty import PosteriorSummary

    s = PosteriorSummary(C, m, cplx, best=False)
    x = _samples(n, C, s.m, cplx, seed, kind0=0)
    for t in range(n):
        s.update(_batch(x[t], cplx))
    return s


@pytest.mark.parametrize("C,m,n", [(4, 257, 6), (2, 1, 2), (3, 70001, 3), (2, 65537, 3), (2, 262401, 3)])
def test_finalize_against_numpy(C, m, n):
    """pooled mean / variance and R-hat against pooled_np / rhat_np on the same accumulators (rtol 1e-13); max R-hat and the
    NaN count exact against numpy on the kernel's own R-hat array (70001 elements: more than one workgroup per stage; 65537:
    257 partials, a second trip of the second stage's loop; 262401: one element beyond the 1024 workgroups of the cap, a
    second trip of the element loop)"""
    from pxmcmc_amd import ops
    from pxmcmc_amd.uncertainty import pooled_np, rhat_np

    s = _filled(C, m, n, seed=C)
    h = s.to_host()
    pm, pv, rh, st = (t.cpu().numpy() for t in ops.moments_finalize(s._count, s._mean, s._m2))
    pm_np, pv_np = pooled_np(h["count"], h["mean"], h["m2"])
    np.testing.assert_allclose(pm, pm_np, rtol=1e-13, atol=0)
    np.testing.assert_allclose(pv, pv_np, rtol=1e-13, atol=0)
    np.testing.assert_allclose(rh, rhat_np(h["count"], h["mean"], h["m2"]), rtol=1e-13, atol=0, equal_nan=True)
    const = np.all(h["m2"] == 0, axis=0)
    assert np.isnan(rh[const]).all() and np.isfinite(rh[~const]).all()  # W == 0 on the constant columns only
    if m > 1:
        assert const.any() and not const.all()
    assert st[1] == np.isnan(rh).sum()
    assert (np.isnan(st[0]) and np.isnan(rh).all()) or st[0] == np.nanmax(rh)
    assert s.max_rhat()[1] == int(st[1])
    np.testing.assert_array_equal(s.rhat().cpu().numpy(), rh)
    np.testing.assert_array_equal(s.pooled_mean().cpu().numpy(), pm)
    np.testing.assert_array_equal(s.pooled_variance().cpu().numpy(), pv)


def test_finalize_complex_and_per_chain_read_out():
    s = _filled(3, 33, 5, cplx=True, seed=2)
    h = s.to_host()
    mean = s.mean().cpu().numpy()
    assert mean.dtype == np.complex128 and mean.shape == (3, 33)
    np.testing.assert_array_equal(mean.real, h["mean"][:, 0::2])
    np.testing.assert_array_equal(mean.imag, h["mean"][:, 1::2])
    var = s.variance().cpu().numpy()
    np.testing.assert_allclose(var, (h["m2"][:, 0::2] + h["m2"][:, 1::2]) / 4, rtol=1e-15)
    np.testing.assert_allclose(s.std().cpu().numpy(), np.sqrt(var), rtol=1e-15)
    assert s.rhat().shape == (66,) and s.pooled_mean().shape == (33,) and s.pooled_mean().is_complex()
    assert s.pooled_variance().shape == (33,) and not s.pooled_variance().is_complex()


def test_finalize_undefined_and_refused():
    """one chain taking part, one sample per chain: NaN; unequal counts: R-hat is refused with a message, the pooled moments
    are still available and exact against pooled_np"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError
    from pxmcmc_amd.uncertainty import PosteriorSummary, pooled_np

    s = PosteriorSummary(3, 40, False, best=False)
    x = _samples(4, 3, 40, False, seed=1)
    s.update(_dev(x[0]))
    pm, pv, rh, st = ops.moments_finalize(s._count, s._mean, s._m2)  # one sample per chain
    assert torch.isnan(rh).all() and torch.isnan(pv).sum() == 0 and list(st.cpu().numpy()[1:]) == [40.0]
    assert np.isnan(st.cpu().numpy()[0])
    s.update(_dev(x[1]), mask=[1, 0, 0])
    s.update(_dev(x[2]), mask=[1, 0, 1])
    with pytest.raises(PxmError, match="common sample count"):
        s.rhat()
    with pytest.raises(PxmError, match="common sample count"):
        s.max_rhat()
    h = s.to_host()
    pm_np, pv_np = pooled_np(h["count"], h["mean"], h["m2"])
    np.testing.assert_allclose(s.pooled_mean().cpu().numpy(), pm_np, rtol=1e-13)
    np.testing.assert_allclose(s.pooled_variance().cpu().numpy(), pv_np, rtol=1e-13)
    one = PosteriorSummary(3, 40, False, best=False)
    for t in range(3):
        one.update(_dev(x[t]), mask=[0, 1, 0])  # a single chain takes part: R-hat undefined, not an error
    assert torch.isnan(one.rhat()).all() and one.max_rhat()[1] == 40
    h = one.to_host()
    np.testing.assert_allclose(one.pooled_mean().cpu().numpy(), pooled_np(h["count"], h["mean"], h["m2"])[0], rtol=1e-13)
    np.testing.assert_array_equal(h["mean"][1], one.pooled_mean().cpu().numpy())  # the one chain's own mean


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_update_is_capturable():
    """one moments_update captured on static buffers and replayed three times, the input overwritten between replays,
    equals three eager updates bit for bit"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.uncertainty import PosteriorSummary

    C, m = 3, 1025
    x = _samples(4, C, m, False, seed=4)
    lp = np.random.default_rng(2).normal(size=(4, C))
    eager, graph = PosteriorSummary(C, m, False), PosteriorSummary(C, m, False)
    for t in range(1, 4):
        eager.update(_dev(x[t]), logpi=_dev(lp[t]))
    X, LP = _dev(x[0]), _dev(lp[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph.update(X, logpi=LP)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = PosteriorSummary(C, m, False)
    g = torch.cuda.CUDAGraph()
    with ops.capture_scope(), torch.cuda.graph(g):
        graph.update(X, logpi=LP)
    assert int(graph.counts.sum()) == 0  # capture does not execute
    for t in range(1, 4):
        X.copy_(_dev(x[t]))
        LP.copy_(_dev(lp[t]))
        g.replay()
    torch.cuda.synchronize()
    for k, v in eager.to_host().items():
        np.testing.assert_array_equal(graph.to_host()[k], v, err_msg=k)


# ---- samplers ----------------------------------------------------------------------------------------------------------------
L_, B_, JMIN_ = 16, 2, 0
PXMALA_SEED = 2  # chosen so that a save candidate of the PxMALA run below has an accepted and a rejected chain (asserted)


def _wavelet_problem(C, sig=0.1, lmda=1e-3):
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.prior import S2_Wavelets_L1

    data = np.random.default_rng(3).normal(size=L_ * (2 * L_ - 1))
    op = SphericalWaveletTransformOperator(data, sig, "synthesis", L_, B_, JMIN_, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, lmda, L=L_, B=B_, J_min=JMIN_)
    return op, reg


def _run(algo, C, summary, track=("logposterior", "L2", "prior", "chain"), use_graph=True, nsamples=12, cplx=False, seed=11,
         chain_offset=0, real_pairs=True):
    from pxmcmc_amd.mcmc import MYULA, SKROCK, PxMALA, PxMCMCParams

    if algo == "pxmala":  # step size of the G4 set-up (tests/golden/g4_pxmala.npz)
        lmda, delta, mu = (float(v) for v in golden("g4_pxmala.npz")["params"][:3])
        op, reg = _wavelet_problem(C, lmda=lmda * mu)
        p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, nsamples=nsamples, nburn=3, ngap=2, verbosity=0, track=list(track))
        s = PxMALA(op, reg, p, tune_delta=True, nchains=C, seed=seed, summary=summary, use_graph=use_graph, max_iter=400)
    else:
        op, reg = _wavelet_problem(C)
        kw = dict(lmda=1e-3, nsamples=nsamples, nburn=3, verbosity=0, track=list(track), complex=cplx)
        if algo == "myula":
            s = MYULA(op, reg, PxMCMCParams(delta=5e-4, ngap=2, **kw), nchains=C, seed=seed, summary=summary, use_graph=use_graph,
                      chain_offset=chain_offset, real_pairs=real_pairs)
        else:
            s = SKROCK(op, reg, PxMCMCParams(delta=2e-3, ngap=1, s=3, **kw), nchains=C, seed=seed, summary=summary,
                       use_graph=use_graph)
    start = np.zeros(op.nparams, dtype=complex if cplx else float)
    _quiet(s.run, start_point=start)
    return s, op


def _check_sampler_summary(s, op, nsaved):
    """the per-chain checks of a run with track including "chain" and summary=("state", "image")"""
    from pxmcmc_amd.uncertainty import chain_to_images, moments_np

    C = s.nchains
    st, im = s.summary["state"], s.summary["image"]
    assert list(st.counts.cpu().numpy()) == list(nsaved) and list(im.counts.cpu().numpy()) == list(nsaved)
    assert st.complex == bool(s.complex) and im.complex
    h = st.to_host()
    best, img_mean = st.best_sample().cpu().numpy(), im.mean().cpu().numpy()
    for c in range(C):
        n = int(nsaved[c])
        chain, logpi = s.chain[c][:n], s.logPi[c][:n]
        cnt, mean_np, m2_np = moments_np(chain)
        comp = chain.view(np.float64).reshape(n, -1) if np.iscomplexobj(chain) else chain
        s_mean, s_m2 = error_scales(comp)
        r_mean = float(np.max(np.abs(h["mean"][c] - mean_np) / np.where(s_mean > 0, s_mean, 1.0)))
        r_m2 = float(np.max(np.abs(h["m2"][c] - m2_np) / np.where(s_m2 > 0, s_m2, 1.0)))
        WORST["mean"], WORST["m2"] = max(WORST["mean"], r_mean), max(WORST["m2"], r_m2)
        assert cnt == n and r_mean <= BOUND and r_m2 <= BOUND, (c, r_mean, r_m2)
        ref = chain_to_images(chain, op.transform).mean(axis=0)
        assert np.abs(img_mean[c] - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max()), c
        np.testing.assert_array_equal(best[c], chain[int(np.argmax(logpi))])
        assert st.best_logpi.cpu().numpy()[c] == logpi.max()


@pytest.mark.parametrize("algo,C,cplx,pairs", [("myula", 4, False, True), ("skrock", 2, True, True), ("myula", 3, False, False)])
def test_sampler_summaries(algo, C, cplx, pairs):
    """(the third case steps on the transform's own plan, which carries ring state between iterations: the image summary must
    not disturb it)"""
    s, op = _run(algo, C, ("state", "image"), cplx=cplx, real_pairs=pairs)
    assert s.used_graph
    if algo == "myula":
        assert s._eng["ring"] and s._eng["pairs"] == pairs
    _check_sampler_summary(s, op, [s.nsamples] * C)
    plain, _ = _run(algo, C, None, cplx=cplx, real_pairs=pairs)  # the no-behaviour-change check
    assert plain.summary is None
    for k in ("chain", "logPi", "L2s", "priors"):
        np.testing.assert_array_equal(getattr(s, k), getattr(plain, k), err_msg=k)


def test_pxmala_masked_summaries():
    """PxMALA saves a different subset of chains at every save candidate: the masked path"""
    C = 3
    s, op = _run("pxmala", C, ("state", "image"), seed=PXMALA_SEED)
    assert not s.stopped_early
    acc = np.asarray(s.acceptance_trace)  # [niter, C]
    j, mixed = np.zeros(C, dtype=int), 0  # the save candidates of nburn = 3, ngap = 2, while every chain still saves
    for a in acc[3::2]:
        if j.max() < s.nsamples and a.min() == 0 and a.max() == 1:
            mixed += 1
        j += (a != 0) & (j < s.nsamples)
    assert mixed > 0, "no save candidate with an accepted and a rejected chain while all chains were still saving"
    _check_sampler_summary(s, op, [s.nsamples] * C)
    plain, _ = _run("pxmala", C, None, seed=PXMALA_SEED)
    for k in ("chain", "logPi", "L2s", "priors", "acceptance_trace"):
        np.testing.assert_array_equal(getattr(s, k), getattr(plain, k), err_msg=k)


def test_summary_without_a_saved_chain_and_graph_vs_eager():
    """summary="state" without "chain" in track: no chain attribute, a full summary, bit-equal to the run that kept the chain;
    graph replay and eager stepping give bit-equal summaries"""
    C = 4
    lean, _ = _run("myula", C, "state", track=("logposterior", "L2", "prior"))
    assert not hasattr(lean, "chain") and set(lean.summary) == {"state"}
    full, _ = _run("myula", C, ("state", "image"))
    eager, _ = _run("myula", C, ("state", "image"), use_graph=False)
    assert full.used_graph and not eager.used_graph
    a = lean.summary["state"].to_host()
    assert list(a["count"]) == [lean.nsamples] * C and np.isfinite(a["mean"]).all() and (a["m2"] > 0).any()
    for space in ("state", "image"):
        f, e = full.summary[space].to_host(), eager.summary[space].to_host()
        for k in f:
            np.testing.assert_array_equal(f[k], e[k], err_msg=f"{space} {k}")
    for k, v in full.summary["state"].to_host().items():
        np.testing.assert_array_equal(a[k], v, err_msg=k)


def test_image_summary_of_a_harmonic_transform_is_refused():
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams
    from pxmcmc_amd.measurements import WeakLensingHarmonic
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.transforms import SphericalWaveletTransform

    L = 8
    tr = SphericalWaveletTransform(L, 2, 0, harmonic=True, max_chains=1)
    op = ForwardOperator(np.zeros(L * L, dtype=complex), 0.1, "synthesis", transform=tr, measurement=WeakLensingHarmonic(L),
                         nparams=tr.ncoefs)
    p = PxMCMCParams(lmda=1e-3, delta=5e-4, nsamples=2, nburn=0, ngap=1, verbosity=0, complex=True)
    with pytest.raises(ValueError, match="harmonic"):
        MYULA(op, L1("synthesis", None, None, 1e-3), p, summary="image")
    assert MYULA(op, L1("synthesis", None, None, 1e-3), p, summary="state")._summary_spaces == ("state",)


# ---- two ranks ---------------------------------------------------------------------------------------------------------------
RANK_WORKER = textwrap.dedent(
    """
    import os, sys
    import numpy as np
    sys.path.insert(0, os.environ["PXM_ROOT"])
    sys.path.insert(0, os.path.join(os.environ["PXM_ROOT"], "tests"))
    import torch
    from pxmcmc_amd import distributed as D
    from pxmcmc_amd.uncertainty import PosteriorSummary, rhat_np
    from test_gpu_moments import _run

    rank, local_rank, world = D.init(backend="gloo")   # both ranks share the one GPU of the test box (RCCL refuses that)
    torch.cuda.set_device(0)
    TOTAL = 4
    first, count = D.shard_chains(TOTAL, rank, world)
    s, _ = _run("myula", count, "state", track=("logposterior",), chain_offset=first)
    mine = s.summary["state"].to_host()
    D.barrier()
    gathered = {k: D.gather_summaries(v).numpy() for k, v in mine.items()}   # end of run: no collective in the sampling loop
    if rank == 0:
        # the same result from the per-rank dicts (rank order), as a job that writes one file per rank would merge them
        halves = [{k: v[r * count:(r + 1) * count] for k, v in gathered.items()} for r in range(world)]
        merged = PosteriorSummary.merge(halves)
        one, _ = _run("myula", TOTAL, "state", track=("logposterior",))
        ref = one.summary["state"]
        r_ref = ref.rhat().cpu().numpy()
        r = rhat_np(merged["count"], merged["mean"], merged["m2"])
        assert list(merged["count"]) == [one.nsamples] * TOTAL
        assert np.isfinite(r_ref).any()
        err = np.nanmax(np.abs(r - r_ref) / r_ref)
        assert np.array_equal(np.isnan(r), np.isnan(r_ref)) and err < 1e-12, err
        print("RANKS-OK", first, count, float(np.nanmax(r)), flush=True)
    D.barrier()
    """
)


def test_two_rank_merge_gives_the_rhat_of_one_batch(tmp_path):
    """two processes (torchrun, gloo rendezvous, both on the box's one GPU) each accumulate the summary of their shard of 4
    chains; merged on the host, R-hat equals that of a single 4-chain run to 1e-12"""
    script = tmp_path / "rank_worker.py"
    script.write_text(RANK_WORKER)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, PXM_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "RANKS-OK 0 2" in res.stdout


def test_zz_report_largest_ratio():
    """Report only: prints the largest ratio to the long-double model (kernel sweeps) and to moments_np (samplers) that the
    tests of this module which ran before it observed.  The assertions are in those tests, element by element; run alone
    this prints zeros."""
    print("largest ratios observed (units of S_mean, S_m2; bound %.2f):" % BOUND, WORST)


# ---- examples ----------------------------------------------------------------------------------------------------------------
def _example(name):
    import runpy

    return runpy.run_path(os.path.join(ROOT, "examples", name))


def test_topography_example_with_summary(tmp_path):
    from pxmcmc_amd.saving import load_mcmc, load_summaries

    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        path, rel, std = _example("topography_synthetic.py")["main"](
            ["--L", "16", "--nsamples", "8", "--ngap", "50", "--chains", "2", "--summary", "--outdir", str(tmp_path)])
    data, _ = load_mcmc(path)
    summ = load_summaries(data)["image"]
    assert "chain" not in data and list(summ["count"]) == [8, 8]
    base = os.path.join(str(tmp_path), "myula_synthesis_0")
    mean = np.load(base + "_mean.npy")
    np.testing.assert_array_equal(np.load(base + "_std.npy"), std)
    assert mean.shape == std.shape == (16 * 31,) and not np.iscomplexobj(mean) and (std > 0).all() and rel < 1.0
    assert "max R-hat over the image (2 chains)" in out.getvalue()


@pytest.mark.parametrize("harmonic", [False, True])
def test_weaklensing_example_with_summary(tmp_path, harmonic):
    from pxmcmc_amd.saving import load_mcmc, load_summaries

    argv = ["--L", "16", "--nsamples", "4", "--ngap", "3", "--nburn", "5", "--chains", "2", "--summary", "--outdir", str(tmp_path)]
    argv += ["--harmonic", "--delta", "1e-6"] if harmonic else ["--algo", "pxmala", "--delta", "1e-9"]
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        out = _example("weaklensing_synthetic.py")["main"](argv)
    space = "state" if harmonic else "image"
    data, _ = load_mcmc(out["path"])
    summ = load_summaries(data)
    assert "chain" not in data and set(summ) == {space} and list(summ[space]["count"]) == [4, 4]
    base = os.path.splitext(out["path"])[0]
    mean, std = np.load(base + "_mean.npy"), np.load(base + "_std.npy")
    assert mean.shape == std.shape and np.iscomplexobj(mean) and np.isfinite(std).all() and np.isfinite(out["rel_err"])
    assert f"max R-hat over the {space} (2 chains)" in text.getvalue()
