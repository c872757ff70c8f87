"""Host side of the streaming posterior summaries (no GPU needed): the numpy statements
``uncertainty.moments_np`` / ``pooled_np`` / ``rhat_np`` against long-double and textbook evaluations, the error model of
the fp64 Welford recurrence the device kernel runs, ``PosteriorSummary.merge`` and the ``summary_*`` fields of a saved run.

tests/test_gpu_moments.py imports the inputs, the long-double model and the error scales from here."""
import numpy as np
import pytest

LD = np.longdouble
U = 2.0 ** -53
# Largest error of the fp64 Welford recurrence (restated in numpy below, one sample at a time) against the long-double
# two-pass values, in units of S_mean = n 2^-53 max|x| and S_m2 = n 2^-53 (sum (x - xbar)^2 + max|x|^2), over the inputs
# of welford_cases() -- measured by test_welford_route_against_long_double, which pins it.  The device kernel is held to
# 4 * C0_MEASURED (device division and contraction of d * (x - mean) into an fma: the margin DESIGN.md sections 13 and 14
# give a kernel over its numpy route).
C0_MEASURED = 0.5
KINDS = 4


def moment_columns(n, m, seed, kind0=None):
    """[n, m] samples whose column j is of kind (j + kind0) % 4 (kind0 = seed unless given): 0 standard normal; 1 constant;
    2 offset 1e8 with unit spread; 3 mixed signs over six decades"""
    rng = np.random.default_rng([seed, n, m])
    x = rng.normal(size=(n, m))
    kind = (np.arange(m) + (seed if kind0 is None else kind0)) % KINDS
    x[:, kind == 1] = rng.normal(size=(kind == 1).sum()) * 3.0
    x[:, kind == 2] += 1e8
    x[:, kind == 3] *= 10.0 ** rng.integers(-3, 4, size=(n, (kind == 3).sum()))
    return x


def two_pass_ld(x):
    """(mean, m2) of the rows of x [n, m] in long double, two passes"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    mean = x.sum(axis=0) / LD(x.shape[0])
    return mean, ((x - mean) ** 2).sum(axis=0)


def error_scales(x):
    """(S_mean, S_m2) per column of x [n, m]"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mx = np.abs(x).max(axis=0)
    _, m2 = two_pass_ld(x)
    return n * U * mx, n * U * (m2.astype(np.float64) + mx * mx)


def ratios(mean, m2, x):
    """largest |mean - mean_ld| / S_mean and |m2 - m2_ld| / S_m2 over the columns (0 where the scale is 0 and the value exact)"""
    mean_ld, m2_ld = two_pass_ld(x)
    s_mean, s_m2 = error_scales(x)
    out = []
    for got, ext, s in ((mean, mean_ld, s_mean), (m2, m2_ld, s_m2)):
        err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ext).astype(np.float64)
        assert np.all(err[s == 0] == 0), "an all-zero column must give exact zeros"
        out.append(float(np.max(np.where(s > 0, err / np.where(s > 0, s, 1.0), 0.0))))
    return tuple(out)


def welford_np(x, count=0, mean=None, m2=None):
    """the recurrence of k_moments_update in fp64, one sample at a time: k = count + 1; d = x - mean; mean += d / k;
    m2 += d * (x - mean_new)"""
    x = np.asarray(x, dtype=np.float64)
    mean = np.zeros(x.shape[1]) if mean is None else mean.copy()
    m2 = np.zeros(x.shape[1]) if m2 is None else m2.copy()
    for row in x:
        count += 1
        d = row - mean
        mean = mean + d / count
        m2 = m2 + d * (row - mean)
    return count, mean, m2


def welford_cases():
    for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 40, 200):
        for seed in range(4):
            yield moment_columns(n, 64, seed)


# ---- moments_np ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 17, 200])
def test_moments_np_against_long_double_two_pass(n):
    """To first order the fp64 two-pass sums err by at most (n - 1) u |partial sum| <= n u max|x| in the mean and, the cross
    term 2 (xbar - mean) sum (x - xbar) being zero, by (n + 2) u sum (x - xbar)^2 <= 2 S_m2 in m2: both ratios stay below 2."""
    from pxmcmc_amd.uncertainty import moments_np

    for seed in range(4):
        x = moment_columns(n, 37, seed)
        cnt, mean, m2 = moments_np(x)
        assert cnt == n and mean.shape == m2.shape == (37,)
        r_mean, r_m2 = ratios(mean, m2, x)
        assert r_mean <= 2.0 and r_m2 <= 2.0, (n, seed, r_mean, r_m2)
    if n == 1:
        assert np.all(m2 == 0) and np.array_equal(mean, x[0])


def test_moments_np_complex_is_per_component():
    from pxmcmc_amd.uncertainty import moments_np

    rng = np.random.default_rng(2)
    z = rng.normal(size=(9, 5)) + 1j * rng.normal(size=(9, 5))
    cnt, mean, m2 = moments_np(z)
    assert cnt == 9 and mean.shape == (10,)
    _, mr, sr = moments_np(z.real)
    _, mi, si = moments_np(z.imag)
    np.testing.assert_array_equal(mean[0::2], mr)
    np.testing.assert_array_equal(mean[1::2], mi)
    np.testing.assert_array_equal(m2[0::2], sr)
    np.testing.assert_array_equal(m2[1::2], si)


# ---- the error model of the recurrence -----------------------------------------------------------------------------------
def test_welford_route_against_long_double():
    """the fp64 Welford recurrence against the long-double two-pass values, in units of the per-element scales -- measured
    here, pinned as C0_MEASURED (the GPU file holds the kernel to 4 * C0_MEASURED)"""
    worst = [0.0, 0.0]
    for x in welford_cases():
        cnt, mean, m2 = welford_np(x)
        assert cnt == x.shape[0]
        const = np.all(x == x[0], axis=0)  # the recurrence leaves a constant column exact: d = 0 from the second sample on
        assert const.any() and np.all(m2[const] == 0) and np.array_equal(mean[const], x[0, const])
        r = ratios(mean, m2, x)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print("largest ratios (mean, m2):", worst)
    assert max(worst) <= C0_MEASURED
    assert max(worst) >= C0_MEASURED / 4  # the pinned value is the measured one, not a loose cap


def test_welford_continues_from_accumulators():
    x = moment_columns(11, 16, 1)
    c1, a1, s1 = welford_np(x[:4])
    c2, a2, s2 = welford_np(x[4:], c1, a1, s1)
    c, a, s = welford_np(x)
    assert c2 == c and np.array_equal(a2, a) and np.array_equal(s2, s)


# ---- R-hat and the pooled moments ----------------------------------------------------------------------------------------
def _accumulators(chains):
    """chains [C, n, m] -> (count [C], mean [C, m], m2 [C, m]) through moments_np"""
    from pxmcmc_amd.uncertainty import moments_np

    parts = [moments_np(c) for c in chains]
    return np.array([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts])


def _rhat_textbook(chains):
    """Gelman et al., Bayesian Data Analysis (3rd ed.), eq. 11.1-11.4, on a [C, n, m] array"""
    C, n, _ = chains.shape
    W = chains.var(axis=1, ddof=1).mean(axis=0)
    B = n * chains.mean(axis=1).var(axis=0, ddof=1)
    return np.sqrt(((n - 1) / n * W + B / n) / W)


def test_rhat_np_against_the_textbook_formula():
    from pxmcmc_amd.uncertainty import rhat_np

    rng = np.random.default_rng(3)
    chains = rng.normal(size=(5, 60, 33)) * rng.uniform(0.5, 2.0, size=(1, 1, 33)) + rng.normal(size=(5, 1, 33)) * 0.3
    np.testing.assert_allclose(rhat_np(*_accumulators(chains)), _rhat_textbook(chains), rtol=1e-12)


def test_rhat_np_is_one_for_iid_chains_and_large_for_shifted_ones():
    from pxmcmc_amd.uncertainty import rhat_np

    rng = np.random.default_rng(4)
    iid = rng.normal(size=(8, 4000, 20))
    r = rhat_np(*_accumulators(iid))
    assert np.all(np.abs(r - 1) < 5e-3), r
    shifted = iid[:4, :500] + 3.0 * np.arange(4)[:, None, None]  # means three standard deviations apart
    assert np.all(rhat_np(*_accumulators(shifted)) > 1.5)


def test_rhat_np_undefined_cases():
    from pxmcmc_amd.uncertainty import pooled_np, rhat_np

    rng = np.random.default_rng(5)
    chains = rng.normal(size=(3, 10, 6))
    chains[:, :, 2] = 1.25  # a constant column: W == 0
    cnt, mean, m2 = _accumulators(chains)
    r = rhat_np(cnt, mean, m2)
    assert np.isnan(r[2]) and np.isfinite(np.delete(r, 2)).all()
    assert np.isnan(rhat_np(cnt[:1], mean[:1], m2[:1])).all()  # one chain
    one = _accumulators(chains[:, :1])
    assert np.isnan(rhat_np(*one)).all()  # one sample per chain
    # a chain without samples takes no part (its accumulators may hold anything)
    cnt0, mean0, m20 = np.append(cnt, 0), np.vstack([mean, np.full((1, 6), np.nan)]), np.vstack([m2, np.full((1, 6), np.nan)])
    np.testing.assert_array_equal(rhat_np(cnt0, mean0, m20), r)
    np.testing.assert_array_equal(pooled_np(cnt0, mean0, m20)[0], pooled_np(cnt, mean, m2)[0])
    # unequal counts: R-hat is refused, the pooled moments are not
    cnt_b, mean_b, m2_b = _accumulators([chains[0], chains[1][:7], chains[2]])
    with pytest.raises(ValueError, match="common sample count"):
        rhat_np(cnt_b, mean_b, m2_b)
    pm, pv = pooled_np(cnt_b, mean_b, m2_b)
    allx = np.concatenate([chains[0], chains[1][:7], chains[2]])
    np.testing.assert_allclose(pm, allx.mean(axis=0), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(pv, allx.var(axis=0, ddof=1), rtol=1e-12, atol=1e-28)
    none = pooled_np(np.zeros(2, dtype=int), np.zeros((2, 3)), np.zeros((2, 3)))
    assert np.isnan(none[0]).all() and np.isnan(none[1]).all()


def test_pooled_np_equals_the_moments_of_the_concatenated_chains():
    from pxmcmc_amd.uncertainty import pooled_np

    chains = np.stack([moment_columns(12, 24, s) for s in range(4)])
    pm, pv = pooled_np(*_accumulators(chains))
    allx = chains.reshape(-1, 24)
    mean_ld, m2_ld = two_pass_ld(allx)
    s_mean, s_m2 = error_scales(allx)
    assert np.all(np.abs(pm.astype(LD) - mean_ld) <= 4 * s_mean)
    assert np.all(np.abs((pv * (allx.shape[0] - 1)).astype(LD) - m2_ld) <= 4 * s_m2)


def test_merge_of_two_halves_equals_the_whole():
    from pxmcmc_amd.uncertainty import PosteriorSummary, rhat_np

    rng = np.random.default_rng(6)
    chains = rng.normal(size=(6, 25, 14))
    cnt, mean, m2 = _accumulators(chains)
    best = rng.normal(size=(6, 14))
    lp = rng.normal(size=6)
    halves = [{"count": cnt[s], "mean": mean[s], "m2": m2[s], "best": best[s], "best_logpi": lp[s]} for s in (slice(0, 3), slice(3, 6))]
    whole = PosteriorSummary.merge(halves)
    assert set(whole) == set(PosteriorSummary.FIELDS)
    np.testing.assert_array_equal(whole["count"], cnt)
    np.testing.assert_array_equal(whole["best"], best)
    np.testing.assert_array_equal(whole["best_logpi"], lp)
    np.testing.assert_array_equal(rhat_np(whole["count"], whole["mean"], whole["m2"]), rhat_np(cnt, mean, m2))
    no_best = PosteriorSummary.merge([{k: h[k] for k in ("count", "mean", "m2")} for h in halves])
    assert set(no_best) == {"count", "mean", "m2"}
    with pytest.raises(ValueError):
        PosteriorSummary.merge([])


# ---- the saved run -------------------------------------------------------------------------------------------------------
class _FakeSummary:
    def __init__(self, host):
        self._host = host

    def to_host(self):
        return self._host


def _run_with_summary(rng, best=True):
    class Run:
        pass

    r = Run()
    r.logPi, r.L2s, r.priors = rng.normal(size=(2, 5)), rng.random((2, 5)), rng.random((2, 5))
    hosts = {}
    for space, m, cplx in (("state", 12, False), ("image", 7, True)):
        h = {"count": np.array([5, 5]), "mean": rng.normal(size=(2, m * (2 if cplx else 1))), "m2": rng.random((2, m * (2 if cplx else 1)))}
        if best:
            h["best"] = rng.normal(size=(2, m)) + (1j * rng.normal(size=(2, m)) if cplx else 0)
            h["best_logpi"] = rng.normal(size=2)
        hosts[space] = h
    r.summary = {k: _FakeSummary(v) for k, v in hosts.items()}
    return r, hosts


def test_save_and_load_round_trip_the_summary_fields(tmp_path):
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.saving import load_mcmc, load_summaries, save_mcmc

    r, hosts = _run_with_summary(np.random.default_rng(7))
    p = PxMCMCParams(nsamples=5, nburn=2, ngap=1, track=["logposterior", "L2", "prior"])
    data, _ = load_mcmc(save_mcmc(r, p, str(tmp_path), filename="run"))
    assert "chain" not in data
    assert {k for k in data if k.startswith("summary_")} == {
        f"summary_{s}_{f}" for s in ("state", "image") for f in ("count", "mean", "m2", "best", "best_logpi")}
    back = load_summaries(data)
    assert set(back) == {"state", "image"}
    for space, h in hosts.items():
        assert set(back[space]) == set(h)
        for k, v in h.items():
            np.testing.assert_array_equal(back[space][k], v)
            assert back[space][k].dtype == np.asarray(v).dtype
    # best=False: those two fields are absent; no summary (None, or no attribute at all): no summary_* key
    r2, _ = _run_with_summary(np.random.default_rng(8), best=False)
    data2, _ = load_mcmc(save_mcmc(r2, p, str(tmp_path), filename="run2"))
    assert not any(k.endswith("best") or k.endswith("best_logpi") for k in data2) and "summary_state_m2" in data2
    r2.summary = None
    data3, _ = load_mcmc(save_mcmc(r2, p, str(tmp_path), filename="run3"))
    assert set(data3) == {"logposterior", "L2s", "priors"}
    del r2.summary
    data4, _ = load_mcmc(save_mcmc(r2, p, str(tmp_path), filename="run4"))
    assert set(data4) == set(data3)


def test_save_mcmc_hdf5_route_writes_the_summary_after_the_reference_datasets(monkeypatch, tmp_path):
    """the HDF5 branch against the recording stub of h5py.File the saving tests use: a sampler without a summary issues the
    calls it always did (tests/golden/g13_save_mcmc_format.json pins them), one with a summary appends its fields"""
    import os
    import sys
    import types

    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.saving import save_mcmc

    calls = []

    class _File:
        def __init__(self, path, mode):
            calls.append(["open", os.path.basename(path), mode])
            self.attrs = {}

        def create_dataset(self, name, data=None, dtype=None):
            calls.append(["dataset", name, None if dtype is None else str(dtype), np.asarray(data)])

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    stub = types.ModuleType("h5py")
    stub.File = _File
    monkeypatch.setitem(sys.modules, "h5py", stub)
    r, hosts = _run_with_summary(np.random.default_rng(9))
    p = PxMCMCParams(nsamples=5, nburn=2, ngap=1, track=["logposterior", "L2", "prior"])
    save_mcmc(r, p, str(tmp_path), filename="run")
    names = [c[1] for c in calls if c[0] == "dataset"]
    assert names[:3] == ["logposterior", "L2s", "priors"]
    assert names[3:] == [f"summary_{s}_{f}" for s in ("state", "image") for f in ("count", "mean", "m2", "best", "best_logpi")]
    for c in calls:
        if c[0] == "dataset" and c[1].startswith("summary_state_"):
            np.testing.assert_array_equal(c[3], hosts["state"][c[1][len("summary_state_"):]])
    calls.clear()
    r.summary = None
    save_mcmc(r, p, str(tmp_path), filename="run")
    assert [c[1] for c in calls if c[0] == "dataset"] == ["logposterior", "L2s", "priors"]


# ---- the samplers' keyword and the C-ABI's argument checks (no device needed) -----------------------------------------------
def test_summary_keyword_is_validated():
    """the samplers' ``summary=`` keyword on stub operators (constructing a sampler launches nothing)"""
    from pxmcmc_amd.mcmc import MYULA, SKROCK, PxMALA, PxMCMCParams

    class Transform:
        harmonic = False

        def inverse(self, X):
            return X

    class Forward:
        setting, nparams, data = "synthesis", 8, np.zeros(8)

        def __init__(self, transform):
            if transform is not None:
                self.transform = transform

    class Prior:
        pass

    op, reg = Forward(Transform()), Prior()
    p = PxMCMCParams(nsamples=2, nburn=0, ngap=1, verbosity=0)
    for cls in (MYULA, PxMALA, SKROCK):
        s = cls(op, reg, p)
        assert s.summary is None and s._summary_spaces == ()
        assert cls(op, reg, p, summary="state")._summary_spaces == ("state",)
        assert cls(op, reg, p, summary=("state", "image", "state"))._summary_spaces == ("state", "image")
        assert cls(op, reg, p, summary="image").summary == {}
        with pytest.raises(ValueError, match="summary must be"):
            cls(op, reg, p, summary="pixels")
        harm = Transform()
        harm.harmonic = True
        with pytest.raises(ValueError, match="harmonic"):
            cls(Forward(harm), reg, p, summary=("state", "image"))
        assert cls(Forward(harm), reg, p, summary="state")._summary_spaces == ("state",)
        with pytest.raises(ValueError, match="transform.inverse"):
            cls(Forward(None), reg, p, summary="image")
        ana = Forward(None)
        ana.setting = "analysis"  # the image is the state itself: no transform needed
        assert cls(ana, reg, p, summary="image")._summary_spaces == ("image",)


def test_moments_entry_points_reject_bad_arguments():
    import ctypes

    from pxmcmc_amd import _lib

    lib = _lib.lib
    buf = (ctypes.c_double * 8)()
    cnt = (ctypes.c_int64 * 2)()
    a = ctypes.addressof
    upd = lambda x, xs, c, mean, m2, lp, bl, bx, m, C: lib.pxm_moments_update(  # noqa: E731
        x, xs, c, mean, m2, None, lp, 1, bl, bx, m, C, None)
    for args, text in (
        ((a(buf), 1, a(cnt), a(buf), a(buf), None, None, None, 4, 0), "C"),
        ((a(buf), 1, a(cnt), a(buf), a(buf), None, None, None, 0, 2), "m >= 1"),
        ((None, 1, a(cnt), a(buf), a(buf), None, None, None, 4, 2), "null buffer"),
        ((a(buf), 1, None, a(buf), a(buf), None, None, None, 4, 2), "null buffer"),
        ((a(buf), 3, a(cnt), a(buf), a(buf), None, None, None, 4, 2), "x_stride"),
        ((a(buf), 1, a(cnt), a(buf), a(buf), a(buf), None, None, 4, 2), "given together"),
    ):
        assert upd(*args) < 0
        assert text in lib.pxm_last_error().decode(), (text, lib.pxm_last_error().decode())
    fin = lambda c, mean, m2, m, C, pm: lib.pxm_moments_finalize(c, mean, m2, m, C, pm, None, None, None, None, None)  # noqa: E731
    for args, text in (
        ((a(cnt), a(buf), a(buf), 4, 0, a(buf)), "C >= 1"),
        ((a(cnt), a(buf), a(buf), 0, 2, a(buf)), "m >= 1"),
        ((a(cnt), None, a(buf), 4, 2, a(buf)), "null buffer"),
        ((a(cnt), a(buf), a(buf), 4, 2, None), "no output"),
    ):
        assert fin(*args) < 0
        assert text in lib.pxm_last_error().decode(), (text, lib.pxm_last_error().decode())
    assert lib.pxm_moments_scratch_doubles(0) == -1
    assert lib.pxm_moments_scratch_doubles(1) == 2 and lib.pxm_moments_scratch_doubles(10 ** 7) == 2048
