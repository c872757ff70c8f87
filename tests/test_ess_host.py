"""Host side of the streaming effective sample size (no GPU needed): the numpy statements
``acov_update_np`` / ``acov_gamma_np`` / ``ess_np`` / ``ess_pooled_np`` against the long-double definition ``autocov_np``
(the error model and its pinned constant), the estimator against AR(1) chains of known autocorrelation time, the pooled
estimate, the undefined cases and the cap, ``PosteriorSummary.merge`` and ``save_mcmc`` with the new keys, and the argument
checks of the constructors and of the C-ABI.

tests/test_gpu_ess.py imports the columns and the numpy route from here."""
import numpy as np
import pytest

KINDS = ("walk", "iid", "offset", "constant", "ramp", "mixed")
NS = (1, 2, 3, 5, 17, 40, 200, 1000)
# largest |gamma_l (accumulators) - gamma_l (long double definition)| / (n 2^-53 max_t |y_t|^2) over the columns, run lengths
# and lags of test_accumulators_against_the_definition, rounded up: measured 0.352 at K = 2 and at K = 8
E0_MEASURED = 0.40


def ess_columns(n, m, seed):
    """[n, m] samples whose column j is of kind KINDS[(j + seed) % 6]: a random walk; iid normal; iid normal at an offset of
    1e8; constant (gamma_0 = 0: no ESS); a ramp; iid normal of a scale that differs by column over twelve decades"""
    rng = np.random.default_rng([seed, n, m])
    x = rng.normal(size=(n, m))
    kind = (np.arange(m) + seed) % len(KINDS)
    x[:, kind == 0] = np.cumsum(x[:, kind == 0], axis=0)
    x[:, kind == 2] += 1e8
    x[:, kind == 3] = rng.normal(size=(kind == 3).sum())
    x[:, kind == 4] = x[:1, kind == 4] + np.arange(n, dtype=np.float64)[:, None] * 0.37
    cols = np.flatnonzero(kind == 5)
    x[:, cols] *= 10.0 ** ((cols % 13) - 6.0)
    return x


def ar1_columns(n, m, phi, seed):
    """[n, m] stationary AR(1) columns of unit innovation variance: autocorrelation time (1 + phi) / (1 - phi)"""
    rng = np.random.default_rng([seed, n, m])
    e = rng.normal(size=(n, m))
    x = np.empty((n, m))
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[t] = phi * x[t - 1] + e[t]
    return x


def assert_bit_equal(got, want, what=""):
    """the same bit patterns, any NaN standing for any other"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape, what)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=str(what))
    np.testing.assert_array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan], err_msg=str(what))


def acov_of(x, K, state=None, count=0):
    """run acov_update_np over the rows of x [n, m] -> (count, acc [K, m], tot [m], head [K, m], last [K, m]); a fresh state
    starts from NaN: it needs no initialisation"""
    from pxmcmc_amd.uncertainty import acov_update_np

    m = x.shape[1]
    acc, tot, head, last = state if state is not None else (np.full((K, m), np.nan), np.full(m, np.nan), np.full((K, m), np.nan),
                                                            np.full((K, m), np.nan))
    for row in x:
        acov_update_np(row, count, acc, tot, head, last)
        count += 1
    return count, acc, tot, head, last


def ess_of_chains(chains, K):
    """chains [C][n_c, m] -> (count [C], acc, tot, head, last) stacked over the chains, the arguments of ess_np"""
    states = [acov_of(np.asarray(x), K) for x in chains]
    return (np.array([s[0] for s in states]),) + tuple(np.stack([s[i] for s in states]) for i in range(1, 5))


@pytest.mark.parametrize("K", [2, 8])
def test_accumulators_against_the_definition(K):
    """gamma_l of the accumulators, read out at every run length of NS on the way, against the definition in long double,
    in units of n 2^-53 max |y|^2: within the pinned constant.  The 1e8 offset costs nothing (the pivot), a constant column
    gives gamma = 0 exactly"""
    from pxmcmc_amd.uncertainty import acov_gamma_np, autocov_np

    worst = 0.0
    for seed in range(3):
        x = ess_columns(NS[-1], 12, seed)
        kind = (np.arange(12) + seed) % len(KINDS)
        state, count = None, 0
        for n in NS:
            count, *state = acov_of(x[count:n], K, state, count)
            assert count == n
            g, mean = acov_gamma_np(n, *state)
            want = autocov_np(x[:n], K)
            assert g.shape == want.shape == (min(K, n), 12)
            y = x[:n] - x[0]
            scale = n * 2.0 ** -53 * (np.abs(y).max(axis=0) ** 2)
            err = np.abs(g.astype(np.longdouble) - want).astype(np.float64)
            assert (g[:, kind == 3] == 0).all() and (err[:, scale == 0] == 0).all()
            ratio = (err[:, scale > 0] / scale[scale > 0]).max() if (scale > 0).any() else 0.0
            worst = max(worst, float(ratio))
            # the mean x_0 + tot / n: n roundings of size u max |y| in tot, one in each y_t and in d, one of u |mean| at the end
            ref = x[:n].astype(np.longdouble).mean(axis=0)
            assert (np.abs(mean - ref) <= 2.0 ** -53 * ((n + 2) * np.abs(y).max(axis=0) + 2 * np.abs(mean))).all()
    print("largest error of gamma_l in units of n 2^-53 max |y|^2 at K = %d: %.3f" % (K, worst))
    assert worst <= E0_MEASURED


def test_state_needs_no_initialisation_and_continues():
    """two runs from states of different garbage agree bit for bit, as does a run made in two parts"""
    x = ess_columns(45, 7, 1)
    _, *a = acov_of(x, 8)
    junk = (np.full((8, 7), 3.0), np.full(7, -2.0), np.full((8, 7), 1e300), np.full((8, 7), np.inf))
    _, *b = acov_of(x, 8, junk)
    n1, *c = acov_of(x[:19], 8)
    _, *c = acov_of(x[19:], 8, c, n1)
    for u, v, w in zip(a, b, c):
        assert_bit_equal(u, v)
        assert_bit_equal(u, w)


@pytest.mark.parametrize("phi", [0.0, 0.5])
def test_ess_of_ar1_chains(phi):
    """256 AR(1) columns, N = 2000, K = 32: the median of ESS / N within 10 % of (1 - phi) / (1 + phi) (single elements
    scatter by tens of per cent and are not tested); hardly any element truncated"""
    from pxmcmc_amd.uncertainty import ess_np

    N, K = 2000, 32
    ess, lag = ess_np(*ess_of_chains([ar1_columns(N, 256, phi, 3)], K))
    assert ess.shape == lag.shape == (1, 256) and np.isfinite(ess).all()
    truth = (1.0 - phi) / (1.0 + phi)
    med = np.median(ess[0]) / N
    print("phi = %g: median ESS / N = %.4f, truth %.4f" % (phi, med, truth))
    assert abs(med / truth - 1.0) < 0.10
    assert (lag[0] % 2 == 0).all() and (lag[0] >= 0).all() and (lag[0] == K).mean() < 0.05


def test_slowly_mixing_chains_are_flagged_truncated():
    """phi = 0.98 (autocorrelation time 99) with K = 32 lags: the sequence cannot end, every element is flagged and its ESS
    lies above the truth -- the documented upper bound"""
    from pxmcmc_amd.uncertainty import ess_np

    N, K, phi = 2000, 32, 0.98
    ess, lag = ess_np(*ess_of_chains([ar1_columns(N, 256, phi, 4)], K))
    assert (lag == K).all()
    assert (ess > N * (1.0 - phi) / (1.0 + phi)).all()


def test_pooled_ess():
    """C chains of one law: the pooled ESS is the sum of the per-chain values (medians within 15 %), and mcse^2 is var+ /
    ESS; chains whose means lie 20 standard deviations apart: the pooled ESS collapses; different counts are refused"""
    from pxmcmc_amd.uncertainty import ess_np, ess_pooled_np

    N, K, C, phi = 2000, 32, 4, 0.5
    chains = [ar1_columns(N, 256, phi, 10 + c) for c in range(C)]
    state = ess_of_chains(chains, K)
    ess, _ = ess_np(*state)
    pooled, mcse = ess_pooled_np(*state)
    assert pooled.shape == mcse.shape == (256,) and np.isfinite(pooled).all() and np.isfinite(mcse).all()
    ratio = np.median(pooled) / np.median(ess.sum(axis=0))
    print("pooled / sum of per-chain ESS (medians): %.4f" % ratio)
    assert abs(ratio - 1.0) < 0.15
    var = np.concatenate(chains).var(axis=0)
    np.testing.assert_allclose(mcse ** 2 * pooled, var, rtol=0.01)  # (var+ is the pooled variance up to O(1 / n))
    apart = [x + 20.0 * c / np.sqrt(1.0 - phi * phi) for c, x in enumerate(chains)]
    far, far_mcse = ess_pooled_np(*ess_of_chains(apart, K))
    # rho_l is 1 at every lag kept, every P_k is 2: tau = 2 K - 1, the largest the K lags can express
    np.testing.assert_allclose(far, C * N / (2 * K - 1.0), rtol=0.01)
    assert (far < 0.06 * ess.sum(axis=0)).all() and (far_mcse > 10 * mcse).all()
    # a single chain: var+ = (n - 1) / n W = gamma_0, rho_l = 1 - n / (n - 1) (1 - gamma_l / gamma_0): the per-chain value up to
    # K / n in tau
    one, _ = ess_pooled_np(*ess_of_chains(chains[:1], K))
    np.testing.assert_allclose(one, ess[0], rtol=2.0 * K / N)
    with pytest.raises(ValueError, match="common sample count"):
        ess_pooled_np(*ess_of_chains([chains[0], chains[1][:-1]], K))
    count, *rest = ess_of_chains(chains, K)
    count[1] = 0  # a chain without samples takes no part
    assert_bit_equal(ess_pooled_np(count, *rest)[0], ess_pooled_np(*ess_of_chains(chains[:1] + chains[2:], K))[0])


def test_undefined_cases_and_the_cap():
    from pxmcmc_amd.uncertainty import ess_np, ess_pooled_np

    x = ess_columns(40, 12, 0)
    kind = np.arange(12) % len(KINDS)
    for n in (0, 1, 2, 3):  # fewer than 4 samples: NaN, lag -1
        ess, lag = ess_np(*ess_of_chains([x[:n]], 8))
        assert np.isnan(ess).all() and (lag == -1).all()
        pooled, mcse = ess_pooled_np(*ess_of_chains([x[:n], x[:n]], 8))
        assert np.isnan(pooled).all() and np.isnan(mcse).all()
    for n in (4, 5, 17, 40):
        ess, lag = ess_np(*ess_of_chains([x[:n]], 8))
        assert np.isnan(ess[0, kind == 3]).all() and (lag[0, kind == 3] == -1).all()  # a constant column
        ok = kind != 3
        assert np.isfinite(ess[0, ok]).all() and (ess[0, ok] > 0).all() and (ess[0, ok] <= n * np.log10(n)).all()
        assert (lag[0, ok] % 2 == 0).all() and (lag[0, ok] <= 2 * (min(8, n) // 2)).all()
        pooled, _ = ess_pooled_np(*ess_of_chains([x[:n], x[:n] + 1.0], 8))
        assert np.isnan(pooled[kind == 3]).all() and np.isfinite(pooled[ok]).all()
    # an antithetic chain: rho_l = (-1)^l (n - l) / n, every P_k = 1 / n, tau = -1 + 8 / n <= 0 -> the cap n log10 n, as in Stan
    n = 100
    alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None] * np.ones((1, 3))
    ess, lag = ess_np(*ess_of_chains([alt], 8))
    np.testing.assert_allclose(ess, n * np.log10(n), rtol=1e-15)
    assert (lag == 8).all()
    # NaN and inf in a column: no ESS there, the other columns are not touched
    bad = x.copy()
    bad[7, 0], bad[9, 1] = np.nan, np.inf
    ess_bad, _ = ess_np(*ess_of_chains([bad], 8))
    ess_ok, _ = ess_np(*ess_of_chains([x], 8))
    assert np.isnan(ess_bad[0, :2]).all()
    assert_bit_equal(ess_bad[0, 2:], ess_ok[0, 2:])


def test_merge_carries_the_ess_keys():
    from pxmcmc_amd.uncertainty import PosteriorSummary

    assert PosteriorSummary.ESS_FIELDS == ("ess_lags", "ess", "ess_lag")
    rng = np.random.default_rng(11)
    base = [{"count": np.array([5, 5]), "mean": rng.normal(size=(2, 6)), "m2": rng.random((2, 6))} for _ in range(2)]
    plain = PosteriorSummary.merge(base)
    with_ess = [dict(d, ess_lags=np.int64(8), ess=rng.random((2, 6)), ess_lag=rng.integers(0, 8, (2, 6)).astype(np.int32)) for d in base]
    whole = PosteriorSummary.merge(with_ess)
    assert set(whole) == set(plain) | set(PosteriorSummary.ESS_FIELDS)
    assert whole["ess_lags"] == 8 and whole["ess"].shape == whole["ess_lag"].shape == (4, 6) and whole["ess_lag"].dtype == np.int32
    np.testing.assert_array_equal(whole["ess"], np.concatenate([d["ess"] for d in with_ess]))
    for dicts in ([with_ess[0], base[1]], [with_ess[0], dict(with_ess[1], ess_lags=np.int64(4))]):  # not all, or not one K
        mixed = PosteriorSummary.merge(dicts)
        assert set(mixed) == set(plain)
        for k in plain:
            np.testing.assert_array_equal(mixed[k], plain[k])


class _FakeSummary:
    def __init__(self, host):
        self._host = host

    def to_host(self):
        return self._host


def test_save_and_load_round_trip_the_ess(tmp_path):
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.saving import load_mcmc, load_summaries, save_mcmc

    class Run:
        pass

    rng = np.random.default_rng(12)
    r = Run()
    r.logPi = rng.normal(size=(2, 5))
    host = {"count": np.array([5, 5]), "mean": rng.normal(size=(2, 7)), "m2": rng.random((2, 7))}
    full = dict(host, ess_lags=np.int64(8), ess=rng.random((2, 7)), ess_lag=rng.integers(0, 8, (2, 7)).astype(np.int32))
    p = PxMCMCParams(nsamples=5, nburn=2, ngap=1, track=["logposterior"])
    r.summary = {"state": _FakeSummary(full)}
    data, attrs = load_mcmc(save_mcmc(r, p, str(tmp_path), filename="ess"))
    assert {k for k in data if k.startswith("summary_")} == {f"summary_state_{f}" for f in ("count", "mean", "m2", "ess", "ess_lag")}
    assert attrs["summary_ess_lags"] == 8
    back = load_summaries(data, attrs)["state"]
    assert set(back) == set(full)
    for k in back:
        np.testing.assert_array_equal(back[k], full[k])
    assert back["ess_lag"].dtype == np.int32
    r.summary = {"state": _FakeSummary(host)}  # without the keyword: the file of before
    data0, attrs0 = load_mcmc(save_mcmc(r, p, str(tmp_path), filename="plain"))
    assert {k for k in data0 if k.startswith("summary_")} == {f"summary_state_{f}" for f in ("count", "mean", "m2")}
    assert "summary_ess_lags" not in attrs0 and set(attrs0) == set(attrs) - {"summary_ess_lags"}


def test_constructors_validate_the_lags():
    """``PosteriorSummary(ess_lags=)`` checks before it touches the device; the samplers' ``summary_ess=`` on stub operators
    (constructing a sampler launches nothing)"""
    from pxmcmc_amd.mcmc import MYULA, SKROCK, PxMALA, PxMCMCParams
    from pxmcmc_amd.uncertainty import PosteriorSummary

    for bad in (0, 1, 3, 7, 66, -2):
        with pytest.raises(ValueError, match="ess_lags"):
            PosteriorSummary(2, 4, False, ess_lags=bad, device="cpu")

    class Transform:
        harmonic = False

        def inverse(self, X):
            return X

    class Forward:
        setting, nparams, data = "synthesis", 8, np.zeros(8)
        transform = Transform()

    p = PxMCMCParams(nsamples=2, nburn=0, ngap=1, verbosity=0)
    for cls in (MYULA, PxMALA, SKROCK):
        assert cls(Forward(), object(), p).summary_ess is None
        assert cls(Forward(), object(), p, summary="state", summary_ess=8).summary_ess == 8
        with pytest.raises(ValueError, match="summary_ess needs summary"):
            cls(Forward(), object(), p, summary_ess=8)
        for bad in (0, 5, 128):
            with pytest.raises(ValueError, match="ess_lags"):
                cls(Forward(), object(), p, summary="state", summary_ess=bad)


def test_acov_entry_points_reject_bad_arguments():
    import ctypes

    from pxmcmc_amd import _lib

    lib = _lib.lib
    buf = (ctypes.c_double * 64)()
    cnt = (ctypes.c_int64 * 2)()
    lag = (ctypes.c_int * 16)()
    a = ctypes.addressof
    b = a(buf)
    upd = lambda x, xs, c, acc, ring, m, C, K: lib.pxm_acov_update(x, xs, c, acc, acc, acc, ring, None, m, C, K, None)  # noqa: E731
    for args, text in (
        ((b, 1, a(cnt), b, b, 4, 0, 2), "C"),
        ((b, 1, a(cnt), b, b, 0, 2, 2), "m >= 1"),
        ((b, 1, a(cnt), b, b, 4, 2, 0), "K must be even"),
        ((b, 1, a(cnt), b, b, 4, 2, 3), "K must be even"),
        ((b, 1, a(cnt), b, b, 4, 2, 66), "K must be even"),
        ((None, 1, a(cnt), b, b, 4, 2, 2), "null buffer"),
        ((b, 1, None, b, b, 4, 2, 2), "null buffer"),
        ((b, 1, a(cnt), None, b, 4, 2, 2), "null buffer"),
        ((b, 1, a(cnt), b, None, 4, 2, 2), "null buffer"),
        ((b, 3, a(cnt), b, b, 4, 2, 2), "x_stride"),
        ((b, 1, a(cnt), b, b, 2 ** 58, 2, 64), "overflows"),
    ):
        assert upd(*args) < 0
        assert text in lib.pxm_last_error().decode(), (text, lib.pxm_last_error().decode())
    ess = lambda c, acc, m, C, K, out, lg, pooled, mcse, stats, scr: lib.pxm_acov_ess(c, acc, acc, acc, acc, m, C, K, out, lg, pooled, mcse, stats, scr, None)  # noqa: E731
    for args, text in (
        ((a(cnt), b, 4, 0, 2, b, a(lag), None, None, None, None), "C >= 1"),
        ((a(cnt), b, 0, 2, 2, b, a(lag), None, None, None, None), "m >= 1"),
        ((a(cnt), b, 4, 2, 5, b, a(lag), None, None, None, None), "K must be even"),
        ((a(cnt), None, 4, 2, 2, b, a(lag), None, None, None, None), "null buffer"),
        ((a(cnt), b, 4, 2, 2, None, a(lag), None, None, None, None), "null buffer"),
        ((a(cnt), b, 4, 2, 2, b, None, None, None, None, None), "null buffer"),
        ((a(cnt), b, 4, 2, 2, b, a(lag), None, b, None, None), "mcse needs ess_pooled"),
        ((a(cnt), b, 4, 2, 2, b, a(lag), None, None, b, None), "stats needs scratch"),
    ):
        assert ess(*args) < 0
        assert text in lib.pxm_last_error().decode(), (text, lib.pxm_last_error().decode())
    assert lib.pxm_acov_stage_depth() == 16
    assert lib.pxm_acov_state_doubles(5, 3, 32) == 480 and lib.pxm_acov_ring_doubles(5, 3, 32) == 15 * 47
    for bad in ((0, 1, 2), (4, 0, 2), (4, 1, 0), (4, 1, 3), (4, 1, 66), (2 ** 58, 2, 64)):
        assert lib.pxm_acov_state_doubles(*bad) == -1 and lib.pxm_acov_ring_doubles(*bad) == -1
    assert lib.pxm_acov_scratch_doubles(0) == -1 and lib.pxm_acov_scratch_doubles(100) == 6 and lib.pxm_acov_scratch_doubles(10 ** 9) == 3 * 1024
