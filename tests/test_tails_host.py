"""Host side of the exact streaming credible intervals (no GPU needed): the capacity rule
``uncertainty.tail_capacity`` against the brute-force minimum, the numpy statements ``tails_update_np`` /
``tails_quantiles_np`` against ``numpy.quantile`` bit for bit, their error paths, ``PosteriorSummary.merge`` with the new
keys, and the argument checks of the C-ABI.

tests/test_gpu_tails.py imports the columns and the numpy route from here."""
import numpy as np
import pytest

KINDS = ("random", "tied", "constant", "increasing", "decreasing", "inf")
ALPHAS = (0.01, 0.05, 0.1, 0.32, 0.5, 1.0)


def tail_columns(n, m, seed, nan=False):
    """[n, m] samples whose column j is of kind KINDS[(j + seed) % 6]: standard normal; rounded to 0.1 (ties); constant;
    strictly increasing; strictly decreasing (every sample enters one tail); normal with +-inf entries.  ``nan``: every
    seventh column also gets NaNs of both signs"""
    rng = np.random.default_rng([seed, n, m])
    x = rng.normal(size=(n, m))
    kind = (np.arange(m) + seed) % len(KINDS)
    x[:, kind == 1] = np.round(x[:, kind == 1], 1) + 0.0  # (no -0.0: numpy orders it with +0.0 arbitrarily, the key below it)
    x[:, kind == 2] = rng.normal(size=(kind == 2).sum())
    ramp = np.arange(n, dtype=np.float64)[:, None] * 0.37
    x[:, kind == 3] = x[:1, kind == 3] + ramp
    x[:, kind == 4] = x[:1, kind == 4] - ramp
    cols = np.flatnonzero(kind == 5)
    rows = rng.integers(0, n, size=(max(1, n // 8), cols.size))
    x[rows, cols[None, :]] = rng.choice([-np.inf, np.inf], size=rows.shape)
    if nan:
        cols = np.arange(0, m, 7)
        rows = rng.integers(0, n, size=(max(1, n // 10), cols.size))
        x[rows, cols[None, :]] = rng.choice([np.nan, -np.nan], size=rows.shape)
    return x


def assert_bit_equal(got, want, what=""):
    """the same bit patterns, any NaN standing for any other (numpy and the device differ in the NaN they produce)"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape, what)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=str(what))
    np.testing.assert_array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan], err_msg=str(what))


def tails_of(x, k, nsamples, count=0, lo=None, hi=None):
    """run tails_update_np over the rows of x [n, m] -> (count, lo [k, m], hi [k, m])"""
    from pxmcmc_amd.uncertainty import tails_update_np

    m = x.shape[1]
    lo = np.full((k, m), np.nan) if lo is None else lo
    hi = np.full((k, m), np.nan) if hi is None else hi
    for row in x:
        tails_update_np(row, count, lo, hi, nsamples)
        count += 1
    return count, lo, hi


def quantiles_via_tails(x, alpha, nsamples, alpha_read=None):
    """(q_lo, q_hi) [m] of the samples x [n, m] by the numpy route, tails sized for (alpha, nsamples)"""
    from pxmcmc_amd.uncertainty import tail_capacity, tails_quantiles_np

    k = tail_capacity(alpha, nsamples)
    n, lo, hi = tails_of(x, k, nsamples)
    q_lo, q_hi = tails_quantiles_np([n], lo[None], hi[None], alpha if alpha_read is None else alpha_read, nsamples)
    return q_lo[0], q_hi[0]


def _split(q, n):
    vi = q * (n - 1)
    fl = min(np.floor(vi), n - 1)
    return int(fl), vi - fl


def _needed(alpha, n):
    """smallest tail length that holds both pairs of order statistics of the read-out at n samples"""
    i_lo, _ = _split(alpha / 2, n)
    i_hi, _ = _split(1 - alpha / 2, n)
    return min(n, max(min(i_lo + 1, n - 1) + 1, n - i_hi))


@pytest.mark.parametrize("alpha", ALPHAS)
def test_tail_capacity_is_the_brute_force_minimum(alpha):
    from pxmcmc_amd.uncertainty import tail_capacity

    for N in range(1, 301):
        k = tail_capacity(alpha, N)
        assert 1 <= k <= N
        assert k == _needed(alpha, N), (alpha, N)
        for n in range(1, N + 1):  # every read-out on the way fits in the slots that hold samples
            assert _needed(alpha, n) <= min(k, n), (alpha, N, n)


def test_tail_capacity_serves_every_count_of_the_documented_run():
    """alpha = 0.05, N = 1000 (k = 26), the configuration DESIGN.md section 15 documents and times: the read-out at every
    n <= N and at alpha' in {alpha, alpha / 2, alpha / 5} fits in the slots that hold samples"""
    from pxmcmc_amd.uncertainty import tail_capacity

    alpha, N = 0.05, 1000
    k = tail_capacity(alpha, N)
    assert k == 26 == _needed(alpha, N)
    for a in (alpha, alpha / 2, alpha / 5):
        for n in range(1, N + 1):
            assert _needed(a, n) <= min(k, n), (a, n)


def test_tail_capacity_examples_and_errors():
    from pxmcmc_amd.uncertainty import tail_capacity

    assert tail_capacity(0.05, 1000) == 26
    assert all(tail_capacity(0.05, N) == 2 for N in range(2, 41))
    assert tail_capacity(0.05, 41) == 3 and tail_capacity(0.05, 100) == 4
    assert tail_capacity(0.1, 41) == 4 and tail_capacity(0.5, 9) == 4 and tail_capacity(0.05, 3) == 2 and tail_capacity(0.05, 2) == 2 and tail_capacity(0.05, 1) == 1
    for bad in (0.0, -0.1, 1.5, np.nan):
        with pytest.raises(ValueError):
            tail_capacity(bad, 10)
    with pytest.raises(ValueError):
        tail_capacity(0.05, 0)


@pytest.mark.parametrize("alpha,N", [(0.05, 40), (0.05, 41), (0.1, 41), (0.5, 9), (0.05, 3), (0.05, 2), (0.05, 1), (0.01, 300), (0.32, 77), (1.0, 12)])
def test_numpy_route_is_bit_equal_to_numpy_quantile(alpha, N):
    for seed in range(2):
        x = tail_columns(N, 13, seed)
        for n in sorted({N, max(1, N // 2), max(1, N - 1), 1}):
            for a in (alpha, alpha / 2, alpha / 5):
                q_lo, q_hi = quantiles_via_tails(x[:n], alpha, N, a)
                with np.errstate(invalid="ignore"):
                    want = np.quantile(x[:n], (a / 2, 1 - a / 2), axis=0)
                assert_bit_equal(q_lo, want[0], (alpha, N, n, a))
                assert_bit_equal(q_hi, want[1], (alpha, N, n, a))


def test_numpy_route_continues_from_its_state_and_ignores_extra_updates():
    from pxmcmc_amd.uncertainty import tail_capacity, tails_quantiles_np

    x = tail_columns(41, 12, 3)
    k = tail_capacity(0.1, 41)
    n1, lo, hi = tails_of(x[:17], k, 41)
    n2, lo, hi = tails_of(x[17:], k, 41, n1, lo, hi)
    _, lo_w, hi_w = tails_of(x, k, 41)
    np.testing.assert_array_equal(np.sort(lo, axis=0), np.sort(lo_w, axis=0))
    np.testing.assert_array_equal(np.sort(hi, axis=0), np.sort(hi_w, axis=0))
    before = lo.copy(), hi.copy()
    n3, lo, hi = tails_of(x[:1] - 100.0, k, 41, n2, lo, hi)  # update 42 of 41: left untouched, reported by the read-out
    assert n3 == 42 and np.array_equal(lo, before[0]) and np.array_equal(hi, before[1])
    with pytest.raises(ValueError, match="sized for 41"):
        tails_quantiles_np([n3], lo[None], hi[None], 0.1, 41)
    # a chain without samples: NaN; chains of a batch are read at their own counts
    q_lo, q_hi = tails_quantiles_np([0, 41], np.stack([lo, lo]), np.stack([hi, hi]), 0.1, 41)
    assert np.isnan(q_lo[0]).all() and np.isnan(q_hi[0]).all()
    with np.errstate(invalid="ignore"):  # (inf - inf in the +-inf columns)
        np.testing.assert_array_equal(q_hi[1] - q_lo[1], np.diff(np.quantile(x, (0.05, 0.95), axis=0), axis=0)[0])


def test_error_paths():
    from pxmcmc_amd.uncertainty import PosteriorSummary, tail_capacity, tails_quantiles_np

    x = tail_columns(100, 6, 0)
    k = tail_capacity(0.05, 100)
    n, lo, hi = tails_of(x, k, 100)
    with pytest.raises(ValueError, match="outside tails"):  # alpha' > alpha
        tails_quantiles_np([n], lo[None], hi[None], 0.2, 100)
    with pytest.raises(ValueError):
        tails_quantiles_np([n], lo[None], hi[None], 1.5, 100)
    with pytest.raises(ValueError):
        tails_quantiles_np([n, n], lo[None], hi[None], 0.05, 100)
    # the constructor checks its arguments before it touches the device
    with pytest.raises(ValueError, match="nsamples"):
        PosteriorSummary(2, 4, False, alpha=0.05)
    for bad in (0.0, 1.01, -0.5):
        with pytest.raises(ValueError, match="alpha"):
            PosteriorSummary(2, 4, False, alpha=bad, nsamples=10, device="cpu")
    with pytest.raises(ValueError, match="nsamples"):
        PosteriorSummary(2, 4, False, alpha=0.05, nsamples=0, device="cpu")


def test_merge_carries_the_tail_keys():
    from pxmcmc_amd.uncertainty import PosteriorSummary

    rng = np.random.default_rng(11)
    base = [{"count": np.array([5, 5]), "mean": rng.normal(size=(2, 6)), "m2": rng.random((2, 6))} for _ in range(2)]
    plain = PosteriorSummary.merge(base)
    assert set(plain) == {"count", "mean", "m2"} and PosteriorSummary.FIELDS == ("count", "mean", "m2", "best", "best_logpi")
    with_tails = [dict(d, alpha=np.float64(0.1), q_lo=rng.normal(size=(2, 6)), q_hi=rng.normal(size=(2, 6))) for d in base]
    whole = PosteriorSummary.merge(with_tails)
    assert set(whole) == {"count", "mean", "m2"} | set(PosteriorSummary.TAIL_FIELDS)
    assert whole["alpha"] == 0.1 and whole["q_lo"].shape == (4, 6)
    np.testing.assert_array_equal(whole["q_hi"], np.concatenate([d["q_hi"] for d in with_tails]))
    for k in plain:
        np.testing.assert_array_equal(whole[k], plain[k])
    mixed = PosteriorSummary.merge([with_tails[0], base[1]])  # not every dict has them: today's result
    assert set(mixed) == set(plain)
    for k in plain:
        np.testing.assert_array_equal(mixed[k], plain[k])
    with pytest.raises(ValueError, match="different alpha"):
        PosteriorSummary.merge([with_tails[0], dict(with_tails[1], alpha=np.float64(0.05))])


class _FakeSummary:
    def __init__(self, host):
        self._host = host

    def to_host(self):
        return self._host


def test_save_and_load_round_trip_the_quantiles(tmp_path):
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.saving import load_mcmc, load_summaries, save_mcmc

    class Run:
        pass

    rng = np.random.default_rng(12)
    r = Run()
    r.logPi = rng.normal(size=(2, 5))
    host = {"count": np.array([5, 5]), "mean": rng.normal(size=(2, 7)), "m2": rng.random((2, 7))}
    tails = dict(host, alpha=np.float64(0.1), q_lo=rng.normal(size=(2, 7)), q_hi=rng.normal(size=(2, 7)))
    p = PxMCMCParams(nsamples=5, nburn=2, ngap=1, track=["logposterior"])
    r.summary = {"state": _FakeSummary(tails)}
    data, attrs = load_mcmc(save_mcmc(r, p, str(tmp_path), filename="tails"))
    assert {k for k in data if k.startswith("summary_")} == {f"summary_state_{f}" for f in ("count", "mean", "m2", "q_lo", "q_hi")}
    assert attrs["summary_alpha"] == 0.1
    back = load_summaries(data)["state"]
    assert set(back) == {"count", "mean", "m2", "q_lo", "q_hi"}
    for k in back:
        np.testing.assert_array_equal(back[k], tails[k])
    assert load_summaries(data, attrs)["state"]["alpha"] == 0.1
    r.summary = {"state": _FakeSummary(host)}  # no tails: today's names and attributes
    data0, attrs0 = load_mcmc(save_mcmc(r, p, str(tmp_path), filename="plain"))
    assert {k for k in data0 if k.startswith("summary_")} == {f"summary_state_{f}" for f in ("count", "mean", "m2")}
    assert "summary_alpha" not in attrs0 and set(attrs0) == set(attrs) - {"summary_alpha"}


def test_summary_alpha_keyword_is_validated():
    """the samplers' ``summary_alpha=`` keyword on stub operators (constructing a sampler launches nothing)"""
    from pxmcmc_amd.mcmc import MYULA, SKROCK, PxMALA, PxMCMCParams

    class Transform:
        harmonic = False

        def inverse(self, X):
            return X

    class Forward:
        setting, nparams, data = "synthesis", 8, np.zeros(8)
        transform = Transform()

    p = PxMCMCParams(nsamples=2, nburn=0, ngap=1, verbosity=0)
    for cls in (MYULA, PxMALA, SKROCK):
        assert cls(Forward(), object(), p).summary_alpha is None
        assert cls(Forward(), object(), p, summary="state", summary_alpha=0.05).summary_alpha == 0.05
        with pytest.raises(ValueError, match="summary_alpha needs summary"):
            cls(Forward(), object(), p, summary_alpha=0.05)
        for bad in (0.0, 1.5):
            with pytest.raises(ValueError, match="alpha"):
                cls(Forward(), object(), p, summary="state", summary_alpha=bad)


def test_tails_entry_points_reject_bad_arguments():
    import ctypes

    from pxmcmc_amd import _lib

    lib = _lib.lib
    buf = (ctypes.c_double * 64)()
    cnt = (ctypes.c_int64 * 2)()
    a = ctypes.addressof
    b = a(buf) + (-a(buf)) % 16
    upd = lambda x, xs, c, lo, thr, m, C, k, N: lib.pxm_tails_update(x, xs, c, lo, lo, thr, thr, lo, None, m, C, k, N, None)  # noqa: E731
    for args, text in (
        ((b, 1, a(cnt), b, b, 4, 0, 2, 10), "C"),
        ((b, 1, a(cnt), b, b, 0, 2, 2, 10), "m >= 1"),
        ((b, 1, a(cnt), b, b, 4, 2, 0, 10), "k <= nsamples"),
        ((b, 1, a(cnt), b, b, 4, 2, 11, 10), "k <= nsamples"),
        ((None, 1, a(cnt), b, b, 4, 2, 2, 10), "null buffer"),
        ((b, 1, None, b, b, 4, 2, 2, 10), "null buffer"),
        ((b, 1, a(cnt), b, None, 4, 2, 2, 10), "null buffer"),
        ((b, 3, a(cnt), b, b, 4, 2, 2, 10), "x_stride"),
        ((b + 8, 1, a(cnt), b, b, 4, 2, 2, 10), "16-byte"),
        ((b, 1, a(cnt), b, b + 8, 4, 2, 2, 10), "16-byte"),
        ((b, 1, a(cnt), b, b, 2 ** 40, 2, 2 ** 30, 2 ** 30), "overflows"),
    ):
        assert upd(*args) < 0
        assert text in lib.pxm_last_error().decode(), (text, lib.pxm_last_error().decode())
    qnt = lambda c, lo, m, C, k, N, alpha, out: lib.pxm_tails_quantiles(c, lo, lo, lo, m, C, k, N, alpha, out, out, None)  # noqa: E731
    for args, text in (
        ((a(cnt), b, 4, 0, 2, 10, 0.05, b), "C >= 1"),
        ((a(cnt), b, 0, 2, 2, 10, 0.05, b), "m >= 1"),
        ((a(cnt), b, 4, 2, 12, 10, 0.05, b), "k <= nsamples"),
        ((a(cnt), None, 4, 2, 2, 10, 0.05, b), "null buffer"),
        ((a(cnt), b, 4, 2, 2, 10, 0.05, None), "null buffer"),
        ((a(cnt), b, 4, 2, 2, 10, 1.5, b), "alpha"),
    ):
        assert qnt(*args) < 0
        assert text in lib.pxm_last_error().decode(), (text, lib.pxm_last_error().decode())
    assert lib.pxm_tails_buffer_doubles(0, 1, 1) == -1 and lib.pxm_tails_buffer_doubles(4, 0, 1) == -1
    assert lib.pxm_tails_buffer_doubles(4, 1, 0) == -1 and lib.pxm_tails_buffer_doubles(2 ** 40, 2, 2 ** 30) == -1
    assert lib.pxm_tails_buffer_doubles(5, 3, 26) == 390
    assert lib.pxm_tails_stage_doubles(5, 3) == 16 * 15 and lib.pxm_tails_stage_doubles(0, 1) == -1
