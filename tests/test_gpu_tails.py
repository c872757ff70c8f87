"""Exact streaming credible intervals on the device: k_tails_update / k_tails_quantiles against the
numpy statements of tests/test_tails_host.py, against ``ops.quantile_range`` of the saved chain (bit for bit) and against
``numpy.quantile``; masks, early and late read-outs, smaller alpha, graph capture, the samplers' ``summary_alpha=`` keyword
and the saved run."""
import numpy as np
import pytest

from test_gpu_moments import _quiet, _wavelet_problem
from test_tails_host import assert_bit_equal, tail_columns, tails_of

pytestmark = pytest.mark.gpu

CMAX = 4  # every buffer of the kernel sweep is allocated for 4 chains
MODES = ("real", "components", "realparts")
# (alpha, N): k = 2; 3; 4; 4; 2 (k < N = 3); k = N = 2 (the tails never get past the fill phase); k = N = 1;
# k = 2 with N - k = 32, two full rings of staged saves and none left at the end (40 and 41 leave some for the read-out)
ALPHA_N = ((0.05, 40), (0.05, 41), (0.1, 41), (0.5, 9), (0.05, 3), (0.05, 2), (0.05, 1), (0.05, 34))
SLOTS = (2, 3, 4, 4, 2, 2, 1, 2)


def _dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _columns(T, C, m, seed, nan=False):
    """[T, C, m]: chain c draws tail_columns with its own seed, so its column kinds are shifted by c"""
    return np.ascontiguousarray(np.stack([tail_columns(T, m, seed + c, nan=nan) for c in range(C)], axis=1))


class _Tails:
    """caller-owned state of the tails entry points for C chains of mm components, allocated for CMAX chains with NaN beyond
    C (count: -7), and the updates that feed it.  ``mode`` as in tests/test_gpu_moments.py: "real" float64 [C, m];
    "components" a complex128 [C, m] state passed as its 2 m real components; "realparts" complex128 [C, m] whose real parts
    are kept (x_stride 2)."""

    def __init__(self, C, mm, alpha, N, mode="real"):
        import torch

        from pxmcmc_amd import ops
        from pxmcmc_amd.uncertainty import tail_capacity

        self.C, self.mm, self.N, self.alpha, self.mode = C, mm, N, alpha, mode
        self.k = tail_capacity(alpha, N)
        nan = float("nan")
        self.count = torch.full((CMAX,), -7, dtype=torch.int64, device="cuda")
        self.lo = torch.full((CMAX, self.k, mm), nan, dtype=torch.float64, device="cuda")
        self.hi = self.lo.clone()
        self.thr_lo = torch.full((CMAX, mm), nan, dtype=torch.float64, device="cuda")
        self.thr_hi = self.thr_lo.clone()
        self.stage = torch.full((CMAX, ops.tails_stage_depth(), mm), nan, dtype=torch.float64, device="cuda")
        self.count[:C] = 0
        self.xbuf = torch.full((CMAX, mm), nan, dtype=torch.complex128 if mode == "realparts" else torch.float64, device="cuda")
        self.junk = np.random.default_rng(mm).normal(size=(C, mm))  # imaginary parts of a "realparts" batch: never read

    def state(self):
        return self.count, self.lo, self.hi, self.thr_lo, self.thr_hi, self.stage

    def update(self, x_t, mask=None):
        """one save of the batch x_t [C, mm] (real components); the counts advance as pxm_moments_update advances them"""
        from pxmcmc_amd import ops

        C = self.C
        self.xbuf[:C] = _dev(x_t + 1j * self.junk) if self.mode == "realparts" else _dev(x_t)
        ops.tails_update(self.xbuf[:C], self.count[:C], self.lo[:C], self.hi[:C], self.thr_lo[:C], self.thr_hi[:C], self.stage[:C], self.N, mask=mask)
        self.count[:C] += 1 if mask is None else mask.to(self.count.dtype)

    def quantiles(self, alpha=None):
        from pxmcmc_amd import ops

        C = self.C
        q_lo, q_hi = ops.tails_quantiles(self.count[:C], self.lo[:C], self.hi[:C], self.stage[:C], self.N, self.alpha if alpha is None else alpha)
        return q_lo.cpu().numpy(), q_hi.cpu().numpy()

    def assert_untouched_beyond_C(self, what):
        C = self.C
        assert (self.count[C:] == -7).all(), what
        for t in (self.lo, self.hi, self.thr_lo, self.thr_hi, self.stage, self.xbuf):
            assert bool(t[C:].isnan().all()), what


def _check_chain(q_lo, q_hi, samples, a_read, alpha, N, what, numpy_too=True):
    """q_lo / q_hi [mm] of one chain, read at ``a_read`` from tails sized for (alpha, N), against its samples [n, mm]:
    bit-equal to the numpy route through such tails and, as a range, to ops.quantile_range of the chain on the device; equal
    to numpy.quantile (``numpy_too``: numpy returns NaN for a column with NaN, those are left to the device comparison)"""
    from pxmcmc_amd import ops
    from pxmcmc_amd.uncertainty import tail_capacity, tails_quantiles_np

    n, lo, hi = tails_of(samples, tail_capacity(alpha, N), N)
    w_lo, w_hi = tails_quantiles_np([n], lo[None], hi[None], a_read, N)
    assert_bit_equal(q_lo, w_lo[0], what)
    assert_bit_equal(q_hi, w_hi[0], what)
    with np.errstate(invalid="ignore"):
        assert_bit_equal(q_hi - q_lo, ops.quantile_range(_dev(samples), a_read).cpu().numpy(), what)
        if numpy_too:
            want = np.quantile(samples, (a_read / 2, 1 - a_read / 2), axis=0)
            np.testing.assert_array_equal(q_lo, want[0], err_msg=str(what))
            np.testing.assert_array_equal(q_hi, want[1], err_msg=str(what))


def _sweep_case(m, C, mode, alpha, N, k):
    mm = 2 * m if mode == "components" else m
    t = _Tails(C, mm, alpha, N, mode)
    assert t.k == k
    x = _columns(N, C, mm, seed=m + N)
    for i in range(N):
        t.update(x[i])
    what = (m, C, mode, alpha, N)
    assert t.count[:C].tolist() == [N] * C
    t.assert_untouched_beyond_C(what)
    q_lo, q_hi = t.quantiles()
    for c in range(C):
        _check_chain(q_lo[c], q_hi[c], x[:, c], alpha, alpha, N, what + (c,))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 257, 1025, 8193])
def test_tails_kernels_elementwise(m, C):
    """every instantiation (x_stride 1 | 2, the complex "components" layout), every capacity case; odd m puts every other row
    8 bytes off a 16-byte boundary (scalar head / tail), m = 1025 is one unrolled pass and a remainder, m = 8193 four
    workgroups"""
    for mode in MODES:
        for (alpha, N), k in zip(ALPHA_N, SLOTS):
            _sweep_case(m, C, mode, alpha, N, k)


def test_nan_columns_are_ordered_as_the_chain_kernel_orders_them():
    """NaN of either sign in a column (below -inf / above +inf by the key): bit-equal to ops.quantile_range of the chain;
    numpy, which returns NaN for such a column, is not consulted"""
    C, m, alpha, N = 2, 257, 0.1, 41
    x = _columns(N, C, m, seed=5, nan=True)
    assert np.isnan(x).any() and (np.signbit(x) & np.isnan(x)).any()
    t = _Tails(C, m, alpha, N)
    for i in range(N):
        t.update(x[i])
    q_lo, q_hi = t.quantiles()
    for c in range(C):
        _check_chain(q_lo[c], q_hi[c], x[:, c], alpha, alpha, N, ("nan", c), numpy_too=False)


def test_masks_and_per_chain_counts():
    """start counts 0, 1, 2 by masked rounds, then full rounds: every chain's intervals are those of its own samples; an
    all-off update changes nothing, bit for bit"""
    import torch

    C, m, alpha, N = 3, 131, 0.1, 41
    start = [0, 1, 2]
    T = N - 2  # chain c ends with start[c] + T - 2 <= N samples
    x = _columns(T, C, m, seed=9)
    t = _Tails(C, m, alpha, N)
    seen = [[] for _ in range(C)]
    for i in range(T):
        on = [int(i < start[c]) for c in range(C)] if i < 2 else [1] * C
        t.update(x[i], mask=_dev(np.array(on, dtype=np.int32)) if i < 2 or i % 2 else None)
        for c in range(C):
            if on[c]:
                seen[c].append(x[i, c])
    assert t.count[:C].tolist() == [len(s) for s in seen] == [T - 2, T - 1, T]
    before = [a.clone() for a in t.state()]
    t.update(x[0] - 50.0, mask=torch.zeros(C, dtype=torch.int32, device="cuda"))
    for a, b in zip(before, t.state()):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    t.assert_untouched_beyond_C("masks")
    q_lo, q_hi = t.quantiles()
    for c in range(C):
        _check_chain(q_lo[c], q_hi[c], np.stack(seen[c]), alpha, alpha, N, ("masks", c))


def test_read_out_before_the_run_ends_and_at_smaller_alpha():
    """n < N (in the fill phase, just past it, and later) and alpha' < alpha equal the chain route at that n and alpha'; a
    chain without samples reads NaN"""
    C, m, alpha, N = 2, 65, 0.1, 100
    x = _columns(N, C, m, seed=2)
    t = _Tails(C, m, alpha, N)
    assert t.k == 6
    q_lo, q_hi = t.quantiles()
    assert np.isnan(q_lo).all() and np.isnan(q_hi).all() and q_lo.shape == (C, m)
    for i in range(N):
        t.update(x[i])
        if i + 1 in (1, 2, 5, 6, 7, 23, 64, 100):
            for a in (alpha, alpha / 2, alpha / 5):
                q_lo, q_hi = t.quantiles(a)
                for c in range(C):
                    _check_chain(q_lo[c], q_hi[c], x[: i + 1, c], a, alpha, N, (i + 1, a, c))


def test_more_updates_than_declared_are_refused_and_leave_the_state():
    import torch

    from pxmcmc_amd._lib import PxmError
    from pxmcmc_amd.uncertainty import PosteriorSummary

    C, m, alpha, N = 2, 33, 0.5, 9
    x = _columns(N + 1, C, m, seed=4)
    s = PosteriorSummary(C, m, False, best=False, alpha=alpha, nsamples=N)
    assert s.tail_slots == 4 and s.tail_bytes() == (2 * 4 + 2 + 16) * 8 * C * m
    for i in range(N):
        s.update(_dev(x[i]))
    rng_ok = s.credible_interval_range().cpu().numpy()
    tails = (s._lo, s._hi, s._thr_lo, s._thr_hi, s._stage)
    before = [a.clone() for a in tails]
    s.update(_dev(x[N] - 100.0))  # would enter every lower tail
    assert s.counts.tolist() == [N + 1] * C
    for a, b in zip(before, tails):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    with pytest.raises(PxmError, match="sized for 9"):
        s.credible_interval()
    with pytest.warns(RuntimeWarning, match="sized for 9"):  # the rest of the summary can still be saved
        host = s.to_host()
    assert set(host) == {"count", "mean", "m2"}
    with pytest.raises(ValueError, match="sized for alpha"):
        PosteriorSummary(C, m, False, best=False, alpha=alpha, nsamples=N).credible_interval(0.6)
    with pytest.raises(ValueError, match="without alpha"):
        PosteriorSummary(C, m, False, best=False).credible_interval()
    with np.errstate(invalid="ignore"):  # (inf - inf in the +-inf columns)
        for c in range(C):
            np.testing.assert_array_equal(rng_ok[c], np.diff(np.quantile(x[:N, c], (alpha / 2, 1 - alpha / 2), axis=0), axis=0)[0])


@pytest.mark.parametrize("cplx", [False, True])
def test_posterior_summary_intervals(cplx):
    """the class on top: the tails pass runs before the moments pass of the same update (which advances the counts), the
    moments are those of a summary without tails, complex states come back complex per component, to_host carries the
    quantiles"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.uncertainty import PosteriorSummary

    C, n, alpha, N = 3, 65, 0.1, 41
    mm = 2 * n if cplx else n
    x = _columns(N, C, mm, seed=6)
    lp = np.random.default_rng(6).normal(size=(N, C))
    s, plain = PosteriorSummary(C, n, cplx, alpha=alpha, nsamples=N), PosteriorSummary(C, n, cplx)
    for i in range(N):
        xt = _dev(x[i])
        xt = torch.view_as_complex(xt.reshape(C, n, 2)) if cplx else xt
        s.update(xt, logpi=_dev(lp[i]))
        plain.update(xt, logpi=_dev(lp[i]))
    host, host_plain = s.to_host(), plain.to_host()
    assert set(host) == set(host_plain) | set(PosteriorSummary.TAIL_FIELDS) and host["alpha"] == alpha
    for k, v in host_plain.items():
        np.testing.assert_array_equal(host[k], v, err_msg=k)
    q_lo, q_hi = s.credible_interval()
    rng = s.credible_interval_range()
    assert q_lo.shape == q_hi.shape == rng.shape == (C, n) and q_lo.is_complex() == rng.is_complex() == cplx
    comp = (lambda t: torch.view_as_real(t).reshape(C, mm)) if cplx else (lambda t: t)
    chain = _dev(x)
    for c in range(C):
        want = ops.quantile_range(chain[:, c], alpha).cpu().numpy()
        assert_bit_equal(comp(rng)[c].cpu().numpy(), want, c)
        with np.errstate(invalid="ignore"):  # (inf - inf in the +-inf columns)
            np.testing.assert_array_equal(want, np.diff(np.quantile(x[:, c], (alpha / 2, 1 - alpha / 2), axis=0), axis=0)[0])
    np.testing.assert_array_equal(host["q_lo"], comp(q_lo).cpu().numpy())
    np.testing.assert_array_equal(host["q_hi"], comp(q_hi).cpu().numpy())
    half = ops.quantile_range(chain[:, 1], alpha / 2).cpu().numpy()
    assert_bit_equal(comp(s.credible_interval_range(alpha / 2))[1].cpu().numpy(), half)


def test_update_with_tails_is_capturable():
    """one captured update (tails pass + moments passes) replayed N times with the sample rewritten in place: state bit-equal
    to eager updates"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.uncertainty import PosteriorSummary

    C, m, alpha, N = 3, 1025, 0.1, 41
    x = _columns(N, C, m, seed=8)
    lp = np.random.default_rng(8).normal(size=(N, C))
    new = lambda: PosteriorSummary(C, m, False, alpha=alpha, nsamples=N)  # noqa: E731
    eager = new()
    for i in range(N):
        eager.update(_dev(x[i]), logpi=_dev(lp[i]))
    X, LP = _dev(x[0]), _dev(lp[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        new().update(X, logpi=LP)  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = new()
    g = torch.cuda.CUDAGraph()
    with ops.capture_scope(), torch.cuda.graph(g):
        graph.update(X, logpi=LP)
    assert int(graph.counts.sum()) == 0  # capture does not execute
    xs, lps = _dev(x), _dev(lp)
    for i in range(N):
        X.copy_(xs[i])
        LP.copy_(lps[i])
        g.replay()
    torch.cuda.synchronize()
    for a, b in zip((eager._lo, eager._hi, eager._thr_lo, eager._thr_hi), (graph._lo, graph._hi, graph._thr_lo, graph._thr_hi)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    for k, v in eager.to_host().items():
        np.testing.assert_array_equal(graph.to_host()[k], v, err_msg=k)


# ---- samplers ----------------------------------------------------------------------------------------------------------------
NS, ALPHA = 41, 0.1
RUNS = {}  # (algo, with tails) -> (sampler, operator, params): each run is made once and shared by the tests below


def _run(algo, tails):
    from conftest import golden
    from pxmcmc_amd.mcmc import MYULA, SKROCK, PxMALA, PxMCMCParams

    if (algo, tails) in RUNS:
        return RUNS[algo, tails]
    C = 3
    kw = dict(nchains=C, seed=2, summary=("state", "image"), summary_alpha=ALPHA if tails else None)
    track = ["logposterior", "L2", "prior", "chain"]
    if algo == "pxmala":  # step size of the G4 set-up (tests/golden/g4_pxmala.npz); max_iter stops the slower chains early
        lmda, delta, mu = (float(v) for v in golden("g4_pxmala.npz")["params"][:3])
        op, reg = _wavelet_problem(C, lmda=lmda * mu)
        p = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, nsamples=NS, nburn=3, ngap=2, verbosity=0, track=track)
        s = PxMALA(op, reg, p, tune_delta=True, max_iter=120, **kw)
    else:
        op, reg = _wavelet_problem(C)
        if algo == "myula":
            p = PxMCMCParams(lmda=1e-3, delta=5e-4, ngap=2, nsamples=NS, nburn=3, verbosity=0, track=track)
            s = MYULA(op, reg, p, **kw)
        else:
            p = PxMCMCParams(lmda=1e-3, delta=2e-3, ngap=1, s=3, nsamples=NS, nburn=3, verbosity=0, track=track)
            s = SKROCK(op, reg, p, **kw)
    _quiet(s.run, start_point=np.zeros(op.nparams))
    RUNS[algo, tails] = (s, op, p)
    return RUNS[algo, tails]


@pytest.mark.parametrize("algo", ["myula", "skrock", "pxmala"])
def test_sampler_intervals_equal_those_of_the_saved_chain(algo):
    """summary[space].credible_interval_range() per chain against uncertainty.credible_interval_range of that chain's saved
    samples (the image space: mapped through chain_to_images, per real component) -- on the device route bit for bit, on the
    numpy route equal; the run itself and its other summary fields are those of the run without summary_alpha"""
    import torch

    from pxmcmc_amd.uncertainty import chain_to_images, credible_interval_range

    s, op, _ = _run(algo, True)
    plain, _, _ = _run(algo, False)
    for k in ("chain", "logPi", "L2s", "priors"):
        np.testing.assert_array_equal(getattr(s, k), getattr(plain, k), err_msg=k)
    C = s.nchains
    counts = s.summary["state"].counts.tolist()
    if algo == "pxmala":  # masked saves, chains stopped at different counts below N
        assert s.stopped_early and len(set(counts)) > 1 and min(counts) >= 1 and max(counts) <= NS, counts
    else:
        assert counts == [NS] * C
    for space in ("state", "image"):
        summ = s.summary[space]
        assert summ.alpha == ALPHA and summ.nsamples == NS and summ.tail_slots == 4 and plain.summary[space].alpha is None
        host, host_plain = summ.to_host(), plain.summary[space].to_host()
        assert set(host) == set(host_plain) | {"alpha", "q_lo", "q_hi"}
        for k, v in host_plain.items():
            np.testing.assert_array_equal(host[k], v, err_msg=f"{space} {k}")
        rng = summ.credible_interval_range()
        rng = (torch.view_as_real(rng).reshape(C, -1) if rng.is_complex() else rng).cpu().numpy()
        for c in range(C):
            saved = s.chain[c][: counts[c]]
            if space == "image":
                saved = np.ascontiguousarray(chain_to_images(saved, op.transform))
                saved = saved.view(np.float64).reshape(saved.shape[0], -1)
            assert_bit_equal(rng[c], credible_interval_range(_dev(saved), ALPHA).cpu().numpy(), (algo, space, c))
            np.testing.assert_array_equal(rng[c], credible_interval_range(saved, ALPHA), err_msg=str((algo, space, c)))


def test_save_and_load_round_trip_the_intervals(tmp_path):
    from pxmcmc_amd.saving import load_mcmc, load_summaries, save_mcmc

    s, _, p = _run("myula", True)
    plain, _, p0 = _run("myula", False)
    data, attrs = load_mcmc(save_mcmc(s, p, str(tmp_path), filename="tails"))
    data0, attrs0 = load_mcmc(save_mcmc(plain, p0, str(tmp_path), filename="plain"))
    fields = ("count", "mean", "m2", "best", "best_logpi")
    assert {k for k in data0 if k.startswith("summary_")} == {f"summary_{sp}_{f}" for sp in ("state", "image") for f in fields}
    assert set(data) - set(data0) == {f"summary_{sp}_{f}" for sp in ("state", "image") for f in ("q_lo", "q_hi")}
    assert attrs["summary_alpha"] == ALPHA and "summary_alpha" not in attrs0
    back = load_summaries(data, attrs)
    for space in ("state", "image"):
        host = s.summary[space].to_host()
        assert set(back[space]) == set(host)
        for k, v in host.items():
            np.testing.assert_array_equal(back[space][k], v, err_msg=f"{space} {k}")
