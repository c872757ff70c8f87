"""Streaming effective sample size on the device: k_acov_update / k_acov_ess against the numpy
statements of tests/test_ess_host.py -- the accumulators bit for bit, the cut of Geyer's sequence exactly, the estimates to
1e-13 --; run lengths around the merges of the ring, masks, read-outs in mid-run, NaN and inf, graph capture, the samplers'
``summary_ess=`` keyword and the saved run."""
import numpy as np
import pytest

from test_ess_host import acov_of, assert_bit_equal, ess_columns
from test_gpu_moments import _quiet, _wavelet_problem

pytestmark = pytest.mark.gpu

CMAX = 4  # every buffer of the kernel sweep is allocated for 4 chains
B = 16  # ops.acov_stage_depth(), asserted below
RTOL = 1e-13  # ess, ess_pooled and mcse against the numpy statement of the same operations (as finalize against rhat_np)
MODES = ("real", "components", "realparts")
# the lags of the sweep and the window length each is compiled at: K = 2, 4 -> k_acov_update<8>; 12 (K < KMAX, a ring of 27
# rows) and 16 (K = KMAX) -> <16>; 32 -> <32>; 64 -> <64>
KS_SWEEP = (2, 4, 12, 16, 32, 64)


def _dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _columns(T, C, m, seed):
    """[T, C, m]: chain c draws ess_columns with its own seed, so its column kinds are shifted by c"""
    return np.ascontiguousarray(np.stack([ess_columns(T, m, seed + c) for c in range(C)], axis=1))


def _checkpoints(K):
    """run lengths at which a run is read out: below 4 (no ESS), below K and below B, B - 1 saves pending, exactly on a
    merge, one past it, the same around later merges, and 3 (K + B) + 5, where the ring has wrapped more than once"""
    last = 3 * (K + B) + 5
    return sorted({3, 5, B - 1, B, B + 1, K - 1, K, K + 1, 2 * B - 1, 2 * B, K + B, 2 * (K + B) + B - 1, last} - {0, 1, 2}), last


class _Acov:
    """caller-owned state of the autocovariance entry points for C chains of mm components, allocated for CMAX chains and
    filled with NaN (count beyond C: -7; the state needs no initialisation), and the updates that feed it.  ``mode`` as in
    tests/test_gpu_tails.py"""

    def __init__(self, C, mm, K, mode="real"):
        import torch

        from pxmcmc_amd import ops

        assert ops.acov_stage_depth() == B
        self.C, self.mm, self.K, self.mode = C, mm, K, mode
        nan = float("nan")
        self.count = torch.full((CMAX,), -7, dtype=torch.int64, device="cuda")
        self.acc = torch.full((CMAX, K, mm), nan, dtype=torch.float64, device="cuda")
        self.head = self.acc.clone()
        self.tot = torch.full((CMAX, mm), nan, dtype=torch.float64, device="cuda")
        self.ring = torch.full((CMAX, K - 1 + B, mm), nan, dtype=torch.float64, device="cuda")
        self.count[:C] = 0
        self.xbuf = torch.full((CMAX, mm), nan, dtype=torch.complex128 if mode == "realparts" else torch.float64, device="cuda")
        self.junk = np.random.default_rng(mm).normal(size=(C, mm))  # imaginary parts of a "realparts" batch: never read

    def state(self):
        return self.count, self.acc, self.tot, self.head, self.ring

    def update(self, x_t, mask=None):
        """one save of the batch x_t [C, mm] (real components); the counts advance as pxm_moments_update advances them"""
        from pxmcmc_amd import ops

        C = self.C
        self.xbuf[:C] = _dev(x_t + 1j * self.junk) if self.mode == "realparts" else _dev(x_t)
        ops.acov_update(self.xbuf[:C], self.count[:C], self.acc[:C], self.tot[:C], self.head[:C], self.ring[:C], mask=mask)
        self.count[:C] += 1 if mask is None else mask.to(self.count.dtype)

    def read(self, pooled=True):
        from pxmcmc_amd import ops

        C = self.C
        out = ops.acov_ess(self.count[:C], self.acc[:C], self.tot[:C], self.head[:C], self.ring[:C], pooled=pooled)
        return [None if t is None else t.cpu().numpy() for t in out]

    def assert_untouched_beyond_C(self, what):
        C = self.C
        assert (self.count[C:] == -7).all(), what
        for t in (self.acc, self.tot, self.head, self.ring, self.xbuf):
            assert bool(t[C:].isnan().all()), what


def _close(got, want, what):
    """equal to RTOL, NaN where the numpy statement has NaN"""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(what))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0, err_msg=str(what))


class _Model:
    """the numpy route beside the device: the state of acov_update_np per chain, advanced save by save, and a copy of its
    acc and tot after the last complete block of B saves -- what the device has merged by then"""

    def __init__(self, C, mm, K):
        self.K = K
        self.state = [[0] + [np.full(sh, np.nan) for sh in ((K, mm), (mm,), (K, mm), (K, mm))] for _ in range(C)]
        self.merged = [None] * C

    def push(self, c, row):
        st = self.state[c]
        st[0], *st[1:] = acov_of(row[None], self.K, st[1:], st[0])
        if st[0] % B == 0:
            self.merged[c] = (st[1].copy(), st[2].copy())

    def push_all(self, x_t):
        for c, row in enumerate(x_t):
            self.push(c, row)

    def stacked(self):
        return (np.array([st[0] for st in self.state]),) + tuple(np.stack([st[i] for st in self.state]) for i in range(1, 5))


def _check_read_out(t, model, what, pooled=True):
    """the read-out of ``t`` against the numpy route ``model`` that saw the same saves: ess_lag exactly, ess / ess_pooled /
    mcse to RTOL, stats; acc and tot bit-equal to the numpy accumulators after the last complete block of every chain
    (untouched NaN before the first merge)"""
    from pxmcmc_amd.uncertainty import ess_np, ess_pooled_np

    C, K = t.C, t.K
    count, *stacked = model.stacked()
    assert t.count[:C].tolist() == count.tolist(), what
    ess, lag, ep, se, st = t.read(pooled)
    w_ess, w_lag = ess_np(count, *stacked)
    np.testing.assert_array_equal(lag, w_lag, err_msg=str(what))
    assert lag.dtype == np.int32
    _close(ess, w_ess, what)
    if pooled:
        w_ep, w_se = ess_pooled_np(count, *stacked)
        _close(ep, w_ep, what)
        _close(se, w_se, what)
    else:
        assert ep is None and se is None
    ok = ~np.isnan(w_ess)
    trunc = ok & (w_lag == 2 * (np.minimum(K, count)[:, None] // 2))
    assert st[1] == (~ok).sum() and st[2] == trunc.sum(), (what, st)
    if ok.any():
        np.testing.assert_allclose(st[0], w_ess[ok].min(), rtol=RTOL, err_msg=str(what))
    else:
        assert np.isnan(st[0]), what
    acc, tot = t.acc[:C].cpu().numpy(), t.tot[:C].cpu().numpy()
    for c in range(C):
        if model.merged[c] is None:
            assert np.isnan(acc[c]).all() and np.isnan(tot[c]).all(), what
            continue
        assert_bit_equal(acc[c], model.merged[c][0], what + ("acc", c))
        assert_bit_equal(tot[c], model.merged[c][1], what + ("tot", c))


def _sweep_case(m, C, K, mode):
    mm = 2 * m if mode == "components" else m
    t = _Acov(C, mm, K, mode)
    points, last = _checkpoints(K)
    x = _columns(last, C, mm, seed=m + K)
    model = _Model(C, mm, K)
    for i in range(last):
        t.update(x[i])
        model.push_all(x[i])
        if i + 1 in points:  # (a read-out in mid-run: the saves go on behind it)
            _check_read_out(t, model, (m, C, K, mode, i + 1))
    t.assert_untouched_beyond_C((m, C, K, mode))
    head, ring = t.head[:C].cpu().numpy(), t.ring[:C].cpu().numpy()
    R = K - 1 + B
    for c in range(C):  # the first K saves, and the last R at their rows
        assert_bit_equal(head[c], x[:K, c])
        for n in range(last - R, last):
            assert_bit_equal(ring[c, n % R], x[n, c])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 257, 1025, 8193])
def test_acov_kernels_elementwise(m, C, mode):
    """every compiled window length (KS_SWEEP) with x_stride 1 ("real"), x_stride 2 ("realparts") and the complex
    "components" layout, at every row length and every run length of _checkpoints; m = 257 is a full workgroup of the update
    and one lane of the next, m = 8193 thirty-three workgroups of the update and 129 of the read-out"""
    for K in KS_SWEEP:
        _sweep_case(m, C, K, mode)


@pytest.mark.parametrize("m", [16385, 65601])
def test_read_out_stats_over_many_workgroups(m):
    """the two-stage reduction of the read-out's stats beyond m = 8193 (129 workgroups of 64 lanes): m = 16385 is 257
    partials, a second trip of the second stage's loop; m = 65601 is one element beyond the 1024 workgroups of the cap, a
    second trip of the element loop.  Constant columns give a NaN count above zero; with and without the pooled outputs; the
    minimum is also that of the kernel's own ess array, exactly"""
    C, K, T = 2, 2, 5
    x = _columns(T, C, m, seed=m)
    t = _Acov(C, m, K)
    model = _Model(C, m, K)
    for i in range(T):
        t.update(x[i])
        model.push_all(x[i])
    for pooled in (True, False):
        _check_read_out(t, model, ("stats", m, pooled), pooled=pooled)
        ess, _, _, _, st = t.read(pooled)
        assert 0 < st[1] == np.isnan(ess).sum() < ess.size and st[0] == np.nanmin(ess), (m, pooled, st)


def test_update_entry_points_name_themselves_in_a_type_error():
    """a sample batch that is not contiguous or not 16-byte aligned, and a strided mask, are refused in the name of the entry
    point that was called"""
    import torch

    from pxmcmc_amd import ops
    from test_gpu_tails import _Tails

    C, m = 2, 6
    wide = torch.zeros((C, 2 * m + 2), dtype=torch.float64, device="cuda")
    strided = wide[:, : 2 * m : 2]
    off = wide.reshape(-1)[1 : 1 + C * m].view(C, m)
    good = torch.zeros((C, m), dtype=torch.float64, device="cuda")
    mask = torch.ones(2 * C, dtype=torch.int32, device="cuda")[::2]
    assert not strided.is_contiguous() and off.is_contiguous() and off.data_ptr() % 16 == 8 and not mask.is_contiguous()
    a = _Acov(C, m, 4)
    acov = lambda X, **kw: ops.acov_update(X, a.count[:C], a.acc[:C], a.tot[:C], a.head[:C], a.ring[:C], **kw)  # noqa: E731
    tl = _Tails(C, m, 0.5, 10)
    tails = lambda X, **kw: ops.tails_update(X, tl.count[:C], tl.lo[:C], tl.hi[:C], tl.thr_lo[:C], tl.thr_hi[:C], tl.stage[:C], tl.N, **kw)  # noqa: E731
    mom = lambda X, **kw: ops.moments_update(X, a.count[:C], good.clone(), good.clone(), **kw)  # noqa: E731
    for name, call in (("acov_update", acov), ("tails_update", tails), ("moments_update", mom)):
        for X in (strided, off):
            with pytest.raises(TypeError, match="^%s: X must be" % name):
                call(X)
        with pytest.raises(TypeError, match="^%s: mask must be" % name):
            call(good, mask=mask)
    assert a.count[:C].tolist() == [0, 0]


def test_read_out_leaves_the_run_as_it_was():
    """a run with a read-out after every save against the uninterrupted run: state and final read-out bit for bit"""
    import torch

    C, m, K, T = 2, 130, 8, 45
    x = _columns(T, C, m, seed=3)
    a, b = _Acov(C, m, K), _Acov(C, m, K)
    for i in range(T):
        a.update(x[i])
        b.update(x[i])
        b.read()
    for u, v in zip(a.state(), b.state()):
        assert torch.equal(u.view(torch.int64), v.view(torch.int64))
    for u, v in zip(a.read(), b.read()):
        assert_bit_equal(u, v)


def test_masks_and_per_chain_counts():
    """start counts 0, 1, 2 by masked rounds, then full rounds: every chain merges at its own phase and its ESS is that of
    its own samples; an all-off update changes nothing, bit for bit; the pooled read-out refuses the differing counts"""
    import torch

    from pxmcmc_amd._lib import PxmError

    C, m, K = 3, 131, 8
    start = [0, 1, 2]
    T = 3 * (K + B) + 5
    x = _columns(T, C, m, seed=9)
    t = _Acov(C, m, K)
    model = _Model(C, m, K)
    for i in range(T):
        on = [int(i < start[c]) for c in range(C)] if i < 2 else [1] * C
        t.update(x[i], mask=_dev(np.array(on, dtype=np.int32)) if i < 2 or i % 2 else None)
        for c in range(C):
            if on[c]:
                model.push(c, x[i, c])
        if i in (20, 33, 34, 35, T - 1):
            _check_read_out(t, model, ("masks", i), pooled=False)
    assert t.count[:C].tolist() == [T - 2, T - 1, T]
    before = [a.clone() for a in t.state()]
    t.update(x[0] - 50.0, mask=torch.zeros(C, dtype=torch.int32, device="cuda"))
    for a, b in zip(before, t.state()):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    t.assert_untouched_beyond_C("masks")
    with pytest.raises(PxmError, match="common sample count"):
        t.read(pooled=True)


def test_nan_and_inf_propagate_as_in_numpy():
    """a NaN, a +inf and a -inf in three columns at saves 0, 7 and 20: the accumulators carry what numpy's do from there on,
    those columns have no ESS, every other column is untouched by them"""
    C, m, K, T = 2, 66, 8, 50
    x = _columns(T, C, m, seed=5)
    x[0, 0, 0], x[7, 0, 1], x[20, 0, 2] = np.nan, np.inf, -np.inf
    x[7, 1, 3], x[0, 1, 4] = np.nan, np.inf
    t = _Acov(C, m, K)
    model = _Model(C, m, K)
    for i in range(T):
        t.update(x[i])
        model.push_all(x[i])
        if i + 1 in (8, 16, 21, 32, 50):
            _check_read_out(t, model, ("nan", i + 1))
    ess = t.read()[0]
    assert np.isnan(ess[0, :3]).all() and np.isnan(ess[1, 3:5]).all()


@pytest.mark.parametrize("cplx", [False, True])
def test_posterior_summary_ess(cplx):
    """the class on top: the lagged-product pass runs before the moments pass of the same update (which advances the counts),
    the moments and the tails are those of a summary without ess_lags, every read-out is in the real-component layout,
    to_host carries the per-chain values"""
    import torch

    from pxmcmc_amd.uncertainty import PosteriorSummary, ess_np, ess_pooled_np

    C, n, K, N = 3, 65, 8, 41
    mm = 2 * n if cplx else n
    x = _columns(N, C, mm, seed=6)
    lp = np.random.default_rng(6).normal(size=(N, C))
    s = PosteriorSummary(C, n, cplx, alpha=0.1, nsamples=N, ess_lags=K)
    plain = PosteriorSummary(C, n, cplx, alpha=0.1, nsamples=N)
    assert s.ess_bytes() == (3 * K + B) * 8 * C * mm and plain.ess_bytes() == 0
    for i in range(N):
        xt = _dev(x[i])
        xt = torch.view_as_complex(xt.reshape(C, n, 2)) if cplx else xt
        s.update(xt, logpi=_dev(lp[i]))
        plain.update(xt, logpi=_dev(lp[i]))
    host, host_plain = s.to_host(), plain.to_host()
    assert set(host) == set(host_plain) | set(PosteriorSummary.ESS_FIELDS) and host["ess_lags"] == K
    for k, v in host_plain.items():
        np.testing.assert_array_equal(host[k], v, err_msg=k)
    full = [acov_of(x[:, c], K) for c in range(C)]
    state = (np.array([f[0] for f in full]),) + tuple(np.stack([f[i] for f in full]) for i in range(1, 5))
    w_ess, w_lag = ess_np(*state)
    w_ep, w_se = ess_pooled_np(*state)
    assert s.ess().shape == s.ess_lag().shape == (C, mm) and s.ess_pooled().shape == s.mcse().shape == (mm,)
    _close(s.ess().cpu().numpy(), w_ess, "ess")
    np.testing.assert_array_equal(s.ess_lag().cpu().numpy(), w_lag)
    _close(s.ess_pooled().cpu().numpy(), w_ep, "pooled")
    _close(s.mcse().cpu().numpy(), w_se, "mcse")
    np.testing.assert_array_equal(host["ess"], s.ess().cpu().numpy())
    np.testing.assert_array_equal(host["ess_lag"], w_lag)
    ok = ~np.isnan(w_ess)
    lo, nnan, ntrunc = s.ess_stats()
    assert nnan == (~ok).sum() and ntrunc == (ok & (w_lag == K)).sum()
    np.testing.assert_allclose(lo, w_ess[ok].min(), rtol=RTOL)
    one = s.ess_readout()  # everything from one read-out
    assert set(one) == {"ess", "ess_lag", "ess_pooled", "mcse", "stats"} and set(s.ess_readout(False)) == {"ess", "ess_lag", "stats"}
    for k, t in (("ess", s.ess()), ("ess_lag", s.ess_lag()), ("ess_pooled", s.ess_pooled()), ("mcse", s.mcse())):
        np.testing.assert_array_equal(one[k].cpu().numpy(), t.cpu().numpy(), err_msg=k)
    line = s.ess_report("image")
    assert "ESS per chain over the image" in line and "max MCSE of the pooled mean" in line and "%.1f" % lo in line
    for call in (plain.ess, plain.ess_lag, plain.ess_pooled, plain.mcse, plain.ess_stats, plain.ess_readout, plain.ess_report):
        with pytest.raises(ValueError, match="without ess_lags"):
            call()


def test_update_with_lagged_products_is_capturable():
    """one captured update (lagged-product pass + moments passes) replayed N times with the sample rewritten in place: state
    bit-equal to eager updates"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.uncertainty import PosteriorSummary

    C, m, K, N = 3, 1025, 32, 70
    x = _columns(N, C, m, seed=8)
    lp = np.random.default_rng(8).normal(size=(N, C))

    def new():
        s = PosteriorSummary(C, m, False, ess_lags=K)
        for t in (s._acc, s._tot, s._head, s._ring):
            t.fill_(float("nan"))
        return s

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
    for a, b in zip((eager._acc, eager._tot, eager._head, eager._ring), (graph._acc, graph._tot, graph._head, graph._ring)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    for k, v in eager.to_host().items():
        np.testing.assert_array_equal(graph.to_host()[k], v, err_msg=k)


# ---- samplers ----------------------------------------------------------------------------------------------------------------
NS, ALPHA, KS = 41, 0.1, 8
RUNS = {}  # (algo, with summary_ess) -> (sampler, operator, params): each run is made once and shared by the tests below


def _run(algo, ess):
    """the runs of tests/test_gpu_tails.py, with the tails, with and without ``summary_ess`` (SKROCK at the step of the MYULA
    run, where its chains stay finite)"""
    from conftest import golden
    from pxmcmc_amd.mcmc import MYULA, SKROCK, PxMALA, PxMCMCParams

    if (algo, ess) in RUNS:
        return RUNS[algo, ess]
    C = 3
    kw = dict(nchains=C, seed=2, summary=("state", "image"), summary_alpha=ALPHA, summary_ess=KS if ess else None)
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
            p = PxMCMCParams(lmda=1e-3, delta=5e-4, ngap=1, s=3, nsamples=NS, nburn=3, verbosity=0, track=track)
            s = SKROCK(op, reg, p, **kw)
    _quiet(s.run, start_point=np.zeros(op.nparams))
    RUNS[algo, ess] = (s, op, p)
    return RUNS[algo, ess]


@pytest.mark.parametrize("algo", ["myula", "skrock", "pxmala"])
def test_sampler_ess_equals_that_of_the_saved_chain(algo):
    """summary[space].ess() per chain against ess_np of that chain's saved samples (the image space: mapped through
    chain_to_images, per real component); the run itself, its moments and its tails are those of the run without
    summary_ess, bit for bit"""
    from pxmcmc_amd._lib import PxmError
    from pxmcmc_amd.uncertainty import chain_to_images, ess_np, ess_pooled_np

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
        assert summ.ess_lags == KS and plain.summary[space].ess_lags is None
        host, host_plain = summ.to_host(), plain.summary[space].to_host()
        assert set(host) == set(host_plain) | {"ess_lags", "ess", "ess_lag"}
        for k, v in host_plain.items():
            np.testing.assert_array_equal(host[k], v, err_msg=f"{space} {k}")
        full = []
        for c in range(C):
            saved = s.chain[c][: counts[c]]
            if space == "image":
                saved = np.ascontiguousarray(chain_to_images(saved, op.transform))
                saved = saved.view(np.float64).reshape(saved.shape[0], -1)
            full.append(acov_of(np.asarray(saved, dtype=np.float64), KS))
        state = (np.array([f[0] for f in full]),) + tuple(np.stack([f[i] for f in full]) for i in range(1, 5))
        w_ess, w_lag = ess_np(*state)
        assert np.isfinite(w_ess).mean() > 0.9, (algo, space)
        np.testing.assert_array_equal(summ.ess_lag().cpu().numpy(), w_lag, err_msg=f"{algo} {space}")
        _close(summ.ess().cpu().numpy(), w_ess, (algo, space))
        if algo == "pxmala":
            with pytest.raises(PxmError, match="common sample count"):
                summ.ess_pooled()
            assert "different counts" in summ.ess_report(space)
        else:
            w_ep, w_se = ess_pooled_np(*state)
            _close(summ.ess_pooled().cpu().numpy(), w_ep, (algo, space))
            _close(summ.mcse().cpu().numpy(), w_se, (algo, space))


def test_save_and_load_round_trip_the_ess(tmp_path):
    from pxmcmc_amd.saving import load_mcmc, load_summaries, save_mcmc

    s, _, p = _run("myula", True)
    plain, _, p0 = _run("myula", False)
    data, attrs = load_mcmc(save_mcmc(s, p, str(tmp_path), filename="ess"))
    data0, attrs0 = load_mcmc(save_mcmc(plain, p0, str(tmp_path), filename="plain"))
    assert set(data) - set(data0) == {f"summary_{sp}_{f}" for sp in ("state", "image") for f in ("ess", "ess_lag")}
    assert attrs["summary_ess_lags"] == KS and "summary_ess_lags" not in attrs0
    for k, v in data0.items():
        np.testing.assert_array_equal(data[k], v, err_msg=k)
    back = load_summaries(data, attrs)
    for space in ("state", "image"):
        host = s.summary[space].to_host()
        assert set(back[space]) == set(host)
        for k, v in host.items():
            np.testing.assert_array_equal(back[space][k], v, err_msg=f"{space} {k}")
