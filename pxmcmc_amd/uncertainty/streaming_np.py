"""
The numpy statements of the streaming accumulators of :class:`~pxmcmc_amd.uncertainty.summary.PosteriorSummary` (DESIGN.md
section 15): what the device kernels compute, in their order of operations, for the tests and for the merge of several ranks.
:func:`moments_np`, :func:`pooled_np` and :func:`rhat_np` state the moments and R-hat; :func:`tail_capacity`,
:func:`tails_update_np` and :func:`tails_quantiles_np` the per-element tails behind the exact credible intervals;
:func:`acov_update_np`, :func:`ess_np` and :func:`ess_pooled_np` the lagged products and the effective sample size,
:func:`autocov_np` their definition.
"""
import numpy as np


# ---- streaming posterior moments, R-hat and best sample ------------------------------------------------
def _components(a):
    """real components of an array along its last axis: complex [..., n] -> float64 [..., 2 n] (re, im interleaved)"""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        a = np.ascontiguousarray(a, dtype=np.complex128)
        return a.view(np.float64).reshape(a.shape[:-1] + (2 * a.shape[-1],))
    return np.asarray(a, dtype=np.float64)


def moments_np(chain):
    """(count, mean, m2) of the samples of ONE chain, ``chain`` [nsamples, nparams]: the two-pass evaluation
    ``mean = sum x / n``, ``m2 = sum (x - mean)^2`` per parameter.  A complex chain is taken per real component
    ([nsamples, 2 nparams], re / im interleaved), as :class:`PosteriorSummary` accumulates it."""
    x = _components(chain)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError("moments_np: a [nsamples >= 1, nparams] array is expected")
    mean = x.sum(axis=0) / x.shape[0]
    return x.shape[0], mean, ((x - mean) ** 2).sum(axis=0)


def _taking_part(count, mean, m2):
    count = np.asarray(count, dtype=np.int64).reshape(-1)
    mean, m2 = np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64)
    if mean.ndim != 2 or mean.shape != m2.shape or mean.shape[0] != count.shape[0]:
        raise ValueError("count [C], mean [C, m] and m2 [C, m] are expected")
    on = count > 0
    return count[on], mean[on], m2[on]


def pooled_np(count, mean, m2):
    """(pooled mean, pooled unbiased variance) [m] over every sample of the chains with ``count > 0``, from the per-chain
    accumulators ``count`` [C], ``mean`` [C, m], ``m2`` [C, m]: Chan's pairwise merge, chain after chain in index order (the
    sequence of operations of ``k_moments_finalize``).  NaN where undefined (no sample; the variance of one sample)."""
    count, mean, m2 = _taking_part(count, mean, m2)
    m = mean.shape[1]
    na, ma, sa = 0.0, np.zeros(m), np.zeros(m)
    for nb, mb, sb in zip(count.astype(np.float64), mean, m2):
        n = na + nb
        d = mb - ma
        ma = ma + d * (nb / n)
        sa = (sa + sb) + (d * d) * (na * nb / n)
        na = n
    nan = np.full(m, np.nan)
    return (ma if na > 0 else nan), (sa / (na - 1.0) if na > 1 else nan)


def rhat_np(count, mean, m2):
    """Gelman-Rubin R-hat [m] of the chains with ``count > 0`` from their accumulators (``count`` [C], ``mean`` / ``m2`` [C, m]).
    With n the common count and C' the number of those chains::

        W = mean_c m2_c / (n - 1);  B = n / (C' - 1) sum_c (mean_c - mean of means)^2;  R = sqrt(((n - 1) / n W + B / n) / W)

    NaN where ``W == 0``, and everywhere when C' < 2 or n < 2.  Chains with different counts raise ``ValueError`` (PxMALA
    chains stopped by ``max_iter``): R-hat compares chains of one length.  The operations are those of ``k_moments_finalize``
    in its order."""
    count, mean, m2 = _taking_part(count, mean, m2)
    m = mean.shape[1]
    if count.size >= 2 and count.min() != count.max():
        raise ValueError("rhat_np: R-hat needs one common sample count, the chains hold between %d and %d samples"
                         % (count.min(), count.max()))
    if count.size < 2 or count[0] < 2:
        return np.full(m, np.nan)
    n, cp = float(count[0]), float(count.size)
    sm, sw = np.zeros(m), np.zeros(m)
    for mb, sb in zip(mean, m2):
        sm = sm + mb
        sw = sw + sb / (n - 1.0)
    mbar, W = sm / cp, sw / cp
    ssq = np.zeros(m)
    for mb in mean:
        d = mb - mbar
        ssq = ssq + d * d
    B = n / (cp - 1.0) * ssq
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(((n - 1.0) / n * W + B / n) / W)
    return np.where(W != 0.0, r, np.nan)


# ---- exact streaming credible intervals: per-element tails ---------------------------------------------
def _quantile_split(q, n):
    """numpy.quantile, method "linear", on n samples: (i, g), the lower order statistic and the interpolation weight -- the
    fp64 arithmetic of ``pxm_quantile_range``"""
    vi = float(q) * float(n - 1)
    fl = min(np.floor(vi), float(n - 1))
    return int(fl), vi - fl


def tail_capacity(alpha, nsamples):
    """k(alpha, N): slots per tail so that the k smallest and the k largest of n samples hold the two pairs of order
    statistics ``np.quantile(x, (alpha' / 2, 1 - alpha' / 2))`` interpolates between, for every n <= N = ``nsamples`` and
    every alpha' <= alpha: ``min(N, max(i_lo(N) + 2, N - i_hi(N)))``."""
    alpha, N = float(alpha), int(nsamples)
    if not (0.0 < alpha <= 1.0):
        raise ValueError("alpha must lie in (0, 1]")
    if N < 1:
        raise ValueError("nsamples must be at least 1")
    i_lo, _ = _quantile_split(alpha / 2, N)
    i_hi, _ = _quantile_split(1 - alpha / 2, N)
    return min(N, max(i_lo + 2, N - i_hi))


def _qkey(x):
    """the order-preserving uint64 key of ``qkey()`` (csrc/qkey.h): NaN, +-inf and +-0 in the order the device selects by"""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def tails_update_np(x, count, lo, hi, nsamples):
    """the numpy statement of one ``pxm_tails_update`` on ONE chain, in place: ``x`` [m] the sample, ``count`` the number of
    samples before it, ``lo`` / ``hi`` [k, m] the k smallest / largest so far (in no particular slot order; the device keeps
    heaps, and the last saves in a ring until it merges them: this states which samples the read-out sees, not where they lie).  ``count < k``: slot ``count`` of both; later a sample below the largest of ``lo`` (above the smallest of ``hi``)
    replaces it; ``count >= nsamples``: nothing.  ``count`` is the caller's to advance."""
    x = np.asarray(x, dtype=np.float64)
    k, m = lo.shape
    count = int(count)
    if count >= int(nsamples):
        return
    if count < k:
        lo[count] = x
        hi[count] = x
        return
    kx, cols = _qkey(x), np.arange(m)
    klo = _qkey(lo)
    s = klo.argmax(axis=0)
    ins = kx < klo[s, cols]
    lo[s[ins], cols[ins]] = x[ins]
    khi = _qkey(hi)
    s = khi.argmin(axis=0)
    ins = kx > khi[s, cols]
    hi[s[ins], cols[ins]] = x[ins]


def _np_lerp(a, b, t):
    """numpy/lib/_function_base_impl.py: _lerp, elementwise"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return np.where(t >= 0.5, b - d * (1.0 - t), a + d * t)


def tails_quantiles_np(count, lo, hi, alpha, nsamples=None):
    """the numpy statement of ``pxm_tails_quantiles``: ``count`` [C], ``lo`` / ``hi`` [C, k, m] -> (q_lo, q_hi) [C, m], the
    linear quantiles at ``alpha / 2`` and ``1 - alpha / 2`` of every chain's ``count[c]`` samples from its two tails (NaN for
    a chain without samples).  ``ValueError`` when an order statistic lies outside the tails, or a count exceeds
    ``nsamples`` (the number of saves the tails were sized for, when given)."""
    count = np.asarray(count, dtype=np.int64).reshape(-1)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if lo.ndim != 3 or lo.shape != hi.shape or lo.shape[0] != count.shape[0]:
        raise ValueError("count [C] and lo / hi [C, k, m] are expected")
    if not (0.0 <= alpha <= 1.0):
        raise ValueError("alpha must lie in [0, 1]")
    C, k, m = lo.shape
    q_lo, q_hi = np.full((C, m), np.nan), np.full((C, m), np.nan)
    for c, n in enumerate(int(v) for v in count):
        if nsamples is not None and n > int(nsamples):
            raise ValueError("chain %d holds %d samples, the tails were sized for %d" % (c, n, nsamples))
        if n == 0:
            continue
        ns = min(k, n)
        for q, tail, out, shift in ((alpha / 2, lo[c, :ns], q_lo, 0), (1 - alpha / 2, hi[c, :ns], q_hi, n - ns)):
            i, g = _quantile_split(q, n)
            top = min(i + 1, n - 1)
            if i - shift < 0 or top - shift >= ns:
                raise ValueError("alpha = %g at %d samples needs order statistics %d and %d, outside tails of %d slots" % (alpha, n, i, top, k))
            srt = np.take_along_axis(tail, np.argsort(_qkey(tail), axis=0, kind="stable"), axis=0)
            out[c] = _np_lerp(srt[i - shift], srt[top - shift], g)
    return q_lo, q_hi


# ---- streaming effective sample size: lagged products --------------------------------------------------
def ess_lag_count(K):
    """K as an int, validated: the number of lags kept for the effective sample size is even, with 2 <= K <= 64"""
    K = int(K)
    if K < 2 or K > 64 or K % 2:
        raise ValueError("ess_lags must be even with 2 <= K <= 64, got %d" % K)
    return K


def acov_update_np(x, count, acc, tot, head, last):
    """the numpy statement of one ``pxm_acov_update`` on ONE chain, in place, by the recurrence without staging: ``x`` [m] the
    sample, ``count`` = n the number of samples before it, ``acc`` [K, m] the lagged products ``acc_l = sum_{t >= l} y_t
    y_{t-l}`` of ``y_t = x_t - x_0``, ``tot`` [m] their sum, ``head`` [K, m] the first K samples, ``last`` [K, m] the latest
    ones (sample t in row ``t % K``).  Every product and every sum is rounded on its own, in save order; the first sample
    zeroes ``acc`` and ``tot``, so the state needs no initialisation.  (The device adds the same terms in the same order, a
    block of saves at a time: its ``acc`` and ``tot`` equal these after every complete block.)  ``count`` is the caller's to
    advance."""
    x = np.asarray(x, dtype=np.float64)
    K, n = acc.shape[0], int(count)
    if n == 0:
        acc[:] = 0.0
        tot[:] = 0.0
    if n < K:
        head[n] = x
    last[n % K] = x
    p = head[0]
    with np.errstate(invalid="ignore", over="ignore"):
        y = x - p
        tot[:] = tot + y
        for l in range(min(n, K - 1) + 1):
            acc[l] = acc[l] + y * (last[(n - l) % K] - p)


def _geyer_np(rho, N):
    """Geyer's initial monotone sequence over ``P_k = rho[2 k] + rho[2 k + 1]``, elementwise over the columns of ``rho``
    [lmax, m] -> (ess [m], ess_lag [m]): stop at the first P_k that is not positive (a NaN included), otherwise ``P_k <-
    min(P_k, P_{k-1})``; ``tau = -1 + 2 sum P_k``; ``ess = min(N / tau, N log10 N)``, the cap where ``tau <= 0``;
    ``ess_lag`` the even lag of the stop, ``2 * (lmax // 2)`` where the sequence never stopped"""
    lmax, m = rho.shape
    total, prev = np.zeros(m), np.full(m, np.inf)
    lag = np.full(m, -1, dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(lmax // 2):
            P = rho[2 * k] + rho[2 * k + 1]
            going = lag < 0
            lag[going & ~(P > 0.0)] = 2 * k
            add = lag < 0
            prev = np.where(add, np.minimum(P, prev), prev)
            total = np.where(add, total + prev, total)
        lag[lag < 0] = 2 * (lmax // 2)
        tau, cap = -1.0 + 2.0 * total, N * np.log10(N)
        return np.where(tau > 0.0, np.minimum(N / tau, cap), cap), lag


def acov_gamma_np(count, acc, tot, head, last):
    """the biased autocovariances about the chain's own mean of ONE chain from its accumulators -> (gamma [min(K, n), m],
    mean [m]): with ``d = tot / n``, ``head_l`` (``tail_l``) the sum of the first (last) l of the ``y_t``::

        gamma_l = (acc_l - d ((tot - head_l) + (tot - tail_l)) + (n - l) d^2) / n,    mean = x_0 + d

    in the order of operations of ``k_acov_ess``"""
    n, K = int(count), acc.shape[0]
    lmax, p = min(K, n), head[0]
    nd = float(n)
    g = np.empty((lmax, acc.shape[1]))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = tot / nd
        dd = d * d
        hc, tc = np.zeros_like(d), np.zeros_like(d)
        for l in range(lmax):
            g[l] = ((acc[l] - d * ((tot - hc) + (tot - tc))) + float(n - l) * dd) / nd
            hc = hc + (head[l] - p)
            tc = tc + (last[(n - 1 - l) % K] - p)
        return g, p + d


def ess_np(count, acc, tot, head, last):
    """the numpy statement of the per-chain part of ``pxm_acov_ess``: ``count`` [C], ``acc`` / ``head`` / ``last`` [C, K, m]
    and ``tot`` [C, m] as :func:`acov_update_np` leaves them -> (ess float64 [C, m], ess_lag int32 [C, m]).  NaN and -1 for a
    chain with fewer than 4 samples and where ``gamma_0`` is not positive and finite."""
    count = np.asarray(count, dtype=np.int64).reshape(-1)
    C, K, m = np.shape(acc)
    ess, lag = np.full((C, m), np.nan), np.full((C, m), -1, dtype=np.int32)
    for c, n in enumerate(int(v) for v in count):
        if n < 4:
            continue
        g, _ = acov_gamma_np(n, acc[c], tot[c], head[c], last[c])
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = (g[0] > 0.0) & (g[0] < np.inf)
            e, la = _geyer_np(g / g[0], float(n))
        ess[c], lag[c] = np.where(ok, e, np.nan), np.where(ok, la, -1)
    return ess, lag


def ess_pooled_np(count, acc, tot, head, last):
    """the numpy statement of the pooled part of ``pxm_acov_ess`` -> (ess_pooled [m], mcse [m]) over the C' chains with
    ``count > 0``, which must share one count n (``ValueError`` otherwise), after Vehtari et al. 2021 without rank
    normalisation::

        W = mean_c n / (n - 1) gamma_0,c;   var+ = (n - 1) / n W + sum_c (mean_c - mean of means)^2 / (C' - 1)
        rho_l = 1 - (W - mean_c n / (n - 1) gamma_l,c) / var+;   ess_pooled = min(C' n / tau, C' n log10(C' n))

    with Geyer's sum for tau, and ``mcse = sqrt(var+ / ess_pooled)``, the standard error of the pooled mean.  NaN for n < 4,
    where a chain has no positive finite ``gamma_0`` and where ``var+`` is not positive and finite."""
    count = np.asarray(count, dtype=np.int64).reshape(-1)
    C, K, m = np.shape(acc)
    on = np.flatnonzero(count > 0)
    nan = np.full(m, np.nan)
    if on.size >= 2 and count[on].min() != count[on].max():
        raise ValueError("ess_pooled_np: the pooled ESS needs one common sample count, the chains hold between %d and %d samples"
                         % (count[on].min(), count[on].max()))
    if on.size == 0 or count[on[0]] < 4:
        return nan, nan.copy()
    n = int(count[on[0]])
    nd, cp, lmax = float(n), float(on.size), min(K, n)
    f = nd / (nd - 1.0)
    G, sm, means, bad = np.zeros((lmax, m)), np.zeros(m), [], np.zeros(m, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in on:
            g, mean = acov_gamma_np(n, acc[c], tot[c], head[c], last[c])
            bad |= ~((g[0] > 0.0) & (g[0] < np.inf))
            G = G + f * g
            sm = sm + mean
            means.append(mean)
        mbar, W = sm / cp, G[0] / cp
        ssq = np.zeros(m)
        for mean in means:
            dm = mean - mbar
            ssq = ssq + dm * dm
        varp = (nd - 1.0) / nd * W
        if on.size > 1:
            varp = varp + ssq / (cp - 1.0)
        ok = ~bad & (varp > 0.0) & (varp < np.inf)
        e, _ = _geyer_np(1.0 - (W - G / cp) / varp, cp * nd)
        e = np.where(ok, e, np.nan)
        return e, np.sqrt(varp / e)


def autocov_np(chain, K):
    """the biased autocovariances of ONE chain [n, m] at lags 0 ... min(K, n) - 1 by their definition, in long double on the
    pivot-shifted samples: ``gamma_l = sum_{t >= l} (y_t - ybar) (y_{t-l} - ybar) / n`` with ``y_t = x_t - x_0`` -> long double
    [min(K, n), m].  The error model of the accumulators is measured against this."""
    x = _components(chain)
    n = x.shape[0]
    y = x.astype(np.longdouble) - x[0].astype(np.longdouble)
    z = y - y.sum(axis=0) / np.longdouble(n)
    return np.stack([(z[l:] * z[:n - l]).sum(axis=0) / np.longdouble(n) for l in range(min(int(K), n))])
