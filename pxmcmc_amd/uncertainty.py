"""
Uncertainty summaries of saved chains (pxmcmc/uncertainty.py:7-56): quantile credible-interval ranges per
parameter and per wavelet scale, and the highest-posterior-density threshold.  Post-run host arithmetic,
as in the reference; ``chain_to_images`` is the batched GPU synthesis the reference's plot scripts do sample
by sample (experiments/earthtopography/plot.py:105-115).

Streaming summaries: :class:`PosteriorSummary` accumulates per-chain moments and the
highest-posterior sample on the device while a sampler runs (``summary=`` of the samplers), so the posterior mean, the
standard-deviation map, the "MAP_X" sample (plot.py:75-76, 122) and R-hat across the chain batch need no saved chain;
:func:`moments_np`, :func:`pooled_np` and :func:`rhat_np` state the same quantities in numpy.  With ``alpha=`` it also keeps
the k smallest and k largest samples of every element (:func:`tail_capacity`), from which ``credible_interval_range()``
gives the numbers of :func:`credible_interval_range` on each chain's saved samples, exactly; :func:`tails_update_np` and
:func:`tails_quantiles_np` state that in numpy.  With ``ess_lags=`` it accumulates the lagged products of the saved samples,
from which ``ess()``, ``ess_pooled()`` and ``mcse()`` give the effective sample size and the standard error of the pooled
mean; :func:`acov_update_np`, :func:`ess_np` and :func:`ess_pooled_np` state that in numpy, :func:`autocov_np` the definition.

Local credible intervals: :func:`local_credible_intervals` turns the MAP point and the level of
:func:`approx_credible_region_threshold` into an error bar per region of the image (:func:`superpixel_regions`), searched on
the device; :func:`lci_terms_np`, :func:`lci_eval_np` and :func:`lci_search_np` state its sums and its search in numpy.

Hypothesis tests of image structure: :func:`hypothesis_test` forms a surrogate image without the
structure of each region (:func:`inpaint_regions`, :func:`smooth_regions`) and follows the objective from the MAP point to it;
:func:`inpaint_step_np` and :func:`inpaint_np` state the inpainting kernel and its iteration in numpy.
"""
import warnings

import numpy as np
import torch

from . import ops
from ._lib import LCI_EMPTY, LCI_NONFINITE, LCI_POINTS, LCI_UNCONSTRAINED
from .utils import _multires_bandlimits, mw_size


def credible_interval_range(chain, alpha=0.05):
    """range of the (1 - alpha) credible interval of every parameter (pxmcmc/uncertainty.py:7-16).  A chain that is already
    resident on the device (a CUDA tensor, float64 [nsamples, nparams]) is reduced there (`pxm_quantile_range`: exact order
    statistics + numpy's interpolation, the same numbers) and a device tensor comes back; numpy in, numpy out on the host as
    in the reference."""
    if isinstance(chain, torch.Tensor) and chain.is_cuda:
        return ops.quantile_range(chain, alpha)
    quantiles = np.quantile(chain, (alpha / 2, 1 - alpha / 2), axis=0)
    return np.diff(quantiles, axis=0)[0]


def wavelet_credible_interval_range(chain, L, B, J_min, alpha=0.05, dirs=1):
    """credible-interval maps per wavelet scale, MW (theta, phi) format (pxmcmc/uncertainty.py:19-40): the quantile
    range of every coefficient at once, cut at the block boundaries of the coefficient vector.  ``dirs = N > 1``
    (extension): wavelet block j comes back as (2N - 1, bl_j, 2 bl_j - 1), one map per orientation."""
    bls = [int(bl) for bl in _multires_bandlimits(L, B, J_min)]
    planes = [1] + [2 * int(dirs) - 1] * (len(bls) - 1)
    edges = np.cumsum([k * mw_size(bl) for bl, k in zip(bls, planes)])
    on_device = isinstance(chain, torch.Tensor) and chain.is_cuda
    chain = chain if on_device else np.asarray(chain)
    if chain.shape[1] != edges[-1]:
        raise ValueError("chain has %d parameters, the wavelet layout %d" % (chain.shape[1], edges[-1]))
    ci = credible_interval_range(chain, alpha)
    blocks = np.split(ci.cpu().numpy() if on_device else ci, edges[:-1])
    if dirs == 1:
        return [blk.reshape(bl, 2 * bl - 1) for blk, bl in zip(blocks, bls)]
    return [blk.reshape(bl, 2 * bl - 1) if k == 1 else blk.reshape(k, bl, 2 * bl - 1) for blk, bl, k in zip(blocks, bls, planes)]


def credible_region_threshold(logpis, alpha=0.05):
    """log-posterior threshold of the credible set (pxmcmc/uncertainty.py:43-51)"""
    return np.quantile(logpis, 1 - alpha)


def approx_credible_region_threshold(objective_map, ndim, alpha=0.05):
    """Approximate threshold of the (1 - alpha) highest-posterior-density region of a log-concave posterior from its MAP
    point alone, without a chain (Pereyra, "Maximum-a-posteriori estimation with Bayesian confidence regions", SIAM J.
    Imaging Sci. 10(1), 2017, theorem 3.1): the region ``{x : F(x) <= F(x_map) + ndim (tau_alpha + 1)}`` with
    ``tau_alpha = sqrt(16 log(3 / alpha) / ndim)`` contains the HPD region, for ``alpha`` in ``(4 exp(-ndim / 3), 1)``.

    :param objective_map: the objective ``F = -log posterior`` at the MAP point (:attr:`pxmcmc_amd.optim.FISTA.objective_map`)
    :param ndim: number of REAL dimensions of the state (``2 n`` for a complex state of n coefficients)
    :raises ValueError: ``alpha`` outside the range of the bound
    """
    ndim = int(ndim)
    if ndim < 1:
        raise ValueError("ndim must be a positive number of real dimensions")
    if not (4 * np.exp(-ndim / 3) < alpha < 1):
        raise ValueError("alpha = %g is outside (4 exp(-ndim / 3), 1) = (%g, 1), the range of the bound" % (alpha, 4 * np.exp(-ndim / 3)))
    tau = np.sqrt(16 * np.log(3 / alpha) / ndim)
    return objective_map + ndim * (tau + 1)


def in_credible_region(logpi, threshold):
    """pxmcmc/uncertainty.py:54-56"""
    return True if logpi <= threshold else False


def chain_to_images(chain, transform, batch=16):
    """map every saved sample through ``transform.inverse`` in chain batches on the GPU -> [nsamples, npix]"""
    chain = np.asarray(chain)
    transform.ensure_chains(batch)
    out = []
    for i in range(0, chain.shape[0], batch):
        out.append(np.asarray(transform.inverse(chain[i : i + batch].astype(complex))))
    return np.concatenate(out, axis=0)


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
def _ess_lags(K):
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


class PosteriorSummary:
    """Device accumulators of a chain batch: per chain the sample count, the running mean and the sum of squared deviations
    of every parameter (Welford's recurrence, ``pxm_moments_update``), and the sample of highest log posterior seen so far.
    What the reference's plot scripts compute from a saved chain -- ``np.mean(chain_pix, axis=0)``, the standard-deviation
    map, ``MAP_X = chain[argmax(logposterior)]`` (experiments/earthtopography/plot.py:75-76, 122) -- without the chain.

    :param nchains: C, chains of the batch
    :param nparams: parameters per chain
    :param complex_: the samples are complex: real and imaginary parts get their own moments (``m = 2 nparams`` real
        components, re / im interleaved).  ``False``: the real parts of the samples are accumulated (``m = nparams``), as the
        samplers' real ``chain`` array keeps them.
    :param best: track the highest-posterior sample (``update`` then needs ``logpi``)
    :param alpha: also keep, per chain and real component, the ``k = tail_capacity(alpha, nsamples)`` smallest and largest
        samples (``pxm_tails_update``), from which :meth:`credible_interval` reads the (1 - alpha') interval of every
        alpha' <= alpha exactly.  ``None``: no tails
    :param nsamples: the number of ``update`` calls the run will make per chain (needed with ``alpha``); a chain updated more
        often keeps its first ``nsamples`` samples in the tails and :meth:`credible_interval` then raises
    :param ess_lags: K, even with 2 <= K <= 64: also accumulate, per chain and real component, the lagged products of the
        samples at lags below K (``pxm_acov_update``), from which :meth:`ess`, :meth:`ess_pooled` and :meth:`mcse` are read.
        ``None``: none

    Intervals are per chain.  A pooled interval over the chain batch is deliberately not offered: exact pooling needs k
    proportional to the pooled sample count, which costs as much as the chain.

    Complex states come back complex: ``mean`` as ``re + i im``, ``variance`` as ``var_re + var_im`` (``E |x - mean|^2``),
    ``best_sample`` as stored.  ``rhat()`` is per REAL component, shape ``[m]`` (``[2 nparams]`` for a complex state: a
    chain batch can have converged in one component and not in the other).  ``to_host()`` / ``merge`` carry the raw
    accumulators in the real-component layout ``[C, m]``, which :func:`pooled_np` and :func:`rhat_np` take.
    """

    FIELDS = ("count", "mean", "m2", "best", "best_logpi")
    TAIL_FIELDS = ("alpha", "q_lo", "q_hi")  # ``to_host()`` of a summary built with ``alpha``
    ESS_FIELDS = ("ess_lags", "ess", "ess_lag")  # ... of a summary built with ``ess_lags``

    def __init__(self, nchains, nparams, complex_, best=True, device=None, alpha=None, nsamples=None, ess_lags=None):
        self.nchains, self.nparams, self.complex = int(nchains), int(nparams), bool(complex_)
        if self.nchains < 1 or self.nparams < 1:
            raise ValueError("PosteriorSummary needs nchains >= 1 and nparams >= 1")
        self.m = self.nparams * (2 if self.complex else 1)
        self.alpha = self.tail_slots = self._lo = self._hi = self._thr_lo = self._thr_hi = self._stage = None
        self.nsamples = None if nsamples is None else int(nsamples)
        if alpha is not None:
            if nsamples is None:
                raise ValueError("PosteriorSummary: alpha needs nsamples, the number of updates the tails are sized for")
            self.tail_slots = tail_capacity(alpha, nsamples)
            self.alpha = float(alpha)
        self.ess_lags = None if ess_lags is None else _ess_lags(ess_lags)
        self._acc = self._tot = self._head = self._ring = None
        dev = ops.device() if device is None else device
        C, m = self.nchains, self.m
        self._count = torch.zeros(C, dtype=torch.int64, device=dev)
        self._mean = torch.zeros((C, m), dtype=torch.float64, device=dev)
        self._m2 = torch.zeros((C, m), dtype=torch.float64, device=dev)
        self.best = bool(best)
        self._best_x = torch.zeros((C, m), dtype=torch.float64, device=dev) if self.best else None
        self._best_logpi = torch.full((C,), -np.inf, dtype=torch.float64, device=dev) if self.best else None
        if self.alpha is not None:
            self._lo = torch.zeros((C, self.tail_slots, m), dtype=torch.float64, device=dev)
            self._hi = torch.zeros_like(self._lo)
            self._stage = torch.zeros((C, ops.tails_stage_depth(), m), dtype=torch.float64, device=dev)
            self._thr_lo = torch.zeros((C, m), dtype=torch.float64, device=dev)
            self._thr_hi = torch.zeros_like(self._thr_lo)
        if self.ess_lags is not None:  # (pxm_acov_update needs no initialisation)
            K = self.ess_lags
            self._acc = torch.empty((C, K, m), dtype=torch.float64, device=dev)
            self._head = torch.empty_like(self._acc)
            self._tot = torch.empty((C, m), dtype=torch.float64, device=dev)
            self._ring = torch.empty((C, K - 1 + ops.acov_stage_depth(), m), dtype=torch.float64, device=dev)

    # ---- accumulation -----------------------------------------------------------------------------------------------
    def update(self, X, logpi=None, mask=None):
        """add one sample per chain: ``X`` [C, nparams] on the device (complex128, or float64 when ``complex_`` is False),
        ``logpi`` [C] its log posterior (float64 or complex128: the real part; needed with ``best``), ``mask`` an int32 [C]
        device tensor or a sequence of chain flags -- chains with a zero keep their accumulators untouched.  One fused pass
        and one small launch on the current stream, behind the lagged-product pass of a summary built with ``ess_lags`` and the
        tails pass of one built with ``alpha``.  With contiguous device tensors for ``X``, ``logpi`` and ``mask`` nothing is
        allocated or copied (the form a captured graph takes); a host ``mask`` or ``logpi`` is uploaded first (a small
        synchronous copy), and a non-contiguous ``X`` is copied."""
        X = ops.as_device(X) if not (isinstance(X, torch.Tensor) and X.is_cuda) else X
        if X.dim() == 1:
            X = X[None]
        if tuple(X.shape) != (self.nchains, self.nparams):
            raise ValueError("update: expected a [%d, %d] sample batch, got %s" % (self.nchains, self.nparams, tuple(X.shape)))
        if not X.is_contiguous() or X.data_ptr() % 16:
            X = X.clone(memory_format=torch.contiguous_format)
        if self.complex:
            if not X.is_complex():
                X = X.to(torch.complex128)
            X = torch.view_as_real(X).reshape(self.nchains, self.m)  # (a view: real components, re / im interleaved)
        if self.best:
            if logpi is None:
                raise ValueError("update: a summary with best=True needs logpi")
            logpi = ops.as_device(logpi) if not (isinstance(logpi, torch.Tensor) and logpi.is_cuda) else logpi.contiguous()
        else:
            logpi = None
        if mask is not None and not (isinstance(mask, torch.Tensor) and mask.is_cuda):
            mask = torch.as_tensor(np.asarray(mask) != 0, dtype=torch.int32).to(self._mean.device)
        if self.ess_lags is not None:  # reads the counts the moments pass is about to advance
            ops.acov_update(X, self._count, self._acc, self._tot, self._head, self._ring, mask=mask)
        if self.alpha is not None:  # (so does this)
            ops.tails_update(X, self._count, self._lo, self._hi, self._thr_lo, self._thr_hi, self._stage, self.nsamples, mask=mask)
        ops.moments_update(X, self._count, self._mean, self._m2, mask=mask, logpi=logpi, best_logpi=self._best_logpi,
                           best_x=self._best_x)

    # ---- read-out ---------------------------------------------------------------------------------------------------
    def _cplx(self, t):
        """[.., m] real components -> [.., nparams] complex128 for a complex state (a view)"""
        return torch.view_as_complex(t.reshape(t.shape[:-1] + (self.nparams, 2))) if self.complex else t

    def _sum_components(self, t):
        return t.reshape(t.shape[:-1] + (self.nparams, 2)).sum(-1) if self.complex else t

    @property
    def counts(self):
        """samples accumulated per chain, int64 [C] (device)"""
        return self._count

    def mean(self):
        """per-chain posterior mean [C, nparams] (device; zero for a chain without a sample)"""
        return self._cplx(self._mean)

    def variance(self):
        """per-chain unbiased variance [C, nparams] (device; NaN for a chain with fewer than two samples)"""
        n = self._count.to(torch.float64)[:, None]
        var = torch.where(n > 1, self._m2 / (n - 1), torch.full_like(self._m2, float("nan")))
        return self._sum_components(var)

    def std(self):
        return torch.sqrt(self.variance())

    def pooled_mean(self):
        """mean over every sample of every chain [nparams] (device)"""
        return self._cplx(ops.moments_finalize(self._count, self._mean, self._m2, rhat=False)[0])

    def pooled_variance(self):
        """unbiased variance over every sample of every chain [nparams] (device)"""
        return self._sum_components(ops.moments_finalize(self._count, self._mean, self._m2, rhat=False)[1])

    def rhat(self):
        """Gelman-Rubin R-hat per real component, [m] (device); raises PxmError when the chains' counts differ"""
        return ops.moments_finalize(self._count, self._mean, self._m2)[2]

    def max_rhat(self):
        """(largest R-hat over the components where it is defined, number of components where it is not)"""
        st = ops.moments_finalize(self._count, self._mean, self._m2)[3].cpu().numpy()
        return float(st[0]), int(st[1])

    def best_sample(self):
        """the sample of highest log posterior of every chain [C, nparams] (device)"""
        if not self.best:
            raise ValueError("this summary was built with best=False")
        return self._cplx(self._best_x)

    @property
    def best_logpi(self):
        """log posterior of ``best_sample()`` per chain, float64 [C] (device; -inf before the first sample)"""
        if not self.best:
            raise ValueError("this summary was built with best=False")
        return self._best_logpi

    # ---- credible intervals from the tails ----------------------------------------------------------------------------
    def _tail_quantiles(self, alpha):
        if self.alpha is None:
            raise ValueError("this summary was built without alpha: it keeps no tails")
        alpha = self.alpha if alpha is None else float(alpha)
        if not (0.0 < alpha <= self.alpha):
            raise ValueError("alpha = %g: the tails were sized for alpha = %g and give any alpha in (0, %g]" % (alpha, self.alpha, self.alpha))
        return ops.tails_quantiles(self._count, self._lo, self._hi, self._stage, self.nsamples, alpha)

    def credible_interval(self, alpha=None):
        """(q_lo, q_hi) [C, nparams] (device): per chain, ``np.quantile(samples, (alpha / 2, 1 - alpha / 2), axis=0)`` of the
        samples accumulated so far, bit for bit; NaN for a chain without samples.  Per real component: for a complex state
        the real (imaginary) parts of the complex results are the quantiles of the real (imaginary) parts.  ``alpha``
        defaults to the constructed one and may be any smaller value; a larger one raises ``ValueError``, a chain updated
        more than ``nsamples`` times ``PxmError``.  Per chain only: there is no pooled interval over the batch."""
        q_lo, q_hi = self._tail_quantiles(alpha)
        return self._cplx(q_lo), self._cplx(q_hi)

    def credible_interval_range(self, alpha=None):
        """``q_hi - q_lo`` of :meth:`credible_interval`, [C, nparams] (device): per chain the numbers
        :func:`credible_interval_range` gives on that chain's saved samples"""
        q_lo, q_hi = self._tail_quantiles(alpha)
        return self._cplx(q_hi - q_lo)

    def tail_bytes(self):
        """device bytes of the tail heaps, their thresholds and the ring of staged saves: ``(2 k + 2 + B) * 8 * C * m`` with
        ``B = ops.tails_stage_depth()`` (0 without ``alpha``)"""
        return 0 if self.alpha is None else (2 * self.tail_slots + 2 + ops.tails_stage_depth()) * 8 * self.nchains * self.m

    # ---- effective sample size from the lagged products ------------------------------------------------------------------
    def _ess(self, pooled):
        if self.ess_lags is None:
            raise ValueError("this summary was built without ess_lags: it keeps no lagged products")
        return ops.acov_ess(self._count, self._acc, self._tot, self._head, self._ring, pooled=pooled)

    def ess_readout(self, pooled=True):
        """ONE read-out of the lagged products -> dict of device tensors ``ess`` [C, m], ``ess_lag`` int32 [C, m],
        ``ess_pooled`` [m], ``mcse`` [m] and ``stats`` [3] (min ESS over the defined values, undefined count, truncated
        count), all in the real-component layout.  ``pooled=False`` leaves ``ess_pooled`` and ``mcse`` out and takes chains
        of any counts; with them, differing counts raise PxmError.  :meth:`ess`, :meth:`ess_lag`, :meth:`ess_pooled`,
        :meth:`mcse` and :meth:`ess_stats` each make such a read-out of their own: take several results from this call."""
        ess, lag, ep, se, st = self._ess(pooled)
        out = {"ess": ess, "ess_lag": lag, "stats": st}
        if pooled:
            out.update(ess_pooled=ep, mcse=se)
        return out

    def ess_report(self, what="state"):
        """one line for a log, from one read-out: smallest and median per-chain ESS over ``what``, the fraction of truncated
        values and the largest Monte-Carlo standard error of the pooled mean (left out, with the reason, when the chains hold
        different counts)"""
        try:
            r, why = self.ess_readout(True), ""
        except ops.PxmError:
            r, why = self.ess_readout(False), "; no pooled MCSE: the chains stopped at different counts"
        lo, nundef, ntrunc = (float(v) for v in r["stats"].cpu().numpy())
        defined = r["ess"].numel() - int(nundef)
        if not defined:
            return f"ESS of the {what}: undefined everywhere (fewer than 4 samples per chain, or nothing moved)"
        line = (f"ESS per chain over the {what} (lags below {self.ess_lags}): min {lo:.1f}, "
                f"median {float(r['ess'][~r['ess'].isnan()].median()):.1f}; {ntrunc / defined:.1%} truncated "
                f"(upper bounds: use more lags or a larger ngap)")
        if "mcse" in r:
            se = r["mcse"][~r["mcse"].isnan()]
            why = f"; max MCSE of the pooled mean {float(se.max()):.3e}" if se.numel() else "; MCSE undefined"
        return line + why

    def ess(self):
        """effective sample size per chain and real component, [C, m] (device): Geyer's initial monotone sequence over the
        autocorrelations at lags below ``ess_lags``; NaN for a chain with fewer than 4 samples and for a component that
        never moved.  Where :meth:`ess_lag` equals ``2 * (min(ess_lags, n) // 2)`` the sequence did not end within the lags
        kept and the value is an upper bound: use more lags, or a larger ``ngap``."""
        return self._ess(False)[0]

    def ess_lag(self):
        """the even lag at which the sequence of :meth:`ess` stopped, int32 [C, m] (device; -1 where ess is NaN)"""
        return self._ess(False)[1]

    def ess_pooled(self):
        """effective sample size of the whole chain batch per real component, [m] (device), after Vehtari et al. 2021 without
        rank normalisation; raises PxmError when the chains' counts differ.  Over several ranks no pooled value is offered:
        sum the per-chain values where R-hat is close to 1."""
        return self._ess(True)[2]

    def mcse(self):
        """Monte-Carlo standard error of :meth:`pooled_mean` per real component, [m] (device): ``sqrt(var+ / ess_pooled)``"""
        return self._ess(True)[3]

    def ess_stats(self):
        """(smallest per-chain ESS over the values that are defined, number that are not, number that are truncated)"""
        st = self._ess(False)[4].cpu().numpy()
        return float(st[0]), int(st[1]), int(st[2])

    def ess_bytes(self):
        """device bytes of the lagged products, the first saves and the ring: ``(3 K + B) * 8 * C * m`` with
        ``B = ops.acov_stage_depth()`` (0 without ``ess_lags``)"""
        return 0 if self.ess_lags is None else (3 * self.ess_lags + ops.acov_stage_depth()) * 8 * self.nchains * self.m

    # ---- host side --------------------------------------------------------------------------------------------------
    def to_host(self):
        """plain dict of numpy arrays: ``count`` int64 [C], ``mean`` / ``m2`` float64 [C, m] in the real-component layout
        and, with ``best``, ``best`` [C, nparams] (complex for a complex state) and ``best_logpi`` [C]; a summary built with
        ``alpha`` adds ``alpha`` (float64 scalar) and its quantiles ``q_lo`` / ``q_hi`` [C, m] in the real-component layout,
        one built with ``ess_lags`` adds ``ess_lags`` (int64 scalar), ``ess`` float64 [C, m] and ``ess_lag`` int32 [C, m].
        Where the tails cannot be read out (a chain updated more than ``nsamples`` times: ``PxmError`` from
        :meth:`credible_interval`) these three are left out with a ``RuntimeWarning``, so that the moments and the best
        sample of the run can still be saved."""
        out = {"count": self._count.cpu().numpy(), "mean": self._mean.cpu().numpy(), "m2": self._m2.cpu().numpy()}
        if self.best:
            out["best"] = self.best_sample().cpu().numpy()
            out["best_logpi"] = self._best_logpi.cpu().numpy()
        if self.alpha is not None:
            try:
                q_lo, q_hi = self._tail_quantiles(None)
            except ops.PxmError as e:
                warnings.warn("PosteriorSummary.to_host: no credible intervals (%s)" % e, RuntimeWarning, stacklevel=2)
            else:
                out.update(alpha=np.float64(self.alpha), q_lo=q_lo.cpu().numpy(), q_hi=q_hi.cpu().numpy())
        if self.ess_lags is not None:
            ess, lag = self._ess(False)[:2]
            out.update(ess_lags=np.int64(self.ess_lags), ess=ess.cpu().numpy(), ess_lag=lag.cpu().numpy())
        return out

    @staticmethod
    def merge(dicts):
        """concatenate the chains of several ``to_host()`` dicts (one per rank, in rank order) -> one such dict;
        ``rhat_np(d["count"], d["mean"], d["m2"])`` of the result is R-hat over all the chains of a multi-rank run.  When
        every dict carries the ``TAIL_FIELDS``, with one common ``alpha``, so does the result: the intervals stay per chain
        (exact pooling over chains would need tails as long as the pooled chain).  Likewise the ``ESS_FIELDS`` when every
        dict carries them with one ``ess_lags``: per-chain values; a pooled ESS over ranks is not offered -- sum the per-chain
        values where R-hat is close to 1"""
        dicts = list(dicts)
        if not dicts:
            raise ValueError("merge: no summaries")
        keys = [k for k in PosteriorSummary.FIELDS if all(k in d for d in dicts)]
        out = {k: np.concatenate([np.asarray(d[k]) for d in dicts], axis=0) for k in keys}
        if all(k in d for d in dicts for k in PosteriorSummary.TAIL_FIELDS):
            alphas = {float(d["alpha"]) for d in dicts}
            if len(alphas) != 1:
                raise ValueError("merge: the summaries were built with different alpha: %s" % sorted(alphas))
            out["alpha"] = np.float64(alphas.pop())
            out.update({k: np.concatenate([np.asarray(d[k]) for d in dicts], axis=0) for k in ("q_lo", "q_hi")})
        if all(k in d for d in dicts for k in PosteriorSummary.ESS_FIELDS) and len({int(d["ess_lags"]) for d in dicts}) == 1:
            out["ess_lags"] = np.int64(dicts[0]["ess_lags"])
            out.update({k: np.concatenate([np.asarray(d[k]) for d in dicts], axis=0) for k in ("ess", "ess_lag")})
        return out


# ---- local credible intervals from the MAP point ------------------------------------------------------
LCI_OK = 0  # status of a region: 0, or the LCI_* bits (these and LCI_POINTS, the values of xi per pass: the header's, from _lib)


def lci_shrink_factor(rounds, q2_positive=True):
    """the guaranteed bound on (width of a final bracket) / (width of the outer bracket) after ``rounds`` rounds: every round
    cuts the bracket to at most 2/31 of itself (joint: the smallest of 32 points and its two neighbours; the round that finds
    the run: 1/31; split: 1/17).  With ``q2 == 0`` the first round goes into the outer bracket, which needs ``S_a``, ``S_b``."""
    return (2.0 / 31.0) ** (int(rounds) - (0 if q2_positive else 1))


def lci_sum_depth(n):
    """the longest chain of additions in a fixed-order sum of ``pxm_lci_eval`` / ``pxm_lci_data_terms`` over n terms (the
    error model of DESIGN.md section 14b): the terms a lane adds one after the other (one workgroup of 256 lanes per 1024
    terms up to 512 workgroups, grid-stride beyond), the 6 levels of the wave tree, the 4 waves of the workgroup, then the
    slices a lane of the finishing wave adds and its tree"""
    n = int(n)
    slices = min(512, max(1, -(-n // 1024)))
    return -(-n // (slices * 256)) + 6 + 4 + -(-slices // 64) + 6


def superpixel_regions(L, size):
    """int32 labels [L, 2L - 1] of the MW grid cut into superpixels of ``size`` rings x ``size`` phi-samples, numbered row
    by row; the last block of a row of blocks, and the last row of blocks, are smaller when ``size`` does not divide"""
    L, size = int(L), int(size)
    if L < 1 or size < 1:
        raise ValueError("superpixel_regions needs L >= 1 and size >= 1")
    t, p = np.arange(L) // size, np.arange(2 * L - 1) // size
    return (t[:, None] * (p[-1] + 1) + p[None, :]).astype(np.int32)


def lci_terms_np(a, b, r, s, w, T):
    """the long-double statement of the sums of one region: ``(q, S_a, S_b)`` with ``q = (1/2 sum w |r|^2, sum w Re(conj(r)
    s), 1/2 sum w |s|^2)``, ``S_a = sum T |a|``, ``S_b = sum T |b|``.  ``a``, ``b`` [n] and ``r``, ``s`` [ndata] real or
    complex, ``w`` [ndata] real, ``T`` [n] or a scalar."""
    ld = np.longdouble

    def parts(v):
        v = np.asarray(v)
        return v.real.astype(ld), (v.imag.astype(ld) if np.iscomplexobj(v) else np.zeros(v.shape, dtype=ld))

    (ar, ai), (br, bi), (rr, ri), (sr, si) = parts(a), parts(b), parts(r), parts(s)
    w, T = np.asarray(w, dtype=np.float64).astype(ld), np.broadcast_to(np.asarray(T, dtype=np.float64), ar.shape).astype(ld)
    half = ld(0.5)
    q = np.array([half * (w * (rr * rr + ri * ri)).sum(), (w * (rr * sr + ri * si)).sum(), half * (w * (sr * sr + si * si)).sum()],
                 dtype=ld)
    return q, (T * np.sqrt(ar * ar + ai * ai)).sum(), (T * np.sqrt(br * br + bi * bi)).sum()


def lci_eval_np(a, b, T, xi):
    """the long-double statement of ``pxm_lci_eval`` for one region: ``P_j = sum_k T_k |a_k + xi_j b_k|`` -> long double
    [len(xi)], the modulus from ``(a_re + xi b_re, a_im + xi b_im)``"""
    ld = np.longdouble
    a, b = np.asarray(a), np.asarray(b)
    xi = np.atleast_1d(np.asarray(xi, dtype=np.float64)).astype(ld)[:, None]
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), a.shape).astype(ld)
    re = a.real.astype(ld) + xi * b.real.astype(ld)
    if np.iscomplexobj(a) or np.iscomplexobj(b):
        im = a.imag.astype(ld) + xi * b.imag.astype(ld)
        return (T * np.sqrt(re * re + im * im)).sum(axis=1)
    return (T * np.abs(re)).sum(axis=1)


def lci_search_np(q, a, b, T, lmda, gamma, rounds=10):
    """the numpy statement of ``pxm_lci_search`` for one region, the same bracket / joint / split rules in float64 (the sums
    are numpy's, so the numbers agree with the device's to rounding, not bit for bit).  ``q`` = (q0, q1, q2).  Returns a
    dict: ``lower``, ``upper`` (the inner points of the final brackets: F <= gamma was evaluated there), ``width_lower``,
    ``width_upper``, ``f_min`` and ``xi_min`` (the smallest F seen), ``outer`` (lo, hi) and ``status``."""
    q0, q1, q2 = (float(v) for v in q)
    lmda, gamma = float(lmda), float(gamma)
    a, b = np.asarray(a), np.asarray(b)
    cplx = np.iscomplexobj(a) or np.iscomplexobj(b)
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), a.shape)
    nan, inf = float("nan"), float("inf")

    def P(xi):
        with np.errstate(invalid="ignore", over="ignore"):
            re = a.real + np.asarray(xi)[:, None] * b.real
            if not cplx:
                return (T * np.abs(re)).sum(axis=1)
            im = a.imag + np.asarray(xi)[:, None] * b.imag
            return (T * np.sqrt(re * re + im * im)).sum(axis=1)

    def result(status, lower, upper, wlo, whi, fmin, ximin, outer):
        if status & LCI_NONFINITE:
            lower = upper = fmin = ximin = nan
        return dict(lower=lower, upper=upper, width_lower=wlo, width_upper=whi, f_min=fmin, xi_min=ximin, outer=outer, status=status)

    Sa, Sb = float(P([0.0])[0]), float((T * np.abs(b)).sum())
    fmin, ximin, outer = inf, nan, (nan, nan)
    if not np.all(np.isfinite([q0, q1, q2, gamma, Sa, Sb])):
        return result(LCI_NONFINITE, nan, nan, nan, nan, nan, nan, outer)
    left = int(rounds)
    if q2 > 0.0:
        cc = q0 - gamma
        disc = q1 * q1 - 4.0 * q2 * cc
        if disc < 0.0:
            return result(LCI_EMPTY, nan, nan, nan, nan, fmin, ximin, outer)
        t = -0.5 * (q1 + np.copysign(np.sqrt(disc), q1))
        r1, r2 = (0.0, 0.0) if t == 0.0 else (t / q2, cc / t)
        lo, hi = min(r1, r2), max(r1, r2)
    else:  # the first round of the device goes into this bracket
        left -= 1
        fmin, ximin = q0 + Sa / lmda, 0.0
        D = Sb - lmda * abs(q1)  # F >= q0 - |q1| |xi| + (|xi| S_b - S_a) / lmda  (q1 = 0 whenever s = 0)
        if not D > 0.0:
            if q1 != 0.0 or fmin <= gamma:
                return result(LCI_UNCONSTRAINED, -inf, inf, 0.0, 0.0, fmin, ximin, outer)
            return result(LCI_EMPTY, nan, nan, nan, nan, fmin, ximin, outer)
        R = (lmda * (gamma - q0) + Sa) / D
        if R < 0.0:
            return result(LCI_EMPTY, nan, nan, nan, nan, fmin, ximin, outer)
        lo, hi = -R, R
    outer = (lo, hi)
    split, lo_in, hi_in = False, nan, nan
    n, h = LCI_POINTS, LCI_POINTS // 2
    for _ in range(left):
        if not split:
            x = np.minimum(lo + (hi - lo) * np.arange(n) / (n - 1.0), hi)
            x[-1] = hi
        else:
            f = np.arange(1.0, h + 1)
            x = np.concatenate([np.minimum(lo + (lo_in - lo) * f / (h + 1.0), lo_in), np.minimum(hi_in + (hi - hi_in) * f / (h + 1.0), hi)])
        Pv = P(x)
        if not np.all(np.isfinite(Pv)):
            return result(LCI_NONFINITE, nan, nan, nan, nan, nan, nan, outer)
        F = ((q2 * x + q1) * x + q0) + Pv / lmda
        jm = int(np.argmin(F))
        if F[jm] < fmin:
            fmin, ximin = float(F[jm]), float(x[jm])
        inside = np.flatnonzero(F <= gamma)
        if not split:
            if inside.size:
                j0, j1 = int(inside[0]), int(inside[-1])
                lo, lo_in, hi_in, hi = x[max(j0 - 1, 0)], x[j0], x[j1], x[min(j1 + 1, n - 1)]
                split = True
            else:
                lo, hi = x[max(jm - 1, 0)], x[min(jm + 1, n - 1)]
        else:
            low, up = inside[inside < h], inside[inside >= h]
            if low.size:
                j0 = int(low[0])
                lo, lo_in = (x[j0 - 1] if j0 > 0 else lo), x[j0]
            else:
                lo = x[h - 1]
            if up.size:
                j1 = int(up[-1])
                hi, hi_in = (x[j1 + 1] if j1 < n - 1 else hi), x[j1]
            else:
                hi = x[h]
    if not split:
        return result(LCI_EMPTY, float(lo), float(hi), float(hi - lo), float(hi - lo), fmin, ximin, outer)
    return result(LCI_OK, float(lo_in), float(hi_in), float(lo_in - lo), float(hi - hi_in), fmin, ximin, outer)


def _lci_check_setup(forward, prior):
    """the scope of the construction: synthesis setting, stock L1 prior, pixel-space transform, diagonal inverse covariance"""
    from .mcmc import _is_stock_l1

    if getattr(forward, "setting", None) != "synthesis":
        raise ValueError("local credible intervals are defined in the synthesis setting (the surrogate lives in coefficient space)")
    if not _is_stock_l1(prior):
        raise ValueError("local credible intervals need the stock synthesis L1 prior: the objective is formed from prior.T")
    tr = getattr(forward, "transform", None)
    if tr is None or not hasattr(tr, "forward") or not hasattr(tr, "inverse"):
        raise ValueError("local credible intervals need forward.transform with forward and inverse")
    if getattr(tr, "harmonic", False):
        raise ValueError("local credible intervals need a pixel-space transform: with harmonic=True there is no image to cut into regions")
    if hasattr(forward.invcov, "matvec"):
        raise ValueError("local credible intervals need a diagonal inverse covariance; a full covariance matrix is not supported")


def _lci_weights(forward):
    """w: the real diagonal inverse covariance of ``optim.gradient_operator(forward)``, float64 [ndata] on the device"""
    from .optim import gradient_operator

    diag = gradient_operator(forward).invcov.diag
    return (diag.real if diag.is_complex() else diag).to(torch.float64).contiguous()


def _lci_preds(forward, X):
    """forward.forward of a [C, N] batch with the data in the dtype of the residual -> (preds [C, ndata], data [ndata])"""
    p = ops.as_device(forward.forward(X))
    dt = forward._resid_dtype(p) if hasattr(forward, "_resid_dtype") else p.dtype
    return p.to(dt).contiguous(), forward.data_dev.to(dt).contiguous()


def map_objective(forward, prior, params, X):
    """``F(X) = 1/2 sum w |forward(X) - data|^2 + (1 / lmda) sum T |X|`` per chain -> float64 [C] on the device (``[1]`` for a
    1-D ``X``), from the reductions the samplers use.  Defined through ``prior.T`` as :mod:`pxmcmc_amd.optim` explains, with
    ``w = Re(invcov)``: the objective FISTA minimises, so at ``FISTA.X_map`` it equals ``FISTA.objective_map`` up to the
    rounding of the prior sum.  Synthesis setting, stock L1 prior, diagonal inverse covariance."""
    _lci_check_setup(forward, prior)
    x, _ = ops._batched(ops.as_device(X))
    p, d = _lci_preds(forward, x)
    w = _lci_weights(forward)
    l2 = ops.reduce_l2(p, d, w.to(p.dtype) if p.is_complex() else w)
    T = prior.T_dev
    l1 = ops.reduce_l1(x) * T if isinstance(T, float) else ops.reduce_l1(x, T)
    return 0.5 * l2.real + l1 / float(params.lmda)


def _regions_setup(fn, forward, X_map, regions, batch):
    """what the region-wise tools from the MAP point share: the MAP point as one complex128 [nparams] device vector, its
    image, the label contract (-1: in no region; 0 ... nregions - 1, each with a pixel) and the batch, to which the
    operators are grown -> (transform, X, x_map, labels, nregions, pixels per region, batch)"""
    tr = forward.transform
    X = ops.as_device(X_map)
    if X.dim() == 2 and X.shape[0] == 1:
        X = X[0]
    if X.dim() != 1 or X.shape[0] != int(forward.nparams):
        raise ValueError("%s: X_map must be one MAP point [nparams]" % fn)
    if batch is None:
        batch = int(getattr(tr, "max_chains", 1))
    batch = int(batch)
    if batch < 1:
        raise ValueError("%s needs batch >= 1 and rounds >= 1" % fn)
    for op in (tr, getattr(forward, "measurement", None)):
        if hasattr(op, "ensure_chains"):
            op.ensure_chains(batch)
    X = X.to(torch.complex128).contiguous()
    x_map = ops.as_device(tr.inverse(X[None]))[0]
    labels = np.asarray(regions)
    if not np.issubdtype(labels.dtype, np.integer) or labels.size != x_map.shape[0]:
        raise ValueError("%s: regions must be an integer label per pixel (%d pixels)" % (fn, x_map.shape[0]))
    if labels.min() < -1 or labels.max() < 0:
        raise ValueError("%s: labels are -1 (no region) or 0 ... nregions - 1, with at least one region" % fn)
    nreg = int(labels.max()) + 1
    counts = np.bincount(labels[labels >= 0].ravel(), minlength=nreg)
    if (counts == 0).any():
        raise ValueError("%s: region %d has no pixel" % (fn, int(np.flatnonzero(counts == 0)[0])))
    return tr, X, x_map, labels, nreg, counts, batch


class LocalCredibleIntervals:
    """the result of :func:`local_credible_intervals`: one entry per region of ``lower``, ``upper``, ``range`` (= upper -
    lower), ``map_value``, ``width`` (the larger of the two final bracket widths: each end is known to that), ``f_min``,
    ``xi_min``, ``status`` (numpy arrays ``[nregions]``), ``outer`` (``[nregions, 2]``: the outer bracket the search started
    from, so ``width <= lci_shrink_factor(rounds) * (outer[:, 1] - outer[:, 0])``), the ``threshold`` used and the ``labels``"""

    FIELDS = ("lower", "upper", "range", "map_value", "width", "f_min", "xi_min", "status", "outer")

    def __init__(self, labels, threshold, **fields):
        self.labels, self.threshold = labels, threshold
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    def to_map(self, values=None):
        """paint one value per region (default: ``range``) back onto the pixels, in the shape of the label array; NaN where
        the label is -1"""
        values = np.asarray(self.range if values is None else values, dtype=np.float64)
        if values.shape != self.lower.shape:
            raise ValueError("to_map: one value per region is expected")
        out = np.full(self.labels.shape, np.nan)
        on = self.labels >= 0
        out[on] = values[self.labels[on]]
        return out


def local_credible_intervals(forward, prior, params, X_map, regions, threshold=None, alpha=0.05, rounds=10, batch=None):
    """Local credible intervals of Cai, Pereyra & McEwen (2018) from the MAP point, searched on the device (DESIGN.md section
    14b).  For every region with indicator image ``zeta`` the surrogate ``X(xi) = X_map + A[(xi - x_map) zeta]`` (``A =
    transform.forward``, ``x_map = transform.inverse(X_map)``) sets the region of the band-limited image to the constant xi;
    the interval is ``{xi : F(X(xi)) <= threshold}``, F the objective of :func:`map_objective`.  **xi is real**: for a complex
    image (a spin field, complex data) the region is set to the real constant xi, its imaginary part to zero.

    :param X_map: the MAP point, ``[N]`` (``FISTA.run``'s result for one chain)
    :param regions: int labels over the pixels (any shape with ``npix`` entries, e.g. :func:`superpixel_regions`); -1: in no
        region; the labels in use must be 0 ... nregions - 1, an unused one raises
    :param threshold: the level gamma; ``None``: :func:`approx_credible_region_threshold` of ``map_objective(X_map)`` with
        ``ndim = forward.nparams`` real dimensions, twice that with ``params.complex`` (the dimension the samplers started
        from this point move in)
    :param rounds: search rounds; every end is then known to ``lci_shrink_factor(rounds)`` of the outer bracket
    :param batch: regions per pass; ``None``: the chain capacity of the operators (``transform.max_chains``).  The operators
        are grown to it (``ensure_chains``); the last batch may be smaller

    Per batch: two ``transform.forward`` calls (``b = A zeta``, ``A (x_map zeta)``), two ``forward.forward`` calls and the
    three ``lci_*`` launches sequences; one read-back at the end.  Returns :class:`LocalCredibleIntervals`."""
    _lci_check_setup(forward, prior)
    if int(rounds) < 1:
        raise ValueError("local_credible_intervals needs batch >= 1 and rounds >= 1")
    tr, X, x_map, labels, nreg, counts, batch = _regions_setup("local_credible_intervals", forward, X_map, regions, batch)
    cplx_state = torch.complex128
    dev = X.device
    lab = torch.from_numpy(labels.reshape(-1).astype(np.int64)).to(dev)
    lmda = float(params.lmda)
    T = prior.T_dev
    w = _lci_weights(forward)
    if threshold is None:
        ndim = int(forward.nparams) * (2 if getattr(params, "complex", False) else 1)
        gamma1 = approx_credible_region_threshold(map_objective(forward, prior, params, X), ndim, alpha)  # (a device tensor)
    else:
        gamma1 = torch.full((1,), float(threshold), dtype=torch.float64, device=dev)
    gamma = gamma1.expand(batch).contiguous()
    out = torch.empty((nreg, 8), dtype=torch.float64, device=dev)
    status = torch.empty(nreg, dtype=torch.int32, device=dev)
    quad = torch.empty((batch, 3), dtype=torch.float64, device=dev)
    ndata = int(forward.data_dev.numel())
    scratch = ops.lci_scratch(max(int(X.shape[0]), ndata), batch, dev)
    ids = torch.arange(batch, device=dev)
    for r0 in range(0, nreg, batch):
        Cb = min(batch, nreg - r0)
        zeta = (lab[None, :] == (r0 + ids[:Cb, None])).to(cplx_state)
        b = ops.as_device(tr.forward(zeta), cplx_state)
        a = X[None] - ops.as_device(tr.forward(zeta * x_map[None]), cplx_state)
        pa, d = _lci_preds(forward, a)
        pb, _ = _lci_preds(forward, b)
        ops.lci_data_terms(pa, pb, d, w, out=quad[:Cb], scratch=scratch)
        ops.lci_search(a, b, T, quad[:Cb], lmda, gamma[:Cb], rounds=rounds, out=out[r0 : r0 + Cb], status=status[r0 : r0 + Cb],
                       scratch=scratch)
    # the one read-back: the results, and the MAP image for the plain mean over every region (summed on the host in pixel
    # order: a device scatter-add would add in an order that changes from call to call)
    flat = torch.cat([out.reshape(-1), status.to(torch.float64), gamma1.reshape(-1)[:1], x_map.real.to(torch.float64)]).cpu().numpy()
    host = flat[: 8 * nreg].reshape(nreg, 8)
    stat, thr, img = flat[8 * nreg : 9 * nreg].astype(np.int32), float(flat[9 * nreg]), flat[9 * nreg + 1 :]
    on = labels.reshape(-1) >= 0
    means = np.bincount(labels.reshape(-1)[on], weights=img[on], minlength=nreg) / counts
    lower, upper = host[:, 0], host[:, 1]
    with np.errstate(invalid="ignore"):
        rng = upper - lower
    return LocalCredibleIntervals(labels, thr, lower=lower, upper=upper, range=rng, map_value=means,
                                  width=np.fmax(host[:, 2], host[:, 3]), f_min=host[:, 4], xi_min=host[:, 5], status=stat,
                                  outer=host[:, 6:8].copy())


# ---- hypothesis tests of image structure from the MAP point --------------------------------------------
HYP_NONFINITE = 8  # status bit of a region whose surrogate, sums or profile are not finite (beside the LCI_* bits)


def inpaint_sum_depth(npix):
    """the longest chain of additions in a fixed-order sum of ``pxm_inpaint_step`` over npix pixels (the error model of
    DESIGN.md section 14c), for both dtypes: a lane adds the two terms of each of its pairs of real pixels one after the
    other (one workgroup of 256 lanes per 1024 pixels up to 512 workgroups, grid-stride beyond; a complex pixel is one
    term, never a longer chain), then the 6 levels of the wave tree, the 4 waves of the workgroup, the slices a lane of the
    finishing wave adds and its tree"""
    n = int(npix)
    slices = min(512, max(1, -(-n // 1024)))
    return 2 * -(-(-(-n // 2)) // (slices * 256)) + 6 + 4 + -(-slices // 64) + 6


def inpaint_step_np(y, x_prev, x_map, labels, region, tol2, done, iters, stat):
    """the numpy statement of ``pxm_inpaint_step``: ``y``, ``x_prev`` [C, npix], ``x_map`` [npix], ``labels`` int [npix],
    ``region``, ``done``, ``iters`` int [C], ``stat`` [C, 2] -> new ``(x_next, done, iters, stat)``.  The select is exact;
    the two sums are formed in long double (``stat`` comes back as long double [C, 2]) and the flag is ``stat[0] <= tol2 *
    stat[1]`` on their float64 roundings, one multiply and one compare.  A slot that is done is copied through and nothing
    of it changes; a label < 0 belongs to no slot; a NaN never freezes a slot."""
    ld = np.longdouble
    y, x_prev, x_map = np.asarray(y), np.asarray(x_prev), np.asarray(x_map)
    labels, region = np.asarray(labels).reshape(-1), np.asarray(region)
    done, iters = np.array(done, dtype=np.int32), np.array(iters, dtype=np.int32)
    stat = np.array(stat, dtype=ld)
    x_next = np.array(x_prev, copy=True)
    for c in range(x_prev.shape[0]):
        if done[c]:
            continue
        inside = (labels == region[c]) & (labels >= 0)
        x_next[c] = np.where(inside, y[c], x_map.astype(x_prev.dtype))
        d = x_next[c] - x_prev[c]  # (each component difference rounded once, as on the device)
        d2 = (d.real.astype(ld) ** 2).sum() + (d.imag.astype(ld) ** 2).sum()
        n2 = (x_next[c].real.astype(ld) ** 2).sum() + (x_next[c].imag.astype(ld) ** 2).sum()
        iters[c] += 1
        stat[c] = d2, n2
        with np.errstate(invalid="ignore", over="ignore"):
            done[c] = int(np.float64(d2) <= np.float64(tol2) * np.float64(n2))
    return x_next, done, iters, stat


def _soft_np(x, T):
    with np.errstate(divide="ignore", invalid="ignore"):
        mod = np.abs(x)
        return np.where(mod > T, x * (1.0 - T / np.where(mod > 0, mod, 1.0)), 0.0 * x)


def inpaint_np(A, Psi, x_map, zeta, tau, iters, tol):
    """the numpy statement of segment inpainting for one region: ``x^0 = x* (1 - zeta)``, ``x^{t+1} = x* (1 - zeta) + zeta
    Psi soft_tau(A x^t)`` for at most ``iters`` iterations, frozen once ``|x^{t+1} - x^t|^2 <= tol^2 |x^{t+1}|^2``.  ``A``,
    ``Psi``: callables (image -> coefficients -> image); ``zeta``: 0 / 1 per pixel; ``tau``: scalar or one value per
    coefficient.  Returns a dict: ``x``, ``iters_used``, ``rel_change`` (of the last iteration made) and ``history`` (the
    relative change of every iteration made)."""
    x_map = np.asarray(x_map)
    inside = np.asarray(zeta).reshape(-1) != 0
    labels = np.where(inside, 0, -1)
    x = np.where(inside, 0.0 * x_map, x_map)[None]
    done, its, stat = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros((1, 2))
    history = []
    for _ in range(int(iters)):
        if done[0]:
            break
        y = np.asarray(Psi(_soft_np(np.asarray(A(x[0])), tau))).astype(x.dtype)[None]
        x, done, its, stat = inpaint_step_np(y, x, x_map, labels, [0], float(tol) ** 2, done, its, stat)
        history.append(float(np.sqrt(stat[0, 0] / stat[0, 1])) if stat[0, 1] > 0 else (0.0 if stat[0, 0] == 0 else np.inf))
    return dict(x=x[0], iters_used=int(its[0]), rel_change=history[-1] if history else np.nan, history=history)


def gaussian_smooth(x, L, sigma, spin=0):
    """``G_sigma * x`` for MW images ``x`` [C, npix] (or [npix]) on the device: one ``ops.ShtPlan(L, spin)`` forward, a multiply
    by ``exp(-l (l + 1) sigma^2 / 2)`` on the ssht index ``l^2 + l + m``, one inverse -> complex128, the shape of ``x``"""
    x = ops.as_device(x, torch.complex128)
    plan = ops.ShtPlan(int(L), int(spin), max_chains=1 if x.dim() == 1 else int(x.shape[0]))
    el = np.repeat(np.arange(int(L)), 2 * np.arange(int(L)) + 1).astype(np.float64)
    g = ops.as_device(np.exp(-el * (el + 1.0) * float(sigma) ** 2 / 2.0))
    return plan.inverse(plan.forward(x) * g)


class SurrogateImages:
    """the result of :func:`inpaint_regions` / :func:`smooth_regions`: ``images`` (complex128 device tensor [nregions, npix]:
    the surrogate of every region), ``iters_used`` (int32 [nregions]), ``rel_change`` (float64 [nregions]: ``|x^{t+1} - x^t|
    / |x^{t+1}|`` of the last iteration a region made), ``frozen`` (bool [nregions]), ``x_map`` (the MAP image, [npix]),
    ``replayed`` (the iterations ran by graph replay) and ``graph_error`` (``None``, or the exception that made capture fall
    back to eager stepping)"""

    def __init__(self, images, iters_used, rel_change, frozen, x_map, replayed=False, graph_error=None):
        self.images, self.iters_used, self.rel_change, self.frozen, self.x_map = images, iters_used, rel_change, frozen, x_map
        self.replayed, self.graph_error = replayed, graph_error


def _rel_change(stat):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(stat[:, 0] / stat[:, 1])


class _SurrogateBatches:
    """The surrogate images of the regions, ``batch`` slots at a time, in static buffers: ``run(r0)`` leaves the surrogates of
    the regions r0 ... r0 + batch - 1 in ``images`` with ``iters`` / ``stat`` / ``done`` beside them, all of them views that
    the next call overwrites.  A slot beyond the last region holds region -1 (no pixel: its image is the MAP image), so
    every batch is a full one and one captured graph serves them all; a slot's numbers do not depend on its batch."""

    def __init__(self, tr, x_map, labels, nreg, batch):
        dev = x_map.device
        self.tr, self.x_map, self.nreg, self.batch = tr, x_map, int(nreg), int(batch)
        self.npix = int(x_map.shape[0])
        self.labels = torch.from_numpy(np.ascontiguousarray(labels.reshape(-1).astype(np.int32))).to(dev)
        self.ids = torch.arange(batch, dtype=torch.int32, device=dev)
        self.region = torch.empty(batch, dtype=torch.int32, device=dev)
        self.done = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.stat = torch.zeros((batch, 2), dtype=torch.float64, device=dev)
        self.XA = torch.empty((batch, self.npix), dtype=torch.complex128, device=dev)
        self.XB = torch.empty_like(self.XA)
        self.scratch = ops.inpaint_scratch(self.npix, batch, dev)
        self.images = self.XA
        self.graph, self.graph_error = None, None

    def _step(self, y, src, dst, tol2):
        ops.inpaint_step(y, src, self.x_map, self.labels, self.region, tol2, self.done, self.iters, self.stat, out=dst,
                         scratch=self.scratch)

    def _begin(self, r0):
        """the regions of the batch, flags and counters cleared"""
        self.region.copy_(torch.where(self.ids + int(r0) < self.nreg, self.ids + int(r0), -1))
        self.done.zero_(), self.iters.zero_(), self.stat.zero_()


class _InpaintBatches(_SurrogateBatches):
    def __init__(self, tr, x_map, labels, nreg, batch, tau, iters, tol, use_graph):
        super().__init__(tr, x_map, labels, nreg, batch)
        self.niter, self.tol2 = int(iters), float(tol) ** 2
        if self.niter < 1 or not (float(tol) >= 0.0 and np.isfinite(float(tol))):
            raise ValueError("inpainting needs iters >= 1 and a finite tol >= 0")
        tau_arr = np.asarray(tau.detach().cpu() if isinstance(tau, torch.Tensor) else tau, dtype=np.float64)
        if tau_arr.size == 1:  # (a python scalar: the wrapper of the threshold kernel then reads nothing back)
            self.tau = float(tau_arr.reshape(-1)[0])
        else:
            self.tau = ops.as_device(tau_arr.reshape(-1), torch.float64)
        if not np.all(tau_arr >= 0.0):
            raise ValueError("inpainting needs tau >= 0")
        self.zero = torch.zeros_like(self.XA)
        if use_graph and self.niter >= 2:
            self._capture()

    def _one(self, src, dst):
        """one iteration from the images in src to dst: A, the threshold, Psi, then the step kernel"""
        coef = ops.as_device(self.tr.forward(src), torch.complex128)
        y = ops.as_device(self.tr.inverse(ops.soft(coef, self.tau)), torch.complex128)
        self._step(y, src, dst, self.tol2)

    def _two(self):
        self._one(self.XA, self.XB)
        self._one(self.XB, self.XA)

    def _init(self, r0):
        """x^0 = x* (1 - zeta) in XA, by the step kernel itself on y = 0 (no indicator array here either)"""
        self._begin(r0)
        self._step(self.zero, self.XB, self.XA, 0.0)
        self.done.zero_(), self.iters.zero_(), self.stat.zero_()

    def _capture(self):
        """two ping-pong iterations in one HIP graph, after a warm-up on a side stream (lazy allocations); when capture
        raises: eager stepping, same results"""
        try:
            self.XB.zero_()
            self._init(0)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._two()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with ops.capture_scope(), torch.cuda.graph(g):
                self._two()
            self.graph = g
        except Exception as exc:  # capture unsupported in this environment
            self.graph, self.graph_error = None, repr(exc)
            torch.cuda.synchronize()

    def run(self, r0):
        self.XB.zero_()  # (x_prev of the initialising step: any finite values)
        self._init(r0)
        for _ in range(self.niter // 2):
            if self.graph is not None:
                self.graph.replay()
            else:
                self._two()
        if self.niter % 2:
            self._one(self.XA, self.XB)
        self.images = self.XB if self.niter % 2 else self.XA
        return self.images


class _SmoothBatches(_SurrogateBatches):
    def __init__(self, tr, x_map, labels, nreg, batch, sigma):
        super().__init__(tr, x_map, labels, nreg, batch)
        sigma = float(sigma)
        if not (sigma >= 0.0 and np.isfinite(sigma)):
            raise ValueError("the smoothing surrogate needs a finite sigma >= 0")
        L = getattr(tr, "L", None)
        if L is None or int(L) * (2 * int(L) - 1) != self.npix:
            raise ValueError("the smoothing surrogate needs a transform of MW images with a bandlimit L")
        self.smooth = gaussian_smooth(x_map, int(L), sigma, int(getattr(tr, "spin", 0)))
        self.XB.copy_(x_map[None].expand(batch, -1))  # x_prev of the one step: rel_change is |x_sgt - x*| / |x_sgt|
        self.Y = self.smooth[None].expand(batch, -1).contiguous()

    def run(self, r0):
        """one step of the step kernel with tol = 0: x_sgt = x* (1 - zeta) + zeta (G_sigma * x*)"""
        self._begin(r0)
        self._step(self.Y, self.XB, self.XA, 0.0)
        return self.images


def _collect_surrogates(batches, nreg):
    """every batch of ``batches`` into one :class:`SurrogateImages` (nregions x npix complex values on the device), with
    one read-back at the end"""
    B = batches.batch
    images = torch.empty((nreg, batches.npix), dtype=torch.complex128, device=batches.x_map.device)
    its, stats, dones = [], [], []
    for r0 in range(0, nreg, B):
        Cb = min(B, nreg - r0)
        images[r0 : r0 + Cb] = batches.run(r0)[:Cb]
        its.append(batches.iters[:Cb].clone()), stats.append(batches.stat[:Cb].clone()), dones.append(batches.done[:Cb].clone())
    stat = torch.cat(stats).cpu().numpy()
    return SurrogateImages(images, torch.cat(its).cpu().numpy(), _rel_change(stat), torch.cat(dones).cpu().numpy() != 0, batches.x_map,
                           replayed=batches.graph is not None, graph_error=batches.graph_error)


def _surrogate_check_setup(forward):
    tr = getattr(forward, "transform", None)
    if getattr(forward, "setting", None) != "synthesis":
        raise ValueError("the surrogate images are defined in the synthesis setting (X_map holds coefficients)")
    if tr is None or not hasattr(tr, "forward") or not hasattr(tr, "inverse") or getattr(tr, "harmonic", False):
        raise ValueError("the surrogate images need a pixel-space forward.transform with forward and inverse")


def inpaint_regions(forward, X_map, regions, tau, iters=100, tol=1e-6, batch=None, use_graph=True):
    """Segment-inpainted surrogates of the MAP image, one per region (Cai, Pereyra & McEwen 2018 II section 4.2; DESIGN.md
    section 14c): with ``A = transform.forward``, ``Psi = transform.inverse``, ``x* = Psi X_map`` and ``zeta`` the indicator of
    a region, ``x^0 = x* (1 - zeta)`` and ``x^{t+1} = x* (1 - zeta) + zeta Psi soft_tau(A x^t)`` for ``iters`` iterations; a
    region freezes once ``|x^{t+1} - x^t|^2 <= tol^2 |x^{t+1}|^2`` (both norms over the whole image) and is copied through
    from then on.  Everything runs on the device and nothing is read back until the end.

    :param regions: int labels over the pixels, the contract of :func:`local_credible_intervals`
    :param tau: the threshold, a scalar or one value per coefficient ``[nparams]``
    :param batch: regions per pass; ``None``: the chain capacity of the transform.  The last batch is filled with slots
        that hold no region; a region's numbers do not depend on its batch
    :param use_graph: capture two iterations into a HIP graph and replay them (eager stepping when capture raises, and
        with ``False``: the same numbers)

    Returns :class:`SurrogateImages` (``nregions x npix`` complex values stay on the device: mind the size)."""
    _surrogate_check_setup(forward)
    tr, _, x_map, labels, nreg, _, batch = _regions_setup("inpaint_regions", forward, X_map, regions, batch)
    return _collect_surrogates(_InpaintBatches(tr, x_map, labels, nreg, batch, tau, iters, tol, use_graph), nreg)


def smooth_regions(forward, X_map, regions, sigma, batch=None):
    """The smoothing surrogates of the MAP image, one per region: ``x* (1 - zeta) + zeta (G_sigma * x*)``, the surrogate for
    testing sub-structure (:func:`gaussian_smooth`, then one step of the inpainting kernel).  Returns
    :class:`SurrogateImages`; ``rel_change`` is ``|x_sgt - x*| / |x_sgt|``."""
    _surrogate_check_setup(forward)
    tr, _, x_map, labels, nreg, _, batch = _regions_setup("smooth_regions", forward, X_map, regions, batch)
    return _collect_surrogates(_SmoothBatches(tr, x_map, labels, nreg, batch, sigma), nreg)


class HypothesisTestResult:
    """the result of :func:`hypothesis_test`, one entry per region: ``physical`` (bool: the surrogate lies outside the
    credible region, ``f_sgt > threshold``; ``False``: inconclusive), ``removable`` (xi+, the end of ``{xi : F(xi) <=
    threshold}`` along the path from the MAP point, xi = 0, to the surrogate, xi = 1: the fraction of the structure that can
    be removed inside the credible region; >= 1, possibly inf, where the test is inconclusive), ``f_sgt`` (= ``profile[:,
    -1]``), ``profile`` (``[nregions, 32]``: F at ``xi`` = j / 31), ``iters_used``, ``rel_change`` (of the surrogate),
    ``status`` (0, or the ``LCI_*`` bits of the search and ``HYP_NONFINITE``), ``xi``, the ``threshold`` used and the ``labels``;
    ``lower`` (xi-) and ``width`` (the larger of the two final bracket widths of the search: each end is known to that)"""

    FIELDS = ("physical", "removable", "lower", "width", "f_sgt", "profile", "iters_used", "rel_change", "status")

    def __init__(self, labels, threshold, xi, **fields):
        self.labels, self.threshold, self.xi = labels, threshold, xi
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    def to_map(self, values=None):
        """paint one value per region (default: ``physical`` as 1.0 / 0.0) back onto the pixels, in the shape of the label
        array; NaN where the label is -1"""
        values = np.asarray(self.physical if values is None else values, dtype=np.float64)
        if values.shape != self.physical.shape:
            raise ValueError("to_map: one value per region is expected")
        out = np.full(self.labels.shape, np.nan)
        on = self.labels >= 0
        out[on] = values[self.labels[on]]
        return out


def hypothesis_test(forward, prior, params, X_map, regions, tau=None, sigma=None, surrogate="inpaint", threshold=None, alpha=0.05,
                    iters=100, tol=1e-6, rounds=10, batch=None):
    """Hypothesis tests of image structure from the MAP point (Cai, Pereyra & McEwen 2018 II section 4.2; DESIGN.md section
    14c).  For every region a surrogate image ``x_sgt`` without the structure is formed -- ``surrogate="inpaint"``:
    :func:`inpaint_regions` with the threshold ``tau``; ``surrogate="smooth"``: :func:`smooth_regions` with the width
    ``sigma`` -- and the objective F of :func:`map_objective` is followed along the straight path ``X(xi) = X_map + xi A(x_sgt
    - x*)``.  ``F(1) > threshold``: the surrogate is outside the credible region, the structure is physical; otherwise the
    test is inconclusive (so it is when the surrogate equals ``x*``).  ``threshold=None``: the level of
    :func:`local_credible_intervals`.  Scope and refusals: those of :func:`local_credible_intervals`.

    Per batch: the surrogate, one ``transform.forward`` and one ``forward.forward`` call, the 32-point profile by
    ``lci_eval`` and ``[xi-, xi+]`` by ``lci_search``; one read-back at the end.  Returns :class:`HypothesisTestResult`."""
    _lci_check_setup(forward, prior)
    if surrogate not in ("inpaint", "smooth"):
        raise ValueError("hypothesis_test: surrogate must be 'inpaint' or 'smooth'")
    if (surrogate == "inpaint") != (tau is not None) or (surrogate == "smooth") != (sigma is not None):
        raise ValueError("hypothesis_test: surrogate='inpaint' takes tau and no sigma, surrogate='smooth' sigma and no tau")
    if int(rounds) < 1:
        raise ValueError("hypothesis_test needs batch >= 1 and rounds >= 1")
    tr, X, x_map, labels, nreg, _, batch = _regions_setup("hypothesis_test", forward, X_map, regions, batch)
    if surrogate == "inpaint":
        batches = _InpaintBatches(tr, x_map, labels, nreg, batch, tau, iters, tol, True)
    else:
        batches = _SmoothBatches(tr, x_map, labels, nreg, batch, sigma)
    dev = X.device
    lmda, T, w = float(params.lmda), prior.T_dev, _lci_weights(forward)
    if threshold is None:
        ndim = int(forward.nparams) * (2 if getattr(params, "complex", False) else 1)
        gamma1 = approx_credible_region_threshold(map_objective(forward, prior, params, X), ndim, alpha)  # (a device tensor)
    else:
        gamma1 = torch.full((1,), float(threshold), dtype=torch.float64, device=dev)
    gamma = gamma1.reshape(-1)[:1].expand(batch).contiguous()
    a = X[None].expand(batch, -1).contiguous()
    pa1, d = _lci_preds(forward, X[None])
    pa = pa1.expand(batch, -1).contiguous()
    xi1 = torch.arange(LCI_POINTS, dtype=torch.float64, device=dev) / (LCI_POINTS - 1.0)
    xi = xi1[None].expand(batch, -1).contiguous()
    out = torch.empty((nreg, 8), dtype=torch.float64, device=dev)
    status = torch.empty(nreg, dtype=torch.int32, device=dev)
    profile = torch.empty((nreg, LCI_POINTS), dtype=torch.float64, device=dev)
    its = torch.empty(nreg, dtype=torch.int32, device=dev)
    stat = torch.empty((nreg, 2), dtype=torch.float64, device=dev)
    quad = torch.empty((batch, 3), dtype=torch.float64, device=dev)
    P = torch.empty((batch, LCI_POINTS + 2), dtype=torch.float64, device=dev)
    scratch = ops.lci_scratch(max(int(X.shape[0]), int(forward.data_dev.numel())), batch, dev)
    for r0 in range(0, nreg, batch):
        Cb = min(batch, nreg - r0)
        x_sgt = batches.run(r0)
        b = ops.as_device(tr.forward(x_sgt - x_map[None]), torch.complex128)
        pb, _ = _lci_preds(forward, b)
        ops.lci_data_terms(pa, pb, d, w, out=quad, scratch=scratch)
        ops.lci_eval(a, b, T, xi, out=P, scratch=scratch)
        q0, q1, q2 = quad[:Cb, 0:1], quad[:Cb, 1:2], quad[:Cb, 2:3]
        profile[r0 : r0 + Cb] = ((q2 * xi[:Cb] + q1) * xi[:Cb] + q0) + P[:Cb, :LCI_POINTS] / lmda
        ops.lci_search(a[:Cb], b[:Cb], T, quad[:Cb], lmda, gamma[:Cb], rounds=rounds, out=out[r0 : r0 + Cb],
                       status=status[r0 : r0 + Cb], scratch=scratch)
        its[r0 : r0 + Cb] = batches.iters[:Cb]
        stat[r0 : r0 + Cb] = batches.stat[:Cb]
    flat = torch.cat([out.reshape(-1), status.to(torch.float64), its.to(torch.float64), stat.reshape(-1), profile.reshape(-1),
                      gamma1.reshape(-1)[:1], xi1]).cpu().numpy()  # the one read-back
    cut = np.cumsum([8 * nreg, nreg, nreg, 2 * nreg, LCI_POINTS * nreg, 1])
    host, st, it, sums, prof, thr, xis = np.split(flat, cut)
    host, sums, prof, thr = host.reshape(nreg, 8), sums.reshape(nreg, 2), prof.reshape(nreg, LCI_POINTS), float(thr[0])
    st = st.astype(np.int32)
    st[~(np.isfinite(prof).all(axis=1) & np.isfinite(sums).all(axis=1))] |= HYP_NONFINITE
    f_sgt = prof[:, -1].copy()
    with np.errstate(invalid="ignore"):
        physical = f_sgt > thr
        # xi = 1 was evaluated: where F(1) <= threshold the end of the set is not left of it, whatever the last bracket says
        removable = np.where(~physical & np.isfinite(f_sgt), np.fmax(host[:, 1], 1.0), host[:, 1])
    return HypothesisTestResult(labels, thr, xis, physical=physical, removable=removable, lower=host[:, 0].copy(),
                                width=np.fmax(host[:, 2], host[:, 3]), f_sgt=f_sgt, profile=prof,
                                iters_used=it.astype(np.int32), rel_change=_rel_change(sums), status=st)
