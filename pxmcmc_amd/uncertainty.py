"""
Uncertainty summaries of saved chains (pxmcmc/uncertainty.py:7-56): quantile credible-interval ranges per
parameter and per wavelet scale, and the highest-posterior-density threshold.  Post-run host arithmetic,
as in the reference; ``chain_to_images`` is the batched GPU synthesis the reference's plot scripts do sample
by sample (experiments/earthtopography/plot.py:105-115).

Streaming summaries: :class:`PosteriorSummary` accumulates per-chain moments and the
highest-posterior sample on the device while a sampler runs (``summary=`` of the samplers), so the posterior mean, the
standard-deviation map, the "MAP_X" sample (plot.py:75-76, 122) and R-hat across the chain batch need no saved chain;
:func:`moments_np`, :func:`pooled_np` and :func:`rhat_np` state the same quantities in numpy.
"""
import numpy as np
import torch

from . import ops
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

    Complex states come back complex: ``mean`` as ``re + i im``, ``variance`` as ``var_re + var_im`` (``E |x - mean|^2``),
    ``best_sample`` as stored.  ``rhat()`` is per REAL component, shape ``[m]`` (``[2 nparams]`` for a complex state: a
    chain batch can have converged in one component and not in the other).  ``to_host()`` / ``merge`` carry the raw
    accumulators in the real-component layout ``[C, m]``, which :func:`pooled_np` and :func:`rhat_np` take.
    """

    FIELDS = ("count", "mean", "m2", "best", "best_logpi")

    def __init__(self, nchains, nparams, complex_, best=True, device=None):
        self.nchains, self.nparams, self.complex = int(nchains), int(nparams), bool(complex_)
        if self.nchains < 1 or self.nparams < 1:
            raise ValueError("PosteriorSummary needs nchains >= 1 and nparams >= 1")
        self.m = self.nparams * (2 if self.complex else 1)
        dev = ops.device() if device is None else device
        C, m = self.nchains, self.m
        self._count = torch.zeros(C, dtype=torch.int64, device=dev)
        self._mean = torch.zeros((C, m), dtype=torch.float64, device=dev)
        self._m2 = torch.zeros((C, m), dtype=torch.float64, device=dev)
        self.best = bool(best)
        self._best_x = torch.zeros((C, m), dtype=torch.float64, device=dev) if self.best else None
        self._best_logpi = torch.full((C,), -np.inf, dtype=torch.float64, device=dev) if self.best else None

    # ---- accumulation -----------------------------------------------------------------------------------------------
    def update(self, X, logpi=None, mask=None):
        """add one sample per chain: ``X`` [C, nparams] on the device (complex128, or float64 when ``complex_`` is False),
        ``logpi`` [C] its log posterior (float64 or complex128: the real part; needed with ``best``), ``mask`` an int32 [C]
        device tensor or a sequence of chain flags -- chains with a zero keep their accumulators untouched.  One fused pass
        and one small launch on the current stream.  With contiguous device tensors for ``X``, ``logpi`` and ``mask`` nothing is
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

    # ---- host side --------------------------------------------------------------------------------------------------
    def to_host(self):
        """plain dict of numpy arrays: ``count`` int64 [C], ``mean`` / ``m2`` float64 [C, m] in the real-component layout
        and, with ``best``, ``best`` [C, nparams] (complex for a complex state) and ``best_logpi`` [C]"""
        out = {"count": self._count.cpu().numpy(), "mean": self._mean.cpu().numpy(), "m2": self._m2.cpu().numpy()}
        if self.best:
            out["best"] = self.best_sample().cpu().numpy()
            out["best_logpi"] = self._best_logpi.cpu().numpy()
        return out

    @staticmethod
    def merge(dicts):
        """concatenate the chains of several ``to_host()`` dicts (one per rank, in rank order) -> one such dict;
        ``rhat_np(d["count"], d["mean"], d["m2"])`` of the result is R-hat over all the chains of a multi-rank run"""
        dicts = list(dicts)
        if not dicts:
            raise ValueError("merge: no summaries")
        keys = [k for k in PosteriorSummary.FIELDS if all(k in d for d in dicts)]
        return {k: np.concatenate([np.asarray(d[k]) for d in dicts], axis=0) for k in keys}
