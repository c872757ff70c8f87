"""
Streaming summaries: :class:`PosteriorSummary` accumulates per-chain moments and the
highest-posterior sample on the device while a sampler runs (``summary=`` of the samplers), so the posterior mean, the
standard-deviation map, the "MAP_X" sample (plot.py:75-76, 122) and R-hat across the chain batch need no saved chain.  With
``alpha=`` it also keeps the k smallest and k largest samples of every element (:func:`tail_capacity`), from which
``credible_interval_range()`` gives the numbers of :func:`~pxmcmc_amd.uncertainty.chains.credible_interval_range` on each
chain's saved samples, exactly.  With ``ess_lags=`` it accumulates the lagged products of the saved samples, from which
``ess()``, ``ess_pooled()`` and ``mcse()`` give the effective sample size and the standard error of the pooled mean.
:mod:`~pxmcmc_amd.uncertainty.streaming_np` states all of it in numpy.
"""
import warnings

import numpy as np
import torch

from .. import ops
from .streaming_np import ess_lag_count, tail_capacity


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
        self.ess_lags = None if ess_lags is None else ess_lag_count(ess_lags)
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

        def joined(k):
            return np.concatenate([np.asarray(d[k]) for d in dicts], axis=0)

        out = {k: joined(k) for k in PosteriorSummary.FIELDS if all(k in d for d in dicts)}
        # a group is (its scalar, its per-chain arrays ...): kept when every dict carries all of it with one common scalar
        for (scalar, *arrays), kind, must_agree in ((PosteriorSummary.TAIL_FIELDS, np.float64, True),
                                                    (PosteriorSummary.ESS_FIELDS, np.int64, False)):
            if not all(k in d for d in dicts for k in (scalar, *arrays)):
                continue
            values = {kind(d[scalar]).item() for d in dicts}
            if len(values) != 1:
                if must_agree:
                    raise ValueError("merge: the summaries were built with different %s: %s" % (scalar, sorted(values)))
                continue
            out[scalar] = kind(values.pop())
            out.update({k: joined(k) for k in arrays})
        return out
