"""Streaming posterior summaries accumulated on the device: moments and R-hat, tail heaps for credible intervals, lagged
autocovariances for the effective sample size (csrc/moments.hip, tails.hip, acov.hip)."""
import torch

from .._lib import check, lib
from ._args import _CPLX, _REAL, _dev_tensors, _p, _stream


def _mask_arg(fn, mask, C_):
    """the optional ``mask`` of the update entry points"""
    if mask is not None:
        _dev_tensors(fn, "mask must be a contiguous int32 [C] device tensor", (mask, torch.int32, (C_,)))


def _moments_rows(fn, X, C_, m):
    """the sample batch of the update entry points as (tensor, x_stride): float64 [C, m] (stride 1), or complex128 [C, m] whose
    real parts are taken (stride 2); a complex state accumulated per component is passed as its float64 [C, 2 n] view"""
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dim() == 2 and X.shape[0] == C_ and X.is_contiguous()
            and X.dtype in (_REAL, _CPLX) and X.shape[1] == m and X.data_ptr() % 16 == 0):
        raise TypeError("%s: X must be a contiguous 16-byte aligned float64 or complex128 [%d, %d] device tensor" % (fn, C_, m))
    return X, (2 if X.dtype == _CPLX else 1)


def moments_update(X, count, mean, m2, mask=None, logpi=None, best_logpi=None, best_x=None):
    """One Welford step per chain, in place on the device accumulators: ``count`` int64 [C], ``mean`` /
    ``m2`` float64 [C, m]; ``X`` float64 [C, m], or complex128 [C, m] whose real parts are accumulated.  ``mask`` int32 [C]:
    chains with a zero are left untouched.  With ``logpi`` (float64 or complex128 [C], real part), ``best_logpi`` [C] and
    ``best_x`` [C, m], a chain whose logpi exceeds its best so far also copies its sample to ``best_x``.  No allocation, no
    synchronisation: the call can be captured in a HIP graph."""
    C_, m = mean.shape
    x, xs = _moments_rows("moments_update", X, C_, m)
    _dev_tensors("moments_update", "count int64 [C], mean / m2 contiguous float64 [C, m] device tensors are expected",
                 (count, torch.int64, (C_,)), (mean, _REAL, (C_, m)), (m2, _REAL, (C_, m)))
    _mask_arg("moments_update", mask, C_)
    ls = 1
    if logpi is not None:
        if best_logpi is None or best_x is None:
            raise ValueError("moments_update: logpi, best_logpi and best_x are given together")
        if logpi.dtype not in (_REAL, _CPLX) or tuple(logpi.shape) != (C_,) or not logpi.is_contiguous() or not logpi.is_cuda:
            raise TypeError("moments_update: logpi must be a contiguous float64 or complex128 [C] device tensor")
        _dev_tensors("moments_update", "best_logpi float64 [C] and best_x contiguous float64 [C, m] are expected",
                     (best_logpi, _REAL, (C_,)), (best_x, _REAL, (C_, m)))
        ls = 2 if logpi.dtype == _CPLX else 1
    elif best_logpi is not None or best_x is not None:
        raise ValueError("moments_update: logpi, best_logpi and best_x are given together")
    check(lib.pxm_moments_update(_p(x), xs, _p(count), _p(mean), _p(m2), _p(mask), _p(logpi), ls, _p(best_logpi), _p(best_x), m, C_,
                                 _stream()))


def moments_finalize(count, mean, m2, rhat=True):
    """Reduce the accumulators of moments_update over chains (in chain order) -> (pooled_mean [m], pooled_var [m], rhat [m],
    stats [2]) on the device: pooled moments over every sample of the chains with count > 0, Gelman-Rubin R-hat of those
    chains, and stats = (max R-hat over the non-NaN elements, number of NaN elements).  ``rhat=False`` leaves the last two
    out (None) and takes any counts; with R-hat requested, chains with different counts raise PxmError."""
    if mean.dim() != 2:
        raise TypeError("moments_finalize: mean must be a float64 [C, m] device tensor")
    C_, m = mean.shape
    _dev_tensors("moments_finalize", "count int64 [C], mean / m2 contiguous float64 [C, m] device tensors are expected",
                 (count, torch.int64, (C_,)), (mean, _REAL, (C_, m)), (m2, _REAL, (C_, m)))
    pm = torch.empty(m, dtype=_REAL, device=mean.device)
    pv = torch.empty_like(pm)
    rh = st = scratch = None
    if rhat:
        rh = torch.empty_like(pm)
        st = torch.empty(2, dtype=_REAL, device=mean.device)
        scratch = torch.empty(int(lib.pxm_moments_scratch_doubles(m)), dtype=_REAL, device=mean.device)
    check(lib.pxm_moments_finalize(_p(count), _p(mean), _p(m2), m, C_, _p(pm), _p(pv), _p(rh), _p(st), _p(scratch), _stream()))
    return pm, pv, rh, st


def _tails_state(fn, lo, hi, thr_lo, thr_hi, stage, count):
    """argument checks of the tails entry points -> (C, k, m)"""
    if not (isinstance(lo, torch.Tensor) and lo.dim() == 3):
        raise TypeError("%s: lo must be a float64 [C, k, m] device tensor" % fn)
    C_, k, m = lo.shape
    B = tails_stage_depth()
    _dev_tensors(fn, "count int64 [C], lo / hi contiguous float64 [C, k, m], thr_lo / thr_hi contiguous float64 [C, m] and stage "
                 "contiguous float64 [C, %d, m] device tensors are expected" % B,
                 (count, torch.int64, (C_,)), (lo, _REAL, (C_, k, m)), (hi, _REAL, (C_, k, m)), (stage, _REAL, (C_, B, m)),
                 *((t, _REAL, (C_, m)) for t in (thr_lo, thr_hi) if t is not None))  # (the read-out has no thresholds)
    if int(lib.pxm_tails_buffer_doubles(m, C_, k)) != lo.numel():
        raise ValueError("%s: bad tail shape [%d, %d, %d]" % (fn, C_, k, m))
    return C_, k, m


def tails_stage_depth():
    """B: the saves ``tails_update`` stages in its ring ``stage`` float64 [C, B, m] between two merges into the heaps"""
    return int(lib.pxm_tails_stage_doubles(1, 1))


def tails_update(X, count, lo, hi, thr_lo, thr_hi, stage, nsamples, mask=None):
    """One save into the per-element tail heaps, in place: ``lo`` / ``hi`` float64 [C, k, m] keep the k
    smallest / largest samples, ``thr_lo`` / ``thr_hi`` [C, m] their thresholds, ``stage`` [C, B, m] (:func:`tails_stage_depth`)
    the saves not merged into them yet; ``X`` as for :func:`moments_update`.  ``count``
    int64 [C] is the number of samples before this one and is not written: call this before the ``moments_update`` of the same
    sample.  ``nsamples`` is the number of saves k was sized for (:func:`pxmcmc_amd.uncertainty.tail_capacity`); a chain
    that has reached it, or that ``mask`` (int32 [C]) switches off, is left untouched.  No allocation, no synchronisation:
    the call can be captured in a HIP graph."""
    C_, k, m = _tails_state("tails_update", lo, hi, thr_lo, thr_hi, stage, count)
    x, xs = _moments_rows("tails_update", X, C_, m)
    _mask_arg("tails_update", mask, C_)
    check(lib.pxm_tails_update(_p(x), xs, _p(count), _p(lo), _p(hi), _p(thr_lo), _p(thr_hi), _p(stage), _p(mask), m, C_, k, int(nsamples),
                               _stream()))


def tails_quantiles(count, lo, hi, stage, nsamples, alpha):
    """Read-out of the tail heaps of :func:`tails_update` -> (q_lo, q_hi) float64 [C, m] on the device: numpy's linear
    quantiles at ``alpha / 2`` and ``1 - alpha / 2`` of every chain's samples (NaN for a chain without any).  Raises PxmError
    when the tails do not hold the order statistics ``alpha`` needs, or a chain saw more than ``nsamples`` saves."""
    C_, k, m = _tails_state("tails_quantiles", lo, hi, None, None, stage, count)
    q_lo = torch.empty((C_, m), dtype=_REAL, device=lo.device)
    q_hi = torch.empty_like(q_lo)
    check(lib.pxm_tails_quantiles(_p(count), _p(lo), _p(hi), _p(stage), m, C_, k, int(nsamples), float(alpha), _p(q_lo), _p(q_hi), _stream()))
    return q_lo, q_hi


def acov_stage_depth():
    """B: the saves ``acov_update`` keeps in its ring between two merges into ``acc`` and ``tot``; the ring has
    ``K - 1 + B`` rows"""
    return int(lib.pxm_acov_stage_depth())


def _acov_state(fn, acc, tot, head, ring, count):
    """argument checks of the autocovariance entry points -> (C, K, m)"""
    if not (isinstance(acc, torch.Tensor) and acc.dim() == 3):
        raise TypeError("%s: acc must be a float64 [C, K, m] device tensor" % fn)
    C_, K, m = acc.shape
    if K < 2 or K > 64 or K % 2:
        raise ValueError("%s: K must be even with 2 <= K <= 64, got %d" % (fn, K))
    B = acov_stage_depth()
    _dev_tensors(fn, "count int64 [C], acc / head contiguous float64 [C, K, m], tot contiguous float64 [C, m] and ring contiguous "
                 "float64 [C, K - 1 + %d, m] device tensors are expected" % B,
                 (count, torch.int64, (C_,)), (acc, _REAL, (C_, K, m)), (tot, _REAL, (C_, m)), (head, _REAL, (C_, K, m)),
                 (ring, _REAL, (C_, K - 1 + B, m)))
    if int(lib.pxm_acov_state_doubles(m, C_, K)) != acc.numel() or int(lib.pxm_acov_ring_doubles(m, C_, K)) != ring.numel():
        raise ValueError("%s: bad state shape [%d, %d, %d]" % (fn, C_, K, m))
    return C_, K, m


def acov_update(X, count, acc, tot, head, ring, mask=None):
    """One save into the lagged-product accumulators of the streaming effective sample size, in place:
    ``acc`` / ``head`` float64 [C, K, m], ``tot`` [C, m], ``ring`` [C, K - 1 + B, m] (:func:`acov_stage_depth`); ``X`` as for
    :func:`moments_update`.  ``count`` int64 [C] is the number of samples before this one and is not written: call this
    before the ``moments_update`` of the same sample.  A chain that ``mask`` (int32 [C]) switches off is left untouched.  The
    state needs no initialisation.  No allocation, no synchronisation: the call can be captured in a HIP graph."""
    C_, K, m = _acov_state("acov_update", acc, tot, head, ring, count)
    x, xs = _moments_rows("acov_update", X, C_, m)
    _mask_arg("acov_update", mask, C_)
    check(lib.pxm_acov_update(_p(x), xs, _p(count), _p(acc), _p(tot), _p(head), _p(ring), _p(mask), m, C_, K, _stream()))


def acov_ess(count, acc, tot, head, ring, pooled=True):
    """Read-out of the accumulators of :func:`acov_update` -> (ess float64 [C, m], ess_lag int32 [C, m], ess_pooled [m], mcse
    [m], stats [3]) on the device: the effective sample size of every chain and element by Geyer's initial monotone sequence
    over the K lags, the even lag at which the sequence stopped (``2 * (min(K, n) // 2)``: it never did, the estimate is
    truncated), the effective sample size pooled over the chains with samples and the Monte-Carlo standard error of their
    pooled mean, and stats = (min ESS over the non-NaN values, NaN count, truncated count) of ``ess``.  Nothing is written to
    the state.  ``pooled=False`` leaves ``ess_pooled`` and ``mcse`` out (None) and takes any counts; with them, chains with
    different counts raise PxmError."""
    C_, K, m = _acov_state("acov_ess", acc, tot, head, ring, count)
    ess = torch.empty((C_, m), dtype=_REAL, device=acc.device)
    lag = torch.empty((C_, m), dtype=torch.int32, device=acc.device)
    ep = se = None
    if pooled:
        ep = torch.empty(m, dtype=_REAL, device=acc.device)
        se = torch.empty_like(ep)
    st = torch.empty(3, dtype=_REAL, device=acc.device)
    scratch = torch.empty(int(lib.pxm_acov_scratch_doubles(m)), dtype=_REAL, device=acc.device)
    check(lib.pxm_acov_ess(_p(count), _p(acc), _p(tot), _p(head), _p(ring), m, C_, K, _p(ess), _p(lag), _p(ep), _p(se), _p(st),
                           _p(scratch), _stream()))
    return ess, lag, ep, se, st
