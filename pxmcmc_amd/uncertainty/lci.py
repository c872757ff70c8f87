"""
Local credible intervals: :func:`local_credible_intervals` turns the MAP point and the level of
:func:`~pxmcmc_amd.uncertainty.chains.approx_credible_region_threshold` into an error bar per region of the image
(:func:`~pxmcmc_amd.uncertainty.regions.superpixel_regions`), searched on the device; :func:`lci_terms_np`,
:func:`lci_eval_np` and :func:`lci_search_np` state its sums and its search in numpy.
"""
import numpy as np
import torch

from .. import ops
from .._lib import LCI_EMPTY, LCI_NONFINITE, LCI_POINTS, LCI_UNCONSTRAINED
from .regions import _check_scope, _lci_preds, _PathSearch, _RegionResult, _regions_setup

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


class LocalCredibleIntervals(_RegionResult):
    """the result of :func:`local_credible_intervals`: one entry per region of ``lower``, ``upper``, ``range`` (= upper -
    lower), ``map_value``, ``width`` (the larger of the two final bracket widths: each end is known to that), ``f_min``,
    ``xi_min``, ``status`` (numpy arrays ``[nregions]``), ``outer`` (``[nregions, 2]``: the outer bracket the search started
    from, so ``width <= lci_shrink_factor(rounds) * (outer[:, 1] - outer[:, 0])``), the ``threshold`` used and the ``labels``;
    ``to_map()`` paints ``range``"""

    FIELDS = ("lower", "upper", "range", "map_value", "width", "f_min", "xi_min", "status", "outer")
    PAINTED = "range"


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
    _check_scope("local_credible_intervals", forward, prior)
    tr, X, x_map, labels, nreg, counts, batch = _regions_setup("local_credible_intervals", forward, X_map, regions, batch, rounds)
    cplx_state = torch.complex128
    dev = X.device
    lab = torch.from_numpy(labels.reshape(-1).astype(np.int64)).to(dev)
    search = _PathSearch(forward, prior, params, X, nreg, batch, threshold, alpha, rounds)
    ids = torch.arange(batch, device=dev)
    for r0 in range(0, nreg, batch):
        Cb = min(batch, nreg - r0)
        zeta = (lab[None, :] == (r0 + ids[:Cb, None])).to(cplx_state)
        b = ops.as_device(tr.forward(zeta), cplx_state)
        a = X[None] - ops.as_device(tr.forward(zeta * x_map[None]), cplx_state)
        pa, d = _lci_preds(forward, a)
        pb, _ = _lci_preds(forward, b)
        search.run(r0, a, b, pa, pb, d)
    # read back with the results: the MAP image for the plain mean over every region (summed on the host in pixel order: a
    # device scatter-add would add in an order that changes from call to call)
    res, (img,) = search.read_back(x_map.real.to(torch.float64))
    on = labels.reshape(-1) >= 0
    means = np.bincount(labels.reshape(-1)[on], weights=img[on], minlength=nreg) / counts
    with np.errstate(invalid="ignore"):
        rng = res["upper"] - res["lower"]
    return LocalCredibleIntervals(labels, res.pop("threshold"), range=rng, map_value=means, **res)

