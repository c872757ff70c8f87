"""The launch of the Gibbs sampler's variance draw (csrc/gibbs.hip): the conditional of the prior
precisions of K contiguous groups given the field, and the per-chain diagonals the conjugate-gradient launches read."""
import numpy as np
import torch

from .. import gibbs_np
from .._lib import GIBBS_SLICE, check, lib
from ._args import _REAL, _batched, _chain_vector, _dt, _p, _scratch, _stream, as_device, device


class GibbsGroups:
    """The groups of a variance draw on the device: the offsets ``bounds`` (K + 1 integers increasing strictly from 0 to n),
    the table that cuts every group into slices of ``GIBBS_SLICE`` elements, one workgroup each, and the mask of the groups
    that keep their precision (``fixed``: group indices).  Built once; the launches read it in place."""

    def __init__(self, bounds, n, fixed=()):
        self.n = int(n)
        self.bounds = gibbs_np.group_bounds(bounds, self.n, "GibbsGroups")
        self.K = self.bounds.size - 1
        fx = np.zeros(self.K, dtype=np.int32)
        idx = np.asarray(list(fixed), dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self.K):
            raise ValueError(f"GibbsGroups: fixed holds group indices 0 <= k < {self.K}")
        fx[idx] = 1
        self.fixed = fx.astype(bool)
        tab, g0 = gibbs_np.slice_table(self.bounds, GIBBS_SLICE)
        self.nslices = int(g0[-1])
        dev = device()
        self.bounds_dev = torch.from_numpy(self.bounds).to(dev)
        self.slice_tab_dev = torch.from_numpy(tab).to(dev).contiguous()
        self.group_slice0_dev = torch.from_numpy(g0).to(dev)
        self.fixed_dev = torch.from_numpy(fx).to(dev)

    def scratch(self, C_):
        """scratch of :func:`group_variance_draw` for C_ chains: two partial sums per slice and chain"""
        return torch.empty(2 * self.nslices * int(C_), dtype=_REAL, device=self.bounds_dev.device)


def _f64(t, shape, dev):
    return isinstance(t, torch.Tensor) and t.dtype == _REAL and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev


def group_variance_draw(X, groups, Dg, D, sqrtD, Minv, q=0.0, h=0.0, d_lo=1e-30, d_hi=1e30, seed=0, chain0=0, it=0, sums=None,
                        trace=None, trace_row=0, scratch=None, expand_only=False):
    """``D_k | x = chi2_nu / sigma_k`` for every chain and every group of ``groups`` (:class:`GibbsGroups`) that is not fixed,
    ``sigma_k = sum_{i in k} |X_i|^2`` and ``nu_k = dof n_k + 2 q - 2``, clamped to ``[d_lo, d_hi]`` (``sigma_k = 0``:
    ``d_hi``); then ``D``, ``sqrtD`` and ``Minv = 1 / (D + h)`` of every element.  At most three launches, no host read.

    ``X``: ``[C, n]`` device array (None with ``expand_only``).  ``Dg``: contiguous float64 ``[C, K]`` device array, updated in
    place.  ``D``, ``sqrtD``, ``Minv``: contiguous float64 ``[C, n]`` device arrays, written.  ``h``: float or float64 ``[C]``
    device vector.  Deviate ``t`` of group k is component ``t & 1`` of element ``b_k + k + (t >> 1)`` of ``randn(n + K + 1, C,
    complex_=True, noise64=True, seed=seed, chain0=chain0, it=it)``.  ``sums``: float64 ``[C, K, 2]`` device array or None,
    receives ``(sigma_k, chi2_k)`` of the sampled groups.  ``trace``: float64 ``[n_trace, C, K]`` device array or None; row
    ``trace_row`` receives ``Dg`` after the draw.  ``expand_only``: only the last launch, from ``Dg`` as given.
    Returns ``Dg``."""
    name = "group_variance_draw"
    if not isinstance(groups, GibbsGroups):
        raise TypeError(f"{name}: groups must be a GibbsGroups")
    dev = groups.bounds_dev.device
    n, K = groups.n, groups.K
    if not (isinstance(Dg, torch.Tensor) and Dg.dim() == 2 and _f64(Dg, (Dg.shape[0], K), dev)):
        raise ValueError(f"{name}: Dg must be a contiguous float64 [C, K] device array")
    C_ = Dg.shape[0]
    if expand_only:
        x, dt = None, 0
    else:
        x, _ = _batched(as_device(X))
        if tuple(x.shape) != (C_, n):
            raise ValueError(f"{name}: X must be [C, n] = [{C_}, {n}]")
        dt = _dt(x)
    for nm, v in (("D", D), ("sqrtD", sqrtD), ("Minv", Minv)):
        if not _f64(v, (C_, n), dev):
            raise ValueError(f"{name}: {nm} must be a contiguous float64 [C, n] device array")
    two_q = gibbs_np.check_q(q, name)
    if not (np.isfinite(d_lo) and np.isfinite(d_hi) and 0 < d_lo <= d_hi):
        raise ValueError(f"{name}: the clamp needs finite 0 < d_lo <= d_hi")
    if isinstance(h, torch.Tensor):
        hv, hs = _chain_vector(h, C_, dev, (_REAL,), f"{name}: h must be a float or a contiguous float64 [C] device vector"), 0.0
    else:
        hv, hs = None, float(h)
    if sums is not None and not _f64(sums, (C_, K, 2), dev):
        raise ValueError(f"{name}: sums must be a contiguous float64 [C, K, 2] device array")
    n_trace = 0
    if trace is not None:
        if not (isinstance(trace, torch.Tensor) and trace.dim() == 3 and _f64(trace, (trace.shape[0], C_, K), dev)):
            raise ValueError(f"{name}: trace must be a contiguous float64 [n_trace, C, K] device array")
        n_trace = trace.shape[0]
    if int(trace_row) < 0:
        raise ValueError(f"{name}: trace_row must not be negative")
    scratch = _scratch(scratch, 2 * groups.nslices * C_, dev, f"{name}: scratch is too small (GibbsGroups.scratch)")
    check(lib.pxm_group_variance_draw(
        _p(x), _p(groups.bounds_dev), K, _p(groups.slice_tab_dev), _p(groups.group_slice0_dev), groups.nslices,
        _p(groups.fixed_dev), two_q, _p(hv), hs, float(d_lo), float(d_hi), int(seed), int(chain0), int(it), _p(Dg), _p(sums),
        _p(trace if n_trace else None), n_trace, int(trace_row), _p(D), _p(sqrtD), _p(Minv), _p(scratch), n, C_, dt,
        int(bool(expand_only)), _stream()))
    return Dg
