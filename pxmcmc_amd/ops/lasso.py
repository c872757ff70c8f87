"""The launch of the sparse posterior's Gibbs sampler (csrc/lasso.hip): the conditional draw of the
per-element prior precisions of the L1 prior given the field, and the per-chain diagonals the conjugate-gradient launches read."""
import numpy as np
import torch

from .._lib import FISTA_SLICES_MAX, check, lib
from ._args import _REAL, _batched, _chain_vector, _dt, _p, _scratch, _stream, _vecT, as_device


def lasso_scratch(C_, dev):
    """scratch of :func:`lasso_precision_draw` with ``sums`` for C_ chains: two partial sums per slice and chain"""
    return _scratch(None, 2 * FISTA_SLICES_MAX * int(C_), dev)


def _f64(t, shape, dev):
    return isinstance(t, torch.Tensor) and t.dtype == _REAL and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev


def lasso_precision_draw(X, T, D, sqrtD, Minv, tscale=1.0, h=0.0, d_lo=1e-30, d_hi=1e30, seed=0, chain0=0, it=0, sums=None,
                         scratch=None):
    """``D_i | x ~ IG(mean = t_i / |X_i|, shape = t_i^2)``, ``t_i = tscale T_i``, for every element of every chain, clamped to
    ``[d_lo, d_hi]``; then ``sqrtD`` and ``Minv = 1 / (D + h)``.  One launch (two with ``sums``), no host read.

    ``X``: ``[C, n]`` device array, float64 or complex128.  ``T``: a positive float, or a float64 ``[n]`` vector shared by the
    chains whose entries must all be positive (a device vector is not read here: the caller vouches for it).  ``D``, ``sqrtD``,
    ``Minv``: contiguous float64 ``[C, n]`` device arrays, written.  ``h``: float or float64 ``[C]`` device vector.  The normal
    of element i is the real part of element i of ``randn(n, C, complex_=True, noise64=True, seed=seed, chain0=chain0, it=it)``;
    the uniform is ``lasso_np.uniform_from_bits`` of the Philox block of the same key and index at iteration ``it + 1``: the
    call owns both iterations.  ``sums``: float64 ``[C, 2]`` device array or None, receives ``sum_i t_i |X_i|`` and the number
    of clamped elements.  ``scratch``: :func:`lasso_scratch` (with ``sums`` only).  Returns ``D``."""
    name = "lasso_precision_draw"
    x, _ = _batched(as_device(X))
    C_, n = x.shape
    dev = x.device
    if n < 1:
        raise ValueError(f"{name}: the state is empty")
    for nm, v in (("D", D), ("sqrtD", sqrtD), ("Minv", Minv)):
        if not _f64(v, (C_, n), dev):
            raise ValueError(f"{name}: {nm} must be a contiguous float64 [C, n] device array")
    if not (np.isfinite(tscale) and tscale > 0):
        raise ValueError(f"{name}: tscale must be finite and positive")
    if not isinstance(T, torch.Tensor) and not (np.all(np.isfinite(T)) and np.all(np.asarray(T) > 0)):
        raise ValueError(f"{name}: every threshold T_i must be finite and positive")
    Tv, Ts = _vecT(T, n, dev)
    if Tv is None and not (np.isfinite(Ts) and Ts > 0):
        raise ValueError(f"{name}: every threshold T_i must be finite and positive")
    if not (np.isfinite(d_lo) and np.isfinite(d_hi) and 0 < d_lo <= d_hi):
        raise ValueError(f"{name}: the clamp needs finite 0 < d_lo <= d_hi")
    if isinstance(h, torch.Tensor):
        hv, hs = _chain_vector(h, C_, dev, (_REAL,), f"{name}: h must be a float or a contiguous float64 [C] device vector"), 0.0
    else:
        hv, hs = None, float(h)
    if sums is not None:
        if not _f64(sums, (C_, 2), dev):
            raise ValueError(f"{name}: sums must be a contiguous float64 [C, 2] device array")
        scratch = _scratch(scratch, 2 * FISTA_SLICES_MAX * C_, dev, f"{name}: scratch is too small (lasso_scratch)")
    else:
        scratch = None
    check(lib.pxm_lasso_precision_draw(_p(x), _p(Tv), Ts, float(tscale), _p(hv), hs, float(d_lo), float(d_hi), int(seed), int(chain0),
                                       int(it), _p(D), _p(sqrtD), _p(Minv), _p(sums), _p(scratch), n, C_, _dt(x), _stream()))
    return D
