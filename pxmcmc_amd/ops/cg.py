"""The launches of the Gaussian posterior (csrc/cg.hip): the two steps of a preconditioned conjugate-gradient iteration, the
prox of the Gaussian prior and the helper that assembles right-hand sides."""
import torch

from .._lib import CG_COEF, FISTA_SLICES_MAX, check, lib
from ._args import _REAL, _batched, _companion, _dt, _p, _result, _scratch, _state_out, _stream, _vecT, as_device

# a chain's row of the coefficient array (include/pxmcmc_amd.h)
CG_ALPHA, CG_BETA, CG_GAMMA_OLD, CG_ALPHA_OLD, CG_RHO, CG_BNORM2, CG_FLAGS, CG_ITERS = range(CG_COEF)


def cg_scratch(C_, dev):
    """scratch of :func:`cg_apply` for C_ chains: three partial sums per slice and chain"""
    return _scratch(None, 3 * FISTA_SLICES_MAX * int(C_), dev)


def cg_coef(bnorm2, dev=None):
    """the coefficient array ``[C, CG_COEF]`` at the start of a solve: zero but for ``||b||^2`` (``[C]`` values)"""
    b = bnorm2 if isinstance(bnorm2, torch.Tensor) else as_device(bnorm2, _REAL)
    b = b.to(dtype=_REAL).reshape(-1)
    coef = torch.zeros((b.numel(), CG_COEF), dtype=_REAL, device=b.device if dev is None else dev)
    coef[:, CG_BNORM2] = b
    return coef


def _coef(coef, C_, dev, name):
    if (not isinstance(coef, torch.Tensor) or coef.dtype != _REAL or tuple(coef.shape) != (C_, CG_COEF) or not coef.is_contiguous()
            or coef.device != dev):
        raise ValueError(f"{name}: coef must be a contiguous float64 [C, {CG_COEF}] device array (cg_coef)")
    return coef


def _shared(b, x, msg):
    """a vector shared by the chains in the state's dtype ([n]), or None"""
    if b is None:
        return None
    t = as_device(b, x.dtype).reshape(-1)
    if t.numel() != x.shape[1]:
        raise ValueError(msg)
    return t


def _diag(v, C_, n, dev, name):
    """a diagonal of the launches -> (vector or None, scalar, chain stride): a float, an ``[n]`` vector shared by the chains
    (stride 0), or one row per chain, which the kernels read in place: a contiguous float64 ``[C, n]`` device array (stride n)"""
    if isinstance(v, torch.Tensor) and v.dim() == 2:
        rows = tuple(v.shape) == (C_, n) and v.dtype == _REAL and v.is_contiguous() and v.device == dev
        if rows:
            return v, 0.0, n
        if v.shape[0] != 1:
            raise ValueError(f"{name}: a per-chain diagonal must be a contiguous float64 [C, n] device array")
    return (*_vecT(v, n, dev), 0)  # (any other [1, n] array is the shared vector, as before)


def _state_inplace(t, x, msg):
    """an array the launch updates in place: the caller's contiguous device array of the state's shape and dtype"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(msg)
    t2 = t if t.dim() == 2 else t.unsqueeze(0)
    if t2.shape != x.shape or t2.dtype != x.dtype or not t2.is_contiguous() or t2.device != x.device:
        raise ValueError(msg)
    return t2


def cg_apply(U, Q, B0, D, R, coef, tol, out=None, scratch=None):
    """The first launch of a CG iteration: ``W = D u + (q + b0)`` and, per chain, the three sums
    ``gamma = sum Re conj(r) u``, ``delta = sum Re conj(u) w``, ``rho = sum |r|^2``, from which the device sets the chain's
    ``alpha`` and ``beta`` in ``coef``, freezes it when ``rho <= tol^2 ||b||^2`` and flags a breakdown.

    ``B0``: ``[n]`` shared by the chains, or None; ``D``: float, ``[n]``, or one row per chain (a contiguous float64 ``[C, n]``
    device array, read in place); ``coef``: :func:`cg_coef`, updated in place.
    ``out``: the buffer of ``W`` (must not alias an input).  Returns ``(W, coef)``.  ``scratch``: :func:`cg_scratch`."""
    name = "cg_apply"
    u, squeeze = _batched(as_device(U))
    q, r = (_companion(t, u, f"{name}: Q and R must have the shape of U") for t in (Q, R))
    b0 = _shared(B0, u, f"{name}: B0 must have one entry per element of a chain")
    C_ = u.shape[0]
    Dv, Ds, Dst = _diag(D, C_, u.shape[1], u.device, name)
    coef = _coef(coef, C_, u.device, name)
    w = torch.empty_like(u) if out is None else _state_out(out, u)
    scratch = _scratch(scratch, 3 * FISTA_SLICES_MAX * C_, u.device, f"{name}: scratch is too small", any_layout=True)
    check(lib.pxm_cg_apply(_p(u), _p(q), _p(b0), _p(Dv), Ds, Dst, _p(r), _p(w), _p(coef), float(tol), _p(scratch), u.shape[1], C_,
                           _dt(u), _stream()))
    return (w[0] if squeeze else w), coef


def cg_update(U, W, P, S, X, R, Minv, coef, out=None):
    """The second launch of a CG iteration: ``p = u + beta p``, ``s = w + beta s``, ``x1 = x + alpha p``, ``r -= alpha s``,
    ``u = Minv r`` with the chain's ``alpha``, ``beta`` of ``coef``.  ``U``, ``P``, ``S`` and ``R`` are device arrays updated
    in place; ``out``: the buffer of ``x1``.  A frozen chain is copied ``X -> x1`` and otherwise left as it is.  ``Minv``:
    float, ``[n]`` or ``[C, n]`` (as ``D`` of :func:`cg_apply`).  Returns ``x1``."""
    name = "cg_update"
    x, squeeze = _batched(as_device(X))
    w = _companion(W, x, f"{name}: W must have the state's shape")
    u, p, s, r = (_state_inplace(t, x, f"{name}: U, P, S and R must be contiguous device arrays of the state's shape and dtype")
                  for t in (U, P, S, R))
    Mv, Ms, Mst = _diag(Minv, x.shape[0], x.shape[1], x.device, name)
    coef = _coef(coef, x.shape[0], x.device, name)
    x1 = torch.empty_like(x) if out is None else _state_out(out, x)
    check(lib.pxm_cg_update(_p(u), _p(w), _p(p), _p(s), _p(x), _p(x1), _p(r), _p(Mv), Ms, Mst, _p(coef), x.shape[1], x.shape[0], _dt(x),
                            _stream()))
    return x1[0] if squeeze else x1


def gauss_prox(X, precision, T, out=None):
    """``X / (1 + T p)``: the prox of ``T 1/2 sum_i p_i |x_i|^2`` in one launch (``precision``: float or ``[n]``)"""
    x, squeeze = _batched(as_device(X))
    Pv, Ps = _vecT(precision, x.shape[1], x.device)
    o = torch.empty_like(x) if out is None else _state_out(out, x)
    check(lib.pxm_gauss_prox(_p(x), _p(Pv), Ps, float(T), _p(o), x.shape[1], x.shape[0], _dt(x), _stream()))
    return o[0] if squeeze else o


def cg_rhs(like, B=None, G=None, g_scale=1.0, Z=None, S=1.0, z_scale=1.0, out=None):
    """``B + g_scale G + z_scale (S o Z)`` in one launch, shaped and typed like the ``[C, n]`` device array ``like``: ``B``
    ``[n]`` is shared by the chains, ``G`` and ``Z`` are ``[C, n]``, ``S`` is a float, ``[n]`` or one row per chain ``[C, n]``; a
    term that is None is left out.  The right-hand sides of the Gaussian posterior's draws, ``H x`` for a start point, ``M^-1 r``."""
    x, squeeze = _batched(like)
    b = _shared(B, x, "cg_rhs: B must have one entry per element of a chain")
    g, z = (t if t is None else _companion(t, x, "cg_rhs: G and Z must have the shape of the result") for t in (G, Z))
    Sv, Ss, Sst = _diag(S, x.shape[0], x.shape[1], x.device, "cg_rhs")
    o = _result(out if out is None or out.dim() == 2 else out.unsqueeze(0), tuple(x.shape), x.dtype, x.device,
                "cg_rhs: out must be a contiguous device array of the result's shape and dtype", on_device=True)
    check(lib.pxm_cg_rhs(_p(b), _p(g), float(g_scale), _p(z), _p(Sv), Ss, Sst, float(z_scale), _p(o), x.shape[1], x.shape[0], _dt(x),
                         _stream()))
    return o[0] if squeeze else o
