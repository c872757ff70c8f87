"""Total variation on the MW grid (csrc/tv.hip): the discrete gradient and its adjoint, the TV value,
the pair form of the primal-dual dual step and the two fused steps.  Images are ``[C, L n]`` (or ``[L n]``), ``n = 2L - 1``;
coefficients are plane-major per chain, ``[C, 2 L n]`` (or ``[2 L n]``)."""
import torch

from .._lib import FISTA_SLICES_MAX, check, lib
from ..tv_np import tv_ring_coefs_np
from ._args import _REAL, _batched, _companion, _dev_tensors, _dt, _p, _result, _scratch, _state_out, _stream, _vecT, as_device
from .host import mw_ring_weights


def tv_ring_coefs(L):
    """the device table ``ab`` of the kernels, float64 ``[2, L]``: ``a_t = q_t / D``, ``b_t = q_t / (D sin theta_t)`` for
    ``t < L - 1`` and zeros on the last ring, ``q = mw_ring_weights(L)``, ``D = 2 pi / (2L - 1)``"""
    L = int(L)
    if L < 2:
        raise ValueError("tv_ring_coefs: L >= 2")
    return as_device(tv_ring_coefs_np(mw_ring_weights(L), L), _REAL)


def _table_L(ab, name):
    """the bandlimit a table was made for, the table checked"""
    if not isinstance(ab, torch.Tensor) or ab.dim() != 2 or ab.shape[0] != 2:
        raise TypeError(f"{name}: ab must be the float64 [2, L] device table of tv_ring_coefs")
    L = int(ab.shape[1])
    _dev_tensors(name, "ab must be the float64 [2, L] device table of tv_ring_coefs", (ab, _REAL, (2, L)))
    if L < 2:
        raise ValueError(f"{name}: L >= 2")
    return L


def _image(X, L, name):
    x, squeeze = _batched(as_device(X))
    if x.shape[1] != L * (2 * L - 1):
        raise ValueError(f"{name}: the image must have L (2L - 1) = {L * (2 * L - 1)} samples, got {x.shape[1]}")
    return x, squeeze


def _coefs(V, L, name):
    v, squeeze = _batched(as_device(V))
    if v.shape[1] != 2 * L * (2 * L - 1):
        raise ValueError(f"{name}: the coefficients must have 2 planes of L (2L - 1) samples ({2 * L * (2 * L - 1)}), got {v.shape[1]}")
    return v, squeeze


def _coefs_of(V, x, msg):
    """the two-plane coefficients that go with the image batch ``x``: [C, 2 L n] in x's dtype"""
    v, _ = _batched(as_device(V, x.dtype))
    if v.shape != (x.shape[0], 2 * x.shape[1]):
        raise ValueError(msg)
    return v


def _out(out, shape, like):
    if out is None:
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    return _result(out if out.dim() == 2 else out.unsqueeze(0), shape, like.dtype, like.device,
                   "out must be a contiguous device array of the result's shape and dtype", on_device=True)


def _pixel_T(T, m, dev, name):
    if T is None:
        raise ValueError(f"{name}: the threshold T is needed")
    try:
        return _vecT(T, m, dev)
    except ValueError:
        raise ValueError(f"{name}: T is a scalar or one value per pixel ({m})") from None


def tv_grad(X, ab, out=None):
    """``A X``: ``[C, L n] -> [C, 2 L n]`` (plane 0: along theta, plane 1: along phi)"""
    L = _table_L(ab, "tv_grad")
    x, squeeze = _image(X, L, "tv_grad")
    o = _out(out, (x.shape[0], 2 * x.shape[1]), x)
    check(lib.pxm_tv_grad(_p(x), _p(ab), _p(o), L, x.shape[0], _dt(x), _stream()))
    return o[0] if squeeze else o


def tv_grad_adjoint(V, ab, out=None):
    """``A^H V``: ``[C, 2 L n] -> [C, L n]``"""
    L = _table_L(ab, "tv_grad_adjoint")
    v, squeeze = _coefs(V, L, "tv_grad_adjoint")
    o = _out(out, (v.shape[0], v.shape[1] // 2), v)
    check(lib.pxm_tv_grad_adjoint(_p(v), _p(ab), _p(o), L, v.shape[0], _dt(v), _stream()))
    return o[0] if squeeze else o


def tv_value(X, ab, T, out=None, scratch=None):
    """``sum_i T_i ||(A X)_i||`` per chain, straight from the image (T: scalar or ``[L n]``) -> float64 ``[C]``"""
    L = _table_L(ab, "tv_value")
    x, _ = _image(X, L, "tv_value")
    Tv, Ts = _pixel_T(T, x.shape[1], x.device, "tv_value")
    C_ = x.shape[0]
    out = _result(out, (C_,), _REAL, x.device, "tv_value: out must be a contiguous float64 [C] device array")
    scratch = _scratch(scratch, FISTA_SLICES_MAX * C_, x.device, "tv_value: scratch is too small", any_layout=True)
    check(lib.pxm_tv_value(_p(x), _p(ab), _p(Tv), Ts, _p(out), _p(scratch), L, C_, _dt(x), _stream()))
    return out


def pd_dual_step_pairs(V, W, T, sigma, rscale, out=None, sums=None, scratch=None):
    """:func:`pd_dual_step` on two-plane coefficients ``[C, 2 m]``: ``V + sigma W`` projected pixel by pixel onto
    ``||v_i|| <= T_i rscale``, the norm taken over the pixel's pair (isotropic total variation).  ``T``: scalar or ``[m]``.
    Returns ``(V1, sums)`` with ``sums`` float64 [C, 3]: ``sum |V1 - V|^2``, ``sum |V1|^2`` and ``sum T_i ||W_i||``.
    ``scratch``: :func:`pd_scratch`."""
    name = "pd_dual_step_pairs"
    v, squeeze = _batched(as_device(V))
    w = _companion(W, v, f"{name}: W must have the shape of V")
    if v.shape[1] % 2:
        raise ValueError(f"{name}: the coefficients have two planes of equal length")
    m = v.shape[1] // 2
    Tv, Ts = _pixel_T(T, m, v.device, name)
    C_ = v.shape[0]
    v1 = torch.empty_like(v) if out is None else _state_out(out, v)
    sums = _result(sums, (C_, 3), _REAL, v.device, f"{name}: sums must be a contiguous float64 [C, 3] device array")
    scratch = _scratch(scratch, 3 * FISTA_SLICES_MAX * C_, v.device, f"{name}: scratch is too small", any_layout=True)
    check(lib.pxm_pd_dual_step_pairs(_p(v), _p(w), _p(Tv), Ts, float(sigma), float(rscale), _p(v1), _p(sums), _p(scratch), m, C_,
                                     _dt(v), _stream()))
    return (v1[0], sums) if squeeze else (v1, sums)


def tv_primal_step(X, G, V, ab, tau, out=None, xbar=True, sums=None, scratch=None):
    """:func:`pd_primal_step` with ``U = A^H V`` formed in the kernel: ``X1 = X - tau (G + A^H V)``, ``Xbar = 2 X1 - X``.
    ``G`` may be None (zero).  ``out``: ``(X1, Xbar)``, or ``X1`` alone with ``xbar=False`` (Xbar is then not written and None
    is returned in its place).  Returns ``(X1, Xbar, sums)``, ``sums`` float64 [C, 2] as :func:`pd_primal_step`."""
    name = "tv_primal_step"
    L = _table_L(ab, name)
    x, squeeze = _image(X, L, name)
    g = None if G is None else _companion(G, x, f"{name}: G must have the state's shape")
    v = _coefs_of(V, x, f"{name}: V must be [C, 2 L n] in the state's dtype")
    o1, ob = (out if xbar else (out, None)) if out is not None else (None, None)
    x1 = torch.empty_like(x) if o1 is None else _state_out(o1, x)
    xb = None if not xbar else (torch.empty_like(x) if ob is None else _state_out(ob, x))
    C_ = x.shape[0]
    sums = _result(sums, (C_, 2), _REAL, x.device, f"{name}: sums must be a contiguous float64 [C, 2] device array")
    scratch = _scratch(scratch, 2 * FISTA_SLICES_MAX * C_, x.device, f"{name}: scratch is too small", any_layout=True)
    check(lib.pxm_tv_primal_step(_p(x), _p(g), _p(v), _p(ab), float(tau), _p(x1), _p(xb), _p(sums), _p(scratch), L, C_, _dt(x),
                                 _stream()))
    if squeeze:
        return x1[0], (None if xb is None else xb[0]), sums
    return x1, xb, sums


def tv_dual_step(V, Xbar, ab, T, sigma, rscale, out=None, sums=None, scratch=None):
    """:func:`pd_dual_step_pairs` with ``W = A Xbar`` formed in the kernel.  Returns ``(V1, sums)``."""
    name = "tv_dual_step"
    L = _table_L(ab, name)
    xb, squeeze = _image(Xbar, L, name)
    v = _coefs_of(V, xb, f"{name}: V must be [C, 2 L n] in the state's dtype")
    Tv, Ts = _pixel_T(T, xb.shape[1], xb.device, name)
    C_ = xb.shape[0]
    v1 = torch.empty_like(v) if out is None else _state_out(out, v)
    sums = _result(sums, (C_, 3), _REAL, v.device, f"{name}: sums must be a contiguous float64 [C, 3] device array")
    scratch = _scratch(scratch, 3 * FISTA_SLICES_MAX * C_, v.device, f"{name}: scratch is too small", any_layout=True)
    check(lib.pxm_tv_dual_step(_p(v), _p(xb), _p(ab), _p(Tv), Ts, float(sigma), float(rscale), _p(v1), _p(sums), _p(scratch), L, C_,
                               _dt(v), _stream()))
    return (v1[0], sums) if squeeze else (v1, sums)
