"""
The numpy statements of total variation on the MW grid, beside :mod:`pxmcmc_amd.optim_np`: the
discrete gradient ``A`` and its adjoint, the isotropic TV value, the pair form of the dual projection, and the pair variants
of the primal-dual iteration, the exact analysis prox and the duality gap.  No torch; every function keeps the dtype of its
arguments, so the statements run in long double as well.

Images are spin-0 MW maps ``[..., L n]``, ``n = 2L - 1``; coefficients are plane-major along the last axis, ``[..., 2 L n]``
(plane 0, the differences along theta, then plane 1, those along phi), as the device arrays ``[C][2][L n]`` are.  Ring t is at ``theta_t = pi (2t + 1) / n``, sample p at ``phi_p = 2 pi p / n``.
With ``D = 2 pi / n`` and the ring weights ``q_t``::

    a_t = q_t / D,   b_t = q_t / (D sin theta_t)   for t < L - 1,      a_{L-1} = b_{L-1} = 0
    (A x)[0][t][p] = a_t (x[t+1][p] - x[t][p])
    (A x)[1][t][p] = b_t (x[t][(p+1) mod n] - x[t][p])
    (A^H v)[t][p]  = a_{t-1} v0[t-1][p] - a_t v0[t][p] + b_t (v1[t][(p-1) mod n] - v1[t][p]),   a_{-1} = 0
    TV(x) = sum_{t,p} T_{t,p} sqrt(|(A x)[0][t][p]|^2 + |(A x)[1][t][p]|^2)   ~   T int |grad x| dOmega
"""
import numpy as np

from .optim_np import pd_primal_np


def tv_ring_coefs_np(q, L):
    """the table ``[2, L]`` of ``(a_t, b_t)`` from the ring weights ``q`` (``ops.mw_ring_weights(L)``, or the first entry of
    every ring of ``oracle.pxmcmc_np.mw_map_weights``), in the dtype of ``q``"""
    q = np.asarray(q)
    L = int(L)
    if L < 2 or q.shape != (L,):
        raise ValueError("tv_ring_coefs_np: L >= 2 and one weight per ring")
    n = 2 * L - 1
    dt = q.dtype.type
    pi = np.arccos(dt(-1))
    delta = 2 * pi / n
    theta = pi * (2 * np.arange(L).astype(q.dtype) + 1) / n
    ab = np.zeros((2, L), dtype=q.dtype)
    ab[0, : L - 1] = q[: L - 1] / delta
    ab[1, : L - 1] = q[: L - 1] / (delta * np.sin(theta[: L - 1]))
    return ab


def _image(x, L):
    n = 2 * L - 1
    x = np.asarray(x)
    if x.shape[-1] != L * n:
        raise ValueError("tv: the image has L (2L - 1) samples")
    return x.reshape(x.shape[:-1] + (L, n)), n


def tv_grad_np(x, ab, L):
    """``A x``: ``[..., L n] -> [..., 2 L n]``"""
    im, n = _image(x, L)
    ab = np.asarray(ab)
    out = np.zeros(im.shape[:-2] + (2, L, n), dtype=np.result_type(im.dtype, ab.dtype))
    out[..., 0, : L - 1, :] = ab[0, : L - 1, None] * (im[..., 1:, :] - im[..., : L - 1, :])
    out[..., 1, :, :] = ab[1, :, None] * (np.roll(im, -1, axis=-1) - im)
    return out.reshape(out.shape[:-3] + (2 * L * n,))


def tv_grad_adjoint_np(v, ab, L):
    """``A^H v``: ``[..., 2 L n] -> [..., L n]``"""
    n = 2 * L - 1
    v = np.asarray(v)
    if v.shape[-1] != 2 * L * n:
        raise ValueError("tv: the coefficients have 2 planes of L (2L - 1) samples")
    ab = np.asarray(ab)
    v = v.reshape(v.shape[:-1] + (2, L, n))
    v0, v1 = v[..., 0, :, :], v[..., 1, :, :]
    av0 = ab[0, :, None] * v0
    out = ab[1, :, None] * (np.roll(v1, 1, axis=-1) - v1) - av0
    out[..., 1:, :] = out[..., 1:, :] + av0[..., : L - 1, :]
    return out.reshape(out.shape[:-2] + (L * n,))


def _pairs(u):
    """``[..., 2 m]`` -> ``[..., 2, m]``"""
    u = np.asarray(u)
    if u.shape[-1] % 2:
        raise ValueError("pairs: the coefficients have two planes of equal length")
    return u.reshape(u.shape[:-1] + (2, u.shape[-1] // 2))


def pair_norm_np(u):
    """the norm over the two planes (and the real and imaginary parts) of every pixel: ``[..., 2 m] -> [..., m]``"""
    u = _pairs(u)
    return np.sqrt((u.real ** 2 + u.imag ** 2).sum(axis=-2))


def tv_value_np(x, ab, L, T=1.0):
    """``sum_i T_i ||(A x)_i||`` over the last axis (T a scalar or ``[L n]``)"""
    return (np.asarray(T) * pair_norm_np(tv_grad_np(x, ab, L))).sum(axis=-1)


def pd_dual_pairs_np(v, w, T, sigma, rscale):
    """``v + sigma w`` (``[..., 2 m]``) projected pixel by pixel onto
    ``||y_i|| <= r_i = T_i rscale``, the norm taken over the pair, as the kernel does it: a pair outside its ball is scaled by
    ``r_i / ||y_i||`` (one division); ``||y_i|| = r_i`` and 0 are kept, ``T_i = 0`` gives 0 and ``r_i = inf`` never binds."""
    y = np.asarray(v + sigma * np.asarray(w))
    y2 = _pairs(y)
    a = pair_norm_np(y)
    r = np.broadcast_to(np.asarray(T) * rscale, a.shape)
    big = a > r
    s = np.ones(a.shape, dtype=a.dtype)
    s[big] = r[big] / a[big]
    out = np.where(big[..., None, :], y2 * s[..., None, :], y2)
    return out.reshape(y.shape)


def primal_dual_pairs_np(grad, A, AH, T, lmda, tau, sigma, x0, iters, v0=None, tol=None):
    """:func:`pxmcmc_amd.optim_np.primal_dual_np` with the pair projection: ``h(u) = (1 / lmda) sum_i T_i ||u_i||``"""
    x = np.array(x0)
    v = np.zeros_like(A(x)) if v0 is None else np.array(v0)
    info = dict(niter=0, dx=np.inf, dv=np.inf, converged=False)
    for k in range(int(iters)):
        x1, xbar = pd_primal_np(x, grad(x), AH(v), tau)
        v1 = pd_dual_pairs_np(v, A(xbar), T, sigma, 1.0 / lmda)
        dx, dv = np.linalg.norm(x1 - x), np.linalg.norm(v1 - v)
        x, v = x1, v1
        info.update(niter=k + 1, dx=dx, dv=dv)
        if tol is not None and dx <= tol * np.linalg.norm(x) and dv <= tol * np.linalg.norm(v):
            info["converged"] = True
            break
    return x, v, info


def analysis_prox_pairs_np(A, AH, T, Z, iters, sigma, return_dual=False):
    """:func:`pxmcmc_amd.optim_np.analysis_prox_np` with the pair projection: the prox of ``p -> sum_i T_i ||(A p)_i||``"""
    Z = np.asarray(Z)
    v = np.zeros_like(A(Z))
    for _ in range(int(iters)):
        v = pd_dual_pairs_np(v, A(Z - AH(v)), T, sigma, 1.0)
    p = Z - AH(v)
    return (p, v) if return_dual else p


def duality_gap_pairs_np(x, v, d, ic, A, AH, T, lmda):
    """:func:`pxmcmc_amd.optim_np.duality_gap_np` for ``h(u) = (1 / lmda) sum_i T_i ||u_i||``: the dual feasible set is
    ``||v_i|| <= T_i / lmda``, onto which ``v`` is projected first"""
    v = pd_dual_pairs_np(np.zeros_like(v), v, T, 1.0, 1.0 / lmda)
    ic = np.asarray(ic, dtype=float)
    primal = 0.5 * np.sum(ic * np.abs(x - d) ** 2) + np.sum(np.asarray(T, dtype=float) * pair_norm_np(A(x))) / lmda
    y = AH(v)
    dual = np.sum((np.conj(y) * d).real) - 0.5 * np.sum(np.abs(y) ** 2 / ic)
    return float(primal - dual)
