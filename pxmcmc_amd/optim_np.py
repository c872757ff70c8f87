"""
The numpy statements of the analysis-setting solvers of :mod:`pxmcmc_amd.optim`: what the two
primal-dual step kernels compute (:func:`pd_primal_np`, :func:`pd_dual_np`), the iteration built from them
(:func:`primal_dual_np`), the exact analysis prox by projected gradient on its dual (:func:`analysis_prox_np`) and the
duality gap of the problem with a diagonal Gaussian data term and identity measurement (:func:`duality_gap_np`).  All of
them take the operators as callables, so they run on dense matrices and on the transforms of ``oracle.pxmcmc_np`` alike.

The problem is ``min_x g(x) + h(A x)``, ``h(u) = (1 / lmda) sum_i T_i |u_i|``; ``A`` maps the state (length n) to the
coefficients (length m), ``AH`` is its adjoint.
"""
import numpy as np


def pd_primal_np(x, g, u, tau):
    """``x1 = x - tau (g + u)``, ``xbar = 2 x1 - x`` (``g = gradg(x)``, ``u = A^H v``) -> (x1, xbar)"""
    x1 = x - tau * (g + u)
    return x1, 2.0 * x1 - x


def pd_dual_np(v, w, T, sigma, rscale):
    """``v + sigma w`` projected element by element onto ``|v_i| <= r_i = T_i rscale``, as the kernel does it: a complex
    element outside its disc is scaled by ``r_i / |.|`` (one division), a real one clamped; ``|.| = r_i`` and 0 are kept,
    ``T_i = 0`` gives 0 and ``r_i = inf`` never binds."""
    y = np.asarray(v + sigma * np.asarray(w))
    r = np.broadcast_to(np.asarray(T, dtype=float) * rscale, y.shape)
    if not np.iscomplexobj(y):
        return np.minimum(np.maximum(y, -r), r)
    a = np.sqrt(y.real ** 2 + y.imag ** 2)
    out = y.copy()
    big = a > r
    out[big] = y[big] * (r[big] / a[big])
    return out


def primal_dual_np(grad, A, AH, T, lmda, tau, sigma, x0, iters, v0=None, tol=None):
    """The forward-backward primal-dual iteration of Condat (2013) and Vu (2013) from ``x0`` (and ``v0``, default 0)::

        x1   = x - tau (grad(x) + AH(v))
        xbar = 2 x1 - x
        v1   = proj_{|v_i| <= T_i / lmda}(v + sigma A(xbar))

    for ``iters`` iterations, or, with ``tol``, until ``||x1 - x|| <= tol ||x1||`` and ``||v1 - v|| <= tol ||v1||`` (a zero
    norm counts as met).  It converges for ``1 / tau - sigma ||A||^2 >= L_g / 2``.
    Returns ``(x, v, info)``: ``info`` holds ``niter``, the last step lengths ``dx``, ``dv`` and ``converged``."""
    x = np.array(x0)
    v = np.zeros_like(A(x)) if v0 is None else np.array(v0)
    info = dict(niter=0, dx=np.inf, dv=np.inf, converged=False)
    for k in range(int(iters)):
        x1, xbar = pd_primal_np(x, grad(x), AH(v), tau)
        v1 = pd_dual_np(v, A(xbar), T, sigma, 1.0 / lmda)
        dx, dv = np.linalg.norm(x1 - x), np.linalg.norm(v1 - v)
        x, v = x1, v1
        info.update(niter=k + 1, dx=dx, dv=dv)
        if tol is not None and dx <= tol * np.linalg.norm(x) and dv <= tol * np.linalg.norm(v):
            info["converged"] = True
            break
    return x, v, info


def analysis_prox_np(A, AH, T, Z, iters, sigma, return_dual=False):
    """``prox`` of ``p -> sum_i T_i |(A p)_i|`` at ``Z`` by ``iters`` projected-gradient iterations on the dual from
    ``v = 0``: ``v <- proj_{|v_i| <= T_i}(v + sigma A(Z - AH(v)))``, ``sigma <= 1 / ||A||^2``; returns ``Z - AH(v)``
    (and ``v``).  The dual objective ``1/2 ||Z - AH v||^2`` does not increase along the iteration."""
    Z = np.asarray(Z)
    v = np.zeros_like(A(Z))
    for _ in range(int(iters)):
        v = pd_dual_np(v, A(Z - AH(v)), T, sigma, 1.0)
    p = Z - AH(v)
    return (p, v) if return_dual else p


def duality_gap_np(x, v, d, ic, A, AH, T, lmda):
    """``P(x) - D(v) >= P(x) - min P`` for ``P(x) = 1/2 sum_i ic_i |x_i - d_i|^2 + (1 / lmda) sum_i T_i |(A x)_i|`` (real
    ``ic_i > 0``, identity measurement) and its Fenchel dual ``D(v) = Re <AH v, d> - 1/2 sum_i |(AH v)_i|^2 / ic_i`` on
    ``|v_i| <= T_i / lmda``.  ``v`` is projected onto that set first, so any ``v`` gives a valid bound.  P is strongly
    convex with modulus ``min ic``, hence ``||x - argmin P|| <= sqrt(2 gap / min ic)``."""
    v = pd_dual_np(np.zeros_like(v), v, T, 1.0, 1.0 / lmda)
    ic = np.asarray(ic, dtype=float)
    primal = 0.5 * np.sum(ic * np.abs(x - d) ** 2) + np.sum(np.asarray(T, dtype=float) * np.abs(A(x))) / lmda
    y = AH(v)
    dual = np.sum((np.conj(y) * d).real) - 0.5 * np.sum(np.abs(y) ** 2 / ic)
    return float(primal - dual)
