"""The elementwise steps of the samplers and optimisers (csrc/elementwise.hip, skrock.hip, fista.hip, primal_dual.hip, sapg.hip)."""
import ctypes as C

import numpy as np
import torch

from .._lib import FISTA_SLICES_MAX, SAPG_GROUPS_MAX, SAPG_SLICES_MAX, check, lib
from ._args import (_CPLX, _REAL, _batched, _chain_vector, _companion, _data_invcov, _delta_args, _dt, _nf, _noise_group, _p,
                    _result, _scratch, _state_out, _stream, _table, _vecT, as_device, device)


def soft(X, T=0.1):
    """utils.soft (pxmcmc/utils.py:55-67)."""
    x, squeeze = _batched(as_device(X))
    Tv, Ts = _vecT(T, x.shape[1], x.device)
    out = torch.empty_like(x)
    check(lib.pxm_soft(_p(x), _p(Tv), Ts, _p(out), x.shape[1], x.shape[0], _dt(x), _stream()))
    return out[0] if squeeze else out


def residual_grad(preds, data, invcov):
    """invcov .* (preds - data), invcov diagonal (pxmcmc/forward.py:66-69)."""
    p, squeeze = _batched(as_device(preds))
    n = p.shape[1]
    d, ic = _data_invcov(data, invcov, n, p.dtype, preds=p)
    out = torch.empty_like(p)
    check(lib.pxm_residual_grad(_p(p), _p(d), _p(ic), int(ic.is_complex()), _p(out), n, p.shape[0], _dt(p), _stream()))
    return out[0] if squeeze else out


def myula_step(X, gradg, T, delta, lmda, noise=None, noise_complex=False, seed=0, chain0=0, it=0, iter_dev=None, out=None,
               noise64=False):
    """chain_step(X, soft(X, T), gradg) in one pass (pxmcmc/mcmc.py:185-201 + prior.py:49-50).
    iter_dev: int64 device counter added to ``it`` when the kernel runs (graph replay); out: result buffer."""
    x, squeeze = _batched(as_device(X))
    g = _companion(gradg, x, "gradg shape mismatch")
    Tv, Ts = _vecT(T, x.shape[1], x.device)
    dd, ds = _delta_args(delta, x.shape[0], x.device)
    w, noise_group = _noise_group(noise, x, noise_complex, noise64, seed, chain0, it, iter_dev)
    out = torch.empty_like(x) if out is None else _state_out(out, x)
    check(
        lib.pxm_myula_step(
            _p(x), _p(g), _p(Tv), Ts, _p(dd), ds, float(lmda), *noise_group, _p(out), x.shape[1],
            x.shape[0], _dt(x), _stream()
        )
    )
    return out[0] if squeeze else out


def chain_step(X, proxf, gradg, delta, lmda, noise=None, noise_complex=False, seed=0, chain0=0, it=0, iter_dev=None, out=None,
               noise64=False):
    """MYULA.chain_step (pxmcmc/mcmc.py:185-201); iter_dev / out as in :func:`myula_step`."""
    x, squeeze = _batched(as_device(X))
    px = _companion(proxf, x, "shape mismatch")
    g = _companion(gradg, x, "shape mismatch")
    dd, ds = _delta_args(delta, x.shape[0], x.device)
    w, noise_group = _noise_group(noise, x, noise_complex, noise64, seed, chain0, it, iter_dev)
    out = torch.empty_like(x) if out is None else _state_out(out, x)
    check(
        lib.pxm_chain_step(
            _p(x), _p(px), _p(g), _p(dd), ds, float(lmda), *noise_group, _p(out), x.shape[1],
            x.shape[0], _dt(x), _stream()
        )
    )
    return out[0] if squeeze else out


def skrock_stage(U, a, b=0.0, c=0.0, e=0.0, r=0.0, T=None, proxf=None, gradg=None, V=None, noise=None, noise_complex=False,
                 seed=0, chain0=0, it=0, iter_dev=None, out=None, noise64=False):
    """One stage of the SKROCK recursion (pxmcmc/mcmc.py:349-368, paper coefficients): ``out = a U + b P + c gradg + e V + r Z``.

    P (when ``b != 0``): ``proxf`` if given, else ``soft(U, T)`` formed in the kernel.  ``gradg`` / ``V``: optional.
    Z (when ``r != 0``): ``noise`` if given, else the device Philox stream of :func:`myula_step` at (seed, chain0 + c, it)
    [+ ``*iter_dev``].  ``out``: result buffer (must not alias an input)."""
    u, squeeze = _batched(as_device(U))
    px, g, v = (t if t is None else _companion(t, u, "skrock_stage: proxf / gradg / V must have the state's shape")
                for t in (proxf if b != 0 else None, gradg, V))
    if b != 0 and px is None and T is None:
        raise ValueError("skrock_stage: a prox term needs proxf or the threshold T")
    Tv, Ts = _vecT(T, u.shape[1], u.device) if (b != 0 and px is None) else (None, 0.0)
    w, noise_group = _noise_group(noise if r != 0 else None, u, noise_complex, noise64, seed, chain0, it, iter_dev)
    out = torch.empty_like(u) if out is None else _state_out(out, u)
    check(
        lib.pxm_skrock_stage(
            _p(u), _p(px), _p(Tv), Ts, _p(g), _p(v), float(a), float(b), float(c), float(e), float(r), *noise_group,
            _p(out), u.shape[1], u.shape[0], _dt(u), _stream()
        )
    )
    return out[0] if squeeze else out


def fista_scratch(C_, dev):
    """scratch of :func:`fista_step` for C_ chains (the stepping engine keeps one: no allocation per iteration)"""
    return _scratch(None, 3 * FISTA_SLICES_MAX * int(C_), dev)


def fista_restart_scratch(C_, dev):
    """scratch of :func:`fista_step_restart` for C_ chains: four partial sums per slice and chain"""
    return _scratch(None, 4 * FISTA_SLICES_MAX * int(C_), dev)


def _fista_args(name, nsums, Y, gradg, X_prev, beta, T, proxf, y_with_proxf, out, sums, scratch):
    """the arguments the two FISTA steps share, checked -> (x0, squeeze, y, g, px, Tv, Ts, bt, x1, y1, sums, scratch);
    ``y_with_proxf``: Y is passed on next to a given proxf (the restarted step reads it)"""
    x0, squeeze = _batched(as_device(X_prev))
    given = proxf is not None
    px, y, g = (t if t is None else _companion(t, x0, f"{name}: Y / gradg / proxf must have the state's shape")
                for t in ((proxf, Y if y_with_proxf else None, None) if given else (None, Y, gradg)))
    if not given and T is None:
        raise ValueError(f"{name}: the threshold T is needed unless proxf is given")
    Tv, Ts = (None, 0.0) if given else _vecT(T, x0.shape[1], x0.device)
    bt = _table(beta, x0.device, f"{name}: beta must be a non-empty contiguous float64 device vector")
    C_ = x0.shape[0]
    if out is None:
        x1, y1 = torch.empty_like(x0), torch.empty_like(x0)
    else:
        x1, y1 = _state_out(out[0], x0), _state_out(out[1], x0)
    sums = _result(sums, (C_, nsums), _REAL, x0.device, f"{name}: sums must be a contiguous float64 [C, {nsums}] device array")
    scratch = _scratch(scratch, nsums * FISTA_SLICES_MAX * C_, x0.device, f"{name}: scratch is too small", any_layout=True)
    return x0, squeeze, y, g, px, Tv, Ts, bt, x1, y1, sums, scratch


def fista_step(Y, gradg, X_prev, gamma, lmda, beta, T=None, proxf=None, it=0, iter_dev=None, out=None, sums=None, scratch=None):
    """One FISTA iteration in one launch: ``X1 = soft(Y - gamma gradg, gamma T / lmda)`` -- or
    ``proxf`` when given (the prior's own prox of ``Y - gamma gradg``; Y, gradg and T are then not read) -- and
    ``Y1 = X1 + beta_k (X1 - X_prev)``.

    ``beta``: the momentum table (float64 device vector, or a sequence); ``beta_k`` is entry ``it`` [+ ``*iter_dev``], read
    when the kernel runs and clamped to the table's last entry.  ``out``: the pair of result buffers ``(X1, Y1)`` (neither
    may alias an input).  Returns ``(X1, Y1, sums)`` with ``sums`` float64 [C, 3]: per chain ``sum |X1 - X_prev|^2``,
    ``sum |X1|^2`` and ``sum T_i |X1_i|`` (NaN with ``proxf``).  ``scratch``: :func:`fista_scratch`."""
    x0, squeeze, y, g, px, Tv, Ts, bt, x1, y1, sums, scratch = _fista_args("fista_step", 3, Y, gradg, X_prev, beta, T, proxf, False,
                                                                          out, sums, scratch)
    check(
        lib.pxm_fista_step(
            _p(y), _p(g), _p(px), _p(Tv), Ts, _p(x0), float(gamma), float(lmda), _p(bt), bt.numel(), int(it), _p(iter_dev),
            _p(x1), _p(y1), _p(sums), _p(scratch), x0.shape[1], x0.shape[0], _dt(x0), _stream()
        )
    )
    return (x1[0], y1[0], sums) if squeeze else (x1, y1, sums)


def fista_step_restart(Y, gradg, X_prev, gamma, lmda, beta, momentum_index, T=None, proxf=None, restarts=None, restart=True,
                       out=None, sums=None, scratch=None):
    """:func:`fista_step` with adaptive (gradient) restart decided per chain on the device.

    ``momentum_index`` ([C] 64-bit integer device vector): chain c steps with ``beta[min(momentum_index[c], len - 1)]``.
    ``sums`` is float64 [C, 4]: the three sums of :func:`fista_step`, then ``r_c = sum Re conj(Y - X1) (X1 - X_prev)``.
    After the step the device sets ``momentum_index[c] = 0`` and adds one to ``restarts[c]`` (optional [C] vector) where
    ``restart`` and ``r_c > 0``, and adds one to ``momentum_index[c]`` everywhere else; ``Y1`` keeps the momentum of this
    step.  ``Y`` is needed with ``proxf`` too (``r_c`` reads it).  A missing ``momentum_index`` is reported by the library.
    ``scratch``: :func:`fista_restart_scratch`.  Returns ``(X1, Y1, sums)``."""
    name = "fista_step_restart"
    x0, squeeze, y, g, px, Tv, Ts, bt, x1, y1, sums, scratch = _fista_args(name, 4, Y, gradg, X_prev, beta, T, proxf, True, out,
                                                                          sums, scratch)
    C_ = x0.shape[0]
    # per-chain 64-bit device counters (torch.int64, or torch.uint64: the library reads them as uint64_t)
    mi, rs = (_chain_vector(t, C_, x0.device, (torch.int64, torch.uint64),
                            f"{name}: {what} must be a contiguous 64-bit integer [C] device vector", optional=True)
              for what, t in (("momentum_index", momentum_index), ("restarts", restarts)))
    check(
        lib.pxm_fista_step_restart(
            _p(y), _p(g), _p(px), _p(Tv), Ts, _p(x0), float(gamma), float(lmda), _p(bt), bt.numel(), _p(mi), _p(rs),
            int(bool(restart)), _p(x1), _p(y1), _p(sums), _p(scratch), x0.shape[1], C_, _dt(x0), _stream()
        )
    )
    return (x1[0], y1[0], sums) if squeeze else (x1, y1, sums)


def pd_scratch(C_, dev):
    """scratch of :func:`pd_primal_step` and :func:`pd_dual_step` for C_ chains (the larger of the two: three partial sums
    per slice and chain; calls on one stream may share it)"""
    return _scratch(None, 3 * FISTA_SLICES_MAX * int(C_), dev)


def pd_primal_step(X, G, U, tau, out=None, sums=None, scratch=None):
    """The primal half of one primal-dual iteration in one launch: ``X1 = X - tau (G + U)`` with
    ``G = gradg(X)`` and ``U = A^H v``, and ``Xbar = 2 X1 - X``.

    ``out``: the pair of result buffers ``(X1, Xbar)`` (neither may alias an input or the other).  Returns ``(X1, Xbar, sums)``
    with ``sums`` float64 [C, 2]: per chain ``sum |X1 - X|^2`` and ``sum |X1|^2``.  ``scratch``: :func:`pd_scratch`."""
    name = "pd_primal_step"
    x, squeeze = _batched(as_device(X))
    g, u = (_companion(t, x, f"{name}: G and U must have the state's shape") for t in (G, U))
    C_ = x.shape[0]
    if out is None:
        x1, xbar = torch.empty_like(x), torch.empty_like(x)
    else:
        x1, xbar = _state_out(out[0], x), _state_out(out[1], x)
    sums = _result(sums, (C_, 2), _REAL, x.device, f"{name}: sums must be a contiguous float64 [C, 2] device array")
    scratch = _scratch(scratch, 2 * FISTA_SLICES_MAX * C_, x.device, f"{name}: scratch is too small", any_layout=True)
    check(lib.pxm_pd_primal_step(_p(x), _p(g), _p(u), float(tau), _p(x1), _p(xbar), _p(sums), _p(scratch), x.shape[1], C_, _dt(x),
                                 _stream()))
    return (x1[0], xbar[0], sums) if squeeze else (x1, xbar, sums)


def pd_dual_step(V, W, T, sigma, rscale, out=None, sums=None, scratch=None):
    """The dual half of one primal-dual iteration in one launch: ``V1`` is ``V + sigma W`` projected
    element by element onto ``|v_i| <= T_i rscale`` (``W = A xbar``; ``rscale = 1 / lmda`` in the iteration, 1 in the dual
    iteration of the analysis prox).

    ``out``: the result buffer (must not alias an input).  Returns ``(V1, sums)`` with ``sums`` float64 [C, 3]: per chain
    ``sum |V1 - V|^2``, ``sum |V1|^2`` and ``sum T_i |W_i|``.  ``scratch``: :func:`pd_scratch`."""
    name = "pd_dual_step"
    v, squeeze = _batched(as_device(V))
    w = _companion(W, v, f"{name}: W must have the shape of V")
    if T is None:
        raise ValueError(f"{name}: the threshold T is needed")
    Tv, Ts = _vecT(T, v.shape[1], v.device)
    C_ = v.shape[0]
    v1 = torch.empty_like(v) if out is None else _state_out(out, v)
    sums = _result(sums, (C_, 3), _REAL, v.device, f"{name}: sums must be a contiguous float64 [C, 3] device array")
    scratch = _scratch(scratch, 3 * FISTA_SLICES_MAX * C_, v.device, f"{name}: scratch is too small", any_layout=True)
    check(lib.pxm_pd_dual_step(_p(v), _p(w), _p(Tv), Ts, float(sigma), float(rscale), _p(v1), _p(sums), _p(scratch), v.shape[1], C_,
                               _dt(v), _stream()))
    return (v1[0], sums) if squeeze else (v1, sums)


def sapg_scratch(C_, dev):
    """scratch of :func:`sapg_step` for C_ chains (the stepping engine keeps one: no allocation per iteration)"""
    return _scratch(None, (SAPG_SLICES_MAX + 1) * int(C_), dev)


def sapg_step(X, gradg, T, delta, lmda, theta, eta, d, rho, eta_min, eta_max, pool=False, trace=None, noise=None,
              noise_complex=False, seed=0, chain0=0, it=0, iter_dev=None, out=None, scratch=None, noise64=False):
    """One SAPG iteration: the MYULA step of :func:`myula_step` with chain c's soft threshold scaled
    by ``theta[c]``, read on the device, then ``eta[c] = clip(eta[c] + rho_k (d - theta[c] G_c))``, ``theta[c] = exp(eta[c])``
    with ``G_c = (1 / lmda) sum_i T_i |X1_i|`` of the new state (``pool``: the chain mean of the ``G_c``).

    ``theta``, ``eta``: contiguous float64 ``[C]`` device vectors, updated in place.  ``rho``: the step-size table (float64
    device vector, or a sequence); ``rho_k`` is entry ``it`` [+ ``*iter_dev``], read when the kernel runs and clamped to the
    table's last entry.  ``trace``: float64 ``[n_trace, C, 3]`` device array or None; row ``it`` [+ ``*iter_dev``], when there
    is one, receives ``(theta, eta, G)``.  ``delta`` is a float (no per-chain step).  Returns ``(X1, theta, eta)``."""
    x, squeeze = _batched(as_device(X))
    g = _companion(gradg, x, "sapg_step: gradg shape mismatch")
    if isinstance(delta, torch.Tensor):
        raise ValueError("sapg_step: delta must be a float (no per-chain step sizes)")
    C_, n = x.shape
    Tv, Ts = _vecT(T, n, x.device)
    w, noise_group = _noise_group(noise, x, noise_complex, noise64, seed, chain0, int(it), iter_dev)
    for name, v in (("theta", theta), ("eta", eta)):
        _chain_vector(v, C_, x.device, (_REAL,), f"sapg_step: {name} must be a contiguous float64 [C] device vector")
    rt = _table(rho, x.device, "sapg_step: rho must be a non-empty contiguous float64 device vector")
    n_trace = 0
    if trace is not None:
        if trace.dim() != 3 or trace.shape[1:] != (C_, 3) or trace.dtype != _REAL or not trace.is_contiguous() or trace.device != x.device:
            raise ValueError("sapg_step: trace must be a contiguous float64 [n_trace, C, 3] device array")
        n_trace = trace.shape[0]
    out = torch.empty_like(x) if out is None else _state_out(out, x)
    scratch = _scratch(scratch, (SAPG_SLICES_MAX + 1) * C_, x.device, "sapg_step: scratch is too small (sapg_scratch)")
    check(
        lib.pxm_sapg_step(
            _p(x), _p(g), _p(Tv), Ts, float(delta), float(lmda), *noise_group,
            _p(theta), _p(eta), float(d), _p(rt), rt.numel(), float(eta_min), float(eta_max), int(bool(pool)),
            _p(trace if n_trace else None), n_trace, _p(out), _p(scratch), n, C_, _dt(x), _stream()
        )
    )
    return (out[0] if squeeze else out), theta, eta


def sapg_groups_scratch(C_, K, dev):
    """scratch of :func:`sapg_step_groups` for C_ chains of K groups"""
    return _scratch(None, (SAPG_SLICES_MAX + 1) * int(K) * int(C_), dev)


def sapg_group_bounds(bounds, n, name="sapg_step_groups"):
    """the offsets ``0 = b_0 < b_1 < ... < b_K = n`` of K contiguous, non-empty groups (any integer sequence), checked by the
    rule of the C-ABI -> int64 numpy array of K + 1"""
    try:
        b = np.asarray(bounds)
        if b.dtype.kind not in "iu":
            raise TypeError
        b = b.astype(np.int64)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: bounds must be a sequence of integers") from None
    if b.ndim != 1 or not 2 <= b.size <= SAPG_GROUPS_MAX + 1:
        raise ValueError(f"{name}: bounds must hold K + 1 offsets, 1 <= K <= {SAPG_GROUPS_MAX}")
    if b[0] != 0 or b[-1] != n or np.any(np.diff(b) <= 0):
        raise ValueError(f"{name}: bounds must increase strictly from 0 to n = {n} (no empty group)")
    return b


def sapg_step_groups(X, gradg, T, delta, lmda, theta, eta, bounds, d, rho, eta_min, eta_max, pool=False, trace=None, noise=None,
                     noise_complex=False, seed=0, chain0=0, it=0, iter_dev=None, out=None, scratch=None, noise64=False):
    """:func:`sapg_step` with one theta per chain and per group: the elements ``bounds[k] <= i <
    bounds[k + 1]`` of chain c are shrunk at ``theta[c, k] T_i``; ``G[c, k] = (1 / lmda) sum T_i |X1_i|`` over the group;
    ``eta[c, k] = clip(eta[c, k] + rho[j, k] (d[k] - theta[c, k] G[c, k]))``, ``theta = exp(eta)`` (``pool``: the chain mean of
    ``G[:, k]``, group by group).

    ``bounds``: K + 1 integers increasing strictly from 0 to n.  ``theta``, ``eta``: contiguous float64 ``[C, K]`` device
    arrays, updated in place.  ``d``: the groups' dimensions, float64 ``[K]`` device vector (or a sequence).  ``rho``: float64
    ``[n_rho, K]`` device table (or a nested sequence); row ``j = it`` [+ ``*iter_dev``], clamped to the last.  ``trace``:
    float64 ``[n_trace, C, K, 3]`` device array or None; row j receives ``(theta, eta, G)``.  ``scratch``:
    :func:`sapg_groups_scratch`.  Returns ``(X1, theta, eta)``."""
    x, squeeze = _batched(as_device(X))
    g = _companion(gradg, x, "sapg_step_groups: gradg shape mismatch")
    if isinstance(delta, torch.Tensor):
        raise ValueError("sapg_step_groups: delta must be a float (no per-chain step sizes)")
    C_, n = x.shape
    b = sapg_group_bounds(bounds, n)
    K = b.size - 1
    Tv, Ts = _vecT(T, n, x.device)
    w, noise_group = _noise_group(noise, x, noise_complex, noise64, seed, chain0, int(it), iter_dev)
    f64 = lambda t, shape: (isinstance(t, torch.Tensor) and t.dtype == _REAL and tuple(t.shape) == shape  # noqa: E731
                            and t.is_contiguous() and t.device == x.device)
    for name, v in (("theta", theta), ("eta", eta)):
        if not f64(v, (C_, K)):
            raise ValueError(f"sapg_step_groups: {name} must be a contiguous float64 [C, K] device array")
    dv = d if isinstance(d, torch.Tensor) else as_device(np.atleast_1d(np.asarray(d, dtype=float)), _REAL)
    if not f64(dv, (K,)):
        raise ValueError("sapg_step_groups: d must be a contiguous float64 [K] device vector")
    rt = rho if isinstance(rho, torch.Tensor) else as_device(np.asarray(rho, dtype=float), _REAL)
    if rt.dim() != 2 or rt.shape[0] < 1 or not f64(rt, (rt.shape[0], K)):
        raise ValueError("sapg_step_groups: rho must be a non-empty contiguous float64 [n_rho, K] device table")
    n_trace = 0
    if trace is not None:
        if not (isinstance(trace, torch.Tensor) and trace.dim() == 4 and f64(trace, (trace.shape[0], C_, K, 3))):
            raise ValueError("sapg_step_groups: trace must be a contiguous float64 [n_trace, C, K, 3] device array")
        n_trace = trace.shape[0]
    out = torch.empty_like(x) if out is None else _state_out(out, x)
    scratch = _scratch(scratch, (SAPG_SLICES_MAX + 1) * K * C_, x.device,
                       "sapg_step_groups: scratch is too small (sapg_groups_scratch)")
    check(
        lib.pxm_sapg_step_groups(
            _p(x), _p(g), _p(Tv), Ts, float(delta), float(lmda), *noise_group,
            _p(theta), _p(eta), b.ctypes.data_as(C.c_void_p), K, _p(dv), _p(rt), rt.shape[0], float(eta_min), float(eta_max),
            int(bool(pool)), _p(trace if n_trace else None), n_trace, _p(out), _p(scratch), n, C_, _dt(x), _stream()
        )
    )
    return (out[0] if squeeze else out), theta, eta


def randn(n, C_=1, complex_=False, seed=0, chain0=0, it=0, noise64=False):
    """N(0,1) draws of the device Philox stream keyed (seed, chain0 + c, it); noise64: Box-Muller in double precision"""
    out = torch.empty((C_, n), dtype=_CPLX if complex_ else _REAL, device=device())
    check(lib.pxm_randn(_p(out), n, C_, int(complex_) | _nf(noise64), seed, chain0, it, _stream()))
    return out


def box_muller(u1, u2, noise64=False):
    """the Box-Muller step of the device noise stream on given uniforms (test aid, include/pxmcmc_amd.h) -> (z0, z1)"""
    a, b = as_device(u1, _REAL).reshape(-1), as_device(u2, _REAL).reshape(-1)
    if a.shape != b.shape:
        raise ValueError("box_muller: u1 and u2 must have the same length")
    z0, z1 = torch.empty_like(a), torch.empty_like(a)
    check(lib.pxm_box_muller(_p(a), _p(b), _p(z0), _p(z1), a.numel(), int(bool(noise64)), _stream()))
    return z0, z1


def select_copy_many(flag, pairs):
    """dst[c] = src[c] for chains with flag[c] != 0, for up to four (src, dst) pairs in one launch."""
    k = len(pairs)
    if not 1 <= k <= 4:
        raise ValueError("select_copy_many takes 1 to 4 array pairs")
    C_ = flag.shape[0]
    if flag.dim() != 1 or flag.dtype != torch.int32 or not flag.is_contiguous():
        raise ValueError("select_copy_many: flag must be a contiguous int32 [C] array")
    for s_, d_ in pairs:
        if s_.shape != d_.shape or s_.dtype != d_.dtype or not s_.is_contiguous() or not d_.is_contiguous():
            raise ValueError("select_copy_many: shape / dtype / layout mismatch")
        # the kernel copies chain c's words [c * len, (c + 1) * len): the per-chain length is the array's size over C, so the
        # leading axis must be the chain axis (one chain may come without it)
        if C_ > 1 and (s_.dim() < 1 or s_.shape[0] != C_):
            raise ValueError("select_copy_many: with %d chains every array must be [%d, ...], got %s" % (C_, C_, tuple(s_.shape)))
    srcs = (C.c_void_p * k)(*[p[0].data_ptr() for p in pairs])
    dsts = (C.c_void_p * k)(*[p[1].data_ptr() for p in pairs])
    ns = (C.c_int64 * k)(*[p[0].numel() // C_ for p in pairs])
    es = (C.c_int * k)(*[p[0].element_size() for p in pairs])
    check(lib.pxm_select_copy_many(_p(flag), k, srcs, dsts, ns, es, C_, _stream()))


def counter_add(counter, inc=1):
    check(lib.pxm_counter_add(_p(counter), int(inc), _stream()))
