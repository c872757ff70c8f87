"""
Thin tensor-level wrappers over the C-ABI: torch supplies device memory and the stream,
every operation is a hand-written HIP kernel behind ``include/pxmcmc_amd.h``.

Conventions: arrays are ``[C, n]`` (chain batch first) or ``[n]`` (one chain); dtype is
float64 or complex128; outputs are fresh tensors (the reference never mutates inputs,
SURVEY.md section 8b).
"""
import ctypes as C
import threading
import weakref

import numpy as np
import torch

from ._lib import NOISE_F64, STATUS_PAIR_SYNC, PxmError, check, lib, require_gpu

_CPLX, _REAL = torch.complex128, torch.float64


def device():
    require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def as_device(x, dtype=None):
    """numpy / torch / sequence -> contiguous tensor on the GPU (float64 or complex128)."""
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if dtype is None:
        dtype = _CPLX if t.is_complex() else _REAL
    return t.to(device=device(), dtype=dtype).contiguous()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _batched(x):
    """[n] -> ([1, n], True); [C, n] -> (x, False)."""
    if x.dim() == 1:
        return x.unsqueeze(0), True
    if x.dim() != 2:
        raise ValueError("expected a 1-D (single chain) or 2-D (chain batch) array")
    return x, False


def _dt(x):
    if x.dtype == _CPLX:
        return 1
    if x.dtype == _REAL:
        return 0
    raise TypeError(f"unsupported dtype {x.dtype}: float64 or complex128 only")


def _vecT(T, n, dev):
    """threshold / weight argument: python scalar -> (null, value); vector -> (tensor, 0)."""
    if T is None:
        return None, 0.0
    if isinstance(T, (int, float)):
        return None, float(T)
    t = as_device(T, _REAL)
    if t.numel() == 1:
        return None, float(t.item())
    if t.numel() != n:
        raise ValueError("threshold / weight vector has the wrong length")
    return t.reshape(-1), 0.0


# ---- elementwise -----------------------------------------------------------------------
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
    d = as_device(data, p.dtype).reshape(-1)
    ic = as_device(invcov)
    if ic.is_complex() and not p.is_complex():
        raise TypeError("complex inverse covariance needs complex predictions")
    ic = ic.reshape(-1)
    if d.numel() != n or ic.numel() != n:
        raise ValueError("data / invcov length mismatch")
    out = torch.empty_like(p)
    check(lib.pxm_residual_grad(_p(p), _p(d), _p(ic), int(ic.is_complex()), _p(out), n, p.shape[0], _dt(p), _stream()))
    return out[0] if squeeze else out


def _nf(noise64):
    """PXM_NOISE_F64 flag of the noise-drawing entry points: the Philox stream's Box-Muller step in double precision"""
    return NOISE_F64 if noise64 else 0


def raise_on_status(status, what):
    """A plan's device status word (pxm_wav_status / pxm_sht_status) -> PxmError when a bounded wait expired"""
    if status:
        bits = []
        if status & STATUS_PAIR_SYNC:
            bits.append("a wave-pair wait or ring-group wait of the fused phi-DFT kernels expired (csrc/dft_wave.h: d5_pair_sync)")
        if status & ~STATUS_PAIR_SYNC:
            bits.append(f"unknown status bits {status:#x}")
        raise PxmError(f"{what}: device status {status:#x}: " + "; ".join(bits) + " -- the results of this plan since its last "
                       "status check are invalid")


def _delta_args(delta, C_, dev):
    if isinstance(delta, torch.Tensor):
        dd = delta.to(device=dev, dtype=_REAL).contiguous()
        if dd.numel() != C_:
            raise ValueError("per-chain delta must have one entry per chain")
        return dd, 0.0
    return None, float(delta)


def _pair_noise_args(noise, x):
    """mode 2 (two real chains per complex slot): injected noise is a real [2 * slots, N] array"""
    if noise is None:
        return None, 2
    w = as_device(noise, _REAL)
    if w.dim() != 2 or w.shape != (2 * x.shape[0], x.shape[1]):
        raise ValueError("real-pair noise must be a float64 [2 * slots, N] array")
    return w, 2


def _noise_args(noise, x, noise_complex):
    if noise is None:
        return None, int(bool(noise_complex))
    w = as_device(noise)
    if w.dim() == 1:
        w = w.unsqueeze(0)
    if w.shape != x.shape:
        raise ValueError("injected noise must have the state's shape")
    if w.is_complex() and not x.is_complex():
        raise TypeError("complex noise needs a complex state")
    return w, int(w.is_complex())


def myula_step(X, gradg, T, delta, lmda, noise=None, noise_complex=False, seed=0, chain0=0, it=0, iter_dev=None, out=None,
               noise64=False):
    """chain_step(X, soft(X, T), gradg) in one pass (pxmcmc/mcmc.py:185-201 + prior.py:49-50).
    iter_dev: int64 device counter added to ``it`` when the kernel runs (graph replay); out: result buffer."""
    x, squeeze = _batched(as_device(X))
    g, _ = _batched(as_device(gradg, x.dtype))
    if g.shape != x.shape:
        raise ValueError("gradg shape mismatch")
    Tv, Ts = _vecT(T, x.shape[1], x.device)
    dd, ds = _delta_args(delta, x.shape[0], x.device)
    w, wc = _noise_args(noise, x, noise_complex)
    out = torch.empty_like(x) if out is None else _out_like(out, x)
    check(
        lib.pxm_myula_step(
            _p(x), _p(g), _p(Tv), Ts, _p(dd), ds, float(lmda), _p(w), wc | _nf(noise64), seed, chain0, it, _p(iter_dev), _p(out), x.shape[1],
            x.shape[0], _dt(x), _stream()
        )
    )
    return out[0] if squeeze else out


def _out_like(out, x):
    o = out if out.dim() == 2 else out.unsqueeze(0)
    if o.shape != x.shape or o.dtype != x.dtype or not o.is_contiguous() or o.device != x.device:
        raise ValueError("out must be a contiguous device array of the state's shape and dtype")
    return o


def chain_step(X, proxf, gradg, delta, lmda, noise=None, noise_complex=False, seed=0, chain0=0, it=0, iter_dev=None, out=None,
               noise64=False):
    """MYULA.chain_step (pxmcmc/mcmc.py:185-201); iter_dev / out as in :func:`myula_step`."""
    x, squeeze = _batched(as_device(X))
    px, _ = _batched(as_device(proxf, x.dtype))
    g, _ = _batched(as_device(gradg, x.dtype))
    if g.shape != x.shape or px.shape != x.shape:
        raise ValueError("shape mismatch")
    dd, ds = _delta_args(delta, x.shape[0], x.device)
    w, wc = _noise_args(noise, x, noise_complex)
    out = torch.empty_like(x) if out is None else _out_like(out, x)
    check(
        lib.pxm_chain_step(
            _p(x), _p(px), _p(g), _p(dd), ds, float(lmda), _p(w), wc | _nf(noise64), seed, chain0, it, _p(iter_dev), _p(out), x.shape[1],
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
    args = []
    for t in (proxf if b != 0 else None, gradg, V):
        if t is None:
            args.append(None)
            continue
        t, _ = _batched(as_device(t, u.dtype))
        if t.shape != u.shape:
            raise ValueError("skrock_stage: proxf / gradg / V must have the state's shape")
        args.append(t)
    px, g, v = args
    if b != 0 and px is None and T is None:
        raise ValueError("skrock_stage: a prox term needs proxf or the threshold T")
    Tv, Ts = _vecT(T, u.shape[1], u.device) if (b != 0 and px is None) else (None, 0.0)
    w, wc = _noise_args(noise, u, noise_complex) if r != 0 else (None, int(bool(noise_complex)))
    out = torch.empty_like(u) if out is None else _out_like(out, u)
    check(
        lib.pxm_skrock_stage(
            _p(u), _p(px), _p(Tv), Ts, _p(g), _p(v), float(a), float(b), float(c), float(e), float(r), _p(w), wc | _nf(noise64),
            seed, chain0, it, _p(iter_dev), _p(out), u.shape[1], u.shape[0], _dt(u), _stream()
        )
    )
    return out[0] if squeeze else out


FISTA_SLICES_MAX = 256  # PXM_FISTA_SLICES_MAX: partial sums per chain of pxm_fista_step


def fista_scratch(C_, dev):
    """scratch of :func:`fista_step` for C_ chains (the stepping engine keeps one: no allocation per iteration)"""
    return torch.empty(3 * FISTA_SLICES_MAX * int(C_), dtype=_REAL, device=dev)


def fista_restart_scratch(C_, dev):
    """scratch of :func:`fista_step_restart` for C_ chains: four partial sums per slice and chain"""
    return torch.empty(4 * FISTA_SLICES_MAX * int(C_), dtype=_REAL, device=dev)


def _fista_args(name, nsums, Y, gradg, X_prev, beta, T, proxf, y_with_proxf, out, sums, scratch):
    """the arguments the two FISTA steps share, checked -> (x0, squeeze, y, g, px, Tv, Ts, bt, x1, y1, sums, scratch);
    ``y_with_proxf``: Y is passed on next to a given proxf (the restarted step reads it)"""
    x0, squeeze = _batched(as_device(X_prev))
    given = proxf is not None
    args = []
    for t in ((proxf, Y if y_with_proxf else None, None) if given else (None, Y, gradg)):
        if t is None:
            args.append(None)
            continue
        t, _ = _batched(as_device(t, x0.dtype))
        if t.shape != x0.shape:
            raise ValueError(f"{name}: Y / gradg / proxf must have the state's shape")
        args.append(t)
    px, y, g = args
    if not given and T is None:
        raise ValueError(f"{name}: the threshold T is needed unless proxf is given")
    Tv, Ts = (None, 0.0) if given else _vecT(T, x0.shape[1], x0.device)
    bt = beta if isinstance(beta, torch.Tensor) else as_device(np.atleast_1d(np.asarray(beta, dtype=float)), _REAL)
    if bt.dtype != _REAL or bt.dim() != 1 or bt.numel() < 1 or not bt.is_contiguous() or bt.device != x0.device:
        raise ValueError(f"{name}: beta must be a non-empty contiguous float64 device vector")
    C_ = x0.shape[0]
    if out is None:
        x1, y1 = torch.empty_like(x0), torch.empty_like(x0)
    else:
        x1, y1 = _out_like(out[0], x0), _out_like(out[1], x0)
    if sums is None:
        sums = torch.empty((C_, nsums), dtype=_REAL, device=x0.device)
    elif sums.shape != (C_, nsums) or sums.dtype != _REAL or not sums.is_contiguous():
        raise ValueError(f"{name}: sums must be a contiguous float64 [C, {nsums}] device array")
    if scratch is None:
        scratch = torch.empty(nsums * FISTA_SLICES_MAX * C_, dtype=_REAL, device=x0.device)
    elif scratch.numel() < nsums * FISTA_SLICES_MAX * C_ or scratch.dtype != _REAL:
        raise ValueError(f"{name}: scratch is too small")
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


def _index_arg(name, what, t, C_, dev):
    """a per-chain 64-bit device counter (torch.int64, or torch.uint64: the library reads it as uint64_t)"""
    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype not in (torch.int64, torch.uint64) or t.shape != (C_,)
                          or not t.is_contiguous() or t.device != dev):
        raise ValueError(f"{name}: {what} must be a contiguous 64-bit integer [C] device vector")
    return t


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
    mi = _index_arg(name, "momentum_index", momentum_index, C_, x0.device)
    rs = _index_arg(name, "restarts", restarts, C_, x0.device)
    check(
        lib.pxm_fista_step_restart(
            _p(y), _p(g), _p(px), _p(Tv), Ts, _p(x0), float(gamma), float(lmda), _p(bt), bt.numel(), _p(mi), _p(rs),
            int(bool(restart)), _p(x1), _p(y1), _p(sums), _p(scratch), x0.shape[1], C_, _dt(x0), _stream()
        )
    )
    return (x1[0], y1[0], sums) if squeeze else (x1, y1, sums)


LCI_POINTS = 32  # PXM_LCI_POINTS: values of xi per slot and pass of pxm_lci_eval
LCI_EMPTY, LCI_UNCONSTRAINED, LCI_NONFINITE = 1, 2, 4  # PXM_LCI_*: bits of the status of pxm_lci_search (0: ok)


def lci_scratch(n, C_, dev):
    """scratch of the three ``lci_*`` calls for C_ slots of vectors up to n long"""
    return torch.empty(int(check(lib.pxm_lci_scratch_doubles(int(n), int(C_)))), dtype=_REAL, device=dev)


def _lci_scratch_arg(fn, scratch, n, C_, dev):
    if scratch is None:
        return lci_scratch(n, C_, dev)
    if scratch.dtype != _REAL or not scratch.is_contiguous() or scratch.numel() < lib.pxm_lci_scratch_doubles(int(n), int(C_)):
        raise ValueError("%s: scratch is too small (lci_scratch)" % fn)
    return scratch


def _lci_pair(fn, a, b):
    x, _ = _batched(as_device(a))
    y, _ = _batched(as_device(b, x.dtype))
    if y.shape != x.shape or x.shape[1] < 1:
        raise ValueError("%s: the two arrays must share one non-empty [C, n] shape" % fn)
    return x, y


def lci_data_terms(preds_a, preds_b, data, w, out=None, scratch=None):
    """``(q0, q1, q2) = (1/2 sum w |r|^2, sum w Re(conj(r) s), 1/2 sum w |s|^2)`` per slot with ``r = preds_a - data`` and
    ``s = preds_b`` -> float64 [C, 3].  ``preds_a``, ``preds_b``: [C, ndata]; ``data`` [ndata] (taken
    in their dtype) and ``w`` [ndata], real, are shared by the slots."""
    pa, pb = _lci_pair("lci_data_terms", preds_a, preds_b)
    C_, nd = pa.shape
    d, wv = as_device(data, pa.dtype).reshape(-1), as_device(w, _REAL).reshape(-1)
    if d.numel() != nd or wv.numel() != nd:
        raise ValueError("lci_data_terms: data / w length mismatch")
    if out is None:
        out = torch.empty((C_, 3), dtype=_REAL, device=pa.device)
    else:
        _dev_tensors("lci_data_terms", "out must be a contiguous float64 [C, 3] device tensor", (out, _REAL, (C_, 3)))
    scratch = _lci_scratch_arg("lci_data_terms", scratch, nd, C_, pa.device)
    check(lib.pxm_lci_data_terms(_p(pa), _p(pb), _p(d), _p(wv), _p(out), _p(scratch), nd, C_, _dt(pa), _stream()))
    return out


def lci_eval(a, b, T, xi, out=None, scratch=None):
    """``P[c, j] = sum_k T_k |a_ck + xi[c, j] b_ck|`` for the 32 real values ``xi[c]`` of every slot, in one pass over ``a``,
    ``b`` [C, n] and ``T`` (vector or scalar) -> float64 [C, 34]: the 32 sums, then ``S_a = sum T |a|`` and ``S_b = sum T |b|``."""
    x, y = _lci_pair("lci_eval", a, b)
    C_, n = x.shape
    Tv, Ts = _vecT(T, n, x.device)
    _dev_tensors("lci_eval", "xi must be a contiguous float64 [C, 32] device tensor", (xi, _REAL, (C_, LCI_POINTS)))
    if out is None:
        out = torch.empty((C_, LCI_POINTS + 2), dtype=_REAL, device=x.device)
    else:
        _dev_tensors("lci_eval", "out must be a contiguous float64 [C, 34] device tensor", (out, _REAL, (C_, LCI_POINTS + 2)))
    scratch = _lci_scratch_arg("lci_eval", scratch, n, C_, x.device)
    check(lib.pxm_lci_eval(_p(x), _p(y), _p(Tv), Ts, _p(xi), _p(out), _p(scratch), n, C_, _dt(x), _stream()))
    return out


def lci_search(a, b, T, quad, lmda, gamma, rounds=10, out=None, status=None, scratch=None):
    """The interval ``{xi : F(xi) <= gamma}`` of ``F(xi) = q0 + q1 xi + q2 xi^2 + (1 / lmda) sum T |a + xi b|`` per slot, by
    ``rounds`` passes of :func:`lci_eval` enqueued on the current stream (nothing is read back; capturable).  ``quad``
    float64 [C, 3] and ``gamma`` float64 [C] on the device.  Returns ``(out, status)``: float64 [C, 8] = (lower, upper, width
    of the lower bracket, of the upper bracket, smallest F seen, its xi, outer bracket lo, hi) and int32 [C] (0, or the
    ``LCI_*`` bits)."""
    x, y = _lci_pair("lci_search", a, b)
    C_, n = x.shape
    Tv, Ts = _vecT(T, n, x.device)
    _dev_tensors("lci_search", "quad [C, 3] and gamma [C] must be contiguous float64 device tensors",
                 (quad, _REAL, (C_, 3)), (gamma, _REAL, (C_,)))
    if out is None:
        out = torch.empty((C_, 8), dtype=_REAL, device=x.device)
    if status is None:
        status = torch.empty(C_, dtype=torch.int32, device=x.device)
    _dev_tensors("lci_search", "out float64 [C, 8] and status int32 [C] must be contiguous device tensors",
                 (out, _REAL, (C_, 8)), (status, torch.int32, (C_,)))
    scratch = _lci_scratch_arg("lci_search", scratch, n, C_, x.device)
    check(lib.pxm_lci_search(_p(x), _p(y), _p(Tv), Ts, _p(quad), float(lmda), _p(gamma), int(rounds), _p(out), _p(status),
                             _p(scratch), n, C_, _dt(x), _stream()))
    return out, status


SAPG_SLICES_MAX = 256  # PXM_SAPG_SLICES_MAX: partial sums per chain of pxm_sapg_step


def sapg_scratch(C_, dev):
    """scratch of :func:`sapg_step` for C_ chains (the stepping engine keeps one: no allocation per iteration)"""
    return torch.empty((SAPG_SLICES_MAX + 1) * int(C_), dtype=_REAL, device=dev)


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
    g, _ = _batched(as_device(gradg, x.dtype))
    if g.shape != x.shape:
        raise ValueError("sapg_step: gradg shape mismatch")
    if isinstance(delta, torch.Tensor):
        raise ValueError("sapg_step: delta must be a float (no per-chain step sizes)")
    C_, n = x.shape
    Tv, Ts = _vecT(T, n, x.device)
    w, wc = _noise_args(noise, x, noise_complex)
    for name, v in (("theta", theta), ("eta", eta)):
        if not isinstance(v, torch.Tensor) or v.shape != (C_,) or v.dtype != _REAL or not v.is_contiguous() or v.device != x.device:
            raise ValueError(f"sapg_step: {name} must be a contiguous float64 [C] device vector")
    rt = rho if isinstance(rho, torch.Tensor) else as_device(np.atleast_1d(np.asarray(rho, dtype=float)), _REAL)
    if rt.dtype != _REAL or rt.dim() != 1 or rt.numel() < 1 or not rt.is_contiguous() or rt.device != x.device:
        raise ValueError("sapg_step: rho must be a non-empty contiguous float64 device vector")
    n_trace = 0
    if trace is not None:
        if trace.dim() != 3 or trace.shape[1:] != (C_, 3) or trace.dtype != _REAL or not trace.is_contiguous() or trace.device != x.device:
            raise ValueError("sapg_step: trace must be a contiguous float64 [n_trace, C, 3] device array")
        n_trace = trace.shape[0]
    out = torch.empty_like(x) if out is None else _out_like(out, x)
    if scratch is None:
        scratch = sapg_scratch(C_, x.device)
    elif scratch.numel() < (SAPG_SLICES_MAX + 1) * C_ or scratch.dtype != _REAL or not scratch.is_contiguous():
        raise ValueError("sapg_step: scratch is too small (sapg_scratch)")
    check(
        lib.pxm_sapg_step(
            _p(x), _p(g), _p(Tv), Ts, float(delta), float(lmda), _p(w), wc | _nf(noise64), seed, chain0, int(it), _p(iter_dev),
            _p(theta), _p(eta), float(d), _p(rt), rt.numel(), float(eta_min), float(eta_max), int(bool(pool)),
            _p(trace if n_trace else None), n_trace, _p(out), _p(scratch), n, C_, _dt(x), _stream()
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


def _red_scratch(C_, dev):
    """caller-owned scratch of the two-stage reductions (torch's caching allocator: stream-ordered reuse)"""
    return torch.empty(int(lib.pxm_reduce_scratch_doubles(int(C_))), dtype=_REAL, device=dev)


def reduce_l1(X, w=None):
    """sum |w X| per chain (pxmcmc/prior.py:28-35,83-84) -> float64 [C]."""
    x, _ = _batched(as_device(X))
    wv = None if w is None else as_device(w, _REAL).reshape(-1)
    if wv is not None and wv.numel() != x.shape[1]:
        raise ValueError("weight length mismatch")
    out = torch.empty(x.shape[0], dtype=_REAL, device=x.device)
    check(lib.pxm_reduce_l1(_p(x), _p(wv), _p(out), _p(_red_scratch(x.shape[0], x.device)), x.shape[1], x.shape[0], _dt(x), _stream()))
    return out


def quantile_range(chain, alpha=0.05):
    """Q(1 - alpha/2) - Q(alpha/2) of every column of a float64 [nsamples, nparams] tensor on the device
    (pxmcmc/uncertainty.py:7-16; numpy.quantile's default method) -> float64 [nparams]."""
    require_gpu()
    c = chain if isinstance(chain, torch.Tensor) else as_device(np.asarray(chain, dtype=np.float64), _REAL)
    if c.dim() != 2 or c.dtype != _REAL:
        raise TypeError("quantile_range: a float64 [nsamples, nparams] array is expected")
    if not c.is_cuda:
        c = c.to(device())
    if c.stride(1) != 1:
        c = c.contiguous()
    out = torch.empty(c.shape[1], dtype=_REAL, device=c.device)
    check(lib.pxm_quantile_range(_p(c), c.shape[0], c.shape[1], c.stride(0), float(alpha), _p(out), _stream()))
    return out


def _dev_tensors(fn, what, *specs):
    """every (tensor, dtype, shape) of ``specs`` is a contiguous device tensor of that dtype and shape, or ``fn`` raises a
    TypeError that says ``what`` is expected"""
    for t, dt, shape in specs:
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
            raise TypeError("%s: %s" % (fn, what))


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


def reduce_l2(preds, data, invcov):
    """vdot(d, invcov d), d = data - preds (pxmcmc/mcmc.py:78-79) -> complex128 [C]."""
    p, _ = _batched(as_device(preds))
    n = p.shape[1]
    d = as_device(data, p.dtype).reshape(-1)
    ic = as_device(invcov).reshape(-1)
    if ic.is_complex() and not p.is_complex():
        raise TypeError("complex inverse covariance needs complex predictions")
    if d.numel() != n or ic.numel() != n:
        raise ValueError("data / invcov length mismatch")
    out = torch.empty(p.shape[0], dtype=_CPLX, device=p.device)
    check(lib.pxm_reduce_l2(_p(p), _p(d), _p(ic), int(ic.is_complex()), _p(out), _p(_red_scratch(p.shape[0], p.device)), n, p.shape[0], _dt(p), _stream()))
    return out


def reduce_vdot(a, b):
    """np.vdot(a, b) per chain -> complex128 [C]"""
    x, _ = _batched(as_device(a))
    y, _ = _batched(as_device(b, x.dtype))
    if x.shape != y.shape:
        raise ValueError("vdot: shape mismatch")
    out = torch.empty(x.shape[0], dtype=_CPLX, device=x.device)
    check(lib.pxm_reduce_vdot(_p(x), _p(y), _p(out), _p(_red_scratch(x.shape[0], x.device)), x.shape[1], x.shape[0], _dt(x), _stream()))
    return out


def logtransition(X1, X2, proxf, gradg, delta, lmda):
    """PxMALA.calc_logtransition, literal (pxmcmc/mcmc.py:281-289) -> complex128 [C]."""
    x1, _ = _batched(as_device(X1))
    x2, _ = _batched(as_device(X2, x1.dtype))
    px, _ = _batched(as_device(proxf, x1.dtype))
    g, _ = _batched(as_device(gradg, x1.dtype))
    dd, ds = _delta_args(delta, x1.shape[0], x1.device)
    out = torch.empty(x1.shape[0], dtype=_CPLX, device=x1.device)
    check(lib.pxm_logtransition(_p(x1), _p(x2), _p(px), _p(g), _p(dd), ds, float(lmda), _p(out), _p(_red_scratch(x1.shape[0], x1.device)), x1.shape[1], x1.shape[0], _dt(x1), _stream()))
    return out


def reduce_scratch_doubles(C_):
    return int(lib.pxm_reduce_scratch_doubles(int(C_)))


def pxmala_propose_scratch(C_, dev):
    """scratch of pxmala_propose for C_ chains (kept by the caller when the totals are deferred to pxmala_finish)"""
    return torch.empty(4 * int(lib.pxm_reduce_scratch_doubles(int(C_))), dtype=_REAL, device=dev)


def pxmala_propose(X, proxf, gradg, T, prior_weights, delta_dev, lmda, Xp, proxf_p, lt_out, prior_out, noise=None,
                   noise_complex=False, seed=0, chain0=0, it=0, iter_dev=None, noise64=False, scratch=None):
    """chain_step + soft + calc_logtransition(X, X') + prior(X') in one pass; writes into the given buffers
    (Xp, proxf_p [C, n]; lt_out complex128 [C]; prior_out float64 [C]).  lt_out = prior_out = None with a caller-owned
    ``scratch`` (pxmala_propose_scratch): the totals are left to pxmala_finish.  proxf = proxf_p = None: the prox arrays
    are neither read nor written (soft(X, T) is formed in the kernel)."""
    if (proxf is None) != (proxf_p is None):
        raise ValueError("pxmala_propose: proxf and proxf_p are given together or not at all")
    x, _ = _batched(X)
    Tv, Ts = _vecT(T, x.shape[1], x.device)
    w, wc = _noise_args(noise, x, noise_complex)
    wp = None if prior_weights is None else as_device(prior_weights, _REAL).reshape(-1)
    if (lt_out is None) != (prior_out is None) or (lt_out is None and scratch is None):
        raise ValueError("pxmala_propose: deferred totals need lt_out = prior_out = None and a caller-owned scratch")
    if scratch is None:
        scratch = pxmala_propose_scratch(x.shape[0], x.device)
    check(
        lib.pxm_pxmala_propose(
            _p(x), _p(proxf), _p(gradg), _p(Tv), Ts, _p(wp), _p(delta_dev), float(lmda), _p(w), wc | _nf(noise64), seed, chain0, int(it),
            _p(iter_dev), _p(Xp), _p(proxf_p), _p(lt_out), _p(prior_out), _p(scratch), x.shape[1], x.shape[0], _dt(x), _stream(),
        )
    )


def pxmala_accept(lt_pc, lt_cp, prior_p, L2_p, mu, logpi_c, L2_c, prior_c, accept, delta_dev, tune, lmda, u=None, seed=0,
                  chain0=0, it=0, iter_dev=None, acc_trace=None, delta_trace=None):
    """Metropolis test + state scalars + delta adaptation + traces on the device (pxmcmc/mcmc.py:244-260,277-279)."""
    C_ = accept.shape[0]
    uu = None if u is None else as_device(u, _REAL).reshape(-1)
    chunk = 0 if acc_trace is None else acc_trace.shape[0]
    check(
        lib.pxm_pxmala_accept(
            _p(lt_pc), _p(lt_cp), _p(prior_p), _p(L2_p), float(mu), _p(logpi_c), _p(L2_c), _p(prior_c), _p(uu), seed, chain0,
            int(it), _p(iter_dev), _p(accept), _p(delta_dev), int(bool(tune)), float(lmda), _p(acc_trace), _p(delta_trace),
            int(chunk), C_, _stream(),
        )
    )


def pxmala_finish(Xp, X, proxf_p, gradg_p, preds_p, data, invcov, propose_scratch, mu, lmda, logpi_c, L2_c, prior_c, accept,
                  delta_dev, tune, lt_pc_out, lt_cp_out, prior_p_out, L2_p_out, scratch, u=None, seed=0, chain0=0, it=0,
                  iter_dev=None, acc_trace=None, delta_trace=None, bump=None, T=None):
    """Reverse transition sum + L2 of the proposal in one grid, then totals (incl. the deferred ones of pxmala_propose) +
    Metropolis test + state scalars + delta adaptation + traces in one workgroup (pxmcmc/mcmc.py:239-260,277-279);
    ``scratch``: 2 * pxm_reduce_scratch_doubles(C) doubles, caller-owned; ``bump``: device iteration counter to advance;
    ``proxf_p = None`` with the threshold ``T``: proxf' = soft(X', T) is formed in the kernel instead of being read."""
    xp, _ = _batched(Xp)
    if proxf_p is None and T is None:
        raise ValueError("pxmala_finish: without proxf_p the threshold T is needed")
    Tv, Ts = _vecT(T, xp.shape[1], xp.device) if proxf_p is None else (None, 0.0)
    pp, _ = _batched(preds_p)
    nd = pp.shape[1]
    d = data.reshape(-1)
    ic = invcov.reshape(-1)
    if d.dtype != pp.dtype or d.numel() != nd or ic.numel() != nd or (ic.is_complex() and not pp.is_complex()):
        raise ValueError("pxmala_finish: data / invcov do not match the predictions")
    for t in (X, proxf_p, gradg_p):
        if t is not None and (t.shape != xp.shape or t.dtype != xp.dtype or not t.is_contiguous()):
            raise ValueError("pxmala_finish: state arrays must share shape, dtype and be contiguous")
    C_ = accept.shape[0]
    uu = None if u is None else as_device(u, _REAL).reshape(-1)
    chunk = 0 if acc_trace is None else acc_trace.shape[0]
    check(
        lib.pxm_pxmala_finish(
            _p(xp), _p(X), _p(proxf_p), _p(Tv), Ts, _p(gradg_p), xp.shape[1], _dt(xp), _p(pp), _p(d), _p(ic), int(ic.is_complex()), nd, _dt(pp),
            _p(propose_scratch), float(mu), float(lmda), _p(logpi_c), _p(L2_c), _p(prior_c), _p(uu), seed, chain0, int(it),
            _p(iter_dev), _p(accept), _p(delta_dev), int(bool(tune)), _p(acc_trace), _p(delta_trace), int(chunk), _p(lt_pc_out),
            _p(lt_cp_out), _p(prior_p_out), _p(L2_p_out), _p(scratch), _p(bump), C_, _stream(),
        )
    )


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


# ---- sparse measurement ----------------------------------------------------------------
class CsrMatrix:
    """A scipy.sparse matrix resident on the GPU in CSR form (int64 indptr, int32 indices, f64 / c128 values)."""

    def __init__(self, mat):
        import scipy.sparse as sp

        m = sp.csr_matrix(mat)
        m.sum_duplicates()
        m.sort_indices()
        self.shape = m.shape
        self.is_complex = np.iscomplexobj(m.data)
        dev = device()
        self.indptr = torch.from_numpy(m.indptr.astype(np.int64)).to(dev)
        self.indices = torch.from_numpy(m.indices.astype(np.int32)).to(dev)
        self.vals = torch.from_numpy(np.ascontiguousarray(m.data.astype(np.complex128 if self.is_complex else np.float64))).to(dev)
        self.nnz = int(m.nnz)

    def matvec(self, X):
        """[ncols] or [C, ncols] -> [nrows] or [C, nrows] (float64 stays float64 under a real matrix)"""
        x, squeeze = _batched(as_device(X))
        if self.is_complex and not x.is_complex():
            x = x.to(_CPLX)
        if x.shape[1] != self.shape[1]:
            raise AssertionError(f"expected length {self.shape[1]}, got {x.shape[1]}")
        out = torch.empty((x.shape[0], self.shape[0]), dtype=x.dtype, device=x.device)
        # chain batches gather from a chain-minor copy of the operand (caller-owned scratch, stream-ordered reuse)
        scratch = torch.empty(x.numel(), dtype=x.dtype, device=x.device) if x.shape[0] > 1 else None
        check(lib.pxm_csr_matvec(_p(self.indptr), _p(self.indices), _p(self.vals), int(self.is_complex), self.shape[0],
                                 self.shape[1], _p(x), _p(out), x.shape[0], _dt(x), _p(scratch), _stream()))
        return out[0] if squeeze else out


# ---- transform plans -------------------------------------------------------------------
_LIVE_PLANS = weakref.WeakSet()  # every ShtPlan / WavPlan with a live handle, whoever owns it (prior, user operator, ...)
_LIVE_LOCK = threading.Lock()     # plans may be created on one thread while a sampler on another polls the registry


def _register_plan(plan):
    with _LIVE_LOCK:
        _LIVE_PLANS.add(plan)


def live_plans():
    """the plans of this process that still hold a device handle: what a sampler polls for expired bounded waits"""
    with _LIVE_LOCK:
        plans = list(_LIVE_PLANS)
    return [pl for pl in plans if getattr(pl, "_h", None)]


class _Plan:
    """What the plan classes share: the device handle ``_h`` (made by ``create(*args, &h)``, listed in the live-plan
    registry, given back to ``destroy`` with the object), the batched call of a transform, and the device status word
    (``status_fn``) reported in the name ``label``."""

    def __init__(self, create, args, destroy, status_fn, label):
        self._destroy, self._status_fn, self._label = destroy, status_fn, label
        h = C.c_void_p()
        check(create(*args, C.byref(h)))
        self._h = h
        _register_plan(self)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:  # lib is None during interpreter shutdown
            self._destroy(h)
            self._h = None

    def _run(self, fn, x, n_in, n_out, out=None):
        x, squeeze = _batched(as_device(x, _CPLX))
        if x.shape[1] != n_in:
            raise AssertionError(f"expected length {n_in}, got {x.shape[1]}")
        if x.shape[0] > self.max_chains:
            raise ValueError("more chains than the plan was created for")
        if out is None:
            out = torch.empty((x.shape[0], n_out), dtype=_CPLX, device=x.device)
        elif out.shape != (x.shape[0], n_out) or out.dtype != _CPLX or not out.is_contiguous():
            raise ValueError("out= buffer has the wrong shape / dtype / layout")
        check(fn(self._h, _p(x), _p(out), x.shape[0], _stream()))
        return out[0] if squeeze else out

    def status(self, clear=False):
        """bit mask of the bounded device waits of this plan that expired (0 = none; include/pxmcmc_amd.h); synchronises"""
        return int(check(self._status_fn(self._h, int(bool(clear)), _stream())))

    def raise_on_fault(self, clear=True):
        """raise PxmError if a kernel of this plan reported an expired wait since the last check (``clear``: reset the word)"""
        raise_on_status(self.status(clear=clear), self._label)


class ShtPlan(_Plan):
    """MW spin spherical-harmonic transforms at bandlimit L (replaces the pyssht calls)."""

    def __init__(self, L, spin=0, max_chains=1):
        require_gpu()
        self.L, self.spin, self.max_chains = int(L), int(spin), int(max_chains)
        self.npix, self.nlm = L * (2 * L - 1), L * L
        super().__init__(lib.pxm_sht_plan_create, (self.L, self.spin, self.max_chains, 0), lib.pxm_sht_plan_destroy,
                         lib.pxm_sht_status, f"ShtPlan(L={self.L}, spin={self.spin})")

    def inverse(self, flm):
        return self._run(lib.pxm_sht_inverse, flm, self.nlm, self.npix)

    def forward(self, f):
        return self._run(lib.pxm_sht_forward, f, self.npix, self.nlm)

    def inverse_adjoint(self, f):
        return self._run(lib.pxm_sht_inverse_adjoint, f, self.npix, self.nlm)

    def forward_adjoint(self, flm):
        return self._run(lib.pxm_sht_forward_adjoint, flm, self.nlm, self.npix)

    def table_bytes(self, op):
        return int(lib.pxm_sht_table_bytes(self._h, op))

    def uses_recursion(self):
        """0, or 16 * ring blocks per wavefront + complex columns per order when inverse / inverse_adjoint take the
        table-free recursion kernels (csrc/sht_rec.hip) instead of the ring-table GEMM"""
        return int(check(lib.pxm_sht_uses_recursion(self._h)))


def _update_out(out, x):
    """the ``out=`` buffer of a fused step: fresh, or a distinct tensor of the state's shape"""
    if out is None:
        return torch.empty_like(x)
    if out.shape != x.shape or out.dtype != _CPLX or not out.is_contiguous() or out.data_ptr() == x.data_ptr():
        raise ValueError("out= buffer must be a distinct contiguous complex128 tensor of the state's shape")
    return out


def _preds_out(preds_out, x, n):
    """the ``preds_out=`` buffer of a fused step: fresh, or [chains of x][n]"""
    if preds_out is None:
        return torch.empty((x.shape[0], n), dtype=_CPLX, device=x.device)
    if preds_out.shape != (x.shape[0], n) or preds_out.dtype != _CPLX or not preds_out.is_contiguous():
        raise ValueError("preds_out= buffer has the wrong shape / dtype / layout")
    return preds_out


class _WaveletPlan(_Plan):
    """The four transforms of a wavelet plan: the entry points ``pxm_<_abi>_*`` between coefficient vectors [ncoefs] and
    images whose length is the attribute named by ``_image`` (``npix`` pixels, or ``nlm`` harmonic coefficients)."""

    def _fn(self, name):
        return getattr(lib, f"pxm_{self._abi}_{name}")

    @property
    def _nimg(self):
        return getattr(self, self._image)

    def synthesis(self, X, out=None):
        return self._run(self._fn("synthesis"), X, self.ncoefs, self._nimg, out=out)

    def synthesis_adjoint(self, f):
        return self._run(self._fn("synthesis_adjoint"), f, self._nimg, self.ncoefs)

    def analysis(self, f):
        return self._run(self._fn("analysis"), f, self._nimg, self.ncoefs)

    def analysis_adjoint(self, X):
        return self._run(self._fn("analysis_adjoint"), X, self.ncoefs, self._nimg)


class WavPlan(_WaveletPlan):
    """Axisymmetric scale-discretised wavelet transforms (replaces the pys2let calls).  ``spin``: spin of the images;
    the coefficients are spin-0 functions in the same layout whatever it is."""

    _abi, _image = "wav", "npix"

    def __init__(self, L, B, J_min, max_chains=1, spin=0):
        require_gpu()
        self.L, self.B, self.J_min, self.max_chains = int(L), float(B), int(J_min), int(max_chains)
        self.spin = int(spin)
        self.npix = L * (2 * L - 1)
        nscal = C.c_int64()
        self.ncoefs = int(check(lib.pxm_wav_ncoefs(self.L, self.B, self.J_min, C.byref(nscal))))
        self.nscal = int(nscal.value)
        super().__init__(lib.pxm_wav_plan_create_spin, (self.L, self.B, self.J_min, self.spin, self.max_chains, 0),
                         lib.pxm_wav_plan_destroy, lib.pxm_wav_status, f"WavPlan(L={self.L}, spin={self.spin})")

    def _update_args(self, x, T, noise, noise_complex, pairs, out):
        """the MYULA-update arguments of the fused steps: thresholds, noise (``pairs``: two real chains per complex slot,
        PXM_MODE_REAL_PAIRS) and the result buffer (fresh, or a distinct tensor of the state's shape)"""
        Tv, Ts = _vecT(T, self.ncoefs, x.device)
        w, wc = _pair_noise_args(noise, x) if pairs else _noise_args(noise, x, noise_complex)
        return Tv, Ts, w, wc, _update_out(out, x)

    def gradg_step(self, X, preds, data, invcov, T, delta, lmda, noise=None, noise_complex=False, seed=0, chain0=0, it=0, out=None,
                   pairs=False, noise64=False):
        """Fused calc_gradg + proxf + chain_step (pxmcmc/mcmc.py:158-160) for the synthesis setting.
        ``pairs``: every complex slot of X carries two real chains (PXM_MODE_REAL_PAIRS)."""
        x, squeeze = _batched(as_device(X, _CPLX))
        p, _ = _batched(as_device(preds, _CPLX))
        if x.shape[1] != self.ncoefs or p.shape[1] != self.npix or p.shape[0] != x.shape[0]:
            raise AssertionError("gradg_step: shape mismatch")
        d = as_device(data, _CPLX).reshape(-1)
        ic = as_device(invcov).reshape(-1)
        if d.numel() != self.npix or ic.numel() != self.npix:
            raise ValueError("data / invcov length mismatch")
        Tv, Ts, w, wc, out = self._update_args(x, T, noise, noise_complex, pairs, out)
        check(
            lib.pxm_wav_gradg_step(
                self._h, _p(x), _p(p), _p(d), _p(ic), int(ic.is_complex()), _p(Tv), Ts, float(delta), float(lmda),
                _p(w), wc | _nf(noise64), seed, chain0, it, _p(out), x.shape[0], _stream(),
            )
        )
        return out[0] if squeeze else out

    # ---- fused iteration for a diagonal inverse covariance (residual rings carried inside the plan) ----
    def _image_args(self, data, invcov):
        d = as_device(data, _CPLX).reshape(-1)
        ic = as_device(invcov).reshape(-1)
        if d.numel() != self.npix or ic.numel() != self.npix:
            raise ValueError("data / invcov length mismatch")
        return d, ic

    def image_init(self, preds, data, invcov):
        p, _ = _batched(as_device(preds, _CPLX))
        if p.shape[1] != self.npix or p.shape[0] > self.max_chains:
            raise AssertionError("image_init: shape mismatch")
        d, ic = self._image_args(data, invcov)
        check(lib.pxm_wav_image_init(self._h, _p(p), _p(d), _p(ic), int(ic.is_complex()), p.shape[0], _stream()))

    def image_step(self, X, data, invcov, T, delta, lmda, noise=None, noise_complex=False, seed=0, chain0=0, it=0,
                   out=None, preds_out=None, pairs=False, noise64=False):
        """calc_gradg + proxf + chain_step + forward of the new state; the residual rings of the current state come
        from the previous ``image_step`` / ``image_init`` on this plan."""
        x, squeeze = _batched(as_device(X, _CPLX))
        if x.shape[1] != self.ncoefs or x.shape[0] > self.max_chains:
            raise AssertionError("image_step: shape mismatch")
        d, ic = self._image_args(data, invcov)
        Tv, Ts, w, wc, out = self._update_args(x, T, noise, noise_complex, pairs, out)
        preds_out = _preds_out(preds_out, x, self.npix)
        check(
            lib.pxm_wav_image_step(
                self._h, _p(x), _p(d), _p(ic), int(ic.is_complex()), _p(Tv), Ts, float(delta), float(lmda),
                _p(w), wc | _nf(noise64), seed, chain0, it, _p(out), _p(preds_out), x.shape[0], _stream(),
            )
        )
        return (out[0], preds_out[0]) if squeeze else (out, preds_out)

    # ---- ring-space MYULA step (identity measurement + uniform inverse covariance) ----
    def ring_set_data(self, data):
        d = as_device(data, _CPLX).reshape(-1)
        if d.numel() != self.npix:
            raise ValueError("data length mismatch")
        check(lib.pxm_wav_ring_set_data(self._h, _p(d), _stream()))

    def ring_init(self, X):
        x, _ = _batched(as_device(X, _CPLX))
        if x.shape[1] != self.ncoefs or x.shape[0] > self.max_chains:
            raise AssertionError("ring_init: shape mismatch")
        check(lib.pxm_wav_ring_init(self._h, _p(x), x.shape[0], _stream()))

    def ring_step(self, X, w, T, delta, lmda, noise=None, noise_complex=False, seed=0, chain0=0, it=0, out=None, pairs=False,
                  noise64=False):
        """calc_gradg + proxf + chain_step + forward for a uniform inverse covariance ``w``; the rings of the
        new state stay inside the plan (``ring_preds`` materialises forward(X) when it is observed)."""
        x, squeeze = _batched(as_device(X, _CPLX))
        if x.shape[1] != self.ncoefs or x.shape[0] > self.max_chains:
            raise AssertionError("ring_step: shape mismatch")
        Tv, Ts, wn, wc, out = self._update_args(x, T, noise, noise_complex, pairs, out)
        w = complex(w)
        check(
            lib.pxm_wav_ring_step(
                self._h, _p(x), w.real, w.imag, _p(Tv), Ts, float(delta), float(lmda), _p(wn), wc | _nf(noise64), seed, chain0, it,
                _p(out), x.shape[0], _stream(),
            )
        )
        return out[0] if squeeze else out

    def ring_preds(self, C_, out=None):
        if out is None:
            out = torch.empty((C_, self.npix), dtype=_CPLX, device=device())
        check(lib.pxm_wav_ring_preds(self._h, _p(out), C_, _stream()))
        return out

    def table_bytes(self, op):
        return int(lib.pxm_wav_table_bytes(self._h, op))

    def exact_dft_scales(self):
        """scales whose 511-point rings the fused step transforms with the exact-length unit (csrc/dft_pfa.h); 0 = Bluestein"""
        return int(check(lib.pxm_wav_exact_dft_scales(self._h)))

    # ---- weak-lensing measurement fused with the synthesis (pxm_wav_wl_*) ----
    def wl_attach(self, pix2data, weight, ndata):
        """pix2data: int32 [npix] pixel -> index in the masked data vector (< 0 masked) or None; weight: float64
        [ndata] (WeakLensing.inv_cov) or None.  The plan keeps the tensors alive."""
        if pix2data is not None:
            pix2data = pix2data.to(device=device(), dtype=torch.int32).contiguous()
            if pix2data.numel() != self.npix:
                raise ValueError("pix2data must have one entry per pixel")
        if weight is not None:
            weight = as_device(weight, _REAL).reshape(-1)
            if weight.numel() != int(ndata):
                raise ValueError("weight must have one entry per datum")
        self._wl = (pix2data, weight, int(ndata))
        check(lib.pxm_wav_wl_attach(self._h, _p(pix2data), _p(weight), int(ndata)))

    def wl_uses_recursion(self):
        """non-zero when the attached spin-2 stage runs the table-free recursion kernels (csrc/sht_rec.hip)"""
        return int(check(lib.pxm_wav_wl_uses_recursion(self._h)))

    def wl_forward(self, X, out=None):
        x, squeeze = _batched(as_device(X, _CPLX))
        if x.shape[1] != self.ncoefs or x.shape[0] > self.max_chains:
            raise AssertionError("wl_forward: shape mismatch")
        nd = self._wl[2]
        if out is None:
            out = torch.empty((x.shape[0], nd), dtype=_CPLX, device=x.device)
        check(lib.pxm_wav_wl_forward(self._h, _p(x), _p(out), x.shape[0], _stream()))
        return out[0] if squeeze else out

    def wl_adjoint(self, gamma, data=None, invcov=None, out=None):
        g, squeeze = _batched(as_device(gamma, _CPLX))
        nd = self._wl[2]
        if g.shape[1] != nd or g.shape[0] > self.max_chains:
            raise AssertionError("wl_adjoint: shape mismatch")
        d = ic = None
        if data is not None:
            d = as_device(data, _CPLX).reshape(-1)
            ic = as_device(invcov).reshape(-1)
            if d.numel() != nd or ic.numel() != nd:
                raise ValueError("data / invcov length mismatch")
        if out is None:
            out = torch.empty((g.shape[0], self.ncoefs), dtype=_CPLX, device=g.device)
        check(lib.pxm_wav_wl_adjoint(self._h, _p(g), _p(d), _p(ic), int(ic.is_complex()) if ic is not None else 0, _p(out),
                                     g.shape[0], _stream()))
        return out[0] if squeeze else out

    def workspace_nonfinite(self):
        """test aid: non-finite values anywhere in the plan's workspace (padding chains' columns included)"""
        return int(check(lib.pxm_wav_workspace_nonfinite(self._h, _stream())))

    # ---- live kernel timing of this plan (bench.py roofline leg) ----
    def profile_enable(self, max_launches):
        check(lib.pxm_wav_profile_enable(self._h, int(max_launches)))

    def profile_read_launches(self, cap):
        """per-launch (ms, algorithmic bytes, workgroups) of the bracketed ring-GEMM launches, in launch order"""
        import numpy as np

        ms, nb, wg, n = np.zeros(cap), np.zeros(cap), np.zeros(cap, dtype=np.int32), C.c_int64()
        check(lib.pxm_wav_profile_read_launches(self._h, ms.ctypes.data, nb.ctypes.data, wg.ctypes.data, int(cap), C.byref(n)))
        k = min(int(n.value), cap)
        return ms[:k], nb[:k], wg[:k]

    def profile_read(self):
        """(gemm: ms, launches, algorithmic bytes, flops), (grouped phi-DFT: ms, launches, algorithmic bytes)"""
        ms, nl, nb, nf = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        check(lib.pxm_wav_profile_read(self._h, C.byref(ms), C.byref(nl), C.byref(nb), C.byref(nf)))
        dms, dnl, dnb = C.c_double(), C.c_int64(), C.c_double()
        check(lib.pxm_wav_profile_read_dft(self._h, C.byref(dms), C.byref(dnl), C.byref(dnb)))
        return (ms.value, nl.value, nb.value, nf.value), (dms.value, dnl.value, dnb.value)


class DirWavPlan(_WaveletPlan):
    """Directional (N = dirs >= 1) scale-discretised wavelet transforms, spin 0 (replaces the pys2let calls with N > 1;
    include/pxmcmc_amd.h, pxm_dwav_*).  Layout [scaling | j = J_min .. J_max], block j = 2N - 1 orientation planes of
    the MW grid at bl_j.  With N = 1 it computes what :class:`WavPlan` computes (without WavPlan's fused sampler steps)."""

    _abi, _image = "dwav", "npix"

    def __init__(self, L, B, J_min, N, max_chains=1):
        require_gpu()
        self.L, self.B, self.J_min, self.N, self.max_chains = int(L), float(B), int(J_min), int(N), int(max_chains)
        self.npix = L * (2 * L - 1)
        nscal = C.c_int64()
        self.ncoefs = int(check(lib.pxm_dwav_ncoefs(self.L, self.B, self.J_min, self.N, C.byref(nscal))))
        self.nscal = int(nscal.value)
        super().__init__(lib.pxm_dwav_plan_create, (self.L, self.B, self.J_min, self.N, self.max_chains, 0),
                         lib.pxm_dwav_plan_destroy, lib.pxm_dwav_status, f"DirWavPlan(L={self.L}, N={self.N})")

    def table_bytes(self):
        """device bytes of the tables the plan reads (inner Wigner tables + its own weights and phases)"""
        return int(lib.pxm_dwav_table_bytes(self._h))

    def info(self):
        """(items, split workgroups per chain, gamma workgroups per chain)"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(lib.pxm_dwav_plan_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value


class HarmWavPlan(_WaveletPlan):
    """Harmonic-space scale-discretised wavelet transforms (replaces pys2let's analysis_lm2lmn / synthesis_lmn2lm and
    their adjoints; include/pxmcmc_amd.h, pxm_hwav_*).  Inputs and outputs are spherical-harmonic coefficients: f_lm
    [L*L] and the layout [scaling: bl_0^2 | j = J_min .. J_max: n = -(N-1), .., N-1: bl_j^2 each] (DESIGN.md section
    13).  N > 1 at spin 0 only."""

    _abi, _image = "hwav", "nlm"

    def __init__(self, L, B, J_min, N=1, spin=0, max_chains=1):
        require_gpu()
        self.L, self.B, self.J_min, self.N, self.max_chains = int(L), float(B), int(J_min), int(N), int(max_chains)
        self.spin = int(spin)
        self.nlm = self.L * self.L
        nscal = C.c_int64()
        self.ncoefs = int(check(lib.pxm_hwav_ncoefs(self.L, self.B, self.J_min, self.N, C.byref(nscal))))
        self.nscal = int(nscal.value)
        super().__init__(lib.pxm_hwav_plan_create, (self.L, self.B, self.J_min, self.N, self.spin, self.max_chains, 0),
                         lib.pxm_hwav_plan_destroy, lib.pxm_hwav_status,
                         f"HarmWavPlan(L={self.L}, N={self.N}, spin={self.spin})")

    def info(self):
        """(items, split workgroups per chain, most items with a non-zero weight at one degree)"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(lib.pxm_hwav_plan_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def myula_step(self, X, data, invcov, kernel, T, delta, lmda, noise_complex=False, seed=0, chain0=0, it=0, iter_dev=None,
                   out=None, preds_out=None, noise64=False):
        """One MYULA iteration of the synthesis setting with a measurement diagonal in (l, m) (``kernel``: None for the
        identity, else WeakLensingHarmonic's k_l) and a diagonal inverse covariance; returns (X', forward(X')).  Noise:
        the Philox stream of :func:`myula_step` at iteration ``it`` (+ ``iter_dev`` on the device)."""
        x, squeeze = _batched(as_device(X, _CPLX))
        if x.shape[1] != self.ncoefs or x.shape[0] > self.max_chains:
            raise AssertionError("myula_step: shape mismatch")
        d = as_device(data, _CPLX).reshape(-1)
        ic = as_device(invcov).reshape(-1)
        if d.numel() != self.nlm or ic.numel() != self.nlm:
            raise ValueError("data / invcov length mismatch")
        k = None
        if kernel is not None:
            k = as_device(kernel, _REAL).reshape(-1)
            if k.numel() != self.nlm:
                raise ValueError("kernel length mismatch")
        Tv, Ts = _vecT(T, self.ncoefs, x.device)
        out, preds_out = _update_out(out, x), _preds_out(preds_out, x, self.nlm)
        check(
            lib.pxm_hwav_myula_step(
                self._h, _p(x), _p(d), _p(ic), int(ic.is_complex()), _p(k), _p(Tv), Ts, float(delta), float(lmda),
                int(bool(noise_complex)) | _nf(noise64), seed, chain0, it, _p(iter_dev), _p(out), _p(preds_out), x.shape[0],
                _stream(),
            )
        )
        return (out[0], preds_out[0]) if squeeze else (out, preds_out)


# ---- device-resident iteration counter (HIP-graph replay) -----------------------------------
class IterCounter:
    """A device int64 registered as the Philox iteration counter of ONE wavelet plan for the lifetime of the
    object.  A plan holds one live counter: a second engine on the same plan (two samplers built on one
    ForwardOperator) raises ``PxmError`` until the first has stopped; ``close`` only releases the registration if
    it is still this object's."""

    def __init__(self, plan, start=0):
        self.plan = plan
        self.t = torch.full((1,), int(start), dtype=torch.int64, device=device())
        check(lib.pxm_wav_set_iter_counter(plan._h, C.c_void_p(self.t.data_ptr())))
        self.active = True

    def set(self, value):
        self.t.fill_(int(value))

    def add(self, inc=1):
        check(lib.pxm_wav_iter_counter_add(self.plan._h, int(inc), _stream()))

    def close(self):
        if self.active:
            if getattr(self.plan, "_h", None):
                lib.pxm_wav_release_iter_counter(self.plan._h, C.c_void_p(self.t.data_ptr()))
            self.active = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class capture_scope:
    """Tells the library that a stream capture is (about to be) in progress: plan teardown inside the scope only
    queues its frees (include/pxmcmc_amd.h, pxm_capture_begin / pxm_capture_end)."""

    def __enter__(self):
        check(lib.pxm_capture_begin())
        return self

    def __exit__(self, *exc):
        lib.pxm_capture_end()
        return False


def tables_trim():
    """free every cached ring table no live plan holds (the cache is per device and shared by plans); MiB released"""
    return int(check(lib.pxm_tables_trim()))


def noise_bits():
    """32: the precision of the Box-Muller step of the device noise stream WITHOUT the flag (the samplers of mcmc.py pass
    the flag by default: ``noise_bits=64``); every noise-drawing call takes
    ``noise64=True`` for the double-precision evaluation (PXM_NOISE_F64, include/pxmcmc_amd.h)"""
    return int(lib.pxm_noise_bits())


# ---- host helpers ------------------------------------------------------------------------
def j_max(L, B):
    return int(check(lib.pxm_j_max(int(L), float(B))))


def wav_bandlimits(L, B, J_min):
    buf = (C.c_int * 64)()
    n = check(lib.pxm_wav_bandlimits(int(L), float(B), int(J_min), buf, 64))
    return [int(buf[i]) for i in range(n)]


def tiling_axisym(L, B, J_min):
    J = j_max(L, B)
    k0 = np.zeros(L)
    k = np.zeros((J + 1, L))
    check(lib.pxm_tiling_axisym(int(L), float(B), int(J_min), k0.ctypes.data, k.ctypes.data))
    return k0, k


def mw_ring_weights(L):
    q = np.zeros(L)
    check(lib.pxm_mw_ring_weights(int(L), q.ctypes.data))
    return q
