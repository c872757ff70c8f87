"""Local credible intervals from the MAP point, searched on the device (csrc/lci.hip)."""
import torch

from .._lib import LCI_POINTS, check, lib
from ._args import _REAL, _batched, _companion, _dev_tensors, _dt, _p, _scratch, _stream, _vecT, as_device


def lci_scratch(n, C_, dev):
    """scratch of the three ``lci_*`` calls for C_ slots of vectors up to n long"""
    return _lci_scratch_arg("lci_scratch", None, n, C_, dev)


def _lci_scratch_arg(fn, scratch, n, C_, dev):
    return _scratch(scratch, int(check(lib.pxm_lci_scratch_doubles(int(n), int(C_)))), dev, "%s: scratch is too small (lci_scratch)" % fn)


def _lci_pair(fn, a, b):
    x, _ = _batched(as_device(a))
    msg = "%s: the two arrays must share one non-empty [C, n] shape" % fn
    y = _companion(b, x, msg)
    if x.shape[1] < 1:
        raise ValueError(msg)
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
