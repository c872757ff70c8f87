"""Per-chain reductions and the quantile range of a saved chain (csrc/reduce.hip)."""
import numpy as np
import torch

from .._lib import check, lib, require_gpu
from ._args import _CPLX, _REAL, _batched, _companion, _data_invcov, _dt, _p, _scratch, _stream, as_device, device


def _red_scratch(C_, dev):
    """caller-owned scratch of the two-stage reductions (torch's caching allocator: stream-ordered reuse)"""
    return _scratch(None, reduce_scratch_doubles(C_), dev)


def reduce_l1(X, w=None):
    """sum |w X| per chain (pxmcmc/prior.py:28-35,83-84) -> float64 [C]."""
    x, _ = _batched(as_device(X))
    wv = None if w is None else as_device(w, _REAL).reshape(-1)
    if wv is not None and wv.numel() != x.shape[1]:
        raise ValueError("weight length mismatch")
    out = torch.empty(x.shape[0], dtype=_REAL, device=x.device)
    check(lib.pxm_reduce_l1(_p(x), _p(wv), _p(out), _p(_red_scratch(x.shape[0], x.device)), x.shape[1], x.shape[0], _dt(x), _stream()))
    return out


def reduce_l2(preds, data, invcov):
    """vdot(d, invcov d), d = data - preds (pxmcmc/mcmc.py:78-79) -> complex128 [C]."""
    p, _ = _batched(as_device(preds))
    n = p.shape[1]
    d, ic = _data_invcov(data, invcov, n, p.dtype, preds=p)
    out = torch.empty(p.shape[0], dtype=_CPLX, device=p.device)
    check(lib.pxm_reduce_l2(_p(p), _p(d), _p(ic), int(ic.is_complex()), _p(out), _p(_red_scratch(p.shape[0], p.device)), n, p.shape[0], _dt(p), _stream()))
    return out


def reduce_vdot(a, b):
    """np.vdot(a, b) per chain -> complex128 [C]"""
    x, _ = _batched(as_device(a))
    y = _companion(b, x, "vdot: shape mismatch")
    out = torch.empty(x.shape[0], dtype=_CPLX, device=x.device)
    check(lib.pxm_reduce_vdot(_p(x), _p(y), _p(out), _p(_red_scratch(x.shape[0], x.device)), x.shape[1], x.shape[0], _dt(x), _stream()))
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


def reduce_scratch_doubles(C_):
    return int(lib.pxm_reduce_scratch_doubles(int(C_)))
