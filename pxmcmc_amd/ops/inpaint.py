"""One iteration of segment inpainting for the hypothesis test of image structure (csrc/inpaint.hip)."""
import torch

from .._lib import check, lib
from ._args import _REAL, _batched, _companion, _dev_tensors, _dt, _p, _result, _scratch, _stream, as_device

_I32 = torch.int32


def inpaint_scratch(npix, C_, dev):
    """scratch of ``inpaint_step`` for C_ slots of images of npix pixels"""
    return _inpaint_scratch_arg(None, npix, C_, dev)


def _inpaint_scratch_arg(scratch, npix, C_, dev):
    return _scratch(scratch, int(check(lib.pxm_inpaint_scratch_doubles(int(npix), int(C_)))), dev,
                    "inpaint_step: scratch is too small (inpaint_scratch)")


def inpaint_step(y, x_prev, x_map, labels, region, tol2, done, iters, stat, out=None, scratch=None):
    """``x_next[c] = done[c] ? x_prev[c] : where(labels == region[c], y[c], x_map)`` (a label < 0 is in no region), and for
    every slot that is not done ``iters[c] += 1``, ``stat[c] = (sum |x_next - x_prev|^2, sum |x_next|^2)`` and ``done[c] =
    stat[c, 0] <= tol2 * stat[c, 1]``.  ``y``, ``x_prev`` [C, npix] float64 or complex128; ``x_map``
    [npix] (taken in their dtype) and ``labels`` int32 [npix] are shared by the slots; ``region``, ``done``, ``iters`` int32
    [C] and ``stat`` float64 [C, 2] are device tensors, the last three updated in place.  Nothing is read back
    (capturable).  ``out``: the buffer of ``x_next``, distinct from ``x_prev`` and ``y``.  Returns ``x_next``."""
    xp, squeeze = _batched(as_device(x_prev))
    msg = "inpaint_step: y and x_prev must share one non-empty [C, npix] shape"
    yy = _companion(y, xp, msg)
    C_, npix = xp.shape
    if npix < 1 or C_ < 1:
        raise ValueError(msg)
    xm = as_device(x_map, xp.dtype).reshape(-1)
    if xm.numel() != npix:
        raise ValueError("inpaint_step: x_map must hold one value per pixel")
    _dev_tensors("inpaint_step", "labels must be a contiguous int32 [npix] device tensor", (labels, _I32, (npix,)))
    _dev_tensors("inpaint_step", "region, done and iters must be contiguous int32 [C] device tensors, stat float64 [C, 2]",
                 (region, _I32, (C_,)), (done, _I32, (C_,)), (iters, _I32, (C_,)), (stat, _REAL, (C_, 2)))
    tol2 = float(tol2)
    if not (tol2 >= 0.0 and tol2 != float("inf")):
        raise ValueError("inpaint_step: tol2 must be finite and >= 0")
    alias = "inpaint_step: out must be a contiguous device array of x_prev's shape and dtype, distinct from x_prev and y"
    if out is not None:
        out = out if out.dim() == 2 else out.unsqueeze(0)
        _result(out, xp.shape, xp.dtype, xp.device, alias, on_device=True, distinct_from=xp)
        _result(out, xp.shape, xp.dtype, xp.device, alias, on_device=True, distinct_from=yy)
    else:
        out = torch.empty_like(xp)
    scratch = _inpaint_scratch_arg(scratch, npix, C_, xp.device)
    check(lib.pxm_inpaint_step(_p(yy), _p(xp), _p(xm), _p(labels), _p(region), tol2, _p(out), _p(done), _p(iters), _p(stat),
                               _p(scratch), npix, C_, _dt(xp), _stream()))
    return out[0] if squeeze else out
