"""What every wrapper does to its arguments before the C-ABI call: tensors onto the device, pointers, and the checks the
wrappers share, each written once.  A helper that refuses takes the message it raises with, so every caller keeps its own
words; the exception class is the helper's.  Given contiguous device tensors of the right dtype -- how the stepping engine
and the captured graphs call the wrappers -- no helper here allocates, copies or synchronises."""
import ctypes as C

import numpy as np
import torch

from .._lib import GEMM_SIDE_INTS, MODE_REAL_PAIRS, NOISE_F64, require_gpu

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


# ---- the checks the wrappers share -------------------------------------------------------------------------------------------
def _companion(t, x, msg):
    """an array that goes with the state ``x`` (gradg, proxf, V, Y, b): batched, in x's dtype, of x's shape"""
    t, _ = _batched(as_device(t, x.dtype))
    if t.shape != x.shape:
        raise ValueError(msg)
    return t


def _data_invcov(data, invcov, n, dtype, preds=None):
    """``data`` (taken in ``dtype``) and the diagonal inverse covariance, flattened, each n long -> (d, ic); ``preds``: the
    predictions they are compared with, which must be complex when the inverse covariance is"""
    d = as_device(data, dtype).reshape(-1)
    ic = as_device(invcov)
    if preds is not None and ic.is_complex() and not preds.is_complex():
        raise TypeError("complex inverse covariance needs complex predictions")
    ic = ic.reshape(-1)
    if d.numel() != n or ic.numel() != n:
        raise ValueError("data / invcov length mismatch")
    return d, ic


def _pixel_map(gidx, npix, ndata, length_msg, range_msg):
    """a pixel -> data map (an entry < 0: masked pixel) -> contiguous int32 [npix] on the GPU whose every entry is < ndata.
    The range is checked here, on the device (one max() reduction, one synchronisation): the kernels index the data vector
    with the entries and the C-ABI cannot see them."""
    if not isinstance(gidx, torch.Tensor):
        gidx = torch.from_numpy(np.ascontiguousarray(np.asarray(gidx)))
    if gidx.numel() != npix:
        raise ValueError(length_msg)
    gidx = gidx.to(device=device()).reshape(-1)
    if npix and int(gidx.max()) >= int(ndata):  # (in the caller's integer type: before the narrowing to int32 can wrap it)
        raise ValueError(range_msg)
    return gidx.to(dtype=torch.int32).contiguous()


def _chain_vector(t, C_, dev, dtypes, msg, optional=False):
    """a per-chain device vector the kernel reads or updates in place: contiguous [C] of one of ``dtypes`` on ``dev``"""
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.shape != (C_,) or not t.is_contiguous() or t.device != dev:
        raise ValueError(msg)
    return t


def _table(t, dev, msg):
    """a table the kernel indexes by the iteration (beta, rho): a non-empty contiguous float64 vector on ``dev``; a sequence
    is uploaded"""
    t = t if isinstance(t, torch.Tensor) else as_device(np.atleast_1d(np.asarray(t, dtype=float)), _REAL)
    if t.dtype != _REAL or t.dim() != 1 or t.numel() < 1 or not t.is_contiguous() or t.device != dev:
        raise ValueError(msg)
    return t


def _result(out, shape, dtype, dev, msg, on_device=False, distinct_from=None):
    """a result buffer: fresh, or the caller's ``out`` when it is a contiguous tensor of that shape and dtype (``on_device``:
    and on ``dev``; ``distinct_from``: and not the memory of that input)"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if (out.shape != shape or out.dtype != dtype or not out.is_contiguous() or (on_device and out.device != dev)
            or (distinct_from is not None and out.data_ptr() == distinct_from.data_ptr())):
        raise ValueError(msg)
    return out


def _state_out(out, x):
    """the ``out=`` buffer a caller gave an elementwise step on the state ``x`` (one chain may come without the chain axis)"""
    return _result(out if out.dim() == 2 else out.unsqueeze(0), x.shape, x.dtype, x.device,
                   "out must be a contiguous device array of the state's shape and dtype", on_device=True)


def _scratch(scratch, n, dev, msg=None, any_layout=False):
    """scratch of n doubles: fresh, or the caller's float64 buffer of at least that many (contiguous unless ``any_layout``)"""
    if scratch is None:
        return torch.empty(n, dtype=_REAL, device=dev)
    if scratch.numel() < n or scratch.dtype != _REAL or not (any_layout or scratch.is_contiguous()):
        raise ValueError(msg)
    return scratch


def _dev_tensors(fn, what, *specs):
    """every (tensor, dtype, shape) of ``specs`` is a contiguous device tensor of that dtype and shape, or ``fn`` raises a
    TypeError that says ``what`` is expected"""
    for t, dt, shape in specs:
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
            raise TypeError("%s: %s" % (fn, what))


# ---- the sides of a GEMM-only plan ----------------------------------------------------------------------------------------------
GEMM_KINDS = ("inv", "fwd", "inv_adj", "fwd_adj", "gram", "gram_split", "gram_split0")  # TableKind of csrc/sht_tables.h
_GEMM_SIDE_KEYS = ("kind", "bl", "L", "two", "ks", "rs", "rows", "el_lo", "hd", "x_ncol", "y_ncol", "x_share", "y_share")


def _gemm_sides(sides, max_chains, pk):
    """the sides of ``GemmPlan`` / ``gemm_plan_geometry`` (dicts with ``kind`` and ``bl`` and any of the other keys of
    include/pxmcmc_amd.h, pxm_gemm_plan_create) -> the int array of the C-ABI, GEMM_SIDE_INTS per side"""
    if not isinstance(sides, (list, tuple)) or not sides or not all(isinstance(s, dict) for s in sides):
        raise TypeError("GemmPlan: sides must be a non-empty list of dicts")
    if int(pk) not in (0, 2, 4):
        raise ValueError("GemmPlan: pk must be 0, 2 or 4")
    if int(max_chains) < 1 or (pk and 2 * int(max_chains) > pk):
        raise ValueError("GemmPlan: max_chains must be >= 1, and at most pk / 2 in a packed list")
    out = (C.c_int * (GEMM_SIDE_INTS * len(sides)))()
    for i, s in enumerate(sides):
        unknown = set(s) - set(_GEMM_SIDE_KEYS)
        if unknown or "kind" not in s or "bl" not in s:
            raise ValueError(f"GemmPlan: side {i} needs kind and bl and knows {', '.join(_GEMM_SIDE_KEYS)}")
        kind = GEMM_KINDS.index(s["kind"]) if s["kind"] in GEMM_KINDS else s["kind"]
        if not isinstance(kind, int) or not 0 <= kind < len(GEMM_KINDS):
            raise ValueError(f"GemmPlan: side {i}: kind must be one of {', '.join(GEMM_KINDS)}")
        lo, hi = s.get("rows") or (0, 0)
        row = (kind, s["bl"], s.get("L", 0), bool(s.get("two")), bool(s.get("ks")), bool(s.get("rs")), lo, hi, s.get("el_lo", 0),
               bool(s.get("hd")), s.get("x_ncol", 0), s.get("y_ncol", 0), s.get("x_share", -1), s.get("y_share", -1), 0, 0)
        out[GEMM_SIDE_INTS * i:GEMM_SIDE_INTS * (i + 1)] = [int(v) for v in row]
    return out


# ---- step size and noise -------------------------------------------------------------------------------------------------------
def _delta_args(delta, C_, dev):
    if isinstance(delta, torch.Tensor):
        dd = delta.to(device=dev, dtype=_REAL).contiguous()
        if dd.numel() != C_:
            raise ValueError("per-chain delta must have one entry per chain")
        return dd, 0.0
    return None, float(delta)


def _nf(noise64):
    """PXM_NOISE_F64 flag of the noise-drawing entry points: the Philox stream's Box-Muller step in double precision"""
    return NOISE_F64 if noise64 else 0


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


def _pair_noise_args(noise, x):
    """PXM_MODE_REAL_PAIRS (two real chains per complex slot): injected noise is a real [2 * slots, N] array"""
    if noise is None:
        return None, MODE_REAL_PAIRS
    w = as_device(noise, _REAL)
    if w.dim() != 2 or w.shape != (2 * x.shape[0], x.shape[1]):
        raise ValueError("real-pair noise must be a float64 [2 * slots, N] array")
    return w, MODE_REAL_PAIRS


def _noise_group(noise, x, noise_complex, noise64, seed, chain0, it, iter_dev):
    """the noise arguments of the generic entry points, in the order of the C-ABI -> (w, (noise, noise_complex | PXM_NOISE_F64,
    seed, chain0, it, iter_dev)); the caller holds ``w`` (the injected noise on the device, or None) until its call has
    been made: the tuple carries only its address"""
    w, wc = _noise_args(noise, x, noise_complex)
    return w, (_p(w), wc | _nf(noise64), seed, chain0, it, _p(iter_dev))
