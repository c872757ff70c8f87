"""The transform plans -- spherical-harmonic, the phi-DFT stage alone, the ring-GEMM stage alone, HEALPix ring synthesis, axisymmetric, directional and
harmonic-space wavelets -- with the fused sampler steps of the wavelet plan, the live-plan registry, the device iteration counter and the capture scope
(csrc/sht_plan.hip, dft_plan.hip, gemm_plan.hip, healpix.hip, wav_plan.hip, wav_ops.hip, wav_wl.hip, dirwav.hip, harmwav.hip)."""
import ctypes as C
import threading
import weakref

import numpy as np
import torch

from .._lib import STATUS_PAIR_SYNC, PxmError, check, lib, require_gpu
from .host import gemm_report
from ._args import (_CPLX, _REAL, _batched, _data_invcov, _dev_tensors, _gemm_sides, _nf, _noise_args, _p, _pair_noise_args, _pixel_map, _result, _stream,
                    _vecT, as_device, device)


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
        out = _result(out, (x.shape[0], n_out), _CPLX, x.device, "out= buffer has the wrong shape / dtype / layout")
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


class DftPlan(_Plan):
    """The phi-DFT stage of the transforms on its own (include/pxmcmc_amd.h, pxm_dft_*): the rings <-> pixels launches of
    an SHT plan at bandlimit L without its ring tables.  Images are [C, L, 2L-1]; ``rings`` / ``pixels`` speak [C, L, 2L-1]
    (chain, ring t, order m = -(L-1) .. L-1) and permute with torch; ``rings_raw`` / ``pixels_raw`` work on the internal
    ring array [2L-1, Rp, Cp] (``ring_array``), padding rows and columns included; ``rings_raw_ex`` / ``pixels_raw_ex`` run
    the same launches with the pixel side (residual, pixel -> data map and weight, an image inside a longer chain) and the
    narrow ring arrays a weak-lensing or wavelet plan gives them."""

    def __init__(self, L, max_chains=1):
        require_gpu()
        self.L, self.max_chains = int(L), int(max_chains)
        self.n = 2 * self.L - 1
        self.Rp, self.Cp = -(-self.L // 16) * 16, -(-self.max_chains // 8) * 8
        super().__init__(lib.pxm_dft_plan_create, (self.L, self.max_chains), lib.pxm_dft_plan_destroy, lib.pxm_dft_status,
                         f"DftPlan(L={self.L})")

    def ring_array(self):
        """a zeroed ring array in the internal layout [2L-1, Rp, Cp]"""
        return torch.zeros((self.n, self.Rp, self.Cp), dtype=_CPLX, device=device())

    def _image(self, f, who):
        f = as_device(f, _CPLX)
        if f.dim() != 3 or tuple(f.shape[1:]) != (self.L, self.n):
            raise ValueError(f"{who}: the image must be [C, {self.L}, {self.n}]")
        if f.shape[0] > self.max_chains:
            raise ValueError("more chains than the plan was created for")
        return f

    def _ring_array(self, G, who):
        _dev_tensors(who, f"G must be a contiguous complex128 [{self.n}, {self.Rp}, {self.Cp}] device tensor",
                     (G, _CPLX, (self.n, self.Rp, self.Cp)))
        return G

    def rings_raw(self, f, G):
        """G[m + L - 1, t, c] = sum_p f[c, t, p] exp(-i m phi_p) for t < L, in place: columns c >= C are zeroed, rows
        t >= L are left as they are; returns G"""
        f, G = self._image(f, "rings_raw"), self._ring_array(G, "rings_raw")
        check(lib.pxm_dft_px2ring(self._h, _p(f), _p(G), f.shape[0], _stream()))
        return G

    def pixels_raw(self, G, C_, out=None):
        """f[c, t, p] = sum_m G[m + L - 1, t, c] exp(+i m phi_p) for the chains c < C_ -> [C_, L, 2L-1]"""
        G = self._ring_array(G, "pixels_raw")
        if not 1 <= int(C_) <= self.max_chains:
            raise ValueError("more chains than the plan was created for")
        out = _result(out, (int(C_), self.L, self.n), _CPLX, G.device, "out= buffer has the wrong shape / dtype / layout")
        check(lib.pxm_dft_ring2px(self._h, _p(G), _p(out), int(C_), _stream()))
        return out

    # ---- the same launches with the pixel side and the ring arrays of the weak-lensing and wavelet plans (pxm_dft_*_ex) ----
    def _px_side(self, who, f, G, gidx, gw, data=None, invcov=None):
        """the arguments of an _ex launch.  f: contiguous complex128 [C, chain_stride] device tensor (with ``gidx``: data
        space, chain_stride = ndata); G: contiguous complex128 [2L-1, Rp, ncol / 2] device tensor; ``gidx``: pixel -> entry
        of a chain (< 0: masked), every entry checked on the device to be < ndata; ``gw``, ``data``, ``invcov``: one entry
        per element of a chain.  -> (ncol, data, invcov, gidx, gw)"""
        cols = G.shape[2] if isinstance(G, torch.Tensor) and G.dim() == 3 else 0
        _dev_tensors(who, f"G must be a contiguous complex128 [{self.n}, {self.Rp}, ncol / 2] device tensor", (G, _CPLX, (self.n, self.Rp, cols)))
        chains, stride = tuple(f.shape) if isinstance(f, torch.Tensor) and f.dim() == 2 else (0, 0)
        _dev_tensors(who, "the pixel side must be a contiguous complex128 [C, chain_stride] device tensor", (f, _CPLX, (chains, stride)))
        if not 1 <= f.shape[0] <= self.max_chains:
            raise ValueError("more chains than the plan was created for")
        if (data is None) != (invcov is None):
            raise ValueError(f"{who}: data and invcov come together")
        if data is not None:
            data, invcov = _data_invcov(data, invcov, stride, _CPLX, preds=f)
        if gidx is not None:
            gidx = _pixel_map(gidx, self.L * self.n, stride, f"{who}: gidx must have one entry per pixel", f"{who}: gidx holds an index >= ndata")
        if gw is not None:
            gw = as_device(gw, _REAL).reshape(-1)
            if gw.numel() != stride:
                raise ValueError(f"{who}: gw must have one entry per datum")
        return 2 * cols, data, invcov, gidx, gw

    def rings_raw_ex(self, f, G, *, ring0=0, data=None, invcov=None, gidx=None, gw=None):
        """``rings_raw`` of the image at the elements [ring0, ring0 + L (2L-1)) of every chain of ``f`` [C, chain_stride], or
        with ``gidx`` of the image whose pixel e is entry gidx[e] of a chain of the data-space ``f`` [C, ndata] (masked:
        zero) times gw[gidx[e]]; with ``data`` / ``invcov`` (one entry per element of a chain) of invcov .* (f - data).  G:
        [2L-1, Rp, ncol / 2] with ncol = 2, 4, 6, 8 or a multiple of 16; returns G"""
        ncol, d, ic, gi, w = self._px_side("rings_raw_ex", f, G, gidx, gw, data, invcov)
        check(lib.pxm_dft_px2ring_ex(self._h, _p(f), f.shape[1], int(ring0), _p(d), _p(ic), int(ic.is_complex()) if ic is not None else 0,
                                     _p(gi), _p(w), f.shape[1] if gi is not None else 0, _p(G), ncol, f.shape[0], _stream()))
        return G

    def pixels_raw_ex(self, G, out, *, ring0=0, gidx=None, gw=None):
        """``pixels_raw`` of the chains c < C into the elements [ring0, ring0 + L (2L-1)) of every chain of ``out``
        [C, chain_stride], or with ``gidx`` pixel e into entry gidx[e] of a chain of the data-space ``out`` [C, ndata], times
        gw[gidx[e]] (masked pixels are dropped); every other element of ``out`` is left as it is; returns out"""
        ncol, _, _, gi, w = self._px_side("pixels_raw_ex", out, G, gidx, gw)
        check(lib.pxm_dft_ring2px_ex(self._h, _p(G), ncol, _p(out), out.shape[1], int(ring0), None, None, 0, _p(gi), _p(w),
                                     out.shape[1] if gi is not None else 0, out.shape[0], _stream()))
        return out

    def rings(self, f):
        """[C, L, 2L-1] image -> [C, L, 2L-1] rings (chain, ring, order)"""
        f = self._image(f, "rings")
        G = self.rings_raw(f, self.ring_array())
        return G[:, :self.L, :f.shape[0]].permute(2, 1, 0).contiguous()

    def pixels(self, G):
        """[C, L, 2L-1] rings (chain, ring, order) -> [C, L, 2L-1] image"""
        g = self._image(G, "pixels")  # (the same shape)
        raw = self.ring_array()
        raw[:, :self.L, :g.shape[0]] = g.permute(2, 1, 0)
        return self.pixels_raw(raw, g.shape[0])


class HpxPlan(_Plan):
    """HEALPix ring synthesis and its adjoint at bandlimit L (include/pxmcmc_amd.h, pxm_hpx_*): the
    exact maps between f_lm [L*L] and the values at the 12 nside^2 pixel centres of a RING-ordered map, spin ``spin`` in
    the ssht convention.  There is no HEALPix analysis here: ``synthesis_adjoint`` carries no quadrature weight."""

    def __init__(self, L, nside, spin=0, max_chains=1):
        require_gpu()
        self.L, self.nside, self.spin, self.max_chains = int(L), int(nside), int(spin), int(max_chains)
        self.nlm, self.npix = self.L * self.L, 12 * self.nside * self.nside
        super().__init__(lib.pxm_hpx_plan_create, (self.L, self.nside, self.spin, self.max_chains), lib.pxm_hpx_plan_destroy,
                         lib.pxm_hpx_status, f"HpxPlan(L={self.L}, nside={self.nside}, spin={self.spin})")

    def synthesis(self, flm, out=None):
        """[C, L*L] -> [C, 12 nside^2]: v_p = sum_lm sY_lm(theta_p, phi_p) f_lm"""
        return self._run(lib.pxm_hpx_synthesis, flm, self.nlm, self.npix, out=out)

    def synthesis_adjoint(self, v, out=None):
        """[C, 12 nside^2] -> [C, L*L]: f_lm = sum_p conj(sY_lm(theta_p, phi_p)) v_p"""
        return self._run(lib.pxm_hpx_synthesis_adjoint, v, self.npix, self.nlm, out=out)

    def table_bytes(self):
        """device bytes of the Legendre table and the twiddles the plan holds"""
        return int(lib.pxm_hpx_table_bytes(self._h))


class GemmPlan(_Plan):
    """The ring-GEMM stage of the transforms on its own (include/pxmcmc_amd.h, pxm_gemm_plan_*): ring tables, a workspace and
    ONE task list made of ``sides`` (dicts: ``kind`` one of ops.GEMM_KINDS, ``bl``, and optionally ``L`` the bandlimit of
    the harmonic-side array, ``two``, ``ks``, ``rs``, ``rows`` = (row_lo, row_hi), ``el_lo``, ``hd``, ``x_ncol``, ``y_ncol``,
    ``x_share``, ``y_share``), appended in order or, with ``pk`` 2 / 4, as one packed side or pair.  ``layout``, ``sides``,
    ``tasks`` and ``tables`` are ops.gemm_report of the plan; the caller fills the arrays with ``write``, runs the list and
    reads results, scratch block and counter back with ``read``."""

    def __init__(self, sides, spin=0, max_chains=8, pk=0):
        require_gpu()
        desc = _gemm_sides(sides, max_chains, pk)
        self.spin, self.max_chains, self.pk, self.n_sides = int(spin), int(max_chains), int(pk), len(sides)
        super().__init__(lib.pxm_gemm_plan_create, (self.spin, self.max_chains, self.pk, desc, self.n_sides), lib.pxm_gemm_plan_destroy,
                         None, f"GemmPlan(spin={self.spin}, sides={self.n_sides}, pk={self.pk})")
        rep = gemm_report(lambda what, side, out, cap: lib.pxm_gemm_plan_report(self._h, what, side, out, cap), self.n_sides)
        self.layout, self.sides, self.tasks, self.tables = rep["layout"], rep["sides"], rep["tasks"], rep["tables"]

    def status(self, clear=False):
        """0: the GEMM kernels have no bounded wait"""
        return 0

    def write(self, offset, src):
        """copies the float64 device tensor ``src`` into the workspace at ``offset`` (doubles)"""
        _dev_tensors("GemmPlan.write", "src must be a contiguous float64 device tensor", (src, _REAL, tuple(getattr(src, "shape", ()))))
        check(lib.pxm_gemm_plan_write(self._h, int(offset), _p(src), src.numel(), _stream()))

    def read(self, offset, n):
        """``n`` doubles of the workspace from ``offset`` on -> a fresh device tensor"""
        if int(n) < 0:
            raise ValueError("GemmPlan.read: negative length")
        out = torch.empty(int(n), dtype=_REAL, device=device())
        check(lib.pxm_gemm_plan_read(self._h, int(offset), _p(out), int(n), _stream()))
        return out

    def _table(self, side, which, n):
        if not 0 <= int(side) < self.n_sides:
            raise ValueError("GemmPlan: no such side")
        out = torch.empty(n, dtype=_REAL, device=device())
        if n:
            check(lib.pxm_gemm_plan_table_read(self._h, int(side), which, _p(out), n, _stream()))
        return out

    def table(self, side=0):
        """the tiled table of a side as the kernel streams it (layout: top of csrc/sht_gemm.hip; ``tables[side]``)"""
        return self._table(side, 0, self.tables[side]["n_tab"] if 0 <= int(side) < self.n_sides else 0)

    def pole(self, side=0):
        """the pole column b of a gram_split0 side, [Rp / 2 even degrees | Rp / 2 odd degrees] (empty for other kinds)"""
        return self._table(side, 1, self.tables[side]["n_pole"] if 0 <= int(side) < self.n_sides else 0)

    def run(self, C_, affine=None, bump=False):
        """launches the list once for ``C_`` chains; ``affine`` = (ns, w): the epilogue out = w (ns acc - data term);
        ``bump``: the counter at ``layout['off_counter']`` advances by one"""
        if not 1 <= int(C_) <= self.max_chains:
            raise ValueError("more chains than the plan was created for")
        ns, w = (0.0, 0.0) if affine is None else affine
        w = complex(w)
        check(lib.pxm_gemm_plan_run(self._h, int(C_), int(affine is not None), float(ns), w.real, w.imag, int(bool(bump)), _stream()))

    def counter(self):
        """the value of the 8-byte counter"""
        return int(self.read(self.layout["off_counter"], 1).view(torch.int64).item())


def _update_out(out, x):
    """the ``out=`` buffer of a fused step: fresh, or a distinct tensor of the state's shape"""
    return _result(out, x.shape, _CPLX, x.device, "out= buffer must be a distinct contiguous complex128 tensor of the state's shape",
                   distinct_from=x)


def _preds_out(preds_out, x, n):
    """the ``preds_out=`` buffer of a fused step: fresh, or [chains of x][n]"""
    return _result(preds_out, (x.shape[0], n), _CPLX, x.device, "preds_out= buffer has the wrong shape / dtype / layout")


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
        d, ic = _data_invcov(data, invcov, self.npix, _CPLX)
        Tv, Ts, w, wc, out = self._update_args(x, T, noise, noise_complex, pairs, out)
        check(
            lib.pxm_wav_gradg_step(
                self._h, _p(x), _p(p), _p(d), _p(ic), int(ic.is_complex()), _p(Tv), Ts, float(delta), float(lmda),
                _p(w), wc | _nf(noise64), seed, chain0, it, _p(out), x.shape[0], _stream(),
            )
        )
        return out[0] if squeeze else out

    # ---- fused iteration for a diagonal inverse covariance (residual rings carried inside the plan) ----
    def image_init(self, preds, data, invcov):
        p, _ = _batched(as_device(preds, _CPLX))
        if p.shape[1] != self.npix or p.shape[0] > self.max_chains:
            raise AssertionError("image_init: shape mismatch")
        d, ic = _data_invcov(data, invcov, self.npix, _CPLX)
        check(lib.pxm_wav_image_init(self._h, _p(p), _p(d), _p(ic), int(ic.is_complex()), p.shape[0], _stream()))

    def image_step(self, X, data, invcov, T, delta, lmda, noise=None, noise_complex=False, seed=0, chain0=0, it=0,
                   out=None, preds_out=None, pairs=False, noise64=False):
        """calc_gradg + proxf + chain_step + forward of the new state; the residual rings of the current state come
        from the previous ``image_step`` / ``image_init`` on this plan."""
        x, squeeze = _batched(as_device(X, _CPLX))
        if x.shape[1] != self.ncoefs or x.shape[0] > self.max_chains:
            raise AssertionError("image_step: shape mismatch")
        d, ic = _data_invcov(data, invcov, self.npix, _CPLX)
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

    def dft_stock(self):
        """whether the fused step runs stock MYULA updates (ops.dft_step_is_stock) on the STOCK kernel instantiation of the
        phi-DFT stage; False with PXM_DFT_STOCK=0 at creation"""
        return bool(check(lib.pxm_wav_dft_stock(self._h)))

    def mem_policy(self):
        """mask of the streams of the ring-space step that the plan's launches access non-temporally (csrc/mem_policy.h:
        bit 0 the X' stores of the fused phi-DFT step, on its STOCK instantiation); 0 with PXM_MEM_POLICY=0 at creation,
        when every launch takes the default-policy kernel instantiations"""
        return int(check(lib.pxm_wav_mem_policy(self._h)))

    def info(self):
        """what the plan's fused launches run on: exact-length DFT scales, STOCK instantiation, cache-policy mask"""
        return {"exact_dft_scales": self.exact_dft_scales(), "dft_stock": self.dft_stock(), "mem_policy": self.mem_policy()}

    # ---- weak-lensing measurement fused with the synthesis (pxm_wav_wl_*) ----
    def wl_attach(self, pix2data, weight, ndata):
        """pix2data: int32 [npix] pixel -> index in the masked data vector (< 0 masked) or None; weight: float64
        [ndata] (WeakLensing.inv_cov) or None.  The plan keeps the tensors alive."""
        if pix2data is not None:
            pix2data = _pixel_map(pix2data, self.npix, ndata, "pix2data must have one entry per pixel",
                                  "wl_attach: pix2data holds an index >= ndata")
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
            d, ic = _data_invcov(data, invcov, nd, _CPLX)
        if out is None:
            out = torch.empty((g.shape[0], self.ncoefs), dtype=_CPLX, device=g.device)
        check(lib.pxm_wav_wl_adjoint(self._h, _p(g), _p(d), _p(ic), int(ic.is_complex()) if ic is not None else 0, _p(out),
                                     g.shape[0], _stream()))
        return out[0] if squeeze else out

    def workspace_nonfinite(self):
        """test aid: non-finite values anywhere in the plan's workspace (padding chains' columns included)"""
        return int(check(lib.pxm_wav_workspace_nonfinite(self._h, _stream())))

    def workspace_read(self):
        """test aid: a copy of the plan's workspace (every ring and harmonic array of its stages), float64 on the device"""
        n = int(check(lib.pxm_wav_workspace_read(self._h, None, 0, _stream())))
        out = torch.empty(n, dtype=_REAL, device=device())
        check(lib.pxm_wav_workspace_read(self._h, _p(out), n, _stream()))
        return out

    # ---- live kernel timing of this plan (bench.py roofline leg) ----
    def profile_enable(self, max_launches):
        check(lib.pxm_wav_profile_enable(self._h, int(max_launches)))

    def profile_read_launches(self, cap):
        """per-launch (ms, algorithmic bytes, workgroups) of the bracketed ring-GEMM launches, in launch order"""
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

    # ---- test aids: the workspace and one stage at a time (pxm_dwav_workspace_*, pxm_dwav_run_stage) ----
    OPS = ("analysis", "analysis_adjoint", "synthesis", "synthesis_adjoint")  # op of run_stage, by index

    def layout(self):
        """the workspace (one complex128 array, offsets in elements) as ``dict(size, flm=(offset, elements), harm, pix,
        max_chains, items, blocks)``: ``items`` one dict per (block, n) item in plan order with the offset of chain 0 of its
        harmonic (``a_off``, ``a_n`` = bl^2 per chain) and pixel (``g_off``, ``g_n`` = bl (2 bl - 1) per chain) operand;
        ``blocks`` one dict per block of the gamma stage, ``goff_row`` the first entry of its row of ``goff``; ``goff`` the
        g-offset table as uploaded: per orientation of a block the offset of g_n in the pixel arena, -1 for a skipped pair"""
        n = int(check(lib.pxm_dwav_workspace_layout(self._h, None, 0)))
        w = (C.c_int64 * n)()
        check(lib.pxm_dwav_workspace_layout(self._h, w, n))
        w = [int(v) for v in w]
        ni, nb = w[5], w[6]
        items = [dict(zip(("block", "n", "bl", "a_off", "a_n", "g_off", "g_n"), w[8 + 8 * i:15 + 8 * i])) for i in range(ni)]
        o = 8 + 8 * ni
        blocks = [dict(zip(("coef_off", "npix", "nplanes", "nn", "blk0", "goff_row"), w[o + 8 * i:o + 8 * i + 6])) for i in range(nb)]
        return dict(size=w[0], flm=(w[1], w[2]), harm=w[3], pix=w[4], max_chains=w[7], items=items, blocks=blocks, goff=w[o + 8 * nb:])

    def write(self, offset, src):
        """copies the complex128 device tensor ``src`` into the workspace at ``offset`` (elements)"""
        _dev_tensors("DirWavPlan.write", "src must be a contiguous complex128 device tensor", (src, _CPLX, tuple(getattr(src, "shape", ()))))
        check(lib.pxm_dwav_workspace_write(self._h, int(offset), _p(src), src.numel(), _stream()))

    def read(self, offset=0, n=None):
        """``n`` elements of the workspace from ``offset`` on (default: to its end) -> a fresh complex128 device tensor"""
        n = self.layout()["size"] - int(offset) if n is None else int(n)
        if n < 0:
            raise ValueError("DirWavPlan.read: negative length")
        out = torch.empty(n, dtype=_CPLX, device=device())
        check(lib.pxm_dwav_workspace_read(self._h, int(offset), _p(out), n, _stream()))
        return out

    def run_stage(self, op, stage, x, C_):
        """enqueues stage 0 .. 3 of operator ``op`` (a name of ``OPS``) alone for ``C_`` chains, as the operator runs it: the
        SHT at L (``x``: the images f, read or written in place), the harmonic split / merge and the inner SHTs (``x``
        None), the gamma stage (``x``: the coefficients X, read or written in place).  ``x``: a contiguous complex128
        device tensor [rows >= C_, npix or ncoefs]; rows >= C_ are not touched."""
        op, stage = self.OPS.index(op), int(stage)
        if not 1 <= int(C_) <= self.max_chains:
            raise ValueError("more chains than the plan was created for")
        outer = stage == (0 if op in (0, 3) else 3)  # the stage that speaks images
        if stage in (0, 3):
            n = self.npix if outer else self.ncoefs
            rows = x.shape[0] if isinstance(x, torch.Tensor) and x.dim() == 2 else 0
            _dev_tensors("DirWavPlan.run_stage", f"x must be a contiguous complex128 [rows >= C, {n}] device tensor", (x, _CPLX, (rows, n)))
            if rows < int(C_):
                raise ValueError("DirWavPlan.run_stage: x has fewer rows than chains")
        else:
            x = None
        check(lib.pxm_dwav_run_stage(self._h, op, stage, _p(x), int(C_), _stream()))
        return x


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
        d, ic = _data_invcov(data, invcov, self.nlm, _CPLX)
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
