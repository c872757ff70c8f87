"""MYULA (pxmcmc/mcmc.py:143-201) and its four engine builders: generic, fused wavelet, fused harmonic, eager."""
import numpy as np
import torch

from .. import ops
from ..measurements import Identity, WeakLensingHarmonic
from ..transforms import SphericalWaveletTransform
from .base import PxMCMC
from .engine import Engine, _Counter
from .params import PxMCMCParams


class MYULA(PxMCMC):
    """The MYULA chain (pxmcmc/mcmc.py:143-201)."""

    def __init__(self, forward, prox, mcmcparams=PxMCMCParams(), **kwargs):
        super().__init__(forward, prox, mcmcparams, **kwargs)
        self._own_step = type(self).chain_step is not MYULA.chain_step  # a subclass's chain_step: called as it is
        self._pairs = False

    def _fusable_wavelet(self):
        f = self.forward
        return (
            getattr(f, "setting", None) == "synthesis"
            and hasattr(getattr(f, "invcov", None), "diag")  # (a full covariance matrix goes through the generic kernels)
            and type(f).calc_gradg.__qualname__.startswith("ForwardOperator")
            and isinstance(getattr(f, "transform", None), SphericalWaveletTransform)
            and f.transform.dirs == 1  # (the fused steps are WavPlan's: axisymmetric only)
            and not f.transform.harmonic  # (... and pixel space)
            and isinstance(getattr(f, "measurement", None), Identity)
            and f.measurement.ndata == f.measurement.npix
            and self._stock_prox
            and not self._own_step
        )

    def _fusable_harmonic(self):
        """the fused harmonic step (HarmWavPlan.myula_step) applies: synthesis, a harmonic SphericalWaveletTransform, a
        measurement diagonal in (l, m) at its bandlimit -- exactly Identity(L^2, L^2) or WeakLensingHarmonic(L) -- a diagonal
        inverse covariance, the stock prox and no subclass chain_step.  Returns the measurement kernel (None: identity), or
        False."""
        f = self.forward
        tr, ms = getattr(f, "transform", None), getattr(f, "measurement", None)
        if not (
            getattr(f, "setting", None) == "synthesis"
            and hasattr(getattr(f, "invcov", None), "diag")
            and type(f).calc_gradg.__qualname__.startswith("ForwardOperator")
            and type(f).forward.__qualname__.startswith("ForwardOperator")
            and isinstance(tr, SphericalWaveletTransform)
            and tr.harmonic
            and self._stock_prox
            and not self._own_step
            and f.invcov.diag.numel() == tr.L ** 2
        ):
            return False
        if type(ms) is Identity and ms.ndata == ms.npix == tr.L ** 2:
            return None
        if type(ms) is WeakLensingHarmonic and ms.L == tr.L:
            return ms.kernel_dev
        return False

    def _advance(self, X, preds, i, delta=None):
        """one MYULA update X -> X_prop (pxmcmc/mcmc.py:158-160), fused where the operators allow"""
        delta = self.delta if delta is None else delta
        if self._pairs:  # X, preds are pair-packed [ceil(C/2), .]
            noise = self._host_noise_pairs(X) if self.rng == "numpy" else None
            return self._pair_plan.gradg_step(
                X, preds, self._pair_data, self.forward.invcov.diag, self.prior.T_dev, delta, self.lmda, noise=noise,
                seed=self.seed, chain0=self.chain_offset, it=i, pairs=True, noise64=self.noise64,
            )
        noise = self._host_noise(X) if self.rng == "numpy" else None
        kw = dict(noise=noise, noise_complex=bool(self.complex), seed=self.seed, chain0=self.chain_offset, it=i,
                  noise64=self.noise64)
        if self._fused_wav:
            f = self.forward
            return f.transform._plan.gradg_step(
                X, preds, f.data_dev_c128, f.invcov.diag, self.prior.T_dev, delta, self.lmda, **kw
            )
        gradg = ops.as_device(self.forward.calc_gradg(preds), X.dtype)
        if self._fused_prox:
            return ops.myula_step(X, gradg, self.prior.T_dev, delta, self.lmda, **kw)
        proxf = ops.as_device(self.prior.proxf(X), X.dtype)
        if self._own_step:
            return ops.as_device(self.chain_step(X, proxf, gradg), X.dtype)
        return ops.chain_step(X, proxf, gradg, delta, self.lmda, **kw)

    def _prepare(self):
        self._fused_wav = self._fusable_wavelet() and isinstance(self.delta, float)
        kernel = self._fusable_harmonic() if isinstance(self.delta, float) else False
        self._fused_harm = kernel is not False
        self._harm_kernel = kernel if self._fused_harm else None
        self._fused_prox = self._stock_prox and not self._own_step
        # the calls of the reference's loop, one by one: host noise, a tensor delta or a subclass's chain_step (and,
        # without graph replay, the operators that have no fused step)
        self._eager_only = self.rng == "numpy" or not (
            self._fused_wav or self._fused_harm or (self.use_graph and isinstance(self.delta, float) and not self._own_step))
        self._it = 0
        self._pairs = False

    # ---- two real chains per complex slot (real data, real state) ---------------------------------
    def _pairs_ok(self, X):
        """The reference's state is real-valued (stored as complex128 with a zero imaginary part) when the
        data, the inverse covariance and the start point are real and params.complex is False."""
        f = self.forward
        return bool(
            self._fused_wav and self.real_pairs and not self.complex
            and self.forward.transform.spin == 0  # (a spin-s image is never real: the pair mode is spin 0 only)
            and not f.data_dev.is_complex() and not f.invcov.diag.is_complex()
            and (not X.is_complex() or not bool((X.imag != 0).any()))
        )

    def _pairs_start(self):
        tr = self.forward.transform
        Cs = (self.nchains + 1) // 2
        if getattr(self, "_pair_plan", None) is None or self._pair_plan.max_chains != Cs:
            self._pair_plan = ops.WavPlan(tr.L, tr.B, tr.J_min, max_chains=Cs)  # tables are shared with tr._plan
        d = self.forward.data_dev.to(torch.float64)
        self._pair_data = torch.complex(d, d).contiguous()  # both chains of a slot see the same data
        self._pairs = True

    def _pack(self, X):
        """[C, n] (real-valued) -> [ceil(C/2), n] complex128: chain 2c + i chain 2c+1"""
        re = X.real if X.is_complex() else X
        if re.shape[0] % 2:
            re = torch.cat((re, re[-1:]))  # odd chain count: the last slot's partner is a discarded copy
        return torch.complex(re[0::2].contiguous(), re[1::2].contiguous())

    def _unpack(self, Xp):
        """inverse of _pack, returned as complex128 [C, n] (the reference's state dtype)"""
        Cs, n = Xp.shape
        out = torch.stack((Xp.real, Xp.imag), dim=1).reshape(2 * Cs, n)[: self.nchains]
        return out.to(torch.complex128)

    def _host_noise_pairs(self, Xp):
        """the reference's draw order (one randn(N) per chain, pxmcmc/mcmc.py:193) as a real [2 slots, N] array"""
        Cs, N = Xp.shape
        w = np.zeros((2 * Cs, N))
        for c in range(self.nchains):
            w[c] = np.random.randn(N)
        return ops.as_device(w)

    # ---- stepping engines ---------------------------------------------------------------------------------------
    def _engine_start(self, X, preds, i0):
        """Static ping-pong state (XA, XB, P), an iteration counter and, with the Philox stream, captured graphs of 2 and
        2 * GRAPH_PAIRS iterations"""
        self._engine_stop()  # an engine left over from an interrupted run gives its counter / buffers back first
        if self._eager_only:
            return self._engine_start_eager(X, preds, i0)
        if self._fused_wav:
            return self._engine_start_fused(X, preds, i0)
        if self._fused_harm:
            return self._engine_start_harmonic(X, preds, i0)
        f = self.forward
        delta, lmda = float(self.delta), self.lmda

        def step(eng, src, dst):
            # the reference's four calls (pxmcmc/mcmc.py:158-163) on the operators' own plans
            kw = dict(noise_complex=bool(self.complex), seed=self.seed, chain0=self.chain_offset, it=0,
                      iter_dev=eng.cnt.t, noise64=self.noise64)
            gradg = ops.as_device(f.calc_gradg(eng.P), src.dtype)
            if self._fused_prox:
                ops.myula_step(src, gradg, self.prior.T_dev, delta, lmda, out=dst, **kw)
            else:
                proxf = ops.as_device(self.prior.proxf(src), src.dtype)
                ops.chain_step(src, proxf, gradg, delta, lmda, out=dst, **kw)
            eng.P.copy_(ops.as_device(f.forward(dst)))
            eng.cnt.add(1)

        return self._engine_start_generic(X, preds, i0, step, lazy=False, graph_ok=True)

    def _engine_start_fused(self, X, preds, i0):
        """The fused wavelet steps of WavPlan, on the plan's registered iteration counter"""
        f = self.forward
        plan, data = f.transform._plan, f.data_dev_c128
        if self._pairs:  # two real chains per complex slot: X, preds are carried pair-packed
            plan, data = self._pair_plan, self._pair_data
            X, preds = self._pack(X), self._pack(preds)
        # per-plan device counter: the steps below read it at execution time
        eng = self._eng = Engine(X, preds, ops.IterCounter(plan, i0), plan=plan, pairs=self._pairs, unpack=self._unpack)
        d, T, delta, lmda = f.invcov.diag, self.prior.T_dev, float(self.delta), self.lmda
        # params.complex: randn + 1j randn (pxmcmc/mcmc.py:193-195) -> PXM_MODE_CPLX_NOISE in the fused epilogues
        kw = dict(noise_complex=bool(self.complex), seed=self.seed, chain0=self.chain_offset, it=0, pairs=self._pairs,
                  noise64=self.noise64)
        # Uniform inverse covariance (scalar sig_d): the image-space residual is applied on the rings and the
        # L-level iDFT/DFT pair between forward() and calc_gradg() drops out (pxm_wav_ring_step); preds is
        # then formed only when it is observed.
        eng.ring = bool(self.ring_shortcut and d.numel() > 0 and bool((d == d[0]).all()))
        if eng.ring:
            w = complex(d[0].item())
            plan.ring_set_data(data)
            eng.reset = lambda: plan.ring_init(eng.XA)  # plan-carried state of (XA, P)
            eng.cnt0 = lambda i: i - 1  # ring_step advances the counter itself, before using it
            eng.form_preds = lambda X: plan.ring_preds(eng.P.shape[0], out=eng.P)  # of the carried rings
            eng.one = lambda src, dst: plan.ring_step(src, w, T, delta, lmda, out=dst, **kw)
        else:
            eng.reset = lambda: plan.image_init(eng.P, data, d)  # residual rings of the state, carried by the plan

            def one(src, dst):
                # calc_gradg + proxf + chain_step + forward of the new state (preds written in place)
                plan.image_step(src, data, d, T, delta, lmda, out=dst, preds_out=eng.P, **kw)
                eng.cnt.add(1)

            eng.one = one
        eng.reset()
        return eng.ready(X, preds, i0, self.use_graph)

    def _engine_start_harmonic(self, X, preds, i0):
        """The fused harmonic step of HarmWavPlan: the whole iteration, preds of the new state included, in one kernel that
        reads the iteration number from the engine's device counter"""
        f = self.forward
        plan = f.transform._plan
        X = ops.as_device(X, torch.complex128).contiguous()
        preds = ops.as_device(preds, torch.complex128)
        eng = self._eng = Engine(X, preds, _Counter(i0), plan=plan)
        data, d, T, delta, lmda, k = f.data_dev_c128, f.invcov.diag, self.prior.T_dev, float(self.delta), self.lmda, self._harm_kernel
        kw = dict(noise_complex=bool(self.complex), seed=self.seed, chain0=self.chain_offset, noise64=self.noise64)

        def one(src, dst):
            plan.myula_step(src, data, d, k, T, delta, lmda, iter_dev=eng.cnt.t, out=dst, preds_out=eng.P, **kw)
            eng.cnt.add(1)

        eng.one = one
        return eng.ready(X, preds, i0, self.use_graph)

    def _engine_start_eager(self, X, preds, i0):
        """The engine of _eager_only: the calls of the reference's loop, iteration by iteration -- _advance with the
        host iteration number (host noise in the reference's draw order), then forward (the synthesis of the
        pair-packed state)"""
        if self._pairs:
            X, preds = self._pack(X), self._pack(preds)
        eng = self._eng = Engine(X, preds, _Counter(i0, host=True), pairs=self._pairs, unpack=self._unpack)
        forward = self._pair_plan.synthesis if self._pairs else (lambda X: ops.as_device(self.forward.forward(X)))

        def one(src, dst):
            X_prop = self._advance(src, eng.P, eng.cnt.i)
            dst.copy_(X_prop)
            eng.P.copy_(forward(X_prop))
            eng.cnt.add(1)

        eng.one = one
        return eng.ready(X, preds, i0, graph_ok=False)

    def run(self, start_point=None):
        """Run the algorithm (pxmcmc/mcmc.py:150-183)."""
        self._prepare()
        X_curr, curr_preds = self._initial_sample(start_point)
        if self._pairs_ok(X_curr):
            self._pairs_start()
        return self._run_engine(X_curr, curr_preds)

    def chain_step(self, X, proxf, gradg):
        """
        Takes a step in the chain (pxmcmc/mcmc.py:185-201):
        ``(1 - delta/lmda) X + (delta/lmda) proxf - delta gradg + sqrt(2 delta) w``.
        """
        x = ops.as_device(X)
        if self.rng == "numpy":
            noise = self._host_noise(x if x.dim() == 2 else x[None])
        else:
            noise = None
            self._it = getattr(self, "_it", 0) + 1
        out = ops.chain_step(
            x, proxf, gradg, self.delta, self.lmda, noise=noise, noise_complex=bool(self.complex),
            seed=self.seed, chain0=self.chain_offset, it=getattr(self, "_it", 0), noise64=self.noise64,
        )
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()
