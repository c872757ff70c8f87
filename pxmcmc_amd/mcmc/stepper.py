"""What everything that steps on the posterior shares -- the samplers, FISTA and SAPG: operators and parameters, the
posterior pieces (L2, logPi, start point), the device status poll and one stepping :class:`~.engine.Engine`."""
import numpy as np
import torch
from scipy.stats import laplace

from .. import ops
from ..prior import _is_stock_l1
from ..transforms import SphericalWaveletTransform
from .engine import Engine, _Counter
from .params import PxMCMCParams


class Stepper:
    """
    :param forward: :class:`forward.ForwardOperator`-like object
    :param prior: prior object implementing ``prior`` and ``proxf``
    :param mcmcparams: :class:`PxMCMCParams`
    """

    _GRAPH_PAIRS = Engine.GRAPH_PAIRS
    _eng = None

    def __init__(self, forward, prior, mcmcparams=PxMCMCParams(), nchains=1, rng="philox", seed=0, chain_offset=0,
                 use_graph=True, ring_shortcut=True, real_pairs=True, noise_bits=64):
        self.forward = forward
        self.prior = prior
        for attr in mcmcparams.__dict__.keys():
            setattr(self, attr, getattr(mcmcparams, attr))
        if rng not in ("philox", "numpy"):
            raise ValueError("rng must be 'philox' or 'numpy'")
        self.nchains = int(nchains)
        self.rng = rng
        self.seed = int(seed)
        self.chain_offset = int(chain_offset)
        self.use_graph = bool(use_graph)
        self.ring_shortcut = bool(ring_shortcut)
        self.real_pairs = bool(real_pairs)
        if noise_bits not in (32, 64):
            raise ValueError("noise_bits must be 32 or 64")
        self.noise_bits = int(noise_bits)
        self.noise64 = self.noise_bits == 64
        self._stock_prox = _is_stock_l1(prior)  # the library's own prox: the step kernels may apply it themselves
        self.nsamples = int(self.nsamples)
        for op in (getattr(forward, "transform", None), getattr(forward, "measurement", None)):
            if hasattr(op, "ensure_chains"):
                op.ensure_chains(self.nchains)

    def run(self, start_point=None):
        raise NotImplementedError

    # ---- device-side pieces -----------------------------------------------------------
    def _state_dtype(self, start=None):
        cplx = bool(self.complex) or isinstance(getattr(self.forward, "transform", None), SphericalWaveletTransform)
        d = self.forward.data
        cplx = cplx or (d.is_complex() if isinstance(d, torch.Tensor) else np.iscomplexobj(d))
        if start is not None:
            cplx = cplx or (start.is_complex() if isinstance(start, torch.Tensor) else np.iscomplexobj(start))
        return torch.complex128 if cplx else torch.float64

    def _l2_dev(self, preds):
        """L2 = vdot(d, invcov @ d) of a [C, ndata] prediction batch -> complex128 [C] (pxmcmc/mcmc.py:78-79)"""
        inputs = self._l2_inputs(preds)
        if inputs is not None:
            return ops.reduce_l2(*inputs)
        p = ops.as_device(preds)  # full inverse covariance (forward.py:75-78): d = preds - data, vdot(-d, W(-d)) = vdot(d, W d)
        dt = self.forward._resid_dtype(p) if hasattr(self.forward, "_resid_dtype") else p.dtype
        d = ops.residual_grad(p.to(dt), self._l2_data_dev(dt), self.forward.invcov.ones)
        return ops.reduce_vdot(d, self.forward.invcov.matvec(d))

    def _l2_data_dev(self, dt):
        """the data vector on the device in the residual's dtype (cached: no host copy per iteration)"""
        cache = getattr(self, "_l2_data", None)
        if cache is None or cache[0] is not self.forward.data or cache[1].dtype != dt:
            src = getattr(self.forward, "data_dev", None)
            src = ops.as_device(self.forward.data) if src is None else src
            self._l2_data = cache = (self.forward.data, src.reshape(-1).to(dt).contiguous())
        return cache[1]

    def _l2_inputs(self, preds):
        """(preds, data, diagonal of invcov) as the L2 reduction takes them; None with a full inverse covariance"""
        if hasattr(self.forward.invcov, "matvec"):
            return None
        p = ops.as_device(preds)
        dt = self.forward._resid_dtype(p) if hasattr(self.forward, "_resid_dtype") else p.dtype
        ic = getattr(self, "_l2_invcov", None)
        if ic is None or ic[0] is not self.forward.invcov:
            inv = self.forward.invcov
            diag = inv.diag if hasattr(inv, "diag") else ops.as_device(inv.diagonal())
            self._l2_invcov = ic = (inv, ops.as_device(diag).reshape(-1).contiguous())
        return p.to(dt), self._l2_data_dev(dt), ic[1]

    def _logpi_dev(self, X, preds):
        """per-chain (logPi, L2, prior) tensors; pxmcmc/mcmc.py:71-82 (L2 carries no factor 1/2)."""
        L2 = self._l2_dev(preds)
        prior = self.prior.prior(X)
        if not isinstance(prior, torch.Tensor):
            prior = torch.as_tensor(np.atleast_1d(np.asarray(prior, dtype=float)), device=L2.device)
        logPi = -self.mu * prior - L2
        return logPi, L2, prior

    def _initial_sample(self, initial_sample=None):
        """pxmcmc/mcmc.py:97-111, returning GPU tensors [C, nparams], [C, ndata]."""
        C, N = self.nchains, self.forward.nparams
        if initial_sample is None:
            if self.rng == "numpy":
                draw = lambda: np.stack([laplace.rvs(size=N) for _ in range(C)])
            else:
                gens = [np.random.default_rng([self.seed, self.chain_offset + c, 0x1A91ACE]) for c in range(C)]
                draw = lambda: np.stack([laplace.rvs(size=N, random_state=g) for g in gens])
            X0 = draw()
            if self.complex:
                X0 = X0 + draw() * 1j
        else:
            if isinstance(initial_sample, torch.Tensor):
                X0 = initial_sample
            elif isinstance(initial_sample, np.ndarray):
                X0 = initial_sample
            else:
                raise TypeError("Expected a 1D numpy array as an initial sample")
            nd = X0.dim() if isinstance(X0, torch.Tensor) else np.ndim(X0)
            if nd == 1:
                if X0.shape[0] != N:
                    raise ValueError("Inital sample given has incorrect size")
                X0 = X0[None, :]
                if C > 1:
                    X0 = X0.repeat(C, 1) if isinstance(X0, torch.Tensor) else np.repeat(X0, C, axis=0)
            elif nd == 2 and C > 1:
                if tuple(X0.shape) != (C, N):
                    raise ValueError("Inital sample given has incorrect size")
            else:
                raise TypeError("Expected a 1D numpy array as an initial sample")
        X_curr = ops.as_device(X0, self._state_dtype(X0)).clone()  # never write into the caller's start point
        curr_preds = ops.as_device(self.forward.forward(X_curr))
        return X_curr, curr_preds

    # ---- device status -----------------------------------------------------------------
    def _device_plans(self):
        """every live transform plan of this process (``ops.live_plans``: a weak registry filled at plan creation) --
        the operators' own plans AND those owned by a prior built on another transform object, by user operators or by
        analysis-setting transforms under any attribute name"""
        return ops.live_plans()

    def _check_device_status(self):
        """Fail loudly (PxmError) if a kernel reported an expired bounded wait since the last check -- called where the
        sampler synchronises with the device anyway: saved samples, progress prints, end of run (the reference raises
        on bad state, pxmcmc/mcmc.py:104-109; a silently corrupted chain is not an outcome)."""
        # The status words are LEFT SET: with two samplers in one process each of them sees a latched fault whichever polls
        # first (a fault is fatal for every chain that ran on the plan; ``plan.status(clear=True)`` is the explicit reset).
        for pl in self._device_plans():
            pl.raise_on_fault(clear=False)

    # ---- noise ---------------------------------------------------------------------------
    def _host_noise(self, shape_like):
        """the reference's draw order: randn(N) [+ 1j randn(N)] per chain (pxmcmc/mcmc.py:193-195)."""
        C, N = shape_like.shape
        w = np.stack([np.random.randn(N) + (np.random.randn(N) * 1j if self.complex else 0) for _ in range(C)])
        return ops.as_device(w)

    # ---- stepping engine: each class's _engine_start(X, preds, i0) builds self._eng and returns it ------------------
    def _engine_start_generic(self, X, preds, i0, step, lazy, graph_ok, reset=None):
        """The engine of the steps that run on the operators' own plans: ``step(eng, src, dst)`` per iteration on static
        buffers, the noise kernels reading the iteration number from a device counter (``eng.cnt.t``).  With ``lazy``
        the steps do not write P: forward(X) is formed where the state is observed.  ``reset(eng)`` rebuilds whatever the
        steps carry besides (XA, P) from the restored start state."""
        X = ops.as_device(X).contiguous()
        preds = ops.as_device(preds)
        eng = self._eng = Engine(X, preds, _Counter(i0))
        eng.one = lambda src, dst: step(eng, src, dst)
        if reset is not None:
            eng.reset = lambda: reset(eng)
        if lazy:
            eng.form_preds = lambda X: eng.P.copy_(ops.as_device(self.forward.forward(X)))
        return eng.ready(X, preds, i0, graph_ok)

    def _engine_advance(self, k):
        self._eng.advance(k)

    def _engine_state(self):
        return self._eng.state()

    def _engine_stop(self):
        if self._eng is not None:
            self._eng.stop()
