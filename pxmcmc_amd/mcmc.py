"""
Samplers of the reference (pxmcmc/mcmc.py:6-383: PxMCMCParams, PxMCMC, MYULA, PxMALA, SKROCK) driving
the HIP kernels.  The plugin protocol is the reference's: the sampler only touches
``forward.forward / calc_gradg / data / invcov / nparams`` and ``prior.proxf / prior.prior``.

Extensions (all optional, defaults reproduce the reference's one-chain behaviour):

* ``nchains``      -- C independent chains advanced together as one ``[C, N]`` batch;
* ``rng``          -- ``"philox"`` (device counter-based stream keyed (seed, chain, iteration),
  independent of how chains are spread over GPUs) or ``"numpy"`` (the reference's global
  ``np.random`` stream in the reference's draw order, for parity runs);
* ``chain_offset`` -- global index of this process's first chain (multi-GPU sharding);
* ``use_graph``    -- replay the fused iteration from a captured HIP graph (default on);
* ``ring_shortcut`` -- with a scalar ``sig_d`` apply the residual on the ring transforms (default on);
* ``noise_bits``   -- 64 (default) or 32: arithmetic of the Box-Muller step of the device Philox stream.  64 evaluates
  log / sqrt / sincos in double precision (table look-ups + short polynomials, csrc/philox.h) as the reference's
  ``np.random.randn`` does (pxmcmc/mcmc.py:193); 32 runs it on the f32 transcendental units (deviates ~1e-6 relative,
  exact fp64 exponent: tail to 8.5 sigma), ~2 % faster at the benchmark size.  Same Philox counters and uniforms either
  way: the two streams agree to ~1e-6;
* ``real_pairs``   -- with REAL data, a real start point and ``params.complex == False`` the reference's
  complex128 state has a zero imaginary part (every operator of the path maps real fields to real
  fields); the fused wavelet path then carries two real chains per complex slot -- chain 2c in the real
  part, chain 2c+1 in the imaginary part -- through the complex-linear transforms and applies prox and
  noise per component (real-signal symmetry).  Same results, half the transform
  work (default on; complex data, as in the reference-literal topography set-up, is never paired);
* ``summary``      -- ``None`` (default), ``"state"``, ``"image"`` or a tuple of both: accumulate every saved sample into a
  device-resident :class:`uncertainty.PosteriorSummary` per space (per-chain mean and variance, highest-posterior sample,
  R-hat across the batch).  ``"state"`` is the sampled vector as ``chain`` would hold it;
  ``"image"`` is ``transform.inverse`` of it in the synthesis setting and the state itself in the analysis setting.  After
  ``run()`` the summaries are in ``self.summary[space]``.  With ``"chain"`` left out of ``track`` no state is copied to the
  host during the run;
* ``summary_alpha`` -- ``None`` (default) or alpha in (0, 1]; needs ``summary``.  The summaries also keep the
  ``tail_capacity(alpha, nsamples)`` smallest and largest saved samples of every element, and
  ``self.summary[space].credible_interval_range()`` then gives, per chain, the (1 - alpha) credible-interval map the
  reference computes from the saved chain (pxmcmc/uncertainty.py:7-16), exactly;
* ``summary_ess``  -- ``None`` (default) or K, even with 2 <= K <= 64; needs ``summary``.  The summaries also accumulate the
  lagged products of the saved samples at lags below K, and ``self.summary[space].ess()`` then gives the effective sample
  size of every chain and element, ``ess_pooled()`` that of the chain batch and ``mcse()`` the standard error of
  ``pooled_mean()``.  Where ``ess_lag()`` reaches K the value is truncated, an upper bound: raise K or ``ngap``.

SKROCK (pxmcmc/mcmc.py:292-383) follows the published recursion (Pereyra, Vargas-Mieles & Zygalakis 2020), which
differs from the reference's literal code for s >= 2 (see :class:`SKROCK`); it takes the keywords above except
``ring_shortcut`` / ``real_pairs``, which it accepts and ignores.
"""
import time

import numpy as np
import torch
from scipy.stats import laplace

from . import ops
from .measurements import Identity, WeakLensingHarmonic
from .prior import L1
from .transforms import SphericalWaveletTransform


class PxMCMCParams:
    """
    Tuning and runtime parameters (pxmcmc/mcmc.py:6-43).

    :param lmda: prox parameter
    :param delta: Forward-Euler step size
    :param mu: regularisation parameter
    :param s: max order of Chebyshev polynomials: the number of stages of :class:`SKROCK` (unused by MYULA / PxMALA)
    :param nsamples: number of samples to save
    :param nburn: burn-in size
    :param ngap: thinning: iterations between saved samples
    :param complex: ``True`` if the sampled parameters are complex
    :param verbosity: print every ``verbosity`` iterations
    :param track: list of variables to keep track of
    """

    def __init__(
        self,
        lmda=3e-5,
        delta=1e-5,
        s=1,
        mu=1,
        nsamples=int(1e6),
        nburn=int(1e3),
        ngap=int(1e2),
        complex=False,
        verbosity=100,
        track=["logposterior", "L2", "prior", "chain"],
    ):
        self.lmda = lmda
        self.delta = delta
        self.mu = mu
        self.s = s
        self.nsamples = nsamples
        self.nburn = nburn
        self.ngap = ngap
        self.complex = complex
        self.verbosity = verbosity
        self.track = track


def _is_stock_l1(prior):
    """True when prior.proxf is the library's own synthesis soft threshold (safe to fuse)."""
    return isinstance(prior, L1) and type(prior).proxf is L1.proxf and type(prior)._proxf_synthesis is L1._proxf_synthesis and prior.setting == "synthesis"


class PxMCMC:
    """
    Base class with the general functions (pxmcmc/mcmc.py:46-140).

    :param forward: :class:`forward.ForwardOperator`-like object
    :param prior: prior object implementing ``prior`` and ``proxf``
    :param mcmcparams: :class:`PxMCMCParams`
    """

    def __init__(self, forward, prior, mcmcparams=PxMCMCParams(), nchains=1, rng="philox", seed=0, chain_offset=0,
                 use_graph=True, ring_shortcut=True, real_pairs=True, noise_bits=64, summary=None, summary_alpha=None,
                 summary_ess=None):
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
        self._pairs = False
        self._stock_prox = _is_stock_l1(prior)  # the library's own prox: the step kernels may apply it themselves
        self.nsamples = int(self.nsamples)
        for op in (getattr(forward, "transform", None), getattr(forward, "measurement", None)):
            if hasattr(op, "ensure_chains"):
                op.ensure_chains(self.nchains)
        self._summary_spaces = self._summary_arg(summary)
        self.summary = {} if self._summary_spaces else None
        self._summary_plan = None
        if summary_alpha is not None:
            from .uncertainty import tail_capacity

            if not self._summary_spaces:
                raise ValueError("summary_alpha needs summary: the tails are part of the streaming summaries")
            tail_capacity(summary_alpha, self.nsamples)  # (validates alpha and nsamples)
        self.summary_alpha = None if summary_alpha is None else float(summary_alpha)
        if summary_ess is not None:
            from .uncertainty import ess_lag_count

            if not self._summary_spaces:
                raise ValueError("summary_ess needs summary: the lagged products are part of the streaming summaries")
            summary_ess = ess_lag_count(summary_ess)
        self.summary_ess = summary_ess
        self._initialise_tracking_arrays()

    def run(self, start_point=None):
        raise NotImplementedError

    # ---- streaming summaries of the saved samples (uncertainty.PosteriorSummary) --------------------------------------------
    def _summary_arg(self, summary):
        """``summary=`` -> tuple of spaces, validated against the operators"""
        spaces = () if summary is None else ((summary,) if isinstance(summary, str) else tuple(summary))
        for sp in spaces:
            if sp not in ("state", "image"):
                raise ValueError("summary must be None, 'state', 'image' or a tuple of both")
        if "image" in spaces and getattr(self.forward, "setting", "synthesis") != "analysis":
            tr = getattr(self.forward, "transform", None)
            if tr is None or not hasattr(tr, "inverse"):
                raise ValueError("summary='image' needs forward.transform.inverse in the synthesis setting")
            if getattr(tr, "harmonic", False):
                raise ValueError("summary='image': a harmonic transform maps to harmonic coefficients, not to an image")
        return tuple(dict.fromkeys(spaces))

    def _summary_image(self, tr, S):
        """transform.inverse of a sample batch, on the device.  The fused wavelet steps carry ring state in the workspace of
        the plan they run on between iterations: when that is the transform's own plan the synthesis runs on a plan of the
        summary's own (same tables, its own workspace), made at the first save"""
        eng = getattr(self, "_eng", None)
        if eng is not None and eng["plan"] is not None and eng["plan"] is getattr(tr, "_plan", None):
            if self._summary_plan is None:
                self._summary_plan = tr._make_plan(self.nchains)
            return self._summary_plan.synthesis(S)
        return ops.as_device(tr.inverse(S))

    def _summary_update(self, X_curr, logPi, chains):
        """the samples being saved -> the summaries (created at the first save of a run, when shapes and device are known).
        The state summary of a full save (MYULA, SKROCK) allocates and copies nothing.  A partial save (PxMALA's ``chains``)
        uploads a [C] mask, at a point where that loop has just read the accept flags back; the image summary allocates the
        images, and with ``params.complex = False`` the real-part copy of the state they are synthesised from."""
        from .uncertainty import PosteriorSummary

        X = ops.as_device(X_curr)
        analysis = getattr(self.forward, "setting", "synthesis") == "analysis"
        mask = None
        if chains is not None:
            mask = np.zeros(self.nchains, dtype=np.int32)
            mask[list(chains)] = 1
        for sp in self._summary_spaces:
            if sp == "state" or analysis:
                S, cplx = X, bool(self.complex)  # as ``chain`` keeps it: the real part unless params.complex
            else:
                tr = self.forward.transform
                if X.is_complex() and not self.complex:  # the image of the sample ``chain`` keeps
                    S = torch.complex(X.real, torch.zeros_like(X.real))
                else:
                    S = X
                S, cplx = self._summary_image(tr, S), True
            if sp not in self.summary:
                self.summary[sp] = PosteriorSummary(self.nchains, S.shape[1], cplx, alpha=self.summary_alpha, nsamples=self.nsamples,
                                                    ess_lags=self.summary_ess)
            self.summary[sp].update(S, logpi=ops.as_device(logPi), mask=mask)

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

    def logpi(self, X, preds):
        """log posterior, L2 norm and prior norm of a model (pxmcmc/mcmc.py:71-82)."""
        logPi, L2, prior = self._logpi_dev(X, preds)
        batched = (X.dim() if isinstance(X, torch.Tensor) else np.ndim(X)) == 2
        if batched:
            return logPi, L2, prior
        cplx = L2.is_complex() and bool(abs(L2[0].imag.item()) > 0)
        f = (lambda v: complex(v[0].item())) if cplx else (lambda v: float(v[0].real.item()))
        return f(logPi), f(L2), float(prior[0].item())

    def _print_progress(self, i, logpi, **kwargs):
        print(
            f"{i+1:,}/{self.nsamples:,} - logposterior: {logpi:.8e} - "
            + " - ".join([f"{k}: {kwargs[k]:.8e}" for k in kwargs]),
        )

    def _initial_sample(self, initial_sample=None):
        """pxmcmc/mcmc.py:97-111, returning GPU tensors [C, nparams], [C, ndata]."""
        C, N = self.nchains, self.forward.nparams
        if self._summary_spaces:
            self.summary = {}  # start of a run: its summaries begin empty
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

    def _initialise_tracking_arrays(self):
        """pxmcmc/mcmc.py:113-128; with nchains > 1 every array gains a leading chain axis."""
        lead = () if self.nchains == 1 else (self.nchains,)
        if "logposterior" in self.track:
            self.logPi = np.zeros(lead + (self.nsamples,))
        if "predictions" in self.track:
            self.preds = np.zeros(lead + (self.nsamples, len(self.forward.data)), dtype=float)
        if "chain" in self.track:
            self.chain = np.zeros(lead + (self.nsamples, self.forward.nparams), dtype=complex if self.complex else float)
        if "L2" in self.track:
            self.L2s = np.zeros(lead + (self.nsamples,), dtype=float)
        if "prior" in self.track:
            self.priors = np.zeros(lead + (self.nsamples,), dtype=float)

    def _tracking(self, j, X_curr, curr_preds, logPi, L2, prior, chains=None):
        """pxmcmc/mcmc.py:130-140.  ``j`` is an int (all chains) or per-chain indices with ``chains``."""
        def put(arr, val):
            val = val.detach().cpu().numpy() if isinstance(val, torch.Tensor) else np.asarray(val)
            if not np.iscomplexobj(arr):
                val = np.real(val)  # the reference's float arrays silently drop the imaginary part
            if self.nchains == 1:
                arr[j] = val[0]
            elif chains is None:
                arr[:, j] = val
            else:
                for c, jc in zip(chains, j):
                    arr[c, jc] = val[c]

        if hasattr(self, "logPi"):
            put(self.logPi, logPi)
        if hasattr(self, "L2s"):
            put(self.L2s, L2)
        if hasattr(self, "priors"):
            put(self.priors, prior)
        if hasattr(self, "preds"):
            put(self.preds, curr_preds)
        if hasattr(self, "chain"):
            put(self.chain, X_curr)
        if self._summary_spaces:
            self._summary_update(X_curr, logPi, chains)

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

    # ---- stepping engine: static buffers, an iteration counter, HIP-graph replay between observable events ----------
    # (each sampler's _engine_start builds one through _engine_new + _engine_ready)
    _GRAPH_PAIRS = 4  # iterations per graph replay = 2 * _GRAPH_PAIRS (fewer, longer launches of the host)

    def _engine_capture(self, warm, restore, bodies):
        """Capture one HIP graph per callable of ``bodies`` -- the only place the samplers capture.  ``warm()`` runs first,
        outside capture on a side stream (lazy allocations, attributes); ``restore()`` then puts the state back and each
        body is captured under ``ops.capture_scope()``: a plan torn down while a capture is in progress (the garbage
        collector may run at any point) only queues its device frees, which the library empties at the end of the scope.
        Capture does not execute, so the state is the restored one afterwards.  Returns (graphs, None), or, when capture
        fails, (None, repr(exc)) with the state restored: eager stepping, same results."""
        try:
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                warm()
            torch.cuda.current_stream().wait_stream(stream)
            torch.cuda.synchronize()
            restore()
            graphs = []
            for body in bodies:
                g = torch.cuda.CUDAGraph()
                with ops.capture_scope(), torch.cuda.graph(g):
                    body()
                graphs.append(g)
            return graphs, None
        except Exception as exc:  # capture unsupported in this environment
            restore()
            return None, repr(exc)

    def _engine_new(self, X, preds, cnt, plan=None, pairs=False):
        """``self._eng``, with every key it ever holds; the builder then sets ``one`` and whichever hooks it needs"""
        self._eng = {
            "XA": X.clone(),  # ping-pong state buffers: the state is in XA (side "A") or XB (side "B")
            "XB": torch.empty_like(X),
            "side": "A",  # which of XA / XB holds the current state
            "P": preds.clone(),  # forward(state): written by every step, or formed on demand (form_preds)
            "form_preds": None,  # form_preds(X) writes P of the state X; set when the steps do not write P
            "P_stale": False,  # P lags the state (set by _engine_advance, cleared by _engine_state; form_preds only)
            "one": None,  # one(src, dst): one iteration from the state in src to dst
            "cnt": cnt,  # iteration counter read by the steps: the plan's ops.IterCounter, or a _Counter
            "cnt0": lambda i: i,  # counter value at which the next step is iteration i
            "reset": lambda: None,  # rebuilds plan-carried state from (XA, P) after a restore
            "plan": plan,  # WavPlan of the fused steps (None: the steps run on the operators' own plans)
            "pairs": pairs,  # state and preds carried pair-packed (MYULA real_pairs)
            "ring": False,  # fused ring-space step (scalar sig_d)
            "graph": None,  # captured graph of 2 iterations (None: eager stepping)
            "graph_long": None,  # captured graph of 2 * _GRAPH_PAIRS iterations
            "graph_error": None,  # repr of the exception that made capture fall back to eager stepping
        }
        return self._eng

    def _engine_ready(self, X, preds, i0, graph_ok):
        """point the counter at iteration i0 and, if ``graph_ok``, capture the graphs of 2 and 2 * _GRAPH_PAIRS
        iterations; (X, preds) is the start state as the engine carries it"""
        eng = self._eng
        eng["cnt"].set(eng["cnt0"](i0))
        if graph_ok:
            XA, XB, one = eng["XA"], eng["XB"], eng["one"]

            def two():
                one(XA, XB)
                one(XB, XA)

            def restore():
                XA.copy_(X)
                eng["P"].copy_(preds)
                eng["cnt"].set(eng["cnt0"](i0))
                eng["reset"]()

            bodies = [lambda n=n: [two() for _ in range(n)] for n in (1, self._GRAPH_PAIRS)]
            graphs, eng["graph_error"] = self._engine_capture(two, restore, bodies)
            eng["graph"], eng["graph_long"] = graphs or (None, None)
        return eng

    def _engine_start_generic(self, X, preds, i0, step, lazy, graph_ok, reset=None):
        """The engine of the steps that run on the operators' own plans: ``step(eng, src, dst)`` per iteration on static
        buffers, the noise kernels reading the iteration number from a device counter (``eng["cnt"].t``).  With ``lazy``
        the steps do not write P: forward(X) is formed where the state is observed.  ``reset(eng)`` rebuilds whatever the
        steps carry besides (XA, P) from the restored start state."""
        X = ops.as_device(X).contiguous()
        preds = ops.as_device(preds)
        eng = self._engine_new(X, preds, _Counter(i0))
        eng["one"] = lambda src, dst: step(eng, src, dst)
        if reset is not None:
            eng["reset"] = lambda: reset(eng)
        if lazy:
            eng["form_preds"] = lambda X: eng["P"].copy_(ops.as_device(self.forward.forward(X)))
        return self._engine_ready(X, preds, i0, graph_ok)

    def _engine_advance(self, k):
        """advance the engine's state by k iterations (graph replays of 2 * _GRAPH_PAIRS + eager remainder)"""
        eng = self._eng
        if k > 0 and eng["form_preds"] is not None:
            eng["P_stale"] = True
        if eng["side"] == "B" and k > 0:  # realign so that replays start from XA
            eng["one"](eng["XB"], eng["XA"])
            eng["side"] = "A"
            k -= 1
        if eng["graph"] is not None:
            per = 2 * self._GRAPH_PAIRS
            while k >= per:
                eng["graph_long"].replay()
                k -= per
            while k >= 2:
                eng["graph"].replay()
                k -= 2
        while k >= 2:
            eng["one"](eng["XA"], eng["XB"])
            eng["one"](eng["XB"], eng["XA"])
            k -= 2
        if k == 1:
            eng["one"](eng["XA"], eng["XB"])
            eng["side"] = "B"

    def _engine_state(self):
        """(X, preds) of the current state as [C, .] arrays (pair-packed engines unpack here: observation only)"""
        eng = self._eng
        X = eng["XA"] if eng["side"] == "A" else eng["XB"]
        if eng["P_stale"]:  # preds on demand: forward(X) of the current state
            eng["form_preds"](X)
            eng["P_stale"] = False
        # observation point: the host is about to read the state -- an expired device wait since the last one raises
        if eng["plan"] is not None:
            eng["plan"].raise_on_fault()
        if eng["pairs"]:
            return self._unpack(X), self._unpack(eng["P"])
        return X, eng["P"]

    def _engine_stop(self):
        """unregister the iteration counter and drop the engine's buffers, graph and closures (the closures
        reference the sampler: without this the plan would only be released by a later garbage collection)"""
        eng = getattr(self, "_eng", None)
        if eng is not None and eng["cnt"] is not None:
            eng["cnt"].close()
            eng["graph"] = eng["graph"] is not None  # keep the flags (ring, pairs, graph) for inspection
            for k in ("one", "XA", "XB", "P", "form_preds", "plan", "cnt", "cnt0", "graph_long", "reset"):
                eng[k] = None

    def _run_engine(self, X_curr, curr_preds):
        """
        Same schedule as the reference loop (pxmcmc/mcmc.py:157-181), but iterations between two events
        (save / progress print) are advanced together: by HIP-graph replays when capture is available.
        """
        nburn, ngap, verb = int(self.nburn), int(self.ngap), int(self.verbosity)
        self._engine_start(X_curr, curr_preds, 0)
        try:
            i = 0  # iterations done
            j = 0  # saved samples (excludes burn-in and thinned samples)
            while j < self.nsamples:
                # next iteration index (0-based) at which something observable happens
                if i < nburn:
                    nxt_save = nburn
                elif ngap == 0:
                    nxt_save = i
                else:
                    nxt_save = i + (-(i - nburn)) % ngap
                nxt_print = i + (verb - 1 - i % verb) if verb > 0 else nxt_save
                stop = min(nxt_save, nxt_print)
                self._engine_advance(stop - i + 1)  # run iterations i..stop
                i = stop
                X_curr, curr_preds = self._engine_state()
                if i >= nburn:
                    if ngap == 0 or (i - nburn) % ngap == 0:
                        if self._eng["plan"] is None:  # steps on the operators' own plans: poll those
                            self._check_device_status()
                        logPi, L2, prior = self._logpi_dev(X_curr, curr_preds)
                        self._tracking(j, X_curr, curr_preds, logPi, L2, prior)
                        j += 1
                    if verb > 0 and (i + 1) % verb == 0:
                        first = (lambda a: a[j - 1] if self.nchains == 1 else a[0, j - 1])
                        self._print_progress(j - 1, first(self.logPi), L2=first(self.L2s), prior=first(self.priors))
                elif verb > 0 and (i + 1) % verb == 0:
                    print("Burning in...")
                i += 1
            X_curr, curr_preds = self._engine_state()
            self._check_device_status()
            self.X_curr, self.curr_preds, self.niter = X_curr.clone(), curr_preds.clone(), i
            self.used_graph = self._eng["graph"] is not None
            self.graph_error = self._eng["graph_error"]
        finally:
            self._engine_stop()
        print("\nDONE")


class _Counter:
    """iteration counter of the engines that step on the operators' own plans (the fused engines use the plan's
    ops.IterCounter): a device int64 ``t`` that the noise kernels read when they run (graph replay), or, with
    ``host=True``, a host int ``i`` that the eager-only engine passes to each call"""

    def __init__(self, start, host=False):
        self.i = int(start)
        self.t = None if host else torch.full((1,), self.i, dtype=torch.int64, device=ops.device())

    def set(self, v):
        self.i = int(v)
        if self.t is not None:
            self.t.fill_(self.i)

    def add(self, inc=1):
        if self.t is None:
            self.i += inc
        else:
            ops.counter_add(self.t, inc)

    def close(self):
        pass


class MYULA(PxMCMC):
    """The MYULA chain (pxmcmc/mcmc.py:143-201)."""

    def __init__(self, forward, prox, mcmcparams=PxMCMCParams(), **kwargs):
        super().__init__(forward, prox, mcmcparams, **kwargs)
        self._own_step = type(self).chain_step is not MYULA.chain_step  # a subclass's chain_step: called as it is

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
        2 * _GRAPH_PAIRS iterations"""
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
                      iter_dev=eng["cnt"].t, noise64=self.noise64)
            gradg = ops.as_device(f.calc_gradg(eng["P"]), src.dtype)
            if self._fused_prox:
                ops.myula_step(src, gradg, self.prior.T_dev, delta, lmda, out=dst, **kw)
            else:
                proxf = ops.as_device(self.prior.proxf(src), src.dtype)
                ops.chain_step(src, proxf, gradg, delta, lmda, out=dst, **kw)
            eng["P"].copy_(ops.as_device(f.forward(dst)))
            eng["cnt"].add(1)

        return self._engine_start_generic(X, preds, i0, step, lazy=False, graph_ok=True)

    def _engine_start_fused(self, X, preds, i0):
        """The fused wavelet steps of WavPlan, on the plan's registered iteration counter"""
        f = self.forward
        plan, data = f.transform._plan, f.data_dev_c128
        if self._pairs:  # two real chains per complex slot: X, preds are carried pair-packed
            plan, data = self._pair_plan, self._pair_data
            X, preds = self._pack(X), self._pack(preds)
        # per-plan device counter: the steps below read it at execution time
        eng = self._engine_new(X, preds, ops.IterCounter(plan, i0), plan=plan, pairs=self._pairs)
        d, T, delta, lmda = f.invcov.diag, self.prior.T_dev, float(self.delta), self.lmda
        # params.complex: randn + 1j randn (pxmcmc/mcmc.py:193-195) -> PXM_MODE_CPLX_NOISE in the fused epilogues
        kw = dict(noise_complex=bool(self.complex), seed=self.seed, chain0=self.chain_offset, it=0, pairs=self._pairs,
                  noise64=self.noise64)
        # Uniform inverse covariance (scalar sig_d): the image-space residual is applied on the rings and the
        # L-level iDFT/DFT pair between forward() and calc_gradg() drops out (pxm_wav_ring_step); preds is
        # then formed only when it is observed.
        eng["ring"] = bool(self.ring_shortcut and d.numel() > 0 and bool((d == d[0]).all()))
        if eng["ring"]:
            w = complex(d[0].item())
            plan.ring_set_data(data)
            eng["reset"] = lambda: plan.ring_init(eng["XA"])  # plan-carried state of (XA, P)
            eng["cnt0"] = lambda i: i - 1  # ring_step advances the counter itself, before using it
            eng["form_preds"] = lambda X: plan.ring_preds(eng["P"].shape[0], out=eng["P"])  # of the carried rings
            eng["one"] = lambda src, dst: plan.ring_step(src, w, T, delta, lmda, out=dst, **kw)
        else:
            eng["reset"] = lambda: plan.image_init(eng["P"], data, d)  # residual rings of the state, carried by the plan

            def one(src, dst):
                # calc_gradg + proxf + chain_step + forward of the new state (preds written in place)
                plan.image_step(src, data, d, T, delta, lmda, out=dst, preds_out=eng["P"], **kw)
                eng["cnt"].add(1)

            eng["one"] = one
        eng["reset"]()
        return self._engine_ready(X, preds, i0, self.use_graph)

    def _engine_start_harmonic(self, X, preds, i0):
        """The fused harmonic step of HarmWavPlan: the whole iteration, preds of the new state included, in one kernel that
        reads the iteration number from the engine's device counter"""
        f = self.forward
        plan = f.transform._plan
        X = ops.as_device(X, torch.complex128).contiguous()
        preds = ops.as_device(preds, torch.complex128)
        eng = self._engine_new(X, preds, _Counter(i0), plan=plan)
        data, d, T, delta, lmda, k = f.data_dev_c128, f.invcov.diag, self.prior.T_dev, float(self.delta), self.lmda, self._harm_kernel
        kw = dict(noise_complex=bool(self.complex), seed=self.seed, chain0=self.chain_offset, noise64=self.noise64)

        def one(src, dst):
            plan.myula_step(src, data, d, k, T, delta, lmda, iter_dev=eng["cnt"].t, out=dst, preds_out=eng["P"], **kw)
            eng["cnt"].add(1)

        eng["one"] = one
        return self._engine_ready(X, preds, i0, self.use_graph)

    def _engine_start_eager(self, X, preds, i0):
        """The engine of _eager_only: the calls of the reference's loop, iteration by iteration -- _advance with the
        host iteration number (host noise in the reference's draw order), then forward (the synthesis of the
        pair-packed state)"""
        if self._pairs:
            X, preds = self._pack(X), self._pack(preds)
        eng = self._engine_new(X, preds, _Counter(i0, host=True), pairs=self._pairs)
        forward = self._pair_plan.synthesis if self._pairs else (lambda X: ops.as_device(self.forward.forward(X)))

        def one(src, dst):
            X_prop = self._advance(src, eng["P"], eng["cnt"].i)
            dst.copy_(X_prop)
            eng["P"].copy_(forward(X_prop))
            eng["cnt"].add(1)

        eng["one"] = one
        return self._engine_ready(X, preds, i0, graph_ok=False)

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


class _PxmalaState:
    """Static device buffers of one PxMALA run (``PxMALA._start_state``); a route allocates what it uses.  All routes: the
    current state ``X preds gradg proxf logpi L2 prior delta``, overwritten per chain where ``accept`` [C] is set, the
    iteration counter ``cnt`` and the two rings of ``_TraceChunks`` that the accept kernels write.  Proposal buffers:
    ``X_prop lt_cp prior_p`` (proposal, q(X'|X), prior(X')) and the stock prior's threshold and weights ``T w_prior`` on
    the fused and separate routes, ``proxf_prop`` on the separate route, ``lt_pc L2_p`` (q(X|X'), L2(X')) and the two
    scratches of partial sums on the fused route; the plugin route's proposal is whatever tensors the user's operators
    return."""

    def __init__(self, start, C, dev, route, traces, prior):
        self.X, self.preds, self.gradg, self.proxf, self.logpi, self.L2, self.prior, self.delta = start
        self.accept = torch.zeros(C, dtype=torch.int32, device=dev)
        self.cnt = _Counter(0)  # device-resident iteration number (graph replay)
        self.acc_trace, self.delta_trace = traces.acc_buf, traces.delta_buf
        if route != "plugin":
            self.T, self.w_prior = prior.T_dev, getattr(prior, "_weights_dev", None)  # (the proposal kernel applies the prox)
            self.X_prop = torch.empty_like(self.X)
            self.lt_cp = torch.empty(C, dtype=torch.complex128, device=dev)
            self.prior_p = torch.empty(C, dtype=torch.float64, device=dev)
        if route == "separate":
            self.proxf_prop = torch.empty_like(self.X)
        if route == "fused":
            self.lt_pc = torch.empty(C, dtype=torch.complex128, device=dev)
            self.L2_p = torch.empty(C, dtype=torch.complex128, device=dev)
            self.prop_scratch = ops.pxmala_propose_scratch(C, dev)
            self.fin_scratch = torch.empty(2 * ops.reduce_scratch_doubles(C), dtype=torch.float64, device=dev)

    def current(self):
        """what an iteration carries over to the next: the tensors a graph capture snapshots and restores"""
        return (self.X, self.preds, self.gradg, self.proxf, self.logpi, self.L2, self.prior, self.delta)


class _TraceChunks:
    """Acceptance flag and delta of every iteration and chain.  The accept kernels write row ``i % depth`` of two
    ``[depth, C]`` device rings; ``after(i)`` reads both back when iteration i filled the last row (the only host
    synchronisation of the traces during a run), ``result`` reads the rows of the last, partial chunk."""

    def __init__(self, depth, C, dev):
        self.depth = depth
        self.acc_buf = torch.zeros((depth, C), dtype=torch.int32, device=dev)
        self.delta_buf = torch.zeros((depth, C), dtype=torch.float64, device=dev)
        self._acc, self._delta = [], []
        self._accepted0 = 0  # accepted proposals of chain 0 in the chunks read back

    def _read(self, rows):
        self._acc.append(self.acc_buf[:rows].cpu().numpy().copy())
        self._delta.append(self.delta_buf[:rows].cpu().numpy().copy())

    def after(self, i):
        if i % self.depth == self.depth - 1:
            self._read(self.depth)
            self._accepted0 += int(self._acc[-1][:, 0].sum())

    def accepted0(self, i):
        """accepted proposals of chain 0 in iterations 0..i (progress line; reads the rows not yet flushed)"""
        k = i % self.depth
        pending = 0 if k == self.depth - 1 else int(self.acc_buf[: k + 1, 0].sum().item())
        return self._accepted0 + pending

    def result(self, niter, delta0, tune_delta):
        """(acceptance_trace, deltas_trace) of ``niter`` iterations as the reference keeps them: lists for one chain,
        ``[niter, C]`` / ``[1 + niter, C]`` arrays otherwise; deltas start with delta0 and grow only with tune_delta"""
        C = self.acc_buf.shape[1]
        if niter % self.depth:
            self._read(niter % self.depth)
        acc = np.concatenate(self._acc) if self._acc else np.zeros((0, C), dtype=np.int32)
        deltas = np.concatenate([np.full((1, C), delta0)] + (self._delta if tune_delta else []))
        if C == 1:
            return [int(v) for v in acc[:, 0]], [float(v) for v in deltas[:, 0]]
        return acc, deltas


class PxMALA(MYULA):
    """
    PxMALA = MYULA proposal + Metropolis-Hastings acceptance (pxmcmc/mcmc.py:204-289).

    One iteration is a fixed sequence of device operations on the static buffers of a ``_PxmalaState``, by the route
    chosen once per run (``_route``): ``_iteration_fused`` or ``_iteration_separate`` (the library's own prior), or
    ``_iteration_plugin`` (a user-supplied prior or ``chain_step``).  ``run`` keeps the schedule: a chain saves on an
    accepted candidate.

    :param bool tune_delta: tune ``delta`` towards an acceptance probability of 0.5
    """

    _CHUNK = 1024
    fuse_tail = True  # totals + Metropolis test of an iteration in pxm_pxmala_finish (False: the separate calls, same numbers)

    def __init__(self, forward, prox, mcmcparams=PxMCMCParams(), tune_delta=True, track_transitions=False, max_iter=None,
                 lap_every=0, **kwargs):
        super().__init__(forward, prox, mcmcparams, **kwargs)
        self.tune_delta = tune_delta
        # extension: every ``lap_every`` iterations the loop synchronises the device and appends (iterations done, seconds
        # since the loop started) to ``laps`` -- the time of any stretch of a long run (e.g. after delta has settled)
        # without a second run; 0 = never
        self.lap_every = int(lap_every)
        self.laps = []
        # extension: stop after this many iterations even if fewer than nsamples were saved (the reference's loop,
        # pxmcmc/mcmc.py:230, only ends on accepted samples: a chain that stops accepting never returns)
        self.max_iter = None if max_iter is None else int(max_iter)
        # extension: keep both calc_logtransition values of every iteration in ``transitions_trace`` (a list of
        # (q(X'|X), q(X|X')) complex128 [C] pairs; the static buffers of a graph replay are read after each replay)
        # ... and (prior(X'), L2(X')) of every proposal (pxmcmc/mcmc.py:242) in ``proposals_trace``
        self.track_transitions = bool(track_transitions)
        self.transitions_trace = []
        self.proposals_trace = []

    # ---- the run's device state and its route ---------------------------------------------------------------------------
    def _route(self):
        """which of the ``_iteration_*`` methods steps this run.  Stock prior (library L1 / S2 soft threshold + weighted L1
        norm): the proposal kernel applies it.  With a diagonal inverse covariance too, the totals of the proposal pass are
        deferred and everything between the proposal's gradient and the conditional copy is two launches
        (pxm_pxmala_finish) instead of seven; the sums are added in the same order either way (``fuse_tail = False``: the
        separate calls, bit-identical)."""
        stock = self._fused_prox and type(self.prior).prior is L1.prior
        if not stock:
            return "plugin"
        return "fused" if self.fuse_tail and not hasattr(self.forward.invcov, "matvec") else "separate"

    def _start_state(self, start_point, route, traces):
        C, dev = self.nchains, ops.device()
        X, preds = self._initial_sample(start_point)
        dt = X.dtype
        X = X.contiguous()
        preds = ops.as_device(preds).clone()
        gradg = ops.as_device(self.forward.calc_gradg(preds), dt).clone()
        proxf = ops.as_device(self.prior.proxf(X), dt).clone()
        logpi, L2, prior = self._logpi_dev(X, preds)
        logpi, L2 = logpi.to(torch.complex128).contiguous(), L2.to(torch.complex128).contiguous()
        prior = prior.to(torch.float64).contiguous()
        delta = torch.full((C,), float(self.delta), dtype=torch.float64, device=dev)
        return _PxmalaState((X, preds, gradg, proxf, logpi, L2, prior, delta), C, dev, route, traces, self.prior)

    # ---- one iteration: three routes, one signature; Philox / adaptation use iteration number i_host + *counter ---------
    def _philox_kw(self, i_host):
        return dict(seed=self.seed, chain0=self.chain_offset, it=i_host)

    def _draw_noise(self, st):  # (``rng="numpy"``: the reference's stream, normals before uniforms)
        return self._host_noise(st.X) if self.rng == "numpy" else None

    def _draw_uniforms(self):
        return np.array([np.random.rand() for _ in range(self.nchains)]) if self.rng == "numpy" else None

    def _proposal_model(self, Xp, dt):
        """forward model and gradient of the proposal (pxmcmc/mcmc.py:232-233)"""
        pp = ops.as_device(self.forward.forward(Xp))
        return pp, ops.as_device(self.forward.calc_gradg(pp), dt)

    def _iteration_fused(self, st, i_host, counter, bump=None):
        """stock prior, fused tail: no prox arrays at all -- soft(X, T) is formed where it is needed; with ``bump`` the
        counter advances inside pxm_pxmala_finish"""
        kw = self._philox_kw(i_host)
        ops.pxmala_propose(st.X, None, st.gradg, st.T, st.w_prior, st.delta, self.lmda, st.X_prop, None, None, None,
                           noise=self._draw_noise(st), noise_complex=bool(self.complex), iter_dev=counter,
                           noise64=self.noise64, scratch=st.prop_scratch, **kw)
        Xp = st.X_prop
        pp, gp = self._proposal_model(Xp, st.X.dtype)
        p_, data_, ic_ = self._l2_inputs(pp)
        ops.pxmala_finish(Xp, st.X, None, gp.contiguous(), p_, data_, ic_, st.prop_scratch, self.mu, self.lmda, st.logpi,
                          st.L2, st.prior, st.accept, st.delta, self.tune_delta, st.lt_pc, st.lt_cp, st.prior_p, st.L2_p,
                          st.fin_scratch, u=self._draw_uniforms(), iter_dev=counter, acc_trace=st.acc_trace,
                          delta_trace=st.delta_trace, bump=bump, T=st.T if st.T is not None else 0.0, **kw)
        self._last_transitions = (st.lt_cp, st.lt_pc)
        self._last_proposal = (st.prior_p, st.L2_p)
        ops.select_copy_many(st.accept, [(Xp, st.X), (pp.to(st.preds.dtype), st.preds), (gp, st.gradg)])

    def _iteration_separate(self, st, i_host, counter, bump=None):
        """stock prior, separate calls: proposal + prox + forward transition + prior in one pass, then the tail"""
        kw = self._philox_kw(i_host)
        ops.pxmala_propose(st.X, st.proxf, st.gradg, st.T, st.w_prior, st.delta, self.lmda, st.X_prop, st.proxf_prop,
                           st.lt_cp, st.prior_p, noise=self._draw_noise(st), noise_complex=bool(self.complex),
                           iter_dev=counter, noise64=self.noise64, scratch=None, **kw)
        self._tail_separate(st, counter, kw, st.X_prop, st.proxf_prop, st.lt_cp, st.prior_p)
        if bump is not None:
            st.cnt.add(1)

    def _iteration_plugin(self, st, i_host, counter, bump=None):
        """user-supplied prior / chain_step: the reference's own sequence of calls (pxmcmc/mcmc.py:231-242)"""
        dt, kw = st.X.dtype, self._philox_kw(i_host)
        noise = self._draw_noise(st)  # (drawn whoever steps: the stream does not depend on the route)
        if not self._own_step:
            Xp = ops.chain_step(st.X, st.proxf, st.gradg, st.delta, self.lmda, noise=noise,
                                noise_complex=bool(self.complex), noise64=self.noise64, **kw)
        else:
            Xp = ops.as_device(self.chain_step(st.X, st.proxf, st.gradg), dt)
        pxp = ops.as_device(self.prior.proxf(Xp), dt)
        ltc = ops.logtransition(st.X, Xp, st.proxf, st.gradg, st.delta, self.lmda)
        prp = self.prior.prior(Xp)
        if not isinstance(prp, torch.Tensor):
            prp = torch.as_tensor(np.atleast_1d(np.asarray(prp, dtype=float)), device=ops.device())
        self._tail_separate(st, counter, kw, Xp, pxp, ltc, prp.to(torch.float64).contiguous())

    def _tail_separate(self, st, counter, kw, Xp, pxp, ltc, prp):
        """from the proposal's forward model to the conditional copy of the accepted states, one call per step"""
        pp, gp = self._proposal_model(Xp, st.X.dtype)
        L2p = self._l2_dev(pp)
        ltp = ops.logtransition(Xp, st.X, pxp, gp, st.delta, self.lmda)
        self._last_transitions = (ltc, ltp)  # q(X'|X), q(X|X') of this iteration (pxmcmc/mcmc.py:240-241)
        self._last_proposal = (prp, L2p)
        ops.pxmala_accept(ltp, ltc, prp, L2p, self.mu, st.logpi, st.L2, st.prior, st.accept, st.delta, self.tune_delta,
                          self.lmda, u=self._draw_uniforms(), iter_dev=counter, acc_trace=st.acc_trace,
                          delta_trace=st.delta_trace, **kw)
        ops.select_copy_many(st.accept, [(Xp, st.X), (pp.to(st.preds.dtype), st.preds), (gp, st.gradg), (pxp, st.proxf)])

    def _capture(self, st, route, iteration):
        """HIP graph of one iteration reading the device counter, which it advances itself (device Philox stream and stock
        prior only; any operator that synchronises or cannot be captured falls back to eager stepping -- same results)"""
        self.graph_error = None
        graph = None
        if self.use_graph and self.rng != "numpy" and route != "plugin":
            snap = [t.clone() for t in st.current()]

            def restore():
                for t, s_ in zip(st.current(), snap):
                    t.copy_(s_)

            graphs, self.graph_error = self._engine_capture(
                lambda: iteration(st, 0, st.cnt.t), restore, [lambda: iteration(st, 0, st.cnt.t, bump=st.cnt.t)])
            graph = graphs[0] if graphs else None
            st.cnt.set(0)
        self.used_graph = graph is not None
        return graph

    def run(self, start_point=None):
        """Run the algorithm (pxmcmc/mcmc.py:218-275); every chain carries its own delta and accept flag.

        Prepare, build the state, choose the route, capture, loop, publish.  With the device Philox stream the iteration is
        replayed from a captured HIP graph; the loop synchronises with the device on save candidates (the accept flags),
        laps, progress prints and full trace chunks only."""
        self._prepare()
        self.laps = []
        self._fused_wav = False  # PxMALA needs gradg and proxf of the proposal separately
        C = self.nchains
        traces = _TraceChunks(self._CHUNK, C, ops.device())
        delta0 = float(self.delta)
        route = self._route()
        st = self._start_state(start_point, route, traces)
        iteration = getattr(self, "_iteration_" + route)
        graph = self._capture(st, route, iteration)

        i = 0
        j = np.zeros(C, dtype=int)
        torch.cuda.synchronize()
        t_loop = time.perf_counter()  # (loop_seconds: the iterations alone, without set-up and graph capture)
        while j.min() < self.nsamples and (self.max_iter is None or i < self.max_iter):
            if graph is not None:
                graph.replay()
            else:
                iteration(st, i, None)
            if self.track_transitions:  # observation only (synchronises): both calc_logtransition values per iteration
                self.transitions_trace.append(tuple(t.cpu().numpy().copy() for t in self._last_transitions))
                self.proposals_trace.append(tuple(t.cpu().numpy().copy() for t in self._last_proposal))
            traces.after(i)
            if i >= self.nburn and (self.ngap == 0 or (i - self.nburn) % self.ngap == 0):
                acc_h = st.accept.cpu().numpy()  # the only per-iteration host sync, on save candidates only
                chains = [c for c in range(C) if acc_h[c] and j[c] < self.nsamples]
                if chains:
                    self._check_device_status()
                    self._tracking(j[chains] if C > 1 else int(j[0]), st.X, st.preds, st.logpi, st.L2, st.prior,
                                   chains=chains if C > 1 else None)
                    j[chains] += 1
            if self.lap_every > 0 and (i + 1) % self.lap_every == 0:
                torch.cuda.synchronize()
                self.laps.append((i + 1, time.perf_counter() - t_loop))
            if self.verbosity > 0 and (i + 1) % self.verbosity == 0:
                self._print_progress(int(j[0]) - 1, float(st.logpi[0].real), L2=float(st.L2[0].real), prior=float(st.prior[0]),
                                     acceptanceRate=traces.accepted0(i) / (i + 1))
            i += 1
        torch.cuda.synchronize()
        self.loop_seconds = time.perf_counter() - t_loop
        self.acceptance_trace, self.deltas_trace = traces.result(i, delta0, self.tune_delta)
        self.delta = float(st.delta[0].item())
        self.delta_dev = st.delta
        self._check_device_status()
        self.X_curr, self.curr_preds, self.niter = st.X, st.preds, i
        # rows of chain / logPi / ... beyond nsaved[c] were never written (zeros): a ``max_iter`` stop says so
        self.nsaved = j.copy() if C > 1 else int(j[0])
        self.stopped_early = bool(j.min() < self.nsamples)
        print("\nDONE")

    def _tune_delta(self, i):
        """pxmcmc/mcmc.py:277-279 (host form, one chain; the run loop adapts on the device)."""
        delta = self.delta * (1 + (self.acceptance_trace[i] - 0.5) / ((i + 1) ** 0.75))
        self.delta = min(max(delta, self.lmda * 1e-8), self.lmda / 2)

    def calc_logtransition(self, X1, X2, proxf, gradg):
        """q(X2|X1), literal (pxmcmc/mcmc.py:281-289)."""
        r = ops.logtransition(X1, X2, proxf, gradg, self.delta, self.lmda)
        batched = (X1.dim() if isinstance(X1, torch.Tensor) else np.ndim(X1)) == 2
        if batched:
            return r
        v = complex(r[0].item())
        return v if v.imag != 0 else v.real


def skrock_coefficients(s, eta=0.05):
    """Recursion coefficients of SKROCK (Pereyra, Vargas-Mieles & Zygalakis, SIAM J. Imaging Sci. 13(2), 2020):
    ``(omega_0, omega_1, mus, nus, ks)`` with ``mus / nus / ks`` indexed 0..s (entry 0 unused, as pxmcmc/mcmc.py:370-383).

    omega_0 = 1 + eta / s^2, omega_1 = T_s(omega_0) / T_s'(omega_0); mu_1 = omega_1 / omega_0, nu_1 = s omega_1 / 2,
    kappa_1 = s omega_1 / omega_0; for j >= 2 mu_j = 2 omega_1 T_{j-1}(omega_0) / T_j(omega_0),
    nu_j = 2 omega_0 T_{j-1}(omega_0) / T_j(omega_0), kappa_j = 1 - nu_j."""
    s = int(s)
    w0 = 1 + eta / (s * s)
    T = [1.0, w0]  # T_j(w0) by the three-term recurrence
    U = [1.0, 2 * w0]  # U_j(w0): T_s'(x) = s U_{s-1}(x)
    for _ in range(2, s + 1):
        T.append(2 * w0 * T[-1] - T[-2])
        U.append(2 * w0 * U[-1] - U[-2])
    w1 = T[s] / (s * U[s - 1])
    mus, nus, ks = np.zeros(s + 1), np.zeros(s + 1), np.zeros(s + 1)
    mus[1], nus[1], ks[1] = w1 / w0, s * w1 / 2, s * w1 / w0
    for j in range(2, s + 1):
        ratio = T[j - 1] / T[j]
        mus[j] = 2 * w1 * ratio
        nus[j] = 2 * w0 * ratio
        ks[j] = 1 - nus[j]
    return w0, w1, mus, nus, ks


class SKROCK(PxMCMC):
    """
    The SKROCK chain (pxmcmc/mcmc.py:292-383): ``s`` gradient evaluations per iteration along a Chebyshev recursion, which
    in return admits a step ``delta`` about ``s^2`` times larger on the stiff part of the posterior; no accept step.

    .. note::

       The recursion is the published one (Pereyra, Vargas-Mieles & Zygalakis 2020, :func:`skrock_coefficients`), not
       the reference's literal code, which diverges for ``s >= 2``: it divides by ``T_j(omega_1)`` instead of
       ``T_j(omega_0)`` (mcmc.py:380), sets ``kappa_j = 1 - nu_0`` instead of ``1 - nu_j`` (mcmc.py:383) and adds
       ``kappa_s`` as a scalar minus ``K_{s-2}`` instead of ``kappa_s K_{s-2}`` (mcmc.py:364-367).  For ``s = 1`` the two
       agree exactly.

    One iteration, with ``Z ~ N(0, I)`` (``+ i N(0, I)`` when ``params.complex``) and
    ``grad log pi(U) = -(U - proxf(U)) / lmda - calc_gradg(forward(U))`` (mcmc.py:84-89)::

        K_0 = X
        K_1 = X + mu_1 delta grad log pi(X + nu_1 sqrt(2 delta) Z) + kappa_1 sqrt(2 delta) Z
        K_j = mu_j delta grad log pi(K_{j-1}) + nu_j K_{j-1} + kappa_j K_{j-2}     (j = 2..s)
        X'  = K_s

    Every stage is one HIP kernel (``pxm_skrock_stage``; the stock synthesis L1 prox is formed inside it); the Philox
    noise of stages 0 and 1 is regenerated from the same counters.  ``forward(X')`` is formed only where it is observed.
    The keywords ``nchains / rng / seed / chain_offset / use_graph / noise_bits`` are MYULA's; ``real_pairs`` (and
    ``ring_shortcut``) are accepted and have no effect: the state stays in the reference layout.
    """

    def __init__(self, forward, prox, mcmcparams=PxMCMCParams(), **kwargs):
        super().__init__(forward, prox, mcmcparams, **kwargs)
        s = self.s
        if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer)) or s < 1:
            raise ValueError("SKROCK needs an integer number of stages s >= 1")
        self.s = int(s)
        self.eta = 0.05
        self.omega_0, self.omega_1, self.mus, self.nus, self.ks = skrock_coefficients(self.s, self.eta)
        self._own_step = type(self).chain_step is not SKROCK.chain_step  # a subclass's chain_step: called as it is
        self._it = 0

    # ---- one iteration on device buffers ----------------------------------------------------------------
    def _stage_coefs(self):
        """(a, b, c, e, r) of stage 0, stage 1 and stages 2..s: out = a U + b P + c gradg + e V + r Z"""
        d, l = float(self.delta), self.lmda
        sq = np.sqrt(2 * d)
        m1 = self.mus[1] * d
        coefs = [(1.0, 0.0, 0.0, 0.0, self.nus[1] * sq), (-m1 / l, m1 / l, -m1, 1.0, self.ks[1] * sq)]
        for j in range(2, self.s + 1):
            m = self.mus[j] * d
            coefs.append((self.nus[j] - m / l, m / l, -m, self.ks[j], 0.0))
        return coefs

    def _iterate(self, X, out, Y, KA, KB, noise, it, iter_dev):
        """X' = K_s of one iteration into ``out`` (Y, KA, KB: scratch of X's shape; none of them aliases X or out)"""
        f = self.forward
        coefs = self._stage_coefs()
        T = self.prior.T_dev if self._stock_prox else None
        kw = dict(noise=noise, noise_complex=bool(self.complex), seed=self.seed, chain0=self.chain_offset, it=it,
                  iter_dev=iter_dev, noise64=self.noise64)
        ops.skrock_stage(X, *coefs[0], out=Y, **kw)  # Y = X + nu_1 sqrt(2 delta) Z
        bufs = (out, KA, KB)  # K_j lives in bufs[(s - j) % 3]: K_s lands in out
        s = self.s
        for j in range(1, s + 1):
            U = Y if j == 1 else bufs[(s - j + 1) % 3]
            V = X if j <= 2 else bufs[(s - j + 2) % 3]
            g = ops.as_device(f.calc_gradg(ops.as_device(f.forward(U))), U.dtype)
            px = None if self._stock_prox else ops.as_device(self.prior.proxf(U), U.dtype)
            # (stage 1 regenerates stage 0's Z from the same counters; stages j >= 2 have r = 0: no noise term)
            ops.skrock_stage(U, *coefs[j], T=T, proxf=px, gradg=g, V=V, out=bufs[(s - j) % 3], **kw)
        return out

    def chain_step(self, X):
        """
        Takes a step in the chain (pxmcmc/mcmc.py:338-347): draws Z and runs the s-stage recursion.

        :param X: current sample ([N] or a [C, N] batch; numpy or device array)
        """
        x, squeeze = ops._batched(ops.as_device(X, self._state_dtype(X)))
        noise = None
        if self.rng == "numpy":
            noise = self._host_noise(x)
        else:
            self._it += 1
        Y, KA, KB, out = (torch.empty_like(x) for _ in range(4))
        self._iterate(x, out, Y, KA, KB, noise, self._it, None)
        out = out[0] if squeeze else out
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()

    # ---- stepping engine ------------------------------------------------------------------------------------
    def _engine_start(self, X, preds, i0):
        """static state (XA, XB, P; Y and two rotating K buffers), a device iteration counter and, with the Philox stream,
        captured graphs of 2 and 2 * _GRAPH_PAIRS iterations.  preds (P) is formed on demand only."""
        self._engine_stop()
        X = ops.as_device(X).contiguous()
        Y, KA, KB = (torch.empty_like(X) for _ in range(3))
        numpy_rng = self.rng == "numpy"

        def step(eng, src, dst):
            if self._own_step:  # a subclass's chain_step: eager, through it
                dst.copy_(ops.as_device(self.chain_step(src), dst.dtype))
            else:
                noise = self._host_noise(src) if numpy_rng else None
                self._iterate(src, dst, Y, KA, KB, noise, 0, eng["cnt"].t)
                eng["cnt"].add(1)

        graph_ok = not numpy_rng and self.use_graph and not self._own_step
        return self._engine_start_generic(X, preds, i0, step, lazy=True, graph_ok=graph_ok)

    def run(self, start_point=None):
        """Run the algorithm (pxmcmc/mcmc.py:308-336): the reference's schedule and tracking arrays; iterations between
        two observable events (save / progress print) are advanced together, from a captured HIP graph with the device
        Philox stream."""
        self._it = 0
        X_curr, curr_preds = self._initial_sample(start_point)
        return self._run_engine(X_curr, curr_preds)
