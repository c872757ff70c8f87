"""The sampler base: tracking arrays, streaming summaries of the saved samples and the reference's save / print schedule
on the stepping engine."""
import numpy as np
import torch

from .. import ops
from .params import PxMCMCParams
from .stepper import Stepper


class PxMCMC(Stepper):
    """
    Base class with the general functions (pxmcmc/mcmc.py:46-140).

    :param forward: :class:`forward.ForwardOperator`-like object
    :param prior: prior object implementing ``prior`` and ``proxf``
    :param mcmcparams: :class:`PxMCMCParams`
    """

    def __init__(self, forward, prior, mcmcparams=PxMCMCParams(), nchains=1, rng="philox", seed=0, chain_offset=0,
                 use_graph=True, ring_shortcut=True, real_pairs=True, noise_bits=64, summary=None, summary_alpha=None,
                 summary_ess=None):
        super().__init__(forward, prior, mcmcparams, nchains=nchains, rng=rng, seed=seed, chain_offset=chain_offset,
                         use_graph=use_graph, ring_shortcut=ring_shortcut, real_pairs=real_pairs, noise_bits=noise_bits)
        self._summary_spaces = self._summary_arg(summary)
        self.summary = {} if self._summary_spaces else None
        self._summary_plan = None
        if summary_alpha is not None:
            from ..uncertainty import tail_capacity

            if not self._summary_spaces:
                raise ValueError("summary_alpha needs summary: the tails are part of the streaming summaries")
            tail_capacity(summary_alpha, self.nsamples)  # (validates alpha and nsamples)
        self.summary_alpha = None if summary_alpha is None else float(summary_alpha)
        if summary_ess is not None:
            from ..uncertainty import ess_lag_count

            if not self._summary_spaces:
                raise ValueError("summary_ess needs summary: the lagged products are part of the streaming summaries")
            summary_ess = ess_lag_count(summary_ess)
        self.summary_ess = summary_ess
        self._initialise_tracking_arrays()

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
        eng = self._eng
        if eng is not None and eng.plan is not None and eng.plan is getattr(tr, "_plan", None):
            if self._summary_plan is None:
                self._summary_plan = tr._make_plan(self.nchains)
            return self._summary_plan.synthesis(S)
        return ops.as_device(tr.inverse(S))

    def _summary_update(self, X_curr, logPi, chains):
        """the samples being saved -> the summaries (created at the first save of a run, when shapes and device are known).
        The state summary of a full save (MYULA, SKROCK) allocates and copies nothing.  A partial save (PxMALA's ``chains``)
        uploads a [C] mask, at a point where that loop has just read the accept flags back; the image summary allocates the
        images, and with ``params.complex = False`` the real-part copy of the state they are synthesised from."""
        from ..uncertainty import PosteriorSummary

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

    def _initial_sample(self, initial_sample=None):
        if self._summary_spaces:
            self.summary = {}  # start of a run: its summaries begin empty
        return super()._initial_sample(initial_sample)

    # ---- what a run reports ------------------------------------------------------------------------------------------
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

    def _run_engine(self, X_curr, curr_preds):
        """
        Same schedule as the reference loop (pxmcmc/mcmc.py:157-181), but iterations between two events
        (save / progress print) are advanced together: by HIP-graph replays when capture is available.
        """
        nburn, ngap, verb = int(self.nburn), int(self.ngap), int(self.verbosity)
        eng = self._engine_start(X_curr, curr_preds, 0)
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
                eng.advance(stop - i + 1)  # run iterations i..stop
                i = stop
                X_curr, curr_preds = eng.state()
                if i >= nburn:
                    if ngap == 0 or (i - nburn) % ngap == 0:
                        if eng.plan is None:  # steps on the operators' own plans: poll those
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
            X_curr, curr_preds = eng.state()
            self._check_device_status()
            self.X_curr, self.curr_preds, self.niter = X_curr.clone(), curr_preds.clone(), i
            self.used_graph = eng.graph is not None
            self.graph_error = eng.graph_error
        finally:
            self._engine_stop()
        print("\nDONE")
