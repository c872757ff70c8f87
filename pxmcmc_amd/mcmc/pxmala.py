"""PxMALA (pxmcmc/mcmc.py:204-289): the run's device state, its trace rings and the three iteration routes."""
import time

import numpy as np
import torch

from .. import ops
from ..prior import L1, L1_Analysis
from .engine import _Counter, capture
from .myula import MYULA
from .params import PxMCMCParams


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
    ``_iteration_plugin`` (a user-supplied prior or ``chain_step``; replayed from a graph too when the prior is the library's
    exact analysis prox, ``_plugin_replayable``).  ``run`` keeps the schedule: a chain saves on an
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

    def _plugin_replayable(self):
        """the plugin route on fixed launches with no host read: the library's exact analysis prox (``prior.L1_Analysis`` and
        its subclasses, ``prior.TV_S2`` among them) under the library's own chain step"""
        return isinstance(self.prior, L1_Analysis) and not self._own_step

    def _iteration_plugin(self, st, i_host, counter, bump=None):
        """user-supplied prior / chain_step: the reference's own sequence of calls (pxmcmc/mcmc.py:231-242)"""
        dt, kw = st.X.dtype, self._philox_kw(i_host)
        noise = self._draw_noise(st)  # (drawn whoever steps: the stream does not depend on the route)
        if not self._own_step:
            Xp = ops.chain_step(st.X, st.proxf, st.gradg, st.delta, self.lmda, noise=noise,
                                noise_complex=bool(self.complex), noise64=self.noise64, iter_dev=counter, **kw)
        else:
            Xp = ops.as_device(self.chain_step(st.X, st.proxf, st.gradg), dt)
        pxp = ops.as_device(self.prior.proxf(Xp), dt)
        ltc = ops.logtransition(st.X, Xp, st.proxf, st.gradg, st.delta, self.lmda)
        prp = self.prior.prior(Xp)
        if not isinstance(prp, torch.Tensor):
            prp = torch.as_tensor(np.atleast_1d(np.asarray(prp, dtype=float)), device=ops.device())
        self._tail_separate(st, counter, kw, Xp, pxp, ltc, prp.to(torch.float64).contiguous())
        if bump is not None:
            st.cnt.add(1)

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
        """HIP graph of one iteration reading the device counter, which it advances itself (device Philox stream; the stock
        prior, or the library's exact analysis prox on the plugin route; any operator that synchronises or cannot be captured
        falls back to eager stepping -- same results)"""
        self.graph_error = None
        graph = None
        if self.use_graph and self.rng != "numpy" and (route != "plugin" or self._plugin_replayable()):
            snap = [t.clone() for t in st.current()]

            def restore():
                for t, s_ in zip(st.current(), snap):
                    t.copy_(s_)

            graphs, self.graph_error = capture(
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
