"""
Maximum-a-posteriori estimation on the samplers' posterior: FISTA (Beck & Teboulle, SIAM J. Imaging Sci. 2(1), 2009) on

    F(X) = g(X) + f(X),   g(X) = 1/2 Re L2(X),   f(X) = (1 / lmda) sum_i T_i |X_i|,   T = prior.T

with the operators' own ``forward`` / ``calc_gradg`` (``calc_gradg(forward(X))`` is the gradient of g) and the prior's own
threshold: f is the potential whose prox MYULA's drift applies, so the estimator finds the mode of the density the chains
sample.  The objective is defined through ``T``, not through ``prior.prior``: ``S2_Wavelets_L1_Power_Weights.prior`` applies
its weights twice, and the estimator minimises the function its prox belongs to.

One iteration is one fused HIP launch (``pxm_fista_step``, or ``pxm_fista_step_restart`` with adaptive restart) around the two
operator calls, replayed from a captured HIP graph by the samplers' stepping engine.
"""
import copy
import warnings

import numpy as np
import torch

from . import ops
from .forward import InverseCovariance
from .mcmc import PxMCMCParams, Stepper


def gradient_operator(forward):
    """The operator whose ``calc_gradg(forward(X))`` is the gradient of ``g = 1/2 Re L2``.  With a real-valued inverse
    covariance that is ``forward`` itself.  With complex data and a real ``sig_d`` the reference's variance rule
    (pxmcmc/forward.py:81-82) makes the inverse covariance ``c = e^{-i pi/4} / sigma^2``; ``Re L2 = sum Re(c) |d|^2`` then
    has the gradient ``Phi^H Re(c) (Phi X - data)``, while ``calc_gradg`` returns the rotated field ``Phi^H c (...)`` on
    which a momentum method is unstable.  For a diagonal inverse covariance a shallow copy of the operator with ``Re(c)`` is
    returned (same transform, measurement and plans); a full complex inverse covariance is refused."""
    inv = getattr(forward, "invcov", None)
    if hasattr(inv, "matvec"):
        if getattr(inv, "is_complex", False) and abs(inv.matrix.imag).max() > 0:
            raise ValueError("FISTA needs a real-valued inverse covariance: with a complex full covariance calc_gradg is "
                             "not the gradient of 1/2 Re L2")
        return forward
    diag = getattr(inv, "diag", None)
    if diag is None or not diag.is_complex() or not bool((diag.imag != 0).any()):
        return forward
    op = copy.copy(forward)
    op.invcov = InverseCovariance(torch.complex(diag.real, torch.zeros_like(diag.real)).contiguous())
    return op


def fista_momentum(n, momentum=True):
    """the table ``beta_k = (t_k - 1) / t_{k+1}``, ``t_0 = 1``, ``t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2`` for k < n
    (all zeros without momentum: plain forward-backward)"""
    beta = np.zeros(int(n))
    if momentum:
        t = 1.0
        for k in range(int(n)):
            t_next = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
            beta[k] = (t - 1.0) / t_next
            t = t_next
    return beta


class FISTA(Stepper):
    """
    MAP point of the posterior of ``(forward, prior, mcmcparams)`` -- the arguments of the samplers -- by FISTA::

        V       = Y_k - gamma calc_gradg(forward(Y_k))
        X_{k+1} = soft(V, gamma T / lmda)
        Y_{k+1} = X_{k+1} + beta_k (X_{k+1} - X_k)

    :param nchains: C start points advanced together as one ``[C, N]`` batch
    :param gamma: step, at most ``1 / L_g``; ``None``: ``1 / forward.gradient_lipschitz(tol=lipschitz_tol)``, shrunk by the
        power iteration's relative tolerance (its estimate approaches ``L_g`` from below)
    :param momentum: ``False`` sets every ``beta_k = 0``: forward-backward splitting, which decreases F monotonically
    :param max_iter: iteration limit (and the length of the momentum table)
    :param tol: stop when ``||X_{k+1} - X_k|| <= tol ||X_{k+1}||`` holds for every chain.  The steps of FISTA shrink like
        ``1 / k`` only (the momentum keeps the iterate moving along directions in which F is flat, such as the null space of
        a redundant frame) while the fixed-point residual is far smaller: ``last_steps`` bounds the latter
    :param check_every: iterations between two checks; between checks the iterations are replayed from the captured graph
    :param use_graph: replay from a captured HIP graph (``False``: the same launches one by one, same results)
    :param restart: ``None``, or ``"gradient"``: adaptive restart (O'Donoghue & Candes 2015), which removes the ``1 / k`` tail.
        Every chain has its own momentum index ``k_c`` on the device and steps with ``beta_{k_c}``; the step also forms
        ``r_c = sum Re conj(Y_k - X_{k+1}) (X_{k+1} - X_k)``, and ``r_c > 0`` sets ``k_c = 0`` (otherwise ``k_c + 1``).  The
        decision is taken on the device after the pass that wrote ``Y_{k+1}``, which keeps its momentum: the reset acts on
        the following step (``beta_0 = 0``, so ``Y_{k+2} = X_{k+2}``), from where the sequence is a fresh FISTA run

    A prior other than the stock synthesis L1 (analysis setting, user prior) is applied through its own ``proxf(V)``, whose
    threshold is the prior's (the prox of ``lmda f``): the iteration then minimises ``g + (lmda / gamma) f``, which is not
    the posterior's MAP unless ``gamma = lmda``, and the prior term and the objective are not formed (NaN in the traces).
    A ``UserWarning`` says so at construction.

    The gradient is taken on :func:`gradient_operator` ``(forward)``: with a complex inverse covariance (complex data and
    a real ``sig_d``) that is the operator with ``Re(invcov)``, whose ``calc_gradg`` is the gradient of ``1/2 Re L2``.

    After :meth:`run`: ``objective``, ``data_term``, ``prior_term``, ``rel_change`` (one ``[C]`` row per check, arrays
    ``[nchecks, C]``), ``checks`` (iterations done at each check), ``niter`` and ``converged`` (per chain), ``X_map`` /
    ``preds_map`` (device arrays), ``objective_map`` (``[C]``), ``used_graph`` and ``last_steps`` (``[C, 2]``: the lengths
    ``||X_K - X_{K-1}||`` and ``||X_{K-1} - X_{K-2}||`` of the last two steps, which bound the fixed-point residual of the
    returned point: ``||X_K - P(X_K)|| <= ||X_K - X_{K-1}|| + beta ||X_{K-1} - X_{K-2}||`` for the nonexpansive step map P).
    With ``restart``: also ``restarts`` (``[nchecks, C]``, restarts so far at each check) and ``nrestarts`` (``[C]``).
    """

    lipschitz_tol = 1e-4

    def __init__(self, forward, prior, mcmcparams=PxMCMCParams(), nchains=1, gamma=None, momentum=True, max_iter=10000,
                 tol=1e-4, check_every=10, use_graph=True, restart=None):
        super().__init__(forward, prior, mcmcparams, nchains=nchains, use_graph=use_graph)
        if int(max_iter) < 1 or int(check_every) < 1:
            raise ValueError("FISTA needs max_iter >= 1 and check_every >= 1")
        if restart not in (None, "gradient"):
            raise ValueError('FISTA: restart is None or "gradient"')
        if restart and not momentum:
            raise ValueError("FISTA: restart needs momentum (forward-backward has none to reset)")
        self.restart = restart
        self.gradient_op = gradient_operator(forward)
        if not self._stock_prox:
            warnings.warn("FISTA: the prior is not the stock synthesis L1, so its own proxf (the prox of lmda f) is applied: the "
                          "iteration minimises g + (lmda / gamma) f, not the posterior, and no objective is recorded")
        if gamma is None:
            gamma = 1.0 / (self.gradient_op.gradient_lipschitz(iters=1000, tol=self.lipschitz_tol) * (1.0 + self.lipschitz_tol))
        if not (np.isfinite(gamma) and gamma > 0):
            raise ValueError("FISTA needs a positive step gamma")
        self.gamma = float(gamma)
        self.momentum = bool(momentum)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.check_every = int(check_every)
        self.beta = fista_momentum(self.max_iter, self.momentum)

    def _engine_start(self, X, preds, i0):
        """static state (XA, XB, P) plus the extrapolated point in YA / YB -- Y of the state in XA lives in YA, of XB in YB --
        the per-chain sums and the momentum table on the device; the kernel reads beta_k at the engine's device counter, or,
        with restart, at the chain's own momentum index, which the step itself advances or resets"""
        self._engine_stop()
        X = ops.as_device(X).contiguous()
        f, gamma, lmda = self.gradient_op, self.gamma, self.lmda
        YA, YB, V = X.clone(), torch.empty_like(X), torch.empty_like(X)
        beta = ops.as_device(self.beta, torch.float64)
        # sums of the step that wrote XA in _sums[0], of the step that wrote XB in _sums[1]: the last two steps' sums
        C, restart = X.shape[0], self.restart is not None
        self._sums = torch.zeros((2, C, 4 if restart else 3), dtype=torch.float64, device=X.device)
        scratch = (ops.fista_restart_scratch if restart else ops.fista_scratch)(C, X.device)
        T = self.prior.T_dev if self._stock_prox else None
        # restart: the chains' momentum indices and restart counts (the library reads them as uint64)
        self._momentum_index = torch.zeros(C, dtype=torch.int64, device=X.device) if restart else None
        self._restarts = torch.zeros(C, dtype=torch.int64, device=X.device) if restart else None

        def step(eng, src, dst):
            Y, Y_next = (YA, YB) if src is eng.XA else (YB, YA)
            g = ops.as_device(f.calc_gradg(ops.as_device(f.forward(Y))), src.dtype)
            kw = dict(out=(dst, Y_next), sums=self._sums[0 if dst is eng.XA else 1], scratch=scratch)
            if self._stock_prox:
                kw["T"] = T
            else:
                ops.skrock_stage(Y, 1.0, c=-gamma, gradg=g, out=V)  # V = Y - gamma gradg
                kw["proxf"] = ops.as_device(self.prior.proxf(V), src.dtype)
            if restart:  # Y is passed next to a given proxf too: the restart sum reads it
                ops.fista_step_restart(Y, g, src, gamma, lmda, beta, self._momentum_index, restarts=self._restarts, **kw)
            elif self._stock_prox:
                ops.fista_step(Y, g, src, gamma, lmda, beta, iter_dev=eng.cnt.t, **kw)
            else:
                ops.fista_step(None, None, src, gamma, lmda, beta, iter_dev=eng.cnt.t, **kw)
            eng.cnt.add(1)

        def reset(eng):
            YA.copy_(eng.XA)
            self._sums.zero_()
            if restart:
                self._momentum_index.zero_()
                self._restarts.zero_()

        return self._engine_start_generic(X, preds, i0, step, lazy=True, graph_ok=self.use_graph, reset=reset)

    def run(self, start_point=None):
        """Iterate from ``start_point`` (``[N]``, or ``[C, N]`` with one row per chain; ``None``: zero) until every chain meets
        the stopping rule or ``max_iter`` is reached.  Returns the MAP point in the caller's array kind (numpy, or a device
        tensor for a tensor start point): ``[N]`` for one chain, ``[C, N]`` for a batch."""
        C = self.nchains
        as_torch = isinstance(start_point, torch.Tensor)
        if start_point is None:
            start_point = np.zeros(self.forward.nparams)
        X, preds = self._initial_sample(start_point)
        self._engine_start(X, preds, 0)
        traces = {k: [] for k in ("objective", "data_term", "prior_term", "rel_change")}
        restarts = []
        self.checks = []
        niter = np.zeros(C, dtype=int)
        met = np.zeros(C, dtype=bool)
        try:
            i = 0
            while i < self.max_iter:
                k = min(self.check_every, self.max_iter - i)
                self._engine_advance(k)
                i += k
                X, preds = self._engine_state()  # forward(X) is formed here, where the state is observed
                self._check_device_status()
                last = 0 if self._eng.side == "A" else 1
                both = self._sums.cpu().numpy()
                s, s_prev = both[last], both[1 - last]
                with np.errstate(invalid="ignore", divide="ignore"):
                    rel = np.where(s[:, 0] == 0.0, 0.0, np.sqrt(s[:, 0]) / np.sqrt(s[:, 1]))
                data_term = 0.5 * self._l2_dev(preds).real.cpu().numpy()
                prior_term = s[:, 2] / self.lmda
                now = rel <= self.tol
                niter = np.where(now & met, niter, i)  # iterations done when the chain first met (and kept) the rule
                met = now
                self.checks.append(i)
                for key, v in zip(traces, (data_term + prior_term, data_term, prior_term, rel)):
                    traces[key].append(np.array(v, dtype=float))
                if self.restart:
                    restarts.append(self._restarts.cpu().numpy().copy())
                if met.all():
                    break
            self.X_map, self.preds_map = X.clone(), preds.clone()
            self.last_steps = np.sqrt(np.stack([s[:, 0], s_prev[:, 0]], axis=1))
            self.used_graph = self._eng.graph is not None
            self.graph_error = self._eng.graph_error
        finally:
            self._engine_stop()
        for key, rows in traces.items():
            setattr(self, key, np.stack(rows))
        self.niter, self.converged = niter, met
        if self.restart:
            self.restarts = np.stack(restarts)
            self.nrestarts = self.restarts[-1]
        self.objective_map = self.objective[-1]
        out = self.X_map if C > 1 else self.X_map[0]
        return out.clone() if as_torch else out.cpu().numpy()
