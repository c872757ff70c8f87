"""
Maximum-a-posteriori estimation on the samplers' posterior: FISTA (Beck & Teboulle, SIAM J. Imaging Sci. 2(1), 2009) on

    F(X) = g(X) + f(X),   g(X) = 1/2 Re L2(X),   f(X) = (1 / lmda) sum_i T_i |X_i|,   T = prior.T

with the operators' own ``forward`` / ``calc_gradg`` (``calc_gradg(forward(X))`` is the gradient of g) and the prior's own
threshold: f is the potential whose prox MYULA's drift applies, so the estimator finds the mode of the density the chains
sample.  The objective is defined through ``T``, not through ``prior.prior``: ``S2_Wavelets_L1_Power_Weights.prior`` applies
its weights twice, and the estimator minimises the function its prox belongs to.

One iteration is one fused HIP launch (``pxm_fista_step``, or ``pxm_fista_step_restart`` with adaptive restart) around the two
operator calls, replayed from a captured HIP graph by the samplers' stepping engine.

In the analysis setting the prior acts on ``A X`` (``A = prior.adj``, ``A^H = prior.fwd``) and the soft threshold is not its
prox unless ``A A^H = I``: :class:`PrimalDual` minimises ``g(X) + (1 / lmda) sum_i T_i |(A X)_i|`` exactly by primal-dual
splitting on two fused HIP launches per iteration, and :func:`analysis_prox` is the exact prox of the analysis prior
(DESIGN.md section 14d).  ``optim_np`` states both in numpy.

A prior with ``pairs = True`` (isotropic total variation, ``prior.TV_S2``) has two-plane coefficients
``[C, 2 m]`` and takes the norm over a pixel's pair: ``h(u) = (1 / lmda) sum_i T_i ||u_i||``, ``T`` a float or ``[m]``.  Both
solvers then project pair by pair (``ops.pd_dual_step_pairs``), and run on the prior's own fused launches when it offers them
(``fused_primal_step``, ``fused_dual_step``).  ``tv_np`` states the pair forms in numpy.
"""
import copy
import warnings

import numpy as np
import torch

from . import ops
from .forward import InverseCovariance, power_iteration
from .mcmc import PxMCMCParams, Stepper
from .ops.cg import CG_BNORM2, CG_FLAGS, CG_ITERS, CG_RHO
from .utils import to_like


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


# ---- Gaussian prior: the exact posterior by batched conjugate gradients --------------------------------
class GaussianPosterior(Stepper):
    """
    The posterior of ``(forward, prior, mcmcparams)`` with a :class:`pxmcmc_amd.prior.Gaussian` prior,

        F(X) = 1/2 Re L2(X) + (T / lmda) 1/2 sum_i p_i |X_i|^2,

    is Gaussian with precision ``H = D + A``: ``D = (T / lmda) p`` and ``A`` the linear part of
    ``x -> calc_gradg(forward(x))``, taken on :func:`gradient_operator` ``(forward)``.  :meth:`run` solves ``H x = b0``,
    ``b0 = -calc_gradg(forward(0))``, for the MAP point, which is the posterior mean (the Wiener filter); :meth:`sample` gives
    exact, independent draws by perturbation-optimisation (Papandreou & Yuille 2010; Orieux, Feron & Giovannelli 2012): the
    same system with the right-hand side ``b0 + Phi^H sqrt(W) omega_1 + sqrt(D) omega_2``, whose covariance is ``H``.

    Every chain of the batch is its own system, solved by the single-reduction preconditioned conjugate gradients of
    Chronopoulos & Gear (1989): one iteration is the operator pair and two HIP launches (``pxm_cg_apply``,
    ``pxm_cg_update``); the step lengths, the convergence freeze and the breakdown guard are per chain and on the device, so
    the iteration is replayed from a captured HIP graph between checks.  ``cg_np`` states it in numpy.

    :param nchains: C systems solved together as one ``[C, N]`` batch (C draws per solve)
    :param tol: a chain is frozen once its recurrence residual satisfies ``||r|| <= tol ||b||``
    :param max_iter: iteration limit
    :param check_every: iterations between two reads of the per-chain coefficients by the host
    :param precond: ``"diag"``: ``M = D + h`` with ``h`` a Hutchinson estimate of ``trace(A) / N`` from 8 Philox Gaussian
        probes through the operator, formed once here; ``None``: the identity; a positive vector ``[N]``: ``M^-1`` itself
    :param use_graph: replay from a captured HIP graph (``False``: the same launches one by one, same results)
    :param seed, chain_offset: draw ``k`` of chain ``c`` uses the float64 Philox stream at ``(seed, chain_offset + c)``,
        iterations ``2 k`` (``omega_1``, data length) and ``2 k + 1`` (``omega_2``, state length)

    Real states (``params.complex = False``, real data, an operator that keeps them real) and complex128 states are both
    supported.  After :meth:`run`: ``niter``, ``converged``, ``breakdown`` (per chain), ``rel_residual`` (``[nchecks, C]``:
    ``||r|| / ||b||`` of the recurrence residual at the last decision before each check), ``checks``, ``X_map`` / ``preds_map``
    (device arrays), ``objective_map`` (``[C]``) and ``used_graph``.  After :meth:`sample`: the same per-chain records of the
    last solve, and ``solve_iterations`` and ``solve_converged`` (``[nsolves, C]``).
    """

    HUTCHINSON_PROBES = 8
    _PROBE_ITER = 1 << 62  # Philox iteration of the probes: off the draws' iterations 2 k, 2 k + 1

    def __init__(self, forward, prior, mcmcparams=PxMCMCParams(), nchains=1, tol=1e-8, max_iter=1000, check_every=10,
                 precond="diag", use_graph=True, seed=0, chain_offset=0):
        if not hasattr(prior, "precision") or getattr(prior, "T", None) is None:
            raise ValueError("GaussianPosterior needs a prior with precision and T (prior.Gaussian)")
        super().__init__(forward, prior, mcmcparams, nchains=nchains, seed=seed, chain_offset=chain_offset, use_graph=use_graph)
        self._solver_setup(tol, max_iter, check_every)
        n, dt = self._n, self._dt
        p = np.asarray(prior.precision, dtype=float)
        if p.ndim and p.size != n:
            raise ValueError(f"GaussianPosterior: the precision has {p.size} entries, the state {n}")
        if not np.all(np.isfinite(p)) or np.any(p < 0):
            raise ValueError("GaussianPosterior: the precision must be finite and not negative")
        scale = float(prior.T) / float(self.lmda)
        self._D = float(p.reshape(-1)[0]) * scale if p.ndim == 0 or n == 1 else ops.as_device(p * scale, torch.float64)
        self._solver_rhs()
        self.precond = precond if precond is None or isinstance(precond, str) else "given"
        self._minv = self._preconditioner(precond)

    def _solver_setup(self, tol, max_iter, check_every):
        """what the solver needs of its arguments whatever the prior: the limits, the gradient operator, the state's size and dtype"""
        name = type(self).__name__
        if int(max_iter) < 1 or int(check_every) < 1:
            raise ValueError(f"{name} needs max_iter >= 1 and check_every >= 1")
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError(f"{name} needs a finite tol >= 0")
        self.tol, self.max_iter, self.check_every = float(tol), int(max_iter), int(check_every)
        self.gradient_op = gradient_operator(self.forward)
        self._n, self._dt = int(self.forward.nparams), self._state_dtype()

    def _solver_rhs(self):
        """``b0 = -calc_gradg(forward(0))``"""
        zero = torch.zeros((1, self._n), dtype=self._dt, device=ops.device())
        self._b0 = torch.zeros(self._n, dtype=self._dt, device=zero.device)
        ops.skrock_stage(self._linear(zero), -1.0, out=self._b0)

    def _state_dtype(self, start=None):
        """complex128 when ``params.complex``, the data or the start point is complex, or when the state is the coefficients
        of a wavelet or harmonic transform (synthesis setting); float64 otherwise"""
        from .transforms import SphericalHarmonicTransform, SphericalWaveletTransform

        f = self.forward
        cplx = bool(self.complex) or (getattr(f, "setting", "synthesis") == "synthesis" and isinstance(
            getattr(f, "transform", None), (SphericalWaveletTransform, SphericalHarmonicTransform)))
        for a in (f.data, start):
            if a is not None:
                cplx = cplx or (a.is_complex() if isinstance(a, torch.Tensor) else np.iscomplexobj(a))
        return torch.complex128 if cplx else torch.float64

    def _linear(self, v):
        """``calc_gradg(forward(v)) = A v - b0`` of a ``[C, N]`` device batch, in the state's dtype"""
        f = self.gradient_op
        return ops.as_device(f.calc_gradg(ops.as_device(f.forward(v))), self._dt)

    def _preconditioner(self, precond):
        """``M^-1`` as the update launch takes it: a float or a float64 ``[N]`` device vector"""
        n, D = self._n, self._D
        if precond is None:
            self.trace_estimate = None
            return 1.0
        if isinstance(precond, str):
            if precond != "diag":
                raise ValueError('GaussianPosterior: precond is "diag", None or a positive vector [nparams]')
            num = den = 0.0
            for k in range(self.HUTCHINSON_PROBES):
                z = ops.randn(n, 1, complex_=self._dt.is_complex, seed=self.seed, chain0=k, it=self._PROBE_ITER, noise64=True)
                Az = ops.cg_rhs(z, B=self._b0, G=self._linear(z))
                num += float(ops.reduce_vdot(z, Az)[0].real)
                den += float(ops.reduce_vdot(z, z)[0].real)
            h = num / den if den > 0 else 0.0
            self.trace_estimate = h
            M = D + h
            if isinstance(M, float):
                if not (np.isfinite(M) and M > 0):
                    raise ValueError("GaussianPosterior: the diagonal preconditioner D + trace(A) / N is not positive")
                return 1.0 / M
            if not bool((M > 0).all()):
                raise ValueError("GaussianPosterior: the diagonal preconditioner D + trace(A) / N is not positive")
            return (1.0 / M).contiguous()
        m = np.asarray(precond.cpu() if isinstance(precond, torch.Tensor) else precond, dtype=float)
        if m.ndim != 1 or m.size != n:
            raise ValueError(f"GaussianPosterior: a given precond is M^-1 as a vector of the state's length {n}, got shape {m.shape}")
        if not np.all(np.isfinite(m)) or np.any(m <= 0):
            raise ValueError("GaussianPosterior: a given precond must be positive and finite")
        self.trace_estimate = None
        return float(m[0]) if n == 1 else ops.as_device(m, torch.float64)

    # ---- the iteration on the stepping engine -----------------------------------------------------------------------------
    def _engine_start(self, X, preds=None, i0=0):
        """static state (XA, XB) plus the residual R, U = M^-1 R, the directions P and S, the work array W and the per-chain
        coefficients; P of the engine is not carried (the solver forms forward(X) once, at the end of :meth:`run`).
        :meth:`_load` puts the system into the static buffers; every solve starts an engine of its own"""
        self._engine_stop()
        X = ops.as_device(X).contiguous()
        C = X.shape[0]
        self._R, self._U, self._P, self._S, self._W = (torch.zeros_like(X) for _ in range(5))
        self._R0, self._U0 = torch.zeros_like(X), torch.zeros_like(X)
        self._coef = ops.cg_coef(torch.zeros(C, dtype=torch.float64, device=X.device))
        self._coef0 = self._coef.clone()
        scratch = ops.cg_scratch(C, X.device)
        R, U, P, S, W, coef, b0, D, minv, tol = self._R, self._U, self._P, self._S, self._W, self._coef, self._b0, self._D, self._minv, self.tol

        def step(eng, src, dst):
            ops.cg_apply(U, self._linear(U), b0, D, R, coef, tol, out=W, scratch=scratch)
            ops.cg_update(U, W, P, S, src, R, minv, coef, out=dst)

        def reset(eng):
            R.copy_(self._R0)
            U.copy_(self._U0)
            P.zero_()
            S.zero_()
            coef.copy_(self._coef0)

        no_preds = torch.zeros((C, 0), dtype=X.dtype, device=X.device)
        return self._engine_start_generic(X, no_preds, i0, step, lazy=False, graph_ok=self.use_graph, reset=reset)

    def _load(self, B, X0=None):
        """a new system into the engine: right-hand sides ``B`` ``[C, N]``, start ``X0`` (None: zero, so ``r = b``)"""
        eng = self._eng
        if X0 is None:
            eng.XA.zero_()
            self._R0.copy_(B)
        else:
            eng.XA.copy_(X0)
            HX = ops.cg_rhs(B, B=self._b0, G=self._linear(eng.XA), Z=eng.XA, S=self._D)
            ops.skrock_stage(B, 1.0, e=-1.0, V=HX, out=self._R0)
        ops.cg_rhs(B, Z=self._R0, S=self._minv, out=self._U0)
        self._coef0.zero_()
        self._coef0[:, CG_BNORM2] = self._reference_norm2(B)
        eng.side = "A"
        eng.reset()

    def _reference_norm2(self, B):
        """``||b||^2`` of the stop rule ``||r|| <= tol ||b||``, per chain: of the right-hand sides themselves"""
        return ops.reduce_vdot(B, B).real

    def _iterate(self):
        """advance until every chain is frozen or ``max_iter`` -> (X, coefficients on the host, residual rows, checks)"""
        rows, checks, i = [], [], 0
        while i < self.max_iter:
            k = min(self.check_every, self.max_iter - i)
            self._engine_advance(k)
            i += k
            self._check_device_status()
            coef = self._coef.cpu().numpy()
            with np.errstate(invalid="ignore", divide="ignore"):
                rows.append(np.where(coef[:, CG_BNORM2] > 0, np.sqrt(coef[:, CG_RHO] / coef[:, CG_BNORM2]), 0.0))
            checks.append(i)
            if (coef[:, CG_FLAGS] != 0).all():
                break
        eng = self._eng
        return (eng.XA if eng.side == "A" else eng.XB), coef, np.stack(rows), checks

    def _record(self, coef, rows, checks):
        flags = coef[:, CG_FLAGS].astype(int)
        self.niter = coef[:, CG_ITERS].astype(int)
        self.breakdown = (flags & ops.CG_BREAKDOWN) != 0
        self.converged = ((flags & ops.CG_FROZEN) != 0) & ~self.breakdown
        self.rel_residual, self.checks = rows, checks
        self.used_graph = self._eng.graph is not None
        self.graph_error = self._eng.graph_error

    def run(self, start_point=None):
        """Solve ``H x = b0`` from ``start_point`` (``[N]``, or ``[C, N]`` with one row per chain; ``None``: zero).  Returns the
        MAP point, which is the posterior mean, in the caller's array kind (numpy, or a device tensor for a tensor start
        point): ``[N]`` for one chain, ``[C, N]`` for a batch."""
        C = self.nchains
        as_torch = isinstance(start_point, torch.Tensor)
        zero_start = start_point is None
        if zero_start:
            start_point = np.zeros(self.forward.nparams)
        X0, _ = self._initial_sample(start_point)
        self._engine_start(X0)
        try:
            B = ops.cg_rhs(X0, B=self._b0)
            self._load(B, None if zero_start else X0)
            X, coef, rows, checks = self._iterate()
            self._record(coef, rows, checks)
            self.X_map = X.clone()
            self.preds_map = ops.as_device(self.forward.forward(self.X_map)).clone()
        finally:
            self._engine_stop()
        data_term = 0.5 * self._l2_dev(self.preds_map).real.cpu().numpy()
        prior_term = np.atleast_1d(ops.as_device(self.prior.prior(self.X_map)).cpu().numpy()) * (float(self.prior.T) / self.lmda)
        self.data_term, self.prior_term = data_term, prior_term
        self.objective_map = data_term + prior_term
        out = self.X_map if C > 1 else self.X_map[0]
        return out.clone() if as_torch else out.cpu().numpy()

    def _draw_operands(self):
        """``(s, sqrt(D))`` of the draws' right-hand sides: ``s = 1 / sqrt(w)`` where the data weight ``w = Re(invcov) > 0``,
        else 0 (masked data need no special case)"""
        inv = self.gradient_op.invcov
        if hasattr(inv, "matvec") or not hasattr(inv, "diag"):
            raise ValueError("GaussianPosterior.sample needs a diagonal inverse covariance: the data perturbation "
                             "sqrt(W) omega_1 is formed element by element (run() accepts a full covariance)")
        w = ops.as_device(inv.diag).real.to(torch.float64).reshape(-1)
        if bool((w < 0).any()):
            raise ValueError("GaussianPosterior.sample: the data weights Re(invcov) must not be negative")
        s = torch.where(w > 0, 1.0 / torch.sqrt(torch.where(w > 0, w, torch.ones_like(w))), torch.zeros_like(w)).contiguous()
        D = self._D
        return s, (float(np.sqrt(D)) if isinstance(D, float) else torch.sqrt(D).contiguous())

    def draw_rhs(self, k):
        """the right-hand sides ``[C, N]`` of draw ``k`` of every chain (device array): ``b0 + calc_gradg(data + s o omega_1)
        + sqrt(D) o omega_2`` with the deviates of the Philox iterations ``2 k`` and ``2 k + 1``.  ``omega_2``, and ``omega_1``
        with it, is complex when the state is: the perturbations then cover the real and the imaginary part of ``F``."""
        g, w2, sqrtD = self._draw_parts(k)
        return ops.cg_rhs(w2, B=self._b0, G=g, Z=w2, S=sqrtD)

    def _draw_parts(self, k):
        """``(calc_gradg(data + s o omega_1), omega_2, sqrt(D))`` of draw ``k``"""
        if getattr(self, "_draw_ops", None) is None:
            self._draw_ops = self._draw_operands()
        s, sqrtD = self._draw_ops
        C, cplx = self.nchains, self._dt.is_complex
        kw = dict(complex_=cplx, seed=self.seed, chain0=self.chain_offset, noise64=True)
        w1 = ops.randn(s.numel(), C, it=2 * int(k), **kw)
        if self.forward.data_dev.is_complex() and not cplx:  # (real state, complex data: the predictions carry the data)
            w1 = w1.to(torch.complex128)
        g = ops.as_device(self.gradient_op.calc_gradg(ops.cg_rhs(w1, B=self.forward.data_dev, Z=w1, S=s)), self._dt)
        return g, ops.randn(self._n, C, it=2 * int(k) + 1, **kw), sqrtD

    def sample(self, ndraws, summary=None, summary_ess=None, summary_alpha=None, first_draw=0, as_torch=False):
        """``ndraws`` exact, independent draws of the posterior, C per solve (draw ``first_draw + k`` of chain ``c`` is row
        ``k C + c``).  Returns them as ``[ndraws, N]`` (numpy, or a device tensor with ``as_torch``).  With ``summary="state"``
        or ``"image"`` (``transform.inverse`` of the draws) every batch of C draws is folded into a
        :class:`pxmcmc_amd.uncertainty.PosteriorSummary` instead, which is returned: its moments, R-hat, ESS (with
        ``summary_ess`` lags) and tails (with ``summary_alpha``) read out as after a sampler run, ``ceil(ndraws / C)`` samples
        per chain.  Two calls with the same ``seed``, ``chain_offset`` and ``first_draw`` return the same bits."""
        if summary not in (None, "state", "image"):
            raise ValueError("summary must be None, 'state' or 'image'")
        if int(ndraws) < 1:
            raise ValueError("sample needs ndraws >= 1")
        self._draw_ops = self._draw_operands()
        C, n = self.nchains, self._n
        nsolves = -(-int(ndraws) // C)
        tr = getattr(self.forward, "transform", None)
        if summary == "image" and (getattr(self.forward, "setting", "synthesis") == "analysis" or not hasattr(tr, "inverse")):
            raise ValueError("summary='image' needs forward.transform.inverse in the synthesis setting")
        post = None
        out = None if summary else torch.empty((nsolves * C, n), dtype=self._dt, device=ops.device())
        start = torch.zeros((C, n), dtype=self._dt, device=ops.device())
        self._engine_start(start)
        its, ok = [], []
        try:
            for k in range(nsolves):
                # one engine, and so one capture, per solve: the first iterations of a system loaded into an engine whose graph
                # had replayed before came out wrong on the MI355X
                if k:
                    self._engine_start(start)
                self._load(self.draw_rhs(int(first_draw) + k))
                X, coef, rows, checks = self._iterate()
                self._record(coef, rows, checks)
                its.append(self.niter.copy())
                ok.append(self.converged.copy())
                if self.breakdown.any() or not self.converged.all():
                    warnings.warn(f"GaussianPosterior.sample: solve {k} did not converge for every chain (breakdown: "
                                  f"{self.breakdown.tolist()}, relative residuals {rows[-1].tolist()})")
                if summary is None:
                    out[k * C:(k + 1) * C].copy_(X)
                    continue
                S = X if summary == "state" else ops.as_device(tr.inverse(X))
                if post is None:
                    from .uncertainty import PosteriorSummary

                    post = PosteriorSummary(C, S.shape[1], S.is_complex(), best=False, alpha=summary_alpha, nsamples=nsolves,
                                            ess_lags=summary_ess)
                post.update(S)
        finally:
            self._engine_stop()
        self.solve_iterations, self.solve_converged = np.stack(its), np.stack(ok)
        if summary:
            return post
        out = out[:int(ndraws)]
        return out.clone() if as_torch else out.cpu().numpy()


    def _gibbs_run(self, nsweeps, nburn, summary, summary_ess, summary_alpha, as_torch, prepare, draw):
        """The sweep loop the Gibbs samplers on this solver share (:class:`GaussianGibbs`, :class:`LassoGibbs`): the exact draw
        of the field at the chains' current diagonals, then ``draw(t, X, kept)``, the conditional draw of the precisions given
        the field ``X`` of sweep ``t``, which rewrites the diagonals in place.  ``prepare(nsweeps, keep)`` runs once the
        arguments are checked and sets the initial diagonals.  Returns what ``run`` returns: the kept field draws, or their
        ``PosteriorSummary``."""
        name = type(self).__name__
        if summary not in (None, "state", "image"):
            raise ValueError("summary must be None, 'state' or 'image'")
        nsweeps, nburn = int(nsweeps), int(nburn)
        if nsweeps < 1 or not 0 <= nburn < nsweeps:
            raise ValueError("run needs nsweeps >= 1 and 0 <= nburn < nsweeps")
        tr = getattr(self.forward, "transform", None)
        if summary == "image" and (getattr(self.forward, "setting", "synthesis") == "analysis" or not hasattr(tr, "inverse")):
            raise ValueError("summary='image' needs forward.transform.inverse in the synthesis setting")
        C, n, keep = self.nchains, self._n, nsweeps - nburn
        dev = ops.device()
        prepare(nsweeps, keep)
        self._draw_ops = self._draw_operands()
        post = None
        out = None if summary else torch.empty((keep, C, n), dtype=self._dt, device=dev)
        start = torch.zeros((C, n), dtype=self._dt, device=dev)
        self._engine_start(start)
        its, ok = [], []
        try:
            for t in range(nsweeps):
                # one engine, and so one capture, per solve: the first iterations of a system loaded into an engine whose graph
                # had replayed before came out wrong on the MI355X
                if t:
                    self._engine_start(start)
                self._load(self.draw_rhs(t))
                X, coef, rows, checks = self._iterate()
                self._record(coef, rows, checks)
                its.append(self.niter.copy())
                ok.append(self.converged.copy())
                if self.breakdown.any() or not self.converged.all():
                    warnings.warn(f"{name}.run: the solve of sweep {t} did not converge for every chain (breakdown: "
                                  f"{self.breakdown.tolist()}, relative residuals {rows[-1].tolist()})")
                draw(t, X, t >= nburn)
                if t < nburn:
                    continue
                if summary is None:
                    out[t - nburn].copy_(X)
                    continue
                S = X if summary == "state" else ops.as_device(tr.inverse(X))
                if post is None:
                    from .uncertainty import PosteriorSummary

                    post = PosteriorSummary(C, S.shape[1], S.is_complex(), best=False, alpha=summary_alpha, nsamples=keep,
                                            ess_lags=summary_ess)
                post.update(S)
        finally:
            self._engine_stop()
        self.solve_iterations, self.solve_converged = np.stack(its), np.stack(ok)
        if summary:
            return post
        return out.clone() if as_torch else out.cpu().numpy()


# ---- Gaussian prior with unknown variances: the Gibbs sampler on the batched solver --------------------
class GaussianGibbs(GaussianPosterior):
    """
    The joint posterior of the field and of the prior variances: the Gibbs sampler of Wandelt, Larson & Lakshminarayanan
    (2004) and Jewell, Levin & Anderson (2004) on the solver of :class:`GaussianPosterior`.  The state is cut into K contiguous
    groups with one precision ``D_k`` each, constant inside the group,

        F(X) = 1/2 Re L2(X) + 1/2 sum_k D_k sum_{i in k} |X_i|^2,   p(v_k) ~ v_k^-q  on the variance  v_k = 1 / D_k,

    and a sweep alternates the exact draw ``x | v, d`` (perturbation-optimisation, one batched CG solve) with the conditional
    ``D_k | x = chi2_nu / sum_{i in k} |x_i|^2``, ``nu_k = dof n_k + 2 q - 2`` (``dof = 2`` for a complex state, 1 for a real
    one), drawn on the device from the Philox stream (``pxm_group_variance_draw``).  Every chain carries its own variances:
    the launches of the solver read per-chain diagonals ``[C, N]``, which the draw rewrites in place.  ``gibbs_np`` states
    the sampler in numpy.

    Takes the arguments of :class:`GaussianPosterior` (``precond`` must be ``"diag"``) and

    :param groups: ``"degree"``: one group per degree l of a :class:`SphericalHarmonicTransform` state (offsets ``l^2``),
        which samples the power spectrum ``C_l``; ``"scale"``: one per wavelet scale (``utils.wavelet_scale_bounds`` of the
        operator's transform), a Gaussian scale model; or K + 1 offsets increasing strictly from 0 to ``nparams``
    :param hyper_q: ``q`` of the hyper-prior: 0 flat, 1 Jeffreys; real with ``2 q`` an integer, at most 2
    :param fixed: indices of groups that keep their initial precision; a group with ``nu_k < 1`` cannot be sampled and must
        be listed (the monopole of degree groups at ``q = 0``)
    :param lmin: with degree groups: fixes the degrees below ``lmin`` (added to ``fixed``)
    :param precision_bounds: ``(d_lo, d_hi)``, finite and positive: the clamp of ``D_k`` (a group whose field is exactly zero
        gets ``d_hi``)

    The initial precisions are the prior's, which must be constant inside every group.  Sweep ``t`` of chain ``c`` uses the
    float64 Philox stream at ``(seed, chain_offset + c)``: iterations ``2 t`` and ``2 t + 1`` for the field draw, iteration
    ``2^61 + t`` for the variances, so ranks that share ``seed`` and number their chains through ``chain_offset`` run
    independent chains, whose summaries merge with ``PosteriorSummary.merge``.

    :meth:`run` here is the sampler, ``run(nsweeps, nburn, ...)``: it replaces the MAP solve ``run(start_point)`` of
    :class:`GaussianPosterior`, which a ``GaussianGibbs`` does not offer (``X_map`` and ``objective_map`` are not set; build a
    ``GaussianPosterior`` with ``prior.Gaussian(precision, T)`` of a sample or of the posterior mean for the Wiener map at
    fixed variances).  :meth:`sample` draws the field at the precisions as the last run left them.

    After :meth:`run`: ``precision_chain`` and ``variance_chain`` (numpy ``[nsweeps - nburn, C, K]``, in the units of
    ``prior.Gaussian``: ``Gaussian(precision_chain[t, c] repeated over the groups, T)`` is that sample's prior), ``cl_chain``
    (the variances, with degree groups), ``hyper_summary`` (a ``PosteriorSummary(C, K)`` over ``log v``: R-hat, ESS and
    quantiles of the spectrum), ``solve_iterations`` and ``solve_converged`` (``[nsweeps, C]``).  The columns of
    ``hyper_summary`` that belong to fixed groups carry no information: their ``log v`` never moves (R-hat and ESS are
    undefined there), and a fixed group whose precision is 0 has ``log v = inf``, which leaves NaN in its column.
    """

    _VAR_ITER = 1 << 61  # Philox iterations of the variance draws: off the field draws (2 t, 2 t + 1) and off _PROBE_ITER

    def __init__(self, forward, prior, mcmcparams=PxMCMCParams(), nchains=1, groups="degree", hyper_q=0.0, fixed=(), lmin=None,
                 precision_bounds=(1e-30, 1e30), tol=1e-8, max_iter=1000, check_every=10, precond="diag", use_graph=True, seed=0,
                 chain_offset=0):
        from . import gibbs_np

        if not (isinstance(precond, str) and precond == "diag"):
            raise ValueError('GaussianGibbs: precond must be "diag" (M = D + trace(A) / N follows the sampled D)')
        super().__init__(forward, prior, mcmcparams, nchains=nchains, tol=tol, max_iter=max_iter, check_every=check_every,
                         precond=precond, use_graph=use_graph, seed=seed, chain_offset=chain_offset)
        n, C = self._n, self.nchains
        self.group_kind = groups if isinstance(groups, str) else "offsets"
        bounds = self._group_offsets(forward, groups)
        fixed = list(fixed)
        if lmin is not None:
            if self.group_kind != "degree":
                raise ValueError('GaussianGibbs: lmin goes with groups="degree"')
            fixed += list(range(min(int(lmin), len(bounds) - 1)))
        self._scale = float(prior.T) / float(self.lmda)
        setup = gibbs_np.check_setup(n, 2 if self._dt.is_complex else 1, bounds, hyper_q, fixed,
                                     np.asarray(prior.precision, dtype=float) * self._scale, precision_bounds)
        self.group_bounds, self.sampled, self.nu = setup["bounds"], setup["sampled"], setup["nu"]
        self.hyper_q, self.precision_bounds = float(hyper_q), (float(precision_bounds[0]), float(precision_bounds[1]))
        self.K = self.group_bounds.size - 1
        self._groups = ops.GibbsGroups(self.group_bounds, n, np.nonzero(~self.sampled)[0])
        dev = ops.device()
        self._Dg0 = ops.as_device(np.tile(setup["D_groups"], (C, 1)), torch.float64)
        self._Dg = self._Dg0.clone()
        # the per-chain diagonals the launches of the solver read in place: the variance draw rewrites them, at these addresses
        self._D, self._sqrtD, self._minv = (torch.empty((C, n), dtype=torch.float64, device=dev) for _ in range(3))
        self._gibbs_scratch = self._groups.scratch(C)
        self._expand()

    @staticmethod
    def _group_offsets(forward, groups):
        """the ``groups`` argument -> K + 1 offsets (checked by ``gibbs_np.check_setup``)"""
        if not isinstance(groups, str):
            return groups
        from .transforms import SphericalHarmonicTransform, SphericalWaveletTransform
        from .utils import wavelet_scale_bounds

        t = getattr(forward, "transform", None)
        if groups == "degree" and isinstance(t, SphericalHarmonicTransform):
            return np.arange(int(t.L) + 1, dtype=np.int64) ** 2
        if groups == "scale" and isinstance(t, SphericalWaveletTransform):
            return wavelet_scale_bounds(t.L, t.B, t.J_min, t.dirs, t.spin, t.harmonic)
        raise ValueError('GaussianGibbs: groups="degree" needs a forward operator whose transform is a SphericalHarmonicTransform, '
                         'groups="scale" one whose transform is a SphericalWaveletTransform (other groups: a sequence of '
                         "offsets from 0 to nparams)")

    def _variance_draw(self, X, it, trace=None, row=0, expand_only=False):
        ops.group_variance_draw(X, self._groups, self._Dg, self._D, self._sqrtD, self._minv, q=self.hyper_q,
                                h=float(self.trace_estimate), d_lo=self.precision_bounds[0], d_hi=self.precision_bounds[1],
                                seed=self.seed, chain0=self.chain_offset, it=it, trace=trace, trace_row=row,
                                scratch=self._gibbs_scratch, expand_only=expand_only)

    def _expand(self):
        """``D``, ``sqrt(D)`` and ``M^-1`` of every element from the group precisions as they stand"""
        self._variance_draw(None, 0, expand_only=True)

    def _draw_operands(self):
        s, _ = super()._draw_operands()
        return s, self._sqrtD

    def run(self, nsweeps, nburn=0, summary=None, summary_ess=None, summary_alpha=None, as_torch=False):
        """``nsweeps`` sweeps of every chain from the prior's precisions; the first ``nburn`` are dropped.  Returns the field
        draws ``[nsweeps - nburn, C, N]`` (numpy, or a device tensor with ``as_torch``); with ``summary="state"`` or ``"image"``
        they are folded into a :class:`pxmcmc_amd.uncertainty.PosteriorSummary` instead, which is returned, as
        :meth:`GaussianPosterior.sample` does.  The variances of the kept sweeps fold into ``hyper_summary`` either way.  Two
        runs with the same ``seed`` and ``chain_offset`` return the same bits."""
        from .uncertainty import PosteriorSummary

        C, K = self.nchains, self.K
        made = {}

        def prepare(nsweeps, keep):
            self._Dg.copy_(self._Dg0)
            self._expand()
            made["trace"] = torch.zeros((nsweeps, C, K), dtype=torch.float64, device=ops.device())
            made["hyper"] = PosteriorSummary(C, K, False, best=False, alpha=summary_alpha, nsamples=keep, ess_lags=summary_ess)

        def draw(t, X, kept):
            self._variance_draw(X, self._VAR_ITER + t, trace=made["trace"], row=t)
            if kept:
                made["hyper"].update(-torch.log(made["trace"][t] / self._scale))  # log v, v = 1 / precision in the prior's units

        out = self._gibbs_run(nsweeps, nburn, summary, summary_ess, summary_alpha, as_torch, prepare, draw)
        self.precision_chain = made["trace"][int(nburn):].cpu().numpy() / self._scale
        with np.errstate(divide="ignore"):
            self.variance_chain = 1.0 / self.precision_chain
        if self.group_kind == "degree":
            self.cl_chain = self.variance_chain
        self.hyper_summary = made["hyper"]
        return out


# ---- L1 prior: the exact Gibbs sampler of the sparse posterior on the batched solver -------------------
class LassoGibbs(GaussianPosterior):
    """
    The posterior of the L1 prior itself -- the objective of :class:`FISTA`,

        F(X) = 1/2 Re L2(X) + (1 / lmda) sum_i T_i |X_i|,

    sampled exactly by data augmentation (Park & Casella 2008; Kyung et al. 2010) on the solver of
    :class:`GaussianPosterior`.  The Laplace prior is a Gaussian scale mixture: every coefficient carries a variance
    ``v_i`` of its own, given which the field is Gaussian with precision ``D_i = 1 / v_i``, and given the field every
    precision is an independent inverse-Gaussian variate, ``D_i | x ~ IG(t_i / |x_i|, t_i^2)`` with ``t_i = T_i / lmda``, for
    real and complex coefficients alike.  A sweep is the exact draw ``x | D, d`` (perturbation-optimisation, one batched CG
    solve) and one element-wise draw on the device (``pxm_lasso_precision_draw``): no step size, no rejection, and no bias
    -- MYULA and SKROCK sample the Moreau-Yosida envelope of this density, PxMALA samples it with a tuned step.
    ``lasso_np`` states the sampler in numpy.

    :param prior: the stock synthesis-setting L1 family (``L1``, ``S2_Wavelets_L1``, ``S2_Wavelets_L1_Power_Weights``) with a
        positive threshold ``T``, a float or one value per coefficient.  Refused: a threshold with an entry that is not
        positive (``T_i = 0`` is a flat prior, which the mixture cannot express), the analysis setting and TV (the mixture
        would be over ``A X``, whose conditional is not diagonal) and a prior with a prox of its own
    :param precision_bounds: ``(d_lo, d_hi)``, finite and positive: the clamp of every ``D_i``.  ``clamped_chain`` counts the
        elements it changed: that many conditionals per sweep were not the model's
    :param tol: a chain's solve stops at ``||r|| <= tol ||b_data||``, ``b_data = b0 + calc_gradg(data + s o omega_1)`` the part
        of the right-hand side that does not depend on ``D``: the precisions of one chain span many decades, and the
        perturbation ``sqrt(D) o omega_2`` of the coefficients near zero would otherwise set the scale of the stop rule for
        the coefficients that matter
    :param max_iter, check_every, use_graph: as for :class:`GaussianPosterior`; the preconditioner is ``M = D + trace(A) / N``
    :param seed, chain_offset: sweep ``t`` of chain ``c`` uses the float64 Philox stream at ``(seed, chain_offset + c)``:
        iterations ``2 t`` and ``2 t + 1`` for the field draw, ``2^60 + 2 t`` and ``2^60 + 2 t + 1`` for the normals and the
        uniforms of the precisions (``2^60 - 2``, ``2^60 - 1`` for the precisions drawn from a start point)

    The forward operator needs a diagonal inverse covariance (the data perturbation is formed element by element).

    :meth:`run` here is the sampler, ``run(nsweeps, nburn, start_point, ...)``, as for :class:`GaussianGibbs`.  After it:
    ``solve_iterations`` and ``solve_converged`` (``[nsweeps, C]``), ``prior_term_chain`` (``[nsweeps - nburn, C]``:
    ``(1 / lmda) sum_i T_i |X_i|`` of every kept draw, the prior term of ``F``) and ``clamped_chain`` (same shape).
    :meth:`sample` draws the field at the precisions as the last run left them.
    """

    def __init__(self, forward, prior, mcmcparams=PxMCMCParams(), nchains=1, precision_bounds=(1e-30, 1e30), tol=1e-8, max_iter=1000,
                 check_every=10, use_graph=True, seed=0, chain_offset=0):
        from . import lasso_np

        if getattr(prior, "pairs", False):
            raise ValueError("LassoGibbs: a total-variation prior is not supported: its norm couples the pair of a pixel and acts "
                             "on A X, so the conditional of the field is not the diagonal system the sampler solves")
        if getattr(prior, "setting", "synthesis") != "synthesis":
            raise ValueError("LassoGibbs: the analysis setting is not supported: the scale mixture would be over the coefficients "
                             "A X, and the prior precision A^H D A is not diagonal in the state")
        inv = getattr(forward, "invcov", None)
        if hasattr(inv, "matvec") or not hasattr(inv, "diag"):
            raise ValueError("LassoGibbs needs a diagonal inverse covariance: the data perturbation sqrt(W) omega_1 of the field "
                             "draw is formed element by element")
        Stepper.__init__(self, forward, prior, mcmcparams, nchains=nchains, seed=seed, chain_offset=chain_offset, use_graph=use_graph)
        if not self._stock_prox or getattr(prior, "T", None) is None:
            raise ValueError("LassoGibbs needs the stock synthesis-setting L1 prior (prior.L1 and its wavelet subclasses, with "
                             "their own prox): the conditionals are those of (1 / lmda) sum_i T_i |X_i|")
        self._solver_setup(tol, max_iter, check_every)
        n, C = self._n, self.nchains
        setup = lasso_np.check_setup(n, prior.T, float(self.lmda), precision_bounds)
        self.precision_bounds = setup["precision_bounds"]
        self._T, self._tscale = prior.T_dev, 1.0 / float(self.lmda)
        D0 = lasso_np.initial_precision(setup["t"], self._dt.is_complex)
        self._D = float(D0) if D0.ndim == 0 or n == 1 else ops.as_device(D0, torch.float64)
        self._solver_rhs()
        self.precond = "diag"
        self._preconditioner("diag")  # (for trace_estimate: M^-1 itself follows the sampled D)
        # the per-chain diagonals the launches of the solver read in place: the precision draw rewrites them, at these addresses
        dev = ops.device()
        self._D0 = ops.as_device(np.broadcast_to(D0, (n,)), torch.float64)
        self._D, self._sqrtD, self._minv = (torch.empty((C, n), dtype=torch.float64, device=dev) for _ in range(3))
        self._lasso_scratch = ops.lasso_scratch(C, dev)
        self._reset_precisions()

    def _reset_precisions(self):
        """``D = t^2 / (m + 1)``, the reciprocal of the prior mean of the variance, in every chain"""
        self._D.copy_(self._D0.unsqueeze(0).expand_as(self._D))
        torch.sqrt(self._D, out=self._sqrtD)
        torch.reciprocal(self._D + float(self.trace_estimate), out=self._minv)

    def _precision_draw(self, X, it, sums=None):
        ops.lasso_precision_draw(X, self._T, self._D, self._sqrtD, self._minv, tscale=self._tscale, h=float(self.trace_estimate),
                                 d_lo=self.precision_bounds[0], d_hi=self.precision_bounds[1], seed=self.seed,
                                 chain0=self.chain_offset, it=it, sums=sums, scratch=self._lasso_scratch)

    def _draw_operands(self):
        s, _ = super()._draw_operands()
        return s, self._sqrtD

    def draw_rhs(self, k):
        """as :meth:`GaussianPosterior.draw_rhs`; also notes the squared norm of the part that does not depend on ``D``, ``b0 +
        calc_gradg(data + s o omega_1)``, for the stop rule of the solve"""
        g, w2, sqrtD = self._draw_parts(k)
        data_part = ops.cg_rhs(w2, B=self._b0, G=g)
        self._data_norm2 = ops.reduce_vdot(data_part, data_part).real
        return ops.cg_rhs(w2, B=self._b0, G=g, Z=w2, S=sqrtD)

    def _reference_norm2(self, B):
        """the stop rule's ``||b||^2``: of the data part of the right-hand side (of all of it where that part vanishes)"""
        full = super()._reference_norm2(B)
        ref = getattr(self, "_data_norm2", None)
        return full if ref is None else torch.where(ref > 0, ref, full)

    def _start_state(self, start_point):
        C, n = self.nchains, self._n
        X0 = ops.as_device(start_point)
        if X0.dim() == 1:
            X0 = X0.unsqueeze(0).expand(C, -1)
        if tuple(X0.shape) != (C, n):
            raise ValueError(f"LassoGibbs.run: the start point is [N] or [C, N] with N = {n}, C = {C}")
        if X0.is_complex() and not self._dt.is_complex:
            raise ValueError("LassoGibbs.run: a complex start point needs a complex state")
        return X0.to(self._dt).contiguous()

    def run(self, nsweeps, nburn=0, start_point=None, summary=None, summary_ess=None, summary_alpha=None, as_torch=False):
        """``nsweeps`` sweeps of every chain; the first ``nburn`` are dropped.  Without a ``start_point`` the precisions start at
        ``t^2 / (m + 1)``; with one (``[N]``, or ``[C, N]`` with one row per chain -- a MAP point of :class:`FISTA`, say, whose
        exact zeros are the ``x = 0`` case of the draw) they are drawn from it.  Returns the field draws ``[nsweeps - nburn, C,
        N]`` (numpy, or a device tensor with ``as_torch``); with ``summary="state"`` or ``"image"`` they are folded into a
        :class:`pxmcmc_amd.uncertainty.PosteriorSummary` instead, which is returned.  Two runs with the same ``seed``,
        ``chain_offset`` and start return the same bits."""
        from . import lasso_np

        made = {}

        def prepare(nsweeps, keep):
            X0 = None if start_point is None else self._start_state(start_point)
            made["sums"] = torch.zeros((nsweeps, self.nchains, 2), dtype=torch.float64, device=ops.device())
            self._data_norm2 = None
            if X0 is None:
                self._reset_precisions()
            else:
                self._precision_draw(X0, lasso_np.DRAW_ITER - 2)

        def draw(t, X, kept):
            self._precision_draw(X, lasso_np.draw_iterations(t)[0], sums=made["sums"][t])

        out = self._gibbs_run(nsweeps, nburn, summary, summary_ess, summary_alpha, as_torch, prepare, draw)
        sums = made["sums"][int(nburn):].cpu().numpy()
        self.prior_term_chain, self.clamped_chain = sums[:, :, 0].copy(), sums[:, :, 1].copy()
        return out


# ---- analysis setting: primal-dual splitting and the exact prox ---------------------------------------
def operator_norm2(fwd, adj, n, dtype=torch.complex128, iters=1000, tol=1e-4, seed=0):
    """``||A||^2`` of the analysis operator ``A = adj`` (state of length ``n`` -> coefficients) with ``A^H = fwd``: the power
    iteration of :meth:`ForwardOperator.gradient_lipschitz` on ``x -> fwd(adj(x))``, with its stopping rule and its caveat --
    the estimate approaches ``||A||^2`` from below, so ``||A||^2 (1 + tol)`` is the safe value.  ``fwd is None and adj is
    None`` means ``A = I``: exactly 1.  Returns a float."""
    if fwd is None and adj is None:
        return 1.0
    if fwd is None or adj is None:
        raise ValueError("operator_norm2: fwd and adj are given together (both None: A = I)")
    AHA = lambda v: ops.as_device(fwd(ops.as_device(adj(v))), dtype)  # noqa: E731
    return power_iteration(AHA, int(n), dtype, iters, tol, seed, "operator_norm2")


def _analysis_pair(prior, dtype):
    """(A, A^H) of an analysis prior as maps between device arrays of ``dtype`` (``fwd is None and adj is None``: A = I)"""
    if prior.fwd is None and prior.adj is None:
        return (lambda x: x), (lambda v: v)
    return (lambda x: ops.as_device(prior.adj(x), dtype)), (lambda v: ops.as_device(prior.fwd(v), dtype))


def _weighted_l1(U, T):
    """``sum_i T_i |U_i|`` per chain through ``reduce_l1`` (T: python float or float64 device vector)"""
    return ops.reduce_l1(U) * T if isinstance(T, float) else ops.reduce_l1(U, T)


def _is_pairs(prior):
    return bool(getattr(prior, "pairs", False))


def _has_fused_steps(prior):
    return _is_pairs(prior) and hasattr(prior, "fused_primal_step") and hasattr(prior, "fused_dual_step")


def _weighted_pairs(U, T):
    """``sum_i T_i ||U_i||`` per chain for two-plane coefficients ``[C, 2 m]``: the third sum of ``ops.pd_dual_step_pairs``"""
    return ops.pd_dual_step_pairs(torch.zeros_like(U), U, T, 1.0, 1.0)[1][:, 2]


def analysis_prox(prior, Z, iters, sigma=None, return_dual=False, fused=True):
    """The prox of the analysis prior at ``Z``, ``argmin_p 1/2 ||p - Z||^2 + sum_i T_i |(A p)_i|`` (``A = prior.adj``,
    ``A^H = prior.fwd``, ``T = prior.T``: the prox of ``lmda f`` that the samplers' drift takes), by ``iters`` iterations of
    projected gradient on its dual from ``v = 0``::

        v <- proj_{|v_i| <= T_i}(v + sigma A (Z - A^H v)),        returns Z - A^H v

    ``sigma``: ``None`` takes ``1 / (||A||^2 (1 + tol))`` from :func:`operator_norm2` (1 for ``A = I``), found once per prior and state shape
    and kept on the prior.  The tight-frame formula of ``L1.proxf`` is one such iteration at ``sigma = 1``, exact only when
    ``A A^H = I``.  Cold-started and stateless: a pure function of ``Z`` on fixed launches (``ops.skrock_stage`` for
    ``Z - A^H v``, ``ops.pd_dual_step`` with ``rscale = 1`` for the projection), so a captured graph replays it.
    A prior with ``pairs`` is projected pair by pair (``ops.pd_dual_step_pairs``, ``T`` per pixel), and with ``fused`` the
    iteration runs on the prior's fused launches when it has them: two launches per iteration, no coefficient-sized
    temporaries, the same bits.
    Returns the point in the caller's array kind; with ``return_dual`` also the dual ``v`` (device array)."""
    z, squeeze = ops._batched(ops.as_device(Z))
    if _is_pairs(prior):
        return _analysis_prox_pairs(prior, Z, z, squeeze, iters, sigma, return_dual, fused and _has_fused_steps(prior))
    A, AH = _analysis_pair(prior, z.dtype)
    sigma = _prox_sigma(prior, z, sigma)
    T = prior.T_dev
    w = A(z)
    v, v1 = torch.zeros_like(w), torch.empty_like(w)
    p = z.clone()
    if int(iters) > 0:
        scratch = ops.pd_scratch(z.shape[0], z.device)
        sums = torch.empty((z.shape[0], 3), dtype=torch.float64, device=z.device)
        for k in range(int(iters)):
            if k:
                ops.skrock_stage(z, 1.0, e=-1.0, V=AH(v), out=p)
                w = A(p)
            ops.pd_dual_step(v, w, T, sigma, 1.0, out=v1, sums=sums, scratch=scratch)
            v, v1 = v1, v
        ops.skrock_stage(z, 1.0, e=-1.0, V=AH(v), out=p)
    out = p[0] if squeeze else p
    out = to_like(out, Z)
    return (out, v[0] if squeeze else v) if return_dual else out


def _prox_sigma(prior, z, sigma):
    """the dual step of :func:`analysis_prox`: the given one checked, or ``1 / (||A||^2 (1 + tol))``, kept on the prior"""
    if sigma is None:
        key = (z.shape[1], z.dtype)
        cache = prior.__dict__.setdefault("_prox_sigma", {})
        if key not in cache:
            tol = PrimalDual.lipschitz_tol  # (A = I: the norm is known exactly, sigma = 1 and one iteration is the prox)
            cache[key] = 1.0 if prior.fwd is None else 1.0 / (operator_norm2(prior.fwd, prior.adj, z.shape[1], z.dtype, tol=tol) * (1.0 + tol))
        sigma = cache[key]
    if not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("analysis_prox needs a positive step sigma")
    return sigma


def _analysis_prox_pairs(prior, Z, z, squeeze, iters, sigma, return_dual, fused):
    """:func:`analysis_prox` for a prior with ``pairs``: the same iteration with the pair projection; ``fused``: ``Z - A^H v``
    and ``A (.)`` are formed inside the prior's two launches"""
    sigma = _prox_sigma(prior, z, sigma)
    T = prior.T_dev
    A, AH = _analysis_pair(prior, z.dtype)
    C = z.shape[0]
    p = z.clone()
    scratch = ops.pd_scratch(C, z.device)
    sums = torch.empty((C, 3), dtype=torch.float64, device=z.device)
    if fused:
        psums = torch.empty((C, 2), dtype=torch.float64, device=z.device)
        v = torch.zeros((C, 2 * z.shape[1]), dtype=z.dtype, device=z.device)
        v1 = torch.empty_like(v)
        for k in range(int(iters)):
            if k:
                prior.fused_primal_step(z, None, v, 1.0, out=p, xbar=False, sums=psums, scratch=scratch)
            prior.fused_dual_step(v, p if k else z, T, sigma, 1.0, out=v1, sums=sums, scratch=scratch)
            v, v1 = v1, v
        if int(iters) > 0:
            prior.fused_primal_step(z, None, v, 1.0, out=p, xbar=False, sums=psums, scratch=scratch)
    else:
        w = A(z)
        v, v1 = torch.zeros_like(w), torch.empty_like(w)
        for k in range(int(iters)):
            if k:
                ops.skrock_stage(z, 1.0, e=-1.0, V=AH(v), out=p)
                w = A(p)
            ops.pd_dual_step_pairs(v, w, T, sigma, 1.0, out=v1, sums=sums, scratch=scratch)
            v, v1 = v1, v
        if int(iters) > 0:
            ops.skrock_stage(z, 1.0, e=-1.0, V=AH(v), out=p)
    out = to_like(p[0] if squeeze else p, Z)
    return (out, v[0] if squeeze else v) if return_dual else out


class PrimalDual(Stepper):
    """
    MAP point of the analysis-setting posterior of ``(forward, prior, mcmcparams)``,

        F(X) = g(X) + h(A X),   g = 1/2 Re L2,   h(u) = (1 / lmda) sum_i T_i |u_i|,   A = prior.adj,  A^H = prior.fwd,

    by the forward-backward primal-dual iteration of Condat (2013) and Vu (2013)::

        X1   = X - tau (calc_gradg(forward(X)) + A^H V)
        Xbar = 2 X1 - X
        V1   = proj_{|v_i| <= T_i / lmda}(V + sigma A Xbar)

    which needs no prox of ``h o A`` and converges for ``1 / tau - sigma ||A||^2 >= L_g / 2``.  The two elementwise updates are
    one HIP launch each (``pxm_pd_primal_step``, ``pxm_pd_dual_step``) around the four operator calls; the iteration is
    replayed from a captured HIP graph between checks.

    :param forward: an operator with ``setting == "analysis"`` (the state is the image)
    :param prior: a prior with ``fwd``, ``adj`` and ``T`` (float, or a vector of the coefficient length), such as
        ``L1("analysis", tr.inverse, tr.inverse_adjoint, T)``; ``fwd is None and adj is None``: ``A = I``
    :param tau, sigma: the steps.  ``None``: ``sigma = balance L_g / (2 ||A||^2)``, ``tau = 1 / (L_g / 2 + sigma ||A||^2)``, with
        ``L_g = gradient_lipschitz (1 + lipschitz_tol)`` and ``||A||^2 =`` :func:`operator_norm2` ``(1 + lipschitz_tol)`` (both
        power iterations approach their value from below).  One given: the other follows from the condition with equality.
        Given steps that violate the condition are refused
    :param balance: ratio of the dual term ``sigma ||A||^2`` to ``L_g / 2`` in ``1 / tau``
    :param tol: stop when ``||X1 - X|| <= tol ||X1||`` and ``||V1 - V|| <= tol ||V1||`` hold for every chain (a zero norm
        counts as met)
    :param max_iter, check_every, use_graph, nchains: as :class:`FISTA`
    :param fused: with a prior that has ``pairs`` and its own fused launches (``prior.TV_S2``): form ``A^H V`` and ``A Xbar``
        inside the two step launches (two launches per iteration beside the data term, no coefficient-sized temporaries).
        ``False`` keeps the composed route -- ``A``, ``A^H``, ``pd_primal_step``, ``pd_dual_step_pairs`` -- which gives the same
        bits.  Ignored for every other prior

    A prior with ``pairs = True`` has two-plane coefficients ``[C, 2 m]``, ``T`` a float or ``[m]``, and
    ``h(u) = (1 / lmda) sum_i T_i ||u_i||`` with the norm over a pixel's pair: the projection is ``pd_dual_step_pairs`` and the
    certificate reads ``||V_i|| <= T_i / lmda``.

    The gradient is taken on :func:`gradient_operator` ``(forward)``, as FISTA does.

    After :meth:`run`: ``objective``, ``data_term``, ``prior_term`` (``reduce_l1(A X, T) / lmda``), ``rel_change``,
    ``rel_change_dual`` and ``stationarity`` (arrays ``[nchecks, C]``; the last is ``||X1 - X|| / tau``, the norm of
    ``gradg + A^H V`` at the previous iterate), ``checks``, ``niter``, ``converged``, ``X_map``, ``V_map`` (the dual
    certificate: ``|V_i| <= T_i / lmda`` and ``gradg(X) + A^H V -> 0``), ``preds_map``, ``objective_map``, ``last_steps``
    (``[C, 2]``: ``||X_K - X_{K-1}||`` and ``||V_K - V_{K-1}||``), ``used_graph``, ``tau``, ``sigma``, ``A_norm2``, ``L_g``.
    """

    lipschitz_tol = 1e-4

    def __init__(self, forward, prior, mcmcparams=PxMCMCParams(), nchains=1, tau=None, sigma=None, balance=1.0, max_iter=10000,
                 tol=1e-4, check_every=10, use_graph=True, fused=True):
        if getattr(forward, "setting", None) != "analysis":
            raise ValueError('PrimalDual needs an analysis-setting operator (forward.setting == "analysis"); FISTA solves the '
                             "synthesis setting")
        if not all(hasattr(prior, a) for a in ("fwd", "adj", "T")) or prior.T is None:
            raise ValueError("PrimalDual needs a prior with fwd, adj and the threshold T (an L1 in the analysis setting)")
        if (prior.fwd is None) != (prior.adj is None):
            raise ValueError("PrimalDual: the prior's fwd and adj are given together (both None: A = I)")
        if getattr(prior, "setting", "analysis") != "analysis":
            raise ValueError('PrimalDual needs an analysis prior (prior.setting == "analysis")')
        super().__init__(forward, prior, mcmcparams, nchains=nchains, use_graph=use_graph)
        if int(max_iter) < 1 or int(check_every) < 1:
            raise ValueError("PrimalDual needs max_iter >= 1 and check_every >= 1")
        if not (np.isfinite(balance) and balance > 0):
            raise ValueError("PrimalDual needs a positive balance")
        self.gradient_op = gradient_operator(forward)
        dt, n = self._state_dtype(), int(forward.nparams)
        self._A, self._AH = _analysis_pair(prior, dt)
        self.ncoefs = int(self._A(torch.zeros((1, n), dtype=dt, device=ops.device())).shape[-1])
        T = prior.T_dev if hasattr(prior, "T_dev") else (float(prior.T) if np.ndim(prior.T) == 0 else
                                                          ops.as_device(np.asarray(prior.T, dtype=float), torch.float64))
        self._pair_prior = _is_pairs(prior)
        self.fused = bool(fused) and _has_fused_steps(prior)
        if self._pair_prior and self.ncoefs % 2:
            raise ValueError(f"PrimalDual: a prior with pairs has two planes of coefficients, A X has {self.ncoefs}")
        nT = self.ncoefs // 2 if self._pair_prior else self.ncoefs
        if not isinstance(T, float) and T.numel() != nT:
            raise ValueError(f"PrimalDual: T has {T.numel()} entries, the coefficients A X have {self.ncoefs}"
                             + (f" in two planes of {nT}" if self._pair_prior else ""))
        self._T = T
        tl = self.lipschitz_tol
        self.L_g = float(self.gradient_op.gradient_lipschitz(iters=1000, tol=tl) * (1.0 + tl))
        identity = prior.fwd is None
        self.A_norm2 = 1.0 if identity else float(operator_norm2(prior.fwd, prior.adj, n, dt, tol=tl) * (1.0 + tl))
        if not (self.L_g > 0 and self.A_norm2 > 0):
            raise ValueError("PrimalDual: the data term and the analysis operator must not vanish")
        half, a2 = 0.5 * self.L_g, self.A_norm2
        if tau is None:
            sigma = balance * half / a2 if sigma is None else float(sigma)
            tau = 1.0 / (half + sigma * a2) if np.isfinite(sigma) and sigma > 0 else np.nan
        elif sigma is None:
            sigma = (1.0 / tau - half) / a2 if np.isfinite(tau) and tau > 0 else np.nan
        if not (np.isfinite(tau) and tau > 0 and np.isfinite(sigma) and sigma > 0 and 1.0 / tau - sigma * a2 >= half * (1 - 1e-12)):
            raise ValueError(f"PrimalDual: the steps must be positive with 1 / tau - sigma ||A||^2 >= L_g / 2 (tau = {tau:g}, sigma = "
                             f"{sigma:g}, ||A||^2 = {a2:g}, L_g = {self.L_g:g})")
        self.tau, self.sigma, self.balance = float(tau), float(sigma), float(balance)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.check_every = int(check_every)

    def _engine_start(self, X, preds, i0):
        """static state (XA, XB, P) plus the dual in VA / VB -- V of the state in XA lives in VA, of XB in VB -- Xbar, and the
        per-chain sums of the two launches by the side they wrote"""
        self._engine_stop()
        X = ops.as_device(X).contiguous()
        f, tau, sigma, rscale, T, A, AH = self.gradient_op, self.tau, self.sigma, 1.0 / self.lmda, self._T, self._A, self._AH
        C = X.shape[0]
        VA = torch.zeros((C, self.ncoefs), dtype=X.dtype, device=X.device)
        VB, Xbar = torch.empty_like(VA), torch.empty_like(X)
        self._V = (VA, VB)
        # sums of the step that wrote XA (VA) in [0], of the step that wrote XB (VB) in [1]
        self._psums = torch.zeros((2, C, 2), dtype=torch.float64, device=X.device)
        self._dsums = torch.zeros((2, C, 3), dtype=torch.float64, device=X.device)
        scratch = ops.pd_scratch(C, X.device)

        def step(eng, src, dst):
            V, V_next = (VA, VB) if src is eng.XA else (VB, VA)
            k = 0 if dst is eng.XA else 1
            g = ops.as_device(f.calc_gradg(ops.as_device(f.forward(src))), src.dtype)
            ops.pd_primal_step(src, g, AH(V), tau, out=(dst, Xbar), sums=self._psums[k], scratch=scratch)
            ops.pd_dual_step(V, A(Xbar), T, sigma, rscale, out=V_next, sums=self._dsums[k], scratch=scratch)

        def step_pairs(eng, src, dst):
            V, V_next = (VA, VB) if src is eng.XA else (VB, VA)
            k = 0 if dst is eng.XA else 1
            g = ops.as_device(f.calc_gradg(ops.as_device(f.forward(src))), src.dtype)
            ops.pd_primal_step(src, g, AH(V), tau, out=(dst, Xbar), sums=self._psums[k], scratch=scratch)
            ops.pd_dual_step_pairs(V, A(Xbar), T, sigma, rscale, out=V_next, sums=self._dsums[k], scratch=scratch)

        def step_fused(eng, src, dst):
            V, V_next = (VA, VB) if src is eng.XA else (VB, VA)
            k = 0 if dst is eng.XA else 1
            g = ops.as_device(f.calc_gradg(ops.as_device(f.forward(src))), src.dtype)
            self.prior.fused_primal_step(src, g, V, tau, out=(dst, Xbar), sums=self._psums[k], scratch=scratch)
            self.prior.fused_dual_step(V, Xbar, T, sigma, rscale, out=V_next, sums=self._dsums[k], scratch=scratch)

        if self._pair_prior:
            step = step_fused if self.fused else step_pairs

        def reset(eng):
            VA.zero_()
            self._psums.zero_()
            self._dsums.zero_()

        return self._engine_start_generic(X, preds, i0, step, lazy=True, graph_ok=self.use_graph, reset=reset)

    def _prior_sum(self, X):
        """``sum_i T_i |(A X)_i|`` per chain (pairs: ``sum_i T_i ||(A X)_i||``)"""
        if self._pair_prior:
            return _weighted_pairs(self._A(X), self._T)
        return _weighted_l1(self._A(X), self._T)

    def run(self, start_point=None):
        """Iterate from ``start_point`` (``[N]``, or ``[C, N]`` with one row per chain; ``None``: zero) and ``V = 0`` until every
        chain meets the stopping rule or ``max_iter`` is reached.  Returns the MAP image in the caller's array kind (numpy,
        or a device tensor for a tensor start point): ``[N]`` for one chain, ``[C, N]`` for a batch."""
        C = self.nchains
        as_torch = isinstance(start_point, torch.Tensor)
        if start_point is None:
            start_point = np.zeros(self.forward.nparams)
        X, preds = self._initial_sample(start_point)
        self._engine_start(X, preds, 0)
        keys = ("objective", "data_term", "prior_term", "rel_change", "rel_change_dual", "stationarity")
        traces = {k: [] for k in keys}
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
                ps, ds = self._psums[last].cpu().numpy(), self._dsums[last].cpu().numpy()
                with np.errstate(invalid="ignore", divide="ignore"):
                    rel_x = np.where(ps[:, 0] == 0.0, 0.0, np.sqrt(ps[:, 0]) / np.sqrt(ps[:, 1]))
                    rel_v = np.where(ds[:, 0] == 0.0, 0.0, np.sqrt(ds[:, 0]) / np.sqrt(ds[:, 1]))
                data_term = 0.5 * self._l2_dev(preds).real.cpu().numpy()
                prior_term = self._prior_sum(X).cpu().numpy() / self.lmda
                now = (rel_x <= self.tol) & (rel_v <= self.tol)
                niter = np.where(now & met, niter, i)  # iterations done when the chain first met (and kept) the rule
                met = now
                self.checks.append(i)
                for key, v in zip(keys, (data_term + prior_term, data_term, prior_term, rel_x, rel_v, np.sqrt(ps[:, 0]) / self.tau)):
                    traces[key].append(np.array(v, dtype=float))
                if met.all():
                    break
            self.X_map, self.preds_map, self.V_map = X.clone(), preds.clone(), self._V[last].clone()
            self.last_steps = np.sqrt(np.stack([ps[:, 0], ds[:, 0]], axis=1))
            self.used_graph = self._eng.graph is not None
            self.graph_error = self._eng.graph_error
        finally:
            self._engine_stop()
            self._V = None
        for key, rows in traces.items():
            setattr(self, key, np.stack(rows))
        self.niter, self.converged = niter, met
        self.objective_map = self.objective[-1]
        out = self.X_map if C > 1 else self.X_map[0]
        return out.clone() if as_torch else out.cpu().numpy()
