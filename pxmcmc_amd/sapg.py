"""
Estimating the regularisation strength from the data: SAPG, the stochastic-approximation proximal-gradient scheme of Vidal,
De Bortoli, Pereyra & Durmus (SIAM J. Imaging Sci. 13(4), 2020), on the samplers' posterior with its prior scaled by theta

    pi_theta(X) ~ exp(-1/2 Re L2(X) - theta G(X)),   G(X) = (1 / lmda) sum_i T_i |X_i|,   T = prior.T = lmda mu w.

G is 1-homogeneous, so the normaliser of ``exp(-theta G)`` is proportional to ``theta^-d`` and the gradient of the marginal
log-likelihood is ``d / theta - E[G | data, theta]``.  A MYULA chain whose soft threshold is ``theta T`` supplies the
expectation one sample at a time, and theta follows the projected stochastic gradient in ``eta = log theta``::

    X_{k+1}   = MYULA step of X_k on pi_{theta_k}
    eta_{k+1} = clip(eta_k + rho_k (d - theta_k G(X_{k+1})), log theta_min, log theta_max),   theta_{k+1} = exp(eta_{k+1})

One iteration is one fused HIP launch pair (``pxm_sapg_step``: the step with theta read on the device and the per-chain sum,
then the move of theta) around the two operator calls, replayed from a captured HIP graph by the samplers' stepping engine
(DESIGN.md section 17).  The estimate is ``mu_hat = mu theta_hat``: what ``--mu`` should have been.

With ``groups`` the prior is ``sum_k theta_k G_k(X)``, ``G_k`` the sum over the k-th contiguous block of the state (a wavelet
scale).  Every ``G_k`` is 1-homogeneous on its own ``d_k`` dimensions, the normaliser factorises into ``prod_k theta_k^-d_k``,
and the same chain moves K numbers per chain by ``d_k - theta_k G_k`` (the multivariate case of the paper;
``pxm_sapg_step_groups``).
"""
import copy

import numpy as np
import torch

from . import ops
from .mcmc import PxMCMCParams, Stepper


def sapg_rho_table(warmup, niter, ndim, scale=10.0, exponent=0.8):
    """the step sizes ``rho_k``: zeros for the ``warmup`` iterations (a plain MYULA warm-up at theta_0), then
    ``scale * j ** -exponent / ndim`` for j = 1 ... niter"""
    warmup, niter = int(warmup), int(niter)
    if warmup < 0 or niter < 1 or not ndim > 0:
        raise ValueError("sapg_rho_table needs warmup >= 0, niter >= 1 and ndim > 0")
    j = np.arange(1, niter + 1, dtype=float)
    return np.concatenate([np.zeros(warmup), scale * j ** (-exponent) / ndim])


class SAPG(Stepper):
    """
    Marginal maximum-likelihood estimate of the scale theta of the prior of ``(forward, prior, mcmcparams)`` -- the
    arguments of the samplers -- so that ``mu_hat = mcmcparams.mu * theta_hat`` is the regularisation strength the data ask
    for.

    :param nchains: C independent chains, each with its own theta (``pool``: one theta driven by the chain mean of G)
    :param theta0: start value, a float or one per chain
    :param theta_min, theta_max: the interval theta is projected onto
    :param warmup: MYULA iterations at theta_0 before theta moves
    :param niter: iterations with a moving theta
    :param burn: of those, the ones left out of the average ``theta_hat``
    :param scale, exponent: ``rho_j = scale * j ** -exponent / ndim`` (:func:`sapg_rho_table`)
    :param ndim: dimension d of the state; ``None``: ``forward.nparams``, twice that with ``mcmcparams.complex``
    :param use_graph: replay from a captured HIP graph (``False``: the same launches one by one, same results)
    :param groups: ``None``: one theta for the whole state.  ``"scale"``: one per block ``[scaling | j = J_min ... J_max]`` of
        ``forward.transform``, a ``SphericalWaveletTransform`` (``utils.wavelet_scale_bounds``).  A sequence of K + 1
        offsets increasing from 0 to ``forward.nparams``: one per block ``[b_k, b_k+1)``.  With groups ``d_k`` is the
        block's own dimension (``ndim`` is not used), ``rho[:, k] = sapg_rho_table(warmup, niter, d_k, scale, exponent)``
        -- normalised by the block's dimension, not the state's -- and ``theta0`` is a float, ``[K]`` or ``[C, K]``.

    The prior must be the stock synthesis L1 (its threshold is what the kernel scales) and ``delta`` a float.  The fused
    ``WavPlan`` / ``HarmWavPlan`` steps bake one threshold per plan and are not used: the iteration runs on the operators'
    own ``forward`` / ``calc_gradg``.

    After :meth:`run`: ``theta_trace``, ``eta_trace``, ``g_trace`` (``[warmup + niter, C]``; row k holds theta_{k+1},
    eta_{k+1} and G(X_{k+1})), ``theta_hat`` (float for one chain or ``pool``, else ``[C]``), ``mu_hat``, ``X_curr``,
    ``used_graph`` and ``graph_error``.  With groups the traces are ``[warmup + niter, C, K]``, ``theta_hat`` is ``[K]`` for
    one chain or ``pool``, else ``[C, K]``, and ``group_bounds`` holds the K + 1 offsets.
    """

    def __init__(self, forward, prior, mcmcparams=PxMCMCParams(), nchains=1, theta0=1.0, theta_min=1e-3, theta_max=1e3,
                 warmup=200, niter=1500, burn=500, scale=10.0, exponent=0.8, ndim=None, pool=False, seed=0, chain_offset=0,
                 noise_bits=64, use_graph=True, groups=None):
        super().__init__(forward, prior, mcmcparams, nchains=nchains, seed=seed, chain_offset=chain_offset, use_graph=use_graph,
                         noise_bits=noise_bits)
        if not self._stock_prox:
            raise ValueError("SAPG needs the stock synthesis L1 prior: the step kernel scales its threshold T by theta (an "
                             "analysis-setting or user prox has no threshold to scale)")
        if not isinstance(self.delta, float):
            raise ValueError("SAPG needs a float delta (no per-chain step sizes)")
        self.warmup, self.niter, self.burn = int(warmup), int(niter), int(burn)
        if self.warmup < 0 or self.niter < 1 or not 0 <= self.burn < self.niter:
            raise ValueError("SAPG needs warmup >= 0, niter >= 1 and 0 <= burn < niter")
        if not (0 < theta_min <= theta_max and np.isfinite(theta_max)):
            raise ValueError("SAPG needs 0 < theta_min <= theta_max")
        self.theta_min, self.theta_max = float(theta_min), float(theta_max)
        self.group_bounds = self._group_bounds(forward, groups)
        if self.group_bounds is None:
            theta0 = np.broadcast_to(np.asarray(theta0, dtype=float), (self.nchains,)).copy()
        else:
            theta0 = self._group_theta0(theta0, self.nchains, len(self.group_bounds) - 1)
        if not np.all((theta0 >= self.theta_min) & (theta0 <= self.theta_max)):
            raise ValueError("SAPG: theta0 must lie in [theta_min, theta_max]")
        self.theta0 = theta0
        self.pool = bool(pool)
        if self.group_bounds is None:
            self.ndim = float(ndim if ndim is not None else forward.nparams * (2 if self.complex else 1))
            self.rho = sapg_rho_table(self.warmup, self.niter, self.ndim, scale, exponent)
        else:  # every group by its own dimension: its gradient d_k - theta_k G_k has that size
            self.ndim = np.diff(self.group_bounds).astype(float) * (2 if self.complex else 1)
            self.rho = np.stack([sapg_rho_table(self.warmup, self.niter, dk, scale, exponent) for dk in self.ndim], axis=1)

    @staticmethod
    def _group_bounds(forward, groups):
        """the ``groups`` argument -> None, or the K + 1 offsets as an int64 array"""
        if groups is None:
            return None
        n = int(forward.nparams)
        if isinstance(groups, str):
            from .transforms import SphericalWaveletTransform
            from .utils import wavelet_scale_bounds

            t = getattr(forward, "transform", None)
            if groups != "scale" or not isinstance(t, SphericalWaveletTransform):
                raise ValueError('SAPG: groups="scale" needs a forward operator whose transform is a SphericalWaveletTransform '
                                 "(other groups: a sequence of offsets from 0 to nparams)")
            groups = wavelet_scale_bounds(t.L, t.B, t.J_min, t.dirs, t.spin, t.harmonic)
        return ops.sapg_group_bounds(groups, n, name="SAPG: groups")

    @staticmethod
    def _group_theta0(theta0, C, K):
        """float, [K] or [C, K] -> [C, K]; a vector of C entries is per group when K == C, so per-chain values are [C, 1]"""
        t = np.asarray(theta0, dtype=float)
        if t.ndim == 1 and C == K > 1 and t.size == C:
            raise ValueError(f"SAPG: theta0 of {C} entries is ambiguous with {C} chains and {K} groups: pass [C, 1] for one "
                             "value per chain or [1, K] for one per group")
        if t.ndim > 2 or (t.ndim == 1 and t.size not in (1, K)) or (t.ndim == 2 and (t.shape[0] not in (1, C) or t.shape[1] not in (1, K))):
            raise ValueError("SAPG: with groups theta0 must be a float, [K] or [C, K]")
        return np.broadcast_to(t, (C, K)).copy()

    def _engine_start(self, X, preds, i0):
        """static state (XA, XB, P) plus theta, eta, the trace and the step-size table on the device; both kernels read the
        iteration number from the engine's device counter"""
        self._engine_stop()
        X = ops.as_device(X).contiguous()
        dev, C = X.device, X.shape[0]
        f, T, delta, lmda = self.forward, self.prior.T_dev, float(self.delta), self.lmda
        eta0 = torch.log(ops.as_device(self.theta0, torch.float64))
        self._eta = eta0.clone()
        self._theta = torch.exp(eta0)
        grouped = self.group_bounds is not None
        self._trace = torch.zeros((len(self.rho), *eta0.shape, 3), dtype=torch.float64, device=dev)
        rho = ops.as_device(self.rho, torch.float64)
        scratch = ops.sapg_groups_scratch(C, eta0.shape[1], dev) if grouped else ops.sapg_scratch(C, dev)
        ndim = ops.as_device(self.ndim, torch.float64) if grouped else self.ndim
        kw = dict(pool=self.pool, trace=self._trace, noise_complex=bool(self.complex), seed=self.seed, chain0=self.chain_offset,
                  it=0, scratch=scratch, noise64=self.noise64)
        lo, hi = float(np.log(self.theta_min)), float(np.log(self.theta_max))

        def step(eng, src, dst):
            gradg = ops.as_device(f.calc_gradg(eng.P), src.dtype)
            if grouped:
                ops.sapg_step_groups(src, gradg, T, delta, lmda, self._theta, self._eta, self.group_bounds, ndim, rho, lo, hi,
                                     iter_dev=eng.cnt.t, out=dst, **kw)
            else:
                ops.sapg_step(src, gradg, T, delta, lmda, self._theta, self._eta, ndim, rho, lo, hi, iter_dev=eng.cnt.t,
                              out=dst, **kw)
            eng.P.copy_(ops.as_device(f.forward(dst)))
            eng.cnt.add(1)

        def reset(eng):  # the capture warm-up moved them
            self._eta.copy_(eta0)
            self._theta.copy_(torch.exp(eta0))
            self._trace.zero_()

        return self._engine_start_generic(X, preds, i0, step, lazy=False, graph_ok=self.use_graph, reset=reset)

    def run(self, start_point=None):
        """``warmup + niter`` iterations from ``start_point`` (``[N]``, or ``[C, N]`` with one row per chain; ``None``: the
        samplers' Laplace draw).  Returns ``theta_hat``: the mean of theta over the iterations after ``warmup + burn``, a
        float for one chain or ``pool``, else ``[C]`` (with groups: ``[K]``, else ``[C, K]``)."""
        X, preds = self._initial_sample(start_point)
        self._engine_start(X, preds, 0)
        try:
            self._engine_advance(len(self.rho))
            X, preds = self._engine_state()
            self._check_device_status()
            trace = self._trace.cpu().numpy()
            self.X_curr, self.curr_preds = X.clone(), preds.clone()
            self.used_graph = self._eng.graph is not None
            self.graph_error = self._eng.graph_error
        finally:
            self._engine_stop()
            self._theta = self._eta = self._trace = None
        self.theta_trace, self.eta_trace, self.g_trace = (np.ascontiguousarray(trace[..., k]) for k in range(3))
        if not np.isfinite(trace).all():
            raise FloatingPointError("SAPG: the chain left the finite range (delta too large for theta_max?)")
        hat = self.theta_trace[self.warmup + self.burn:].mean(axis=0)
        if self.group_bounds is not None:
            self.theta_hat = hat[0].copy() if (self.nchains == 1 or self.pool) else hat
        else:
            self.theta_hat = float(hat[0]) if (self.nchains == 1 or self.pool) else hat
        self.mu_hat = self.mu * self.theta_hat
        return self.theta_hat

    def apply(self, prior, params):
        """copies of ``(prior, params)`` with the threshold ``T`` and ``mu`` scaled by ``theta_hat`` (its chain mean), ready
        for MYULA / PxMALA / SKROCK / FISTA; the inputs are not modified.

        With groups one scalar cannot carry K factors: ``T_i`` and the prior's weights are scaled by ``s_k(i)``, the chain
        mean of ``theta_hat`` of element i's group (``T`` becomes a vector), and ``mu`` stays, so that ``logPi = -mu
        prior(X) - L2`` keeps matching the threshold ``T' = lmda mu w'``."""
        if self.group_bounds is not None:
            return self._apply_groups(prior, params)
        s = float(np.mean(self.theta_hat))
        new_prior, new_params = copy.copy(prior), copy.copy(params)
        new_prior.T = prior.T * s
        if hasattr(new_prior, "_T_dev"):
            new_prior._T_dev = None
        new_params.mu = params.mu * s
        return new_prior, new_params

    def _apply_groups(self, prior, params):
        s = np.asarray(self.theta_hat, dtype=float).reshape(-1, len(self.group_bounds) - 1).mean(axis=0)
        per_element = np.repeat(s, np.diff(self.group_bounds))
        new_prior, new_params = copy.copy(prior), copy.copy(params)
        new_prior.T = np.asarray(prior.T, dtype=float) * per_element
        new_prior._T_dev = None
        if getattr(prior, "map_weights", None) is not None:
            new_prior.map_weights = np.asarray(prior.map_weights) * per_element
        w = prior._weights_dev
        wnew = per_element if w is None else w.cpu().numpy() * per_element
        new_prior._weights_dev = ops.as_device(wnew, torch.float64)
        return new_prior, new_params
