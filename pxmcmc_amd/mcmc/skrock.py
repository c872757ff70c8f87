"""SKROCK (pxmcmc/mcmc.py:292-383) on the published recursion coefficients."""
import numpy as np
import torch

from .. import ops
from .base import PxMCMC
from .params import PxMCMCParams


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
        captured graphs of 2 and 2 * GRAPH_PAIRS iterations.  preds (P) is formed on demand only."""
        self._engine_stop()
        X = ops.as_device(X).contiguous()
        Y, KA, KB = (torch.empty_like(X) for _ in range(3))
        numpy_rng = self.rng == "numpy"

        def step(eng, src, dst):
            if self._own_step:  # a subclass's chain_step: eager, through it
                dst.copy_(ops.as_device(self.chain_step(src), dst.dtype))
            else:
                noise = self._host_noise(src) if numpy_rng else None
                self._iterate(src, dst, Y, KA, KB, noise, 0, eng.cnt.t)
                eng.cnt.add(1)

        graph_ok = not numpy_rng and self.use_graph and not self._own_step
        return self._engine_start_generic(X, preds, i0, step, lazy=True, graph_ok=graph_ok)

    def run(self, start_point=None):
        """Run the algorithm (pxmcmc/mcmc.py:308-336): the reference's schedule and tracking arrays; iterations between
        two observable events (save / progress print) are advanced together, from a captured HIP graph with the device
        Philox stream."""
        self._it = 0
        X_curr, curr_preds = self._initial_sample(start_point)
        return self._run_engine(X_curr, curr_preds)
