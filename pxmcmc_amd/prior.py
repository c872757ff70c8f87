"""
Prior plugin API of the reference (pxmcmc/prior.py:8-149) on the GPU: L1 norm and its
soft-thresholding prox, with MW quadrature weighting (and optional wavelet-power weighting) on the sphere.
"""
import numpy as np
import torch

from . import ops
from .transforms import SphericalGradientTransform
from .utils import _multires_bandlimits, mw_map_weights, mw_size, sample_positions, to_like, wavelet_tiling


class L1:
    """
    Base L1-norm prior; the prox is soft thresholding (pxmcmc/prior.py:8-53).

    :param string setting: 'analysis' or 'synthesis'
    :param fwd: transform handle (e.g. ``Transform.forward``), used in the analysis setting
    :param adj: adjoint transform handle, used in the analysis setting
    :param T: soft threshold, float or vector
    """

    def __init__(self, setting, fwd, adj, T):
        assert setting in ["analysis", "synthesis"]
        self.setting = setting
        self.fwd = fwd
        self.adj = adj
        self.T = T
        self._T_dev = None

    @property
    def T_dev(self):
        """threshold as the kernels take it: python float, or float64 GPU vector"""
        if isinstance(self.T, (int, float)):
            return float(self.T)
        if self._T_dev is None or self._T_dev[0] is not self.T:
            self._T_dev = (self.T, ops.as_device(np.asarray(self.T, dtype=float), torch.float64))
        return self._T_dev[1]

    _weights_dev = None

    def prior(self, X):
        """sum |X| per chain (pxmcmc/prior.py:28-35); float for one chain, float64 tensor [C] for a batch."""
        r = ops.reduce_l1(X, self._weights_dev)
        if (isinstance(X, torch.Tensor) and X.dim() == 2) or (not isinstance(X, torch.Tensor) and np.ndim(X) == 2):
            return r
        return float(r[0])

    def proxf(self, X):
        """pxmcmc/prior.py:37-53."""
        if self.setting == "synthesis":
            return self._proxf_synthesis(X)
        return self._proxf_analysis(X)

    def _proxf_synthesis(self, X):
        return to_like(ops.soft(X, self.T_dev), X)

    def _proxf_analysis(self, X):
        x = ops.as_device(X)
        a = ops.as_device(self.adj(x))
        return to_like(x + ops.as_device(self.fwd(ops.soft(a, self.T_dev) - a)), X)


def _is_stock_l1(prior):
    """True when prior.proxf is the library's own synthesis soft threshold (safe to fuse)."""
    return isinstance(prior, L1) and type(prior).proxf is L1.proxf and type(prior)._proxf_synthesis is L1._proxf_synthesis and prior.setting == "synthesis"


class L1_Analysis(L1):
    """
    Analysis-setting L1 prior ``sum_i T_i |(A X)_i|`` (``A = adj``, ``A^H = fwd``) with its exact prox (extension; DESIGN.md
    section 14d).  ``L1("analysis", ...)`` applies the tight-frame formula ``X + A^H (soft(A X) - A X)`` of the reference
    (pxmcmc/prior.py:52-53), which is the prox only when ``A A^H = I``; this class runs ``prox_iters`` iterations of
    projected gradient on the prox's dual (:func:`pxmcmc_amd.optim.analysis_prox`): fixed launches and no host read, so the
    samplers replay it from their captured graph.

    :param fwd: ``A^H``, coefficients -> state (e.g. ``Transform.inverse``)
    :param adj: ``A``, state -> coefficients (e.g. ``Transform.inverse_adjoint``)
    :param T: threshold, float or vector of the coefficient length
    :param prox_iters: dual iterations per prox
    """

    def __init__(self, fwd, adj, T, prox_iters=16):
        super().__init__("analysis", fwd, adj, T)
        if int(prox_iters) < 1:
            raise ValueError("L1_Analysis needs prox_iters >= 1")
        self.prox_iters = int(prox_iters)

    def prior(self, X):
        """sum_i T_i |(A X)_i| per chain; float for one chain, float64 tensor [C] for a batch (as ``L1.prior``)."""
        x = ops.as_device(X)
        u = x if self.adj is None else ops.as_device(self.adj(x))
        T = self.T_dev
        r = ops.reduce_l1(u) * T if isinstance(T, float) else ops.reduce_l1(u, T)
        return r if x.dim() == 2 else float(r[0])

    def proxf(self, X):
        from .optim import analysis_prox  # (optim imports the samplers, which import this module)

        return analysis_prox(self, X, self.prox_iters)


class TV_S2(L1_Analysis):
    """
    Isotropic total variation on the MW grid (extension)::

        TV(X) = sum_{t,p} T_{t,p} sqrt(|(A X)[0][t][p]|^2 + |(A X)[1][t][p]|^2)   ~   T int |grad X| dOmega

    with ``A`` the discrete gradient of :class:`pxmcmc_amd.transforms.SphericalGradientTransform` (the quadrature weight is
    folded into ``A``).  An analysis prior: ``adj = A``, ``fwd = A^H``, and ``pairs = True`` -- the norm of ``h`` and the
    projection of its dual act on the two gradient components of a pixel together.  ``proxf`` is the exact prox by
    ``prox_iters`` dual iterations (:func:`pxmcmc_amd.optim.analysis_prox`) on the fused launches ``ops.tv_primal_step`` /
    ``ops.tv_dual_step``; ``prior`` is ``ops.tv_value``.  No plan and no tables beyond ``2 L`` ring coefficients.

    :param int L: bandlimit of the image, ``[L (2L - 1)]`` samples, real or complex
    :param T: threshold, float or one value per pixel ``[L (2L - 1)]``
    :param prox_iters: dual iterations per prox
    """

    pairs = True

    def __init__(self, L, T, prox_iters=16):
        self.transform = SphericalGradientTransform(L)
        self.L = self.transform.L
        if np.ndim(T) != 0:
            T = np.asarray(T, dtype=float).reshape(-1)
            if T.size != self.transform.npix:
                raise ValueError(f"TV_S2: T is a float or one value per pixel ({self.transform.npix}), got {T.size}")
        super().__init__(self.transform.forward_adjoint, self.transform.forward, T, prox_iters=prox_iters)

    def prior(self, X):
        """TV(X) per chain; float for one chain, float64 tensor [C] for a batch (as ``L1.prior``)."""
        x = ops.as_device(X)
        r = ops.tv_value(x, self.transform.ab, self.T_dev)
        return r if x.dim() == 2 else float(r[0])

    # the fused launches of the primal-dual iteration and of the prox's dual iteration (optim.PrimalDual, optim.analysis_prox)
    def fused_primal_step(self, X, G, V, tau, **kw):
        return ops.tv_primal_step(X, G, V, self.transform.ab, tau, **kw)

    def fused_dual_step(self, V, Xbar, T, sigma, rscale, **kw):
        return ops.tv_dual_step(V, Xbar, self.transform.ab, T, sigma, rscale, **kw)


class S2_Wavelets_L1(L1):
    """
    L1 regulariser for wavelets on S2 with MW quadrature weighting (pxmcmc/prior.py:56-84).

    ``dirs = N > 1`` (extension): every orientation plane of scale j carries that scale's ``mw_map_weights(bl_j)``, so
    ``len(map_weights) == ncoefs`` of the directional layout.  The reference builds one grid of weights per scale
    whatever N is, a vector of the wrong length for N > 1.
    """

    def __init__(self, setting, fwd, adj, T, L, B, J_min, dirs=1, spin=0):
        super().__init__(setting, fwd, adj, T)
        self.L = L
        self.B = B
        self.J_min = J_min
        self.J_max = ops.j_max(L, B)
        self.nscales = self.J_max - J_min + 1
        self.dirs = dirs
        self.spin = spin
        if setting == "synthesis":
            bls = _multires_bandlimits(L, B, J_min, dirs, spin)
            planes = [1] + [2 * int(dirs) - 1] * (len(bls) - 1)
            self.map_weights = np.concatenate([np.tile(mw_map_weights(int(el)), k) for el, k in zip(bls, planes)])
        else:
            raise NotImplementedError
        self.T = self.T * self.map_weights
        self._weights_dev = ops.as_device(self.map_weights, torch.float64)


class S2_Wavelets_L1_Power_Weights(S2_Wavelets_L1):
    """
    L1 regulariser for wavelets on S2 with pixel-area, wavelet-power and wavelet-decay weighting
    (pxmcmc/prior.py:87-149; eqns 33 & 34 of Wallis et al 2017).

    As in the reference the threshold ends up weighted by the quadrature weights AND the power weights
    (prior.py:81,108), and ``prior`` applies the power weights twice (prior.py:110-111 through :83-84).

    :param float eta: wavelet decay tuning parameter
    """

    def __init__(self, setting, fwd, adj, T, L, B, J_min, dirs=1, spin=0, eta=1):
        if dirs != 1:
            # the reference reads the power and peak of psi_{l0}, identically zero for even N
            raise NotImplementedError("S2_Wavelets_L1_Power_Weights: directional wavelets (dirs > 1) are not supported")
        super().__init__(setting, fwd, adj, T, L, B, J_min, dirs, spin)
        self.eta = eta
        if setting != "synthesis":
            raise NotImplementedError
        self.map_weights = self._power_weight_map()
        self.T = self.T * self.map_weights
        self._weights_dev = ops.as_device(self.map_weights * self.map_weights, torch.float64)

    def _power_weight_map(self):
        """One weight per coefficient, block by block [scaling | j = J_min .. J_max]: every sample of a block
        carries 2 pi^2 peak^eta / (power * nsamples) * sin(theta) with the block's own grid (pxmcmc/prior.py:113-149).
        Rows of the table below: (grid bandlimit, harmonic power of the kernel, peak degree ** eta)."""
        phi_l, psi_lm = wavelet_tiling(self.B, self.L, self.dirs, self.J_min, self.spin)
        el = np.arange(self.L)
        table = [(int(np.nonzero(phi_l)[0].max()) + 1, np.vdot(phi_l, phi_l).real, 1.0)]  # scaling: no peak factor
        for bl, psi in zip(_multires_bandlimits(self.L, self.B, self.J_min)[1:], psi_lm.T):
            table.append((int(bl), np.vdot(psi, psi).real, float(np.argmax(psi[el * el + el])) ** self.eta))
        blocks = []
        for bl, power, peak in table:
            thetas, _ = sample_positions(bl)
            ring = (2 * np.pi ** 2) * peak / (power * mw_size(bl)) * np.sin(thetas)
            blocks.append(np.repeat(ring, 2 * bl - 1))
        return np.concatenate(blocks)


class Gaussian:
    """
    Gaussian prior on the state (extension): ``prior(X) = 1/2 sum_i p_i |X_i|^2`` per chain, whose prox
    is the shrinkage ``proxf(X) = X / (1 + T p)``.  With the Gaussian likelihood of a ``ForwardOperator`` the posterior is
    Gaussian: :class:`pxmcmc_amd.optim.GaussianPosterior` gives its mean (the Wiener filter) and exact draws.  Following the
    convention of :class:`pxmcmc_amd.optim.FISTA` the posterior is ``F(X) = 1/2 Re L2(X) + (T / lmda) 1/2 sum_i p_i |X_i|^2``.
    MYULA, PxMALA and SKROCK take it through ``proxf`` like any user prior.

    :param precision: ``p``, a non-negative float or one non-negative value per parameter
    :param T: the product ``lmda * mu`` that :class:`L1` also takes
    """

    setting = "synthesis"
    fwd = adj = None

    def __init__(self, precision, T):
        p = np.asarray(precision, dtype=float)
        if p.ndim > 1 or not np.all(np.isfinite(p)) or np.any(p < 0):
            raise ValueError("Gaussian: the precision is a non-negative finite float or vector [nparams]")
        if not (np.isfinite(T) and T >= 0):
            raise ValueError("Gaussian: T must be finite and not negative")
        self.precision = float(p) if p.ndim == 0 else p.copy()
        self.T = float(T)
        self._dev = {}

    @classmethod
    def from_power_spectrum(cls, cl, L, T):
        """``p = 1 / C_l`` repeated over the ``2 l + 1`` orders of degree l in ssht index order (``l^2 + l + m``), for a state
        of harmonic coefficients ``f_lm [L^2]``; ``cl`` holds at least ``L`` values, all positive"""
        cl = np.asarray(cl, dtype=float).reshape(-1)
        if cl.size < int(L):
            raise ValueError(f"Gaussian.from_power_spectrum: cl holds {cl.size} values, bandlimit {L} needs {int(L)}")
        cl = cl[:int(L)]
        if not np.all(np.isfinite(cl)) or np.any(cl <= 0):
            bad = int(np.flatnonzero(~(np.isfinite(cl) & (cl > 0)))[0])
            raise ValueError(f"Gaussian.from_power_spectrum: C_l must be positive and finite (C_{bad} = {cl[bad]:g}): a degree "
                             "without power has no finite precision; give it a small positive C_l to pin it to zero")
        return cls(np.repeat(1.0 / cl, 2 * np.arange(int(L)) + 1), T)

    @property
    def precision_dev(self):
        """the precision as the kernels take it: python float, or float64 GPU vector"""
        if isinstance(self.precision, float):
            return self.precision
        if "p" not in self._dev:
            self._dev["p"] = ops.as_device(self.precision, torch.float64)
        return self._dev["p"]

    def _value_operands(self, x):
        """(zeros, precision vector) of the state's length, the operands of the one reduction of :meth:`prior`"""
        key = (x.shape[-1], x.dtype)
        if key not in self._dev:
            p = self.precision_dev
            pv = torch.full((key[0],), p, dtype=torch.float64, device=x.device) if isinstance(p, float) else p
            if pv.numel() != key[0]:
                raise ValueError(f"Gaussian: the precision has {pv.numel()} entries, the state {key[0]}")
            self._dev[key] = (torch.zeros(key[0], dtype=x.dtype, device=x.device), pv)
        return self._dev[key]

    def prior(self, X):
        """``1/2 sum_i p_i |X_i|^2`` per chain; float for one chain, float64 tensor [C] for a batch (as ``L1.prior``)"""
        x = ops.as_device(X)
        zeros, pv = self._value_operands(x)
        r = ops.reduce_l2(x, zeros, pv).real * 0.5
        return r if x.dim() == 2 else float(r[0])

    def proxf(self, X):
        """``X / (1 + T p)``, one launch"""
        return to_like(ops.gauss_prox(X, self.precision_dev, self.T), X)
