"""
Transform plugin API of the reference (pxmcmc/transforms.py:8-166) on the GPU.

``SphericalWaveletTransform`` replaces the four pys2let calls (transforms.py:95-98) with the
HIP wavelet plan.  Arrays are 1-D ``[n]`` (the reference's shape) or ``[C, n]`` chain batches;
numpy in -> numpy out, torch in -> torch (GPU) out.
"""
from . import ops
from .utils import to_like


class Transform:
    """Base class to wrap transformations (pxmcmc/transforms.py:8-33)."""

    def forward(self):
        raise NotImplementedError

    def inverse(self):
        raise NotImplementedError

    def forward_adjoint(self):
        raise NotImplementedError

    def inverse_adjoint(self):
        raise NotImplementedError


class IdentityTransform(Transform):
    """Identity transform (pxmcmc/transforms.py:36-56)."""

    def __init__(self):
        pass

    def forward(self, X):
        return X

    def forward_adjoint(self, X):
        return X

    def inverse(self, X):
        return X

    def inverse_adjoint(self, X):
        return X


class SphericalWaveletTransform(Transform):
    """
    Spherical wavelet transforms (pxmcmc/transforms.py:59-166), ``upsample=0``.  ``dirs = N > 1``: directional wavelets;
    each wavelet block holds 2N - 1 orientation planes.  ``spin != 0`` (``dirs = 1`` only): images
    are spin-s MW maps, the coefficients keep the spin-0 layout.  ``harmonic=True``: inputs and
    outputs are spherical-harmonic coefficients, f_lm [L^2] and one ssht-indexed bl_j^2 block per (scale, n)
    (pys2let's analysis_lm2lmn / synthesis_lmn2lm and their adjoints).

    :param int max_chains: largest chain batch the transform will be called with (extension)
    """

    def __init__(self, L, B, J_min, dirs=1, spin=0, harmonic=False, max_chains=1):
        if int(dirs) != dirs or dirs < 1:
            raise ValueError("dirs must be a positive integer")
        if int(spin) != spin:
            raise ValueError("spin must be an integer")
        if spin != 0 and dirs != 1:
            raise NotImplementedError("spin wavelets are axisymmetric only (dirs = 1; DESIGN.md sections 12, 13)")
        if abs(spin) >= L:
            raise ValueError("|spin| must be < L")
        spin = int(spin)
        self.L = L
        self.B = B
        self.J_min = J_min
        self.J_max = ops.j_max(L, B)
        self.nscales = self.J_max - self.J_min + 1
        self.dirs = dirs
        self.spin = spin
        self.harmonic = bool(harmonic)
        self.params = {"B": B, "L": L, "J_min": J_min, "N": dirs, "spin": spin, "upsample": 0}
        self.max_chains = max_chains
        self._plan = self._make_plan(max_chains)
        self._get_ncoefs()

    def _make_plan(self, C):
        """harmonic: the harmonic-space plan; dirs = 1: the axisymmetric plan with the fused sampler steps; dirs > 1: the
        directional plan (SO(3) stages)"""
        if self.harmonic:
            return ops.HarmWavPlan(self.L, self.B, self.J_min, int(self.dirs), spin=self.spin, max_chains=C)
        if self.dirs == 1:
            return ops.WavPlan(self.L, self.B, self.J_min, max_chains=C, spin=self.spin)
        return ops.DirWavPlan(self.L, self.B, self.J_min, int(self.dirs), max_chains=C)

    def ensure_chains(self, C):
        """Grow the plan's chain capacity (workspace is allocated at plan creation)."""
        if C > self.max_chains:
            self.max_chains = C
            self._plan = self._make_plan(C)

    def forward(self, X):
        """image (or f_lm) -> wavelet coefficients (pys2let.analysis_px2wav / analysis_lm2lmn, transforms.py:101-112)."""
        return to_like(self._plan.analysis(X), X)

    def inverse(self, X):
        """wavelet coefficients -> image (pys2let.synthesis_wav2px, transforms.py:114-127)."""
        return to_like(self._plan.synthesis(X), X)

    def inverse_adjoint(self, X):
        """image -> wavelet coefficients (pys2let.synthesis_adjoint_px2wav, transforms.py:129-139)."""
        return to_like(self._plan.synthesis_adjoint(X), X)

    def forward_adjoint(self, X):
        """wavelet coefficients -> image (pys2let.analysis_adjoint_wav2px, transforms.py:141-154)."""
        return to_like(self._plan.analysis_adjoint(X), X)

    def _get_ncoefs(self):
        """transforms.py:156-166 counts by running an analysis; the plan knows the sizes."""
        self.nscal = self._plan.nscal
        self.nwav = self._plan.ncoefs - self._plan.nscal
        self.ncoefs = self._plan.ncoefs


class SphericalGradientTransform(Transform):
    """
    The discrete gradient on the MW grid of bandlimit ``L`` (extension): ``forward`` is
    ``A: [L n] -> [2 L n]`` (``n = 2L - 1``; plane 0 the weighted differences along theta, plane 1 those along phi, the
    quadrature weight folded in), ``forward_adjoint`` is ``A^H``.  ``A`` annihilates constants, so there is no inverse.
    With ``prior.L1_Analysis(tr.forward_adjoint, tr.forward, T)`` it gives anisotropic total variation;
    :class:`pxmcmc_amd.prior.TV_S2` is the isotropic form.  No plan and no tables beyond ``2 L`` ring coefficients.
    """

    def __init__(self, L):
        self.L = int(L)
        self.ab = ops.tv_ring_coefs(self.L)
        self.npix = self.L * (2 * self.L - 1)
        self.ncoefs = 2 * self.npix

    def forward(self, X):
        return to_like(ops.tv_grad(X, self.ab), X)

    def forward_adjoint(self, X):
        return to_like(ops.tv_grad_adjoint(X, self.ab), X)

    def inverse(self, X):
        raise NotImplementedError("SphericalGradientTransform has no inverse: the gradient annihilates constants")

    def inverse_adjoint(self, X):
        raise NotImplementedError("SphericalGradientTransform has no inverse: the gradient annihilates constants")


class SphericalHarmonicTransform(Transform):
    """
    The MW spherical-harmonic transform as a :class:`Transform` whose state is ``f_lm [L^2]`` in ssht index order
    (extension): ``inverse`` is the synthesis ``f_lm -> f [L (2L - 1)]``, ``forward`` the analysis, and
    the two adjoints are those of :class:`pxmcmc_amd.ops.ShtPlan`.  With ``measurements.WeakLensing``, ``Identity``,
    ``HealpixSampling`` or ``WeakLensingHealpix`` and ``prior.Gaussian.from_power_spectrum`` it is the classic Wiener setting:
    harmonic state, ``1 / C_l`` prior, masks and noise diagonal in data space.

    :param int max_chains: largest chain batch the transform will be called with
    """

    def __init__(self, L, spin=0, max_chains=1):
        if int(L) != L or L < 1:
            raise ValueError("L must be a positive integer")
        if int(spin) != spin or abs(spin) >= L:
            raise ValueError("spin must be an integer with |spin| < L")
        self.L, self.spin, self.max_chains = int(L), int(spin), int(max_chains)
        self.ncoefs = self.L * self.L
        self.npix = self.L * (2 * self.L - 1)
        self._plan = ops.ShtPlan(self.L, self.spin, max_chains=self.max_chains)

    def ensure_chains(self, C):
        """Grow the plan's chain capacity (workspace is allocated at plan creation)."""
        if C > self.max_chains:
            self.max_chains = int(C)
            self._plan = ops.ShtPlan(self.L, self.spin, max_chains=self.max_chains)

    def forward(self, X):
        """image -> f_lm"""
        return to_like(self._plan.forward(X), X)

    def inverse(self, X):
        """f_lm -> image"""
        return to_like(self._plan.inverse(X), X)

    def inverse_adjoint(self, X):
        """image -> f_lm, the adjoint of :meth:`inverse`"""
        return to_like(self._plan.inverse_adjoint(X), X)

    def forward_adjoint(self, X):
        """f_lm -> image, the adjoint of :meth:`forward`"""
        return to_like(self._plan.forward_adjoint(X), X)
