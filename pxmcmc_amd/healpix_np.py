"""
The HEALPix ring synthesis and its adjoint in numpy (RING order): the statement of ``ops.HpxPlan`` the tests hold the
kernels to, and the operators of ``rng="numpy"`` debugging.

    synthesis          v_p  = sum_lm sY_lm(theta_p, phi_p) f_lm
    synthesis_adjoint  f_lm = sum_p conj(sY_lm(theta_p, phi_p)) v_p              (no quadrature weight)

with sY_lm = lam_lm(theta) exp(i m phi), lam_lm = (-1)^s sqrt((2l+1)/4pi) d^l_{m,-s} from
``oracle.wigner.wigner_d_recursion``.  Both are separable: a sum over l per ring and order, then a sum over the orders per
pixel of the ring.  ``dtype=np.float64`` rounds the table and does every sum in double precision;
``dtype=np.longdouble`` keeps 64-bit mantissas throughout (the model the GPU tests measure against).
"""
import numpy as np

from .utils import healpix_rings


class HealpixModel:
    def __init__(self, L, nside, spin=0, dtype=np.float64):
        from oracle.wigner import wigner_d_recursion

        self.L, self.nside, self.spin = int(L), int(nside), int(spin)
        if self.L < 1 or abs(self.spin) >= self.L or self.nside < 1:
            raise ValueError("HealpixModel: need L >= 1, |spin| < L and nside >= 1")
        self.real = np.dtype(dtype).type
        self.cplx = np.result_type(self.real, np.complex64).type if self.real is not np.longdouble else np.clongdouble
        self.nphi, theta, phi0, self.start = healpix_rings(self.nside, np.longdouble)
        self.npix, self.nlm = 12 * self.nside ** 2, self.L ** 2
        el = np.arange(self.L).astype(np.longdouble)
        pi = np.longdouble("3.141592653589793238462643383279502884")
        d = wigner_d_recursion(self.L, -self.spin, theta, dtype=np.longdouble)  # [m + L - 1, ring, l]
        self.lam = ((-1.0) ** self.spin * np.sqrt((2 * el + 1) / (4 * pi)) * d).astype(self.real)
        m = np.arange(-(self.L - 1), self.L).astype(np.longdouble)
        self._m, self._phi0, self._pi, self._phases = m, phi0, pi, {}
        # index of (l, m) in the coefficient vector, per order; -1 where l < |m|
        ls = np.arange(self.L)
        ms = np.arange(-(self.L - 1), self.L)
        self.idx = np.where(ls[None, :] >= np.abs(ms)[:, None], ls[None, :] ** 2 + ls[None, :] + ms[:, None], -1)

    def phase(self, r):
        """E[j, m + L - 1] = exp(i m phi_j) on ring r (made on demand and shared by the rings of one length and shift)"""
        n = int(self.nphi[r])
        key = (n, bool(self._phi0[r] != 0))  # rings of one length and shift share their azimuths
        if key not in self._phases:
            self._phases[key] = self._phase(r, n)
        return self._phases[key]

    def _phase(self, r, n):
        a = np.outer(self._phi0[r] + 2 * self._pi * np.arange(n) / np.longdouble(n), self._m)
        return (np.cos(a) + 1j * np.sin(a)).astype(self.cplx)

    def _flm_by_order(self, flm):
        """F[m + L - 1, l] = f_lm (0 where l < |m|)"""
        f = np.asarray(flm).astype(self.cplx)
        return np.where(self.idx >= 0, f[np.maximum(self.idx, 0)], 0)

    def ring_orders(self, flm):
        """G[r, m + L - 1] = sum_l lam_lm(theta_r) f_lm"""
        return np.einsum("mrl,ml->rm", self.lam, self._flm_by_order(flm))

    def synthesis(self, flm):
        G = self.ring_orders(flm)
        return np.concatenate([self.phase(r) @ G[r] for r in range(len(self.nphi))])

    def synthesis_adjoint(self, v):
        v = np.asarray(v).astype(self.cplx)
        Gt = np.stack([self.phase(r).conj().T @ v[s:s + n] for r, (s, n) in enumerate(zip(self.start, self.nphi))])
        F = np.einsum("mrl,rm->ml", self.lam, Gt)
        out = np.zeros(self.nlm, dtype=self.cplx)
        out[self.idx[self.idx >= 0]] = F[self.idx >= 0]
        return out

    # ---- the scales the error bounds of the tests are stated in ----
    def synthesis_scale(self, flm):
        """S_p = sum_lm |lam_lm(theta_r)| |f_lm| for every pixel p of ring r"""
        a = np.abs(self._flm_by_order(flm)).astype(np.float64)
        S = np.einsum("mrl,ml->r", np.abs(self.lam).astype(np.float64), a)
        return np.repeat(S, self.nphi)

    def adjoint_scale(self, v):
        """S_lm = sum_p |lam_lm(theta_r(p))| |v_p|"""
        a = np.abs(np.asarray(v)).astype(np.float64)
        ring = np.array([a[s:s + n].sum() for s, n in zip(self.start, self.nphi)])
        F = np.einsum("mrl,r->ml", np.abs(self.lam).astype(np.float64), ring)
        out = np.zeros(self.nlm)
        out[self.idx[self.idx >= 0]] = F[self.idx >= 0]
        return out


class HealpixSamplingNp:
    """``measurements.HealpixSampling`` in numpy, for the oracle's loops (``oracle.pxmcmc_np``) and ``rng="numpy"``
    debugging: the MW transforms are ``oracle.ssht``'s, the ring synthesis is :class:`HealpixModel` in float64."""

    def __init__(self, L, nside, spin=0, kernel=None, mask=None, harmonic=False, weights=None):
        self.L, self.nside, self.spin, self.harmonic = int(L), int(nside), int(spin), bool(harmonic)
        self.model = HealpixModel(L, nside, spin)
        npix = self.model.npix
        self.mask = np.ones(npix, dtype=bool) if mask is None else np.asarray(mask).astype(bool).reshape(-1)
        self.ndata = int(self.mask.sum())
        self.npix = self.L ** 2 if self.harmonic else self.L * (2 * self.L - 1)
        self.weights = np.ones(self.ndata) if weights is None else np.asarray(weights, dtype=float)
        self.kernel_lm = None if kernel is None else np.repeat(np.asarray(kernel, dtype=float), 2 * np.arange(self.L) + 1)

    def _k(self, flm):
        return flm if self.kernel_lm is None else flm * self.kernel_lm

    def forward(self, x):
        from oracle import ssht

        flm = np.asarray(x, dtype=complex) if self.harmonic else ssht.forward(np.asarray(x).reshape(self.L, 2 * self.L - 1), self.L, 0)
        return self.model.synthesis(self._k(flm))[self.mask] * self.weights

    def adjoint(self, y):
        from oracle import ssht

        full = np.zeros(self.model.npix, dtype=complex)
        full[self.mask] = np.asarray(y) * self.weights
        flm = self._k(self.model.synthesis_adjoint(full))
        return flm if self.harmonic else ssht.forward_adjoint(flm, self.L, 0).flatten()


class WeakLensingHealpixNp(HealpixSamplingNp):
    """``measurements.WeakLensingHealpix`` in numpy"""

    def __init__(self, L, nside, mask=None, ngal=None, harmonic=False):
        el = np.arange(int(L), dtype=float)
        k = np.zeros(int(L))
        k[2:] = -np.sqrt(((el[2:] + 2.0) * (el[2:] - 1.0)) / ((el[2:] + 1.0) * el[2:]))
        npix = 12 * int(nside) ** 2
        m = np.ones(npix, dtype=bool) if mask is None else np.asarray(mask).astype(bool).reshape(-1)
        w = None if ngal is None else np.sqrt(2.0 * np.asarray(ngal, dtype=float).reshape(-1)[m] / 0.37 ** 2)
        super().__init__(L, nside, spin=2, kernel=k, mask=m, harmonic=harmonic, weights=w)
        self.inv_cov = self.weights
