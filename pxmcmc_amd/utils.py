"""
Host-side helpers mirroring the hot-path subset of pxmcmc/utils.py.

``soft`` runs on the GPU; layout helpers and the MW quadrature weights are setup-time
numpy, as in the reference.
"""
import numpy as np
import torch

from . import ops


def to_like(result, like):
    """Return ``result`` (a GPU tensor) as numpy when the caller passed numpy, else as is."""
    if isinstance(like, torch.Tensor):
        return result
    return result.cpu().numpy()


def flatten_mlm(wav_lm, scal_lm):
    """pxmcmc/utils.py:11-22: scaling coefficients first, wavelets flattened column-major."""
    if isinstance(wav_lm, torch.Tensor):
        buff = wav_lm.T.reshape(-1) if wav_lm.dim() > 1 else wav_lm
        return torch.cat((scal_lm, buff))
    buff = np.ravel(wav_lm, order="F")
    return np.concatenate((scal_lm, buff))


def expand_mlm(mlm, nscales=None, nscalcoefs=None, flatten_wavs=False):
    """pxmcmc/utils.py:25-52: (wavelets, scaling) of a flat vector -- either ``nscales`` + 1 blocks of equal length
    (wavelets as the columns of a complex [len, nscales] array, or concatenated) or a split after ``nscalcoefs``."""
    if (nscales is None) == (nscalcoefs is None):
        raise ValueError("Set either 'nscales', or 'nscalcoefs'" if nscales is None
                         else "Give only one of 'nscales' or 'nscalcoefs'")
    if nscalcoefs is not None:
        return mlm[..., nscalcoefs:], mlm[..., :nscalcoefs]
    mlm = np.asarray(mlm)
    per_block = mlm.size // (nscales + 1)
    assert per_block > 0
    blocks = mlm[: (nscales + 1) * per_block].reshape(nscales + 1, per_block)
    wavs = blocks[1:].astype(complex)
    return (wavs.reshape(-1) if flatten_wavs else np.ascontiguousarray(wavs.T)), blocks[0]


def soft(X, T=0.1):
    """pxmcmc/utils.py:55-67: soft thresholding (HIP kernel pxm_soft)."""
    return to_like(ops.soft(X, T), X)


def _multires_bandlimits(L, B, J_min, dirs=1, spin=0):
    """pxmcmc/utils.py:116-125: highest non-zero el + 1 of the scaling function and every wavelet."""
    k0, k = ops.tiling_axisym(L, B, J_min)
    rows = [k0] + [k[j] for j in range(J_min, k.shape[0])]
    return np.array([int(np.nonzero(r)[0].max()) + 1 for r in rows], dtype=int)


def wavelet_scale_bounds(L, B, J_min, dirs=1, spin=0, harmonic=False):
    """[ext] the offsets of the blocks ``[scaling | j = J_min ... J_max]`` in the coefficient vector of
    ``SphericalWaveletTransform(L, B, J_min, dirs, spin, harmonic)``: K + 1 integers from 0 to ``ncoefs``.  A block of
    bandlimit bl_j holds ``mw_size(bl_j)`` samples per plane in pixel space and ``bl_j ** 2`` harmonic coefficients per plane
    with ``harmonic``; the scaling block is one plane, a wavelet scale ``2 * dirs - 1`` orientation planes in pixel space (the
    rule of ``S2_Wavelets_L1.map_weights``) and ``dirs`` blocks, one per n, in harmonic space; a spin
    keeps the spin-0 layout.  The groups of ``SAPG(groups="scale")``."""
    bls = _multires_bandlimits(L, B, J_min, dirs, spin)
    planes = [1] + [int(dirs) if harmonic else 2 * int(dirs) - 1] * (len(bls) - 1)
    sizes = [(int(bl) ** 2 if harmonic else mw_size(int(bl))) * k for bl, k in zip(bls, planes)]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def dir_component(L, N):
    """[ext] the directionality component s_lm [L*L] of s2let's directional wavelets:
    ``nu sqrt(2^-g C(g, (g - m)/2))`` for m = -g, -g + 2, .., g with g = gamma_l the largest integer <= min(N - 1, l) of
    the parity of N - 1, 0 elsewhere; nu = 1 for odd N, i for even N.  N = 1: s_l0 = 1."""
    from math import comb

    s = np.zeros(L * L, dtype=complex)
    nu = 1.0 if N % 2 else 1j
    for el in range(L):
        g = min(N - 1, el)
        if (N - 1 - g) % 2:
            g -= 1
        if g < 0:
            continue
        for m in range(-g, g + 1, 2):
            s[el * el + el + m] = nu * np.sqrt(2.0 ** -g * comb(g, (g - m) // 2))
    return s


def wavelet_tiling(B, L, N=1, J_min=0, spin=0):
    """[ext] pys2let.wavelet_tiling (pxmcmc/utils.py:117, prior.py:121,132):
    ``phi_l[L] = sqrt((2l+1)/4pi) kappa0(l)`` and ``psi_lm[L*L, nscales]`` with
    ``psi_lm = sqrt((2l+1)/8pi^2) kappa_j(l) s_lm``, one column per scale j = J_min..J_max; s_lm is the directionality
    component (:func:`dir_component`, s_l0 = 1 for N = 1).  The harmonic normalisation is parity-unpinned (DESIGN.md
    section 2); only supports, ``sum |.|^2`` and peak degrees are consumed by the callers.  ``spin = s != 0`` (N = 1
    only): the spin-0 tiling with every degree l < |s| zeroed."""
    if spin != 0 and N != 1:
        raise NotImplementedError("spin wavelets are axisymmetric only (N = 1)")
    k0, k = ops.tiling_axisym(L, B, J_min)
    el = np.arange(L)
    phi_l = np.sqrt((2 * el + 1) / (4 * np.pi)) * k0
    psi_lm = np.zeros((L * L, k.shape[0] - J_min), dtype=complex)
    if N == 1:
        for col, j in enumerate(range(J_min, k.shape[0])):
            psi_lm[el * el + el, col] = np.sqrt((2 * el + 1) / (8 * np.pi ** 2)) * k[j]
        if spin != 0:
            phi_l[: abs(spin)] = 0.0
            psi_lm[: abs(spin) ** 2] = 0.0
        return phi_l, psi_lm
    s = dir_component(L, N)
    ell = np.repeat(el, 2 * el + 1)
    for col, j in enumerate(range(J_min, k.shape[0])):
        psi_lm[:, col] = (np.sqrt((2 * el + 1) / (8 * np.pi ** 2)) * k[j])[ell] * s
    return phi_l, psi_lm


def sample_positions(L):
    """[ext] pyssht.sample_positions for MW sampling: theta_t = pi (2t+1)/(2L-1), phi_p = 2 pi p/(2L-1)."""
    return np.pi * (2 * np.arange(L) + 1) / (2 * L - 1), 2 * np.pi * np.arange(2 * L - 1) / (2 * L - 1)


def mw_weights(m):
    """pxmcmc/utils.py:249-259: w(m) = int_0^pi exp(i m theta) sin(theta) dtheta = (1 + (-1)^m) / (1 - m^2), and
    +-i pi/2 at the removable points m = +-1."""
    m = int(m)
    if abs(m) == 1:
        return 0.5j * np.pi * m
    return (1.0 + (-1.0) ** m) / (1.0 - m * m)


def weights_theta(L):
    """pxmcmc/utils.py:262-267: quadrature weights on the 2L-1 rings of the theta-extended MW grid.  The reference's
    FFT of w(m) exp(-i m pi/(2L-1)) is the cosine series below at theta_t = pi (2t+1)/(2L-1), written out (the m = +-1
    pair gives pi sin(theta), the odd rest vanishes)."""
    n = 2 * L - 1
    theta = np.pi * (2 * np.arange(n) + 1) / n
    even = np.arange(2, L, 2)
    series = np.pi * np.sin(theta) + 2.0 + (np.cos(np.outer(theta, even)) @ (4.0 / (1.0 - even * even)) if even.size else 0.0)
    return series * (2 * np.pi / n ** 2)


def mw_map_weights(L):
    """pxmcmc/utils.py:270-283: exact MW quadrature weights, shape (L(2L-1),) -- the ring weights of the library
    (`pxm_mw_ring_weights`: mirror rings of the extended grid folded onto the L sampled ones), constant along phi."""
    return np.repeat(ops.mw_ring_weights(int(L)), 2 * int(L) - 1)


def s2_integrate(f, L):
    """pxmcmc/utils.py:286-301."""
    f = f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
    return (mw_map_weights(L) * f).sum()


def mw_size(L):
    """[ext] pys2let.mw_size (pxmcmc/forward.py:1,109)."""
    return L * (2 * L - 1)


# J2000 north galactic pole and the ICRS -> Galactic rotation astropy applies (its Galactic frame is defined
# through FK5 J2000; the ICRS / FK5 frame bias of ~20 mas is far below any pixel of a mask)
_NGP_RA, _NGP_DEC = np.radians(192.8594812065348), np.radians(27.12825118085622)


def galactic_latitude(lon_deg, lat_deg):
    """galactic latitude b (degrees) of ICRS (lon, lat) in degrees"""
    ra, dec = np.radians(lon_deg), np.radians(lat_deg)
    sinb = np.sin(dec) * np.sin(_NGP_DEC) + np.cos(dec) * np.cos(_NGP_DEC) * np.cos(ra - _NGP_RA)
    return np.degrees(np.arcsin(np.clip(sinb, -1.0, 1.0)))


def build_mask(L, size=20):
    """
    Mask for the galactic plane and the equatorial band, MW format, 0 at masked positions
    (pxmcmc/utils.py:320-349).  The reference builds the coordinates as lon = phi - 180, lat = theta - 90 degrees
    (:337-339) and masks |galactic latitude| < size through astropy; the same rotation is applied here directly
    (parity unpinned against astropy, which is absent from this image).
    """
    thetas, phis = sample_positions(L)
    mask = np.ones((L, 2 * L - 1))
    mask[np.abs(90 - np.degrees(thetas)) < size, :] = 0
    thetaarray, phiarray = np.meshgrid(np.degrees(thetas) - 90, np.degrees(phis) - 180, indexing="ij")
    mask[np.abs(galactic_latitude(phiarray, thetaarray)) < size] = 0
    return mask


def healpix_rings(nside, dtype=np.float64):
    """[ext] the rings of a HEALPix map in RING order (what healpy.ringinfo reports): ``(nphi, theta, phi0, start)``, one
    entry per ring i = 1 .. 4 nside - 1, north to south -- pixels on the ring, colatitude of the ring, azimuth of its first
    pixel, index of its first pixel.  With i' = min(i, 4 nside - i): polar caps (i' < nside) nphi = 4 i',
    z = 1 - i'^2 / (3 nside^2), phi0 = pi / (4 i'); belt nphi = 4 nside, z = 4/3 - 2 i' / (3 nside), phi0 = pi / (4 nside) for
    even i' - nside and 0 for odd; the southern rings have -z.  Evaluated in long double and returned as ``dtype``.  NESTED
    order and reading FITS files are out of scope: reorder a NESTED map to RING order before it comes here."""
    nside = int(nside)
    if nside < 1:
        raise ValueError("healpix_rings: need nside >= 1")
    ld = np.longdouble
    i = np.arange(1, 4 * nside)
    ip = np.minimum(i, 4 * nside - i)
    cap = ip < nside
    nphi = np.where(cap, 4 * ip, 4 * nside).astype(np.int64)
    ipl, ns = ip.astype(ld), ld(nside)
    z = np.where(cap, 1 - ipl * ipl / (3 * ns * ns), ld(4) / 3 - 2 * ipl / (3 * ns))
    z = np.where(i > 2 * nside, -z, z)
    shifted = cap | ((ip - nside) % 2 == 0)
    pi = ld("3.141592653589793238462643383279502884")
    phi0 = np.where(shifted, pi / nphi.astype(ld), ld(0))
    start = np.concatenate([[0], np.cumsum(nphi)[:-1]]).astype(np.int64)
    return nphi, np.arccos(z).astype(dtype), phi0.astype(dtype), start


def healpix_pixel_centres(nside, dtype=np.float64):
    """[ext] ``(theta, phi)`` of the 12 nside^2 pixel centres in RING order (healpy.pix2ang of every pixel): ring by ring
    north to south, phi ascending on a ring (:func:`healpix_rings`).  NESTED order and FITS files are out of scope."""
    nphi, theta, phi0, _ = healpix_rings(nside, np.longdouble)
    pi = np.longdouble("3.141592653589793238462643383279502884")
    phi = np.concatenate([p0 + 2 * pi * np.arange(n) / np.longdouble(n) for n, p0 in zip(nphi, phi0)])
    return np.repeat(theta, nphi).astype(dtype), phi.astype(dtype)
