"""
Uncertainty summaries of saved chains (pxmcmc/uncertainty.py:7-56): quantile credible-interval ranges per
parameter and per wavelet scale, and the highest-posterior-density threshold.  Post-run host arithmetic,
as in the reference; ``chain_to_images`` is the batched GPU synthesis the reference's plot scripts do sample
by sample (experiments/earthtopography/plot.py:105-115).
"""
import numpy as np
import torch

from .. import ops
from ..utils import _multires_bandlimits, mw_size


def credible_interval_range(chain, alpha=0.05):
    """range of the (1 - alpha) credible interval of every parameter (pxmcmc/uncertainty.py:7-16).  A chain that is already
    resident on the device (a CUDA tensor, float64 [nsamples, nparams]) is reduced there (`pxm_quantile_range`: exact order
    statistics + numpy's interpolation, the same numbers) and a device tensor comes back; numpy in, numpy out on the host as
    in the reference."""
    if isinstance(chain, torch.Tensor) and chain.is_cuda:
        return ops.quantile_range(chain, alpha)
    quantiles = np.quantile(chain, (alpha / 2, 1 - alpha / 2), axis=0)
    return np.diff(quantiles, axis=0)[0]


def wavelet_credible_interval_range(chain, L, B, J_min, alpha=0.05, dirs=1):
    """credible-interval maps per wavelet scale, MW (theta, phi) format (pxmcmc/uncertainty.py:19-40): the quantile
    range of every coefficient at once, cut at the block boundaries of the coefficient vector.  ``dirs = N > 1``
    (extension): wavelet block j comes back as (2N - 1, bl_j, 2 bl_j - 1), one map per orientation."""
    bls = [int(bl) for bl in _multires_bandlimits(L, B, J_min)]
    planes = [1] + [2 * int(dirs) - 1] * (len(bls) - 1)
    edges = np.cumsum([k * mw_size(bl) for bl, k in zip(bls, planes)])
    on_device = isinstance(chain, torch.Tensor) and chain.is_cuda
    chain = chain if on_device else np.asarray(chain)
    if chain.shape[1] != edges[-1]:
        raise ValueError("chain has %d parameters, the wavelet layout %d" % (chain.shape[1], edges[-1]))
    ci = credible_interval_range(chain, alpha)
    blocks = np.split(ci.cpu().numpy() if on_device else ci, edges[:-1])
    if dirs == 1:
        return [blk.reshape(bl, 2 * bl - 1) for blk, bl in zip(blocks, bls)]
    return [blk.reshape(bl, 2 * bl - 1) if k == 1 else blk.reshape(k, bl, 2 * bl - 1) for blk, bl, k in zip(blocks, bls, planes)]


def credible_region_threshold(logpis, alpha=0.05):
    """log-posterior threshold of the credible set (pxmcmc/uncertainty.py:43-51)"""
    return np.quantile(logpis, 1 - alpha)


def approx_credible_region_threshold(objective_map, ndim, alpha=0.05):
    """Approximate threshold of the (1 - alpha) highest-posterior-density region of a log-concave posterior from its MAP
    point alone, without a chain (Pereyra, "Maximum-a-posteriori estimation with Bayesian confidence regions", SIAM J.
    Imaging Sci. 10(1), 2017, theorem 3.1): the region ``{x : F(x) <= F(x_map) + ndim (tau_alpha + 1)}`` with
    ``tau_alpha = sqrt(16 log(3 / alpha) / ndim)`` contains the HPD region, for ``alpha`` in ``(4 exp(-ndim / 3), 1)``.

    :param objective_map: the objective ``F = -log posterior`` at the MAP point (:attr:`pxmcmc_amd.optim.FISTA.objective_map`)
    :param ndim: number of REAL dimensions of the state (``2 n`` for a complex state of n coefficients)
    :raises ValueError: ``alpha`` outside the range of the bound
    """
    ndim = int(ndim)
    if ndim < 1:
        raise ValueError("ndim must be a positive number of real dimensions")
    if not (4 * np.exp(-ndim / 3) < alpha < 1):
        raise ValueError("alpha = %g is outside (4 exp(-ndim / 3), 1) = (%g, 1), the range of the bound" % (alpha, 4 * np.exp(-ndim / 3)))
    tau = np.sqrt(16 * np.log(3 / alpha) / ndim)
    return objective_map + ndim * (tau + 1)


def in_credible_region(logpi, threshold):
    """pxmcmc/uncertainty.py:54-56"""
    return True if logpi <= threshold else False


def chain_to_images(chain, transform, batch=16):
    """map every saved sample through ``transform.inverse`` in chain batches on the GPU -> [nsamples, npix]"""
    chain = np.asarray(chain)
    transform.ensure_chains(batch)
    out = []
    for i in range(0, chain.shape[0], batch):
        out.append(np.asarray(transform.inverse(chain[i : i + batch].astype(complex))))
    return np.concatenate(out, axis=0)
