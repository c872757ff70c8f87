"""
What the region-wise tools from the MAP point share (DESIGN.md sections 14b, 14c): the scope they are defined in
(:func:`_check_scope`), the objective and its level (:func:`map_objective`, :func:`_level`), the MAP image and the label
contract (:func:`_regions_setup`, :func:`superpixel_regions`), the search of ``{xi : F(a + xi b) <= gamma}`` per region with
its one read-back (:class:`_PathSearch`) and the result painted back onto the pixels (:class:`_RegionResult`).
:mod:`~pxmcmc_amd.uncertainty.lci` and :mod:`~pxmcmc_amd.uncertainty.hyp` differ in the path ``(a, b)`` they search along.
"""
import numpy as np
import torch

from .. import ops
from ..prior import _is_stock_l1
from .chains import approx_credible_region_threshold


def _check_scope(fn, forward, *prior):
    """the scope of the tool ``fn``: synthesis setting and a pixel-space transform; given the prior (the tool forms the
    objective F) also the stock L1 prior and a diagonal inverse covariance"""
    objective = bool(prior)
    if getattr(forward, "setting", None) != "synthesis":
        raise ValueError("%s is defined in the synthesis setting (X_map holds coefficients: the surrogate lives in coefficient space)" % fn)
    if objective and not _is_stock_l1(prior[0]):
        raise ValueError("%s needs the stock synthesis L1 prior: the objective is formed from prior.T" % fn)
    tr = getattr(forward, "transform", None)
    if tr is None or not hasattr(tr, "forward") or not hasattr(tr, "inverse"):
        raise ValueError("%s needs forward.transform with forward and inverse" % fn)
    if getattr(tr, "harmonic", False):
        raise ValueError("%s needs a pixel-space transform: with harmonic=True there is no image to cut into regions" % fn)
    if objective and hasattr(forward.invcov, "matvec"):
        raise ValueError("%s needs a diagonal inverse covariance; a full covariance matrix is not supported" % fn)


def superpixel_regions(L, size):
    """int32 labels [L, 2L - 1] of the MW grid cut into superpixels of ``size`` rings x ``size`` phi-samples, numbered row
    by row; the last block of a row of blocks, and the last row of blocks, are smaller when ``size`` does not divide"""
    L, size = int(L), int(size)
    if L < 1 or size < 1:
        raise ValueError("superpixel_regions needs L >= 1 and size >= 1")
    t, p = np.arange(L) // size, np.arange(2 * L - 1) // size
    return (t[:, None] * (p[-1] + 1) + p[None, :]).astype(np.int32)


def _lci_weights(forward):
    """w: the real diagonal inverse covariance of ``optim.gradient_operator(forward)``, float64 [ndata] on the device"""
    from ..optim import gradient_operator

    diag = gradient_operator(forward).invcov.diag
    return (diag.real if diag.is_complex() else diag).to(torch.float64).contiguous()


def _lci_preds(forward, X):
    """forward.forward of a [C, N] batch with the data in the dtype of the residual -> (preds [C, ndata], data [ndata])"""
    p = ops.as_device(forward.forward(X))
    dt = forward._resid_dtype(p) if hasattr(forward, "_resid_dtype") else p.dtype
    return p.to(dt).contiguous(), forward.data_dev.to(dt).contiguous()


def map_objective(forward, prior, params, X):
    """``F(X) = 1/2 sum w |forward(X) - data|^2 + (1 / lmda) sum T |X|`` per chain -> float64 [C] on the device (``[1]`` for a
    1-D ``X``), from the reductions the samplers use.  Defined through ``prior.T`` as :mod:`pxmcmc_amd.optim` explains, with
    ``w = Re(invcov)``: the objective FISTA minimises, so at ``FISTA.X_map`` it equals ``FISTA.objective_map`` up to the
    rounding of the prior sum.  Synthesis setting, stock L1 prior, diagonal inverse covariance."""
    _check_scope("map_objective", forward, prior)
    x, _ = ops._batched(ops.as_device(X))
    p, d = _lci_preds(forward, x)
    w = _lci_weights(forward)
    l2 = ops.reduce_l2(p, d, w.to(p.dtype) if p.is_complex() else w)
    T = prior.T_dev
    l1 = ops.reduce_l1(x) * T if isinstance(T, float) else ops.reduce_l1(x, T)
    return 0.5 * l2.real + l1 / float(params.lmda)


def _level(forward, prior, params, X, batch, threshold, alpha):
    """the level gamma on the device -> (float64 [1], its [batch] expansion): ``threshold``, or with ``None``
    :func:`approx_credible_region_threshold` of ``map_objective(X)`` in the real dimensions the samplers move in"""
    if threshold is None:
        ndim = int(forward.nparams) * (2 if getattr(params, "complex", False) else 1)
        gamma1 = approx_credible_region_threshold(map_objective(forward, prior, params, X), ndim, alpha)  # (a device tensor)
    else:
        gamma1 = torch.full((1,), float(threshold), dtype=torch.float64, device=X.device)
    return gamma1, gamma1.expand(batch).contiguous()


def _regions_setup(fn, forward, X_map, regions, batch, rounds=None):
    """the MAP point as one complex128 [nparams] device vector, its image, the label contract (-1: in no region; 0 ...
    nregions - 1, each with a pixel), the batch, to which the operators are grown, and the search rounds of a caller that has
    them -> (transform, X, x_map, labels, nregions, pixels per region, batch)"""
    tr = forward.transform
    X = ops.as_device(X_map)
    if X.dim() == 2 and X.shape[0] == 1:
        X = X[0]
    if X.dim() != 1 or X.shape[0] != int(forward.nparams):
        raise ValueError("%s: X_map must be one MAP point [nparams]" % fn)
    if batch is None:
        batch = int(getattr(tr, "max_chains", 1))
    batch = int(batch)
    if batch < 1 or (rounds is not None and int(rounds) < 1):
        raise ValueError("%s needs batch >= 1 and rounds >= 1" % fn)
    for op in (tr, getattr(forward, "measurement", None)):
        if hasattr(op, "ensure_chains"):
            op.ensure_chains(batch)
    X = X.to(torch.complex128).contiguous()
    x_map = ops.as_device(tr.inverse(X[None]))[0]
    labels = np.asarray(regions)
    if not np.issubdtype(labels.dtype, np.integer) or labels.size != x_map.shape[0]:
        raise ValueError("%s: regions must be an integer label per pixel (%d pixels)" % (fn, x_map.shape[0]))
    if labels.min() < -1 or labels.max() < 0:
        raise ValueError("%s: labels are -1 (no region) or 0 ... nregions - 1, with at least one region" % fn)
    nreg = int(labels.max()) + 1
    counts = np.bincount(labels[labels >= 0].ravel(), minlength=nreg)
    if (counts == 0).any():
        raise ValueError("%s: region %d has no pixel" % (fn, int(np.flatnonzero(counts == 0)[0])))
    return tr, X, x_map, labels, nreg, counts, batch


class _PathSearch:
    """``{xi : F(a + xi b) <= gamma}`` for every region, ``batch`` of them at a time, F the objective of
    :func:`map_objective`: the weights, the threshold of the prior and the level, the results ``out`` [nregions, 8] and
    ``status`` [nregions] on the device, and the buffers of a batch (``quad`` [batch, 3], the ``ops.lci_scratch``)"""

    def __init__(self, forward, prior, params, X, nreg, batch, threshold, alpha, rounds):
        dev = X.device
        self.nreg, self.rounds = int(nreg), rounds
        self.lmda, self.T, self.w = float(params.lmda), prior.T_dev, _lci_weights(forward)
        self.gamma1, self.gamma = _level(forward, prior, params, X, batch, threshold, alpha)
        self.out = torch.empty((self.nreg, 8), dtype=torch.float64, device=dev)
        self.status = torch.empty(self.nreg, dtype=torch.int32, device=dev)
        self.quad = torch.empty((batch, 3), dtype=torch.float64, device=dev)
        self.scratch = ops.lci_scratch(max(int(X.shape[0]), int(forward.data_dev.numel())), batch, dev)

    def run(self, r0, a, b, pa, pb, d, between=None):
        """the regions r0 ... r0 + len(a) - 1: the data terms of the ``len(pa)`` rows of predictions ``pa``, ``pb`` into
        ``quad`` (a caller whose batches are always full hands over more rows than it searches), ``between(quad)`` if given,
        then the search along ``(a, b)`` into ``out`` and ``status``"""
        rows = a.shape[0]
        ops.lci_data_terms(pa, pb, d, self.w, out=self.quad[: pa.shape[0]], scratch=self.scratch)
        if between is not None:
            between(self.quad)
        ops.lci_search(a, b, self.T, self.quad[:rows], self.lmda, self.gamma[:rows], rounds=self.rounds,
                       out=self.out[r0 : r0 + rows], status=self.status[r0 : r0 + rows], scratch=self.scratch)

    def read_back(self, *extras):
        """the one read-back: the results, the level and the caller's ``extras`` (flat float64 device tensors) in one copy ->
        (dict of ``lower``, ``upper``, ``width`` (the larger of the two final bracket widths), ``f_min``, ``xi_min``,
        ``outer`` [nregions, 2], ``status`` int32 and ``threshold`` (a float), the extras as numpy arrays)"""
        parts = [self.out.reshape(-1), self.status.to(torch.float64), self.gamma1.reshape(-1)[:1], *extras]
        host, status, thr, *extras = np.split(torch.cat(parts).cpu().numpy(), np.cumsum([p.numel() for p in parts])[:-1])
        host = host.reshape(self.nreg, 8)
        return dict(lower=host[:, 0], upper=host[:, 1], width=np.fmax(host[:, 2], host[:, 3]), f_min=host[:, 4], xi_min=host[:, 5],
                    outer=host[:, 6:8].copy(), status=status.astype(np.int32), threshold=float(thr[0])), extras


class _RegionResult:
    """one entry per region of every name in ``FIELDS``, the ``threshold`` used and the ``labels``"""

    FIELDS = ()
    PAINTED = None  # the field ``to_map`` paints by default

    def __init__(self, labels, threshold, **fields):
        self.labels, self.threshold = labels, threshold
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    def to_map(self, values=None):
        """paint one value per region (default: the field ``PAINTED``, a bool as 1.0 / 0.0) back onto the pixels, in the
        shape of the label array; NaN where the label is -1"""
        painted = getattr(self, self.PAINTED)
        values = np.asarray(painted if values is None else values, dtype=np.float64)
        if values.shape != painted.shape:
            raise ValueError("to_map: one value per region is expected")
        out = np.full(self.labels.shape, np.nan)
        on = self.labels >= 0
        out[on] = values[self.labels[on]]
        return out

