"""
Hypothesis tests of image structure: :func:`hypothesis_test` forms a surrogate image without the
structure of each region (:func:`inpaint_regions`, :func:`smooth_regions`) and follows the objective from the MAP point to it;
:func:`inpaint_step_np` and :func:`inpaint_np` state the inpainting kernel and its iteration in numpy.
"""
import numpy as np
import torch

from .. import ops
from .._lib import LCI_POINTS
from .regions import _check_scope, _lci_preds, _PathSearch, _RegionResult, _regions_setup

HYP_NONFINITE = 8  # status bit of a region whose surrogate, sums or profile are not finite (beside the LCI_* bits)


def inpaint_sum_depth(npix):
    """the longest chain of additions in a fixed-order sum of ``pxm_inpaint_step`` over npix pixels (the error model of
    DESIGN.md section 14c), for both dtypes: a lane adds the two terms of each of its pairs of real pixels one after the
    other (one workgroup of 256 lanes per 1024 pixels up to 512 workgroups, grid-stride beyond; a complex pixel is one
    term, never a longer chain), then the 6 levels of the wave tree, the 4 waves of the workgroup, the slices a lane of the
    finishing wave adds and its tree"""
    n = int(npix)
    slices = min(512, max(1, -(-n // 1024)))
    return 2 * -(-(-(-n // 2)) // (slices * 256)) + 6 + 4 + -(-slices // 64) + 6


def inpaint_step_np(y, x_prev, x_map, labels, region, tol2, done, iters, stat):
    """the numpy statement of ``pxm_inpaint_step``: ``y``, ``x_prev`` [C, npix], ``x_map`` [npix], ``labels`` int [npix],
    ``region``, ``done``, ``iters`` int [C], ``stat`` [C, 2] -> new ``(x_next, done, iters, stat)``.  The select is exact;
    the two sums are formed in long double (``stat`` comes back as long double [C, 2]) and the flag is ``stat[0] <= tol2 *
    stat[1]`` on their float64 roundings, one multiply and one compare.  A slot that is done is copied through and nothing
    of it changes; a label < 0 belongs to no slot; a NaN never freezes a slot."""
    ld = np.longdouble
    y, x_prev, x_map = np.asarray(y), np.asarray(x_prev), np.asarray(x_map)
    labels, region = np.asarray(labels).reshape(-1), np.asarray(region)
    done, iters = np.array(done, dtype=np.int32), np.array(iters, dtype=np.int32)
    stat = np.array(stat, dtype=ld)
    x_next = np.array(x_prev, copy=True)
    for c in range(x_prev.shape[0]):
        if done[c]:
            continue
        inside = (labels == region[c]) & (labels >= 0)
        x_next[c] = np.where(inside, y[c], x_map.astype(x_prev.dtype))
        d = x_next[c] - x_prev[c]  # (each component difference rounded once, as on the device)
        d2 = (d.real.astype(ld) ** 2).sum() + (d.imag.astype(ld) ** 2).sum()
        n2 = (x_next[c].real.astype(ld) ** 2).sum() + (x_next[c].imag.astype(ld) ** 2).sum()
        iters[c] += 1
        stat[c] = d2, n2
        with np.errstate(invalid="ignore", over="ignore"):
            done[c] = int(np.float64(d2) <= np.float64(tol2) * np.float64(n2))
    return x_next, done, iters, stat


def _soft_np(x, T):
    with np.errstate(divide="ignore", invalid="ignore"):
        mod = np.abs(x)
        return np.where(mod > T, x * (1.0 - T / np.where(mod > 0, mod, 1.0)), 0.0 * x)


def inpaint_np(A, Psi, x_map, zeta, tau, iters, tol):
    """the numpy statement of segment inpainting for one region: ``x^0 = x* (1 - zeta)``, ``x^{t+1} = x* (1 - zeta) + zeta
    Psi soft_tau(A x^t)`` for at most ``iters`` iterations, frozen once ``|x^{t+1} - x^t|^2 <= tol^2 |x^{t+1}|^2``.  ``A``,
    ``Psi``: callables (image -> coefficients -> image); ``zeta``: 0 / 1 per pixel; ``tau``: scalar or one value per
    coefficient.  Returns a dict: ``x``, ``iters_used``, ``rel_change`` (of the last iteration made) and ``history`` (the
    relative change of every iteration made)."""
    x_map = np.asarray(x_map)
    inside = np.asarray(zeta).reshape(-1) != 0
    labels = np.where(inside, 0, -1)
    x = np.where(inside, 0.0 * x_map, x_map)[None]
    done, its, stat = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros((1, 2))
    history = []
    for _ in range(int(iters)):
        if done[0]:
            break
        y = np.asarray(Psi(_soft_np(np.asarray(A(x[0])), tau))).astype(x.dtype)[None]
        x, done, its, stat = inpaint_step_np(y, x, x_map, labels, [0], float(tol) ** 2, done, its, stat)
        history.append(float(np.sqrt(stat[0, 0] / stat[0, 1])) if stat[0, 1] > 0 else (0.0 if stat[0, 0] == 0 else np.inf))
    return dict(x=x[0], iters_used=int(its[0]), rel_change=history[-1] if history else np.nan, history=history)


def gaussian_smooth(x, L, sigma, spin=0):
    """``G_sigma * x`` for MW images ``x`` [C, npix] (or [npix]) on the device: one ``ops.ShtPlan(L, spin)`` forward, a multiply
    by ``exp(-l (l + 1) sigma^2 / 2)`` on the ssht index ``l^2 + l + m``, one inverse -> complex128, the shape of ``x``"""
    x = ops.as_device(x, torch.complex128)
    plan = ops.ShtPlan(int(L), int(spin), max_chains=1 if x.dim() == 1 else int(x.shape[0]))
    el = np.repeat(np.arange(int(L)), 2 * np.arange(int(L)) + 1).astype(np.float64)
    g = ops.as_device(np.exp(-el * (el + 1.0) * float(sigma) ** 2 / 2.0))
    return plan.inverse(plan.forward(x) * g)


class SurrogateImages:
    """the result of :func:`inpaint_regions` / :func:`smooth_regions`: ``images`` (complex128 device tensor [nregions, npix]:
    the surrogate of every region), ``iters_used`` (int32 [nregions]), ``rel_change`` (float64 [nregions]: ``|x^{t+1} - x^t|
    / |x^{t+1}|`` of the last iteration a region made), ``frozen`` (bool [nregions]), ``x_map`` (the MAP image, [npix]),
    ``replayed`` (the iterations ran by graph replay) and ``graph_error`` (``None``, or the exception that made capture fall
    back to eager stepping)"""

    def __init__(self, images, iters_used, rel_change, frozen, x_map, replayed=False, graph_error=None):
        self.images, self.iters_used, self.rel_change, self.frozen, self.x_map = images, iters_used, rel_change, frozen, x_map
        self.replayed, self.graph_error = replayed, graph_error


def _rel_change(stat):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(stat[:, 0] / stat[:, 1])


class _SurrogateBatches:
    """The surrogate images of the regions, ``batch`` slots at a time, in static buffers: ``run(r0)`` leaves the surrogates of
    the regions r0 ... r0 + batch - 1 in ``images`` with ``iters`` / ``stat`` / ``done`` beside them, all of them views that
    the next call overwrites.  A slot beyond the last region holds region -1 (no pixel: its image is the MAP image), so
    every batch is a full one and one captured graph serves them all; a slot's numbers do not depend on its batch."""

    def __init__(self, tr, x_map, labels, nreg, batch):
        dev = x_map.device
        self.tr, self.x_map, self.nreg, self.batch = tr, x_map, int(nreg), int(batch)
        self.npix = int(x_map.shape[0])
        self.labels = torch.from_numpy(np.ascontiguousarray(labels.reshape(-1).astype(np.int32))).to(dev)
        self.ids = torch.arange(batch, dtype=torch.int32, device=dev)
        self.region = torch.empty(batch, dtype=torch.int32, device=dev)
        self.done = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.stat = torch.zeros((batch, 2), dtype=torch.float64, device=dev)
        self.XA = torch.empty((batch, self.npix), dtype=torch.complex128, device=dev)
        self.XB = torch.empty_like(self.XA)
        self.scratch = ops.inpaint_scratch(self.npix, batch, dev)
        self.images = self.XA
        self.graph, self.graph_error = None, None

    def _step(self, y, src, dst, tol2):
        ops.inpaint_step(y, src, self.x_map, self.labels, self.region, tol2, self.done, self.iters, self.stat, out=dst,
                         scratch=self.scratch)

    def _begin(self, r0):
        """the regions of the batch, flags and counters cleared"""
        self.region.copy_(torch.where(self.ids + int(r0) < self.nreg, self.ids + int(r0), -1))
        self.done.zero_(), self.iters.zero_(), self.stat.zero_()


class _InpaintBatches(_SurrogateBatches):
    def __init__(self, tr, x_map, labels, nreg, batch, tau, iters, tol, use_graph):
        super().__init__(tr, x_map, labels, nreg, batch)
        self.niter, self.tol2 = int(iters), float(tol) ** 2
        if self.niter < 1 or not (float(tol) >= 0.0 and np.isfinite(float(tol))):
            raise ValueError("inpainting needs iters >= 1 and a finite tol >= 0")
        tau_arr = np.asarray(tau.detach().cpu() if isinstance(tau, torch.Tensor) else tau, dtype=np.float64)
        if tau_arr.size == 1:  # (a python scalar: the wrapper of the threshold kernel then reads nothing back)
            self.tau = float(tau_arr.reshape(-1)[0])
        else:
            self.tau = ops.as_device(tau_arr.reshape(-1), torch.float64)
        if not np.all(tau_arr >= 0.0):
            raise ValueError("inpainting needs tau >= 0")
        self.zero = torch.zeros_like(self.XA)
        if use_graph and self.niter >= 2:
            self._capture()

    def _one(self, src, dst):
        """one iteration from the images in src to dst: A, the threshold, Psi, then the step kernel"""
        coef = ops.as_device(self.tr.forward(src), torch.complex128)
        y = ops.as_device(self.tr.inverse(ops.soft(coef, self.tau)), torch.complex128)
        self._step(y, src, dst, self.tol2)

    def _two(self):
        self._one(self.XA, self.XB)
        self._one(self.XB, self.XA)

    def _init(self, r0):
        """x^0 = x* (1 - zeta) in XA, by the step kernel itself on y = 0 (no indicator array here either)"""
        self._begin(r0)
        self._step(self.zero, self.XB, self.XA, 0.0)
        self.done.zero_(), self.iters.zero_(), self.stat.zero_()

    def _capture(self):
        """two ping-pong iterations in one HIP graph, after a warm-up on a side stream (lazy allocations); when capture
        raises: eager stepping, same results"""
        try:
            self.XB.zero_()
            self._init(0)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._two()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with ops.capture_scope(), torch.cuda.graph(g):
                self._two()
            self.graph = g
        except Exception as exc:  # capture unsupported in this environment
            self.graph, self.graph_error = None, repr(exc)
            torch.cuda.synchronize()

    def run(self, r0):
        self.XB.zero_()  # (x_prev of the initialising step: any finite values)
        self._init(r0)
        for _ in range(self.niter // 2):
            if self.graph is not None:
                self.graph.replay()
            else:
                self._two()
        if self.niter % 2:
            self._one(self.XA, self.XB)
        self.images = self.XB if self.niter % 2 else self.XA
        return self.images


class _SmoothBatches(_SurrogateBatches):
    def __init__(self, tr, x_map, labels, nreg, batch, sigma):
        super().__init__(tr, x_map, labels, nreg, batch)
        sigma = float(sigma)
        if not (sigma >= 0.0 and np.isfinite(sigma)):
            raise ValueError("the smoothing surrogate needs a finite sigma >= 0")
        L = getattr(tr, "L", None)
        if L is None or int(L) * (2 * int(L) - 1) != self.npix:
            raise ValueError("the smoothing surrogate needs a transform of MW images with a bandlimit L")
        self.smooth = gaussian_smooth(x_map, int(L), sigma, int(getattr(tr, "spin", 0)))
        self.XB.copy_(x_map[None].expand(batch, -1))  # x_prev of the one step: rel_change is |x_sgt - x*| / |x_sgt|
        self.Y = self.smooth[None].expand(batch, -1).contiguous()

    def run(self, r0):
        """one step of the step kernel with tol = 0: x_sgt = x* (1 - zeta) + zeta (G_sigma * x*)"""
        self._begin(r0)
        self._step(self.Y, self.XB, self.XA, 0.0)
        return self.images


def _collect_surrogates(batches, nreg):
    """every batch of ``batches`` into one :class:`SurrogateImages` (nregions x npix complex values on the device), with
    one read-back at the end"""
    B = batches.batch
    images = torch.empty((nreg, batches.npix), dtype=torch.complex128, device=batches.x_map.device)
    its, stats, dones = [], [], []
    for r0 in range(0, nreg, B):
        Cb = min(B, nreg - r0)
        images[r0 : r0 + Cb] = batches.run(r0)[:Cb]
        its.append(batches.iters[:Cb].clone()), stats.append(batches.stat[:Cb].clone()), dones.append(batches.done[:Cb].clone())
    stat = torch.cat(stats).cpu().numpy()
    return SurrogateImages(images, torch.cat(its).cpu().numpy(), _rel_change(stat), torch.cat(dones).cpu().numpy() != 0, batches.x_map,
                           replayed=batches.graph is not None, graph_error=batches.graph_error)


def inpaint_regions(forward, X_map, regions, tau, iters=100, tol=1e-6, batch=None, use_graph=True):
    """Segment-inpainted surrogates of the MAP image, one per region (Cai, Pereyra & McEwen 2018 II section 4.2; DESIGN.md
    section 14c): with ``A = transform.forward``, ``Psi = transform.inverse``, ``x* = Psi X_map`` and ``zeta`` the indicator of
    a region, ``x^0 = x* (1 - zeta)`` and ``x^{t+1} = x* (1 - zeta) + zeta Psi soft_tau(A x^t)`` for ``iters`` iterations; a
    region freezes once ``|x^{t+1} - x^t|^2 <= tol^2 |x^{t+1}|^2`` (both norms over the whole image) and is copied through
    from then on.  Everything runs on the device and nothing is read back until the end.

    :param regions: int labels over the pixels, the contract of :func:`local_credible_intervals`
    :param tau: the threshold, a scalar or one value per coefficient ``[nparams]``
    :param batch: regions per pass; ``None``: the chain capacity of the transform.  The last batch is filled with slots
        that hold no region; a region's numbers do not depend on its batch
    :param use_graph: capture two iterations into a HIP graph and replay them (eager stepping when capture raises, and
        with ``False``: the same numbers)

    Returns :class:`SurrogateImages` (``nregions x npix`` complex values stay on the device: mind the size)."""
    _check_scope("inpaint_regions", forward)
    tr, _, x_map, labels, nreg, _, batch = _regions_setup("inpaint_regions", forward, X_map, regions, batch)
    return _collect_surrogates(_InpaintBatches(tr, x_map, labels, nreg, batch, tau, iters, tol, use_graph), nreg)


def smooth_regions(forward, X_map, regions, sigma, batch=None):
    """The smoothing surrogates of the MAP image, one per region: ``x* (1 - zeta) + zeta (G_sigma * x*)``, the surrogate for
    testing sub-structure (:func:`gaussian_smooth`, then one step of the inpainting kernel).  Returns
    :class:`SurrogateImages`; ``rel_change`` is ``|x_sgt - x*| / |x_sgt|``."""
    _check_scope("smooth_regions", forward)
    tr, _, x_map, labels, nreg, _, batch = _regions_setup("smooth_regions", forward, X_map, regions, batch)
    return _collect_surrogates(_SmoothBatches(tr, x_map, labels, nreg, batch, sigma), nreg)


class HypothesisTestResult(_RegionResult):
    """the result of :func:`hypothesis_test`, one entry per region: ``physical`` (bool: the surrogate lies outside the
    credible region, ``f_sgt > threshold``; ``False``: inconclusive), ``removable`` (xi+, the end of ``{xi : F(xi) <=
    threshold}`` along the path from the MAP point, xi = 0, to the surrogate, xi = 1: the fraction of the structure that can
    be removed inside the credible region; >= 1, possibly inf, where the test is inconclusive), ``f_sgt`` (= ``profile[:,
    -1]``), ``profile`` (``[nregions, 32]``: F at ``xi`` = j / 31), ``iters_used``, ``rel_change`` (of the surrogate),
    ``status`` (0, or the ``LCI_*`` bits of the search and ``HYP_NONFINITE``), ``xi``, the ``threshold`` used and the ``labels``;
    ``lower`` (xi-) and ``width`` (the larger of the two final bracket widths of the search: each end is known to that);
    ``to_map()`` paints ``physical`` as 1.0 / 0.0"""

    FIELDS = ("physical", "removable", "lower", "width", "f_sgt", "profile", "iters_used", "rel_change", "status")
    PAINTED = "physical"

    def __init__(self, labels, threshold, xi, **fields):
        super().__init__(labels, threshold, **fields)
        self.xi = xi


def hypothesis_test(forward, prior, params, X_map, regions, tau=None, sigma=None, surrogate="inpaint", threshold=None, alpha=0.05,
                    iters=100, tol=1e-6, rounds=10, batch=None):
    """Hypothesis tests of image structure from the MAP point (Cai, Pereyra & McEwen 2018 II section 4.2; DESIGN.md section
    14c).  For every region a surrogate image ``x_sgt`` without the structure is formed -- ``surrogate="inpaint"``:
    :func:`inpaint_regions` with the threshold ``tau``; ``surrogate="smooth"``: :func:`smooth_regions` with the width
    ``sigma`` -- and the objective F of :func:`map_objective` is followed along the straight path ``X(xi) = X_map + xi A(x_sgt
    - x*)``.  ``F(1) > threshold``: the surrogate is outside the credible region, the structure is physical; otherwise the
    test is inconclusive (so it is when the surrogate equals ``x*``).  ``threshold=None``: the level of
    :func:`local_credible_intervals`.  Scope and refusals: those of :func:`local_credible_intervals`.

    Per batch: the surrogate, one ``transform.forward`` and one ``forward.forward`` call, the 32-point profile by
    ``lci_eval`` and ``[xi-, xi+]`` by ``lci_search``; one read-back at the end.  Returns :class:`HypothesisTestResult`."""
    _check_scope("hypothesis_test", forward, prior)
    if surrogate not in ("inpaint", "smooth"):
        raise ValueError("hypothesis_test: surrogate must be 'inpaint' or 'smooth'")
    if (surrogate == "inpaint") != (tau is not None) or (surrogate == "smooth") != (sigma is not None):
        raise ValueError("hypothesis_test: surrogate='inpaint' takes tau and no sigma, surrogate='smooth' sigma and no tau")
    tr, X, x_map, labels, nreg, _, batch = _regions_setup("hypothesis_test", forward, X_map, regions, batch, rounds)
    if surrogate == "inpaint":
        batches = _InpaintBatches(tr, x_map, labels, nreg, batch, tau, iters, tol, True)
    else:
        batches = _SmoothBatches(tr, x_map, labels, nreg, batch, sigma)
    dev = X.device
    search = _PathSearch(forward, prior, params, X, nreg, batch, threshold, alpha, rounds)
    a = X[None].expand(batch, -1).contiguous()
    pa1, d = _lci_preds(forward, X[None])
    pa = pa1.expand(batch, -1).contiguous()
    xi1 = torch.arange(LCI_POINTS, dtype=torch.float64, device=dev) / (LCI_POINTS - 1.0)
    xi = xi1[None].expand(batch, -1).contiguous()
    profile = torch.empty((nreg, LCI_POINTS), dtype=torch.float64, device=dev)
    its = torch.empty(nreg, dtype=torch.int32, device=dev)
    stat = torch.empty((nreg, 2), dtype=torch.float64, device=dev)
    P = torch.empty((batch, LCI_POINTS + 2), dtype=torch.float64, device=dev)
    for r0 in range(0, nreg, batch):
        Cb = min(batch, nreg - r0)
        x_sgt = batches.run(r0)
        b = ops.as_device(tr.forward(x_sgt - x_map[None]), torch.complex128)
        pb, _ = _lci_preds(forward, b)

        def profile_rows(quad):
            """F at the 32 points of the live rows, from the sums just formed (every batch of ``batches`` is a full one)"""
            ops.lci_eval(a, b, search.T, xi, out=P, scratch=search.scratch)
            q0, q1, q2 = quad[:Cb, 0:1], quad[:Cb, 1:2], quad[:Cb, 2:3]
            profile[r0 : r0 + Cb] = ((q2 * xi[:Cb] + q1) * xi[:Cb] + q0) + P[:Cb, :LCI_POINTS] / search.lmda

        search.run(r0, a[:Cb], b[:Cb], pa, pb, d, between=profile_rows)
        its[r0 : r0 + Cb] = batches.iters[:Cb]
        stat[r0 : r0 + Cb] = batches.stat[:Cb]
    res, (it, sums, prof, xis) = search.read_back(its.to(torch.float64), stat.reshape(-1), profile.reshape(-1), xi1)
    sums, prof, thr = sums.reshape(nreg, 2), prof.reshape(nreg, LCI_POINTS), res["threshold"]
    st = res["status"]
    st[~(np.isfinite(prof).all(axis=1) & np.isfinite(sums).all(axis=1))] |= HYP_NONFINITE
    f_sgt = prof[:, -1].copy()
    with np.errstate(invalid="ignore"):
        physical = f_sgt > thr
        # xi = 1 was evaluated: where F(1) <= threshold the end of the set is not left of it, whatever the last bracket says
        removable = np.where(~physical & np.isfinite(f_sgt), np.fmax(res["upper"], 1.0), res["upper"])
    return HypothesisTestResult(labels, thr, xis, physical=physical, removable=removable, lower=res["lower"], width=res["width"],
                                f_sgt=f_sgt, profile=prof, iters_used=it.astype(np.int32), rel_change=_rel_change(sums), status=st)
