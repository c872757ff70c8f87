#!/usr/bin/env python
"""
End-to-end use of the drop-in API, following the flow of the reference's
experiments/earthtopography/main.py:72-185 on synthetic data (the ETOPO1 file needs healpy):

    build data -> SphericalWaveletTransformOperator -> PxMCMCParams -> S2_Wavelets_L1 -> MYULA.run() -> save_mcmc
    -> credible-interval maps of the saved samples.

    python examples/topography_synthetic.py --L 32 --nsamples 50 --ngap 100 --chains 4 --outdir /tmp

Both routes write the 95 % credible-interval map of chain 0 as ``*_ci.npy``.  ``--summary image --summary-alpha A`` keeps no
chain and writes the (1 - A) map from the streaming summary of the images instead: at A = 0.05, the alpha of the chain route,
the two files are equal.

``--analysis-map`` runs no chain: it finds the MAP image of the analysis-setting posterior by primal-dual splitting
(``pxmcmc_amd.optim.PrimalDual``) and writes it as ``analysis_map_<jobid>.npy``; ``--mu`` scales the prior,
``--analysis-balance`` the ratio of the two steps.

``--tv-map`` does the same with the total-variation prior ``pxmcmc_amd.prior.TV_S2`` on the image itself (no wavelet plan) and
writes ``tv_map_<jobid>.npy``; ``--tv`` samples that posterior in the analysis setting (``--algo`` as usual) and writes the
posterior mean and the credible-interval map.  ``--tv-strength`` is the threshold T per unit of ``lmda * mu``.
"""
import argparse
import copy
import os
import sys
from datetime import datetime

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pxmcmc_amd import ops  # noqa: E402
from pxmcmc_amd.forward import ForwardOperator, SphericalWaveletTransformOperator  # noqa: E402
from pxmcmc_amd.measurements import Identity  # noqa: E402
from pxmcmc_amd.mcmc import MYULA, SKROCK, PxMALA, PxMCMCParams  # noqa: E402
from pxmcmc_amd.optim import FISTA, LassoGibbs, PrimalDual  # noqa: E402
from pxmcmc_amd.prior import L1, S2_Wavelets_L1, TV_S2  # noqa: E402
from pxmcmc_amd.sapg import SAPG  # noqa: E402
from pxmcmc_amd.saving import save_mcmc  # noqa: E402
from pxmcmc_amd.transforms import IdentityTransform  # noqa: E402
from pxmcmc_amd.uncertainty import (chain_to_images, credible_interval_range, hypothesis_test, local_credible_intervals,  # noqa: E402
                                    superpixel_regions)
from pxmcmc_amd.utils import _multires_bandlimits  # noqa: E402


def map_start(forwardop, regulariser, params, L_g, start_point, tol=1e-3, max_iter=2000, restart=None):
    """FISTA on the samplers' posterior as the chain's start point.  The steps of FISTA shrink like 1 / k, so the run is
    bounded: at most ``max_iter`` operator pairs, stopping at a relative step of ``tol`` (a start point, not a final
    estimate; ``restart="gradient"``, --map-restart, removes that tail).  1 / (L_g (1 + 1e-3)) is a valid step for the real-part operator FISTA uses with complex data as well."""
    fista = FISTA(forwardop, regulariser, params, gamma=1 / (L_g * (1 + 1e-3)), tol=tol, max_iter=max_iter, restart=restart)
    x = fista.run(start_point=start_point)
    its = f"{int(fista.niter[0])} iterations" + (f", {int(fista.nrestarts[0])} restarts" if restart else "")
    if fista._stock_prox:
        print(f"MAP start: FISTA stopped after {its} (converged: {bool(fista.converged[0])}), "
              f"objective {fista.objective_map[0]:.6e}")
    else:  # the prior's own prox carries its own threshold: the fixed point of that iteration, not the posterior's MAP
        print(f"start point: fixed point of the prior's own prox-gradient iteration (g + (lmda / gamma) f, not the MAP) after "
              f"{its} (converged: {bool(fista.converged[0])})")
    return x


def analysis_map(data, args, L, B, J_min, truth):
    """--analysis-map: the MAP image of the analysis-setting posterior 1/2 Re L2(x) + (1 / lmda) sum_i T_i |(A x)_i| (the state
    is the image, A = transform.inverse_adjoint) by primal-dual splitting.  T carries the quadrature
    weights of the coefficients' grids, as the synthesis prior's threshold does.  Writes the image beside the run."""
    forwardop = SphericalWaveletTransformOperator(data, args.sigma, "analysis", L, B, J_min, max_chains=1)
    tr = forwardop.transform
    lmda = 1e-3
    weights = S2_Wavelets_L1("synthesis", None, None, 1.0, L=L, B=B, J_min=J_min).map_weights
    regulariser = L1("analysis", tr.inverse, tr.inverse_adjoint, lmda * args.mu * weights / weights.mean())
    params = PxMCMCParams(lmda=lmda, mu=args.mu, verbosity=0)
    est = PrimalDual(forwardop, regulariser, params, balance=args.analysis_balance, tol=1e-6, max_iter=20000)
    x = est.run(start_point=np.zeros(forwardop.nparams))
    rel = np.sqrt(np.mean(np.abs(x.real - truth) ** 2)) / np.sqrt(np.mean(np.abs(truth) ** 2))
    path = os.path.join(args.outdir, f"analysis_map_{args.jobid}.npy")
    np.save(path, x.real)
    print(f"analysis MAP: tau = {est.tau:.4e}, sigma = {est.sigma:.4e} (||A||^2 = {est.A_norm2:.4f}, L_g = {est.L_g:.4e}); "
          f"{int(est.niter[0])} iterations (converged: {bool(est.converged[0])}, graph replay: {est.used_graph}), objective "
          f"{est.objective_map[0]:.6e} = {est.data_term[-1, 0]:.6e} + {est.prior_term[-1, 0]:.6e}, stationarity "
          f"{est.stationarity[-1, 0]:.3e}; error against the truth {rel:.3f} (noise {args.sigma:.3f}); image in {path}")
    return path, rel, est


def tv_operators(data, args, L, lmda, prox_iters=16):
    """the analysis-setting operator whose state is the image itself (identity measurement, float64 state for real data) and
    the isotropic TV prior on the MW grid"""
    P = data.size
    forwardop = ForwardOperator(data, args.sigma, "analysis", IdentityTransform(), Identity(P, P), nparams=P)
    return forwardop, TV_S2(L, lmda * args.mu * args.tv_strength, prox_iters=prox_iters)


def tv_map(data, args, L, truth):
    """--tv-map: the MAP image of 1/2 Re L2(x) + (1 / lmda) T TV(x) by primal-dual splitting on the fused TV launches.
    Writes the image beside the run."""
    lmda = 1e-3
    forwardop, regulariser = tv_operators(data, args, L, lmda)
    params = PxMCMCParams(lmda=lmda, mu=args.mu, verbosity=0)
    est = PrimalDual(forwardop, regulariser, params, balance=args.analysis_balance, tol=1e-6, max_iter=20000)
    x = est.run(start_point=np.zeros(forwardop.nparams))
    rel = np.sqrt(np.mean(np.abs(x.real - truth) ** 2)) / np.sqrt(np.mean(np.abs(truth) ** 2))
    path = os.path.join(args.outdir, f"tv_map_{args.jobid}.npy")
    np.save(path, x.real)
    print(f"TV MAP: tau = {est.tau:.4e}, sigma = {est.sigma:.4e} (||A||^2 = {est.A_norm2:.4e}, L_g = {est.L_g:.4e}); "
          f"{int(est.niter[0])} iterations (converged: {bool(est.converged[0])}, graph replay: {est.used_graph}, fused launches: "
          f"{est.fused}), objective {est.objective_map[0]:.6e} = {est.data_term[-1, 0]:.6e} + {est.prior_term[-1, 0]:.6e}, "
          f"stationarity {est.stationarity[-1, 0]:.3e}; error against the truth {rel:.3f} (noise {args.sigma:.3f}); image in {path}")
    return path, rel, est


def tv_sample(data, args, L, truth):
    """--tv: sample the TV posterior in the analysis setting on the generic stepping engine; the prox is the exact one
    (TV_S2.proxf), replayed from the captured graph.  Writes the chain, the posterior mean and the credible-interval map."""
    lmda = 1e-3
    forwardop, regulariser = tv_operators(data, args, L, lmda)
    delta = 0.8 / (1.0 / args.sigma ** 2 + 1.0 / lmda)
    if args.algo == "skrock":
        delta *= args.s ** 2
    params = PxMCMCParams(nsamples=args.nsamples, nburn=args.nburn, ngap=args.ngap, delta=delta, lmda=lmda, mu=args.mu, s=args.s,
                          verbosity=max(1, args.ngap * 10))
    cls = {"myula": MYULA, "pxmala": PxMALA, "skrock": SKROCK}[args.algo]
    mcmc = cls(forwardop, regulariser, params, nchains=args.chains)
    start = datetime.now()
    mcmc.run(start_point=np.asarray(data, dtype=float).copy())
    elapsed = datetime.now() - start
    base = os.path.join(args.outdir, f"{args.algo}_tv_{args.jobid}")
    path = save_mcmc(mcmc, params, args.outdir, filename=f"{args.algo}_tv_{args.jobid}", L=L, sigma=args.sigma,
                     nparams=forwardop.nparams, setting="analysis", time=str(elapsed), chains=args.chains)
    images = np.asarray(mcmc.chain if args.chains == 1 else mcmc.chain[0]).real  # the state is the image
    mean, ci = images.mean(axis=0), credible_interval_range(images)
    np.save(base + "_mean.npy", mean)
    np.save(base + "_ci.npy", ci)
    rel = np.sqrt(np.mean(np.abs(mean - truth) ** 2)) / np.sqrt(np.mean(np.abs(truth) ** 2))
    print(f"saved {path}; {mcmc.niter} iterations x {args.chains} chain(s) in {elapsed} (graph replay: {mcmc.used_graph}); "
          f"posterior-mean error {rel:.3f} (noise {args.sigma:.3f}); median 95% CI width {np.median(ci):.3f}")
    return path, rel, ci


def local_ci_maps(forwardop, regulariser, params, x_map, L, size, base):
    """--local-ci SIZE: the local credible intervals of the MAP point on superpixels of SIZE x SIZE samples (DESIGN.md section
    14b), at the approximate 95 % HPD level; writes the lower / upper / range maps beside the run"""
    lci = local_credible_intervals(forwardop, regulariser, params, x_map, superpixel_regions(L, size))
    ok = lci.status == 0
    for name in ("lower", "upper", "range"):
        np.save(f"{base}_lci_{name}.npy", lci.to_map(getattr(lci, name)))
    print(f"local credible intervals: {ok.sum()} of {ok.size} superpixels of {size} x {size} samples have an interval at the "
          f"level {lci.threshold:.6e}; median range {np.median(lci.range[ok]) if ok.any() else float('nan'):.4f}; "
          f"maps in {base}_lci_lower.npy / _upper.npy / _range.npy")
    return lci


def hyp_test_maps(forwardop, regulariser, params, x_map, L, size, frac, base):
    """--hyp-test SIZE: the hypothesis test of structure of every superpixel of SIZE x SIZE samples
    at the approximate 95 % HPD level, with the inpainting threshold tau = frac max |A x*|; writes the physical (1 / 0) and
    removable maps beside those of the local credible intervals"""
    tr = forwardop.transform
    X = ops.as_device(np.asarray(x_map).astype(complex))
    tau = float(frac) * float(ops.as_device(tr.forward(ops.as_device(tr.inverse(X[None])))).abs().max())
    hyp = hypothesis_test(forwardop, regulariser, params, x_map, superpixel_regions(L, size), tau=tau)
    np.save(f"{base}_hyp_physical.npy", hyp.to_map(hyp.physical))
    np.save(f"{base}_hyp_removable.npy", hyp.to_map(hyp.removable))
    print(f"hypothesis tests: {int(hyp.physical.sum())} of {hyp.physical.size} superpixels of {size} x {size} samples hold "
          f"structure that is physical at the level {hyp.threshold:.6e} (tau = {tau:.3e}; the others: inconclusive); "
          f"maps in {base}_hyp_physical.npy / _removable.npy")
    return hyp


def estimate_mu(forwardop, regulariser, params, delta_myula, args, start_point):
    """--estimate-mu: SAPG (a MYULA chain whose threshold scale theta moves towards the marginal maximum-likelihood value,
    DESIGN.md section 17) on the sampler's own operators first; returns the prior and the parameters with T and mu scaled by
    theta_hat.  The chain takes MYULA's step whatever --algo is."""
    p = copy.copy(params)
    p.delta = float(delta_myula)
    sapg = SAPG(forwardop, regulariser, p, nchains=args.chains, warmup=args.sapg_warmup, niter=args.sapg_iters,
                burn=args.sapg_iters // 3, groups="scale" if args.estimate_mu_per_scale else None)
    theta_hat = sapg.run(start_point=start_point)
    if args.estimate_mu_per_scale:
        print(f"SAPG per scale ({args.sapg_warmup} + {args.sapg_iters} iterations, graph replay: {sapg.used_graph}), mu given: {params.mu}")
        print_theta_per_scale(sapg, forwardop.transform)
    else:
        print(f"SAPG ({args.sapg_warmup} + {args.sapg_iters} iterations, graph replay: {sapg.used_graph}): theta_hat = "
              f"{np.round(theta_hat, 6)}, mu_hat = {np.round(sapg.mu_hat, 6)} (mu given: {params.mu})")
    return sapg.apply(regulariser, params)


def print_theta_per_scale(sapg, transform):
    """--estimate-mu-per-scale: one line per block [scaling | j = J_min ... J_max] with its bandlimit, its size and the chain
    mean of theta_hat (what SAPG.apply scales the block's thresholds by)"""
    bls = _multires_bandlimits(transform.L, transform.B, transform.J_min)
    names = ["scaling"] + [f"j = {j}" for j in range(transform.J_min, transform.J_max + 1)]
    hat = np.asarray(sapg.theta_hat).reshape(-1, len(names)).mean(axis=0)
    for name, bl, size, th in zip(names, bls, np.diff(sapg.group_bounds), hat):
        print(f"  {name:>8}: bandlimit {int(bl):4d}, {int(size):8d} coefficients, theta_hat = {th:.6g}")


def lasso_gibbs(forwardop, regulariser, params, args, L_g, truth):
    """--lasso-gibbs NSWEEPS: exact draws of the L1 posterior itself by the Gibbs sampler on the batched CG solver (no step size,
    no Moreau-Yosida envelope): a quarter of the sweeps are burn-in, the rest fold into a PosteriorSummary of the images"""
    nsweeps = args.lasso_gibbs
    nburn = nsweeps // 4
    las = LassoGibbs(forwardop, regulariser, params, nchains=args.chains, tol=1e-6, max_iter=2000)
    start_point = None
    if args.map_start:
        start_point = map_start(forwardop, regulariser, params, L_g, np.zeros(forwardop.nparams, dtype=complex),
                                restart="gradient" if args.map_restart else None)
    start = datetime.now()
    summ = las.run(nsweeps, nburn=nburn, start_point=start_point, summary="image", summary_ess=args.summary_ess,
                   summary_alpha=args.summary_alpha)
    elapsed = datetime.now() - start
    base = os.path.join(args.outdir, f"lassogibbs_{args.setting}_{args.jobid}")
    mean, std = summ.pooled_mean().cpu().numpy().real, np.sqrt(summ.pooled_variance().cpu().numpy())
    np.save(base + "_mean.npy", mean)
    np.save(base + "_std.npy", std)
    its = las.solve_iterations.max(axis=1)
    print(f"LassoGibbs: {nsweeps} sweeps ({nburn} burn-in) x {args.chains} chain(s) in {elapsed}; CG iterations per sweep: median "
          f"{int(np.median(its))}, range {int(its.min())}-{int(its.max())} (all converged: {bool(las.solve_converged.all())}); "
          f"clamped precisions per sweep and chain: {las.clamped_chain.mean():.1f}")
    if args.chains > 1:
        rmax, nundef = summ.max_rhat()
        print(f"max R-hat over the image ({args.chains} chains): {rmax:.4f} ({nundef} components undefined)")
    if args.summary_ess is not None:
        print(summ.ess_report("image"))
    rel = np.sqrt(np.mean(np.abs(mean - truth) ** 2)) / np.sqrt(np.mean(np.abs(truth) ** 2))
    print(f"saved {base}_mean.npy / _std.npy; posterior-mean error {rel:.3f} (noise {args.sigma:.3f}); median posterior std "
          f"{np.median(std):.3f}; mean prior term {las.prior_term_chain.mean():.6e}")
    return base, rel, std


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=32, help="Angular bandlimit. Default 32.")
    ap.add_argument("--algo", type=str, default="myula", help="'myula', 'pxmala' or 'skrock'")
    ap.add_argument("--s", type=int, default=5, help="SKROCK: number of Chebyshev stages (gradient evaluations per iteration)")
    ap.add_argument("--setting", type=str, default="synthesis")
    ap.add_argument("--sigma", type=float, default=0.05, help="Noise level added to the data.")
    ap.add_argument("--mu", type=float, default=1.0)
    ap.add_argument("--nsamples", type=int, default=50)
    ap.add_argument("--ngap", type=int, default=100)
    ap.add_argument("--nburn", type=int, default=0)
    ap.add_argument("--chains", type=int, default=1, help="independent chains batched on the GPU")
    ap.add_argument("--dirs", type=int, default=1, help="wavelet directions N (1: axisymmetric; > 1: directional)")
    ap.add_argument("--spin", type=int, default=0, help="spin S of the field (S != 0: a complex spin-S field, dirs = 1)")
    ap.add_argument("--map-start", action="store_true", help="start the chain(s) at the MAP point found by FISTA first")
    ap.add_argument("--map-restart", action="store_true",
                    help="with --map-start: FISTA with adaptive (gradient) restart, decided per chain on the device")
    ap.add_argument("--analysis-map", action="store_true",
                    help="only find the MAP image of the analysis-setting posterior by primal-dual splitting (spin 0, dirs 1) "
                         "and write it; no chain is run")
    ap.add_argument("--analysis-balance", type=float, default=1.0, metavar="R",
                    help="with --analysis-map: the ratio sigma ||A||^2 / (L_g / 2) of the two steps (PrimalDual's balance)")
    ap.add_argument("--tv-map", action="store_true",
                    help="only find the MAP image under the total-variation prior TV_S2 by primal-dual splitting (spin 0) and "
                         "write it; no chain is run")
    ap.add_argument("--tv", action="store_true", help="sample the image under the total-variation prior TV_S2 (spin 0)")
    ap.add_argument("--tv-strength", type=float, default=1.0, metavar="T",
                    help="with --tv-map / --tv: the TV threshold per unit of lmda * mu")
    ap.add_argument("--local-ci", type=int, default=None, metavar="SIZE",
                    help="with --map-start: local credible intervals of the MAP point on superpixels of SIZE x SIZE samples")
    ap.add_argument("--hyp-test", type=int, default=None, metavar="SIZE",
                    help="with --map-start: hypothesis tests of structure (is it physical, or can it be removed inside the "
                         "credible region?) on superpixels of SIZE x SIZE samples, by segment inpainting")
    ap.add_argument("--hyp-tau-frac", type=float, default=0.1, metavar="F",
                    help="with --hyp-test: the inpainting threshold tau = F max |A x*| (the default 0.1 is a choice, not a "
                         "measured optimum)")
    ap.add_argument("--estimate-mu", action="store_true",
                    help="estimate the regularisation strength by SAPG first and sample with mu_hat = mu * theta_hat")
    ap.add_argument("--estimate-mu-per-scale", action="store_true",
                    help="--estimate-mu with one theta per wavelet scale (SAPG groups='scale'): prints theta_hat per scale and "
                         "samples with every scale's thresholds and weights scaled by its own theta_hat")
    ap.add_argument("--sapg-warmup", type=int, default=100, help="--estimate-mu: MYULA iterations before theta moves")
    ap.add_argument("--sapg-iters", type=int, default=600, help="--estimate-mu: iterations with a moving theta")
    ap.add_argument("--lasso-gibbs", type=int, default=None, metavar="NSWEEPS",
                    help="sample the L1 posterior exactly with the Gibbs sampler on the batched CG solver instead of --algo: NSWEEPS "
                         "sweeps, a quarter of them burn-in, folded into the image summary (synthesis setting, spin 0, dirs 1; "
                         "honours --chains, --map-start, --summary-ess and --summary-alpha; --summary is implied)")
    ap.add_argument("--summary", nargs="?", const="image", default=None, choices=("image",),
                    help="accumulate the posterior mean / standard deviation / R-hat on the GPU instead of saving the chain")
    ap.add_argument("--summary-alpha", type=float, default=None,
                    help="with --summary: also keep the per-pixel tails that give the (1 - alpha) credible-interval map exactly")
    ap.add_argument("--summary-ess", type=int, default=None, metavar="K",
                    help="with --summary: also accumulate the autocovariances at lags below K (even, 2..64) and print the "
                         "effective sample size and the standard error of the mean map")
    ap.add_argument("--outdir", type=str, default=".")
    ap.add_argument("--jobid", type=str, default="0")
    args = ap.parse_args(argv)
    args.estimate_mu = args.estimate_mu or args.estimate_mu_per_scale
    if args.lasso_gibbs is not None:
        if args.lasso_gibbs < 4 or args.setting != "synthesis" or args.spin != 0 or args.dirs != 1 or args.estimate_mu:
            ap.error("--lasso-gibbs takes at least 4 sweeps, the synthesis setting, spin 0 and dirs 1, and not --estimate-mu")
        args.summary = "image"
    if args.summary_alpha is not None and not args.summary:
        ap.error("--summary-alpha needs --summary")
    if args.summary_ess is not None and not args.summary:
        ap.error("--summary-ess needs --summary")
    if args.map_restart and not args.map_start:
        ap.error("--map-restart needs --map-start")
    if args.local_ci is not None and not args.map_start:
        ap.error("--local-ci needs --map-start")
    if args.hyp_test is not None and not args.map_start:
        ap.error("--hyp-test needs --map-start")

    L, B, J_min, setting = args.L, 1.5, 2, args.setting  # B, J_min as in main.py:72-74

    # synthetic "topography": a band-limited real field with a red spectrum, sampled on the MW grid
    rng = np.random.default_rng(0)
    flm = np.zeros(L * L, dtype=complex)
    spin = args.spin
    if spin == 0:
        for el in range(L):
            m = np.arange(1, el + 1)
            flm[el * el + el] = rng.normal() / (1 + el)
            v = (rng.normal(size=el) + 1j * rng.normal(size=el)) / (np.sqrt(2) * (1 + el))
            flm[el * el + el + m] = v
            flm[el * el + el - m] = (-1.0) ** m * np.conj(v)
        truth = ops.ShtPlan(L, 0).inverse(flm).cpu().numpy().real
    else:  # a spin-S field (shear, polarisation Q + iU) is complex: no l < |S| harmonics, no reality symmetry
        for el in range(abs(spin), L):
            flm[el * el : (el + 1) ** 2] = (rng.normal(size=2 * el + 1) + 1j * rng.normal(size=2 * el + 1)) / (np.sqrt(2) * (1 + el))
        truth = ops.ShtPlan(L, spin).inverse(flm).cpu().numpy()
    truth /= np.sqrt(np.mean(np.abs(truth) ** 2))
    if spin == 0:
        data = truth + args.sigma * rng.normal(size=truth.size)
    else:
        data = truth + args.sigma * (rng.normal(size=truth.size) + 1j * rng.normal(size=truth.size)) / np.sqrt(2)

    if args.analysis_map:
        if spin != 0 or args.dirs != 1:
            ap.error("--analysis-map takes spin 0 and dirs 1")
        return analysis_map(data, args, L, B, J_min, truth)

    if args.tv_map or args.tv:
        if spin != 0:
            ap.error("--tv-map and --tv take spin 0")
        return (tv_map if args.tv_map else tv_sample)(data, args, L, truth)

    forwardop = SphericalWaveletTransformOperator(data, args.sigma, setting, L, B, J_min, dirs=args.dirs, spin=spin,
                                                 max_chains=args.chains)
    lmda = 1e-6
    # step size inside the MYULA bound 1 / (L_g + 1 / lmda), L_g = ||S||^2 / sigma^2 (power iteration on the operator)
    L_g = forwardop.gradient_lipschitz(iters=50, tol=1e-3)  # (at most 50 operator pairs at start-up)
    delta = delta_myula = 0.8 / (L_g + 1 / lmda)
    print(f"L_g = {L_g:.6e}: MYULA step bound 1 / (L_g + 1 / lmda) = {1 / (L_g + 1 / lmda):.6e}, delta = {delta:.6e}")
    if args.algo == "skrock":  # SKROCK is stable up to (2 - 4 eta / 3) s^2 / L: the same margin, s^2 times the step
        delta *= args.s ** 2

    params = PxMCMCParams(nsamples=args.nsamples, nburn=args.nburn, ngap=args.ngap, delta=delta, lmda=lmda, mu=args.mu,
                          s=args.s, complex=spin != 0, verbosity=max(1, args.ngap * 10))
    if args.summary:  # no saved chain: every sample goes into the device-resident summary of the images instead
        params.track = [t for t in params.track if t != "chain"]
    regulariser = S2_Wavelets_L1(setting, forwardop.transform.inverse, forwardop.transform.inverse_adjoint,
                                 params.lmda * params.mu, L=L, B=B, J_min=J_min, dirs=args.dirs, spin=spin)
    print(f"Number of data points: {len(data)}")
    print(f"Number of model parameters: {forwardop.nparams}")
    if args.lasso_gibbs is not None:
        return lasso_gibbs(forwardop, regulariser, params, args, L_g, truth)
    cls = {"myula": MYULA, "pxmala": PxMALA, "skrock": SKROCK}[args.algo]
    start_point = np.zeros(forwardop.nparams)
    if args.estimate_mu:
        regulariser, params = estimate_mu(forwardop, regulariser, params, delta_myula, args,
                                          start_point.astype(complex) if spin else start_point)
    mcmc = cls(forwardop, regulariser, params, nchains=args.chains, summary=args.summary, summary_alpha=args.summary_alpha,
               summary_ess=args.summary_ess)
    if args.map_start:
        start_point = map_start(forwardop, regulariser, params, L_g, start_point.astype(complex) if spin else start_point,
                                restart="gradient" if args.map_restart else None)
        if args.local_ci is not None:
            local_ci_maps(forwardop, regulariser, params, start_point, L, args.local_ci,
                          os.path.join(args.outdir, f"{args.algo}_{setting}_{args.jobid}"))
        if args.hyp_test is not None:
            hyp_test_maps(forwardop, regulariser, params, start_point, L, args.hyp_test, args.hyp_tau_frac,
                          os.path.join(args.outdir, f"{args.algo}_{setting}_{args.jobid}"))
    start = datetime.now()
    mcmc.run(start_point=start_point)
    elapsed = datetime.now() - start

    path = save_mcmc(mcmc, params, args.outdir, filename=f"{args.algo}_{setting}_{args.jobid}", L=L, B=B, J_min=J_min,
                     sigma=args.sigma, nparams=forwardop.nparams, setting=setting, time=str(elapsed), chains=args.chains,
                     **({"spin": spin} if spin else {}))
    base = os.path.join(args.outdir, f"{args.algo}_{setting}_{args.jobid}")
    if args.summary:
        summ = mcmc.summary["image"]
        mean, std = summ.pooled_mean().cpu().numpy(), np.sqrt(summ.pooled_variance().cpu().numpy())
        if spin == 0:
            mean = mean.real
        np.save(base + "_mean.npy", mean)
        np.save(base + "_std.npy", std)
        if args.chains > 1:
            rmax, nundef = summ.max_rhat()
            print(f"max R-hat over the image ({args.chains} chains): {rmax:.4f} ({nundef} components undefined)")
        if args.summary_ess is not None:
            print(summ.ess_report("image"))
        rel = np.sqrt(np.mean(np.abs(mean - truth) ** 2)) / np.sqrt(np.mean(np.abs(truth) ** 2))
        print(f"saved {path} and {base}_mean.npy / _std.npy; {mcmc.niter} iterations x {args.chains} chain(s) in {elapsed}; "
              f"posterior-mean error {rel:.3f} (noise {args.sigma:.3f}); median posterior std {np.median(std):.3f}")
        if args.summary_alpha is None:
            return path, rel, std  # (no chain and no tails, so no quantile map: the third item is the posterior standard deviation)
        # the map the chain route below writes (chain 0, real part), from the tails the summary kept instead of a chain
        ci = summ.credible_interval_range()[0].cpu().numpy().real
        np.save(base + "_ci.npy", ci)
        print(f"{base}_ci.npy: median {100 * (1 - args.summary_alpha):g}% CI width {np.median(ci):.3f} "
              f"({summ.tail_bytes() / 2 ** 20:.1f} MiB of tails)")
        return path, rel, ci
    chain = mcmc.chain if args.chains == 1 else mcmc.chain[0]
    images = chain_to_images(chain, forwardop.transform)  # every saved sample mapped to the sphere
    if spin == 0:
        images = images.real
    ci = credible_interval_range(images.real)  # (spin S: of the real part, e.g. Q of Q + iU)
    np.save(base + "_ci.npy", ci)
    mean = images.mean(axis=0)
    rel = np.sqrt(np.mean(np.abs(mean - truth) ** 2)) / np.sqrt(np.mean(np.abs(truth) ** 2))
    print(f"saved {path}; {mcmc.niter} iterations x {args.chains} chain(s) in {elapsed}; "
          f"posterior-mean error {rel:.3f} (noise {args.sigma:.3f}); median 95% CI width {np.median(ci):.3f}")
    return path, rel, ci


if __name__ == "__main__":
    main()
