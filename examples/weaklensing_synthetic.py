#!/usr/bin/env python
"""
Weak-lensing mass mapping through the drop-in API, following the reference's
experiments/weaklensing/main.py:85-147 (BASELINE.json configs[4]) on a synthetic convergence field (the reference
reads a HEALPix kappa map with healpy, absent here):

    synthetic kappa (SURVEY.md section 8d, C5 spectrum)
      -> prepare_gammas = the load_gammas preparation of main.py:23-39 without healpy: band-limit, 50-arcmin
         Gaussian beam (applied in harmonic space: b_l = exp(-l(l+1) sigma^2 / 2), what hp.smoothing does), MW map by the
         inverse SHT, shear through WeakLensing.forward
      -> build_mask(L, size) (Euclid-like: ecliptic band + galactic plane, pxmcmc/utils.py:320-349), ngal = 30
      -> ForwardOperator(gammas, 1 / inv_cov, setting, SphericalWaveletTransform, WeakLensing)
      -> S2_Wavelets_L1 -> MYULA / PxMALA(tune_delta=True) / SKROCK -> save_mcmc.
With --harmonic the posterior lives in harmonic space: the data are the shear harmonics of the smoothed field (full sky,
no mask), the operator is WeakLensingHarmonic with SphericalWaveletTransform(harmonic=True), the prior L1, and the chain
starts from the wavelet analysis of the Kaiser-Squires estimate (WeakLensingHarmonic.sks_estimate).
With --healpix NSIDE the shear is read at the pixel centres of a HEALPix map in RING order, as a catalogue binned with healpy
is: the data are WeakLensingHealpix.forward of the smoothed field (an exact synthesis at the pixel centres, no map2alm), the
mask is |galactic latitude| < --mask-size computed from the pixel centres, and the samplers run on WeakLensingHealpix with
S2_Wavelets_L1 (every --algo; the generic stepping engine).

    python examples/weaklensing_synthetic.py --L 64 --algo pxmala --nsamples 20 --ngap 20 --nburn 100 --outdir /tmp
"""
import argparse
import copy
import os
import sys
import time
from datetime import datetime

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pxmcmc_amd import ops  # noqa: E402
from pxmcmc_amd.forward import ForwardOperator  # noqa: E402
from pxmcmc_amd.mcmc import MYULA, SKROCK, PxMALA, PxMCMCParams  # noqa: E402
from pxmcmc_amd.measurements import WeakLensing, WeakLensingHarmonic, WeakLensingHealpix  # noqa: E402
from pxmcmc_amd.optim import FISTA  # noqa: E402
from pxmcmc_amd.prior import L1, S2_Wavelets_L1  # noqa: E402
from pxmcmc_amd.sapg import SAPG  # noqa: E402
from pxmcmc_amd.saving import save_mcmc  # noqa: E402
from pxmcmc_amd.transforms import SphericalWaveletTransform  # noqa: E402
from pxmcmc_amd.uncertainty import hypothesis_test, local_credible_intervals, superpixel_regions  # noqa: E402
from pxmcmc_amd.utils import _multires_bandlimits, build_mask, galactic_latitude, healpix_pixel_centres  # noqa: E402

BEAM_SIGMA = np.radians(50 / 60)  # 50 arcmin (experiments/weaklensing/main.py:35)


def synthetic_kappa_lm(L, seed=3):
    """harmonic coefficients of a real Gaussian convergence field, C_l ~ (1 + l)^-1.5 exp(-(l / 200)^2), no monopole /
    dipole (klm[:4] = 0: the weak-lensing kernel annihilates them, pxmcmc/measurements.py:166-170)"""
    rng = np.random.default_rng(seed)
    klm = np.zeros(L * L, dtype=complex)
    for el in range(2, L):
        amp = np.sqrt((1.0 + el) ** -1.5 * np.exp(-((el / 200.0) ** 2)))
        klm[el * el + el] = amp * rng.normal()
        m = np.arange(1, el + 1)
        v = amp * (rng.normal(size=el) + 1j * rng.normal(size=el)) / np.sqrt(2)
        klm[el * el + el + m] = v
        klm[el * el + el - m] = (-1.0) ** m * np.conj(v)
    return klm


def beam(L, sigma=BEAM_SIGMA):
    """Gaussian beam window b_l = exp(-l (l + 1) sigma^2 / 2) repeated over m (what healpy.smoothing(sigma=...) applies)"""
    el = np.repeat(np.arange(L), 2 * np.arange(L) + 1)
    return np.exp(-0.5 * el * (el + 1.0) * sigma ** 2)


def prepare_gammas(klm, L, wl, sigma=BEAM_SIGMA):
    """experiments/weaklensing/main.py:23-39 from harmonic coefficients: smooth, map to the MW grid, shear.
    Returns (gamma data vector in the masked data space, smoothed kappa on the MW grid)."""
    kappa_mw = ops.ShtPlan(L, 0).inverse(klm * beam(L, sigma)).cpu().numpy()
    return wl.forward(kappa_mw), kappa_mw.reshape(L, 2 * L - 1)


def step_hint(forward_operator, params, args):
    """print MYULA's step bound 1 / (L_g + 1 / lmda) beside --delta (SKROCK: s^2 times it); returns L_g"""
    L_g = forward_operator.gradient_lipschitz(iters=50, tol=1e-3)  # (at most 50 operator pairs at start-up)
    bound = 1 / (L_g + 1 / params.lmda)
    print(f"L_g = {L_g:.6e}: step bound 1 / (L_g + 1 / lmda) = {bound:.6e} (--delta {args.delta:.6e}"
          + (f", SKROCK with s = {args.s}: {bound * args.s ** 2:.6e})" if args.algo == "skrock" else ")"))
    return L_g


def map_start(forward_operator, prior, params, L_g, start_point=None, tol=1e-3, max_iter=2000, restart=None):
    """FISTA on the samplers' posterior as the chain's start point.  The shear data are complex with a real sig_d, so the
    inverse covariance is complex (pxmcmc/forward.py:81-82) and FISTA takes its gradient on the operator with Re(invcov),
    for which 1 / L_g of the full operator is a valid (smaller) step.  The steps of FISTA shrink like 1 / k, so the run is
    bounded: at most ``max_iter`` operator pairs, stopping at a relative step of ``tol`` (a start point, not a final
    estimate; ``restart="gradient"``, --map-restart, removes that tail)."""
    fista = FISTA(forward_operator, prior, params, gamma=1 / (L_g * (1 + 1e-3)), tol=tol, max_iter=max_iter, restart=restart)
    x = fista.run(start_point=start_point)
    its = f"{int(fista.niter[0])} iterations" + (f", {int(fista.nrestarts[0])} restarts" if restart else "")
    if fista._stock_prox:
        print(f"MAP start: FISTA stopped after {its} (converged: {bool(fista.converged[0])}), "
              f"objective {fista.objective_map[0]:.6e}")
    else:  # the prior's own prox carries its own threshold: the fixed point of that iteration, not the posterior's MAP
        print(f"start point: fixed point of the prior's own prox-gradient iteration (g + (lmda / gamma) f, not the MAP) after "
              f"{its} (converged: {bool(fista.converged[0])})")
    return x


def local_ci_maps(forward_operator, prior, params, x_map, L, size, base):
    """--local-ci SIZE: the local credible intervals of the MAP convergence on superpixels of SIZE x SIZE samples (DESIGN.md
    section 14b), at the approximate 95 % HPD level; writes the lower / upper / range maps"""
    lci = local_credible_intervals(forward_operator, prior, params, x_map, superpixel_regions(L, size))
    ok = lci.status == 0
    for name in ("lower", "upper", "range"):
        np.save(f"{base}_lci_{name}.npy", lci.to_map(getattr(lci, name)))
    print(f"local credible intervals: {ok.sum()} of {ok.size} superpixels of {size} x {size} samples have an interval at the "
          f"level {lci.threshold:.6e}; median range {np.median(lci.range[ok]) if ok.any() else float('nan'):.4f}; "
          f"maps in {base}_lci_lower.npy / _upper.npy / _range.npy")
    return lci


def hyp_test_maps(forward_operator, prior, params, x_map, L, size, frac, base):
    """--hyp-test SIZE: the hypothesis test of structure of every superpixel of SIZE x SIZE samples
    at the approximate 95 % HPD level, with the inpainting threshold tau = frac max |A x*|; writes the physical (1 / 0) and
    removable maps beside those of the local credible intervals"""
    tr = forward_operator.transform
    X = ops.as_device(np.asarray(x_map).astype(complex))
    tau = float(frac) * float(ops.as_device(tr.forward(ops.as_device(tr.inverse(X[None])))).abs().max())
    hyp = hypothesis_test(forward_operator, prior, params, x_map, superpixel_regions(L, size), tau=tau)
    np.save(f"{base}_hyp_physical.npy", hyp.to_map(hyp.physical))
    np.save(f"{base}_hyp_removable.npy", hyp.to_map(hyp.removable))
    print(f"hypothesis tests: {int(hyp.physical.sum())} of {hyp.physical.size} superpixels of {size} x {size} samples hold "
          f"structure that is physical at the level {hyp.threshold:.6e} (tau = {tau:.3e}; the others: inconclusive); "
          f"maps in {base}_hyp_physical.npy / _removable.npy")
    return hyp


def estimate_mu(forward_operator, prior, params, L_g, args, start_point=None):
    """--estimate-mu: SAPG (a MYULA chain whose threshold scale theta moves towards the marginal maximum-likelihood value,
    DESIGN.md section 17) on the sampler's own operators first; returns the prior and the parameters with T and mu scaled by
    theta_hat.  The chain takes --delta, or 0.8 of MYULA's bound when that is smaller."""
    p = copy.copy(params)
    p.delta = float(min(params.delta, 0.8 / (L_g + 1 / params.lmda)))
    sapg = SAPG(forward_operator, prior, p, nchains=args.chains, warmup=args.sapg_warmup, niter=args.sapg_iters,
                burn=args.sapg_iters // 3, seed=args.seed, groups="scale" if args.estimate_mu_per_scale else None)
    theta_hat = sapg.run(start_point=start_point)
    if args.estimate_mu_per_scale:
        print(f"SAPG per scale ({args.sapg_warmup} + {args.sapg_iters} iterations at delta = {p.delta:.3e}, graph replay: "
              f"{sapg.used_graph}), mu given: {params.mu}")
        print_theta_per_scale(sapg, forward_operator.transform)
    else:
        print(f"SAPG ({args.sapg_warmup} + {args.sapg_iters} iterations at delta = {p.delta:.3e}, graph replay: {sapg.used_graph}): "
              f"theta_hat = {np.round(theta_hat, 6)}, mu_hat = {np.round(sapg.mu_hat, 6)} (mu given: {params.mu})")
    return sapg.apply(prior, params)


def print_theta_per_scale(sapg, transform):
    """--estimate-mu-per-scale: one line per block [scaling | j = J_min ... J_max] with its bandlimit, its size and the chain
    mean of theta_hat (what SAPG.apply scales the block's thresholds by)"""
    bls = _multires_bandlimits(transform.L, transform.B, transform.J_min)
    names = ["scaling"] + [f"j = {j}" for j in range(transform.J_min, transform.J_max + 1)]
    hat = np.asarray(sapg.theta_hat).reshape(-1, len(names)).mean(axis=0)
    for name, bl, size, th in zip(names, bls, np.diff(sapg.group_bounds), hat):
        print(f"  {name:>8}: bandlimit {int(bl):4d}, {int(size):8d} coefficients, theta_hat = {th:.6g}")


def build_sampler(args, forward_operator, prior, params, space):
    """the sampler of --algo; with --summary the saved samples go into a device-resident summary of ``space`` ("image", or
    "state" for the harmonic posterior, whose transform has no image) and "chain" leaves ``track``"""
    if args.summary:
        params.track = [t for t in params.track if t != "chain"]
    kw = dict(nchains=args.chains, seed=args.seed, summary=space if args.summary else None, summary_alpha=args.summary_alpha,
              summary_ess=args.summary_ess)
    if args.algo == "myula":
        return MYULA(forward_operator, prior, params, **kw)
    if args.algo == "pxmala":
        return PxMALA(forward_operator, prior, params, tune_delta=True, **kw)
    if args.algo == "skrock":
        return SKROCK(forward_operator, prior, params, **kw)
    raise ValueError("algo must be 'myula', 'pxmala' or 'skrock'")


def summary_maps(args, mcmc, space, path):
    """--summary: pooled mean and standard deviation of ``space`` over every chain, written beside the run; max R-hat; with
    --summary-alpha the (1 - alpha) credible-interval map of chain 0 (per real component), from the tails the summary kept"""
    summ = mcmc.summary[space]
    mean, std = summ.pooled_mean().cpu().numpy(), np.sqrt(summ.pooled_variance().cpu().numpy())
    base = os.path.splitext(path)[0]
    np.save(base + "_mean.npy", mean)
    np.save(base + "_std.npy", std)
    if args.chains > 1:
        rmax, nundef = summ.max_rhat()
        print(f"max R-hat over the {space} ({args.chains} chains): {rmax:.4f} ({nundef} components undefined)")
    if args.summary_ess is not None:
        print(summ.ess_report(space))
    print(f"posterior mean and standard deviation of the {space}: {base}_mean.npy, {base}_std.npy")
    if args.summary_alpha is not None:
        ci = summ.credible_interval_range()[0].cpu().numpy()
        np.save(base + "_ci.npy", ci)
        print(f"{100 * (1 - args.summary_alpha):g}% credible-interval map of the {space} (chain 0): {base}_ci.npy")
    return mean


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--outdir", type=str, default=".")
    ap.add_argument("--jobid", type=str, default="0")
    ap.add_argument("--algo", type=str, default="myula", help="'myula', 'pxmala' or 'skrock'")
    ap.add_argument("--s", type=int, default=5, help="SKROCK: number of Chebyshev stages (gradient evaluations per iteration)")
    ap.add_argument("--setting", type=str, default="synthesis")
    ap.add_argument("--delta", type=float, default=1e-6, help="PxMCMC step size. Default 1e-6 (main.py:73)")
    ap.add_argument("--mu", type=float, default=1.0)
    ap.add_argument("--L", type=int, default=512, help="Angular bandlimit. Default 512 (main.py:82).")
    ap.add_argument("--mask-size", type=float, default=10.0, help="width of the two masked bands in degrees (main.py:91)")
    ap.add_argument("--nsamples", type=int, default=10)
    ap.add_argument("--ngap", type=int, default=50)
    ap.add_argument("--nburn", type=int, default=100)
    ap.add_argument("--chains", type=int, default=1, help="independent chains batched on the GPU")
    ap.add_argument("--dirs", type=int, default=1, help="wavelet directions N (1: axisymmetric; > 1: directional)")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--map-start", action="store_true", help="start the chain(s) at the MAP point found by FISTA first")
    ap.add_argument("--map-restart", action="store_true",
                    help="with --map-start: FISTA with adaptive (gradient) restart, decided per chain on the device")
    ap.add_argument("--local-ci", type=int, default=None, metavar="SIZE",
                    help="with --map-start: local credible intervals of the MAP point on superpixels of SIZE x SIZE samples "
                         "(pixel-space posterior only)")
    ap.add_argument("--hyp-test", type=int, default=None, metavar="SIZE",
                    help="with --map-start: hypothesis tests of structure (is it physical, or can it be removed inside the "
                         "credible region?) on superpixels of SIZE x SIZE samples, by segment inpainting (pixel-space posterior only)")
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
    ap.add_argument("--summary", nargs="?", const=True, default=None, choices=("image", "state"),
                    help="accumulate the posterior mean / standard deviation / R-hat on the GPU instead of saving the chain: "
                         "of the image, or with --harmonic of the state (the value may be left out; the other one is an error)")
    ap.add_argument("--summary-alpha", type=float, default=None,
                    help="with --summary: also keep the per-element tails that give the (1 - alpha) credible-interval map exactly")
    ap.add_argument("--summary-ess", type=int, default=None, metavar="K",
                    help="with --summary: also accumulate the autocovariances at lags below K (even, 2..64) and print the "
                         "effective sample size and the standard error of the mean map")
    ap.add_argument("--harmonic", action="store_true",
                    help="harmonic-space posterior: WeakLensingHarmonic + harmonic wavelets + L1, started from sks_estimate")
    ap.add_argument("--healpix", type=int, default=None, metavar="NSIDE",
                    help="read the shear at the pixel centres of a HEALPix map (RING order) of this nside: WeakLensingHealpix")
    ap.add_argument("--wiener", action="store_true",
                    help="Gaussian prior 1 / C_l on kappa_lm: the Wiener map by batched conjugate gradients (optim.GaussianPosterior)")
    ap.add_argument("--wiener-draws", type=int, default=0, metavar="N",
                    help="--wiener: also N exact posterior draws (--chains per solve) and the standard-deviation map of kappa")
    ap.add_argument("--gibbs-cl", type=int, default=0, metavar="NSWEEPS",
                    help="--wiener: also sample the power spectrum C_l jointly with the map by NSWEEPS Gibbs sweeps of --chains chains "
                         "(optim.GaussianGibbs; the first quarter is burn-in) and write its posterior mean and 95 %% band")
    args = ap.parse_args(argv)
    args.estimate_mu = args.estimate_mu or args.estimate_mu_per_scale
    if args.wiener_draws and not args.wiener:
        ap.error("--wiener-draws needs --wiener")
    if args.gibbs_cl and not args.wiener:
        ap.error("--gibbs-cl needs --wiener")
    if args.gibbs_cl and args.gibbs_cl < 4:
        ap.error("--gibbs-cl needs at least 4 sweeps")
    if args.wiener and (args.harmonic or args.healpix is not None or args.map_start or args.estimate_mu or args.summary):
        ap.error("--wiener runs on its own: the MW pixel-space data, no sampler options")
    if args.healpix is not None and (args.harmonic or args.local_ci is not None or args.hyp_test is not None):
        ap.error("--healpix runs the pixel-space posterior without --local-ci / --hyp-test (their regions are MW superpixels of the data grid)")
    if args.summary_alpha is not None and not args.summary:
        ap.error("--summary-alpha needs --summary")
    if args.summary_ess is not None and not args.summary:
        ap.error("--summary-ess needs --summary")
    if args.map_restart and not args.map_start:
        ap.error("--map-restart needs --map-start")
    if args.local_ci is not None and (not args.map_start or args.harmonic):
        ap.error("--local-ci needs --map-start and the pixel-space posterior (no --harmonic)")
    if args.hyp_test is not None and (not args.map_start or args.harmonic):
        ap.error("--hyp-test needs --map-start and the pixel-space posterior (no --harmonic)")
    if args.summary not in (None, True, "state" if args.harmonic else "image"):
        ap.error("--summary %s: the summary is of the %s" % (args.summary, "state with --harmonic" if args.harmonic else "image without --harmonic"))

    L, B, J_min, setting = args.L, 2, 2, args.setting  # main.py:85-88
    if args.harmonic:
        return _main_harmonic(args, L, B, J_min, setting)

    if args.healpix is not None:
        # galactic-plane mask from the pixel centres (lon = phi - 180, lat = 90 - theta degrees), shear at the pixel centres
        theta, phi = healpix_pixel_centres(args.healpix)
        hmask = np.abs(galactic_latitude(np.degrees(phi) - 180, 90 - np.degrees(theta))) >= args.mask_size
        measurement = WeakLensingHealpix(L, args.healpix, mask=hmask, ngal=np.full(hmask.size, 30.0), max_chains=args.chains)
        mask = np.ones((L, 2 * L - 1))  # (the kappa error below is taken on the whole MW grid)
        print(f"HEALPix data: nside = {args.healpix}, {hmask.size} pixels, masked fraction {1 - hmask.mean():.3f}")
    else:
        # Euclid-like mask and synthetic shear data (main.py:90-93)
        mask = build_mask(L, size=args.mask_size)
        measurement = WeakLensing(L, mask, ngal=np.full_like(mask, 30), max_chains=args.chains)
    gammas_truth, kappa_truth = prepare_gammas(synthetic_kappa_lm(L, args.seed), L, measurement)

    if args.wiener:
        return _main_wiener(args, L, measurement, mask, gammas_truth, kappa_truth)
    transform = SphericalWaveletTransform(L, B, J_min, dirs=args.dirs, max_chains=args.chains)
    forward_operator = ForwardOperator(gammas_truth, 1 / measurement.inv_cov, setting, transform=transform,
                                       measurement=measurement, nparams=transform.ncoefs)
    params = PxMCMCParams(nsamples=args.nsamples, nburn=args.nburn, ngap=args.ngap, delta=args.delta, lmda=args.delta / 2,
                          mu=args.mu, s=args.s, complex=False, verbosity=max(1, args.ngap * 10))
    prior = S2_Wavelets_L1(setting, transform.inverse, transform.inverse_adjoint, params.lmda * params.mu, L=L, B=B,
                           J_min=J_min, dirs=args.dirs)
    print(f"Number of data points: {gammas_truth.size}")
    print(f"Number of model parameters: {forward_operator.nparams}")
    L_g = step_hint(forward_operator, params, args)
    if args.healpix is not None and args.delta * L_g > 1:
        print(f"--delta {args.delta:.3e} is above 1 / L_g = {1 / L_g:.3e} for these data (12 nside^2 weighted pixels): MYULA and SKROCK "
              f"diverge there; pass a --delta near the bound above")
    if args.estimate_mu:
        prior, params = estimate_mu(forward_operator, prior, params, L_g, args)
    start_point = map_start(forward_operator, prior, params, L_g, restart="gradient" if args.map_restart else None) if args.map_start else None
    if args.local_ci is not None:
        local_ci_maps(forward_operator, prior, params, start_point, L, args.local_ci,
                      os.path.join(args.outdir, f"{args.algo}_{setting}_{args.jobid}"))
    if args.hyp_test is not None:
        hyp_test_maps(forward_operator, prior, params, start_point, L, args.hyp_test, args.hyp_tau_frac,
                      os.path.join(args.outdir, f"{args.algo}_{setting}_{args.jobid}"))
    mcmc = build_sampler(args, forward_operator, prior, params, "image")

    now = datetime.now()
    t0 = time.perf_counter()
    mcmc.run(start_point=start_point)
    elapsed = time.perf_counter() - t0
    filename = f"{args.algo}_{setting}_{now.strftime('%d%m%y_%H%M%S')}_{args.jobid}"
    path = save_mcmc(mcmc, params, args.outdir, filename=filename, L=L, B=B, J_min=J_min, nparams=forward_operator.nparams,
                     setting=setting, time=str(elapsed), chains=args.chains)

    if args.summary:
        kappa_mean = summary_maps(args, mcmc, "image", path).real.reshape(L, 2 * L - 1)
    else:
        chain = mcmc.chain if args.chains == 1 else mcmc.chain[0]
        kappa_mean = np.asarray(transform.inverse(chain.mean(axis=0))).real.reshape(L, 2 * L - 1)
    seen = mask.astype(bool)
    rel = np.linalg.norm((kappa_mean - kappa_truth.real)[seen]) / np.linalg.norm(kappa_truth.real[seen])
    niter = int(mcmc.niter)
    print(f"saved {path}; {niter} iterations x {args.chains} chain(s) in {elapsed:.2f} s = {elapsed / max(niter, 1) * 1e3:.3f} ms "
          f"per iteration; posterior-mean kappa error on the unmasked sky {rel:.3f}; masked fraction {1 - seen.mean():.3f}")
    return {"path": path, "rel_err": rel, "ms_per_iter": elapsed / max(niter, 1) * 1e3, "mcmc": mcmc,
            "operator": forward_operator, "mask": mask, "gammas": gammas_truth}


def synthetic_cl(L, sigma=BEAM_SIGMA):
    """the power spectrum of the smoothed field of :func:`synthetic_kappa_lm`; the monopole and dipole, which it leaves out and
    the shear does not see, get the quadrupole's power so that the prior pins them near zero with a finite precision"""
    el = np.arange(L, dtype=float)
    cl = (1.0 + el) ** -1.5 * np.exp(-((el / 200.0) ** 2)) * np.exp(-el * (el + 1.0) * sigma ** 2)
    cl[:2] = cl[min(2, L - 1)]
    return cl


def _main_wiener(args, L, measurement, mask, gammas_truth, kappa_truth):
    """--wiener: harmonic state kappa_lm with the 1 / C_l prior of the synthetic spectrum; the Wiener map is the exact
    posterior mean, --wiener-draws N adds the exact standard-deviation map from N independent posterior draws"""
    from pxmcmc_amd.optim import GaussianPosterior
    from pxmcmc_amd.prior import Gaussian
    from pxmcmc_amd.transforms import SphericalHarmonicTransform

    if args.setting != "synthesis":
        raise ValueError("--wiener runs the synthesis setting")
    transform = SphericalHarmonicTransform(L, max_chains=args.chains)
    forward_operator = ForwardOperator(gammas_truth, 1 / measurement.inv_cov, "synthesis", transform=transform,
                                       measurement=measurement, nparams=L * L)
    params = PxMCMCParams(nsamples=args.nsamples, nburn=args.nburn, ngap=args.ngap, delta=args.delta, lmda=args.delta / 2,
                          mu=args.mu, s=args.s, complex=True, verbosity=0)
    # T / lmda = mu: the posterior is 1/2 Re L2 + mu 1/2 sum |kappa_lm|^2 / C_l
    prior = Gaussian.from_power_spectrum(synthetic_cl(L), L, params.lmda * params.mu)
    print(f"Number of data points: {gammas_truth.size}")
    print(f"Number of model parameters: {forward_operator.nparams}")
    step_hint(forward_operator, params, args)
    post = GaussianPosterior(forward_operator, prior, params, nchains=args.chains, seed=args.seed)
    t0 = time.perf_counter()
    klm = post.run()
    elapsed = time.perf_counter() - t0
    klm = klm if args.chains == 1 else klm[0]
    kappa = np.asarray(transform.inverse(klm)).real.reshape(L, 2 * L - 1)
    seen = mask.astype(bool)
    rel = np.linalg.norm((kappa - kappa_truth.real)[seen]) / np.linalg.norm(kappa_truth.real[seen])
    base = os.path.join(args.outdir, f"wiener_{args.jobid}")
    np.save(base + "_kappa.npy", kappa)
    print(f"Wiener filter: {int(post.niter.max())} CG iterations (converged: {bool(post.converged.all())}, relative residual "
          f"{float(post.rel_residual[-1].max()):.2e}, graph replay: {post.used_graph}) in {elapsed:.2f} s; kappa error on the "
          f"unmasked sky {rel:.3f}; saved {base}_kappa.npy")
    out = {"rel_err": rel, "niter": post.niter, "solver": post, "operator": forward_operator, "mask": mask, "kappa": kappa}
    if args.wiener_draws:
        t0 = time.perf_counter()
        summary = post.sample(args.wiener_draws, summary="image")
        elapsed = time.perf_counter() - t0
        std = np.sqrt(summary.pooled_variance().cpu().numpy()).reshape(L, 2 * L - 1)
        np.save(base + "_kappa_std.npy", std)
        print(f"{args.wiener_draws} exact posterior draws in {post.solve_iterations.shape[0]} solves of {args.chains} ("
              f"{int(post.solve_iterations.max())} iterations at most) in {elapsed:.2f} s; standard deviation of kappa: median "
              f"{np.median(std):.3e} seen, {np.median(std[~seen]) if (~seen).any() else float('nan'):.3e} masked; saved {base}_kappa_std.npy")
        out["kappa_std"] = std
    if args.gibbs_cl:
        out.update(_gibbs_cl(args, L, forward_operator, prior, params, base))
    return out


def _gibbs_cl(args, L, forward_operator, prior, params, base):
    """--gibbs-cl NSWEEPS: the joint posterior of kappa_lm and its variances by Gibbs sampling from the synthetic spectrum as
    the start; the monopole and dipole, which the shear does not see, keep their prior variance (lmin = 2).  The posterior of
    DESIGN.md section 23 gives the real and the imaginary part of kappa_lm the variance v_l each, E |kappa_lm|^2 = 2 v_l, so
    the sampled v_l is set next to C_l / 2 of the spectrum the field was drawn from."""
    from pxmcmc_amd.optim import GaussianGibbs

    # (the masked weak-lensing system is badly conditioned: a draw solved to 1e-6 of its right-hand side takes thousands of
    # iterations, and is exact for every purpose of a Monte-Carlo estimate)
    gibbs = GaussianGibbs(forward_operator, prior, params, nchains=args.chains, groups="degree", lmin=2, seed=args.seed, tol=1e-6,
                          max_iter=6000, check_every=50)
    nburn = args.gibbs_cl // 4
    t0 = time.perf_counter()
    gibbs.run(args.gibbs_cl, nburn=nburn, summary="state")
    elapsed = time.perf_counter() - t0
    cl = gibbs.cl_chain.reshape(-1, L)  # (reported in the units of prior.Gaussian: 1 / precision = C_l)
    lo, hi = np.quantile(cl, [0.025, 0.975], axis=0)
    rhat = gibbs.hyper_summary.rhat().cpu().numpy() if args.chains > 1 else np.full(L, np.nan)
    table = np.stack([np.arange(L), synthetic_cl(L) / 2, cl.mean(axis=0), lo, hi, rhat], axis=1)
    np.save(base + "_cl.npy", table)
    inside = float(np.mean((table[2:, 1] >= lo[2:]) & (table[2:, 1] <= hi[2:])))
    print(f"Gibbs C_l: {args.gibbs_cl} sweeps ({nburn} burn-in) of {args.chains} chain(s) in {elapsed:.2f} s, "
          f"{int(gibbs.solve_iterations.max())} CG iterations at most (all converged: {bool(gibbs.solve_converged.all())}); half the spectrum "
          f"of the field lies in the 95 % band at {inside:.0%} of the degrees l >= 2; largest R-hat of log C_l "
          f"{np.nanmax(rhat[2:]) if args.chains > 1 else float('nan'):.3f}; saved {base}_cl.npy (l, C_l / 2 of the field, mean, 2.5 %, 97.5 %, R-hat)")
    return {"cl_table": table, "gibbs": gibbs}


def _main_harmonic(args, L, B, J_min, setting):
    """--harmonic: shear harmonics glm = k_l (b_l kappa_lm) + noise, full sky; start point = analysis(sks_estimate(glm))"""
    if setting != "synthesis":
        raise ValueError("--harmonic runs the synthesis setting")
    measurement = WeakLensingHarmonic(L)
    klm_truth = synthetic_kappa_lm(L, args.seed) * beam(L)
    sig_d = 0.37 / np.sqrt(2 * 30.0)  # shape noise of 30 galaxies per sample, per component
    rng = np.random.default_rng(args.seed + 1)
    glm = measurement.forward(klm_truth) + sig_d * (rng.normal(size=L * L) + 1j * rng.normal(size=L * L))
    glm[:4] = 0
    transform = SphericalWaveletTransform(L, B, J_min, dirs=args.dirs, harmonic=True, max_chains=args.chains)
    forward_operator = ForwardOperator(glm, sig_d, setting, transform=transform, measurement=measurement,
                                       nparams=transform.ncoefs)
    params = PxMCMCParams(nsamples=args.nsamples, nburn=args.nburn, ngap=args.ngap, delta=args.delta, lmda=args.delta / 2,
                          mu=args.mu, s=args.s, complex=True, verbosity=max(1, args.ngap * 10))
    prior = L1(setting, None, None, params.lmda * params.mu)
    X0 = transform.forward(measurement.sks_estimate(glm))
    print(f"harmonic set-up: {L * L} shear harmonics, {forward_operator.nparams} wavelet coefficients")
    L_g = step_hint(forward_operator, params, args)
    if args.estimate_mu:
        prior, params = estimate_mu(forward_operator, prior, params, L_g, args, start_point=X0)
    if args.map_start:
        X0 = map_start(forward_operator, prior, params, L_g, start_point=X0, restart="gradient" if args.map_restart else None)
    mcmc = build_sampler(args, forward_operator, prior, params, "state")
    now = datetime.now()
    t0 = time.perf_counter()
    mcmc.run(start_point=X0)
    elapsed = time.perf_counter() - t0
    filename = f"{args.algo}_harmonic_{setting}_{now.strftime('%d%m%y_%H%M%S')}_{args.jobid}"
    path = save_mcmc(mcmc, params, args.outdir, filename=filename, L=L, B=B, J_min=J_min, nparams=forward_operator.nparams,
                     setting=setting, time=str(elapsed), chains=args.chains)
    if args.summary:
        klm_mean = np.asarray(transform.inverse(summary_maps(args, mcmc, "state", path)))
    else:
        chain = mcmc.chain if args.chains == 1 else mcmc.chain[0]
        klm_mean = np.asarray(transform.inverse(chain.mean(axis=0)))
    rel = np.linalg.norm(klm_mean[4:] - klm_truth[4:]) / np.linalg.norm(klm_truth[4:])
    niter = int(mcmc.niter)
    print(f"saved {path}; {niter} iterations x {args.chains} chain(s) in {elapsed:.2f} s = {elapsed / max(niter, 1) * 1e3:.3f} ms "
          f"per iteration; posterior-mean kappa_lm error {rel:.3f} (harmonic, fused step: {getattr(mcmc, '_fused_harm', False)})")
    return {"path": path, "rel_err": rel, "ms_per_iter": elapsed / max(niter, 1) * 1e3, "mcmc": mcmc,
            "operator": forward_operator, "gammas": glm}


if __name__ == "__main__":
    main()
