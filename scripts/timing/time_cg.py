"""The Gaussian posterior's CG iteration at L = 256 with 16 chains: harmonic state (N = L^2), the
weak-lensing measurement and a 1 / C_l prior.

  python scripts/timing/time_cg.py [--out FILE] [--L L] [--chains C]

Reports, as the median of 5 device-synchronised regions (and their spread):
  * pxm_cg_apply and pxm_cg_update alone, with their algorithmic bytes and the fraction of 8 TB/s;
  * pxm_fista_step at the same n and C in the same session, the yardstick for a stream-plus-sums kernel;
  * one replayed iteration of the solver against the sum of its launches (operator pair + the two CG launches);
  * the same iteration composed from existing ops calls plus torch reductions with a host read of alpha and beta.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pxmcmc_amd import ops  # noqa: E402
from pxmcmc_amd.forward import ForwardOperator  # noqa: E402
from pxmcmc_amd.mcmc import PxMCMCParams  # noqa: E402
from pxmcmc_amd.measurements import WeakLensing  # noqa: E402
from pxmcmc_amd.optim import GaussianPosterior  # noqa: E402
from pxmcmc_amd.prior import Gaussian  # noqa: E402
from pxmcmc_amd.transforms import SphericalHarmonicTransform  # noqa: E402
from pxmcmc_amd.utils import build_mask  # noqa: E402

PEAK = 8e12  # HBM3E peak of the MI355X, bytes/s


def region_us(fn, reps=50, regions=5):
    """device time of one call: median over `regions` regions of `reps` back-to-back calls between two events"""
    for _ in range(5):
        fn()
    times = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / reps * 1e3)
    med = statistics.median(times)
    return med, (max(times) - min(times)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--chains", type=int, default=16)
    args = ap.parse_args()
    L, C = args.L, args.chains
    n = L * L
    rng = np.random.default_rng(0)
    mask = build_mask(L, size=10.0)
    wl = WeakLensing(L, mask, ngal=np.full_like(mask, 30), max_chains=C)
    tr = SphericalHarmonicTransform(L, max_chains=C)
    data = (rng.normal(size=wl.ndata) + 1j * rng.normal(size=wl.ndata)) * 0.05
    op = ForwardOperator(data, 1 / wl.inv_cov, "synthesis", transform=tr, measurement=wl, nparams=n)
    params = PxMCMCParams(lmda=1.0, delta=1e-3, mu=1.0, nsamples=1, nburn=0, ngap=1, complex=True, verbosity=0)
    prior = Gaussian.from_power_spectrum(1e-3 * (1.0 + np.arange(L)) ** -1.5, L, 1.0)
    post = GaussianPosterior(op, prior, params, nchains=C, tol=0.0, max_iter=40, check_every=40)
    res = {"L": L, "chains": C, "n": n}

    dev = ops.device()
    z = lambda: ops.randn(n, C, complex_=True, seed=1, it=int(rng.integers(1 << 30)), noise64=True)  # noqa: E731
    U, Q, R, W, P, S, X, X1 = (z() for _ in range(8))
    coef = ops.cg_coef(torch.ones(C, dtype=torch.float64, device=dev))
    coef[:, 0], coef[:, 1], coef[:, 2], coef[:, 3], coef[:, 7] = 1e-3, 0.5, 1.0, 1e-3, 1.0
    keep = coef.clone()
    scratch = ops.cg_scratch(C, dev)
    D, b0, minv = post._D, post._b0, post._minv

    def apply_():
        coef.copy_(keep)
        ops.cg_apply(U, Q, b0, D, R, coef, 0.0, out=W, scratch=scratch)

    t_copy, _ = region_us(lambda: coef.copy_(keep))
    t_apply, s_apply = region_us(apply_)
    t_apply -= t_copy
    t_update, s_update = region_us(lambda: ops.cg_update(U, W, P, S, X, R, minv, keep, out=X1))
    bytes_apply = C * n * 64 + n * 24
    bytes_update = C * n * 176 + n * 8
    res["cg_apply_us"], res["cg_apply_spread"] = t_apply, s_apply
    res["cg_apply_bytes"], res["cg_apply_frac_peak"] = bytes_apply, bytes_apply / (t_apply * 1e-6) / PEAK
    res["cg_update_us"], res["cg_update_spread"] = t_update, s_update
    res["cg_update_bytes"], res["cg_update_frac_peak"] = bytes_update, bytes_update / (t_update * 1e-6) / PEAK

    # the yardstick: pxm_fista_step (Y, G, X0 in; X1, Y1 out; three sums) at the same n and C
    beta = ops.as_device(np.full(8, 0.5), torch.float64)
    fs, fscr = torch.empty((C, 3), dtype=torch.float64, device=dev), ops.fista_scratch(C, dev)
    t_fista, s_fista = region_us(lambda: ops.fista_step(U, Q, X, 1e-3, 1.0, beta, T=1e-3, out=(X1, W), sums=fs, scratch=fscr))
    bytes_fista = C * n * 80
    res["fista_step_us"], res["fista_step_spread"] = t_fista, s_fista
    res["fista_step_frac_peak"] = bytes_fista / (t_fista * 1e-6) / PEAK
    res["cg_apply_rate_vs_fista"] = res["cg_apply_frac_peak"] / res["fista_step_frac_peak"]
    res["cg_update_rate_vs_fista"] = res["cg_update_frac_peak"] / res["fista_step_frac_peak"]

    # the operator pair alone, then one replayed iteration of the solver
    t_pair, s_pair = region_us(lambda: post._linear(U), reps=10)
    res["operator_pair_us"], res["operator_pair_spread"] = t_pair, s_pair
    post._engine_start(torch.zeros((C, n), dtype=torch.complex128, device=dev))
    post._load(ops.cg_rhs(U, B=b0))
    res["used_graph"] = post._eng.graph is not None
    t_iter, s_iter = region_us(lambda: post._engine_advance(8), reps=5)
    post._engine_stop()
    res["replayed_iteration_us"], res["replayed_iteration_spread"] = t_iter / 8, s_iter
    res["sum_of_launches_us"] = t_pair + t_apply + t_update

    # the same iteration from existing ops calls + torch reductions, alpha and beta read by the host
    def composed():
        q = post._linear(U)
        w = ops.cg_rhs(U, B=b0, G=q, Z=U, S=D)
        gam = float(torch.sum((R.conj() * U).real))
        dlt = float(torch.sum((U.conj() * w).real))
        alpha, beta_ = gam / dlt, 0.5
        ops.skrock_stage(U, 1.0, e=beta_, V=P, out=X1)
        ops.skrock_stage(w, 1.0, e=beta_, V=S, out=W)
        ops.skrock_stage(X, 1.0, e=alpha, V=X1, out=Q)
        ops.skrock_stage(R, 1.0, e=-alpha, V=W, out=Q)
        ops.cg_rhs(U, Z=Q, S=minv, out=X1)

    t_comp, s_comp = region_us(composed, reps=10)
    res["composed_iteration_us"], res["composed_iteration_spread"] = t_comp, s_comp
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
