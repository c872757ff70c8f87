"""The Gibbs sampler's variance draw and sweep at L = 256 with 16 chains, for degree groups (harmonic
state, weak-lensing measurement, 1 / C_l prior) and for scale groups (wavelet coefficients, identity measurement).

  python scripts/timing/time_gibbs.py [--out FILE] [--L L] [--chains C] [--sweeps S] [--groups degree scale]

Reports per kind of groups, as the median of 5 device-synchronised regions (and their spread):
  * pxm_group_variance_draw (three launches) replayed from a captured graph;
  * the same result composed from torch: index_add segment sums, ops.randn, elementwise operations;
  * a whole sweep (right-hand sides, the batched CG solve, the draw) by a host clock around a run that ends in a device
    read, and the CG iterations of every sweep.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pxmcmc_amd import gibbs_np, ops  # noqa: E402
from pxmcmc_amd.forward import ForwardOperator, SphericalWaveletTransformOperator  # noqa: E402
from pxmcmc_amd.mcmc import PxMCMCParams  # noqa: E402
from pxmcmc_amd.measurements import WeakLensing  # noqa: E402
from pxmcmc_amd.optim import GaussianGibbs  # noqa: E402
from pxmcmc_amd.prior import Gaussian  # noqa: E402
from pxmcmc_amd.transforms import SphericalHarmonicTransform  # noqa: E402
from pxmcmc_amd.utils import build_mask  # noqa: E402


MAX_ITER = 6000  # the weak-lensing system is badly conditioned: thousands of iterations at tol = 1e-6


def region_us(fn, reps=20, regions=5):
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


def sampler(kind, L, C):
    rng = np.random.default_rng(0)
    if kind == "degree":
        mask = build_mask(L, size=10.0)
        wl = WeakLensing(L, mask, ngal=np.full_like(mask, 30), max_chains=C)
        tr = SphericalHarmonicTransform(L, max_chains=C)
        data = (rng.normal(size=wl.ndata) + 1j * rng.normal(size=wl.ndata)) * 0.05
        op = ForwardOperator(data, 1 / wl.inv_cov, "synthesis", transform=tr, measurement=wl, nparams=L * L)
        params = PxMCMCParams(lmda=1.0, delta=1e-3, mu=1.0, nsamples=1, nburn=0, ngap=1, complex=True, verbosity=0)
        prior = Gaussian.from_power_spectrum(1e-3 * (1.0 + np.arange(L)) ** -1.5, L, 1.0)
        return GaussianGibbs(op, prior, params, nchains=C, groups="degree", lmin=2, tol=1e-6, max_iter=MAX_ITER, check_every=50, seed=1)
    op = SphericalWaveletTransformOperator(rng.normal(size=L * (2 * L - 1)), 1.0, "synthesis", L, 2, 2, max_chains=C)
    params = PxMCMCParams(lmda=1.0, delta=1e-3, mu=1.0, nsamples=1, nburn=0, ngap=1, verbosity=0)
    return GaussianGibbs(op, Gaussian(1.0, 1.0), params, nchains=C, groups="scale", tol=1e-6, max_iter=MAX_ITER, check_every=50, seed=1)


def torch_draw(gib, X, it):
    """the variance draw composed from torch and ops.randn -> a closure that returns (Dg, D, sqrtD, Minv)"""
    b, K, n, C = gib.group_bounds, gib.K, gib._n, gib.nchains
    dev = X.device
    gid = torch.from_numpy(np.repeat(np.arange(K), np.diff(b))).to(dev)
    # pair index -> group and the mask of the deviates t < nu of every pair (gibbs_np.deviate_index)
    pair_gid = np.zeros(n + K + 1, dtype=np.int64)
    use = np.zeros((n + K + 1, 2))
    for k in range(K):
        lo, hi = b[k] + k, b[k + 1] + k + 1
        pair_gid[lo:hi] = k
        if gib.sampled[k]:
            t = np.arange(int(gib.nu[k]))
            idx, comp = gibbs_np.deviate_index(b, k, t)
            use[idx, comp] = 1.0
    pair_gid, use = torch.from_numpy(pair_gid).to(dev), torch.from_numpy(use).to(dev)
    sampled = torch.from_numpy(gib.sampled).to(dev)
    old = gib._Dg0.clone()
    h, (d_lo, d_hi) = float(gib.trace_estimate), gib.precision_bounds

    def run():
        a = torch.view_as_real(X) if X.is_complex() else X.unsqueeze(-1)
        sig = torch.zeros((C, K), dtype=torch.float64, device=dev).index_add_(1, gid, (a * a).sum(-1))
        om = torch.view_as_real(ops.randn(n + K + 1, C, complex_=True, seed=gib.seed, chain0=gib.chain_offset, it=it, noise64=True))
        chi = torch.zeros((C, K), dtype=torch.float64, device=dev).index_add_(1, pair_gid, (om * om * use).sum(-1))
        Dg = torch.where(sampled, torch.where(sig > 0, torch.clamp(chi / sig, d_lo, d_hi), torch.full_like(sig, d_hi)), old)
        D = Dg[:, gid].contiguous()
        return Dg, D, torch.sqrt(D), 1.0 / (D + h)

    return run


def measure(kind, L, C, sweeps):
    gib = sampler(kind, L, C)
    n, K = gib._n, gib.K
    res = {"n": n, "K": K, "nslices": gib._groups.nslices, "trace_estimate": gib.trace_estimate}
    X = ops.randn(n, C, complex_=gib._dt.is_complex, seed=3, it=5, noise64=True)
    it = gib._VAR_ITER
    # the call, eager and replayed from a graph
    eager = lambda: gib._variance_draw(X, it)  # noqa: E731
    res["draw_eager_us"], res["draw_eager_spread"] = region_us(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.capture_scope(), torch.cuda.graph(g):
        eager()
    res["draw_replayed_us"], res["draw_replayed_spread"] = region_us(g.replay)
    # the torch composition, and that it computes the same precisions (sums in another order: a few ulps)
    gib._Dg.copy_(gib._Dg0)
    eager()
    composed = torch_draw(gib, X, it)
    Dg_t = composed()[0]
    res["composition_max_rel_diff"] = float(((Dg_t - gib._Dg).abs() / gib._Dg.abs().clamp_min(1e-300)).max())
    res["draw_torch_us"], res["draw_torch_spread"] = region_us(composed)
    res["torch_over_replayed"] = res["draw_torch_us"] / res["draw_replayed_us"]
    # algorithmic bytes of the call: the state once, three [C, n] arrays out
    res["draw_bytes"] = C * n * ((16 if gib._dt.is_complex else 8) + 24)
    del g
    # whole sweeps
    gib.run(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gib.run(sweeps)
    torch.cuda.synchronize()
    res["sweep_ms"] = (time.perf_counter() - t0) / sweeps * 1e3
    res["sweeps"] = sweeps
    res["cg_iterations_per_sweep"] = gib.solve_iterations.max(axis=1).tolist()
    res["all_converged"] = bool(gib.solve_converged.all())
    res["last_rel_residual_max"] = float(gib.rel_residual[-1].max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--groups", nargs="+", default=["degree", "scale"], choices=["degree", "scale"])
    args = ap.parse_args()
    res = {"L": args.L, "chains": args.chains}
    for kind in args.groups:
        res[kind] = measure(kind, args.L, args.chains, args.sweeps)
        print(json.dumps({kind: res[kind]}), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
