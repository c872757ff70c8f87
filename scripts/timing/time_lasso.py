"""The sparse posterior's Gibbs sampler: the precision draw and a sweep at L = 256 with 16 chains on the
wavelet synthesis operator with the identity measurement, and MYULA's bias against the exact sampler at L = 32.

  python scripts/timing/time_lasso.py [--out FILE] [--L L] [--chains C] [--sweeps S] [--bias-L L] [--bias-sweeps S]

Reports, as the median of 5 device-synchronised regions of 20 calls (and their spread):
  * pxm_lasso_precision_draw, without and with sums, eager and replayed from a captured graph, with the bytes the call moves
    and the rate that gives;
  * the same arithmetic composed from torch: ops.randn for the normals, torch.rand for the uniforms (the library has no
    uniform entry point, so the composition is compared in distribution: the mean of log D), elementwise operations;
  * whole sweeps (right-hand sides, the batched CG solve, the draw) by a host clock around a run that ends in a device read,
    and the CG iterations of every sweep;
  * with --bias-L: the relative difference of the posterior-mean and standard-deviation maps of the image between MYULA at
    the step of examples/topography_synthetic.py and LassoGibbs, both through PosteriorSummary.
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

from pxmcmc_amd import ops  # noqa: E402
from pxmcmc_amd.forward import SphericalWaveletTransformOperator  # noqa: E402
from pxmcmc_amd.mcmc import MYULA, PxMCMCParams  # noqa: E402
from pxmcmc_amd.optim import LassoGibbs  # noqa: E402
from pxmcmc_amd.prior import S2_Wavelets_L1  # noqa: E402


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


def replayed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.capture_scope(), torch.cuda.graph(g):
        fn()
    return g


def problem(L, C, sigma, lmda, mu=1.0, B=1.5, J_min=2, seed=0):
    """the synthetic topography of examples/topography_synthetic.py: a band-limited real field with a red spectrum plus noise"""
    rng = np.random.default_rng(seed)
    flm = np.zeros(L * L, dtype=complex)
    for el in range(L):
        m = np.arange(1, el + 1)
        flm[el * el + el] = rng.normal() / (1 + el)
        v = (rng.normal(size=el) + 1j * rng.normal(size=el)) / (np.sqrt(2) * (1 + el))
        flm[el * el + el + m] = v
        flm[el * el + el - m] = (-1.0) ** m * np.conj(v)
    truth = ops.ShtPlan(L, 0).inverse(flm).cpu().numpy().real
    truth /= np.sqrt(np.mean(truth ** 2))
    data = truth + sigma * rng.normal(size=truth.size)
    op = SphericalWaveletTransformOperator(data, sigma, "synthesis", L, B, J_min, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", op.transform.inverse, op.transform.inverse_adjoint, lmda * mu, L=L, B=B, J_min=J_min)
    return op, reg, truth


def torch_draw(las, X, it):
    """the precision draw composed from torch and ops.randn -> a closure that returns (D, sqrtD, Minv)"""
    n, C = las._n, las.nchains
    t = (las._T * las._tscale) if isinstance(las._T, torch.Tensor) else torch.full((n,), las._T * las._tscale, dtype=torch.float64, device=X.device)
    h, (d_lo, d_hi) = float(las.trace_estimate), las.precision_bounds
    gen = torch.Generator(device=X.device).manual_seed(1)

    def run():
        z = ops.randn(n, C, complex_=True, seed=las.seed, chain0=las.chain_offset, it=it, noise64=True).real
        u = torch.rand((C, n), dtype=torch.float64, device=X.device, generator=gen)
        rt = 1.0 / t
        a, zt = X.abs() * rt, z * rt
        g = 0.5 * (zt * zt)
        d1 = 1.0 / ((a + g) + torch.sqrt(g * (g + 2.0 * a)))
        raw = torch.where(u * (1.0 + a * d1) > 1.0, 1.0 / (a * (a * d1)), d1)
        D = torch.clamp(raw, d_lo, d_hi)
        return D, torch.sqrt(D), 1.0 / (D + h)

    return run


def measure(L, C, sweeps):
    op, reg, _ = problem(L, C, sigma=1.0, lmda=1.0)
    params = PxMCMCParams(lmda=1.0, delta=1e-3, mu=1.0, nsamples=1, nburn=0, ngap=1, verbosity=0)
    las = LassoGibbs(op, reg, params, nchains=C, tol=1e-6, max_iter=6000, check_every=50, seed=1)
    n = las._n
    res = {"n": n, "trace_estimate": las.trace_estimate}
    X = ops.randn(n, C, complex_=True, seed=3, it=5, noise64=True)
    it = 1 << 60
    sums = torch.zeros((C, 2), dtype=torch.float64, device=X.device)
    for name, sm in (("draw", None), ("draw_sums", sums)):
        eager = lambda sm=sm: las._precision_draw(X, it, sums=sm)  # noqa: E731
        res[name + "_eager_us"], res[name + "_eager_spread"] = region_us(eager)
        g = replayed(eager)
        res[name + "_replayed_us"], res[name + "_replayed_spread"] = region_us(g.replay)
        del g
    # algorithmic bytes of the call: the state once, three [C, n] arrays out (T, 8 bytes per element, is shared by the chains)
    res["draw_bytes"] = C * n * (16 + 24) + 8 * n
    res["draw_GBps"] = res["draw_bytes"] / res["draw_replayed_us"] * 1e-3
    res["draw_elements_per_s"] = C * n / res["draw_replayed_us"] * 1e6
    res["clamped_fraction"] = float(sums[:, 1].sum() / (C * n))
    kernel_mean_logD = float(torch.log(las._D).mean())
    composed = torch_draw(las, X, it)
    res["mean_logD_kernel"], res["mean_logD_torch"] = kernel_mean_logD, float(torch.log(composed()[0]).mean())
    res["draw_torch_us"], res["draw_torch_spread"] = region_us(composed)
    res["torch_over_replayed"] = res["draw_torch_us"] / res["draw_replayed_us"]
    # whole sweeps
    las.run(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    las.run(sweeps)
    torch.cuda.synchronize()
    res["sweep_ms"] = (time.perf_counter() - t0) / sweeps * 1e3
    res["sweeps"] = sweeps
    res["cg_iterations_per_sweep"] = las.solve_iterations.max(axis=1).tolist()
    res["all_converged"] = bool(las.solve_converged.all())
    res["last_rel_residual_max"] = float(las.rel_residual[-1].max())
    res["clamped_per_sweep"] = las.clamped_chain.mean(axis=1).tolist()
    return res


def bias(L, C, sweeps, sigma=0.05, lmda=1e-6, nsamples=400, ngap=100, nburn=10000):
    """MYULA at the example's default step against LassoGibbs, both through PosteriorSummary of the image"""
    op, reg, truth = problem(L, C, sigma, lmda)
    L_g = op.gradient_lipschitz(iters=50, tol=1e-3)
    delta = 0.8 / (L_g + 1 / lmda)
    res = {"L": L, "chains": C, "delta": delta, "sigma": sigma, "lmda": lmda}
    params = PxMCMCParams(nsamples=nsamples, nburn=nburn, ngap=ngap, delta=delta, lmda=lmda, mu=1.0, verbosity=0)
    params.track = [t for t in params.track if t != "chain"]
    las = LassoGibbs(op, reg, params, nchains=C, tol=1e-6, max_iter=2000, seed=1)
    t0 = time.perf_counter()
    exact = las.run(sweeps, nburn=sweeps // 4, summary="image", summary_ess=16)
    res["gibbs_s"] = time.perf_counter() - t0
    res["gibbs_sweeps"], res["gibbs_cg_iterations"] = sweeps, [int(las.solve_iterations.min()), int(las.solve_iterations.max())]
    res["gibbs_max_rhat"] = float(exact.max_rhat()[0])
    res["gibbs_ess_report"] = exact.ess_report("image")
    my = MYULA(op, reg, params, nchains=C, summary="image", summary_ess=16)
    t0 = time.perf_counter()
    my.run(start_point=np.zeros(op.nparams))
    res["myula_s"] = time.perf_counter() - t0
    approx = my.summary["image"]
    res["myula_iterations"], res["myula_max_rhat"] = int(my.niter), float(approx.max_rhat()[0])
    res["myula_ess_report"] = approx.ess_report("image")
    m_e, m_a = exact.pooled_mean().cpu().numpy().real, approx.pooled_mean().cpu().numpy().real
    s_e, s_a = np.sqrt(exact.pooled_variance().cpu().numpy()), np.sqrt(approx.pooled_variance().cpu().numpy())
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))  # noqa: E731
    res["mean_rel_diff"], res["std_rel_diff"] = rel(m_a, m_e), rel(s_a, s_e)
    res["std_ratio_median"] = float(np.median(s_a / s_e))
    res["mean_error_gibbs"], res["mean_error_myula"] = rel(m_e, truth), rel(m_a, truth)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--bias-L", type=int, default=None)
    ap.add_argument("--bias-sweeps", type=int, default=400)
    ap.add_argument("--bias-chains", type=int, default=4)
    args = ap.parse_args()
    res = {"L": args.L, "chains": args.chains}
    if args.L > 0:
        res["draw"] = measure(args.L, args.chains, args.sweeps)
        print(json.dumps({"draw": res["draw"]}), flush=True)
    if args.bias_L:
        res["bias"] = bias(args.bias_L, args.bias_chains, args.bias_sweeps)
        print(json.dumps({"bias": res["bias"]}), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
