"""The primal-dual iteration of optim.PrimalDual at L = 256, B = 2, J_min = 2 with 16 chains in the
analysis setting.

  python scripts/timing/time_pd.py [--out FILE]   the five parts of one iteration alone (calc_gradg(forward(x)), A^H v, the
                                                  primal launch, A xbar, the dual launch: device time from events around
                                                  back-to-back calls, median of 5 such regions); the two step launches against
                                                  the same updates composed from torch operations on the same arrays, and
                                                  their HBM rate on the algorithmic bytes; one iteration eager and replayed
                                                  (median of 5 device-synchronised regions after warm-up)
"""
import argparse
import contextlib
import io
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
from pxmcmc_amd.mcmc import PxMCMCParams  # noqa: E402
from pxmcmc_amd.optim import PrimalDual  # noqa: E402
from pxmcmc_amd.prior import L1  # noqa: E402

L, B, J_MIN, C = 256, 2.0, 2, 16
COPY_RATE = 6.29e12  # measured float4 copy rate of the MI355X, bytes/s
LMDA, SIG = 1e-3, 0.05


def launch_us(fn, reps=20, regions=5):
    """device time of one call: the median over `regions` regions of `reps` back-to-back calls between two events (after 3
    warm-up calls) -> (median, the regions' values)"""
    for _ in range(3):
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
    return statistics.median(times), times


def iteration_ms(s, iters=16, regions=5):
    s._engine_advance(2 * iters)  # warm-up
    times = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s._engine_advance(iters)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / iters * 1e3)
    return statistics.median(times), times


def started(s, op):
    with contextlib.redirect_stdout(io.StringIO()):
        X, preds = s._initial_sample(np.zeros(op.nparams))
    s._engine_start(X, preds, 0)
    return s


def torch_primal(X, G, U, tau, X1, Xbar):
    """the primal update and its two sums from torch operations"""
    torch.add(G, U, out=X1)
    torch.add(X, X1, alpha=-tau, out=X1)
    torch.sub(2 * X1, X, out=Xbar)
    d = X1 - X
    return (d.real ** 2 + d.imag ** 2).sum(dim=1), (X1.real ** 2 + X1.imag ** 2).sum(dim=1)


def torch_dual(V, W, T, sigma, rscale, V1):
    """the dual update and its three sums from torch operations"""
    w = torch.add(V, W, alpha=sigma)
    a = w.abs()
    r = T * rscale
    torch.mul(w, torch.where(a > r, r / a, torch.ones_like(a)), out=V1)
    d = V1 - V
    return (d.real ** 2 + d.imag ** 2).sum(dim=1), (V1.real ** 2 + V1.imag ** 2).sum(dim=1), (T * W.abs()).sum(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P = L * (2 * L - 1)
    rng = np.random.default_rng(0)
    data = rng.normal(size=P)
    op = SphericalWaveletTransformOperator(data, SIG, "analysis", L, B, J_MIN, max_chains=C)
    tr = op.transform
    m = tr.ncoefs
    reg = L1("analysis", tr.inverse, tr.inverse_adjoint, LMDA * (0.5 + rng.random(m)))
    dev = ops.device()
    res = {"config": {"L": L, "B": B, "J_min": J_MIN, "chains": C, "npix": P, "ncoefs": m}}
    t0 = time.perf_counter()
    est = PrimalDual(op, reg, PxMCMCParams(lmda=LMDA, mu=1.0, verbosity=0), nchains=C, max_iter=4096)
    res["setup"] = {"seconds": time.perf_counter() - t0, "L_g": est.L_g, "A_norm2": est.A_norm2, "tau": est.tau, "sigma": est.sigma}

    # the five parts alone, on the same arrays
    X = torch.randn(C, P, dtype=torch.complex128, device=dev)
    G, U, X1, Xbar = torch.randn_like(X), torch.randn_like(X), torch.empty_like(X), torch.empty_like(X)
    V = torch.randn(C, m, dtype=torch.complex128, device=dev)
    W, V1 = torch.randn_like(V), torch.empty_like(V)
    T = reg.T_dev
    ps = torch.empty((C, 2), dtype=torch.float64, device=dev)
    ds = torch.empty((C, 3), dtype=torch.float64, device=dev)
    scratch = ops.pd_scratch(C, dev)
    f = est.gradient_op
    timed = {
        "gradg_forward": launch_us(lambda: f.calc_gradg(f.forward(X))),
        "AH_v": launch_us(lambda: tr.inverse(V)),
        "pd_primal_step": launch_us(lambda: ops.pd_primal_step(X, G, U, est.tau, out=(X1, Xbar), sums=ps, scratch=scratch), reps=50),
        "A_xbar": launch_us(lambda: tr.inverse_adjoint(X)),
        "pd_dual_step": launch_us(lambda: ops.pd_dual_step(V, W, T, est.sigma, 1.0 / LMDA, out=V1, sums=ds, scratch=scratch), reps=50),
        "torch_primal": launch_us(lambda: torch_primal(X, G, U, est.tau, X1, Xbar), reps=50),
        "torch_dual": launch_us(lambda: torch_dual(V, W, T, est.sigma, 1.0 / LMDA, V1), reps=50),
    }
    t = {k: v[0] for k, v in timed.items()}
    res["launch_us"] = t  # (the two step entries: the step kernel and its finishing kernel)
    res["launch_us_regions"] = {k: v[1] for k, v in timed.items()}
    nbytes = {"pd_primal_step": 5 * C * P * 16, "pd_dual_step": 3 * C * m * 16 + m * 8}
    res["bytes"] = nbytes
    res["TBps"] = {k: nbytes[k] / (t[k] * 1e-6) / 1e12 for k in nbytes}
    res["fraction_of_copy_rate"] = {k: res["TBps"][k] * 1e12 / COPY_RATE for k in nbytes}
    res["torch_over_kernel"] = {"primal": t["torch_primal"] / t["pd_primal_step"], "dual": t["torch_dual"] / t["pd_dual_step"]}
    res["parts_sum_us"] = sum(t[k] for k in ("gradg_forward", "AH_v", "pd_primal_step", "A_xbar", "pd_dual_step"))

    # one iteration, replayed and eager
    for name, graph in (("replayed", True), ("eager", False)):
        s = started(PrimalDual(op, reg, PxMCMCParams(lmda=LMDA, mu=1.0, verbosity=0), nchains=C, tau=est.tau, sigma=est.sigma,
                               max_iter=4096, use_graph=graph), op)
        assert (s._eng["graph"] is not None) == graph, s._eng["graph_error"]
        med, regions = iteration_ms(s)
        s._engine_stop()
        res["iteration_ms_" + name] = {"median": med, "regions": regions}
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
