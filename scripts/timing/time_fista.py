"""FISTA at the configs[2] size (L = 256, B = 2, J_min = 2, 16 chains), with SKROCK measured in the
same run for comparison.

  python scripts/timing/time_fista.py [--out FILE]   the pxm_fista_step launch alone (stock and given-prox forms), the
                                                     pxm_fista_step_restart launch alone (both forms) and pxm_skrock_stage at
                                                     j >= 2 alone, on the same arrays (device time from events around
                                                     back-to-back calls, median of 5 such regions and their spread, and the
                                                     HBM rate on each kernel's algorithmic bytes); a replayed FISTA iteration,
                                                     plain and restarted, and a replayed SKROCK s = 1 iteration (median of 5
                                                     device-synchronised regions after warm-up)
           [--convergence L [L ...]]                 also: iterations to tol = 1e-4 and the objective reached, plain and
                                                     restarted, one chain from zero on the wavelet problem at each L
                                                     (B = 2, J_min = 2, sigma = 0.05)
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
from pxmcmc_amd.mcmc import SKROCK, PxMCMCParams  # noqa: E402
from pxmcmc_amd.optim import FISTA  # noqa: E402
from pxmcmc_amd.prior import S2_Wavelets_L1  # noqa: E402

L, B, J_MIN, C = 256, 2.0, 2, 16
COPY_RATE = 6.29e12  # measured float4 copy rate of the MI355X, bytes/s
LMDA, DELTA = 1e-6, 1e-7


def launch_us(fn, reps=50, regions=5):
    """device time of one call: the median over `regions` regions of `reps` back-to-back calls between two events (after 5
    warm-up calls) -> (median, the regions' values)"""
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
    return statistics.median(times), times


def spread(times):
    """(max - min) / median of a list of regions"""
    return (max(times) - min(times)) / statistics.median(times)


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
    assert s._eng["graph"] is not None, s._eng["graph_error"]
    return s


def convergence(L_, tol=1e-4, max_iter=10000):
    """plain and restarted FISTA on the wavelet problem at bandlimit L_ (one chain from zero): iterations, objective"""
    data = np.random.default_rng(5).normal(size=L_ * (2 * L_ - 1))
    lmda = 1e-3
    op = SphericalWaveletTransformOperator(data, 0.05, "synthesis", L_, B, J_MIN, max_chains=1)
    reg = S2_Wavelets_L1("synthesis", None, None, lmda, L=L_, B=B, J_min=J_MIN)
    gamma = 1.0 / (op.gradient_lipschitz(iters=1000, tol=1e-4) * (1 + 1e-4))
    out = {"L": L_, "ncoefs": op.nparams, "tol": tol, "max_iter": max_iter}
    # the rule measures the step, not the distance to the minimum, and the steps after a restart are short: the third run
    # tells how many restarted iterations reach the objective at which the plain run stopped
    for name, restart, tol_ in (("plain", None, tol), ("restarted", "gradient", tol), ("restarted_tight", "gradient", tol * 1e-3)):
        est = FISTA(op, reg, PxMCMCParams(lmda=lmda, mu=1.0, verbosity=0), gamma=gamma, tol=tol_, max_iter=max_iter, restart=restart)
        t0 = time.perf_counter()
        est.run()
        out[name] = {"tol": tol_, "niter": int(est.niter[0]), "converged": bool(est.converged[0]),
                     "objective": float(est.objective_map[0]), "rel_change": float(est.rel_change[-1, 0]),
                     "seconds": time.perf_counter() - t0}
        if restart:
            out[name]["nrestarts"] = int(est.nrestarts[0])
            below = np.nonzero(est.objective[:, 0] <= out["plain"]["objective"])[0]
            out[name]["iterations_to_plain_objective"] = int(est.checks[below[0]]) if below.size else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--convergence", type=int, nargs="*", default=[], metavar="L")
    a = ap.parse_args()
    P = L * (2 * L - 1)
    data = np.random.default_rng(0).normal(size=P)
    op = SphericalWaveletTransformOperator(data, 0.05, "synthesis", L, B, J_MIN, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L, B=B, J_min=J_MIN)
    n = op.nparams
    dev = ops.device()
    res = {"config": {"L": L, "B": B, "J_min": J_MIN, "chains": C, "ncoefs": n, "graph": True}}
    t0 = time.perf_counter()
    Lg = op.gradient_lipschitz()
    res["gradient_lipschitz"] = {"L_g": Lg, "seconds": time.perf_counter() - t0}

    # the two streaming launches alone, on the same arrays
    state = C * n * 16
    X = (torch.randn(C, n, dtype=torch.complex128, device=dev) * 1e-3).contiguous()
    G, V, out, out2 = torch.randn_like(X), torch.randn_like(X), torch.empty_like(X), torch.empty_like(X)
    T = reg.T_dev
    it = torch.zeros(1, dtype=torch.int64, device=dev)
    beta = ops.as_device(np.full(8, 0.5), torch.float64)
    sums = torch.empty((C, 3), dtype=torch.float64, device=dev)
    scratch = ops.fista_scratch(C, dev)
    sums4 = torch.empty((C, 4), dtype=torch.float64, device=dev)
    scratch4 = ops.fista_restart_scratch(C, dev)
    index, nrest = torch.zeros(C, dtype=torch.int64, device=dev), torch.zeros(C, dtype=torch.int64, device=dev)
    gamma = 1.0 / Lg
    sk = SKROCK(op, reg, PxMCMCParams(lmda=LMDA, delta=DELTA, s=5, verbosity=0), nchains=C)
    co = sk._stage_coefs()
    kw3, kw4 = dict(out=(out, out2), sums=sums, scratch=scratch), dict(out=(out, out2), sums=sums4, scratch=scratch4)
    timed = {  # G doubles as the given proxf array: any array of the state's shape moves the same bytes
        "fista_step": launch_us(lambda: ops.fista_step(X, G, V, gamma, LMDA, beta, T=T, iter_dev=it, **kw3)),
        "fista_step_restart": launch_us(lambda: ops.fista_step_restart(X, G, V, gamma, LMDA, beta, index, T=T, restarts=nrest, **kw4)),
        "fista_step_given": launch_us(lambda: ops.fista_step(None, None, V, gamma, LMDA, beta, proxf=G, iter_dev=it, **kw3)),
        "fista_step_restart_given": launch_us(lambda: ops.fista_step_restart(X, None, V, gamma, LMDA, beta, index, proxf=G,
                                                                             restarts=nrest, **kw4)),
        "skrock_stagej": launch_us(lambda: ops.skrock_stage(X, *co[2], T=T, gradg=G, V=V, out=out, iter_dev=it)),
    }
    t = {k: v[0] for k, v in timed.items()}
    # read Y, gradg, X_k (U, gradg, V) and T, write 2 (1); given prox: read proxf, X_k (and Y with restart), write 2
    nbytes = {"fista_step": 5 * state + n * 8, "fista_step_restart": 5 * state + n * 8, "fista_step_given": 4 * state,
              "fista_step_restart_given": 5 * state, "skrock_stagej": 4 * state + n * 8}
    res["launch_us"] = t  # (the fista entries: the step kernel and its finishing kernel)
    res["launch_us_regions"] = {k: v[1] for k, v in timed.items()}
    res["launch_spread"] = {k: spread(v[1]) for k, v in timed.items()}
    res["restart_over_plain"] = {"stock": t["fista_step_restart"] / t["fista_step"], "margin": 2 * spread(timed["fista_step"][1]),
                                 "given": t["fista_step_restart_given"] / t["fista_step_given"], "given_bytes_ratio": 5 / 4}
    res["bytes"] = nbytes
    res["TBps"] = {k: nbytes[k] / (t[k] * 1e-6) / 1e12 for k in t}
    res["fraction_of_copy_rate"] = {k: res["TBps"][k] * 1e12 / COPY_RATE for k in t}
    res["fista_rate_over_stage_rate"] = res["TBps"]["fista_step"] / res["TBps"]["skrock_stagej"]

    # replayed iterations
    f = started(FISTA(op, reg, PxMCMCParams(lmda=LMDA, verbosity=0), nchains=C, gamma=1.0 / (Lg * 1.0001), max_iter=4096), op)
    med_f, all_f = iteration_ms(f)
    f._engine_stop()
    fr = started(FISTA(op, reg, PxMCMCParams(lmda=LMDA, verbosity=0), nchains=C, gamma=1.0 / (Lg * 1.0001), max_iter=4096,
                       restart="gradient"), op)
    med_r, all_r = iteration_ms(fr)
    fr._engine_stop()
    s1 = started(SKROCK(op, reg, PxMCMCParams(lmda=LMDA, delta=DELTA, s=1, nsamples=1, nburn=0, ngap=1, verbosity=0), nchains=C, seed=1), op)
    med_s, all_s = iteration_ms(s1)
    s1._engine_stop()
    res["iteration_ms"] = {"fista": med_f, "fista_regions": all_f, "fista_restart": med_r, "fista_restart_regions": all_r,
                           "skrock_s1": med_s, "skrock_s1_regions": all_s, "fista_over_skrock_s1": med_f / med_s,
                           "fista_restart_over_fista": med_r / med_f}
    res["convergence"] = [convergence(L_) for L_ in a.convergence]
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
