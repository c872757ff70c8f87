"""SAPG at the configs[2] size (L = 256, B = 2, J_min = 2, 16 chains), beside MYULA in the same run.

  python scripts/timing/time_sapg.py [--out FILE]   pxm_sapg_step (step kernel + update kernel), pxm_sapg_step_groups with one
                                                    theta per wavelet scale and pxm_myula_step alone on the same arrays: device
                                                    time from events around back-to-back calls, the three
                                                    taken in turn over 7 rounds (median, min, max), and the HBM rate on the
                                                    algorithmic bytes; a replayed SAPG iteration without and with
                                                    groups="scale" and a replayed MYULA iteration
                                                    on the operators' own plans (the generic engine SAPG runs on: the fused
                                                    wavelet step is switched off for the comparison), median of 5
                                                    device-synchronised regions after warm-up
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
from pxmcmc_amd.mcmc import MYULA, PxMCMCParams  # noqa: E402
from pxmcmc_amd.prior import S2_Wavelets_L1  # noqa: E402
from pxmcmc_amd.sapg import SAPG  # noqa: E402
from pxmcmc_amd.utils import wavelet_scale_bounds  # noqa: E402

L, B, J_MIN, C = 256, 2.0, 2, 16
COPY_RATE = 6.29e12  # measured float4 copy rate of the MI355X, bytes/s
LMDA, DELTA = 1e-6, 1e-7


def launch_us(fn, reps=50):
    """mean device time of one call, from events around `reps` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P = L * (2 * L - 1)
    data = np.random.default_rng(0).normal(size=P)
    op = SphericalWaveletTransformOperator(data, 0.05, "synthesis", L, B, J_MIN, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L, B=B, J_min=J_MIN)
    n = op.nparams
    dev = ops.device()
    res = {"config": {"L": L, "B": B, "J_min": J_MIN, "chains": C, "ncoefs": n, "graph": True, "noise_bits": 64}}

    # the two launches alone, on the same arrays
    state = C * n * 16
    X = (torch.randn(C, n, dtype=torch.complex128, device=dev) * 1e-3).contiguous()
    G, out = torch.randn_like(X), torch.empty_like(X)
    T = reg.T_dev
    it = torch.zeros(1, dtype=torch.int64, device=dev)
    theta, eta = torch.ones(C, dtype=torch.float64, device=dev), torch.zeros(C, dtype=torch.float64, device=dev)
    rho = ops.as_device(np.zeros(8), torch.float64)
    scratch = ops.sapg_scratch(C, dev)
    bounds = wavelet_scale_bounds(L, B, J_MIN)
    K = len(bounds) - 1
    res["config"]["groups"] = {"K": K, "bounds": bounds.tolist()}
    theta_g, eta_g = torch.ones((C, K), dtype=torch.float64, device=dev), torch.zeros((C, K), dtype=torch.float64, device=dev)
    rho_g, d_g = ops.as_device(np.zeros((8, K)), torch.float64), ops.as_device(2.0 * np.diff(bounds), torch.float64)
    scratch_g = ops.sapg_groups_scratch(C, K, dev)
    calls = {
        "sapg_step": lambda: ops.sapg_step(X, G, T, DELTA, LMDA, theta, eta, float(n), rho, -7.0, 7.0, iter_dev=it, out=out,
                                           scratch=scratch, noise64=True),
        "sapg_step_groups": lambda: ops.sapg_step_groups(X, G, T, DELTA, LMDA, theta_g, eta_g, bounds, d_g, rho_g, -7.0, 7.0,
                                                         iter_dev=it, out=out, scratch=scratch_g, noise64=True),
        "myula_step": lambda: ops.myula_step(X, G, T, DELTA, LMDA, iter_dev=it, out=out, noise64=True),
    }
    for fn in calls.values():
        for _ in range(5):
            fn()
    rounds = {k: [] for k in calls}
    for _ in range(7):
        for k, fn in calls.items():
            rounds[k].append(launch_us(fn))
    nbytes = 3 * state + n * 8  # read X, gradg and T; write X'
    res["launch_us"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in rounds.items()}
    res["bytes"] = nbytes
    res["TBps"] = {k: nbytes / (statistics.median(v) * 1e-6) / 1e12 for k, v in rounds.items()}
    res["fraction_of_copy_rate"] = {k: res["TBps"][k] * 1e12 / COPY_RATE for k in rounds}
    res["sapg_over_myula"] = statistics.median(rounds["sapg_step"]) / statistics.median(rounds["myula_step"])
    res["groups_over_sapg"] = statistics.median(rounds["sapg_step_groups"]) / statistics.median(rounds["sapg_step"])

    # replayed iterations on the generic engine
    p = PxMCMCParams(lmda=LMDA, delta=DELTA, nsamples=1, nburn=0, ngap=1, verbosity=0)
    s = SAPG(op, reg, p, nchains=C, warmup=64, niter=4096, burn=0, seed=1)
    med_s, all_s = iteration_ms(started(s, op))
    s._engine_stop()
    sg = SAPG(op, reg, p, nchains=C, warmup=64, niter=4096, burn=0, seed=1, groups="scale")
    med_g, all_g = iteration_ms(started(sg, op))
    sg._engine_stop()
    m = MYULA(op, reg, p, nchains=C, seed=1)
    m._prepare()
    m._fused_wav = False  # the operators' own plans, as SAPG steps
    med_m, all_m = iteration_ms(started(m, op))
    m._engine_stop()
    res["iteration_ms"] = {"sapg": med_s, "sapg_regions": all_s, "sapg_groups": med_g, "sapg_groups_regions": all_g,
                           "sapg_groups_over_sapg": med_g / med_s, "myula_generic": med_m, "myula_generic_regions": all_m,
                           "sapg_over_myula_generic": med_s / med_m}
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
