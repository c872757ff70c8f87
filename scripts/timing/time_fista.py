"""FISTA at the configs[2] size (L = 256, B = 2, J_min = 2, 16 chains), with SKROCK measured in the
same run for comparison.

  python scripts/timing/time_fista.py [--out FILE]   the pxm_fista_step launch alone and pxm_skrock_stage at j >= 2 alone
                                                     (device time from events around back-to-back calls, and the HBM rate
                                                     on each kernel's algorithmic bytes); a replayed FISTA iteration and a
                                                     replayed SKROCK s = 1 iteration (median of 5 device-synchronised regions
                                                     after warm-up)
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


def launch_us(fn, reps=50):
    """mean device time of one call, from events around `reps` back-to-back calls (after 5 warm-up calls)"""
    for _ in range(5):
        fn()
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
    assert s._eng["graph"] is not None, s._eng.get("graph_error")
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
    sk = SKROCK(op, reg, PxMCMCParams(lmda=LMDA, delta=DELTA, s=5, verbosity=0), nchains=C)
    co = sk._stage_coefs()
    t = {
        "fista_step": launch_us(lambda: ops.fista_step(X, G, V, 1.0 / Lg, LMDA, beta, T=T, iter_dev=it, out=(out, out2), sums=sums,
                                                       scratch=scratch)),
        "skrock_stagej": launch_us(lambda: ops.skrock_stage(X, *co[2], T=T, gradg=G, V=V, out=out, iter_dev=it)),
    }
    nbytes = {"fista_step": 5 * state + n * 8, "skrock_stagej": 4 * state + n * 8}  # read Y, gradg, X_k (U, gradg, V) and T; write 2 (1)
    res["launch_us"] = t  # (fista_step: the step kernel and its finishing kernel)
    res["bytes"] = nbytes
    res["TBps"] = {k: nbytes[k] / (t[k] * 1e-6) / 1e12 for k in t}
    res["fraction_of_copy_rate"] = {k: res["TBps"][k] * 1e12 / COPY_RATE for k in t}
    res["fista_rate_over_stage_rate"] = res["TBps"]["fista_step"] / res["TBps"]["skrock_stagej"]

    # replayed iterations
    f = started(FISTA(op, reg, PxMCMCParams(lmda=LMDA, verbosity=0), nchains=C, gamma=1.0 / (Lg * 1.0001), max_iter=4096), op)
    med_f, all_f = iteration_ms(f)
    f._engine_stop()
    s1 = started(SKROCK(op, reg, PxMCMCParams(lmda=LMDA, delta=DELTA, s=1, nsamples=1, nburn=0, ngap=1, verbosity=0), nchains=C, seed=1), op)
    med_s, all_s = iteration_ms(s1)
    s1._engine_stop()
    res["iteration_ms"] = {"fista": med_f, "fista_regions": all_f, "skrock_s1": med_s, "skrock_s1_regions": all_s,
                           "fista_over_skrock_s1": med_f / med_s}
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
