"""SKROCK at the configs[2] size (L = 256, B = 2, J_min = 2, 16 chains, fp64 Philox, graph replay).

  python scripts/timing/time_skrock.py [--out FILE]    iteration time for s = 1, 5, 10 (median of 5 timed regions after
                                                       warm-up, device-synchronised) and the time of each launch alone
                                                       (stage 0, stage 1, stage j >= 2, forward, calc_gradg) with the stage
                                                       kernel's HBM rate on its algorithmic bytes
  python scripts/timing/time_skrock.py --trace S       a short replayed run at s = S only (for rocprofv3 --kernel-trace --stats)
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
from pxmcmc_amd.prior import S2_Wavelets_L1  # noqa: E402

L, B, J_MIN, C = 256, 2.0, 2, 16
COPY_RATE = 6.29e12  # measured float4 copy rate of the MI355X, bytes/s
LMDA, DELTA = 1e-6, 1e-7


def stage_bytes(C, n, kind):
    """algorithmic bytes of one stage launch on a complex128 [C, n] state with the stock soft threshold (T: float64 [n])"""
    state = C * n * 16
    if kind == "stage0":  # read X, write Y (Z from Philox)
        return 2 * state
    return 4 * state + n * 8  # read U, gradg, V and T, write K


def problem():
    P = L * (2 * L - 1)
    data = np.random.default_rng(0).normal(size=P)
    op = SphericalWaveletTransformOperator(data, 0.05, "synthesis", L, B, J_MIN, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L, B=B, J_min=J_MIN)
    return op, reg


def sampler(op, reg, s):
    p = PxMCMCParams(lmda=LMDA, delta=DELTA, s=s, nsamples=1, nburn=0, ngap=1, verbosity=0)
    sk = SKROCK(op, reg, p, nchains=C, seed=1)
    with contextlib.redirect_stdout(io.StringIO()):
        X, preds = sk._initial_sample(np.zeros(op.nparams))
    sk._engine_start(X, preds, 0)
    assert sk._eng["graph"] is not None, sk._eng["graph_error"]
    return sk


def iteration_ms(sk, iters=16, regions=5):
    sk._engine_advance(2 * iters)  # warm-up
    times = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sk._engine_advance(iters)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / iters * 1e3)
    return statistics.median(times), times


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0)
    a = ap.parse_args()
    op, reg = problem()
    n = op.nparams
    if a.trace:
        sk = sampler(op, reg, a.trace)
        iteration_ms(sk, iters=16, regions=2)
        sk._engine_stop()
        print(f"traced s = {a.trace}: {n} coefficients x {C} chains")
        return
    res = {"config": {"L": L, "B": B, "J_min": J_MIN, "chains": C, "ncoefs": n, "noise": "philox fp64", "graph": True}}
    # launches alone
    dev = ops.device()
    X = (torch.randn(C, n, dtype=torch.complex128, device=dev) * 1e-3).contiguous()
    G, V, out = torch.randn_like(X), torch.randn_like(X), torch.empty_like(X)
    T = reg.T_dev
    sk = SKROCK(op, reg, PxMCMCParams(lmda=LMDA, delta=DELTA, s=5, verbosity=0), nchains=C)
    co = sk._stage_coefs()
    it = torch.zeros(1, dtype=torch.int64, device=dev)
    kw = dict(noise_complex=False, seed=1, chain0=0, it=0, iter_dev=it, noise64=True)
    t = {
        "stage0": launch_us(lambda: ops.skrock_stage(X, *co[0], out=out, **kw)),
        "stage1": launch_us(lambda: ops.skrock_stage(X, *co[1], T=T, gradg=G, V=V, out=out, **kw)),
        "stagej": launch_us(lambda: ops.skrock_stage(X, *co[2], T=T, gradg=G, V=V, out=out, **kw)),
        "forward": launch_us(lambda: op.forward(X), reps=20),
    }
    P = op.forward(X)
    t["calc_gradg"] = launch_us(lambda: op.calc_gradg(P), reps=20)
    res["launch_us"] = t
    res["stage_bytes"] = {k: stage_bytes(C, n, k) for k in ("stage0", "stage1", "stagej")}
    res["stage_TBps"] = {k: res["stage_bytes"][k] / (t[k] * 1e-6) / 1e12 for k in ("stage0", "stage1", "stagej")}
    res["stagej_fraction_of_copy_rate"] = res["stage_TBps"]["stagej"] * 1e12 / COPY_RATE
    print(json.dumps(res, indent=1), flush=True)
    res["iteration"] = {}
    for s in (1, 5, 10):
        sk = sampler(op, reg, s)
        med, all_ = iteration_ms(sk)
        sk._engine_stop()
        launches = t["stage0"] + t["stage1"] + (s - 1) * t["stagej"] + s * (t["forward"] + t["calc_gradg"])
        res["iteration"][s] = {"ms_median": med, "ms_regions": all_, "sum_of_launches_ms": launches * 1e-3,
                               "ratio": med / (launches * 1e-3)}
        print(f"s = {s:2d}: {med:.3f} ms/iteration (sum of its launches alone {launches * 1e-3:.3f} ms, "
              f"ratio {med / (launches * 1e-3):.3f})", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
