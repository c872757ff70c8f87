"""
Cost of one streaming-summary update at the benchmark size -- L = 256, B = 2, J_min = 2, 16 chains:
305 060 complex coefficients per chain, m = 610 120 real components -- beside one MYULA iteration of the same configuration.

  update      pxm_moments_update (the streaming pass and the one-workgroup launch that advances the counts): median of 5
              device-synchronised regions of 20 calls each, with and without best-sample tracking.  Algorithmic traffic:
              read x, mean, m2 and write mean, m2 = 5 * 8 * C * m bytes (about 390 MB), reported against 8 TB/s.
  cold        the same call after 512 MiB of unrelated traffic has passed through the 256 MiB last-level cache, as in a run
              where sampler iterations separate two updates: median of 5 regions of one call each, device events around it.
              (Back-to-back calls re-read accumulators that the previous call left in that cache.)
  realparts   the route of a sampler with params.complex = False (the benchmark configuration): the real parts of the
              complex128 state (x_stride 2), m = 305 060 per chain, 48 * C * n bytes (about 234 MB), warm and cold.
  iteration   one replayed MYULA iteration (fused ring-space step, two real chains per slot), same regions.

    python scripts/timing/time_summary.py [--out FILE.json]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pxmcmc_amd import ops  # noqa: E402
from pxmcmc_amd.forward import SphericalWaveletTransformOperator  # noqa: E402
from pxmcmc_amd.mcmc import MYULA, PxMCMCParams  # noqa: E402
from pxmcmc_amd.prior import S2_Wavelets_L1  # noqa: E402
from pxmcmc_amd.uncertainty import PosteriorSummary  # noqa: E402

L, B, J_MIN, C = 256, 2.0, 2, 16
HBM_RATE = 8e12  # bytes/s
LMDA, DELTA = 1e-6, 1e-7


def regions_ms(fn, calls=20, regions=5):
    """median over `regions` of the time of one call, each region `calls` back-to-back calls between two synchronisations"""
    for _ in range(calls):
        fn()
    times = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / calls * 1e3)
    return statistics.median(times), times


def cold_ms(fn, regions=5):
    """median device time of one call whose operands are not in the last-level cache: a 512 MiB copy runs before each"""
    src = torch.empty(512 << 20, dtype=torch.uint8, device=ops.device())
    dst = torch.empty_like(src)
    times = []
    for _ in range(regions + 1):
        dst.copy_(src)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times[1:]), times[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    data = np.random.default_rng(0).normal(size=L * (2 * L - 1))
    op = SphericalWaveletTransformOperator(data, 0.05, "synthesis", L, B, J_MIN, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L, B=B, J_min=J_MIN)
    n = op.nparams
    dev = ops.device()
    res = {"config": {"L": L, "B": B, "J_min": J_MIN, "chains": C, "ncoefs": n, "m": 2 * n}}

    X = torch.randn(C, n, dtype=torch.complex128, device=dev)
    logpi = torch.randn(C, dtype=torch.float64, device=dev)
    nbytes = 5 * 8 * C * 2 * n
    res["algorithmic_bytes"] = nbytes
    for name, best in (("update", False), ("update_best", True)):
        s = PosteriorSummary(C, n, True, best=best)
        med, times = regions_ms(lambda: s.update(X, logpi=logpi if best else None))
        res[name] = {"ms": med, "regions_ms": times, "TBps": nbytes / (med * 1e-3) / 1e12,
                     "fraction_of_8TBps": nbytes / (med * 1e-3) / HBM_RATE}
        med, times = cold_ms(lambda: s.update(X, logpi=logpi if best else None))
        res[name + "_cold"] = {"ms": med, "regions_ms": times, "TBps": nbytes / (med * 1e-3) / 1e12,
                               "fraction_of_8TBps": nbytes / (med * 1e-3) / HBM_RATE}

    # params.complex = False (the benchmark configuration): the real parts of the complex128 state, x_stride 2 -- m = n
    # components per chain, 16 B read per 8 B used: (16 + 4 * 8) * C * n bytes
    nbytes_re = 48 * C * n
    res["algorithmic_bytes_realparts"] = nbytes_re
    s = PosteriorSummary(C, n, False, best=True)
    for name, timer in (("update_realparts_best", regions_ms), ("update_realparts_best_cold", cold_ms)):
        med, times = timer(lambda: s.update(X, logpi=logpi))
        res[name] = {"ms": med, "regions_ms": times, "TBps": nbytes_re / (med * 1e-3) / 1e12,
                     "fraction_of_8TBps": nbytes_re / (med * 1e-3) / HBM_RATE}

    p = PxMCMCParams(lmda=LMDA, delta=DELTA, nsamples=1, nburn=0, ngap=1, verbosity=0)
    my = MYULA(op, reg, p, nchains=C, seed=1)
    my._prepare()
    with contextlib.redirect_stdout(io.StringIO()):
        X0, preds = my._initial_sample(np.zeros(n))
    if my._pairs_ok(X0):
        my._pairs_start()
    my._engine_start(X0, preds, 0)
    assert my._eng["graph"] is not None, my._eng["graph_error"]
    med, times = regions_ms(lambda: my._engine_advance(16), calls=4)
    my._engine_stop()
    res["myula_iteration"] = {"ms": med / 16, "regions_ms": [t / 16 for t in times]}
    res["update_over_iteration"] = {k: res[k]["ms"] / res["myula_iteration"]["ms"]
                                    for k in ("update_best", "update_best_cold", "update_realparts_best", "update_realparts_best_cold")}
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
