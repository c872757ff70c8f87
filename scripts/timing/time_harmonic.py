"""Harmonic-space wavelets at L = 256, B = 2, J_min = 2, 16 chains.

  python scripts/timing/time_harmonic.py [--out FILE]   per (N, spin) in {(1, 0), (4, 0), (1, 2)}: plan-creation time, the
                                                        four operators (median of 5 device-synchronised regions after
                                                        warm-up) with their algorithmic bytes over kernel time, and the
                                                        MYULA iteration under graph replay (identity measurement, vector
                                                        sig_d): the fused harmonic step against the generic engine
  python scripts/timing/time_harmonic.py --trace N      a short replayed fused MYULA run at (N, 0) only (for
                                                        rocprofv3 --kernel-trace --stats)
Algorithmic bytes: what a kernel must read and write once -- split: f_lm reads of every item + X written; merge: X read +
f_lm written; fused step: X read and written, preds written, data and invcov read.
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
from pxmcmc_amd.forward import ForwardOperator  # noqa: E402
from pxmcmc_amd.measurements import Identity  # noqa: E402
from pxmcmc_amd.mcmc import MYULA, PxMCMCParams  # noqa: E402
from pxmcmc_amd.prior import L1  # noqa: E402
from pxmcmc_amd.transforms import SphericalWaveletTransform  # noqa: E402

L, B, J_MIN, C = 256, 2.0, 2, 16
LMDA, DELTA = 1e-6, 1e-7
PEAK = 8.0e12  # bytes / s


def timed(fn, reps=5, inner=10):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) / inner)
    return statistics.median(ts)


class _IdSub(Identity):
    """a measurement subclass: MYULA takes the generic engine"""


def myula_iteration(N, spin, generic, steps=64):
    rng = np.random.default_rng(0)
    data = rng.normal(size=L * L) + 1j * rng.normal(size=L * L)
    tr = SphericalWaveletTransform(L, B, J_MIN, dirs=N, spin=spin, harmonic=True, max_chains=C)
    ms = (_IdSub if generic else Identity)(L * L, L * L)
    op = ForwardOperator(data, np.linspace(0.04, 0.06, L * L), "synthesis", transform=tr, measurement=ms, nparams=tr.ncoefs)
    p = PxMCMCParams(lmda=LMDA, delta=DELTA, nsamples=1, nburn=0, ngap=1, verbosity=0)
    s = MYULA(op, L1("synthesis", None, None, LMDA), p, nchains=C, seed=1)
    X0 = np.random.default_rng(1).normal(size=(C, op.nparams)) * 0.01 + 0j
    with contextlib.redirect_stdout(io.StringIO()):
        s._prepare()
        X, preds = s._initial_sample(X0)
        s._engine_start(X, preds, 0)
    try:
        assert s._eng["graph"] is not None, s._eng["graph_error"]
        assert s._fused_harm == (not generic)
        s._engine_advance(16)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            s._engine_advance(steps)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) / steps)
        return statistics.median(ts)
    finally:
        s._engine_stop()


def measure(N, spin):
    torch.cuda.synchronize()
    t = time.perf_counter()
    plan = ops.HarmWavPlan(L, B, J_MIN, N, spin=spin, max_chains=C)
    torch.cuda.synchronize()
    res = {"N": N, "spin": spin, "ncoefs": plan.ncoefs, "plan_create_s": time.perf_counter() - t, "kact": plan.info()[2]}
    rng = np.random.default_rng(N + 10 * spin)
    X = ops.as_device(rng.normal(size=(C, plan.ncoefs)) + 1j * rng.normal(size=(C, plan.ncoefs)))
    f = ops.as_device(rng.normal(size=(C, L * L)) + 1j * rng.normal(size=(C, L * L)))
    xb, fb = 16 * C * plan.ncoefs, 16 * C * L * L
    bytes_ = {"synthesis": xb + fb, "analysis_adjoint": xb + fb, "analysis": 2 * xb, "synthesis_adjoint": 2 * xb}
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        fn = getattr(plan, name)
        ms = 1e3 * timed(lambda: fn(arg))
        res[name + "_ms"] = ms
        res[name + "_frac_of_8TBs"] = bytes_[name] / (ms * 1e-3) / PEAK
    data = ops.as_device(rng.normal(size=L * L) + 1j * rng.normal(size=L * L))
    ic = ops.as_device(np.linspace(1.0, 2.0, L * L))
    out, P = torch.empty_like(X), torch.empty_like(f)
    ms = 1e3 * timed(lambda: plan.myula_step(X, data, ic, None, 1e-3, DELTA, LMDA, out=out, preds_out=P, noise64=True))
    res["fused_step_ms"] = ms
    res["fused_step_frac_of_8TBs"] = (2 * xb + fb + 24 * L * L) / (ms * 1e-3) / PEAK
    del plan
    res["myula_iteration_fused_ms"] = 1e3 * myula_iteration(N, spin, False)
    res["myula_iteration_generic_ms"] = 1e3 * myula_iteration(N, spin, True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=None, help="N: a short replayed fused MYULA run only")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.trace is not None:
        print(json.dumps({"N": a.trace, "myula_iteration_fused_ms": 1e3 * myula_iteration(a.trace, 0, False, steps=32)}))
        return
    out = [measure(1, 0), measure(4, 0), measure(1, 2)]
    for r in out:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
