"""Spin wavelets at L = 256, B = 2, J_min = 2, 16 chains.

  python scripts/timing/time_spin.py [--out FILE]   per spin s in {0, 2, 3}: plan-creation time from an empty table cache,
                                                    table bytes, the four operators (median of 5 device-synchronised
                                                    regions after warm-up); per s in {0, 2}: the MYULA iteration under graph
                                                    replay in the complex layout (params.complex, complex data), scalar
                                                    sig_d (ring-space step) and vector sig_d (image step)
  python scripts/timing/time_spin.py --trace S      a short replayed MYULA run (scalar sig_d) at spin S only (for
                                                    rocprofv3 --kernel-trace --stats)
"""
import argparse
import contextlib
import gc
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

L, B, J_MIN, C = 256, 2.0, 2, 16
LMDA, DELTA = 1e-6, 1e-7


def timed(fn, reps=5, inner=5):
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


def myula_iteration(spin, vector_sig, steps=64):
    P = L * (2 * L - 1)
    rng = np.random.default_rng(0)
    data = rng.normal(size=P) + 1j * rng.normal(size=P)  # complex data: the complex layout at every spin
    sig = np.linspace(0.04, 0.06, P) if vector_sig else 0.05
    op = SphericalWaveletTransformOperator(data, sig, "synthesis", L, B, J_MIN, spin=spin, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L, B=B, J_min=J_MIN, spin=spin)
    p = PxMCMCParams(lmda=LMDA, delta=DELTA, nsamples=1, nburn=0, ngap=1, verbosity=0, complex=True)
    s = MYULA(op, reg, p, nchains=C, seed=1)
    X0 = np.random.default_rng(1).normal(size=(C, op.nparams)) * 0.01 + 0j
    with contextlib.redirect_stdout(io.StringIO()):
        s._prepare()
        X, preds = s._initial_sample(X0)
        if s._pairs_ok(X):
            s._pairs_start()
        s._engine_start(X, preds, 0)
    try:
        assert s._eng["graph"] is not None, s._eng["graph_error"]
        assert s._fused_wav and not s._pairs and s._eng["ring"] == (not vector_sig)
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


def measure(spin, sampler):
    gc.collect()
    ops.tables_trim()  # plan creation below builds every table it needs
    torch.cuda.synchronize()
    t = time.perf_counter()
    plan = ops.WavPlan(L, B, J_MIN, max_chains=C, spin=spin)
    torch.cuda.synchronize()
    create_s = time.perf_counter() - t
    rng = np.random.default_rng(spin + 10)
    X = ops.as_device(rng.normal(size=(C, plan.ncoefs)) + 1j * rng.normal(size=(C, plan.ncoefs)))
    f = ops.as_device(rng.normal(size=(C, plan.npix)) + 1j * rng.normal(size=(C, plan.npix)))
    res = {"spin": spin, "plan_create_s": create_s, "table_bytes_synthesis": plan.table_bytes(0),
           "table_bytes_synthesis_adjoint": plan.table_bytes(1)}
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        fn = getattr(plan, name)
        res[name + "_ms"] = 1e3 * timed(lambda: fn(arg))
    del plan
    if sampler:
        res["myula_iteration_ring_ms"] = 1e3 * myula_iteration(spin, False)
        res["myula_iteration_image_ms"] = 1e3 * myula_iteration(spin, True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=None, help="spin: a short replayed MYULA run only")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.trace is not None:
        print(json.dumps({"spin": a.trace, "myula_iteration_ring_ms": 1e3 * myula_iteration(a.trace, False, steps=32)}))
        return
    out = [measure(0, True), measure(2, True), measure(3, False)]
    for r in out:
        print(json.dumps(r))
    r0, r2 = out[0], out[1]
    print(json.dumps({"myula_ring_ratio_s2_over_s0": r2["myula_iteration_ring_ms"] / r0["myula_iteration_ring_ms"],
                      "myula_image_ratio_s2_over_s0": r2["myula_iteration_image_ms"] / r0["myula_iteration_image_ms"]}))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
