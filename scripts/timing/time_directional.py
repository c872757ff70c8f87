"""Directional wavelets at L = 256, B = 2, J_min = 2, 16 chains, N in {1 (directional plan), 2, 4}.

  python scripts/timing/time_directional.py [--out FILE]   per N: plan-creation time, table bytes, the four operators
                                                           (median of 5 device-synchronised regions after warm-up), the
                                                           algorithmic bytes of each new kernel launch (durations: the
                                                           rocprofv3 trace below), and the MYULA iteration under graph replay (generic engine)
  python scripts/timing/time_directional.py --trace N      a short replayed MYULA run at N only (for
                                                           rocprofv3 --kernel-trace --stats)
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

L, B, J_MIN, C = 256, 2.0, 2, 16
HBM_SPEC = 8.0e12  # MI355X HBM3E spec, bytes/s
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


def shapes(N):
    """(bl of every (block, n) item, bl of every block, planes of every block) of the plan at (L, B, J_MIN, N)"""
    bls = ops.wav_bandlimits(L, B, J_MIN)
    items = [bls[0]] + [bl for bl in bls[1:] for n in range(-(N - 1), N, 2) if abs(n) < bl]
    planes = [1] + [2 * N - 1] * (len(bls) - 1)
    return items, bls, planes


def kernel_bytes(N):
    """algorithmic bytes of one launch of each new kernel for C chains (complex128: 16 B an element)"""
    items, bls, planes = shapes(N)
    split = sum(C * bl * bl * 16 for bl in items) + C * L * L * 16  # read f_lm once, write every item
    merge = split  # read every item, write f_lm
    nn = [1] + [sum(1 for n in range(-(N - 1), N, 2) if abs(n) < bl) for bl in bls[1:]]
    gamma = sum(C * bl * (2 * bl - 1) * 16 * (k + q) for bl, k, q in zip(bls, nn, planes))  # read g_n, write the planes
    return {"split": split, "merge": merge, "gamma": gamma}


def myula_iteration(N, steps=64):
    P = L * (2 * L - 1)
    data = np.random.default_rng(0).normal(size=P)
    op = SphericalWaveletTransformOperator(data, 0.05, "synthesis", L, B, J_MIN, dirs=N, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L, B=B, J_min=J_MIN, dirs=N)
    p = PxMCMCParams(lmda=LMDA, delta=DELTA, nsamples=1, nburn=0, ngap=1, verbosity=0)
    s = MYULA(op, reg, p, nchains=C, seed=1)
    X0 = np.random.default_rng(1).normal(size=(C, op.nparams)) * 0.01
    with contextlib.redirect_stdout(io.StringIO()):
        s._prepare()
        X, preds = s._initial_sample(X0)
        s._engine_start(X, preds, 0)
    try:
        assert s._eng["graph"] is not None, s._eng["graph_error"]
        s._engine_advance(16)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            s._engine_advance(steps)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) / steps)
        return statistics.median(ts), s._fused_wav
    finally:
        s._engine_stop()


def measure(N):
    torch.cuda.synchronize()
    t = time.perf_counter()
    plan = ops.DirWavPlan(L, B, J_MIN, N, max_chains=C)
    torch.cuda.synchronize()
    create_s = time.perf_counter() - t
    rng = np.random.default_rng(N)
    X = ops.as_device(rng.normal(size=(C, plan.ncoefs)) + 0j)
    f = ops.as_device(rng.normal(size=(C, plan.npix)) + 0j)
    res = {"N": N, "ncoefs": plan.ncoefs, "items_split_gamma_blocks": plan.info(), "plan_create_s": create_s,
           "table_bytes": plan.table_bytes(), "kernel_alg_bytes": kernel_bytes(N)}
    for name, arg in (("synthesis", X), ("synthesis_adjoint", f), ("analysis", f), ("analysis_adjoint", X)):
        fn = getattr(plan, name)
        res[name + "_ms"] = 1e3 * timed(lambda: fn(arg))
    it, fused = myula_iteration(N)
    res["myula_iteration_ms"] = 1e3 * it
    res["myula_fused_path"] = bool(fused)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0, help="N: a short replayed MYULA run only")
    ap.add_argument("--dirs", default="1,2,4")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.trace:
        it, _ = myula_iteration(a.trace, steps=32)
        print(json.dumps({"N": a.trace, "myula_iteration_ms": 1e3 * it}))
        return
    out = [measure(int(n)) for n in a.dirs.split(",")]
    for r in out:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
