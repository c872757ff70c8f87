"""Hypothesis tests of image structure at L = 256, B = 2, J_min = 2, 16 slots.

  python scripts/timing/time_hyp.py [--out FILE] [--L L]

  * one inpainting iteration split into its four parts (A, the threshold, Psi, the step kernel): device time from events
    around back-to-back calls;
  * the step kernel's rate on its algorithmic bytes (x_prev read and x_next written for every slot, the labels and the MAP
    image once; y only inside the regions) against the rate of a device-to-device copy of the same buffers;
  * the same step composed from torch (a mask, where, two norms with temporaries) with and without the host read of the
    norms that decides when to stop;
  * 20 iterations stepped eagerly and by graph replay (host clock around a device synchronise);
  * the whole hypothesis_test call for superpixels of 16 x 16 samples.
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
from pxmcmc_amd.mcmc import PxMCMCParams  # noqa: E402
from pxmcmc_amd.prior import S2_Wavelets_L1  # noqa: E402
from pxmcmc_amd.uncertainty import hypothesis_test, superpixel_regions  # noqa: E402
from pxmcmc_amd.uncertainty.hyp import _InpaintBatches  # noqa: E402

B, J_MIN, C = 2.0, 2, 16
LMDA, SIGMA = 1e-3, 0.1


def launch_us(fn, reps=20):
    """mean device time of one call, from events around `reps` back-to-back calls (after 3 warm-up calls)"""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def host_s(fn, reps=3):
    """median host time of one call around a device synchronise, after a warm-up call"""
    times = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times[1:]), times[0]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--L", type=int, default=256)
    args = ap.parse_args(argv)
    L = args.L
    rng = np.random.default_rng(0)
    npix = L * (2 * L - 1)
    data = rng.normal(size=npix)
    op = SphericalWaveletTransformOperator(data, SIGMA, "synthesis", L, B, J_MIN, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L, B=B, J_min=J_MIN)
    p = PxMCMCParams(lmda=LMDA, mu=1.0, verbosity=0)
    tr, dev = op.transform, ops.device()
    X = ops.soft(ops.as_device(tr.forward(ops.as_device(data.astype(complex)))), reg.T_dev * 50.0)
    x_map = ops.as_device(tr.inverse(X[None]))[0]
    tau = 0.1 * float(ops.as_device(tr.forward(x_map)).abs().max())
    labels = superpixel_regions(L, 16)
    nreg = int(labels.max()) + 1
    res = {"L": L, "slots": C, "npix": npix, "ncoefs": int(op.nparams), "regions": nreg, "tau": tau}

    eng = _InpaintBatches(tr, x_map, labels, nreg, C, tau, 20, 1e-6, use_graph=True)
    res["graph_captured"] = eng.graph is not None
    res["graph_error"] = eng.graph_error
    eng._init(0)
    XA, XB = eng.XA, eng.XB
    coef = ops.as_device(tr.forward(XA))
    soft = ops.soft(coef, tau)
    y = ops.as_device(tr.inverse(soft))
    res["A_us"] = launch_us(lambda: tr.forward(XA))
    res["soft_us"] = launch_us(lambda: ops.soft(coef, tau))
    res["Psi_us"] = launch_us(lambda: tr.inverse(soft))

    def step():
        eng._step(y, XA, XB, eng.tol2)

    res["step_us"] = launch_us(step, reps=200)  # (both kernels; the image changes by more than tol: no slot freezes)
    res["slots_frozen_by_the_timed_step"] = int(eng.done.sum())
    inside = int((labels.reshape(-1)[None, :] == np.arange(C)[:, None]).sum())
    nbytes = C * npix * 32 + npix * (16 + 4) + inside * 16
    res["step_algorithmic_MB"] = nbytes / 1e6
    res["step_TBps_algorithmic"] = nbytes / (res["step_us"] * 1e-6) / 1e12
    t_copy = launch_us(lambda: XB.copy_(XA), reps=200)
    res["copy_us"] = t_copy
    res["copy_TBps"] = C * npix * 32 / (t_copy * 1e-6) / 1e12
    res["step_rate_over_copy_rate"] = res["step_TBps_algorithmic"] / res["copy_TBps"]

    lab = eng.labels
    ids = torch.arange(C, device=dev)

    def torch_step(read):
        zeta = lab[None, :] == ids[:, None]
        nxt = torch.where(zeta, y, x_map[None])
        d2 = torch.linalg.vector_norm(nxt - XA, dim=1) ** 2
        n2 = torch.linalg.vector_norm(nxt, dim=1) ** 2
        return (d2 <= eng.tol2 * n2).cpu() if read else (d2, n2)

    res["torch_step_us"] = launch_us(lambda: torch_step(False), reps=200)
    res["torch_step_with_host_read_s"] = host_s(lambda: torch_step(True), reps=9)[0]
    res["torch_step_over_step"] = res["torch_step_us"] / res["step_us"]

    def iterate(graph):
        eng._init(0)
        for _ in range(10):
            graph.replay() if graph is not None else eng._two()

    res["eager_20_iterations_s"] = host_s(lambda: iterate(None))[0]
    if eng.graph is not None:
        res["replay_20_iterations_s"] = host_s(lambda: iterate(eng.graph))[0]
    res["iterations_used"] = sorted(set(int(v) for v in eng.iters.cpu().numpy()))

    out = {}

    def whole():
        out["r"] = hypothesis_test(op, reg, p, X, labels, tau=tau, iters=20, batch=C)

    res["hypothesis_test_s"], res["hypothesis_test_first_call_s"] = host_s(whole)
    r = out["r"]
    res["physical"] = int(r.physical.sum())
    res["status_counts"] = {int(k): int(v) for k, v in zip(*np.unique(r.status, return_counts=True))}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
