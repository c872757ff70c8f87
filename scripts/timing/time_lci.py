"""Local credible intervals at the configs[2] size (L = 256, B = 2, J_min = 2), 16 slots.

  python scripts/timing/time_lci.py [--out FILE] [--L L]

  * pxm_lci_eval alone (32 values of xi per slot in one pass): device time from events around back-to-back calls, the rate
    on its algorithmic bytes (a and b of every slot once, 32 B per coefficient, and T once; also on the 40 B per coefficient a
    slot alone would read) against the 8 TB/s of the part, and the fp64 square roots it issues per second;
  * the same 32 evaluations the way a user has them without it: a temporary a + xi b and ops.reduce_l1 per value of xi;
  * the whole pxm_lci_search of 10 rounds on that batch;
  * the whole local_credible_intervals call for superpixels of 16 x 16 samples (host clock around a device synchronise,
    median of 3 after a warm-up call).
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
from pxmcmc_amd.uncertainty import local_credible_intervals, superpixel_regions  # noqa: E402

B, J_MIN, C = 2.0, 2, 16
HBM_PEAK = 8e12  # bytes/s
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--L", type=int, default=256)
    args = ap.parse_args(argv)
    L = args.L
    rng = np.random.default_rng(0)
    data = rng.normal(size=L * (2 * L - 1))
    op = SphericalWaveletTransformOperator(data, SIGMA, "synthesis", L, B, J_MIN, max_chains=C)
    reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L, B=B, J_min=J_MIN)
    p = PxMCMCParams(lmda=LMDA, mu=1.0, verbosity=0)
    n, dev = op.nparams, ops.device()
    res = {"L": L, "slots": C, "ncoefs": n}

    a = ops.as_device(rng.normal(size=(C, n)) + 1j * rng.normal(size=(C, n)))
    b = ops.as_device((rng.normal(size=(C, n)) + 1j * rng.normal(size=(C, n))) * (rng.random((C, n)) < 0.3))
    T = reg.T_dev
    xi = ops.as_device(rng.normal(size=(C, 32)))
    P = torch.empty((C, 34), dtype=torch.float64, device=dev)
    scratch = ops.lci_scratch(n, C, dev)
    t_eval = launch_us(lambda: ops.lci_eval(a, b, T, xi, out=P, scratch=scratch))
    nbytes = C * n * 32 + n * 8
    res["eval_us"] = t_eval
    res["eval_TBps_algorithmic"] = nbytes / (t_eval * 1e-6) / 1e12
    res["eval_TBps_40B_per_coefficient"] = C * n * 40 / (t_eval * 1e-6) / 1e12
    res["eval_share_of_8TBps"] = nbytes / (t_eval * 1e-6) / HBM_PEAK
    res["eval_sqrt_per_s"] = C * n * 34 / (t_eval * 1e-6)

    def by_reduce_l1():
        for j in range(32):
            ops.reduce_l1(a + xi[:, j : j + 1] * b, T)

    res["reduce_l1_route_us"] = launch_us(by_reduce_l1, reps=5)
    res["reduce_l1_route_over_eval"] = res["reduce_l1_route_us"] / t_eval
    # the two routes give the same sums
    ref = torch.stack([ops.reduce_l1(a + xi[:, j : j + 1] * b, T) for j in range(32)], dim=1)
    res["max_rel_difference_of_the_routes"] = float(((P[:, :32] - ref).abs() / ref).max())

    quad = ops.as_device(np.tile([1.0, 0.0, 50.0], (C, 1)))
    gamma = (P[:, 32] / LMDA + 1.0 + 0.05 * n).contiguous()
    out = torch.empty((C, 8), dtype=torch.float64, device=dev)
    st = torch.empty(C, dtype=torch.int32, device=dev)
    res["search_10_rounds_us"] = launch_us(lambda: ops.lci_search(a, b, T, quad, LMDA, gamma, rounds=10, out=out, status=st,
                                                                  scratch=scratch), reps=5)
    res["search_status"] = sorted(set(int(v) for v in st.cpu().numpy()))

    X = ops.soft(ops.as_device(op.transform.forward(ops.as_device(data.astype(complex)))), T * 50.0)
    labels = superpixel_regions(L, 16)
    times = []
    for i in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = local_credible_intervals(op, reg, p, X, labels, batch=C)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res["local_credible_intervals_regions"] = int(labels.max()) + 1
    res["local_credible_intervals_s"] = statistics.median(times[1:])
    res["local_credible_intervals_all_s"] = times
    res["local_credible_intervals_status_counts"] = {int(k): int(v) for k, v in zip(*np.unique(r.status, return_counts=True))}
    res["median_range"] = float(np.nanmedian(r.range))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
