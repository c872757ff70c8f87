"""Total variation on the MW grid at L = 256 and L = 512 with 16 chains, real and complex images.

  python scripts/timing/time_tv.py [--out FILE] [--L 256 512]
      the six launches of csrc/tv.hip alone (device time from events around back-to-back calls, median of 5 such regions),
      their algorithmic bytes with neighbour reads counted once and the fraction of 8 TB/s those bytes reach; the composed
      pairs the two fused steps replace, timed the same way; and one replayed iteration of optim.PrimalDual with prior.TV_S2,
      fused and composed in the same session (median of 5 device-synchronised regions after warm-up)
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
from pxmcmc_amd.mcmc import PxMCMCParams  # noqa: E402
from pxmcmc_amd.measurements import Identity  # noqa: E402
from pxmcmc_amd.optim import PrimalDual  # noqa: E402
from pxmcmc_amd.prior import TV_S2  # noqa: E402
from pxmcmc_amd.transforms import IdentityTransform  # noqa: E402

C = 16
PEAK = 8.0e12  # HBM peak of the MI355X, bytes/s
LMDA, SIG, T_TV = 1.0, 0.3, 40.0


def launch_us(fn, reps=50, regions=5):
    """device time of one call: the median over `regions` regions of `reps` back-to-back calls between two events (after 3
    warm-up calls) -> (median, the regions' values)"""
    for _ in range(3):
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


def iteration_us(s, iters=64, regions=5):
    s._engine_advance(2 * iters)  # warm-up
    times = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s._engine_advance(iters)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / iters * 1e6)
    return statistics.median(times), times


def one_size(L, cplx):
    dev = ops.device()
    dt = torch.complex128 if cplx else torch.float64
    e = 16 if cplx else 8  # bytes per element
    m = L * (2 * L - 1)
    ab = ops.tv_ring_coefs(L)
    X, G, Xbar = (torch.randn(C, m, dtype=dt, device=dev) for _ in range(3))
    V, W = (torch.randn(C, 2 * m, dtype=dt, device=dev) for _ in range(2))
    X1, Xb1, U = torch.empty_like(X), torch.empty_like(X), torch.empty_like(X)
    V1 = torch.empty_like(V)
    T = torch.rand(m, dtype=torch.float64, device=dev) + 0.5
    ps = torch.empty((C, 2), dtype=torch.float64, device=dev)
    ds = torch.empty((C, 3), dtype=torch.float64, device=dev)
    val = torch.empty(C, dtype=torch.float64, device=dev)
    scratch = ops.pd_scratch(C, dev)
    tau, sigma, rscale = 0.05, 0.7, 1.0
    timed = {
        "tv_grad": launch_us(lambda: ops.tv_grad(X, ab, out=W)),
        "tv_grad_adjoint": launch_us(lambda: ops.tv_grad_adjoint(V, ab, out=U)),
        "tv_value": launch_us(lambda: ops.tv_value(X, ab, T, out=val, scratch=scratch)),
        "pd_dual_step_pairs": launch_us(lambda: ops.pd_dual_step_pairs(V, W, T, sigma, rscale, out=V1, sums=ds, scratch=scratch)),
        "tv_primal_step": launch_us(lambda: ops.tv_primal_step(X, G, V, ab, tau, out=(X1, Xb1), sums=ps, scratch=scratch)),
        "tv_dual_step": launch_us(lambda: ops.tv_dual_step(V, Xbar, ab, T, sigma, rscale, out=V1, sums=ds, scratch=scratch)),
        "pd_primal_step": launch_us(lambda: ops.pd_primal_step(X, G, U, tau, out=(X1, Xb1), sums=ps, scratch=scratch)),
    }
    t = {k: v[0] for k, v in timed.items()}
    # algorithmic bytes per launch, all chains, a neighbour read counted once; the vector T is shared by the chains
    px = C * m * e
    nbytes = {
        "tv_grad": 3 * px, "tv_grad_adjoint": 3 * px, "tv_value": px + m * 8, "pd_dual_step_pairs": 6 * px + m * 8,
        "tv_primal_step": 6 * px, "tv_dual_step": 5 * px + m * 8, "pd_primal_step": 5 * px,
    }
    res = {"L": L, "complex": cplx, "chains": C, "npix": m, "launch_us": t, "launch_us_regions": {k: v[1] for k, v in timed.items()},
           "bytes": nbytes, "bytes_per_pixel": {k: v / (C * m) for k, v in nbytes.items()},
           "fraction_of_8TBps": {k: nbytes[k] / (t[k] * 1e-6) / PEAK for k in nbytes}}
    res["composed_us"] = {"primal": t["tv_grad_adjoint"] + t["pd_primal_step"], "dual": t["tv_grad"] + t["pd_dual_step_pairs"]}
    res["fused_speedup"] = {"primal": res["composed_us"]["primal"] / t["tv_primal_step"],
                            "dual": res["composed_us"]["dual"] / t["tv_dual_step"]}

    # one replayed iteration of PrimalDual, fused and composed
    rng = np.random.default_rng(0)
    data = rng.normal(size=m) + (1j * rng.normal(size=m) if cplx else 0)
    op = ForwardOperator(data, SIG, "analysis", IdentityTransform(), Identity(m, m), nparams=m)
    reg = TV_S2(L, T_TV)
    prm = PxMCMCParams(lmda=LMDA, mu=1.0, verbosity=0, complex=cplx)
    steps = None
    for name, fused in (("fused", True), ("composed", False)):
        kw = {} if steps is None else dict(tau=steps[0], sigma=steps[1])
        s = PrimalDual(op, reg, prm, nchains=C, max_iter=1 << 20, fused=fused, **kw)
        steps = (s.tau, s.sigma)
        with contextlib.redirect_stdout(io.StringIO()):
            Xs, preds = s._initial_sample(np.zeros(m, dtype=data.dtype))
        s._engine_start(Xs, preds, 0)
        assert s._eng.graph is not None, s._eng.graph_error
        med, regions = iteration_us(s)
        s._engine_stop()
        res["iteration_us_" + name] = {"median": med, "regions": regions}
    res["A_norm2"], res["tau"], res["sigma"] = s.A_norm2, s.tau, s.sigma
    res["iteration_speedup"] = res["iteration_us_composed"]["median"] / res["iteration_us_fused"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--L", type=int, nargs="+", default=[256, 512])
    a = ap.parse_args()
    res = {"runs": [one_size(L, cplx) for L in a.L for cplx in (False, True)]}
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
