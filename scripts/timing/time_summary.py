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
  tails       the exact credible intervals of a run of N = 1000 saves at alpha = 0.05 (k = 26 slots per tail), for the real
              parts (m = 305 060 per chain) and for the complex state (m = 610 120), fresh standard-normal samples:
                fill      one pxm_tails_update in the fill phase (count = k / 2), cold;
                steady    pxm_tails_update at the end of the run, a fresh sample each time, cold: one save that stages its
                          sample in the ring and one that merges the full ring into the heaps; a steady-state save is
                          (15 staging + 1 merging) / 16 of them (B = 16), beside the cold pxm_moments_update of the same
                          layout; algorithmic traffic x + two thresholds = 24 B per element, reported against 8 TB/s;
                readout   one pxm_tails_quantiles (host-timed: it synchronises);
                run       the N saves (device events around every pxm_tails_update, summed) plus the read-out, against
                parent    the route without tails for the same map: one row copy into a device-resident [N, C m] chain
                          per save (events, summed) plus pxm_quantile_range of it at the end (held a ring of rows and four
                          chains at a time, see time_tails: same bytes, bounded device memory).
              A run with tails must not take longer than the route without them: the script exits with an error if one does.
  ess         the streaming effective sample size of a run of N = 1000 saves at K = 32 lags, same two layouts and samples:
                steady    pxm_acov_update at the end of the run, cold: one save that only copies its row into the ring and
                          one that also merges its block of B = 16 into the lagged products; a steady-state save is
                          (15 + 1) / 16 of them, beside the cold pxm_moments_update of the same layout;
                readout   one pxm_acov_ess with the pooled outputs (host-timed: it synchronises);
                run       the N saves (device events around every pxm_acov_update, summed) plus the read-out, against
                parent    the route without the feature: one row copy per save into a device-resident chain (as for the
                          tails) plus, at the end, the same K lagged sums of the mean-centred chain with torch, four chains
                          at a time.
              The same acceptance condition as for the tails.

    python scripts/timing/time_summary.py [--out FILE.json] [--sections moments,tails,ess,iteration]
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
from pxmcmc_amd.uncertainty import PosteriorSummary, tail_capacity  # noqa: E402

L, B, J_MIN, C = 256, 2.0, 2, 16
HBM_RATE = 8e12  # bytes/s
LMDA, DELTA = 1e-6, 1e-7
TAIL_N, TAIL_ALPHA = 1000, 0.05
ESS_N, ESS_LAGS = 1000, 32
PARENT_RING, PARENT_BLOCK = 64, 4  # rows of the copy ring, chains per select of the route without tails (device memory bound)


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


def cold_ms(fn, regions=5, prep=None):
    """median device time of one call whose operands are not in the last-level cache: a 512 MiB copy runs before each
    (and after ``prep``, which readies the call's input)"""
    src = torch.empty(512 << 20, dtype=torch.uint8, device=ops.device())
    dst = torch.empty_like(src)
    times = []
    for _ in range(regions + 1):
        if prep is not None:
            prep()
        dst.copy_(src)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times[1:]), times[1:]


def summed_events_ms(steps, fn):
    """sum over ``steps`` calls fn(i, before, after) of the device time between the two events fn records"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for i, (a, b) in enumerate(pairs):
        fn(i, a, b)
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs)


def time_tails(X, cplx):
    """the ``tails`` block of the module docstring for one layout: ``cplx`` the complex state per component (m = 2 n), else
    the real parts of X (x_stride 2, m = n)"""
    C_, n = X.shape
    m = 2 * n if cplx else n
    N, alpha = TAIL_N, TAIL_ALPHA
    k = tail_capacity(alpha, N)
    B_ = ops.tails_stage_depth()
    dev = X.device
    rows = (lambda: torch.view_as_real(X).reshape(C_, m)) if cplx else (lambda: X)  # what the entry points are handed
    alg = 24 * C_ * m
    out = {"m": m, "k": k, "N": N, "alpha": alpha, "tail_bytes": (2 * k + 2 + B_) * 8 * C_ * m, "chain_bytes": N * 8 * C_ * m,
           "algorithmic_bytes": alg}
    rate = lambda ms: {"ms": ms, "fraction_of_8TBps": alg / (ms * 1e-3) / HBM_RATE}  # noqa: E731

    s = PosteriorSummary(C_, n, cplx, best=False)
    med, times = cold_ms(lambda: s.update(X), prep=X.normal_)
    out["moments_cold"] = dict(rate(med), regions_ms=times)

    count = torch.zeros(C_, dtype=torch.int64, device=dev)
    lo = torch.zeros((C_, k, m), dtype=torch.float64, device=dev)
    hi, thr_lo = torch.zeros_like(lo), torch.zeros((C_, m), dtype=torch.float64, device=dev)
    thr_hi = torch.zeros_like(thr_lo)
    stage = torch.zeros((C_, B_, m), dtype=torch.float64, device=dev)
    save = lambda: ops.tails_update(rows(), count, lo, hi, thr_lo, thr_hi, stage, N)  # noqa: E731
    for _ in range(k // 2):
        X.normal_()
        save()
        count += 1
    med, times = cold_ms(save, prep=X.normal_)  # (count stays: every call refills slot k / 2)
    out["fill_cold"] = dict(rate(med), regions_ms=times)

    def one_save(i, a, b):
        X.normal_()
        a.record()
        save()
        b.record()
        count.add_(1)

    count.zero_()  # the run from its start (the fill phase never reads a slot it has not written in this run)
    run_ms = summed_events_ms(N, one_save)
    assert count.tolist() == [N] * C_
    t0 = time.perf_counter()
    q_lo, q_hi = ops.tails_quantiles(count, lo, hi, stage, N, alpha)
    torch.cuda.synchronize()
    readout_ms = (time.perf_counter() - t0) * 1e3
    out["saves_ms"], out["readout_ms"], out["run_ms"] = run_ms, readout_ms, run_ms + readout_ms
    last_merge = k + (N - k) // B_ * B_ - 1  # the last save of the run that fills the ring
    count.fill_(last_merge - 1)
    med_s, times = cold_ms(save, prep=X.normal_)
    out["stage_cold"] = {"ms": med_s, "regions_ms": times}
    count.fill_(last_merge)
    med_m, times = cold_ms(save, prep=X.normal_)  # (the ring holds fresh samples of the calls before)
    out["merge_cold"] = {"ms": med_m, "regions_ms": times}
    med = ((B_ - 1) * med_s + med_m) / B_
    out["steady_cold"] = rate(med)
    out["steady_over_moments"] = med / out["moments_cold"]["ms"]
    tails_range = (q_hi - q_lo)[0, :4096].clone()
    del lo, hi, thr_lo, thr_hi, stage, q_lo, q_hi, s

    torch.cuda.empty_cache()

    # The route without tails: a row copy into a device-resident chain per save, pxm_quantile_range at the end.  The whole
    # chain is N * 8 * C * m bytes (39 / 78 GB); to bound device memory the N copies go, at their full size, into a ring of
    # PARENT_RING rows (far larger than the last-level cache, so every row is written to HBM as in the chain), and the select
    # runs on the columns of PARENT_BLOCK chains at a time, on fresh samples -- the same bytes and sweeps as on the whole chain.
    ring = torch.empty((PARENT_RING, C_ * m), dtype=torch.float64, device=dev)
    src = (lambda: torch.view_as_real(X).reshape(C_, m)) if cplx else (lambda: X.real)  # (a strided view: one copy kernel)

    def one_copy(i, a, b):
        X.normal_()
        a.record()
        ring[i % PARENT_RING].view(C_, m).copy_(src())
        b.record()

    copies_ms = summed_events_ms(N, one_copy)
    del ring
    torch.cuda.empty_cache()
    assert C_ % PARENT_BLOCK == 0
    chain = torch.empty((N, PARENT_BLOCK * m), dtype=torch.float64, device=dev)
    select_ms = 0.0
    for _ in range(C_ // PARENT_BLOCK):
        chain.normal_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rng = ops.quantile_range(chain, alpha)
        torch.cuda.synchronize()
        select_ms += (time.perf_counter() - t0) * 1e3
    out["parent"] = {"copies_ms": copies_ms, "select_ms": select_ms, "run_ms": copies_ms + select_ms,
                     "select_block_bytes": chain.numel() * 8}
    out["run_over_parent"] = out["run_ms"] / out["parent"]["run_ms"]
    # (different samples in the two routes: only the scale of the two maps is compared)
    out["median_range"] = {"tails": float(tails_range.median()), "parent": float(rng[:4096].median())}
    del chain
    torch.cuda.empty_cache()
    return out


def time_ess(X, cplx):
    """the ``ess`` block of the module docstring for one layout (``cplx`` as for time_tails)"""
    C_, n = X.shape
    m = 2 * n if cplx else n
    N, K = ESS_N, ESS_LAGS
    B_ = ops.acov_stage_depth()
    dev = X.device
    rows = (lambda: torch.view_as_real(X).reshape(C_, m)) if cplx else (lambda: X)
    out = {"m": m, "K": K, "N": N, "ess_bytes": (3 * K + B_) * 8 * C_ * m, "chain_bytes": N * 8 * C_ * m}

    s = PosteriorSummary(C_, n, cplx, best=False)
    med, times = cold_ms(lambda: s.update(X), prep=X.normal_)
    out["moments_cold"] = {"ms": med, "regions_ms": times}
    del s

    count = torch.zeros(C_, dtype=torch.int64, device=dev)
    acc = torch.empty((C_, K, m), dtype=torch.float64, device=dev)
    head, tot = torch.empty_like(acc), torch.empty((C_, m), dtype=torch.float64, device=dev)
    ring = torch.empty((C_, K - 1 + B_, m), dtype=torch.float64, device=dev)
    save = lambda: ops.acov_update(rows(), count, acc, tot, head, ring)  # noqa: E731

    def one_save(i, a, b):
        X.normal_()
        a.record()
        save()
        b.record()
        count.add_(1)

    run_ms = summed_events_ms(N, one_save)
    assert count.tolist() == [N] * C_
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ess, lag, pooled, mcse, stats = ops.acov_ess(count, acc, tot, head, ring)
    torch.cuda.synchronize()
    readout_ms = (time.perf_counter() - t0) * 1e3
    out["saves_ms"], out["readout_ms"], out["run_ms"] = run_ms, readout_ms, run_ms + readout_ms
    st = stats.cpu().numpy()
    out["ess"] = {"min": float(st[0]), "median": float(ess.median()), "nan": int(st[1]), "truncated": int(st[2]),
                  "pooled_median": float(pooled.median()), "mcse_max": float(mcse.max())}
    last_merge = N // B_ * B_ - 1  # the last save of the run that completes a block
    count.fill_(last_merge - 1)
    med_s, times = cold_ms(save, prep=X.normal_)
    out["stage_cold"] = {"ms": med_s, "regions_ms": times}
    count.fill_(last_merge)
    med_m, times = cold_ms(save, prep=X.normal_)
    out["merge_cold"] = {"ms": med_m, "regions_ms": times}
    med = ((B_ - 1) * med_s + med_m) / B_
    out["steady_cold"] = {"ms": med}
    out["steady_over_moments"] = med / out["moments_cold"]["ms"]
    del acc, head, tot, ring, ess, lag, pooled, mcse
    torch.cuda.empty_cache()

    # The route without the feature: the row copies of time_tails, then the K lagged sums of the mean-centred chain with
    # torch, on the columns of PARENT_BLOCK chains at a time (fresh samples: the same bytes and sweeps as on the whole chain).
    copy_ring = torch.empty((PARENT_RING, C_ * m), dtype=torch.float64, device=dev)
    src = (lambda: torch.view_as_real(X).reshape(C_, m)) if cplx else (lambda: X.real)

    def one_copy(i, a, b):
        X.normal_()
        a.record()
        copy_ring[i % PARENT_RING].view(C_, m).copy_(src())
        b.record()

    copies_ms = summed_events_ms(N, one_copy)
    del copy_ring
    torch.cuda.empty_cache()
    assert C_ % PARENT_BLOCK == 0
    chain = torch.empty((N, PARENT_BLOCK * m), dtype=torch.float64, device=dev)
    gamma = torch.empty((K, PARENT_BLOCK * m), dtype=torch.float64, device=dev)
    sums_ms = 0.0
    for _ in range(C_ // PARENT_BLOCK):
        chain.normal_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chain -= chain.mean(dim=0)
        for l in range(K):
            torch.sum(chain[l:] * chain[: N - l], dim=0, out=gamma[l])
        gamma /= N
        torch.cuda.synchronize()
        sums_ms += (time.perf_counter() - t0) * 1e3
    out["parent"] = {"copies_ms": copies_ms, "lagged_sums_ms": sums_ms, "run_ms": copies_ms + sums_ms, "block_bytes": chain.numel() * 8}
    out["run_over_parent"] = out["run_ms"] / out["parent"]["run_ms"]
    del chain, gamma
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="moments,tails,ess,iteration")
    a = ap.parse_args()
    sections = set(a.sections.split(","))
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
    for name, best in (("update", False), ("update_best", True)) if "moments" in sections else ():
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
    for name, timer in (("update_realparts_best", regions_ms), ("update_realparts_best_cold", cold_ms)) if "moments" in sections else ():
        med, times = timer(lambda: s.update(X, logpi=logpi))
        res[name] = {"ms": med, "regions_ms": times, "TBps": nbytes_re / (med * 1e-3) / 1e12,
                     "fraction_of_8TBps": nbytes_re / (med * 1e-3) / HBM_RATE}

    del s
    if "tails" in sections:
        res["tails_realparts"] = time_tails(X, False)
        res["tails_complex"] = time_tails(X, True)
    if "ess" in sections:
        res["ess_realparts"] = time_ess(X, False)
        res["ess_complex"] = time_ess(X, True)

    if "iteration" in sections:
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
                                        for k in ("update_best", "update_best_cold", "update_realparts_best", "update_realparts_best_cold")
                                        if k in res}
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    slower = {k: v["run_over_parent"] for k, v in res.items() if isinstance(v, dict) and v.get("run_over_parent", 0) > 1}
    if slower:  # the acceptance condition of DESIGN.md section 15
        sys.exit("a streaming run takes longer than the route without it: %s" % slower)


if __name__ == "__main__":
    main()
