"""HEALPix ring synthesis at L = 256, nside = 128, 16 chains.

  python scripts/timing/time_healpix.py [--out FILE]  per spin s in {0, 2}: plan-creation time, table bytes, HpxPlan.synthesis
                                                      and synthesis_adjoint beside ShtPlan(256, s).inverse and inverse_adjoint
                                                      in the same process (median of 5 device-synchronised regions after
                                                      warm-up), their ratios; then the MYULA iteration under graph replay on
                                                      WeakLensingHealpix beside the same model on WeakLensing
  python scripts/timing/time_healpix.py --trace S     a few calls of both operators at spin S only (for
                                                      rocprofv3 --kernel-trace --stats: the split by stage)
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
from pxmcmc_amd.mcmc import MYULA, PxMCMCParams  # noqa: E402
from pxmcmc_amd.measurements import WeakLensing, WeakLensingHealpix  # noqa: E402
from pxmcmc_amd.prior import S2_Wavelets_L1  # noqa: E402
from pxmcmc_amd.transforms import SphericalWaveletTransform  # noqa: E402

L, NSIDE, C, B, J_MIN = 256, 128, 16, 2.0, 2
LMDA, DELTA = 5e-7, 1e-6


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


def legendre_bytes(spin):
    """algorithmic bytes of one Legendre-stage launch: the table rows l >= max(|m|, |s|) of every order once per pass of
    8 chains, the f_lm and the ring array once"""
    R, Rp, M = 4 * NSIDE - 1, -(-(4 * NSIDE - 1) // 64) * 64, 2 * L - 1
    orders = range(L) if spin == 0 else range(-(L - 1), L)
    rows = sum(L - max(abs(m), abs(spin)) for m in orders)
    return rows * Rp * 8 * -(-C // 8) + 16 * C * (L * L + R * M)


def operators(spin):
    torch.cuda.synchronize()
    t = time.perf_counter()
    plan = ops.HpxPlan(L, NSIDE, spin, max_chains=C)
    torch.cuda.synchronize()
    create_s = time.perf_counter() - t
    sht = ops.ShtPlan(L, spin, max_chains=C)
    rng = np.random.default_rng(spin)
    flm = rng.normal(size=(C, L * L)) + 1j * rng.normal(size=(C, L * L))
    flm[:, : spin * spin] = 0
    flm = ops.as_device(flm)
    v = ops.as_device(rng.normal(size=(C, plan.npix)) + 1j * rng.normal(size=(C, plan.npix)))
    f = ops.as_device(rng.normal(size=(C, sht.npix)) + 1j * rng.normal(size=(C, sht.npix)))
    res = {"spin": spin, "plan_create_s": create_s, "table_bytes": plan.table_bytes(), "legendre_bytes": legendre_bytes(spin),
           "hpx_synthesis_ms": 1e3 * timed(lambda: plan.synthesis(flm)),
           "hpx_synthesis_adjoint_ms": 1e3 * timed(lambda: plan.synthesis_adjoint(v)),
           "sht_inverse_ms": 1e3 * timed(lambda: sht.inverse(flm)),
           "sht_inverse_adjoint_ms": 1e3 * timed(lambda: sht.inverse_adjoint(f))}
    res["synthesis_over_sht_inverse"] = res["hpx_synthesis_ms"] / res["sht_inverse_ms"]
    res["adjoint_over_sht_inverse_adjoint"] = res["hpx_synthesis_adjoint_ms"] / res["sht_inverse_adjoint_ms"]
    return res


def myula_iteration(healpix, steps=32):
    """seconds per replayed MYULA iteration of the weak-lensing model, the shear read at HEALPix pixels or on the MW grid"""
    rng = np.random.default_rng(0)
    if healpix:
        wl = WeakLensingHealpix(L, NSIDE, ngal=np.full(12 * NSIDE * NSIDE, 30.0), max_chains=C)
    else:
        wl = WeakLensing(L, ngal=np.full((L, 2 * L - 1), 30.0), max_chains=C)
    tr = SphericalWaveletTransform(L, B, J_MIN, max_chains=C)
    data = rng.normal(size=wl.ndata) + 1j * rng.normal(size=wl.ndata)
    op = ForwardOperator(data, 1 / wl.inv_cov, "synthesis", transform=tr, measurement=wl, nparams=tr.ncoefs)
    reg = S2_Wavelets_L1("synthesis", tr.inverse, tr.inverse_adjoint, LMDA, L=L, B=B, J_min=J_MIN)
    p = PxMCMCParams(lmda=LMDA, delta=DELTA, nsamples=1, nburn=0, ngap=1, verbosity=0)
    s = MYULA(op, reg, p, nchains=C, seed=1)
    with contextlib.redirect_stdout(io.StringIO()):
        s._prepare()
        X, preds = s._initial_sample(np.zeros(op.nparams))
        s._engine_start(X, preds, 0)
    try:
        assert s._eng.graph is not None, s._eng.graph_error
        s._engine_advance(8)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            s._engine_advance(steps)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) / steps)
        return statistics.median(ts), bool(s._fused_wav)
    finally:
        s._engine_stop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=None, help="spin: a few calls of both operators only")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.trace is not None:
        plan = ops.HpxPlan(L, NSIDE, a.trace, max_chains=C)
        flm = torch.zeros((C, L * L), dtype=torch.complex128, device=ops.device())
        v = torch.ones((C, plan.npix), dtype=torch.complex128, device=ops.device())
        for _ in range(6):
            plan.synthesis(flm)
            plan.synthesis_adjoint(v)
        torch.cuda.synchronize()
        print(json.dumps({"spin": a.trace, "calls": 6}))
        return
    out = [operators(0), operators(2)]
    for r in out:
        print(json.dumps(r), flush=True)
    hpx, fused_h = myula_iteration(True)
    mw, fused_m = myula_iteration(False)
    it = {"myula_iteration_healpix_ms": 1e3 * hpx, "myula_iteration_mw_ms": 1e3 * mw, "healpix_over_mw": hpx / mw,
          "fused_step_healpix": fused_h, "fused_step_mw": fused_m}
    print(json.dumps(it))
    out.append(it)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
