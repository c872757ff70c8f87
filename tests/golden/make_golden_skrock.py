"""
Generate the golden fixture G16 (tests/golden/g16_skrock.npz): seeded trajectories of the REFERENCE's own SKROCK
(pxmcmc/mcmc.py:292-383) at s = 1 on a G5-style identity toy, real and ``complex=True``.  At s = 1 the reference's
recursion equals the published one (the two differ for s >= 2; see pxmcmc_amd.mcmc.SKROCK).

The reference is imported at generation time only, as make_golden.py does; only the data file is committed.

    python tests/golden/make_golden_skrock.py
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402


def main():
    mcmc, forward, measurements, transforms, prior, utils = _import_reference()
    r0 = np.random.default_rng(16)
    N = 128
    truth = r0.normal(size=N)
    data = truth + 0.1 * r0.normal(size=N)
    lmda, delta, mu, nsamples, nburn, ngap = 2e-3, 1e-3, 1.0, 30, 5, 2
    out = {"data": data, "params": np.array([lmda, delta, mu, nsamples, nburn, ngap])}
    for tag, cplx, seed in (("real", False, 161), ("cplx", True, 162)):
        op = forward.ForwardOperator(data, 0.1, "synthesis", transforms.IdentityTransform(), measurements.Identity(N, N),
                                     nparams=N)
        reg = prior.L1("synthesis", None, None, lmda * mu)
        p = mcmc.PxMCMCParams(lmda=lmda, delta=delta, mu=mu, s=1, nsamples=nsamples, nburn=nburn, ngap=ngap, complex=cplx,
                              verbosity=0, track=["logposterior", "L2", "prior", "chain", "predictions"])
        sk = mcmc.SKROCK(op, reg, p)
        X0 = 0.1 * r0.normal(size=N) + (0.1j * r0.normal(size=N) if cplx else 0)
        np.random.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            sk.run(start_point=X0)
        out[f"{tag}_X0"] = X0
        out[f"{tag}_seed"] = np.array(seed)
        out[f"{tag}_chain"] = sk.chain
        out[f"{tag}_logPi"], out[f"{tag}_L2s"], out[f"{tag}_priors"] = sk.logPi, sk.L2s, sk.priors
        out[f"{tag}_preds"] = sk.preds
        out[f"{tag}_coefs"] = np.array([sk.omega_0, sk.omega_1, sk.mus[1], sk.nus[1], sk.ks[1]])
    np.savez_compressed(os.path.join(HERE, "g16_skrock.npz"), **out)


if __name__ == "__main__":
    main()
