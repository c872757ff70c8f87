"""The parameter object of the samplers (pxmcmc/mcmc.py:6-43)."""


class PxMCMCParams:
    """
    Tuning and runtime parameters (pxmcmc/mcmc.py:6-43).

    :param lmda: prox parameter
    :param delta: Forward-Euler step size
    :param mu: regularisation parameter
    :param s: max order of Chebyshev polynomials: the number of stages of :class:`SKROCK` (unused by MYULA / PxMALA)
    :param nsamples: number of samples to save
    :param nburn: burn-in size
    :param ngap: thinning: iterations between saved samples
    :param complex: ``True`` if the sampled parameters are complex
    :param verbosity: print every ``verbosity`` iterations
    :param track: list of variables to keep track of
    """

    def __init__(
        self,
        lmda=3e-5,
        delta=1e-5,
        s=1,
        mu=1,
        nsamples=int(1e6),
        nburn=int(1e3),
        ngap=int(1e2),
        complex=False,
        verbosity=100,
        track=["logposterior", "L2", "prior", "chain"],
    ):
        self.lmda = lmda
        self.delta = delta
        self.mu = mu
        self.s = s
        self.nsamples = nsamples
        self.nburn = nburn
        self.ngap = ngap
        self.complex = complex
        self.verbosity = verbosity
        self.track = track
