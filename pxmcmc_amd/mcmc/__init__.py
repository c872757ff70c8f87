"""
Samplers of the reference (pxmcmc/mcmc.py:6-383: PxMCMCParams, PxMCMC, MYULA, PxMALA, SKROCK) driving
the HIP kernels.  The plugin protocol is the reference's: the sampler only touches
``forward.forward / calc_gradg / data / invcov / nparams`` and ``prior.proxf / prior.prior``.

Extensions (all optional, defaults reproduce the reference's one-chain behaviour):

* ``nchains``      -- C independent chains advanced together as one ``[C, N]`` batch;
* ``rng``          -- ``"philox"`` (device counter-based stream keyed (seed, chain, iteration),
  independent of how chains are spread over GPUs) or ``"numpy"`` (the reference's global
  ``np.random`` stream in the reference's draw order, for parity runs);
* ``chain_offset`` -- global index of this process's first chain (multi-GPU sharding);
* ``use_graph``    -- replay the fused iteration from a captured HIP graph (default on);
* ``ring_shortcut`` -- with a scalar ``sig_d`` apply the residual on the ring transforms (default on);
* ``noise_bits``   -- 64 (default) or 32: arithmetic of the Box-Muller step of the device Philox stream.  64 evaluates
  log / sqrt / sincos in double precision (table look-ups + short polynomials, csrc/philox.h) as the reference's
  ``np.random.randn`` does (pxmcmc/mcmc.py:193); 32 runs it on the f32 transcendental units (deviates ~1e-6 relative,
  exact fp64 exponent: tail to 8.5 sigma), ~2 % faster at the benchmark size.  Same Philox counters and uniforms either
  way: the two streams agree to ~1e-6;
* ``real_pairs``   -- with REAL data, a real start point and ``params.complex == False`` the reference's
  complex128 state has a zero imaginary part (every operator of the path maps real fields to real
  fields); the fused wavelet path then carries two real chains per complex slot -- chain 2c in the real
  part, chain 2c+1 in the imaginary part -- through the complex-linear transforms and applies prox and
  noise per component (real-signal symmetry).  Same results, half the transform
  work (default on; complex data, as in the reference-literal topography set-up, is never paired);
* ``summary``      -- ``None`` (default), ``"state"``, ``"image"`` or a tuple of both: accumulate every saved sample into a
  device-resident :class:`uncertainty.PosteriorSummary` per space (per-chain mean and variance, highest-posterior sample,
  R-hat across the batch).  ``"state"`` is the sampled vector as ``chain`` would hold it;
  ``"image"`` is ``transform.inverse`` of it in the synthesis setting and the state itself in the analysis setting.  After
  ``run()`` the summaries are in ``self.summary[space]``.  With ``"chain"`` left out of ``track`` no state is copied to the
  host during the run;
* ``summary_alpha`` -- ``None`` (default) or alpha in (0, 1]; needs ``summary``.  The summaries also keep the
  ``tail_capacity(alpha, nsamples)`` smallest and largest saved samples of every element, and
  ``self.summary[space].credible_interval_range()`` then gives, per chain, the (1 - alpha) credible-interval map the
  reference computes from the saved chain (pxmcmc/uncertainty.py:7-16), exactly;
* ``summary_ess``  -- ``None`` (default) or K, even with 2 <= K <= 64; needs ``summary``.  The summaries also accumulate the
  lagged products of the saved samples at lags below K, and ``self.summary[space].ess()`` then gives the effective sample
  size of every chain and element, ``ess_pooled()`` that of the chain batch and ``mcse()`` the standard error of
  ``pooled_mean()``.  Where ``ess_lag()`` reaches K the value is truncated, an upper bound: raise K or ``ngap``.

SKROCK (pxmcmc/mcmc.py:292-383) follows the published recursion (Pereyra, Vargas-Mieles & Zygalakis 2020), which
differs from the reference's literal code for s >= 2 (see :class:`SKROCK`); it takes the keywords above except
``ring_shortcut`` / ``real_pairs``, which it accepts and ignores.
"""
from .base import PxMCMC
from .engine import Engine, _Counter  # noqa: F401
from .myula import MYULA
from .params import PxMCMCParams
from .pxmala import PxMALA
from .skrock import SKROCK, skrock_coefficients
from .stepper import Stepper

__all__ = ["PxMCMCParams", "Stepper", "PxMCMC", "MYULA", "PxMALA", "SKROCK", "skrock_coefficients", "Engine"]
