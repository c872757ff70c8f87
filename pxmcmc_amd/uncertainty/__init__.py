"""
Uncertainty quantification, by concern:

* :mod:`.chains` -- the reference's post-run functions on saved chains (pxmcmc/uncertainty.py:7-56): quantile
  credible-interval ranges per parameter and per wavelet scale, the highest-posterior-density threshold and its approximation
  from the MAP point alone, ``chain_to_images``.
* :mod:`.summary` -- :class:`PosteriorSummary`, the streaming summaries a sampler accumulates on the device (DESIGN.md section
  15): moments, R-hat, best sample, exact credible intervals from tails, effective sample size.
* :mod:`.streaming_np` -- the numpy statements of those accumulators.
* :mod:`.regions` -- what the region-wise tools from the MAP point share: scope, objective and level, label contract, the
  path search with its one read-back, the result painted onto the pixels.
* :mod:`.lci` -- local credible intervals and the numpy statements of their sums and search.
* :mod:`.hyp` -- hypothesis tests of image structure: the inpainting and smoothing surrogates, their
  numpy statements, ``hypothesis_test``.
"""
from .._lib import LCI_EMPTY, LCI_NONFINITE, LCI_POINTS, LCI_UNCONSTRAINED
from .chains import (approx_credible_region_threshold, chain_to_images, credible_interval_range, credible_region_threshold,
                     in_credible_region, wavelet_credible_interval_range)
from .hyp import (HYP_NONFINITE, HypothesisTestResult, SurrogateImages, gaussian_smooth, hypothesis_test, inpaint_np,
                  inpaint_regions, inpaint_step_np, inpaint_sum_depth, smooth_regions)
from .lci import (LCI_OK, LocalCredibleIntervals, lci_eval_np, lci_search_np, lci_shrink_factor, lci_sum_depth, lci_terms_np,
                  local_credible_intervals)
from .regions import map_objective, superpixel_regions
from .streaming_np import (acov_gamma_np, acov_update_np, autocov_np, ess_lag_count, ess_np, ess_pooled_np, moments_np,
                           pooled_np, rhat_np, tail_capacity, tails_quantiles_np, tails_update_np)
from .summary import PosteriorSummary

__all__ = [
    "LCI_EMPTY", "LCI_NONFINITE", "LCI_POINTS", "LCI_UNCONSTRAINED", "LCI_OK", "HYP_NONFINITE",
    "credible_interval_range", "wavelet_credible_interval_range", "credible_region_threshold",
    "approx_credible_region_threshold", "in_credible_region", "chain_to_images",
    "moments_np", "pooled_np", "rhat_np", "tail_capacity", "tails_update_np", "tails_quantiles_np", "ess_lag_count",
    "acov_update_np", "acov_gamma_np", "ess_np", "ess_pooled_np", "autocov_np", "PosteriorSummary",
    "superpixel_regions", "map_objective",
    "lci_shrink_factor", "lci_sum_depth", "lci_terms_np", "lci_eval_np", "lci_search_np", "LocalCredibleIntervals",
    "local_credible_intervals",
    "inpaint_sum_depth", "inpaint_step_np", "inpaint_np", "gaussian_smooth", "SurrogateImages", "inpaint_regions",
    "smooth_regions", "HypothesisTestResult", "hypothesis_test",
]
