"""The layout of the ``pxmcmc_amd.uncertainty`` package: every public name the single module exported before it was split is
still an attribute of the package, the one ``to_map`` of the two region results paints as either did, and
``PosteriorSummary.merge`` treats its groups as it did (a common ``alpha`` is kept and a differing one raises; differing
``ess_lags`` drop the group; a group one dict lacks is dropped)."""
import numpy as np
import pytest

import pxmcmc_amd.uncertainty as uncertainty
from pxmcmc_amd.uncertainty import HypothesisTestResult, LocalCredibleIntervals, PosteriorSummary

# the public names of pxmcmc_amd/uncertainty.py at the commit before the split, read off that file
PUBLIC_NAMES = (
    "credible_interval_range", "wavelet_credible_interval_range", "credible_region_threshold",
    "approx_credible_region_threshold", "in_credible_region", "chain_to_images",
    "moments_np", "pooled_np", "rhat_np", "tail_capacity", "tails_update_np", "tails_quantiles_np",
    "acov_update_np", "acov_gamma_np", "ess_np", "ess_pooled_np", "autocov_np", "PosteriorSummary",
    "LCI_OK", "LCI_EMPTY", "LCI_NONFINITE", "LCI_UNCONSTRAINED", "LCI_POINTS",
    "lci_shrink_factor", "lci_sum_depth", "superpixel_regions", "lci_terms_np", "lci_eval_np", "lci_search_np",
    "map_objective", "LocalCredibleIntervals", "local_credible_intervals",
    "HYP_NONFINITE", "inpaint_sum_depth", "inpaint_step_np", "inpaint_np", "gaussian_smooth", "SurrogateImages",
    "inpaint_regions", "smooth_regions", "HypothesisTestResult", "hypothesis_test",
)


def test_every_public_name_is_still_exported():
    assert len(set(PUBLIC_NAMES)) == 42
    missing = [name for name in PUBLIC_NAMES if not hasattr(uncertainty, name)]
    assert not missing, missing
    assert uncertainty.__file__.endswith("__init__.py")


def _results(labels):
    """one result of either type over three regions, its default field and another one filled"""
    some = np.zeros(3)
    lci = LocalCredibleIntervals(labels, 1.0, **{**dict.fromkeys(LocalCredibleIntervals.FIELDS, some), "range": np.array([0.5, 1.5, 2.5])})
    hyp = HypothesisTestResult(labels, 1.0, np.linspace(0.0, 1.0, 32),
                               **{**dict.fromkeys(HypothesisTestResult.FIELDS, some), "physical": np.array([True, False, True])})
    return (lci, [0.5, 1.5, 2.5]), (hyp, [1.0, 0.0, 1.0])


def test_to_map_paints_the_regions_and_leaves_nan_outside():
    labels = np.array([[0, 1, -1], [2, 2, 0]], dtype=np.int32)
    for res, default in _results(labels):
        for values, want in ((None, default), ([7.0, 8.0, 9.0], [7.0, 8.0, 9.0])):
            m = res.to_map(values)
            assert m.shape == (2, 3) and m.dtype == np.float64
            assert np.array_equal(m, [[want[0], want[1], np.nan], [want[2], want[2], want[0]]], equal_nan=True)
        for bad in (np.zeros(2), np.zeros(4), np.zeros((3, 1))):
            with pytest.raises(ValueError, match="one value per region"):
                res.to_map(bad)
        assert res.threshold == 1.0 and res.labels is labels


def _host(C, alpha=None, ess_lags=None, first=0.0):
    """a hand-made ``to_host()`` dict of C chains and m = 2 components"""
    d = {"count": np.full(C, 5, dtype=np.int64), "mean": first + np.arange(2.0 * C).reshape(C, 2), "m2": np.ones((C, 2)),
         "best": np.zeros((C, 2)), "best_logpi": np.zeros(C)}
    if alpha is not None:
        d.update(alpha=np.float64(alpha), q_lo=np.full((C, 2), -1.0), q_hi=np.full((C, 2), 1.0))
    if ess_lags is not None:
        d.update(ess_lags=np.int64(ess_lags), ess=np.full((C, 2), 4.0), ess_lag=np.full((C, 2), 2, dtype=np.int32))
    return d


def test_merge_keeps_drops_and_refuses_groups():
    moments, tails, ess = PosteriorSummary.FIELDS, PosteriorSummary.TAIL_FIELDS, PosteriorSummary.ESS_FIELDS
    # one common alpha and one common ess_lags: both groups are kept, the chains in rank order
    a, b = _host(2, alpha=0.1, ess_lags=8), _host(3, alpha=0.1, ess_lags=8, first=100.0)
    out = PosteriorSummary.merge([a, b])
    assert list(out) == list(moments + tails + ess)
    assert out["alpha"] == 0.1 and type(out["alpha"]) is np.float64 and out["ess_lags"] == 8 and type(out["ess_lags"]) is np.int64
    for k in moments + tails[1:] + ess[1:]:
        assert np.array_equal(out[k], np.concatenate([a[k], b[k]], axis=0)) and out[k].dtype == a[k].dtype
    # differing alpha raises
    with pytest.raises(ValueError, match="different alpha"):
        PosteriorSummary.merge([a, _host(3, alpha=0.2, ess_lags=8)])
    # differing ess_lags drop the ESS fields without raising; the tails stay
    out = PosteriorSummary.merge([a, _host(3, alpha=0.1, ess_lags=4)])
    assert list(out) == list(moments + tails)
    # a group missing from one dict is dropped, whichever dict lacks it, and so is a single field of the moments
    assert list(PosteriorSummary.merge([a, _host(3, ess_lags=8)])) == list(moments + ess)
    assert list(PosteriorSummary.merge([_host(2, alpha=0.1), b])) == list(moments + tails)
    assert list(PosteriorSummary.merge([_host(2), b])) == list(moments)
    no_best = {k: v for k, v in _host(3).items() if k not in ("best", "best_logpi")}
    assert list(PosteriorSummary.merge([a, no_best])) == ["count", "mean", "m2"]
    # a group that lacks one of its arrays counts as missing; the differing alpha beside it is then not looked at
    partial = {k: v for k, v in _host(3, alpha=0.2, ess_lags=8).items() if k != "q_hi"}
    assert list(PosteriorSummary.merge([a, partial])) == list(moments + ess)
    with pytest.raises(ValueError, match="no summaries"):
        PosteriorSummary.merge([])
