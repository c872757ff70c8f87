"""
On-disk format of a finished run (pxmcmc/saving.py:5-36): one file whose datasets are
``logposterior, predictions, chain, L2s, priors, acceptances (int8), deltas`` and whose attributes are the
fields of :class:`mcmc.PxMCMCParams` plus any keyword arguments.

The reference writes HDF5 through ``h5py``.  When ``h5py`` is importable this module writes the identical
``<filename>.hdf5``; where it is not (this image), the same datasets go into ``<filename>.npz`` under the same
names, with the attributes as one JSON document in the ``__attrs__`` entry.  ``load_mcmc`` reads either.
"""
import json
import os

import numpy as np

from .uncertainty import PosteriorSummary

_SUMMARY_FIELDS = PosteriorSummary.FIELDS  # the datasets of PosteriorSummary.to_host()
# ... of a summary built with alpha / with ess_lags; the scalar of either group becomes the attribute summary_alpha / summary_ess_lags
_TAIL_FIELDS = tuple(k for k in PosteriorSummary.TAIL_FIELDS if k != "alpha")
_ESS_FIELDS = tuple(k for k in PosteriorSummary.ESS_FIELDS if k != "ess_lags")

_DATASETS = (
    ("logPi", "logposterior", None),
    ("preds", "predictions", None),
    ("chain", "chain", None),
    ("L2s", "L2s", None),
    ("priors", "priors", None),
    ("acceptance_trace", "acceptances", "i1"),
    ("deltas_trace", "deltas", None),
)


def _attr_value(v):
    if isinstance(v, (np.generic,)):
        return v.item()
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (list, tuple)):
        return [_attr_value(x) for x in v]
    if isinstance(v, complex):
        return {"re": v.real, "im": v.imag}
    return v


def _summary_datasets(mcmc):
    """[(name, array)] of a sampler run with ``summary=``: ``summary_<space>_{count,mean,m2,best,best_logpi}`` (the raw
    accumulators, real-component layout; extension -- a run without a summary writes none of them), and with
    ``summary_alpha`` the quantile maps ``summary_<space>_{q_lo,q_hi}``; {"summary_alpha": alpha} then, else {}.  A summary
    whose tails cannot be read out (``PosteriorSummary.to_host`` warns) is written without the maps and the attribute.  With
    ``summary_ess`` the per-chain effective sample sizes ``summary_<space>_{ess,ess_lag}`` and {"summary_ess_lags": K}."""
    out, attrs = [], {}
    for space, summ in (getattr(mcmc, "summary", None) or {}).items():
        host = summ.to_host()
        out += [(f"summary_{space}_{k}", host[k]) for k in _SUMMARY_FIELDS + _TAIL_FIELDS + _ESS_FIELDS if k in host]
        if "alpha" in host:
            attrs["summary_alpha"] = float(host["alpha"])
        if "ess_lags" in host:
            attrs["summary_ess_lags"] = int(host["ess_lags"])
    return out, attrs


def save_mcmc(mcmc, params, outpath, filename="outputs", **kwargs):
    """
    Saves the MCMC run (pxmcmc/saving.py:5-36).  Any variable selected by the sampler's ``track`` option is a
    dataset; runtime parameters and ``**kwargs`` are attributes.  Returns the path written.
    """
    present = [(attr, name, dtype) for attr, name, dtype in _DATASETS if hasattr(mcmc, attr)]
    summaries, summary_attrs = _summary_datasets(mcmc)
    attrs = {k: getattr(params, k) for k in params.__dict__.keys()}
    attrs.update(summary_attrs)
    attrs.update(kwargs)
    try:
        import h5py
    except ImportError:
        h5py = None
    if h5py is not None:  # the reference's calls, one for one (pinned by tests/golden/g13_save_mcmc_format.json)
        path = os.path.join(outpath, f"{filename}.hdf5")
        with h5py.File(path, "w") as f:
            for attr, name, dtype in present:
                if dtype is None:
                    f.create_dataset(name, data=getattr(mcmc, attr))
                else:
                    f.create_dataset(name, data=getattr(mcmc, attr), dtype=dtype)
            for name, arr in summaries:
                f.create_dataset(name, data=arr)
            for k, v in attrs.items():
                f.attrs[k] = v
        return path
    data = {}
    for attr, name, dtype in present:
        arr = np.asarray(getattr(mcmc, attr))
        data[name] = arr.astype(dtype) if dtype else arr
    data.update(summaries)
    path = os.path.join(outpath, f"{filename}.npz")
    np.savez(path, __attrs__=np.array(json.dumps({k: _attr_value(v) for k, v in attrs.items()})), **data)
    return path


def load_summaries(data, attrs=None):
    """the ``summary_*`` datasets of a loaded run -> {space: host dict} as ``PosteriorSummary.to_host()`` returns them;
    with the run's attributes, a space that carries ``q_lo`` / ``q_hi`` also gets its ``alpha`` and one that carries ``ess``
    its ``ess_lags``"""
    out = {}
    for name, arr in data.items():
        if name.startswith("summary_"):
            for k in sorted(_SUMMARY_FIELDS + _TAIL_FIELDS + _ESS_FIELDS, key=len, reverse=True):  # ("best_logpi" before "best")
                if name.endswith("_" + k):
                    out.setdefault(name[len("summary_"):-len(k) - 1], {})[k] = arr
                    break
    if attrs is not None and "summary_alpha" in attrs:
        for host in out.values():
            if "q_lo" in host:
                host["alpha"] = np.float64(attrs["summary_alpha"])
    if attrs is not None and "summary_ess_lags" in attrs:
        for host in out.values():
            if "ess" in host:
                host["ess_lags"] = np.int64(attrs["summary_ess_lags"])
    return out


def load_mcmc(path):
    """Read a file written by :func:`save_mcmc` -> (datasets dict, attributes dict); ``load_summaries(datasets)`` groups the
    ``summary_*`` datasets of a run with ``summary=`` by space."""
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            data = {k: z[k] for k in z.files if k != "__attrs__"}
            attrs = json.loads(str(z["__attrs__"]))
        return data, attrs
    import h5py

    with h5py.File(path, "r") as f:
        return {k: f[k][()] for k in f.keys()}, dict(f.attrs)
