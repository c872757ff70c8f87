"""The refusals of ``pxmcmc_amd.ops``: one row per ``raise`` a caller can reach -- the call, the exception class and the
fixed words of the message (anchored at the ``name:`` prefix where there is one).  The classes are mixed for historical
reasons (ValueError, TypeError, AssertionError); callers match on them, so they are pinned as they are.  Every call is refused
on the host before a kernel is launched; the shapes are the smallest the checks need."""
from types import SimpleNamespace

import pytest

pytestmark = pytest.mark.gpu

C, N = 2, 8  # chains, elements of the array wrappers
M, K_TAIL, K_LAGS = 8, 3, 4  # the summary families


@pytest.fixture(scope="module")
def g():
    import scipy.sparse as sp
    import torch

    from pxmcmc_amd import _lib, ops
    from pxmcmc_amd.ops import _p

    dev = ops.device()
    g = SimpleNamespace(ops=ops, torch=torch, dev=dev)
    g.r = lambda *shape, dtype=torch.float64: torch.ones(shape, dtype=dtype, device=dev)
    g.c = lambda *shape: torch.ones(shape, dtype=torch.complex128, device=dev)
    g.i = lambda *shape, dtype=torch.int64: torch.zeros(shape, dtype=dtype, device=dev)
    g.x = g.r(C, N)
    g.strided = g.r(C, 2 * M)[:, ::2]
    g.off = g.r(C * M + 2)[1:1 + C * M].view(C, M)
    assert not g.strided.is_contiguous() and g.off.is_contiguous() and g.off.data_ptr() % 16 == 8
    g.beta, g.mi = g.r(4), g.i(C)
    g.theta, g.eta, g.rho = g.r(C), g.r(C), g.r(4)
    g.xi = g.r(C, ops.LCI_POINTS)
    Bt, Ba = ops.tails_stage_depth(), ops.acov_stage_depth()
    g.count = g.i(C)
    g.moments = dict(count=g.count, mean=g.r(C, M), m2=g.r(C, M))
    g.tails = dict(count=g.count, lo=g.r(C, K_TAIL, M), hi=g.r(C, K_TAIL, M), thr_lo=g.r(C, M), thr_hi=g.r(C, M),
                   stage=g.r(C, Bt, M), nsamples=100)
    g.acov = dict(count=g.count, acc=g.r(C, K_LAGS, M), tot=g.r(C, M), head=g.r(C, K_LAGS, M), ring=g.r(C, K_LAGS - 1 + Ba, M))
    g.acov_of = lambda K, m: dict(count=g.count, acc=g.r(C, K, m), tot=g.r(C, m), head=g.r(C, K, m), ring=g.r(C, K - 1 + Ba, m))
    g.csr = ops.CsrMatrix(sp.identity(4, format="csr"))
    g.sht = ops.ShtPlan(8, max_chains=C)
    g.wav = ops.WavPlan(16, 2, 2, max_chains=C)
    g.wav.wl_attach(None, None, g.wav.npix)
    g.hwav = ops.HarmWavPlan(16, 2, 2, max_chains=C)
    g.dft = ops.DftPlan(8, max_chains=C)  # images [c, 8, 15], ring array [15, 16, 8]
    g.G = g.dft.ring_array()
    g.dft_abi = lambda name, a, b, n: ops.check(getattr(_lib.lib, name)(g.dft._h, _p(a), _p(b), n, None))
    g.lib, g.p = _lib.lib, _p
    g.gemm = ops.GemmPlan([dict(kind="inv", bl=8)], max_chains=C)  # workspace: counter block, operand, result, scratch rows
    g.gemm_pk = ops.GemmPlan([dict(kind="fwd", bl=8)], max_chains=1, pk=2)
    g.gemm_abi = lambda name, *a: ops.check(getattr(_lib.lib, name)(*a))
    g.X = g.c(C, g.wav.ncoefs)
    g.img, g.w_img = g.c(g.wav.npix), g.r(g.wav.npix)
    g.XH = g.c(C, g.hwav.ncoefs)
    g.lm, g.w_lm = g.c(g.hwav.nlm), g.r(g.hwav.nlm)
    yield g
    torch.cuda.synchronize()


def _fista(g, fn, **kw):
    a = dict(Y=g.x, gradg=g.x, X_prev=g.x, gamma=0.5, lmda=1.0, beta=g.beta, T=0.1)
    if fn == "fista_step_restart":
        a["momentum_index"] = g.mi
    a.update(kw)
    return getattr(g.ops, fn)(**a)


def _sapg(g, **kw):
    a = dict(X=g.x, gradg=g.x, T=0.1, delta=0.1, lmda=1.0, theta=g.theta, eta=g.eta, d=float(N), rho=g.rho, eta_min=-5.0,
             eta_max=5.0)
    a.update(kw)
    return g.ops.sapg_step(**a)


def _update(g, family, **kw):
    a = dict({"moments": g.moments, "tails": g.tails, "acov": g.acov}[family], X=g.r(C, M))
    a.update(kw)
    return getattr(g.ops, family + "_update")(**a)


def _propose(g, **kw):
    a = dict(X=g.x, proxf=None, gradg=g.x, T=0.1, prior_weights=None, delta_dev=g.r(C), lmda=1.0, Xp=g.r(C, N), proxf_p=None,
             lt_out=None, prior_out=None, scratch=g.ops.pxmala_propose_scratch(C, g.dev))
    a.update(kw)
    return g.ops.pxmala_propose(**a)


def _finish(g, **kw):
    rs = g.ops.reduce_scratch_doubles(C)
    a = dict(Xp=g.x, X=g.r(C, N), proxf_p=None, gradg_p=g.r(C, N), preds_p=g.r(C, N), data=g.r(N), invcov=g.r(N),
             propose_scratch=g.r(4 * rs), mu=1.0, lmda=1.0, logpi_c=g.r(C), L2_c=g.r(C), prior_c=g.r(C),
             accept=g.i(C, dtype=g.torch.int32), delta_dev=g.r(C), tune=False, lt_pc_out=g.c(C), lt_cp_out=g.c(C), prior_p_out=g.r(C),
             L2_p_out=g.r(C), scratch=g.r(2 * rs), T=0.1)
    a.update(kw)
    return g.ops.pxmala_finish(**a)


def _step_args(g):
    return dict(T=0.1, delta=0.1, lmda=1.0)


DFT_P = 8 * 15  # pixels of an image of g.dft


def _dft_ex(g, to_rings=True, **kw):
    """pxm_dft_px2ring_ex / pxm_dft_ring2px_ex on g.dft with arguments that are in order but for ``kw``"""
    a = dict(f=g.c(C, DFT_P), chain_stride=DFT_P, ring0=0, data=None, invcov=None, gidx=None, gw=None, ndata=0, G=g.G, ncol=16, C=C)
    a.update(kw)
    p = g.p
    px = (a["chain_stride"], a["ring0"], p(a["data"]), p(a["invcov"]), 0, p(a["gidx"]), p(a["gw"]), a["ndata"])
    if to_rings:
        return g.ops.check(g.lib.pxm_dft_px2ring_ex(g.dft._h, p(a["f"]), *px, p(a["G"]), a["ncol"], a["C"], None))
    return g.ops.check(g.lib.pxm_dft_ring2px_ex(g.dft._h, p(a["G"]), a["ncol"], p(a["f"]), *px, a["C"], None))


def _gidx(g, value=0, n=DFT_P):
    return g.i(n, dtype=g.torch.int32) + value


V, T_, A = ValueError, TypeError, AssertionError

ROWS = [
    # ---- steps ----
    ("batched-3d", lambda g: g.ops.soft(g.r(2, 2, 2), 0.1), V, r"^expected a 1-D \(single chain\) or 2-D \(chain batch\) array"),
    ("vecT-length", lambda g: g.ops.soft(g.x, g.r(N + 1)), V, r"^threshold / weight vector has the wrong length"),
    ("residual_grad-complex-invcov", lambda g: g.ops.residual_grad(g.x, g.r(N), g.c(N)), T_,
     r"^complex inverse covariance needs complex predictions"),
    ("residual_grad-data-length", lambda g: g.ops.residual_grad(g.x, g.r(N + 1), g.r(N)), V, r"^data / invcov length mismatch"),
    ("residual_grad-invcov-length", lambda g: g.ops.residual_grad(g.x, g.r(N), g.r(N + 1)), V, r"^data / invcov length mismatch"),
    ("myula_step-gradg", lambda g: g.ops.myula_step(g.x, g.r(C, N + 1), 0.1, 0.1, 1.0), V, r"^gradg shape mismatch"),
    ("myula_step-noise-shape", lambda g: g.ops.myula_step(g.x, g.x, 0.1, 0.1, 1.0, noise=g.r(C, N + 1)), V,
     r"^injected noise must have the state's shape"),
    ("myula_step-noise-complex", lambda g: g.ops.myula_step(g.x, g.x, 0.1, 0.1, 1.0, noise=g.c(C, N)), T_,
     r"^complex noise needs a complex state"),
    ("myula_step-delta", lambda g: g.ops.myula_step(g.x, g.x, 0.1, g.r(C + 1), 1.0), V,
     r"^per-chain delta must have one entry per chain"),
    ("myula_step-out-dtype", lambda g: g.ops.myula_step(g.x, g.x, 0.1, 0.1, 1.0, out=g.r(C, N, dtype=g.torch.float32)), V,
     r"^out must be a contiguous device array of the state's shape and dtype"),
    ("myula_step-out-strided", lambda g: g.ops.myula_step(g.x, g.x, 0.1, 0.1, 1.0, out=g.r(C, 2 * N)[:, ::2]), V,
     r"^out must be a contiguous device array of the state's shape and dtype"),
    ("chain_step-proxf", lambda g: g.ops.chain_step(g.x, g.r(C, N + 1), g.x, 0.1, 1.0), V, r"^shape mismatch"),
    ("chain_step-gradg", lambda g: g.ops.chain_step(g.x, g.x, g.r(C + 1, N), 0.1, 1.0), V, r"^shape mismatch"),
    ("chain_step-out", lambda g: g.ops.chain_step(g.x, g.x, g.x, 0.1, 1.0, out=g.r(C, N + 1)), V, r"^out must be a contiguous device array"),
    ("skrock_stage-V", lambda g: g.ops.skrock_stage(g.x, 1.0, V=g.r(C, N + 1)), V,
     r"^skrock_stage: proxf / gradg / V must have the state's shape"),
    ("skrock_stage-proxf", lambda g: g.ops.skrock_stage(g.x, 1.0, b=1.0, proxf=g.r(C, N + 1)), V,
     r"^skrock_stage: proxf / gradg / V must have the state's shape"),
    ("skrock_stage-no-prox", lambda g: g.ops.skrock_stage(g.x, 1.0, b=1.0), V, r"^skrock_stage: a prox term needs proxf or the threshold T"),
    ("skrock_stage-noise", lambda g: g.ops.skrock_stage(g.x, 1.0, r=1.0, noise=g.r(C, N + 1)), V,
     r"^injected noise must have the state's shape"),
    ("box_muller-lengths", lambda g: g.ops.box_muller(g.r(4), g.r(5)), V, r"^box_muller: u1 and u2 must have the same length"),
    # ---- SAPG ----
    ("sapg_step-gradg", lambda g: _sapg(g, gradg=g.r(C, N + 1)), V, r"^sapg_step: gradg shape mismatch"),
    ("sapg_step-delta", lambda g: _sapg(g, delta=g.r(C)), V, r"^sapg_step: delta must be a float \(no per-chain step sizes\)"),
    ("sapg_step-theta-dtype", lambda g: _sapg(g, theta=g.r(C, dtype=g.torch.float32)), V,
     r"^sapg_step: theta must be a contiguous float64 \[C\] device vector"),
    ("sapg_step-theta-length", lambda g: _sapg(g, theta=g.r(C + 1)), V, r"^sapg_step: theta must be a contiguous float64 \[C\] device vector"),
    ("sapg_step-eta-length", lambda g: _sapg(g, eta=g.r(C + 1)), V, r"^sapg_step: eta must be a contiguous float64 \[C\] device vector"),
    ("sapg_step-rho-empty", lambda g: _sapg(g, rho=g.r(0)), V, r"^sapg_step: rho must be a non-empty contiguous float64 device vector"),
    ("sapg_step-trace", lambda g: _sapg(g, trace=g.r(5, C, 2)), V,
     r"^sapg_step: trace must be a contiguous float64 \[n_trace, C, 3\] device array"),
    ("sapg_step-out", lambda g: _sapg(g, out=g.r(C, N + 1)), V, r"^out must be a contiguous device array"),
    ("sapg_step-scratch", lambda g: _sapg(g, scratch=g.r(1)), V, r"^sapg_step: scratch is too small \(sapg_scratch\)"),
    # ---- local credible intervals ----
    ("lci_eval-pair", lambda g: g.ops.lci_eval(g.x, g.r(C, N + 1), 0.1, g.xi), V,
     r"^lci_eval: the two arrays must share one non-empty \[C, n\] shape"),
    ("lci_search-pair", lambda g: g.ops.lci_search(g.x, g.r(C + 1, N), 0.1, g.r(C, 3), 1.0, g.r(C)), V,
     r"^lci_search: the two arrays must share one non-empty \[C, n\] shape"),
    ("lci_data_terms-pair", lambda g: g.ops.lci_data_terms(g.r(C, 0), g.r(C, 0), g.r(0), g.r(0)), V,
     r"^lci_data_terms: the two arrays must share one non-empty \[C, n\] shape"),
    ("lci_eval-xi", lambda g: g.ops.lci_eval(g.x, g.x, 0.1, g.r(C, 31)), T_,
     r"^lci_eval: xi must be a contiguous float64 \[C, 32\] device tensor"),
    ("lci_eval-out", lambda g: g.ops.lci_eval(g.x, g.x, 0.1, g.xi, out=g.r(C, 32)), T_,
     r"^lci_eval: out must be a contiguous float64 \[C, 34\] device tensor"),
    ("lci_eval-scratch", lambda g: g.ops.lci_eval(g.x, g.x, 0.1, g.xi, scratch=g.r(1)), V, r"^lci_eval: scratch is too small \(lci_scratch\)"),
    ("lci_data_terms-out", lambda g: g.ops.lci_data_terms(g.x, g.x, g.r(N), g.r(N), out=g.r(C, 4)), T_,
     r"^lci_data_terms: out must be a contiguous float64 \[C, 3\] device tensor"),
    ("lci_data_terms-data", lambda g: g.ops.lci_data_terms(g.x, g.x, g.r(N + 1), g.r(N)), V, r"^lci_data_terms: data / w length mismatch"),
    ("lci_data_terms-w", lambda g: g.ops.lci_data_terms(g.x, g.x, g.r(N), g.r(N + 1)), V, r"^lci_data_terms: data / w length mismatch"),
    ("lci_data_terms-scratch", lambda g: g.ops.lci_data_terms(g.x, g.x, g.r(N), g.r(N), scratch=g.r(1)), V,
     r"^lci_data_terms: scratch is too small \(lci_scratch\)"),
    ("lci_search-quad", lambda g: g.ops.lci_search(g.x, g.x, 0.1, g.r(C, 2), 1.0, g.r(C)), T_,
     r"^lci_search: quad \[C, 3\] and gamma \[C\] must be contiguous float64 device tensors"),
    ("lci_search-gamma", lambda g: g.ops.lci_search(g.x, g.x, 0.1, g.r(C, 3), 1.0, g.r(C + 1)), T_,
     r"^lci_search: quad \[C, 3\] and gamma \[C\] must be contiguous float64 device tensors"),
    ("lci_search-out", lambda g: g.ops.lci_search(g.x, g.x, 0.1, g.r(C, 3), 1.0, g.r(C), out=g.r(C, 7)), T_,
     r"^lci_search: out float64 \[C, 8\] and status int32 \[C\] must be contiguous device tensors"),
    ("lci_search-status", lambda g: g.ops.lci_search(g.x, g.x, 0.1, g.r(C, 3), 1.0, g.r(C), status=g.i(C)), T_,
     r"^lci_search: out float64 \[C, 8\] and status int32 \[C\] must be contiguous device tensors"),
    ("lci_search-scratch", lambda g: g.ops.lci_search(g.x, g.x, 0.1, g.r(C, 3), 1.0, g.r(C), scratch=g.r(1)), V,
     r"^lci_search: scratch is too small \(lci_scratch\)"),
    # ---- reductions ----
    ("reduce_l1-weight", lambda g: g.ops.reduce_l1(g.x, g.r(N + 1)), V, r"^weight length mismatch"),
    ("reduce_l2-data", lambda g: g.ops.reduce_l2(g.x, g.r(N + 1), g.r(N)), V, r"^data / invcov length mismatch"),
    ("reduce_l2-invcov", lambda g: g.ops.reduce_l2(g.x, g.r(N), g.r(N + 1)), V, r"^data / invcov length mismatch"),
    ("reduce_l2-complex-invcov", lambda g: g.ops.reduce_l2(g.x, g.r(N), g.c(N)), T_, r"^complex inverse covariance needs complex predictions"),
    ("reduce_vdot-shape", lambda g: g.ops.reduce_vdot(g.x, g.r(C, N + 1)), V, r"^vdot: shape mismatch"),
    ("quantile_range-1d", lambda g: g.ops.quantile_range(g.r(N)), T_, r"^quantile_range: a float64 \[nsamples, nparams\] array is expected"),
    ("quantile_range-float32", lambda g: g.ops.quantile_range(g.r(4, N, dtype=g.torch.float32)), T_,
     r"^quantile_range: a float64 \[nsamples, nparams\] array is expected"),
    # ---- streaming summaries ----
    *[(f"{fam}_update-X-{what}", lambda g, fam=fam, what=what: _update(g, fam, X=getattr(g, what)), T_,
       rf"^{fam}_update: X must be a contiguous 16-byte aligned float64 or complex128 \[{C}, {M}\] device tensor")
      for fam in ("moments", "tails", "acov") for what in ("strided", "off")],
    *[(f"{fam}_update-mask", lambda g, fam=fam: _update(g, fam, mask=g.i(C)), T_,
       rf"^{fam}_update: mask must be a contiguous int32 \[C\] device tensor") for fam in ("moments", "tails", "acov")],
    *[(f"{fam}_update-count", lambda g, fam=fam: _update(g, fam, count=g.i(C, dtype=g.torch.int32)), T_, rf"^{fam}_update: count int64 \[C\], ")
      for fam in ("moments", "tails", "acov")],
    ("moments_update-logpi-alone", lambda g: _update(g, "moments", logpi=g.r(C)), V,
     r"^moments_update: logpi, best_logpi and best_x are given together"),
    ("moments_update-best-alone", lambda g: _update(g, "moments", best_logpi=g.r(C), best_x=g.r(C, M)), V,
     r"^moments_update: logpi, best_logpi and best_x are given together"),
    ("moments_update-logpi-dtype", lambda g: _update(g, "moments", logpi=g.r(C, dtype=g.torch.float32), best_logpi=g.r(C), best_x=g.r(C, M)),
     T_, r"^moments_update: logpi must be a contiguous float64 or complex128 \[C\] device tensor"),
    ("moments_update-best_x", lambda g: _update(g, "moments", logpi=g.r(C), best_logpi=g.r(C), best_x=g.r(C, M + 1)), T_,
     r"^moments_update: best_logpi float64 \[C\] and best_x contiguous float64 \[C, m\] are expected"),
    ("moments_finalize-mean-1d", lambda g: g.ops.moments_finalize(g.count, g.r(M), g.r(M)), T_,
     r"^moments_finalize: mean must be a float64 \[C, m\] device tensor"),
    ("moments_finalize-m2", lambda g: g.ops.moments_finalize(g.count, g.r(C, M), g.r(C, M + 1)), T_, r"^moments_finalize: count int64 \[C\], "),
    ("tails_update-lo-2d", lambda g: _update(g, "tails", lo=g.r(C, M)), T_, r"^tails_update: lo must be a float64 \[C, k, m\] device tensor"),
    ("tails_update-k", lambda g: _update(g, "tails", lo=g.r(C, 0, M), hi=g.r(C, 0, M)), V, rf"^tails_update: bad tail shape \[{C}, 0, {M}\]"),
    ("tails_quantiles-hi", lambda g: g.ops.tails_quantiles(g.count, g.tails["lo"], g.r(C, K_TAIL + 1, M), g.tails["stage"], 100, 0.05), T_,
     r"^tails_quantiles: count int64 \[C\], "),
    ("acov_update-acc-2d", lambda g: _update(g, "acov", acc=g.r(C, M)), T_, r"^acov_update: acc must be a float64 \[C, K, m\] device tensor"),
    ("acov_update-K-odd", lambda g: _update(g, "acov", **g.acov_of(3, M)), V, r"^acov_update: K must be even with 2 <= K <= 64, got 3"),
    ("acov_update-m", lambda g: _update(g, "acov", **g.acov_of(K_LAGS, 0)), V, rf"^acov_update: bad state shape \[{C}, {K_LAGS}, 0\]"),
    ("acov_ess-ring", lambda g: g.ops.acov_ess(**dict(g.acov, ring=g.r(C, K_LAGS, M))), T_, r"^acov_ess: count int64 \[C\], "),
    # ---- PxMALA ----
    ("pxmala_propose-proxf-alone", lambda g: _propose(g, proxf=g.x), V,
     r"^pxmala_propose: proxf and proxf_p are given together or not at all"),
    ("pxmala_propose-no-scratch", lambda g: _propose(g, scratch=None), V,
     r"^pxmala_propose: deferred totals need lt_out = prior_out = None and a caller-owned scratch"),
    ("pxmala_propose-lt-alone", lambda g: _propose(g, lt_out=g.c(C)), V,
     r"^pxmala_propose: deferred totals need lt_out = prior_out = None and a caller-owned scratch"),
    ("pxmala_propose-float32", lambda g: _propose(g, X=g.r(C, N, dtype=g.torch.float32)), T_,
     r"^unsupported dtype torch.float32: float64 or complex128 only"),
    ("pxmala_finish-no-T", lambda g: _finish(g, T=None), V, r"^pxmala_finish: without proxf_p the threshold T is needed"),
    ("pxmala_finish-data-dtype", lambda g: _finish(g, data=g.c(N)), V, r"^pxmala_finish: data / invcov do not match the predictions"),
    ("pxmala_finish-invcov-length", lambda g: _finish(g, invcov=g.r(N + 1)), V, r"^pxmala_finish: data / invcov do not match the predictions"),
    ("pxmala_finish-state", lambda g: _finish(g, X=g.r(C, N + 1)), V, r"^pxmala_finish: state arrays must share shape, dtype and be contiguous"),
    # ---- select_copy_many ----
    ("select_copy_many-0", lambda g: g.ops.select_copy_many(g.i(C, dtype=g.torch.int32), []), V, r"^select_copy_many takes 1 to 4 array pairs"),
    ("select_copy_many-5", lambda g: g.ops.select_copy_many(g.i(C, dtype=g.torch.int32), [(g.x, g.r(C, N))] * 5), V,
     r"^select_copy_many takes 1 to 4 array pairs"),
    ("select_copy_many-flag", lambda g: g.ops.select_copy_many(g.i(C), [(g.x, g.r(C, N))]), V,
     r"^select_copy_many: flag must be a contiguous int32 \[C\] array"),
    ("select_copy_many-dtype", lambda g: g.ops.select_copy_many(g.i(C, dtype=g.torch.int32), [(g.x, g.c(C, N))]), V,
     r"^select_copy_many: shape / dtype / layout mismatch"),
    ("select_copy_many-axis", lambda g: g.ops.select_copy_many(g.i(C, dtype=g.torch.int32), [(g.r(3, N), g.r(3, N))]), V,
     rf"^select_copy_many: with {C} chains every array must be \[{C}, \.\.\.\], got \(3, {N}\)"),
    # ---- sparse, status ----
    ("csr-matvec-length", lambda g: g.csr.matvec(g.r(5)), A, r"^expected length 4, got 5"),
    ("raise_on_status", lambda g: g.ops.raise_on_status(2, "plan"), "PxmError", r"^plan: device status 0x2: a wave-pair wait"),
    # ---- plans ----
    ("plan-length", lambda g: g.sht.inverse(g.c(5)), A, r"^expected length 64, got 5"),
    ("plan-chains", lambda g: g.sht.inverse(g.c(C + 1, 64)), V, r"^more chains than the plan was created for"),
    ("plan-out", lambda g: g.wav.synthesis(g.X, out=g.c(C, 3)), V, r"^out= buffer has the wrong shape / dtype / layout"),
    ("dft-image-shape", lambda g: g.dft.rings(g.c(C, 8, 16)), V, r"^rings: the image must be \[C, 8, 15\]"),
    ("dft-image-flat", lambda g: g.dft.rings_raw(g.c(C, 8 * 15), g.G), V, r"^rings_raw: the image must be \[C, 8, 15\]"),
    ("dft-rings-shape", lambda g: g.dft.pixels(g.c(C, 9, 15)), V, r"^pixels: the image must be \[C, 8, 15\]"),
    ("dft-image-chains", lambda g: g.dft.rings(g.c(C + 1, 8, 15)), V, r"^more chains than the plan was created for"),
    ("dft-pixels_raw-chains", lambda g: g.dft.pixels_raw(g.G, C + 1), V, r"^more chains than the plan was created for"),
    ("dft-pixels_raw-no-chain", lambda g: g.dft.pixels_raw(g.G, 0), V, r"^more chains than the plan was created for"),
    ("dft-G-none", lambda g: g.dft.rings_raw(g.c(C, 8, 15), None), T_,
     r"^rings_raw: G must be a contiguous complex128 \[15, 16, 8\] device tensor"),
    ("dft-G-dtype", lambda g: g.dft.rings_raw(g.c(C, 8, 15), g.r(15, 16, 8)), T_,
     r"^rings_raw: G must be a contiguous complex128 \[15, 16, 8\] device tensor"),
    ("dft-G-shape", lambda g: g.dft.pixels_raw(g.c(15, 8, 8), C), T_,
     r"^pixels_raw: G must be a contiguous complex128 \[15, 16, 8\] device tensor"),
    ("dft-G-strided", lambda g: g.dft.pixels_raw(g.c(15, 16, 16)[:, :, ::2], C), T_,
     r"^pixels_raw: G must be a contiguous complex128 \[15, 16, 8\] device tensor"),
    ("dft-G-host", lambda g: g.dft.rings_raw(g.c(C, 8, 15), g.G.cpu()), T_,
     r"^rings_raw: G must be a contiguous complex128 \[15, 16, 8\] device tensor"),
    ("dft-pixels_raw-out", lambda g: g.dft.pixels_raw(g.G, C, out=g.c(C, 8, 16)), V, r"^out= buffer has the wrong shape / dtype / layout"),
    ("dft-abi-null-image", lambda g: g.dft_abi("pxm_dft_px2ring", None, g.G, C), "PxmError", r"^pxm_dft_px2ring: null argument"),
    ("dft-abi-null-rings", lambda g: g.dft_abi("pxm_dft_ring2px", None, g.c(C, 8, 15), C), "PxmError", r"^pxm_dft_ring2px: null argument"),
    ("dft-abi-chains", lambda g: g.dft_abi("pxm_dft_px2ring", g.c(C, 8, 15), g.G, C + 1), "PxmError",
     r"^pxm_dft_px2ring: C outside \[1, max_chains\]"),
    ("dft-abi-unaligned", lambda g: g.dft_abi("pxm_dft_ring2px", g.r(2 * g.G.numel() + 2)[1:], g.c(C, 8, 15), C), "PxmError",
     r"^pxm_dft_ring2px: the ring array must be 16-byte aligned"),
    # the _ex entry points: every refusal of the pixel side and the column count, decided before a launch
    ("dft-ex-ncol", lambda g: _dft_ex(g, ncol=10), "PxmError", r"^pxm_dft_px2ring_ex: ncol must be 2, 4, 6, 8 or a multiple of 16"),
    ("dft-ex-ncol-ring2px", lambda g: _dft_ex(g, False, ncol=24), "PxmError",
     r"^pxm_dft_ring2px_ex: ncol must be 2, 4, 6, 8 or a multiple of 16"),
    ("dft-ex-chains-ncol", lambda g: _dft_ex(g, ncol=2), "PxmError", r"^pxm_dft_px2ring_ex: C chains need ncol >= 2 C"),
    ("dft-ex-chains", lambda g: _dft_ex(g, C=C + 1), "PxmError", r"^pxm_dft_px2ring_ex: C outside \[1, max_chains\]"),
    ("dft-ex-null", lambda g: _dft_ex(g, False, f=None), "PxmError", r"^pxm_dft_ring2px_ex: null argument"),
    ("dft-ex-unaligned", lambda g: _dft_ex(g, G=g.r(2 * g.G.numel() + 2)[1:]), "PxmError",
     r"^pxm_dft_px2ring_ex: the ring array must be 16-byte aligned"),
    ("dft-ex-data-alone", lambda g: _dft_ex(g, data=g.c(DFT_P)), "PxmError", r"^pxm_dft_px2ring_ex: data and invcov come together"),
    ("dft-ex-invcov-alone", lambda g: _dft_ex(g, invcov=g.r(DFT_P)), "PxmError", r"^pxm_dft_px2ring_ex: data and invcov come together"),
    ("dft-ex-ring2px-residual", lambda g: _dft_ex(g, False, data=g.c(DFT_P), invcov=g.r(DFT_P)), "PxmError",
     r"^pxm_dft_ring2px_ex: the residual \(data, invcov\) is fused into pixels -> rings only"),
    ("dft-ex-gw-alone", lambda g: _dft_ex(g, gw=g.r(DFT_P)), "PxmError",
     r"^pxm_dft_px2ring_ex: a weight gw needs the pixel -> data map gidx"),
    ("dft-ex-gidx-ring0", lambda g: _dft_ex(g, False, gidx=_gidx(g), ndata=DFT_P, ring0=1), "PxmError",
     r"^pxm_dft_ring2px_ex: a pixel -> data map needs ring0 == 0"),
    ("dft-ex-gidx-ndata", lambda g: _dft_ex(g, gidx=_gidx(g, -1), ndata=0, chain_stride=0), "PxmError",
     r"^pxm_dft_px2ring_ex: a pixel -> data map needs ndata >= 1"),
    ("dft-ex-gidx-stride", lambda g: _dft_ex(g, gidx=_gidx(g), ndata=100), "PxmError",
     r"^pxm_dft_px2ring_ex: with a pixel -> data map the chains are ndata apart"),
    ("dft-ex-ring0-negative", lambda g: _dft_ex(g, ring0=-1), "PxmError", r"^pxm_dft_px2ring_ex: ring0 must be >= 0"),
    ("dft-ex-ring0-past", lambda g: _dft_ex(g, f=g.c(C, DFT_P + 4), chain_stride=DFT_P + 4, ring0=5), "PxmError",
     r"^pxm_dft_px2ring_ex: the image \[ring0, ring0 \+ L \(2L-1\)\) must lie inside a chain"),
    ("dft-ex-stride-short", lambda g: _dft_ex(g, False, chain_stride=DFT_P - 1), "PxmError",
     r"^pxm_dft_ring2px_ex: the image \[ring0, ring0 \+ L \(2L-1\)\) must lie inside a chain"),
    ("dft-rings_raw_ex-gidx-range", lambda g: g.dft.rings_raw_ex(g.c(C, 100), g.G, gidx=_gidx(g, 100)), V,
     r"^rings_raw_ex: gidx holds an index >= ndata"),
    ("dft-pixels_raw_ex-gidx-range", lambda g: g.dft.pixels_raw_ex(g.G, g.c(C, 100), gidx=g.i(DFT_P) + 2 ** 32 + 5), V,
     r"^pixels_raw_ex: gidx holds an index >= ndata"),
    ("dft-rings_raw_ex-gidx-length", lambda g: g.dft.rings_raw_ex(g.c(C, 100), g.G, gidx=_gidx(g, 0, DFT_P + 1)), V,
     r"^rings_raw_ex: gidx must have one entry per pixel"),
    ("dft-rings_raw_ex-gw-length", lambda g: g.dft.rings_raw_ex(g.c(C, 100), g.G, gidx=_gidx(g), gw=g.r(99)), V,
     r"^rings_raw_ex: gw must have one entry per datum"),
    ("dft-rings_raw_ex-gw-alone", lambda g: g.dft.rings_raw_ex(g.c(C, DFT_P), g.G, gw=g.r(DFT_P)), "PxmError",
     r"^pxm_dft_px2ring_ex: a weight gw needs the pixel -> data map gidx"),
    ("dft-rings_raw_ex-data-alone", lambda g: g.dft.rings_raw_ex(g.c(C, DFT_P), g.G, data=g.c(DFT_P)), V,
     r"^rings_raw_ex: data and invcov come together"),
    ("dft-rings_raw_ex-data-length", lambda g: g.dft.rings_raw_ex(g.c(C, DFT_P), g.G, data=g.c(DFT_P + 1), invcov=g.r(DFT_P)), V,
     r"^data / invcov length mismatch"),
    ("dft-rings_raw_ex-image", lambda g: g.dft.rings_raw_ex(g.c(C, 8, 15), g.G), T_,
     r"^rings_raw_ex: the pixel side must be a contiguous complex128 \[C, chain_stride\] device tensor"),
    ("dft-rings_raw_ex-chains", lambda g: g.dft.rings_raw_ex(g.c(C + 1, DFT_P), g.G), V, r"^more chains than the plan was created for"),
    ("dft-pixels_raw_ex-G-rows", lambda g: g.dft.pixels_raw_ex(g.c(15, 8, 4), g.c(C, DFT_P)), T_,
     r"^pixels_raw_ex: G must be a contiguous complex128 \[15, 16, ncol / 2\] device tensor"),
    ("dft-pixels_raw_ex-ncol", lambda g: g.dft.pixels_raw_ex(g.c(15, 16, 5), g.c(C, DFT_P)), "PxmError",
     r"^pxm_dft_ring2px_ex: ncol must be 2, 4, 6, 8 or a multiple of 16"),
    ("dft-pixels_raw_ex-ring0", lambda g: g.dft.pixels_raw_ex(g.G, g.c(C, DFT_P + 4), ring0=5), "PxmError",
     r"^pxm_dft_ring2px_ex: the image \[ring0, ring0 \+ L \(2L-1\)\) must lie inside a chain"),
    ("gemm-sides-type", lambda g: g.ops.GemmPlan(dict(kind="inv", bl=8)), T_, r"^GemmPlan: sides must be a non-empty list of dicts"),
    ("gemm-sides-empty", lambda g: g.ops.GemmPlan([]), T_, r"^GemmPlan: sides must be a non-empty list of dicts"),
    ("gemm-side-key", lambda g: g.ops.GemmPlan([dict(kind="inv", bl=8, scale=True)]), V, r"^GemmPlan: side 0 needs kind and bl and knows"),
    ("gemm-side-kind", lambda g: g.ops.GemmPlan([dict(kind="legendre", bl=8)]), V, r"^GemmPlan: side 0: kind must be one of inv, fwd"),
    ("gemm-pk", lambda g: g.ops.GemmPlan([dict(kind="fwd", bl=8)], max_chains=1, pk=3), V, r"^GemmPlan: pk must be 0, 2 or 4"),
    ("gemm-pk-chains", lambda g: g.ops.GemmPlan([dict(kind="fwd", bl=8)], max_chains=2, pk=2), V,
     r"^GemmPlan: max_chains must be >= 1, and at most pk / 2 in a packed list"),
    ("gemm-pitch-unpacked", lambda g: g.ops.GemmPlan([dict(kind="fwd", bl=8, x_ncol=4)]), "PxmError",
     r"^pxm_gemm_plan_create: a row pitch of its own needs a packed list"),
    ("gemm-pair-tables", lambda g: g.ops.GemmPlan([dict(kind="fwd", bl=8), dict(kind="fwd", bl=16)], max_chains=1, pk=2), "PxmError",
     r"^pxm_gemm_plan_create: the two sides of a packed pair share one table"),
    ("gemm-share-later", lambda g: g.ops.GemmPlan([dict(kind="fwd", bl=8, y_share=0)]), "PxmError",
     r"^pxm_gemm_plan_create: a side shares arrays of an earlier side only"),
    ("gemm-split-Rp", lambda g: g.ops.GemmPlan([dict(kind="gram_split", bl=8, two=True)]), "PxmError",
     r"^build_gram_split: the parity split needs spin-0 tables and Rp % 32 == 0"),
    ("gemm-pole-streaming", lambda g: g.ops.GemmPlan([dict(kind="gram_split0", bl=32)]), "PxmError",
     r"^upload_tasks: a streaming list with a row pitch of its own"),
    ("gemm-pole-scale", lambda g: g.ops.GemmPlan([dict(kind="gram_split0", bl=32, two=True, ks=True)]).run(1), "PxmError",
     r"^launch_gemm: a pole term outside the Gram list"),
    ("gemm-write-dtype", lambda g: g.gemm.write(16, g.c(4)), T_, r"^GemmPlan.write: src must be a contiguous float64 device tensor"),
    ("gemm-write-host", lambda g: g.gemm.write(16, g.r(4).cpu()), T_, r"^GemmPlan.write: src must be a contiguous float64 device tensor"),
    ("gemm-write-past", lambda g: g.gemm.write(g.gemm.layout["ws_doubles"] - 3, g.r(4)), "PxmError",
     r"^pxm_gemm_plan_write: range outside the workspace"),
    ("gemm-write-negative", lambda g: g.gemm.write(-1, g.r(4)), "PxmError", r"^pxm_gemm_plan_write: range outside the workspace"),
    ("gemm-read-past", lambda g: g.gemm.read(g.gemm.layout["ws_doubles"], 1), "PxmError",
     r"^pxm_gemm_plan_read: range outside the workspace"),
    ("gemm-read-negative", lambda g: g.gemm.read(0, -1), V, r"^GemmPlan.read: negative length"),
    ("gemm-table-side", lambda g: g.gemm.table(1), V, r"^GemmPlan: no such side"),
    ("gemm-run-chains", lambda g: g.gemm.run(C + 1), V, r"^more chains than the plan was created for"),
    ("gemm-run-packed-affine", lambda g: g.gemm_pk.run(1, affine=(1.0, 1.0)), "PxmError",
     r"^pxm_gemm_plan_run: the packed kernels have no affine epilogue and no counter"),
    ("gemm-abi-null-plan", lambda g: g.gemm_abi("pxm_gemm_plan_run", None, 1, 0, 0.0, 0.0, 0.0, 0, None), "PxmError",
     r"^pxm_gemm_plan_run: null plan"),
    ("gemm-abi-chains", lambda g: g.gemm_abi("pxm_gemm_plan_run", g.gemm._h, C + 1, 0, 0.0, 0.0, 0.0, 0, None), "PxmError",
     r"^pxm_gemm_plan_run: C outside \[1, max_chains\]"),
    ("gemm-abi-table-more", lambda g: g.gemm_abi("pxm_gemm_plan_table_read", g.gemm._h, 0, 1, g.r(4).data_ptr(), 4, None), "PxmError",
     r"^pxm_gemm_plan_table_read: more doubles than the table has"),
    ("gemm-abi-report-what", lambda g: g.gemm_abi("pxm_gemm_plan_report", g.gemm._h, 3, 0, None, 0), "PxmError",
     r"^pxm_gemm_plan_report: what must be 0"),
    ("gradg_step-shape", lambda g: g.wav.gradg_step(g.c(C, g.wav.ncoefs + 1), g.c(C, g.wav.npix), g.img, g.w_img, **_step_args(g)), A,
     r"^gradg_step: shape mismatch"),
    ("gradg_step-data", lambda g: g.wav.gradg_step(g.X, g.c(C, g.wav.npix), g.c(g.wav.npix + 1), g.w_img, **_step_args(g)), V,
     r"^data / invcov length mismatch"),
    ("image_init-shape", lambda g: g.wav.image_init(g.c(C, g.wav.npix + 1), g.img, g.w_img), A, r"^image_init: shape mismatch"),
    ("image_init-invcov", lambda g: g.wav.image_init(g.c(C, g.wav.npix), g.img, g.r(g.wav.npix + 1)), V, r"^data / invcov length mismatch"),
    ("image_step-shape", lambda g: g.wav.image_step(g.c(C, g.wav.ncoefs + 1), g.img, g.w_img, **_step_args(g)), A,
     r"^image_step: shape mismatch"),
    ("image_step-preds_out", lambda g: g.wav.image_step(g.X, g.img, g.w_img, preds_out=g.c(C, 3), **_step_args(g)), V,
     r"^preds_out= buffer has the wrong shape / dtype / layout"),
    ("image_step-out-alias", lambda g: g.wav.image_step(g.X, g.img, g.w_img, out=g.X, **_step_args(g)), V,
     r"^out= buffer must be a distinct contiguous complex128 tensor of the state's shape"),
    ("ring_set_data-length", lambda g: g.wav.ring_set_data(g.c(g.wav.npix + 1)), V, r"^data length mismatch"),
    ("ring_init-shape", lambda g: g.wav.ring_init(g.c(C, g.wav.ncoefs + 1)), A, r"^ring_init: shape mismatch"),
    ("ring_step-shape", lambda g: g.wav.ring_step(g.c(C + 1, g.wav.ncoefs), 1.0, **_step_args(g)), A, r"^ring_step: shape mismatch"),
    ("ring_step-out-alias", lambda g: g.wav.ring_step(g.X, 1.0, out=g.X, **_step_args(g)), V,
     r"^out= buffer must be a distinct contiguous complex128 tensor of the state's shape"),
    ("ring_step-pair-noise", lambda g: g.wav.ring_step(g.X, 1.0, noise=g.r(C, g.wav.ncoefs), pairs=True, **_step_args(g)), V,
     r"^real-pair noise must be a float64 \[2 \* slots, N\] array"),
    ("ring_step-noise", lambda g: g.wav.ring_step(g.X, 1.0, noise=g.r(C, g.wav.ncoefs + 1), **_step_args(g)), V,
     r"^injected noise must have the state's shape"),
    ("wl_attach-pix2data", lambda g: g.wav.wl_attach(g.i(g.wav.npix + 1, dtype=g.torch.int32), None, g.wav.npix), V,
     r"^pix2data must have one entry per pixel"),
    ("wl_attach-pix2data-range", lambda g: g.wav.wl_attach(g.i(g.wav.npix, dtype=g.torch.int32) + 100, None, 100), V,
     r"^wl_attach: pix2data holds an index >= ndata"),
    ("wl_attach-weight", lambda g: g.wav.wl_attach(None, g.r(5), g.wav.npix), V, r"^weight must have one entry per datum"),
    ("wl_forward-shape", lambda g: g.wav.wl_forward(g.c(C, g.wav.ncoefs + 1)), A, r"^wl_forward: shape mismatch"),
    ("wl_adjoint-shape", lambda g: g.wav.wl_adjoint(g.c(C, g.wav.npix + 1)), A, r"^wl_adjoint: shape mismatch"),
    ("wl_adjoint-data", lambda g: g.wav.wl_adjoint(g.c(C, g.wav.npix), data=g.c(g.wav.npix + 1), invcov=g.w_img), V,
     r"^data / invcov length mismatch"),
    ("hwav-myula_step-shape", lambda g: g.hwav.myula_step(g.c(C, g.hwav.ncoefs + 1), g.lm, g.w_lm, None, **_step_args(g)), A,
     r"^myula_step: shape mismatch"),
    ("hwav-myula_step-data", lambda g: g.hwav.myula_step(g.XH, g.c(g.hwav.nlm + 1), g.w_lm, None, **_step_args(g)), V,
     r"^data / invcov length mismatch"),
    ("hwav-myula_step-kernel", lambda g: g.hwav.myula_step(g.XH, g.lm, g.w_lm, g.r(g.hwav.nlm + 1), **_step_args(g)), V,
     r"^kernel length mismatch"),
    ("hwav-myula_step-out-alias", lambda g: g.hwav.myula_step(g.XH, g.lm, g.w_lm, None, out=g.XH, **_step_args(g)), V,
     r"^out= buffer must be a distinct contiguous complex128 tensor of the state's shape"),
    ("hwav-myula_step-preds_out", lambda g: g.hwav.myula_step(g.XH, g.lm, g.w_lm, None, preds_out=g.c(C, 3), **_step_args(g)), V,
     r"^preds_out= buffer has the wrong shape / dtype / layout"),
]

# the two FISTA steps share their checks, each in its own name
for _fn, _nsums in (("fista_step", 3), ("fista_step_restart", 4)):
    ROWS += [
        (f"{_fn}-gradg", lambda g, fn=_fn: _fista(g, fn, gradg=g.r(C, N + 1)), V, rf"^{_fn}: Y / gradg / proxf must have the state's shape"),
        (f"{_fn}-no-T", lambda g, fn=_fn: _fista(g, fn, T=None), V, rf"^{_fn}: the threshold T is needed unless proxf is given"),
        (f"{_fn}-beta-empty", lambda g, fn=_fn: _fista(g, fn, beta=g.r(0)), V,
         rf"^{_fn}: beta must be a non-empty contiguous float64 device vector"),
        (f"{_fn}-beta-float32", lambda g, fn=_fn: _fista(g, fn, beta=g.r(4, dtype=g.torch.float32)), V,
         rf"^{_fn}: beta must be a non-empty contiguous float64 device vector"),
        (f"{_fn}-beta-host", lambda g, fn=_fn: _fista(g, fn, beta=g.torch.ones(4, dtype=g.torch.float64)), V,
         rf"^{_fn}: beta must be a non-empty contiguous float64 device vector"),
        (f"{_fn}-out", lambda g, fn=_fn: _fista(g, fn, out=(g.r(C, N), g.r(C, N + 1))), V, r"^out must be a contiguous device array"),
        (f"{_fn}-sums", lambda g, fn=_fn: _fista(g, fn, sums=g.r(C, 5)), V,
         rf"^{_fn}: sums must be a contiguous float64 \[C, {_nsums}\] device array"),
        (f"{_fn}-scratch", lambda g, fn=_fn: _fista(g, fn, scratch=g.r(1)), V, rf"^{_fn}: scratch is too small"),
    ]
ROWS += [
    ("fista_step_restart-index-int32", lambda g: _fista(g, "fista_step_restart", momentum_index=g.i(C, dtype=g.torch.int32)), V,
     r"^fista_step_restart: momentum_index must be a contiguous 64-bit integer \[C\] device vector"),
    ("fista_step_restart-index-length", lambda g: _fista(g, "fista_step_restart", momentum_index=g.i(C + 1)), V,
     r"^fista_step_restart: momentum_index must be a contiguous 64-bit integer \[C\] device vector"),
    ("fista_step_restart-restarts", lambda g: _fista(g, "fista_step_restart", restarts=g.i(C + 1)), V,
     r"^fista_step_restart: restarts must be a contiguous 64-bit integer \[C\] device vector"),
]


def test_every_row_has_its_own_name():
    assert len({row[0] for row in ROWS}) == len(ROWS)


@pytest.mark.parametrize("call,exc,pattern", [pytest.param(*row[1:], id=row[0]) for row in ROWS])
def test_refusal(g, call, exc, pattern):
    exc = getattr(g.ops, exc) if isinstance(exc, str) else exc
    with pytest.raises(exc, match=pattern) as info:
        call(g)
    assert type(info.value) is exc  # the class itself, not a subclass
