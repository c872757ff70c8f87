"""Local credible intervals on the GPU (csrc/lci.hip, pxmcmc_amd.uncertainty.local_credible_intervals):
pxm_lci_eval and pxm_lci_data_terms against the long-double model element by element, batch independence, pxm_lci_search on
the instances, the status cases and the end-point properties of tests/test_lci_host.py, graph replay, and the whole call on
Identity and WeakLensing operators against a, b, r, s built with the oracle's operators."""
import numpy as np
import pytest

from test_lci_host import (F_ld, LD, ROUNDS, TERM_ROUNDINGS, U, check_ok_result, check_status_case, f_tol, make_instance,
                           status_cases)

pytestmark = pytest.mark.gpu

C_MAX = 16  # slots the buffers are allocated for


def _buf(a, n, cplx):
    """[C, n] array in a [C_MAX, n] device buffer, NaN beyond C"""
    import torch

    from pxmcmc_amd import ops

    t = torch.full((C_MAX, n), float("nan"), dtype=torch.complex128 if cplx else torch.float64, device=ops.device())
    t[: a.shape[0]] = ops.as_device(a, t.dtype)
    return t


def _vectors(n, C, cplx, seed):
    rng = np.random.default_rng(seed)
    vec = (lambda: rng.normal(size=(C, n)) + 1j * rng.normal(size=(C, n))) if cplx else (lambda: rng.normal(size=(C, n)))
    a, b = vec(), vec() * (rng.random((C, n)) < 0.3)
    xi = rng.normal(size=(C, 32)) * 2.0
    if n >= 2:  # a kink exactly at xi[c, 5] in element 1 of every slot
        b[:, 1] = 1.0
        a[:, 1] = -xi[:, 5]
    return a, b, xi, rng


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("vecT", [False, True], ids=["scalarT", "vectorT"])
def test_eval_against_long_double_model(n, C, cplx, vecT):
    """every P[c, j], S_a and S_b within (depth(n) + TERM_ROUNDINGS) U sum|terms| of the long-double model (DESIGN.md section
    14b: the chain of additions of the fixed-order sum plus the roundings of a term); nothing written beyond C"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.uncertainty import lci_eval_np, lci_sum_depth

    a, b, xi, rng = _vectors(n, C, cplx, seed=10 * n + C + 2 * cplx + vecT)
    T = rng.random(n) + 0.05 if vecT else 0.37
    dev = ops.device()
    X = torch.full((C_MAX, 32), float("nan"), dtype=torch.float64, device=dev)
    X[:C] = ops.as_device(xi)
    P = torch.full((C_MAX, 34), float("nan"), dtype=torch.float64, device=dev)
    ops.lci_eval(_buf(a, n, cplx)[:C], _buf(b, n, cplx)[:C], ops.as_device(T) if vecT else T, X[:C], out=P[:C])
    torch.cuda.synchronize()
    assert torch.isnan(P[C:]).all()
    got = P[:C].cpu().numpy()
    assert np.isfinite(got).all()
    bound_c = (lci_sum_depth(n) + TERM_ROUNDINGS) * U
    worst = 0.0
    for c in range(C):
        want = np.concatenate([lci_eval_np(a[c], b[c], T, xi[c]), lci_eval_np(a[c], 0 * b[c], T, [0.0]), lci_eval_np(b[c], 0 * b[c], T, [0.0])])
        err = np.abs(got[c].astype(LD) - want)  # (the terms are non-negative: sum|terms| is the sum itself)
        ok = err <= bound_c * want
        assert ok.all(), (c, np.flatnonzero(~ok), err[~ok], want[~ok])
        worst = max(worst, float((err[want > 0] / (bound_c * want[want > 0])).max(initial=0.0)))
    if n >= 2 and cplx:
        assert np.isfinite(got[:, 5]).all()
    print(f"eval n={n} C={C} cplx={cplx} vecT={vecT}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_data_terms_against_long_double_model(n, C, cplx):
    """(q0, q1, q2) within (depth(n) + TERM_ROUNDINGS) U sum|terms| of the long-double sums; |term| of q1 is w |r| |s|"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.uncertainty import lci_sum_depth, lci_terms_np

    pa, pb, _, rng = _vectors(n, C, cplx, seed=77 * n + C + cplx)
    d = rng.normal(size=n) + (1j * rng.normal(size=n) if cplx else 0)
    w = rng.random(n) + 0.5
    quad = torch.full((C_MAX, 3), float("nan"), dtype=torch.float64, device=ops.device())
    ops.lci_data_terms(_buf(pa, n, cplx)[:C], _buf(pb, n, cplx)[:C], d, w, out=quad[:C])
    torch.cuda.synchronize()
    assert torch.isnan(quad[C:]).all()
    got = quad[:C].cpu().numpy()
    bound_c = (lci_sum_depth(n) + TERM_ROUNDINGS) * U
    worst = 0.0
    for c in range(C):
        r = pa[c] - d
        q, _, _ = lci_terms_np(r, r, r, pb[c], w, 1.0)
        mag = np.array([q[0], (w.astype(LD) * np.abs(r).astype(LD) * np.abs(pb[c]).astype(LD)).sum() * (1 + 4 * U), q[2]])
        # (r = pa - d is rounded once, here as on the device; product, fma and the product with w: inside TERM_ROUNDINGS)
        err = np.abs(got[c].astype(LD) - q)
        assert (err <= bound_c * mag).all(), (c, err, bound_c * mag)
        worst = max(worst, float((err[mag > 0] / (bound_c * mag[mag > 0])).max(initial=0.0)))
    print(f"data terms n={n} C={C} cplx={cplx}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_a_slot_alone_equals_the_slot_in_a_batch(cplx):
    """eval, data terms and search: slot c alone and slot c in a batch of 16, bit for bit (n = 4099: several slices)"""
    import torch

    from pxmcmc_amd import ops

    n, C = 4099, 16
    a, b, xi, rng = _vectors(n, C, cplx, seed=5 + cplx)
    T = ops.as_device(rng.random(n) + 0.05)
    d, w = rng.normal(size=n) + (1j * rng.normal(size=n) if cplx else 0), rng.random(n) + 0.5
    A, B, X = _buf(a, n, cplx), _buf(b, n, cplx), ops.as_device(xi)
    gamma = ops.as_device(np.full(C, 1e5))
    P = ops.lci_eval(A, B, T, X)
    quad = ops.lci_data_terms(A, B, d, w)
    out, st = ops.lci_search(A, B, T, quad, 0.7, gamma, rounds=4)
    for c in (0, 7, 15):
        sl = slice(c, c + 1)
        assert torch.equal(ops.lci_eval(A[sl], B[sl], T, X[sl]).view(torch.int64), P[sl].view(torch.int64))
        q1 = ops.lci_data_terms(A[sl], B[sl], d, w)
        assert torch.equal(q1.view(torch.int64), quad[sl].view(torch.int64))
        o1, s1 = ops.lci_search(A[sl], B[sl], T, q1, 0.7, gamma[sl], rounds=4)
        assert torch.equal(o1.view(torch.int64), out[sl].view(torch.int64)) and torch.equal(s1, st[sl])
    assert (st == 0).all()


def _dev_search(inst, rounds=ROUNDS):
    """pxm_lci_search on one instance of the host test -> the dict lci_search_np returns"""
    from pxmcmc_amd import ops

    a, b = np.asarray(inst["a"])[None], np.asarray(inst["b"])[None]
    if np.iscomplexobj(a) != np.iscomplexobj(b):
        a, b = a.astype(complex), b.astype(complex)
    T = inst["T"]
    out, st = ops.lci_search(ops.as_device(a), ops.as_device(b), ops.as_device(T) if np.ndim(T) else float(T),
                             ops.as_device(np.asarray(inst["q"], dtype=np.float64)[None]), inst["lmda"],
                             ops.as_device(np.array([inst["gamma"]])), rounds=rounds)
    o = out.cpu().numpy()[0]
    return dict(lower=o[0], upper=o[1], width_lower=o[2], width_upper=o[3], f_min=o[4], xi_min=o[5], outer=(o[6], o[7]),
                status=int(st.cpu().numpy()[0]))


def test_search_on_the_host_tests_instances():
    """the three end-point properties, evaluated with the long-double model, on the 200 instances of the host test"""
    from pxmcmc_amd.uncertainty import lci_shrink_factor, lci_sum_depth

    worst = 0.0
    for seed in range(200):
        inst = make_instance(seed)
        res = _dev_search(inst)
        assert res["status"] == 0, (seed, res)
        worst = max(worst, check_ok_result(inst, res, lci_sum_depth(inst["n"])) / lci_shrink_factor(ROUNDS, inst["q"][2] > 0))
    print(f"largest final width / (guaranteed factor x outer bracket): {worst:.3e}")


@pytest.mark.parametrize("case", status_cases(), ids=lambda c: c[0])
def test_status_cases(case):
    """every status from its designed case; a NaN in a ends with nonfinite, NaN outputs and a clean return"""
    import torch

    from pxmcmc_amd.uncertainty import lci_sum_depth

    name, inst, want = case
    res = _dev_search(inst)
    torch.cuda.synchronize()
    check_status_case(name, inst, want, res, lci_sum_depth(inst["n"]))


def test_bad_arguments_are_refused():
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError

    x = torch.ones((2, 8), dtype=torch.float64, device=ops.device())
    quad, gamma = torch.ones((2, 3), dtype=torch.float64, device=x.device), torch.ones(2, dtype=torch.float64, device=x.device)
    with pytest.raises(PxmError):
        ops.lci_search(x, x, 0.1, quad, 0.5, gamma, rounds=0)
    with pytest.raises(PxmError):
        ops.lci_search(x, x, 0.1, quad, -1.0, gamma)
    with pytest.raises(TypeError):
        ops.lci_search(x, x, 0.1, quad[:1], 0.5, gamma)
    with pytest.raises(ValueError):
        ops.lci_eval(x, x[:1], 0.1, torch.zeros((2, 32), dtype=torch.float64, device=x.device))


def test_graph_replay_equals_eager():
    """the whole search captured into a HIP graph and replayed, on new inputs, equals the eager call bit for bit"""
    import torch

    from pxmcmc_amd import ops

    n, C = 1500, 3
    a, b, _, rng = _vectors(n, C, True, seed=42)
    a2 = a + 0.1 * rng.normal(size=a.shape)
    T = ops.as_device(rng.random(n) + 0.05)
    A, B = ops.as_device(a), ops.as_device(b)
    quad = ops.as_device(np.tile([2.0, -0.5, 1.5], (C, 1)))
    gamma = ops.as_device(np.full(C, 5e3))
    scratch = ops.lci_scratch(n, C, A.device)
    new = lambda: (torch.full((C, 8), float("nan"), dtype=torch.float64, device=A.device),  # noqa: E731
                   torch.full((C,), -1, dtype=torch.int32, device=A.device))
    run = lambda o, s: ops.lci_search(A, B, T, quad, 0.4, gamma, rounds=ROUNDS, out=o, status=s, scratch=scratch)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*new())  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    go, gs = new()
    g = torch.cuda.CUDAGraph()
    with ops.capture_scope(), torch.cuda.graph(g):
        run(go, gs)
    assert torch.isnan(go).all()  # capture does not execute
    for src in (a, a2):
        A.copy_(ops.as_device(src))
        g.replay()
        torch.cuda.synchronize()
        eo, es = run(*new())
        torch.cuda.synchronize()
        assert (es == 0).all()
        assert torch.equal(eo.view(torch.int64), go.view(torch.int64)) and torch.equal(es, gs)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
L16, B16, JMIN16, SIZE, LMDA = 16, 2, 0, 4, 2e-3
E2E = {}  # which -> (operator, prior, params, X_map, the FISTA run, oracle transform, oracle forward, data, w): built once


def _e2e(which):
    import contextlib
    import io

    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.forward import ForwardOperator, SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.optim import FISTA
    from pxmcmc_amd.prior import S2_Wavelets_L1
    from pxmcmc_amd.transforms import SphericalWaveletTransform

    if which in E2E:
        return E2E[which]
    L = L16
    rng = np.random.default_rng(11)
    oT = ref.SphericalWaveletTransform(L, B16, JMIN16)
    if which == "identity":
        npix = L * (2 * L - 1)
        truth = oT.inverse((rng.normal(size=oT.ncoefs) * (rng.random(oT.ncoefs) < 0.1)).astype(complex)).real
        sig = 0.1
        data = truth + sig * rng.normal(size=npix)
        op = SphericalWaveletTransformOperator(data, sig, "synthesis", L, B16, JMIN16, max_chains=3)
        ofwd = lambda X: oT.inverse(X)  # noqa: E731
        w = np.full(npix, 1 / sig ** 2)
    else:
        from pxmcmc_amd.measurements import WeakLensing
        from pxmcmc_amd.utils import build_mask

        mask = build_mask(L, size=20.0)
        wl = WeakLensing(L, mask, ngal=np.full_like(mask, 30), max_chains=3)
        owl = ref.WeakLensing(L, mask, np.full_like(mask, 30))
        data = (rng.normal(size=wl.ndata) + 1j * rng.normal(size=wl.ndata)) * 0.05
        tr = SphericalWaveletTransform(L, B16, JMIN16, max_chains=3)
        op = ForwardOperator(data, 1 / wl.inv_cov, "synthesis", transform=tr, measurement=wl, nparams=tr.ncoefs)
        ofwd = lambda X: owl.forward(oT.inverse(X))  # noqa: E731
        w = ref.invcov_diag(data, 1 / owl.inv_cov).real
    assert op.nparams == oT.ncoefs == 1147
    reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L, B=B16, J_min=JMIN16)
    p = PxMCMCParams(lmda=LMDA, mu=1.0, complex=False, verbosity=0)
    est = FISTA(op, reg, p, tol=1e-3, max_iter=3000)
    with contextlib.redirect_stdout(io.StringIO()):
        X = est.run()
    E2E[which] = (op, reg, p, X, est, oT, ofwd, np.asarray(data), w)
    return E2E[which]


def _device_inputs(op, X, labels, batch=3):
    """a, b and (q0, q1, q2) of every region as the device forms them, through the operators' own calls -> numpy arrays"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.uncertainty.regions import _lci_preds, _lci_weights

    tr = op.transform
    Xd = ops.as_device(np.asarray(X).astype(complex))
    x_map = ops.as_device(tr.inverse(Xd[None]))[0]
    lab = torch.from_numpy(labels.reshape(-1).astype(np.int64)).to(Xd.device)
    A, Bs, Q = [], [], []
    for r0 in range(0, int(labels.max()) + 1, batch):
        ids = torch.arange(r0, min(r0 + batch, int(labels.max()) + 1), device=Xd.device)
        zeta = (lab[None, :] == ids[:, None]).to(torch.complex128)
        b = ops.as_device(tr.forward(zeta), torch.complex128)
        a = Xd[None] - ops.as_device(tr.forward(zeta * x_map[None]), torch.complex128)
        pa, d = _lci_preds(op, a)
        pb, _ = _lci_preds(op, b)
        A.append(a.cpu().numpy()), Bs.append(b.cpu().numpy()), Q.append(ops.lci_data_terms(pa, pb, d, _lci_weights(op)).cpu().numpy())
    return np.concatenate(A), np.concatenate(Bs), np.concatenate(Q)


@pytest.mark.parametrize("which", ["identity", "weaklensing"])
def test_local_credible_intervals_end_to_end(which):
    """L = 16, B = 2, J_min = 0, 4 x 4 superpixels (32 regions) in batches of 3 (the last one ragged): every region ok (finite
    ends under the masked weak-lensing operator as well), lower <= map_value <= upper for Identity, and the end-point
    properties of EVERY region against a, b, r, s built with the oracle's operators, and the width bound"""
    from pxmcmc_amd.uncertainty import (approx_credible_region_threshold, lci_shrink_factor, lci_sum_depth, lci_terms_np,
                                        local_credible_intervals, map_objective, superpixel_regions)

    op, reg, p, X, est, oT, ofwd, data, w = _e2e(which)
    labels = superpixel_regions(L16, SIZE)
    assert labels.max() + 1 == 32
    F_map = map_objective(op, reg, p, X).cpu().numpy()
    print(f"{which}: map_objective {F_map[0]:.10e}, FISTA.objective_map {est.objective_map[0]:.10e}")
    assert abs(F_map[0] - est.objective_map[0]) <= 1e-12 * abs(F_map[0])
    res = local_credible_intervals(op, reg, p, X, labels, rounds=ROUNDS, batch=3)
    assert res.threshold == pytest.approx(approx_credible_region_threshold(F_map[0], op.nparams), rel=1e-14)
    assert res.lower.shape == (32,) and (res.status == 0).all(), res.status
    assert np.isfinite(res.lower).all() and np.isfinite(res.upper).all() and (res.range == res.upper - res.lower).all()
    Xc = np.asarray(X).astype(complex)
    x_map = oT.inverse(Xc)
    flat = labels.reshape(-1)
    # the widths: the guaranteed factor per round, plus the rounding of the points (as the host test asks)
    span = res.outer[:, 1] - res.outer[:, 0]
    assert np.isfinite(res.outer).all() and (span > 0).all()
    assert (res.width <= lci_shrink_factor(ROUNDS) * span + 64 * U * np.abs(res.outer).max(axis=1)).all(), (res.width, span)
    dev_a, dev_b, dev_q = _device_inputs(op, X, labels)
    depth, T, gamma = lci_sum_depth(op.nparams), np.asarray(reg.T), LD(res.threshold)
    worst = 0.0
    for r in range(32):
        zeta = (flat == r).astype(float)
        assert res.map_value[r] == pytest.approx(x_map.real[flat == r].mean(), abs=1e-10)
        if which == "identity":
            assert res.lower[r] <= res.map_value[r] <= res.upper[r], r
        a, b = Xc - oT.forward(x_map * zeta), oT.forward(zeta)
        q, _, _ = lci_terms_np(a, b, ofwd(a) - data, ofwd(b), w, T)
        inst = dict(a=a, b=b, T=T, q=np.array(q, dtype=np.float64), lmda=LMDA, gamma=res.threshold, n=a.size)
        # The device searched F of ITS a, b, q, which differ from the oracle's by the round-off of the transforms.  F moves by
        # at most |dq0| + |dq1| |xi| + |dq2| xi^2 + sum T (|da| + |xi| |db|) / lmda, formed here from the differences
        # themselves; the rounding of one evaluation (f_tol) comes on top.  That the differences are round-off is asserted:
        # the slack stays below 1e-9 of the level (the transforms agree to ~n 2^-53 of their scale, 1 / lmda = 500 amplifies
        # the prior's share), orders below the distance of the level to min F.
        da, db = np.abs(dev_a[r] - a), np.abs(dev_b[r] - b)
        dq = np.abs(dev_q[r] - inst["q"])

        def slack(x):
            v = dq[0] + dq[1] * abs(x) + dq[2] * x * x + float((T * (da + abs(x) * db)).sum()) / LMDA + f_tol(inst, x, depth)
            assert v <= 1e-9 * abs(res.threshold), (r, x, v, dq, da.max(), db.max())
            return v

        for x in (res.lower[r], res.upper[r]):
            assert F_ld(inst, x) <= gamma + slack(x), (r, x)
        for x in (res.lower[r] - res.width[r], res.upper[r] + res.width[r]):  # (width: the larger of the two brackets)
            assert F_ld(inst, x) >= gamma - slack(x), (r, x)
        worst = max(worst, slack(res.lower[r]), slack(res.upper[r]))
    print(f"{which}: largest slack / level {worst / abs(res.threshold):.3e}")
    painted = res.to_map()
    assert painted.shape == labels.shape and np.array_equal(painted[0, 0], res.range[0])
    print(f"{which}: median range {np.median(res.range):.4f}, largest final width {res.width.max():.3e}")


def test_ragged_batches_equal_one_batch():
    """batch 3 (ragged) and batch 8 give the same numbers bit for bit; -1 labels are left out; an empty label raises"""
    from pxmcmc_amd.uncertainty import local_credible_intervals, superpixel_regions

    op, reg, p, X, *_ = _e2e("identity")
    labels = superpixel_regions(L16, 8)  # 2 x 4 = 8 regions
    r3 = local_credible_intervals(op, reg, p, X, labels, threshold=None, batch=3)
    r8 = local_credible_intervals(op, reg, p, X, labels, batch=8)
    for k in ("lower", "upper", "f_min", "status", "map_value"):  # (NaN ends where a region's set is empty)
        assert np.array_equal(getattr(r3, k), getattr(r8, k), equal_nan=k != "status"), k
    assert (r3.status == 0).sum() >= 6 and np.isnan(r3.lower[r3.status != 0]).all()
    lab = labels.copy()
    lab[lab == 7] = -1
    r7 = local_credible_intervals(op, reg, p, X, lab, batch=3)
    assert r7.lower.shape == (7,) and np.array_equal(r7.lower, r3.lower[:7], equal_nan=True) and np.isnan(r7.to_map()[-1, -1])
    lab[lab == 2] = 5
    with pytest.raises(ValueError, match="region 2 has no pixel"):
        local_credible_intervals(op, reg, p, X, lab)


def test_refused_configurations():
    from pxmcmc_amd.forward import ForwardOperator, SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.measurements import WeakLensingHarmonic
    from pxmcmc_amd.prior import L1, S2_Wavelets_L1
    from pxmcmc_amd.transforms import SphericalWaveletTransform
    from pxmcmc_amd.uncertainty import local_credible_intervals, map_objective, superpixel_regions

    L = 8
    npix = L * (2 * L - 1)
    rng = np.random.default_rng(0)
    data = rng.normal(size=npix)
    p = PxMCMCParams(lmda=LMDA, mu=1.0, verbosity=0)
    labels = superpixel_regions(L, 4)
    reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L, B=2, J_min=0)
    good = SphericalWaveletTransformOperator(data, 0.1, "synthesis", L, 2, 0)
    X = np.zeros(good.nparams, dtype=complex)

    class OwnProx(S2_Wavelets_L1):
        def proxf(self, X):
            return super().proxf(X)

    full = SphericalWaveletTransformOperator(data, np.eye(npix) * 0.01, "synthesis", L, 2, 0)
    analysis = SphericalWaveletTransformOperator(data, 0.1, "analysis", L, 2, 0)
    trh = SphericalWaveletTransform(L, 2, 0, harmonic=True)
    dh = rng.normal(size=L * L) + 1j * rng.normal(size=L * L)
    harm = ForwardOperator(dh, 0.1, "synthesis", transform=trh, measurement=WeakLensingHarmonic(L), nparams=trh.ncoefs)
    for op, prior, x, what in ((full, reg, X, "full covariance"), (analysis, reg, np.zeros(npix), "synthesis setting"),
                               (good, OwnProx("synthesis", None, None, LMDA, L=L, B=2, J_min=0), X, "stock synthesis L1"),
                               (harm, L1("synthesis", None, None, LMDA), np.zeros(trh.ncoefs, dtype=complex), "harmonic")):
        with pytest.raises(ValueError, match=what):
            local_credible_intervals(op, prior, p, x, labels)
        with pytest.raises(ValueError, match=what):
            map_objective(op, prior, p, x)
    with pytest.raises(ValueError):
        local_credible_intervals(good, reg, p, X, labels.astype(float))  # labels must be integers
    with pytest.raises(ValueError):
        local_credible_intervals(good, reg, p, X, labels[:-1])  # one label per pixel


def test_example_writes_the_maps(tmp_path, capsys):
    """examples/topography_synthetic.py --map-start --local-ci 4 at L = 16: the three maps are written and painted per region"""
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("topography_synthetic", os.path.join(root, "examples", "topography_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--L", "16", "--nsamples", "2", "--ngap", "2", "--map-start", "--local-ci", "4", "--outdir", str(tmp_path)])
    assert "local credible intervals: " in capsys.readouterr().out
    rng = np.load(tmp_path / "myula_synthesis_0_lci_range.npy")
    lo, hi = np.load(tmp_path / "myula_synthesis_0_lci_lower.npy"), np.load(tmp_path / "myula_synthesis_0_lci_upper.npy")
    assert rng.shape == (16, 31) and np.isfinite(rng).any()
    ok = np.isfinite(rng)
    assert np.array_equal(rng[ok], (hi - lo)[ok]) and (rng[ok] > 0).all()
    assert (rng[:4, :4] == rng[0, 0]).all() or np.isnan(rng[0, 0])
    with pytest.raises(SystemExit):
        mod.main(["--L", "16", "--local-ci", "4", "--outdir", str(tmp_path)])  # needs --map-start
