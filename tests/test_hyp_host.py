"""Host model of the hypothesis tests of image structure (pxmcmc_amd/uncertainty/hyp.py, csrc/inpaint.hip):
the numpy statement of the step kernel, the properties of segment inpainting on the oracle's wavelet transform, and the
decision on a planted structure, formed in numpy from lci_terms_np / lci_eval_np.  tests/test_gpu_hyp.py holds the kernel
and the device route to the same statements and the same planted structure."""
import numpy as np
import pytest

from pxmcmc_amd.uncertainty import (approx_credible_region_threshold, inpaint_np, inpaint_step_np, inpaint_sum_depth,
                                    lci_eval_np, lci_search_np, lci_terms_np, superpixel_regions)

LD = np.longdouble
L16, B16, JMIN16, SIZE, LMDA, SIG = 16, 2, 0, 4, 2e-3, 0.1
NPIX = L16 * (2 * L16 - 1)
BLOB_REGION, BACKGROUND_REGION = 19, 0
XI = np.arange(32) / 31.0


# ---- the planted structure ---------------------------------------------------------------------------------------------------
def planted_data(oT, amp):
    """the blob amp exp(-((t - 9.5)^2 + (p - 13.5)^2) / (2 1.5^2)) on the grid t = 0 ... 15, p = 0 ... 30, band-limited by
    Psi A, plus noise of sigma = 0.1 from rng(5) -> real data [npix]"""
    t, p = np.meshgrid(np.arange(L16), np.arange(2 * L16 - 1), indexing="ij")
    blob = amp * np.exp(-((t - 9.5) ** 2 + (p - 13.5) ** 2) / (2 * 1.5 ** 2))
    truth = oT.inverse(oT.forward(blob.reshape(-1).astype(complex))).real
    return truth + SIG * np.random.default_rng(5).normal(size=NPIX)


def fista_np(oT, data, T, iters=400):
    """FISTA on F(X) = 1/2 sum w |Psi X - d|^2 + (1 / lmda) sum T |X|, w = 1 / sigma^2, from X = 0"""
    from oracle import pxmcmc_np as ref

    w = 1.0 / SIG ** 2
    v = np.random.default_rng(0).normal(size=oT.ncoefs).astype(complex)
    for _ in range(30):  # power iteration on Psi^+ Psi (approaches the norm from below: the margin below)
        v = oT.inverse_adjoint(oT.inverse(v))
        nrm = np.linalg.norm(v)
        v /= nrm
    step = 1.0 / (1.1 * w * nrm)
    X = Z = np.zeros(oT.ncoefs, dtype=complex)
    t = 1.0
    for _ in range(iters):
        Xn = ref.soft(Z - step * oT.inverse_adjoint(w * (oT.inverse(Z) - data)), step * T / LMDA)
        tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        Z = Xn + ((t - 1.0) / tn) * (Xn - X)
        X, t = Xn, tn
    return X


def decision_np(oT, data, T, X, x_map, region, frac, iters=60, tol=1e-6):
    """the test of one region in numpy: the inpainted surrogate, then F along X* + xi A(x_sgt - x*) at xi = j / 31 ->
    dict(profile, gamma, F_map, units = (F_sgt - gamma) / (gamma - F*), physical, removable, inpaint)"""
    w = np.full(NPIX, 1.0 / SIG ** 2)
    zeta = (superpixel_regions(L16, SIZE).reshape(-1) == region).astype(float)
    tau = frac * np.abs(oT.forward(x_map)).max()
    inp = inpaint_np(oT.forward, oT.inverse, x_map, zeta, tau, iters, tol)
    a, b = X, oT.forward(inp["x"] - x_map)
    q, _, _ = lci_terms_np(a, b, oT.inverse(a) - data, oT.inverse(b), w, T)
    prof = q[0] + q[1] * XI.astype(LD) + q[2] * XI.astype(LD) ** 2 + lci_eval_np(a, b, T, XI) / LD(LMDA)
    F_map = float(prof[0])
    gamma = float(approx_credible_region_threshold(F_map, oT.ncoefs))
    res = lci_search_np(np.array(q, dtype=np.float64), a, b, T, LMDA, gamma)
    physical = bool(prof[-1] > gamma)
    removable = res["upper"] if physical else max(res["upper"], 1.0)
    return dict(profile=np.array(prof, dtype=np.float64), gamma=gamma, F_map=F_map, physical=physical, removable=removable,
                units=float((prof[-1] - gamma) / (gamma - F_map)), inpaint=inp, search=res)


PLANTED = {}


def planted(amp):
    """(oracle transform, data, T, X*, x*) of the planted structure with amplitude amp: built once"""
    from oracle import pxmcmc_np as ref

    if amp not in PLANTED:
        oT = ref.SphericalWaveletTransform(L16, B16, JMIN16)
        assert oT.ncoefs == 1147
        T = ref.S2_Wavelets_L1("synthesis", None, None, LMDA, L16, B16, JMIN16).T
        data = planted_data(oT, amp)
        X = fista_np(oT, data, T)
        PLANTED[amp] = (oT, data, T, X, oT.inverse(X))
    return PLANTED[amp]


# ---- the kernel's statement ----------------------------------------------------------------------------------------------------
def _step_inputs(npix, C, cplx, seed):
    rng = np.random.default_rng(seed)
    vec = (lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)) if cplx else (lambda *s: rng.normal(size=s))
    y, x_prev, x_map = vec(C, npix), vec(C, npix), vec(npix)
    labels = rng.integers(-1, 4, size=npix)
    return y, x_prev, x_map, labels


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_step_statement(cplx):
    npix, C = 37, 6
    y, x_prev, x_map, labels = _step_inputs(npix, C, cplx, 1 + cplx)
    region = np.array([0, 1, 2, 3, 7, 1])  # 7: an empty region
    x_prev[3] = np.where(labels == 3, y[3], x_map) + 0.1 * x_prev[3]  # close to its next image: this slot freezes
    done0, iters0 = np.array([0, 1, 0, 0, 0, 1], np.int32), np.array([3, 5, 0, 9, 2, 4], np.int32)
    stat0 = np.arange(2.0 * C).reshape(C, 2) + 100
    tol2 = 0.5
    x_next, done, iters, stat = inpaint_step_np(y, x_prev, x_map, labels, region, tol2, done0, iters0, stat0)
    for c in range(C):
        if done0[c]:  # an already-done slot: everything untouched
            assert np.array_equal(x_next[c], x_prev[c]) and done[c] == 1 and iters[c] == iters0[c]
            assert np.array_equal(stat[c], stat0[c])
            continue
        inside = labels == region[c]
        assert iters[c] == iters0[c] + 1
        assert np.array_equal(x_next[c][inside], y[c][inside]) and np.array_equal(x_next[c][~inside], x_map[~inside])
        d2 = float((np.abs(x_next[c] - x_prev[c]).astype(LD) ** 2).sum())
        n2 = float((np.abs(x_next[c]).astype(LD) ** 2).sum())
        assert float(stat[c, 0]) == pytest.approx(d2, rel=1e-14) and float(stat[c, 1]) == pytest.approx(n2, rel=1e-14)
        assert done[c] == int(np.float64(stat[c, 0]) <= tol2 * np.float64(stat[c, 1]))
    assert np.array_equal(x_next[4], np.broadcast_to(x_map, (npix,)))  # the empty region gives x_map
    assert not np.shares_memory(x_next, x_prev) and done0[0] == 0 and iters0[0] == 3  # the inputs are left as they were
    assert done.sum() > done0.sum() and (done == 0).any()  # both outcomes of the flag occur


def test_step_minus_one_labels_belong_to_no_slot():
    npix = 20
    y, x_prev, x_map, _ = _step_inputs(npix, 2, True, 3)
    labels = np.full(npix, -1)
    labels[5:9] = 0
    zeros = np.zeros(2, np.int32)
    x_next, *_ = inpaint_step_np(y, x_prev, x_map, labels, [-1, 0], 0.0, zeros, zeros, np.zeros((2, 2)))
    assert np.array_equal(x_next[0], x_map)  # region -1 holds no pixel, though 16 labels are -1
    assert np.array_equal(x_next[1][5:9], y[1][5:9]) and np.array_equal(np.delete(x_next[1], range(5, 9)), np.delete(x_map, range(5, 9)))


def test_step_nan_does_not_freeze_and_equal_images_do():
    npix = 9
    y, x_prev, x_map, _ = _step_inputs(npix, 3, False, 4)
    labels = np.zeros(npix, np.int64)
    y[0, 2] = np.nan
    x_prev[1] = y[1]  # no change at all: d2 = 0 <= tol2 n2 even with tol2 = 0
    zeros = np.zeros(3, np.int32)
    _, done, iters, stat = inpaint_step_np(y, x_prev, x_map, labels, [0, 0, 0], 0.0, zeros, zeros, np.zeros((3, 2)))
    assert np.isnan(stat[0]).all() and done[0] == 0
    assert stat[1, 0] == 0 and done[1] == 1 and done[2] == 0 and (iters == 1).all()
    _, done, _, _ = inpaint_step_np(y, x_prev, x_map, labels, [0, 0, 0], 1e300, zeros, zeros, np.zeros((3, 2)))
    assert done[0] == 0 and done[2] == 1  # a huge tol2 freezes everything but the NaN slot


def test_sum_depth():
    assert inpaint_sum_depth(1) == 2 + 6 + 4 + 1 + 6
    assert inpaint_sum_depth(1024) == 4 + 6 + 4 + 1 + 6  # 512 pairs over 256 lanes: two pairs, four terms per lane
    assert inpaint_sum_depth(4099) == 2 * 2 + 6 + 4 + 1 + 6  # 5 slices; 2050 pairs over 1280 lanes
    assert inpaint_sum_depth(130816) == 2 * 2 + 6 + 4 + 2 + 6  # L = 256: 128 slices
    assert inpaint_sum_depth(2 ** 22) == 2 * 16 + 6 + 4 + 8 + 6  # 512 slices, grid-stride


# ---- the properties of the iteration on the oracle transform --------------------------------------------------------------
def test_inpainting_properties():
    oT, data, T, X, x_map = planted(5)
    labels = superpixel_regions(L16, SIZE).reshape(-1)
    zeta = (labels == BLOB_REGION).astype(float)
    outside = zeta == 0
    top = np.abs(oT.forward(x_map)).max()
    # outside D: x* bit for bit after any number of iterations
    for iters in (1, 2, 7):
        x = inpaint_np(oT.forward, oT.inverse, x_map, zeta, 0.2 * top, iters, 0.0)["x"]
        assert np.array_equal(x[outside], x_map[outside]) and not np.array_equal(x[~outside], x_map[~outside])
    # tau = 0: x^1 = x* (1 - zeta) + zeta Psi A x^0
    x0 = x_map * (1 - zeta)
    x1 = inpaint_np(oT.forward, oT.inverse, x_map, zeta, 0.0, 1, 0.0)["x"]
    assert np.array_equal(x1, np.where(outside, x_map, oT.inverse(oT.forward(x0))))
    # convergence: the relative change falls below 1e-10 within 60 iterations at tau = 0.2 max |A x*|
    res = inpaint_np(oT.forward, oT.inverse, x_map, zeta, 0.2 * top, 60, 1e-10)
    print(f"relative change per iteration: {['%.1e' % h for h in res['history'][::5]]}; frozen after {res['iters_used']}")
    assert res["iters_used"] < 60 and res["rel_change"] <= 1e-10
    assert res["history"][-2] > 1e-10  # (frozen at the first iteration below the tolerance, not later)
    # an empty region: the surrogate is x*, frozen at the second iteration
    res = inpaint_np(oT.forward, oT.inverse, x_map, np.zeros(NPIX), 0.2 * top, 60, 1e-6)
    assert np.array_equal(res["x"], x_map) and res["iters_used"] == 1 and res["rel_change"] == 0.0


# ---- the decision on the planted structure -----------------------------------------------------------------------------------
CASES = [(5, BLOB_REGION, 0.2, True), (5, BLOB_REGION, 0.05, True), (5, BACKGROUND_REGION, 0.2, False),
         (5, BACKGROUND_REGION, 0.05, False), (0, BLOB_REGION, 0.2, False), (0, BACKGROUND_REGION, 0.2, False)]


@pytest.mark.parametrize("amp,region,frac,want", CASES)
def test_decision_on_a_planted_structure(amp, region, frac, want):
    """the blob's superpixel is physical at amp = 5; the background superpixel, and both at amp = 0, are inconclusive;
    |F_sgt - gamma| is at least one (gamma - F*), so that FISTA's tolerance cannot flip the result; removable < 1 exactly
    where the test says physical"""
    oT, data, T, X, x_map = planted(amp)
    res = decision_np(oT, data, T, X, x_map, region, frac)
    print(f"amp {amp} region {region} tau {frac} max: (F_sgt - gamma) / (gamma - F*) = {res['units']:.2f}, removable "
          f"{res['removable']:.4f}, inpainting iterations {res['inpaint']['iters_used']} (rel. change {res['inpaint']['rel_change']:.1e})")
    assert res["physical"] == want
    assert (res["units"] >= 1.0) if want else (res["units"] <= -0.5)
    assert (res["removable"] < 1.0) == want
    assert res["search"]["status"] == 0 and res["search"]["lower"] <= 0.0 <= res["removable"]
    assert res["profile"][0] == pytest.approx(res["F_map"]) and (np.diff(res["profile"], 2) >= -1e-9 * abs(res["gamma"])).all()
