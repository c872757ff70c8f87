"""Total variation on the GPU (csrc/tv.hip): the gradient, its adjoint and the TV value against long-double statements with
derived rounding bounds on every element; the pair projection against its long-double statement with planted edge cases; the
fused primal-dual steps against the composed launches bit for bit; refusals; optim.PrimalDual and optim.analysis_prox with
prior.TV_S2 against the numpy statements of pxmcmc_amd.tv_np; the anisotropic form through the generic launches; and the
samplers in the analysis setting on a float64 state."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

from test_tv_host import (CAP_TOL, EPS, LD, PAIR_RSCALE, PAIR_SIGMA, cap_relative_gap, dense_gradient, gamma, pair_inputs,
                          pair_step_ext, parts, polar_cap_problem)

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 5, 12, 182]  # 12: 276 pixels, two workgroups per chain; 182: 66066 pixels > 256 x 256, the grid-stride loop
C_RUN, C_MAX = 3, 4  # chains launched, chains the buffers are allocated for: nothing may be written past the launch's C


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _dev(a):
    """a [C, n] numpy array in a NaN-filled device buffer of C_MAX chains"""
    import torch

    from pxmcmc_amd import ops

    dt = torch.complex128 if np.iscomplexobj(a) else torch.float64
    t = torch.full((C_MAX, a.shape[1]), float("nan"), dtype=dt, device=ops.device())
    t[: a.shape[0]] = ops.as_device(a, dt)
    return t


def _nan(like, width=None, real=False):
    import torch

    shape = (C_MAX, like.shape[1] if width is None else width)
    return torch.full(shape, float("nan"), dtype=torch.float64 if real else like.dtype, device=like.device)


def _untouched(*bufs):
    import torch

    return all(bool(torch.isnan(b[C_RUN:].real if b.is_complex() else b[C_RUN:]).all()) for b in bufs)


def _launches(solo):
    """the chains of one batched launch, or one launch per chain"""
    return [slice(c, c + 1) for c in range(C_RUN)] if solo else [slice(0, C_RUN)]


def _draw(rng, cplx, *shape):
    return rng.normal(size=shape) + (1j * rng.normal(size=shape) if cplx else 0)


@pytest.fixture(scope="module")
def tables():
    """the device table and its float64 host copy per size (the long-double statements run on the same float64 table)"""
    from pxmcmc_amd import ops

    out = {}
    for L in SIZES:
        ab = ops.tv_ring_coefs(L)
        out[L] = (ab, ab.cpu().numpy())
    return out


def _components(a):
    return [a.real, a.imag] if np.iscomplexobj(a) else [a]


def _grad_magnitudes(xa, ab, L):
    """sum of the magnitudes of the terms of every element of A x: a_t (|x[t+1]| + |x[t]|), b_t (|x[p+1]| + |x[p]|)"""
    n = 2 * L - 1
    im = np.abs(xa).reshape(-1, L, n)
    out = np.zeros((im.shape[0], 2, L, n), dtype=LD)
    out[:, 0, : L - 1] = ab[0, : L - 1, None] * (im[:, 1:] + im[:, : L - 1])
    out[:, 1] = ab[1, :, None] * (np.roll(im, -1, axis=-1) + im)
    return out.reshape(im.shape[0], 2 * L * n)


def _adjoint_magnitudes(va, ab, L):
    n = 2 * L - 1
    v = np.abs(va).reshape(-1, 2, L, n)
    out = ab[0, :, None] * v[:, 0] + ab[1, :, None] * (np.roll(v[:, 1], 1, axis=-1) + v[:, 1])
    out[:, 1:] += ab[0, : L - 1, None] * v[:, 0, : L - 1]
    return out.reshape(v.shape[0], L * n)


def _pair2(u):
    """the kernel's sum of squares of a pair in float64, every product and sum rounded: [C, 2 m] -> [C, m]"""
    u = u.reshape(u.shape[0], 2, -1)
    if np.iscomplexobj(u):
        return (u[:, 0].real ** 2 + u[:, 0].imag ** 2) + (u[:, 1].real ** 2 + u[:, 1].imag ** 2)
    return u[:, 0] ** 2 + u[:, 1] ** 2


def _ld_sum(t):
    return t.astype(LD).sum(axis=-1)


# ---- 1. the operator kernels against the long-double statement -----------------------------------------------------------------------
@pytest.mark.parametrize("L", SIZES)
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_grad_adjoint_and_value_against_the_long_double_statement(tables, L, cplx):
    """Per real component, with u = 2^-53 and gamma_k = k u / (1 - k u) applied to the sum of the magnitudes of the element's
    terms: A rounds the difference and the product (k = 2); A^H rounds the difference, the product and two fma (k = 4).
    A term of the TV value, T sqrt(d0^2 + d1^2 [+ ...]), carries 2 roundings in each d, hence 5 in a square, at most 7 in the
    sum of squares (two levels of additions for a complex pair), half of that and one more through the root, one for the
    product with T: k = 8 covers it; the sum adds the sum-order bound m eps of its non-negative terms."""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.tv_np import pair_norm_np, tv_grad_adjoint_np, tv_grad_np

    ab_dev, ab = tables[L]
    abl = ab.astype(LD)
    m = L * (2 * L - 1)
    rng = np.random.default_rng(100 + 2 * L + cplx)
    X, V = _draw(rng, cplx, C_RUN, m), _draw(rng, cplx, C_RUN, 2 * m)
    T = 0.5 + rng.random(m)
    bX, bV = _dev(X), _dev(V)
    got = {}
    for solo in (False, True):
        g, a = _nan(bX, 2 * m), _nan(bX)
        val = _nan(bX, 2, real=True)  # column 0: scalar T, column 1: vector T
        for sl in _launches(solo):
            ops.tv_grad(bX[sl], ab_dev, out=g[sl])
            ops.tv_grad_adjoint(bV[sl], ab_dev, out=a[sl])
            val[sl, 0] = ops.tv_value(bX[sl], ab_dev, 1.5)
            val[sl, 1] = ops.tv_value(bX[sl], ab_dev, ops.as_device(T, torch.float64))
        torch.cuda.synchronize()
        assert _untouched(g, a, val)
        got[solo] = [t[:C_RUN].cpu().numpy() for t in (g, a, val)]
    for one, alone in zip(got[False], got[True]):
        assert np.array_equal(one, alone)  # every chain equals the chain run alone, bit for bit
    G, AH, val = got[False]
    assert np.isfinite(G.view(float)).all() and np.isfinite(AH.view(float)).all()
    for gc, xc in zip(_components(G), _components(X)):
        err = np.abs(gc.astype(LD) - tv_grad_np(xc.astype(LD), abl, L))
        bound = gamma(2) * _grad_magnitudes(xc.astype(LD), abl, L)
        print(f"L={L} cplx={cplx}: A x, worst error / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3f}")
        assert np.all(err <= bound)
    assert np.all(G.reshape(C_RUN, 2, L, -1)[:, :, L - 1] == 0)  # the pole ring
    for ac, vc in zip(_components(AH), _components(V)):
        err = np.abs(ac.astype(LD) - tv_grad_adjoint_np(vc.astype(LD), abl, L))
        bound = gamma(4) * _adjoint_magnitudes(vc.astype(LD), abl, L)
        print(f"L={L} cplx={cplx}: A^H v, worst error / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3f}")
        assert np.all(err <= bound)
    pn = np.sqrt(sum(tv_grad_np(xc.astype(LD), abl, L) ** 2 for xc in _components(X)).reshape(C_RUN, 2, m).sum(axis=1))
    for k, Tk in enumerate((LD(1.5), T.astype(LD))):
        want = (Tk * pn).sum(axis=1)
        diff = np.abs(val[:, k].astype(LD) - want)
        print(f"L={L} cplx={cplx}: TV value, |got - exact| / exact {(diff / want).astype(float)} (bound {gamma(8) + m * EPS:.3e})")
        assert np.all(diff <= (gamma(8) + m * EPS) * want)
    assert pair_norm_np(tv_grad_np(X, ab, L)).shape == (C_RUN, m)


# ---- 2. the pair projection ----------------------------------------------------------------------------------------------------------
def _run_pairs(V, W, T, solo):
    import torch

    from pxmcmc_amd import ops

    bV, bW = _dev(V), _dev(W)
    b1, sums = _nan(bV), _nan(bV, 3, real=True)
    Td = ops.as_device(T, torch.float64) if np.ndim(T) else float(T)
    for sl in _launches(solo):
        ops.pd_dual_step_pairs(bV[sl], bW[sl], Td, PAIR_SIGMA, PAIR_RSCALE, out=b1[sl], sums=sums[sl])
    torch.cuda.synchronize()
    assert _untouched(b1, sums)
    return b1[:C_RUN].cpu().numpy(), sums[:C_RUN].cpu().numpy()


@pytest.mark.parametrize("L", SIZES)
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("vecT", [False, True], ids=["scalarT", "vectorT"])
def test_pair_projection_against_the_long_double_statement(L, cplx, vecT):
    """||V1_i - exact_i|| <= 4 eps max(||w_i||, r_i) on every pair, the form of the complex projection of tests/test_gpu_pd.py.
    In units of eps / 2: w = fma(sigma, W, V) 1, r = T rscale 1, the norm 2.5 (a complex pair has four squares and two levels
    of additions: three roundings deep under the root, halved, and the root's own), r / a 1, the product 1 -- 6.5, i.e. 3.25
    eps relative to max(||w||, r).  No pair is within 2^-40 of its radius except the planted ones, which are exact.  The sums
    against long-double sums of the kernel's own float64 terms: m eps of each (non-negative terms in any order)."""
    m = L * (2 * L - 1)
    V, W, T = pair_inputs(m, C_RUN, cplx, vecT, seed=300 + 4 * L + 2 * cplx + vecT)
    V1, sums = _run_pairs(V, W, T, solo=False)
    sV1, ssums = _run_pairs(V, W, T, solo=True)
    assert np.array_equal(V1, sV1) and np.array_equal(sums, ssums)
    ext, a, r = pair_step_ext(V, W, T, PAIR_SIGMA, PAIR_RSCALE)
    err = np.sqrt(((parts(V1.reshape(C_RUN, 2, m)) - ext) ** 2).sum(axis=(1, 3)))
    bound = 4 * EPS * np.maximum(a, r)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0, np.inf))
    print(f"L={L} cplx={cplx} vecT={vecT}: worst error / bound {float(ratio.max()):.3f}")
    assert np.isfinite(V1.view(float)).all() and np.all(err <= bound)
    v1 = V1.reshape(C_RUN, 2, m)
    if m >= 8:
        i = np.arange(m) % 8
        on = (2 + 4j, 4 + 8j) if cplx else (6.0, 8.0)
        assert np.all(a[:, i == 1] == 5) and np.all(v1[:, 0, i == 1] == 0.5 * on[0]) and np.all(v1[:, 1, i == 1] == 0.5 * on[1])
        assert np.all(v1[:, :, i == 2] == 0)
        if vecT:
            assert np.all(v1[:, :, i == 3] == 0) and np.all(a[:, i == 3] > 0)
        inside = a < r
        keep = np.broadcast_to(inside[:, None, :], v1.shape)
        exact_in = (V + PAIR_SIGMA * W).reshape(C_RUN, 2, m)[keep]
        assert inside.any() and (a > r).any() and np.abs(v1[keep] - exact_in).max() <= EPS * np.abs(exact_in).max()
    Tm = np.broadcast_to(np.asarray(T, dtype=float), (m,))
    want = [_ld_sum(_pair2(V1 - V)), _ld_sum(_pair2(V1)), _ld_sum(Tm * np.sqrt(_pair2(W)))]
    for k, w in enumerate(want):
        diff = np.abs(sums[:, k].astype(LD) - w)
        print(f"  sum {k}: |sum - long-double sum| / sum {(diff / np.where(w == 0, 1, w)).astype(float)} (bound {m * EPS:.3e})")
        assert np.all(diff <= m * EPS * w)


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_pair_projection_with_an_infinite_radius(cplx):
    """r = inf never binds: the pair is v + sigma w, exactly, however large"""
    import torch

    from pxmcmc_amd import ops

    rng = np.random.default_rng(7)
    V, W = _draw(rng, cplx, 1, 16), 1e150 * _draw(rng, cplx, 1, 16)
    T = np.full(8, np.inf)
    T[::2] = 1.0
    V1, _ = ops.pd_dual_step_pairs(ops.as_device(V), ops.as_device(W), ops.as_device(T, torch.float64), 0.5, 0.5)
    v1, w = V1.cpu().numpy().reshape(2, 8), (V + 0.5 * W).reshape(2, 8)
    assert np.array_equal(v1[:, 1::2], w[:, 1::2]) and np.isfinite(v1.view(float)).all()
    nrm = np.sqrt((np.abs(v1[:, ::2]) ** 2).sum(axis=0))
    assert np.all(np.abs(nrm - 0.5) <= 4 * EPS)


# ---- 3. fused against composed, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", SIZES)
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_fused_steps_equal_the_composed_launches_bit_for_bit(tables, L, cplx):
    """tv_primal_step = tv_grad_adjoint then pd_primal_step; tv_dual_step = tv_grad then pd_dual_step_pairs (scalar and
    vector T); the G = None, Xbar = None form = skrock_stage(z, 1, e = -1, V = A^H v): outputs and sums, and every chain of
    the batch equals the chain run alone"""
    import torch

    from pxmcmc_amd import ops

    ab_dev, _ = tables[L]
    m = L * (2 * L - 1)
    rng = np.random.default_rng(500 + 2 * L + cplx)
    X, G, Xb = _draw(rng, cplx, C_RUN, m), 30.0 * _draw(rng, cplx, C_RUN, m), _draw(rng, cplx, C_RUN, m)
    V = 3.0 * _draw(rng, cplx, C_RUN, 2 * m)
    T = ops.as_device(0.4 * (0.5 + rng.random(m)), torch.float64)
    tau, sigma, rscale = 0.037, 0.81, 1.3
    bX, bG, bXb, bV = _dev(X), _dev(G), _dev(Xb), _dev(V)
    runs = {}
    for solo in (False, True):
        o = dict(
            fX1=_nan(bX), fXbar=_nan(bX), fps=_nan(bX, 2, real=True), cX1=_nan(bX), cXbar=_nan(bX), cps=_nan(bX, 2, real=True),
            fV1=_nan(bV), fds=_nan(bV, 3, real=True), cV1=_nan(bV), cds=_nan(bV, 3, real=True),
            fV1s=_nan(bV), fdss=_nan(bV, 3, real=True), cV1s=_nan(bV), cdss=_nan(bV, 3, real=True),
            fP=_nan(bX), fPs=_nan(bX, 2, real=True), cP=_nan(bX))
        for sl in _launches(solo):
            ops.tv_primal_step(bX[sl], bG[sl], bV[sl], ab_dev, tau, out=(o["fX1"][sl], o["fXbar"][sl]), sums=o["fps"][sl])
            ops.pd_primal_step(bX[sl], bG[sl], ops.tv_grad_adjoint(bV[sl], ab_dev), tau, out=(o["cX1"][sl], o["cXbar"][sl]),
                               sums=o["cps"][sl])
            ops.tv_dual_step(bV[sl], bXb[sl], ab_dev, T, sigma, rscale, out=o["fV1"][sl], sums=o["fds"][sl])
            ops.pd_dual_step_pairs(bV[sl], ops.tv_grad(bXb[sl], ab_dev), T, sigma, rscale, out=o["cV1"][sl], sums=o["cds"][sl])
            ops.tv_dual_step(bV[sl], bXb[sl], ab_dev, 0.3, sigma, rscale, out=o["fV1s"][sl], sums=o["fdss"][sl])
            ops.pd_dual_step_pairs(bV[sl], ops.tv_grad(bXb[sl], ab_dev), 0.3, sigma, rscale, out=o["cV1s"][sl], sums=o["cdss"][sl])
            x1, none, _ = ops.tv_primal_step(bX[sl], None, bV[sl], ab_dev, 1.0, out=o["fP"][sl], xbar=False, sums=o["fPs"][sl])
            assert none is None
            ops.skrock_stage(bX[sl], 1.0, e=-1.0, V=ops.tv_grad_adjoint(bV[sl], ab_dev), out=o["cP"][sl])
        torch.cuda.synchronize()
        assert _untouched(*o.values())
        runs[solo] = {k: t[:C_RUN].cpu().numpy() for k, t in o.items()}
    r = runs[False]
    for k in r:
        assert np.isfinite(r[k].view(float)).all(), k
        assert np.array_equal(r[k], runs[True][k]), k
    for f, c in (("fX1", "cX1"), ("fXbar", "cXbar"), ("fps", "cps"), ("fV1", "cV1"), ("fds", "cds"), ("fV1s", "cV1s"),
                 ("fdss", "cdss"), ("fP", "cP")):
        assert np.array_equal(r[f], r[c]), (f, c)
    assert not np.array_equal(r["fV1"], r["fV1s"]) and np.any(r["fV1"] != V)  # the projection binds somewhere


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_launched():
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError, lib

    dev = ops.device()
    L, C = 3, 2
    m = L * (2 * L - 1)
    ab = ops.tv_ring_coefs(L)
    x, g, xb = (torch.ones((C, m), dtype=torch.float64, device=dev) for _ in range(3))
    v, w = (torch.ones((C, 2 * m), dtype=torch.float64, device=dev) for _ in range(2))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
    o1, o2, oc, val, ps, ds = nan(C, m), nan(C, m), nan(C, 2 * m), nan(C), nan(C, 2), nan(C, 3)
    scratch = ops.pd_scratch(C, dev)
    Tv = torch.ones(m, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731

    def grad(X=x, AB=ab, out=oc, L=L, C=C, dtype=0):
        return lib.pxm_tv_grad(p(X), p(AB), p(out), L, C, dtype, st)

    def adjoint(V=v, AB=ab, out=o1, L=L, C=C, dtype=0):
        return lib.pxm_tv_grad_adjoint(p(V), p(AB), p(out), L, C, dtype, st)

    def value(X=x, AB=ab, T=None, Ts=1.0, out=val, scr=scratch, L=L, C=C, dtype=0):
        return lib.pxm_tv_value(p(X), p(AB), p(T), Ts, p(out), p(scr), L, C, dtype, st)

    def pairs(V=v, W=w, T=None, Ts=0.1, sigma=0.5, rscale=1.0, V1=oc, sums=ds, scr=scratch, m=m, C=C, dtype=0):
        return lib.pxm_pd_dual_step_pairs(p(V), p(W), p(T), Ts, sigma, rscale, p(V1), p(sums), p(scr), m, C, dtype, st)

    def primal(X=x, G=g, V=v, AB=ab, tau=0.1, X1=o1, Xb=o2, sums=ps, scr=scratch, L=L, C=C, dtype=0):
        return lib.pxm_tv_primal_step(p(X), p(G), p(V), p(AB), tau, p(X1), p(Xb), p(sums), p(scr), L, C, dtype, st)

    def dual(V=v, Xb=xb, AB=ab, T=None, Ts=0.1, sigma=0.5, rscale=1.0, V1=oc, sums=ds, scr=scratch, L=L, C=C, dtype=0):
        return lib.pxm_tv_dual_step(p(V), p(Xb), p(AB), p(T), Ts, sigma, rscale, p(V1), p(sums), p(scr), L, C, dtype, st)

    refused = {
        "pxm_tv_grad": [lambda: grad(out=x), lambda: grad(L=1), lambda: grad(C=0), lambda: grad(C=65536), lambda: grad(dtype=2),
                        lambda: grad(AB=None), lambda: grad(X=None), lambda: grad(out=None)],
        "pxm_tv_grad_adjoint": [lambda: adjoint(out=v), lambda: adjoint(L=1), lambda: adjoint(L=0), lambda: adjoint(AB=None),
                                lambda: adjoint(dtype=-1), lambda: adjoint(out=None)],
        "pxm_tv_value": [lambda: value(out=x), lambda: value(L=1), lambda: value(Ts=-1.0), lambda: value(Ts=float("nan")),
                         lambda: value(scr=None), lambda: value(out=None), lambda: value(out=scratch)],
        "pxm_pd_dual_step_pairs": [lambda: pairs(V1=v), lambda: pairs(V1=w), lambda: pairs(sigma=0.0), lambda: pairs(sigma=-1.0),
                                   lambda: pairs(sigma=float("inf")), lambda: pairs(rscale=0.0), lambda: pairs(Ts=-0.1),
                                   lambda: pairs(m=-1), lambda: pairs(C=65536), lambda: pairs(sums=None), lambda: pairs(W=None)],
        "pxm_tv_primal_step": [lambda: primal(X1=x), lambda: primal(Xb=g), lambda: primal(X1=v), lambda: primal(Xb=o1),
                               lambda: primal(tau=0.0), lambda: primal(tau=-0.1), lambda: primal(tau=float("nan")),
                               lambda: primal(L=1), lambda: primal(X1=None), lambda: primal(V=None), lambda: primal(sums=None)],
        "pxm_tv_dual_step": [lambda: dual(V1=v), lambda: dual(V1=xb), lambda: dual(sigma=0.0), lambda: dual(rscale=-1.0),
                             lambda: dual(Ts=-0.1), lambda: dual(L=1), lambda: dual(AB=None), lambda: dual(scr=None),
                             lambda: dual(T=oc)],
    }
    for fn, calls in refused.items():
        for k, call in enumerate(calls):
            assert call() < 0, (fn, k)
            msg = lib.pxm_last_error().decode()
            assert msg.startswith(fn + ":"), (fn, k, msg)
    torch.cuda.synchronize()
    for t in (o1, o2, oc, val, ps, ds):
        assert torch.isnan(t).all()  # nothing ran
    for t in (x, g, xb, v, w):
        assert torch.equal(t, torch.ones_like(t))
    # through the wrappers: the library's refusal arrives as PxmError, the wrappers' own checks as ValueError / TypeError
    with pytest.raises(PxmError, match="alias"):
        ops.tv_primal_step(x, g, v, ab, 0.1, out=(x, o2))
    with pytest.raises(PxmError, match="tau"):
        ops.tv_primal_step(x, g, v, ab, 0.0)
    with pytest.raises(PxmError, match="sigma"):
        ops.tv_dual_step(v, xb, ab, 0.1, -0.5, 1.0)
    with pytest.raises(ValueError, match="per pixel"):  # wrong T length: the coefficient length instead of the pixel count
        ops.tv_dual_step(v, xb, ab, torch.ones(2 * m, dtype=torch.float64, device=dev), 0.5, 1.0)
    with pytest.raises(ValueError, match="per pixel"):
        ops.pd_dual_step_pairs(v, w, torch.ones(2 * m, dtype=torch.float64, device=dev), 0.5, 1.0)
    with pytest.raises(ValueError, match="per pixel"):
        ops.tv_value(x, ab, torch.ones(m + 1, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):  # wrong plane count: one plane, three planes
        ops.tv_grad_adjoint(x, ab)
    with pytest.raises(ValueError):
        ops.tv_primal_step(x, g, torch.ones((C, 3 * m), dtype=torch.float64, device=dev), ab, 0.1)
    with pytest.raises(ValueError):
        ops.tv_dual_step(x, xb, ab, 0.1, 0.5, 1.0)
    with pytest.raises(ValueError):
        ops.pd_dual_step_pairs(v[:, :-1], w[:, :-1], 0.1, 0.5, 1.0)
    with pytest.raises(ValueError):  # an image of another size than the table's
        ops.tv_grad(x[:, :-1], ab)
    with pytest.raises(ValueError):
        ops.tv_value(x, ab, None)
    with pytest.raises(ValueError):  # a result buffer of another dtype
        ops.tv_grad(x, ab, out=oc.to(torch.complex128))
    with pytest.raises(TypeError):
        ops.tv_grad(x, ab.cpu())
    with pytest.raises(TypeError):
        ops.tv_grad(x, ab.reshape(-1))
    with pytest.raises(ValueError):
        ops.tv_ring_coefs(1)
    # and the valid calls go through
    assert grad() == 0 and adjoint() == 0 and value() == 0 and primal() == 0 and dual(T=Tv, V1=w) == 0 and pairs(T=Tv, V1=xb.new_empty((C, 2 * m))) == 0
    torch.cuda.synchronize()
    for t in (o1, o2, oc, val, ps, ds):
        assert torch.isfinite(t).all()


# ---- 5. PrimalDual with TV_S2 on the polar cap -----------------------------------------------------------------------------------------
def _cap_setup(L, cplx):
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import TV_S2
    from pxmcmc_amd.transforms import IdentityTransform

    p = polar_cap_problem(L, cplx=cplx)
    P = p["d"].size
    op = ForwardOperator(p["d"], p["sig"], "analysis", IdentityTransform(), Identity(P, P), nparams=P)
    reg = TV_S2(L, p["T"])
    prm = PxMCMCParams(lmda=p["lmda"], mu=1.0, verbosity=0, complex=cplx)
    X0 = np.stack([np.zeros_like(p["d"]), p["d"].copy()])
    return p, op, reg, prm, X0


def _four_runs(op, reg, prm, X0, iters):
    """eager / replayed x fused / composed -> {(graph, fused): (X, estimator)}"""
    from pxmcmc_amd.optim import PrimalDual

    runs = {}
    for graph in (True, False):
        for fused in (True, False):
            est = PrimalDual(op, reg, prm, nchains=2, tol=0.0, max_iter=iters, check_every=iters // 2, use_graph=graph, fused=fused)
            X = est.run(start_point=X0)
            assert est.used_graph == graph, est.graph_error
            assert est.fused == fused
            runs[(graph, fused)] = (X, est)
    return runs


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_primal_dual_tv_50_iterations(cplx):
    """L = 8, 2 chains from two starts: eager against replayed and fused against composed are bit-equal (state, dual and
    traces), and equal primal_dual_pairs_np with the estimator's steps to 1e-10 relative.  The gradient is the estimator's:
    with complex data and a real sig_d the inverse covariance is e^{-i pi/4} / sig^2 and g takes its real part
    (optim.gradient_operator)"""
    import torch

    from pxmcmc_amd.tv_np import primal_dual_pairs_np

    p, op, reg, prm, X0 = _cap_setup(8, cplx)
    runs = _four_runs(op, reg, prm, X0, 50)
    X, est = runs[(True, True)]
    assert X.dtype == (np.complex128 if cplx else np.float64) and est.X_map.dtype == (torch.complex128 if cplx else torch.float64)
    for key, (Xo, eo) in runs.items():
        assert np.array_equal(X, Xo) and np.array_equal(est.V_map.cpu().numpy(), eo.V_map.cpu().numpy()), key
        for k in ("objective", "data_term", "prior_term", "rel_change", "rel_change_dual", "stationarity", "last_steps"):
            assert np.array_equal(getattr(est, k), getattr(eo, k)), (key, k)
    assert est.A_norm2 == pytest.approx(p["a2"] * (1 + 1e-4), rel=2e-4) and est.A_norm2 <= p["a2"] * (1 + 1e-4) * (1 + 1e-10)
    V = est.V_map.cpu().numpy()
    ic = est.gradient_op.invcov.diag.real.cpu().numpy()
    assert np.allclose(ic, p["ic"] * (np.cos(np.pi / 4) if cplx else 1.0), rtol=4 * EPS)
    for c in range(2):
        x, v, _ = primal_dual_pairs_np(lambda x: ic * (x - p["d"]), p["A"], p["AH"], p["T"], p["lmda"], est.tau, est.sigma, X0[c], 50)
        ex, ev = np.abs(X[c] - x).max() / np.abs(x).max(), np.abs(V[c] - v).max() / np.abs(v).max()
        print(f"cplx={cplx} chain {c}: |x - numpy| / max|x| = {ex:.3e}, |v - numpy| / max|v| = {ev:.3e}")
        assert ex <= 1e-10 and ev <= 1e-10
    # the prior term is the TV value of the state
    assert np.allclose(est.prior_term[-1], reg.prior(est.X_map).cpu().numpy() / p["lmda"], rtol=64 * EPS)


def test_primal_dual_tv_reaches_the_map():
    """L = 8, real data, tolerance 1e-6 checked every iteration: the iteration count equals the numpy statement's for both
    starts, the relative duality gap is at most twice the one numpy reaches, and V_map satisfies the pair-norm constraint"""
    from pxmcmc_amd.optim import PrimalDual
    from pxmcmc_amd.tv_np import pair_norm_np, primal_dual_pairs_np

    p, op, reg, prm, X0 = _cap_setup(8, False)
    est = PrimalDual(op, reg, prm, nchains=2, tol=CAP_TOL, max_iter=6000, check_every=1)
    X = est.run(start_point=X0)
    V = est.V_map.cpu().numpy()
    assert est.used_graph and est.fused and est.converged.all()
    print(f"tau {est.tau:.4e} sigma {est.sigma:.4e} ||A||^2 {est.A_norm2:.4f} L_g {est.L_g:.4f}")
    # chain c keeps stepping until both have stopped: the count is compared at the chain's own stop, the gap at the end
    for c in range(2):
        x, v, info = primal_dual_pairs_np(p["grad"], p["A"], p["AH"], p["T"], p["lmda"], est.tau, est.sigma, X0[c], 6000, tol=CAP_TOL)
        gap_np, gap = cap_relative_gap(p, x, v), cap_relative_gap(p, X[c], V[c])
        print(f"chain {c}: numpy {info['niter']} iterations, gap {gap_np:.3e}; device {est.niter[c]} iterations, gap {gap:.3e}")
        assert info["converged"] and est.niter[c] == info["niter"]
        assert 0 <= gap <= 2 * gap_np
        assert np.all(pair_norm_np(V[c]) <= p["T"] / p["lmda"] * (1 + 4 * EPS))


def test_a_pairs_prior_without_fused_launches_takes_the_composed_route():
    """any prior with ``pairs`` is accepted: one that offers no fused launches runs on A, A^H, pd_primal_step and
    pd_dual_step_pairs and gives TV_S2's bits; T must have one value per pixel, not per coefficient"""
    from pxmcmc_amd.optim import PrimalDual

    class PairsPrior:
        pairs, setting = True, "analysis"

        def __init__(self, tr, T):
            self.fwd, self.adj, self.T = tr.forward_adjoint, tr.forward, T

    p, op, reg, prm, X0 = _cap_setup(5, False)
    m = p["d"].size
    plain = PairsPrior(reg.transform, np.full(m, p["T"]))
    est = PrimalDual(op, plain, prm, nchains=2, tol=0.0, max_iter=20, check_every=20)
    ref = PrimalDual(op, reg, prm, nchains=2, tol=0.0, max_iter=20, check_every=20)
    assert not est.fused and ref.fused and est.ncoefs == 2 * m
    X, Xr = est.run(start_point=X0), ref.run(start_point=X0)
    assert np.array_equal(X, Xr) and np.array_equal(est.V_map.cpu().numpy(), ref.V_map.cpu().numpy())
    assert np.array_equal(est.prior_term, ref.prior_term) and not np.array_equal(X, X0)
    with pytest.raises(ValueError, match="two planes"):
        PrimalDual(op, PairsPrior(reg.transform, np.full(2 * m, p["T"])), prm)


# ---- 6. the anisotropic form through the generic launches ------------------------------------------------------------------------------
def test_anisotropic_tv_through_l1_analysis():
    """SphericalGradientTransform with L1_Analysis at L = 5: the operator kernels under the generic pd_primal_step /
    pd_dual_step; 30 iterations equal primal_dual_np (V1 and X) to 1e-10 relative, and operator_norm2 is within its own
    tolerance of the dense value and never above it"""
    import torch

    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.optim import PrimalDual, operator_norm2
    from pxmcmc_amd.optim_np import primal_dual_np
    from pxmcmc_amd.prior import L1_Analysis
    from pxmcmc_amd.transforms import IdentityTransform, SphericalGradientTransform

    L = 5
    p = polar_cap_problem(L)
    P = p["d"].size
    tr = SphericalGradientTransform(L)
    assert tr.ncoefs == 2 * P
    with pytest.raises(NotImplementedError):
        tr.inverse(p["d"])
    with pytest.raises(NotImplementedError):
        tr.inverse_adjoint(p["d"])
    got = tr.forward(p["d"])
    assert isinstance(got, np.ndarray) and np.abs(got - p["A"](p["d"])).max() <= 4 * EPS * np.abs(got).max()
    T = 5.0 * (0.5 + np.random.default_rng(4).random(2 * P))
    reg = L1_Analysis(tr.forward_adjoint, tr.forward, T)
    op = ForwardOperator(p["d"], p["sig"], "analysis", IdentityTransform(), Identity(P, P), nparams=P)
    est = PrimalDual(op, reg, PxMCMCParams(lmda=1.0, mu=1.0, verbosity=0), tol=0.0, max_iter=30, check_every=30)
    assert not est.fused
    X = est.run(start_point=np.zeros(P))
    x, v, _ = primal_dual_np(p["grad"], p["A"], p["AH"], T, 1.0, est.tau, est.sigma, np.zeros(P), 30)
    V = est.V_map.cpu().numpy()[0]
    ex, ev = np.abs(X - x).max() / np.abs(x).max(), np.abs(V - v).max() / np.abs(v).max()
    print(f"anisotropic, 30 iterations: |x - numpy| {ex:.3e}, |v - numpy| {ev:.3e} (relative)")
    assert est.used_graph and ex <= 1e-10 and ev <= 1e-10 and np.all(np.abs(V) <= T * (1 + 4 * EPS)) and np.any(np.abs(V) == T)
    dense = np.linalg.norm(dense_gradient(L, p["ab"]), 2) ** 2
    tol = 1e-4
    a2 = operator_norm2(tr.forward_adjoint, tr.forward, P, torch.float64, iters=1000, tol=tol)
    print(f"||A||^2: power iteration {a2:.8f}, dense {dense:.8f}, relative gap {(dense - a2) / dense:.3e}")
    assert a2 <= dense * (1 + 1e-10) and dense - a2 <= tol * dense
    assert dense == pytest.approx(p["a2"], rel=1e-12)


# ---- 7. the exact prox ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 12])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_tv_prox_and_prior(L, cplx):
    """TV_S2.proxf equals analysis_prox_pairs_np at the same iteration count and step to 1e-11 relative, equals the composed
    route bit for bit, is a pure function of its argument, and a captured graph replays it bit for bit; TV_S2.prior equals
    tv_value_np (m terms: m eps relative)"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.mcmc.engine import capture
    from pxmcmc_amd.optim import analysis_prox
    from pxmcmc_amd.prior import TV_S2
    from pxmcmc_amd.tv_np import analysis_prox_pairs_np, pair_norm_np, tv_value_np

    p = polar_cap_problem(L, cplx=cplx, seed=3)
    m = p["d"].size
    rng = np.random.default_rng(70 + L)
    Z = np.stack([p["d"], p["d"] + 0.1 * _draw(rng, cplx, m)])
    T = 0.2 * (0.5 + rng.random(m))
    reg = TV_S2(L, T, prox_iters=12)
    assert reg.pairs and reg.setting == "analysis" and reg.prox_iters == 12
    got, v = analysis_prox(reg, Z, 12, return_dual=True)
    sigma = reg._prox_sigma[(m, torch.complex128 if cplx else torch.float64)]
    assert sigma == pytest.approx(1 / (p["a2"] * (1 + 1e-4)), rel=2e-4) and sigma * p["a2"] < 1
    assert isinstance(got, np.ndarray) and got.dtype == Z.dtype and np.array_equal(reg.proxf(Z), got)
    assert np.all(pair_norm_np(v.cpu().numpy()) <= T * (1 + 4 * EPS))
    for c in range(2):
        want = analysis_prox_pairs_np(p["A"], p["AH"], T, Z[c], 12, sigma)
        err = np.abs(got[c] - want).max() / np.abs(Z[c]).max()
        print(f"L={L} cplx={cplx} chain {c}: |prox - numpy| / max|Z| = {err:.3e}, moved {np.abs(want - Z[c]).max():.3e}")
        assert err <= 1e-11 and np.abs(want - Z[c]).max() > 1e-3
    assert np.array_equal(analysis_prox(reg, Z, 12, fused=False), got)
    assert np.array_equal(reg.proxf(Z[0]), got[0])
    z = ops.as_device(Z)
    out = torch.full_like(z, float("nan"))
    body = lambda: out.copy_(reg.proxf(z))  # noqa: E731
    graphs, error = capture(body, lambda: out.fill_(float("nan")), [body])
    assert graphs is not None, error
    assert torch.isnan(out.real if cplx else out).all()  # capture does not execute
    graphs[0].replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), got)
    z.copy_(ops.as_device(Z[::-1].copy()))  # the graph reads its static input
    graphs[0].replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), got[::-1])
    pr = reg.prior(Z)
    want = tv_value_np(Z, p["ab"], L, T)
    assert isinstance(pr, torch.Tensor) and np.allclose(pr.cpu().numpy(), want, rtol=gamma(8) + m * EPS, atol=0)
    assert isinstance(reg.prior(Z[0]), float) and reg.prior(Z[0]) == float(pr[0])
    with pytest.raises(ValueError, match="per pixel"):
        TV_S2(L, np.ones(2 * m))


# ---- 8. the samplers on a float64 state ----------------------------------------------------------------------------------------------
def _sampler_setup(L=5):
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import TV_S2
    from pxmcmc_amd.transforms import IdentityTransform

    p = polar_cap_problem(L, seed=5)
    P = p["d"].size
    lmda, mu = 1e-2, 1.0
    op = ForwardOperator(p["d"], p["sig"], "analysis", measurement=Identity(P, P), nparams=P, transform=IdentityTransform())
    reg = TV_S2(L, lmda * mu * 2.0, prox_iters=4)
    delta = 0.8 / (p["ic"] + 1 / lmda)
    return p, op, reg, lmda, mu, delta


def test_myula_with_tv_against_the_numpy_statement():
    """L = 5, 2 chains, 20 iterations, float64 state.  With host-supplied noise (rng = "numpy": randn(N) per chain and
    iteration from numpy's global stream) the chain equals the numpy statement of the iteration,
    X1 = (1 - d/l) X + (d/l) prox(X) - d gradg(X) + sqrt(2 d) w with prox = analysis_prox_pairs_np, to 1e-10 relative; with
    the device stream, graph replay equals eager bit for bit."""
    import torch

    from pxmcmc_amd.mcmc import MYULA, PxMCMCParams
    from pxmcmc_amd.tv_np import analysis_prox_pairs_np

    p, op, reg, lmda, mu, delta = _sampler_setup()
    C, P = 2, p["d"].size
    prm = PxMCMCParams(lmda=lmda, delta=delta, mu=mu, nsamples=20, nburn=0, ngap=1, verbosity=0)
    X0 = 0.1 * p["d"]
    s = MYULA(op, reg, prm, nchains=C, rng="numpy")
    np.random.seed(1234)
    _quiet(s.run, start_point=X0)
    assert s.X_curr.dtype == torch.float64 and s.niter == 20
    sigma = reg._prox_sigma[(P, torch.float64)]
    np.random.seed(1234)
    x = np.stack([X0, X0])
    for _ in range(20):
        w = np.stack([np.random.randn(P) for _ in range(C)])
        px = np.stack([analysis_prox_pairs_np(p["A"], p["AH"], reg.T, xc, 4, sigma) for xc in x])
        x = (1 - delta / lmda) * x + (delta / lmda) * px - delta * p["grad"](x) + np.sqrt(2 * delta) * w
    err = np.abs(s.X_curr.cpu().numpy() - x).max() / np.abs(x).max()
    print(f"MYULA with TV_S2, 20 iterations: |X - numpy| / max|X| = {err:.3e}")
    assert err <= 1e-10 and not np.array_equal(x[0], x[1])
    runs = {}
    for graph in (True, False):
        s = MYULA(op, reg, prm, nchains=C, seed=6, use_graph=graph)
        _quiet(s.run, start_point=X0)
        assert s.used_graph == graph, s.graph_error
        runs[graph] = (np.asarray(s.chain).copy(), s.X_curr.cpu().numpy().copy(), np.asarray(s.logPi).copy())
    for a, b in zip(runs[True], runs[False]):
        assert np.isfinite(a.view(float)).all() and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["PxMALA", "SKROCK"])
def test_pxmala_and_skrock_run_with_tv(name):
    """10 iterations each in the analysis setting with TV_S2 on a float64 state: finite values, replayed from the graph, and
    the replayed run equals the eager one bit for bit"""
    import torch

    from pxmcmc_amd import mcmc

    p, op, reg, lmda, mu, delta = _sampler_setup()
    prm = mcmc.PxMCMCParams(lmda=lmda, delta=delta, mu=mu, nsamples=10, nburn=0, ngap=1, verbosity=0, s=3)
    kw = dict(max_iter=10) if name == "PxMALA" else {}
    runs = {}
    for graph in (True, False):
        s = getattr(mcmc, name)(op, reg, prm, nchains=2, seed=9, use_graph=graph, **kw)
        _quiet(s.run, start_point=0.1 * p["d"])
        assert s.used_graph == graph, s.graph_error
        assert s.niter == 10 and s.X_curr.dtype == torch.float64 and torch.isfinite(s.X_curr).all()
        assert np.isfinite(np.asarray(s.logPi)).all() and np.isfinite(np.asarray(s.chain).view(float)).all()
        runs[graph] = (s.X_curr.cpu().numpy().copy(), np.asarray(s.chain).copy(), np.asarray(s.logPi).copy())
    for a, b in zip(runs[True], runs[False]):
        assert np.array_equal(a, b)
    assert np.any(runs[True][0] != 0.1 * p["d"])
