"""The generic kernels past their grid caps (csrc/elementwise.hip ew_grid, skrock.hip sk_grid, spmv.hip pxm_csr_matvec and its
transpose helper): every operation at a length that needs a second trip of the kernel's grid-stride loop, element by element
against the long-double models and derived bounds of tests/test_generic_caps_host.py.  Every output buffer the test can own is
pre-filled with NaN, so an element the kernel never writes fails instead of inheriting a recycled allocation, and every
assertion names the worst element."""
import numpy as np
import pytest

import test_generic_caps_host as H
from test_generic_caps_host import assert_same, assert_within

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _np(t):
    return t.cpu().numpy()


def _dev(x):
    """a copy of a shared (read-only) host array, or a scalar threshold as it is, on the device"""
    from pxmcmc_amd import ops

    return x if np.ndim(x) == 0 else ops.as_device(np.array(x))


def _nan_like(x):
    import torch

    return torch.full_like(x, NAN)


def _nan(shape, cplx):
    import torch

    from pxmcmc_amd import ops

    return torch.full(shape, NAN, dtype=torch.complex128 if cplx else torch.float64, device=ops.device())


# ---- a. elementwise: n = 524288 + 257, C = 2 -------------------------------------------------------------------------------------
def _soft(x, T):
    """ops.soft with a NaN-filled output of the test's own"""
    from pxmcmc_amd._lib import check, lib
    from pxmcmc_amd.ops._args import _dt, _p, _stream, _vecT

    Tv, Ts = _vecT(_dev(T), x.shape[1], x.device)
    out = _nan_like(x)
    check(lib.pxm_soft(_p(x), _p(Tv), Ts, _p(out), x.shape[1], x.shape[0], _dt(x), _stream()))
    return _np(out)


@pytest.mark.parametrize("cplx", [False, True])
def test_soft_past_the_cap(cplx):
    v = H.ew_inputs(cplx)
    X = v["X"]
    assert X.shape == (2, 524545)
    xd = _dev(X)
    for name, T in (("scalar T", H.EW_TS), ("vector T", v["T"])):
        got = _soft(xd, T)
        if cplx:
            assert_within(got, H.soft_model(X, T), H.soft_cplx_bound(X), f"complex soft, {name}")
        else:
            assert_same(got, H.soft_f64(X, T), f"real soft, {name}")


@pytest.mark.parametrize("kind", ["real", "complex-real-invcov", "complex-complex-invcov"])
def test_residual_past_the_cap(kind):
    from pxmcmc_amd._lib import check, lib
    from pxmcmc_amd.ops._args import _dt, _p, _stream

    cplx = kind != "real"
    v = H.ew_inputs(cplx)
    p, d, ic = v["X"], v["d"], v["ic_cplx" if kind == "complex-complex-invcov" else "ic_real"]
    pd, dd, icd = _dev(p), _dev(d), _dev(ic)
    out = _nan_like(pd)
    check(lib.pxm_residual_grad(_p(pd), _p(dd), _p(icd), int(icd.is_complex()), _p(out), p.shape[1], p.shape[0], _dt(pd), _stream()))
    assert_within(_np(out), H.residual_model(p, d, ic), H.residual_bound(p, d, ic), f"residual, {kind}")


@pytest.mark.parametrize("cplx,noise_cplx", [(False, False), (True, False), (True, True)])
def test_chain_and_myula_step_past_the_cap(cplx, noise_cplx):
    """injected noise; scalar delta and one delta per chain; the MYULA step under a scalar and under a vector threshold"""
    import torch

    from pxmcmc_amd import ops

    v = H.ew_inputs(cplx)
    X, P, g, w = v["X"], v["P"], v["g"], v["w_cplx" if noise_cplx else "w_real"]
    xd, pd, gd, wd = (_dev(t) for t in (X, P, g, w))
    tag = f"{'complex' if cplx else 'real'} state, {'complex' if noise_cplx else 'real'} noise"
    for dname, delta in (("scalar delta", H.EW_DELTA), ("per-chain delta", np.array(H.EW_DELTAS))):
        ddev = delta if np.ndim(delta) == 0 else torch.tensor(delta, dtype=torch.float64, device=ops.device())
        out = _nan_like(xd)
        ops.chain_step(xd, pd, gd, ddev, H.EW_LMDA, noise=wd, out=out)
        model, bound = H.chain_step_model(X, P, g, w, delta, H.EW_LMDA)
        assert_within(_np(out), model, bound, f"chain step, {tag}, {dname}")
        for tname, T in (("scalar T", H.EW_TS), ("vector T", v["T"])):
            out = _nan_like(xd)
            ops.myula_step(xd, gd, _dev(T), ddev, H.EW_LMDA, noise=wd, out=out)
            model, bound = H.myula_step_model(X, g, T, w, delta, H.EW_LMDA)
            assert_within(_np(out), model, bound, f"MYULA step, {tag}, {dname}, {tname}")


def test_weaklensing_pieces_past_the_cap():
    """harmonic mapping at n = 524545; mask gather and scatter of 524545 data out of / into 525788 pixels, with and without
    weights; the scatter leaves exact zeros everywhere else"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import check, lib
    from pxmcmc_amd.ops._args import _p, _stream

    v = H.wl_inputs()
    C, n, npix = H.EW_C, H.EW_N, H.WL_NPIX
    assert (n, npix) == (524545, 524288 + 1500)
    flm, kern = _dev(v["flm"]), _dev(v["kernel"])
    out = _nan_like(flm)
    check(lib.pxm_wl_harmonic_mapping(_p(flm), _p(kern), _p(out), n, C, _stream()))
    got = _np(out)
    assert_same(got, H.wl_mapping_f64(v["flm"], v["kernel"]), "weak-lensing harmonic mapping")
    assert_same(got[:, :4], 0.0, "weak-lensing harmonic mapping, first four entries")
    idx = v["idx"]
    idxd = torch.from_numpy(idx.copy()).to(ops.device())
    f, g = _dev(v["f"]), _dev(v["g"])
    hole = np.ones(npix, dtype=bool)
    hole[idx] = False
    assert hole.sum() == npix - n
    for wname, w in (("no weights", None), ("weights", v["w"])):
        wd = None if w is None else _dev(w)
        out = _nan((C, n), True)
        check(lib.pxm_wl_mask_gather(_p(f), _p(idxd), _p(wd), _p(out), npix, n, C, _stream()))
        assert_same(_np(out), H.wl_gather_f64(v["f"], idx, w), f"weak-lensing mask gather, {wname}")
        full = _nan((C, npix), True)
        check(lib.pxm_wl_mask_scatter(_p(g), _p(idxd), _p(wd), _p(full), npix, n, C, _stream()))
        got = _np(full)
        assert_same(got, H.wl_scatter_f64(v["g"], idx, npix, w), f"weak-lensing mask scatter, {wname}")
        assert_same(got[:, hole], 0.0, f"weak-lensing mask scatter, {wname}: masked pixels")


# ---- b. Philox past the first pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise64", [True, False])
def test_philox_stream_past_the_cap(noise64):
    """ops.randn over the whole length against the numpy Philox: the real stream on chains 10, 11, 12 (both halves of a chain
    pair), the complex stream on two chains; tolerances of test_philox_stream_matches_oracle"""
    from oracle import philox
    from pxmcmc_amd import ops

    n, seed, it = H.EW_N, 12345, 77
    bits, atol = (64, 1e-13) if noise64 else (32, 2e-5)
    r = _np(ops.randn(n, C_=3, complex_=False, seed=seed, chain0=10, it=it, noise64=noise64))
    for k in range(3):
        assert_within(r[k], philox.randn_real(n, seed, 10 + k, it, bits), atol, f"real Philox stream, chain {10 + k}, {bits} bits")
    c = _np(ops.randn(n, C_=2, complex_=True, seed=seed, chain0=4, it=it, noise64=noise64))
    for k in range(2):
        assert_within(c[k], philox.randn_complex(n, seed, 4 + k, it, bits), atol, f"complex Philox stream, chain {4 + k}, {bits} bits")


@pytest.mark.parametrize("noise64", [True, False])
def test_myula_step_draws_the_stream_past_the_cap(noise64):
    """X = 0, g = 0, T = 0, delta = 1 / 2: sqrt(2 delta) is exactly 1 and the step's output is its noise, which must be ops.randn
    of the same (seed, chain0, it) bit for bit -- the element index the stepping kernel hands to Philox in its second pass --
    directly and with the iteration split between the argument and the device counter"""
    import torch

    from pxmcmc_amd import ops

    n, seed, it = H.EW_N, 31, 11
    for cplx, C, chain0 in ((False, 3, 10), (True, 2, 4)):
        Z = _np(ops.randn(n, C_=C, complex_=cplx, seed=seed, chain0=chain0, it=it, noise64=noise64))
        zero = torch.zeros((C, n), dtype=torch.complex128 if cplx else torch.float64, device=ops.device())
        kw = dict(noise_complex=cplx, seed=seed, chain0=chain0, noise64=noise64)
        out = _nan_like(zero)
        ops.myula_step(zero, zero, 0.0, 0.5, 1.0, it=it, out=out, **kw)
        assert_same(_np(out), Z, f"MYULA step's Philox draws, {'complex' if cplx else 'real'}")
        cnt = torch.full((1,), it - 4, dtype=torch.int64, device=ops.device())
        out = _nan_like(zero)
        ops.myula_step(zero, zero, 0.0, 0.5, 1.0, it=4, iter_dev=cnt, out=out, **kw)
        assert_same(_np(out), Z, f"MYULA step's Philox draws through iter_dev, {'complex' if cplx else 'real'}")


# ---- c. SKROCK stage: C = 64, n = 2 * 8192 + 257, three passes of 32 workgroups per chain -----------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
def test_skrock_stage_past_the_cap(cplx):
    """test_stage_kernel_matches_numpy (tests/test_gpu_skrock.py) at three passes of the capped grid: its three coefficient sets,
    the prox from a scalar T, from a vector T and given, Z drawn once from the Philox stream and then both regenerated by the
    kernel and fed back as injected noise; the r = 1 call bit-equal to ops.randn"""
    from pxmcmc_amd import ops

    C, n = H.SK_C, H.SK_N
    assert (C, n) == (64, 16641)
    v = H.sk_inputs(cplx)
    U, P, G, V, Tvec = v["U"], v["P"], v["G"], v["V"], v["T"]
    ud, pd, gd, vd = (_dev(t) for t in (U, P, G, V))
    seed, chain0, it = 7, 5, 11
    proxes = {"scalarT": (H.SK_TS, None), "vectorT": (Tvec, None), "given": (None, P)}
    soft = {}
    for noise_cplx in ([True, False] if cplx else [False]):
        ntag = f"{'complex' if cplx else 'real'} state, {'complex' if noise_cplx else 'real'} noise"
        key = dict(noise_complex=noise_cplx, seed=seed, chain0=chain0, it=it)
        for noise64 in (True, False):  # Philox Z of the stage kernel, bit for bit (a = b = c = e = 0, r = 1)
            zd = ops.randn(n, C, complex_=noise_cplx, noise64=noise64, seed=seed, chain0=chain0, it=it)
            out = _nan_like(ud)
            ops.skrock_stage(ud, 0.0, r=1.0, noise64=noise64, out=out, **key)
            assert_same(_np(out), _np(zd), f"SKROCK stage's Philox draws, {ntag}, noise64 = {noise64}")
        zd = ops.randn(n, C, complex_=noise_cplx, noise64=True, seed=seed, chain0=chain0, it=it)
        Z = _np(zd)
        for name, (a, b, c, e, r) in H.SK_COEFS.items():
            for prox in (proxes if b else ["none"]):
                if cplx and not noise_cplx and (r == 0 or prox not in ("none", "given")):
                    continue  # real noise on a complex state: the noise term only, with no prox and with one
                T, Pgiven = proxes[prox] if b else (None, None)
                if b and Pgiven is None and prox not in soft:
                    soft[prox] = H.soft_model(U, T)
                model, bound = H.skrock_stage_model(U, a, b, c, e, r, P=Pgiven if Pgiven is not None else soft.get(prox), G=G, V=V, Z=Z)
                kw = dict(b=b, c=c, e=e, r=r, T=None if T is None else _dev(T), proxf=pd if Pgiven is not None else None, gradg=gd if c else None,
                          V=vd if e else None, noise64=True, **key)
                for how in (("Philox", "injected") if r else ("no noise",)):
                    out = _nan_like(ud)
                    ops.skrock_stage(ud, a, out=out, noise=zd if how == "injected" else None, **kw)
                    assert_within(_np(out), model, bound, f"SKROCK {name}, prox {prox}, {ntag}, {how}")


# ---- d. / e. CSR product ---------------------------------------------------------------------------------------------------------
class _Csr:
    """a CSR matrix on the device, as ops.CsrMatrix holds it, from arrays of the test's own"""

    def __init__(self, indptr, indices, vals, shape):
        import torch

        from pxmcmc_amd import ops

        dev = ops.device()
        self.shape, self.is_complex = shape, np.iscomplexobj(vals)
        self.indptr = torch.from_numpy(np.array(indptr, dtype=np.int64)).to(dev)
        self.indices = torch.from_numpy(np.array(indices, dtype=np.int32)).to(dev)
        self.vals = torch.from_numpy(np.array(vals)).to(dev)

    def matvec(self, x):
        """CsrMatrix.matvec's call of pxm_csr_matvec on [C, ncols], with a NaN-filled output and a NaN-filled scratch"""
        import torch

        from pxmcmc_amd._lib import check, lib
        from pxmcmc_amd.ops._args import _dt, _p, _stream

        assert x.dim() == 2 and x.shape[1] == self.shape[1] and x.is_contiguous() and (x.is_complex() or not self.is_complex)
        out = torch.full((x.shape[0], self.shape[0]), NAN, dtype=x.dtype, device=x.device)
        scratch = torch.full((x.numel(),), NAN, dtype=x.dtype, device=x.device) if x.shape[0] > 1 else None
        check(lib.pxm_csr_matvec(_p(self.indptr), _p(self.indices), _p(self.vals), int(self.is_complex), self.shape[0],
                                 self.shape[1], _p(x), _p(out), x.shape[0], _dt(x), _p(scratch), _stream()))
        return _np(out)


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("cplx_mat,cplx_vec", H.CSR_KINDS)
def test_csr_rows_past_the_cap(cplx_mat, cplx_vec, adjoint):
    """65797 rows by 70001 columns (one wave per row: 65536 rows a pass), or its conjugate transpose as a CSR of its own (70001
    rows); C = 1 on the direct path, C = 2 and 3 on the chain-minor path (3: the 2 + 1 register-block tail); every row within
    the summation bound of the model, empty rows exactly zero, every chain of a batch equal to its own single-chain product"""
    indptr, indices, vals, shape = H.csr_rows_case(cplx_mat, adjoint)
    assert shape == ((70001, 65797) if adjoint else (65797, 70001))
    M = _Csr(indptr, indices, vals, shape)
    x = H.csr_rows_vectors(cplx_vec, adjoint)
    xd = _dev(x)
    y, _, bound = H.csr_rows_model(cplx_mat, cplx_vec, adjoint)
    empty = np.flatnonzero(np.diff(indptr) == 0)
    if not adjoint:
        assert set(H.CSR_EMPTY) == set(empty.tolist()) == {5, 65543}
    tag = f"{'complex' if cplx_mat else 'real'} matrix{' (adjoint)' if adjoint else ''}, {'complex' if cplx_vec else 'real'} vector"
    single = np.stack([M.matvec(xd[c:c + 1].contiguous())[0] for c in range(3)])
    for c in range(3):
        assert_within(single[c], y[c], bound[c], f"CSR rows, {tag}, chain {c} alone")
    assert_same(single[:, empty], 0.0, f"CSR rows, {tag}: empty rows")
    for C in (2, 3):
        got = M.matvec(xd[:C].contiguous())
        assert_within(got, y[:C], bound[:C], f"CSR rows, {tag}, C = {C}")
        assert_same(got[:, empty], 0.0, f"CSR rows, {tag}, C = {C}: empty rows")
        assert_same(got, single[:C], f"CSR rows, {tag}, C = {C} against the single-chain products")


def test_csr_columns_past_the_transpose_cap():
    """64 rows by 1048576 + 3 columns, two real chains (16.8 MB: chain-minor path): the columns past the first pass of
    k_chains_to_minor (4096 workgroups of 256 threads) reach the gather -- the scratch starts as NaN"""
    indptr, indices, vals, shape, x = H.csr_cols_case()
    assert shape == (64, 1048579)
    M = _Csr(indptr, indices, vals, shape)
    xd = _dev(x)
    y, S = H.csr_model(indptr, indices, vals, x)
    got = M.matvec(xd)
    assert_within(got, y, H.csr_bound(indptr, S), "CSR columns, C = 2")
    single = np.stack([M.matvec(xd[c:c + 1].contiguous())[0] for c in range(2)])
    assert_same(got, single, "CSR columns, C = 2 against the single-chain products")
