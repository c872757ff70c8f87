"""Host side of the table-free ring stage (csrc/rec_core.h, csrc/tables.cpp): the recursion the kernels run, emulated in
double precision operation for operation (pxm_host_rec_table), against the x87 long-double ring tables the GEMM path
streams (pxm_host_sht_tables) -- no GPU needed."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

from pxmcmc_amd._lib import lib

LD, CLD = np.longdouble, np.clongdouble
EPS = 2.0 ** -52

# ---- what the GPU tests of the forced geometries (tests/test_gpu_rec.py) share with the CPU tests below ----------------------
# (spin, chains) of a plan -> NC = chains (spin != 0: all orders stored) or 2 chains (spin 0: +-m pairs) complex columns
REC_CONFIGS = [(2, 1), (0, 1), (2, 2), (0, 2), (2, 4)]
REC_NC = {(2, 1): 1, (0, 1): 2, (2, 2): 2, (0, 2): 4, (2, 4): 4}
# (L, forced R) -> wavefronts per workgroup.  Ring blocks of 64 rings; block b is northern when its centre ring is; a wave
# takes up to R consecutive blocks of one hemisphere.
#   L = 130: blocks N S S(2 rings)         R = 1: 3 waves;  R = 2, 4: {0} {1, 2} -- a wave of two blocks, one nearly empty
#   L = 200: blocks N N S S(8 rings)       R = 1: 4;        R = 2, 4: {0, 1} {2, 3} -- full R = 2 waves
#   L = 385: blocks N N N S S S S(1 ring)  R = 1: 7;        R = 2: {0, 1} {2} {3, 4} {5, 6};  R = 4: {0, 1, 2} {3, 4, 5, 6}
REC_WAVES = {(130, 1): 3, (130, 2): 2, (130, 4): 2, (200, 1): 4, (200, 2): 2, (200, 4): 2, (385, 1): 7, (385, 2): 4, (385, 4): 2}
# (L, R, NC) whose ring -> el kernel needs more than 48 KiB of LDS: the per-instantiation dynamic-LDS opt-in
REC_OVER_48K = {(200, 1, 4), (385, 1, 2), (385, 2, 2), (385, 2, 4), (385, 4, 4)}
REC_NO_GEOMETRY = {(385, 1, 4)}  # 7 waves x 401 x 64 B = 175 KiB > 150 KiB


def rec_geometry(L, spin, chains):
    """(R, NC, waves, LDS bytes) of pxm_host_rec_geometry, or None where the size has no geometry"""
    out = (C.c_int * 4)()
    if lib.pxm_host_rec_geometry(L, spin, chains, out) < 0:
        assert b"pxm_host_rec_geometry" in lib.pxm_last_error()
        return None
    return tuple(out)


def _tables(L, spin, m):
    B, R = np.zeros((L, L)), np.zeros((L, L))
    assert lib.pxm_host_sht_tables(L, spin, m, B.ctypes.data_as(C.c_void_p), None) == 0
    assert lib.pxm_host_rec_table(L, spin, m, R.ctypes.data_as(C.c_void_p)) == 0
    return B, R


def one_order_ms(L, spin):
    """the orders of the one-order-per-chain inputs: lowest, |s| - 1 (el0 = |s| > |m|), middle, extreme"""
    ms = [0, 1, -1, abs(spin) - 1, L // 2, -(L // 2) + 1, L - 2, -(L - 1), L - 1]
    return list(dict.fromkeys(ms))


def rec_inputs(L, spin, chains, seed):
    """Inputs of the per-element tests: `chains` dense Gaussian chains, then one chain per order of one_order_ms --
    flm [K][L^2] with the degrees below |s| zero, f [K][L (2L - 1)] (one order: f[t][p] = g[t] e^{i m phi_p})"""
    rng = np.random.default_rng(seed)
    n, ms = 2 * L - 1, one_order_ms(L, spin)
    K = chains + len(ms)
    el = np.arange(L)
    flm = rng.normal(size=(K, L * L)) + 1j * rng.normal(size=(K, L * L))
    flm[:, : spin * spin] = 0
    f = rng.normal(size=(K, L, n)) + 1j * rng.normal(size=(K, L, n))
    for k, m in enumerate(ms, start=chains):
        keep = np.zeros(L * L, dtype=bool)
        keep[(el * el + el + m)[max(abs(m), abs(spin)):]] = True
        flm[k, ~keep] = 0
        f[k] = f[k, :, :1] * np.exp(2j * np.pi * ((m * np.arange(n)) % n) / n)
    return flm, f.reshape(K, L * n)


@functools.lru_cache(maxsize=4)
def _ld_phases(L):
    """cos, sin of 2 pi ((m p) mod n) / n in long double for m, p = 0 .. L - 1 (n = 2L - 1); the other three quadrants of
    the DFT matrix follow by symmetry"""
    n = 2 * L - 1
    k = np.outer(np.arange(L), np.arange(L)) % n
    ang = k.astype(LD) * (2 * np.arccos(LD(-1)) / n)
    return np.cos(ang), np.sin(ang)


def _cmul(a, M):
    """complex long double a @ real long double M"""
    return np.ascontiguousarray(a.real) @ M + 1j * (np.ascontiguousarray(a.imag) @ M)


def _rings_to_px_ld(G, L):
    """f[t][p] = sum_m G[m + L - 1][t] e^{2 pi i ((m p) mod n) / n} in long double, orders +-m and pixels p, n - p folded"""
    n = 2 * L - 1
    Cm, Sm = _ld_phases(L)
    A, D = G[L - 1:] + G[L - 1::-1], G[L - 1:] - G[L - 1::-1]  # [m = 0 .. L - 1][t]
    A[0] = G[L - 1]
    live = np.flatnonzero(np.abs(A).any(axis=1) | np.abs(D).any(axis=1))
    a, b = _cmul(A[live].T, Cm[live]), 1j * _cmul(D[live].T, Sm[live])  # [t][p = 0 .. L - 1]
    f = np.empty((L, n), dtype=CLD)
    f[:, :L] = a + b
    f[:, L:] = (a - b)[:, :0:-1]  # p' = n - p, p = L - 1 .. 1
    return f


def _px_to_rings_ld(f, L):
    """G[m + L - 1][t] = sum_p f[t][p] e^{-2 pi i ((m p) mod n) / n} in long double: the conjugate transpose of the above"""
    n = 2 * L - 1
    Cm, Sm = _ld_phases(L)
    f = f.astype(CLD)
    fp, fm = f[:, :L].copy(), np.zeros((L, L), dtype=CLD)
    fp[:, 1:] += f[:, :L - 1:-1]  # f[t][p] + f[t][n - p], p = 1 .. L - 1
    fm[:, 1:] = f[:, 1:L] - f[:, :L - 1:-1]
    u, v = _cmul(fp, Cm.T), _cmul(fm, Sm.T)  # [t][m = 0 .. L - 1]
    G = np.empty((n, L), dtype=CLD)
    G[L - 1:] = (u - 1j * v).T
    G[L - 1::-1] = (u + 1j * v).T  # (m = 0: sin = 0 exactly, both forms agree)
    return G


RecModel = collections.namedtuple("RecModel", "ref scale err")


def rec_stage_model(L, spin, flm=None, f=None):
    """What inverse / inverse_adjoint (pyssht.inverse / inverse_adjoint, pxmcmc/measurements.py:225,237) of a plan on the
    recursion kernels are held to, per element: {"inverse": RecModel, "inverse_adjoint": RecModel} for flm [K][L^2] and
    f [K][L (2L - 1)], each RecModel(ref, scale, err) of the output's shape.

    ref    inverse: G[m][t] = sum_el B^m[t][el] flm[el, m] with the rows of pxm_host_sht_tables, accumulated in long double,
           f[t][p] = sum_m G[m][t] e^{2 pi i ((m p) mod n) / n} in long double; inverse_adjoint: the conjugate transpose of
           the same two steps
    scale  inverse: S[t] = sum_m sum_el |B^m[t][el]| |flm[el, m]| of the pixel's ring, at least 1e-120 max_t S (the kernels
           drop values below 2^-448 of the double range by design); inverse_adjoint: sum_t |B^m[t][el]| ||f[t, :]||_2
    err    |model - ref| of the CPU model: the same contractions in double with the rows of pxm_host_rec_table (the
           operation-for-operation emulation of the kernels' recursion) and numpy's double FFT"""
    n, ms = 2 * L - 1, np.arange(-(L - 1), L)
    el = np.arange(L)
    if flm is not None:
        flm = np.asarray(flm, dtype=complex).reshape(-1, L * L)
        K = len(flm)
        G_ref, G_mod, S = np.zeros((K, n, L), dtype=CLD), np.zeros((K, n, L), dtype=complex), np.zeros((K, L))
    if f is not None:
        f = np.asarray(f, dtype=complex).reshape(-1, L, n)
        K2 = len(f)
        Gf_ref = np.stack([_px_to_rings_ld(x, L) for x in f])  # [K2][m][t]
        Gf_mod = np.fft.fft(f, axis=2)[:, :, ms % n].transpose(0, 2, 1)
        rownorm = np.linalg.norm(f, axis=2)  # [K2][t]
        H_ref, H_mod, Hs = np.zeros((K2, L * L), dtype=CLD), np.zeros((K2, L * L), dtype=complex), np.zeros((K2, L * L))
    for i, m in enumerate(ms):
        el0 = max(abs(m), abs(spin))
        B, R = (x[:, el0:] for x in _tables(L, spin, int(m)))  # [t][el >= el0]
        Bl, idx = B.astype(LD), (el * el + el + m)[el0:]
        if flm is not None:
            h = flm[:, idx]
            live = np.flatnonzero(np.abs(h).any(axis=1))
            G_ref[live, i] = _cmul(h[live].astype(CLD), Bl.T)
            G_mod[:, i] = h @ R.T
            S += np.abs(h) @ np.abs(B).T
        if f is not None:
            H_ref[:, idx] = _cmul(Gf_ref[:, i], Bl)
            H_mod[:, idx] = Gf_mod[:, i] @ R
            Hs[:, idx] = rownorm @ np.abs(B)
    out = {}
    if flm is not None:
        ref = np.stack([_rings_to_px_ld(G, L) for G in G_ref]).reshape(K, L * n)
        buf = np.zeros((K, L, n), dtype=complex)
        buf[:, :, ms % n] = G_mod.transpose(0, 2, 1)
        model = (np.fft.ifft(buf, axis=2) * n).reshape(K, L * n)
        S = np.maximum(S, 1e-120 * S.max(axis=1, keepdims=True))
        out["inverse"] = RecModel(ref, np.repeat(S, n, axis=1), np.abs(model - ref).astype(float))
    if f is not None:
        out["inverse_adjoint"] = RecModel(H_ref, Hs, np.abs(H_mod - H_ref).astype(float))
    return out


def rec_adjoint_scale(L, spin, f):
    """the scale of rec_stage_model for inverse_adjoint alone (no reference): sum_t |B^m[t][el]| ||f[t, :]||_2, [K][L^2]"""
    f = np.asarray(f, dtype=complex).reshape(-1, L, 2 * L - 1)
    rownorm, el = np.linalg.norm(f, axis=2), np.arange(L)
    Hs, B = np.zeros((len(f), L * L)), np.zeros((L, L))
    for m in range(-(L - 1), L):
        el0 = max(abs(m), abs(spin))
        assert lib.pxm_host_sht_tables(L, spin, m, B.ctypes.data_as(C.c_void_p), None) == 0
        Hs[:, (el * el + el + m)[el0:]] = rownorm @ np.abs(B[:, el0:])
    return Hs


def model_cap(L, coherent=False):
    """What the CPU model's own err / scale may reach: el^1.5 eps, the growth law documented below for the rows the model
    contracts with.  `coherent` (inverse_adjoint of a one-order image): every pixel of a ring adds up in the one order,
    |G[m][t]| = n |g[t]| = sqrt(n) ||f[t, :]||_2, so the same row error weighs sqrt(n) = sqrt(2L - 1) more against the
    scale, which is built on the ring's 2-norm."""
    return L ** 1.5 * EPS * (np.sqrt(2 * L - 1) if coherent else 1.0)


def model_tol(model, chains, cap):
    """tol = 4 max(err / scale) of the CPU model over the elements of `chains` (the margin is for what the device
    legitimately does otherwise: the order of the sums over el, lanes, blocks and waves, g folded into the operand, the DFT
    unit in place of numpy's FFT).  The model itself is held to `cap` (model_cap): a model that lost precision must not
    widen the device's bound unnoticed."""
    err, scale = model.err[chains], model.scale[chains]
    assert not err[scale == 0].any()  # (degrees below |s|: exactly zero on both sides)
    ratio = (err[scale > 0] / scale[scale > 0]).max()
    assert 0 < ratio <= cap, (ratio, cap)
    return 4 * ratio


def within(got, model, chains, tol):
    """max |got - ref| / (tol scale) over the elements of `chains`: <= 1 when the bound holds for every element"""
    ref, scale = model.ref[chains], model.scale[chains]
    d = np.abs(np.asarray(got).astype(CLD) - ref).astype(float)
    if d[scale == 0].any():
        return np.inf
    return (d[scale > 0] / (tol * scale[scale > 0])).max()


@pytest.mark.parametrize("L,tol", [(3, 1e-15), (10, 4e-15), (64, 1e-13), (257, 2e-12), (512, 1e-11)])
def test_recursion_rows_equal_the_long_double_tables(L, tol):
    """B^m[t][el] = (-1)^s sqrt((2el+1)/4pi) d^el_{m,-s}(theta_t) (what pyssht.inverse / inverse_adjoint contract with,
    pxmcmc/measurements.py:225,237): the scaled double-precision recursion with the pole-distance form of the step stays
    within el^1.5 eps of the long-double rows, for spins 0 and 2, low / middle / extreme orders, every ring incl. the polar
    ones whose seeds lie 1400 decades below the double range"""
    for spin in (0, 2):
        worst = 0.0
        for m in sorted({0, 1, -1, 2, -2, 3, L // 4, -(L // 4), L // 2, -(L // 2) + 1, L - 2, -(L - 1), L - 1}):
            if abs(m) >= L:
                continue
            B, R = _tables(L, spin, m)
            assert np.isfinite(R).all()
            worst = max(worst, np.abs(B - R).max())
            el0 = max(abs(m), spin)
            assert not R[:, :el0].any()  # rows below max(|m|, |s|) are exactly zero
        assert worst <= tol, (L, spin, worst)


def test_recursion_symmetries_and_seed_scale():
    """d^el_{-m,0} = (-1)^m d^el_{m,0} (the +-m pairing of the spin-0 kernels) and rows that never reach the double range stay 0"""
    L = 96
    for m in (1, 2, 17, 95):
        Bp, Rp = _tables(L, 0, m)
        Bm, Rm = _tables(L, 0, -m)
        np.testing.assert_allclose(Rm, (-1) ** m * Rp, rtol=0, atol=1e-15)
    # L = 512, m = 511: only el = 511, values ~ sin^511(theta): 1e-136 on mid-latitude rings, below 1e-300 near the poles
    B, R = _tables(512, 2, 511)
    assert np.abs(B - R).max() < 2 ** -447 and R[0, 511] == 0.0 and abs(R[255, 511]) > 0.1  # (values below 2^-448 are dropped)


def test_recursion_kernels_isa_has_no_unguarded_dpp_read_after_valu_write():
    """gfx950: a VGPR written by a VALU instruction must not be read as a DPP source within two wait states.  The compiler
    guards its own DPP instructions but cannot see inside the inline assembly of the recursion kernels (`v_fmac_f64_dpp` /
    `v_mov_b64_dpp ... row_newbcast`); `dpp_fence` is what keeps the register rotation of the look-ahead away from them (a
    version without it returned 5e17 in one instantiation).  Static check of the compiled ISA of every instantiation."""
    import importlib.util
    import os
    import shutil

    from conftest import ROOT

    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("check_dpp_hazard", os.path.join(ROOT, "scripts", "dev", "check_dpp_hazard.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import subprocess
    import tempfile

    d = tempfile.mkdtemp(prefix="pxm_dpp_")
    src = os.path.join(ROOT, "pxmcmc_amd", "csrc", "sht_rec.hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", os.path.join(d, "o.o"),
                    "--save-temps=obj"], check=True, cwd=os.path.dirname(src), capture_output=True)
    worst = mod.check(os.path.join(d, "sht_rec-hip-amdgcn-amd-amdhsa-gfx950.s"))
    shutil.rmtree(d, ignore_errors=True)
    assert worst >= 2, worst


# ---- geometry (rec_geometry of csrc/sht_rec.hip through pxm_host_rec_geometry) -------------------------------------------------
def test_natural_geometry_first_sizes_and_limits(monkeypatch):
    """the first size at which a plan takes each of the nine (R, NC) instantiations of k_rec_e2r / k_rec_r2e by itself,
    and the largest size each (spin, chains) has a geometry for (8 waves, 150 KiB of LDS): every smaller size down to
    L = 3 has one too"""
    monkeypatch.delenv("PXM_REC_R", raising=False)
    first = {(3, 2, 1): (1, 1), (3, 0, 1): (1, 2), (3, 0, 2): (1, 4), (512, 2, 1): (2, 1), (512, 2, 2): (2, 2), (385, 0, 2): (2, 4),
             (513, 0, 2): (4, 4), (683, 2, 1): (4, 1), (683, 2, 2): (4, 2)}
    for (L, spin, chains), want in first.items():
        assert rec_geometry(L, spin, chains)[:2] == want, (L, spin, chains)
        assert all(rec_geometry(l, spin, chains)[:2] != want for l in range(3, L)), (L, spin, chains)
    limits = {(0, 1): 1024, (0, 2): 584, (0, 4): 0, (2, 1): 1536, (2, 2): 1024, (2, 4): 584, (2, 3): 0}
    for (spin, chains), top in limits.items():
        have = [l for l in range(3, 1700) if rec_geometry(l, spin, chains)]
        assert have == list(range(3, top + 1)), (spin, chains, have[-1:] or None)
    g = rec_geometry(512, 2, 1)
    assert g == (2, 1, 4, 4 * (512 + 16) * 16)  # [waves][L + 16][2 NC] doubles


def test_forced_geometry_at_the_gpu_test_shapes(monkeypatch):
    """PXM_REC_R makes its value the only candidate, under the same limits: the shapes tests/test_gpu_rec.py runs have the
    wave layouts they were chosen for (REC_WAVES), cross 48 KiB of LDS exactly where listed, and a value without a
    geometry -- or one that is not 1, 2 or 4 -- leaves the size without one"""
    over, none = set(), set()
    for (L, R), waves in REC_WAVES.items():
        monkeypatch.setenv("PXM_REC_R", str(R))
        for spin, chains in REC_CONFIGS:
            nc = REC_NC[spin, chains]
            g = rec_geometry(L, spin, chains)
            if g is None:
                none.add((L, R, nc))
                continue
            assert g == (R, nc, waves, waves * (L + 16) * 16 * nc), (L, R, spin, chains, g)
            if g[3] > 48 * 1024:
                over.add((L, R, nc))
    assert over == REC_OVER_48K and none == REC_NO_GEOMETRY
    monkeypatch.setenv("PXM_REC_R", "1")
    assert rec_geometry(512, 2, 1)[:3] == (1, 1, 8) and rec_geometry(513, 2, 1) is None  # 9 waves
    monkeypatch.setenv("PXM_REC_R", "4")
    assert rec_geometry(3, 2, 1)[:3] == (4, 1, 1) and rec_geometry(1536, 2, 1)[0] == 4 and rec_geometry(1537, 2, 1) is None
    for bad in ("3", "0", "8", "x"):
        monkeypatch.setenv("PXM_REC_R", bad)
        assert rec_geometry(130, 2, 1) is None
    monkeypatch.setenv("PXM_REC_R", "")  # (an empty value is no value)
    assert rec_geometry(130, 2, 1)[:2] == (1, 1)
    monkeypatch.delenv("PXM_REC_R")
    out = (C.c_int * 4)()
    assert lib.pxm_host_rec_geometry(0, 0, 1, out) < 0 and lib.pxm_host_rec_geometry(130, 0, 1, None) < 0
    from pxmcmc_amd import ops

    assert ops.rec_geometry(130, 0, 2) == (1, 4, 3, 3 * 146 * 64) and ops.rec_geometry(130, 0, 4) is None


# ---- the per-element model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spin", [0, 2])
def test_stage_model_reference_matches_the_oracle(spin):
    """sign and layout conventions of rec_stage_model: its long-double reference against the oracle's table + FFT
    transforms at L = 130 (1e-11 of the maximum), dense and one-order inputs; the double model within el^1.5 eps of the
    reference per element (model_tol, model_cap), with no element of a one-order chain left without a scale"""
    from oracle import ssht

    L = 130
    flm, f = rec_inputs(L, spin, 1, seed=7 + spin)
    pick = [0, 1, len(flm) - 1]  # dense, m = 0, m = L - 1
    M = rec_stage_model(L, spin, flm[pick], f[pick])
    for k, c in enumerate(pick):
        want = ssht.inverse(flm[c], L, spin).reshape(-1)
        assert np.abs(M["inverse"].ref[k] - want).max() <= 1e-11 * np.abs(want).max()
        want = ssht.inverse_adjoint(f[c].reshape(L, 2 * L - 1), L, spin)
        assert np.abs(M["inverse_adjoint"].ref[k] - want).max() <= 1e-11 * np.abs(want).max()
    for op in ("inverse", "inverse_adjoint"):
        assert M[op].ref.dtype == CLD and np.finfo(LD).eps < 2e-19
        tol = model_tol(M[op], slice(None), model_cap(L, coherent=op == "inverse_adjoint"))
        assert within(M[op].ref, M[op], slice(None), tol) == 0 and within(M[op].ref + 8 * M[op].err, M[op], slice(None), tol) > 1
    assert (M["inverse"].scale > 0).all()
    lm = np.arange(L * L)
    assert ((M["inverse_adjoint"].scale > 0) == (lm >= spin * spin)).all()
