"""Host-side set-up helpers: no GPU needed (csrc/tables.cpp, host_api.cpp)."""
import ctypes as C

import numpy as np

from .._lib import check, lib


def j_max(L, B):
    return int(check(lib.pxm_j_max(int(L), float(B))))


def wav_bandlimits(L, B, J_min):
    buf = (C.c_int * 64)()
    n = check(lib.pxm_wav_bandlimits(int(L), float(B), int(J_min), buf, 64))
    return [int(buf[i]) for i in range(n)]


def tiling_axisym(L, B, J_min):
    J = j_max(L, B)
    k0 = np.zeros(L)
    k = np.zeros((J + 1, L))
    check(lib.pxm_tiling_axisym(int(L), float(B), int(J_min), k0.ctypes.data, k.ctypes.data))
    return k0, k


def mw_ring_weights(L):
    q = np.zeros(L)
    check(lib.pxm_mw_ring_weights(int(L), q.ctypes.data))
    return q


def rec_geometry(L, spin, chains):
    """(R, NC, waves, lds_bytes) of the table-free ring stage (csrc/sht_rec.hip) for a plan of this size, honouring
    PXM_REC_R, or None where the size has no geometry and the plan keeps its ring tables"""
    out = (C.c_int * 4)()
    if lib.pxm_host_rec_geometry(int(L), int(spin), int(chains), out) < 0:
        return None
    return tuple(int(v) for v in out)


DFT_UNITS = ("radix2", "pair", "quad")  # out[0] of pxm_host_dft_geometry


def dft_geometry(L):
    """(unit, M, per_workgroup, threads, lds_bytes, exact) of the phi-DFT stage (csrc/dft.hip: dft_geometry) of a plan at
    bandlimit L, honouring PXM_DFT_NO_W and PXM_DFT_PFA: ``unit`` one of DFT_UNITS, ``per_workgroup`` chains (radix2, quad)
    or rings (pair) per workgroup, ``exact`` whether the 511-point rings take the exact-length body.  Raises PxmError
    where the stage has no unit for the size (L >= 1025), in the words every plan constructor refuses it with."""
    out = (C.c_int * 6)()
    check(lib.pxm_host_dft_geometry(int(L), out))
    return (DFT_UNITS[out[0]], int(out[1]), int(out[2]), int(out[3]), int(out[4]), bool(out[5]))


def hpx_geometry(L, nside):
    """``dict(rings, npix, lds_bytes, nside_max, threads, rings_padded)`` of ``ops.HpxPlan(L, nside)`` (csrc/healpix.hip):
    ``lds_bytes`` the LDS of a phi-stage workgroup (the longest ring, 4 nside points), ``nside_max`` the largest nside whose
    longest ring fits a CU's LDS.  Raises PxmError, in the words the plan refuses with, for L >= 1025, nside < 1 and
    nside > nside_max."""
    out = (C.c_int64 * 6)()
    check(lib.pxm_host_hpx_geometry(int(L), int(nside), out))
    return dict(zip(("rings", "npix", "lds_bytes", "nside_max", "threads", "rings_padded"), (int(v) for v in out)))


def hpx_rings(nside):
    """(nphi, theta, phi0, start) per ring as the library's host code computes them (utils.healpix_rings is the numpy statement)"""
    R = 4 * int(nside) - 1
    nphi, theta, phi0, start = np.zeros(max(R, 1), np.int32), np.zeros(max(R, 1)), np.zeros(max(R, 1)), np.zeros(max(R, 1), np.int64)
    check(lib.pxm_host_hpx_rings(int(nside), nphi.ctypes.data, theta.ctypes.data, phi0.ctypes.data, start.ctypes.data))
    return nphi, theta, phi0, start


def hpx_lambda(L, spin, m, theta):
    """lam[t, l] = (-1)^s sqrt((2l+1)/4pi) d^l_{m,-s}(theta[t]), l < L: the long-double recursion the plan fills its table with"""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    out = np.zeros((theta.size, int(L)))
    check(lib.pxm_host_hpx_lambda(int(L), int(spin), int(m), theta.ctypes.data, theta.size, out.ctypes.data))
    return out


def harm_weights(L, B, J_min, N=1, spin=0, harmonic=False):
    """(wa, ws, rows): the split and merge weights of the harmonic stage as ``ops.DirWavPlan(L, B, J_min, N)`` (``harmonic``
    False; spin 0, the pairs |n| >= bl_j skipped) or ``ops.HarmWavPlan(L, B, J_min, N, spin)`` (True) uploads them, complex
    [rows, L] each, item by item in plan order; ``rows`` int [rows, 3] = (block, n, bl) of each (csrc/harm_stage.hip)"""
    args = (int(L), float(B), int(J_min), int(N), int(spin), int(bool(harmonic)))
    n = int(check(lib.pxm_host_harm_weights(*args, None, None, None, 0)))
    wa, ws, rows = np.zeros((n, int(L)), dtype=complex), np.zeros((n, int(L)), dtype=complex), np.zeros((n, 3), dtype=np.int32)
    check(lib.pxm_host_harm_weights(*args, wa.ctypes.data, ws.ctypes.data, rows.ctypes.data, n))
    return wa, ws, rows


def dir_component(L, N):
    """the directionality component s_lm [L*L] as the library builds it for the weight rows (utils.dir_component is the numpy
    statement; csrc/harm_stage.hip: dir_component)"""
    s = np.zeros(int(L) * int(L), dtype=complex)
    check(lib.pxm_host_dir_component(int(L), int(N), s.ctypes.data))
    return s


def dwav_phases(N):
    """ph[q, k] = e^{i n_k gamma_q}, [2N-1, N], n_k = -(N-1) + 2k, gamma_q = 2 pi q / (2N-1): the table the gamma stage of
    ``ops.DirWavPlan`` reads (csrc/harm_stage.hip: dw_phases)"""
    ph = np.zeros((2 * int(N) - 1, int(N)), dtype=complex)
    check(lib.pxm_host_dwav_phases(int(N), ph.ctypes.data))
    return ph


DFT_STEP_FIELDS = ("X", "T", "noise", "iter_dev", "rdata", "rinvcov", "gidx", "gw")  # bits of pxm_host_dft_step_is_stock


def dft_step_is_stock(fields, mode, chain0):
    """whether a fused rings -> X' -> rings launch that carries the optional operands named in ``fields`` (names of
    DFT_STEP_FIELDS) with update mode ``mode`` (PXM_MODE_*) and first chain ``chain0`` is the stock MYULA update, which the
    pair unit of the phi-DFT stage runs on its STOCK kernel instantiations (csrc/sht_core.h: dft_step_is_stock)"""
    bits = 0
    for f in fields:
        bits |= 1 << DFT_STEP_FIELDS.index(f)
    return bool(check(lib.pxm_host_dft_step_is_stock(bits, int(mode), int(chain0))))


def noise_bits():
    """32: the precision of the Box-Muller step of the device noise stream WITHOUT the flag (the samplers of mcmc.py pass
    the flag by default: ``noise_bits=64``); every noise-drawing call takes
    ``noise64=True`` for the double-precision evaluation (PXM_NOISE_F64, include/pxmcmc_amd.h)"""
    return int(lib.pxm_noise_bits())


# ---- reports of a GEMM-only plan (include/pxmcmc_amd.h: pxm_gemm_plan_report) ------------------------------------------------------
GEMM_TASK_FIELDS = ("m_unit", "row0", "n_rt", "k_beg", "k_end", "pole_n", "nslab", "side", "par", "row_lo", "row_hi", "row_lo1",
                    "row_hi1", "sign1", "side_b", "m")
_GEMM_HEAD = ("ncol", "n_sides", "n_tasks", "flags", "nslab", "pk", "ws_doubles", "off_scratch", "scratch_doubles", "off_counter",
              "max_chains", "paired")
_GEMM_SIDE = ("off_x", "off_x2", "off_y", "off_ks", "off_rs", "off_hd", "xL", "xRp", "xn", "yL", "yRp", "yn", "n_x", "n_y", "n_tab",
              "n_pole")
_GEMM_TABLE = ("n_m", "Rp", "paired", "n_tab", "n_pole", "L", "spin", "kind")


def _gemm_words(call, what, side):
    """the int64 words of report ``what``: ``call(what, side, out, cap)`` is asked for the size, then for the words"""
    n = check(call(what, side, None, 0))
    out = (C.c_int64 * max(int(n), 1))()
    check(call(what, side, out, n))
    return np.array(out[:n], dtype=np.int64)


def gemm_report(call, n_sides):
    """the three reports of a GEMM-only plan as ``{layout, sides, tasks, tables}``: ``layout`` the header words by name,
    ``sides`` one dict per side, ``tasks`` the [n, 16] list in launch order (columns GEMM_TASK_FIELDS), ``tables`` per side
    the bookkeeping of its tiled table with ``orders`` [n_m, 5] = (m, m_off, k_beg, odd_off, odd_k_beg)"""
    w = _gemm_words(call, 0, 0)
    rep = {"layout": dict(zip(_GEMM_HEAD, (int(v) for v in w[:16]))),
           "sides": [dict(zip(_GEMM_SIDE, (int(v) for v in w[16 + 16 * i:32 + 16 * i]))) for i in range(n_sides)],
           "tasks": _gemm_words(call, 1, 0).reshape(-1, len(GEMM_TASK_FIELDS)), "tables": []}
    for i in range(n_sides):
        t = _gemm_words(call, 2, i)
        tab = dict(zip(_GEMM_TABLE, (int(v) for v in t[:8])))
        tab["orders"] = t[8:].reshape(-1, 5)
        rep["tables"].append(tab)
    return rep


def gemm_plan_geometry(sides, spin=0, max_chains=8, pk=0):
    """``gemm_report`` of the GEMM-only plan ``ops.GemmPlan(sides, spin, max_chains, pk)`` built in dry-run mode: the real task
    builders, launch order (PXM_GEMM_ORDER) and address-range check, no GPU.  Raises PxmError where the creation refuses."""
    from ._args import _gemm_sides

    desc = _gemm_sides(sides, max_chains, pk)
    return gemm_report(lambda what, side, out, cap: lib.pxm_host_gemm_plan_report(int(spin), int(max_chains), int(pk), desc, len(sides),
                                                                                  what, side, out, cap), len(sides))
