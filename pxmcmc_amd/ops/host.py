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


def noise_bits():
    """32: the precision of the Box-Muller step of the device noise stream WITHOUT the flag (the samplers of mcmc.py pass
    the flag by default: ``noise_bits=64``); every noise-drawing call takes
    ``noise64=True`` for the double-precision evaluation (PXM_NOISE_F64, include/pxmcmc_amd.h)"""
    return int(lib.pxm_noise_bits())
