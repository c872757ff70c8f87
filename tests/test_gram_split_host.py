"""CPU-side checks of the parity-split Gram table (csrc/sht_tables.h: TAB_GRAM_SPLIT): the structure of the oracle's Gram
matrix that the split rests on, the address ranges of the split and dense Gram lists (dry-run plans), the stored size."""
import functools

import numpy as np
import pytest


def _lib():
    from pxmcmc_amd import _lib

    return _lib.lib


@functools.lru_cache(maxsize=None)
def _odd_parts(L):
    """max |G[(l, m), (l', m)]| over l + l' odd, per order m >= 0, relative to the largest entry of G = Y^H Y (spin 0)"""
    from oracle import ssht

    Y = ssht.spin_harmonic_matrix(L, 0)
    G = Y.conj().T @ Y
    scale = np.abs(G).max()
    odd = np.zeros(L)
    for m in range(L):
        els = np.arange(m, L)
        idx = els * els + els + m
        Gm = G[np.ix_(idx, idx)]
        mask = (els[:, None] + els[None, :]) % 2 == 1
        odd[m] = np.abs(Gm[mask]).max() if mask.any() else 0.0
    return odd / scale


@pytest.mark.parametrize("L", [16, 33])
def test_odd_parity_part_of_the_gram_matrix_vanishes_for_m_ge_1_only(L):
    """G^m[l][l'] = sum_t B^m[t][l] B^m[t][l'] over the L MW rings: for m >= 1 the entries with l + l' odd are zero to
    round-off (measured 1e-15 at L = 16, 2.5e-15 at L = 33; the bound leaves room for other BLAS builds), for m = 0 the
    pole ring leaves a real odd-parity part (measured 0.28 / 0.26 of the largest entry): m = 0 must stay dense."""
    odd = _odd_parts(L)
    print(f"L={L}: odd part m>=1 {odd[1:].max():.3e}, m=0 {odd[0]:.3f}")
    assert odd[1:].max() <= 1e-13
    assert odd[0] >= 0.1


@pytest.mark.parametrize("split", ["default", "0"])
@pytest.mark.parametrize("C", [1, 16])
@pytest.mark.parametrize("L", [32, 40, 64, 96, 256])
def test_gram_list_address_ranges(L, C, split, monkeypatch):
    """every address the Gram launch can form with the per-task row pitch lies inside one allocation: the split list
    (Rp % 32 == 0), the dense fallback (L = 40: Rp = 48) and the forced dense list; the spin-2 plan is always dense"""
    lib = _lib()
    if split == "0":
        monkeypatch.setenv("PXM_GRAM_SPLIT", "0")
    else:
        monkeypatch.delenv("PXM_GRAM_SPLIT", raising=False)
    n = lib.pxm_host_check_address_ranges(L, 2.0, 2, 0, C, 2)
    assert n >= 0, lib.pxm_last_error().decode()
    n2 = lib.pxm_host_check_address_ranges(L, 2.0, 2, 2, C, 2 | 8)
    assert n2 >= 0, lib.pxm_last_error().decode()


def test_split_list_checks_more_ranges_than_the_dense_one(monkeypatch):
    """the split list is the longer one (two short tasks per order instead of one or two), so the switch is seen to act"""
    lib = _lib()
    monkeypatch.delenv("PXM_GRAM_SPLIT", raising=False)
    n_split = lib.pxm_host_check_address_ranges(256, 2.0, 2, 0, 16, 2)
    n40 = lib.pxm_host_check_address_ranges(40, 2.0, 2, 0, 16, 2)
    monkeypatch.setenv("PXM_GRAM_SPLIT", "0")
    assert n_split > lib.pxm_host_check_address_ranges(256, 2.0, 2, 0, 16, 2) > 0
    assert n40 == lib.pxm_host_check_address_ranges(40, 2.0, 2, 0, 16, 2)


@pytest.mark.parametrize("L", [64, 256])
def test_range_check_still_refuses_a_short_workspace_with_the_split_list(L, monkeypatch):
    lib = _lib()
    monkeypatch.delenv("PXM_GRAM_SPLIT", raising=False)
    shape = (L, 2.0, 2, 0, 16, 2)
    assert lib.pxm_host_check_address_ranges(*shape) > 0
    monkeypatch.setenv("PXM_RANGE_SELFTEST", "workspace:8")
    assert lib.pxm_host_check_address_ranges(*shape) < 0
    assert "GEMM task address range" in lib.pxm_last_error().decode()
    monkeypatch.setenv("PXM_RANGE_SELFTEST", "ring table:2048")  # every table one k-chunk short, the split one included
    assert lib.pxm_host_check_address_ranges(*shape) < 0
    assert "ring-table stream" in lib.pxm_last_error().decode()
    monkeypatch.delenv("PXM_RANGE_SELFTEST")
    assert lib.pxm_host_check_address_ranges(*shape) > 0


def _split_entries(Rp):
    """doubles of the split table as derived: an order is two halves from round_down(ceil((m - p) / 2), 16) where the
    modelled work (row tiles x (contraction steps + 32)) of the halves is below the dense block's, else the dense block"""
    Rh, total = Rp // 2, Rp * Rp

    def work(n, kb):
        return (n - kb) // 16 * (n - kb + 32)

    for m in range(1, Rp):
        kd, kh = m // 16 * 16, [((m - p + 1) // 2) // 16 * 16 for p in (0, 1)]
        if sum(work(Rh, k) for k in kh) < work(Rp, kd):
            total += sum((Rh - k) ** 2 for k in kh)
        else:
            total += (Rp - kd) ** 2
    return total


def test_split_table_size(monkeypatch):
    """L = 256: the stored split table is the derived 0.55 of the dense one (bound 0.6); L = 40 (Rp = 48) and spin 2
    fall back to the dense table"""
    lib = _lib()

    def both(L, spin):
        monkeypatch.delenv("PXM_GRAM_SPLIT", raising=False)
        a = lib.pxm_host_gram_table_bytes(L, 2.0, 2, spin, 16)
        monkeypatch.setenv("PXM_GRAM_SPLIT", "0")
        b = lib.pxm_host_gram_table_bytes(L, 2.0, 2, spin, 16)
        assert a > 0 and b > 0, lib.pxm_last_error().decode()
        return a, b

    split, dense = both(256, 0)
    assert dense == 8 * sum((256 - m // 16 * 16) ** 2 for m in range(256))
    assert split == 8 * _split_entries(256)
    print(f"L=256: split {split / 1e6:.2f} MB, dense {dense / 1e6:.2f} MB, ratio {split / dense:.4f}")
    assert split <= 0.6 * dense
    split, dense = both(40, 0)
    assert split == dense
    split, dense = both(64, 2)
    assert split == dense
