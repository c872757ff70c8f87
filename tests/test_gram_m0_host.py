"""CPU-side checks of the order-0 halves of the split Gram list (csrc/sht_tables.h: TAB_GRAM_SPLIT0): the rank-one
cross-parity part of the oracle's order-0 Gram block that the pole term rests on, a numpy model of the two half
products plus the pole term, and the address ranges of the three Gram lists (dry-run plans)."""
import functools

import numpy as np
import pytest


def _lib():
    from pxmcmc_amd import _lib

    return _lib.lib


@functools.lru_cache(maxsize=None)
def _order0(L):
    """(G^0, b): the order-0 block of G = Y^H Y / (2L - 1) on the oracle -- Y^H Y sums the 2L - 1 samples of every ring, the
    tables' G^m = sum_t B^m[t][l] B^m[t][l'] counts a ring once -- and the order-0 column of Y on the pole ring theta = pi"""
    from oracle import ssht

    Y = ssht.spin_harmonic_matrix(L, 0)
    n = 2 * L - 1
    els = np.arange(L)
    idx = els * els + els
    G0 = (Y.conj().T @ Y)[np.ix_(idx, idx)] / n
    pole = Y[(L - 1) * n:, :][:, idx]
    assert np.abs(pole - pole[0]).max() == 0.0  # the samples of the pole ring are one value
    assert np.abs(G0.imag).max() == 0.0 and np.abs(pole[0].imag).max() == 0.0
    G0.setflags(write=False)
    return G0.real, pole[0].real


# measured on the oracle: 1.6e-15 at L = 16, 1.4e-15 at L = 33, relative to the largest entry of G^0; ten times that for
# other BLAS builds
CROSS_BOUND = {16: 1.6e-14, 33: 1.4e-14}


@pytest.mark.parametrize("L", [16, 33])
def test_cross_parity_block_of_order_0_is_the_pole_term(L):
    """G^0[2i][2j + 1] = 1/2 b_{2i} b_{2j+1}, b the order-0 column at theta = pi (sign (-1)^l): measured residual 1.6e-15
    (L = 16) and 1.4e-15 (L = 33) of the largest entry, bound ten times that; the cross block itself is 0.27 / 0.26 of the
    largest entry, so the bound is no formality.  The parity permutation [[ee, eo], [oe, oo]] moves entries and changes
    none: its diagonal blocks are the doubles G^0[2i + p][2j + p]."""
    G0, b = _order0(L)
    scale = np.abs(G0).max()
    assert np.all(np.sign(b) == (-1.0) ** np.arange(L))
    cross = G0[0::2, 1::2]
    res = np.abs(cross - 0.5 * np.outer(b[0::2], b[1::2])).max() / scale
    print(f"L={L}: cross-parity block {np.abs(cross).max() / scale:.3f}, residual against 1/2 b_e b_o^T {res:.3e}")
    assert np.abs(cross).max() / scale >= 0.1
    assert res <= CROSS_BOUND[L]
    assert np.abs(G0[1::2, 0::2] - 0.5 * np.outer(b[1::2], b[0::2])).max() / scale <= CROSS_BOUND[L]
    perm = np.concatenate([np.arange(0, L, 2), np.arange(1, L, 2)])
    Gp = G0[np.ix_(perm, perm)]
    ne = (L + 1) // 2
    assert np.array_equal(Gp[:ne, :ne], G0[0::2, 0::2]) and np.array_equal(Gp[ne:, ne:], G0[1::2, 1::2])
    assert np.array_equal(Gp[:ne, ne:], cross)


def _model_order0(G, b, x):
    """the order-0 path of the split list: two half products on the diagonal blocks of the permuted matrix and the pole
    term 1/2 b_own (b_other . x_other) -- the cross-parity blocks of G are never read"""
    y = np.zeros_like(x)
    for p in (0, 1):
        s = b[1 - p::2] @ x[1 - p::2]
        y[p::2] = G[p::2, p::2] @ x[p::2] + 0.5 * np.outer(b[p::2], s)
    return y


@pytest.mark.parametrize("Rp", [32, 96])
def test_numpy_model_of_the_order_0_halves_against_the_dense_product(Rp):
    """On a matrix with the structure the tables have (D without odd-parity entries plus 1/2 b b^T) and random complex
    operands the model reproduces the dense product to round-off: both sum Rp products per entry, in different orders.
    Bound: Rp * eps * max |G| * max |x| per entry, relative to max |y| (measured 4.1e-16 / 4.4e-16)."""
    rng = np.random.default_rng(Rp)
    b = rng.normal(size=Rp) * (-1.0) ** np.arange(Rp)
    D = rng.normal(size=(Rp, Rp))
    D = D + D.T
    D[(np.arange(Rp)[:, None] + np.arange(Rp)[None, :]) % 2 == 1] = 0.0
    G = D + 0.5 * np.outer(b, b)
    x = rng.normal(size=(Rp, 6)) + 1j * rng.normal(size=(Rp, 6))
    y = _model_order0(G, b, x)
    ref = G @ x
    err = np.abs(y - ref).max() / np.abs(ref).max()
    bound = Rp * np.finfo(float).eps * np.abs(G).max() * np.abs(x).max() / np.abs(ref).max()
    print(f"Rp={Rp}: model against dense {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    # an operand of one parity only: the pole term is the whole cross-parity answer
    for p in (0, 1):
        xp = x.copy()
        xp[1 - p::2] = 0.0
        yp = _model_order0(G, b, xp)
        assert np.abs(yp - G @ xp).max() / np.abs(ref).max() <= bound
        assert np.abs(yp[1 - p::2]).max() > 0.0


@pytest.mark.parametrize("split", ["default", "1", "0"])
@pytest.mark.parametrize("C", [1, 16])
@pytest.mark.parametrize("L", [32, 40, 64, 96, 256])
def test_gram_list_address_ranges_of_the_three_lists(L, C, split, monkeypatch):
    """every address of the Gram launch -- the order-0 halves on the permuted table, their pole columns and the other
    parity's operand rows included -- lies inside one allocation, for the new list, the list with order 0 dense and the
    dense list (L = 40: Rp = 48, dense whatever the switch says)"""
    lib = _lib()
    if split == "default":
        monkeypatch.delenv("PXM_GRAM_SPLIT", raising=False)
    else:
        monkeypatch.setenv("PXM_GRAM_SPLIT", split)
    n = lib.pxm_host_check_address_ranges(L, 2.0, 2, 0, C, 2)
    assert n > 0, lib.pxm_last_error().decode()


def test_order_0_halves_add_ranges_to_the_check(monkeypatch):
    """unset > PXM_GRAM_SPLIT=1 > PXM_GRAM_SPLIT=0 in ranges checked: one more task and the pole-term loads, so the
    switch is seen to act; the stored table is the same size with and without the order-0 halves; L = 40 ignores it"""
    lib = _lib()

    def count(L, val):
        if val is None:
            monkeypatch.delenv("PXM_GRAM_SPLIT", raising=False)
        else:
            monkeypatch.setenv("PXM_GRAM_SPLIT", val)
        return lib.pxm_host_check_address_ranges(L, 2.0, 2, 0, 16, 2), lib.pxm_host_gram_table_bytes(L, 2.0, 2, 0, 16)

    (n_new, b_new), (n_1, b_1), (n_0, b_0) = count(256, None), count(256, "1"), count(256, "0")
    assert n_new > n_1 > n_0 > 0
    assert b_new == b_1 < b_0
    assert count(40, None) == count(40, "1") == count(40, "0")


def test_range_check_refuses_a_short_pole_column(monkeypatch):
    lib = _lib()
    monkeypatch.delenv("PXM_GRAM_SPLIT", raising=False)
    shape = (64, 2.0, 2, 0, 16, 2)
    assert lib.pxm_host_check_address_ranges(*shape) > 0
    monkeypatch.setenv("PXM_RANGE_SELFTEST", "pole column:8")
    assert lib.pxm_host_check_address_ranges(*shape) < 0
    assert "pole column" in lib.pxm_last_error().decode()
    monkeypatch.setenv("PXM_GRAM_SPLIT", "1")  # no order-0 halves, no pole column
    assert lib.pxm_host_check_address_ranges(*shape) > 0
