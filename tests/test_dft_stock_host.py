"""Truth table of the predicate that sends a fused rings -> X' -> rings launch of the phi-DFT stage to the STOCK kernel
instantiations (csrc/sht_core.h: dft_step_is_stock, through pxm_host_dft_step_is_stock; no GPU): stock is the conjunction

    fused update (X), threshold vector (T), Philox noise (no injected array), two real chains per slot from an even first
    chain, the device-resident iteration addend, neither residual (rdata / rinvcov) nor gather (gidx / gw)

and every single deviation from it is generic."""
import itertools

import pytest

from pxmcmc_amd import ops

MODE_REAL_NOISE, MODE_CPLX_NOISE, MODE_REAL_PAIRS = 0, 1, 2
STOCK_FIELDS = ("X", "T", "iter_dev")
OTHER_FIELDS = ("noise", "rdata", "rinvcov", "gidx", "gw")


def test_field_names_cover_the_eight_bits():
    assert set(ops.DFT_STEP_FIELDS) == set(STOCK_FIELDS) | set(OTHER_FIELDS) and len(ops.DFT_STEP_FIELDS) == 8


def test_the_conjunction_is_stock():
    for chain0 in (0, 6, 2**40):
        assert ops.dft_step_is_stock(STOCK_FIELDS, MODE_REAL_PAIRS, chain0)


@pytest.mark.parametrize("missing", STOCK_FIELDS)
def test_a_missing_operand_is_generic(missing):
    """plain output (no X), scalar T, no device addend"""
    assert not ops.dft_step_is_stock([f for f in STOCK_FIELDS if f != missing], MODE_REAL_PAIRS, 6)


@pytest.mark.parametrize("extra", OTHER_FIELDS)
def test_an_extra_operand_is_generic(extra):
    """injected noise, residual data / inverse covariance, gather index / weight"""
    assert not ops.dft_step_is_stock(STOCK_FIELDS + (extra,), MODE_REAL_PAIRS, 6)


@pytest.mark.parametrize("mode", [MODE_REAL_NOISE, MODE_CPLX_NOISE])
def test_complex_modes_are_generic(mode):
    assert not ops.dft_step_is_stock(STOCK_FIELDS, mode, 6)


@pytest.mark.parametrize("chain0", [1, 7, 2**40 + 1])
def test_an_odd_first_chain_is_generic(chain0):
    assert not ops.dft_step_is_stock(STOCK_FIELDS, MODE_REAL_PAIRS, chain0)


def test_whole_table():
    """all 2^8 operand sets x three modes x both parities: stock exactly on the conjunction"""
    n_stock = 0
    for bits in itertools.product((False, True), repeat=8):
        fields = tuple(f for f, b in zip(ops.DFT_STEP_FIELDS, bits) if b)
        for mode in (MODE_REAL_NOISE, MODE_CPLX_NOISE, MODE_REAL_PAIRS):
            for chain0 in (6, 7):
                want = set(fields) == set(STOCK_FIELDS) and mode == MODE_REAL_PAIRS and chain0 == 6
                assert ops.dft_step_is_stock(fields, mode, chain0) == want, (fields, mode, chain0)
                n_stock += want
    assert n_stock == 1


def test_bits_outside_the_field_mask_are_refused():
    from pxmcmc_amd import _lib

    assert _lib.lib.pxm_host_dft_step_is_stock(1 << 8, MODE_REAL_PAIRS, 6) < 0
    assert b"eight bits" in _lib.lib.pxm_last_error()
