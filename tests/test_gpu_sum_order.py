"""The summation order of the per-chain sums (csrc/reduce.h), pinned bit for bit.  The other tests of these sums compare two
device paths with each other; all of them go through the same helpers, so they would still agree if the order changed.  Here a
numpy model of the order is compared with the device in the three places where numpy forms every term exactly as the kernel
does (one rounded operation per term, or contraction off): ops.reduce_l1, the sums of ops.fista_step with a given prox, and
the G of ops.sapg_step's trace."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _tree64(v):
    """the __shfl_down halving tree over the last axis (64 lanes), offsets 32 ... 1: what lane 0 holds"""
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def fixed_order_sum(terms, slices, block=256):
    """sum of one chain's non-negative float64 terms in the order of csrc/reduce.h"""
    n, stride = terms.size, slices * block
    passes = -(-n // stride)
    padded = np.zeros(passes * stride)  # (a thread past the end adds nothing; x + 0.0 is x for x >= 0)
    padded[:n] = terms
    acc = np.zeros((slices, block))
    for k in range(passes):  # 1. thread t of slice b adds elements b block + t + k slices block one after the other
        acc = acc + padded[k * stride:(k + 1) * stride].reshape(slices, block)
    waves = _tree64(acc.reshape(slices, block // 64, 64))  # 2. the lanes of each wave by the tree
    part = np.zeros(slices)
    for w in range(block // 64):  # 3. thread 0 adds the waves one after the other, from 0.0
        part = part + waves[:, w]
    rows = -(-slices // 64)
    padded = np.zeros(rows * 64)
    padded[:slices] = part
    lanes = np.zeros(64)
    for r in range(rows):  # 4. lane l of the finishing kernel adds slices l, l + 64, ..., then the tree
        lanes = lanes + padded[r * 64:(r + 1) * 64]
    return float(_tree64(lanes))


def red_slices(n):
    return int(min(1024, max(64, (n + 2047) // 2048)))


def chain_slices(n, most=256):
    return int(min(most, max(1, (n + 255) // 256)))


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    print("device", [float(x).hex() for x in got.ravel()], "model", [float(x).hex() for x in want.ravel()])
    return np.array_equal(got.view(np.int64), want.view(np.int64))


@pytest.mark.parametrize("n", [133121, 300, 1024 * 2048 + 2049])
def test_reduce_l1(n):
    """terms |x|; 133121 elements: 66 slices (the slice stage wraps past lane 63) and the grid strides; 300: 64 slices, most
    of them empty, and a partial last wave; 2099201: the slice count stops at RED_SLICES_MAX = 1024 (uncapped it would be
    1026), which the caller-owned scratch is sized by -- 9 passes of the grid, 16 rows of slices in the finishing kernel"""
    from pxmcmc_amd import ops

    C = 3
    assert red_slices(n) == {133121: 66, 300: 64, 2099201: 1024}[n]
    X = np.random.default_rng(n).normal(size=(C, n))
    got = ops.reduce_l1(ops.as_device(X)).cpu().numpy()
    want = [fixed_order_sum(np.abs(X[c]), red_slices(n)) for c in range(C)]
    assert _same_bits(got, want)


@pytest.mark.parametrize("n", [70001, 257])
def test_fista_sums_given_prox(n):
    """sums 0 and 1 of a step with a given prox (contraction off: d * d and x1 * x1 are numpy's products); 70001 elements:
    256 slices and the grid strides; 257: two slices"""
    from pxmcmc_amd import ops

    C = 2
    assert chain_slices(n) == (256 if n == 70001 else 2)
    rng = np.random.default_rng(n)
    P, X0 = rng.normal(size=(C, n)), rng.normal(size=(C, n))
    _, _, sums = ops.fista_step(None, None, ops.as_device(X0), 0.5, 1.0, [0.3], proxf=ops.as_device(P))
    sums = sums.cpu().numpy()
    d = P - X0
    want = [[fixed_order_sum(d[c] * d[c], chain_slices(n)), fixed_order_sum(P[c] * P[c], chain_slices(n))] for c in range(C)]
    assert _same_bits(sums[:, :2], want)


@pytest.mark.parametrize("n", [70001, 257])
def test_sapg_trace_sum(n):
    """G_c of the trace row = (sum_i T_i |X1_i|) / lmda from the step's own output (contraction off: t * fabs(x1) is numpy's
    product); same two lengths"""
    import torch

    from pxmcmc_amd import ops

    C, delta, lmda = 2, 0.9e-2, 2.5e-2
    rng = np.random.default_rng(n)
    X, g, T = rng.normal(size=(C, n)), rng.normal(size=(C, n)), np.abs(rng.normal(size=n))
    theta = ops.as_device(np.array([0.7, 1.9]), torch.float64)
    eta = torch.log(theta)
    trace = torch.full((1, C, 3), float("nan"), dtype=torch.float64, device=ops.device())
    X1, _, _ = ops.sapg_step(ops.as_device(X), ops.as_device(g), ops.as_device(T, torch.float64), delta, lmda, theta, eta, float(n),
                             [0.0], -50.0, 50.0, pool=False, trace=trace, seed=4)
    X1 = X1.cpu().numpy()
    want = [fixed_order_sum(T * np.abs(X1[c]), chain_slices(n)) / lmda for c in range(C)]
    assert _same_bits(trace[0, :, 2].cpu().numpy(), want)
