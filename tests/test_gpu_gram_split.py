"""The ring-space MYULA step on the parity-split Gram list (csrc/sht_tables.h: TAB_GRAM_SPLIT) against the oracle's literal
loop and against the dense list (PXM_GRAM_SPLIT=0) on the same inputs.

Shapes: L = 32 (one k-chunk pair per half, kb_p = 0 throughout), L = 64 (kb_p steps from 0 to 16 at m = 31 .. 33,
differently for the two parities), L = 96 (three row tiles per half), L = 40 (Rp = 48: the dense fallback).  Layouts: one
complex chain, three complex chains in an eight-slot plan (padding chains), 16 real chains as 8 pair slots."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, J_MIN, K = 2, 2, 3
SIGMA, LMDA, DELTA = 0.05, 1e-6, 1e-7
SHAPES = [32, 64, 96, 40]
LAYOUTS = ["c1", "c3", "pairs16"]


@functools.lru_cache(maxsize=None)
def _oracle_transform(L):
    from oracle import pxmcmc_np as ref

    return ref.SphericalWaveletTransform(L, B, J_MIN)


@functools.lru_cache(maxsize=None)
def _inputs(L, layout):
    from oracle import pxmcmc_np as ref

    T = _oracle_transform(L)
    P = L * (2 * L - 1)
    rng = np.random.default_rng(1000 * L + len(layout))
    data = rng.normal(size=P)
    if layout != "pairs16":
        data = data.astype(complex)  # one complex slot per chain: complex data, complex uniform inverse covariance
    C = {"c1": 1, "c3": 3, "pairs16": 16}[layout]
    op = ref.ForwardOperator(data, SIGMA, "synthesis", T, ref.Identity(P, P), T.ncoefs)
    assert np.all(op.invcov == op.invcov[0])
    thr = ref.S2_Wavelets_L1("synthesis", None, None, LMDA, L, B, J_MIN).T
    X0 = rng.normal(size=(C, T.ncoefs)) * 1e-3
    noise = rng.normal(size=(K, C, T.ncoefs))
    return op, data, thr, X0, noise


@functools.lru_cache(maxsize=None)
def _oracle_run(L, layout):
    """K literal iterations per checked chain: {chain: (X, preds)}"""
    from oracle import pxmcmc_np as ref

    op, _, thr, X0, noise = _inputs(L, layout)
    out = {}
    for c in {"c1": (0,), "c3": (0, 1, 2), "pairs16": (0, 9, 15)}[layout]:
        X = X0[c].astype(complex)
        preds = op.forward(X)
        for k in range(K):
            X = ref.chain_step(X, ref.soft(X, thr), op.calc_gradg(preds), DELTA, LMDA, noise[k][c])
            preds = op.forward(X)
        out[c] = (X, preds)
    return out


@functools.lru_cache(maxsize=None)
def _gpu_run(L, layout, split):
    """the same K iterations through ring_step: (X, preds over every slot of the plan, status) as numpy"""
    import torch

    from pxmcmc_amd import ops

    op, data, thr, X0, noise = _inputs(L, layout)
    pairs = layout == "pairs16"
    old = os.environ.pop("PXM_GRAM_SPLIT", None)
    if not split:
        os.environ["PXM_GRAM_SPLIT"] = "0"
    try:
        plan = ops.WavPlan(L, B, J_MIN, max_chains={"c1": 1, "c3": 8, "pairs16": 8}[layout])
        if pairs:
            d = ops.as_device(data, torch.float64)
            plan.ring_set_data(torch.complex(d, d).contiguous())  # (the Gram lists are made here: the switch is read now)
            X = torch.complex(ops.as_device(X0[0::2]), ops.as_device(X0[1::2]))
        else:
            plan.ring_set_data(ops.as_device(data, torch.complex128))
            X = ops.as_device(X0, torch.complex128)
    finally:
        os.environ.pop("PXM_GRAM_SPLIT", None)
        if old is not None:
            os.environ["PXM_GRAM_SPLIT"] = old
    T_dev = ops.as_device(thr)
    out = torch.empty_like(X)
    plan.ring_init(X)
    for k in range(K):
        plan.ring_step(X, complex(op.invcov[0]), T_dev, DELTA, LMDA, noise=ops.as_device(noise[k]), out=out, pairs=pairs)
        X, out = out, X
    preds = plan.ring_preds(plan.max_chains)
    return X.cpu().numpy(), preds.cpu().numpy(), plan.status(), plan.workspace_nonfinite()


def _chain(A, c, pairs):
    return (A[c // 2].real if c % 2 == 0 else A[c // 2].imag) if pairs else A[c]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("L", SHAPES)
def test_ring_step_on_the_split_gram_list_matches_the_oracle(L, layout):
    """three ring_step iterations with injected noise against the oracle's literal loop (bench.parity_leg), 1e-11 of
    max |X| (the figure of tests/test_gpu_spinwav.py for ring_step)"""
    Xg, Pg, status, nonfinite = _gpu_run(L, layout, True)
    assert status == 0 and nonfinite == 0
    pairs = layout == "pairs16"
    for c, (Xo, Po) in _oracle_run(L, layout).items():
        if pairs:
            assert np.abs(Xo.imag).max() < 1e-12 * np.abs(Xo).max()
            Xo, Po = Xo.real, Po.real
        ex = np.abs(_chain(Xg, c, pairs) - Xo).max() / np.abs(Xo).max()
        ep = np.abs(_chain(Pg, c, pairs) - Po).max() / np.abs(Po).max()
        print(f"L={L} {layout} chain {c}: X {ex:.2e}, preds {ep:.2e}")
        assert ex < 1e-11
        assert ep < 1e-11
    if layout == "c3":  # slots 3 .. 7 of the plan carry no chain: the Gram epilogue writes them as zero, so do their rings
        assert not Pg[3:].any()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("L", SHAPES)
def test_split_and_dense_gram_lists_agree(L, layout):
    """X and ring_preds of the split list and of PXM_GRAM_SPLIT=0 on the same inputs: 1e-12 relative (the figure
    tests/test_gpu_fullsize.py holds two DFT units to); no bounded wait expired in either plan"""
    Xs, Ps, st_s, nf_s = _gpu_run(L, layout, True)
    Xd, Pd, st_d, nf_d = _gpu_run(L, layout, False)
    assert st_s == 0 and st_d == 0 and nf_s == 0 and nf_d == 0
    ex = np.abs(Xs - Xd).max() / np.abs(Xd).max()
    ep = np.abs(Ps - Pd).max() / np.abs(Pd).max()
    print(f"L={L} {layout}: split vs dense X {ex:.2e}, preds {ep:.2e}")
    assert ex < 1e-12
    assert ep < 1e-12
    if L == 40:  # the fallback IS the dense list
        assert np.array_equal(Xs, Xd) and np.array_equal(Ps, Pd)
