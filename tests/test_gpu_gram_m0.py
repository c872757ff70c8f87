"""The ring-space MYULA step on the Gram list with order 0 split as well (csrc/sht_tables.h: TAB_GRAM_SPLIT0: two half tasks
on the parity-permuted order-0 block plus the rank-one pole term) against the list with order 0 dense (PXM_GRAM_SPLIT=1),
the dense list (PXM_GRAM_SPLIT=0) and the oracle's literal loop, on the inputs of tests/test_gpu_gram_split.py.

Shapes: L = 32 (one row tile per half: the smallest size with halves and a reduction), L = 64, L = 96 (three row tiles per
half), L = 40 (Rp = 48: the dense fallback).  Layouts: one complex chain, three complex chains in an eight-slot plan, 16 real
chains as 8 pair slots."""
import functools
import os

import numpy as np
import pytest

import test_gpu_gram_split as base  # the inputs and the oracle runs are shared with that module (computed once)

pytestmark = pytest.mark.gpu

B, J_MIN, K = base.B, base.J_MIN, base.K
DELTA, LMDA = base.DELTA, base.LMDA
SHAPES, LAYOUTS = [32, 64, 96, 40], ["c1", "c3", "pairs16"]
C_OF = {"c1": 1, "c3": 3, "pairs16": 16}
SLOTS_OF = {"c1": 1, "c3": 8, "pairs16": 8}


def _make_plan(L, layout, data, split):
    """a plan whose Gram list is built under PXM_GRAM_SPLIT = split (None: unset, the new list)"""
    import torch

    from pxmcmc_amd import ops

    old = os.environ.pop("PXM_GRAM_SPLIT", None)
    if split is not None:
        os.environ["PXM_GRAM_SPLIT"] = split
    try:
        plan = ops.WavPlan(L, B, J_MIN, max_chains=SLOTS_OF[layout])
        if layout == "pairs16":
            d = ops.as_device(data, torch.float64)
            plan.ring_set_data(torch.complex(d, d).contiguous())  # (the Gram lists are made here: the switch is read now)
        else:
            plan.ring_set_data(ops.as_device(data, torch.complex128))
    finally:
        os.environ.pop("PXM_GRAM_SPLIT", None)
        if old is not None:
            os.environ["PXM_GRAM_SPLIT"] = old
    return plan


def _device_state(X0, layout):
    import torch

    from pxmcmc_amd import ops

    if layout == "pairs16":
        return torch.complex(ops.as_device(X0[0::2]), ops.as_device(X0[1::2]))
    return ops.as_device(X0, torch.complex128)


def _steps(plan, op, thr, X, noise, layout):
    import torch

    from pxmcmc_amd import ops

    T_dev = ops.as_device(thr)
    out = torch.empty_like(X)
    plan.ring_init(X)
    for k in range(len(noise)):
        plan.ring_step(X, complex(op.invcov[0]), T_dev, DELTA, LMDA, noise=ops.as_device(noise[k]), out=out, pairs=layout == "pairs16")
        X, out = out, X
    preds = plan.ring_preds(plan.max_chains)
    return X.cpu().numpy(), preds.cpu().numpy(), plan.status(), plan.workspace_nonfinite()


@functools.lru_cache(maxsize=None)
def _gpu_run(L, layout, split):
    op, data, thr, X0, noise = base._inputs(L, layout)
    return _steps(_make_plan(L, layout, data, split), op, thr, _device_state(X0, layout), noise, layout)


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("L", SHAPES)
def test_order_0_halves_against_the_other_lists_and_the_oracle(L, layout):
    """three ring_step iterations with injected noise: the new list against PXM_GRAM_SPLIT=1 and =0 on the same inputs
    within 1e-12 of max |X| / max |preds|, against the oracle's literal loop within 1e-11 (the bounds of
    tests/test_gpu_gram_split.py); slots without a chain stay exactly zero; L = 40 is the dense list, bit for bit"""
    Xn, Pn, st, nf = _gpu_run(L, layout, None)
    assert st == 0 and nf == 0
    for split in ("1", "0"):
        Xs, Ps, st_s, nf_s = _gpu_run(L, layout, split)
        assert st_s == 0 and nf_s == 0
        ex, ep = _rel(Xn, Xs), _rel(Pn, Ps)
        print(f"L={L} {layout}: new list vs PXM_GRAM_SPLIT={split}: X {ex:.2e}, preds {ep:.2e}")
        assert ex < 1e-12
        assert ep < 1e-12
        if L == 40:
            assert np.array_equal(Xn, Xs) and np.array_equal(Pn, Ps)
    pairs = layout == "pairs16"
    for c, (Xo, Po) in base._oracle_run(L, layout).items():
        if pairs:
            Xo, Po = Xo.real, Po.real
        ex, ep = _rel(base._chain(Xn, c, pairs), Xo), _rel(base._chain(Pn, c, pairs), Po)
        print(f"L={L} {layout} chain {c}: oracle X {ex:.2e}, preds {ep:.2e}")
        assert ex < 1e-11
        assert ep < 1e-11
    if layout == "c3":  # slots 3 .. 7 carry no chain
        assert not Pn[3:].any()


@functools.lru_cache(maxsize=None)
def _one_parity_inputs(L, layout, parity):
    """the inputs of the module with a start point whose synthesised signal has, at order 0, only degrees of one parity
    (every other order as drawn): X0 = analysis of such a signal, so the Gram operand of the first step has that structure"""
    from oracle import ssht

    op, data, thr, X0, noise = base._inputs(L, layout)
    T = base._oracle_transform(L)
    rng = np.random.default_rng(7 * L + parity)
    els = np.arange(L)
    cplx = layout != "pairs16"
    X = np.empty(X0.shape, dtype=complex if cplx else float)
    for c in range(X0.shape[0]):
        flm = rng.normal(size=L * L) + 1j * rng.normal(size=L * L)
        if not cplx:  # a real signal: f_{l,-m} = (-1)^m conj(f_{l,m})
            for el in range(L):
                flm[el * el + el] = flm[el * el + el].real
                for m in range(1, el + 1):
                    flm[el * el + el - m] = (-1) ** m * np.conj(flm[el * el + el + m])
        flm[(els * els + els)[els % 2 != parity]] = 0.0
        Xc = T.forward(ssht.inverse(flm, L)) * 1e-3
        if not cplx:
            assert np.abs(Xc.imag).max() < 1e-12 * np.abs(Xc).max()
        X[c] = Xc if cplx else Xc.real
    return op, data, thr, X, noise[:1]


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("L,layout", [(32, "c3"), (64, "pairs16")])
def test_pole_term_alone_carries_the_cross_parity_answer(L, layout, parity):
    """one step from a state whose order-0 Gram operand has only even (parity 0) or only odd degrees: the half task of the
    empty parity multiplies zeros and its whole result is the pole term, so a missing, doubled or mis-signed term shows in
    full.  Same bounds: 1e-12 against the two other lists, 1e-11 against the oracle's literal step."""
    from oracle import pxmcmc_np as ref

    op, data, thr, X0, noise = _one_parity_inputs(L, layout, parity)
    runs = {s: _steps(_make_plan(L, layout, data, s), op, thr, _device_state(X0, layout), noise, layout) for s in (None, "1", "0")}
    Xn, Pn, st, nf = runs[None]
    assert st == 0 and nf == 0
    for s in ("1", "0"):
        ex, ep = _rel(Xn, runs[s][0]), _rel(Pn, runs[s][1])
        print(f"L={L} {layout} parity {parity}: new list vs PXM_GRAM_SPLIT={s}: X {ex:.2e}, preds {ep:.2e}")
        assert ex < 1e-12
        assert ep < 1e-12
    pairs = layout == "pairs16"
    for c in (0, C_OF[layout] - 1):
        Xc = X0[c].astype(complex)
        Xo = ref.chain_step(Xc, ref.soft(Xc, thr), op.calc_gradg(op.forward(Xc)), DELTA, LMDA, noise[0][c])
        Po = op.forward(Xo)
        if pairs:
            Xo, Po = Xo.real, Po.real
        ex, ep = _rel(base._chain(Xn, c, pairs), Xo), _rel(base._chain(Pn, c, pairs), Po)
        print(f"L={L} {layout} parity {parity} chain {c}: oracle X {ex:.2e}, preds {ep:.2e}")
        assert ex < 1e-11
        assert ep < 1e-11
    if layout == "c3":
        assert not Pn[3:].any()


def test_graph_replay_of_the_new_list_equals_eager_stepping():
    """two ring_step iterations captured in a graph and replayed give the bits of the same two iterations stepped eagerly
    (L = 64, three complex chains): the pole reduction has a fixed summation order"""
    import torch

    from pxmcmc_amd import ops

    L, layout = 64, "c3"
    op, data, thr, X0, noise = base._inputs(L, layout)
    plan = _make_plan(L, layout, data, None)
    T_dev = ops.as_device(thr)
    n0, n1 = ops.as_device(noise[0]), ops.as_device(noise[1])
    w = complex(op.invcov[0])
    X = _device_state(X0, layout)
    A, Bf = torch.empty_like(X), torch.empty_like(X)

    def two_steps():
        plan.ring_step(X, w, T_dev, DELTA, LMDA, noise=n0, out=A)
        plan.ring_step(A, w, T_dev, DELTA, LMDA, noise=n1, out=Bf)

    plan.ring_init(X)
    two_steps()
    eager_X, eager_P = Bf.cpu().numpy().copy(), plan.ring_preds(plan.max_chains).cpu().numpy()
    plan.ring_init(X)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.capture_scope(), torch.cuda.graph(g):
        two_steps()
    A.zero_()
    Bf.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(Bf.cpu().numpy(), eager_X)
    assert np.array_equal(plan.ring_preds(plan.max_chains).cpu().numpy(), eager_P)
    assert plan.status() == 0
