"""The ring GEMM with its epilogue operands fetched at task start (csrc/sht_gemm.hip: the data term of the Gram step, the
per-row scale of the forward combine and b of the pole term go to LDS before the main loop; the per-thread pole sum is formed
there too): three ring_step iterations against the oracle's literal loop (1e-11) and against the dense Gram list on the same
inputs (1e-12), the bounds of tests/test_gpu_gram_split.py and tests/test_gpu_gram_m0.py.

Shapes: L = 32 (one row tile per half, one-chunk tasks, pole tasks) and L = 64 (tasks of 1 .. 4 row tiles, so waves without a
tile and tasks shorter than the 128 rows of the LDS array), L = 40 (Rp = 48, not a multiple of 32: the dense fallback, no pole
term).  Layouts: 16 real chains as 8 pair slots, three complex chains in an eight-slot plan (padding chains), 16 complex chains
(32 columns: the two-column-tile kernels, which the other test files do not launch on the Gram list)."""
import functools
import os

import numpy as np
import pytest

import test_gpu_gram_split as base  # inputs and oracle runs of the layouts that module has are shared with it (computed once)

pytestmark = pytest.mark.gpu

B, J_MIN, K = base.B, base.J_MIN, base.K
SIGMA, DELTA, LMDA = base.SIGMA, base.DELTA, base.LMDA
LAYOUTS = ["pairs16", "c3", "c16"]
C_OF = {"pairs16": 16, "c3": 3, "c16": 16}
SLOTS_OF = {"pairs16": 8, "c3": 8, "c16": 16}
ORACLE_CHAINS = {"c16": (0, 8, 15)}  # (8: the first chain of the second column tile)


@functools.lru_cache(maxsize=None)
def _inputs(L, layout):
    """(op, data, thr, X0, noise): the base module's for its layouts, the same recipe for 16 complex chains"""
    if layout != "c16":
        return base._inputs(L, layout)
    from oracle import pxmcmc_np as ref

    T = base._oracle_transform(L)
    P = L * (2 * L - 1)
    rng = np.random.default_rng(1000 * L + 16)
    data = rng.normal(size=P).astype(complex)
    op = ref.ForwardOperator(data, SIGMA, "synthesis", T, ref.Identity(P, P), T.ncoefs)
    assert np.all(op.invcov == op.invcov[0])
    thr = ref.S2_Wavelets_L1("synthesis", None, None, LMDA, L, B, J_MIN).T
    X0 = rng.normal(size=(16, T.ncoefs)) * 1e-3
    noise = rng.normal(size=(K, 16, T.ncoefs))
    return op, data, thr, X0, noise


@functools.lru_cache(maxsize=None)
def _oracle_run(L, layout):
    """K literal iterations per checked chain: {chain: (X, preds)}"""
    if layout != "c16":
        return base._oracle_run(L, layout)
    from oracle import pxmcmc_np as ref

    op, _, thr, X0, noise = _inputs(L, layout)
    out = {}
    for c in ORACLE_CHAINS[layout]:
        X = X0[c].astype(complex)
        preds = op.forward(X)
        for k in range(K):
            X = ref.chain_step(X, ref.soft(X, thr), op.calc_gradg(preds), DELTA, LMDA, noise[k][c])
            preds = op.forward(X)
        out[c] = (X, preds)
    return out


def _make_plan(L, layout, data, split):
    """a plan whose Gram list is built under PXM_GRAM_SPLIT = split (None: unset, the list a user gets)"""
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
    op, data, thr, X0, noise = _inputs(L, layout)
    return _steps(_make_plan(L, layout, data, split), op, thr, _device_state(X0, layout), noise, layout)


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _check_lists_and_oracle(tag, layout, runs, oracle):
    """runs: {split: (X, preds, status, nonfinite)} with None = the default list; oracle: {chain: (X, preds)}"""
    Xn, Pn, st, nf = runs[None]
    assert st == 0 and nf == 0
    for split, (Xs, Ps, st_s, nf_s) in runs.items():
        if split is None:
            continue
        assert st_s == 0 and nf_s == 0
        ex, ep = _rel(Xn, Xs), _rel(Pn, Ps)
        print(f"{tag}: default list vs PXM_GRAM_SPLIT={split}: X {ex:.2e}, preds {ep:.2e}")
        assert ex < 1e-12
        assert ep < 1e-12
    pairs = layout == "pairs16"
    for c, (Xo, Po) in oracle.items():
        if pairs:
            Xo, Po = Xo.real, Po.real
        ex, ep = _rel(base._chain(Xn, c, pairs), Xo), _rel(base._chain(Pn, c, pairs), Po)
        print(f"{tag} chain {c}: oracle X {ex:.2e}, preds {ep:.2e}")
        assert ex < 1e-11
        assert ep < 1e-11
    if layout == "c3":  # slots 3 .. 7 carry no chain: the Gram epilogue writes them as zero, so do their rings
        assert not Pn[3:].any()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("L", [32, 64, 40])
def test_three_steps_against_the_dense_list_and_the_oracle(L, layout):
    """three ring_step iterations with injected noise: the default list against the dense one within 1e-12 of max |X| /
    max |preds| (L = 40: the default IS the dense list, bit for bit), against the oracle's literal loop within 1e-11;
    slots without a chain stay exactly zero"""
    runs = {s: _gpu_run(L, layout, s) for s in (None, "0")}
    _check_lists_and_oracle(f"L={L} {layout}", layout, runs, _oracle_run(L, layout))
    if L == 40:
        assert np.array_equal(runs[None][0], runs["0"][0]) and np.array_equal(runs[None][1], runs["0"][1])


def _one_step_oracle(op, thr, X0, noise, chains):
    from oracle import pxmcmc_np as ref

    out = {}
    for c in chains:
        Xc = X0[c].astype(complex)
        Xo = ref.chain_step(Xc, ref.soft(Xc, thr), op.calc_gradg(op.forward(Xc)), DELTA, LMDA, noise[0][c])
        out[c] = (Xo, op.forward(Xo))
    return out


def _one_step_case(tag, L, layout, op, data, thr, X0, noise):
    runs = {s: _steps(_make_plan(L, layout, data, s), op, thr, _device_state(X0, layout), noise[:1], layout) for s in (None, "0")}
    _check_lists_and_oracle(tag, layout, runs, _one_step_oracle(op, thr, X0, noise, (0, C_OF[layout] - 1)))
    return runs[None]


@pytest.mark.parametrize("L,layout", [(32, "c16"), (64, "pairs16"), (32, "c3")])
def test_one_step_from_zero_state(L, layout):
    """X = 0: the contraction of the Gram launch multiplies zeros and the data term read at task start is its whole output"""
    op, data, thr, X0, noise = _inputs(L, layout)
    Xn, _, _, _ = _one_step_case(f"L={L} {layout} X=0", L, layout, op, data, thr, np.zeros_like(X0), noise)
    assert Xn.any()


@pytest.mark.parametrize("L,layout", [(32, "c16"), (64, "pairs16"), (32, "c3")])
def test_one_step_with_zero_data(L, layout):
    """data = 0: the data term is zero, the row scales of the forward combine are still live"""
    from oracle import pxmcmc_np as ref

    op, data, thr, X0, noise = _inputs(L, layout)
    T = base._oracle_transform(L)
    P = L * (2 * L - 1)
    data0 = np.zeros_like(data)
    op0 = ref.ForwardOperator(data0, SIGMA, "synthesis", T, ref.Identity(P, P), T.ncoefs)
    _one_step_case(f"L={L} {layout} data=0", L, layout, op0, data0, thr, X0, noise)


@functools.lru_cache(maxsize=None)
def _one_parity_state(L, layout, parity):
    """a start point whose synthesised signal has, at order 0, only degrees of one parity (every other order as drawn):
    X0 = analysis of such a signal, so the Gram operand of the first step has that structure"""
    from oracle import ssht

    X0 = _inputs(L, layout)[3]
    T = base._oracle_transform(L)
    rng = np.random.default_rng(11 * L + parity)
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
    return X


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("L,layout", [(32, "c16"), (64, "pairs16"), (32, "c3")])
def test_early_pole_sum_alone_carries_the_cross_parity_answer(L, layout, parity):
    """one step from a state whose order-0 Gram operand has only even (parity 0) or only odd degrees: the half task of the
    empty parity multiplies zeros, and the pole sum it formed before its loop is its whole result"""
    op, data, thr, _, noise = _inputs(L, layout)
    _one_step_case(f"L={L} {layout} parity {parity}", L, layout, op, data, thr, _one_parity_state(L, layout, parity), noise)


def test_graph_replay_equals_eager_stepping():
    """two ring_step iterations captured in a graph and replayed give the bits of the same two iterations stepped eagerly
    (L = 64, 16 complex chains: two column groups per launch)"""
    import torch

    from pxmcmc_amd import ops

    L, layout = 64, "c16"
    op, data, thr, X0, noise = _inputs(L, layout)
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
