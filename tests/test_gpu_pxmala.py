"""The PxMALA iteration kernels on the GPU (csrc/pxmala.hip: k_pxmala_propose, k_pxmala_tail_partial, k_pxmala_accept2 /
accept3; csrc/elementwise.hip: k_select_copy_many; philox_uniform) against the extended-precision model of tests/test_pxmala_host.py: every
element of the proposal, every sum, the stored log transition terms, the Metropolis decision at a known distance from the
model's log acceptance ratio, the delta adaptation with its clamps, the trace ring, the device counter, the uniform stream
and the conditional copy.  Every buffer is allocated for more chains than are used and prefilled with NaN or a sentinel;
every test asserts that nothing past the used chains is written.  Below them, whole PxMALA.run runs: the early-stop flag, the
fused tail against the separate calls, and the route of a user-supplied prior against the numpy sampler."""
import contextlib
import io

import numpy as np
import pytest

from oracle import philox
from test_pxmala_host import (C0_MEASURED, EPS, LMDA, _f64abs, _ld, accept_chain_model, error_scale, l1_sum_bound, l2_ext,
                              l2_sum_bound, logtrans_bound, logtrans_ext, propose_ext, propose_inputs, ratio_to_ext, sq_sum_bound,
                              soft_ext, sum_l1_ext, sum_sq_ext, tail_inputs, trans_scale, transition_term_ext)

pytestmark = pytest.mark.gpu

C_BOUND = 4 * C0_MEASURED  # the margin tests/test_gpu_fista.py gives its kernel over its numpy route: device sqrt / division
PAD = 2  # chains the buffers are allocated for beyond the used ones
SENT_I, SENT_F = -77, -12345.0  # sentinels of the trace rings
NAN_BITS = 0x7FF80000DEADBEEF  # a NaN with a payload: "kept bit for bit" is checked through an int64 view
MU = 1.3


def _t():
    import torch

    return torch


def _dt(cplx):
    return _t().complex128 if cplx else _t().float64


def _padded(a, dt=None, fill=float("nan")):
    """numpy [C, ...] -> device buffer [C + PAD, ...] of NaN (or ``fill``) holding a in its first rows"""
    from pxmcmc_amd import ops

    torch = _t()
    a = np.asarray(a)
    dt = dt or _dt(np.iscomplexobj(a))
    t = torch.full((a.shape[0] + PAD,) + a.shape[1:], fill, dtype=dt, device=ops.device())
    t[: a.shape[0]] = ops.as_device(a, dt) if dt in (torch.float64, torch.complex128) else torch.as_tensor(a, dtype=dt, device=t.device)
    return t


def _empty(C, tail, dt, fill=float("nan")):
    from pxmcmc_amd import ops

    return _t().full((C + PAD,) + tuple(tail), fill, dtype=dt, device=ops.device())


def _bits(t):
    """the tensor's bytes as int64 (numpy)"""
    torch = _t()
    t = t.contiguous()
    if t.dtype == torch.int32:
        return t.cpu().numpy().astype(np.int64)
    return (torch.view_as_real(t) if t.is_complex() else t).view(torch.int64).cpu().numpy()


def _untouched(t, C):
    """nothing past chain C: the padding still holds its NaN"""
    tail = t[C:]
    return bool(_t().isnan(tail.real if tail.is_complex() else tail).all())


def _slices(n):
    return int(min(1024, max(64, (n + 2047) // 2048)))


def _T_arg(T):
    from pxmcmc_amd import ops

    return ops.as_device(T, _t().float64) if np.ndim(T) else float(T)


# ---- proposal ---------------------------------------------------------------------------------------------------------------
def _run_propose(inp, C, given_prox, use_wts, deferred=False, chains=None, philox_kw=None):
    """pxm_pxmala_propose on chains [0, C) (or the listed ones, one launch each) -> dict of device tensors"""
    from pxmcmc_amd import ops

    torch = _t()
    X, G, W, T, wts, delta, lmda = (inp[k] for k in ("X", "G", "W", "T", "wts", "delta", "lmda"))
    n, cplx = X.shape[1], np.iscomplexobj(X)
    bX, bG, bD = _padded(X[:C]), _padded(G[:C]), _padded(delta[:C])
    bW = None if philox_kw else _padded(W[:C])
    Td = _T_arg(T)
    bP = bPp = None
    if given_prox:
        bP = _empty(C, (n,), _dt(cplx))
        bP[:C] = ops.soft(bX[:C], Td)
        bPp = _empty(C, (n,), _dt(cplx))
    bXp = _empty(C, (n,), _dt(cplx))
    lt, prior = (None, None) if deferred else (_empty(C, (), torch.complex128), _empty(C, (), torch.float64))
    per_chain = 4 * _slices(n)
    scratch = torch.full((4 * ops.reduce_scratch_doubles(C + PAD),), float("nan"), dtype=torch.float64, device=bX.device)
    for sl in ([slice(0, C)] if chains is None else [slice(c, c + 1) for c in chains]):
        sc = scratch if chains is None else scratch[sl.start * per_chain:]
        kw = dict(philox_kw) if philox_kw else dict(noise=bW[sl])
        if philox_kw and chains is not None:
            kw["chain0"] = kw.get("chain0", 0) + sl.start
        ops.pxmala_propose(bX[sl], None if bP is None else bP[sl], bG[sl], Td, wts if use_wts else None, bD[sl], lmda, bXp[sl],
                           None if bPp is None else bPp[sl], None if lt is None else lt[sl], None if prior is None else prior[sl],
                           scratch=sc, **kw)
    torch.cuda.synchronize()
    assert _untouched(bXp, C) and (bPp is None or _untouched(bPp, C)) and (lt is None or (_untouched(lt, C) and _untouched(prior, C)))
    assert bool(torch.isnan(scratch[C * per_chain:]).all()) and not bool(torch.isnan(scratch[: C * per_chain]).any())
    return dict(X=bX, G=bG, D=bD, P=bP, Xp=bXp, Pp=bPp, lt=lt, prior=prior, scratch=scratch, T=Td)


def _partial_sums(scratch, C, slices, width):
    """the per-slice partial sums of a reduction, added here in extended precision -> [C, width]"""
    part = scratch[: C * slices * width].cpu().numpy().reshape(C, slices, width)
    return np.sum(_ld(part), axis=1)


OPTIONS = {  # (given prox, vector T, weights, complex draw on a complex state)
    "kernelprox-vecT-wts-cnoise": (False, True, True, True),
    "givenprox-scalarT-nowts-rnoise": (True, False, False, False),
    "kernelprox-scalarT-wts-rnoise": (False, False, True, False),
    "givenprox-vecT-nowts-cnoise": (True, True, False, True),
}


@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 257, 32769, 133121])
def test_proposal_against_extended_model(n, C, cplx, opt):
    """X' and P' per element within 4 x C0_MEASURED x 2^-52 S_e of the model; S (from the slices), A, lt and the prior within
    the sum bounds of tests/test_pxmala_host.py; a given prox soft(X, T) equals the kernel-formed one bit for bit; each chain
    equals the chain run alone; 32769 = 64 slices x 512 threads + 1 (grid stride), 133121 -> 66 slices (second trip of the
    totals loop)"""
    given, vecT, use_wts, ncplx = OPTIONS[opt]
    inp = propose_inputs(n, C, cplx, vecT, seed=1000 + n + 7 * C + 2 * cplx + sum(map(ord, opt)), noise_cplx=ncplx)
    X, G, W, T, wts, delta, lmda = (inp[k] for k in ("X", "G", "W", "T", "wts", "delta", "lmda"))
    if n == 1 and vecT:
        inp["T"] = T = float(T[0])
    out = _run_propose(inp, C, given, use_wts)
    Xp, lt, prior = out["Xp"][:C].cpu().numpy(), out["lt"][:C].cpu().numpy(), out["prior"][:C].cpu().numpy()
    assert np.isfinite(Xp.view(float)).all()
    P_in = out["P"][:C].cpu().numpy() if given else None
    eXp, ePp, er = propose_ext(X, P_in, G, W, T, delta, lmda)
    p64 = P_in if given else np.asarray(soft_ext(_ld(X), T)).astype(X.dtype)
    S_e = error_scale(X, p64, G, W, delta, lmda)
    worst = ratio_to_ext(Xp, eXp, S_e)
    if given:
        worst = max(worst, ratio_to_ext(out["Pp"][:C].cpu().numpy(), ePp, S_e))
    e_x = C_BOUND * EPS * S_e
    e_r = C_BOUND * EPS * (S_e + trans_scale(X, Xp, p64, G, delta, lmda))
    wt = wts if use_wts else None
    RS = _slices(n)
    part = _partial_sums(out["scratch"], C, RS, 4)
    bS, bA = sq_sum_bound(er, e_r, n), l1_sum_bound(eXp, e_x, wt, n)
    S_ext, A_ext = sum_sq_ext(er), sum_l1_ext(eXp, wt)
    S_got = part[:, 0] + (1j * part[:, 1] if cplx else 0)
    assert cplx or np.all(part[:, 1] == 0)
    rS = float(np.max(_f64abs(S_got - S_ext) / bS))
    rA = float(np.max(_f64abs(part[:, 2] - A_ext) / np.where(bA > 0, bA, 1)))
    rlt = float(np.max(_f64abs(_ld(lt) - logtrans_ext(S_ext, delta)) / logtrans_bound(S_ext, bS, delta)))
    rpr = float(np.max(_f64abs(_ld(prior) - A_ext) / np.where(bA > 0, bA, 1)))
    print(f"n={n} C={C} cplx={cplx} {opt}: worst element ratio {worst:.3f} (bound {C_BOUND:.2f}); sums, error / bound: "
          f"S {rS:.3e} A {rA:.3e} lt {rlt:.3e} prior {rpr:.3e} (bound 1)")
    assert worst <= C_BOUND
    assert max(rS, rA, rlt, rpr) <= 1.0
    # the other form of the prox: bit for bit (X', the sums; P' is only written with a given prox)
    other = _run_propose(inp, C, not given, use_wts)
    for k in ("Xp", "lt", "prior"):
        assert np.array_equal(_bits(other[k][:C]), _bits(out[k][:C])), k
    if not given:  # P' of the given-prox form against the model too
        rP = ratio_to_ext(other["Pp"][:C].cpu().numpy(), ePp, S_e)
        print(f"    P' (given-prox launch): {rP:.3f}")
        assert rP <= C_BOUND
        if vecT and n >= 17:
            Pp = other["Pp"][:C].cpu().numpy()
            assert np.all(Pp[:, [9, 16]] == 0) and np.array_equal(Pp[:, 5], Xp[:, 5])  # T above every |x|; T = 0 keeps X'
    if C > 1:  # each chain alone
        alone = _run_propose(inp, C, given, use_wts, chains=range(C))
        for k in ("Xp", "Pp", "lt", "prior"):
            assert out[k] is None or np.array_equal(_bits(alone[k][:C]), _bits(out[k][:C])), k


@pytest.mark.parametrize("noise64", [False, True], ids=["bm32", "bm64"])
@pytest.mark.parametrize("kind", ["f64", "c128-real-draw", "c128-complex-draw"])
def test_proposal_philox_path_equals_injected_draw(kind, noise64):
    """the Philox path has no model value: it must equal, bit for bit, the launch that is fed ops.randn's draw of the same
    (seed, chain0, it + *iter_dev, noise64) as injected noise; it and *iter_dev both non-zero"""
    from pxmcmc_amd import ops

    torch = _t()
    cplx, ncplx = kind != "f64", kind == "c128-complex-draw"
    n, C, seed, chain0, it, it_dev = 2051, 3, 99, 5, 3, 4
    inp = propose_inputs(n, C, cplx, True, seed=77, noise_cplx=ncplx)
    draw = ops.randn(n, C_=C, complex_=ncplx, seed=seed, chain0=chain0, it=it + it_dev, noise64=noise64)
    inp["W"] = draw.cpu().numpy()
    injected = _run_propose(inp, C, False, True)
    cnt = torch.full((1,), it_dev, dtype=torch.int64, device=ops.device())
    kw = dict(noise=None, noise_complex=ncplx, seed=seed, chain0=chain0, it=it, iter_dev=cnt, noise64=noise64)
    drawn = _run_propose(inp, C, False, True, philox_kw=kw)
    for k in ("Xp", "lt", "prior"):
        assert np.array_equal(_bits(drawn[k][:C]), _bits(injected[k][:C])), k
    assert int(cnt[0]) == it_dev
    alone = _run_propose(inp, C, False, True, philox_kw=kw, chains=range(C))  # chain0 + c keys the draw, not the launch
    assert np.array_equal(_bits(alone["Xp"][:C]), _bits(drawn["Xp"][:C]))
    wrong = _run_propose(inp, C, False, True, philox_kw=dict(kw, iter_dev=None))  # the counter is part of the draw
    assert not np.array_equal(_bits(wrong["Xp"][:C]), _bits(drawn["Xp"][:C]))


# ---- tail + accept --------------------------------------------------------------------------------------------------------
class _Iteration:
    """one PxMALA iteration on the device up to the accept test: the proposal (totals immediate and deferred), the tail
    inputs, and the accept state; ``finish`` / ``accept`` run the two routes on copies of the state"""

    def __init__(self, n, nd, C, cplx, dcplx, icplx, vecT, given_prox, seed, delta=None):
        from pxmcmc_amd import ops

        torch = _t()
        self.n, self.nd, self.C, self.cplx, self.given = n, nd, C, cplx, given_prox
        inp = propose_inputs(n, C, cplx, vecT, seed=seed)
        if n == 1 and vecT:
            inp["T"] = float(inp["T"][0])
        if delta is not None:
            inp["delta"] = np.asarray(delta, dtype=float)
        self.inp = inp
        self.t = t = tail_inputs(n, nd, C, cplx, dcplx, icplx, vecT, seed=seed + 1)
        self.lmda, self.delta, self.T, self.wts = inp["lmda"], inp["delta"], inp["T"], inp["wts"]
        self.now = _run_propose(inp, C, given_prox, True)
        self.later = _run_propose(inp, C, given_prox, True, deferred=True)
        assert np.array_equal(_bits(self.later["Xp"][:C]), _bits(self.now["Xp"][:C]))
        self.Gp = _padded(t["G"])  # the proposal's gradient
        self.preds, self.data, self.invcov = _padded(t["preds"]), ops.as_device(t["data"]), ops.as_device(t["invcov"])
        self.X1, self.X2 = self.now["Xp"][:C].cpu().numpy(), inp["X"]
        self.P1 = self.now["Pp"][:C].cpu().numpy() if given_prox else None
        self.fin_scratch_len = 2 * ops.reduce_scratch_doubles(C)
        self.dev = ops.device()
        self.torch = torch

    def state(self, logpi_c, L2_c, prior_c, delta=None):
        return dict(logpi=_padded(logpi_c, self.torch.complex128), L2=_padded(L2_c, self.torch.complex128), prior=_padded(prior_c),
                    delta=_padded(self.delta if delta is None else delta), accept=_empty(self.C, (), self.torch.int32, fill=SENT_I))

    def traces(self, chunk):
        if not chunk:
            return None, None
        return (self.torch.full((chunk + 1, self.C), SENT_I, dtype=self.torch.int32, device=self.dev),
                self.torch.full((chunk + 1, self.C), SENT_F, dtype=self.torch.float64, device=self.dev))

    def finish(self, st, u, tune, it=0, counter=None, bump=None, chunk=0, seed=0, chain0=0):
        from pxmcmc_amd import ops

        torch, C = self.torch, self.C
        tot = dict(lt_pc=_empty(C, (), torch.complex128), lt_cp=_empty(C, (), torch.complex128), prior_p=_empty(C, (), torch.float64),
                   L2_p=_empty(C, (), torch.complex128))
        scratch = torch.full((self.fin_scratch_len + 64,), float("nan"), dtype=torch.float64, device=self.dev)
        at, dtr = self.traces(chunk)
        ops.pxmala_finish(self.now["Xp"][:C], self.now["X"][:C], self.now["Pp"][:C] if self.given else None, self.Gp[:C], self.preds[:C],
                          self.data, self.invcov, self.later["scratch"], MU, self.lmda, st["logpi"][:C], st["L2"][:C], st["prior"][:C],
                          st["accept"][:C], st["delta"][:C], tune, tot["lt_pc"][:C], tot["lt_cp"][:C], tot["prior_p"][:C], tot["L2_p"][:C],
                          scratch, u=u, seed=seed, chain0=chain0, it=it, iter_dev=counter, acc_trace=None if at is None else at[:chunk],
                          delta_trace=None if dtr is None else dtr[:chunk], bump=bump, T=None if self.given else self.now["T"])
        torch.cuda.synchronize()
        assert all(_untouched(v, C) for v in tot.values()) and bool(torch.isnan(scratch[self.fin_scratch_len:]).all())
        self.check_padding(st)
        return tot, scratch, (at, dtr)

    def accept(self, st, tot, u, tune, it=0, counter=None, chunk=0, seed=0, chain0=0):
        from pxmcmc_amd import ops

        C = self.C
        at, dtr = self.traces(chunk)
        ops.pxmala_accept(tot["lt_pc"][:C], tot["lt_cp"][:C], tot["prior_p"][:C], tot["L2_p"][:C], MU, st["logpi"][:C], st["L2"][:C],
                          st["prior"][:C], st["accept"][:C], st["delta"][:C], tune, self.lmda, u=u, seed=seed, chain0=chain0, it=it,
                          iter_dev=counter, acc_trace=None if at is None else at[:chunk], delta_trace=None if dtr is None else dtr[:chunk])
        self.torch.cuda.synchronize()
        self.check_padding(st)
        return at, dtr

    def check_padding(self, st):
        C = self.C
        assert all(_untouched(st[k], C) for k in ("logpi", "L2", "prior", "delta")) and bool((st["accept"][C:] == SENT_I).all())


DATA_KINDS = {"data-f64": (False, False), "data-c128-real-invcov": (True, False), "data-c128-complex-invcov": (True, True)}


@pytest.mark.parametrize("shape", [(133121, 300), (63, 133121)], ids=["n133121-nd300", "n63-nd133121"])
@pytest.mark.parametrize("dkind", list(DATA_KINDS))
@pytest.mark.parametrize("cplx", [False, True], ids=["state-f64", "state-c128"])
def test_tail_against_extended_model(cplx, dkind, shape):
    """all six k_pxmala_tail_partial instantiations, n != n_data (66 slices on one side, 64 on the other): the reverse
    transition sum and the L2 (from their slices) and the stored lt_pc / lt_cp / prior_p / L2_p against the model, the bound
    propagated through -(d/2) S^2; the deferred totals equal the immediate ones bit for bit; ops.logtransition / reduce_l2 /
    reduce_l1 / reduce_vdot at the same shapes against the model, and bit-equal to what the fused tail stores"""
    from pxmcmc_amd import ops

    n, nd = shape
    dcplx, icplx = DATA_KINDS[dkind]
    C = 3
    given = not cplx if dcplx else cplx  # both prox forms on both state types
    itn = _Iteration(n, nd, C, cplx, dcplx, icplx, True, given, seed=500 + n % 1000 + 3 * cplx + 5 * dcplx + 7 * icplx)
    t, delta, lmda = itn.t, itn.delta, itn.lmda
    rng = np.random.default_rng(1)
    st = itn.state(rng.normal(size=C) + 0j, rng.normal(size=C) + 0j, rng.normal(size=C))
    tot, scratch, _ = itn.finish(st, np.full(C, 0.5), tune=0)
    got = {k: v[:C].cpu().numpy() for k, v in tot.items()}
    # deferred totals of the proposal == immediate ones
    assert np.array_equal(_bits(tot["lt_cp"][:C]), _bits(itn.now["lt"][:C])) and np.array_equal(_bits(tot["prior_p"][:C]), _bits(itn.now["prior"][:C]))
    # reverse transition: inputs X1 = X' (as stored), X2 = X, P' (as stored, or formed from T), G'
    er = transition_term_ext(itn.X1, itn.X2, itn.P1, t["G"], delta, lmda, T=itn.T)
    p64 = itn.P1 if given else np.asarray(soft_ext(_ld(itn.X1), itn.T)).astype(itn.X1.dtype)
    e_r = C_BOUND * EPS * trans_scale(itn.X1, itn.X2, p64, t["G"], delta, lmda)
    S_ext, bS = sum_sq_ext(er), sq_sum_bound(er, e_r, n)
    RS, RD = _slices(n), _slices(nd)
    assert RS != RD and max(RS, RD) == 66
    plt = _partial_sums(scratch, C, RS, 2)
    pl2 = _partial_sums(scratch[ops.reduce_scratch_doubles(C):], C, RD, 2)
    rS = float(np.max(_f64abs(plt[:, 0] + 1j * plt[:, 1] - S_ext) / bS))
    L2_ext, bL2 = l2_ext(t["preds"], t["data"], t["invcov"]), l2_sum_bound(t["preds"], t["data"], t["invcov"], nd)
    rL2s = float(np.max(_f64abs(pl2[:, 0] + 1j * pl2[:, 1] - L2_ext) / bL2))
    rlt = float(np.max(_f64abs(_ld(got["lt_pc"]) - logtrans_ext(S_ext, delta)) / logtrans_bound(S_ext, bS, delta)))
    rL2 = float(np.max(_f64abs(_ld(got["L2_p"]) - L2_ext) / bL2))
    # the forward terms: the model of the proposal (as in test_proposal_against_extended_model)
    inp = itn.inp
    P_in = itn.now["P"][:C].cpu().numpy() if given else None
    eXp, _, efr = propose_ext(inp["X"], P_in, inp["G"], inp["W"], itn.T, delta, lmda)
    pf64 = P_in if given else np.asarray(soft_ext(_ld(inp["X"]), itn.T)).astype(inp["X"].dtype)
    S_e = error_scale(inp["X"], pf64, inp["G"], inp["W"], delta, lmda)
    bSf = sq_sum_bound(efr, C_BOUND * EPS * (S_e + trans_scale(inp["X"], itn.X1, pf64, inp["G"], delta, lmda)), n)
    bA = l1_sum_bound(eXp, C_BOUND * EPS * S_e, itn.wts, n)
    rcp = float(np.max(_f64abs(_ld(got["lt_cp"]) - logtrans_ext(sum_sq_ext(efr), delta)) / logtrans_bound(sum_sq_ext(efr), bSf, delta)))
    rpr = float(np.max(_f64abs(_ld(got["prior_p"]) - sum_l1_ext(eXp, itn.wts)) / bA))
    print(f"state c128={cplx} {dkind} n={n} nd={nd}: error / bound: reverse S {rS:.3e} L2 slices {rL2s:.3e} lt_pc {rlt:.3e} L2_p {rL2:.3e} "
          f"lt_cp {rcp:.3e} prior_p {rpr:.3e} (bound 1)")
    assert max(rS, rL2s, rlt, rL2, rcp, rpr) <= 1.0
    if not cplx:
        assert np.all(got["lt_pc"].imag == 0) and np.all(got["lt_cp"].imag == 0)
    if not dcplx:
        assert np.all(got["L2_p"].imag == 0)
    # the separate reductions: the same totals bit for bit, and the model through them
    Pdev = itn.now["Pp"][:C] if given else ops.soft(itn.now["Xp"][:C], itn.now["T"])
    lt_sep = ops.logtransition(itn.now["Xp"][:C], itn.now["X"][:C], Pdev, itn.Gp[:C], itn.now["D"][:C], lmda)
    l2_sep = ops.reduce_l2(itn.preds[:C], itn.data, itn.invcov)
    assert np.array_equal(_bits(lt_sep), _bits(tot["lt_pc"][:C])) and np.array_equal(_bits(l2_sep), _bits(tot["L2_p"][:C]))
    l1_sep = ops.reduce_l1(itn.now["Xp"][:C], itn.wts).cpu().numpy()  # X' exact here: only the sum's own roundings
    x1 = _ld(itn.X1)
    rl1 = float(np.max(_f64abs(_ld(l1_sep) - sum_l1_ext(x1, itn.wts)) / l1_sum_bound(x1, 0.0, itn.wts, n)))
    e64 = t["data"][None, :] - t["preds"]
    b64 = t["invcov"][None, :] * e64
    vd = ops.reduce_vdot(e64, b64).cpu().numpy()
    tv = np.abs(e64) * np.abs(b64)
    rvd = float(np.max(_f64abs(_ld(vd) - np.sum(np.conj(_ld(e64)) * _ld(b64), axis=1)) / ((4 * EPS + nd * EPS) * tv.sum(axis=1))))
    print(f"    separate reductions: reduce_l1 {rl1:.3e} reduce_vdot {rvd:.3e} (bound 1)")
    assert max(rl1, rvd) <= 1.0
    # the state of the chains moved as the flags say (u = 0.5, whatever they are): covered per pattern in the accept tests
    acc = st["accept"][:C].cpu().numpy()
    assert set(acc.tolist()) <= {0, 1}


def _wanted_flags(C):
    """accept / reject alternating within each round of five chains, shifted from round to round"""
    return np.array([((c % 5) + (c // 5)) % 2 == 0 for c in range(C)])


@pytest.mark.parametrize("C", [1, 4, 5, 6, 11, 17])
def test_accept_decisions_state_delta_and_traces(C):
    """pxm_pxmala_finish and pxm_pxmala_accept on the same totals give identical outputs, and both the model's: log u sits a
    relative 1e-9 below (accept) or above (reject) the model's logalpha, alternating within each round of five chains;
    accepted chains take logpi' = -mu prior' - L2', L2', prior', rejected ones keep theirs bit for bit (a NaN logalpha
    rejects); delta: untouched with tune = 0, the model's to 2 ulp with tune = 1, both clamps reached; chunk = 4, it = 3,
    *iter_dev = 3 writes trace row 2 only, with the adapted delta; bump aliased to iter_dev leaves the counter one higher
    after every chain has used the old value (trace row and adaptation exponent)"""
    from pxmcmc_amd import ops

    torch = _t()
    n, nd, it, it_dev, chunk = 63, 5, 3, 3, 4
    rng = np.random.default_rng(40 + C)
    delta = LMDA * (0.2 + 0.25 * rng.random(C))
    delta[0] = LMDA / 2  # accepts: the upper clamp
    if C > 1:
        delta[1] = LMDA * 1e-8  # rejects: the lower clamp
    itn = _Iteration(n, nd, C, True, True, True, True, False, seed=900 + C, delta=delta)
    zero = np.zeros(C)
    # first pass: the totals (they do not depend on the accept state)
    tot, _, _ = itn.finish(itn.state(zero + 0j, zero + 0j, zero), np.full(C, 0.5), tune=0)
    got = {k: v[:C].cpu().numpy() for k, v in tot.items()}
    # ... are the ones the separate kernels give, chain by chain (a slot or role mix-up of the fused totals shows here)
    Pdev = ops.soft(itn.now["Xp"][:C], itn.now["T"])
    assert np.array_equal(_bits(ops.logtransition(itn.now["Xp"][:C], itn.now["X"][:C], Pdev, itn.Gp[:C], itn.now["D"][:C], LMDA)), _bits(tot["lt_pc"][:C]))
    assert np.array_equal(_bits(ops.reduce_l2(itn.preds[:C], itn.data, itn.invcov)), _bits(tot["L2_p"][:C]))
    assert np.array_equal(_bits(itn.now["lt"][:C]), _bits(tot["lt_cp"][:C])) and np.array_equal(_bits(itn.now["prior"][:C]), _bits(tot["prior_p"][:C]))
    assert len(set(got["L2_p"].tolist())) == C and len(set(got["prior_p"].tolist())) == C  # every chain its own totals
    # the state: logpi_c puts the model's logalpha at -target
    want = _wanted_flags(C)
    target = 0.5 + rng.random(C)
    pre = accept_chain_model(got["lt_pc"], got["lt_cp"], got["prior_p"], got["L2_p"], MU, LMDA, zero + 0j, zero + 0j, zero, np.full(C, 0.5), delta, 0, False)
    logpi_c = np.asarray(pre["logalpha"] + target, dtype=float) + 1j * rng.normal(size=C)
    L2_c, prior_c = rng.normal(size=C) + 1j * rng.normal(size=C), np.abs(rng.normal(size=C))
    if C >= 6:
        logpi_c[5] = np.nan + 0.25j  # NaN logalpha: rejects whatever u is
        want[5] = False
    la = accept_chain_model(got["lt_pc"], got["lt_cp"], got["prior_p"], got["L2_p"], MU, LMDA, logpi_c, L2_c, prior_c, np.full(C, 0.5), delta, 0, False)["logalpha"]
    la_f = np.where(np.isnan(la.astype(float)), -1.0, la)
    assert np.all(np.abs(la_f.astype(float) + np.where(np.isnan(la.astype(float)), 1.0, target)) < 1e-9)
    u = np.exp(la_f * np.where(want, 1 + 1e-9, 1 - 1e-9)).astype(float)  # log u < logalpha accepts
    if C >= 6:
        u[5] = 1e-300
    for tune in (1, 0):
        model = accept_chain_model(got["lt_pc"], got["lt_cp"], got["prior_p"], got["L2_p"], MU, LMDA, logpi_c, L2_c, prior_c, u, delta,
                                   it + it_dev, bool(tune), chunk=chunk)
        assert np.array_equal(model["accept"].astype(bool), want) and model["row"] == 2
        sf, sa = itn.state(logpi_c, L2_c, prior_c), itn.state(logpi_c, L2_c, prior_c)
        before = {k: _bits(v) for k, v in sf.items()}
        cnt_f = torch.full((1,), it_dev, dtype=torch.int64, device=itn.dev)
        cnt_a = torch.full((1,), it_dev, dtype=torch.int64, device=itn.dev)
        tot2, _, (atf, dtf) = itn.finish(sf, u, tune, it=it, counter=cnt_f, bump=cnt_f, chunk=chunk)
        ata, dta = itn.accept(sa, tot, u, tune, it=it, counter=cnt_a, chunk=chunk)
        assert int(cnt_f[0]) == it_dev + 1 and int(cnt_a[0]) == it_dev  # bumped once, behind the last reader
        for k in tot:
            assert np.array_equal(_bits(tot2[k]), _bits(tot[k])), k
        for k in sf:  # the two routes: identical
            assert np.array_equal(_bits(sf[k]), _bits(sa[k])), k
        assert np.array_equal(_bits(atf), _bits(ata)) and np.array_equal(_bits(dtf), _bits(dta))
        acc = sf["accept"][:C].cpu().numpy().astype(bool)
        assert np.array_equal(acc, want), (acc, want)
        after = {k: _bits(v) for k, v in sf.items()}
        rej = np.flatnonzero(~want)
        for k in ("logpi", "L2", "prior"):  # rejected: bit for bit, NaN included
            assert np.array_equal(after[k][rej], before[k][rej]), k
        a_ = np.flatnonzero(want)
        assert np.array_equal(after["L2"][a_], _bits(tot["L2_p"])[a_]) and np.array_equal(after["prior"][a_], _bits(tot["prior_p"])[a_])
        lp = sf["logpi"][:C].cpu().numpy()
        lp_err = np.abs(lp[a_] - model["logpi"][a_])
        assert np.all(lp_err <= 2 * EPS * (MU * np.abs(got["prior_p"][a_]) + np.abs(got["L2_p"][a_]))) and np.array_equal(lp[a_].imag, -got["L2_p"][a_].imag)
        d_after = sf["delta"][:C].cpu().numpy()
        if tune:
            ulp = float(np.max(np.abs(_ld(d_after) - model["delta"]) / (EPS * model["delta"])).astype(float))
            print(f"C={C}: delta adaptation, worst distance from the model {ulp:.3f} ulp (bound 2)")
            assert ulp <= 2.0
            assert d_after[0] == LMDA / 2 and (C == 1 or d_after[1] == LMDA * 1e-8)  # the clamps, exactly
            free = np.arange(C) >= 2
            assert np.all(d_after[free] != delta[free])
        else:
            assert np.array_equal(after["delta"], before["delta"])
        at, dtr = atf.cpu().numpy(), dtf.cpu().numpy()
        others = [0, 1, 3, 4]  # (row 4: past the ring)
        assert np.all(at[others] == SENT_I) and np.all(dtr[others] == SENT_F)
        assert np.array_equal(at[2].astype(bool), want) and np.array_equal(dtr[2], d_after)  # the adapted delta


@pytest.mark.parametrize("seed", [7, 2 ** 63 + 11])
def test_metropolis_uniform_stream(seed):
    """with u = None the kernel draws philox_uniform(seed, chain0 + c, it + *iter_dev): with lt_pc.re = log(oracle uniform) x
    (1 -+ 1e-12) and every other term zero, one launch accepts every chain and the other rejects every chain -- a uniform
    shared between chains, or one that ignores chain0 or the device counter, fails"""
    from pxmcmc_amd import ops

    torch = _t()
    C, chain0, it, it_dev = 17, 5, 2, 4
    uo = np.array([philox.uniform(seed, chain0 + c, it + it_dev) for c in range(C)])
    assert len(set(uo.tolist())) == C
    cnt = torch.full((1,), it_dev, dtype=torch.int64, device=ops.device())
    z = np.zeros(C)
    for factor, expect in ((1 - 1e-12, 1), (1 + 1e-12, 0)):
        lt_pc = _padded(np.log(uo) * factor + 0j, torch.complex128)
        tot = dict(lt_pc=lt_pc, lt_cp=_padded(z + 0j, torch.complex128), prior_p=_padded(z), L2_p=_padded(z + 0j, torch.complex128))
        st = dict(logpi=_padded(z + 0j, torch.complex128), L2=_padded(z + 1j, torch.complex128), prior=_padded(z + 3.0), delta=_padded(z + 1e-3),
                  accept=_empty(C, (), torch.int32, fill=SENT_I))
        ops.pxmala_accept(tot["lt_pc"][:C], tot["lt_cp"][:C], tot["prior_p"][:C], tot["L2_p"][:C], MU, st["logpi"][:C], st["L2"][:C],
                          st["prior"][:C], st["accept"][:C], st["delta"][:C], 0, LMDA, u=None, seed=seed, chain0=chain0, it=it, iter_dev=cnt)
        torch.cuda.synchronize()
        acc = st["accept"].cpu().numpy()
        print(f"seed={seed} factor 1{factor - 1:+.0e}: flags {acc[:C].tolist()}")
        assert np.all(acc[:C] == expect) and np.all(acc[C:] == SENT_I)
        assert all(_untouched(st[k], C) for k in ("logpi", "L2", "prior", "delta"))
        assert np.all(st["prior"][:C].cpu().numpy() == (0.0 if expect else 3.0))


# ---- select_copy_many -------------------------------------------------------------------------------------------------------
LENGTHS = [1, 257, 16385, 40000]  # 16385 and 40000: longer than the clamped grid of 64 x 256 words, every thread loops


@pytest.mark.parametrize("npairs", [1, 2, 3, 4])
@pytest.mark.parametrize("C", [1, 6, 17])
def test_select_copy_many(C, npairs):
    """selected chains equal the source, unselected ones keep a NaN-payload fill bit for bit (int64 view), for 1 to 4 pairs of
    mixed float64 / complex128, flags all zero, all one and mixed; a [C] pair has one element per chain"""
    from pxmcmc_amd import ops

    torch = _t()
    rng = np.random.default_rng(C * 10 + npairs)
    dev = ops.device()
    lens = [LENGTHS[(k + C + npairs) % 4] for k in range(npairs)]
    flagsets = [np.zeros(C, dtype=np.int32), np.ones(C, dtype=np.int32), (rng.random(C) < 0.5).astype(np.int32) * 7]
    flagsets[2][0], flagsets[2][-1] = (3, 0) if C > 1 else (3, 3)
    for flags in flagsets:
        pairs, srcs, dsts = [], [], []
        for k, m in enumerate(lens):
            cplx = (k + npairs) % 2 == 1
            words = m * (2 if cplx else 1)
            s64 = torch.from_numpy(rng.integers(-2 ** 62, 2 ** 62, size=(C + 1, words))).to(dev)
            d64 = torch.full((C + 1, words), NAN_BITS, dtype=torch.int64, device=dev)
            view = (lambda t: torch.view_as_complex(t.view(torch.float64).reshape(C + 1, m, 2))) if cplx else (lambda t: t.view(torch.float64))
            s, d = view(s64), view(d64)
            if m == 1 and C > 1:
                s, d = s.reshape(C + 1), d.reshape(C + 1)  # [C]: one element per chain
            pairs.append((s[:C], d[:C]))
            srcs.append(s64)
            dsts.append(d64)
        fl = torch.full((C + 1,), 1, dtype=torch.int32, device=dev)  # (the flag past C is set: the kernel must not look)
        fl[:C] = torch.from_numpy(flags).to(dev)
        ops.select_copy_many(fl[:C], pairs)
        torch.cuda.synchronize()
        for s64, d64 in zip(srcs, dsts):
            got, src = d64.cpu().numpy(), s64.cpu().numpy()
            sel = flags != 0
            assert np.array_equal(got[:C][sel], src[:C][sel]) and np.all(got[:C][~sel] == NAN_BITS) and np.all(got[C] == NAN_BITS)


def test_select_copy_many_refuses_arrays_without_a_chain_axis():
    """a pair whose shape is not [C, ...] for C > 1 raises before any launch (the kernel would copy C x numel words)"""
    from pxmcmc_amd import ops

    torch = _t()
    dev = ops.device()
    flag = torch.ones(3, dtype=torch.int32, device=dev)
    good = (torch.zeros((3, 8), dtype=torch.float64, device=dev), torch.ones((3, 8), dtype=torch.float64, device=dev))
    for shape in ((8,), (4, 8), (1, 3, 8), ()):
        bad = (torch.zeros(shape, dtype=torch.float64, device=dev), torch.ones(shape, dtype=torch.float64, device=dev))
        with pytest.raises(ValueError):
            ops.select_copy_many(flag, [good, bad])
        torch.cuda.synchronize()
        assert bool((bad[1] == 1).all()) and bool((good[1] == 1).all())  # nothing ran
    with pytest.raises(ValueError):
        ops.select_copy_many(flag.to(torch.int64), [good])
    one = torch.ones(1, dtype=torch.int32, device=dev)  # one chain may come without the axis
    a, b = torch.arange(8, dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.float64, device=dev)
    ops.select_copy_many(one, [(a, b)])
    assert bool((a == b).all())


# ---- whole runs: the schedule, the routes of an iteration against each other and against the oracle -------------------------
def _quiet(fn, **kw):
    import warnings

    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(**kw)


def test_pxmala_max_iter_stop_is_flagged():
    """PxMALA(max_iter=...): a run that ends before nsamples were saved says so (`stopped_early`, `nsaved`) instead of
    returning zero rows unmarked (advisor finding, round 4)."""
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMALA, PxMCMCParams
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.transforms import IdentityTransform

    n = 64
    rng = np.random.default_rng(0)
    data = rng.normal(size=n)
    op = ForwardOperator(data, 0.1, "synthesis", IdentityTransform(), Identity(n, n), n)
    T = IdentityTransform()
    reg = L1("synthesis", T.forward, T.forward_adjoint, 1e-3)
    p = PxMCMCParams(lmda=2e-3, delta=1e-3, nsamples=50, nburn=0, ngap=1, verbosity=0)
    s = PxMALA(op, reg, p, max_iter=5, seed=1)
    with contextlib.redirect_stdout(io.StringIO()):
        s.run(start_point=np.zeros(n))
    assert s.niter == 5 and s.stopped_early and 0 <= s.nsaved <= 5
    s2 = PxMALA(op, reg, PxMCMCParams(lmda=2e-3, delta=1e-3, nsamples=3, nburn=0, ngap=1, verbosity=0), seed=1)
    with contextlib.redirect_stdout(io.StringIO()):
        s2.run(start_point=np.zeros(n))
    assert not s2.stopped_early and s2.nsaved == 3


@pytest.mark.parametrize("C", [1, 3, 17])
def test_pxmala_fused_tail_equals_separate_calls(C):
    """pxm_pxmala_finish (deferred totals of the proposal pass + reverse transition sum and L2 in one grid + totals and
    Metropolis test in one workgroup, the iteration counter advanced inside) against the separate calls it replaces
    (pxm_pxmala_propose totals, pxm_reduce_l2, pxm_logtransition, pxm_pxmala_accept, pxm_counter_add): the slices are
    summed by the same bodies and added in the same order, so chains, traces and both transition values are IDENTICAL --
    graph replay and eager stepping, real and complex states, 1 / 3 / 17 chains (17: more chains than waves)."""
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMALA, PxMCMCParams
    from pxmcmc_amd.measurements import Identity, WeakLensing
    from pxmcmc_amd.prior import L1, S2_Wavelets_L1
    from pxmcmc_amd.transforms import IdentityTransform, SphericalWaveletTransform

    rng = np.random.default_rng(5)
    problems = []
    n = 5000
    T = IdentityTransform()
    problems.append((ForwardOperator(rng.normal(size=n), 0.3, "synthesis", T, Identity(n, n), n),
                     L1("synthesis", T.forward, T.forward_adjoint, 2e-3), n, 4e-3, 2e-3))
    L, B, J = 16, 2, 2
    tr = SphericalWaveletTransform(L, B, J, max_chains=C)
    mask = np.ones((L, 2 * L - 1), dtype=int)
    mask[6:9, :] = 0
    wl = WeakLensing(L, mask, ngal=rng.integers(5, 40, size=mask.shape), max_chains=C)
    data = rng.normal(size=int(mask.sum())) + 1j * rng.normal(size=int(mask.sum()))
    op = ForwardOperator(data, 1 / wl.inv_cov, "synthesis", transform=tr, measurement=wl, nparams=tr.ncoefs)
    problems.append((op, S2_Wavelets_L1("synthesis", tr.inverse, tr.inverse_adjoint, 1e-6, L=L, B=B, J_min=J), tr.ncoefs, 1e-6, 2e-6))
    rejected = accepted = 0
    for op, reg, nparams, lmda, delta in problems:
        p = PxMCMCParams(lmda=lmda, delta=delta, nsamples=4, nburn=3, ngap=2, verbosity=0, track=["chain", "logposterior", "L2", "prior"])
        runs = {}
        for fuse in (True, False):
            for graph in (True, False):
                s = PxMALA(op, reg, p, tune_delta=True, nchains=C, seed=11, track_transitions=True, use_graph=graph, max_iter=60)
                s.fuse_tail = fuse
                _quiet(s.run, start_point=np.zeros(nparams))
                assert s.used_graph == graph, s.graph_error
                runs[fuse, graph] = (np.asarray(s.chain), np.asarray(s.acceptance_trace), np.asarray(s.deltas_trace),
                                     np.asarray(s.logPi), np.asarray(s.L2s), np.asarray(s.priors),
                                     np.asarray([t[0] for t in s.transitions_trace]), np.asarray([t[1] for t in s.transitions_trace]))
        ref = runs[False, False]
        accepted += ref[1].sum()
        rejected += ref[1].size - ref[1].sum()
        for key, got in runs.items():
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a, b, err_msg=str(key))
    assert accepted > 0 and rejected > 0  # accepted and rejected proposals in the compared windows


def test_pxmala_fused_tail_equals_separate_calls_at_the_slice_cap():
    """The same identity at a state of 2.2 M elements: every reduction runs with RED_SLICES_MAX = 1024 slices (16 per lane in
    the one-workgroup totals), the size class of BASELINE configs[4] (1.2 M complex coefficients)."""
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMALA, PxMCMCParams
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.transforms import IdentityTransform

    n, C = 2_200_000, 2
    rng = np.random.default_rng(9)
    T = IdentityTransform()
    op = ForwardOperator(rng.normal(size=n), 0.3, "synthesis", T, Identity(n, n), n)
    reg = L1("synthesis", T.forward, T.forward_adjoint, 2e-3)
    p = PxMCMCParams(lmda=4e-3, delta=2e-3, nsamples=2, nburn=2, ngap=1, verbosity=0, track=["logposterior", "L2", "prior"])
    runs = {}
    for fuse in (True, False):
        s = PxMALA(op, reg, p, tune_delta=True, nchains=C, seed=4, track_transitions=True, max_iter=8)
        s.fuse_tail = fuse
        _quiet(s.run, start_point=np.zeros(n))
        runs[fuse] = (np.asarray(s.acceptance_trace), np.asarray(s.deltas_trace), np.asarray(s.logPi), np.asarray(s.L2s),
                      np.asarray(s.priors), np.asarray([t[0] for t in s.transitions_trace]),
                      np.asarray([t[1] for t in s.transitions_trace]), s.X_curr.cpu().numpy() if hasattr(s.X_curr, "cpu") else np.asarray(s.X_curr))
    for a, b in zip(runs[True], runs[False]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("C", [1, 3])
def test_pxmala_plugin_route_matches_numpy_sampler(C):
    """The route of a user-supplied prior (``_iteration_plugin``: the reference's own sequence of calls) against
    oracle.pxmcmc_np.pxmala_run, chain by chain on the sampler's own ``np.random`` stream (per iteration: the normals of
    every chain, then the uniforms of every chain): an analysis-setting L1 on the identity transform is not the stock prox.
    12 iterations, the first 3 burn-in, every later accepted one saved.  The inputs are conditioned on the oracle alone:
    with this seed every chain accepts and rejects, every chain saves, and |log u - logalpha| is at least 0.30 over all
    iterations and chains (C = 1: 1.335; C = 3: 0.309) -- a rounding difference cannot flip a decision."""
    from oracle import pxmcmc_np as ref
    from pxmcmc_amd.forward import ForwardOperator
    from pxmcmc_amd.mcmc import PxMALA, PxMCMCParams
    from pxmcmc_amd.measurements import Identity
    from pxmcmc_amd.prior import L1
    from pxmcmc_amd.transforms import IdentityTransform

    n, lmda, mu, delta0, niter, nburn, seed = 64, 2e-3, 1.0, 1e-3, 12, 3, 2
    rng = np.random.default_rng(0)
    data = rng.normal(size=n)
    X0 = data + rng.normal(size=(C, n)) * 0.1
    # the oracle's runs, on the draws the sampler will make
    np.random.seed(seed)
    nz, un = np.zeros((niter, C, n)), np.zeros((niter, C))
    for i in range(niter):
        for c in range(C):
            nz[i, c] = np.random.randn(n)
        for c in range(C):
            un[i, c] = np.random.rand()
    oT = ref.IdentityTransform()
    oop = ref.ForwardOperator(data, 0.1, "analysis", oT, ref.Identity(n, n), n)
    oreg = ref.L1("analysis", oT.inverse, oT.inverse_adjoint, lmda * mu)
    outs = [ref.pxmala_run(oop, oreg, lmda, delta0, mu, 10 ** 6, nburn, 1, X0[c], lambda i: nz[i, c], lambda i: un[i, c],
                           tune=True, max_iter=niter) for c in range(C)]
    margin = min(float(np.abs(np.log(un[:, c]) - out["logalpha"]).min()) for c, out in enumerate(outs))
    print(f"C={C}: smallest |log u - logalpha| of the oracle's runs {margin:.3f}")
    assert margin >= 1e-6
    for out in outs:
        assert 0 < out["acceptance_trace"].sum() < niter and len(out["chain"]) > 0
    # the sampler
    T = IdentityTransform()
    op = ForwardOperator(data, 0.1, "analysis", T, Identity(n, n), n)
    reg = L1("analysis", T.inverse, T.inverse_adjoint, lmda * mu)
    p = PxMCMCParams(lmda=lmda, delta=delta0, mu=mu, nsamples=niter, nburn=nburn, ngap=1, verbosity=0)
    s = PxMALA(op, reg, p, tune_delta=True, nchains=C, rng="numpy", max_iter=niter)
    np.random.seed(seed)
    _quiet(s.run, start_point=X0 if C > 1 else X0[0])
    assert not s._stock_prox and s._route() == "plugin" and not s.used_graph and s.niter == niter
    acc = np.asarray(s.acceptance_trace).reshape(niter, C)
    deltas = np.asarray(s.deltas_trace).reshape(niter + 1, C)
    chain, nsaved = s.chain.reshape(C, niter, n), np.atleast_1d(s.nsaved)
    for c, out in enumerate(outs):
        assert list(acc[:, c]) == list(out["acceptance_trace"])
        np.testing.assert_allclose(deltas[:, c], out["deltas_trace"], rtol=1e-13)
        assert nsaved[c] == len(out["chain"])
        np.testing.assert_allclose(chain[c, : nsaved[c]], out["chain"], rtol=0, atol=1e-9 * np.abs(out["chain"][0]).max())
