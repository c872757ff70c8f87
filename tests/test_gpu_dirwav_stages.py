"""The orientation stages on the GPU, one at a time, against long-double statements on the tables the library exports
("Error model and tests of the orientation stages"): the gamma stage of csrc/dirwav.hip in both directions and
every instantiation, the harmonic split and merge of csrc/harm_stage.hip through the stage hook of DirWavPlan and through
HarmWavPlan's operators, the operators as the composition of their stages, the inner SHTs against ShtPlan, and the
isolation of chains and of calls.  Every run is C = 3 chains on a plan of 4, with the workspace and the outputs NaN-filled
first: whatever a launch must not write is still NaN afterwards."""
import ctypes
import functools

import numpy as np
import pytest

from test_dirwav_stages_host import (NS, SHAPES, Stages, _cplx, cmul_ld, gamma_back_ld, gamma_fwd_ld, merge_ld, worst_ratio)

pytestmark = pytest.mark.gpu

CMAX, C = 4, 3
CASES = [(L, B, J, N) for (L, B, J) in SHAPES for N in NS if N <= L] + [(16, 2.0, 1, 16)]
SOME = [(L, B, J, N) for (L, B, J) in SHAPES for N in (2, 5, 12)]  # n = +-1, the even n and the odd n up to 11
# gamma is the last stage of the operators that end in coefficients and the first of those that start from them
GAMMA_FWD = {0: "analysis", 1: "synthesis_adjoint"}  # norm -> operator
GAMMA_BACK = {0: "analysis_adjoint", 1: "synthesis"}


@functools.lru_cache(maxsize=None)
def _plan(L, B, J_min, N, cmax=CMAX):
    from pxmcmc_amd import ops

    return ops.DirWavPlan(L, B, J_min, N, max_chains=cmax)


@functools.lru_cache(maxsize=None)
def _stages(L, B, J_min, N):
    return Stages(L, B, J_min, N)


@functools.lru_cache(maxsize=None)
def _sht(bl, spin):
    from pxmcmc_amd import ops

    return ops.ShtPlan(bl, spin, max_chains=CMAX)


def _nan(*shape):
    import torch

    return torch.full(shape, complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.complex128).cuda()


def _padded(a, n):
    """[C, n] values in a NaN-filled [CMAX, n] device buffer"""
    out = _nan(CMAX, n)
    out[: a.shape[0]] = _dev(a)
    return out


def _regions(lay, what):
    """[(offset, elements)] of the chains c < C of ``what``: 'flm', 'harm' or 'pix' operands"""
    if what == "flm":
        return [(lay["flm"][0], C * (lay["flm"][1] // lay["max_chains"]))]
    key = "a" if what == "harm" else "g"
    return [(it[key + "_off"], C * it[key + "_n"]) for it in lay["items"]]


def _assert_only_written(ws, lay, *what):
    """the workspace read-out ``ws`` is NaN everywhere but in the regions named by ``what``, which are finite"""
    live = np.zeros(lay["size"], dtype=bool)
    for w in what:
        for off, n in _regions(lay, w):
            assert not live[off : off + n].any(), "operands overlap"
            live[off : off + n] = True
    assert np.isfinite(ws[live].view(float)).all(), "an entry the stage must write is not finite"
    assert np.isnan(ws[~live].real).all() and np.isnan(ws[~live].imag).all(), "a write outside the stage's operands"


def _check_layout(plan, S):
    lay = plan.layout()
    assert [(it["block"], it["n"], it["bl"]) for it in lay["items"]] == S.items
    assert [b["coef_off"] for b in lay["blocks"]] == list(S.coef_off[:-1]) and plan.ncoefs == S.ncoefs
    assert [(b["npix"], b["nplanes"]) for b in lay["blocks"]] == list(zip(S.npix, S.nplanes))
    assert lay["max_chains"] == CMAX and lay["flm"] == (0, CMAX * S.L * S.L) and lay["harm"] == CMAX * S.L * S.L
    end = lay["harm"]
    for key in ("a", "g"):  # the operands follow one another, CMAX chains each, and fill the workspace
        for it in lay["items"]:
            assert it[key + "_off"] == end and it[key + "_n"] == (it["bl"] ** 2 if key == "a" else it["bl"] * (2 * it["bl"] - 1))
            end += CMAX * it[key + "_n"]
    assert end == lay["size"] and lay["pix"] == lay["items"][0]["g_off"]
    # the uploaded g-offset table: per block and orientation the item's pixel operand, -1 for a skipped pair
    want = []
    for b, blk in enumerate(lay["blocks"]):
        assert blk["goff_row"] == b * S.N and blk["nn"] == (S.N if b else 1)
        row = [-1] * S.N
        for d, k in S.block_items(b):
            row[k] = lay["items"][d]["g_off"] - lay["pix"]
        want += row
    assert lay["goff"] == want
    return lay


def _put(plan, lay, key, arrs):
    for it, a in zip(lay["items"], arrs):
        plan.write(it[key + "_off"], _dev(a))


def _get(ws, it, key):
    n = it[key + "_n"]
    return ws[it[key + "_off"] : it[key + "_off"] + C * n].reshape(C, n)


# ---- the gamma stage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B,J_min,N", CASES)
def test_gamma_stage_matches_long_double(L, B, J_min, N):
    """k_dw_gamma_fwd<NK> / k_dw_gamma_back<NK> alone, norm 0 and 1: every element within gamma(N + 2) sc sum_k (|ph_r g_r| +
    |ph_i g_i|) (the imaginary part: the cross terms) of the long-double sum over the exported phases -- a product pair
    and a subtraction per term, N - 1 additions and the scale, with or without fma contraction; sc = 1 / (2N - 1) as the
    kernel forms it in float64.  The back direction sums 2N - 1 terms, for which the rigorous count is 2N + 1: the
    gamma(N + 2) asserted there too is the tighter bound the stage is held to, met with room by rounding errors that do not
    all line up (worst measured ratio 0.68, at N = 2), but not a worst-case bound -- a miss by the back direction alone, just
    above 1 after a change of seeds or shapes, is to be read against gamma(2N + 1) before a kernel is suspected.  The
    scaling block and N = 1 are copies.  Chain 3 of the output, the skipped pairs (which
    have no slot: nothing but the items' operands may be written) and the rest of the workspace stay NaN."""
    plan, S = _plan(L, B, J_min, N), _stages(L, B, J_min, N)
    lay = _check_layout(plan, S)
    rng = np.random.default_rng(1000 * L + 10 * N + J_min)
    pix = [_cplx(rng, C, it["g_n"]) for it in lay["items"]]
    X0 = _cplx(rng, C, S.ncoefs)
    worst = {}
    for norm in (0, 1):
        # forward: the items' pixel operands -> X
        plan.write(0, _nan(lay["size"]))
        _put(plan, lay, "g", pix)
        X = plan.run_stage(GAMMA_FWD[norm], 3, _nan(CMAX, S.ncoefs), C).cpu().numpy()
        assert np.isnan(X[C:].real).all() and np.isnan(X[C:].imag).all()
        ws = plan.read().cpu().numpy()
        _assert_only_written(ws, lay, "pix")
        for it, a in zip(lay["items"], pix):
            assert np.array_equal(_get(ws, it, "g"), a)  # (the input is left as it was)
        r = 0.0
        for b in range(len(S.bls)):
            G, got, sc = S.stack(b, dict(enumerate(pix))), S.planes(b, X[:C]), S.scale(b, norm)
            if S.nplanes[b] == 1:
                assert sc == 1.0 and np.array_equal(got[0], G[0]), ("copy", b)
            else:
                r = np.maximum(r, worst_ratio(got, *gamma_fwd_ld(S.ph, G, sc), N + 2))
        worst[f"fwd{norm}"] = float(r)
        # back: X -> the items' pixel operands
        plan.write(0, _nan(lay["size"]))
        Xin = _padded(X0, S.ncoefs)
        plan.run_stage(GAMMA_BACK[norm], 0, Xin, C)
        assert np.array_equal(Xin[:C].cpu().numpy(), X0)
        ws = plan.read().cpu().numpy()
        _assert_only_written(ws, lay, "pix")
        r = 0.0
        for b in range(len(S.bls)):
            W, sc = S.planes(b, X0), S.scale(b, norm)
            ref = None if S.nplanes[b] == 1 else gamma_back_ld(S.ph, W, sc)
            for d, k in S.block_items(b):
                got = _get(ws, lay["items"][d], "g")
                if ref is None:
                    assert np.array_equal(got, W[0]), ("copy", b)
                else:
                    r = np.maximum(r, worst_ratio(got, *(v[k] for v in ref), N + 2))
        worst[f"back{norm}"] = float(r)
    print(f"DW-RATIO gamma L={L} B={B} J_min={J_min} N={N} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- the harmonic split and merge -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B,J_min,N", CASES)
def test_split_merge_stage_matches_long_double(L, B, J_min, N):
    """k_dw_split / k_dw_merge through the stage hook, with both weight tables and their conjugates: the split within
    gamma(2) (|w_r f_r| + |w_i f_i|) (a product pair and a subtraction), the merge within gamma(t + 1) of the magnitude sum
    over its t contributing items; nothing but chains c < C of the items' harmonic operands (split) or of flm (merge) is
    written"""
    plan, S = _plan(L, B, J_min, N), _stages(L, B, J_min, N)
    lay = _check_layout(plan, S)
    rng = np.random.default_rng(2000 * L + 10 * N + J_min)
    f = _cplx(rng, C, L * L)
    harm = [_cplx(rng, C, it["a_n"]) for it in lay["items"]]
    worst = {}
    for op, which, cj in (("analysis", 0, 0), ("synthesis_adjoint", 1, 1)):
        plan.write(0, _nan(lay["size"]))
        plan.write(lay["flm"][0], _dev(f))
        plan.run_stage(op, 1, None, C)
        ws = plan.read().cpu().numpy()
        _assert_only_written(ws, lay, "flm", "harm")
        assert np.array_equal(ws[: C * L * L].reshape(C, L * L), f)
        r = 0.0
        for it, w in zip(lay["items"], S.weights(which, cj)):
            r = np.maximum(r, worst_ratio(_get(ws, it, "a"), *cmul_ld(w[None, :], f[:, : w.size]), 2))
        worst["split_" + op] = float(r)
    for op, which, cj in (("analysis_adjoint", 0, 1), ("synthesis", 1, 0)):
        plan.write(0, _nan(lay["size"]))
        _put(plan, lay, "a", harm)
        plan.run_stage(op, 2, None, C)
        ws = plan.read().cpu().numpy()
        _assert_only_written(ws, lay, "flm", "harm")
        for it, a in zip(lay["items"], harm):
            assert np.array_equal(_get(ws, it, "a"), a)
        *ref, t = merge_ld(S.weights(which, cj), harm, L)
        worst["merge_" + op] = worst_ratio(ws[: C * L * L].reshape(C, L * L), *ref, t[None, :] + 1)
    print(f"DW-RATIO split-merge L={L} B={B} J_min={J_min} N={N} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


HW_CASES = [(L, B, J, N, 0) for (L, B, J) in SHAPES for N in (1, 2, 5, 12)] + [(16, 2.0, 1, 1, 2), (13, 1.5, 1, 1, -3)]


@pytest.mark.parametrize("L,B,J_min,N,spin", HW_CASES)
def test_harmwav_operators_match_long_double(L, B, J_min, N, spin):
    """HarmWavPlan's four operators are the same two kernels on coefficient vectors (cstride = ncoefs): the same bounds
    against the exported harmonic rows, C = 3 chains of NaN-filled [4, .] outputs.  With a spin the rows l < |s| are zero:
    those entries must be exact zeros (a zero magnitude sum admits no error)."""
    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import check, lib

    plan = ops.HarmWavPlan(L, B, J_min, N, spin=spin, max_chains=CMAX)
    wa, ws, rows = ops.harm_weights(L, B, J_min, N, spin, True)
    el = np.repeat(np.arange(L), 2 * np.arange(L) + 1)
    bls = [int(r[2]) for r in rows]
    off = np.concatenate([[0], np.cumsum([bl * bl for bl in bls])]).astype(int)
    assert plan.ncoefs == off[-1]
    wa = [wa[d][el[: bl * bl]] for d, bl in enumerate(bls)]
    ws = [ws[d][el[: bl * bl]] for d, bl in enumerate(bls)]
    rng = np.random.default_rng(3000 * L + 10 * N + spin)
    f, X = _cplx(rng, C, L * L), _cplx(rng, C, plan.ncoefs)
    vp = ctypes.c_void_p

    def run(name, arg, n_out):
        src, out = _padded(arg, arg.shape[1]), _nan(CMAX, n_out)
        check(getattr(lib, "pxm_hwav_" + name)(plan._h, vp(src.data_ptr()), vp(out.data_ptr()), C, None))
        out = out.cpu().numpy()
        assert np.isnan(out[C:].real).all() and np.isnan(out[C:].imag).all(), name
        return out[:C]

    worst = {}
    for name, w in (("analysis", wa), ("synthesis_adjoint", [np.conj(v) for v in ws])):
        got = run(name, f, plan.ncoefs)
        worst[name] = max(worst_ratio(got[:, off[d] : off[d + 1]], *cmul_ld(w[d][None, :], f[:, : w[d].size]), 2) for d in range(len(bls)))
    for name, w in (("synthesis", ws), ("analysis_adjoint", [np.conj(v) for v in wa])):
        *ref, t = merge_ld(w, [X[:, off[d] : off[d + 1]] for d in range(len(bls))], L)
        worst[name] = worst_ratio(run(name, X, L * L), *ref, t[None, :] + 1)
    print(f"DW-RATIO harmwav L={L} B={B} J_min={J_min} N={N} spin={spin} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- composition ----------------------------------------------------------------------------------------------------------
def _operator_inputs(plan, rng):
    X, f = _cplx(rng, C, plan.ncoefs), _cplx(rng, C, plan.npix)
    return {"analysis": (f, plan.ncoefs), "analysis_adjoint": (X, plan.npix), "synthesis": (X, plan.npix),
            "synthesis_adjoint": (f, plan.ncoefs)}


@pytest.mark.parametrize("L,B,J_min,N", CASES)
def test_operators_equal_their_stages(L, B, J_min, N):
    """each operator and its four stages run one by one through the hook give the same bits; chain 3 of the output stays NaN"""
    import torch

    plan = _plan(L, B, J_min, N)
    lay = plan.layout()
    rng = np.random.default_rng(4000 * L + 10 * N + J_min)
    for name, (arg, n_out) in _operator_inputs(plan, rng).items():
        whole = getattr(plan, name)(arg).clone()
        plan.write(0, _nan(lay["size"]))
        src, out = _padded(arg, arg.shape[1]), _nan(CMAX, n_out)
        plan.run_stage(name, 0, src, C)
        plan.run_stage(name, 1, None, C)
        plan.run_stage(name, 2, None, C)
        plan.run_stage(name, 3, out, C)
        assert torch.isfinite(torch.view_as_real(whole)).all()
        assert torch.equal(out[:C], whole), name
        assert torch.isnan(torch.view_as_real(out[C:])).all(), name


SHT_STAGE = {"analysis": (2, "inverse", "a"), "analysis_adjoint": (1, "inverse_adjoint", "g"), "synthesis": (1, "forward", "g"),
             "synthesis_adjoint": (2, "forward_adjoint", "a")}  # operator -> (stage, ShtPlan method, the operand it reads)


@pytest.mark.parametrize("L,B,J_min,N", SOME)
def test_inner_sht_stage_equals_shtplan(L, B, J_min, N):
    """the SHT stage of every item, for the four operators, gives the bits of ops.ShtPlan(bl, -n, max_chains) on the same
    operand: the inner transforms are the plans that have their own models"""
    plan = _plan(L, B, J_min, N)
    lay = plan.layout()
    rng = np.random.default_rng(5000 * L + 10 * N + J_min)
    for name, (stage, method, src) in SHT_STAGE.items():
        dst = "g" if src == "a" else "a"
        ins = [_cplx(rng, C, it[src + "_n"]) for it in lay["items"]]
        plan.write(0, _nan(lay["size"]))
        _put(plan, lay, src, ins)
        plan.run_stage(name, stage, None, C)
        ws = plan.read().cpu().numpy()
        for it, a in zip(lay["items"], ins):
            want = getattr(_sht(it["bl"], -it["n"]), method)(a).cpu().numpy()
            assert np.array_equal(_get(ws, it, dst), want), (name, it["block"], it["n"])


# ---- isolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B,J_min,N", SOME + [(16, 2.0, 1, 1), (16, 2.0, 1, 16)])
def test_chains_and_calls_are_isolated(L, B, J_min, N):
    """for the four operators: every chain of a batch of 3 equals the chain run alone on a plan of one chain, and a call on
    a workspace NaN-filled through ``write`` gives the bits of the call on the fresh plan, every element finite"""
    import torch

    from pxmcmc_amd import ops

    fresh = ops.DirWavPlan(L, B, J_min, N, max_chains=CMAX)
    one = _plan(L, B, J_min, N, 1)
    size = fresh.layout()["size"]
    rng = np.random.default_rng(6000 * L + 10 * N + J_min)
    ins = _operator_inputs(fresh, rng)
    first = {name: getattr(fresh, name)(arg).clone() for name, (arg, _) in ins.items()}
    for name, (arg, _) in ins.items():
        assert torch.isfinite(torch.view_as_real(first[name])).all(), name
        fresh.write(0, _nan(size))
        assert torch.equal(getattr(fresh, name)(arg), first[name]), ("stale workspace", name)
        for c in range(C):
            assert torch.equal(getattr(one, name)(arg[c]), first[name][c]), ("chain alone", name, c)
