"""The table-free ring stage (csrc/sht_rec.hip): Wigner rows by recursion instead of the ring-table GEMM for the inverse /
inverse_adjoint transforms (pyssht.inverse / inverse_adjoint, pxmcmc/measurements.py:225,237) of few-column plans."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from test_rec_host import (REC_CONFIGS, REC_NC, REC_NO_GEOMETRY, model_cap, model_tol, rec_adjoint_scale, rec_geometry, rec_inputs,
                           rec_stage_model, within)

pytestmark = pytest.mark.gpu


def test_wavefront_transpose_reduce_selftest():
    """reduce16: 16 per-lane values summed over the 64 lanes; every lane of quad q ends with the total of the value id it
    reports (v_permlane32_swap / v_permlane16_swap / DPP network of k_rec_r2e)"""
    from pxmcmc_amd._lib import check, lib

    out = np.zeros(128)
    check(lib.pxm_rec_reduce_selftest(out.ctypes.data_as(C.c_void_p)))
    lanes = np.arange(64)
    ids = out[64:].astype(int)
    assert sorted(set(ids)) == list(range(16)) and all(np.bincount(ids) == 4)
    assert np.array_equal(ids, 8 * ((lanes >> 2) & 1) + 4 * ((lanes >> 3) & 1) + 2 * ((lanes >> 4) & 1) + ((lanes >> 5) & 1))
    expect = np.array([sum(1000.0 * (j + 1) + ln * (j + 1) * 0.5 for ln in range(64)) for j in range(16)])
    np.testing.assert_allclose(out[:64], expect[ids], rtol=1e-15)


@pytest.mark.parametrize("L,spin,nch", [(3, 0, 1), (10, 0, 1), (10, 2, 1), (16, 2, 2), (33, 0, 2), (64, 2, 1), (65, 0, 1), (100, 2, 4),
                                        (130, 0, 1), (130, 2, 2), (144, 2, 1)])
def test_recursion_ring_stage_matches_oracle_and_gemm(monkeypatch, L, spin, nch):
    """inverse and inverse_adjoint through the recursion kernels against the oracle's transforms (1e-11 of the output scale)
    and against the same plan size on the ring-table GEMM; forward / forward_adjoint of the same plan keep their tables"""
    from oracle import ssht
    from pxmcmc_amd import ops

    rng = np.random.default_rng(L * 10 + spin)
    flm = rng.normal(size=(nch, L * L)) + 1j * rng.normal(size=(nch, L * L))
    for el in range(abs(spin)):
        flm[:, el * el:(el + 1) ** 2] = 0
    f = rng.normal(size=(nch, L * (2 * L - 1))) + 1j * rng.normal(size=(nch, L * (2 * L - 1)))
    monkeypatch.setenv("PXM_REC", "1")
    pr = ops.ShtPlan(L, spin, max_chains=nch)
    assert pr.uses_recursion() > 0
    monkeypatch.setenv("PXM_REC", "0")
    pg = ops.ShtPlan(L, spin, max_chains=nch)
    assert pg.uses_recursion() == 0
    inv_r, inv_g = pr.inverse(flm).cpu().numpy(), pg.inverse(flm).cpu().numpy()
    adj_r, adj_g = pr.inverse_adjoint(f).cpu().numpy(), pg.inverse_adjoint(f).cpu().numpy()
    for c in range(nch):
        want = ssht.inverse(flm[c], L, spin).reshape(-1)
        assert np.abs(inv_r[c] - want).max() <= 1e-11 * np.abs(want).max()
        want = ssht.inverse_adjoint(f[c].reshape(L, 2 * L - 1), L, spin)
        assert np.abs(adj_r[c] - want).max() <= 1e-11 * np.abs(want).max()
    assert np.abs(inv_r - inv_g).max() <= 1e-11 * np.abs(inv_g).max()
    assert np.abs(adj_r - adj_g).max() <= 1e-11 * np.abs(adj_g).max()
    # fewer chains than the plan was made for; the other two transforms are untouched
    one = pr.inverse(flm[0]).cpu().numpy()
    assert np.array_equal(one, inv_r[0])
    np.testing.assert_array_equal(pr.forward(f).cpu().numpy(), pg.forward(f).cpu().numpy())


def test_recursion_ring_stage_L512_against_gemm_and_dot_test(monkeypatch):
    """L = 512, spins 0 and 2, one chain (the launches of BASELINE configs[4]): the recursion kernels against the ring-table GEMM
    (whose tables are the long-double recursion rounded to double) and the adjoint dot test between the two new kernels"""
    from pxmcmc_amd import ops

    L = 512
    rng = np.random.default_rng(5)
    for spin in (2, 0):
        flm = rng.normal(size=L * L) + 1j * rng.normal(size=L * L)
        flm[: spin * spin] = 0
        f = rng.normal(size=L * (2 * L - 1)) + 1j * rng.normal(size=L * (2 * L - 1))
        monkeypatch.setenv("PXM_REC", "1")
        pr = ops.ShtPlan(L, spin, max_chains=1)
        assert pr.uses_recursion() > 0
        inv_r, adj_r = pr.inverse(flm).cpu().numpy(), pr.inverse_adjoint(f).cpu().numpy()
        del pr
        monkeypatch.setenv("PXM_REC", "0")
        pg = ops.ShtPlan(L, spin, max_chains=1)
        inv_g, adj_g = pg.inverse(flm).cpu().numpy(), pg.inverse_adjoint(f).cpu().numpy()
        del pg
        ops.tables_trim()
        assert np.abs(inv_r - inv_g).max() <= 2e-11 * np.abs(inv_g).max()
        assert np.abs(adj_r - adj_g).max() <= 2e-11 * np.abs(adj_g).max()
        lhs, rhs = np.vdot(f, inv_r), np.vdot(adj_r, flm)
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


# ---- every (R, NC) instantiation of k_rec_e2r / k_rec_r2e, forced by PXM_REC_R at sizes that take seconds --------------------
# A plan takes R = 2 by itself from L = 385 (spin 0, two chains) / 512 and R = 4 from L = 513 / 683 only: sizes whose ring
# tables are 0.5 - 1 GB.  PXM_REC_R runs the same code objects at L = 130 (three ring blocks, the last with 2 rings, the
# centre one southern, L no multiple of 16: the look-ahead reads the zero padding; R = 2, 4: a wave of two blocks, one nearly
# empty), L = 200 (two blocks per hemisphere: full R = 2 waves; R = 1 with NC = 4 needs more than 48 KiB of LDS) and L = 385
# (R = 4: a wave of four live blocks and one of three; (2, 2), (2, 4), (4, 4) need more than 48 KiB) --
# tests/test_rec_host.py::test_forced_geometry_at_the_gpu_test_shapes holds the layouts.
@contextlib.contextmanager
def _environ(**kv):
    """environment variables set (or, for None, unset) inside the block: a module-scoped fixture has no monkeypatch"""
    def put(values):
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    old = {k: os.environ.get(k) for k in kv}
    try:
        put(kv)
        yield
    finally:
        put(old)


def _rec_env(R):
    """the switches a plan reads when it is made: R = 0 the ring-table GEMM, else the recursion kernels with R forced"""
    return _environ(PXM_REC="1" if R else "0", PXM_REC_R=str(R) if R else None)


def _sht_plan(L, spin, chains, R):
    from pxmcmc_amd import ops

    with _rec_env(R):
        plan = ops.ShtPlan(L, spin, max_chains=chains)
    # (a silent fall-back to the GEMM would make every test below vacuous)
    assert plan.uses_recursion() == (16 * R + REC_NC[spin, chains] if R else 0), (L, spin, chains, R, plan.uses_recursion())
    return plan


class _Shared:
    """plans, inputs and the long-double model of a (L, spin), made once for the module"""

    def __init__(self):
        self.plans, self.ins, self.models = {}, {}, {}

    def plan(self, L, spin, chains, R):
        key = (L, spin, chains, R)
        if key not in self.plans:
            self.plans[key] = _sht_plan(L, spin, chains, R)
        return self.plans[key]

    def inputs(self, L, spin):
        """flm, f (rec_inputs) and the number of dense chains in front of the one-order ones"""
        if (L, spin) not in self.ins:
            nd = max(c for s, c in REC_CONFIGS if s == spin)
            self.ins[L, spin] = rec_inputs(L, spin, nd, seed=1000 * L + spin) + (nd,)
        return self.ins[L, spin]

    def model(self, L, spin):
        if (L, spin) not in self.models:
            flm, f, _ = self.inputs(L, spin)
            self.models[L, spin] = rec_stage_model(L, spin, flm, f)
        return self.models[L, spin]


@pytest.fixture(scope="module")
def shared():
    from pxmcmc_amd import ops

    s = _Shared()
    yield s
    s.plans.clear()
    s.models.clear()
    ops.tables_trim()


@pytest.mark.parametrize("spin,chains", REC_CONFIGS)
@pytest.mark.parametrize("L", [130, 200])
def test_forced_R_inverse_is_bit_identical_across_R(shared, L, spin, chains):
    """k_rec_e2r: a lane's arithmetic (rec_step, the fmac of each column, the rescale check per 16 degrees) does not depend
    on how ring blocks are grouped into waves, and a block's hemisphere (its zeta, its coefficient table) does not depend
    on R either: inverse of a dense input under R = 2 and R = 4 equals R = 1 bit for bit"""
    import torch

    flm = shared.inputs(L, spin)[0][:chains]
    want = shared.plan(L, spin, chains, 1).inverse(flm)
    assert bool(torch.isfinite(torch.view_as_real(want)).all()) and float(want.abs().max()) > 1
    for R in (2, 4):
        assert torch.equal(shared.plan(L, spin, chains, R).inverse(flm), want), R


@pytest.mark.parametrize("spin,chains", REC_CONFIGS)
@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("L", [130, 200])
def test_forced_R_every_instantiation_against_the_model_per_element(shared, L, R, spin, chains):
    """All nine (R, NC) of both kernels through ShtPlan: |got - ref| <= tol scale for EVERY element, ref the long-double
    reference of tests/test_rec_host.py::rec_stage_model, scale the sum of magnitudes behind the element and
    tol = 4 x the CPU model's own max(err / scale) on the same inputs.  Dense Gaussian chains, and one order per chain
    (one_order_ms, spread over the chains of a call and over calls): polar rings and extreme orders are held relative to
    their own magnitude -- the scaled seeds and the REC_BIG rescale.

    Measured on an MI355X, the device's max(|got - ref| / scale) over the model's max(err / scale), bound 4 -- lowest ..
    highest over the nine instantiations:
                           L = 130           L = 200         model's max(err / scale)
      inverse, dense       0.994 .. 1.003    0.998 .. 1.001    1.2e-15 .. 9.7e-15
      inverse, one order   1.006 .. 1.016    1.001 .. 1.002    5.8e-15 .. 1.7e-14
      adjoint, dense       0.987 .. 1.008    0.994 .. 1.014    3.8e-15 .. 1.5e-14
      adjoint, one order   0.976 .. 1.022    0.993 .. 1.032    7.3e-14 .. 4.5e-13   (coherent rings, model_cap)
    The device sits on the model: what both have in common -- the recursion's rows against the long-double ones -- is the
    error, and the order of the sums is a few percent of it.  The first case of an (L, spin) computes the model: 2.6 s
    at (200, spin 2), the slowest of these tests; every other case takes under 0.1 s."""
    flm, f, nd = shared.inputs(L, spin)
    M = shared.model(L, spin)
    plan = shared.plan(L, spin, chains, R)
    orders = np.arange(nd, len(flm))
    families = {"dense": np.arange(chains)[None], "one order": np.resize(orders, (-(-len(orders) // chains), chains))}
    worst = {}
    for op, x in (("inverse", flm), ("inverse_adjoint", f)):
        for family, calls in families.items():
            tol = model_tol(M[op], np.unique(calls), model_cap(L, coherent=(op, family) == ("inverse_adjoint", "one order")))
            r = max(within(getattr(plan, op)(x[c]).cpu().numpy(), M[op], c, tol) for c in calls)
            print(f"REC_RATIO L={L} R={R} NC={REC_NC[spin, chains]} spin={spin} chains={chains} {op} {family}: "
                  f"device/model = {4 * r:.3f} (tol = {tol:.3g})")
            worst[op, family] = 4 * r
    assert all(v <= 4 for v in worst.values()), worst


@pytest.mark.parametrize("spin,chains", [c for c in REC_CONFIGS if c[1] > 1])
@pytest.mark.parametrize("R", [1, 2, 4])
def test_forced_R_partial_batches_L130(shared, R, spin, chains):
    """a plan for `chains` chains called with fewer (NC = 2 and 4; a plan with NC = 1, or spin 0 with one chain, has no
    smaller batch): the chains that run equal the full batch bit for bit, in both kernels, and the columns of the chains
    that were left out are as they were -- the full batch, and `forward` on the same workspace, repeat bit for bit"""
    import torch

    L = 130
    plan = shared.plan(L, spin, chains, R)
    flm, f, _ = shared.inputs(L, spin)
    flm, f = flm[:chains], f[:chains]
    inv, adj, fwd = plan.inverse(flm), plan.inverse_adjoint(f), plan.forward(f)
    for c in range(1, chains):
        assert torch.equal(plan.inverse(flm[:c]), inv[:c]), c
        assert torch.equal(plan.inverse_adjoint(f[:c]), adj[:c]), c
    assert torch.equal(plan.inverse(flm[0]), inv[0]) and torch.equal(plan.inverse_adjoint(f[0]), adj[0])
    assert torch.equal(plan.forward(f), fwd) and torch.equal(plan.inverse(flm), inv) and torch.equal(plan.inverse_adjoint(f), adj)


@pytest.fixture(scope="module", params=[2, 0], ids=["spin2", "spin0"])
def big(request):
    """L = 385, one spin at a time: the plans of every (chains, R) that has a geometry, the ring-table GEMM plan where
    R = 1 has none, dense inputs and the scale of inverse_adjoint"""
    from pxmcmc_amd import ops

    L, spin = 385, request.param
    rng = np.random.default_rng(385 + spin)
    configs = [c for s, c in REC_CONFIGS if s == spin]
    flm = rng.normal(size=(max(configs), L * L)) + 1j * rng.normal(size=(max(configs), L * L))
    flm[:, : spin * spin] = 0
    f = rng.normal(size=(max(configs), L * (2 * L - 1))) + 1j * rng.normal(size=(max(configs), L * (2 * L - 1)))
    plans = {}
    for chains in configs:
        for R in (1, 2, 4):
            if (L, R, REC_NC[spin, chains]) in REC_NO_GEOMETRY:
                with _rec_env(R):
                    assert rec_geometry(L, spin, chains) is None
                R = 0
            plans[chains, R] = _sht_plan(L, spin, chains, R)
    yield L, spin, configs, plans, flm, f, rec_adjoint_scale(L, spin, f)
    plans.clear()
    ops.tables_trim()


def test_forced_R_L385_inverse_is_bit_identical_across_R(big):
    """as at L = 130 and 200, with full R = 4 waves (four live blocks, and three); where R = 1 has no geometry (NC = 4:
    175 KiB of LDS) R = 4 is compared with R = 2"""
    import torch

    L, spin, configs, plans, flm, f, scale = big
    for chains in configs:
        want = plans[chains, 1 if (chains, 1) in plans else 2].inverse(flm[:chains])
        assert bool(torch.isfinite(torch.view_as_real(want)).all()) and float(want.abs().max()) > 1
        for R in (2, 4):
            assert torch.equal(plans[chains, R].inverse(flm[:chains]), want), (chains, R)


def test_forced_R_L385_inverse_adjoint_and_dot_test(big, shared):
    """k_rec_r2e under R = 2 and 4 against the R = 1 plan (NC <= 2) or the ring-table GEMM plan (NC = 4), per element
    within tol scale: scale as in rec_stage_model, tol the one of the dense chains at L = 200 grown by (385 / 200)^1.5 (the
    el^1.5 law of tests/test_rec_host.py); and the dot test between the two kernels, <f, inverse(flm)> =
    <inverse_adjoint(f), flm> per chain to 1e-12.

    Measured on an MI355X, max |diff| / (tol scale), bound 1: 0.001 against R = 1 (the same rows, another order of the
    sums), 0.24 .. 0.56 against the GEMM (rows of the recursion against the long-double rows); tol 0.9e-13 .. 1.6e-13.
    The fixture of a spin (nine plans at spin 2, and the ring tables of the GEMM plan) takes 4.5 s."""
    L, spin, configs, plans, flm, f, scale = big
    M200 = shared.model(200, spin)["inverse_adjoint"]
    worst = {}
    for chains in configs:
        tol = model_tol(M200, np.arange(chains), model_cap(200)) * (L / 200) ** 1.5
        want = plans[chains, 1 if (chains, 1) in plans else 0].inverse_adjoint(f[:chains]).cpu().numpy()
        for R in (2, 4):
            got = plans[chains, R].inverse_adjoint(f[:chains]).cpu().numpy()
            d, s = np.abs(got - want), scale[:chains]
            assert not d[s == 0].any()
            worst[chains, R] = (d[s > 0] / (tol * s[s > 0])).max()
            print(f"REC_RATIO L={L} R={R} NC={REC_NC[spin, chains]} spin={spin} chains={chains} inverse_adjoint vs "
                  f"{'R=1' if (chains, 1) in plans else 'GEMM'}: |diff| / (tol scale) = {worst[chains, R]:.3f} (tol = {tol:.3g})")
            inv = plans[chains, R].inverse(flm[:chains]).cpu().numpy()
            for c in range(chains):
                lhs, rhs = np.vdot(f[c], inv[c]), np.vdot(got[c], flm[c])
                assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (chains, R, c, abs(lhs - rhs) / abs(lhs))
    assert all(v <= 1 for v in worst.values()), worst


@pytest.mark.parametrize("chains", [1, 2, 4])
def test_forced_R_weak_lensing_stage_L130(chains):
    """the spin-2 stage of wl_forward / wl_adjoint of a WavPlan under R = 2 and 4 (NC = chains): the second operand of
    k_rec_pack, the per-el scale of both kernels and the narrow ring array, against the same plan on the ring-table GEMM"""
    import torch

    from pxmcmc_amd import ops

    L, B, J = 130, 2.0, 2
    rng = np.random.default_rng(130 + chains)
    theta = np.pi * (2 * np.arange(L) + 1) / (2 * L - 1)
    mask = np.ones((L, 2 * L - 1), dtype=bool)
    mask[np.abs(90 - np.degrees(theta)) < 8, :] = False
    mask[:, 30:47] = False
    nd = int(mask.sum())
    pix2data = torch.from_numpy(np.where(mask.reshape(-1), np.cumsum(mask.reshape(-1)) - 1, -1).astype(np.int32))
    weight = rng.uniform(0.5, 2.0, size=nd)

    def run(R, X, gam):
        with _rec_env(R):
            plan = ops.WavPlan(L, B, J, max_chains=chains)
            plan.wl_attach(pix2data, weight, nd)
        assert plan.wl_uses_recursion() == (16 * R + chains if R else 0), (R, plan.wl_uses_recursion())
        if X is None:
            X = rng.normal(size=(chains, plan.ncoefs)) + 1j * rng.normal(size=(chains, plan.ncoefs))
            gam = rng.normal(size=(chains, nd)) + 1j * rng.normal(size=(chains, nd))
        return X, gam, plan.wl_forward(X).cpu().numpy(), plan.wl_adjoint(gam).cpu().numpy()

    X, gam, fwd0, adj0 = run(0, None, None)
    for R in (2, 4):
        _, _, fwd, adj = run(R, X, gam)
        for c in range(chains):
            assert np.abs(fwd[c] - fwd0[c]).max() <= 1e-11 * np.abs(fwd0[c]).max(), (R, c)
            assert np.abs(adj[c] - adj0[c]).max() <= 1e-11 * np.abs(adj0[c]).max(), (R, c)
    ops.tables_trim()
