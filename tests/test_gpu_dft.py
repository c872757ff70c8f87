"""Every phi-DFT unit on a DFT-only plan (ops.DftPlan: no ring tables), element by element against the long-double model of
tests/test_dft_host.py, at the smallest ring lengths at which each kernel instantiation exists (CASES there).

Tolerance, the rule of test_gpu_rec.py: the float64 model of the algorithm (bluestein64 at the unit's transform length M)
measures what the arithmetic costs, max |model - dft_ld| / (eps ||ring||_2) over the rows compared, itself capped at
MODEL_CAP; the device may be 4 x that per element, relative to the 2-norm of ITS ring -- the factor covers another order
of the sums (eight points per lane, the first stage folded into the tables, the exact-length body's Rader / prime-factor
route in place of Bluestein), nothing else.

Measured device / model error ratios (MI355X, max over the cases of a unit, both directions; printed per case as
``DFT-RATIO``): see DESIGN.md, "phi-DFT units against the model".
"""
import numpy as np
import pytest
from test_dft_host import (CASES, CLD, EPS, MODEL_CAP, case_id, dense, dft_ld, expected_geometry, impulse_spectrum, model_M,
                           model_ratio, root_table)

pytestmark = pytest.mark.gpu

ENV_KEYS = ("PXM_DFT_NO_W", "PXM_DFT_PFA")
REF_PRODUCTS = 16 << 20  # long-double products of the dense reference per direction (~0.3 s): rows = REF_PRODUCTS / n^2 <= 64
ONE_PER_UNIT = [c for c in CASES if c[1:] in ((5, {}), (35, {}), (67, {}), (129, {}), (256, {}), (257, {}))] + [
    ("radix2", 9, {"PXM_DFT_NO_W": "1"}), ("radix2", 513, {})]


def _plan(monkeypatch, case, max_chains):
    """a DFT-only plan created under the case's environment (read at creation only)"""
    from pxmcmc_amd import ops

    _, L, env = case
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = expected_geometry(L, env)
    assert ops.dft_geometry(L) == want
    plan = ops.DftPlan(L, max_chains)
    for k in env:
        monkeypatch.delenv(k)
    return plan, want


def _chains(case):
    """(max_chains, batch sizes): 5 (Cp = 8) with 1, 3 and 5 chains; at L = 1024 (270 MB of rings) 2 chains only"""
    return (2, (2,)) if case[1] == 1024 else (5, (1, 3, 5))


def _cpu(t):
    return t.cpu().numpy()


def _bits(a, b):
    import torch

    return torch.equal(torch.view_as_real(a), torch.view_as_real(b))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _impulse_positions(L, C):
    """p[c, t] = (7 t + 13 c) mod n: over rings and chains every p occurs for L >= 5"""
    n = 2 * L - 1
    return (7 * np.arange(L)[None, :] + 13 * np.arange(C)[:, None]) % n


def _impulses(L, C):
    n, p = 2 * L - 1, _impulse_positions(L, C)
    f = np.zeros((C, L, n), dtype=complex)
    f[np.arange(C)[:, None], np.arange(L)[None, :], p] = 1.0
    return f


def _sample_rows(L, C, rings_per_set, n):
    """(t, c) rows of the dense comparison: ring 0, ring L - 1, the rings on either side of the ring-set boundaries (all of
    them where the budget REF_PRODUCTS allows, else the first, the last and an even spread), every live chain slot.  The
    rings in between are covered by the impulses."""
    budget = max(2 * C, 4, min(64, REF_PRODUCTS // (n * n)))
    rings = {0, L - 1}
    bounds = list(range(rings_per_set, L, rings_per_set)) if rings_per_set > 1 else list(range(1, L))
    room = max(0, (budget - 2) // 2)
    if len(bounds) > room:
        pick = np.unique(np.linspace(0, len(bounds) - 1, room).round().astype(int)) if room else []
        bounds = [bounds[i] for i in pick]
    for b in bounds:
        rings |= {b - 1, b}
    rings = sorted(rings)
    rows = [(t, i % C) for i, t in enumerate(rings)]
    rows += [(rings[-1 - (c % len(rings))], c) for c in range(C) if c not in {r[1] for r in rows}]
    return rows


@pytest.fixture(scope="module")
def impulse_model():
    """max over the n unit impulses of the model's error / eps, per (n, M, direction): computed once.  (n = 2047: over every
    fourth impulse -- a maximum over fewer rows, so never a wider bound; over all of them it is pinned in test_dft_host.)"""
    cache = {}

    def ratio(n, M, sign):
        if (n, M, sign) not in cache:
            p = np.arange(0, n, 4 if n > 1100 else 1)
            x = np.zeros((len(p), n))
            x[np.arange(len(p)), p] = 1.0
            cache[n, M, sign] = model_ratio(x, M, sign, ref=impulse_spectrum(n, p, sign))
            assert cache[n, M, sign] <= MODEL_CAP
        return cache[n, M, sign]

    return ratio


def _order_index(L):
    """DFT bin of the order stored at index i of the public ring axis: m = i - (L - 1), bin m mod n"""
    return np.arange(-(L - 1), L) % (2 * L - 1)


def _row_ratio(got, ref, norm):
    """max over the elements of each row of |got - ref| / (eps ||row||_2), then over rows"""
    err = np.abs(got.astype(CLD) - ref).astype(float).max(axis=-1)
    return float((err / (EPS * norm)).max())


# ---- checks 1-3: impulses (closed form) and dense rings against dft_ld, both directions, every batch size ----------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_unit_against_the_model(case, monkeypatch, impulse_model):
    unit, L, _ = case
    n, M, bins = 2 * L - 1, model_M(case), _order_index(L)
    Cmax, Cs = _chains(case)
    plan, geom = _plan(monkeypatch, case, Cmax)
    rings_per_set = geom[2] if geom[0] == "pair" else 1
    f_imp, p = _impulses(L, Cmax), _impulse_positions(L, Cmax)
    fd, gd = dense(1000 + L, Cmax, L, n), dense(2000 + L, Cmax, L, n)
    # impulses: rings[c, t, m] = exp(-i m phi_p), pixels of a unit order q - (L - 1) at ring t: exp(+i m phi_p)
    m_of = np.arange(-(L - 1), L)
    want_r = [root_table(n)[(p[c][:, None] * m_of[None, :]) % n] for c in range(Cmax)]
    want_p = [np.conj(root_table(n))[((p[c] - (L - 1))[:, None] * np.arange(n)[None, :]) % n] for c in range(Cmax)]
    tol_imp = {s: 4 * impulse_model(n, M, s) for s in (-1, +1)}
    worst = {}
    for C in Cs:
        got_r, got_p = _cpu(plan.rings(f_imp[:C])), _cpu(plan.pixels(f_imp[:C]))  # (f_imp as rings: a unit order per ring)
        for c in range(C):
            for name, got, want, s in (("rings", got_r[c], want_r[c], -1), ("pixels", got_p[c], want_p[c], +1)):
                r = _row_ratio(got, want, 1.0)
                worst[name, "imp"] = max(worst.get((name, "imp"), 0.0), r / (tol_imp[s] / 4) if tol_imp[s] else 0.0)
                assert r <= tol_imp[s], (case_id(case), name, "impulses", C, c, r, tol_imp[s])
        # dense: sampled rows against the long-double DFT
        rows = _sample_rows(L, C, rings_per_set, n)
        ts, cs = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        assert {0, L - 1} <= set(ts.tolist()) and set(cs.tolist()) == set(range(C))
        got_r, got_p = _cpu(plan.rings(fd[:C])), _cpu(plan.pixels(gd[:C]))
        x_r = fd[cs, ts]
        x_p = np.zeros((len(rows), n), dtype=complex)
        x_p[:, bins] = gd[cs, ts]  # the rings of a row in bin order
        for name, x, got, s in (("rings", x_r, got_r[cs, ts], -1), ("pixels", x_p, got_p[cs, ts], +1)):
            full = dft_ld(x, s)  # in bin order
            ref = full[:, bins] if name == "rings" else full
            mr = model_ratio(x, M, s, ref=full)
            assert 0 < mr <= MODEL_CAP or n == 1, (mr, MODEL_CAP)
            r = _row_ratio(got, ref, np.linalg.norm(x, axis=-1))
            worst[name, "dense"] = max(worst.get((name, "dense"), 0.0), r / mr if mr else 0.0)
            assert r <= 4 * mr, (case_id(case), name, "dense", C, r, mr)
    assert plan.status() == 0
    print(f"DFT-RATIO {case_id(case)} unit={unit} n={n} M={M} device/model: " + " ".join(
        f"{k[0]}-{k[1]}={v:.2f}" for k, v in sorted(worst.items())))


# ---- check 2b: rings 2^40 apart in scale -- the bound is per ring ----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rings_of_different_scale_do_not_meet(case, monkeypatch):
    """Neighbouring rings (and chains) 2^40 apart: every ring stays within the bound relative to ITS OWN norm, and -- a
    power of two commutes with every rounding short of under- and overflow -- equals the unscaled result times its factor
    bit for bit.  A value leaking from a large ring into a small one at the 1e-13 level of the large one fails both."""
    import torch

    unit, L, _ = case
    n, M, bins = 2 * L - 1, model_M(case), _order_index(L)
    Cmax, Cs = _chains(case)
    C = Cs[-1]
    plan, geom = _plan(monkeypatch, case, Cmax)
    scale = 2.0 ** (40 * ((np.arange(L)[None, :] + np.arange(C)[:, None]) % 2))[:, :, None]
    fd = dense(3000 + L, C, L, n)
    sc = torch.from_numpy(scale).cuda()
    for fn in (plan.rings, plan.pixels):
        plain, scaled = fn(fd), fn(fd * scale)
        assert _bits(scaled, plain * sc), (case_id(case), fn.__name__)
    rows = _sample_rows(L, C, geom[2] if geom[0] == "pair" else 1, n)[:16]
    ts, cs = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    x = (fd * scale)[cs, ts]
    got = _cpu(plan.rings(fd * scale))[cs, ts]
    ref = dft_ld(x)
    mr = model_ratio(x, M, ref=ref)
    assert mr <= MODEL_CAP
    assert _row_ratio(got, ref[:, bins], np.linalg.norm(x, axis=-1)) <= 4 * mr


# ---- checks 4, 5: the batch shape and the padding never show in a live value -----------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_batch_shape_and_padding_leave_the_bits_alone(case, monkeypatch):
    """Chain c has the same bits in a batch of 1, 3 or 5 and alone in a one-chain plan (the quad unit's one-chain kernels
    and the half-filled pair, the radix-2 unit's partial groups, the pair unit's second chain group with one live chain).
    rings_raw: the live values do not depend on what the ring array held; for every ring t < L ALL padding columns
    c >= C come out exactly zero (the pair, quad and exact-length kernels skip chain groups without a live chain and let the
    last live group zero the rest of its 128-byte lines; the radix-2 kernel transforms zeros for them); the padding rows
    t >= L are never written.  pixels_raw: padding rows and columns of the ring array are never part of a live value."""
    import torch

    from pxmcmc_amd import ops

    _, L, _ = case
    n = 2 * L - 1
    Cmax, Cs = _chains(case)
    plan, _ = _plan(monkeypatch, case, Cmax)
    one, _ = _plan(monkeypatch, case, 1)
    assert isinstance(plan, ops.DftPlan) and (plan.Rp, plan.Cp) == (-(-L // 16) * 16, 8)
    f = torch.from_numpy(dense(4000 + L, Cmax, L, n)).cuda()
    g = torch.from_numpy(dense(5000 + L, Cmax, L, n)).cuda()
    gen = torch.Generator().manual_seed(L)
    junk = torch.view_as_complex(torch.rand(n, plan.Rp, plan.Cp, 2, dtype=torch.float64, generator=gen) + 0.5).cuda()
    ref_r = [one.rings(f[c:c + 1])[0] for c in range(Cmax)]
    ref_p = [one.pixels(g[c:c + 1])[0] for c in range(Cmax)]
    for C in Cs:
        got_r, got_p = plan.rings(f[:C]), plan.pixels(g[:C])
        for c in range(C):
            assert _bits(got_r[c], ref_r[c]) and _bits(got_p[c], ref_p[c]), (case_id(case), C, c)
        # rings_raw into zeros and into finite O(1) garbage
        G0, G1 = plan.rings_raw(f[:C], plan.ring_array()), plan.rings_raw(f[:C], junk.clone())
        assert _bits(G0[:, :L, :C].contiguous(), G1[:, :L, :C].contiguous())
        assert _bits(G0[:, :L, :C].permute(2, 1, 0).contiguous(), got_r)
        for G, fill in ((G0, None), (G1, junk)):
            assert bool((torch.view_as_real(G[:, :L, C:]) == 0).all()), (case_id(case), C)
            if plan.Rp > L:
                rest = G[:, L:, :].contiguous()
                assert _bits(rest, torch.zeros_like(rest) if fill is None else fill[:, L:, :].contiguous())
        # pixels_raw: live rings in a clean array and in one whose padding rows and columns hold garbage
        raw0, raw1 = plan.ring_array(), junk.clone()
        live = g[:C].permute(2, 1, 0)
        raw0[:, :L, :C] = live
        raw1[:, :L, :C] = live
        p0, p1 = plan.pixels_raw(raw0, C), plan.pixels_raw(raw1, C)
        assert _bits(p0, p1) and _bits(p0, got_p), (case_id(case), C)
    assert plan.status() == 0 and one.status() == 0


# ---- nine chains: Cp = 16, two 128-byte halves per (m, ring) line ----------------------------------------------------------------------
@pytest.mark.parametrize("case", ONE_PER_UNIT, ids=case_id)
def test_nine_chains(case, monkeypatch, impulse_model):
    import torch

    unit, L, _ = case
    n, M, bins, C = 2 * L - 1, model_M(case), _order_index(L), 9
    plan, geom = _plan(monkeypatch, case, C)
    one, _ = _plan(monkeypatch, case, 1)
    assert plan.Cp == 16
    f_imp, p, m_of = _impulses(L, C), _impulse_positions(L, C), np.arange(-(L - 1), L)
    got_r, got_p = _cpu(plan.rings(f_imp)), _cpu(plan.pixels(f_imp))
    for c in range(C):
        want_r = root_table(n)[(p[c][:, None] * m_of[None, :]) % n]
        want_p = np.conj(root_table(n))[((p[c] - (L - 1))[:, None] * np.arange(n)[None, :]) % n]
        assert _row_ratio(got_r[c], want_r, 1.0) <= 4 * impulse_model(n, M, -1), (case_id(case), c)
        assert _row_ratio(got_p[c], want_p, 1.0) <= 4 * impulse_model(n, M, +1), (case_id(case), c)
    fd = torch.from_numpy(dense(6000 + L, C, L, n)).cuda()
    got_r, got_p = plan.rings(fd), plan.pixels(fd)
    for c in range(C):
        assert _bits(got_r[c], one.rings(fd[c:c + 1])[0]) and _bits(got_p[c], one.pixels(fd[c:c + 1])[0]), (case_id(case), c)
    rows = _sample_rows(L, C, geom[2] if geom[0] == "pair" else 1, n)[-18:]
    ts, cs = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    x = _cpu(fd)[cs, ts]
    ref = dft_ld(x)
    mr = model_ratio(x, M, ref=ref)
    assert _row_ratio(_cpu(got_r)[cs, ts], ref[:, bins], np.linalg.norm(x, axis=-1)) <= 4 * mr
    assert plan.status() == 0


# ---- check 6: round trip and adjointness, one case per unit ----------------------------------------------------------------------------
def round_trip_taus(case, f, g):
    """(tau_f, tau_i) of test_round_trip_and_dot: 4 eps x the model's measured ratio per direction, on the first rings of
    chain 0 of the image f and of the rings g (both [C, L, 2L-1]); shared with tests/test_gpu_dft_px.py"""
    L = case[1]
    n, M, bins = 2 * L - 1, model_M(case), _order_index(L)
    k = min(L, 8)  # rows that measure the model's ratio: the first rings of chain 0
    xg = np.zeros((k, n), dtype=complex)
    xg[:, bins] = g[0, :k]
    return 4 * EPS * model_ratio(f[0, :k], M, -1), 4 * EPS * model_ratio(xg, M, +1)


@pytest.mark.parametrize("case", ONE_PER_UNIT, ids=case_id)
def test_round_trip_and_dot(case, monkeypatch):
    """pixels(rings(f)) = n f and <rings(f), g> = <f, pixels(g)>.  Bounds from check 3: with tau = 4 ratio eps per
    direction, the rings of a ring are off by at most tau_f ||f||_2 each, which the n-term sum back turns into at most
    n tau_f ||f||_2, and the way back adds tau_i ||rings||_2 = tau_i sqrt(n) ||f||_2: n (tau_f + tau_i) ||f||_2 bounds both.
    The dot products differ by at most sum over rings of tau_f ||f||_2 ||g||_1 + tau_i ||g||_2 ||f||_1."""
    unit, L, _ = case
    n, C = 2 * L - 1, 3
    plan, _ = _plan(monkeypatch, case, 5)
    f, g = dense(7000 + L, C, L, n), dense(8000 + L, C, L, n)
    tau_f, tau_i = round_trip_taus(case, f, g)
    rings = plan.rings(f)
    back = _cpu(plan.pixels(rings))
    nf = np.linalg.norm(f, axis=-1)
    err = np.abs(back.astype(CLD) - n * f.astype(CLD)).astype(float).max(axis=-1)
    assert (err <= n * (tau_f + tau_i) * nf).all(), (case_id(case), (err / (n * nf * EPS)).max())
    lhs = np.sum(np.conj(g.astype(CLD)) * _cpu(rings).astype(CLD))
    rhs = np.sum(np.conj(_cpu(plan.pixels(g)).astype(CLD)) * f.astype(CLD))
    slack = np.sum(tau_f * nf * np.abs(g).sum(axis=-1) + tau_i * np.linalg.norm(g, axis=-1) * np.abs(f).sum(axis=-1))
    assert abs(complex(lhs - rhs)) <= slack, (case_id(case), abs(complex(lhs - rhs)), slack)
    assert plan.status() == 0
