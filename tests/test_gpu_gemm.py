"""Every ring-GEMM kernel variant (csrc/sht_gemm.hip: k_sht_gemm, k_sht_gemm_pk) on a GEMM-only plan (ops.GemmPlan: ring tables,
one workspace, one task list -- no DFT stage, no update kernels), element by element against the long-double model of
tests/test_gemm_host.py on the tables read back from the device, at the smallest shapes at which each instantiation exists
(CASES there; the host tests assert what each shape is there for and that together they launch all 26 instantiations).

Per case: every element a correct launch writes is inside gamma_N S of the model (no sampling, a bound per element: a row of
small magnitude is held to ITS magnitude); every other double of the result arrays and of the scratch row block keeps the
sentinel bit for bit; impulse operands pick the table entries out one at a time, each held to a dozen u of itself; the
counter advances once per call.  Then the launch orders, the bit-identity statements and the device tables entry by entry.

Measured device / bound figures (MI355X; printed per case as ``GEMM-RATIO``: max |dev - model| / (u S), beside the same figure
for a float64 numpy evaluation of the model): DESIGN.md, "Error model and tests of the ring GEMM".
"""
import numpy as np
import pytest
from test_gemm_host import (AFFINE, CASE_IDS, CASES, F, LD, SENTINEL, U, case, case_report, gamma, gemm_ld, host_dense, launched_columns,
                            make_inputs, products, table_blocks, worst_ratio)

pytestmark = pytest.mark.gpu

REF_PRODUCTS = 64 << 20  # long-double products of the model of one run (~0.4 s)


def _plan(cs, monkeypatch):
    from pxmcmc_amd import ops

    plan = case_report(cs, monkeypatch, ops.GemmPlan)
    return plan, dict(layout=plan.layout, sides=plan.sides, tasks=plan.tasks, tables=plan.tables)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).cuda()


def _load(plan, rep, inp):
    """the inputs into the workspace; the result arrays and the scratch row block as the sentinel"""
    import torch

    lay = rep["layout"]
    for s, d in zip(rep["sides"], inp):
        for key, off in (("x", "off_x"), ("x2", "off_x2"), ("ks", "off_ks"), ("rs", "off_rs"), ("hd", "off_hd")):
            if d[key] is not None:
                plan.write(s[off], _dev(d[key]))
        plan.write(s["off_y"], torch.full((s["n_y"],), SENTINEL, dtype=torch.float64, device="cuda"))
    plan.write(lay["off_scratch"], torch.full((lay["scratch_doubles"],), SENTINEL, dtype=torch.float64, device="cuda"))


def _fetch(plan, rep):
    """(result array per side, scratch row block) as numpy"""
    ys = [plan.read(s["off_y"], s["n_y"]).cpu().numpy().reshape(2 * s["yL"] - 1, s["yRp"], s["yn"]) for s in rep["sides"]]
    return ys, plan.read(rep["layout"]["off_scratch"], rep["layout"]["scratch_doubles"]).cpu().numpy()


def _tables(plan, rep, cs):
    blocks = [table_blocks(rep["tables"][i], plan.table(i).cpu().numpy(), s["kind"]) for i, s in enumerate(cs["sides"])]
    poles = [plan.pole(i).cpu().numpy() if s["kind"] == "gram_split0" else None for i, s in enumerate(cs["sides"])]
    return blocks, poles


def _check(cs, rep, ys, scratch, res, smask, what):
    """every written element inside its bound, everything else the sentinel; -> max |dev - model| / (u S)"""
    worst = 0.0
    for i, (y, r) in enumerate(zip(ys, res)):
        assert r["mask"].any()
        assert (y[~r["mask"]] == SENTINEL).all(), (cs["id"], what, "side", i, "wrote outside the model's mask",
                                                    int((y[~r["mask"]] != SENTINEL).sum()))
        assert (y[r["mask"]] != SENTINEL).all(), (cs["id"], what, "side", i, "left a row of the model's mask unwritten",
                                                   int((y[r["mask"]] == SENTINEL).sum()))
        q, ok = worst_ratio(y, r)
        if not ok:
            err = np.abs(y.astype(LD) - r["val"].astype(LD)).astype(float)
            bad = np.argwhere(r["mask"] & (err > gamma(r["N"]) * r["S"] + r["N"] * 2.0 ** -1074))
            raise AssertionError((cs["id"], what, "side", i, "elements outside gamma_N S", len(bad), "first (m_idx, row, col)",
                                  bad[0].tolist(), "ratio", q))
        worst = max(worst, q)
    assert (scratch[~smask] == SENTINEL).all() and (scratch[smask] != SENTINEL).all(), (cs["id"], what, "scratch row block")
    return worst


@pytest.mark.parametrize("cs", CASES, ids=CASE_IDS)
def test_case_against_the_model(cs, monkeypatch):
    plan, rep = _plan(cs, monkeypatch)
    blocks, poles = _tables(plan, rep, cs)
    affine = AFFINE if cs["affine"] else None
    dev_worst, f64_worst, calls = 0.0, 0.0, 0
    for n, C in enumerate(cs["Cs"]):
        assert products(rep, C) <= REF_PRODUCTS
        inp = make_inputs(rep, 100 + n)
        _load(plan, rep, inp)
        plan.run(C, affine=affine, bump=cs["affine"])
        calls += int(cs["affine"])
        assert plan.counter() == calls  # once per call, whatever the number of column groups
        ys, scratch = _fetch(plan, rep)
        res, smask = gemm_ld(rep, blocks, inp, C, affine, poles)
        dev_worst = max(dev_worst, _check(cs, rep, ys, scratch, res, smask, f"dense C={C}"))
        f64, _ = gemm_ld(rep, blocks, inp, C, affine, poles, dtype=np.float64)
        f64_worst = max([f64_worst] + [worst_ratio(f["val"], r)[0] for f, r in zip(f64, res)])
    print(f"GEMM-RATIO {cs['id']} device={dev_worst:.2f} float64={f64_worst:.2f}  [u S]")


@pytest.mark.parametrize("cs", CASES, ids=CASE_IDS)
def test_impulses_pick_single_entries(cs, monkeypatch):
    """operand row k of column c is 1 where k = c + columns * j, run after run until every k has been hit: each output is ONE
    table entry times its scales (plus, in a pole task, one entry of the pole term) and is held to (1 + 10) u of its own
    magnitude -- a wrong k or row mapping shows on entries far too small to show in a dense sum"""
    plan, rep = _plan(cs, monkeypatch)
    blocks, poles = _tables(plan, rep, cs)
    C = cs["Cs"][0]
    ncols = launched_columns(rep, C)
    worst, hit = 0.0, 0
    for j in range(-(-max(s["xRp"] for s in rep["sides"]) // ncols)):
        inp = make_inputs(rep, 200 + j, impulse=(j, ncols))
        _load(plan, rep, inp)
        plan.run(C)
        ys, scratch = _fetch(plan, rep)
        res, smask = gemm_ld(rep, blocks, inp, C, None, poles)
        assert max(int(r["N"].max()) for r in res) <= 12  # one product (two with a pole term) and the fixed roundings
        worst = max(worst, _check(cs, rep, ys, scratch, res, smask, f"impulses j={j}"))
        hit += sum(int((y[r["mask"]] != 0).sum()) for y, r in zip(ys, res))
    assert hit > 0
    print(f"GEMM-RATIO {cs['id']} impulses device={worst:.2f}  [u |entry|]")


# ---- launch order ------------------------------------------------------------------------------------------------------------------------
def test_launch_orders_give_the_same_bits(monkeypatch):
    """PXM_GEMM_ORDER = plain, bins, xcd (padding entries: asserted on the host) run the same tasks: bit-identical results"""
    got = {}
    for cs in (c for c in CASES if c["order"]):
        plan, rep = _plan(cs, monkeypatch)
        inp = make_inputs(rep, 300)
        _load(plan, rep, inp)
        plan.run(cs["Cs"][0], affine=AFFINE)
        got[cs["order"]] = (_fetch(plan, rep)[0][0], rep["tasks"])
    assert (got["xcd"][1][:, F["n_rt"]] == 0).any()
    assert not np.array_equal(got["plain"][1], got["xcd"][1][:len(got["plain"][1])])
    for order in ("bins", "xcd"):
        assert np.array_equal(got["plain"][0].view(np.int64), got[order][0].view(np.int64)), order


# ---- bit identity ------------------------------------------------------------------------------------------------------------------------
def _run_chain_columns(cs, monkeypatch, x, ks, C, other=None, affine=None, x2=None, hd=None):
    """runs the case's list with the columns of ``x`` [planes, rows, 2 k] as its first chains (``other``: what the remaining
    columns hold) -> the result columns of those chains"""
    plan, rep = _plan(cs, monkeypatch)
    inp = make_inputs(rep, 999 if other is None else other)
    n = x.shape[2]
    inp[0]["x"][:, :, :n] = x
    if x2 is not None:
        inp[0]["x2"][:, :, :n] = x2
    if hd is not None:
        inp[0]["hd"][:] = hd
    if ks is not None:
        inp[0]["ks"][:] = ks
    _load(plan, rep, inp)
    plan.run(C, affine=affine)
    return _fetch(plan, rep)[0][0][:, :, :n].copy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def test_a_chain_does_not_depend_on_the_batch(monkeypatch):
    """One list (the inverse at L = 64 with a k scale) and one operand for chains 0 .. 3: their results are the same bits
    whatever the other columns hold, for every C <= capacity, and between 8-, 16- and 24-slot plans -- the summation order
    of an element does not depend on the column tile it sits in (CT = 1 and 2, the group at col0 = 32)."""
    rng = np.random.default_rng(5)
    L, Rp = 64, 64
    x, ks = rng.standard_normal((2 * L - 1, Rp, 8)), rng.standard_normal(Rp)
    cases = {slots: case(f"bits-{slots}", [dict(kind="inv", bl=L, ks=True)], slots=slots) for slots in (8, 16, 24)}
    ref = _run_chain_columns(cases[8], monkeypatch, x, ks, 8)
    assert not (ref == SENTINEL).any()
    assert _same_bits(ref, _run_chain_columns(cases[8], monkeypatch, x, ks, 8, other=1))
    for slots in (8, 16, 24):
        for C in sorted({4, 5, 8, 9, slots}):
            if C <= slots:
                assert _same_bits(ref, _run_chain_columns(cases[slots], monkeypatch, x, ks, C, other=C)), (slots, C)


def test_affine_chains_do_not_depend_on_the_batch(monkeypatch):
    """the same for the Gram step with its epilogue at L = 64: chains 0 .. 2 of C = 3, 5 and 16 on 8- and 16-slot plans.  The
    parity halves (gram_split) keep their bits throughout.  With the pole tasks (gram_split0) they keep them for every C and
    whatever the other columns hold on ONE plan; between an 8- and a 16-slot plan only the planes of the orders m != 0 do: the
    pole sum deals its rows over 512 / (8 CT) row groups, so the order-0 plane is summed in another order with CT = 2 (each
    order inside the bound of the case tests; the difference is printed)."""
    rng = np.random.default_rng(6)
    L, Rp = 64, 64
    x, x2, hd = rng.standard_normal((2 * L - 1, Rp, 6)), rng.standard_normal((2 * L - 1, Rp, 6)), rng.standard_normal((2 * L - 1, Rp, 2))
    for kind in ("gram_split", "gram_split0"):
        sides = [dict(kind=kind, bl=L, two=True, hd=True)]
        ref = {slots: _run_chain_columns(case(f"bits-{kind}-{slots}", sides, slots=slots), monkeypatch, x, None, 3, affine=AFFINE, x2=x2, hd=hd)
               for slots in (8, 16)}
        assert (ref[8] != SENTINEL).any()
        for slots, C in ((8, 5), (8, 8), (16, 5), (16, 16)):
            got = _run_chain_columns(case(f"bits-{kind}-{slots}", sides, slots=slots), monkeypatch, x, None, C, other=C, affine=AFFINE, x2=x2, hd=hd)
            assert _same_bits(ref[slots], got), (kind, slots, C)
        rest = np.arange(2 * L - 1) != L - 1
        assert _same_bits(ref[8][rest], ref[16][rest]), kind
        if kind == "gram_split":
            assert _same_bits(ref[8], ref[16])
        else:
            d = np.abs(ref[8][L - 1] - ref[16][L - 1])
            print(f"GEMM-POLE-ORDER order-0 plane, 8 against 16 slots: max difference {d.max() / (U * np.abs(ref[8][L - 1]).max()):.2f} u of the largest entry")


def test_packed_against_unpacked(monkeypatch):
    """The packed kernels (one tile of 16 / pk slabs, two chunks of look-ahead) and the unpacked ones run the same body: an
    element's accumulator takes the 16-k chunks of its task in ascending order, four k-steps per MFMA, the operand staged as
    (x + x2) * ks in both.  Neither the look-ahead depth nor the column a value sits in enters the arithmetic, so the results
    are the same bits: asserted for the forward (row scale, mask) and the forward adjoint (k scale) at L = 112, pk = 2 and 4."""
    rng = np.random.default_rng(7)
    L, Rp = 112, 112
    n = 2 * L - 1
    for kind, extra in (("fwd", dict(rs=True, rows=(5, L - 3))), ("fwd_adj", dict(ks=True))):
        for pk in (2, 4):
            x = rng.standard_normal((n, Rp, pk))
            sc = rng.standard_normal(Rp)
            out = []
            for cs in (case("unpacked", [dict(kind=kind, bl=L, **extra)], slots=pk // 2),
                       case("packed", [dict(kind=kind, bl=L, **extra)], slots=pk // 2, pk=pk)):
                plan, rep = _plan(cs, monkeypatch)
                inp = make_inputs(rep, 400)
                inp[0]["x"][:, :, :pk] = x
                inp[0]["rs" if kind == "fwd" else "ks"][:] = sc
                _load(plan, rep, inp)
                plan.run(pk // 2)
                out.append(_fetch(plan, rep)[0][0][:, :, :pk].copy())
            assert _same_bits(*out), (kind, pk, float(np.abs(out[0] - out[1]).max()))


# ---- the tables themselves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,spin", [(40, 0), (40, 2), (64, 0), (64, 2)])
def test_device_tables_entry_by_entry(L, spin, monkeypatch):
    """k_build_fwd and k_build_gram (plain double loops over the L rings) against long-double evaluations from the host B and the
    quadrature matrix: |dev - ref| <= gamma_(L + 2) S per entry, S the sum of the absolute products (+ u |ref| for the host
    forward table, which is the long-double sum rounded once).  The inverse tables are the host B bit for bit."""
    from oracle import ssht

    Rp = -(-L // 16) * 16
    Q = ssht._quadrature_gram(L)
    sc = 2 * np.pi / (2 * L - 1)
    blocks = {}
    for kind in ("inv", "fwd", "inv_adj", "fwd_adj", "gram"):
        plan, rep = _plan(case("tables", [dict(kind=kind, bl=L)], spin=spin), monkeypatch)
        blocks[kind] = table_blocks(rep["tables"][0], plan.table(0).cpu().numpy(), kind)
    worst = {"fwd": 0.0, "gram": 0.0}
    for m in (range(L) if spin == 0 else range(-(L - 1), L)):
        B, A = host_dense(L, spin, m)[:L, :L], host_dense(L, spin, m, fwd=True)[:L, :L]  # (A: the long-double sum, rounded once)
        kb = max(abs(m), abs(spin)) // 16 * 16
        inv, fwd, gram = blocks["inv"][m, -1], blocks["fwd"][m, -1], blocks["gram"][m, -1]
        assert np.array_equal(inv[:L, kb:L], B[:, kb:]) and not inv[:, L:].any() and not inv[L:, kb:].any()
        assert np.array_equal(blocks["inv_adj"][m, -1][kb:, :], inv[:, kb:].T)
        assert np.array_equal(blocks["fwd_adj"][m, -1][:, kb:], fwd[kb:, :].T)
        Sf = sc * (np.abs(B).T @ np.abs(Q[+1 if (m + spin) % 2 == 0 else -1])) * (1 + 1e-9)
        err = np.abs(fwd[kb:L, :L] - A[kb:])
        assert (err <= gamma(L + 2) * Sf[kb:] + U * np.abs(A[kb:])).all(), ("fwd", m, float((err / (U * Sf[kb:] + 1e-300)).max()))
        assert not fwd[kb:, L:].any() and not fwd[L:, :].any()
        worst["fwd"] = max(worst["fwd"], float((err / (U * Sf[kb:] + 1e-300)).max()))
        G = B.T.astype(LD) @ B.astype(LD)
        Sg = (np.abs(B).T @ np.abs(B)) * (1 + 1e-9)
        err = np.abs((gram[kb:L, kb:L].astype(LD) - G[kb:, kb:]).astype(float))
        assert (err <= gamma(L) * Sg[kb:, kb:] + L * 2.0 ** -1074).all(), ("gram", m, float((err / (U * Sg[kb:, kb:] + 1e-300)).max()))
        assert not gram[kb:, L:].any() and not gram[L:, kb:].any()
        worst["gram"] = max(worst["gram"], float((err / (U * Sg[kb:, kb:] + 1e-300)).max()))
    print(f"GEMM-TABLE-RATIO L={L} spin={spin} fwd={worst['fwd']:.2f} gram={worst['gram']:.2f}  [u S]")


def test_split_gram_tables_hold_the_dense_doubles(monkeypatch):
    """gram_split / gram_split0 at L = 64 against the dense Gram table, bit for bit: the halves [2 i + p][2 j + p], the orders
    kept dense, the parity-permuted order 0; the pole column against B^0[theta = pi] of the host"""
    L, Rp = 64, 64
    tabs = {}
    for kind in ("gram", "gram_split", "gram_split0"):
        plan, rep = _plan(case("tables", [dict(kind=kind, bl=L, two=True)]), monkeypatch)
        tabs[kind] = table_blocks(rep["tables"][0], plan.table(0).cpu().numpy(), kind)
        if kind == "gram_split0":
            pole = plan.pole(0).cpu().numpy()
    B0 = host_dense(L, 0, 0)
    assert np.array_equal(pole, np.r_[B0[L - 1, 0::2], B0[L - 1, 1::2]])
    perm = np.r_[np.arange(0, Rp, 2), np.arange(1, Rp, 2)]
    halves = 0
    for kind in ("gram_split", "gram_split0"):
        for (m, par), blk in tabs[kind].items():
            dense = tabs["gram"][m, -1]
            want = dense[np.ix_(perm, perm)] if par == 2 else dense if par < 0 else dense[par::2, par::2]
            if kind == "gram_split0" and m == 0 and par in (0, 1):
                want = dense[par::2, par::2]
            # (a half starts at a tile boundary of its own, below the dense block's: what it stores there lies below the
            # order, l < m, and is zero)
            stored, both = ~np.isnan(blk), ~np.isnan(blk) & ~np.isnan(want)
            assert both.any() and np.array_equal(blk[both], want[both]) and not blk[stored & ~both].any(), (kind, m, par)
            halves += par in (0, 1)
    assert halves > 4
