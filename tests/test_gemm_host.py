"""The model the ring-GEMM kernels (csrc/sht_gemm.hip) are held to, and what can be said about it without a GPU.

``gemm_ld`` evaluates, for the task list a GEMM-only plan reports (ops.gemm_plan_geometry / ops.GemmPlan: launch order,
row0, n_rt, k range, masks -- never an offset), the expression the kernel comments state,

    y = sign1^(slab & 1) rs[row] E( sum_k T[row][k] ks[k] (x[k] + x2[k]) + 1/2 b_own[row] sum_r b_other[r] (x + x2)_other[r] ),

E the identity or the complex product w (ns acc - hd[row]) per chain, in long double, with the mask of what a correct
launch writes, the same expression S with every term replaced by its absolute value and the number N of roundings on the
longest path to each element.  A device result is held to |dev - model| <= gamma_N S, gamma_N = N u / (1 - N u),
u = 2^-53: the bound of a dot product in any summation order, with or without FMA ("Error model and tests of
the ring GEMM", has the count).  Terms that are exactly zero round nothing, so N counts the non-zero operand rows of a
column: an impulse operand is held to a dozen u of the one product it selects.

The tests here pin the de-tiler to a tiler written from the layout comment, the model to the oracle's transforms, the bound
to float64 evaluations of every case, and the list geometry every GPU case of tests/test_gpu_gemm.py is there for.
"""
import itertools

import numpy as np
import pytest

LD = np.longdouble
U = 2.0 ** -53
SENTINEL = -6.02214076e123  # finite; no result of these inputs has its bits
ROUNDINGS_EXTRA = 10  # second-operand add, k scale, pole: two factors and its add, ns, data term, complex product (2), row scale
KINDS = ("inv", "fwd", "inv_adj", "fwd_adj", "gram", "gram_split", "gram_split0")
ROWS_EL = {"fwd", "inv_adj", "gram", "gram_split", "gram_split0"}  # kinds whose rows are degrees
K_EL = {"inv", "fwd_adj", "gram", "gram_split", "gram_split0"}  # kinds whose contraction runs over degrees
F = {name: i for i, name in enumerate(("m_unit", "row0", "n_rt", "k_beg", "k_end", "pole_n", "nslab", "side", "par", "row_lo",
                                        "row_hi", "row_lo1", "row_hi1", "sign1", "side_b", "m"))}


def _ops():
    from pxmcmc_amd import ops

    return ops


# ---- the tiled layout (top of csrc/sht_gemm.hip) ---------------------------------------------------------------------------------------
def tile(D, n, row_beg, k_beg):
    """[n, n] matrix -> its tiles, written from the layout comment: for every tile of 16 rows the contraction index runs in
    chunks of 8; one chunk is [lane 64][2], double h of lane l = D[16 rt + (l & 15)][8 kk2 + 4 h + (l >> 4)] (from row_beg, k_beg)"""
    out = []
    for rt in range((n - row_beg) // 16):
        for kk2 in range((n - k_beg) // 8):
            for lane in range(64):
                for h in range(2):
                    out.append(D[row_beg + 16 * rt + (lane & 15), k_beg + 8 * kk2 + 4 * h + (lane >> 4)])
    return np.array(out, dtype=float)


def tile_kernel(D, Rp, n, row_beg, k_beg, transposed, par):
    """what k_tile_table (csrc/sht_tables.hip) stores of the dense [Rp, Rp] matrix D in each of its modes: par -1 the matrix
    (or its transpose), 0 / 1 the half of the even / odd degrees, 2 the whole matrix permuted by parity, even degrees first"""
    idx = np.arange(n)
    if par == 2:
        src = np.where(idx < n // 2, 2 * idx, 2 * (idx - n // 2) + 1)
    elif par >= 0:
        src = 2 * idx + par
    else:
        src = idx
    M = (D.T if transposed else D)[np.ix_(src, src)]
    return tile(M, n, row_beg, k_beg)


def detile(raw, n, row_beg, k_beg):
    """the inverse of ``tile``: [n, n], NaN where nothing is stored (rows below row_beg, columns below k_beg)"""
    nrt, nk2 = (n - row_beg) // 16, (n - k_beg) // 8
    t = np.asarray(raw[:nrt * nk2 * 128], dtype=float).reshape(nrt, nk2, 4, 16, 2)  # [rt][kk2][lane >> 4][lane & 15][h]
    D = np.full((n, n), np.nan)
    # row = 16 rt + (lane & 15); k = 8 kk2 + 4 h + (lane >> 4)
    D[row_beg:, k_beg:] = t.transpose(0, 3, 1, 4, 2).reshape(16 * nrt, 8 * nk2)
    return D


def table_blocks(tab, raw, kind):
    """the blocks of a side's tiled table by (order m, parity half): -1 a block that spans the order, 0 / 1 the even- /
    odd-degree half of the split Gram kinds (for the permuted order 0 of gram_split0: its diagonal blocks, and the whole
    permuted matrix under (0, 2))"""
    kind = KINDS[kind] if isinstance(kind, (int, np.integer)) else kind
    Rp, blocks = tab["Rp"], {}
    for m, off, kb, odd_off, odd_kb in tab["orders"]:
        m, off, kb = int(m), int(off), int(kb)
        if kind == "gram_split0" and m == 0:
            P = detile(raw[off:], Rp, 0, 0)
            blocks[0, 2], blocks[0, 0], blocks[0, 1] = P, P[:Rp // 2, :Rp // 2], P[Rp // 2:, Rp // 2:]
        elif odd_off >= 0:
            blocks[m, 0] = detile(raw[off:], Rp // 2, kb, kb)
            blocks[m, 1] = detile(raw[int(odd_off):], Rp // 2, int(odd_kb), int(odd_kb))
        else:
            blocks[m, -1] = detile(raw[off:], Rp, kb if kind in ROWS_EL else 0, kb if kind in K_EL else 0)
    return blocks


# ---- host tables in the layout of the device tables ------------------------------------------------------------------------------------
_HOST = {}


def host_dense(L, spin, m, fwd=False):
    """B [Rp ring, Rp el] (fwd: A [Rp el, Rp ring]) of order m from pxm_host_sht_tables, zero-padded to Rp"""
    if (L, spin, m, fwd) not in _HOST:
        from pxmcmc_amd._lib import lib

        Rp = -(-L // 16) * 16
        D, P = np.zeros((L, L)), np.zeros((Rp, Rp))
        if fwd and L > 64:
            # (the exact-quadrature table costs L^3 long-double products per order on the host; above L = 64 the host tests,
            # which are about the arithmetic and the list, take B^T times the ring weights instead: the same zero pattern)
            D = (host_dense(L, spin, m)[:L, :L] * _ops().mw_ring_weights(L)[:, None]).T
        else:
            assert lib.pxm_host_sht_tables(L, spin, m, None if fwd else D.ctypes.data, D.ctypes.data if fwd else None) == 0
        P[:L, :L] = D
        _HOST[L, spin, m, fwd] = P
    return _HOST[L, spin, m, fwd]


def host_blocks(tab, kind):
    """``table_blocks`` of a table built on the host (the Gram matrix as a float64 product): what the model runs on where
    there is no GPU; same keys, same NaN where the device stores nothing"""
    kind = KINDS[kind] if isinstance(kind, (int, np.integer)) else kind
    L, spin, Rp, blocks = tab["L"], tab["spin"], tab["Rp"], {}
    for m, _, kb, odd_off, odd_kb in tab["orders"]:
        m, kb = int(m), int(kb)
        D = host_dense(L, spin, m, kind in ("fwd", "fwd_adj"))
        D = (D.T if kind in ("inv_adj", "fwd_adj") else D.T @ D if kind.startswith("gram") else D).copy()
        if kind == "gram_split0" and m == 0:
            perm = np.r_[np.arange(0, Rp, 2), np.arange(1, Rp, 2)]
            P = D[np.ix_(perm, perm)]
            blocks[0, 2], blocks[0, 0], blocks[0, 1] = P, P[:Rp // 2, :Rp // 2], P[Rp // 2:, Rp // 2:]
        elif odd_off >= 0:
            for par, k0 in ((0, kb), (1, int(odd_kb))):
                H = D[par::2, par::2].copy()
                H[:k0], H[:, :k0] = np.nan, np.nan
                blocks[m, par] = H
        else:
            D[:kb if kind in ROWS_EL else 0] = np.nan
            D[:, :kb if kind in K_EL else 0] = np.nan
            blocks[m, -1] = D
    return blocks


def host_pole(L):
    """b_l = B^0[theta = pi][l] by parity, [Rp / 2 even degrees | Rp / 2 odd degrees] (the last ring is the pole)"""
    Rp = -(-L // 16) * 16
    B = host_dense(L, 0, 0)
    b = np.zeros(Rp)
    b[:Rp // 2], b[Rp // 2:] = B[L - 1, 0::2], B[L - 1, 1::2]
    return b


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def make_inputs(rep, seed, impulse=None):
    """per side {x, x2, ks, rs, hd, y}: normal draws 2^-6 .. 2^6 apart in EVERY entry, padding rows and dead columns included;
    shared arrays are the same objects.  ``impulse`` = (j, columns): operand row k of column c < columns is 1 where
    k = c + columns * j, the second operand zero -- every output is one table entry times its scales (two with a pole term).
    y starts as the sentinel."""
    rng = np.random.default_rng(seed)

    def draw(*shape):
        return rng.standard_normal(shape) * 2.0 ** rng.integers(-6, 7, size=shape)

    out = []
    for i, s in enumerate(rep["sides"]):
        d = {}
        shape_x, shape_y = (2 * s["xL"] - 1, s["xRp"], s["xn"]), (2 * s["yL"] - 1, s["yRp"], s["yn"])
        xs = _shared(rep, i, "x")
        if xs is not None:
            d["x"], d["x2"] = out[xs]["x"], out[xs]["x2"]
        else:
            d["x"] = draw(*shape_x)
            d["x2"] = draw(*shape_x) if s["off_x2"] >= 0 else None
            if impulse is not None:
                d["x"][:] = 0.0
                k, c = np.arange(s["xRp"])[:, None], np.arange(s["xn"])[None, :]
                d["x"][:, (k == c + impulse[1] * impulse[0]) & (c < impulse[1])] = 1.0
                if d["x2"] is not None:
                    d["x2"][:] = 0.0
        ys = _shared(rep, i, "y")
        if ys is not None:
            d["y"], d["hd"] = out[ys]["y"], out[ys]["hd"]
        else:
            d["y"] = np.full(shape_y, SENTINEL)
            d["hd"] = draw(shape_y[0], shape_y[1], 2) if s["off_hd"] >= 0 else None
        d["ks"] = draw(s["xRp"]) if s["off_ks"] >= 0 else None
        d["rs"] = draw(s["yRp"]) if s["off_rs"] >= 0 else None
        out.append(d)
    return out


def _shared(rep, i, which):
    """index of the earlier side whose operand (x) / result (y) array side i uses, or None"""
    key = "off_" + which
    for j in range(i):
        if rep["sides"][j][key] == rep["sides"][i][key]:
            return j
    return None


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def launched_columns(rep, C):
    """columns a run for C chains launches: the packed tile's pk columns, or the column groups (32 columns while 32 remain, 16
    after) that hold a live chain"""
    lay = rep["layout"]
    if lay["pk"]:
        return lay["pk"]
    n = 0
    for col0 in range(0, lay["ncol"], 32):
        if C - col0 // 2 <= 0:
            break
        n = col0 + (32 if lay["ncol"] - col0 >= 32 else 16)
    return n


def variants(rep, C):
    """the kernel instantiations a run of this list for C chains launches: ("pk", PK, TWO, SK), ("pole", CT) or
    (CT, NSLAB, TWO, SK), by the rule of launch_gemm / launch_gemm_packed / run_tasks"""
    lay = rep["layout"]
    two, sk, pole = bool(lay["flags"] & 1), bool(lay["flags"] & 2), bool(lay["flags"] & 4)
    if lay["pk"]:
        return {("pk", lay["pk"], two, sk)}
    out = set()
    for col0 in range(0, launched_columns(rep, C), 32):
        ct = 2 if lay["ncol"] - col0 >= 32 else 1
        out.add(("pole", ct) if pole else (ct, lay["nslab"], two, sk))
    return out


ALL_VARIANTS = ({(ct, ns, two, sk) for ct in (1, 2) for ns in (1, 2) for two in (False, True) for sk in (False, True)}
                | {("pole", 1), ("pole", 2)} | {("pk", pk, two, sk) for pk in (2, 4) for two in (False, True) for sk in (False, True)})


def _plane(a, midx, par):
    """plane of order index midx of an array; a parity half sees it two rows at a time: half-row r = row 2 r + par"""
    p = a[midx]
    return p if par < 0 else p.reshape(p.shape[0] // 2, 2, p.shape[1])[:, par]


def gemm_ld(rep, blocks, inp, C, affine=None, poles=None, dtype=LD):
    """-> (val, mask, S, N per side, scratch mask): what a correct launch of the reported list writes into each side's result
    array (``dtype`` arithmetic; long double: the model, float64: an evaluation the bound must hold for as well), where, the
    absolute-value expression S and the rounding count N; ``scratch`` marks the doubles of the scratch row block that the
    -m slab of order 0 writes.  blocks[side], poles[side]: the de-tiled table and pole column."""
    lay, paired = rep["layout"], bool(rep["layout"]["paired"])
    ncols = launched_columns(rep, C)
    cols = np.arange(ncols)
    res = [dict(val=np.zeros(d["y"].shape, dtype=dtype), mask=np.zeros(d["y"].shape, dtype=bool), S=np.zeros(d["y"].shape),
                N=np.zeros(d["y"].shape, dtype=np.int64)) for d in inp]
    for i in range(len(inp)):  # shared result arrays share their model
        j = _shared(rep, i, "y")
        if j is not None:
            res[i] = res[j]
    scratch = np.zeros(lay["scratch_doubles"], dtype=bool)
    for t in rep["tasks"]:
        if t[F["n_rt"]] == 0:
            continue
        m, par, row0, nrow = int(t[F["m"]]), int(t[F["par"]]), int(t[F["row0"]]), 16 * int(t[F["n_rt"]])
        kb, ke, pole_n, sa = int(t[F["k_beg"]]), int(t[F["k_end"]]), int(t[F["pole_n"]]), int(t[F["side"]])
        rows = np.arange(row0, row0 + nrow)
        T = blocks[sa][m, par][row0:row0 + nrow, kb:ke]
        assert np.isfinite(T).all(), "a task reads table entries that are not stored"
        groups = [(0, sa)] + ([(1, int(t[F["side_b"]]))] if paired and t[F["side_b"]] >= 0 else [])
        for g, si in groups:
            s, d = rep["sides"][si], inp[si]
            lo, hi = int(t[F["row_lo1" if g else "row_lo"]]), int(t[F["row_hi1" if g else "row_hi"]])
            keep = (rows >= lo) & (rows < hi)
            for slab, ms in enumerate((m, -m) if paired else (m,)):
                x = _plane(d["x"], ms + s["xL"] - 1, par)[:, :ncols]
                x2 = _plane(d["x2"], ms + s["xL"] - 1, par)[:, :ncols] if d["x2"] is not None else None
                ks = d["ks"][kb:ke, None] if d["ks"] is not None else None

                def staged(rws, absolute, scale):
                    v = np.abs(x[rws]) if absolute else x[rws].astype(dtype)
                    if x2 is not None:
                        v = v + (np.abs(x2[rws]) if absolute else x2[rws].astype(dtype))
                    if scale is not None:
                        v = v * (np.abs(scale) if absolute else scale.astype(dtype))
                    return v

                xs, xa = staged(slice(kb, ke), False, ks), staged(slice(kb, ke), True, ks)
                nz = np.flatnonzero((xa != 0).any(axis=1))
                acc = T[:, nz].astype(dtype) @ xs[nz]
                S = (np.abs(T[:, nz]) @ xa[nz]) * (1 + 2.0 ** -40)  # (float64: rounded up by more than its own error)
                N = np.broadcast_to((xa != 0).sum(axis=0) + ROUNDINGS_EXTRA, acc.shape).copy()
                if pole_n:
                    b = poles[sa]
                    b_own, b_oth = b[par * pole_n + rows], b[(1 - par) * pole_n:(2 - par) * pole_n]
                    xo = _plane(d["x"], s["xL"] - 1, 1 - par)[:pole_n, :ncols]
                    xo2 = _plane(d["x2"], s["xL"] - 1, 1 - par)[:pole_n, :ncols] if d["x2"] is not None else 0.0
                    sc = b_oth.astype(dtype) @ (xo.astype(dtype) + (xo2.astype(dtype) if d["x2"] is not None else 0))
                    sca = np.abs(b_oth) @ (np.abs(xo) + np.abs(xo2))
                    acc = acc + dtype(0.5) * b_own.astype(dtype)[:, None] * sc[None, :]
                    S = S + 0.5 * np.abs(b_own)[:, None] * sca[None, :] * (1 + 2.0 ** -40)
                    N = N + ((np.abs(xo) + np.abs(xo2)) != 0).sum(axis=0)[None, :]
                if affine is not None:
                    ns, w = affine
                    hd = _plane(d["hd"], ms + s["yL"] - 1, par)[rows] if d["hd"] is not None else np.zeros((nrow, 2))
                    u = dtype(ns) * acc - np.tile(hd, (1, ncols // 2)).astype(dtype)
                    Su = abs(ns) * S + np.abs(np.tile(hd, (1, ncols // 2)))
                    wr, wi = dtype(w.real), dtype(w.imag)
                    v = np.empty_like(u)
                    v[:, 0::2] = wr * u[:, 0::2] - wi * u[:, 1::2]
                    v[:, 1::2] = wr * u[:, 1::2] + wi * u[:, 0::2]
                    Sv = abs(w.real) * Su + abs(w.imag) * Su.reshape(nrow, -1, 2)[:, :, ::-1].reshape(nrow, -1)
                    N = np.maximum(N, N.reshape(nrow, -1, 2)[:, :, ::-1].reshape(nrow, -1))
                    dead = cols >= 2 * C  # padding chains are written as zero
                    v[:, dead], Sv[:, dead] = 0, 0
                    acc, S = v, Sv
                if d["rs"] is not None:
                    acc, S = acc * d["rs"][rows, None].astype(dtype), S * np.abs(d["rs"][rows, None])
                if slab & 1:
                    acc = acc * dtype(int(t[F["sign1"]]))
                if paired and m == 0 and slab == 1:  # the -m slab of order 0 goes to the scratch row block
                    pitch = s["yn"] * (2 if par >= 0 else 1)
                    at = (max(par, 0) * s["yn"] + rows[keep, None] * pitch + cols[None, :]).ravel()
                    scratch[at] = True
                    continue
                r = res[si]
                for name, a in (("val", acc), ("S", S), ("N", N), ("mask", True)):
                    pl = _plane(r[name], ms + s["yL"] - 1, par)
                    pl[rows[keep], :ncols] = a[keep] if name != "mask" else True
    return res, scratch


def gamma(N):
    return N * U / (1 - N * U)


TINY = 2.0 ** -1074  # a product that underflows is off by up to the smallest subnormal instead of u times itself


def worst_ratio(got, r):
    """max over the written elements of |got - model| / (u S) (where S is far above the underflow threshold) and whether every
    one is inside gamma_N S + N 2^-1074"""
    err = np.abs(got.astype(LD) - r["val"].astype(LD)).astype(float)[r["mask"]]
    S, N = r["S"][r["mask"]], r["N"][r["mask"]]
    ok = bool((err <= gamma(N) * S + N * TINY).all())
    big = S > 1e-280
    q = err[big] / (U * S[big])
    return (float(q.max()) if q.size else 0.0), ok


# ---- the cases (shared with tests/test_gpu_gemm.py) ---------------------------------------------------------------------------------------
def case(cid, sides, spin=0, slots=8, pk=0, runs=((None, None),), order=None, affine=False, want=None, shifts=None):
    """runs: (C or None = every slot, ...); want: the geometry the case is there for (asserted in test_case_geometry)"""
    return dict(id=cid, sides=sides, spin=spin, slots=slots, pk=pk, Cs=tuple(c or slots for c, _ in runs), order=order,
                affine=affine, want=want or {}, shifts=shifts)


def _cases():
    c = []
    four = ("inv", "fwd", "inv_adj", "fwd_adj")
    for spin, kind in itertools.product((0, 2), four):  # one row tile, one chunk, masks inactive
        c.append(case(f"one-tile-s{spin}-{kind}", [dict(kind=kind, bl=16)], spin=spin,
                      want=dict(n_rt={1}, chunks={1}, nslab=2 if spin == 0 else 1, flags=0)))
    for kind in four:  # Rp = 48: not a multiple of 32, zero padding rows
        c.append(case(f"pad-L40-{kind}", [dict(kind=kind, bl=40)], runs=((3, None),), want=dict(Rp=48)))
    for kind in four:  # tasks of 1 .. 8 row tiles and a second task per order, chunk counts 1 .. 9, table starts above 0
        el = kind in K_EL
        extras = dict(ks=True) if el else dict(rs=True)
        for tag, opt in (("plain", {}), ("scaled", dict(extras)),
                         ("cut17", dict(extras, el_lo=17, **({} if el else dict(rows=(17, 120))))),
                         ("cut48", dict(el_lo=48, **({} if el else dict(rows=(48, 130)))))):
            full = dict(n_rt={1, 8} if el else set(range(1, 9)), chunks=set(range(1, 10)) if el else {9}, two_tasks_per_order=True,
                        k_above_0=el)
            c.append(case(f"L130-{kind}-{tag}", [dict(kind=kind, bl=130, **opt)],
                          want=full if tag in ("plain", "scaled") else dict(Rp=144, k_above_0=el)))
    for L, slots in ((40, 8), (64, 16)):  # unpaired tables; the weak-lensing inverse has second operand and scale
        for two, ks in itertools.product((False, True), repeat=2):
            c.append(case(f"unpaired-L{L}-two{int(two)}-ks{int(ks)}", [dict(kind="inv", bl=L, two=two, ks=ks)], spin=2, slots=slots,
                          want=dict(nslab=1, flags=int(two) + 2 * int(ks))))
    for two, ks in itertools.product((False, True), repeat=2):  # CT = 2, then CT = 1 at col0 = 32; a skipped second group
        sd = [dict(kind="inv", bl=64, two=two, ks=ks)]
        c.append(case(f"ct2-L64-16slots-two{int(two)}-ks{int(ks)}", sd, slots=16, runs=((16, None), (9, None)), want=dict(nslab=2)))
        c.append(case(f"ct21-L64-24slots-two{int(two)}-ks{int(ks)}", sd, slots=24, runs=((24, None), (17, None), (16, None)),
                      want=dict(nslab=2, skipped_group_at=16)))
    # all-scales list: two bandlimits into one L-layout result, disjoint row masks, per-task two / has_sk selects
    c.append(case("all-scales-fwd", [dict(kind="fwd", bl=32, L=64, rs=True, rows=(0, 32), two=True, ks=True),
                                     dict(kind="fwd", bl=64, L=64, rs=True, rows=(32, 64), el_lo=32, y_share=0)],
                  want=dict(flags=3, mixed_two=True)))
    c.append(case("all-scales-fwd_adj", [dict(kind="fwd_adj", bl=32, L=64, ks=True), dict(kind="fwd_adj", bl=64, L=64, x_share=0)],
                  want=dict(flags=2, both_sides=True)))
    for L, slots, C in ((40, 8, 3), (64, 8, 3), (40, 16, 16), (64, 16, 16), (40, 24, 17), (64, 24, 17)):  # affine epilogue, dense Gram
        c.append(case(f"affine-gram-L{L}-{C}of{slots}", [dict(kind="gram", bl=L, two=True, hd=True)], slots=slots, runs=((C, None),),
                      affine=True, want=dict(flags=1)))
    for kind, L in itertools.product(("gram_split", "gram_split0"), (32, 64, 96)):  # parity halves, dense orders, pole tasks
        c.append(case(f"{kind}-L{L}", [dict(kind=kind, bl=L, two=True, hd=True)], runs=((5, None),), affine=True,
                      want=dict(halves=True, dense_orders=True, pole=kind == "gram_split0")))
    c.append(case("pole-L96-16slots", [dict(kind="gram_split0", bl=96, two=True, hd=True)], slots=16, runs=((16, None),), affine=True,
                  want=dict(pole=True, pole_n=48)))
    c.append(case("pole-L160-8slots", [dict(kind="gram_split0", bl=160, two=True, hd=True)], runs=((8, None),), affine=True,
                  want=dict(pole=True, pole_n=80)))
    c.append(case("pole-L96-24slots", [dict(kind="gram_split0", bl=96, two=True, hd=True)], slots=24, runs=((17, None),), affine=True,
                  want=dict(pole=True, pole_n=48)))
    # packed tiles: synthesis forward (rs + mask) and forward adjoint (ks), one side and a pair, narrow and plan pitch
    n = 0
    for pk, two, fwd, L in itertools.product((2, 4), (False, True), (True, False), (16, 112)):
        pair, narrow = bool((n >> 1) & 1) ^ (L == 112), bool((n >> 2) & 1) ^ (L == 16)  # (each with every pk, kind and L)
        n += 1
        nc = dict(x_ncol=pk, y_ncol=pk) if narrow else {}
        base = dict(kind="fwd", bl=L, rs=True, rows=(5, L - 3), two=two, **nc) if fwd else dict(kind="fwd_adj", bl=L, ks=True, two=two, **nc)
        sides = [base, dict(base, **(dict(rows=(0, L - 7), el_lo=3) if fwd else dict(el_lo=19)))] if pair else [base]
        c.append(case(f"packed-pk{pk}-{'fwd' if fwd else 'fwd_adj'}-two{int(two)}-L{L}-{'pair' if pair else 'one'}-{'narrow' if narrow else 'plan'}",
                      sides, slots=pk // 2, pk=pk, want=dict(pk=pk, slabs=4 if pair else 2, flags=int(two) + (0 if fwd else 2),
                                                             chunks={1} if L == 16 else ({7} if fwd else set(range(1, 8))))))
    for order in ("plain", "bins", "xcd"):
        # (the parity-split Gram list: 97 tasks of unequal length, which leave the eight queues of xcd unequal)
        c.append(case(f"order-{order}", [dict(kind="gram_split", bl=64, two=True, hd=True)], order=order, runs=((5, None),), affine=True,
                      want=dict(padding=order == "xcd")))
    return c


CASES = _cases()
CASE_IDS = [cs["id"] for cs in CASES]


def case_report(cs, monkeypatch, plan_cls=None):
    """the dry-run report of a case (or, given ops.GemmPlan, the plan), created under the case's launch order"""
    if cs["order"]:
        monkeypatch.setenv("PXM_GEMM_ORDER", cs["order"])
    else:
        monkeypatch.delenv("PXM_GEMM_ORDER", raising=False)
    if plan_cls is not None:
        return plan_cls(cs["sides"], spin=cs["spin"], max_chains=cs["slots"], pk=cs["pk"])
    return _ops().gemm_plan_geometry(cs["sides"], spin=cs["spin"], max_chains=cs["slots"], pk=cs["pk"])


AFFINE = (0.75, complex(-0.625, 1.5))


def products(rep, C):
    """long-double products of the model of one run"""
    t = rep["tasks"]
    return int((16 * t[:, F["n_rt"]] * (t[:, F["k_end"]] - t[:, F["k_beg"]])).sum()) * launched_columns(rep, C) * \
        (2 if rep["layout"]["paired"] else 1)


# ---- tests ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par,transposed", [(-1, 0), (-1, 1), (0, 0), (1, 0), (2, 0)])
def test_detiler_inverts_the_tiler(par, transposed):
    """every mode of k_tile_table: the tiles, written from the layout comment, of the matrix the mode selects; de-tiled they are
    that matrix from (row_beg, k_beg) on and NaN before"""
    Rp = 64
    D = np.arange(Rp * Rp, dtype=float).reshape(Rp, Rp) + 0.5
    n = Rp // 2 if par in (0, 1) else Rp
    for row_beg, k_beg in ((0, 0), (16, 0), (0, 16), (16, 16)):
        raw = tile_kernel(D, Rp, n, row_beg, k_beg, transposed, par)
        assert raw.size == (n - row_beg) // 16 * ((n - k_beg) // 8) * 128
        src = {2: np.r_[np.arange(0, Rp, 2), np.arange(1, Rp, 2)], 0: np.arange(0, Rp, 2), 1: np.arange(1, Rp, 2)}.get(par, np.arange(Rp))
        want = (D.T if transposed else D)[np.ix_(src, src)]
        got = detile(raw, n, row_beg, k_beg)
        assert np.array_equal(got[row_beg:, k_beg:], want[row_beg:, k_beg:])
        assert np.isnan(got[:row_beg]).all() and np.isnan(got[:, :k_beg]).all()
        # the first chunk of the first tile, by hand: lane l, double h <- row l & 15, k 4 h + (l >> 4)
        assert raw[2 * 17 + 1] == want[row_beg + 1, k_beg + 4 + 1]


@pytest.mark.parametrize("spin", [0, 2])
def test_model_against_the_oracle(spin, monkeypatch):
    """gemm_ld on host tables is the Legendre stage of the oracle's transforms: G = Binv H (inverse), H = Afwd G (forward)"""
    from oracle import ssht

    L, C = 20, 3
    O = ssht.MWTransform(L, spin)
    for kind, mats in (("inv", O.Binv), ("fwd", O.Afwd)):
        cs = case("oracle", [dict(kind=kind, bl=L)], spin=spin)
        rep = case_report(cs, monkeypatch)
        inp = make_inputs(rep, 7)
        res, _ = gemm_ld(rep, [host_blocks(rep["tables"][0], kind)], inp, C)
        for m in range(-(L - 1), L):
            want = mats[m + L - 1].astype(LD) @ inp[0]["x"][m + L - 1, :L].astype(LD)
            got = res[0]["val"][m + L - 1, :L]
            scale = np.abs(mats[m + L - 1]) @ np.abs(inp[0]["x"][m + L - 1, :L])
            kb = abs(m) // 16 * 16 if kind == "fwd" else 0  # degrees below the order's first tile are not written: zero
            assert res[0]["mask"][m + L - 1, kb:L].all() and not res[0]["mask"][m + L - 1, :kb].any() and not want[:kb].any()
            # (the oracle's tables and the library's agree to 1e-13 of an entry: test_host_ring_tables_match_oracle)
            # except on the pole ring of an order m != 0, where sin(pi)^|m| is not zero in double and differs between the two
            n = L - 1 if (kind == "inv" and m != 0) else L
            tol = 2e-13 * (scale + np.abs(inp[0]["x"][m + L - 1, :L]).sum(axis=0)[None, :])  # (relative and absolute)
            assert (np.abs((got - want).astype(float))[:n] <= tol[:n]).all(), (kind, m)


def _host_model(cs, rep, C, seed, dtype, impulse=None):
    blocks = [host_blocks(rep["tables"][i], s["kind"]) for i, s in enumerate(cs["sides"])]
    poles = [host_pole(s["bl"]) if s["kind"] == "gram_split0" else None for s in cs["sides"]]
    inp = make_inputs(rep, seed, impulse)
    return gemm_ld(rep, blocks, inp, C, AFFINE if cs["affine"] else None, poles, dtype)


@pytest.mark.parametrize("cs", CASES, ids=CASE_IDS)
def test_bound_holds_for_a_float64_evaluation(cs, monkeypatch):
    """the float64 numpy evaluation of every case's inputs stays inside gamma_N S of the long-double model: the bound holds
    for the reference alone.  (Printed as GEMM-RATIO-F64; DESIGN.md records the figures.)"""
    rep = case_report(cs, monkeypatch)
    C = cs["Cs"][0]
    assert products(rep, C) <= 64 << 20, products(rep, C)
    ref, s_ref = _host_model(cs, rep, C, 11, LD)
    f64, s_f64 = _host_model(cs, rep, C, 11, np.float64)
    worst = 0.0
    for r, f in zip(ref, f64):
        assert np.array_equal(r["mask"], f["mask"])
        q, ok = worst_ratio(f["val"], r)
        worst = max(worst, q)
        assert ok, (cs["id"], q)
    assert np.array_equal(s_ref, s_f64)
    print(f"GEMM-RATIO-F64 {cs['id']} {worst:.2f}")


def _geometry(rep):
    t = rep["tasks"][rep["tasks"][:, F["n_rt"]] > 0]
    return t, (t[:, F["k_end"]] - t[:, F["k_beg"]]) // 16


@pytest.mark.parametrize("cs", CASES, ids=CASE_IDS)
def test_case_geometry(cs, monkeypatch):
    """the dry-run list of every GPU case has what the case is there for"""
    rep = case_report(cs, monkeypatch)
    lay, want = rep["layout"], cs["want"]
    t, chunks = _geometry(rep)
    assert lay["n_tasks"] == len(rep["tasks"]) and lay["ncol"] == 2 * (-(-cs["slots"] // 8) * 8)
    assert lay["pk"] == cs["pk"] and lay["nslab"] == (4 if cs["pk"] else (2 if cs["spin"] == 0 else 1))
    assert (t[:, F["side"]] >= 0).all() and (t[:, F["row0"]] % 16 == 0).all() and (t[:, F["k_beg"]] % 16 == 0).all()
    for key, val in want.items():
        if key == "n_rt":
            assert set(t[:, F["n_rt"]].tolist()) == val
        elif key == "chunks":
            assert set(chunks.tolist()) == val, sorted(set(chunks.tolist()))
        elif key == "nslab":
            assert lay["nslab"] == val and set(t[:, F["nslab"]].tolist()) == {val}
        elif key == "flags":
            assert lay["flags"] == val, lay["flags"]
        elif key == "Rp":
            assert rep["tables"][0]["Rp"] == val and val % 32 != 0
        elif key == "two_tasks_per_order":
            per = np.bincount(t[:, F["m_unit"]])
            assert per.max() == 2
        elif key == "k_above_0":
            assert bool((t[:, F["k_beg"]] > 0).any()) == val
            assert (rep["tables"][0]["orders"][:, 2] > 0).any()  # table blocks that start above 0 (tab_skip / kb)
        elif key == "skipped_group_at":
            assert launched_columns(rep, val) == 32 < lay["ncol"] and launched_columns(rep, val + 1) == lay["ncol"]
        elif key == "mixed_two":
            assert set(t[:, F["side"]].tolist()) == {0, 1} and len({bool(s.get("two")) for s in cs["sides"]}) == 2
        elif key == "both_sides":
            assert set(t[:, F["side"]].tolist()) == {0, 1} and len({bool(s.get("ks")) for s in cs["sides"]}) == 2
        elif key == "halves":
            assert {-1, 0, 1} <= set(t[:, F["par"]].tolist())
        elif key == "dense_orders":
            assert ((t[:, F["par"]] == -1) & (t[:, F["m"]] > 0)).any() or cs["sides"][0]["bl"] <= 32
        elif key == "pole":
            assert bool((t[:, F["pole_n"]] > 0).any()) == val and bool(lay["flags"] & 4) == val
            assert ((t[:, F["pole_n"]] > 0) == ((t[:, F["m"]] == 0) & (t[:, F["par"]] >= 0))).all()
        elif key == "pole_n":
            assert set(t[t[:, F["pole_n"]] > 0, F["pole_n"]].tolist()) == {val}
        elif key == "pk":
            assert lay["pk"] == val
        elif key == "slabs":
            assert set(t[:, F["nslab"]].tolist()) == {val} and (t[:, F["side_b"]] >= 0).all() == (val == 4)
        elif key == "padding":
            assert bool((rep["tasks"][:, F["n_rt"]] == 0).any()) == val
        else:
            raise AssertionError(key)


def test_the_cases_reach_every_instantiation(monkeypatch):
    """launch_gemm and launch_gemm_packed can select 26 kernels: each is launched by a run of some case"""
    seen = {}
    for cs in CASES:
        rep = case_report(cs, monkeypatch)
        for C in cs["Cs"]:
            for v in variants(rep, C):
                seen.setdefault(v, []).append(cs["id"])
    assert set(seen) == ALL_VARIANTS, ALL_VARIANTS ^ set(seen)
    assert len(ALL_VARIANTS) == 26


def test_launch_orders_permute_one_list(monkeypatch):
    """plain, bins and xcd order the same tasks; xcd pads its queues with empty entries"""
    reps = {cs["order"]: case_report(cs, monkeypatch) for cs in CASES if cs["order"]}
    key = lambda rep: sorted(map(tuple, rep["tasks"][rep["tasks"][:, F["n_rt"]] > 0].tolist()))
    assert key(reps["plain"]) == key(reps["bins"]) == key(reps["xcd"])
    assert (reps["xcd"]["tasks"][:, F["n_rt"]] == 0).any() and not (reps["plain"]["tasks"][:, F["n_rt"]] == 0).any()
    assert not np.array_equal(reps["plain"]["tasks"], reps["xcd"]["tasks"][:len(reps["plain"]["tasks"])])


def test_refusals_of_the_dry_run_plan():
    """the launchers' and the builders' own refusals surface: a pole term outside the Gram list, a split table where the
    parity split does not exist, a packed list for more chains than its tile carries"""
    ops = _ops()
    with pytest.raises(ops.PxmError, match="row pitch of its own|pole term outside the Gram list"):
        ops.gemm_plan_geometry([dict(kind="gram_split0", bl=64, hd=True)], max_chains=16)
    with pytest.raises(ops.PxmError, match="parity split needs spin-0 tables and Rp % 32 == 0"):
        ops.gemm_plan_geometry([dict(kind="gram_split", bl=40, two=True)])
    with pytest.raises(ValueError, match="at most pk / 2 in a packed list"):
        ops.gemm_plan_geometry([dict(kind="fwd", bl=16)], max_chains=2, pk=2)
    with pytest.raises(ops.PxmError, match="a packed pair share one table"):
        ops.gemm_plan_geometry([dict(kind="fwd", bl=16), dict(kind="fwd", bl=32)], max_chains=1, pk=2)
    with pytest.raises(ops.PxmError, match="needs a packed list"):
        ops.gemm_plan_geometry([dict(kind="fwd", bl=16, x_ncol=4)])
    with pytest.raises(ValueError, match="kind must be one of"):
        ops.gemm_plan_geometry([dict(kind="nope", bl=16)])
