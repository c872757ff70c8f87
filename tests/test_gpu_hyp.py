"""Hypothesis tests of image structure on the GPU (csrc/inpaint.hip, pxmcmc_amd.uncertainty.inpaint_regions / hypothesis_test;
DESIGN.md section 14c): pxm_inpaint_step against its numpy statement, batch independence, graph replay and refusals;
inpaint_regions against the same iteration composed from torch.where and host norms; the whole test on the planted structure
of tests/test_hyp_host.py (Identity) and under masked weak lensing, the smoothing surrogate, and the example."""
import numpy as np
import pytest

from test_hyp_host import (BACKGROUND_REGION, BLOB_REGION, L16, B16, JMIN16, LMDA, SIG, SIZE, decision_np, planted,
                           planted_data)
from test_lci_host import F_ld, LD, U, f_tol

pytestmark = pytest.mark.gpu

C_MAX = 16  # slots the buffers are allocated for
TERM_ROUNDINGS = 4  # of one term of a sum: the two component differences, the product and the fma


def _i32(a):
    import torch

    from pxmcmc_amd import ops

    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int32))).to(ops.device())


def _nan_buf(rows, n, cplx):
    import torch

    from pxmcmc_amd import ops

    return torch.full((rows, n), float("nan"), dtype=torch.complex128 if cplx else torch.float64, device=ops.device())


def _bits(t):
    import torch

    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int64)


def _inputs(npix, C, cplx, seed, full=False):
    rng = np.random.default_rng(seed)
    vec = (lambda *s: rng.normal(size=s) + 1j * rng.normal(size=s)) if cplx else (lambda *s: rng.normal(size=s))
    y, x_prev, x_map = vec(C, npix), vec(C, npix), vec(npix)
    labels = np.zeros(npix, np.int32) if full else rng.integers(-1, 3, size=npix).astype(np.int32)
    region = np.array([0, 1, 7, 2, -1] * 4)[:C].astype(np.int32)  # 7: an empty region; -1: no region at all
    scale = 10.0 ** rng.uniform(-3, 0, size=C)  # how far x_prev is from the next image: ratios d2 / n2 over six decades
    nxt = np.where((labels[None] == region[:, None]) & (labels[None] >= 0), y, x_map[None])
    x_prev = nxt + scale[:, None] * x_prev
    return y, x_prev, x_map, labels, region, rng


def _tol2_between(ratios, bound):
    """a tol2 that splits the slots' ratios d2 / n2 (or lies beside the only one), none of them within the sum bound of it"""
    r = np.sort(np.asarray(ratios, dtype=np.float64))
    tol2 = float(np.sqrt(r[len(r) // 2 - 1] * r[len(r) // 2])) if len(r) > 1 and r[len(r) // 2 - 1] > 0 else float(r[-1] * 2.0)
    assert (np.abs(r / tol2 - 1.0) > 4 * bound).all(), (r, tol2)  # (both sums within `bound`: the ratio within ~2 bound)
    return tol2


def _launch(y, x_prev, x_map, labels, region, tol2, done0, iters0, stat0, cplx, C):
    """the step on [C] slots of [C_MAX] NaN-filled / marked buffers -> device tensors (x_next, done, iters, stat)"""
    import torch

    from pxmcmc_amd import ops

    npix = x_map.shape[0]
    dt = torch.complex128 if cplx else torch.float64
    Y, XP, XN = _nan_buf(C_MAX, npix, cplx), _nan_buf(C_MAX, npix, cplx), _nan_buf(C_MAX, npix, cplx)
    Y[:C], XP[:C] = ops.as_device(y, dt), ops.as_device(x_prev, dt)
    done, iters = _i32(np.full(C_MAX, -7)), _i32(np.full(C_MAX, -7))
    done[:C], iters[:C] = _i32(done0), _i32(iters0)
    stat = torch.full((C_MAX, 2), float("nan"), dtype=torch.float64, device=Y.device)
    stat[:C] = ops.as_device(stat0)
    out = ops.inpaint_step(Y[:C], XP[:C], ops.as_device(x_map, dt), _i32(labels), _i32(region), tol2, done[:C], iters[:C],
                           stat[:C], out=XN[:C])
    torch.cuda.synchronize()
    assert out.data_ptr() == XN.data_ptr()
    assert torch.isnan(XN[C:]).all() and torch.isnan(stat[C:]).all()
    assert (done[C:] == -7).all() and (iters[C:] == -7).all()  # nothing written beyond C
    return XN[:C], done[:C], iters[:C], stat[:C]


@pytest.mark.parametrize("npix", [1, 63, 64, 65, 257, 4099, 4100])
@pytest.mark.parametrize("C", [1, 3, 16])
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_step_against_its_statement(npix, C, cplx):
    """x_next, done and iters bit for bit; |stat - exact| <= (inpaint_sum_depth(npix) + 4) 2^-53 exact (non-negative terms,
    four roundings per term); the device's flag is stat[0] <= tol2 stat[1] of its own stat; slots that were done keep
    everything.  Mixed labels (with -1, an empty region, a region -1) and the full region; even npix takes the 16-byte
    path of the real kernel (4100: several slices), odd npix the 8-byte one.
    Largest error / bound over all cases on one MI355X: 0.083."""
    from pxmcmc_amd.uncertainty import inpaint_step_np, inpaint_sum_depth

    bound = (inpaint_sum_depth(npix) + TERM_ROUNDINGS) * U
    worst = 0.0
    for k, full in enumerate((False, True)):
        y, x_prev, x_map, labels, region, rng = _inputs(npix, C, cplx, 100 * npix + 10 * C + 2 * cplx + k, full)
        done0 = rng.integers(0, 2, size=C).astype(np.int32)
        done0[:3] = [k] if C == 1 else [0, 1, 0]  # (C = 1: not done with the mixed labels, done with the full region)
        iters0 = rng.integers(0, 50, size=C).astype(np.int32)
        stat0 = rng.random((C, 2)) + 5.0
        _, _, _, exact = inpaint_step_np(y, x_prev, x_map, labels, region, 0.0, done0, iters0, stat0)
        live = done0 == 0
        ratios = (exact[live, 0] / exact[live, 1]).astype(np.float64)
        tol2 = _tol2_between(ratios, bound) if live.any() else 0.3
        want_x, want_done, want_iters, exact = inpaint_step_np(y, x_prev, x_map, labels, region, tol2, done0, iters0, stat0)
        XN, done, iters, stat = _launch(y, x_prev, x_map, labels, region, tol2, done0, iters0, stat0, cplx, C)
        got_x, got_stat = XN.cpu().numpy(), stat.cpu().numpy()
        assert np.array_equal(got_x.view(np.int64), np.ascontiguousarray(want_x).view(np.int64))
        assert np.array_equal(done.cpu().numpy(), want_done) and np.array_equal(iters.cpu().numpy(), want_iters)
        assert np.array_equal(got_stat[~live], stat0[~live])
        err = np.abs(got_stat.astype(LD) - exact)[live]
        assert (err <= bound * exact[live]).all(), (err, bound * exact[live])
        assert np.array_equal(done.cpu().numpy()[live], (got_stat[live, 0] <= tol2 * got_stat[live, 1]).astype(np.int32))
        if live.any():
            worst = max(worst, float((err / (bound * exact[live])).max()))
            if C > 1 and not full:
                assert 0 < want_done[live].sum() < live.sum()  # both outcomes of the flag
    print(f"step npix={npix} C={C} cplx={cplx}: largest error / bound {worst:.3f}")


def test_step_nan_never_freezes():
    from pxmcmc_amd.uncertainty import inpaint_step_np

    npix, C = 300, 2
    y, x_prev, x_map, labels, region, _ = _inputs(npix, C, True, 9, full=True)
    y[0, 17] = np.nan
    zeros = np.zeros(C, np.int32)
    _, done, iters, stat = _launch(y, x_prev, x_map, labels, region[:1].repeat(C), 1e300, zeros, zeros, np.zeros((C, 2)), True, C)
    _, want_done, _, _ = inpaint_step_np(y, x_prev, x_map, labels, region[:1].repeat(C), 1e300, zeros, zeros, np.zeros((C, 2)))
    assert done.cpu().tolist() == want_done.tolist() == [0, 1] and iters.cpu().tolist() == [1, 1]
    assert np.isnan(stat.cpu().numpy()[0]).all()


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("npix", [4099, 4100])
def test_a_slot_alone_equals_the_slot_in_a_batch(npix, cplx):
    """slot c alone and slot c in a batch of 16, bit for bit: image, sums, flag and counter (several slices)"""
    C = 16
    y, x_prev, x_map, labels, region, rng = _inputs(npix, C, cplx, 21 + cplx)
    zeros = np.zeros(C, np.int32)
    XN, done, iters, stat = _launch(y, x_prev, x_map, labels, region, 1e-3, zeros, zeros, np.zeros((C, 2)), cplx, C)
    for c in (0, 7, 15):
        sl = slice(c, c + 1)
        x1, d1, i1, s1 = _launch(y[sl], x_prev[sl], x_map, labels, region[sl], 1e-3, zeros[:1], zeros[:1], np.zeros((1, 2)), cplx, 1)
        assert (_bits(x1) == _bits(XN[sl])).all() and (_bits(s1) == _bits(stat[sl])).all()
        assert d1.tolist() == done[sl].tolist() and i1.tolist() == iters[sl].tolist()
    assert 0 < int(done.sum()) < C


def test_graph_replay_equals_eager():
    """two ping-pong steps captured into a HIP graph and replayed, on new inputs, equal the eager calls bit for bit"""
    import torch

    from pxmcmc_amd import ops

    npix, C = 1500, 3
    y, x_prev, x_map, labels, region, rng = _inputs(npix, C, True, 33)
    dt = torch.complex128
    Y, XA, XB, XM = ops.as_device(y, dt), ops.as_device(x_prev, dt), _nan_buf(C, npix, True), ops.as_device(x_map, dt)
    lab, reg = _i32(labels), _i32(region)
    scratch = ops.inpaint_scratch(npix, C, Y.device)
    new = lambda: (_i32(np.zeros(C)), _i32(np.zeros(C)), torch.zeros((C, 2), dtype=torch.float64, device=Y.device))  # noqa: E731

    def run(state, a, b):
        ops.inpaint_step(Y, a, XM, lab, reg, 1e-4, *state, out=b, scratch=scratch)
        ops.inpaint_step(Y, b, XM, lab, reg, 1e-4, *state, out=a, scratch=scratch)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(new(), XA.clone(), XB.clone())  # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gstate = new()
    g = torch.cuda.CUDAGraph()
    with ops.capture_scope(), torch.cuda.graph(g):
        run(gstate, XA, XB)
    assert torch.isnan(XB).all() and (gstate[1] == 0).all()  # capture does not execute
    for src in (x_prev, x_prev + 0.1 * rng.normal(size=x_prev.shape)):
        XA.copy_(ops.as_device(src, dt))
        for t in gstate:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        EA, EB, estate = ops.as_device(src, dt), _nan_buf(C, npix, True), new()
        run(estate, EA, EB)
        torch.cuda.synchronize()
        assert (_bits(EA) == _bits(XA)).all() and (_bits(EB) == _bits(XB)).all()
        assert all((_bits(e) == _bits(s)).all() if e.dtype == torch.float64 else torch.equal(e, s) for e, s in zip(estate, gstate))
        assert (estate[1] >= 1).all() and int(estate[0].sum()) >= 1  # (the second step finds the image unchanged: frozen)


def test_bad_arguments_are_refused():
    """bad shapes, dtypes, aliases, a negative tol2 and C < 1 are refused before any launch: NaN-filled outputs stay"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd._lib import PxmError, lib

    npix, C = 40, 2
    dev = ops.device()
    x = torch.ones((C, npix), dtype=torch.float64, device=dev)
    y, xm = 2 * x, torch.zeros(npix, dtype=torch.float64, device=dev)
    lab, reg = _i32(np.zeros(npix)), _i32(np.zeros(C))
    out = _nan_buf(C, npix, False)
    done, iters = _i32(np.zeros(C)), _i32(np.full(C, 5))
    stat = torch.full((C, 2), float("nan"), dtype=torch.float64, device=dev)
    step = lambda **k: ops.inpaint_step(**{**dict(y=y, x_prev=x, x_map=xm, labels=lab, region=reg, tol2=0.1, done=done,  # noqa: E731
                                                  iters=iters, stat=stat, out=out), **k})
    for exc, bad in ((ValueError, dict(out=x)), (ValueError, dict(out=y)), (ValueError, dict(tol2=-1.0)),
                     (ValueError, dict(tol2=float("nan"))), (ValueError, dict(y=y[:1])), (ValueError, dict(x_map=xm[:-1])),
                     (TypeError, dict(labels=lab.to(torch.int64))), (TypeError, dict(labels=lab[:-1])),
                     (TypeError, dict(region=reg[:1])), (TypeError, dict(done=done.to(torch.float64))),
                     (TypeError, dict(stat=stat[:, :1])), (ValueError, dict(out=out.to(torch.complex128))),
                     (ValueError, dict(y=y[:0], x_prev=x[:0])), (ValueError, dict(scratch=torch.empty(1, dtype=torch.float64, device=dev))),
                     (ValueError, dict(tol2=float("inf")))):
        with pytest.raises(exc):
            step(**bad)
    # the C-ABI's own refusals: a partial overlap the wrapper's pointer comparison does not see, C < 1, a negative tol2
    big = _nan_buf(1, (C + 1) * npix, False).reshape(-1)
    big[: C * npix] = 1.0
    with pytest.raises(PxmError, match="overlap"):
        step(x_prev=big[: C * npix].view(C, npix), out=big[npix:].view(C, npix))
    p = lambda t: t.data_ptr()  # noqa: E731
    sc = ops.inpaint_scratch(npix, C, dev)
    for tol2, nc in ((-1.0, C), (0.1, 0)):
        assert lib.pxm_inpaint_step(p(y), p(x), p(xm), p(lab), p(reg), tol2, p(out), p(done), p(iters), p(stat), p(sc), npix, nc, 0, None) < 0
    assert lib.pxm_inpaint_scratch_doubles(npix, 0) < 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(stat).all() and torch.isnan(big[C * npix :]).all()
    assert (iters == 5).all() and (done == 0).all()


# ---- inpaint_regions against the iteration composed from torch ---------------------------------------------------------------------
E2E = {}


def _identity_e2e():
    """the planted structure of the host test (amp = 5) under the Identity measurement: operator, prior, params, FISTA's X*"""
    import contextlib
    import io

    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.mcmc import PxMCMCParams
    from pxmcmc_amd.optim import FISTA
    from pxmcmc_amd.prior import S2_Wavelets_L1

    if "identity" not in E2E:
        oT = planted(5)[0]
        data = planted_data(oT, 5)
        op = SphericalWaveletTransformOperator(data, SIG, "synthesis", L16, B16, JMIN16, max_chains=3)
        reg = S2_Wavelets_L1("synthesis", None, None, LMDA, L=L16, B=B16, J_min=JMIN16)
        p = PxMCMCParams(lmda=LMDA, mu=1.0, complex=False, verbosity=0)
        est = FISTA(op, reg, p, tol=1e-3, max_iter=3000)
        with contextlib.redirect_stdout(io.StringIO()):
            X = est.run()
        E2E["identity"] = (op, reg, p, X)
    return E2E["identity"]


def _e2e(which):
    if which == "identity":
        return _identity_e2e()
    from test_gpu_lci import _e2e as lci_e2e

    return lci_e2e("weaklensing")[:4]


def _two_regions():
    """labels with the blob's superpixel as region 0, the background superpixel as region 1 and -1 elsewhere"""
    from pxmcmc_amd.uncertainty import superpixel_regions

    sp = superpixel_regions(L16, SIZE)
    return np.where(sp == BLOB_REGION, 0, np.where(sp == BACKGROUND_REGION, 1, -1)).astype(np.int32)


def _tau(op, X, frac):
    from pxmcmc_amd import ops

    tr = op.transform
    Xd = ops.as_device(np.asarray(X).astype(complex))
    x_map = ops.as_device(tr.inverse(Xd[None]))
    return frac * float(ops.as_device(tr.forward(x_map)).abs().max())


def _composed(op, X, labels, tau, iters, tol):
    """the same iteration from the same device operators, torch.where and norms on the host -> (images after every
    iteration [iters + 1, C, npix] as numpy, iters_used, the ratios d2 / n2 of every iteration made)"""
    import torch

    from pxmcmc_amd import ops

    tr = op.transform
    Xd = ops.as_device(np.asarray(X).astype(complex))
    x_map = ops.as_device(tr.inverse(Xd[None]))[0]
    lab = torch.from_numpy(labels.reshape(-1).astype(np.int64)).to(Xd.device)
    C = int(labels.max()) + 1
    zeta = lab[None, :] == torch.arange(C, device=Xd.device)[:, None]
    x = torch.where(zeta, torch.zeros_like(x_map)[None], x_map[None]).contiguous()
    done, used, ratios, images = np.zeros(C, bool), np.zeros(C, np.int32), [], [x.cpu().numpy()]
    for _ in range(iters):
        y = ops.as_device(tr.inverse(ops.soft(ops.as_device(tr.forward(x)), tau)))
        nxt = torch.where(zeta, y, x_map[None])
        nxt[torch.from_numpy(done).to(x.device)] = x[torch.from_numpy(done).to(x.device)]
        d2 = (torch.view_as_real(nxt - x) ** 2).sum(dim=(1, 2)).cpu().numpy()
        n2 = (torch.view_as_real(nxt) ** 2).sum(dim=(1, 2)).cpu().numpy()
        ratios.append(np.where(done, np.nan, d2 / n2))
        used += ~done
        done = done | (~done & (d2 <= tol * tol * n2))
        x = nxt.contiguous()
        images.append(x.cpu().numpy())
    return np.stack(images), used, np.array(ratios)


def test_inpaint_regions_equals_the_torch_composition():
    """tau = 0.05 max |A x*|, tol = 1e-6, 60 iterations: the background slot freezes, the blob's slot does not; the images
    agree bit for bit at every iteration looked at (no ratio lies within the sum bound of tol^2, asserted, so both routes
    freeze at the same iteration); the frozen slot's image and iters_used stop changing and the other's do not; graph
    replay and eager stepping give the same bits"""
    from pxmcmc_amd.uncertainty import inpaint_regions, inpaint_sum_depth

    op, reg, p, X = _identity_e2e()
    labels, tol, iters = _two_regions(), 1e-6, 60
    tau = _tau(op, X, 0.05)
    images, used, ratios = _composed(op, X, labels, tau, iters, tol)
    bound = (inpaint_sum_depth(labels.size) + TERM_ROUNDINGS) * U
    live = np.isfinite(ratios) & (ratios > 0)
    assert (np.abs(ratios[live] / tol ** 2 - 1.0) > 4 * bound + 1e-12).all()  # (the host's norms: numpy's order, ~1e-13)
    print(f"composed: iterations used {used}, last ratios {np.sqrt(ratios[-1])}; closest ratio / tol^2 - 1: "
          f"{np.abs(ratios[live] / tol ** 2 - 1.0).min():.2e}")
    assert used[0] == iters and 2 <= used[1] < 30  # the blob's slot never freezes, the background slot does
    for t in (1, 2, 3, int(used[1]) - 1, int(used[1]), int(used[1]) + 2, 59, 60):
        res = inpaint_regions(op, X, labels, tau, iters=t, tol=tol, batch=2, use_graph=t == 60)
        assert np.array_equal(res.images.cpu().numpy().view(np.int64), images[t].view(np.int64)), t
        assert np.array_equal(res.iters_used, np.minimum(used, t)), (t, res.iters_used)
        assert res.frozen.tolist() == [False, t >= used[1]]
        assert res.replayed == (t == 60) and res.graph_error is None
    eager = inpaint_regions(op, X, labels, tau, iters=iters, tol=tol, batch=2, use_graph=False)
    assert (_bits(eager.images) == _bits(res.images)).all() and np.array_equal(eager.rel_change, res.rel_change)
    assert res.rel_change[0] == pytest.approx(1.5e-4, rel=0.5) and res.rel_change[1] <= tol  # (1.5e-4: the host test's figure)
    # the frozen slot stopped changing, the other did not
    assert np.array_equal(images[used[1]][1], images[-1][1]) and not np.array_equal(images[used[1]][0], images[-1][0])
    outside = labels.reshape(-1) != 0
    assert np.array_equal(images[-1][0][outside], images[0][0][outside])  # outside D: x* bit for bit


def test_inpaint_regions_freezes_and_does_not_depend_on_the_batch():
    """tau = 0.2 max |A x*|: the blob's slot freezes (the host test: after 14 iterations); 8 regions in batches of 3 (ragged)
    and of 8, and by graph replay and eagerly: identical bits"""
    from pxmcmc_amd.uncertainty import inpaint_regions, superpixel_regions

    op, reg, p, X = _identity_e2e()
    tau = _tau(op, X, 0.2)
    two = inpaint_regions(op, X, _two_regions(), tau, iters=60, tol=1e-6, batch=2)
    host = decision_np(*planted(5), BLOB_REGION, 0.2)["inpaint"]
    print(f"tau = 0.2 max: iterations used {two.iters_used} (host: {host['iters_used']}), rel. change {two.rel_change}")
    assert two.frozen.all() and abs(int(two.iters_used[0]) - host["iters_used"]) <= 1 and (two.rel_change <= 1e-6).all()
    labels = superpixel_regions(L16, 8)  # 2 x 4 = 8 regions
    r3 = inpaint_regions(op, X, labels, tau, iters=9, tol=1e-3, batch=3)
    r8 = inpaint_regions(op, X, labels, tau, iters=9, tol=1e-3, batch=8)
    e3 = inpaint_regions(op, X, labels, tau, iters=9, tol=1e-3, batch=3, use_graph=False)
    assert r3.replayed and r8.replayed and not e3.replayed
    for other in (r8, e3):
        assert (_bits(r3.images) == _bits(other.images)).all()
        assert np.array_equal(r3.iters_used, other.iters_used) and np.array_equal(r3.rel_change, other.rel_change)
    assert r3.images.shape == (8, labels.size) and r3.iters_used.min() >= 2
    lab = labels.copy()
    lab[lab == 2] = 5
    with pytest.raises(ValueError, match="region 2 has no pixel"):
        inpaint_regions(op, X, lab, tau)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _path_instances(op, reg, p, X, images, x_map):
    """per region the instance (a, b, T, q, lmda) of the path as the device forms it, r + s and the linearity defect
    forward(X* + b) - (forward(X*) + forward(b)) -> list of dicts, and the device's F(X* + b)"""
    from pxmcmc_amd import ops
    from pxmcmc_amd.uncertainty import lci_terms_np, map_objective
    from pxmcmc_amd.uncertainty.regions import _lci_preds, _lci_weights

    tr = op.transform
    Xd = ops.as_device(np.asarray(X).astype(complex))
    w = _lci_weights(op).cpu().numpy()
    T = np.asarray(reg.T)
    insts, direct = [], []
    for r0 in range(0, images.shape[0], 3):
        b = ops.as_device(tr.forward(images[r0 : r0 + 3] - x_map[None]))
        a = Xd[None].expand(b.shape[0], -1).contiguous()
        pa, d = _lci_preds(op, a)
        pb, _ = _lci_preds(op, b)
        pab, _ = _lci_preds(op, a + b)
        direct.append(map_objective(op, reg, p, a + b).cpu().numpy())
        for c in range(b.shape[0]):
            rr, ss = (pa[c] - d).cpu().numpy(), pb[c].cpu().numpy()
            q, _, _ = lci_terms_np(a[c].cpu().numpy(), b[c].cpu().numpy(), rr, ss, w, T)
            e = np.abs((pab[c] - pa[c] - pb[c]).cpu().numpy())
            insts.append(dict(a=a[c].cpu().numpy(), b=b[c].cpu().numpy(), T=T, q=np.array(q, dtype=np.float64), lmda=LMDA,
                              n=a.shape[1], qmag=float(0.5 * (w * (np.abs(rr) + np.abs(ss)) ** 2).sum()),
                              defect=float((w * (np.abs(rr + ss) * e + 0.5 * e * e)).sum())))
    return insts, np.concatenate(direct)


def _check_result(op, reg, p, X, res, sur, rounds_ok=True):
    """F_sgt = map_objective(X* + b) and profile[0] = F(X*) to the LCI error model; the end-point properties of removable"""
    from pxmcmc_amd.uncertainty import lci_sum_depth, map_objective

    n_any = max(op.nparams, int(op.data_dev.numel()))  # a chain of additions no summation order exceeds
    depth = lci_sum_depth(n_any)
    F_map = float(map_objective(op, reg, p, X).cpu().numpy()[0])
    insts, direct = _path_instances(op, reg, p, X, sur.images, sur.x_map)
    gamma = LD(res.threshold)
    worst = 0.0
    for r, inst in enumerate(insts):
        # both routes also sum the data terms: (chain + roundings of a term) U sum |terms| each, sum |terms| <= qmag
        sums = (depth + n_any + 12) * U * inst["qmag"]
        tol1 = f_tol(inst, 1.0, depth) + f_tol(inst, 1.0, n_any) + sums + inst["defect"]
        assert inst["defect"] <= 1e-9 * abs(res.threshold), (r, inst["defect"])  # (the defect is round-off)
        assert abs(res.f_sgt[r] - direct[r]) <= tol1, (r, res.f_sgt[r], direct[r], tol1)
        tol0 = f_tol(inst, 0.0, depth) + f_tol(inst, 0.0, n_any) + sums
        assert abs(res.profile[r, 0] - F_map) <= tol0, (r, res.profile[r, 0], F_map, tol0)
        worst = max(worst, abs(res.f_sgt[r] - direct[r]) / tol1, abs(res.profile[r, 0] - F_map) / tol0)
        assert res.f_sgt[r] == res.profile[r, -1] and bool(res.physical[r]) == bool(res.f_sgt[r] > res.threshold)
        assert (res.removable[r] < 1.0) == bool(res.physical[r]), (r, res.removable[r], res.physical[r])
        if res.status[r] == 0:  # F <= gamma at xi+, F >= gamma one final width beyond it; xi- <= 0 <= xi+
            x = res.removable[r]
            assert res.lower[r] <= 0.0 <= x
            assert F_ld(inst, x) <= gamma + f_tol(inst, x, depth), (r, x)
            assert F_ld(inst, x + res.width[r]) >= gamma - f_tol(inst, x + res.width[r], depth), (r, x)
    return worst


def test_hypothesis_test_identity_matches_the_host_decisions():
    """the planted blob: physical at both thresholds with the host test's margin, the background inconclusive; every one
    of the 32 superpixels obeys the error model and the end-point properties"""
    from pxmcmc_amd.uncertainty import hypothesis_test, inpaint_regions, superpixel_regions

    op, reg, p, X = _identity_e2e()
    labels = superpixel_regions(L16, SIZE)
    for frac in (0.2, 0.05):
        tau = _tau(op, X, frac)
        res = hypothesis_test(op, reg, p, X, labels, tau=tau, iters=60, batch=3)
        assert res.physical.shape == (32,) and res.physical.dtype == bool and res.profile.shape == (32, 32)
        assert (res.status & ~3 == 0).all(), res.status  # nothing non-finite
        units = (res.f_sgt - res.threshold) / (res.threshold - res.profile[:, 0])
        for region in (BLOB_REGION, BACKGROUND_REGION):
            host = decision_np(*planted(5), region, frac)
            print(f"tau {frac} max, region {region}: device {units[region]:.2f}, host {host['units']:.2f} (gamma - F*); removable "
                  f"{res.removable[region]:.4f} / {host['removable']:.4f}; iterations {res.iters_used[region]}")
            assert bool(res.physical[region]) == host["physical"] == (region == BLOB_REGION)
            assert (units[region] >= 1.0) if host["physical"] else (units[region] <= -0.5)
        sur = inpaint_regions(op, X, labels, tau, iters=60, batch=3)
        assert np.array_equal(sur.iters_used, res.iters_used) and np.array_equal(sur.rel_change, res.rel_change)
        worst = _check_result(op, reg, p, X, res, sur)
        print(f"tau {frac} max: {int(res.physical.sum())} of 32 physical; largest |F - direct| / bound {worst:.3f}")
    painted = res.to_map()
    assert painted.shape == labels.shape and painted[labels == BLOB_REGION].min() == 1.0 and painted[0, 0] == 0.0


def test_hypothesis_test_weaklensing():
    """masked weak lensing: finite statuses, a boolean decision per region, the error model and the end-point properties;
    the regions inside the masked band are inconclusive"""
    from pxmcmc_amd.uncertainty import HYP_NONFINITE, LCI_NONFINITE, hypothesis_test, inpaint_regions, superpixel_regions
    from pxmcmc_amd.utils import build_mask

    op, reg, p, X = _e2e("weaklensing")
    labels = superpixel_regions(L16, SIZE)
    tau = _tau(op, X, 0.1)
    res = hypothesis_test(op, reg, p, X, labels, tau=tau, iters=20, batch=3)
    assert res.physical.shape == (32,) and res.physical.dtype == bool
    assert (res.status & (HYP_NONFINITE | LCI_NONFINITE) == 0).all() and np.isfinite(res.profile).all()
    mask = build_mask(L16, size=20.0)
    masked = np.array([not mask[labels == r].any() for r in range(32)])
    assert masked.any() and not res.physical[masked].any()
    sur = inpaint_regions(op, X, labels, tau, iters=20, batch=3)
    worst = _check_result(op, reg, p, X, res, sur)
    print(f"weak lensing: tau {tau:.3e}, {int(res.physical.sum())} of 32 physical, {int(masked.sum())} regions masked; "
          f"largest |F - direct| / bound {worst:.3f}")


def test_smooth_surrogate_and_refusals():
    """surrogate='smooth': outside D untouched, inside D the ShtPlan smoothing bit for bit; sigma = 0 leaves x* (b = 0:
    inconclusive, not an error); the refusals of the setup"""
    import torch

    from pxmcmc_amd import ops
    from pxmcmc_amd.forward import SphericalWaveletTransformOperator
    from pxmcmc_amd.uncertainty import gaussian_smooth, hypothesis_test, smooth_regions, superpixel_regions

    op, reg, p, X = _identity_e2e()
    labels = superpixel_regions(L16, SIZE)
    flat = labels.reshape(-1)
    sigma = 0.3
    sur = smooth_regions(op, X, labels, sigma, batch=3)
    x_map = sur.x_map
    plan = ops.ShtPlan(L16, 0)
    el = np.repeat(np.arange(L16), 2 * np.arange(L16) + 1).astype(np.float64)
    want = plan.inverse(plan.forward(x_map) * ops.as_device(np.exp(-el * (el + 1.0) * sigma ** 2 / 2.0)))
    assert (_bits(want) == _bits(gaussian_smooth(x_map, L16, sigma))).all() and not torch.equal(want, x_map)
    img, xm, sm = sur.images.cpu().numpy(), x_map.cpu().numpy(), want.cpu().numpy()
    for r in range(32):
        inside = flat == r
        assert np.array_equal(img[r][~inside], xm[~inside]) and np.array_equal(img[r][inside], sm[inside])
    assert (sur.iters_used == 1).all()
    res = hypothesis_test(op, reg, p, X, labels, sigma=sigma, surrogate="smooth", batch=3)
    worst = _check_result(op, reg, p, X, res, sur)
    print(f"smooth: {int(res.physical.sum())} of 32 physical, F_sgt - gamma of the blob "
          f"{res.f_sgt[BLOB_REGION] - res.threshold:.3f}; largest |F - direct| / bound {worst:.3f}")
    same = hypothesis_test(op, reg, p, X, labels, sigma=0.0, surrogate="smooth", batch=8)
    assert not same.physical.any() and (same.removable >= 1.0).all() and (same.rel_change < 1e-12).all()
    for bad in (dict(tau=0.1, sigma=0.1), dict(), dict(sigma=0.1), dict(tau=0.1, surrogate="smooth"), dict(tau=0.1, surrogate="other"),
                dict(tau=-1.0), dict(tau=0.1, rounds=0), dict(tau=0.1, iters=0)):
        with pytest.raises(ValueError):
            hypothesis_test(op, reg, p, X, labels, **bad)
    analysis = SphericalWaveletTransformOperator(planted_data(planted(5)[0], 5), SIG, "analysis", L16, B16, JMIN16)
    with pytest.raises(ValueError, match="synthesis setting"):
        hypothesis_test(analysis, reg, p, np.zeros(L16 * (2 * L16 - 1)), labels, tau=0.1)
    with pytest.raises(ValueError):
        hypothesis_test(op, reg, p, X, labels.astype(float), tau=0.1)


def test_example_writes_the_maps(tmp_path, capsys):
    """examples/topography_synthetic.py --map-start --hyp-test 4 at L = 16: both maps are written and painted per region"""
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("topography_synthetic", os.path.join(root, "examples", "topography_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(["--L", "16", "--nsamples", "2", "--ngap", "2", "--map-start", "--hyp-test", "4", "--outdir", str(tmp_path)])
    assert "hypothesis tests: " in capsys.readouterr().out
    phys = np.load(tmp_path / "myula_synthesis_0_hyp_physical.npy")
    rem = np.load(tmp_path / "myula_synthesis_0_hyp_removable.npy")
    assert phys.shape == rem.shape == (16, 31) and np.isin(phys, (0.0, 1.0)).all()
    assert (phys[:4, :4] == phys[0, 0]).all() and (rem[:4, :4] == rem[0, 0]).all()
    assert ((rem < 1.0) == (phys == 1.0)).all()
    with pytest.raises(SystemExit):
        mod.main(["--L", "16", "--hyp-test", "4", "--outdir", str(tmp_path)])  # needs --map-start
