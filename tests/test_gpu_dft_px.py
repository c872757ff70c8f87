"""The global-memory side of every phi-DFT unit on a DFT-only plan (ops.DftPlan.rings_raw_ex / pixels_raw_ex): the pixel-side
functors of csrc/update.h (residual with a real or complex inverse covariance, scatter / gather through a pixel -> data map, its
weight), the narrow ring arrays of the weak-lensing attachment (2, 4, 6, 8 doubles per row) and an image inside a longer chain
(ring0 != 0, chain_stride > L (2L-1)) -- one case per kernel body (PX_CASES of tests/test_dft_host.py).

No tolerance: all of that arithmetic is elementwise and outside the transform, so every launch is held to BIT equality with
the plain launch (rings_raw / pixels_raw, which tests/test_gpu_dft.py holds to the long-double model) of an image computed
with torch.
  * real inverse covariance and weight: the device rounds three times -- the difference, one product per component with
    invcov, one with gw; nothing for a multiply-add to contract.  The test forms the same three roundings on the real views.
  * complex inverse covariance: the device's complex product may contract to fused multiply-adds, so the inputs are integers
    for which every intermediate is exact in any order (test_dft_host.test_integer_residual_inputs_are_exact_in_float64).
Everything a launch must not touch holds a sentinel (a NaN with a payload, compared as int64): entries of the data vector no
pixel maps to, the elements of a chain around the image, 4112 bytes on either side of a narrow ring array.  Only the round
trip through the mask has a bound, the one test_gpu_dft.test_round_trip_and_dot derives.
"""
import functools

import numpy as np
import pytest
from test_dft_host import PX_CASES, PX_CHAINS, PX_EXTRA, case_id, dense, px_index_map, px_integer_inputs_of, px_mask
from test_gpu_dft import ONE_PER_UNIT, _bits, _plan, round_trip_taus

pytestmark = pytest.mark.gpu

CMAX, CS = PX_CHAINS, (1, 3, 5)  # the wide array: ncol = 16
NARROW = ((2, 1), (4, 1), (4, 2), (6, 3), (8, 3), (8, 4))  # (ncol, C)
SCATTER_VARIANTS = ("res-real", "res-cplx", "gidx", "gidx-gw", "gidx-res-real-gw", "gidx-res-cplx-gw")
SENTINEL = 0x7FF8DEADBEEF0001  # a quiet NaN with a payload: nothing computes it, and a launch that reads it shows
GUARD = 257  # complex elements on either side of a narrow ring array: 4112 bytes, the view 16-byte (and no better) aligned
RING0, TAIL = 37, 11  # an image inside a longer chain: elements before and after it
PFA0 = ("pair8", 256, {"PXM_DFT_PFA": "0"})


# ---- inputs: built once per L on the host ------------------------------------------------------------------------------------------------
def _real_inputs(seed, N):
    """f [CMAX, N], data [N] complex, invcov [N] and gw [N] real: arbitrary doubles (invcov of either sign)"""
    rng = np.random.default_rng(seed)
    cplx = lambda *shape: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return cplx(CMAX, N), cplx(N), rng.uniform(0.5, 2.0, N) * rng.choice([-1.0, 1.0], N), rng.uniform(0.5, 2.0, N)


@functools.lru_cache(maxsize=None)
def _host(L):
    """space None: pixel space; 0 / PX_EXTRA: the data space of px_index_map(L, extra)"""
    P = L * (2 * L - 1)
    h = {"kept": np.flatnonzero(px_mask(L).reshape(-1))}
    for k, space in enumerate((None, 0, PX_EXTRA)):
        gidx, N = (None, P) if space is None else px_index_map(L, space)
        h[space] = {"gidx": gidx, "N": N, "real": _real_inputs(9300 + 16 * L + k, N), "int": px_integer_inputs_of(L, space)}
    return h


def _dev(x):
    import torch

    return None if x is None else torch.from_numpy(np.array(x)).cuda()  # (a copy: the cached host arrays are read-only)


def _side(L, space, kind):
    """device tensors of one input set: f [CMAX, N], data [N], invcov [N] (real for kind 'real', complex for 'int'), gw [N],
    gidx int32 [P] or None, and the kept pixels with the entries they map to (int64)"""
    h = _host(L)
    f, d, w, gw = (_dev(a) for a in h[space][kind])
    kept = _dev(h["kept"])
    gidx = _dev(h[space]["gidx"])
    return f, d, w, gw, gidx, kept, (None if gidx is None else gidx[kept].long())


def _sentinel(*shape, real=False):
    import torch

    n = int(np.prod(shape)) * (1 if real else 2)
    t = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda").view(torch.float64)
    return t.view(shape) if real else torch.view_as_complex(t.view(-1, 2)).view(shape)


def _raw_bits(t):
    import torch

    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int64)


def _same_bits(a, b):
    """equal as bit patterns (sentinels included)"""
    import torch

    return a.shape == b.shape and torch.equal(_raw_bits(a), _raw_bits(b))


def _all_sentinel(t):
    return bool((_raw_bits(t) == SENTINEL).all())


def _junk(seed, *shape):
    """finite O(1) values"""
    import torch

    gen = torch.Generator().manual_seed(seed)
    return torch.view_as_complex(torch.rand(*shape, 2, dtype=torch.float64, generator=gen) + 0.5).cuda()


# ---- what the device computes, rounding by rounding ----------------------------------------------------------------------------------------
def _times_real(x, w):
    """one real multiplication per component"""
    import torch

    return torch.view_as_complex(torch.view_as_real(x) * w[:, None])


def _pixel_values(f, d=None, w=None, gw=None):
    """gw .* (w .* (f - d)) along the last axis: the difference, then one product per component with a real w (complex w:
    integer inputs, exact in any order), then one with gw"""
    x = f
    if d is not None:
        r = x - d
        x = w * r if w.is_complex() else _times_real(r, w)
    return x if gw is None else _times_real(x, gw)


def _image(x, kept, src, L):
    """[C, N] values -> the plain image [C, L, 2L-1]: pixel kept[i] holds entry src[i], masked pixels zero (src None: x is
    the image)"""
    import torch

    n = 2 * L - 1
    if src is None:
        return x.reshape(x.shape[0], L, n).contiguous()
    E = torch.zeros((x.shape[0], L * n), dtype=x.dtype, device=x.device)
    E[:, kept] = x[:, src]
    return E.view(x.shape[0], L, n)


def _check_ring_array(G, want, fill, L, C, what):
    """chains c < C as in the plain launch, columns c >= C of the rows t < L zero, rows t >= L as the array held them"""
    import torch

    assert _bits(G[:, :L, :C].contiguous(), want[:, :L, :C].contiguous()), what
    assert bool((torch.view_as_real(G[:, :L, C:]) == 0).all()), what
    if G.shape[1] > L:
        assert _same_bits(G[:, L:, :], fill[:, L:, :]), what


def _variant(v):
    return "gidx" in v, ("real" if "res-real" in v else "int" if "res-cplx" in v else None), "gw" in v


# ---- check 1: scatter / residual side on the wide array -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", SCATTER_VARIANTS)
@pytest.mark.parametrize("case", PX_CASES, ids=case_id)
def test_scatter_and_residual_equal_the_plain_launch(case, variant, monkeypatch):
    """rings_raw_ex of f (data space with a map) with residual and weight == rings_raw of the image torch forms from the same
    arrays, bit for bit, for 1, 3 and 5 chains, into a zeroed array and into one of finite garbage; with a map, for a data
    vector of exactly the kept pixels and for one with PX_EXTRA entries nothing maps to (never read: they change no bit)."""
    _, L, _ = case
    n = 2 * L - 1
    use_map, res, use_gw = _variant(variant)
    plan, _ = _plan(monkeypatch, case, CMAX)
    junk = _junk(L, n, plan.Rp, plan.Cp)
    zero = plan.ring_array()
    for space in ((0, PX_EXTRA) if use_map else (None,)):
        f, d, w, gw, gidx, kept, src = _side(L, space, res or "real")
        d, w = (d, w) if res else (None, None)
        gw = gw if use_gw else None
        E = _image(_pixel_values(f, d, w, gw), kept, src, L)
        for C in CS:
            want = plan.rings_raw(E[:C], plan.ring_array())
            for fill in (zero, junk):
                G = plan.rings_raw_ex(f[:C], fill.clone(), data=d, invcov=w, gidx=gidx, gw=gw)
                _check_ring_array(G, want, fill, L, C, (case_id(case), variant, space, C, fill is junk))
    assert plan.status() == 0


# ---- check 2: gather side --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PX_CASES, ids=case_id)
def test_gather_equals_the_plain_launch(case, monkeypatch):
    """pixels_raw_ex through the map: entry gidx[e] of chain c holds pixel e of pixels_raw (times gw[gidx[e]], one real
    multiplication per component) bit for bit; every other bit of the sentinel-filled output -- the PX_EXTRA entries no pixel
    maps to, and nothing else, since the map is injective -- stays."""
    import torch

    _, L, _ = case
    n = 2 * L - 1
    plan, _ = _plan(monkeypatch, case, CMAX)
    g = _dev(dense(5000 + L, CMAX, L, n))
    for space in (0, PX_EXTRA):
        _, _, _, gw, gidx, kept, src = _side(L, space, "real")
        N = gw.numel()
        referenced = torch.zeros(N, dtype=torch.bool, device="cuda")
        referenced[src] = True
        assert int(referenced.sum()) == N - space == kept.numel()
        for C in CS:
            raw = plan.ring_array()
            raw[:, :L, :C] = g[:C].permute(2, 1, 0)
            ref = plan.pixels_raw(raw, C).reshape(C, L * n)[:, kept]
            for w in (None, gw):
                out = plan.pixels_raw_ex(raw, _sentinel(C, N), gidx=gidx, gw=w)
                want = _sentinel(C, N)
                want[:, src] = ref if w is None else _times_real(ref, w[src])
                assert _same_bits(out, want), (case_id(case), space, C, w is not None)
                assert _all_sentinel(out[:, ~referenced]) and not bool(torch.isnan(torch.view_as_real(out[:, referenced])).any())
    assert plan.status() == 0


# ---- check 3: narrow ring arrays -------------------------------------------------------------------------------------------------------------
def _guarded(fill):
    """fill [n, Rp, Cp] -> (buffer, view): the ring array as a view in the middle of a sentinel-filled buffer"""
    size = fill.numel()
    buf = _sentinel(GUARD + size + GUARD)
    view = buf[GUARD:GUARD + size].view(fill.shape)
    view.copy_(fill)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0 and GUARD * 16 >= 4096
    return buf, view


def _guards_intact(buf):
    return _all_sentinel(buf[:GUARD]) and _all_sentinel(buf[-GUARD:])


@pytest.mark.parametrize("ncol,C", NARROW, ids=[f"ncol{a}-C{b}" for a, b in NARROW])
@pytest.mark.parametrize("case", PX_CASES, ids=case_id)
def test_narrow_ring_arrays(case, ncol, C, monkeypatch):
    """Ring arrays of 2, 4, 6 and 8 doubles per row, both directions, plain and through map and weight: chain c has the bits of
    the wide launch, padding columns and rows behave as on the wide array, and no bit outside the array changes.  The
    exact-length unit takes the Bluestein body of the pair unit below 8 doubles per row: there its reference is the wide launch
    of a plan created with PXM_DFT_PFA=0, which differs in bits from the exact-length plan's own -- so the comparison shows
    which body ran."""
    unit, L, _ = case
    n, Cp = 2 * L - 1, ncol // 2
    plan, _ = _plan(monkeypatch, case, CMAX)
    other = _plan(monkeypatch, PFA0, CMAX)[0] if unit == "exact" else None
    ref_plan = other if other is not None and ncol < 8 else plan
    not_ref = plan if ref_plan is other else other  # exact-length case: the plan of the body that must NOT have run
    f, _, _, _, _, kept, _ = _side(L, None, "real")
    y, _, _, gw, gidx, _, src = _side(L, PX_EXTRA, "real")
    N = gw.numel()
    junk = _junk(L + ncol, n, plan.Rp, Cp)
    g = _dev(dense(5000 + L, CMAX, L, n))[:C]
    # pixels -> rings
    for name, x, E, kw in (("plain", f, _image(f[:C], kept, None, L), {}),
                           ("map", y, _image(_pixel_values(y[:C], gw=gw), kept, src, L), dict(gidx=gidx, gw=gw))):
        want = ref_plan.rings_raw(E, ref_plan.ring_array())
        if other is not None:  # the two bodies do not agree in bits: the comparison below tells them apart
            assert not _bits(want[:, :L, :C].contiguous(), not_ref.rings_raw(E, plan.ring_array())[:, :L, :C].contiguous())
        for fill in (junk.new_zeros(junk.shape), junk):
            buf, view = _guarded(fill)
            plan.rings_raw_ex(x[:C], view, **kw)
            _check_ring_array(view, want, fill, L, C, (case_id(case), ncol, C, name, fill is junk))
            assert _guards_intact(buf), (case_id(case), ncol, C, name)
    # rings -> pixels: padding rows and columns of the array hold garbage
    buf, view = _guarded(junk)
    view[:, :L, :C] = g.permute(2, 1, 0)
    raw = ref_plan.ring_array()
    raw[:, :L, :C] = g.permute(2, 1, 0)
    ref = ref_plan.pixels_raw(raw, C).reshape(C, L * n)
    if other is not None:
        assert not _bits(ref, not_ref.pixels_raw(raw, C).reshape(C, L * n))
    assert _same_bits(plan.pixels_raw_ex(view, _sentinel(C, L * n)), ref), (case_id(case), ncol, C, "plain")
    want = _sentinel(C, N)
    want[:, src] = _times_real(ref[:, kept], gw[src])
    assert _same_bits(plan.pixels_raw_ex(view, _sentinel(C, N), gidx=gidx, gw=gw), want), (case_id(case), ncol, C, "map")
    assert _guards_intact(buf)
    assert plan.status() == 0 and (other is None or other.status() == 0)


# ---- check 4: an image inside a longer chain -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PX_CASES, ids=case_id)
def test_image_inside_a_longer_chain(case, monkeypatch):
    """ring0 = 37 and chains 37 + L (2L-1) + 11 apart, sentinels around the image (in f, data and invcov alike: a launch that
    read one would carry a NaN into a ring): the rings are those of the bare image, plain and with the pixel-space residual;
    on the way back the image region is pixels_raw and the 48 other elements of every chain keep every bit."""
    _, L, _ = case
    n, C = 2 * L - 1, 3
    P = L * n
    stride = RING0 + P + TAIL
    plan, _ = _plan(monkeypatch, case, CMAX)
    junk = _junk(L, n, plan.Rp, plan.Cp)

    def inside(x):
        """x [.., P] -> [.., stride] with sentinels around it"""
        long = _sentinel(*x.shape[:-1], stride, real=not x.is_complex())
        long[..., RING0:RING0 + P] = x
        return long

    for kind, res in (("real", False), ("real", True), ("int", True)):
        f, d, w, _, _, kept, _ = _side(L, None, kind)
        d, w = (d, w) if res else (None, None)
        want = plan.rings_raw(_image(_pixel_values(f[:C], d, w), kept, None, L), plan.ring_array())
        for fill in (plan.ring_array(), junk):
            G = plan.rings_raw_ex(inside(f[:C]), fill.clone(), ring0=RING0, data=None if d is None else inside(d),
                                  invcov=None if w is None else inside(w))
            _check_ring_array(G, want, fill, L, C, (case_id(case), kind, res, fill is junk))
    raw = junk.clone()
    raw[:, :L, :C] = _dev(dense(5000 + L, C, L, n)).permute(2, 1, 0)
    out = plan.pixels_raw_ex(raw, _sentinel(C, stride), ring0=RING0)
    assert _same_bits(out[:, RING0:RING0 + P], plan.pixels_raw(raw, C).reshape(C, P)), case_id(case)
    assert _all_sentinel(out[:, :RING0]) and _all_sentinel(out[:, RING0 + P:]), case_id(case)
    assert plan.status() == 0


# ---- check 5: round trip through the mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ONE_PER_UNIT, ids=case_id)
def test_round_trip_through_the_mask(case, monkeypatch):
    """gather(pixels(rings(scatter(y)))) = n y on the entries a pixel maps to, within the bound of
    test_gpu_dft.test_round_trip_and_dot for the scattered image: n (tau_f + tau_i) ||ring||_2 per element of a ring, tau = 4 eps
    x the model's measured ratio per direction."""
    _, L, _ = case
    n, C = 2 * L - 1, 3
    plan, _ = _plan(monkeypatch, case, CMAX)
    h = _host(L)
    for space in (0, PX_EXTRA):
        y = h[space]["real"][0][:C]
        kept, src = h["kept"], h[space]["gidx"][h["kept"]]
        E = np.zeros((C, L * n), dtype=complex)
        E[:, kept] = y[:, src]
        E = E.reshape(C, L, n)
        tau_f, tau_i = round_trip_taus(case, E, dense(8000 + L, C, L, n))
        gidx = _dev(h[space]["gidx"])
        G = plan.rings_raw_ex(_dev(y), plan.ring_array(), gidx=gidx)
        out = plan.pixels_raw_ex(G, _sentinel(C, y.shape[1]), gidx=gidx)
        rest = np.setdiff1d(np.arange(y.shape[1]), src)
        assert len(rest) == space and _all_sentinel(out[:, _dev(rest)])
        back = np.zeros((C, L * n), dtype=complex)
        back[:, kept] = out.cpu().numpy()[:, src]
        err = np.abs(back.reshape(C, L, n) - n * E).max(axis=-1)
        bound = n * (tau_f + tau_i) * np.linalg.norm(E, axis=-1)
        assert (err <= bound).all(), (case_id(case), space, (err / np.maximum(bound, 1e-300)).max())
    assert plan.status() == 0
