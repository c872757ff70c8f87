"""
The numpy statement of the Gibbs sampler on the sparse posterior (:class:`pxmcmc_amd.optim.LassoGibbs`, csrc/lasso.hip;
DESIGN.md section 25): the posterior of the L1 prior itself,

    p(x | d) ~ exp(-F(x)),   F(x) = 1/2 Re L2(x) + sum_i t_i |x_i|,   t_i = T_i / lmda,

sampled exactly by data augmentation (Park & Casella 2008; Kyung et al. 2010 for the group form).  The Laplace prior is a
Gaussian scale mixture (Andrews & Mallows 1974): with ``x`` one coefficient seen as ``m`` real numbers (1: real state, 2:
complex state)

    exp(-t |x|)  ~  int N(x; 0, v I_m) Gamma(v; (m + 1) / 2, t^2 / 2) dv

so given the variances the field is Gaussian with per-element precision ``D_i = 1 / v_i`` -- the exact draw of
:class:`pxmcmc_amd.optim.GaussianPosterior` -- and given the field every precision is an independent inverse-Gaussian variate,

    D_i | x  ~  IG(mean = t_i / |x_i|, shape = t_i^2)            for m = 1 and m = 2 alike.

The draw is the transformation of Michael, Schucany & Haas (1976) multiplied through by its conjugate, so that nothing cancels
and nothing divides by ``|x|`` (:func:`precision_draw_np` gives the operation sequence; at ``x = 0`` it is the Levy limit
``t^2 / z^2``).  Its two deviates per element are a normal ``z`` and a uniform ``u``; where they come from on the device is
:func:`draw_iterations` and :func:`uniform_from_bits`.

Here: the draw in float64, operation by operation as the kernel does it (:func:`precision_draw_np`), in extended precision with
the forward-error bound of that operation sequence and the elements whose branch the bound cannot decide
(:func:`precision_draw_ld`), the setup checks (:func:`check_setup`), the initial precisions (:func:`initial_precision`), a
reference sampler on a dense ``Phi`` (:func:`lasso_sweep_np`, :func:`lasso_gibbs_np`), the separable identity model with its
posterior moments by quadrature (:func:`identity_lasso_gibbs_np`, :func:`identity_moments`) and the moments of the conditional
(:func:`inverse_gaussian_moments`).
"""
import numpy as np

from . import cg_np

EPS = cg_np.EPS
LD = np.longdouble
TINY = 2.0 ** -1074  # the spacing of the subnormal doubles: what a product or a quotient that underflows is off by at most

# The Philox iterations of the precision draw of sweep t: 2^60 + 2 t for the normals z, 2^60 + 2 t + 1 for the uniforms u --
# off the field draws (2 t, 2 t + 1), the variance draws of GaussianGibbs (2^61 + t) and the Hutchinson probes (2^62).
DRAW_ITER = 1 << 60


def draw_iterations(t):
    """the Philox iterations ``(it_z, it_u)`` of the precision draw of sweep ``t``; the launch takes ``it_z`` and owns both"""
    return DRAW_ITER + 2 * int(t), DRAW_ITER + 2 * int(t) + 1


def uniform_from_bits(words):
    """the uniform of a Philox block ``words`` (uint32 ``[..., 4]``, ``oracle.philox.philox4x32_10``): the first 52 bits ``a`` of
    words 1 and 0 as ``(a + 1/2) 2^-52``.  Exact (``2 a + 1 < 2^53``), in (0, 1)."""
    w = np.asarray(words).astype(np.uint64)
    a = ((w[..., 1] << np.uint64(32)) | w[..., 0]) >> np.uint64(12)
    return (a.astype(np.float64) + 0.5) * 2.0 ** -52


# ---- the setup -------------------------------------------------------------------------------------------------------------
def check_setup(n, T, lmda, precision_bounds, name="LassoGibbs"):
    """Everything the sampler's construction refuses that the host can see: a threshold ``T`` (a float or ``[n]``) that is not
    finite and positive, ``lmda`` likewise, and a clamp that is not a finite positive pair -> dict of ``t`` (``T / lmda``, a
    float or ``[n]``) and ``precision_bounds``"""
    T = np.asarray(T, dtype=float)
    if T.ndim > 1 or (T.ndim == 1 and T.size != n):
        raise ValueError(f"{name}: the threshold T is a float or one value per parameter ({n}), got shape {T.shape}")
    if not np.all(np.isfinite(T)) or np.any(T <= 0):
        raise ValueError(f"{name}: every threshold T_i must be finite and positive: the conditional of a precision is "
                         f"inverse-Gaussian with shape (T_i / lmda)^2, and T_i = 0 is a flat prior it cannot express")
    if not (np.isfinite(lmda) and lmda > 0):
        raise ValueError(f"{name}: lmda must be finite and positive")
    try:
        d_lo, d_hi = (float(v) for v in precision_bounds)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: precision_bounds is a pair (d_lo, d_hi)") from None
    if not (np.isfinite(d_lo) and np.isfinite(d_hi) and 0 < d_lo <= d_hi):
        raise ValueError(f"{name}: precision_bounds must be finite with 0 < d_lo <= d_hi")
    t = T / float(lmda)
    return dict(t=float(t) if t.ndim == 0 else t, precision_bounds=(d_lo, d_hi))


def initial_precision(t, complex_):
    """``D = t^2 / (m + 1)``: the reciprocal of the prior mean ``(m + 1) / t^2`` of the variance ``v``"""
    return np.asarray(t, dtype=float) ** 2 / (3.0 if complex_ else 2.0)


def inverse_gaussian_moments(t, ax):
    """``(E D, Var D, E 1/D)`` of ``IG(mean = t / |x|, shape = t^2)``: ``mu``, ``mu^3 / shape``, ``1 / mu + 1 / shape``"""
    t, ax = np.asarray(t, dtype=float), np.asarray(ax, dtype=float)
    mu = t / ax
    return mu, mu ** 3 / t ** 2, ax / t + 1.0 / t ** 2


# ---- the conditional draw --------------------------------------------------------------------------------------------------
def _abs(x):
    x = np.asarray(x)
    return np.sqrt(x.real * x.real + x.imag * x.imag) if np.iscomplexobj(x) else np.abs(x)


def precision_draw_np(x, t, z, u, h=0.0, d_lo=1e-30, d_hi=1e30):
    """The draw in float64, operation by operation as ``k_lasso_draw`` does it, for arrays of any one shape (``t``, ``h``
    broadcast): ``x`` the field (real or complex), ``t`` the scaled thresholds, ``z`` the normals, ``u`` the uniforms.

        rt = 1 / t;  a = |x| rt;  zt = z rt;  g = 0.5 (zt zt);  D1 = 1 / ((a + g) + sqrt(g (g + 2 a)))
        raw = D1  unless  u (1 + a D1) > 1,  then  1 / (a (a D1))

    -> dict of ``D`` (clamped), ``sqrtD``, ``Minv = 1 / (D + h)``, ``raw``, ``first`` (the branch), ``terms`` (``t |x|``, whose
    sum is the prior term) and ``clamped`` (the clamp changed the value)"""
    ax = _abs(x)
    t = np.broadcast_to(np.asarray(t, dtype=float), ax.shape)
    z, u = np.asarray(z, dtype=float), np.asarray(u, dtype=float)
    with np.errstate(all="ignore"):
        rt = 1.0 / t
        a, zt = ax * rt, z * rt
        g = 0.5 * (zt * zt)
        d1 = 1.0 / ((a + g) + np.sqrt(g * (g + 2.0 * a)))
        first = ~(u * (1.0 + a * d1) > 1.0)
        raw = np.where(first, d1, 1.0 / (a * (a * d1)))
        D = np.where(raw >= d_lo, raw, d_lo)  # fmax(raw, d_lo), a NaN giving d_lo, ...
        D = np.where(D <= d_hi, D, d_hi)  # ... then fmin(., d_hi)
        return dict(D=D, sqrtD=np.sqrt(D), Minv=1.0 / (D + h), raw=raw, first=first, terms=t * ax, clamped=D != raw)


def _sqrt_err(p, e):
    """how far the square root moves when its non-negative argument ``p`` moves by at most ``e`` (and stays non-negative):
    downwards ``e / (sqrt(p) + sqrt(p - e))`` for ``p >= e``; for ``p < e`` at most ``sqrt(p)`` down and ``sqrt(p + e) -
    sqrt(p)`` up, both below ``sqrt(e)``"""
    with np.errstate(divide="ignore", invalid="ignore"):
        big = p >= e
        down = e / np.where(big & (p > 0), np.sqrt(p) + np.sqrt(np.where(big, p - e, 0)), 1)
        return np.where(big, np.where(e > 0, down, 0), np.maximum(np.sqrt(p), np.sqrt(p + e) - np.sqrt(p)))


def _recip_err(v, e):
    """how far ``1 / v`` moves when ``v > 0`` moves by at most ``e``: ``e / (v (v - e))``; infinite once ``e >= v``"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(e < v, e / (v * np.where(e < v, v - e, 1)), np.inf)


def precision_draw_ld(x, t, z, u, h=0.0, d_lo=1e-30, d_hi=1e30, tscale=None):
    """:func:`precision_draw_np` in extended precision -> dict of ``D``, ``sqrtD``, ``Minv``, ``terms`` (float64 values of the
    extended-precision results), their bounds ``D_bound``, ``sqrtD_bound``, ``Minv_bound``, ``terms_bound``, ``first`` (the
    branch), ``branch_value`` and ``branch_bound`` (``u (1 + a D1)`` and the bound of its float64 evaluation), ``ambiguous``
    (``|branch_value - 1| <= branch_bound``: the float64 evaluation may take either branch, and the bounds of that element
    hold for the branch of ``first`` only), ``clamped`` and ``clamp_open`` (the bound does not decide whether the clamp
    binds; ``D`` is then within its bound either way).

    ``tscale``: ``t`` is then ``tscale * t`` with that product rounded, as the kernel forms it from ``T`` (one more rounding).

    The bound is the forward error of the float64 operation sequence, propagated operation by operation: a rounded operation
    adds ``2^-53`` of its result, an input error ``e`` moves a product ``p q`` by ``|p| e_q + |q| e_p``, a sum by the sum of the
    errors, a reciprocal ``1 / v`` by ``e / (v (v - e))`` and a square root by ``e / (sqrt(p) + sqrt(p - e))``; a product that
    may underflow adds one subnormal spacing ``2^-1074``, and ``re^2 + im^2`` of a complex element three of them.  Every
    quantity is non-negative, so no term cancels and no condition number enters.  One more unit on every result covers the
    second-order terms and this model's own rounding (``2^-64`` per operation).  No constant is fitted."""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    if cplx:
        s2 = x.real.astype(LD) ** 2 + x.imag.astype(LD) ** 2
        ax = np.sqrt(s2)
        # two rounded products and a rounded sum (each may underflow), then the root, one more rounding
        e_ax = _sqrt_err(s2, 2 * LD(EPS) * s2 + 3 * LD(TINY)) + LD(EPS) * ax
    else:
        ax = np.abs(x.astype(LD))
        e_ax = np.zeros(ax.shape, dtype=LD)
    t = np.broadcast_to(np.asarray(t, dtype=float), ax.shape).astype(LD)
    e_t = np.zeros(ax.shape, dtype=LD)
    if tscale is not None:
        t = LD(tscale) * t
        e_t = LD(EPS) * t
    z, u, E = np.asarray(z, dtype=float).astype(LD), np.asarray(u, dtype=float).astype(LD), LD(EPS)
    h = np.asarray(h, dtype=float).astype(LD)
    with np.errstate(all="ignore"):
        rt = 1 / t
        e_rt = _recip_err(t, e_t) + E * rt
        a = ax * rt
        e_a = ax * e_rt + rt * e_ax + E * a + LD(TINY)
        zt = z * rt
        e_zt = np.abs(z) * e_rt + E * np.abs(zt) + LD(TINY)
        g = LD(0.5) * zt * zt
        e_g = np.abs(zt) * e_zt + E * g + LD(TINY)  # d(zt^2 / 2) = zt d(zt); the halving is exact
        q = g + 2 * a
        e_q = e_g + 2 * e_a + E * q
        p = g * q
        e_p = g * e_q + q * e_g + E * p + LD(TINY)
        s = np.sqrt(p)
        e_s = _sqrt_err(p, e_p) + E * s
        ag = a + g
        den = ag + s
        e_den = (e_a + e_g + E * ag) + e_s + E * den
        d1 = 1 / den
        e_d1 = _recip_err(den, e_den) + E * d1
        m = a * d1
        e_m = a * e_d1 + d1 * e_a + E * m + LD(TINY)
        w = 1 + m
        e_w = e_m + E * w
        v = u * w
        e_v = u * e_w + E * v
        first = ~(v > 1)
        r = a * m
        e_r = a * e_m + m * e_a + E * r + LD(TINY)
        d2 = 1 / r
        e_d2 = _recip_err(r, e_r) + E * d2
        raw = np.where(first, d1, d2)
        e_raw = np.where(first, e_d1, e_d2) + E * raw  # (+ one unit: second order, and the model's own rounding)
        # (x = 0 and z = 0 exactly: the denominator is zero in either arithmetic and the first branch is infinite, exactly)
        e_raw = np.where(den == 0, 0, np.where(np.isnan(e_raw), np.inf, e_raw))
        # the clamp: a value the bound keeps on one side of a limit is that limit exactly; next to a limit either is allowed
        lo, hi = raw - e_raw, raw + e_raw
        above, below = lo >= d_hi, hi <= d_lo
        inside = (lo >= d_lo) & (hi <= d_hi)
        D = np.where(above, LD(d_hi), np.where(below, LD(d_lo), np.minimum(np.maximum(raw, LD(d_lo)), LD(d_hi))))
        e_D = np.where(above | below, 0, np.minimum(e_raw, LD(d_hi) - LD(d_lo)))
        sq = np.sqrt(D)
        e_sq = _sqrt_err(D, e_D) + 2 * E * sq
        Dh = D + h
        mi = 1 / Dh
        e_mi = _recip_err(Dh, e_D + E * Dh) + 2 * E * mi
        terms = t * ax
        e_terms = t * e_ax + ax * e_t + 2 * E * terms + LD(TINY)
    f = lambda v: np.asarray(v, dtype=float)  # noqa: E731
    return dict(D=f(D), sqrtD=f(sq), Minv=f(mi), terms=f(terms), D_bound=f(e_D), sqrtD_bound=f(e_sq), Minv_bound=f(e_mi),
                terms_bound=f(e_terms), first=first, branch_value=f(v), branch_bound=f(e_v), ambiguous=np.abs(v - 1) <= e_v,
                clamped=~((raw >= d_lo) & (raw <= d_hi)), clamp_open=~(above | below | inside))


def sums_ld(ld):
    """the two sums of the launch for one chain from :func:`precision_draw_ld` of its elements -> ``(prior_term, bound,
    clamped, clamped_slack)``: the bound of the prior term is ``N 2^-53 sum |term|`` for the additions (a term passes through
    at most N - 1 of them in the fixed order, and one unit more) plus the terms' own bounds; the count is exact up to the
    elements whose clamp the bound leaves open"""
    terms = ld["terms"].astype(LD).ravel()
    total = np.sum(terms)
    bound = terms.size * LD(EPS) * total + np.sum(ld["terms_bound"].astype(LD))
    return float(total), float(bound), int(np.count_nonzero(ld["clamped"] & ~ld["clamp_open"])), int(np.count_nonzero(ld["clamp_open"]))


# ---- the sampler on a dense Phi ----------------------------------------------------------------------------------------------
def lasso_sweep_np(Phi, w, data, t, D, omega1, omega2, z, u, d_lo, d_hi):
    """One sweep of one chain on the dense model ``data = Phi x + noise`` with data weights ``w``: the exact draw ``x | D, d``
    by perturbation-optimisation (:func:`cg_np.draw_rhs_np`, a dense solve) with the deviates ``omega1`` (data length) and
    ``omega2`` (state length), then ``D | x`` with the normals ``z`` and the uniforms ``u`` -> ``(x, D_new, H)``"""
    Phi = np.asarray(Phi)
    w = np.asarray(w, dtype=float)
    H = Phi.conj().T @ (w[:, None] * Phi) + np.diag(D)
    b0 = Phi.conj().T @ (w * np.asarray(data))
    x = np.linalg.solve(H, cg_np.draw_rhs_np(Phi, w, D, b0, omega1, omega2))
    return x, precision_draw_np(x, t, z, u, 0.0, d_lo, d_hi)["D"], H


def lasso_gibbs_np(Phi, w, data, t, nsweeps, nchains, deviates, D0=None, d_lo=1e-30, d_hi=1e30, complex_=None):
    """The sampler: ``nsweeps`` sweeps of ``nchains`` chains from the precisions ``D0`` (``[n]`` or ``[C, n]``; None:
    :func:`initial_precision`).  ``deviates(s, c)`` returns ``(omega1 [m], omega2 [n], z [n], u [n])`` of sweep s and chain c.
    -> ``(X [nsweeps, C, n], D [nsweeps, C, n])``: the field draws and the precisions after every sweep"""
    Phi = np.asarray(Phi)
    n = Phi.shape[1]
    cplx = (np.iscomplexobj(Phi) or np.iscomplexobj(data)) if complex_ is None else bool(complex_)
    tv = np.broadcast_to(np.asarray(t, dtype=float), (n,))
    cur = np.broadcast_to(initial_precision(tv, cplx) if D0 is None else np.asarray(D0, dtype=float), (nchains, n)).copy()
    X = np.zeros((nsweeps, nchains, n), dtype=complex if cplx else float)
    D = np.zeros((nsweeps, nchains, n))
    for s in range(nsweeps):
        for c in range(nchains):
            w1, w2, z, u = deviates(s, c)
            X[s, c], cur[c], _ = lasso_sweep_np(Phi, w, data, tv, cur[c], w1, w2, z, u, d_lo, d_hi)
        D[s] = cur
    return X, D


def identity_lasso_gibbs_np(data, noise_var, t, nsweeps, nchains, rng, d_lo=1e-30, d_hi=1e30):
    """:func:`lasso_gibbs_np` for the identity model ``d = x + noise`` (``Phi = I``, ``w = 1 / noise_var`` per real component;
    ``data`` real or complex ``[n]``), vectorised over the chains, the deviates from ``rng`` -> ``X [nsweeps, C, n]``"""
    d = np.asarray(data)
    cplx = np.iscomplexobj(d)
    n, w = d.size, 1.0 / float(noise_var)
    tv = np.broadcast_to(np.asarray(t, dtype=float), (n,))
    D = np.tile(initial_precision(tv, cplx), (nchains, 1))
    normal = (lambda: rng.standard_normal((nchains, n)) + 1j * rng.standard_normal((nchains, n))) if cplx else (
        lambda: rng.standard_normal((nchains, n)))
    X = np.zeros((nsweeps, nchains, n), dtype=d.dtype)
    for s in range(nsweeps):
        x = (w * d + np.sqrt(w) * normal() + np.sqrt(D) * normal()) / (w + D)
        D = precision_draw_np(x, tv, rng.standard_normal((nchains, n)), rng.uniform(size=(nchains, n)), 0.0, d_lo, d_hi)["D"]
        X[s] = x
    return X


# ---- the identity model's posterior moments by quadrature ------------------------------------------------------------------------
def identity_moments(d, noise_var, t, points=200001):
    """``(E x, E |x|^2)`` of one element of the identity model, ``p(x | d) ~ exp(-|x - d|^2 / (2 noise_var) - t |x|)``
    (``noise_var`` per real component), by the trapezoid rule.  Real ``d``: on ``x`` over ``d +- 12 sigma`` widened to hold 0.
    Complex ``d``: the density depends on the angle through ``Re conj(d) x`` only; the angle integrates to Bessel functions
    ``I_0``, ``I_1`` (scaled, ``scipy.special.ive``) and the radius is integrated, ``E x = (d / |d|) E[r I_1 / I_0]``."""
    sig = np.sqrt(noise_var)
    if not np.iscomplexobj(d):
        d = float(d)
        x = np.linspace(min(d, 0.0) - 12 * sig, max(d, 0.0) + 12 * sig, int(points))
        logp = -(x - d) ** 2 / (2 * noise_var) - t * np.abs(x)
        p = np.exp(logp - logp.max())
        return float(np.sum(p * x) / np.sum(p)), float(np.sum(p * x * x) / np.sum(p))
    from scipy.special import ive

    ad = abs(d)
    r = np.linspace(0.0, ad + 12 * sig, int(points))
    k = r * ad / noise_var
    # int exp(k cos phi) d phi = 2 pi I_0(k) = 2 pi ive(0, k) e^k; with the Gaussian: exp(-(r - |d|)^2 / (2 noise_var))
    logp = -(r - ad) ** 2 / (2 * noise_var) - t * r
    p0 = r * ive(0, k) * np.exp(logp - logp.max())
    p1 = r * ive(1, k) * np.exp(logp - logp.max())
    mean = (d / ad if ad > 0 else 0.0) * np.sum(p1 * r) / np.sum(p0)
    return complex(mean), float(np.sum(p0 * r * r) / np.sum(p0))
