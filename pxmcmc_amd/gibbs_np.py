"""
The numpy statement of the Gibbs sampler on the Gaussian posterior (:class:`pxmcmc_amd.optim.GaussianGibbs`, csrc/gibbs.hip;
DESIGN.md section 24): the joint posterior of the field and of the prior variances, sampled by alternating the exact draw
``x | v, d`` of :class:`pxmcmc_amd.optim.GaussianPosterior` with the conditional ``v | x`` (Wandelt, Larson &
Lakshminarayanan 2004; Jewell, Levin & Anderson 2004).

The state ``x`` of length n is cut into K contiguous groups by offsets ``0 = b_0 < ... < b_K = n``; group k has
``n_k = b_{k+1} - b_k`` elements and one precision ``D_k`` (the precision of ``F``)::

    F(x) = 1/2 Re L2(x) + 1/2 sum_k D_k sigma_k,   sigma_k = sum_{i in k} |x_i|^2

With the hyper-prior ``p(v_k) ~ v_k^-q`` on the variance ``v_k = 1 / D_k`` the conditional is

    D_k | x  =  chi2_nu / sigma_k,   nu_k = dof n_k + 2 q - 2      (:func:`nu_rule`)

``dof = 2`` for a complex state (both components of an element have variance ``v_k``) and 1 for a real one.  The chi-square
deviate is the sum of ``nu_k`` squared normals; which normals of the Philox stream those are is :func:`deviate_index`.

Here: the rules (:func:`group_bounds`, :func:`check_q`, :func:`nu_rule`, :func:`sampled_groups`, :func:`deviate_index`,
:func:`slice_table`), the conditional draw in float64 (:func:`variance_draw_np`) and in extended precision with the forward-error
bound of the kernels' float64 operation sequence (:func:`variance_draw_ld`, :func:`expand_ld`), a reference sweep and sampler on
a dense ``Phi`` (:func:`gibbs_sweep_np`, :func:`gibbs_run_np`) and the 1-D marginal posterior of ``v_k`` for the identity model
by quadrature (:func:`identity_log_variance_moments`).
"""
import numpy as np

from . import cg_np

EPS = cg_np.EPS
LD = np.longdouble
Q_MAX = 2.0  # the largest hyper-prior exponent the deviate assignment covers (see deviate_index)


# ---- the rules ---------------------------------------------------------------------------------------------------------------
def group_bounds(bounds, n, name="GaussianGibbs"):
    """the offsets ``0 = b_0 < b_1 < ... < b_K = n`` of K contiguous, non-empty groups (any integer sequence), checked ->
    int64 numpy array of K + 1"""
    try:
        b = np.asarray(bounds)
        if b.dtype.kind not in "iu":
            raise TypeError
        b = b.astype(np.int64)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: the group offsets must be a sequence of integers") from None
    if b.ndim != 1 or b.size < 2:
        raise ValueError(f"{name}: the group offsets must hold K + 1 values, K >= 1")
    if b[0] != 0 or b[-1] != n or np.any(np.diff(b) <= 0):
        raise ValueError(f"{name}: the group offsets must increase strictly from 0 to n = {n} (no empty group)")
    return b


def check_q(q, name="GaussianGibbs"):
    """the hyper-prior exponent: real, ``2 q`` an integer, ``q <= 2`` -> ``2 q`` as an int"""
    q = float(q)
    if not np.isfinite(q) or 2 * q != np.rint(2 * q):
        raise ValueError(f"{name}: hyper_q must be a real number with 2 q an integer")
    if q > Q_MAX:
        raise ValueError(f"{name}: hyper_q must be at most {Q_MAX:g}: a group owns n_k + 1 Philox pairs, 2 n_k + 2 deviates")
    return int(np.rint(2 * q))


def nu_rule(nk, dof, q):
    """``nu = dof n_k + 2 q - 2``, the degrees of freedom of the conditional of a group of ``n_k`` elements (an integer or an
    integer array)"""
    if dof not in (1, 2):
        raise ValueError("dof is 1 (real state) or 2 (complex state)")
    return int(dof) * np.asarray(nk, dtype=np.int64) + (check_q(q) - 2)


def sampled_groups(bounds, dof, q, fixed=(), name="GaussianGibbs"):
    """-> (sampled [K] bool, nu [K]): a group is sampled unless it is listed in ``fixed``; a group with ``nu < 1`` cannot be
    sampled and must be listed there"""
    b = np.asarray(bounds, dtype=np.int64)
    K = b.size - 1
    nu = nu_rule(np.diff(b), dof, q)
    fx = np.zeros(K, dtype=bool)
    idx = np.asarray(list(fixed), dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= K):
        raise ValueError(f"{name}: fixed holds group indices 0 <= k < {K}")
    fx[idx] = True
    bad = np.nonzero((nu < 1) & ~fx)[0]
    if bad.size:
        raise ValueError(f"{name}: the groups {bad.tolist()} have nu = dof n_k + 2 q - 2 < 1 and cannot be sampled: list them "
                         f"in fixed (they keep their initial precision)")
    return ~fx, nu


def check_setup(n, dof, bounds, q, fixed, D, precision_bounds, name="GaussianGibbs"):
    """Everything the sampler's construction refuses, on the host: the offsets, the exponent, an unsampled group that is not
    fixed, a clamp that is not finite and positive, and an initial precision ``D`` (a float or ``[n]``) that is not constant
    inside a group -> dict of ``bounds`` [K + 1], ``sampled`` [K], ``nu`` [K] and ``D_groups`` [K]"""
    b = group_bounds(bounds, n, name)
    sampled, nu = sampled_groups(b, dof, q, fixed, name)
    try:
        d_lo, d_hi = (float(v) for v in precision_bounds)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: precision_bounds is a pair (d_lo, d_hi)") from None
    if not (np.isfinite(d_lo) and np.isfinite(d_hi) and 0 < d_lo <= d_hi):
        raise ValueError(f"{name}: precision_bounds must be finite with 0 < d_lo <= d_hi")
    D = np.asarray(D, dtype=float)
    if D.ndim > 1 or (D.ndim == 1 and D.size != n):
        raise ValueError(f"{name}: the initial precision is a float or one value per parameter")
    if not np.all(np.isfinite(D)) or np.any(D < 0):
        raise ValueError(f"{name}: the initial precision must be finite and not negative")
    Dv = np.broadcast_to(D, (n,))
    first = Dv[b[:-1]]
    if np.any(Dv != np.repeat(first, np.diff(b))):
        raise ValueError(f"{name}: the initial precision must be constant inside every group")
    return dict(bounds=b, sampled=sampled, nu=nu, D_groups=np.array(first, dtype=float))


def deviate_index(bounds, k, t):
    """deviate ``t`` of group ``k`` -> ``(index, component)``: component ``t & 1`` of the fp64 complex-stream Philox pair at
    counter index ``b_k + k + (t >> 1)``, element ``index`` of ``ops.randn(n + K + 1, C, complex_=True, noise64=True)``.  Group k
    owns the indices ``b_k + k ... b_{k+1} + k``: ``n_k + 1`` pairs, disjoint from every other group's for any offsets, enough
    for ``nu <= 2 n_k + 2``, which ``q <= 2`` guarantees for both dofs."""
    b = np.asarray(bounds, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    return b[k] + k + (t >> 1), t & 1


def group_deviates(omega, bounds, k, nu):
    """the ``nu`` normal deviates of group ``k`` from one chain's complex stream ``omega`` [n + K + 1]"""
    idx, comp = deviate_index(bounds, k, np.arange(int(nu)))
    z = np.asarray(omega)[idx]
    return np.where(comp == 0, z.real, z.imag)


def slice_table(bounds, S):
    """the groups cut into slices of ``S`` elements -> ``(tab [nslices, 2], group_slice0 [K + 1])``, int64: row s of ``tab`` is
    ``(k, j)``, the elements ``b_k + j S ... `` of group k, ordered by k, then j; ``group_slice0[k]`` the first slice of group k"""
    b = np.asarray(bounds, dtype=np.int64)
    per = (np.diff(b) + S - 1) // S
    g0 = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    k = np.repeat(np.arange(b.size - 1, dtype=np.int64), per)
    j = np.arange(g0[-1], dtype=np.int64) - g0[k]
    return np.ascontiguousarray(np.stack([k, j], axis=1)), g0


# ---- the conditional draw ----------------------------------------------------------------------------------------------------
def _abs2(x):
    x = np.asarray(x)
    return x.real ** 2 + x.imag ** 2 if np.iscomplexobj(x) else x * x


def variance_draw_np(x, bounds, q, sampled, D_old, omega, d_lo, d_hi):
    """one chain: the new group precisions ``[K]`` given the field ``x`` [n] and the chain's complex deviate stream ``omega``
    [n + K + 1]; a group that is not sampled keeps ``D_old[k]``; ``sigma_k`` not > 0 gives ``d_hi``"""
    b = np.asarray(bounds, dtype=np.int64)
    dof = 2 if np.iscomplexobj(x) else 1
    nu = nu_rule(np.diff(b), dof, q)
    D = np.array(D_old, dtype=float)
    for k in np.nonzero(np.asarray(sampled))[0]:
        sig = float(np.sum(_abs2(x[b[k]:b[k + 1]])))
        chi = float(np.sum(group_deviates(omega, b, k, nu[k]) ** 2))
        D[k] = min(max(chi / sig, d_lo), d_hi) if sig > 0 else d_hi
    return D


def variance_draw_ld(x, bounds, q, sampled, D_old, omega, d_lo, d_hi):
    """:func:`variance_draw_np` in extended precision -> dict of ``sigma``, ``chi2``, ``D`` ([K]; NaN sums for a group that is
    not sampled) and their bounds ``sigma_bound``, ``chi2_bound``, ``D_bound``: the forward error of the kernels' float64
    operation sequence.

    A bound on a sum is (N + r) 2^-53 sum |term|, as in :func:`cg_np.cg_sums_ld`: the N terms are added in a fixed order (lane,
    wave tree, waves, slices) in which a term passes through at most N - 1 additions, and a term itself is r roundings --
    ``|x|^2`` of a complex element is two products and a sum (r = 3), of a real one a product (r = 1), a squared deviate a
    product (r = 1; nu terms).  ``D = chi2 / sigma`` is one more rounding on the quotient of the two:
    ``|D' - D| <= D ((1 + e_chi) (1 + 2^-53) / (1 - e_sigma) - 1)`` with the relative bounds e of the sums, plus one unit for
    the second-order terms and this model's own rounding.  A clamped value is exact."""
    b = np.asarray(bounds, dtype=np.int64)
    cplx = np.iscomplexobj(x)
    nu = nu_rule(np.diff(b), 2 if cplx else 1, q)
    K = b.size - 1
    out = {key: np.full(K, np.nan) for key in ("sigma", "chi2", "sigma_bound", "chi2_bound")}
    out["D"], out["D_bound"] = np.array(D_old, dtype=float), np.zeros(K)
    for k in np.nonzero(np.asarray(sampled))[0]:
        xs = np.asarray(x[b[k]:b[k + 1]])
        terms = (xs.real.astype(LD) ** 2 + xs.imag.astype(LD) ** 2) if cplx else xs.astype(LD) ** 2
        z2 = group_deviates(omega, b, k, nu[k]).astype(LD) ** 2
        sig, chi = np.sum(terms), np.sum(z2)
        e_sig = LD((terms.size + (3 if cplx else 1)) * EPS)
        e_chi = LD((z2.size + 1) * EPS)
        out["sigma"][k], out["chi2"][k] = float(sig), float(chi)
        out["sigma_bound"][k], out["chi2_bound"][k] = float(e_sig * sig), float(e_chi * chi)
        if not sig > 0:
            out["D"][k] = d_hi
            continue
        D = chi / sig
        bound = D * ((1 + e_chi) * (1 + LD(EPS)) / (1 - e_sig) - 1 + LD(EPS))
        # the clamp: a value the bound keeps on one side of a limit is that limit exactly; next to a limit either is allowed
        lo, hi = float(D - bound), float(D + bound)
        if lo >= d_hi or hi <= d_lo:
            out["D"][k], out["D_bound"][k] = (d_hi if lo >= d_hi else d_lo), 0.0
        else:
            out["D"][k], out["D_bound"][k] = float(min(max(D, LD(d_lo)), LD(d_hi))), float(bound)
    return out


def expand_np(Dg, bounds, h):
    """one chain: ``(D, sqrt(D), 1 / (D + h))`` of every element from the group precisions ``Dg`` [K]"""
    D = np.repeat(np.asarray(Dg, dtype=float), np.diff(np.asarray(bounds, dtype=np.int64)))
    return D, np.sqrt(D), 1.0 / (D + h)


def expand_ld(Dg, bounds, h):
    """:func:`expand_np` in extended precision -> ``((D, sqrtD, Minv), (bounds))``: ``D`` is a copy (bound 0), the square root
    one correctly rounded operation (2 units with the model's own), ``1 / (D + h)`` a rounded sum and a rounded division (3)"""
    D = np.repeat(np.asarray(Dg, dtype=float), np.diff(np.asarray(bounds, dtype=np.int64))).astype(LD)
    sq, mi = np.sqrt(D), 1 / (D + LD(h))
    return (D.astype(float), sq, mi), (np.zeros(D.size), 2 * EPS * np.abs(sq), 3 * EPS * np.abs(mi))


# ---- the sampler on a dense Phi -------------------------------------------------------------------------------------------------
def gibbs_sweep_np(Phi, w, data, bounds, q, sampled, Dg, omega1, omega2, omega_v, d_lo, d_hi):
    """One sweep of one chain on the dense model ``data = Phi x + noise`` with data weights ``w`` (the diagonal inverse
    covariance): the exact draw ``x | D, d`` by perturbation-optimisation (:func:`cg_np.draw_rhs_np`, a dense solve) with the
    deviates ``omega1`` (data length) and ``omega2`` (state length), then ``D | x`` with the stream ``omega_v``.
    -> ``(x, Dg_new)``"""
    Phi = np.asarray(Phi)
    w = np.asarray(w, dtype=float)
    D = expand_np(Dg, bounds, 0.0)[0]
    H = Phi.conj().T @ (w[:, None] * Phi) + np.diag(D)
    b0 = Phi.conj().T @ (w * np.asarray(data))
    x = np.linalg.solve(H, cg_np.draw_rhs_np(Phi, w, D, b0, omega1, omega2))
    return x, variance_draw_np(x, bounds, q, sampled, Dg, omega_v, d_lo, d_hi)


def gibbs_run_np(Phi, w, data, bounds, q, fixed, Dg0, nsweeps, nchains, normals, d_lo=1e-30, d_hi=1e30, complex_=None):
    """The sampler: ``nsweeps`` sweeps of ``nchains`` chains from the group precisions ``Dg0`` [K].  ``normals(t, c)`` returns
    the deviates ``(omega1 [m], omega2 [n], omega_v [n + K + 1] complex)`` of sweep t and chain c.
    -> ``(X [nsweeps, C, n], Dg [nsweeps, C, K])``: the field draws and the precisions after every sweep"""
    Phi = np.asarray(Phi)
    n = Phi.shape[1]
    b = group_bounds(bounds, n)
    cplx = np.iscomplexobj(Phi) or np.iscomplexobj(data) if complex_ is None else bool(complex_)
    sampled, _ = sampled_groups(b, 2 if cplx else 1, q, fixed)
    K = b.size - 1
    X = np.zeros((nsweeps, nchains, n), dtype=complex if cplx else float)
    Dg = np.zeros((nsweeps, nchains, K))
    cur = np.tile(np.asarray(Dg0, dtype=float), (nchains, 1))
    for t in range(nsweeps):
        for c in range(nchains):
            w1, w2, wv = normals(t, c)
            X[t, c], cur[c] = gibbs_sweep_np(Phi, w, data, b, q, sampled, cur[c], w1, w2, wv, d_lo, d_hi)
        Dg[t] = cur
    return X, Dg


def identity_gibbs_np(data, noise_var, bounds, q, Dg0, nsweeps, nchains, rng, d_lo=1e-30, d_hi=1e30):
    """:func:`gibbs_run_np` for the real identity model ``d = x + noise`` (``Phi = I``, ``w = 1 / noise_var``), vectorised over
    the chains and with the chi-square deviates summed from ``rng.standard_normal`` -> ``Dg [nsweeps, C, K]``"""
    d = np.asarray(data, dtype=float)
    b = group_bounds(bounds, d.size)
    nk = np.diff(b)
    sampled, nu = sampled_groups(b, 1, q, ())
    w = 1.0 / float(noise_var)
    cur = np.tile(np.asarray(Dg0, dtype=float), (nchains, 1))
    out = np.zeros((nsweeps, nchains, b.size - 1))
    for t in range(nsweeps):
        D = np.repeat(cur, nk, axis=1)
        rhs = w * d + np.sqrt(w) * rng.standard_normal((nchains, d.size)) + np.sqrt(D) * rng.standard_normal((nchains, d.size))
        x = rhs / (w + D)
        sig = np.add.reduceat(x * x, b[:-1], axis=1)
        chi = np.stack([np.sum(rng.standard_normal((nchains, int(v))) ** 2, axis=1) for v in nu], axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            cur = np.where(sig > 0, np.clip(chi / sig, d_lo, d_hi), d_hi)
        out[t] = cur
    return out


# ---- the identity model's marginal posterior of a group variance, by quadrature ------------------------------------------------
def identity_log_variance_moments(S, nk, noise_var, q=0.0, dof=1, span=80.0, points=400001):
    """Mean and variance of ``log v`` under the marginal posterior of one group's variance in the identity model
    ``d = x + noise``: with the field integrated out the ``dof n_k`` real components of the group's data are
    ``N(0, v + noise_var)``, so

        p(v | d)  ~  v^-q (v + noise_var)^(-dof n_k / 2) exp(-S / (2 (v + noise_var))),   S = sum_{i in k} |d_i|^2

    (``noise_var`` per real component).  Trapezoid rule in ``u = log v`` over ``[-span, span]`` (the density in u carries the
    Jacobian ``v``).  Proper for ``q < 1`` at ``v -> 0`` and for ``dof n_k / 2 + q > 1`` at infinity."""
    u = np.linspace(-span, span, int(points))
    v = np.exp(u)
    logp = (1.0 - q) * u - 0.5 * dof * nk * np.log(v + noise_var) - 0.5 * S / (v + noise_var)
    p = np.exp(logp - logp.max())
    du = u[1] - u[0]
    trapezoid = lambda y: float(du * (np.sum(y) - 0.5 * (y[0] + y[-1])))  # noqa: E731
    z = trapezoid(p)
    m = trapezoid(p * u) / z
    return m, trapezoid(p * (u - m) ** 2) / z
