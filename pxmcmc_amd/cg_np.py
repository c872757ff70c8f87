"""
The numpy statement of the Gaussian posterior's solver (:class:`pxmcmc_amd.optim.GaussianPosterior`, csrc/cg.hip; DESIGN.md
section 23): the two launches of one preconditioned conjugate-gradient iteration (:func:`cg_apply_np`, :func:`cg_decide_np`,
:func:`cg_update_np`), the iteration built from them (:func:`pcg_np`), the construction of the exact posterior draws as dense
matrices (:func:`draw_factor_np`, :func:`draw_rhs_np`) and the assignment of the Philox deviates to the draws
(:func:`draw_iterations`).  ``*_ld`` are the same launches in extended precision together with the forward-error bound of the
float64 operation sequence the kernels run; the GPU tests hold every output element to that bound.

The system is ``H x = b`` per chain, ``H = D + A`` Hermitian positive definite: ``D`` the prior precision scaled by
``T / lmda`` (a vector or a float), ``A`` the linear part of ``x -> calc_gradg(forward(x))``, ``b0 = -calc_gradg(forward(0))``.
The recurrences are the single-reduction PCG of Chronopoulos & Gear (1989)::

    u = Minv r;  q = A u - b0
    apply:   w = D u + (q + b0);  gamma = sum Re conj(r) u,  delta = sum Re conj(u) w,  rho = sum |r|^2
    decide:  frozen, or rho <= tol^2 ||b||^2  ->  alpha = beta = 0, frozen
             beta = gamma / gamma_old (0 on the first), denom = delta - beta gamma / alpha_old,
             denom not > 0, or gamma, delta not finite  ->  frozen with the breakdown flag;  else alpha = gamma / denom
    update:  p = u + beta p;  s = w + beta s;  x = x + alpha p;  r = r - alpha s;  u = Minv r

A chain's coefficients are a row ``[alpha, beta, gamma_old, alpha_old, rho, ||b||^2, flags, iterations]``.
"""
import numpy as np

ALPHA, BETA, GAMMA_OLD, ALPHA_OLD, RHO, BNORM2, FLAGS, ITERS = range(8)
FROZEN, BREAKDOWN = 1, 2
EPS = 2.0 ** -53  # unit roundoff of float64
LD = np.longdouble


def new_coef(bnorm2):
    """a chain's coefficient row at the start of a solve: zero but for ``||b||^2``"""
    row = np.zeros(8)
    row[BNORM2] = bnorm2
    return row


def _re_dot(a, b):
    """``sum Re conj(a) b``"""
    return float(np.sum(a.real * b.real + a.imag * b.imag)) if np.iscomplexobj(a) or np.iscomplexobj(b) else float(np.sum(a * b))


def cg_apply_np(u, q, b0, D, r):
    """one chain: ``w = D u + (q + b0)`` and the sums ``(gamma, delta, rho)``"""
    w = D * u + (q + (0.0 if b0 is None else b0))
    return w, (_re_dot(r, u), _re_dot(u, w), float(np.sum(np.abs(r) ** 2)))


def cg_decide_np(row, sums, tol):
    """the finishing kernel's decision for one chain: the new coefficient row from the old one and the three sums"""
    row = np.array(row, dtype=float)
    if row[FLAGS] != 0:
        row[ALPHA] = row[BETA] = 0.0
        return row
    gam, dlt, rho = sums
    row[RHO] = rho
    if rho <= (tol * tol) * row[BNORM2]:
        row[ALPHA] = row[BETA] = 0.0
        row[FLAGS] = FROZEN
        return row
    first = row[ITERS] == 0
    with np.errstate(all="ignore"):
        beta = 0.0 if first else gam / row[GAMMA_OLD]
        denom = dlt if first else dlt - beta * gam / row[ALPHA_OLD]
    if not denom > 0 or not np.isfinite(gam) or not np.isfinite(dlt):
        row[ALPHA] = row[BETA] = 0.0
        row[FLAGS] = FROZEN | BREAKDOWN
        return row
    alpha = gam / denom
    row[ALPHA], row[BETA], row[GAMMA_OLD], row[ALPHA_OLD] = alpha, beta, gam, alpha
    row[ITERS] += 1
    return row


def cg_update_np(u, w, p, s, x, r, minv, row):
    """one chain: ``(p, s, x, r, u)`` after the update with the row's ``alpha``, ``beta``; a frozen chain is returned as it is"""
    if row[FLAGS] != 0:
        return p, s, x, r, u
    alpha, beta = row[ALPHA], row[BETA]
    p = u + beta * p
    s = w + beta * s
    x = x + alpha * p
    r = r - alpha * s
    return p, s, x, r, minv * r


def pcg_np(A, D, b, x0=None, minv=1.0, tol=1e-8, max_iter=1000, bnorm2=None):
    """Solve ``(D + A) x = b`` for one chain by the iteration above.  ``A``: a callable ``v -> A v`` (the linear part; the
    solver's ``q + b0``), or a dense matrix.  ``bnorm2``: the reference of the stop rule ``rho <= tol^2 bnorm2`` (None:
    ``||b||^2``).  Returns ``(x, info)`` with ``niter``, ``frozen``, ``breakdown`` and
    ``rel_residual`` (``sqrt(rho) / ||b||`` of the recurrence residual at the last decision)."""
    Av = A if callable(A) else (lambda v: A @ v)
    b = np.asarray(b)
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=b.dtype)
    r = b - (D * x + Av(x))
    u = minv * r
    p, s = np.zeros_like(b), np.zeros_like(b)
    row = new_coef(float(np.sum(np.abs(b) ** 2)) if bnorm2 is None else float(bnorm2))
    for _ in range(int(max_iter)):
        w, sums = cg_apply_np(u, Av(u), None, D, r)
        row = cg_decide_np(row, sums, tol)
        if row[FLAGS] != 0:
            break
        p, s, x, r, u = cg_update_np(u, w, p, s, x, r, minv, row)
    with np.errstate(all="ignore"):
        rel = np.sqrt(row[RHO] / row[BNORM2]) if row[BNORM2] > 0 else 0.0
    return x, dict(niter=int(row[ITERS]), frozen=bool(int(row[FLAGS]) & FROZEN), breakdown=bool(int(row[FLAGS]) & BREAKDOWN),
                   rel_residual=float(rel), coef=row)


# ---- the launches in extended precision, with the forward-error bound of the kernels' float64 operation sequence --------------
# A bound is (roundings + 1) * 2^-53 * (sum of the magnitudes of the terms): `roundings` counts the float64 roundings on the
# path from the inputs to the element (an fma is one), the magnitudes are those of the exact terms, and the + 1 covers the
# second-order terms and this model's own rounding (2^-64 per operation).  No constant is fitted to what a kernel returns.
def _parts(a):
    """the real components of an array as extended precision [..., k] (k = 2 for complex: the kernels work per component)"""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return np.stack([a.real, a.imag], axis=-1).astype(LD)
    return a.astype(LD)[..., None]


def _join(parts, cplx):
    return parts[..., 0] + 1j * parts[..., 1] if cplx else parts[..., 0]


def _vec(v, n):
    """a float or an [n] vector -> extended precision [n, 1]"""
    return np.broadcast_to(np.asarray(v, dtype=float).astype(LD), (n,))[:, None]


def cg_apply_ld(u, q, b0, D, r):
    """one chain -> ``(w, w_bound)``: ``w`` and its per-component bound as complex (or real) arrays whose real and imaginary
    parts are those of the components (``r`` is not read: the sums are :func:`cg_sums_ld`, on the kernel's own ``w``)"""
    cplx = np.iscomplexobj(u)
    n = u.shape[-1]
    U, Q = _parts(u), _parts(q)
    B = _parts(np.zeros(n) if b0 is None else b0.astype(u.dtype))
    Dv = _vec(D, n)
    w = Dv * U + Q + B
    # fl(q + b0), then one fma: 2 roundings
    bound = 3 * EPS * (np.abs(Dv * U) + np.abs(Q) + np.abs(B))
    return _join(w, cplx), _join(bound, cplx)


def cg_sums_ld(u, w, r):
    """``(gamma, delta, rho)`` of one chain from the arrays the kernel summed, and the bounds: every term is 1 (real) or 3
    (complex) roundings, the N terms are added with at most N - 1 further roundings each"""
    U, W, R = _parts(u), _parts(w), _parts(r)
    n = U.shape[0]
    per_term = 3 if U.shape[-1] == 2 else 1
    sums, bounds = [], []
    for a, b in ((R, U), (U, W), (R, R)):
        sums.append(float(np.sum(a * b)))
        bounds.append(float((n + per_term) * EPS * np.sum(np.abs(a * b))))
    return tuple(sums), tuple(bounds)


def cg_decide_ld(row, sums, tol, delta_bound=0.0):
    """:func:`cg_decide_np` on the kernel's own sums -> ``(row, bound)`` with a bound for alpha and beta (zero for the
    entries that are copies): beta is one division; denom is a product, a division and a difference on beta; alpha one more
    division, its error amplified by ``|alpha| / |denom|``.  ``delta_bound``: the uncertainty of the given ``delta`` (the
    kernel keeps gamma and rho in the row but not delta, which a caller then re-sums), carried into alpha's bound."""
    new = cg_decide_np(row, sums, tol)
    bound = np.zeros(8)
    if new[FLAGS] != 0 or row[FLAGS] != 0:
        return new, bound
    gam, dlt, _ = (LD(v) for v in sums)
    first = row[ITERS] == 0
    beta = LD(0) if first else gam / LD(row[GAMMA_OLD])
    corr = LD(0) if first else beta * gam / LD(row[ALPHA_OLD])
    denom = dlt - corr
    alpha = gam / denom
    b_beta = 0.0 if first else 2 * EPS * abs(beta)
    b_denom = float(delta_bound) + (0.0 if first else 5 * EPS * (abs(dlt) + abs(corr)))
    bound[BETA] = float(b_beta)
    bound[ALPHA] = float(2 * EPS * abs(alpha) + abs(alpha) * b_denom / abs(denom))
    bound[GAMMA_OLD] = 0.0
    bound[ALPHA_OLD] = bound[ALPHA]
    exact = np.array(new)
    exact[ALPHA], exact[BETA], exact[ALPHA_OLD] = float(alpha), float(beta), float(alpha)
    return exact, bound


def cg_update_ld(u, w, p, s, x, r, minv, row):
    """one chain -> ``((p, s, x, r, u), (bounds))`` after the update with the row's alpha and beta; a frozen chain is returned
    as it is with zero bounds (bit for bit)"""
    cplx = np.iscomplexobj(x)
    if row[FLAGS] != 0:
        zero = [np.zeros(np.shape(a), dtype=np.asarray(a).dtype) for a in (p, s, x, r, u)]
        return (p, s, x, r, u), tuple(zero)
    n = x.shape[-1]
    al, be = LD(row[ALPHA]), LD(row[BETA])
    U, W, P, S, X, R = (_parts(a) for a in (u, w, p, s, x, r))
    M = _vec(minv, n)
    p1, mp = be * P + U, np.abs(be * P) + np.abs(U)            # 1 rounding
    s1, ms = be * S + W, np.abs(be * S) + np.abs(W)            # 1
    x1, mx = al * p1 + X, abs(al) * mp + np.abs(X)             # 2: p1, then the fma
    r1, mr = R - al * s1, abs(al) * ms + np.abs(R)             # 2
    u1, mu = M * r1, np.abs(M) * mr                            # 3
    outs = tuple(_join(a, cplx) for a in (p1, s1, x1, r1, u1))
    bounds = tuple(_join((k + 1) * EPS * m, cplx) for k, m in ((1, mp), (1, ms), (2, mx), (2, mr), (3, mu)))
    return outs, bounds


def within(got, want, bound):
    """every component of ``got`` within its bound of ``want`` (complex arrays: real and imaginary parts separately)"""
    got, want, bound = np.asarray(got), np.asarray(want), np.asarray(bound)
    if np.iscomplexobj(want):
        return bool(np.all(np.abs(got.real - want.real) <= bound.real) and np.all(np.abs(got.imag - want.imag) <= bound.imag))
    return bool(np.all(np.abs(got - want) <= bound))


# ---- the prior ---------------------------------------------------------------------------------------------------------------
def gauss_prox_np(x, precision, T):
    """``x / (1 + T p)``: the minimiser of ``1/2 |z - x|^2 + T 1/2 p |z|^2``"""
    return x / (1.0 + T * np.asarray(precision, dtype=float))


def power_spectrum_precision_np(cl, L):
    """``1 / C_l`` repeated over the ``2 l + 1`` orders in ssht index order (``l^2 + l + m``)"""
    cl = np.asarray(cl, dtype=float)
    return np.repeat(1.0 / cl[:L], 2 * np.arange(L) + 1)


# ---- exact draws ---------------------------------------------------------------------------------------------------------------
def draw_iterations(k):
    """the Philox iteration numbers of draw ``k``: ``(2 k, 2 k + 1)`` for ``omega_1`` (data length) and ``omega_2`` (state)"""
    return 2 * int(k), 2 * int(k) + 1


def draw_factor_np(Phi, w, D):
    """``G = [Phi^H sqrt(W), sqrt(D)]`` (dense): ``G G^H = Phi^H W Phi + D = H``, so ``b0 + G omega`` with a standard normal
    ``omega`` has covariance ``H`` and ``H^-1`` of it is a draw of the posterior (perturbation-optimisation).  Masked data
    (``w = 0``) contribute zero columns."""
    Phi = np.asarray(Phi)
    n = Phi.shape[1]
    Dv = np.broadcast_to(np.asarray(D, dtype=float), (n,))
    return np.concatenate([Phi.conj().T * np.sqrt(np.asarray(w, dtype=float))[None, :], np.diag(np.sqrt(Dv))], axis=1)


def draw_rhs_np(Phi, w, D, b0, omega1, omega2):
    """the right-hand side of one draw the way the solver forms it: ``b0 + Phi^H W (s o omega1) + sqrt(D) o omega2`` with
    ``s = 1 / sqrt(w)`` where ``w > 0``, else 0 -- ``calc_gradg(data + s o omega1)`` is ``Phi^H W (s o omega1) - b0 + b0``"""
    w = np.asarray(w, dtype=float)
    with np.errstate(divide="ignore"):
        s = np.where(w > 0, 1.0 / np.sqrt(w), 0.0)
    n = np.asarray(Phi).shape[1]
    Dv = np.broadcast_to(np.asarray(D, dtype=float), (n,))
    return b0 + np.asarray(Phi).conj().T @ (w * (s * omega1)) + np.sqrt(Dv) * omega2
