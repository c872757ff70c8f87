"""The Gibbs sampler on the sparse posterior, on the host (pxmcmc_amd/lasso_np.py): the float64 draw
against its extended-precision model, the clamp, the distribution of the draw, the numpy sampler against the identity
model's posterior moments by quadrature, the stop rule of the solve, what construction refuses, and the check that no
element of the GPU tests' draws lies near its branch threshold (tests/test_gpu_lasso.py compares every element)."""
import numpy as np
import pytest

from pxmcmc_amd import cg_np
from pxmcmc_amd import lasso_np as LN

# ---- the draws of the GPU tests (tests/test_gpu_lasso.py runs the kernel on the same inputs) ------------------------------------
DRAW_SIZES = (1, 2, 255, 256, 257, 256 * 256 + 3)  # 256: one pass of a workgroup; 256 * 256: the grid-stride cap of the launch
DRAW_SEED, DRAW_CHAIN0, DRAW_SWEEP = 11, 5, 3
DRAW_CLAMP = (0.2, 20.0)  # both limits bind on a share of the elements of every case with n >= 255


def draw_case(n, cplx):
    """the inputs of the draw at size n -> dict of ``C`` (3 for odd n, else 1), ``x`` [C, n] (chain 1 of 3 exactly zero, and
    every seventh element of chain 0), ``T`` (a float or [n]), ``tscale``, ``h`` (a float or [C]): the four combinations of
    scalar / vector T and h over the sizes and dtypes"""
    rng = np.random.default_rng([n, int(cplx), 25])
    C = 3 if n % 2 else 1
    x = rng.normal(size=(C, n)) + (1j * rng.normal(size=(C, n)) if cplx else 0)
    x = x * rng.uniform(0.1, 3.0, size=(C, 1))
    x[0, ::7] = 0
    if C == 3:
        x[1] = 0
    vec_t = (n + int(cplx)) % 2 == 0
    vec_h = (not vec_t) if C == 3 else vec_t
    T = rng.uniform(0.5, 2.0, size=n) if vec_t else 1.3
    h = rng.uniform(0.1, 1.0, size=C) if vec_h else 0.37
    return dict(C=C, x=x, T=T, tscale=0.7, h=h)


def philox_words(seed, chain, n, it):
    """the Philox blocks ``[n, 4]`` of the counters ``(i, it)``, ``i < n``, under the key of ``(seed, chain)`` (the layout of
    oracle.philox.normal_pairs)"""
    from oracle import philox

    m64 = (1 << 64) - 1
    key = (int(seed) + int(chain) * 0x9E3779B97F4A7C15) & m64
    it = int(it) & m64
    ctr = np.zeros((n, 4), dtype=np.uint32)
    idx = np.arange(n, dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2], ctr[:, 3] = it & 0xFFFFFFFF, it >> 32
    k = np.tile(np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint32), (n, 1))
    return philox.philox4x32_10(ctr, k)


def draw_uniforms(n, C, seed=DRAW_SEED, chain0=DRAW_CHAIN0, it_z=None):
    """the uniforms ``[C, n]`` of a launch at normal iteration ``it_z`` (default: sweep DRAW_SWEEP), rebuilt from the bits"""
    it_z = LN.draw_iterations(DRAW_SWEEP)[0] if it_z is None else it_z
    return np.stack([LN.uniform_from_bits(philox_words(seed, chain0 + c, n, it_z + 1)) for c in range(C)])


def draw_model(case, z, u):
    """the extended-precision model of a case's launch, chain by chain -> list of ``precision_draw_ld`` dicts"""
    hv = np.broadcast_to(np.asarray(case["h"], dtype=float), (case["C"],))
    return [LN.precision_draw_ld(case["x"][c], case["T"], z[c], u[c], hv[c], *DRAW_CLAMP, tscale=case["tscale"])
            for c in range(case["C"])]


# ---- the identity model of the distribution tests (tests/test_gpu_lasso.py runs the GPU sampler on the real one) ----------------
IDENTITY_CHAINS, IDENTITY_SWEEPS, IDENTITY_BURN = 16, 400, 50
IDENTITY_T = np.repeat([0.5, 2.0, 5.0], 4)
IDENTITY_D = np.tile([0.0, 0.3, 1.5, -2.0], 3)
IDENTITY_NOISE_VARS = (0.25, 1.0)
# R-hat of the numpy sampler on the real identity model at noise variance 0.25 (12 elements, 16 chains, 350 kept sweeps), the
# largest element's, over ten generator seeds: between 1.0021 and 1.0065, mean 1.0034, standard deviation 0.0014
# (test_numpy_sampler_rhat prints them).  The GPU sampler's R-hat must stay below the largest plus that spread.
IDENTITY_RHAT = (1.0065, 0.0014)


def identity_expected(noise_var, cplx):
    d = IDENTITY_D * ((1 + 0.5j) if cplx else 1.0)
    mom = [LN.identity_moments(di, noise_var, ti) for di, ti in zip(d, IDENTITY_T)]
    return d, np.array([m[0] for m in mom]), np.array([m[1] for m in mom])


def z_scores(samples, expected):
    """``samples`` [nsweeps, C, n] (real) after burn-in -> per element (mean of the chain means - expected) / (standard error
    of the chain means)"""
    means = samples.mean(axis=0)
    se = means.std(axis=0, ddof=1) / np.sqrt(means.shape[0])
    return (means.mean(axis=0) - expected) / se


def rhat_of(samples):
    from pxmcmc_amd.uncertainty import streaming_np

    S, C, _ = samples.shape
    mean = samples.mean(axis=0)
    return streaming_np.rhat_np(np.full(C, S), mean, ((samples - mean) ** 2).sum(axis=0))


# ---- the draw ------------------------------------------------------------------------------------------------------------------
def _assert_within(got, ld, keys=("D", "sqrtD", "Minv")):
    ok = ~ld["ambiguous"]
    for key in keys:
        err, bound = np.abs(got[key] - ld[key]), ld[key + "_bound"]
        assert np.all(err[ok] <= bound[ok]), (key, np.max(err[ok] / np.where(bound[ok] > 0, bound[ok], 1)))


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_float64_draw_within_the_extended_precision_bound(cplx):
    """random inputs, and the grid |x| in {0, 1e-300, 1e-9, 1, 1e100} x t in {1e-6, 1, 1e6} with u next to 0 (first branch) and
    next to 1 (second branch wherever a D1 exceeds 2^-53): D, sqrt(D) and M^-1 of the float64 operation sequence lie within
    the bound of the extended-precision model; both branches occur; on ordinary inputs the bound is a few units of roundoff"""
    rng = np.random.default_rng(40 + cplx)
    phase = (lambda size: np.exp(2j * np.pi * rng.uniform(size=size))) if cplx else (lambda size: rng.choice([-1.0, 1.0], size=size))
    n = 4000
    x = rng.normal(size=n) * phase(n) * 10.0 ** rng.uniform(-3, 3, size=n)
    t = 10.0 ** rng.uniform(-3, 3, size=n)
    z, u = rng.normal(size=n), rng.uniform(size=n)
    got, ld = LN.precision_draw_np(x, t, z, u, 0.3), LN.precision_draw_ld(x, t, z, u, 0.3)
    _assert_within(got, ld)
    assert not ld["ambiguous"].any() and got["first"].any() and (~got["first"]).any() and np.array_equal(got["first"], ld["first"])
    assert np.all(ld["D_bound"] <= 60 * LN.EPS * ld["D"])  # (about 25 roundings on the longest path, error terms doubled at most)
    ax, tt = np.meshgrid([0.0, 1e-300, 1e-9, 1.0, 1e100], [1e-6, 1.0, 1e6], indexing="ij")
    reps = 16
    ax, tt = np.repeat(ax.ravel(), 2 * reps), np.repeat(tt.ravel(), 2 * reps)
    xe = ax * phase(ax.size)
    ze = rng.normal(size=ax.size)
    ue = np.tile(np.repeat([2.0 ** -53, 1 - 2.0 ** -53], reps), 15)
    got, ld = LN.precision_draw_np(xe, tt, ze, ue, 0.0, 1e-300, 1e300), LN.precision_draw_ld(xe, tt, ze, ue, 0.0, 1e-300, 1e300)
    _assert_within(got, ld)
    assert np.all(np.isfinite(got["D"])) and np.all(got["D"] > 0)
    assert np.all(got["first"][ue < 0.5]) and np.all(got["first"][ax == 0])
    second = ~got["first"]
    assert second[(ax == 1.0) & (ue > 0.5)].any() and second[(ax == 1e100) & (ue > 0.5)].any() and second[(ax == 1e-9) & (ue > 0.5)].any()
    # x = 0 is the Levy limit t^2 / z^2
    lim = (tt / ze) ** 2
    zero = (ax == 0) & (lim < 1e299) & (lim > 1e-299)
    assert np.allclose(got["D"][zero], lim[zero], rtol=1e-14, atol=0)


def test_rounded_threshold_scale_is_part_of_the_model():
    """``tscale``: t = tscale T rounded once, as the kernel forms it; the float64 draw at that rounded t lies within the bound"""
    rng = np.random.default_rng(3)
    n = 500
    x, T, z, u = rng.normal(size=n), rng.uniform(0.5, 2.0, size=n), rng.normal(size=n), rng.uniform(size=n)
    got = LN.precision_draw_np(x, 0.7 * T, z, u, 0.1)
    ld = LN.precision_draw_ld(x, T, z, u, 0.1, tscale=0.7)
    _assert_within(got, ld)
    assert np.all(np.abs(got["terms"] - ld["terms"]) <= ld["terms_bound"])


def test_clamp_limits_hit_exactly():
    """a raw value beyond a limit by more than its bound is that limit, bit for bit, in both models; the clamp is counted"""
    x = np.array([0.0, 1e-3, 1.0, 1e3, 1e3, 0.0])
    t = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    z = np.array([1e-3, 1.0, 1.0, 1.0, 1.0, 0.0])
    u = np.array([0.5, 0.9999, 0.3, 0.5, 0.9999999, 0.5])
    got, ld = LN.precision_draw_np(x, t, z, u, 0.0, 1e-2, 1e2), LN.precision_draw_ld(x, t, z, u, 0.0, 1e-2, 1e2)
    # t^2 / z^2 = 1e6; the second branch at mean 1e3; an ordinary value; D1 ~ 1e-3; x = z = 0 (inf)
    assert got["D"].tolist()[:2] == [1e2, 1e2] and got["D"][3] == 1e-2 and got["D"][5] == 1e2 and 1e-2 < got["D"][2] < 1e2
    assert got["clamped"].tolist() == [True, True, False, True, got["D"][4] != got["raw"][4], True]
    assert np.array_equal(ld["D"][[0, 1, 3, 5]], got["D"][[0, 1, 3, 5]]) and not ld["D_bound"][[0, 1, 3, 5]].any()
    assert np.array_equal(ld["clamped"], got["clamped"]) and not ld["clamp_open"].any()
    assert np.array_equal(got["sqrtD"][[0, 3]], [10.0, 0.1]) and np.array_equal(got["Minv"][[0, 3]], [1e-2, 1e2])
    total, bound, count, slack = LN.sums_ld(ld)
    assert count == int(got["clamped"].sum()) and slack == 0 and abs(total - float(np.sum(got["terms"]))) <= bound


@pytest.mark.parametrize("t,ax", [(3.0, 0.5), (0.7, 4.0), (1e-3, 1e3)])
def test_draw_distribution(t, ax):
    """2 x 10^5 draws: the sample means of D and 1 / D within 5 standard errors of t / |x| and |x| / t + 1 / t^2 -- the
    standard error of D from the known variance mu^3 / shape, that of 1 / D from the sample -- for a real and for a complex x"""
    N = 200000
    rng = np.random.default_rng(int(1000 * t) + 7)
    mu, var, inv = LN.inverse_gaussian_moments(t, ax)
    for x in (ax, ax * np.exp(0.7j)):
        D = LN.precision_draw_np(np.full(N, x), t, rng.standard_normal(N), rng.uniform(size=N), 0.0, 1e-300, 1e300)["D"]
        zD = (D.mean() - mu) / np.sqrt(var / N)
        zi = ((1 / D).mean() - inv) / ((1 / D).std(ddof=1) / np.sqrt(N))
        print(f"t {t}, |x| {ax}: mean D {D.mean():.6g} (expected {mu:.6g}, z {zD:.2f}), mean 1/D {(1 / D).mean():.6g} ({inv:.6g}, z {zi:.2f})")
        assert abs(zD) <= 5 and abs(zi) <= 5


def test_draw_distribution_at_zero():
    """x = 0: D = t^2 / chi2_1; the sample median within 5 standard errors of its median (the standard error of a sample
    median is 1 / (2 f sqrt(N)) with the density f at the median)"""
    from scipy.stats import chi2

    N, t = 200000, 1.7
    rng = np.random.default_rng(9)
    D = LN.precision_draw_np(np.zeros(N), t, rng.standard_normal(N), rng.uniform(size=N), 0.0, 1e-300, 1e300)["D"]
    ym = chi2.median(1)
    med = t * t / ym
    f = chi2.pdf(ym, 1) * ym * ym / (t * t)  # density of D = t^2 / y at the median: f_y(y) |dy / dD|
    z = (np.median(D) - med) / (1 / (2 * f * np.sqrt(N)))
    print(f"x = 0: median {np.median(D):.6g}, expected {med:.6g}, z {z:.2f}")
    assert abs(z) <= 5


# ---- the sampler ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_var", IDENTITY_NOISE_VARS)
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_numpy_sampler_on_the_identity_model(cplx, noise_var):
    """d = x + noise, 12 elements with (t, d) over {0.5, 2, 5} x {0, 0.3, 1.5, -2} (complex: d (1 + i / 2)), 16 chains, 400 sweeps
    of which 50 burn-in: the posterior mean and E |x|^2 of every element within 5 standard errors (of the 16 chain means) of
    the quadrature values"""
    d, mean, second = identity_expected(noise_var, cplx)
    X = LN.identity_lasso_gibbs_np(d, noise_var, IDENTITY_T, IDENTITY_SWEEPS, IDENTITY_CHAINS,
                                   np.random.default_rng(100 + 2 * cplx + int(4 * noise_var)))[IDENTITY_BURN:]
    z = [z_scores(X.real, mean.real), z_scores(np.abs(X) ** 2, second)] + ([z_scores(X.imag, mean.imag)] if cplx else [])
    print("expected mean", mean, "E|x|^2", second, "z", z)
    assert all(np.all(np.abs(zz) <= 5.0) for zz in z), z


def test_numpy_sampler_rhat():
    """the R-hat the numpy sampler reaches on the real identity model at noise variance 0.25, over ten seeds: the figures of
    IDENTITY_RHAT, which bound the GPU sampler's in tests/test_gpu_lasso.py"""
    d, _, _ = identity_expected(0.25, False)
    worst = np.array([rhat_of(LN.identity_lasso_gibbs_np(d, 0.25, IDENTITY_T, IDENTITY_SWEEPS, IDENTITY_CHAINS,
                                                         np.random.default_rng(500 + s))[IDENTITY_BURN:]).max() for s in range(10)])
    print("largest R-hat per seed", worst, "max", worst.max(), "mean", worst.mean(), "std", worst.std(ddof=1))
    assert abs(worst.max() - IDENTITY_RHAT[0]) < 5e-5 and abs(worst.std(ddof=1) - IDENTITY_RHAT[1]) < 5e-5


def test_dense_sampler_on_the_identity_against_its_formula():
    """``lasso_gibbs_np`` with ``Phi = I`` fed given deviates against the closed form of the identity model written out here"""
    rng = np.random.default_rng(1)
    n, C, S, w = 12, 2, 3, 4.0
    d = IDENTITY_D
    dev = {(s, c): (rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n), rng.uniform(size=n))
           for s in range(S) for c in range(C)}
    X, D = LN.lasso_gibbs_np(np.eye(n), np.full(n, w), d, IDENTITY_T, S, C, lambda s, c: dev[s, c])
    for c in range(C):
        cur = LN.initial_precision(IDENTITY_T, False)
        assert np.array_equal(cur, IDENTITY_T ** 2 / 2)
        for s in range(S):
            w1, w2, z, u = dev[s, c]
            x = (w * d + np.sqrt(w) * w1 + np.sqrt(cur) * w2) / (w + cur)
            assert np.allclose(X[s, c], x, rtol=1e-12, atol=0)
            cur = LN.precision_draw_np(X[s, c], IDENTITY_T, z, u)["D"]
            assert np.array_equal(D[s, c], cur)


def test_stop_rule_reference_norm():
    """A dense system (n = 48) whose D spans twelve decades inside the chain, solved by cg_np's iteration with the diagonal
    preconditioner M = D + trace(A) / N, tol = 1e-6.  Stopped at ||r|| <= tol ||b_data|| -- the data part of the right-hand
    side, b0 + Phi^H W (s o omega_1) -- the field meets the dense solve to tol: ||x - x*|| <= tol ||x*||.  Stopped at
    tol ||b||, which sqrt(D) o omega_2 of the largest precisions dominates (||b|| / ||b_data|| is printed: 4000 to 12000), it
    stops several iterations earlier, is further from the dense solve in every trial and does not meet it to tol in all of
    them: that stop rule does not keep what tol promises."""
    rng = np.random.default_rng(3)
    m, n, tol = 96, 48, 1e-6
    Phi = rng.normal(size=(m, n)) / np.sqrt(m)
    w = np.ones(m)
    truth = np.where(rng.uniform(size=n) < 0.25, 2 * rng.normal(size=n), 0.0)
    data = Phi @ truth + rng.normal(size=m)
    A = Phi.T @ (w[:, None] * Phi)
    b0 = Phi.T @ (w * data)
    errors = []
    for trial in range(8):
        D = 10.0 ** rng.uniform(-2, 10, size=n)
        D[:6] = 10.0 ** rng.uniform(-2, 0, size=6)
        assert D.max() / D.min() > 1e11
        w1, w2 = rng.normal(size=m), rng.normal(size=n)
        bd = cg_np.draw_rhs_np(Phi, w, 0.0, b0, w1, w2)
        b = cg_np.draw_rhs_np(Phi, w, D, b0, w1, w2)
        xs = np.linalg.solve(A + np.diag(D), b)
        minv = 1 / (D + np.trace(A) / n)
        x_data, info_data = cg_np.pcg_np(A, D, b, minv=minv, tol=tol, max_iter=500, bnorm2=float(bd @ bd))
        x_full, info_full = cg_np.pcg_np(A, D, b, minv=minv, tol=tol, max_iter=500)
        e_data, e_full = np.linalg.norm(x_data - xs) / np.linalg.norm(xs), np.linalg.norm(x_full - xs) / np.linalg.norm(xs)
        print(f"trial {trial}: ||b|| / ||b_data|| {np.linalg.norm(b) / np.linalg.norm(bd):.3g}; data reference {info_data['niter']} "
              f"iterations, relative error {e_data:.3e}; ||b|| reference {info_full['niter']} iterations, relative error {e_full:.3e}")
        assert info_data["frozen"] and info_full["frozen"] and info_full["niter"] < info_data["niter"]
        assert e_data <= tol and e_data < e_full
        errors.append(e_full)
    assert max(errors) > tol


def test_refusals():
    ok = dict(n=5, T=1.0, lmda=2.0, precision_bounds=(1e-6, 1e6))
    assert LN.check_setup(**ok)["t"] == 0.5
    assert LN.check_setup(**dict(ok, T=np.arange(1.0, 6.0)))["t"].tolist() == [0.5, 1.0, 1.5, 2.0, 2.5]
    for T in (0.0, -1.0, np.nan, np.inf, [1.0, 2.0, 0.0, 1.0, 1.0], [1.0, 2.0, -3.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="positive"):
            LN.check_setup(**dict(ok, T=T))
    for T in ([1.0, 2.0], np.ones((5, 1))):
        with pytest.raises(ValueError, match="one value per parameter"):
            LN.check_setup(**dict(ok, T=T))
    for lmda in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError, match="lmda"):
            LN.check_setup(**dict(ok, lmda=lmda))
    for pb in ((0.0, 1.0), (1.0, np.inf), (np.nan, 1.0), (-1.0, 1.0), (2.0, 1.0), (1.0,)):
        with pytest.raises(ValueError, match="precision_bounds"):
            LN.check_setup(**dict(ok, precision_bounds=pb))


def test_deviate_layout():
    """the iterations of the precision draws are off every other consumer's, and the uniform is exact and rebuilt from the bits"""
    its = [it for t in range(1000) for it in LN.draw_iterations(t)]
    others = {2 * t for t in range(1000)} | {2 * t + 1 for t in range(1000)} | {(1 << 61) + t for t in range(1000)} | {1 << 62}
    assert len(set(its)) == 2000 and not set(its) & others and not {LN.DRAW_ITER - 2, LN.DRAW_ITER - 1} & (others | set(its))
    words = np.array([[0, 0, 5, 6], [0xFFFFFFFF, 0xFFFFFFFF, 0, 0], [0x00001000, 0, 1, 2], [0xFFFFF000, 0x7FFFFFFF, 9, 9]], dtype=np.uint32)
    u = LN.uniform_from_bits(words)
    assert u.tolist() == [2.0 ** -53, 1 - 2.0 ** -53, 1.5 * 2.0 ** -52, 0.5 - 2.0 ** -53]
    w = philox_words(DRAW_SEED, DRAW_CHAIN0, 1000, LN.draw_iterations(0)[1])
    u = LN.uniform_from_bits(w)
    assert np.all((u > 0) & (u < 1)) and np.all(u * 2.0 ** 53 % 2 == 1) and 0.45 < u.mean() < 0.55  # odd multiples of 2^-53


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", DRAW_SIZES)
def test_no_gpu_case_is_ambiguous(n, cplx):
    """The seeds, chain numbers, iterations and sizes of the GPU tests, with z from oracle.philox and u from the bits: no element
    lies within 1000 x the model's bound of the branch threshold u (1 + a D1) = 1, and none within it of a clamp limit.  (The
    oracle's normals are numpy's float64 Box-Muller, 1e-15 from the device's: a thousandth of the margin.)  So the GPU
    comparison leaves out no element."""
    from oracle import philox

    case = draw_case(n, cplx)
    it_z = LN.draw_iterations(DRAW_SWEEP)[0]
    z = np.stack([philox.normal_pairs(DRAW_SEED, DRAW_CHAIN0 + c, np.arange(n, dtype=np.uint64), it_z, bits=64)[0] for c in range(case["C"])])
    u = draw_uniforms(n, case["C"])
    hit_lo = hit_hi = 0
    for ld in draw_model(case, z, u):
        assert np.all(np.abs(ld["branch_value"] - 1) > 1000 * ld["branch_bound"])
        assert not ld["ambiguous"].any() and not ld["clamp_open"].any()
        near = (np.abs(ld["D"] - DRAW_CLAMP[0]) <= 1000 * ld["D_bound"]) | (np.abs(ld["D"] - DRAW_CLAMP[1]) <= 1000 * ld["D_bound"])
        assert not (near & ~ld["clamped"]).any()
        hit_lo, hit_hi = hit_lo + int(np.sum(ld["D"] == DRAW_CLAMP[0])), hit_hi + int(np.sum(ld["D"] == DRAW_CLAMP[1]))
    if n >= 255:
        assert hit_lo > 0 and hit_hi > 0
