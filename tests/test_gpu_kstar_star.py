"""GPU: the star path of the K* pass (kstar_kernel with star_geom_kernel's table: the rows of a collinear star from two
inner products per star) against NumPy references formed from direct differences, dense, and against the same library
with PPBO_KSTAR_STAR=0 (one inner product per row).

How the checks reach the kernel:
  * models of up to 1024 rows in node form would be scored by the one-launch kernel, so both engines of this file are
    created with PPBO_FUSED=0: every model here takes kstar_kernel -> quadform_kernel -> score_kernel;
  * a K* row is read bit for bit as the posterior mean of a mean-only model with alpha = e_j (every other row adds
    0 * k = +0 to the sum);
  * hand-built posteriors (random alpha, Lambda and operator G of the right sparsity) make mean and variance plain
    linear / quadratic functions of K* that NumPy evaluates from its own K*:
        mu = K*' alpha,   var = sf2 + sum_stars [ld_o k_o^2 + sum_j (ld_j k_j^2 + 2 lo_j k_j k_o)] + |G K*|^2 (node)
                                                                                           or + |H E|^2  (edge),
    E the edge layout: rows [0, n_q) zero, row n_q + q m + t = lo_j (k_j - k_obs(q)).

Bounds (the project's own): K* entries 1e-12 sf2 (the K* / Sigma parity level), var between the two paths 1e-8 sf2, var
against golden vectors 1e-6 sf2, mu 1e-9 relative in the max norm.  Against the NumPy references of the hand-built
posteriors the entries of alpha, Lambda and G are O(1) and N <= 288, so the same 1e-9 (mu, relative) and 1e-8 sf2 (var,
relative to sf2; |var| <= 20 sf2 there) leave five orders of magnitude over the rounding of a depth-288 fp64 sum."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

KERNELS = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")


def _engine(**env):
    """An Engine whose ctx read the given PPBO_* knobs when it was created (they are per ctx, read once)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def star():
    e = _engine(PPBO_FUSED=0, PPBO_KSTAR_STAR=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def plain():
    e = _engine(PPBO_FUSED=0, PPBO_KSTAR_STAR=0)
    yield e
    e.close()


def host(t):
    return t.detach().cpu().numpy()


# ---- NumPy references: direct differences, dense ----------------------------------------------------------------------
def scaled(P, theta):
    """Rows in the coordinates the kernel takes its differences in (ARD: x / l_d, then l = 1)."""
    l = theta[1]
    return (np.asarray(P, float), float(l)) if np.ndim(l) == 0 else (np.asarray(P, float) / np.asarray(l, float), 1.0)


def kstar_ref(X, Xc, theta, kernel):
    """K* [N, M] from the differences x_j - c themselves."""
    Xs, l = scaled(X, theta)
    Cs, _ = scaled(Xc, theta)
    r2 = ((Xs[:, None, :] - Cs[None, :, :]) ** 2).sum(-1)
    sf2 = float(theta[2]) ** 2
    if kernel == "SE_kernel":
        return sf2 * np.exp(-0.5 * r2 / l ** 2)
    if kernel == "RQ_kernel":
        return sf2 / (1.0 + r2 / (4.0 * l ** 2)) ** 2
    r = np.sqrt(r2)
    if kernel == "Matern52_kernel":
        a = np.sqrt(5.0) * r / l
        return sf2 * (1.0 + a + a * a / 3.0) * np.exp(-a)
    a = np.sqrt(3.0) * r / l
    return sf2 * (1.0 + a) * np.exp(-a)


def mean_var_ref(K, alpha, ld, lo, G, m, form, sf2):
    from ppbo_amd.engine import FORM_EDGE
    N, M = K.shape
    mb, n_q = m + 1, N // (m + 1)
    Ks = K.reshape(n_q, mb, M)
    ko = Ks[:, :1, :]
    lds, los = ld.reshape(n_q, mb, 1), lo.reshape(n_q, mb, 1)
    t = (lds[:, :1] * ko ** 2).sum((0, 1)) + (Ks[:, 1:] * (lds[:, 1:] * Ks[:, 1:] + 2.0 * los[:, 1:] * ko)).sum((0, 1))
    if form == FORM_EDGE:
        E = np.zeros_like(K)
        E[n_q:] = (los[:, 1:] * (Ks[:, 1:] - ko)).reshape(n_q * m, M)
        Y = G @ E
    else:
        Y = G @ K
    return K.T @ alpha, sf2 + t + (Y ** 2).sum(0)


# ---- designs and hand-built posteriors --------------------------------------------------------------------------------
def star_design(rng, n_q, m, D, direction="general", zero_row=False, zero_star=False):
    """n_q stars of m + 1 rows: x_obs and m points x_obs + s_j xi with s_j of both signs.  direction: "axis" (xi along one
    coordinate, as the feedback of a coordinate query) or "general" (every coordinate of xi non-zero).  zero_row: star 0
    holds a pseudo row equal to its observation (s_j = 0); zero_star: the last star has xi = 0."""
    X = np.empty((n_q, m + 1, D))
    for q in range(n_q):
        xo = 0.3 + 0.4 * rng.random(D)
        if direction == "axis":
            xi = np.zeros(D)
            xi[q % D] = 1.0
        else:
            xi = rng.uniform(0.2, 1.0, D) * rng.choice([-1.0, 1.0], D)
        s = rng.uniform(-0.3, 0.3, m)
        s[0] = -0.25                      # (a negative s_j in every star)
        if zero_row and q == 0:
            s[m // 2] = 0.0
        if zero_star and q == n_q - 1:
            xi[:] = 0.0
        X[q, 0] = xo
        X[q, 1:] = xo + s[:, None] * xi
    return X.reshape(n_q * (m + 1), D)


def operator(rng, N, m, form):
    """A random operator of the form's sparsity: node form block lower triangular in stars of m + 1 rows; edge form lower
    triangular, zero in the n_q observation rows and columns, positive diagonal."""
    from ppbo_amd.engine import FORM_EDGE
    n_q = N // (m + 1)
    G = rng.standard_normal((N, N)) / np.sqrt(N)
    i, j = np.indices((N, N))
    if form == FORM_EDGE:
        G = np.where(j <= i, G, 0.0)
        G[:n_q] = 0.0
        G[:, :n_q] = 0.0
        G[np.arange(n_q, N), np.arange(n_q, N)] = 0.5 + rng.random(N - n_q)
    else:
        G = np.where(j // (m + 1) <= i // (m + 1), G, 0.0)
    return G


class Hand:
    """A hand-built posterior on the host, and its device twin on any engine."""

    def __init__(self, rng, X, theta, kernel, m, form):
        N = X.shape[0]
        self.X, self.theta, self.kernel, self.m, self.form = X, theta, kernel, m, form
        self.alpha = rng.standard_normal(N)
        self.ld = -rng.random(N)
        self.lo = rng.random(N)
        self.lo[::m + 1] = 0.0
        self.G = operator(rng, N, m, form)
        self.sf2 = float(theta[2]) ** 2

    def on(self, eng, alpha=None, mean_only=False):
        from ppbo_amd.engine import Posterior, theta_key
        Xd, _, scale = eng._ard(self.X, self.theta, self.kernel)
        a = eng.dev(self.alpha if alpha is None else alpha)
        if mean_only:
            return Posterior(self.kernel, theta_key(self.theta), self.m, Xd, a, None, None, None, scale=scale)
        return Posterior(self.kernel, theta_key(self.theta), self.m, Xd, a, eng.dev(self.ld), eng.dev(self.lo),
                         eng.dev(self.G), scale=scale, form=self.form)

    def reference(self, Xc):
        K = kstar_ref(self.X, Xc, self.theta, self.kernel)
        return (K,) + mean_var_ref(K, self.alpha, self.ld, self.lo, self.G, self.m, self.form, self.sf2)


def kstar_rows(eng, hand, Xc, rows):
    """Rows of K* as the kernel forms them, bit for bit: the mean of a mean-only model with alpha = e_j."""
    from ppbo_amd.engine import SCORE_MEAN
    N = hand.X.shape[0]
    post = hand.on(eng, alpha=np.zeros(N), mean_only=True)
    Xd = eng.dev(Xc)
    out = np.empty((len(rows), Xd.shape[0]))
    for i, j in enumerate(rows):
        post.alpha.zero_()
        post.alpha[j] = 1.0
        out[i] = host(eng.predict(post, Xd, score=SCORE_MEAN, want_var=False, want_best=False)["mu"])
    return out


def check_paths(star, plain, hand, Xc, label=""):
    """Both paths against the NumPy reference and against each other; returns the star path's (mu, var)."""
    from ppbo_amd.engine import SCORE_VARIANCE
    K, mu0, var0 = hand.reference(Xc)
    a = star.predict(hand.on(star), Xc, score=SCORE_VARIANCE)
    b = plain.predict(hand.on(plain), Xc, score=SCORE_VARIANCE)
    mu_a, var_a, mu_b, var_b = host(a["mu"]), host(a["var"]), host(b["mu"]), host(b["var"])
    ms, vs = np.abs(mu0).max(), hand.sf2
    figs = dict(mu_ref=np.abs(mu_a - mu0).max() / ms, var_ref=np.abs(var_a - var0).max() / vs,
                mu_paths=np.abs(mu_a - mu_b).max() / ms, var_paths=np.abs(var_a - var_b).max() / hand.sf2)
    print(f"{label} N={hand.X.shape[0]} M={Xc.shape[0]} " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
    assert figs["mu_ref"] <= 1e-9 and figs["var_ref"] <= 1e-8
    assert figs["mu_paths"] <= 1e-9 and figs["var_paths"] <= 1e-8
    return mu_a, var_a


# ---- the tests --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n_q,D,M", [(3, 5, 3, 513), (25, 3, 20, 511), (31, 9, 20, 70000), (32, 3, 5, 513), (40, 2, 5, 513)])
@pytest.mark.parametrize("form", [0, 1])
def test_star_sizes_and_the_staging_boundary(star, plain, m, n_q, D, M, form):
    """m = 3 (eight stars per 32 staged rows), m = 25 (26-row stars: one per step, where 32-row steps would straddle them),
    m = 31 with 70000 candidates (two chunks; pick_split gives four splits of 2 stars and a last one of 1), m = 32 and m = 40 (stars
    longer than a step, staged in pieces: a last piece of one row, and of nine).  Node and edge layout."""
    rng = np.random.default_rng(1000 * m + n_q)
    X = star_design(rng, n_q, m, D, "general", zero_row=True)
    hand = Hand(rng, X, [1.0, 0.45, 1.3], "SE_kernel", m, form)
    Xc = rng.random((M, D))
    if M > 4096:                    # the reference on a subset that holds both chunks' ends
        sel = np.r_[0:600, 65536 - 300:65536 + 300, M - 600:M]
        K, mu0, var0 = hand.reference(Xc[sel])
        from ppbo_amd.engine import SCORE_VARIANCE
        a = star.predict(hand.on(star), Xc, score=SCORE_VARIANCE)
        b = plain.predict(hand.on(plain), Xc, score=SCORE_VARIANCE)
        assert np.abs(host(a["mu"])[sel] - mu0).max() <= 1e-9 * np.abs(mu0).max()
        assert np.abs(host(a["var"])[sel] - var0).max() <= 1e-8 * hand.sf2
        assert np.abs(host(a["mu"]) - host(b["mu"])).max() <= 1e-9 * np.abs(mu0).max()
        assert np.abs(host(a["var"]) - host(b["var"])).max() <= 1e-8 * hand.sf2
        assert a["best_idx"] == b["best_idx"] == int(np.argmax(host(a["var"])))
    else:
        check_paths(star, plain, hand, Xc, f"m={m} form={form}")


@pytest.mark.parametrize("direction", ["axis", "general"])
def test_directions_entry_by_entry(star, plain, direction):
    """Axis-aligned and general xi, negative s_j, a pseudo row equal to its observation, a star with xi = 0: every K*
    entry against direct differences and against the plain path at 1e-12 sf2 -- and the two paths are different code:
    on collinear stars some entry differs in its last bits (the switch switches something)."""
    rng = np.random.default_rng(7 if direction == "axis" else 8)
    m, n_q, D = 5, 4, 4
    X = star_design(rng, n_q, m, D, direction, zero_row=True, zero_star=True)
    theta = [1.0, 0.5, 1.2]
    hand = Hand(rng, X, theta, "SE_kernel", m, 0)
    Xc = np.concatenate([rng.random((61, D)), X[[0, 3, 7, 23]]])      # (four candidates on design rows)
    K0 = kstar_ref(X, Xc, theta, "SE_kernel")
    rows = np.arange(X.shape[0])
    Ka, Kb = kstar_rows(star, hand, Xc, rows), kstar_rows(plain, hand, Xc, rows)
    sf2 = hand.sf2
    print(f"{direction}: star-ref {np.abs(Ka - K0).max() / sf2:.2e} plain-ref {np.abs(Kb - K0).max() / sf2:.2e} "
          f"star-plain {np.abs(Ka - Kb).max() / sf2:.2e}")
    assert np.abs(Ka - K0).max() <= 1e-12 * sf2
    assert np.abs(Ka - Kb).max() <= 1e-12 * sf2
    assert not np.array_equal(Ka, Kb)
    # the star with xi = 0: every row is its observation's row
    last = Ka[(n_q - 1) * (m + 1):]
    assert np.array_equal(last, np.repeat(last[:1], m + 1, 0))


def test_a_star_off_its_line_keeps_the_plain_path(star, plain):
    """One star perturbed off its line by 1e-9 (the others collinear): its K* rows are bit for bit the plain path's, the
    model's mean and variance agree with the plain path and the reference."""
    rng = np.random.default_rng(21)
    m, n_q, D = 7, 5, 6
    X = star_design(rng, n_q, m, D, "general")
    off = 2
    X[off * (m + 1) + 3, 1] += 1e-9
    for form in (0, 1):
        hand = Hand(rng, X, [1.0, 0.4, 1.1], "Matern52_kernel", m, form)
        Xc = rng.random((300, D))
        check_paths(star, plain, hand, Xc, f"mixed form={form}")
    rows = np.arange(off * (m + 1), (off + 1) * (m + 1))
    Ka, Kb = kstar_rows(star, hand, Xc, rows), kstar_rows(plain, hand, Xc, rows)
    assert np.array_equal(Ka, Kb)
    others = np.arange(0, off * (m + 1))
    assert not np.array_equal(kstar_rows(star, hand, Xc, others), kstar_rows(plain, hand, Xc, others))


@pytest.mark.parametrize("M", [1, 2, 511, 513, 1025])
@pytest.mark.parametrize("form", [0, 1])
def test_candidate_counts(star, plain, M, form):
    """The odd tail and the scalar store path (M = 1, 511, 513, 1025: the last lane holds one candidate, and an odd M
    makes the whole last workgroup store entry by entry), one, two and three workgroups of candidates."""
    rng = np.random.default_rng(300 + M)
    m, n_q, D = 31, 3, 10
    hand = Hand(rng, star_design(rng, n_q, m, D, "axis"), [1.0, 0.6, 1.0], "RQ_kernel", m, form)
    check_paths(star, plain, hand, rng.random((M, D)), f"M={M} form={form}")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("D,ard", [(3, False), (20, True), (33, False), (3, True), (20, False), (33, True)])
def test_kernel_families_and_dimension_buckets(star, plain, kernel, D, ard):
    """SE, RQ, Matern-5/2 and Matern-3/2, isotropic and with per-dimension length scales, in the D buckets 4, 20 and 48."""
    rng = np.random.default_rng(D * 10 + ard)
    m, n_q = 9, 4
    l = rng.uniform(0.5, 1.5, D) * np.sqrt(D / 3.0) * 0.5 if ard else 0.5 * np.sqrt(D / 3.0)
    hand = Hand(rng, star_design(rng, n_q, m, D, "general" if ard else "axis", zero_row=True), [1.0, l, 1.4], kernel, m, 1)
    check_paths(star, plain, hand, rng.random((130, D)), f"{kernel} D={D} ard={ard}")


def test_edge_values(star):
    """A candidate on a design row of a real posterior: var >= -1e-12 sf2.  A candidate with a NaN coordinate: a NaN row
    that is never the argmax."""
    from ppbo_amd.engine import FORM_EDGE, SCORE_VARIANCE
    rng = np.random.default_rng(5)
    m, n_q, D = 15, 6, 5
    N = n_q * (m + 1)
    X = star_design(rng, n_q, m, D, "axis")
    th = [1.0, 0.4, 1.3]
    S = star.gram(X, th, "SE_kernel")
    f = 0.5 * star.dgemv(star.potrf_(S.clone()), rng.standard_normal(N), lower=True)
    post = star.posterior(X, th, "SE_kernel", star.pd_inverse(S), f, m, form=FORM_EDGE)
    Xc = np.concatenate([X[[0, 1, 17, N - 1]], rng.random((96, D))])
    Xc[50, 2] = np.nan
    out = star.predict(post, Xc, score=SCORE_VARIANCE, want_score=True)
    mu, var, sc = host(out["mu"]), host(out["var"]), host(out["score"])
    assert np.isnan(mu[50]) and np.isnan(var[50]) and np.isnan(sc[50])
    ok = np.arange(Xc.shape[0]) != 50
    assert np.all(np.isfinite(mu[ok])) and np.all(var[ok] >= -1e-12 * th[2] ** 2)
    assert out["best_idx"] != 50 and out["best_idx"] == int(np.nanargmax(sc))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def fixtures(star, plain):
    """c2 and c3 scored once on both paths (their own 512 candidates), shared by the tests below."""
    from ppbo_amd.engine import FORM_EDGE, SCORE_POINTWISE_EI
    out = {}
    for name in ("c2", "c3"):
        g = load(name)
        th, kern, m = g["theta"], str(g["kernel"]), int(g["m"])
        res = []
        for e in (star, plain):
            post = e.posterior(g["X"], th, kern, e.pd_inverse(e.gram(g["X"], th, kern)), g["fMAP"], m, form=FORM_EDGE)
            res.append(e.predict(post, g["Xc"], score=SCORE_POINTWISE_EI, mustar=float(np.max(g["mu"])), want_score=True))
        out[name] = (g, res[0], res[1])
    return out


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_fixtures_both_paths_and_the_golden_vectors(fixtures, name):
    """var between the paths <= 1e-8 sf2, against the golden vectors <= 1e-6 sf2; mu <= 1e-9 relative; the switch and the
    default give the same argmax."""
    g, a, b = fixtures[name]
    sf2 = float(g["theta"][2]) ** 2
    mu_a, mu_b, var_a, var_b = host(a["mu"]), host(b["mu"]), host(a["var"]), host(b["var"])
    print(f"{name}: var star-plain {np.abs(var_a - var_b).max() / sf2:.2e} sf2, var star-golden "
          f"{np.abs(var_a - g['var']).max() / sf2:.2e} sf2, mu star-plain {np.abs(mu_a - mu_b).max() / np.abs(mu_b).max():.2e}, "
          f"mu star-golden {np.abs(mu_a - g['mu']).max() / np.abs(g['mu']).max():.2e}")
    assert np.abs(var_a - var_b).max() <= 1e-8 * sf2
    assert np.abs(var_a - g["var"]).max() <= 1e-6 * sf2
    assert np.abs(mu_a - mu_b).max() <= 1e-9 * np.abs(mu_b).max()
    assert a["best_idx"] == b["best_idx"] == int(np.argmax(host(a["score"])))


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_fixtures_kstar_entries(star, plain, name):
    """K* of the fixture's 512 candidates, every row, star path against the plain path and against direct differences:
    <= 1e-12 sf2."""
    g = load(name)
    th, kern, m = [float(t) for t in g["theta"]], str(g["kernel"]), int(g["m"])
    X, Xc = g["X"], g["Xc"]
    N = X.shape[0]
    rows = np.arange(N)
    hand = Hand(np.random.default_rng(0), X, th, kern, m, 1)
    Ka, Kb = kstar_rows(star, hand, Xc, rows), kstar_rows(plain, hand, Xc, rows)
    K0 = kstar_ref(X[rows], Xc, th, kern)
    sf2 = th[2] ** 2
    print(f"{name}: K* star-plain {np.abs(Ka - Kb).max() / sf2:.2e} sf2, star-direct {np.abs(Ka - K0).max() / sf2:.2e} sf2, "
          f"plain-direct {np.abs(Kb - K0).max() / sf2:.2e} sf2 over {len(rows)} rows")
    assert np.abs(Ka - Kb).max() <= 1e-12 * sf2
    assert np.abs(Ka - K0).max() <= 1e-12 * sf2
    assert not np.array_equal(Ka, Kb)          # (the fixtures' stars are collinear: the star path ran)
