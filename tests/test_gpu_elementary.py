"""GPU: the hand-written fp64 elementary functions -- exp_nonpos, sqrt_nonneg (csrc/common.h) and rff_cos_fast
(csrc/rffmath.h) -- per element, through every device path that evaluates a covariance or a random-Fourier feature.
Each call is shaped so that ONE output element is ONE function value (the other point of every pair is the origin, the
weights are one-hot: all other terms add exact zeros), and each value is compared with mpmath at 300 bits on the exact
fp64 inputs (elementary_points.py; test_elementary_host.py shows on the CPU that the bounds are attainable).
Part 4: candidate rows with a NaN or infinite coordinate in ppbo_predict / ppbo_predict_record."""
import ctypes as C
import os

import mpmath
import numpy as np
import pytest

import elementary_points as ep

pytestmark = pytest.mark.gpu

TWO51 = 2.0 ** -51
RADIAL = ["SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel"]
THETA = (0.1, ep.LENGTHSCALE, 1.0)          # (sigma, l = 2^-6, sigma_f = 1)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def eng_valu():
    """A ctx whose ppbo_rff_score runs rff_score_kernel (the switch is read once per ctx)."""
    from ppbo_amd.engine import Engine
    old = os.environ.get("PPBO_RFF_SCORE_MFMA")
    os.environ["PPBO_RFF_SCORE_MFMA"] = "0"
    try:
        e = Engine(0)
    finally:
        if old is None:
            del os.environ["PPBO_RFF_SCORE_MFMA"]
        else:
            os.environ["PPBO_RFF_SCORE_MFMA"] = old
    yield e
    e.close()


def host(t):
    return t.detach().cpu().numpy()


# ---- part 1: the covariance values -----------------------------------------------------------------------------------------
def coords(kernel):
    if kernel == "Matern52_kernel":
        return ep.matern_points(52)
    if kernel == "Matern32_kernel":
        return ep.matern_points(32)
    if kernel == "RQ_kernel":
        return ep.rq_points()
    return ep.exp_points()[0]


def rows(x, D):
    """Points with x in the first coordinate and zeros in the others."""
    X = np.zeros((len(x), D))
    X[:, 0] = x
    return X


def matern_bound(nu):
    """|k - k_exact| allowed at each point of matern_points(nu), sigma_f = 1, as first-order error propagation through
    matern_ae / matern_value (common.h) with u = 2^-52:
      a^ = fl(c0 * sqrt_nonneg(s)): sqrt_nonneg within 1 ulp (<= u relative) and one rounding of the product (u / 2):
                                    a^ = a (1 + da), |da| <= 1.5 u
      e^ = exp_nonpos(-a^):         exp(-a^) = exp(-a) (1 -+ a da): relative 1.5 a u; then exp_nonpos's own 1 ulp(e),
                                    which is 5e-324 where e is subnormal or flushed to 0
      p^ = 1 + a^ + a^2 / 3 (resp. 1 + a^):  a p'(a) / p(a) < 2, so da costs 3 u; the rounded 1/3 and the two fma
                                    roundings (one addition for nu = 3/2) at most 1.25 u
      k^ = fl(sf2 * fl(p^ e^)):     two roundings, u / 2 each, the last one at least 5e-324 / 2 absolute
    bound(a) = p(a) (ulp(exp(-a)) + 1.5 a u exp(-a)) + 5.5 u k + 5e-324,   with 3 + 1.25 + 0.5 + 0.5 = 5.25 <= 5.5."""
    a, val = ep.matern_reference(nu)
    u = mpmath.mpf(2) ** -52
    out = []
    with ep.mp_ctx():
        for t, k in zip(a, val):
            e = mpmath.exp(-t)
            p = 1 + t + t * t / 3 if nu == 52 else 1 + t
            ulp_e = mpmath.mpf(float(np.spacing(ep.mp_to_float(e))))
            out.append(p * (ulp_e + 1.5 * t * u * e) + 5.5 * u * k + mpmath.mpf(5e-324))
    return out


_BOUNDS = {}


def check_cov(kernel, got, label):
    """got[i] = k(x_i, 0) at coords(kernel) against the kernel's bound; prints and returns the measured worst case."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    x = coords(kernel)
    assert got.shape == x.shape and np.all(np.isfinite(got)) and np.all(got >= 0.0)
    if kernel in ("SE_kernel", "RQ_kernel"):
        cr, exact = ep.exp_reference() if kernel == "SE_kernel" else ep.rq_reference()
        dist = np.abs(ep.ordinal(got) - ep.ordinal(cr))
        with ep.mp_ctx():
            abs_err = [abs(mpmath.mpf(g) - e) for g, e in zip(got.tolist(), exact)]
            err = np.array([float(d / u) for d, u in zip(abs_err, ep.spacing(cr).tolist())])
            rel = np.array([float(d / e) for d, e in zip(abs_err, exact)]) if kernel == "RQ_kernel" else None
        assert got[x == 0.0].tolist() == [1.0] * int((x == 0.0).sum())
        if kernel == "SE_kernel":
            arg = ep.exp_points()[1]
            sub = cr < 2.2250738585072014e-308
            print(f"{label} {kernel}: worst {err[~sub].max():.3f} ulp (normal), {err[sub].max():.3f} ulp of 5e-324 "
                  f"(subnormal band); at most {dist.max()} representable values from the rounded reference")
            assert np.all(got[arg <= -745.2] == 0.0), "exp must be exactly 0 below the underflow threshold and the clamp"
            i = int(dist.argmax())
            assert dist[i] <= 1, (label, kernel, x[i], got[i], cr[i])
            return err.max()
        # RQ: sf2 / (t * t).  Where t = 1 + c0 s is exact (the first RQ_EXACT_T points) the product and the division are
        # the only roundings: 2 ulp.  Where t is rounded as well (the 26-bit coordinates) its 2^-53 doubles in t^2:
        # (2 + 1 + 1) 2^-53 = 4 x 2^-53 relative, which is between 2 and 4 ulp -- 2 ulp is not attainable there (the
        # same three IEEE operations in NumPy reach 2.55 ulp on these points)
        n = ep.RQ_EXACT_T
        print(f"{label} {kernel}: exact t: worst {err[:n].max():.3f} ulp, at most {dist[:n].max()} representable values "
              f"from the rounded reference; rounded t: worst {rel[n:].max() * 2.0 ** 53:.3f} x 2^-53 relative "
              f"({err[n:].max():.3f} ulp)")
        i = int(dist[:n].argmax())
        assert dist[i] <= 2, (label, kernel, x[i], got[i], cr[i])
        i = n + int(rel[n:].argmax())
        assert rel[i] <= 4.0 * 2.0 ** -53, (label, kernel, x[i], got[i], cr[i])
        return err.max()
    nu = 52 if kernel == "Matern52_kernel" else 32
    if nu not in _BOUNDS:
        _BOUNDS[nu] = matern_bound(nu)
    a, val = ep.matern_reference(nu)
    with ep.mp_ctx():
        err = [abs(mpmath.mpf(g) - v) for g, v in zip(got.tolist(), val)]
        ratio = np.array([float(e / b) for e, b in zip(err, _BOUNDS[nu])])
        ulps = np.array([float(e / mpmath.mpf(float(np.spacing(ep.mp_to_float(v))))) for e, v in zip(err, val)])
        af = np.array([float(t) for t in a])
    i = int(ratio.argmax())
    print(f"{label} {kernel}: worst error {ratio[i]:.3f} of the bound (a = {af[i]:.3f}, {ulps[i]:.1f} ulp); largest "
          f"{ulps.max():.1f} ulp at a = {af[ulps.argmax()]:.1f}; {ulps[af < 40].max():.2f} ulp for a < 40")
    assert got[x == 0.0].tolist() == [1.0], "s = 0 must give exactly sigma_f^2"
    assert np.all(got[af >= 800.0] == 0.0), "the cap at a = 800 must give exactly 0"
    assert (af >= 800.0).sum() >= 32 and (af < 40).sum() > 1000
    assert ratio[i] <= 1.0, (label, kernel, x[i], got[i], float(val[i]))
    return ratio[i]


@pytest.mark.parametrize("D", [1, 20])
@pytest.mark.parametrize("kernel", RADIAL)
def test_cross_cov_per_element(eng, kernel, D):
    """ppbo_cross_cov with X1 = the origin: K[0, j] = k(x_j, 0) from direct differences (crosscov_kernel).  SE within 1
    representable value of the rounded exp, RQ within 2 (exact t; 4 x 2^-53 relative where t is rounded), Matern inside
    matern_bound; exact 0 below the underflow threshold / at the cap, exact sigma_f^2 at 0.
    Measured (MI355X, the same on every entry point and D): SE 0.854 ulp, 0.695 ulp of 5e-324 in the subnormal band, never
    more than 1 representable value off; RQ 1.313 ulp with exact t, 2.826 x 2^-53 relative (2.551 ulp) with rounded t;
    Matern-5/2 0.500 of the bound (a = 734.6, exp(-a) subnormal), 27.1 ulp for a < 40; Matern-3/2 0.492 of the bound,
    29.2 ulp for a < 40."""
    x = coords(kernel)
    K = host(eng.cross_cov(np.zeros((1, D)), rows(x, D), THETA, kernel))
    check_cov(kernel, K[0], f"cross_cov D={D}")


@pytest.mark.parametrize("D", [1, 20])
@pytest.mark.parametrize("kernel", RADIAL)
def test_gram_per_element(eng, kernel, D):
    """ppbo_gram with shrink = 0 and row 0 = the origin (gram_mfma_kernel: the expansion |x|^2 + |0|^2 - 2 x.0 is x^2
    exactly): row 0 and column 0 per element, bitwise equal to each other, and a diagonal of exactly sigma_f^2."""
    x = coords(kernel)
    S = eng.gram(np.concatenate([np.zeros((1, D)), rows(x, D)]), THETA, kernel, shrink=0.0)
    row, col, diag = host(S[0, 1:]), host(S[1:, 0]), host(S.diagonal())
    assert np.array_equal(row, col)
    assert np.all(diag == 1.0)
    check_cov(kernel, row, f"gram D={D}")


def one_hot_model(eng, kernel, N, D, with_G):
    """A ppbo_model by hand: design row 0 = the origin, alpha = e_0, so mu(x_c) = k(x_c, 0) and every other row adds an
    exact zero.  with_G: a zero node-form operator and zero Lambda (the one-launch kernel only takes models that carry an
    operator); else d_G = NULL, the mean-only three-launch form."""
    import torch
    from ppbo_amd import _lib
    from ppbo_amd.engine import KERNEL_IDS
    X = np.random.default_rng(N).random((N, D))
    X[0] = 0.0
    keep = dict(X=eng.dev(X), alpha=torch.zeros(N, dtype=torch.float64, device=eng.device))
    keep["alpha"][0] = 1.0
    md = _lib.Model()
    md.kernel_id, md.N, md.D, md.m = KERNEL_IDS[kernel], N, D, 12
    md.theta = eng._theta(THETA)
    md.d_X, md.d_alpha = keep["X"].data_ptr(), keep["alpha"].data_ptr()
    md.d_lam_diag = md.d_lam_off = md.d_G = md.d_Gt = 0
    md.kstar_fp32, md.form = 0, 0
    if with_G:
        keep["z"] = torch.zeros(N, dtype=torch.float64, device=eng.device)
        keep["G"] = torch.zeros(N, N, dtype=torch.float64, device=eng.device)
        md.d_lam_diag = md.d_lam_off = keep["z"].data_ptr()
        md.d_G = keep["G"].data_ptr()
    return md, keep


@pytest.mark.parametrize("N,D,fused", [(52, 1, True), (1300, 20, False)])
@pytest.mark.parametrize("kernel", RADIAL)
def test_predict_mean_per_element(eng, kernel, N, D, fused):
    """ppbo_predict's mean through a one-hot model: N = 52 is scored by the one-launch kernel (fused.hip; it needs an
    operator, here a zero G), N = 1300 with d_G = NULL by kstar_kernel -- the profile counters say which ran, and
    ppbo_posterior_form names the same split."""
    from ppbo_amd.engine import FORM_EDGE, FORM_NODE
    x = coords(kernel)
    md, keep = one_hot_model(eng, kernel, N, D, with_G=fused)
    assert eng.posterior_form(kernel, N, D, 12) == (FORM_NODE if fused else FORM_EDGE)
    Xc, mu = eng.dev(rows(x, D)), eng.empty(len(x))
    eng.profile(True)
    try:
        rc = eng.lib.ppbo_predict(eng.ctx, C.byref(md), C.c_void_p(Xc.data_ptr()), len(x), 0, 0.0,
                                  C.c_void_p(mu.data_ptr()), None, None, None, None, eng._stream())
        eng._check(rc, "ppbo_predict")
        n_fused, n_kstar = eng.profile_read("fused_score")[1], eng.profile_read("kstar")[1]
    finally:
        eng.profile(False)
    assert (n_fused, n_kstar) == ((1, 0) if fused else (0, 1))
    check_cov(kernel, host(mu), f"predict N={N} ({'fused' if fused else 'kstar'})")


@pytest.mark.parametrize("D", [1, 20])
@pytest.mark.parametrize("kernel", RADIAL)
def test_path_score_kernel_half_per_element(eng, kernel, D):
    """ppbo_path_score_multi with W_prior = 0 and V = e_0: score[0][c] = k(x_c, 0) from the kernel half of
    path_score_multi_kernel (r^2 = |x_c|^2 - 2 (x_i.x_c - |x_i|^2 / 2) on the matrix cores)."""
    x = coords(kernel)
    N, F = 40, 32
    X = np.random.default_rng(3).random((N, D))
    X[0] = 0.0
    V = np.zeros((1, N))
    V[0, 0] = 1.0
    W = np.random.default_rng(4).standard_normal((F, D))
    sc = eng.path_score_multi(rows(x, D), W, np.zeros(F), THETA, kernel, X, np.zeros((1, F)), V)
    check_cov(kernel, host(sc)[0], f"path_score_multi D={D}")


# ---- part 2: the cosine ----------------------------------------------------------------------------------------------------
def blocks():
    ph, _ = ep.cos_points()
    return [ph[i:i + ep.COS_F] for i in range(0, len(ph), ep.COS_F)]


def basis(block, via, D):
    """(W [F, D], b [F]) whose phase against x = (1, 0, ..., 0) is block[f] exactly: W[f, 0] = block[f] and b = 0
    (via = "W"; the other columns of W meet zero coordinates), or W = 0 and b = block (via = "b")."""
    W = np.zeros((ep.COS_F, D))
    b = np.zeros(ep.COS_F)
    if via == "W":
        W[:, 1:] = np.random.default_rng(9).standard_normal((ep.COS_F, D - 1))
        W[:, 0] = block
    else:
        b[:] = block
    return W, b


def ones_rows(n, D):
    X = np.zeros((n, D))
    X[:, 0] = 1.0
    return X


def check_cos(got, label, idx=None):
    """got[i] = cos(phase_i) (at the indices idx of cos_points(), default all) within 2^-51 absolute, with the right sign
    next to every k pi/2, exactly 1 at +-0 and bitwise even; prints the worst case of the fast and the library range."""
    ph, near = ep.cos_points()
    ref = ep.cos_reference()
    full = idx is None
    idx = np.arange(len(ph)) if full else np.asarray(idx)
    got = np.ascontiguousarray(got, dtype=np.float64)
    assert got.shape == idx.shape
    p, r, nr = ph[idx], ref[idx], near[idx]
    err = np.abs(got - r)
    fast = np.abs(p) < ep.COS_FAST_RANGE
    parts = [f"{name} {err[m].max() * 2.0 ** 53:.4f} x 2^-53 at {p[m][err[m].argmax()]!r}"
             for name, m in (("fast range", fast), ("library range", ~fast)) if m.any()]
    print(f"{label}: worst |error| " + ", ".join(parts))
    i = int(np.nanargmax(np.where(np.isnan(err), np.inf, err)))
    assert err[i] <= TWO51, (label, p[i], got[i], r[i])
    assert np.array_equal(np.signbit(got[nr]), np.signbit(r[nr])), "wrong side of a zero of the cosine"
    assert np.all(got[p == 0.0] == 1.0)
    if full:
        assert np.array_equal(got, got[ep.cos_negated_index()]), "cos(-x) != cos(x)"
    return err.max()


def test_cos_points_mix_both_paths_in_every_group():
    ph, _ = ep.cos_points()
    slow = ~(np.abs(ph) < ep.COS_FAST_RANGE)
    for g in (4, 64):
        s = slow.reshape(-1, g)
        assert np.all(s.any(axis=1)) and np.all((~s).any(axis=1))


@pytest.mark.parametrize("via", ["W", "b"])
@pytest.mark.parametrize("D,N", [(1, 2), (1, 1), (20, 2)])
def test_rff_project_cos_per_element(eng, via, D, N):
    """ppbo_rff_project, Phi[f, n] = cos(phase_f) for every point n: the 16-byte-store form (N = 2) and the scalar one
    (N = 1), dimension buckets 4 and 20.
    Measured (MI355X, the same on every entry point): fast range 2.0000 x 2^-53 (at 980365.8988048842), library range
    1.0000 x 2^-53 (at 4542589.448146066); bound 4 x 2^-53."""
    got = []
    for block in blocks():
        W, b = basis(block, via, D)
        Phi = host(eng.rff_project(ones_rows(N, D), W, b, ep.COS_SIGMA_F))
        assert all(np.array_equal(Phi[:, 0], Phi[:, n]) for n in range(N))
        got.append(Phi[:, 0])
    check_cos(np.concatenate(got), f"rff_project D={D} N={N} via {via}")


@pytest.mark.parametrize("via", ["W", "b"])
def test_rff_score_multi_cos_per_element(eng, via):
    """ppbo_rff_score_multi with Omega = the identity (S = F = 512): score[s][c] = cos(phase_s) for both candidates.
    Measured: as test_rff_project_cos_per_element (the same routine on the same phases)."""
    got = []
    for block in blocks():
        W, b = basis(block, via, 1)
        sc = host(eng.rff_score_multi(ones_rows(2, 1), W, b, ep.COS_SIGMA_F, np.eye(ep.COS_F)))
        assert np.array_equal(sc[:, 0], sc[:, 1])
        got.append(sc[:, 0])
    check_cos(np.concatenate(got), f"rff_score_multi via {via}")


@pytest.mark.parametrize("via", ["W", "b"])
def test_path_score_feature_half_cos_per_element(eng, via):
    """ppbo_path_score_multi with V = 0 and W_prior = the identity: the feature half of path_score_multi_kernel
    (sigma_f = 16 and F = 512 through theta; the kernel half adds 0 x k)."""
    X = np.random.default_rng(5).random((8, 1))
    got = []
    for block in blocks():
        W, b = basis(block, via, 1)
        sc = host(eng.path_score_multi(ones_rows(1, 1), W, b, (0.1, 0.5, ep.COS_SIGMA_F), "SE_kernel", X,
                                       np.eye(ep.COS_F), np.zeros((ep.COS_F, 8))))
        got.append(sc[:, 0])
    check_cos(np.concatenate(got), f"path_score_multi via {via}")


@pytest.mark.parametrize("mfma", [1, 0])
def test_rff_score_cos_per_element(eng, eng_valu, mfma):
    """ppbo_rff_score, rff_score_mfma_kernel (default) and rff_score_kernel (PPBO_RFF_SCORE_MFMA=0), omega one-hot.
    (a) every phase as a CANDIDATE against the weight w_0 = 1 (phase = 1 x_c + 0 exactly): the lanes of a wavefront
        hold different candidates, so this is where rff_score_kernel's ballot sees mixed groups;
    (b) x = 1 and phase = W_f (then b_f), one call per feature for a subset of 48 features that holds every kind of
        phase of the sweep."""
    e = eng if mfma else eng_valu
    ph, near = ep.cos_points()
    F = ep.COS_F
    W = np.zeros((F, 1))
    W[0, 0] = 1.0
    om = np.zeros(F)
    om[0] = 1.0
    sc, _, _ = e.rff_score(np.array(ph).reshape(-1, 1), W, np.zeros(F), ep.COS_SIGMA_F, om)
    check_cos(host(sc), f"rff_score mfma={mfma} (a) phases as candidates")
    rng = np.random.default_rng(48)
    special = np.flatnonzero((ph == 0.0) | (np.abs(ph) == 5e-324) | (np.abs(ph) == 1e-300) |
                             (np.abs(ph) == ep.COS_FAST_RANGE) | (np.abs(ph) == np.nextafter(ep.COS_FAST_RANGE, 0.0)))
    idx = np.unique(np.concatenate([special, rng.choice(np.flatnonzero(near), 16, replace=False),
                                    rng.choice(len(ph), 48 - 16 - len(special), replace=False)]))
    for via in ("W", "b"):
        got = []
        for i in idx:
            blk = blocks()[i // F]
            Wb, b = basis(blk, via, 1)
            om = np.zeros(F)
            om[i % F] = 1.0
            s, _, _ = e.rff_score(ones_rows(2, 1), Wb, b, ep.COS_SIGMA_F, om)
            s = host(s)
            assert s[0] == s[1]
            got.append(s[0])
        check_cos(np.array(got), f"rff_score mfma={mfma} (b) via {via}", idx)


# ---- part 4: candidate rows with a non-finite coordinate ----------------------------------------------------------------------
def fitted(eng, kernel, N, form):
    rng = np.random.default_rng(N + len(kernel))
    D, m = 6, 12
    X = rng.random((N, D))
    th = [1.0, 0.4, 1.3]
    Sigma = eng.gram(X, th, kernel)
    f = 0.5 * eng.dgemv(eng.potrf_(Sigma.clone()), rng.standard_normal(N), lower=True)
    return eng.posterior(X, th, kernel, eng.pd_inverse(Sigma), f, m, form=form)


@pytest.mark.parametrize("N", [52, 1300])
@pytest.mark.parametrize("kernel", RADIAL + ["camphor_copper_kernel"])
def test_predict_non_finite_candidate_rows(eng, kernel, N):
    """A candidate row with a NaN or infinite coordinate gets NaN in mu, var and score and never wins the argmax; the
    finite rows are bit for bit those of the same call with finite values in the bad rows; when every row is bad the
    best is (NaN, -1), from ppbo_predict and in ppbo_predict_record's record.  All five kernels (D = 6), the three
    scores, N = 52 (node form: the one-launch kernel for the radial kernels) and N = 1300, both operator forms and the
    mean-only call without an operator; M = 300 with bad rows at 0, 127, 128 and the last."""
    from ppbo_amd.engine import FORM_EDGE, FORM_NODE, SCORE_MEAN, SCORE_POINTWISE_EI, SCORE_VARIANCE
    M, D = 300, 6
    rng = np.random.default_rng(N)
    clean = rng.random((M, D))
    bad = np.array([0, 127, 128, M - 1])
    dirty = clean.copy()
    dirty[0, 0] = np.nan
    dirty[127, 3] = np.inf
    dirty[128, D - 1] = -np.inf
    dirty[M - 1] = np.nan
    good = np.setdiff1d(np.arange(M), bad)
    for form in (FORM_NODE, FORM_EDGE):
        post = fitted(eng, kernel, N, form)
        fused = form == FORM_NODE and N == 52 and kernel != "camphor_copper_kernel"
        eng.profile(True)
        try:
            eng.predict(post, clean, score=SCORE_VARIANCE)
            assert (eng.profile_read("fused_score")[1], eng.profile_read("kstar")[1]) == ((1, 0) if fused else (0, 1))
        finally:
            eng.profile(False)
        mustar = float(host(eng.predict(post, clean)["mu"]).max())
        for score, want_var in ((SCORE_MEAN, True), (SCORE_POINTWISE_EI, True), (SCORE_VARIANCE, True), (SCORE_MEAN, False)):
            a = eng.predict(post, clean, score=score, mustar=mustar, want_var=want_var, want_score=True)
            b = eng.predict(post, dirty, score=score, mustar=mustar, want_var=want_var, want_score=True)
            for key in ("mu", "var", "score"):
                if a[key] is None:
                    assert key == "var" and not want_var
                    continue
                ya, yb = host(a[key]), host(b[key])
                assert np.all(np.isnan(yb[bad])), (kernel, N, form, score, key, yb[bad])
                assert np.array_equal(ya[good], yb[good]), (kernel, N, form, score, key)
            sb = host(b["score"])
            first = int(good[np.argmax(sb[good])])
            assert (b["best_idx"], b["best_val"]) == (first, sb[first])
            # (predict_record hands the operator over for the variance scores only: its mean-score record is the
            # mean-only call's, which a model the one-launch kernel takes matches to rounding, not bit for bit)
            rec = host(eng.predict_record(post, dirty, score=score, mustar=mustar, index_offset=1000))
            if score != SCORE_MEAN or not want_var:
                assert (rec[0], rec[1]) == (sb[first], 1000.0 + first)
            else:
                assert rec[1] >= 1000.0 and int(rec[1]) - 1000 in good and rec[0] == rec[0]
            # a bad row placed where the clean call's best sits does not win either
            moved = clean.copy()
            moved[a["best_idx"], 1] = np.nan
            c = eng.predict(post, moved, score=score, mustar=mustar, want_var=want_var, want_score=True)
            assert c["best_idx"] != a["best_idx"] and c["best_val"] <= a["best_val"]
            # nothing finite: (NaN, -1)
            none = eng.predict(post, np.full((M, D), np.nan), score=score, mustar=mustar, want_var=want_var)
            assert none["best_idx"] == -1 and np.isnan(none["best_val"])
            rec = host(eng.predict_record(post, np.full((M, D), np.inf), score=score, mustar=mustar, index_offset=1000))
            assert np.isnan(rec[0]) and rec[1] == -1.0
