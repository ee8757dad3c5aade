"""CPU: the curvature surface (ppbo_predict_curvatures / Engine.predict_curvatures / GPModel.curvature_pred / sharpness /
mean_hessian) -- the NumPy statement itself against central differences of the slope statement, the prior constants
against second differences of the column, the embedded camphor identity, the binding table, and the refusals that are
decided before anything reaches a device."""
import os
import re
import types

import numpy as np
import pytest

import curvature_numpy as cn
import slopes_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIAL = ("SE_kernel", "RQ_kernel", "Matern52_kernel")
LS6 = np.array([0.4, 0.6, 0.5, 1.0, 0.8, 0.7])

# 1. The column is the derivative, along the path, of the slope column: with a unit direction u and step h,
#    (g(x + h u; u + h a) - g(x - h u; u - h a)) / 2h, g = slopes_numpy.slope_column, truncates at h^2 / 6 times the
#    ratio of the column's third derivative along the path to the column itself -- at most a few (1 / l_eff)^2, with
#    l_eff the shortest length the kernel varies on (0.25 for the radial cases, l / 2 pi = 0.064 for camphor's periodic
#    dimensions) -- and rounds at eps / h of the slope column's scale.  H1 = 1e-5: truncation <= 1e-10 / 6 * 10 / 0.064^2
#    = 4e-8, rounding ~ 1e-11 / l_eff.  FD_TOL = 1e-6 is 25 times that; a wrong coefficient (SE's 2 c0^2 for 4 c0^2, a
#    missing n2 term, a wrong sign of d^2 s) is an error of order 1.
# 2. The prior is the second derivative, in the design point y = x + b u at b = 0, of the column c(x, u; y) (the
#    covariance of the curvature at x with f(y), differentiated twice more): the second central difference
#    (c(x; x + h u) - 2 c(x; x) + c(x; x - h u)) / h^2.  It rounds at 4 eps c(x; x) / (h^2 prior) = 4 eps l^2 / (q h^2)
#    (c(x; x) = sf^2 / l^2 times 1, 1, 5/3; q = 3, 9/2, 25) and truncates at h^2 / 12 times the ratio of the kernel's
#    sixth to its fourth derivative at 0 (SE: 5 / l^2).  H2 = 2e-5: rounding <= 4 * 2.2e-16 * 0.36 / (3 * 4e-10) = 2.7e-7
#    (SE, l = 0.6), truncation <= 4e-10 * 5 / (12 * 0.064^2) = 4e-8 (camphor).  Held to FD_TOL = 1e-6 -- except Matern-5/2,
#    whose kernel has the odd term -sf^2 |a|^5 / 45 (a = sqrt5 r / l): its column along the line carries
#    -(4/9) sf^2 c0^2 |a|^3, whose second difference adds the FIRST-order term (8/9) sqrt5 h / l relative to the prior
#    (at most 1.6e-4 for l = 0.25).  That bound is added for Matern-5/2 alone; the constant 25 (against 3 or 9/2) misses it
#    by four orders.  This pins 3, 9/2, 25 and the camphor constant without a fourth-order difference.
# Observed on the CPU (the worst case of each kind): column 2.1e-9 (radial), 3.4e-8 (camphor), with an acceleration
# 7.0e-9; prior 9.3e-8 (SE, RQ), 3.1e-8 (camphor); Matern-5/2 1.14e-4 of its 1.15e-4 (l = 0.35) and 1.27e-4 of its 1.31e-4
# (ARD): the first-order term is what is seen, the next one has the other sign.
H1 = 1e-5
H2 = 2e-5
FD_TOL = 1e-6
EPS = np.finfo(float).eps


def _case(kernel, ard):
    """(X, theta, Xq, Xi) of a small design with queries (some ON design rows) and directions of every length."""
    rng = np.random.default_rng(len(kernel) + 17 * ard)
    cam = kernel in (sn.CAMPHOR, sn.CAMPHOR_ARD)
    D = 6 if cam else 4
    if kernel == sn.CAMPHOR_ARD:
        l = LS6
    elif cam:
        l = 0.5
    else:
        l = rng.uniform(0.25, 0.6, D) if ard else 0.35
    theta = [0.05, l, 0.7]
    X = rng.random((20, D))
    Xq = rng.random((40, D))
    Xq[:4] = X[:4]
    Xi = rng.standard_normal((40, D))
    Xi[:5] *= 1e-3
    Xi[5:10] *= 30.0
    return X, theta, Xq, Xi


CASES = [(k, False) for k in RADIAL] + [(k, True) for k in RADIAL] + [(sn.CAMPHOR, False), (sn.CAMPHOR_ARD, True)]


@pytest.mark.parametrize("kernel,ard", CASES)
def test_column_is_the_central_difference_of_the_slope_column(kernel, ard):
    X, theta, Xq, Xi = _case(kernel, ard)
    n = np.linalg.norm(Xi, axis=1)[:, None]
    U = Xi / n
    c = cn.curvature_column(Xq, Xi, X, theta, kernel)
    fd = (sn.slope_column(Xq + H1 * U, U, X, theta, kernel) - sn.slope_column(Xq - H1 * U, U, X, theta, kernel)) / (2.0 * H1) * n * n
    e = np.max(np.abs(c - fd) / np.abs(c).max(axis=1, keepdims=True))
    print(f"curvature column {kernel} ard={ard}: {e:.2e}")
    assert e <= FD_TOL
    if kernel in RADIAL:
        # a curved path: gamma(a) = x + a u + a^2 acc / 2, gamma'(a) = u + a acc
        Xa = np.random.default_rng(5).standard_normal(Xi.shape) * 3.0
        ca = cn.curvature_column(Xq, U, X, theta, kernel, Xa)
        hp = sn.slope_column(Xq + H1 * U + 0.5 * H1 * H1 * Xa, U + H1 * Xa, X, theta, kernel)
        hm = sn.slope_column(Xq - H1 * U + 0.5 * H1 * H1 * Xa, U - H1 * Xa, X, theta, kernel)
        ea = np.max(np.abs(ca - (hp - hm) / (2.0 * H1)) / np.abs(ca).max(axis=1, keepdims=True))
        print(f"curvature column with an acceleration {kernel} ard={ard}: {ea:.2e}")
        assert ea <= FD_TOL
        assert not np.array_equal(ca, cn.curvature_column(Xq, U, X, theta, kernel))


@pytest.mark.parametrize("kernel,ard", CASES)
def test_prior_is_the_second_difference_of_the_column_in_the_design_point(kernel, ard):
    _, theta, Xq, Xi = _case(kernel, ard)
    n = np.linalg.norm(Xi, axis=1)
    U = Xi / n[:, None]
    col = lambda i, y: cn.curvature_column(Xq[i:i + 1], U[i:i + 1], y[None, :], theta, kernel)[0, 0]  # noqa: E731
    fd = np.array([(col(i, Xq[i] + H2 * U[i]) - 2.0 * col(i, Xq[i]) + col(i, Xq[i] - H2 * U[i])) / (H2 * H2) for i in range(len(Xq))])
    prior = cn.curvature_prior(Xi, theta, kernel)
    e = np.max(np.abs(prior - fd * n ** 4) / prior)
    tol = FD_TOL
    if kernel == "Matern52_kernel":
        tol += 8.0 / 9.0 * np.sqrt(5.0) * H2 / np.min(np.broadcast_to(theta[1], (Xq.shape[1],)))
    print(f"curvature prior {kernel} ard={ard}: {e:.2e} (bound {tol:.2e})")
    assert e <= tol


def test_prior_constants():
    """12 kappa''(0): 3 (SE), 9/2 (RQ), 25 (Matern-5/2) times sf^2 |xi|^4 / l^4, plus the slope's constant times |acc|^2 / l^2;
    Matern-3/2 is refused."""
    xi = np.array([[0.3, -1.2, 0.5, 0.0, 2.0, -0.7]])
    acc = np.array([[1.0, 0.5, -0.25, 2.0, 0.0, 0.125]])
    sf, l = 0.7, 0.4
    n2 = (xi ** 2).sum() / l ** 2
    for kernel, q4, q2 in zip(RADIAL, (3.0, 4.5, 25.0), (1.0, 1.0, 5.0 / 3.0)):
        want = sf ** 2 * q4 * n2 * n2
        # (both sides round some ten times on the way: 16 eps)
        assert abs(cn.curvature_prior(xi, [0.05, l, sf], kernel)[0] - want) <= 16 * EPS * want
        want += sf ** 2 * q2 * (acc ** 2).sum() / l ** 2
        assert abs(cn.curvature_prior(xi, [0.05, l, sf], kernel, acc)[0] - want) <= 16 * EPS * want
    with pytest.raises(ValueError):
        cn.curvature_prior(xi, [0.05, l, sf], "Matern32_kernel")
    with pytest.raises(ValueError):
        cn.curvature_column(xi, xi, xi, [0.05, l, sf], "Matern32_kernel")
    assert cn.curvature_prior(np.zeros((1, 6)), [0.05, l, sf], sn.CAMPHOR)[0] == 0.0


def test_embedded_camphor_identity():
    """The camphor-ARD column and prior in six coordinates are the SE statement on (e(x), J_e(x) xi, e'') -- the host's
    acceleration (Engine's camphor_embed_accelerations) against second differences of the embedding first."""
    from ppbo_amd.engine import camphor_embed_accelerations, camphor_embed_directions
    from ppbo_amd.random_fourier_sampler import camphor_embed_host
    rng = np.random.default_rng(3)
    X, Xi, Xd = rng.random((9, 6)), rng.standard_normal((9, 6)), rng.random((12, 6))
    Xi[:2] *= 1e-3
    Xi[2:4] *= 30.0
    J, E2 = camphor_embed_directions(X, Xi, LS6), camphor_embed_accelerations(X, Xi, LS6)
    assert E2.shape == (9, 11) and np.all(E2[:, 4] == 0.0)
    U = Xi / np.linalg.norm(Xi, axis=1)[:, None]
    h = 1e-4         # second difference of sin / cos: rounds at eps / (2 pi h)^2 = 5e-10, truncates at (2 pi h)^2 / 12 = 3e-8
    fd = (camphor_embed_host(X + h * U, LS6) - 2.0 * camphor_embed_host(X, LS6) + camphor_embed_host(X - h * U, LS6)) / (h * h)
    E2u = camphor_embed_accelerations(X, U, LS6)
    assert np.abs(E2u - fd).max() <= 1e-6 * np.abs(E2u).max()
    assert np.array_equal(camphor_embed_accelerations(X, -Xi, LS6), E2)
    th6, th11 = [0.05, LS6, 0.7], [0.05, 1.0, 0.7]
    c6 = cn.curvature_column(X, Xi, Xd, th6, sn.CAMPHOR_ARD)
    c11 = cn.curvature_column(camphor_embed_host(X, LS6), J, camphor_embed_host(Xd, LS6), th11, "SE_kernel", E2)
    assert np.max(np.abs(c6 - c11) / np.abs(c6).max(axis=1, keepdims=True)) <= 1e-12
    p6, p11 = cn.curvature_prior(Xi, th6, sn.CAMPHOR_ARD), cn.curvature_prior(J, th11, "SE_kernel", E2)
    assert np.max(np.abs(p6 - p11) / p6) <= 1e-13
    # without the acceleration the embedded statement is another quantity
    assert np.max(np.abs(p6 - cn.curvature_prior(J, th11, "SE_kernel")) / p6) > 1e-3
    # the scalar-l camphor kernel is the profile (l, l, l + 0.05, l, l, l)
    a = cn.curvature_column(X, Xi, Xd, [0.05, 0.5, 0.7], sn.CAMPHOR)
    b = cn.curvature_column(X, Xi, Xd, [0.05, 0.5 + np.array([0, 0, 0.05, 0, 0, 0]), 0.7], sn.CAMPHOR_ARD)
    assert np.array_equal(a, b)


def test_curvature_probability():
    import scipy.stats
    mu, var = np.meshgrid(np.linspace(-3.0, 3.0, 61), np.concatenate([[-1e-3, 0.0], np.logspace(-12, 1, 27)]))
    p = cn.curvature_probability(mu, var)
    pos = var > 0
    assert np.abs(p[pos] - scipy.stats.norm.cdf(-mu[pos] / np.sqrt(var[pos]))).max() <= 4 * np.finfo(float).eps
    # var = 0 (or below): the sign of mu_c decides, mu_c = 0 gives 1/2
    assert list(cn.curvature_probability([-1.0, 0.0, 2.0, -0.0], [0.0, 0.0, -1.0, 0.0])) == [1.0, 0.5, 0.0, 0.5]
    assert np.all(cn.curvature_probability(np.zeros(29), var[:, 0]) == 0.5)
    assert np.abs(p + cn.curvature_probability(-mu, var) - 1.0).max() <= 2 * np.finfo(float).eps
    assert np.isnan(cn.curvature_probability(np.nan, 1.0)) and np.isnan(cn.curvature_probability(1.0, np.nan))


def test_reference_removes_variance_only():
    """curvature_reference on a small dense posterior: the data only ever remove variance, and the mean is c' alpha."""
    from oracle import ppbo_oracle as orc
    rng = np.random.default_rng(8)
    m, D = 3, 4
    X = rng.random((20, D))
    theta = [0.05, 0.35, 0.7]
    for kernel in RADIAL:
        Sinv = orc.pd_inverse(orc.regularize_covariance(sn.cross(X, X, theta, kernel), orc.SHRINKAGE))
        f, _ = orc.fit_fmap_newton(0.3 * rng.standard_normal(20), Sinv, m, theta[0], gtol=1e-10, maxiter=500)
        alpha, A = cn.operator_from_fit(X, theta, kernel, m, f)
        Xq, Xi = rng.random((30, D)), rng.standard_normal((30, D))
        mu, var, c = cn.curvature_reference(Xq, Xi, X, theta, kernel, alpha, A)
        prior = cn.curvature_prior(Xi, theta, kernel)
        assert np.array_equal(mu, c @ alpha)
        assert np.all(var > 0.0) and np.all(var <= prior * (1.0 + 1e-12))


# ---------------------------------------------------------------- the plumbing
def test_binding_header_and_constants():
    from ppbo_amd import _lib, engine
    assert _lib.ABI_VERSION == 9
    assert "ppbo_predict_curvatures" in _lib.SIGNATURES and len(_lib.SIGNATURES["ppbo_predict_curvatures"]) == 14
    slopes = _lib.SIGNATURES["ppbo_predict_slopes"]
    assert _lib.SIGNATURES["ppbo_predict_curvatures"] == slopes[:4] + [slopes[3]] + slopes[4:]
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "ppbo_predict_curvatures" in set(re.findall(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(", code))
    assert re.search(r"PPBO_CURV_MEAN\s*=\s*0\s*,\s*PPBO_CURV_VARIANCE\s*=\s*1\s*,\s*PPBO_CURV_PROB\s*=\s*2", code)
    sig = re.search(r"ppbo_predict_curvatures\s*\(([^)]*)\)", code).group(1)
    assert [a.split()[-1].lstrip("*") for a in sig.split(",")] == ["ctx", "model", "d_X", "d_Xi", "d_Xa", "M", "score_kind", "d_mu",
                                                                  "d_var", "d_prob", "d_score", "h_best_val", "h_best_idx", "stream"]
    assert (_lib.CURV_MEAN, _lib.CURV_VARIANCE, _lib.CURV_PROB) == (0, 1, 2)
    assert (engine.CURV_MEAN, engine.CURV_VARIANCE, engine.CURV_PROB) == (0, 1, 2)
    assert hasattr(engine.Engine, "predict_curvatures")
    from ppbo_amd.gp_model import GPModel
    assert all(hasattr(GPModel, a) for a in ("curvature_pred", "sharpness", "mean_hessian"))


def test_library_exports_the_entry_point():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    assert hasattr(_lib.load(), "ppbo_predict_curvatures")


class _NoDevice:
    """Stands where the library handle would: any call through it is a failure of the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the refusal came after a device call ({name})")


def _stub_engine():
    from ppbo_amd.engine import Engine
    eng = Engine.__new__(Engine)          # no ctx, no library: nothing below may touch either
    eng.lib, eng.ctx, eng.device = _NoDevice(), None, "none"
    eng.dev = lambda a, dtype=None: (_ for _ in ()).throw(AssertionError("the refusal came after an upload"))
    return eng


def _stub_post(camphor, D, kernel="SE_kernel"):
    from ppbo_amd.engine import Posterior
    return Posterior(kernel, (0.05, 0.3, 1.0), 3, types.SimpleNamespace(shape=(8, 11 if camphor else D)), None, None,
                     None, None, camphor=np.ones(6) if camphor else None)


@pytest.mark.parametrize("camphor", [False, True])
def test_predict_curvatures_refuses_before_the_device(camphor):
    eng = _stub_engine()
    D = 6 if camphor else 4
    post = _stub_post(camphor, D)
    z = np.zeros
    for X, Xi in ((z((5, D)), z((4, D))), (z((5, D)), z((5, D + 1))), (z((5, D + 1)), z((5, D + 1))), (z(D), z(D)),
                  (z((0, D)), z((0, D))), (z((5, D, 1)), z((5, D, 1))), (z((5, D)), z(D))):
        with pytest.raises(ValueError, match="predict_curvatures"):
            eng.predict_curvatures(post, X, Xi)
    for kind in (3, -1):
        with pytest.raises(ValueError, match="predict_curvatures.*score kind"):
            eng.predict_curvatures(post, z((5, D)), z((5, D)), score=kind)
    if not camphor:
        with pytest.raises(ValueError, match="predict_curvatures.*Matern32"):
            eng.predict_curvatures(_stub_post(False, D, "Matern32_kernel"), z((5, D)), z((5, D)))


def test_gp_model_refusals():
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = None
    gp.xstar = np.zeros(3)
    with pytest.raises(RuntimeError) as want:
        gp.mu_Sigma_pred(np.zeros((2, 3)))
    for call in (lambda: gp.curvature_pred(np.zeros(3), np.ones(3)), gp.sharpness, gp.mean_hessian,
                 lambda: gp.sharpness(np.ones(3)), lambda: gp.mean_hessian(np.ones(3))):
        with pytest.raises(RuntimeError) as got:
            call()
        assert str(got.value) == str(want.value)
    # a shape mismatch and a Matern-3/2 model are ValueErrors before anything reaches the device
    gp._post = _stub_post(False, 4)
    gp._post.G = object()
    gp.eng = _stub_engine()
    for X, Xi in ((np.zeros((3, 4)), np.zeros((2, 4))), (np.zeros(4), np.zeros(5)), (np.zeros(5), np.zeros(5)),
                  (np.zeros((3, 4)), np.zeros(4))):
        with pytest.raises(ValueError, match="predict_curvatures"):
            gp.curvature_pred(X, Xi)
    with pytest.raises(ValueError, match="predict_curvatures"):
        gp.sharpness(np.zeros(5))
    with pytest.raises(ValueError, match="predict_curvatures"):
        gp.mean_hessian(np.zeros(5))
    gp._post = _stub_post(False, 4, "Matern32_kernel")
    gp._post.G = object()
    for call in (lambda: gp.curvature_pred(np.zeros(4), np.ones(4)), lambda: gp.sharpness(np.zeros(4)), lambda: gp.mean_hessian(np.zeros(4))):
        with pytest.raises(ValueError, match="Matern32"):
            call()
