"""CPU: the slope surface (ppbo_predict_slopes / Engine.predict_slopes / GPModel.slope_pred / GPModel.sensitivity) --
the NumPy statement itself against central differences of a dense kernel and its posterior, the binding table, and the
refusals that are decided on shapes before anything reaches a device."""
import os
import re
import types

import numpy as np
import pytest

import slopes_numpy as sn
from oracle import ppbo_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIAL = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")

# The central differences.  With step h along xi the mean difference (mu(x + h xi) - mu(x - h xi)) / 2h and the column
# difference d / 2h, d = k(x + h xi, X) - k(x - h xi, X), carry a truncation error O(h^2) and a rounding error O(eps / h)
# of their scale; the prior term (2 sf^2 - 2 k(x + h xi, x - h xi)) / 4h^2 rounds at eps / (h^2 / l^2) and truncates at
# O(h^2) -- except for Matern-3/2, whose kernel is only once differentiable at 0 (k = sf^2 (1 - a^2 / 2 + a^3 / 3 - ...),
# a = 2 sqrt3 h / l for a unit step): there the truncation is 2a / 3, first order in h.  Swept on the CPU (the ten cases
# below, worst error relative to the scale each assertion names; prior / variance without Matern-3/2, then Matern-3/2):
#     h       column    mean      prior, var   Matern-3/2 prior, var
#     1e-3    2.2e-4    1.1e-4    1.7e-4       7.3e-3
#     1e-4    2.2e-6    1.1e-6    1.7e-6       7.4e-4
#     1e-5    2.2e-8    1.1e-8    1.7e-7       7.4e-5
#     1e-6    1.9e-9    2.0e-9    2.1e-5       1.0e-5
#     1e-7    1.1e-8    9.3e-9    1.6e-3       4.5e-4
# H = 1e-5 is the bottom of the prior term's trade-off and two orders from the bottom of the others; FD_TOL = 1e-6 is 6x
# the worst smooth figure there, and a wrong constant (a factor 5/3 or 3, a missing 4 pi^2, l for l + 0.05: 20 %) misses
# it by five orders.  Matern-3/2's prior term and variance are checked at its own first-order bound 2a / 3 (+ FD_TOL),
# at most 9.3e-5 (l = 0.25, the shortest length scale drawn): a wrong constant 3 misses that by four orders.
H = 1e-5
FD_TOL = 1e-6


def _design(rng, n_q, D, m):
    rows = []
    for q in range(n_q):
        x = rng.random(D)
        rows.append(x)
        for a in np.linspace(0.05, 0.95, m):
            y = x.copy()
            y[q % D] = a
            rows.append(y)
    return np.array(rows)


def _case(kernel, ard):
    """(X, theta, m, alpha, A, Xq, Xi) of a small dense model with its posterior (oracle), queries and directions."""
    rng = np.random.default_rng(len(kernel) + 17 * ard)
    cam = kernel in (sn.CAMPHOR, sn.CAMPHOR_ARD)
    D, m, n_q = (6, 3, 5) if cam else (4, 3, 5)
    if kernel == sn.CAMPHOR_ARD:
        l = np.array([0.4, 0.6, 0.5, 1.0, 0.8, 0.7])
    elif cam:
        l = 0.5
    else:
        l = rng.uniform(0.25, 0.6, D) if ard else 0.35
    theta = [0.05, l, 0.7]
    X = _design(rng, n_q, D, m)
    Sinv = orc.pd_inverse(orc.regularize_covariance(sn.cross(X, X, theta, kernel), orc.SHRINKAGE))
    f, _ = orc.fit_fmap_newton(0.3 * rng.standard_normal(X.shape[0]), Sinv, m, theta[0], gtol=1e-10, maxiter=500)
    alpha, A = sn.operator_from_fit(X, theta, kernel, m, f)
    Xq = rng.random((40, D))
    Xi = rng.standard_normal((40, D))
    Xi[:5] *= 1e-3                      # short and long directions: everything is homogeneous in xi
    Xi[5:10] *= 30.0
    return X, theta, m, alpha, A, Xq, Xi


CASES = [(k, False) for k in RADIAL] + [(k, True) for k in RADIAL] + [(sn.CAMPHOR, False), (sn.CAMPHOR_ARD, True)]


@pytest.mark.parametrize("kernel,ard", CASES)
def test_statement_against_central_differences(kernel, ard):
    X, theta, m, alpha, A, Xq, Xi = _case(kernel, ard)
    n = np.linalg.norm(Xi, axis=1)
    U = Xi / n[:, None]                # unit steps: h is a length; slopes along Xi are n times those along U
    mu, var, g = sn.slope_reference(Xq, Xi, X, theta, kernel, alpha, A)
    kp, km = sn.cross(Xq + H * U, X, theta, kernel), sn.cross(Xq - H * U, X, theta, kernel)
    d = (kp - km) / (2.0 * H) * n[:, None]
    # the column itself, entry by entry, against the largest entry of its row
    e_g = np.max(np.abs(g - d) / np.abs(g).max(axis=1, keepdims=True))
    # the mean: the difference of the posterior mean k(x, X) alpha
    mu_fd = (kp @ alpha - km @ alpha) / (2.0 * H) * n
    e_mu = np.max(np.abs(mu - mu_fd) / (np.abs(g) @ np.abs(alpha)))
    # the variance: Var[(f(x + h u) - f(x - h u)) / 2h] n^2 under cov(a, b) = k(a, b) - k(a, X) A k(X, b), i.e.
    # (c(+, +) + c(-, -) - 2 c(+, -)) / 4h^2 with the two prior and the three data terms collected
    sf2 = float(theta[2]) ** 2
    kpm = np.array([sn.cross(Xq[i:i + 1] + H * U[i], Xq[i:i + 1] - H * U[i], theta, kernel)[0, 0] for i in range(len(Xq))])
    prior_fd = (2.0 * sf2 - 2.0 * kpm) / (4.0 * H * H) * n * n
    prior = sn.slope_prior(Xi, theta, kernel)
    e_prior = np.max(np.abs(prior - prior_fd) / prior)
    var_fd = prior_fd - np.einsum("ij,ij->i", d, d @ A)
    e_var = np.max(np.abs(var - var_fd) / prior)
    print(f"slopes statement {kernel} ard={ard}: column {e_g:.2e}, mean {e_mu:.2e}, prior {e_prior:.2e}, var {e_var:.2e}")
    assert e_g <= FD_TOL and e_mu <= FD_TOL
    tol_prior = FD_TOL
    if kernel == "Matern32_kernel":
        tol_prior += 2.0 / 3.0 * 2.0 * np.sqrt(3.0) * H / np.min(np.broadcast_to(theta[1], (X.shape[1],)))
    assert e_prior <= tol_prior and e_var <= tol_prior
    assert np.all(var > 0.0) and np.all(var <= prior * (1.0 + 1e-12))       # data only ever remove variance


def test_prior_constants():
    """-2 kappa'(0): 1 (SE, RQ), 5/3 (Matern-5/2), 3 (Matern-3/2) times sf^2 |xi|^2 / l^2; camphor with the profile l_2."""
    xi = np.array([[0.3, -1.2, 0.5, 0.0, 2.0, -0.7]])
    sf, l = 0.7, 0.4
    base = sf ** 2 * (xi ** 2).sum() / l ** 2
    for kernel, c in zip(RADIAL, (1.0, 1.0, 5.0 / 3.0, 3.0)):
        assert abs(sn.slope_prior(xi, [0.05, l, sf], kernel)[0] - c * base) <= 4e-16 * c * base
    want = sf ** 2 * (4 * np.pi ** 2 * (xi[0, [0, 1, 3, 4, 5]] ** 2).sum() / l ** 2 + xi[0, 2] ** 2 / (l + 0.05) ** 2)
    assert abs(sn.slope_prior(xi, [0.05, l, sf], sn.CAMPHOR)[0] - want) <= 4e-16 * want
    assert sn.slope_prior(np.zeros((1, 6)), [0.05, l, sf], sn.CAMPHOR)[0] == 0.0


def test_slope_probability():
    import scipy.stats
    mu, var = np.meshgrid(np.linspace(-3.0, 3.0, 61), np.concatenate([[-1e-3, 0.0], np.logspace(-12, 1, 27)]))
    p = sn.slope_probability(mu, var)
    pos = var > 0
    assert np.abs(p[pos] - scipy.stats.norm.cdf(mu[pos] / np.sqrt(var[pos]))).max() <= 4 * np.finfo(float).eps
    assert list(sn.slope_probability([-1.0, 0.0, 2.0], [0.0, 0.0, -1.0])) == [0.0, 0.5, 1.0]
    assert np.all(sn.slope_probability(np.zeros(29), var[:, 0]) == 0.5)
    assert np.abs(p + sn.slope_probability(-mu, var) - 1.0).max() <= 2 * np.finfo(float).eps
    assert np.isnan(sn.slope_probability(np.nan, 1.0)) and np.isnan(sn.slope_probability(1.0, np.nan))


def test_camphor_ard_directions_are_the_embeddings_derivative():
    """Engine's host map of a direction (J_e(x) xi) against central differences of the embedding, and the SE kernel on
    embedded rows against the per-coordinate camphor statement."""
    from ppbo_amd.engine import camphor_embed_directions
    from ppbo_amd.random_fourier_sampler import camphor_embed_host, camphor_embed_jacobian
    rng = np.random.default_rng(3)
    ls = np.array([0.4, 0.6, 0.5, 1.0, 0.8, 0.7])
    X, Xi = rng.random((9, 6)), rng.standard_normal((9, 6))
    J = camphor_embed_directions(X, Xi, ls)
    assert J.shape == (9, 11)
    for i in range(9):
        assert np.abs(J[i] - camphor_embed_jacobian(X[i], ls) @ Xi[i]).max() <= 1e-14 * np.abs(J[i]).max()
    fd = (camphor_embed_host(X + 1e-6 * Xi, ls) - camphor_embed_host(X - 1e-6 * Xi, ls)) / 2e-6
    assert np.abs(J - fd).max() <= 1e-8 * np.abs(J).max()
    # SE(l = 1) slopes on (e(x), J xi) are the camphor slopes on (x, xi)
    Xd = rng.random((12, 6))
    th = [0.05, ls, 0.7]
    g6 = sn.slope_column(X, Xi, Xd, th, sn.CAMPHOR_ARD)
    g11 = sn.slope_column(camphor_embed_host(X, ls), J, camphor_embed_host(Xd, ls), [0.05, 1.0, 0.7], "SE_kernel")
    assert np.abs(g6 - g11).max() <= 1e-13 * np.abs(g6).max()
    p6, p11 = sn.slope_prior(Xi, th, sn.CAMPHOR_ARD), sn.slope_prior(J, [0.05, 1.0, 0.7], "SE_kernel")
    assert np.abs(p6 - p11).max() <= 1e-14 * p6.max()
    assert np.array_equal(camphor_embed_directions(X, -Xi, ls), -J)


# ---------------------------------------------------------------- the plumbing
def test_binding_header_and_constants():
    from ppbo_amd import _lib, engine
    assert _lib.ABI_VERSION == 9
    assert "ppbo_predict_slopes" in _lib.SIGNATURES
    assert _lib.SIGNATURES["ppbo_predict_slopes"] == _lib.SIGNATURES["ppbo_predict_pairs"] and len(_lib.SIGNATURES["ppbo_predict_slopes"]) == 13
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "ppbo_predict_slopes" in set(re.findall(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(", code))
    assert re.search(r"PPBO_SLOPE_MEAN\s*=\s*0\s*,\s*PPBO_SLOPE_VARIANCE\s*=\s*1\s*,\s*PPBO_SLOPE_PROB\s*=\s*2", code)
    sig = re.search(r"ppbo_predict_slopes\s*\(([^)]*)\)", code).group(1)
    assert [a.split()[-1].lstrip("*") for a in sig.split(",")] == ["ctx", "model", "d_X", "d_Xi", "M", "score_kind", "d_mu", "d_var",
                                                                  "d_prob", "d_score", "h_best_val", "h_best_idx", "stream"]
    assert (_lib.SLOPE_MEAN, _lib.SLOPE_VARIANCE, _lib.SLOPE_PROB) == (0, 1, 2)
    assert (engine.SLOPE_MEAN, engine.SLOPE_VARIANCE, engine.SLOPE_PROB) == (0, 1, 2)
    assert hasattr(engine.Engine, "predict_slopes")
    from ppbo_amd.gp_model import GPModel
    assert hasattr(GPModel, "slope_pred") and hasattr(GPModel, "sensitivity")


def test_library_exports_the_entry_point():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    assert hasattr(_lib.load(), "ppbo_predict_slopes")


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


def _stub_post(camphor, D):
    from ppbo_amd.engine import Posterior
    return Posterior("SE_kernel", (0.05, 0.3, 1.0), 3, types.SimpleNamespace(shape=(8, 11 if camphor else D)), None, None,
                     None, None, camphor=np.ones(6) if camphor else None)


@pytest.mark.parametrize("camphor", [False, True])
def test_predict_slopes_refuses_shapes_before_the_device(camphor):
    eng = _stub_engine()
    D = 6 if camphor else 4
    post = _stub_post(camphor, D)
    z = np.zeros
    for X, Xi in ((z((5, D)), z((4, D))), (z((5, D)), z((5, D + 1))), (z((5, D + 1)), z((5, D + 1))), (z(D), z(D)),
                  (z((0, D)), z((0, D))), (z((5, D, 1)), z((5, D, 1))), (z((5, D)), z(D))):
        with pytest.raises(ValueError, match="predict_slopes"):
            eng.predict_slopes(post, X, Xi)
    with pytest.raises(ValueError, match="score kind"):
        eng.predict_slopes(post, z((5, D)), z((5, D)), score=3)


def test_slope_pred_refusals():
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = None
    with pytest.raises(RuntimeError) as a:
        gp.slope_pred(np.zeros(3), np.ones(3))
    with pytest.raises(RuntimeError) as b:
        gp.mu_Sigma_pred(np.zeros((2, 3)))
    assert str(a.value) == str(b.value)
    gp.xstar = np.zeros(3)
    with pytest.raises(RuntimeError) as c:
        gp.sensitivity()
    assert str(c.value) == str(b.value)
    # a shape mismatch is a ValueError before anything reaches the device
    gp._post = _stub_post(False, 4)
    gp._post.G = object()
    gp.eng = _stub_engine()
    for X, Xi in ((np.zeros((3, 4)), np.zeros((2, 4))), (np.zeros(4), np.zeros(5)), (np.zeros(5), np.zeros(5)),
                  (np.zeros((3, 4)), np.zeros(4))):
        with pytest.raises(ValueError, match="predict_slopes"):
            gp.slope_pred(X, Xi)
    with pytest.raises(ValueError, match="predict_slopes"):
        gp.sensitivity(np.zeros(5))
