"""GPU: per-dimension length scales (ARD) through every device path -- Gram and cross-covariance against the NumPy closed
form (tests/test_ard_host.py), the fit / posterior / line EI against the reference-run fixtures of tests/golden/ard/
(tools/make_golden_ard.py), equal entries against a scalar l, the isotropic oracle on scaled inputs, relevance, mu_star's
search in the caller's coordinates, the two scoring paths, the RFF basis and the loop.  Tolerances are those of the SE
tests of the same quantities (test_gpu_parity.py)."""
import os

import numpy as np
import pytest
import scipy.stats

from conftest import load_golden
from oracle import ppbo_oracle as orc
from test_ard_host import ard_closed_form

pytestmark = pytest.mark.gpu

RADIAL = ["SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel"]
FIXTURES = ["ard/se_d4", "ard/m52_d6"]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _engine(fused):
    from ppbo_amd.engine import Engine
    old = os.environ.get("PPBO_FUSED")
    os.environ["PPBO_FUSED"] = str(fused)
    try:
        return Engine(0)
    finally:
        if old is None:
            del os.environ["PPBO_FUSED"]
        else:
            os.environ["PPBO_FUSED"] = old


def host(t):
    return t.detach().cpu().numpy()


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


def theta_of(g):
    return [float(g["theta_sf"][0]), g["theta_l"], float(g["theta_sf"][1])]


def _fit(eng, X, theta, kernel, m, f_init):
    r = eng.gp_fit(X, theta, kernel, m, f_init, gtol=1e-6)
    assert r["post"] is not None
    return r


def _design(D, n_q, m=3, seed=0):
    """A design of the reference's layout (query row, then its m pseudo-observations)."""
    rng = np.random.default_rng(seed)
    return rng.random((n_q * (m + 1), D)), m


# ---------------------------------------------------------------- 1. Gram / cross-covariance
@pytest.mark.parametrize("kernel", RADIAL)
@pytest.mark.parametrize("D", [4, 8, 12, 16, 20, 24, 32, 48, 64])
def test_gram_and_cross_cov_closed_form(eng, kernel, D):
    rng = np.random.default_rng(D)
    X, Xc = rng.random((96, D)), rng.random((40, D))
    l = np.geomspace(0.05, 2.0, D)
    rng.shuffle(l)
    th = [0.1, l, 0.7]
    S = host(eng.gram(X, th, kernel))
    ref = orc.regularize_covariance(ard_closed_form(X, X, th, kernel), orc.SHRINKAGE, False)
    assert rel(S, ref) <= 1e-12
    K = host(eng.cross_cov(X, Xc, th, kernel))
    assert rel(K, ard_closed_form(X, Xc, th, kernel)) <= 1e-12


def test_kernels_module_takes_a_vector(eng):
    from ppbo_amd import kernels
    rng = np.random.default_rng(2)
    X1, X2 = rng.random((7, 3)), rng.random((5, 3))
    th = [0.1, np.array([0.1, 0.5, 2.0]), 1.1]
    for name in RADIAL:
        assert rel(kernels.BY_NAME[name](X1, X2, th), ard_closed_form(X1, X2, th, name)) <= 1e-12
    with pytest.raises(ValueError):
        kernels.camphor_copper_kernel(rng.random((3, 6)), rng.random((2, 6)), [0.1, np.ones(6), 1.0])
    with pytest.raises(ValueError):
        kernels.SE_kernel(X1, X2, [0.1, np.ones(4), 1.0])


# ---------------------------------------------------------------- 2. reference fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_fit_predict_line_vs_fixture(eng, name):
    from ppbo_amd.engine import SCORE_MEAN
    g = load_golden(name)
    th, kern, m = theta_of(g), str(g["kernel"]), int(g["m"])
    sf2 = th[2] ** 2
    assert rel(host(eng.gram(g["X"], th, kern)), g["Sigma"]) < 1e-12
    r = _fit(eng, g["X"], th, kern, m, g["f_init"])
    assert np.abs(host(r["fMAP"]) - g["fMAP"]).max() <= 3e-5 * np.abs(g["fMAP"]).max()
    # the posterior at the reference's f_MAP: mu, sigma^2 at the SE tolerances
    post = eng.posterior(g["X"], th, kern, r["Sigma_inv"], g["fMAP"], m)
    out = eng.predict(post, g["Xc"], score=SCORE_MEAN)
    assert rel(host(out["mu"]), g["mu"]) < 1e-6
    assert np.abs(host(out["var"]) - g["var"]).max() <= 1e-6 * sf2
    mu, cov = eng.predict_cov(post, g["line_grid"])
    assert rel(host(mu), g["line_mu"]) < 1e-6
    assert np.abs(host(cov) - g["line_cov"]).max() <= 1e-6 * sf2
    # line EI on the same draws: the reference's line as (alpha, xi, x), against the oracle's EI of the fixture's mean and
    # covariance with the same z
    xi, x = g["line_xi"], g["line_x"]
    d = int(np.argmax(xi))
    alphas = (g["line_grid"][:, d] - x[d]) / xi[d]
    z = np.random.default_rng(11).standard_normal((150, 70))
    jit = 1e-9 * sf2
    mustar = float(g["line_mustar"])
    ei, _ = eng.line_acq_xi(post, xi[None, :], x[None, :], alphas, z, mustar, jitter=jit)
    e0 = orc.line_ei(g["line_mu"], g["line_cov"], z, mustar, jitter=jit)
    assert abs(float(host(ei)[0]) - e0) <= 1e-6 * max(abs(e0), 1e-3 * np.sqrt(sf2))


# ---------------------------------------------------------------- 3. equal entries against a scalar l
@pytest.mark.parametrize("kernel", RADIAL)
def test_equal_entries_match_scalar(eng, kernel):
    from ppbo_amd.engine import SCORE_MEAN
    D = 6
    X, m = _design(D, 12, seed=1)
    l = 0.35
    ths, thv = [0.05, l, 0.4], [0.05, np.full(D, l), 0.4]
    sf2 = 0.16
    rng = np.random.default_rng(3)
    f0 = rng.standard_normal(X.shape[0]) * 0.1
    rs, rv = _fit(eng, X, ths, kernel, m, f0), _fit(eng, X, thv, kernel, m, f0)
    assert rv["post"].scale is not None and rs["post"].scale is None
    fs, fv = host(rs["fMAP"]), host(rv["fMAP"])
    assert np.abs(fv - fs).max() <= 3e-5 * np.abs(fs).max()
    Xc = rng.random((700, D))
    os_, ov = (eng.predict(r["post"], Xc, score=SCORE_MEAN) for r in (rs, rv))
    assert rel(host(ov["mu"]), host(os_["mu"])) < 1e-6
    assert np.abs(host(ov["var"]) - host(os_["var"])).max() <= 1e-6 * sf2
    xis, xs = rng.random((8, D)), rng.random((8, D))
    alphas, z = np.linspace(0.005, 0.995, 70), rng.standard_normal((200, 70))
    mustar = float(host(os_["mu"]).max())
    es, _ = eng.line_acq_xi(rs["post"], xis, xs, alphas, z, mustar, jitter=1e-9 * sf2)
    ev, _ = eng.line_acq_xi(rv["post"], xis, xs, alphas, z, mustar, jitter=1e-9 * sf2)
    assert np.abs(host(ev) - host(es)).max() <= 1e-6 * max(np.abs(host(es)).max(), 1e-3 * np.sqrt(sf2))


def _model(kernel, theta, D, n_q=12, m=3, seed=0, incremental=False):
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    st = PPBO_settings(D=D, bounds=((0, 1),) * D, xi_acquisition_function="EI-EXT-FAST", kernel=kernel, m=m,
                       theta_initial=theta, verbose=False, skip_computations_during_initialization=False)
    gp = GPModel(st, incremental=incremental)
    rng = np.random.default_rng(seed)
    rows = []
    for q in range(n_q):
        xi = np.zeros(D)
        xi[q % D] = 1.0
        x = rng.random(D)
        x[q % D] = 0.0
        a = rng.random()
        rows.append(np.concatenate([a * xi + x, xi, [a]]))
    gp.update_feedback_processing_object(np.array(rows))
    gp.update_data()
    gp.turn_initialization_off()
    return gp, st


def test_mu_star_and_evidence_equal_entries(eng):
    # sigma comparable to sigma_f: at sigma << sigma_f T has several local maxima, and two fits whose Grams
    # differ in the last bits may settle in different ones; f_MAP is only defined to the stopping rule: two tight fits
    D, l = 5, 0.3
    np.random.seed(3)                         # (the pseudo-observations' grid draws from the global stream)
    gs, _ = _model("SE_kernel", [0.3, l, 0.4], D)
    np.random.seed(3)
    gv, _ = _model("SE_kernel", [0.3, np.full(D, l), 0.4], D)
    assert np.array_equal(gs.X, gv.X)
    gs.fMAP_gtol = gv.fMAP_gtol = 1e-8
    np.random.seed(4)
    gs.update_model()
    np.random.seed(4)
    gv.update_model()
    assert np.abs(gv.fMAP - gs.fMAP).max() <= 3e-5 * np.abs(gs.fMAP).max()
    assert abs(gv.mustar - gs.mustar) <= 1e-6 * abs(gs.mustar)
    np.random.seed(9)
    es = gs.evidence([1.0, l, 0.4], None)
    np.random.seed(9)
    ev = gv.evidence([1.0, np.full(D, l), 0.4], None)
    lpl = np.log(scipy.stats.lognorm.pdf(l, s=0.5, scale=np.exp(-1.4)))
    assert abs((ev - es) - (D - 1) * lpl) <= 1e-6 * max(1.0, abs(es))


# ---------------------------------------------------------------- 4. the isotropic oracle on scaled inputs (C2 shape)
def test_isotropic_oracle_on_scaled_inputs(eng):
    from ppbo_amd.engine import SCORE_MEAN
    g = load_golden("c2")
    X, m = g["X"], int(g["m"])
    D = X.shape[1]
    l = np.array([0.1, 0.26, 0.5, 0.9, 1.6, 2.5])[:D]
    th = [float(g["theta"][0]), l, float(g["theta"][2])]
    r = _fit(eng, X, th, "SE_kernel", m, g["f_init"])
    f = host(r["fMAP"])
    Xc = g["Xc"]
    out = eng.predict(r["post"], Xc, score=SCORE_MEAN)
    s = 1.0 / l
    th1 = [th[0], 1.0, th[2]]
    S0 = orc.gram(X * s, th1, "SE_kernel")
    Sinv0 = orc.pd_inverse(S0)
    P0 = orc.posterior_covariance(Sinv0, f, m, th[0])
    A0 = orc.variance_operator(Sinv0, P0, faithful=False, lam=orc.lambda_dense(f, m, th[0]))
    mu0, var0 = orc.predict_mean_var(Xc * s, X * s, th1, Sinv0 @ f, A0, "SE_kernel")
    assert rel(host(out["mu"]), mu0) < 1e-6
    assert np.abs(host(out["var"]) - var0).max() <= 1e-6 * th[2] ** 2


# ---------------------------------------------------------------- 5. relevance
@pytest.mark.parametrize("kernel", RADIAL)
def test_irrelevant_dimensions_do_not_move_the_posterior(eng, kernel):
    from ppbo_amd.engine import SCORE_MEAN
    D = 8
    X, m = _design(D, 10, seed=5)
    l = np.full(D, 1e3)
    l[2], l[5] = 0.2, 0.4
    th = [0.05, l, 0.5]
    r = _fit(eng, X, th, kernel, m, np.random.default_rng(6).standard_normal(X.shape[0]) * 0.1)
    rng = np.random.default_rng(7)
    Xc = rng.random((300, D))
    # a move of delta along dimension d changes r^2 by about delta^2 / l_d^2: at l_d = 1e3 a change below 1e-6 relative
    # holds for moves of up to ~0.3 in each of the six dimensions; moves of 0.1
    Xm = Xc.copy()
    others = [d for d in range(D) if d not in (2, 5)]
    Xm[:, others] += 0.1 * (2.0 * rng.random((300, len(others))) - 1.0)
    a, b = (eng.predict(r["post"], P, score=SCORE_MEAN) for P in (Xc, Xm))
    assert rel(host(b["mu"]), host(a["mu"])) < 1e-6
    assert rel(host(b["var"]), host(a["var"])) < 1e-6
    # the same move along a relevant dimension does change the posterior
    Xr = Xc.copy()
    Xr[:, 2] += 0.1 * (2.0 * rng.random(300) - 1.0)
    c = eng.predict(r["post"], Xr, score=SCORE_MEAN)
    assert rel(host(c["mu"]), host(a["mu"])) > 1e-2


# ---------------------------------------------------------------- 6. mu_star on an ARD model
@pytest.mark.parametrize("screen_fp32", [True, False])
@pytest.mark.parametrize("kernel", ["SE_kernel", "Matern52_kernel"])
def test_mu_star_in_the_callers_coordinates(eng, kernel, screen_fp32):
    D = 5
    l = np.array([0.08, 0.25, 0.5, 1.0, 3.0])
    gp, _ = _model(kernel, [0.05, l, 0.4], D, n_q=14, seed=11)
    gp.mustar_screen_fp32 = screen_fp32
    np.random.seed(12)
    gp.update_model()
    x, mu = gp.xstar, gp.mustar
    assert np.all(x >= 0.0) and np.all(x <= 1.0)
    alpha = host(gp._post_mean.alpha)
    th = gp.theta

    def mu_np(P):
        return ard_closed_form(np.atleast_2d(P), gp.X, th, kernel) @ alpha

    assert abs(mu_np(x)[0] - mu) <= 1e-9 * max(1.0, abs(mu))
    R = np.random.default_rng(13).random((1 << 16, D))
    best = max(mu_np(R[k:k + 8192]).max() for k in range(0, 1 << 16, 8192))
    assert mu >= best - 1e-9 * abs(best)
    # projected gradient of the closed form vanishes at x*
    h, g = 1e-6, np.zeros(D)
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        g[d] = (mu_np(np.clip(x + e, 0, 1))[0] - mu_np(np.clip(x - e, 0, 1))[0]) / (np.clip(x + e, 0, 1)[d] - np.clip(x - e, 0, 1)[d])
    pg = np.where(((x <= 0.0) & (g < 0.0)) | ((x >= 1.0) & (g > 0.0)), 0.0, g)
    assert np.abs(pg).max() <= 1e-5 * max(abs(mu), 1e-3) / l.min()
    # the device gradient in the caller's coordinates equals the closed form's
    mg, gg = eng.mean_grad(gp._post_mean, np.clip(R[:4], 0, 1))
    for k in range(4):
        for d in range(D):
            e = np.zeros(D)
            e[d] = 1e-6
            fd = (mu_np(R[k] + e)[0] - mu_np(R[k] - e)[0]) / 2e-6
            assert abs(host(gg)[k, d] - fd) <= 1e-5 * max(1.0, np.abs(host(gg)[k]).max())


def test_single_trial_search_refuses_ard(eng):
    D = 4
    X, m = _design(D, 6)
    r = _fit(eng, X, [0.05, np.array([0.1, 0.2, 0.4, 0.8]), 0.4], "SE_kernel", m, np.zeros(X.shape[0]))
    with pytest.raises(ValueError):
        eng.mean_search(r["post"], np.random.default_rng(0).random((100, D)))
    from ppbo_amd.dist import ShardedSearch
    with pytest.raises(ValueError):
        ShardedSearch(eng, r["post"], np.random.default_rng(0).random((100, D)), 0, 0)


# ---------------------------------------------------------------- 7. one-launch and three-launch scorers
@pytest.mark.parametrize("kernel", RADIAL)
def test_one_launch_and_three_launch_agree(kernel):
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    D = 10
    X, m = _design(D, 30, seed=8)                   # N = 120 <= 500
    th = [0.05, np.geomspace(0.1, 2.0, D), 0.4]
    f0 = np.random.default_rng(9).standard_normal(X.shape[0]) * 0.1
    Xc = np.random.default_rng(10).random((5000, D))
    res = {}
    for fused in (0, 1):
        e = _engine(fused)
        try:
            r = _fit(e, X, th, kernel, m, f0)
            e.profile(True)
            out = e.predict(r["post"], Xc, score=SCORE_POINTWISE_EI, mustar=0.0, want_score=True)
            res[fused] = (host(out["mu"]), host(out["var"]), host(out["score"]), out["best_idx"])
            if fused:
                assert e.profile_read("fused_score")[1] == 1, "the one-launch kernel took the ARD model"
        finally:
            e.close()
    sf2 = th[2] ** 2
    assert rel(res[1][0], res[0][0]) < 1e-9
    assert np.abs(res[1][1] - res[0][1]).max() <= 1e-9 * sf2
    assert np.abs(res[1][2] - res[0][2]).max() <= 1e-9 * max(np.abs(res[0][2]).max(), 1e-3)


# ---------------------------------------------------------------- 8. the RFF basis
def test_rff_gram_and_return_xstar(eng):
    from ppbo_amd.random_fourier_sampler import Hsampler
    D = 4
    l = np.array([0.15, 0.3, 0.8, 2.0])
    gp, _ = _model("SE_kernel", [0.05, l, 0.6], D, n_q=10, seed=21)
    np.random.seed(22)
    gp.update_model()
    hs = Hsampler(gp, nFeatures=16384)
    np.random.seed(23)
    hs.generate_basis()
    Phi = host(eng.rff_project(gp.X, hs.W, hs.b.ravel(), gp.theta[2]))
    K = ard_closed_form(gp.X, gp.X, gp.theta, "SE_kernel")
    # Monte-Carlo: each entry of Phi^T Phi is a mean of F terms of variance <= 2 sf^4 / F
    assert np.abs(Phi.T @ Phi - K).max() <= 6 * np.sqrt(2.0 / 16384) * gp.theta[2] ** 2
    hs.update_phi_X()
    hs.update_omega_MAP()
    hs.update_covariancematrix()
    om = hs.sample_omega()
    x = hs.return_xstar(om)
    assert x is not None and np.all(x >= 0) and np.all(x <= 1)
    sc, bv, _ = hs.score_candidates(np.random.default_rng(24).random((20000, D)), om)
    fx = float(hs.phiVec(x).ravel() @ om)
    assert fx >= bv - 1e-9 * abs(bv)


# ---------------------------------------------------------------- 9. the loop
@pytest.mark.parametrize("incremental", [False, True])
def test_run_ppbo_loop_with_ard(eng, incremental):
    from ppbo_amd.numerical_main import line_search_user, run_ppbo_loop
    from ppbo_amd.ppbo_settings import PPBO_settings
    D = 4
    lo, hi = np.zeros(D), np.ones(D)
    w = np.array([4.0, 1.0, 0.1, 0.01])

    def objective(P):
        return ((np.atleast_2d(P) - 0.3) ** 2 * w).sum(axis=1)

    st = PPBO_settings(D=D, bounds=list(zip(lo, hi)), xi_acquisition_function="EI-EXT-FAST",
                       theta_initial=[0.05, np.array([0.2, 0.4, 1.0, 3.0]), 0.4], m=5, verbose=False,
                       EI_EXR_mc_samples=50, EI_EXR_BO_maxiter=5)
    np.random.seed(31)
    xi0 = np.eye(D)[:2]
    x0 = np.random.uniform(0, 1, (2, D))
    res, xs, mus, gp = run_ppbo_loop(line_search_user(objective, lo, hi), xi0, x0, 5, st, incremental=incremental)
    assert res.shape == (7, 2 * D + 1)
    assert np.all(np.isfinite(xs[2:])) and np.all(xs[2:] >= 0) and np.all(xs[2:] <= 1)
    assert gp._post.scale is not None
    if incremental:
        assert gp.n_appends >= 1


def test_optimize_theta_keeps_the_profile(eng):
    D = 3
    p0 = np.array([0.1, 0.3, 0.9])
    gp, _ = _model("SE_kernel", [1.0, p0, 0.4], D, n_q=8, seed=41)
    np.random.seed(42)
    gp.update_model()
    gp.optimize_theta(workers=2)
    l = np.asarray(gp.theta[1])
    assert l.shape == (D,)
    assert np.allclose(l / np.exp(np.mean(np.log(l))), p0 / np.exp(np.mean(np.log(p0))), rtol=1e-12)
    assert len(gp.theta_search_log) == 60
