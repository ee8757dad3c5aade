"""GPU: the Matern-5/2 and Matern-3/2 kernels through every device path -- Gram (matrix cores, every D bucket),
cross-covariance, the fit, the three scoring paths (three-launch, one-launch, fp32 K*) and the sharded record, the mean
gradient and mu_star's ascent, the line acquisitions, the evidence, the RFF basis and the loop -- against their NumPy
statement (tests/test_matern_host.py) and the reference-run fixtures of tests/golden/matern/
(tools/make_golden_matern.py).  Tolerances are those of the SE tests of the same quantities (test_gpu_parity.py)."""
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle import ppbo_oracle as orc
from test_matern_host import NU, matern, matern_grad

pytestmark = pytest.mark.gpu

FIXTURES = ["matern/m52_small", "matern/m32_small", "matern/m52_c2"]
KERNELS = list(NU)


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


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def engines():
    e = {k: _engine(k) for k in (0, 1)}
    yield e
    for v in e.values():
        v.close()


def host(t):
    return t.detach().cpu().numpy()


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


# ---------------------------------------------------------------- Gram / cross-covariance
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("D", [1, 2, 3, 5, 6, 9, 16, 20, 33])
def test_gram_closed_form(eng, kernel, D):
    rng = np.random.default_rng(D)
    N = 197 if D != 9 else 64 * 3 + 1
    X = rng.random((N, D))
    X[7] = X[3]                                 # a repeated row: r = 0 off the diagonal
    th = [0.05, 0.31 * np.sqrt(D), 0.7]
    S = host(eng.gram(X, th, kernel))
    want = orc.regularize_covariance(matern(X, X, th, kernel), orc.SHRINKAGE)
    assert rel(S, want) < 1e-12
    assert np.array_equal(S, S.T)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("D", [1, 2, 3, 5, 6, 9, 16, 20, 33])
@pytest.mark.parametrize("n1,n2", [(1, 1), (3, 130), (200, 77)])
def test_cross_cov_closed_form(eng, kernel, D, n1, n2):
    rng = np.random.default_rng(n1 * 1000 + n2 + D)
    X1, X2 = rng.random((n1, D)), rng.random((n2, D))
    X2[0] = X1[0]
    th = [0.05, 0.31, 0.7]
    K = host(eng.cross_cov(X1, X2, th, kernel))
    assert rel(K, matern(X1, X2, th, kernel)) < 1e-12


# ---------------------------------------------------------------- fixtures
def _sinv(eng, g):
    S = eng.gram(g["X"], g["theta"], str(g["kernel"]))
    return S, eng.pd_inverse(S)


def _posterior(eng, g, want_P=False):
    _, Sinv = _sinv(eng, g)
    return eng.posterior(g["X"], g["theta"], str(g["kernel"]), Sinv, g["fMAP"], int(g["m"]), want_P=want_P), Sinv


@pytest.mark.parametrize("name", FIXTURES)
def test_gram_vs_fixture(eng, name):
    g = load_golden(name)
    S = host(eng.gram(g["X"], g["theta"], str(g["kernel"])))
    c = g["Sigma_corner"].shape[0]
    assert rel(S[:c, :c], g["Sigma_corner"]) < 1e-12
    assert rel(S.sum(axis=1), g["Sigma_rowsum"]) < 1e-12
    assert rel(S[g["Sigma_ii"], g["Sigma_jj"]], g["Sigma_samples"]) < 1e-12


@pytest.mark.parametrize("name", FIXTURES)
def test_fit_fmap_vs_fixture(eng, name):
    g = load_golden(name)
    m, sig = int(g["m"]), float(g["theta"][0])
    _, Sinv = _sinv(eng, g)
    fmap, st = eng.fit_fmap(Sinv, g["f_init"], m, sig, gtol=1e-6)
    f = host(fmap)
    _, grad = eng.T_and_grad(Sinv, f, m, sig)
    assert np.linalg.norm(host(grad)) <= max(float(g["gradnorm_fMAP"]), 2e-6)
    post = eng.posterior(g["X"], g["theta"], str(g["kernel"]), Sinv, g["fMAP"], m, want_P=True)
    _, gref = eng.T_and_grad(Sinv, g["fMAP"], m, sig)
    ref_gap = np.abs(host(post.P) @ host(gref)).max()
    assert np.abs(f - g["fMAP"]).max() <= 1e-5 * np.abs(g["fMAP"]).max() + 1.5 * ref_gap
    assert st["T"] >= float(g["T_fMAP"]) - 1e-7 * max(1.0, abs(float(g["T_fMAP"])))


@pytest.mark.parametrize("name", FIXTURES)
def test_gp_fit_one_call(eng, name):
    g = load_golden(name)
    r = eng.gp_fit(g["X"], g["theta"], str(g["kernel"]), int(g["m"]), g["f_init"], gtol=1e-6)
    assert r["stats"]["converged"]
    f = host(r["fMAP"])
    assert np.abs(f - g["fMAP"]).max() <= 3e-5 * np.abs(g["fMAP"]).max()


@pytest.mark.parametrize("name", FIXTURES)
def test_predict_mean_var_vs_fixture(eng, name):
    from ppbo_amd.engine import SCORE_MEAN
    g = load_golden(name)
    post, _ = _posterior(eng, g)
    out = eng.predict(post, g["Xc"], score=SCORE_MEAN, want_score=True)
    mu, var = host(out["mu"]), host(out["var"])
    sf2 = float(g["theta"][2]) ** 2
    assert rel(mu, g["mu"]) < 1e-6
    assert np.abs(var - g["var"]).max() <= 1e-6 * sf2
    assert rel(host(post.alpha), g["alpha"]) < 1e-6
    one = eng.predict(post, g["Xc"][:16], want_var=False)
    assert rel(host(one["mu"]), g["mu_pred16"]) < 1e-6


@pytest.mark.parametrize("name", FIXTURES)
def test_posterior_covariance_vs_fixture(eng, name):
    g = load_golden(name)
    post, _ = _posterior(eng, g, want_P=True)
    P = host(post.P)
    c = g["P_corner"].shape[0]
    scale = np.abs(g["P_diag"]).max()
    assert np.abs(np.diag(P) - g["P_diag"]).max() <= 1e-6 * scale
    assert np.abs(P[:c, :c] - g["P_corner"]).max() <= 1e-6 * scale


@pytest.mark.parametrize("name", FIXTURES)
def test_predict_cov_line_vs_fixture(eng, name):
    g = load_golden(name)
    post, _ = _posterior(eng, g)
    mu, cov = eng.predict_cov(post, g["line_grid"])
    sf2 = float(g["theta"][2]) ** 2
    assert rel(host(mu), g["line_mu"]) < 1e-6
    assert np.abs(host(cov) - g["line_cov"]).max() <= 1e-6 * sf2


@pytest.mark.parametrize("name", FIXTURES)
def test_line_acq_vs_oracle_and_fixture(eng, name):
    g = load_golden(name)
    post, _ = _posterior(eng, g)
    rng = np.random.default_rng(11)
    D = int(g["D"])
    B, G, S = 5, 70, 150
    al = np.linspace(0.005, 0.995, G)
    grids = []
    for b in range(B):
        xi = np.zeros(D); xi[b % D] = 1.0
        x = rng.random(D); x[b % D] = 0.0
        grids.append(orc.line_grid(xi, x, al))
    grids[0] = g["line_grid"]
    grid = np.stack(grids)
    z = rng.standard_normal((S, G))
    sf2 = float(g["theta"][2]) ** 2
    mustar = float(g["line_mustar"])
    jit = 1e-9 * sf2
    ei, vm = eng.line_acq(post, grid, z, mustar, jitter=jit)
    ei, vm = host(ei), host(vm)
    for b in range(B):
        mu_b, cov_b = eng.predict_cov(post, grid[b])
        e0 = orc.line_ei(host(mu_b), host(cov_b), z, mustar, jitter=jit)
        v0 = orc.line_varmax(host(mu_b), host(cov_b), z, jitter=jit)
        assert abs(ei[b] - e0) <= 1e-6 * max(abs(e0), 1e-3 * np.sqrt(sf2))
        assert abs(vm[b] - v0) <= 1e-5 * max(abs(v0), 1e-6 * sf2)
    zz = rng.standard_normal((4000, G))
    e_big, _ = eng.line_acq(post, grid[:1], zz, mustar, jitter=jit)
    smp = orc.line_samples(g["line_mu"], g["line_cov"], zz, jit).max(axis=1)
    se = np.std(np.maximum(smp - mustar, 0)) * np.sqrt(2 / 4000)
    assert abs(float(host(e_big)[0]) - float(g["line_ei_ref4000"])) <= 4 * se + 1e-12


def _gp_model(g, acq="PCD"):
    from test_gpu_dropin import _model
    return _model(g, acq)


@pytest.mark.parametrize("name", ["matern/m52_small", "matern/m32_small"])
def test_evidence_vs_fixture(name):
    g = load_golden(name)
    gp, st = _gp_model(g)
    gp.set_theta(); gp.update_Sigma(gp.theta); gp.update_Sigma_inv(gp.theta)
    for th, f0, v in zip(g["ev_theta"], g["ev_finit"], g["ev_value"]):
        gp._draw_prior = lambda f0=f0: gp.eng.dev(f0)
        mine = gp.evidence(list(th), None)
        assert abs(mine - float(v)) <= 1e-5 * max(1.0, abs(float(v))), (list(th), mine, float(v))


# ---------------------------------------------------------------- scoring paths
@pytest.mark.parametrize("name", FIXTURES)
def test_scoring_paths_agree(engines, name):
    """predict_record's argmax through the three-launch path, the one-launch path (N <= 500, D <= 16), the fp32 K*
    option and the sharded search at world = 1: each equals the argmax of its own score vector, exactly."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    g = load_golden(name)
    rng = np.random.default_rng(4)
    Xc = np.concatenate([g["Xc"], rng.random((3000, int(g["D"])))])
    mustar = float(np.max(g["mu"]))
    sf2 = float(g["theta"][2]) ** 2
    res = {}
    for fused, e in engines.items():
        post, _ = _posterior(e, g)
        for fp32 in (False, True):
            out = e.predict(post, Xc, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True, kstar_fp32=fp32)
            sc = host(out["score"])
            assert out["best_idx"] == int(np.argmax(sc)) and out["best_val"] == sc.max()
            rec = host(e.predict_record(post, Xc, SCORE_POINTWISE_EI, mustar, kstar_fp32=fp32))
            assert rec[0] == sc.max() and int(rec[1]) == int(np.argmax(sc))
            assert e.search_sharded(post, Xc, SCORE_POINTWISE_EI, mustar, 100, kstar_fp32=fp32) == (sc.max(), int(np.argmax(sc)) + 100)
            res[(fused, fp32)] = (host(out["mu"]), host(out["var"]))
    mu0, var0 = res[(0, False)]
    mu1, var1 = res[(1, False)]
    assert rel(mu1, mu0) < 1e-12 and np.abs(var1 - var0).max() <= 1e-12 * sf2
    # the fp32 kernel evaluation: the tolerance the SE fp32 option is held to
    muf, varf = res[(0, True)]
    assert rel(muf, mu0) < 1e-4 and np.abs(varf - var0).max() <= 1e-4 * sf2
    if int(g["N"]) <= 500:
        e = engines[1]
        post, _ = _posterior(e, g)
        e.profile(True); e.profile_reset()
        e.predict(post, Xc, score=SCORE_POINTWISE_EI, mustar=mustar)
        assert e.profile_read("fused_score")[1] == 1, "the one-launch kernel took the Matern model"
        e.profile(False)


# ---------------------------------------------------------------- mean gradient, mu_star
@pytest.mark.parametrize("name", FIXTURES)
def test_mean_grad_vs_numpy(eng, name):
    g = load_golden(name)
    post, _ = _posterior(eng, g)
    Xc = g["Xc"][:96].copy()
    Xc[0] = g["X"][0]                                   # r = 0 to a design row
    mu, grad = eng.mean_grad(post, Xc)
    a = host(post.alpha)
    kern = str(g["kernel"])
    mu0 = matern(Xc, g["X"], g["theta"], kern) @ a
    grad0 = np.stack([a @ matern_grad(x, g["X"], g["theta"], kern) for x in Xc])
    assert rel(host(mu), mu0) < 1e-9
    assert rel(host(mu)[1:], g["mu"][1:96]) < 1e-5
    assert np.abs(host(grad) - grad0).max() <= 1e-9 * max(np.abs(grad0).max(), 1e-300)


@pytest.mark.parametrize("name", FIXTURES)
def test_mu_star_at_least_the_reference_de(name):
    g = load_golden(name)
    gp, st = _gp_model(g)
    gp.set_theta(); gp.update_Sigma(gp.theta); gp.update_Sigma_inv(gp.theta)
    gp.fMAP = g["fMAP"].copy()
    gp._refresh_mean_state(gp.eng.dev(g["fMAP"]))
    xstar, mustar, _ = gp.mu_star()
    de = float(g["de_mustar"])
    # the same f_MAP as the reference's DE run: the device ascent must find a mean at least as high
    assert float(mustar) >= de - 1e-9 * max(1.0, abs(de)), (float(mustar), de)


# ---------------------------------------------------------------- RFF
def test_rff_project_gram_approaches_matern52(eng):
    from ppbo_amd.random_fourier_sampler import matern_spectral_draw
    rng = np.random.default_rng(7)
    F, D = 2 ** 16, 3
    th = [0.05, 0.35, 0.8]
    W = matern_spectral_draw(F, D, th[1], NU["Matern52_kernel"], rng=rng)
    b = rng.uniform(0, 2 * np.pi, F)
    X = rng.random((40, D))
    Phi = host(eng.rff_project(X, W, b, th[2]))
    assert Phi.shape == (F, 40)
    err = np.abs(Phi.T @ Phi - matern(X, X, th, "Matern52_kernel")).max()
    assert err <= 5 * th[2] ** 2 * np.sqrt(2 / F), err


def test_hsampler_draws_a_matern_basis():
    from ppbo_amd.random_fourier_sampler import Hsampler
    g = load_golden("matern/m52_small")
    gp, _ = _gp_model(g)
    gp.set_theta()
    hs = Hsampler.__new__(Hsampler)
    hs.kernel, hs.nFeatures, hs.D, hs.theta = "Matern52_kernel", 4096, int(g["D"]), gp.theta
    np.random.seed(1)
    hs.generate_basis()
    assert hs.W.shape == (4096, int(g["D"])) and np.all(np.isfinite(hs.W))


# ---------------------------------------------------------------- loops
def _six_hump(v):
    x, y = v[..., 0], v[..., 1]
    return (4 - 2.1 * x ** 2 + x ** 4 / 3) * x ** 2 + x * y + (-4 + 4 * y ** 2) * y ** 2


# Bound on the final distance to the nearest optimum.  The SE loop of the same shape reaches 0.019 (seed 0) and the
# reference 0.065; test_gpu_dropin holds SE to 0.15.  The Matern posterior mean is rougher between the queries, so its
# x* could sit farther from the optimum; the bound is the reference run's own 0.065.  Measured on seeds 0 / 1 / 2: 0.014 /
# 0.006 / 0.002 (profiles/r07_matern.txt).
SIX_HUMP_BOUND = 0.065


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_six_hump_camel_loop_matern52(seed, capsys):
    from ppbo_amd.misc import hypercube_corners
    from ppbo_amd.numerical_main import line_search_user, run_ppbo_loop
    from ppbo_amd.ppbo_settings import PPBO_settings
    np.random.seed(seed)
    bounds = ((-3, 3), (-2, 2))
    lo, hi = np.array([-3.0, -2.0]), np.array([3.0, 2.0])
    st = PPBO_settings(D=2, bounds=bounds, xi_acquisition_function="PCD", m=25, theta_initial=[0.01, 0.26, 0.1],
                       verbose=False, kernel="Matern52_kernel")
    xis = np.tile(np.diag(hi), (2, 1))
    xs = hypercube_corners(bounds)[:4].astype(float)
    results, xstars, mustars, gp = run_ppbo_loop(line_search_user(_six_hump, lo, hi), xis, xs, 21, st)
    assert all(f["converged"] for f in gp.fit_log), gp.fit_log
    assert "---!!!---" not in capsys.readouterr().out
    opt = np.array([[0.0898, -0.7126], [-0.0898, 0.7126]])
    dist = np.min(np.linalg.norm(opt - xstars[-1][None, :], axis=1))
    print(f"six-hump Matern-5/2 seed {seed}: final distance {dist:.4f}")
    assert dist <= SIX_HUMP_BOUND, f"final x* {xstars[-1]} is {dist:.3f} from the optimum"


# Hartmann6 (f* = -3.322) with EI-EXT-FAST: the SE drop-in test asks min f <= -3.0 after 16 PCD queries; the same bar.
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_hartmann6_loop_matern52(seed, capsys, monkeypatch):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import ppbo_hartmann6
    from ppbo_amd import ppbo_settings as ps
    orig = ps.PPBO_settings

    def with_matern(*a, **k):
        k["kernel"] = "Matern52_kernel"
        return orig(*a, **k)

    monkeypatch.setattr(ps, "PPBO_settings", with_matern)
    gp, hist = ppbo_hartmann6.run(queries=16, strategy="EI-EXT-FAST", m=31, seed=seed)
    assert gp.kernel.__name__ == "Matern52_kernel"
    assert all(f["converged"] for f in gp.fit_log)
    assert "---!!!---" not in capsys.readouterr().out
    best = min(h["fx"] for h in hist)
    print(f"hartmann6 Matern-5/2 seed {seed}: best f {best:.4f}")
    assert best <= -3.0, hist


# ---------------------------------------------------------------- unknown ids
def test_every_kernel_entry_rejects_id_5(eng, monkeypatch):
    from ppbo_amd import _lib
    from ppbo_amd.engine import Posterior, SCORE_POINTWISE_EI
    g = load_golden("matern/m52_small")
    post, _ = _posterior(eng, g)
    monkeypatch.setitem(_lib.KERNEL_IDS, "bogus", 5)
    bad = Posterior("bogus", post.theta, post.m, post.X, post.alpha, post.lam_diag, post.lam_off, post.G)
    Xc = g["Xc"][:64]
    calls = [
        lambda: eng.gram(g["X"], g["theta"], "bogus"),
        lambda: eng.cross_cov(g["X"], Xc, g["theta"], "bogus"),
        lambda: eng.gp_fit(g["X"], g["theta"], "bogus", int(g["m"]), g["f_init"]),
        lambda: eng.predict(bad, Xc),
        lambda: eng.predict_record(bad, Xc, SCORE_POINTWISE_EI, 0.0),
        lambda: eng.search_sharded(bad, Xc, SCORE_POINTWISE_EI, 0.0),
        lambda: eng.predict_cov(bad, Xc[:8]),
        lambda: eng.mean_grad(bad, Xc[:8]),
        lambda: eng.mean_ascent(bad, Xc[:8]),
        lambda: eng.mean_search(bad, Xc),
        lambda: eng.line_acq(bad, np.stack([g["line_grid"]]), np.zeros((4, g["line_grid"].shape[0])), 0.0),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="invalid argument"):
            call()
