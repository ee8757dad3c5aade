"""GPU: camphor-copper with one length scale per coordinate (camphor_copper_ard_kernel) -- Gram and cross-covariance
against the NumPy form (tests/test_camphor_ard_host.py), the reference-run camphor fixtures (cam_small, c5) at the
profile l = (l, l, l + 0.05, l, l, l) at the tolerances of test_gpu_parity.py, the evidence at the profile against the
scalar kernel's, mean_grad and mu_star in the caller's coordinates, the evidence gradient, the length-scale fit, the
incremental mode, the loop and the refusals."""
import numpy as np
import pytest
import scipy.stats

from conftest import load_golden
from test_camphor_ard_host import camphor_ard_numpy, camphor_reference_formula, embed_numpy

pytestmark = pytest.mark.gpu

CAM = "camphor_copper_ard_kernel"
SPREAD = np.array([0.1, 0.1, 0.5, 1.0, 1.0, 1.0])


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def host(t):
    return t.detach().cpu().numpy()


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


def profile(l):
    return float(l) + np.array([0.0, 0.0, 0.05, 0.0, 0.0, 0.0])


def _gp(X, m, theta, incremental=False):
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    st = PPBO_settings(D=6, bounds=((0, 1),) * 6, xi_acquisition_function="EI-EXT-FAST", kernel=CAM, m=m,
                       theta_initial=theta, verbose=False)
    gp = GPModel(st, incremental=incremental)
    gp.X, gp.N = np.asarray(X, dtype=float), X.shape[0]
    gp._dX = gp.eng.dev(gp.X)
    gp.theta = theta
    return gp


def _post(eng, X, theta, m, f):
    S = eng.gram(X, theta, CAM)
    return eng.posterior(X, theta, CAM, eng.pd_inverse(S), f, m), S


# ---------------------------------------------------------------- Gram / cross-covariance
@pytest.mark.parametrize("l", [profile(0.26), SPREAD, np.array([0.05, 0.3, 0.8, 0.5, 0.2, 1.5])])
def test_gram_and_cross_cov_match_numpy(eng, l):
    rng = np.random.default_rng(3)
    X, Y = rng.random((200, 6)), rng.random((77, 6))
    th = [0.05, l, 0.7]
    S = host(eng.gram(X, th, CAM))
    ref = camphor_ard_numpy(X, X, l, 0.7)
    ref = (1 - 1e-6) * ref + 1e-6 * np.trace(ref) / len(X) * np.eye(len(X))
    assert rel(S, ref) <= 1e-12
    K = host(eng.cross_cov(X, Y, th, CAM))
    assert rel(K, camphor_ard_numpy(X, Y, l, 0.7)) <= 1e-12
    from ppbo_amd import kernels
    assert rel(kernels.camphor_copper_ard_kernel(X[:5], Y[:9], th), camphor_ard_numpy(X[:5], Y[:9], l, 0.7)) <= 1e-12


def test_short_length_scales_error_is_bounded(eng):
    """At l_d = 0.01 the squared distance of the embedded rows is formed against |e|^2 ~ sum 1 / l_d^2 = 5e4.  The pairs
    whose kernel value is O(1) are the near-coincident ones: Y = X + offsets of about 1e-3, kernel values 0.05 ... 1."""
    rng = np.random.default_rng(4)
    X = rng.random((128, 6))
    Y = X[:64] + rng.uniform(-1e-3, 1e-3, (64, 6))
    l = np.full(6, 0.01)
    K = host(eng.cross_cov(X, Y, [0.05, l, 1.0], CAM))
    ref = camphor_ard_numpy(X, Y, l, 1.0)
    diag = np.arange(64)
    assert ref[diag, diag].min() > 0.02                   # the near pairs are well inside the kernel's range
    err_rel = np.max(np.abs(K[diag, diag] - ref[diag, diag]) / ref[diag, diag])
    err_abs = np.max(np.abs(K - ref))
    print(f"l = 0.01: near pairs max relative error {err_rel:.3e}, all pairs max absolute error {err_abs:.3e} (sigma_f = 1)")
    assert err_rel <= 1e-9
    assert err_abs <= 1e-9


# ---------------------------------------------------------------- reference fixtures at the profile
@pytest.mark.parametrize("name", ["cam_small", "c5"])
def test_profile_reproduces_the_camphor_fixtures(eng, name):
    from ppbo_amd.engine import SCORE_MEAN
    g = load_golden(name)
    m, th_s = int(g["m"]), [float(v) for v in g["theta"]]
    for th in (th_s, [th_s[0], profile(th_s[1]), th_s[2]]):          # scalar l and the explicit profile
        S = eng.gram(g["X"], th, CAM)
        Sh = host(S)
        c = g["Sigma_corner"].shape[0]
        assert rel(Sh[:c, :c], g["Sigma_corner"]) < 1e-12
        assert rel(Sh.sum(axis=1), g["Sigma_rowsum"]) < 1e-12
        assert rel(Sh[g["Sigma_ii"], g["Sigma_jj"]], g["Sigma_samples"]) < 1e-12
        Sinv = eng.pd_inverse(S)
        fmap, st = eng.fit_fmap(Sinv, g["f_init"], m, th[0], gtol=1e-6)
        post = eng.posterior(g["X"], th, CAM, Sinv, g["fMAP"], m, want_P=True)
        _, gref = eng.T_and_grad(Sinv, g["fMAP"], m, th[0])
        ref_gap = np.abs(host(post.P) @ host(gref)).max()
        assert np.abs(host(fmap) - g["fMAP"]).max() <= 1e-5 * np.abs(g["fMAP"]).max() + 1.5 * ref_gap
        out = eng.predict(post, g["Xc"], score=SCORE_MEAN)
        sf2 = th[2] ** 2
        assert rel(host(out["mu"]), g["mu"]) < 1e-6
        assert np.abs(host(out["var"]) - g["var"]).max() <= 1e-6 * sf2
        mu, cov = eng.predict_cov(post, g["line_grid"])
        assert rel(host(mu), g["line_mu"]) < 1e-6
        assert np.abs(host(cov) - g["line_cov"]).max() <= 1e-6 * sf2
        # line EI: the reference's own grid against the scalar kernel with the same draws, then the formed-on-device line
        rng = np.random.default_rng(11)
        z = rng.standard_normal((4000, g["line_grid"].shape[0]))
        mustar, jit = float(g["line_mustar"]), 1e-9 * sf2
        post_s = eng.posterior(g["X"], th_s, "camphor_copper_kernel", Sinv, g["fMAP"], m)
        ei, vm = eng.line_acq(post, g["line_grid"][None], z, mustar, jitter=jit)
        ei_s, vm_s = eng.line_acq(post_s, g["line_grid"][None], z, mustar, jitter=jit)
        assert abs(host(ei)[0] - host(ei_s)[0]) <= 1e-6 * max(abs(host(ei_s)[0]), 1e-3 * np.sqrt(sf2))
        assert abs(host(ei)[0] - float(g["line_ei_ref4000"])) <= 0.1 * abs(float(g["line_ei_ref4000"])) + 1e-3 * np.sqrt(sf2)
        xi, x = g["line_xi"], g["line_x"]
        alphas = np.linspace(0.005, 0.995, 70)
        ei_xi, _ = eng.line_acq_xi(post, xi[None], x[None], alphas, z[:, :70], mustar, jitter=jit)
        grid = (alphas[:, None] * xi[None, :] + x[None, :])[None]
        ei_g, _ = eng.line_acq(post_s, grid, z[:, :70], mustar, jitter=jit)
        assert abs(host(ei_xi)[0] - host(ei_g)[0]) <= 1e-6 * max(abs(host(ei_g)[0]), 1e-3 * np.sqrt(sf2))


def test_spread_length_scales_against_the_reference_run(eng):
    """tests/golden/camphor_ard/spread.npz (tools/make_golden_camphor_ard.py): the reference's own fit, posterior,
    mu_Sigma_pred and line at l = (0.1, 0.1, 0.5, 1, 1, 1), at the tolerances of test_gpu_ard.py."""
    from oracle import ppbo_oracle as orc
    from ppbo_amd.engine import SCORE_MEAN
    g = load_golden("camphor_ard/spread")
    th = [float(g["theta_sf"][0]), g["theta_l"], float(g["theta_sf"][1])]
    m, sf2 = int(g["m"]), float(g["theta_sf"][1]) ** 2
    assert rel(host(eng.gram(g["X"], th, CAM)), g["Sigma"]) < 1e-12
    r = eng.gp_fit(g["X"], th, CAM, m, g["f_init"], gtol=1e-6)
    assert r["post"] is not None
    assert np.abs(host(r["fMAP"]) - g["fMAP"]).max() <= 3e-5 * np.abs(g["fMAP"]).max()
    post = eng.posterior(g["X"], th, CAM, r["Sigma_inv"], g["fMAP"], m)
    assert rel(host(post.alpha), g["alpha"]) < 1e-6
    out = eng.predict(post, g["Xc"], score=SCORE_MEAN)
    assert rel(host(out["mu"]), g["mu"]) < 1e-6
    assert np.abs(host(out["var"]) - g["var"]).max() <= 1e-6 * sf2
    mu, cov = eng.predict_cov(post, g["line_grid"])
    assert rel(host(mu), g["line_mu"]) < 1e-6
    assert np.abs(host(cov) - g["line_cov"]).max() <= 1e-6 * sf2
    # line EI: the reference's line as (alpha, xi, x), formed and embedded on the device, against the oracle's EI of the
    # fixture's mean and covariance with the same draws
    xi, x = g["line_xi"], g["line_x"]
    d = int(np.argmax(xi))
    alphas = (g["line_grid"][:, d] - x[d]) / xi[d]
    z = np.random.default_rng(11).standard_normal((150, 70))
    jit = 1e-9 * sf2
    mustar = float(g["line_mustar"])
    ei, _ = eng.line_acq_xi(post, xi[None, :], x[None, :], alphas, z, mustar, jitter=jit)
    e0 = orc.line_ei(g["line_mu"], g["line_cov"], z, mustar, jitter=jit)
    assert abs(float(host(ei)[0]) - e0) <= 1e-6 * max(abs(e0), 1e-3 * np.sqrt(sf2))
    ei_g, _ = eng.line_acq(post, g["line_grid"][None], z, mustar, jitter=jit)
    assert abs(float(host(ei_g)[0]) - e0) <= 1e-6 * max(abs(e0), 1e-3 * np.sqrt(sf2))


def test_evidence_at_the_profile_equals_the_scalar_kernels(eng):
    """The scalar kernel's evidence and the new kernel's at its profile differ only in the prior: one lognormal term
    on l against six, five at l and one at l + 0.05."""
    g = load_golden("cam_small")
    m, th = int(g["m"]), [1.0, float(g["theta"][1]), 2.0]
    X = g["X"]
    gp_s = _gp(X, m, th)
    gp_s.kernel = __import__("ppbo_amd.kernels", fromlist=["x"]).camphor_copper_kernel
    gp_a = _gp(X, m, th)
    gp_s.update_Sigma(th)
    gp_a.update_Sigma(th)
    np.random.seed(5)
    v_s = gp_s.evidence(th, None)
    np.random.seed(5)
    v_a = gp_a.evidence(th, None)
    one = lambda x: np.log(scipy.stats.lognorm.pdf(x, s=0.5, scale=np.exp(-1.4)))  # noqa: E731
    l = th[1]
    assert abs((v_a - v_s) - (4 * one(l) + one(l + 0.05))) <= 1e-8 * max(1.0, abs(v_s))


# ---------------------------------------------------------------- mean gradient and mu_star in the caller's coordinates
def _spread_post(eng, N=384, m=3, seed=6):
    rng = np.random.default_rng(seed)
    X = rng.random((N, 6))
    th = [0.3, SPREAD, 1.2]
    r = eng.gp_fit(X, th, CAM, m, rng.standard_normal(N), gtol=1e-6, start_is_whitened=True)
    assert r["post"] is not None
    return r["post"], X


def test_mean_grad_matches_finite_differences(eng):
    post, _ = _spread_post(eng)
    rng = np.random.default_rng(9)
    P = rng.random((24, 6))
    mu, grad = eng.mean_grad(post, P)
    mu0 = host(eng.predict(post, P, want_var=False)["mu"])
    assert rel(host(mu), mu0) <= 1e-12
    h = 1e-6
    fd = np.empty((24, 6))
    for d in range(6):
        Pp, Pm = P.copy(), P.copy()
        Pp[:, d] += h
        Pm[:, d] -= h
        fd[:, d] = (host(eng.predict(post, Pp, want_var=False)["mu"]) - host(eng.predict(post, Pm, want_var=False)["mu"])) / (2 * h)
    assert np.abs(host(grad) - fd).max() <= 1e-6 * np.abs(fd).max()


def test_mu_star_beats_a_dense_sample_and_is_stationary(eng):
    post, X = _spread_post(eng)
    rng = np.random.default_rng(10)
    pool = eng.dev(rng.random((65536, 6)))
    shifts = rng.random((3, 6))
    for fp32 in (True, False):
        xs, mus = eng.mean_search_multi(post, pool, shifts, "design", X[0], K=16, iters=200, tol=1e-10, screen_fp32=fp32)
        xs, mus = host(xs).reshape(-1, 6), host(mus).reshape(-1)
        ok = np.isfinite(mus)
        b = int(np.argmax(np.where(ok, mus, -np.inf)))
        xb, vb = xs[b], mus[b]
        assert np.all((xb >= 0) & (xb <= 1))
        assert abs(vb - host(eng.predict(post, xb[None], want_var=False)["mu"])[0]) <= 1e-12 * max(1.0, abs(vb))
        dense = host(eng.predict(post, rng.random((200000, 6)), want_var=False)["mu"]).max()
        assert vb >= dense - 1e-12 * abs(dense)
        xa, ma, _ = eng.mean_ascent(post, xb[None], iters=400, tol=1e-12)
        _, g = eng.mean_grad(post, host(xa))
        g, x = host(g)[0], host(xa)[0]
        pg = np.where(((x <= 0) & (g < 0)) | ((x >= 1) & (g > 0)), 0.0, g)
        assert np.abs(pg).max() <= 1e-5 * max(abs(host(ma)[0]), 1.0)
        assert host(ma)[0] >= vb - 1e-12 * abs(vb)


def test_refusals(eng):
    from ppbo_amd import dist
    post, X = _spread_post(eng, N=64)
    with pytest.raises(ValueError):
        eng.mean_search(post, X)
    with pytest.raises(ValueError):
        dist.ShardedSearch(eng, post, X, 0, 0)
    with pytest.raises(ValueError):
        eng.search_sharded(post, X)
    with pytest.raises(ValueError):
        eng.gram(np.random.rand(8, 5), [0.1, 0.3, 1.0], CAM)
    md = eng._model(post, False)
    import ctypes as C
    bad = np.array([0.1, 0.1, -0.5, 1.0, 1.0, 1.0])
    rc = eng.lib.ppbo_camphor_embed(eng.ctx, C.c_void_p(post.Xc.data_ptr()), 4, eng._dptr(bad),
                                    C.c_void_p(post.X.data_ptr()), eng._stream())
    assert rc < 0 and "invalid argument" in eng._err()
    # in place (6 columns in, 11 out over the same memory) is refused
    buf = eng.empty(4, 11)
    rc = eng.lib.ppbo_camphor_embed(eng.ctx, C.c_void_p(buf.data_ptr()), 4, eng._dptr(SPREAD), C.c_void_p(buf.data_ptr()),
                                    eng._stream())
    assert rc < 0 and "overlap" in eng._err()
    md.D = 6
    assert md.coords.kind == 2 and md.coords.d_Xc == post.Xc.data_ptr()      # the camphor map, on a model that is not D = 11
    rc = eng.lib.ppbo_mean_grad(eng.ctx, C.byref(md), C.c_void_p(post.Xc.data_ptr()), 1,
                                C.c_void_p(post.alpha.data_ptr()), C.c_void_p(post.X.data_ptr()), eng._stream())
    assert rc < 0 and "invalid argument" in eng._err()


# ---------------------------------------------------------------- evidence gradient and the fit
def _design(n_q, m, seed):
    return np.random.default_rng(seed).random((n_q * (m + 1), 6))


def test_evidence_grad_matches_central_differences_and_repeats(eng):
    X = _design(16, 3, 12)
    th = [1.0, np.array([0.3, 0.6, 0.9, 1.2, 0.5, 1.0]), 2.0]
    gp = _gp(X, 3, th)
    gp.update_Sigma(th)
    f0 = gp._draw_prior()
    v, g, _, _, fm = gp.evidence_grad(th, f_initial=f0, gtol=1e-10)
    v2, g2, _, _, _ = gp.evidence_grad(th, f_initial=f0, gtol=1e-10)
    assert v == v2 and np.array_equal(g, g2)
    assert g.shape == (7,)
    p = np.append(th[1], th[2])
    fd = np.empty(7)
    for k in range(7):
        h = 1e-5 * p[k]
        vals = []
        for s in (1.0, -1.0):
            q = p.copy()
            q[k] += s * h
            vals.append(gp.evidence_grad([1.0, q[:6], q[6]], f_initial=fm, gtol=1e-10)[0])
        fd[k] = (vals[0] - vals[1]) / (2 * h)
    assert np.max(np.abs(g - fd) / np.maximum(np.abs(fd), 1e-3 * np.abs(fd).max())) <= 1e-4
    # a scalar l: the gradient of the six expanded length scales
    _, gs, _, _, _ = gp.evidence_grad([1.0, 0.4, 2.0], f_initial=f0, gtol=1e-10)
    _, gv, _, _, _ = gp.evidence_grad([1.0, profile(0.4), 2.0], f_initial=f0, gtol=1e-10)
    assert gs.shape == (7,) and np.allclose(gs, gv, rtol=1e-12, atol=1e-12 * np.abs(gv).max())


def _relevance_model(seed, n_q=40, m=5):
    """Preference data from u(z) = -sin^2(pi (z0 - 0.3 - 0.3 z1)) - 0.5 sin^2(pi (z1 - 0.6)): a utility of the two
    translations only.  Queries run along e_0 and e_1 with every other coordinate uniform, and the answer is the line's
    maximiser, so the answers depend on x and y and carry no information about z or the angles."""
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    rng = np.random.default_rng(seed)
    grid = np.linspace(0.0, 1.0, 2001)
    rows = []
    for q in range(n_q):
        d = q % 2
        xi = np.zeros(6)
        xi[d] = 1.0
        x = rng.random(6)
        x[d] = 0.0
        Z = x[None, :] + grid[:, None] * xi[None, :]
        u = -np.sin(np.pi * (Z[:, 0] - 0.3 - 0.3 * Z[:, 1])) ** 2 - 0.5 * np.sin(np.pi * (Z[:, 1] - 0.6)) ** 2
        a = grid[int(np.argmax(u))]
        rows.append(np.concatenate([a * xi + x, xi, [a]]))
    st = PPBO_settings(D=6, bounds=((0, 1),) * 6, xi_acquisition_function="EI-EXT-FAST", m=m, kernel=CAM,
                       theta_initial=[1.0, 0.5, 1.0], verbose=False, skip_computations_during_initialization=False)
    gp = GPModel(st)
    np.random.seed(seed)
    gp.update_feedback_processing_object(np.array(rows))
    gp.update_data()
    gp.turn_initialization_off()
    gp.update_model()
    return gp


def test_optimize_theta_ard_ranks_translations_against_angles(eng):
    from ppbo_amd.gp_model import THETA_BOX
    gp = _relevance_model(61)
    np.random.seed(62)
    gp.optimize_theta_ard(maxfun=60, start=[1.0, 0.5, 1.0])
    log = gp.theta_search_log
    assert 1 <= len(log) <= 60
    assert log[0][0].shape == (6,) and np.allclose(log[0][0], profile(0.5))     # the scalar start is the profile
    v_start, v_best = log[0][2], max(v for _, _, v in log)
    assert v_best >= v_start
    l = np.asarray(gp.theta[1])
    print("fitted l:", l, "evidence", v_start, "->", v_best)
    assert l.shape == (6,)
    (llo, lhi), _ = THETA_BOX
    assert np.all(l >= llo * (1 - 1e-12)) and np.all(l <= lhi * (1 + 1e-12))
    # the translations carry the utility, the angles (and z) do not
    assert np.min(l[3:]) > np.max(l[:2]), l
    assert l[2] > np.max(l[:2]), l


def test_run_ppbo_loop_and_incremental_mode(eng):
    from ppbo_amd.numerical_main import line_search_user, run_ppbo_loop
    from ppbo_amd.ppbo_settings import PPBO_settings
    lo, hi = np.zeros(6), np.ones(6)

    def objective(P):
        P = np.atleast_2d(P)
        return (np.sin(np.pi * (P - 0.3)) ** 2 * np.array([4.0, 4.0, 1.0, 0.1, 0.1, 0.1])).sum(axis=1)

    out = []
    for incremental in (False, True):
        st = PPBO_settings(D=6, bounds=list(zip(lo, hi)), xi_acquisition_function="EI-EXT-FAST", kernel=CAM,
                           theta_initial=[1.0, 0.3, 1.0], m=5, verbose=False, EI_EXR_mc_samples=50, EI_EXR_BO_maxiter=5,
                           theta_optimizer="ard-gradient")
        np.random.seed(71)
        xi0 = np.eye(6)[:3]
        x0 = np.random.uniform(0, 1, (3, 6))
        res, xs, mus, gp = run_ppbo_loop(line_search_user(objective, lo, hi), xi0, x0, 2, st,
                                         optimize_hyperparameters_after_initialization=not incremental,
                                         incremental=incremental)
        assert res.shape == (5, 13) and np.all(np.isfinite(xs[3:]))
        out.append(gp)
    gp = out[1]
    assert gp.n_appends > 0                     # Sigma^-1 was bordered, not refactorised, for an appended query
    # the incremental model's state against a cold fit of the same design and theta: Sigma^-1, and f_MAP found from a
    # zero start by the trust region to a tight tolerance
    th = gp.theta
    S = gp.eng.gram(gp.X, th, CAM)
    Sinv = gp.eng.pd_inverse(S)
    assert rel(host(gp._dSigma_inv), host(Sinv)) <= 1e-6
    f_cold, st = gp.eng.fit_fmap(Sinv, np.zeros(gp.N), gp.m, th[0], gtol=1e-9, maxiter=500)
    f_cold = host(f_cold)
    # gp.fMAP stops at |grad T| < 1e-4: its distance to the exact maximiser is its Newton step |P grad T|
    post_c = gp.eng.posterior(gp.X, th, CAM, Sinv, f_cold, gp.m, want_P=True)
    _, g_inc = gp.eng.T_and_grad(Sinv, gp.fMAP, gp.m, th[0])
    gap = np.abs(host(post_c.P) @ host(g_inc)).max()
    assert np.abs(gp.fMAP - f_cold).max() <= 1e-6 * np.abs(f_cold).max() + 2.0 * gap
    # and the mean the incremental model predicts is the cold Sigma^-1's at its f_MAP
    post = gp.eng.posterior(gp.X, th, CAM, Sinv, gp.fMAP, gp.m)
    P = np.random.default_rng(1).random((64, 6))
    assert rel(gp.mu_pred_batch(P), host(gp.eng.predict(post, P, want_var=False)["mu"])) <= 1e-6
