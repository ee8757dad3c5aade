"""GPU: pathwise posterior samples -- ppbo_path_score_multi against tests/pathwise_numpy.py (three D buckets, ragged sizes,
every radial kernel, one ARD case, bitwise repeatable; its two halves against ppbo_rff_score_multi and the posterior
mean), ppbo_path_search_multi path by path against the host value, the screen and L-BFGS-B, the moments of
Hsampler.sample_paths against the closed-form covariance and the GP posterior (and the diagonal weight-space posterior
outside that band), reproducibility, the refusals, and sample_xstars without the keyword against the parent's bits."""
import ctypes as C
import types

import numpy as np
import pytest
import scipy.optimize
import torch

import pathwise_numpy as pw
from conftest import load_golden

pytestmark = pytest.mark.gpu

CAP = 1024                       # PPBO_RFF_MULTI_MAX_S
KERNEL_IDS = {"SE_kernel": 0, "RQ_kernel": 1, "camphor_copper_kernel": 2, "Matern52_kernel": 3, "Matern32_kernel": 4}


@pytest.fixture(scope="module")
def eng():
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _star_design(rng, n_q, D, m=25):
    """n_q stars of m + 1 = 26 rows (a query point and m points along one coordinate): N = 26 n_q, off the 32-row tile."""
    rows = []
    for q in range(n_q):
        x = rng.random(D)
        rows.append(x.copy())
        for a in np.linspace(0.005, 0.995, m):
            y = x.copy()
            y[q % D] = a
            rows.append(y)
    return np.array(rows)


def _problem(rng, D, S, F, n_q, kernel, ard=False, vscale=100.0):
    M = 65536 + 123
    l = rng.uniform(0.25, 0.6, D) if ard else 0.3 * np.sqrt(D / 6.0)
    th = [0.05, l, 0.7]
    X = _star_design(rng, n_q, D)
    Xc, W, b = rng.random((M, D)), rng.standard_normal((F, D)) / l, rng.uniform(0, 2 * np.pi, F)
    Wp, V = rng.standard_normal((S, F)), vscale * rng.standard_normal((S, X.shape[0]))
    return Xc, W, b, th, X, Wp, V


def _score_error(got, Xc, Wp, V, W, b, X, th, kernel, chunk=8192):
    """Per path: max_c |got - want| / max_c (sum_f |w_f phi_f| + sum_i |v_i| k_ci) (the sum of absolute terms: k v
    cancels heavily when |v| is large)."""
    err, scale = np.zeros(got.shape[0]), np.zeros(got.shape[0])
    for c0 in range(0, Xc.shape[0], chunk):
        xs = Xc[c0:c0 + chunk]
        want = pw.paths(xs, Wp, V, W, b, X, th, kernel)
        err = np.maximum(err, np.abs(got[:, c0:c0 + chunk] - want).max(axis=1))
        scale = np.maximum(scale, pw.paths_abs(xs, Wp, V, W, b, X, th, kernel).max(axis=1))
    return err / scale


# ---------------------------------------------------------------- 1. the multi-path scoring kernel
CASES = [(6, 1, 1000, 7, "SE_kernel", False), (20, 17, 4096, 40, "SE_kernel", False), (40, 256, 4096, 40, "SE_kernel", False),
         (6, 17, 1000, 7, "RQ_kernel", False), (20, 17, 1000, 7, "Matern52_kernel", False),
         (6, 256, 1000, 7, "Matern32_kernel", False), (20, 256, 1000, 7, "RQ_kernel", False),
         (40, 17, 1000, 7, "Matern52_kernel", False), (40, 1, 1000, 7, "Matern32_kernel", False),
         (6, 17, 1000, 7, "SE_kernel", True)]


@pytest.mark.parametrize("D,S,F,n_q,kernel,ard", CASES)
def test_path_score_multi_matches_numpy(eng, D, S, F, n_q, kernel, ard):
    """Bound: the 1e-9 test_score_multi_matches_oracle holds the feature half to, on the sum-of-absolute-terms measure."""
    rng = np.random.default_rng(1000 * D + S + len(kernel))
    Xc, W, b, th, X, Wp, V = _problem(rng, D, S, F, n_q, kernel, ard)
    assert X.shape[0] == 26 * n_q and X.shape[0] % 32 != 0
    sc = eng.path_score_multi(Xc, W, b, th, kernel, X, Wp, V)
    assert tuple(sc.shape) == (S, Xc.shape[0])
    rel = _score_error(sc.cpu().numpy(), Xc, Wp, V, W, b, X, th, kernel)
    print(f"path_score_multi D={D} S={S} F={F} N={X.shape[0]} {kernel} ard={ard}: worst error / scale = {rel.max():.3e}")
    assert np.all(rel <= 1e-9), rel.max()
    # one fixed summation order: a second call is bitwise equal
    assert torch.equal(sc, eng.path_score_multi(Xc, W, b, th, kernel, X, Wp, V))


def test_path_score_halves(eng):
    """V = 0: ppbo_rff_score_multi's result (to that test's tolerance); W_prior = 0, v = alpha: predict's mean."""
    from ppbo_amd.engine import SCORE_MEAN
    rng = np.random.default_rng(5)
    g = load_golden("rq")
    X, th, kern, m = g["X"], [float(v) for v in g["theta"]], str(g["kernel"]), int(g["m"])
    N, D = X.shape
    F, S = 1000, 17
    Xc, W, b = rng.random((4096 + 17, D)), rng.standard_normal((F, D)) / th[1], rng.uniform(0, 2 * np.pi, F)
    Wp = rng.standard_normal((S, F))
    got = eng.path_score_multi(Xc, W, b, th, kern, X, Wp, np.zeros((S, N))).cpu().numpy()
    want = eng.rff_score_multi(Xc, W, b, th[2], Wp).cpu().numpy()
    assert np.all(np.abs(got - want).max(axis=1) <= 1e-9 * np.abs(want).max(axis=1)), np.abs(got - want).max()
    r = eng.gp_fit(X, th, kern, m, g["f_init"], gtol=1e-6)
    post = r["post"]
    mu = eng.predict(post, Xc, score=SCORE_MEAN, want_var=False, want_best=False)["mu"].cpu().numpy()
    alpha = post.alpha.reshape(1, N)
    got = eng.path_score_multi(Xc, W, b, th, kern, X, np.zeros((1, F)), alpha).cpu().numpy()[0]
    assert np.abs(got - mu).max() <= 1e-5 * np.abs(mu).max(), np.abs(got - mu).max()       # the mean's parity tolerance


# ---------------------------------------------------------------- 2. the batched search, path by path
@pytest.mark.parametrize("D,S,kernel,ard", [(6, 1, "SE_kernel", False), (6, 33, "Matern52_kernel", False),
                                            (20, 33, "SE_kernel", False), (20, 1, "RQ_kernel", False),
                                            (6, 5, "Matern32_kernel", True)])
def test_path_search_multi_per_sample(eng, D, S, kernel, ard):
    rng = np.random.default_rng(10 * D + S)
    F, K, n_q = 1024, 16, 7
    Xc, W, b, th, X, Wp, V = _problem(rng, D, S, F, n_q, kernel, ard, vscale=3.0)
    cand = Xc[:8192 + 5]
    x, v, found = eng.path_search_multi(cand, W, b, th, kernel, X, Wp, V, K=K, iters=100)
    assert x.shape == (S, K, D) and v.shape == (S, K) and found.shape == (S,)
    sc = eng.path_score_multi(cand, W, b, th, kernel, X, Wp, V).cpu().numpy()
    for k in range(S):
        n = int(found[k])
        assert 1 <= n <= K
        assert np.all(v[k, n:] == -np.inf)
        xk, vk = x[k, :n], v[k, :n]
        assert np.all((xk >= 0) & (xk <= 1))
        host = pw.paths(xk, Wp[k], V[k], W, b, X, th, kernel)[0]
        scale = pw.paths_abs(xk, Wp[k], V[k], W, b, X, th, kernel)[0]
        assert np.all(np.abs(host - vk) <= 1e-12 * scale), np.abs(host - vk).max()
        best = vk.max()
        assert best >= sc[k].max() - 1e-12 * np.abs(sc[k]).max()
        # L-BFGS-B from the returned best point gains less than the margin the RFF search test allows (1e-6)
        i = int(np.argmax(vk))
        r = scipy.optimize.minimize(lambda y: -float(pw.paths(y, Wp[k], V[k], W, b, X, th, kernel)[0, 0]), xk[i],
                                    jac=lambda y: -pw.path_grad(y, Wp[k], V[k], W, b, X, th, kernel), method="L-BFGS-B",
                                    bounds=((0, 1),) * D, options={"maxiter": 200})
        ref = float(pw.paths(np.clip(r.x, 0, 1), Wp[k], V[k], W, b, X, th, kernel)[0, 0])
        assert best >= ref - 1e-6 * abs(ref), (k, best, ref)


# ---------------------------------------------------------------- 3. the sampler: moments, reproducibility
def _case(name):
    g = load_golden(name)
    if "theta" in g:
        th = [float(v) for v in g["theta"]]
    else:
        th = [float(g["theta_sf"][0]), np.asarray(g["theta_l"], dtype=float), float(g["theta_sf"][1])]
    return g, g["X"], th, str(g["kernel"]), int(g["m"])


def _fitted_sampler(eng, name, F, seed):
    """An Hsampler on a stand-in GP model that carries the device fit of the fixture (Sigma_inv, fMAP, posterior_covariance
    as NumPy attributes and the device tensors a GPModel keeps)."""
    from ppbo_amd.random_fourier_sampler import Hsampler
    g, X, th, kern, m = _case(name)
    N, D = X.shape
    r = eng.gp_fit(X, th, kern, m, g["f_init"], gtol=1e-6)
    post = eng.posterior(X, th, kern, r["Sigma_inv"], r["fMAP"], m, want_P=True)
    loc = g["Xc"][np.argsort(g["mu"])[-4:]]
    gp = types.SimpleNamespace(eng=eng, D=D, m=m, X=X, xstar=loc[-1], xstars_local=loc, n_gausshermite_sample_points=None,
                               obs_indices=np.arange(0, N, m + 1), kernel=types.SimpleNamespace(__name__=kern), theta=th,
                               _dSigma_inv=r["Sigma_inv"], Sigma_inv=r["Sigma_inv"].cpu().numpy(),
                               fMAP=r["fMAP"].cpu().numpy(), posterior_covariance=post.P.cpu().numpy(), _post=post)
    hs = Hsampler(gp, F)
    np.random.seed(seed)
    hs.generate_basis()
    hs.update_phi_X()
    return hs, gp


@pytest.mark.parametrize("name", ["smoke", "rq", "matern/m52_small", "ard/se_d4"])
def test_path_moments(eng, name):
    """n = 4096 paths at one seed, 200 test points.  Against the closed form C (exact for the basis): variance ratio
    within 1 +- 5 sqrt(2 / n), mean within 5 sqrt(C_ii / n) -- a 5-sigma band over 200 points x 2 statistics fails a
    correct sampler with probability < 1e-3 at a fixed seed.  Against the GP posterior: the same bands widened by the RFF
    error of this basis, measured with pathwise_numpy alone (max |C_ii / var - 1| at F = 2000: 0.04 .. 0.06 on these
    fixtures).  The diagonal weight-space posterior (sample_omegas) is outside that band on ard/se_d4: measured on the
    CPU, its variance is up to 2.3 x the GP's there (1.5 - 1.6 x on the other three)."""
    F, n = 2000, 4096
    hs, gp = _fitted_sampler(eng, name, F, 70)
    Xq = np.random.default_rng(71).random((200, hs.D))
    paths = hs.sample_paths(n, seed=72)
    assert paths.n == n and tuple(paths.W_prior.shape) == (n, F) and tuple(paths.V.shape) == (n, hs.X.shape[0])
    G = paths.evaluate(Xq)
    assert tuple(G.shape) == (n, 200)
    G = G.cpu().numpy()
    Cv = pw.path_var(Xq, hs.W, hs.b, hs.X, hs.theta, hs.kernel, gp.Sigma_inv, gp.posterior_covariance)
    gv = pw.gp_var(Xq, hs.X, hs.theta, hs.kernel, gp.Sigma_inv, gp.posterior_covariance)
    mean = pw.path_mean(Xq, hs.X, hs.theta, hs.kernel, gp.Sigma_inv, gp.fMAP)
    band = 5.0 * np.sqrt(2.0 / n)
    ratio = G.var(axis=0, ddof=1) / Cv
    zmean = np.abs(G.mean(axis=0) - mean) / np.sqrt(Cv / n)
    rff_err = np.abs(Cv / gv - 1.0).max()
    print(f"{name}: var / C in {ratio.min():.3f} .. {ratio.max():.3f} (band {band:.3f}), max |mean - mu| / se = {zmean.max():.2f}, "
          f"RFF error max |C / var_gp - 1| = {rff_err:.3f}")
    assert np.all(np.abs(ratio - 1.0) <= band), (ratio.min(), ratio.max())
    assert np.all(zmean <= 5.0), zmean.max()
    # the user-facing claim: the GP posterior itself (mu_Sigma_pred's mean and variance), up to the RFF error
    gratio = G.var(axis=0, ddof=1) / gv
    assert np.all(np.abs(gratio - 1.0) <= (1.0 + rff_err) * band + rff_err), (gratio.min(), gratio.max())
    out = eng.predict(gp._post, Xq, want_best=False)
    assert np.abs(out["mu"].cpu().numpy() - mean).max() <= 1e-5 * np.abs(mean).max()
    assert np.abs(out["var"].cpu().numpy() - gv).max() <= 1e-5 * hs.theta[2] ** 2
    if name == "ard/se_d4":
        np.random.seed(73)
        hs.update_omega_MAP()
        hs.update_covariancematrix()
        Om = hs.sample_omegas(n, seed=74)
        Gd = np.concatenate([eng.rff_score_multi(Xq, hs.W, hs.b, hs.theta[2], Om[c0:c0 + CAP]).cpu().numpy()
                             for c0 in range(0, n, CAP)])
        dratio = Gd.var(axis=0, ddof=1) / gv
        print(f"{name}: diagonal weight-space posterior var / var_gp in {dratio.min():.3f} .. {dratio.max():.3f}")
        assert np.abs(dratio - 1.0).max() > (1.0 + rff_err) * band + rff_err, dratio.max()


def test_paths_draw_is_the_host_formula(eng):
    """W_prior and z are the ppbo_randn stream of the seed; V is pathwise_numpy.assemble on them."""
    hs, gp = _fitted_sampler(eng, "rq", 512, 80)
    n, F, N = 33, 512, hs.X.shape[0]
    p = hs.sample_paths(n, seed=81)
    draws = eng.randn(81, n * (F + N)).cpu().numpy()
    w, z = draws[:n * F].reshape(n, F), draws[n * F:].reshape(n, N)
    assert np.array_equal(p.W_prior.cpu().numpy(), w)
    L = np.linalg.cholesky(gp.posterior_covariance)
    Fs, V = pw.assemble(z, w, gp.fMAP, L, hs.phi_X, gp.Sigma_inv)
    scale = (np.abs(Fs) + np.abs(w) @ np.abs(hs.phi_X)) @ np.abs(gp.Sigma_inv)      # sum of absolute terms of V
    assert np.all(np.abs(p.V.cpu().numpy() - V) <= 1e-9 * scale), (np.abs(p.V.cpu().numpy() - V) / scale).max()


def test_paths_reproducible(eng):
    hs, _ = _fitted_sampler(eng, "smoke", 512, 90)
    a, b2, c = hs.sample_paths(19, seed=5), hs.sample_paths(19, seed=5), hs.sample_paths(19, seed=6)
    assert torch.equal(a.W_prior, b2.W_prior) and torch.equal(a.V, b2.V)
    assert not torch.equal(a.W_prior, c.W_prior) and not torch.equal(a.V, c.V)
    Xq = np.random.default_rng(91).random((300, hs.D))
    assert torch.equal(a.evaluate(Xq), b2.evaluate(Xq))
    hs._xstar_candidates()                      # the resident pool is drawn on first use: before the seeded calls
    np.random.seed(92)
    X1, V1 = a.xstars()
    np.random.seed(92)
    X2, V2 = b2.xstars()
    assert np.array_equal(X1, X2) and np.array_equal(V1, V2)
    assert X1.shape == (19, hs.D) and np.all((X1 >= 0) & (X1 <= 1)) and np.all(np.isfinite(V1))
    host = np.array([pw.paths(X1[k], a.W_prior[k].cpu().numpy(), a.V[k].cpu().numpy(), hs.W, hs.b, hs.X, hs.theta,
                              hs.kernel)[0, 0] for k in range(19)])
    scale = np.array([pw.paths_abs(X1[k], a.W_prior[k].cpu().numpy(), a.V[k].cpu().numpy(), hs.W, hs.b, hs.X, hs.theta,
                                   hs.kernel)[0, 0] for k in range(19)])
    assert np.all(np.abs(host - V1) <= 1e-12 * scale)
    # the keyword routes through the same calls; seed=None draws the seed from NumPy's global stream
    np.random.seed(92)
    X3, V3 = hs.sample_xstars(19, seed=5, posterior="pathwise")
    assert np.array_equal(X1, X3) and np.array_equal(V1, V3)
    np.random.seed(93)
    d1 = hs.sample_paths(3)
    np.random.seed(93)
    assert torch.equal(d1.V, hs.sample_paths(3).V)


# ---------------------------------------------------------------- 4. refusals
def test_path_refusals(eng):
    from ppbo_amd.random_fourier_sampler import Hsampler
    rng = np.random.default_rng(40)
    M, D, F, N, S = 256, 6, 64, 52, 3
    th = [0.05, 0.3, 0.5]
    cand, W, b, X = rng.random((M, D)), rng.standard_normal((F, D)), rng.random(F), rng.random((N, D))
    Wp, V = rng.standard_normal((S, F)), rng.standard_normal((S, N))
    args = dict(cand=cand, W=W, b=b, theta=th, kernel="SE_kernel", X=X, Wp=Wp, V=V)
    for kw in (dict(Wp=np.zeros((0, F)), V=np.zeros((0, N))), dict(Wp=np.zeros((CAP + 1, F)), V=np.zeros((CAP + 1, N))),
               dict(K=0), dict(K=1025), dict(V=np.zeros((S, N + 1))), dict(V=np.zeros((S + 1, N))),
               dict(kernel="camphor_copper_kernel")):
        with pytest.raises(ValueError):
            eng.path_search_multi(**dict(args, **kw))
    with pytest.raises(ValueError):
        eng.path_score_multi(cand, W, b, th, "SE_kernel", X, Wp, np.zeros((S, N - 1)))
    # the sampler's refusals: a camphor kernel, a GP model without a fit, an unknown posterior
    g = load_golden("cam_small")
    Xg = g["X"]
    gp = types.SimpleNamespace(eng=eng, D=6, m=int(g["m"]), X=Xg, xstar=Xg[0], xstars_local=Xg[:2],
                               n_gausshermite_sample_points=None, obs_indices=np.arange(0, len(Xg), int(g["m"]) + 1),
                               kernel=types.SimpleNamespace(__name__="camphor_copper_kernel"),
                               theta=[float(v) for v in g["theta"]])
    hs = Hsampler(gp, 64)
    np.random.seed(41)
    hs.generate_basis()
    with pytest.raises(NotImplementedError, match="camphor_copper_kernel"):
        hs.sample_paths(4, seed=1)
    gp2 = types.SimpleNamespace(eng=eng, D=D, m=25, X=X, xstar=X[0], xstars_local=X[:2], n_gausshermite_sample_points=None,
                                obs_indices=np.arange(0, N, 26), kernel=types.SimpleNamespace(__name__="SE_kernel"), theta=th)
    hs2 = Hsampler(gp2, F)
    np.random.seed(42)
    hs2.generate_basis()
    with pytest.raises(RuntimeError, match="no fitted posterior"):
        hs2.sample_paths(4, seed=1)
    with pytest.raises(ValueError, match="posterior"):
        hs2.sample_xstars(4, posterior="other")
    # the C-ABI itself
    dc, dW, db, dX, dWp, dV = (eng.dev(a) for a in (cand, W, b, X, Wp, V))
    xs, vals, fnd = eng.empty(4 * 1025 * 65), eng.empty(4 * 1025), torch.zeros(4, dtype=torch.int32, device=eng.device)
    sc = eng.empty(4 * M)
    p = (lambda t: None if t is None else C.c_void_p(t.data_ptr()))
    th3 = (C.c_double * 3)(*th)

    def search(Sv=S, K=8, Dv=D, kid=0, cand_p=dc, x_p=xs, f_p=fnd, v_p=dV):
        return eng.lib.ppbo_path_search_multi(eng.ctx, kid, th3, p(cand_p), M, Dv, p(dW), F, p(db), p(dWp), p(dX), N, p(v_p),
                                              None, Sv, K, 0.05, 10, 1e-10, p(x_p), p(vals), p(f_p), eng._stream())

    def score(Sv=S, kid=0, Dv=D):
        return eng.lib.ppbo_path_score_multi(eng.ctx, kid, th3, p(dc), M, Dv, p(dW), F, p(db), p(dWp), p(dX), N, p(dV), Sv,
                                             p(sc), eng._stream())

    assert search() == 0 and score() == 0
    for kw in (dict(Sv=0), dict(Sv=CAP + 1), dict(K=0), dict(K=1025), dict(Dv=65), dict(kid=KERNEL_IDS["camphor_copper_kernel"]),
               dict(kid=17), dict(cand_p=None), dict(x_p=None), dict(f_p=None), dict(v_p=None)):
        assert search(**kw) != 0, kw
        assert "invalid argument" in eng._err(), kw
    for kw in (dict(Sv=0), dict(Sv=CAP + 1), dict(Dv=65), dict(kid=KERNEL_IDS["camphor_copper_kernel"]), dict(kid=17)):
        assert score(**kw) != 0, kw
        assert "invalid argument" in eng._err(), kw
    assert search() == 0                                # the context is still usable
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. the default is untouched
# sample_xstars(5, seed=63) on the rq fixture (F = 512; seeds 60 / 61 / 62 for the basis, omega_MAP and the candidates),
# recorded on an MI355X from the commit this feature was built on ("Dispatch kernel ids once, drop 30 dead instances,
# share search code"), before any of it existed
PARENT_X = [['0x1.267458da53e3bp-2', '0x1.ee1d9c635d606p-1', '0x1.b2bf9b6cfd237p-1', '0x1.1129decb56d58p-1'],
            ['0x1.44de508093edep-3', '0x0.0p+0', '0x1.81b8b5023cf79p-4', '0x0.0p+0'],
            ['0x1.0000000000000p+0', '0x1.40a0e354c8226p-2', '0x1.8bc1a6f515d37p-1', '0x1.0bba4cc403fd5p-1'],
            ['0x1.740785338f098p-2', '0x1.e4b4a0d467a4dp-1', '0x1.0000000000000p+0', '0x1.2fb2be5ff1655p-1'],
            ['0x1.d4110b02fb3adp-2', '0x1.087731f540c53p-1', '0x1.601fc54f90c1cp-1', '0x1.ef57c5a3ac323p-2']]
PARENT_V = ['0x1.7451ee49f3a53p+0', '0x1.de0acc1e0bb08p-1', '0x1.a42db11aec70ap+0', '0x1.98c2e955b811ap+0',
            '0x1.d41772b4b67cep+0']


def test_sample_xstars_default_is_bitwise_the_parent(eng):
    from ppbo_amd.random_fourier_sampler import Hsampler
    g, X, th, kern, m = _case("rq")
    N, D = X.shape
    loc = g["Xc"][np.argsort(g["mu"])[-4:]]
    gp = types.SimpleNamespace(eng=eng, D=D, m=m, X=X, xstar=loc[-1], xstars_local=loc, n_gausshermite_sample_points=None,
                               obs_indices=np.arange(0, N, m + 1), kernel=types.SimpleNamespace(__name__=kern), theta=th)
    hs = Hsampler(gp, 512)
    np.random.seed(60)
    hs.generate_basis()
    hs.update_phi_X()
    np.random.seed(61)
    hs.update_omega_MAP()
    hs.update_covariancematrix()
    np.random.seed(62)
    Xs, V = hs.sample_xstars(5, seed=63)
    assert np.array_equal(Xs, np.array([[float.fromhex(v) for v in r] for r in PARENT_X]))
    assert np.array_equal(V, np.array([float.fromhex(v) for v in PARENT_V]))
    # the keyword's default by name: the same call (the resident pool exists now, so both draw the same rotation)
    np.random.seed(64)
    X1, V1 = hs.sample_xstars(5, seed=63)
    np.random.seed(64)
    X2, V2 = hs.sample_xstars(5, seed=63, posterior="weights")
    assert np.array_equal(X1, X2) and np.array_equal(V1, V2)
