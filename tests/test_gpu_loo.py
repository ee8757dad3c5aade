"""GPU: the answer scores -- ppbo_loo_answers / ppbo_score_answers, Engine.loo_answers / score_answers and GPModel.loo_pred,
inconsistent_answers, answers_score, loo_score -- against the NumPy statement (tests/loo_numpy.py) on the same draws, shape
edges, bitwise repeatability and independence of the stars, the status codes, the Monte-Carlo path against quadrature, the
refusals and the drop-in surface.

The bound is the project's 1e-6: the cavity covariance relative to max|C_q|, the cavity mean relative to max|m_q|, the
agreement, the edge probabilities and the log score absolute."""
import ctypes as C
import functools

import numpy as np
import pytest

import loo_numpy as ln
from conftest import load_golden
from oracle import ppbo_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-6


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def host(t):
    return t.detach().cpu().numpy()


def _compare(out, ref, b, label):
    """Holds a loo_answers result to the statement's; returns the worst figures (cov, mean, agree, edge, lpd)."""
    n_q = len(ref["agree"])
    assert np.array_equal(host(out["info"]), ref["info"]), (label, host(out["info"]), ref["info"])
    cm, cv, cc = host(out["cav_mean"]), host(out["cav_var"]), host(out["cav_cov"])
    w_c = max(np.abs(cc[q] - ref["cav_cov"][q]).max() / np.abs(ref["cav_cov"][q]).max() for q in range(n_q))
    w_v = max(np.abs(cv.reshape(n_q, b)[q] - np.diag(ref["cav_cov"][q])).max() / np.abs(ref["cav_cov"][q]).max()
              for q in range(n_q))
    w_m = np.abs(cm - ref["cav_mean"]).max() / np.abs(ref["cav_mean"]).max()
    w_a = np.abs(host(out["agreement"]) - ref["agree"]).max()
    w_e = np.abs(host(out["edge"]).ravel() - ref["edge"]).max()
    w_l = 0.0 if ref["lpd"] is None else np.abs(host(out["lpd"]) - ref["lpd"]).max()
    print(f"loo_answers {label}: cov {w_c:.2e} var {w_v:.2e} mean {w_m:.2e} agree {w_a:.2e} edge {w_e:.2e} lpd {w_l:.2e}")
    assert max(w_c, w_v, w_a, w_e, w_l) <= TOL, (label, w_c, w_v, w_a, w_e, w_l)
    for q in range(n_q):
        assert np.array_equal(cc[q], cc[q].T)                      # C_q comes out symmetric to the bit
    assert np.array_equal(host(out["edge"])[:, 0], host(out["agreement"]))
    assert w_m <= TOL, (label, "cavity mean relative to max|m_q|", w_m, "max|m_q|", np.abs(ref["cav_mean"]).max())
    return w_c, w_m, w_a, w_e, w_l


# ---------------------------------------------------------------- 1. parity on the goldens, same draws
@pytest.mark.parametrize("name", ["smoke", "rq", "cam_small", "c2"])
def test_loo_answers_against_the_statement(eng, name):
    """P and f from the oracle's fit in NumPy, uploaded: only the new kernels are under test.

    Measured on an MI355X (cov and mean relative, the rest absolute):
        smoke      cov 5.3e-13  mean 7.4e-13  agree 1.4e-14  edge 4.3e-14  lpd 2.7e-12
        rq         cov 7.2e-13  mean 8.7e-13  agree 2.9e-14  edge 5.7e-14  lpd 1.3e-11
        cam_small  cov 4.2e-13  mean 3.9e-07  agree 3.9e-15  edge 2.9e-14  lpd 2.1e-11
        c2         cov 5.7e-12  mean 3.4e-11  agree 7.9e-13  edge 2.6e-12  lpd 1.1e-10
    cam_small is the hard one for the cavity mean: four independent queries, so without its own answer a star falls back to
    the prior mean and m_q = f_I - C_q g_q cancels from max|f| = 7.0e-3 to max|m_q| = 1.9e-8, at blocks P_II of condition
    number up to 1.6e7.  The statement carries out its two inversions in extended precision for that reason
    (loo_numpy.cavity: 2.9e-7 of max|m_q| from 60-digit arithmetic there; with np.linalg.inv in fp64 the STATEMENT was 5.8e-5
    off, the device's route -- no inverse of P_II is formed -- 4.3e-7 when restated in NumPy)."""
    g = load_golden(name)
    X, m, th, f = g["X"], int(g["m"]), [float(v) for v in g["theta"]], g["fMAP"].ravel()
    Sinv = orc.pd_inverse(orc.gram(X, th, str(g["kernel"])))
    P = orc.posterior_covariance(Sinv, f, m, th[0])
    z = np.random.default_rng(5).standard_normal((1000, m + 1))
    jit = 1e-10 * th[2] ** 2
    ref = ln.loo(P, f, m, th[0], z, jit)
    assert np.all(ref["info"] == 0)
    out = eng.loo_answers(P, f, m, th[0], z=z, jitter=jit, want_cov=True)
    _compare(out, ref, m + 1, name)


# ---------------------------------------------------------------- 2. shape edges on synthetic inputs
def _synthetic(rng, n_q, b, sigma=1.0, f_scale=0.05):
    """P = A A' / N + I / 2 and a small f: every cavity is positive definite (held on the statement where it is used)."""
    N = n_q * b
    A = rng.standard_normal((N, N))
    return A @ A.T / N + 0.5 * np.eye(N), f_scale * sigma * rng.standard_normal(N)


# b: one edge, two, a tile of 16 and one past it, the reference's default star, both matrices in LDS (62) and the second in
# global memory (63), the LDS limit (128)
@pytest.mark.parametrize("b", [2, 3, 16, 17, 26, 62, 63, 128])
def test_loo_answers_shape_edges(eng, b):
    rng = np.random.default_rng(100 + b)
    sigma = 1.0
    for n_q in (1, 5):
        P, f = _synthetic(rng, n_q, b, sigma)
        zs = rng.standard_normal((1000, b))
        for S in (1, 15, 16, 17, 1000):
            z = zs[:S]
            ref = ln.loo(P, f, b - 1, sigma, z, 1e-12)
            assert np.all(ref["info"] == 0)
            out = eng.loo_answers(P, f, b - 1, sigma, z=z, jitter=1e-12, want_cov=True)
            _compare(out, ref, b, f"b={b} n_q={n_q} S={S}")


# ---------------------------------------------------------------- 3. bits
@pytest.mark.parametrize("b", [17, 63])
def test_bits_repeat_and_a_star_alone(eng, b):
    rng = np.random.default_rng(31)
    n_q, S, sigma = 5, 600, 1.0
    P, f = _synthetic(rng, n_q, b, sigma)
    z = rng.standard_normal((S, b))
    keys = ("lpd", "agreement", "edge", "cav_mean", "cav_var", "cav_cov", "info")
    a = eng.loo_answers(P, f, b - 1, sigma, z=z, jitter=1e-12, want_cov=True)
    a = {k: host(a[k]).copy() for k in keys}
    r = eng.loo_answers(P, f, b - 1, sigma, z=z, jitter=1e-12, want_cov=True)
    for k in keys:
        assert np.array_equal(a[k], host(r[k])), k
    # star q alone (N = b, its own block of P) gets the bits it gets inside the full call
    for q in (0, 3, n_q - 1):
        I = slice(q * b, (q + 1) * b)
        s = eng.loo_answers(P[I, I].copy(), f[I], b - 1, sigma, z=z, jitter=1e-12, want_cov=True)
        assert np.array_equal(host(s["lpd"])[0], a["lpd"][q]) and np.array_equal(host(s["agreement"])[0], a["agreement"][q])
        assert np.array_equal(host(s["edge"])[0], a["edge"][q]) and np.array_equal(host(s["cav_cov"])[0], a["cav_cov"][q])
        assert np.array_equal(host(s["cav_mean"]), a["cav_mean"][I]) and np.array_equal(host(s["cav_var"]), a["cav_var"][I])
    # without draws: the same closed-form outputs
    c = eng.loo_answers(P, f, b - 1, sigma, S=0, jitter=1e-12, want_cov=True)
    assert c["lpd"] is None
    for k in keys[1:]:
        assert np.array_equal(a[k], host(c[k])), k


# ---------------------------------------------------------------- 4. status
def test_status_codes_touch_one_star_only(eng):
    rng = np.random.default_rng(41)
    n_q, b, S, sigma = 4, 8, 200, 0.01
    P, f = _synthetic(rng, n_q, b, sigma, f_scale=1e-4)
    z = rng.standard_normal((S, b))
    keys = ("lpd", "agreement", "edge", "cav_mean", "cav_var", "cav_cov")
    good = eng.loo_answers(P, f, b - 1, sigma, z=z, want_cov=True)
    assert np.all(host(good["info"]) == 0) and np.all(ln.loo(P, f, b - 1, sigma)["info"] == 0)
    good = {k: host(good[k]).copy() for k in keys}
    P1, f1 = P.copy(), f.copy()
    I1, I2 = slice(b, 2 * b), slice(2 * b, 3 * b)
    P1[b + 3, b + 3] = -1.0                                    # star 1: a negative diagonal entry of P_II
    P1[I2, I2] = 100.0 * np.eye(b)                             # star 2: large P, Delta = -1, small sigma
    f1[I2] = 0.0
    f1[2 * b] = sigma
    ref = ln.loo(P1, f1, b - 1, sigma)
    assert list(ref["info"]) == [0, 1, 2, 0] and ref["min_eig"][2] < 0.0       # the statement: indefinite
    bad = eng.loo_answers(P1, f1, b - 1, sigma, z=z, want_cov=True)
    assert list(host(bad["info"])) == [0, 1, 2, 0]
    for k in keys:
        v, g0 = host(bad[k]).reshape(n_q, -1), good[k].reshape(n_q, -1)
        assert np.isnan(v[1]).all() and np.isnan(v[2]).all(), k
        assert np.array_equal(v[0], g0[0]) and np.array_equal(v[3], g0[3]), k
    # a NaN in f: that star's cavity cannot be formed, the others are untouched
    f2 = f.copy()
    f2[b + 2] = np.nan
    nn = eng.loo_answers(P, f2, b - 1, sigma, z=z, want_cov=True)
    assert host(nn["info"])[1] != 0 and np.isnan(host(nn["lpd"])[1]) and np.isnan(host(nn["edge"])[1]).all()
    assert np.array_equal(host(nn["lpd"])[[0, 2, 3]], good["lpd"][[0, 2, 3]])


# ---------------------------------------------------------------- 5. the Monte-Carlo path against quadrature
def test_log_score_against_gauss_hermite(eng):
    """m = 1: l depends on f_1 - f_0 alone, so lpd is a 1-D integral; 65536 device draws (ppbo_randn) within 5 standard
    errors, estimated from the statement's own sample on those draws."""
    rng = np.random.default_rng(61)
    n_q, b, S, sigma = 6, 2, 65536, 0.5
    P, f = _synthetic(rng, n_q, b, sigma, f_scale=0.1)
    ref = ln.loo(P, f, 1, sigma)
    assert np.all(ref["info"] == 0)
    z = eng.randn(12345, S, b)
    out = eng.loo_answers(P, f, 1, sigma, z=z, jitter=0.0, want_cov=True)
    lpd, zh = host(out["lpd"]), host(z)
    for q in range(n_q):
        I = slice(q * b, (q + 1) * b)
        e = np.exp(ln.ell(ln.draws(ref["cav_mean"][I], ref["cav_cov"][q], zh), sigma))
        se = e.std(ddof=1) / (e.mean() * np.sqrt(S))
        quad = ln.lpd_quadrature_m1(ref["cav_mean"][I], ref["cav_cov"][q], sigma)
        print(f"m = 1 star {q}: lpd {lpd[q]:.6f}, quadrature {quad:.6f}, se {se:.2e}")
        assert abs(lpd[q] - quad) <= 5.0 * se, (q, lpd[q], quad, se)


# ---------------------------------------------------------------- 6. held-out answers under the full posterior
@functools.lru_cache(maxsize=None)
def _model(name):
    from ppbo_amd.engine import get_engine
    eng = get_engine(0)
    g = load_golden(name)
    X, m, th, kern, f = g["X"], int(g["m"]), [float(v) for v in g["theta"]], str(g["kernel"]), g["fMAP"].ravel()
    Sinv = orc.pd_inverse(orc.gram(X, th, kern))
    P = orc.posterior_covariance(Sinv, f, m, th[0])
    A = orc.variance_operator(Sinv, P, faithful=False, lam=orc.lambda_dense(f, m, th[0]))
    post = eng.posterior(X, th, kern, eng.dev(Sinv), f, m)
    return dict(post=post, g=g, X=X, th=th, kern=kern, f=f, Sinv=Sinv, P=P, A=A)


@pytest.mark.parametrize("G", [2, 26, 70, 128])
@pytest.mark.parametrize("name", ["smoke", "rq"])
def test_score_answers_against_the_statement(eng, name, G):
    """The statement fed with the oracle's mu_Sigma_pred of each group (the same shrinkage), the same draws."""
    mod = _model(name)
    D, th = mod["X"].shape[1], mod["th"]
    rng = np.random.default_rng(70 + G)
    S = 300
    z = rng.standard_normal((S, G))
    jit = 1e-9 * th[2] ** 2
    for B in (1, 7):
        groups = rng.random((B, G, D))
        if G == 70:
            groups[0] = mod["g"]["line_grid"]                       # the fixture's own query line
        mc = [orc.mu_sigma_pred(groups[k], mod["X"], th, mod["Sinv"], mod["f"], mod["P"], mod["kern"], faithful=False,
                                A=mod["A"]) for k in range(B)]
        ref = ln.heldout(np.stack([a for a, _ in mc]), np.stack([c for _, c in mc]), th[0], z, jit)
        out = eng.score_answers(mod["post"], groups, z=z, jitter=jit)
        w = [np.abs(host(out[k]) - ref[r]).max() for k, r in (("lpd", "lpd"), ("agreement", "agree"), ("edge", "edge"))]
        print(f"score_answers {name} G={G} B={B}: lpd {w[0]:.2e} agree {w[1]:.2e} edge {w[2]:.2e}")
        assert max(w) <= TOL, (name, G, B, w)
        again = eng.score_answers(mod["post"], groups, z=z, jitter=jit)
        c0 = eng.score_answers(mod["post"], groups, S=0, jitter=jit)
        for k in ("lpd", "agreement", "edge"):
            assert np.array_equal(host(out[k]), host(again[k])), k
        assert c0["lpd"] is None and np.array_equal(host(c0["edge"]), host(out["edge"]))
        if G == 2:
            # the prior block left as it is and no jitter: the agreement is the duel's p
            a = host(eng.score_answers(mod["post"], groups, S=0, shrink=0.0, jitter=0.0)["agreement"])
            p = host(eng.predict_pairs(mod["post"], groups[:, 0], groups[:, 1], want_best=False)["prob"])
            assert np.abs(a - p).max() <= TOL, (a, p)


def test_a_nan_point_poisons_its_group_only(eng):
    mod = _model("smoke")
    rng = np.random.default_rng(81)
    B, G, S = 3, 17, 64
    groups, z = rng.random((B, G, mod["X"].shape[1])), rng.standard_normal((S, G))
    good = eng.score_answers(mod["post"], groups, z=z, jitter=1e-9)
    groups2 = groups.copy()
    groups2[1, 5, 0] = np.nan
    bad = eng.score_answers(mod["post"], groups2, z=z, jitter=1e-9)
    for k in ("lpd", "agreement", "edge"):
        v, g0 = host(bad[k]).reshape(B, -1), host(good[k]).reshape(B, -1)
        assert np.isnan(v[1]).all(), k
        assert np.array_equal(v[[0, 2]], g0[[0, 2]]), k


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_outputs_and_context_alone(eng):
    import torch
    from ppbo_amd.engine import SHRINKAGE, _ptr
    rng = np.random.default_rng(91)
    n_q, b, S, sigma = 3, 5, 40, 1.0
    N = n_q * b
    P, f = _synthetic(rng, n_q, b, sigma)
    z = rng.standard_normal((S, b))
    before = eng.loo_answers(P, f, b - 1, sigma, z=z, want_cov=True)
    dP, df, dz = eng.dev(P), eng.dev(f), eng.dev(z)
    SENT = 7.0
    outs = [torch.full((n,), SENT, dtype=torch.float64, device=eng.device) for n in (n_q, n_q, N, N, N, N * b)]
    info = torch.full((n_q,), 7, dtype=torch.int32, device=eng.device)

    def call(P=dP, ldp=N, f=df, N=N, m=b - 1, sigma=sigma, z=dz, S=S, jit=0.0, outs=outs, info=info):
        rc = eng.lib.ppbo_loo_answers(eng.ctx, _ptr(P), ldp, _ptr(f), N, m, sigma, _ptr(z), S, jit, *[_ptr(o) for o in outs],
                                      _ptr(info), eng._stream())
        return rc, eng._err()

    nan, inf = float("nan"), float("inf")
    for kw in (dict(P=None), dict(f=None), dict(m=0), dict(m=-1), dict(m=128, N=129 * 4), dict(N=N + 1), dict(N=0),
               dict(ldp=N - 1), dict(S=-1), dict(z=None), dict(S=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=nan),
               dict(sigma=inf), dict(jit=-1e-9), dict(jit=nan), dict(jit=inf), dict(outs=[None] * 6, info=None)):
        rc, msg = call(**kw)
        assert rc != 0 and "invalid argument" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in outs) and bool((info == 7).all())
    rc, _ = call()
    assert rc == 0
    assert np.array_equal(host(outs[0]), host(before["lpd"])) and np.array_equal(host(info), host(before["info"]))
    # S = 0 with neither draws nor lpd: the closed-form part alone
    rc, _ = call(z=None, S=0, outs=[None] + outs[1:])
    assert rc == 0 and np.array_equal(host(outs[1]), host(before["agreement"]))
    # the model entry
    mod = _model("smoke")
    post = mod["post"]
    B, G = 2, 9
    dg, dz2 = eng.dev(rng.random((B, G, mod["X"].shape[1]))), eng.dev(rng.standard_normal((S, G)))
    md, bare = eng._model(post, True), eng._model(post, False)
    so = [torch.full((n,), SENT, dtype=torch.float64, device=eng.device) for n in (B, B, B * G)]

    def call_m(model=md, grid=dg, B=B, G=G, z=dz2, S=S, jit=0.0, outs=so):
        rc = eng.lib.ppbo_score_answers(eng.ctx, C.byref(model) if model is not None else None, _ptr(grid), B, G, SHRINKAGE,
                                        _ptr(z), S, jit, *[_ptr(o) for o in outs], eng._stream())
        return rc, eng._err()

    for kw in (dict(model=None), dict(grid=None), dict(B=0), dict(G=1), dict(G=0), dict(G=129), dict(S=-1), dict(z=None),
               dict(S=0), dict(jit=-1.0), dict(jit=nan), dict(jit=inf), dict(outs=[None] * 3), dict(model=bare)):
        rc, msg = call_m(**kw)
        assert rc != 0 and "invalid argument" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in so)
    assert call_m()[0] == 0
    after = eng.loo_answers(P, f, b - 1, sigma, z=z, want_cov=True)
    for k in ("lpd", "agreement", "edge", "cav_mean", "cav_var", "cav_cov", "info"):
        assert np.array_equal(host(before[k]), host(after[k])), k


# ---------------------------------------------------------------- 8. through GPModel
def _gp(D, m, theta, kernel, X, X_obs, bounds=None):
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    st = PPBO_settings(D=D, bounds=bounds or ((0.0, 1.0),) * D, xi_acquisition_function="PCD", theta_initial=theta, m=m,
                       verbose=False, kernel=kernel)
    gp = GPModel(st)
    np.random.seed(0)
    gp.update_feedback_processing_object(X_obs)
    gp.FP.X = X.copy()
    gp.update_data()
    gp.initialization_running = False
    return gp


def test_update_model_then_the_flipped_answer_is_named():
    m, D = 15, 2
    X = ln.flipped_design(12, m, D, 3, flip=5)
    stars = X.reshape(12, m + 1, D)
    X_obs = np.zeros((12, 2 * D + 1))
    for q in range(12):
        d = q % D
        X_obs[q, :D], X_obs[q, D + d], X_obs[q, -1] = stars[q, 0], 1.0, stars[q, 0, d]
    gp = _gp(D, m, [0.05, 0.3, 0.5], "SE_kernel", X, X_obs)
    gp.update_model()
    worst = gp.inconsistent_answers(1, seed=1)
    assert list(worst["query"]) == [5] and worst["X"].shape == (1, m + 1, D)
    assert np.array_equal(worst["X"][0], stars[5])
    r = gp.loo_pred(seed=1)
    assert int(np.argmin(r["lpd"])) == 5 and int(np.argmin(r["agreement"])) == 5
    assert r["lpd"][5] == worst["lpd"][0] and r["edge_prob"].shape == (12, m) and np.all(r["info"] == 0)
    assert gp.loo_score(seed=1) == float(r["lpd"].sum())
    # a fit at the same theta by the evidence's route, state untouched: the same score up to the two fits' stopping rules.
    # Two optimisers that both stop at a small gradient agree to ~3e-5 max|f| in f_MAP (the smoke run's bound), i.e. to
    # ~6e-4 max|f| in Delta = f / sigma at sigma = 0.05; |d lpd / d Delta| <= max phi2 = 0.28 per query, 12 queries, max|f|
    # of order 1: 12 x 0.28 x 6e-4 = 2e-3, held with a factor of 5
    f_before = np.array(gp.fMAP, copy=True)
    s_theta = gp.loo_score(theta=[0.05, 0.3, 0.5], seed=1)
    print(f"loo_score: fitted model {float(r['lpd'].sum()):.6f}, a fit at the same theta {s_theta:.6f}")
    assert abs(s_theta - float(r["lpd"].sum())) <= 1e-2 and np.array_equal(f_before, gp.fMAP)
    h = gp.answers_score(X, seed=2)
    assert h["lpd"].shape == (12,) and h["edge_prob"].shape == (12, m) and h["total"] == float(h["lpd"].sum())


@pytest.mark.parametrize("name, kernel", [("camphor_ard/spread", "camphor_copper_ard_kernel"), ("ard/se_d4", "SE_kernel")])
def test_loo_pred_is_kernel_agnostic(name, kernel):
    g = load_golden(name)
    D, m = int(g["D"]), int(g["m"])
    theta = [float(g["theta_sf"][0]), g["theta_l"].copy(), float(g["theta_sf"][1])]
    gp = _gp(D, m, theta, kernel, g["X"], g["X_obs"])
    gp.set_theta(); gp.update_Sigma(gp.theta); gp.update_Sigma_inv(gp.theta)
    gp.fMAP = g["fMAP"].copy()
    gp._post = gp.eng.posterior(gp._dX, gp.theta, gp.kernel.__name__, gp._dSigma_inv, gp.eng.dev(gp.fMAP), gp.m)
    gp._post_mean = gp._post
    r = gp.loo_pred(n_draws=1024, seed=3)
    n_q = g["X"].shape[0] // (m + 1)
    assert r["lpd"].shape == r["agreement"].shape == (n_q,) and r["edge_prob"].shape == (n_q, m)
    assert np.all(r["info"] == 0) and np.all(np.isfinite(r["lpd"])) and np.all((r["agreement"] > 0) & (r["agreement"] < 1))
    # against the statement on the model's own P and f_MAP, the draws of the seed
    z = host(gp.eng.randn(3, 1024, m + 1))
    ref = ln.loo(gp.posterior_covariance, g["fMAP"].ravel(), m, theta[0], z, 1e-10 * theta[2] ** 2)
    assert np.abs(r["lpd"] - ref["lpd"]).max() <= TOL and np.abs(r["agreement"] - ref["agree"]).max() <= TOL
    assert gp.loo_score(n_draws=1024, seed=3) == float(r["lpd"].sum())
    assert np.array_equal(gp.loo_pred(n_draws=1024, seed=3)["lpd"], r["lpd"])
    np.random.seed(9)
    a = gp.loo_pred(n_draws=256)["lpd"]
    np.random.seed(9)
    assert np.array_equal(gp.loo_pred(n_draws=256)["lpd"], a)          # seed = None: off the global NumPy stream
    h = gp.answers_score(g["X"][:2 * (m + 1)], n_draws=256, seed=4)
    assert h["lpd"].shape == (2,) and np.all(np.isfinite(h["lpd"])) and h["edge_prob"].shape == (2, m)
