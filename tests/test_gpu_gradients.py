"""GPU: gradients -- ppbo_predict_gradients / Engine.predict_gradients / GPModel.gradient_pred, xstar_covariance,
loosest_direction, active_subspace against the NumPy statement (tests/gradients_numpy.py: the D coordinate columns of
tests/slopes_numpy.py, the oracle's dense variance operator symmetrised; held to the slope statement in
tests/test_gradients_host.py), against the device's own ppbo_mean_grad and ppbo_predict_slopes, the structure of C, the NaN
rules, the scores and their argmax, and the refusals.

Bound (TOL = 1e-6, the package's parity standard), per entry: |m_d - ref| against sum_j |g_jd alpha_j| (the mean is a sum
that cancels down from it), |C_de - ref| against sqrt(P_dd P_ee) (the covariance is a difference that cancels down from the
prior).  Every test prints the worst values it meets.

Measured on MI355X (the worst entry over all parity cases; profiles/r25_gradients.txt has them case by case): mean 1.5e-9 and
covariance 1.9e-9 (SE, D = 6, N = 546), camphor on cam_small 2.5e-10 / 6.5e-10, the camphor-ARD model 1.8e-15 / 6.4e-16;
m against ppbo_mean_grad 8.2e-16; xi' C xi against predict_slopes' variance 3.7e-15 of the prior, xi' m against its mean
1.9e-14; D = 1 against the slope along 1: mean 0, variance 3.3e-15; smallest eigenvalue of C >= 9.4e-3 of the largest prior
entry; active_subspace against the statement 2.1e-12; the rotated ridge 4.24 degrees on the device's fit."""
import ctypes as C
import functools

import numpy as np
import pytest

import gradients_numpy as gn
import slopes_numpy as sn
from test_gpu_slopes import RADIAL, TOL, _fitted, _fitted_camphor, _fitted_camphor_ard, _forms, _stub_gp, host

pytestmark = pytest.mark.gpu
CHUNK = 512                # points per chunk of ppbo_predict_gradients


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _model(which):
    """'camphor-node', 'camphor-edge', 'camphor_ard', or 'SE-6-8-3-node[-ard]' = _fitted(kernel, D, n_q, m, form, ard)."""
    if which == "camphor_ard":
        return _fitted_camphor_ard()
    p = which.split("-")
    if p[0] == "camphor":
        return _fitted_camphor(p[1])
    return _fitted(p[0] + "_kernel", int(p[1]), int(p[2]), int(p[3]), p[4], ard=len(p) > 5)


def _points(rng, mod, M=37):
    """M uniform points, the first few ON design rows (every g_jd of that row is 0 there)."""
    N, D = mod["X"].shape
    X = rng.random((M, D))
    k = min(5, M)
    X[:k] = mod["X"][rng.integers(0, N, k)]
    return X


@functools.lru_cache(maxsize=None)
def _reference(which, M, seed):
    """(X, m0, C0, mean scale, cov scale) of _points(seed) on the model: computed once, shared, never written to."""
    mod = _model(which)
    X = _points(np.random.default_rng(seed), mod, M)
    m0, C0, g = gn.gradient_reference(X, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"])
    out = (X, m0, C0, gn.mean_scale(g, mod["alpha"]), gn.cov_scale(mod["th"], mod["kernel"], X.shape[1]))
    for a in out[1:]:                    # (X goes to the device through torch, which wants a writable array)
        a.setflags(write=False)
    return out


def _parity(eng, which, M=37, seed=3, **kw):
    mod = _model(which)
    X, m0, C0, ms, cs = _reference(which, M, seed)
    out = eng.predict_gradients(mod["post"], X, **kw)
    m, Cv = host(out["mean"]), host(out["cov"])
    assert m.shape == m0.shape and Cv.shape == C0.shape
    assert np.all(np.isfinite(m)) and np.all(np.isfinite(Cv))
    e_m, e_c = np.max(np.abs(m - m0) / ms), np.max(np.abs(Cv - C0) / cs)
    print(f"gradients parity {which} M={M}: |m - ref| / sum|g alpha| = {e_m:.2e}, |C - ref| / sqrt(P P) = {e_c:.2e}")
    assert e_m <= TOL and e_c <= TOL
    return X, out


# ---------------------------------------------------------------- 1. parity with the NumPy statement
# (D, n_q, m): one and two 16-column tiles (16, 17), N = 78 off every tile edge, stars of 41 > 32 rows (the one-sided,
# non-symmetric line_cov form), the largest bucket, and N = 546 > 512 (at least two row slices)
SE_SHAPES = [(1, 8, 3), (16, 8, 3), (17, 8, 3), (40, 2, 40), (64, 4, 3), (6, 21, 25)]
PARITY = ([f"{k[:-7]}-{D}-{n_q}-{m}-{f}" for k in RADIAL for (D, n_q, m) in ((6, 8, 3), (20, 3, 25)) for f in ("node", "edge")]
          + [f"SE-{D}-{n_q}-{m}-{f}" for (D, n_q, m) in SE_SHAPES for f in ("node", "edge")]
          + [f"Matern52-{D}-{n_q}-{m}-{f}-ard" for (D, n_q, m) in ((6, 3, 25), (20, 3, 25)) for f in ("node", "edge")]
          + ["camphor-node", "camphor-edge", "camphor_ard"])


@pytest.mark.parametrize("which", PARITY)
def test_parity(eng, which):
    X, out = _parity(eng, which)
    Cv = host(out["cov"])
    # structure: symmetric bit for bit; positive semi-definite up to the parity bound
    assert np.array_equal(Cv, Cv.transpose(0, 2, 1))
    mod = _model(which)
    low = np.linalg.eigvalsh(Cv).min() / gn.prior_diagonal(mod["th"], mod["kernel"], X.shape[1]).max()
    print(f"gradients structure {which}: smallest eigenvalue / largest prior entry = {low:.3e}")
    assert low >= -TOL


def test_chunk_boundary(eng):
    """One point more than a chunk at D = 6: the rows on both sides of the boundary are held to the statement, and the
    winner's index is the global row."""
    from ppbo_amd.engine import GRAD_NORM2
    which = "SE-6-8-3-node"
    X, out = _parity(eng, which, M=CHUNK + 1, seed=9, score=GRAD_NORM2, want_score=True)
    m, Cv, sc = host(out["mean"]), host(out["cov"]), host(out["score"])
    want = (m * m).sum(axis=1) + np.trace(Cv, axis1=1, axis2=2)
    assert np.max(np.abs(sc - want) / want) <= 1e-13
    assert out["best_idx"] == int(np.argmax(sc)) and out["best_val"] == sc.max()
    # the winner moved behind the boundary
    i = int(np.argmax(sc))
    Xs = X.copy()
    Xs[[i, CHUNK]] = Xs[[CHUNK, i]]
    moved = _model(which)["post"]
    out2 = eng.predict_gradients(moved, Xs, score=GRAD_NORM2, want_mean=False, want_cov=False, want_score=True)
    assert out2["mean"] is None and out2["cov"] is None
    sc2 = host(out2["score"])
    assert out2["best_idx"] == int(np.argmax(sc2)) and out2["best_val"] == sc2.max()
    assert abs(sc2[CHUNK] - sc[i]) <= 1e-12 * sc[i]


@pytest.mark.parametrize("which", ["RQ-20-3-25-edge", "camphor-node", "camphor_ard"])
def test_repeated_call_gives_equal_bits(eng, which):
    from ppbo_amd.engine import GRAD_TRACE
    mod = _model(which)
    X = _reference(which, 37, 3)[0]
    a = eng.predict_gradients(mod["post"], X, score=GRAD_TRACE, want_score=True)
    b = eng.predict_gradients(mod["post"], X, score=GRAD_TRACE, want_score=True)
    for k in ("mean", "cov", "score"):
        assert np.array_equal(host(a[k]).view(np.int64), host(b[k]).view(np.int64))
    assert (a["best_idx"], a["best_val"]) == (b["best_idx"], b["best_val"])


# ---------------------------------------------------------------- 2. against the device's own other paths
OTHER = ["SE-20-3-25-node", "Matern32-6-8-3-edge", "Matern52-6-3-25-node-ard", "camphor-node", "camphor_ard"]


@pytest.mark.parametrize("which", OTHER)
def test_mean_against_mean_grad(eng, which):
    mod = _model(which)
    X, _, _, ms, _ = _reference(which, 37, 3)
    m = host(eng.predict_gradients(mod["post"], X, want_cov=False)["mean"])
    _, grad = eng.mean_grad(mod["post"], X)
    e = np.max(np.abs(m - host(grad)) / ms)
    print(f"gradients against mean_grad {which}: |m - grad mu| / sum|g alpha| = {e:.2e}")
    assert e <= 2 * TOL


@pytest.mark.parametrize("which", OTHER)
def test_quadratic_form_against_predict_slopes(eng, which):
    """Each side is within TOL of the same reference, and |xi' dC xi| <= TOL D prior for entries within TOL sqrt(P P)."""
    mod = _model(which)
    X = _reference(which, 37, 3)[0]
    D = X.shape[1]
    Xi = np.random.default_rng(21).standard_normal(X.shape) * 10.0 ** np.random.default_rng(22).uniform(-2.0, 1.0, (X.shape[0], 1))
    out = eng.predict_gradients(mod["post"], X)
    m, Cv = host(out["mean"]), host(out["cov"])
    sl = eng.predict_slopes(mod["post"], X, Xi, want_best=False)
    prior = sn.slope_prior(Xi, mod["th"], mod["kernel"])
    e_v = np.max(np.abs(np.einsum("id,ide,ie->i", Xi, Cv, Xi) - host(sl["var"])) / prior)
    g = sn.slope_column(X, Xi, mod["X"], mod["th"], mod["kernel"])
    e_m = np.max(np.abs(np.einsum("id,id->i", m, Xi) - host(sl["mu"])) / (np.abs(g) @ np.abs(mod["alpha"])))
    print(f"gradients against predict_slopes {which}: |xi'C xi - var_s| / prior = {e_v:.2e}, |xi'm - mu_s| / sum|g alpha| = {e_m:.2e}")
    assert e_v <= (D + 1) * TOL and e_m <= 2 * TOL


@pytest.mark.parametrize("form", ["node", "edge"])
def test_one_dimension_is_the_slope_along_one(eng, form):
    which = f"SE-1-8-3-{form}"
    mod = _model(which)
    X, _, _, ms, cs = _reference(which, 37, 3)
    out = eng.predict_gradients(mod["post"], X)
    sl = eng.predict_slopes(mod["post"], X, np.ones_like(X), want_best=False)
    e_m = np.max(np.abs(host(out["mean"])[:, 0] - host(sl["mu"])) / ms[:, 0])
    e_c = np.max(np.abs(host(out["cov"])[:, 0, 0] - host(sl["var"])) / cs[0, 0])
    print(f"gradients D = 1 {form}: mean {e_m:.2e}, variance {e_c:.2e}")
    assert e_m <= 2 * TOL and e_c <= 2 * TOL


# ---------------------------------------------------------------- 3. NaN rules, scores, the argmax
@pytest.mark.parametrize("which", ["Matern52-6-8-3-node", "Matern52-6-3-25-edge-ard", "camphor-edge", "camphor_ard"])
def test_nan_rows_scores_and_argmax(eng, which):
    from ppbo_amd.engine import GRAD_NONE, GRAD_NORM2, GRAD_TRACE
    mod = _model(which)
    post = mod["post"]
    X = _points(np.random.default_rng(10), mod, 101)
    X[60] = X[20]                                   # duplicate rows: a tie goes to the first
    clean = eng.predict_gradients(post, X, score=GRAD_TRACE, want_score=True)
    Xb = X.copy()
    Xb[3, 2 % X.shape[1]], Xb[99, 0], Xb[64, -1] = np.nan, np.inf, -np.inf
    bad = np.zeros(101, dtype=bool)
    bad[[3, 99, 64]] = True
    for kind in (GRAD_TRACE, GRAD_NORM2):
        out = eng.predict_gradients(post, Xb, score=kind, want_score=True)
        m, Cv, sc = host(out["mean"]), host(out["cov"]), host(out["score"])
        assert np.all(np.isnan(m[bad])) and np.all(np.isnan(Cv[bad])) and np.all(np.isnan(sc[bad]))
        assert np.array_equal(m[~bad], host(clean["mean"])[~bad]) and np.array_equal(Cv[~bad], host(clean["cov"])[~bad])
        want = np.trace(Cv, axis1=1, axis2=2) + ((m * m).sum(axis=1) if kind == GRAD_NORM2 else 0.0)
        assert np.max(np.abs(sc[~bad] - want[~bad]) / np.abs(want[~bad])) <= 1e-12
        assert out["best_idx"] == int(np.nanargmax(sc)) and out["best_val"] == np.nanmax(sc) and not bad[out["best_idx"]]
        assert sc[60] == sc[20]
    assert np.array_equal(host(clean["score"])[~bad], host(eng.predict_gradients(post, Xb, score=GRAD_TRACE, want_score=True)["score"])[~bad])
    tie = eng.predict_gradients(post, X[[5, 20, 7, 60]][[1, 3]], score=GRAD_TRACE)
    assert tie["best_idx"] == 0
    none = eng.predict_gradients(post, Xb[[3, 99, 64]], score=GRAD_NORM2, want_score=True)
    assert none["best_idx"] == -1 and np.isnan(none["best_val"]) and np.all(np.isnan(host(none["score"])))
    unscored = eng.predict_gradients(post, X[:4], score=GRAD_NONE)
    assert unscored["best_idx"] == -1 and np.isnan(unscored["best_val"]) and unscored["score"] is None
    # the mean alone needs no operator: a model without G, bit for bit the mean of the full call
    kernel = mod["kernel"]
    bare = eng.mean_posterior(mod["X"], mod["th"], kernel, mod["m"], post.alpha)
    mean = eng.predict_gradients(bare, Xb, want_cov=False)
    assert mean["cov"] is None
    assert np.array_equal(host(mean["mean"])[~bad], host(clean["mean"])[~bad]) and np.all(np.isnan(host(mean["mean"])[bad]))


def test_metric_through_the_library(eng):
    """h_metric weighs the diagonal: both kinds against NumPy on the call's own outputs; NULL is all ones."""
    from ppbo_amd.engine import GRAD_NORM2, GRAD_TRACE, _ptr
    mod = _model("RQ-6-8-3-edge")
    post = mod["post"]
    X = _reference("RQ-6-8-3-edge", 37, 3)[0]
    dx, mean, cov, sc = eng.dev(X), eng.empty(37, 6), eng.empty(37, 6, 6), eng.empty(37)
    md = eng._model(post, True)
    w = np.array([0.5, 2.0, 1.0, 7.0, 0.01, 3.0])
    for metric in (None, w):
        for kind in (GRAD_TRACE, GRAD_NORM2):
            bv, bi = C.c_double(0.0), C.c_int64(-2)
            rc = eng.lib.ppbo_predict_gradients(eng.ctx, C.byref(md), _ptr(dx), 37, eng._dptr(metric) if metric is not None else None,
                                                kind, _ptr(mean), _ptr(cov), _ptr(sc), C.byref(bv), C.byref(bi), eng._stream())
            assert rc == 0, eng._err()
            m, Cv, s = host(mean), host(cov), host(sc)
            ww = np.ones(6) if metric is None else w
            want = (ww * (np.diagonal(Cv, axis1=1, axis2=2) + (m * m if kind == GRAD_NORM2 else 0.0))).sum(axis=1)
            assert np.max(np.abs(s - want) / want) <= 1e-13
            assert bi.value == int(np.argmax(s)) and bv.value == s.max()


# ---------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_context_usable(eng):
    from ppbo_amd.engine import GRAD_NONE, GRAD_NORM2, GRAD_TRACE, _ptr
    mod = _model("SE-6-8-3-node")
    post = mod["post"]
    X = _reference("SE-6-8-3-node", 37, 3)[0]
    before = eng.predict_gradients(post, X)
    dx, mean, cov, sc = eng.dev(X), eng.empty(37, 6), eng.empty(37, 6, 6), eng.empty(37)
    md, md32, bare = eng._model(post, True), eng._model(post, True, kstar_fp32=True), eng._model(post, False)
    nolam = eng._model(post, True)
    nolam.d_lam_diag = 0

    def call(model, x, M, kind, d_cov=None, d_score=None, metric=None):
        rc = eng.lib.ppbo_predict_gradients(eng.ctx, C.byref(model) if model is not None else None, _ptr(x), M,
                                            eng._dptr(np.asarray(metric, dtype=np.float64)) if metric is not None else None, kind,
                                            _ptr(mean), _ptr(d_cov), _ptr(d_score), None, None, eng._stream())
        return rc, eng._err()

    for args in ((None, dx, 37, GRAD_NONE), (md, None, 37, GRAD_NONE), (md, dx, 0, GRAD_NONE), (md, dx, -5, GRAD_NONE),
                 (md, dx, 2 ** 31, GRAD_NONE), (md, dx, 37, 3), (md, dx, 37, -1), (md32, dx, 37, GRAD_NONE),
                 (md, dx, 37, GRAD_TRACE, None, None, [1, 1, 0, 1, 1, 1]), (md, dx, 37, GRAD_TRACE, None, None, [1, -2, 1, 1, 1, 1]),
                 (md, dx, 37, GRAD_TRACE, None, None, [1, 1, 1, np.inf, 1, 1]), (md, dx, 37, GRAD_TRACE, None, None, [np.nan, 1, 1, 1, 1, 1]),
                 (bare, dx, 37, GRAD_TRACE), (bare, dx, 37, GRAD_NORM2, None, sc), (bare, dx, 37, GRAD_NONE, cov),
                 (nolam, dx, 37, GRAD_NONE, cov), (nolam, dx, 37, GRAD_TRACE)):
        rc, msg = call(*args)
        assert rc != 0 and "invalid argument" in msg, (args[2:4], rc, msg)
    assert call(bare, dx, 37, GRAD_NONE)[0] == 0          # the mean alone: no operator needed
    assert call(md, dx, 37, GRAD_NORM2, cov, sc, [1, 2, 3, 4, 5, 6])[0] == 0
    after = eng.predict_gradients(post, X)
    for k in ("mean", "cov"):
        assert np.array_equal(host(before[k]), host(after[k]))
    with pytest.raises(ValueError, match="predict_gradients"):
        eng.predict_gradients(post, X[:, :5])
    with pytest.raises(ValueError, match="score kind"):
        eng.predict_gradients(post, X, score=7)


# ---------------------------------------------------------------- 5. GPModel
def test_gradient_pred_is_the_engine_call(eng):
    for which in ("SE-6-8-3-node", "camphor_ard"):
        mod = _model(which)
        X = _reference(which, 37, 3)[0]
        gp = _stub_gp(eng, mod)
        m, Cv = gp.gradient_pred(X)
        out = eng.predict_gradients(mod["post"], X)
        assert np.array_equal(m, host(out["mean"])) and np.array_equal(Cv, host(out["cov"]))
        one = gp.gradient_pred(X[7])
        assert one[0].shape == (1, X.shape[1]) and one[1].shape == (1, X.shape[1], X.shape[1])
        assert np.max(np.abs(one[1][0] - Cv[7])) <= 1e-9 * np.abs(Cv[7]).max()


def _peak_and_saddle(eng, gp, mod):
    """An interior maximiser of the posterior mean with a negative definite Hessian, and a point whose Hessian has a
    positive eigenvalue."""
    D = mod["X"].shape[1]
    xs, _ = eng.mean_search(mod["post"], np.random.default_rng(1).random((4096, D)))
    peak = next((x for x in xs if np.all((x > 0.02) & (x < 0.98)) and np.linalg.eigvalsh(gp.mean_hessian(x)).max() < 0.0), None)
    saddle = next((x for x in np.random.default_rng(2).random((64, D)) if np.linalg.eigvalsh(gp.mean_hessian(x)).max() > 0.0), None)
    assert peak is not None and saddle is not None
    return peak, saddle


def test_xstar_covariance_and_loosest_direction(eng):
    mod = _model("SE-3-8-3-node")
    gp = _stub_gp(eng, mod)
    peak, saddle = _peak_and_saddle(eng, gp, mod)
    r = gp.xstar_covariance(peak)
    H = gp.mean_hessian(peak)
    m, Cv = gp.gradient_pred(peak)
    want = gn.xstar_covariance(H, Cv[0])
    assert np.array_equal(r["hessian"], H) and np.array_equal(r["grad_cov"], Cv[0]) and np.array_equal(r["grad_mean"], m[0])
    assert np.max(np.abs(r["cov"] - want)) <= 1e-12 * np.abs(want).max()
    assert np.all(np.diff(r["lengths"]) <= 0.0) and np.all(r["lengths"] >= 0.0)
    assert np.max(np.abs(r["axes"] @ r["cov"] @ r["axes"].T - np.diag(r["lengths"] ** 2))) <= 1e-10 * r["lengths"][0] ** 2
    xi = gp.loosest_direction(peak)
    a = np.abs(r["axes"][0])
    assert np.array_equal(xi, a / a.max()) and xi.max() == 1.0
    gp.xstar = peak
    assert np.array_equal(gp.loosest_direction(), xi) and np.array_equal(gp.xstar_covariance()["cov"], r["cov"])
    with pytest.raises(ValueError, match="negative definite"):
        gp.xstar_covariance(saddle)
    with pytest.raises(ValueError, match="negative definite"):
        gp.loosest_direction(saddle)
    m32 = _model("Matern32-6-8-3-node")
    with pytest.raises(ValueError, match="Matern32_kernel"):
        _stub_gp(eng, m32).xstar_covariance(m32["X"][0])


def test_active_subspace_on_given_points(eng):
    for which in ("SE-6-8-3-edge", "Matern52-6-3-25-node-ard", "camphor_ard"):
        mod = _model(which)
        X, m0, C0, _, _ = _reference(which, 37, 3)
        w, V = _stub_gp(eng, mod).active_subspace(X=X)
        A0 = gn.active_matrix(m0, C0)
        A = V.T @ np.diag(w) @ V
        e = np.max(np.abs(A - A0)) / np.abs(A0).max()
        print(f"gradients active subspace {which}: |A - ref| / max|ref| = {e:.2e}")
        assert e <= TOL and np.all(np.diff(w) <= 0.0)
        assert np.max(np.abs(V @ V.T - np.eye(X.shape[1]))) <= 1e-12
    w1, V1 = _stub_gp(eng, mod).active_subspace(n_points=64, seed=4)
    w2, V2 = _stub_gp(eng, mod).active_subspace(X=np.random.default_rng(4).random((64, 6)))
    assert np.array_equal(w1, w2) and np.array_equal(V1, V2)


def test_rotated_ridge_leads_the_active_subspace(eng):
    """gradients_numpy.ridge_design fitted on the device: the leading eigenvector is within 10 degrees of the one direction
    the design varies in (the NumPy statement on an oracle fit: 4.2 degrees, tests/test_gradients_host.py) -- a direction
    no coordinate-wise importance can name."""
    R = gn.RIDGE
    X, u = gn.ridge_design()
    r = eng.gp_fit(X, R["theta"], R["kernel"], R["m"], np.zeros(X.shape[0]), gtol=1e-6, start_is_whitened=True, form=_forms()["edge"])
    assert r["post"] is not None
    w, V = _stub_gp(eng, dict(post=r["post"])).active_subspace(X=gn.ridge_points())
    angle = gn.angle_degrees(V[0], u)
    print(f"gradients ridge on the device: angle {angle:.2f} degrees, eigenvalues {w[0]:.3f} {w[1]:.3f}")
    assert angle <= 10.0
    assert np.abs(u).max() < 0.95           # rotated: no coordinate axis
