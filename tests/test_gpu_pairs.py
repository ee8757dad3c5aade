"""GPU: duels -- ppbo_predict_pairs / Engine.predict_pairs / GPModel.preference_pred against the NumPy statement
(tests/pairs_numpy.py: oracle kernels on direct differences, the oracle's dense variance operator), the exact identities
of the construction, the reference-pinned covariance path, chunking, the argmax and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import pairs_numpy as pn
from conftest import golden_names, load_golden
from test_gpu_pathwise import _star_design

pytestmark = pytest.mark.gpu

ALL = golden_names()
RADIAL = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")
M_PAR = 2048 + 5          # ragged tail, odd, and enough columns for the padded-G path
TOL = 1e-6                # the package's parity tolerance (README, "Parity")


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def host(t):
    return t.detach().cpu().numpy()


def _theta(rng, D, ard):
    return [0.05, rng.uniform(0.25, 0.6, D) * np.sqrt(D / 6.0) if ard else 0.3 * np.sqrt(D / 6.0), 0.7]


@functools.lru_cache(maxsize=None)
def _fitted(kernel, D, form, n_q=7, m=25, ard=False):
    """One fitted star-design model per shape, shared by the tests: dict(post, X, th, m, alpha, A) with (alpha, A) the
    host's own (pairs_numpy.operator_from_fit on the device's f_MAP; nothing else of the device enters)."""
    from ppbo_amd.engine import get_engine
    eng = get_engine(0)
    rng = np.random.default_rng(1000 * D + 10 * n_q + m + (form or 0) + 7 * RADIAL.index(kernel))
    X = _star_design(rng, n_q, D, m)
    th = _theta(rng, D, ard)
    r = eng.gp_fit(X, th, kernel, m, rng.standard_normal(X.shape[0]), gtol=1e-6, start_is_whitened=True, form=form)
    assert r["post"] is not None and r["stats"]["converged"]
    alpha, A = pn.operator_from_fit(X, th, kernel, m, host(r["fMAP"]))
    return dict(post=r["post"], X=X, th=th, m=m, kernel=kernel, alpha=alpha, A=A)


@functools.lru_cache(maxsize=None)
def _fitted_golden(name, form):
    from ppbo_amd.engine import get_engine
    eng = get_engine(0)
    g = load_golden(name)
    X, th, kernel, m = g["X"], [float(v) for v in g["theta"]], str(g["kernel"]), int(g["m"])
    r = eng.gp_fit(X, th, kernel, m, g["f_init"], gtol=1e-6, form=form)
    assert r["post"] is not None
    alpha, A = pn.operator_from_fit(X, th, kernel, m, host(r["fMAP"]))
    return dict(post=r["post"], X=X, th=th, m=m, kernel=kernel, alpha=alpha, A=A)


def _pairs(rng, mod, M):
    """M duels in the box: uniform points, a few design rows on either side."""
    D = mod["X"].shape[1]
    Xa, Xb = rng.random((M, D)), rng.random((M, D))
    k = min(16, M // 4)
    Xa[:k] = mod["X"][rng.integers(0, mod["X"].shape[0], k)]
    Xb[k:2 * k] = mod["X"][rng.integers(0, mod["X"].shape[0], k)]
    return Xa, Xb


def _parity(eng, mod, M=M_PAR, seed=3, label=""):
    from ppbo_amd.misc import preference_probability
    Xa, Xb = _pairs(np.random.default_rng(seed), mod, M)
    out = eng.predict_pairs(mod["post"], Xa, Xb)
    mu, var, p = host(out["mu"]), host(out["var"]), host(out["prob"])
    mu0, var0 = pn.pair_reference(Xa, Xb, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"])
    p0 = preference_probability(mu0, var0, mod["th"][0])
    sf2 = float(mod["th"][2]) ** 2
    e_mu, e_var, e_p = np.abs(mu - mu0).max() / np.abs(mu0).max(), np.abs(var - var0).max() / sf2, np.abs(p - p0).max()
    print(f"pairs parity {label}: |mu_d - ref| / max|ref| = {e_mu:.2e}, |var_d - ref| / sf2 = {e_var:.2e}, |p - ref| = {e_p:.2e}")
    assert e_mu <= TOL and e_var <= TOL and e_p <= TOL
    assert out["best_idx"] == int(np.argmax(p)) and out["best_val"] == p.max()


# ---------------------------------------------------------------- 1. parity
def _forms():
    from ppbo_amd.engine import FORM_EDGE, FORM_NODE
    return {"node": FORM_NODE, "edge": FORM_EDGE}


@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("D", [6, 20, 40])
@pytest.mark.parametrize("kernel", RADIAL)
def test_parity_radial(eng, kernel, D, form):
    """Worst errors measured on MI355X over these 24 cases are recorded in DESIGN.md section 7."""
    _parity(eng, _fitted(kernel, D, _forms()[form]), label=f"{kernel} D={D} {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_ard(eng, form):
    _parity(eng, _fitted("Matern52_kernel", 6, _forms()[form], ard=True), label=f"Matern52 ARD D=6 {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_camphor(eng, form):
    _parity(eng, _fitted_golden("cam_small", _forms()[form]), label=f"camphor cam_small {form}")


# ---------------------------------------------------------------- 2. exact identities
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("Matern52_kernel", 20), ("RQ_kernel", 40)])
def test_exact_identities(eng, kernel, D, form):
    mod = _fitted(kernel, D, _forms()[form])
    Xa, Xb = _pairs(np.random.default_rng(5), mod, 777)
    same = eng.predict_pairs(mod["post"], Xa, Xa.copy())
    assert np.all(host(same["mu"]) == 0.0) and np.all(host(same["var"]) == 0.0) and np.all(host(same["prob"]) == 0.5)
    assert same["best_idx"] == 0 and same["best_val"] == 0.5          # all tied: the first index
    ab, ba = eng.predict_pairs(mod["post"], Xa, Xb), eng.predict_pairs(mod["post"], Xb, Xa)
    assert np.array_equal(host(ab["mu"]), -host(ba["mu"]))
    assert np.array_equal(host(ab["var"]), host(ba["var"]))
    assert np.abs(host(ab["prob"]) + host(ba["prob"]) - 1.0).max() <= 2 * np.finfo(float).eps
    again = eng.predict_pairs(mod["post"], Xa, Xb)
    for k in ("mu", "var", "prob"):
        assert np.array_equal(host(ab[k]), host(again[k]))
    assert (ab["best_idx"], ab["best_val"]) == (again["best_idx"], again["best_val"])


def test_exact_identities_camphor(eng):
    mod = _fitted_golden("cam_small", None)
    Xa, Xb = _pairs(np.random.default_rng(6), mod, 300)
    same = eng.predict_pairs(mod["post"], Xa, Xa.copy())
    assert np.all(host(same["mu"]) == 0.0) and np.all(host(same["var"]) == 0.0) and np.all(host(same["prob"]) == 0.5)
    ab, ba = eng.predict_pairs(mod["post"], Xa, Xb), eng.predict_pairs(mod["post"], Xb, Xa)
    assert np.array_equal(host(ab["mu"]), -host(ba["mu"])) and np.array_equal(host(ab["var"]), host(ba["var"]))


# ---------------------------------------------------------------- 3. near ties
@pytest.mark.parametrize("kernel", RADIAL)
def test_near_ties(eng, kernel):
    """Xb = Xa + 1e-4 u.  Asserted: var_d finite, >= -1e-12 sf2, within 1e-6 sf2 of the dense reference.  Reported, not
    gated (the dense fp64 reference loses digits at this separation too): the relative error of var_d."""
    mod = _fitted(kernel, 6, None)
    rng = np.random.default_rng(8)
    Xa = rng.random((1000, 6))
    u = rng.standard_normal((1000, 6))
    Xb = np.clip(Xa + 1e-4 * u / np.linalg.norm(u, axis=1, keepdims=True), 0.0, 1.0)
    out = eng.predict_pairs(mod["post"], Xa, Xb)
    var = host(out["var"])
    _, var0 = pn.pair_reference(Xa, Xb, mod["X"], mod["th"], kernel, mod["alpha"], mod["A"])
    sf2 = float(mod["th"][2]) ** 2
    print(f"near ties {kernel}: var_d in [{var.min():.3e}, {var.max():.3e}], reference in [{var0.min():.3e}, {var0.max():.3e}], "
          f"worst |var_d - ref| / |ref| = {np.max(np.abs(var - var0) / np.abs(var0)):.2e}")
    assert np.all(np.isfinite(var)) and var.min() >= -1e-12 * sf2
    assert np.abs(var - var0).max() <= TOL * sf2


# ---------------------------------------------------------------- 4. the reference-pinned covariance path
def _golden_gp(g):
    """The set-up of tests/test_gpu_dropin.py: a GPModel on the reference's own design and f_MAP."""
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    st = PPBO_settings(D=int(g["D"]), bounds=tuple(map(tuple, g["bounds"])), xi_acquisition_function="PCD",
                       theta_initial=list(g["theta"]), m=int(g["m"]), verbose=False, kernel=str(g["kernel"]))
    gp = GPModel(st)
    np.random.seed(0)
    gp.update_feedback_processing_object(g["X_obs"])
    gp.FP.X = g["X"].copy()
    gp.update_data()
    gp.set_theta(); gp.update_Sigma(gp.theta); gp.update_Sigma_inv(gp.theta)
    gp.fMAP = g["fMAP"].copy()
    gp.initialization_running = False
    gp._post = gp.eng.posterior(gp._dX, gp.theta, gp.kernel.__name__, gp._dSigma_inv, gp.eng.dev(gp.fMAP), gp.m)
    gp._post_mean = gp._post
    return gp


@pytest.mark.parametrize("name", [n for n in ("rq", "smoke") if n in ALL])
def test_tie_to_mu_Sigma_pred(name):
    """var_d = C_aa + C_bb - 2 C_ab - 2 s k(a, b) and mu_d = mu_a - mu_b with (mu, C) = mu_Sigma_pred: the reference
    shrinks its M x M prior block by s (diagonal back to sf2), the duel does not."""
    g = load_golden(name)
    gp = _golden_gp(g)
    rng = np.random.default_rng(12)
    pts = rng.random((32, gp.D))
    ia, ib = rng.integers(0, 32, 64), rng.integers(0, 32, 64)
    ib = np.where(ia == ib, (ib + 1) % 32, ib)
    mu, Cv = gp.mu_Sigma_pred(pts)
    mu_d, var_d, p = gp.preference_pred(pts[ia], pts[ib])
    s, sf2 = gp.COVARIANCE_SHRINKAGE, float(g["theta"][2]) ** 2
    kab = pn.pair_kernel(pts[ia], pts[ib], [float(v) for v in g["theta"]], str(g["kernel"]))
    want = Cv[ia, ia] + Cv[ib, ib] - 2.0 * Cv[ia, ib] - 2.0 * s * kab
    print(f"tie to mu_Sigma_pred {name}: |var_d - want| / sf2 = {np.abs(var_d - want).max() / sf2:.2e}, "
          f"|mu_d - want| / max|mu| = {np.abs(mu_d - (mu[ia] - mu[ib])).max() / np.abs(mu).max():.2e}")
    assert np.abs(var_d - want).max() <= TOL * sf2
    assert np.abs(mu_d - (mu[ia] - mu[ib])).max() <= TOL * np.abs(mu).max()
    from ppbo_amd.misc import preference_probability
    assert np.abs(p - preference_probability(mu_d, var_d, gp.theta[0])).max() <= 4 * np.finfo(float).eps


# ---------------------------------------------------------------- 5. shapes that take other branches
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("m,n_q,D", [(31, 4, 6), (25, 80, 20)])
def test_parity_other_shapes(eng, m, n_q, D, form):
    """N = 128 (aligned: the model's own G, lean main loop) and N = 2080 (padded operands at full width)."""
    _parity(eng, _fitted("SE_kernel", D, _forms()[form], n_q=n_q, m=m), label=f"SE D={D} N={n_q * (m + 1)} {form}")


# ---------------------------------------------------------------- 6. chunking
def test_chunks_equal_separate_calls(eng):
    mod = _fitted("SE_kernel", 6, None)
    M = 65536 + 123
    Xa, Xb = _pairs(np.random.default_rng(9), mod, M)
    full = eng.predict_pairs(mod["post"], Xa, Xb, want_score=True)
    h = M // 2
    lo, hi = eng.predict_pairs(mod["post"], Xa[:h], Xb[:h]), eng.predict_pairs(mod["post"], Xa[h:], Xb[h:])
    for k in ("mu", "var", "prob"):
        assert np.array_equal(host(full[k]), np.concatenate([host(lo[k]), host(hi[k])]))
    p = host(full["prob"])
    assert np.array_equal(host(full["score"]), p)
    i = int(np.argmax(p))
    assert full["best_idx"] == i and full["best_val"] == p[i]
    # the winner moved into the second chunk: the index that comes back is the global row
    j = 65536 + 7
    Xa[[i, j]], Xb[[i, j]] = Xa[[j, i]], Xb[[j, i]]
    moved = eng.predict_pairs(mod["post"], Xa, Xb, want_mu=False, want_var=False, want_prob=False)
    assert moved["best_idx"] == (j if np.count_nonzero(p == p[i]) == 1 else min(j, int(np.flatnonzero(p == p[i])[0])))
    assert moved["best_val"] == p[i]


# ---------------------------------------------------------------- 7. score kinds, NaN rows, the mean without an operator
@pytest.mark.parametrize("form", ["node", "edge"])
def test_score_kinds_and_argmax(eng, form):
    from ppbo_amd.engine import PAIR_MEAN, PAIR_PROB, PAIR_VARIANCE
    mod = _fitted("RQ_kernel", 6, _forms()[form])
    Xa, Xb = _pairs(np.random.default_rng(10), mod, 3001)
    clean = eng.predict_pairs(mod["post"], Xa, Xb)
    Xa[3, 2], Xb[10, 0], Xa[2999, 5] = np.nan, np.nan, np.inf
    bad = np.zeros(3001, dtype=bool)
    bad[[3, 10, 2999]] = True
    for kind, key in ((PAIR_MEAN, "mu"), (PAIR_VARIANCE, "var"), (PAIR_PROB, "prob")):
        out = eng.predict_pairs(mod["post"], Xa, Xb, score=kind, want_score=True)
        sc = host(out["score"])
        assert np.array_equal(sc, host(out[key]), equal_nan=True)
        for k in ("mu", "var", "prob"):
            v = host(out[k])
            assert np.all(np.isnan(v[bad])) and np.array_equal(v[~bad], host(clean[k])[~bad])
        assert out["best_idx"] == int(np.nanargmax(sc)) and out["best_val"] == np.nanmax(sc)
        assert not bad[out["best_idx"]]
    # nothing but NaN rows: (NaN, -1)
    none = eng.predict_pairs(mod["post"], Xa[[3, 10]], Xb[[3, 10]])
    assert none["best_idx"] == -1 and np.isnan(none["best_val"])
    # the mean alone needs no operator: a model without G, bit for bit the mean of the full call
    post = mod["post"]
    bare = eng.mean_posterior(mod["X"], mod["th"], mod["kernel"], mod["m"], post.alpha)
    mean = eng.predict_pairs(bare, Xa, Xb, score=PAIR_MEAN, want_var=False, want_prob=False, want_score=True)
    assert mean["var"] is None and mean["prob"] is None
    assert np.array_equal(host(mean["mu"])[~bad], host(clean["mu"])[~bad]) and np.all(np.isnan(host(mean["mu"])[bad]))
    assert mean["best_idx"] == int(np.nanargmax(host(mean["score"])))


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_context_usable(eng):
    from ppbo_amd.engine import PAIR_MEAN, PAIR_PROB, _ptr
    mod = _fitted("SE_kernel", 6, None)
    post = mod["post"]
    Xa, Xb = _pairs(np.random.default_rng(11), mod, 100)
    before = eng.predict_pairs(post, Xa, Xb)
    da, db, mu = eng.dev(Xa), eng.dev(Xb), eng.empty(100)
    md, md32, bare = eng._model(post, True), eng._model(post, True, kstar_fp32=True), eng._model(post, False)

    def call(model, a, b, M, kind):
        rc = eng.lib.ppbo_predict_pairs(eng.ctx, C.byref(model) if model is not None else None, _ptr(a), _ptr(b), M, kind,
                                        _ptr(mu), None, None, None, None, None, eng._stream())
        return rc, eng._err()

    for args in ((None, da, db, 100, PAIR_PROB), (md, None, db, 100, PAIR_PROB), (md, da, None, 100, PAIR_PROB),
                 (md, da, db, 0, PAIR_PROB), (md, da, db, -5, PAIR_PROB), (md, da, db, 2 ** 31, PAIR_PROB),
                 (md, da, db, 100, 3), (md, da, db, 100, -1), (md32, da, db, 100, PAIR_PROB), (bare, da, db, 100, PAIR_PROB)):
        rc, msg = call(*args)
        assert rc < 0 and msg.startswith("invalid argument"), (args[3:], rc, msg)
    assert call(bare, da, db, 100, PAIR_MEAN)[0] == 0          # the mean alone: no operator needed
    after = eng.predict_pairs(post, Xa, Xb)
    for k in ("mu", "var", "prob"):
        assert np.array_equal(host(before[k]), host(after[k]))
    with pytest.raises(ValueError, match="predict_pairs"):
        eng.predict_pairs(post, Xa, Xb[:50])
    with pytest.raises(ValueError, match="predict_pairs"):
        eng.predict_pairs(post, Xa[:, :5], Xb[:, :5])
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = None
    with pytest.raises(RuntimeError, match="posterior covariance unavailable"):
        gp.preference_pred(Xa[0], Xb[0])


# ---------------------------------------------------------------- 9. the drop-in surface
def _six_hump(v):
    x, y = v[..., 0], v[..., 1]
    return (4 - 2.1 * x ** 2 + x ** 4 / 3) * x ** 2 + x * y + (-4 + 4 * y ** 2) * y ** 2


def test_preference_pred_on_the_six_hump_camel_loop():
    """BASELINE config 1 (D = 2, 4 corner queries + 21 PCD queries, m = 25): the model prefers its x* to the corner of the
    box farthest from it, and no point to itself."""
    from ppbo_amd.misc import hypercube_corners
    from ppbo_amd.numerical_main import line_search_user, run_ppbo_loop
    from ppbo_amd.ppbo_settings import PPBO_settings
    np.random.seed(0)
    bounds = ((-3, 3), (-2, 2))
    lo, hi = np.array([-3.0, -2.0]), np.array([3.0, 2.0])
    st = PPBO_settings(D=2, bounds=bounds, xi_acquisition_function="PCD", m=25, theta_initial=[0.01, 0.26, 0.1],
                       verbose=False)
    xis = np.tile(np.diag(hi), (2, 1))
    xs = hypercube_corners(bounds)[:4].astype(float)
    _, _, _, gp = run_ppbo_loop(line_search_user(_six_hump, lo, hi), xis, xs, 21, st)
    xstar = np.asarray(gp.xstar, dtype=float)
    far = np.where(xstar < 0.5, 1.0, 0.0)
    mu_d, var_d, p = gp.preference_pred(xstar, far)
    print(f"six-hump camel: P(x* > far corner) = {p[0]:.4f} (mu_d = {mu_d[0]:.3e}, var_d = {var_d[0]:.3e})")
    assert mu_d.shape == var_d.shape == p.shape == (1,)
    assert p[0] > 0.5 and mu_d[0] > 0.0 and var_d[0] >= 0.0
    mu0, var0, p0 = gp.preference_pred(xstar, xstar)
    assert (mu0[0], var0[0], p0[0]) == (0.0, 0.0, 0.5)
    # device input, many pairs
    import torch
    A = torch.as_tensor(np.tile(xstar, (5, 1)), device=gp.eng.device)
    B = torch.as_tensor(np.tile(far, (5, 1)), device=gp.eng.device)
    mu5, var5, p5 = gp.preference_pred(A, B)
    assert np.all(mu5 == mu_d[0]) and np.all(var5 == var_d[0]) and np.all(p5 == p[0])
