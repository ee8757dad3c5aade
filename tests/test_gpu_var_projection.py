"""GPU: the projected edge form (ppbo_var_projection_build and the entries that read ppbo_model.proj) against the same entries
without a projection.

The models are real edge-form posteriors of small star designs (ppbo_posterior on a smooth latent vector, or ppbo_gp_fit):
a RANDOM operator of the edge form's sparsity has no decaying spectrum, so nothing could be projected.  N = 384 (n_q = 12,
m = 31) is the smallest shape with r_max = 128; N = 416 (n_q = 16, m = 25) has ragged 26-row stars and padded operands.

Bounds: the projection's own -- |var_p - var| <= proj.bound <= tol sf2, var_p >= var -- plus 1e-14 sf2 for the rounding of
two differently ordered fp64 sums of terms of size <= a few sf2 (depth <= 2048: ~1e-15 sf2; the one-sided check scales it
with the largest |var| of the call, the size of the summed terms).  The golden-vector bound
(1e-6 sf2) and the search's 1e-9 relative are the project's and the issue's own."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 1e-10
ROUND = 1e-14


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def host(t):
    return t.detach().cpu().numpy()


def star_design(rng, n_q, m, D):
    X = np.empty((n_q, m + 1, D))
    for q in range(n_q):
        xo = 0.3 + 0.4 * rng.random(D)
        xi = rng.uniform(0.2, 1.0, D) * rng.choice([-1.0, 1.0], D)
        s = rng.uniform(-0.3, 0.3, m)
        s[0] = -0.25
        X[q, 0] = xo
        X[q, 1:] = xo + s[:, None] * xi
    return X.reshape(n_q * (m + 1), D)


def r_max(N, m):
    return ((N - N // (m + 1)) * 4 // 10) // 128 * 128


# name -> (n_q, m, D, kernel, length scale(s)); sigma = 0.1, sigma_f = 1.3, latent vector 0.5 L z
DESIGNS = {
    "se": (12, 31, 2, "SE_kernel", 0.8),
    "ragged": (16, 25, 2, "SE_kernel", 1.5),
    "ard": (12, 31, 2, "SE_kernel", [0.6, 1.2]),
    "matern52": (12, 31, 2, "Matern52_kernel", 3.0),
}


def smooth_posterior(eng, n_q, m, D, kernel, l, form=None, seed=1):
    from ppbo_amd.engine import FORM_EDGE
    rng = np.random.default_rng(seed)
    X = star_design(rng, n_q, m, D)
    th = [0.1, l, 1.3]
    S = eng.gram(X, th, kernel)
    f = 0.5 * eng.dgemv(eng.potrf_(S.clone()), rng.standard_normal(X.shape[0]), lower=True)
    return eng.posterior(X, th, kernel, eng.pd_inverse(S), f, m, form=FORM_EDGE if form is None else form), rng


@pytest.fixture(scope="module")
def built(eng):
    """Every design's posterior with its projection, built once."""
    out = {}
    for name, (n_q, m, D, kernel, l) in DESIGNS.items():
        post, rng = smooth_posterior(eng, n_q, m, D, kernel, l)
        out[name] = (post, eng.project_variance(post, TOL), rng.random((70000, D)))
    return out


# ---- the three entries, called directly: pj (None or a VarianceProjection) travels in the model, ppbo_model.proj -------------
def call_predict(eng, post, Xc, score, mustar, pj):
    """(mu, var, score, best value, best index) of ppbo_predict."""
    from ppbo_amd.engine import _ptr
    Xd = eng._points(post, Xc)
    M = Xd.shape[0]
    md = eng._model(post, True, projection=pj)
    mu, var, sc = eng.empty(M), eng.empty(M), eng.empty(M)
    bv, bi = C.c_double(0.0), C.c_int64(-1)
    rc = eng.lib.ppbo_predict(eng.ctx, C.byref(md), _ptr(Xd), M, int(score), float(mustar), _ptr(mu), _ptr(var), _ptr(sc),
                              C.byref(bv), C.byref(bi), eng._stream())
    eng._check(rc, "ppbo_predict")
    return host(mu), host(var), host(sc), bv.value, bi.value


def call_record(eng, post, Xc, score, mustar, pj, offset=1000):
    from ppbo_amd.engine import _ptr
    Xd = eng._points(post, Xc)
    md = eng._model(post, True, projection=pj)
    rec = eng.empty(2)
    rc = eng.lib.ppbo_predict_record(eng.ctx, C.byref(md), _ptr(Xd), Xd.shape[0], int(score), float(mustar), offset, _ptr(rec),
                                     eng._stream())
    eng._check(rc, "ppbo_predict_record")
    return host(rec)


def call_search(eng, post, Xc, score, mustar, pj, offset=1000):
    from ppbo_amd.engine import _ptr
    Xd = eng._points(post, Xc)
    md = eng._model(post, True, projection=pj)
    bv, bi = C.c_double(0.0), C.c_int64(-1)
    rc = eng.lib.ppbo_search_sharded(eng.ctx, C.byref(md), _ptr(Xd), Xd.shape[0], int(score), float(mustar), offset,
                                     C.byref(bv), C.byref(bi), eng._stream())
    eng._check(rc, "ppbo_search_sharded")
    return bv.value, bi.value


# ---- the tests --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 513, 70000])
@pytest.mark.parametrize("name", list(DESIGNS))
def test_projected_against_exact(eng, built, name, M):
    """mu bit for bit; 0 <= var - var_p <= bound <= tol sf2 (+ rounding); the same argmax record.  M = 70000: two chunks."""
    from ppbo_amd.engine import SCORE_VARIANCE
    post, pj, Xall = built[name]
    n_q, m = DESIGNS[name][:2]
    sf2 = 1.3 ** 2
    assert pj.rows % 128 == 0 and 0 < pj.rows <= r_max(n_q * (m + 1), m) and pj.struct.rows_padded == pj.rows
    assert 0.0 <= pj.bound <= TOL * sf2
    Xc = Xall[:M]
    mu, var, sc, bv, bi = call_predict(eng, post, Xc, SCORE_VARIANCE, 0.0, None)
    mu_p, var_p, sc_p, bv_p, bi_p = call_predict(eng, post, Xc, SCORE_VARIANCE, 0.0, pj)
    d = var_p - var
    print(f"{name} M={M} rows={pj.rows} bound={pj.bound / sf2:.2e} sf2, var_p - var in [{d.min() / sf2:.2e}, {d.max() / sf2:.2e}] sf2, "
          f"largest reduction {(sf2 - var).max() / sf2:.2e} sf2")
    assert np.array_equal(mu, mu_p)
    assert np.abs(d).max() <= pj.bound + ROUND * sf2 and np.abs(d).max() <= TOL * sf2 + ROUND * sf2
    # the projection never over-subtracts: var_p >= var up to the rounding of the sums, which scales with their terms
    assert d.min() >= -ROUND * max(sf2, np.abs(var).max())
    assert bi == bi_p and abs(bv - bv_p) <= pj.bound + ROUND * sf2
    rec, rec_p = call_record(eng, post, Xc, SCORE_VARIANCE, 0.0, None), call_record(eng, post, Xc, SCORE_VARIANCE, 0.0, pj)
    assert rec[1] == rec_p[1] == 1000 + bi and abs(rec[0] - rec_p[0]) <= pj.bound + ROUND * sf2


def test_two_builds_give_the_same_bits(eng, built):
    post, pj, _ = built["ragged"]
    first = host(pj.T).copy()
    post.proj = None
    again = eng.project_variance(post, TOL)
    assert again is not pj and again.rows == pj.rows and again.bound == pj.bound
    assert np.array_equal(first, host(again.T))
    # the layout promised to the contraction: zero columns [0, n_q) and [N, ld), nothing but zeros behind row `rows`
    N, n_q = post.X.shape[0], post.X.shape[0] // (post.m + 1)
    assert not first[:, :n_q].any() and not first[:, N:].any() and not first[pj.rows:].any()
    assert first[:pj.rows, n_q:N].any()


def assert_same_bits(eng, post, pj, Xc):
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    assert pj.rows == 0
    a, b = call_predict(eng, post, Xc, SCORE_POINTWISE_EI, 0.1, None), call_predict(eng, post, Xc, SCORE_POINTWISE_EI, 0.1, pj)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3:] == b[3:]
    assert np.array_equal(call_record(eng, post, Xc, SCORE_POINTWISE_EI, 0.1, None), call_record(eng, post, Xc, SCORE_POINTWISE_EI, 0.1, pj))
    assert call_search(eng, post, Xc, SCORE_POINTWISE_EI, 0.1, None) == call_search(eng, post, Xc, SCORE_POINTWISE_EI, 0.1, pj)


def test_tolerance_out_of_reach(eng):
    """D = 20, a short length scale, N = 384, fitted: r_max = 128 leaves ~4e-11 sf2 (the shrinkage nugget), so a tolerance of
    1e-13 is refused -- rows == 0, and a model that carries it gives the bits of one that carries none."""
    from ppbo_amd.engine import FORM_EDGE
    rng = np.random.default_rng(1)
    X = star_design(rng, 12, 31, 20)
    fit = eng.gp_fit(X, [0.1, 0.3, 1.3], "SE_kernel", 31, np.zeros(384), form=FORM_EDGE)
    assert fit["post"] is not None
    pj = eng.project_variance(fit["post"], 1e-13)
    assert pj.rows == 0 and pj.struct.rows_padded == 0
    assert_same_bits(eng, fit["post"], pj, rng.random((600, 20)))


@pytest.mark.parametrize("n_q,D", [(4, 2), (12, 20)])
def test_node_form_models_take_no_projection(eng, n_q, D):
    """A model the one-launch kernel takes (N = 128, D = 2) and a node-form model of the three-launch path (N = 384, D = 20)."""
    from ppbo_amd.engine import FORM_NODE
    post, rng = smooth_posterior(eng, n_q, 31, D, "SE_kernel", 0.8 * np.sqrt(D / 2.0), form=FORM_NODE)
    assert_same_bits(eng, post, eng.project_variance(post, TOL), rng.random((600, D)))


REFUSED = "invalid argument: the variance projection was not built for a model of this N, m and form"


def test_a_projection_of_another_model_is_refused(eng, built):
    from ppbo_amd.engine import SCORE_VARIANCE
    post, _, Xall = built["ragged"]
    other = built["se"][1]
    with pytest.raises(RuntimeError, match=REFUSED):
        call_predict(eng, post, Xall[:64], SCORE_VARIANCE, 0.0, other)
    # ... and so is one handed to a node-form model
    from ppbo_amd.engine import FORM_NODE
    node, rng = smooth_posterior(eng, 12, 31, 20, "SE_kernel", 2.5, form=FORM_NODE)
    with pytest.raises(RuntimeError, match=REFUSED):
        call_predict(eng, node, rng.random((64, 20)), SCORE_VARIANCE, 0.0, other)


@pytest.mark.parametrize("field,value", [("ld", 400), ("rows_padded", 192), ("rows", 256), ("rows_padded", 1 << 20), ("d_T", None)])
def test_a_projection_that_does_not_fit_is_refused(eng, built, field, value):
    """The model's own projection (N = 384: ld = 384, rows = rows_padded = 128) with one member spoiled, in model.proj: a
    wrong stride, a padded row count that is no multiple of 128, more rows than padded rows, more padded rows than the model
    allows, no T -- each refused by all four reading entries."""
    from ppbo_amd import _lib
    from ppbo_amd.engine import SCORE_VARIANCE, VarianceProjection
    post, pj, Xall = built["se"]
    assert (pj.struct.ld, pj.struct.rows, pj.struct.rows_padded) == (384, 128, 128)
    st = _lib.VarProjection.from_buffer_copy(pj.struct)
    setattr(st, field, value)
    bad = VarianceProjection(pj.T, st, TOL)
    for call in (call_predict, call_record, call_search):
        with pytest.raises(RuntimeError, match=REFUSED):
            call(eng, post, Xall[:64], SCORE_VARIANCE, 0.0, bad)
    with pytest.raises(RuntimeError, match=REFUSED):
        eng.prune_report(post, Xall[:64], SCORE_VARIANCE, projection=bad)


def test_c3_fixture(eng):
    """The flagship model: rows <= 768; var within 1e-10 sf2 of the exact path on 4096 seeded candidates and within the
    project's 1e-6 sf2 of the golden vectors; the persistent search returns the same index with and without the projection."""
    from ppbo_amd.dist import ShardedSearch
    from ppbo_amd.engine import FORM_EDGE, SCORE_POINTWISE_EI
    g = dict(np.load(os.path.join(GOLDEN, "c3.npz"), allow_pickle=False))
    th, kern, m = g["theta"], str(g["kernel"]), int(g["m"])
    sf2 = float(th[2]) ** 2
    post = eng.posterior(g["X"], th, kern, eng.pd_inverse(eng.gram(g["X"], th, kern)), g["fMAP"], m, form=FORM_EDGE)
    pj = eng.project_variance(post, TOL)
    print(f"c3: rows={pj.rows} bound={pj.bound / sf2:.3e} sf2")
    assert pj.rows % 128 == 0 and 0 < pj.rows <= 768 and pj.bound <= TOL * sf2
    Xc = np.random.default_rng(4096).random((4096, g["X"].shape[1]))
    mustar = float(np.max(g["mu"]))
    mu, var, sc, bv, bi = call_predict(eng, post, Xc, SCORE_POINTWISE_EI, mustar, None)
    mu_p, var_p, sc_p, bv_p, bi_p = call_predict(eng, post, Xc, SCORE_POINTWISE_EI, mustar, pj)
    d = var_p - var
    print(f"c3: var_p - var in [{d.min() / sf2:.2e}, {d.max() / sf2:.2e}] sf2, largest reduction {(sf2 - var).max() / sf2:.2e} sf2")
    assert np.array_equal(mu, mu_p)
    assert d.min() >= -ROUND * sf2 and d.max() <= TOL * sf2 and d.max() <= pj.bound + ROUND * sf2
    gold = call_predict(eng, post, g["Xc"], SCORE_POINTWISE_EI, mustar, pj)
    print(f"c3: var_p against the golden vectors {np.abs(gold[1] - g['var']).max() / sf2:.2e} sf2")
    assert np.abs(gold[1] - g["var"]).max() <= 1e-6 * sf2
    on = ShardedSearch(eng, post, Xc, 0, SCORE_POINTWISE_EI, mustar, project=True)
    off = ShardedSearch(eng, post, Xc, 0, SCORE_POINTWISE_EI, mustar, project=False)
    assert on.projection is pj and off.projection is None
    (v_on, i_on), (v_off, i_off) = on.step(), off.step()
    assert i_on == i_off == bi and abs(v_on - v_off) <= 1e-9 * abs(v_off)


def bits(out):
    """Every array and number of an entry's result (a dict, a tuple, a tensor, an array or a scalar), as bytes."""
    if isinstance(out, dict):
        return [b for k in sorted(out) for b in bits(out[k])]
    if isinstance(out, (tuple, list)):
        return [b for v in out for b in bits(v)]
    if out is None:
        return [b""]
    return [np.ascontiguousarray(host(out) if hasattr(out, "detach") else out).tobytes()]


def test_every_other_entry_ignores_the_models_projection(eng, built, monkeypatch):
    """With EVERY descriptor carrying the posterior's projection (Engine._model patched), the entries that do not read
    ppbo_model.proj return the bits of the unpatched call; ppbo_predict, which reads it, stays within the projection's bound
    of the unprojected variance and does not return its bits, so the projection is not simply dropped everywhere."""
    from ppbo_amd.engine import Engine, SCORE_POINTWISE_EI, SCORE_VARIANCE
    post, pj, Xall = built["se"]          # N = 384, rows = 128: the smallest design of this file that is projected
    assert pj.rows > 0
    sf2 = 1.3 ** 2
    rng = np.random.default_rng(7)
    Xa, Xb, Xf = Xall[:300], Xall[300:600], Xall[600:616]
    Xi = rng.standard_normal((300, 2))
    grid, z = rng.random((4, 8, 2)), rng.standard_normal((16, 8))
    calls = {
        "pairs": lambda: eng.predict_pairs(post, Xa, Xb, want_score=True),
        "slopes": lambda: eng.predict_slopes(post, Xa, Xi, want_score=True),
        "tournament": lambda: eng.predict_tournament(post, Xa, Xf, want_cov=True, want_prob=True),
        "kg": lambda: eng.predict_kg(post, Xa, Xf, want_kinks=True),
        "search_batch": lambda: eng.search_batch(post, Xa, 3, SCORE_POINTWISE_EI, 0.1, want_var_cond=True),
        "cov": lambda: eng.predict_cov(post, Xa[:64]),
        "line_acq": lambda: eng.line_acq(post, grid, z, 0.1, jitter=1e-9 * sf2),
        "gradients": lambda: eng.predict_gradients(post, Xa),
        "mean_grad": lambda: eng.mean_grad(post, Xa),
    }
    plain = {name: bits(call()) for name, call in calls.items()}
    exact = eng.predict(post, Xa, SCORE_VARIANCE)
    projected = eng.predict(post, Xa, SCORE_VARIANCE, projection=pj)
    d = host(projected["var"]) - host(exact["var"])
    print(f"predict: var_p - var in [{d.min() / sf2:.2e}, {d.max() / sf2:.2e}] sf2, bound {pj.bound / sf2:.2e} sf2")
    assert np.array_equal(host(projected["mu"]), host(exact["mu"]))
    assert np.abs(d).max() <= pj.bound + ROUND * sf2 and d.any()

    model = Engine._model
    monkeypatch.setattr(Engine, "_model", lambda self, p, with_var=True, kstar_fp32=False, projection=None:
                        model(self, p, with_var, kstar_fp32, pj))
    assert eng._model(post).proj.rows == pj.rows
    for name, call in calls.items():
        assert bits(call()) == plain[name], name
    # ... and predict now reads it without being asked to
    assert bits(eng.predict(post, Xa, SCORE_VARIANCE)) == bits(projected)
