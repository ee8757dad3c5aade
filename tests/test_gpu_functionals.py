"""GPU: averages and contrasts -- ppbo_predict_functionals / Engine.predict_functionals / GPModel.functional_pred and its
layers against the NumPy statement (tests/functionals_numpy.py: oracle kernels on direct differences, the oracle's dense
variance operator, w' K w as the plain dense sum), the ties to ppbo_predict and ppbo_predict_pairs, the exact identities
of the construction, near-cancelling contrasts, chunking, the argmax, the NaN rule and the refusals.

Bound (TOL = 1e-6, the package's parity standard), normalised as the duel's: max|mu - ref| / max|ref|,
max|var - ref| / (sf^2 (sum |w|)^2), max|p - ref|.

Measured on MI355X (the worst row over all cases; profiles/r19_functionals.txt has them by group size): mean 9.2e-9 (1.5e-7
in the one M = 1 case, normalised by its single value; 2.3e-7 at N = 2080), variance 8.9e-9, |p - ref| 1.1e-9 (1.2e-8 at
N = 2080); G = 1 against ppbo_predict 4.7e-14 / 9.0e-15, G = 2 with (1, -1) against ppbo_predict_pairs 1.1e-13 / 3.0e-15."""
import ctypes as C
import functools

import numpy as np
import pytest

import functionals_numpy as fn
from test_gpu_pairs import RADIAL, TOL, _fitted, _fitted_golden, _forms, _six_hump, host

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
# (G, M, weights): every group size and column count of the issue, shared and per-group weights of the three kinds
COMBOS = ((1, 257, "random shared"), (2, 256, "contrast per group"), (3, 255, "average"), (16, 257, "random per group"),
          (17, 1, "contrast shared"), (64, 255, "random per group"), (64, 256, "average"), (2, 257, "random shared"))


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _groups(rng, mod, M, G):
    """M groups of G points in the box: uniform, a few of them design rows."""
    N, D = mod["X"].shape
    Xg = rng.random((M, G, D))
    k = max(1, min(16, M // 4))
    Xg[:k, 0] = mod["X"][rng.integers(0, N, k)]
    if G > 1:
        Xg[-k:, G - 1] = mod["X"][rng.integers(0, N, k)]
    return Xg


def _weights(rng, M, G, kind):
    shape = (M, G) if "per group" in kind else (G,)
    if kind.startswith("average"):
        return np.full(G, 1.0 / G)
    w = rng.standard_normal(shape)
    if kind.startswith("contrast"):
        w = w - w.mean(axis=-1, keepdims=True) if G > 1 else np.zeros(shape)
    return w


def _errors(mod, Xg, w, mu, var, p, threshold=0.0):
    mu0, var0 = fn.functional_reference(Xg, w, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"])
    p0 = fn.threshold_probability(mu0, var0, threshold)
    sf2 = float(mod["th"][2]) ** 2
    scale = sf2 * np.abs(np.broadcast_to(w, Xg.shape[:2])).sum(axis=1) ** 2
    return (np.abs(mu - mu0).max() / np.abs(mu0).max(), np.max(np.abs(var - var0) / scale), np.abs(p - p0).max())


def _parity(eng, mod, combos=COMBOS, seed=3, label=""):
    worst = np.zeros(3)
    for G, M, kind in combos:
        rng = np.random.default_rng(seed + 100 * G + M)
        Xg, w = _groups(rng, mod, M, G), _weights(rng, M, G, kind)
        thr = 0.0 if G % 2 else 0.05
        out = eng.predict_functionals(mod["post"], Xg, w, threshold=thr)
        mu, var, p = host(out["mu"]), host(out["var"]), host(out["prob"])
        if not np.any(w):          # G = 1 contrast: all-zero weights, exactly (0, 0, P(0 > thr))
            assert np.all(mu == 0.0) and np.all(var == 0.0)
            continue
        e = np.array(_errors(mod, Xg, w, mu, var, p, thr))
        worst = np.maximum(worst, e)
        print(f"functionals parity {label} G={G} M={M} {kind}: |mu - ref| / max|ref| = {e[0]:.2e}, "
              f"|var - ref| / (sf2 (sum|w|)^2) = {e[1]:.2e}, |p - ref| = {e[2]:.2e}")
        assert np.all(e <= TOL), (G, M, kind, e)
        assert out["best_idx"] == int(np.argmax(p)) and out["best_val"] == p.max()
    print(f"functionals parity {label} worst: mu {worst[0]:.2e}, var {worst[1]:.2e}, p {worst[2]:.2e}")


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("D", [6, 20, 40])
@pytest.mark.parametrize("kernel", RADIAL)
def test_parity_radial(eng, kernel, D, form):
    """Worst errors measured on MI355X over these cases are recorded in DESIGN.md section 7."""
    _parity(eng, _fitted(kernel, D, _forms()[form]), label=f"{kernel} D={D} {form}")


@pytest.mark.parametrize("D", [3, 50])
def test_parity_dimension_edges(eng, D):
    """D = 3 (one k-step, three of its four lanes' dimensions live) and D = 50 (the widest bucket, 14 padded dimensions)."""
    _parity(eng, _fitted("SE_kernel", D, None), combos=COMBOS[2:6], label=f"SE D={D}")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_ard(eng, form):
    _parity(eng, _fitted("Matern52_kernel", 6, _forms()[form], ard=True), label=f"Matern52 ARD D=6 {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_camphor(eng, form):
    _parity(eng, _fitted_golden("cam_small", _forms()[form]), label=f"camphor cam_small {form}")


def _stub_gp(eng, mod):
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp.eng, gp._post = eng, mod["post"]
    return gp


def test_parity_camphor_ard_through_functional_pred(eng):
    """SE on the 11 embedded columns with x~ = e(x), against the six-coordinate statement; host and device input."""
    from test_gpu_slopes import _fitted_camphor_ard
    mod = _fitted_camphor_ard()
    gp = _stub_gp(eng, mod)
    for G, M, kind in ((3, 257, "random per group"), (17, 64, "contrast shared"), (64, 33, "average")):
        rng = np.random.default_rng(G)
        Xg, w = _groups(rng, mod, M, G), _weights(rng, M, G, kind)
        mu, var, p = gp.functional_pred(Xg, w)
        e = _errors(mod, Xg, w, mu, var, p)
        print(f"functionals parity camphor ARD (functional_pred) G={G} M={M} {kind}: mu {e[0]:.2e}, var {e[1]:.2e}, p {e[2]:.2e}")
        assert max(e) <= TOL
    import torch
    dmu, dvar, dp = gp.functional_pred(torch.as_tensor(Xg[:5], device=eng.device), torch.as_tensor(w, device=eng.device))
    assert np.array_equal(dmu, mu[:5]) and np.array_equal(dvar, var[:5]) and np.array_equal(dp, p[:5])
    one = gp.functional_pred(Xg[7], w)
    assert one[0].shape == (1,) and one[0][0] == mu[7] and one[1][0] == var[7]


@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("m,n_q,D", [(31, 4, 6), (25, 80, 20)])
def test_parity_other_shapes(eng, m, n_q, D, form):
    """N = 128 (aligned: the model's own G, a slab = whole stars) and N = 2080 (padded operands, many row splits, a
    star's observation row carried across slabs)."""
    _parity(eng, _fitted("SE_kernel", D, _forms()[form], n_q=n_q, m=m), combos=(COMBOS[1], COMBOS[3], COMBOS[5]),
            label=f"SE D={D} N={n_q * (m + 1)} {form}")


# ---------------------------------------------------------------- 2. ties to the existing entries
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("Matern32_kernel", 20), ("RQ_kernel", 40), ("camphor", 6)])
def test_ties_to_predict_and_predict_pairs(eng, kernel, D, form):
    """G = 1, w = 1 is ppbo_predict's mean and variance; G = 2, w = (1, -1) is ppbo_predict_pairs' mu_d and var_d.  Other
    instructions, so not bitwise: the parity bound."""
    mod = _fitted_golden("cam_small", _forms()[form]) if kernel == "camphor" else _fitted(kernel, D, _forms()[form])
    rng = np.random.default_rng(21)
    sf2 = float(mod["th"][2]) ** 2
    Xg = _groups(rng, mod, 513, 2)
    one = eng.predict_functionals(mod["post"], Xg[:, :1].copy(), np.ones(1))
    ref = eng.predict(mod["post"], Xg[:, 0].copy(), want_best=False)
    e_mu = np.abs(host(one["mu"]) - host(ref["mu"])).max() / np.abs(host(ref["mu"])).max()
    e_var = np.abs(host(one["var"]) - host(ref["var"])).max() / sf2
    print(f"tie to predict {kernel} D={D} {form}: mu {e_mu:.2e}, var {e_var:.2e}")
    assert e_mu <= TOL and e_var <= TOL
    two = eng.predict_functionals(mod["post"], Xg, np.array([1.0, -1.0]))
    duel = eng.predict_pairs(mod["post"], Xg[:, 0].copy(), Xg[:, 1].copy(), want_best=False)
    e_mu = np.abs(host(two["mu"]) - host(duel["mu"])).max() / np.abs(host(duel["mu"])).max()
    e_var = np.abs(host(two["var"]) - host(duel["var"])).max() / (4.0 * sf2)
    print(f"tie to predict_pairs {kernel} D={D} {form}: mu {e_mu:.2e}, var {e_var:.2e}")
    assert e_mu <= TOL and e_var <= TOL


# ---------------------------------------------------------------- 3. exact identities
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("Matern52_kernel", 20), ("RQ_kernel", 40), ("camphor", 6)])
def test_exact_identities(eng, kernel, D, form):
    mod = _fitted_golden("cam_small", _forms()[form]) if kernel == "camphor" else _fitted(kernel, D, _forms()[form])
    post = mod["post"]
    rng = np.random.default_rng(5)
    M = 333
    a = _groups(rng, mod, M, 1)
    same = eng.predict_functionals(post, np.concatenate([a, a], axis=1), np.array([1.0, -1.0]))
    assert np.all(host(same["mu"]) == 0.0) and np.all(host(same["var"]) == 0.0) and np.all(host(same["prob"]) == 0.5)
    assert same["best_idx"] == 0 and same["best_val"] == 0.5          # all tied: the first index
    for G, per in ((5, True), (17, False)):
        Xg = _groups(rng, mod, M, G)
        zero = eng.predict_functionals(post, Xg, np.zeros((M, G) if per else G))
        assert np.all(host(zero["mu"]) == 0.0) and np.all(host(zero["var"]) == 0.0) and np.all(host(zero["prob"]) == 0.5)
        w = rng.standard_normal((M, G) if per else G)
        pos, neg, dbl = (eng.predict_functionals(post, Xg, f * w) for f in (1.0, -1.0, 2.0))
        assert np.array_equal(host(pos["mu"]), -host(neg["mu"]))
        assert np.array_equal(host(pos["var"]), host(neg["var"]))
        assert np.abs(host(pos["prob"]) + host(neg["prob"]) - 1.0).max() <= 2 * EPS
        assert np.array_equal(host(dbl["mu"]), 2.0 * host(pos["mu"]))
        assert np.array_equal(host(dbl["var"]), 4.0 * host(pos["var"]))
        again = eng.predict_functionals(post, Xg, w)
        for k in ("mu", "var", "prob"):
            assert np.array_equal(host(pos[k]), host(again[k]))
        assert (pos["best_idx"], pos["best_val"]) == (again["best_idx"], again["best_val"])
    # var = 0 at mu = threshold gives 1/2, the sign decides otherwise
    thr = eng.predict_functionals(post, np.concatenate([a, a], axis=1), np.array([1.0, -1.0]), threshold=0.25)
    assert np.all(host(thr["prob"]) == 0.0)
    thr = eng.predict_functionals(post, np.concatenate([a, a], axis=1), np.array([1.0, -1.0]), threshold=-0.25)
    assert np.all(host(thr["prob"]) == 1.0)


def test_chunk_edge_and_half_calls(eng):
    """M = 65541 at G = 2 crosses a chunk: parity on rows either side of the edge, one call against two half-calls
    bitwise, and the argmax across chunks."""
    mod = _fitted("SE_kernel", 6, None)
    rng = np.random.default_rng(9)
    M = 65541
    Xg, w = _groups(rng, mod, M, 2), rng.standard_normal((M, 2))
    full = eng.predict_functionals(mod["post"], Xg, w, want_score=True)
    h = M // 2
    lo = eng.predict_functionals(mod["post"], Xg[:h], w[:h])
    hi = eng.predict_functionals(mod["post"], Xg[h:], w[h:])
    for k in ("mu", "var", "prob"):
        assert np.array_equal(host(full[k]), np.concatenate([host(lo[k]), host(hi[k])]))
    sel = np.r_[0:64, 65536 - 64:65541]
    e = _errors(mod, Xg[sel], w[sel], host(full["mu"])[sel], host(full["var"])[sel], host(full["prob"])[sel])
    print(f"functionals parity across the chunk edge (M = 65541, G = 2): mu {e[0]:.2e}, var {e[1]:.2e}, p {e[2]:.2e}")
    assert max(e) <= TOL
    p = host(full["prob"])
    assert np.array_equal(host(full["score"]), p)
    i = int(np.argmax(p))
    assert full["best_idx"] == i and full["best_val"] == p[i]
    # shared weights take the same chunk steps
    ws = eng.predict_functionals(mod["post"], Xg, w[0].copy())
    tail = eng.predict_functionals(mod["post"], Xg[65536:], w[0].copy())
    assert np.array_equal(host(ws["mu"])[65536:], host(tail["mu"])) and np.array_equal(host(ws["var"])[65536:], host(tail["var"]))


# ---------------------------------------------------------------- 4. near-cancellation
@pytest.mark.parametrize("kernel", RADIAL)
def test_near_cancellation(eng, kernel):
    """w = (1/G, ..., 1/G, -1) on a cloud of radius 1e-4 around x against x itself.  Asserted: var finite,
    >= -1e-12 sf2, within 1e-6 sf2 (sum|w|)^2 of the dense reference.  Reported, not gated (the dense fp64 reference loses
    digits at this separation too): the relative error of var."""
    mod = _fitted(kernel, 6, None)
    rng = np.random.default_rng(8)
    M, G = 500, 8
    x = rng.random((M, 1, 6))
    u = rng.standard_normal((M, G, 6))
    cloud = np.clip(x + 1e-4 * u / np.linalg.norm(u, axis=2, keepdims=True), 0.0, 1.0)
    Xg = np.concatenate([cloud, x], axis=1)
    w = np.concatenate([np.full(G, 1.0 / G), [-1.0]])
    out = eng.predict_functionals(mod["post"], Xg, w)
    var = host(out["var"])
    _, var0 = fn.functional_reference(Xg, w, mod["X"], mod["th"], kernel, mod["alpha"], mod["A"])
    sf2 = float(mod["th"][2]) ** 2
    print(f"near cancellation {kernel}: var in [{var.min():.3e}, {var.max():.3e}], reference in [{var0.min():.3e}, "
          f"{var0.max():.3e}], worst |var - ref| / |ref| = {np.max(np.abs(var - var0) / np.abs(var0)):.2e}")
    assert np.all(np.isfinite(var)) and var.min() >= -1e-12 * sf2
    assert np.abs(var - var0).max() <= TOL * sf2 * np.abs(w).sum() ** 2


# ---------------------------------------------------------------- 5. score kinds, NaN groups, the mean without an operator
@pytest.mark.parametrize("form", ["node", "edge"])
def test_score_kinds_nan_groups_and_argmax(eng, form):
    from ppbo_amd.engine import FUNCTIONAL_MEAN, FUNCTIONAL_PROB, FUNCTIONAL_VARIANCE
    mod = _fitted("RQ_kernel", 6, _forms()[form])
    rng = np.random.default_rng(10)
    M, G = 1001, 5
    Xg, w = _groups(rng, mod, M, G), rng.standard_normal((M, G))
    w[3] = 0.0                                         # a poisoned group with zero weights is NaN all the same
    clean = eng.predict_functionals(mod["post"], Xg, w)
    Xg[3, 2, 1], Xg[10, 0, 0], Xg[999, 4, 5] = np.nan, np.nan, np.inf
    bad = np.zeros(M, dtype=bool)
    bad[[3, 10, 999]] = True
    for kind, key in ((FUNCTIONAL_MEAN, "mu"), (FUNCTIONAL_VARIANCE, "var"), (FUNCTIONAL_PROB, "prob")):
        out = eng.predict_functionals(mod["post"], Xg, w, score=kind, want_score=True)
        sc = host(out["score"])
        assert np.array_equal(sc, host(out[key]), equal_nan=True)
        for k in ("mu", "var", "prob"):
            v = host(out[k])
            assert np.all(np.isnan(v[bad])) and np.array_equal(v[~bad], host(clean[k])[~bad])    # neighbours untouched
        assert out["best_idx"] == int(np.nanargmax(sc)) and out["best_val"] == np.nanmax(sc)
        assert not bad[out["best_idx"]]
    none = eng.predict_functionals(mod["post"], Xg[[3, 10]], w[[3, 10]])
    assert none["best_idx"] == -1 and np.isnan(none["best_val"])
    # the mean alone needs no operator: a model without G, bit for bit the mean of the full call
    bare = eng.mean_posterior(mod["X"], mod["th"], mod["kernel"], mod["m"], mod["post"].alpha)
    mean = eng.predict_functionals(bare, Xg, w, score=FUNCTIONAL_MEAN, want_var=False, want_prob=False, want_score=True)
    assert mean["var"] is None and mean["prob"] is None
    assert np.array_equal(host(mean["mu"])[~bad], host(clean["mu"])[~bad]) and np.all(np.isnan(host(mean["mu"])[bad]))
    assert mean["best_idx"] == int(np.nanargmax(host(mean["score"])))


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_context_usable(eng):
    from ppbo_amd.engine import FUNCTIONAL_MEAN, FUNCTIONAL_PROB, _ptr
    mod = _fitted("SE_kernel", 6, None)
    post = mod["post"]
    rng = np.random.default_rng(11)
    M, G = 100, 4
    Xg, w = _groups(rng, mod, M, G), rng.standard_normal((M, G))
    before = eng.predict_functionals(post, Xg, w)
    dx, dw = eng.dev(Xg), eng.dev(w)
    mu = eng.dev(np.full(M, -7.0))                      # the sentinel a refused call must leave alone
    md, md32, bare = eng._model(post, True), eng._model(post, True, kstar_fp32=True), eng._model(post, False)

    def call(model, x, wt, ws, M_, G_, thr, kind):
        rc = eng.lib.ppbo_predict_functionals(eng.ctx, C.byref(model) if model is not None else None, _ptr(x), _ptr(wt), ws,
                                              M_, G_, thr, kind, _ptr(mu), None, None, None, None, None, eng._stream())
        return rc, eng._err()

    P = FUNCTIONAL_PROB
    for args in ((None, dx, dw, G, M, G, 0.0, P), (md, None, dw, G, M, G, 0.0, P), (md, dx, None, G, M, G, 0.0, P),
                 (md, dx, dw, G, 0, G, 0.0, P), (md, dx, dw, G, -5, G, 0.0, P), (md, dx, dw, G, 2 ** 31, G, 0.0, P),
                 (md, dx, dw, G, M, G, 0.0, 3), (md, dx, dw, G, M, G, 0.0, -1), (md32, dx, dw, G, M, G, 0.0, P),
                 (bare, dx, dw, G, M, G, 0.0, P),
                 (md, dx, dw, 0, M, 0, 0.0, P), (md, dx, dw, 65, M, 65, 0.0, P), (md, dx, dw, -1, M, -1, 0.0, P),
                 (md, dx, dw, 1, M, G, 0.0, P), (md, dx, dw, G + 1, M, G, 0.0, P), (md, dx, dw, -G, M, G, 0.0, P),
                 (md, dx, dw, G, M, G, float("nan"), P), (md, dx, dw, G, M, G, float("inf"), P),
                 (md, dx, dw, G, M, G, float("-inf"), P)):
        rc, msg = call(*args)
        assert rc < 0 and msg.startswith("invalid argument"), (args[3:], rc, msg)
    assert np.all(host(mu) == -7.0)                     # nothing was launched
    assert call(bare, dx, dw, G, M, G, 0.0, FUNCTIONAL_MEAN)[0] == 0          # the mean alone: no operator needed
    assert np.array_equal(host(mu), host(before["mu"]))
    after = eng.predict_functionals(post, Xg, w)
    for k in ("mu", "var", "prob"):
        assert np.array_equal(host(before[k]), host(after[k]))
    with pytest.raises(ValueError, match="predict_functionals"):
        eng.predict_functionals(post, Xg, w[:50])
    with pytest.raises(ValueError, match="predict_functionals"):
        eng.predict_functionals(post, rng.random((3, 65, 6)), np.ones(65))
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = None
    with pytest.raises(RuntimeError, match="posterior covariance unavailable"):
        gp.functional_pred(Xg[0], w[0])


# ---------------------------------------------------------------- 7. the drop-in surface
@functools.lru_cache(maxsize=None)
def _camel_gp():
    """BASELINE config 1, the loop of test_gpu_pairs.py (D = 2, 4 corner queries + 21 PCD queries, m = 25)."""
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
    return run_ppbo_loop(line_search_user(_six_hump, lo, hi), xis, xs, 21, st)[3]


def test_layers_on_the_six_hump_camel_loop():
    gp = _camel_gp()
    xstar = np.asarray(gp.xstar, dtype=float)
    far = np.where(xstar < 0.5, 1.0, 0.0)
    # contrast_pred of singletons is preference_pred's mu_d and var_d (another kernel: the parity bound)
    mu_d, var_d, _ = gp.preference_pred(xstar, far)
    mu_c, var_c, p_c = gp.contrast_pred(xstar, far)
    sf2 = float(gp.theta[2]) ** 2
    print(f"six-hump camel: contrast_pred against preference_pred: mu {abs(mu_c[0] - mu_d[0]) / abs(mu_d[0]):.2e}, "
          f"var {abs(var_c[0] - var_d[0]) / (4 * sf2):.2e}; P(x* better than the far corner) = {p_c[0]:.4f}")
    assert mu_c.shape == var_c.shape == p_c.shape == (1,)
    assert abs(mu_c[0] - mu_d[0]) <= TOL * abs(mu_d[0]) and abs(var_c[0] - var_d[0]) <= TOL * 4 * sf2
    assert p_c[0] > 0.5
    # shortlists: the neighbours of x* against the neighbours of the far corner
    rng = np.random.default_rng(0)
    A = np.clip(xstar + 0.02 * rng.standard_normal((5, 2)), 0.0, 1.0)
    B = np.clip(far + 0.02 * rng.standard_normal((7, 2)), 0.0, 1.0)
    mu_s, var_s, p_s = gp.contrast_pred(A, B)
    mu_pts = np.array([gp.mu_pred(x) for x in np.concatenate([A, B])]).reshape(-1)
    assert abs(mu_s[0] - (mu_pts[:5].mean() - mu_pts[5:].mean())) <= TOL * np.abs(mu_pts).max()
    assert var_s[0] >= 0.0 and p_s[0] > 0.5
    with pytest.raises(ValueError, match="contrast_pred"):
        gp.contrast_pred(rng.random((40, 2)), rng.random((25, 2)))
    # average_pred: zero offsets are the point itself; a cloud is the mean of its points; clipped to the box
    pts = rng.random((9, 2))
    mu0, var0 = gp.average_pred(pts, np.zeros((1, 2)))
    one = gp.eng.predict(gp._post, pts, want_best=False)
    assert np.abs(mu0 - host(one["mu"])).max() <= TOL * np.abs(host(one["mu"])).max()
    assert np.abs(var0 - host(one["var"])).max() <= TOL * sf2
    off = 0.05 * rng.standard_normal((6, 2))
    mu_a, var_a = gp.average_pred(pts, off)
    cloud = np.clip(pts[:, None, :] + off[None, :, :], 0.0, 1.0)
    mu_cl = host(gp.eng.predict(gp._post, cloud.reshape(-1, 2), want_var=False, want_best=False)["mu"]).reshape(9, 6)
    assert np.abs(mu_a - mu_cl.mean(axis=1)).max() <= TOL * np.abs(mu_cl).max()
    assert np.all(var_a >= 0.0) and np.all(var_a <= sf2 * (1 + 1e-9))
    # robust_xstar with zero offsets is the pool's mean argmax
    x0, m0, v0 = gp.robust_xstar(np.zeros((1, 2)))
    cand = host(gp._candidate_pool())
    if gp.xstars_local is not None and len(gp.xstars_local):
        cand = np.concatenate([cand, np.atleast_2d(gp.xstars_local)])
    sc = gp.eng.predict(gp._post, cand, want_var=False)
    assert np.any(np.all(cand == x0, axis=1))
    assert abs(m0 - sc["best_val"]) <= TOL * abs(sc["best_val"]) and 0.0 <= v0 <= sf2 * (1 + 1e-9)
    # with offsets: the returned row is a candidate, its values are average_pred's there, and no other candidate (a
    # sample of them through average_pred) has a larger averaged mean
    xr, mr, vr = gp.robust_xstar(off)
    assert xr.shape == (2,) and np.any(np.all(cand == xr, axis=1))
    mu_r, var_r = gp.average_pred(xr, off)          # (another call size: other row splits, so not bitwise)
    assert abs(mu_r[0] - mr) <= TOL * abs(mr) and abs(var_r[0] - vr) <= TOL * sf2
    mu_some, _ = gp.average_pred(cand[::257], off)
    assert mu_some.max() <= mr + TOL * abs(mr)
