"""GPU: slopes -- ppbo_predict_slopes / Engine.predict_slopes / GPModel.slope_pred / GPModel.sensitivity against the NumPy
statement (tests/slopes_numpy.py: analytic kernel derivatives on direct differences, the oracle's dense variance
operator; itself checked by central differences in tests/test_slopes_host.py), against ppbo_mean_grad, the exact
identities of the construction, the NaN rules, the argmax and the refusals.

Bound (TOL = 1e-6, the package's parity standard), per row: |mu_s - ref| against sum_j |g_j alpha_j| (the mean is a sum
that cancels down from it), |var_s - ref| against the prior term (the variance is a difference that cancels down from
it).  p is held to the device's own (mu_s, var_s) at 4 eps; its distance from the reference's p is printed.

Measured on MI355X (the worst row over all cases; profiles/r17_slopes.txt has them case by case): mean 1.1e-9 (camphor on
cam_small; the radial kernels 3.6e-10), variance 9.6e-10, |p - ref| 8.4e-11; mu_s against xi . grad mu of ppbo_mean_grad
2.1e-14 (camphor; the radial kernels and ARD 6.8e-16)."""
import ctypes as C
import functools

import numpy as np
import pytest

import slopes_numpy as sn
from conftest import load_golden
from test_gpu_pathwise import _star_design

pytestmark = pytest.mark.gpu

RADIAL = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")
TOL = 1e-6                # the package's parity tolerance (README, "Parity")
EPS = np.finfo(float).eps
SPREAD = np.array([0.4, 0.6, 0.5, 1.0, 0.8, 0.7])


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def host(t):
    return t.detach().cpu().numpy()


def _forms():
    from ppbo_amd.engine import FORM_EDGE, FORM_NODE
    return {"node": FORM_NODE, "edge": FORM_EDGE}


@functools.lru_cache(maxsize=None)
def _fitted(kernel, D, n_q, m, form, ard=False):
    """One fitted star-design model per shape, shared by the tests: dict(post, X, th, m, kernel, alpha, A) with (alpha, A)
    the host's own (slopes_numpy.operator_from_fit on the device's f_MAP; nothing else of the device enters)."""
    from ppbo_amd.engine import get_engine
    eng = get_engine(0)
    rng = np.random.default_rng(1000 * D + 10 * n_q + m + 7 * RADIAL.index(kernel))
    X = _star_design(rng, n_q, D, m)
    th = [0.05, rng.uniform(0.25, 0.6, D) * np.sqrt(D / 6.0) if ard else 0.3 * np.sqrt(D / 6.0), 0.7]
    r = eng.gp_fit(X, th, kernel, m, rng.standard_normal(X.shape[0]), gtol=1e-6, start_is_whitened=True, form=_forms()[form])
    assert r["post"] is not None
    alpha, A = sn.operator_from_fit(X, th, kernel, m, host(r["fMAP"]))
    return dict(post=r["post"], X=X, th=th, m=m, kernel=kernel, alpha=alpha, A=A)


@functools.lru_cache(maxsize=None)
def _fitted_camphor(form):
    from ppbo_amd.engine import get_engine
    eng = get_engine(0)
    g = load_golden("cam_small")
    X, th, kernel, m = g["X"], [float(v) for v in g["theta"]], str(g["kernel"]), int(g["m"])
    r = eng.gp_fit(X, th, kernel, m, g["f_init"], gtol=1e-6, form=_forms()[form])
    assert r["post"] is not None
    alpha, A = sn.operator_from_fit(X, th, kernel, m, host(r["fMAP"]))
    return dict(post=r["post"], X=X, th=th, m=m, kernel=kernel, alpha=alpha, A=A)


@functools.lru_cache(maxsize=None)
def _fitted_camphor_ard():
    from ppbo_amd.engine import get_engine
    eng = get_engine(0)
    rng = np.random.default_rng(6)
    X, m = rng.random((64, 6)), 3
    th = [0.3, SPREAD, 1.2]
    r = eng.gp_fit(X, th, sn.CAMPHOR_ARD, m, rng.standard_normal(64), gtol=1e-6, start_is_whitened=True)
    assert r["post"] is not None
    alpha, A = sn.operator_from_fit(X, th, sn.CAMPHOR_ARD, m, host(r["fMAP"]))
    return dict(post=r["post"], X=X, th=th, m=m, kernel=sn.CAMPHOR_ARD, alpha=alpha, A=A)


def _rows(rng, mod, M):
    """M (point, direction) rows: uniform points, the first few ON design rows (g_j = 0 there); directions of every
    length from 1e-3 to 30."""
    N, D = mod["X"].shape
    X, Xi = rng.random((M, D)), rng.standard_normal((M, D))
    k = min(16, (M + 3) // 4)
    X[:k] = mod["X"][rng.integers(0, N, k)]
    Xi *= 10.0 ** rng.uniform(-3.0, 1.5, (M, 1))
    return X, Xi


def _errors(mod, X, Xi, mu, var, p):
    """The three error measures of the module docstring for device results (mu, var, p) on the rows (X, Xi)."""
    mu0, var0, g = sn.slope_reference(X, Xi, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"])
    e_mu = np.max(np.abs(mu - mu0) / (np.abs(g) @ np.abs(mod["alpha"])))
    e_var = np.max(np.abs(var - var0) / sn.slope_prior(Xi, mod["th"], mod["kernel"]))
    e_p = np.abs(p - sn.slope_probability(mu0, var0)).max()
    return e_mu, e_var, e_p


def _parity(eng, mod, M=257, seed=3, label=""):
    X, Xi = _rows(np.random.default_rng(seed), mod, M)
    out = eng.predict_slopes(mod["post"], X, Xi)
    mu, var, p = host(out["mu"]), host(out["var"]), host(out["prob"])
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var)) and np.all(np.isfinite(p))
    e_mu, e_var, e_p = _errors(mod, X, Xi, mu, var, p)
    print(f"slopes parity {label} M={M}: |mu_s - ref| / sum|g alpha| = {e_mu:.2e}, |var_s - ref| / prior = {e_var:.2e}, "
          f"|p - ref| = {e_p:.2e}")
    assert e_mu <= TOL and e_var <= TOL
    assert np.abs(p - sn.slope_probability(mu, var)).max() <= 4 * EPS
    assert out["best_idx"] == int(np.argmax(p)) and out["best_val"] == p.max()
    return X, Xi, out


# ---------------------------------------------------------------- 1. parity with the NumPy statement
# (D, n_q, m): N = 32 (m = 3) in the buckets 6 and 48, N = 78 (m = 25, off every tile edge) in the bucket 20
SHAPES = [(6, 8, 3), (20, 3, 25), (40, 8, 3)]


@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("D,n_q,m", SHAPES)
@pytest.mark.parametrize("kernel", RADIAL)
def test_parity_radial(eng, kernel, D, n_q, m, form):
    _parity(eng, _fitted(kernel, D, n_q, m, form), label=f"{kernel} D={D} N={n_q * (m + 1)} {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("D,n_q,m", [(3, 8, 3), (50, 3, 25)])
def test_parity_smallest_and_largest_bucket(eng, D, n_q, m, form):
    """DP = 4 and DP = 64 (two 64-vectors per lane: the register-heaviest instance)."""
    _parity(eng, _fitted("Matern52_kernel", D, n_q, m, form), label=f"Matern52 D={D} N={n_q * (m + 1)} {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("n_q,m", [(3, 40), (200, 3)])
def test_parity_row_splits(eng, n_q, m, form):
    """More than one row split in the K* launch: stars of 41 rows (a split = one star, staged in two steps of KS_RJ = 32
    rows), and N = 800 in 50 splits of four stars."""
    _parity(eng, _fitted("RQ_kernel", 6, n_q, m, form), label=f"RQ D=6 N={n_q * (m + 1)} {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_ard(eng, form):
    _parity(eng, _fitted("Matern52_kernel", 6, 3, 25, form, ard=True), label=f"Matern52 ARD D=6 N=78 {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_camphor(eng, form):
    _parity(eng, _fitted_camphor(form), label=f"camphor cam_small {form}")


def _stub_gp(eng, mod, xstar=None):
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp.eng, gp._post, gp.xstar = eng, mod["post"], xstar
    return gp


def test_parity_camphor_ard_through_slope_pred(eng):
    """SE on the 11 embedded columns with x~ = e(x), xi~ = J_e(x) xi, against the six-coordinate statement."""
    mod = _fitted_camphor_ard()
    X, Xi = _rows(np.random.default_rng(4), mod, 257)
    mu, var, p = _stub_gp(eng, mod).slope_pred(X, Xi)
    e_mu, e_var, e_p = _errors(mod, X, Xi, mu, var, p)
    print(f"slopes parity camphor ARD (slope_pred) M=257: |mu_s - ref| / sum|g alpha| = {e_mu:.2e}, "
          f"|var_s - ref| / prior = {e_var:.2e}, |p - ref| = {e_p:.2e}")
    assert e_mu <= TOL and e_var <= TOL
    import torch
    dmu, dvar, dp = _stub_gp(eng, mod).slope_pred(torch.as_tensor(X[:5], device=eng.device), torch.as_tensor(Xi[:5], device=eng.device))
    assert np.array_equal(dmu, mu[:5]) and np.array_equal(dvar, var[:5]) and np.array_equal(dp, p[:5])
    one = _stub_gp(eng, mod).slope_pred(X[7], Xi[7])
    assert all(v.shape == (1,) for v in one) and (one[0][0], one[1][0], one[2][0]) == (mu[7], var[7], p[7])


@pytest.mark.parametrize("form", ["node", "edge"])
def test_workgroup_edges_and_batch_independence(eng, form):
    """M = 1, 255, 256, 257 (the edges of the KS_THREADS workgroup): parity, and the same rows inside a larger batch are
    bitwise what they are in a smaller one."""
    mod = _fitted("RQ_kernel", 6, 3, 25, form)
    X, Xi, big = _parity(eng, mod, M=257, label=f"RQ D=6 N=78 {form}")
    for M in (1, 255, 256):
        out = eng.predict_slopes(mod["post"], X[:M], Xi[:M])
        mu, var, p = host(out["mu"]), host(out["var"]), host(out["prob"])
        e_mu, e_var, _ = _errors(mod, X[:M], Xi[:M], mu, var, p)
        assert e_mu <= TOL and e_var <= TOL
        for k, v in (("mu", mu), ("var", var), ("prob", p)):
            assert np.array_equal(v, host(big[k])[:M])
        assert out["best_idx"] == int(np.argmax(p)) and out["best_val"] == p.max()


def test_chunk_boundary(eng):
    """65537 rows at N = 32: the second chunk holds one row."""
    mod = _fitted("SE_kernel", 6, 8, 3, "node")
    M = 65537
    X, Xi = _rows(np.random.default_rng(9), mod, M)
    out = eng.predict_slopes(mod["post"], X, Xi, want_score=True)
    mu, var, p = host(out["mu"]), host(out["var"]), host(out["prob"])
    e_mu, e_var, e_p = _errors(mod, X, Xi, mu, var, p)
    print(f"slopes parity SE D=6 N=32 node M={M}: |mu_s - ref| / sum|g alpha| = {e_mu:.2e}, |var_s - ref| / prior = {e_var:.2e}, "
          f"|p - ref| = {e_p:.2e}")
    assert e_mu <= TOL and e_var <= TOL
    assert np.array_equal(host(out["score"]), p)
    assert out["best_idx"] == int(np.argmax(p)) and out["best_val"] == p.max()
    last = eng.predict_slopes(mod["post"], X[-1:], Xi[-1:])
    head = eng.predict_slopes(mod["post"], X[:300], Xi[:300])
    for k, v in (("mu", mu), ("var", var), ("prob", p)):
        assert host(last[k])[0] == v[-1] and np.array_equal(host(head[k]), v[:300])
    # the winner moved into the second chunk: the index that comes back is the global row
    i = int(np.argmax(p))
    X[[i, M - 1]], Xi[[i, M - 1]] = X[[M - 1, i]], Xi[[M - 1, i]]
    moved = eng.predict_slopes(mod["post"], X, Xi, want_mu=False, want_var=False, want_prob=False)
    assert moved["best_val"] == p[i]
    assert moved["best_idx"] == (M - 1 if np.count_nonzero(p == p[i]) == 1 else min(M - 1, int(np.flatnonzero(p == p[i])[0])))


# ---------------------------------------------------------------- 2. the mean against ppbo_mean_grad
@pytest.mark.parametrize("which", ["SE", "RQ", "Matern52", "Matern32", "ard", "camphor", "camphor_ard"])
def test_mean_against_mean_grad(eng, which):
    """mu_s = xi . grad mu with the gradient of existing device code, on the same rows, under the parity bound."""
    if which == "camphor":
        mod = _fitted_camphor("node")
    elif which == "camphor_ard":
        mod = _fitted_camphor_ard()
    elif which == "ard":
        mod = _fitted("Matern52_kernel", 6, 3, 25, "node", ard=True)
    else:
        mod = _fitted(which + "_kernel", 20, 3, 25, "node")
    X, Xi = _rows(np.random.default_rng(13), mod, 257)
    mu = host(eng.predict_slopes(mod["post"], X, Xi, want_var=False, want_prob=False, score=0)["mu"])
    _, grad = eng.mean_grad(mod["post"], X)
    want = np.einsum("ij,ij->i", host(grad), Xi)
    g = sn.slope_column(X, Xi, mod["X"], mod["th"], mod["kernel"])
    e = np.max(np.abs(mu - want) / (np.abs(g) @ np.abs(mod["alpha"])))
    print(f"slopes against mean_grad {which}: |mu_s - xi.grad mu| / sum|g alpha| = {e:.2e}")
    assert e <= TOL


# ---------------------------------------------------------------- 3. exact identities
def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("which", ["SE-node", "RQ-edge", "Matern52-node", "Matern32-edge", "camphor-node", "camphor-edge", "camphor_ard"])
def test_exact_identities(eng, which):
    if which.startswith("camphor_ard"):
        mod = _fitted_camphor_ard()
    elif which.startswith("camphor"):
        mod = _fitted_camphor(which.split("-")[1])
    else:
        k, form = which.split("-")
        mod = _fitted(k + "_kernel", {"SE": 6, "RQ": 20, "Matern52": 40, "Matern32": 6}[k], *{"SE": (8, 3), "RQ": (3, 25), "Matern52": (8, 3), "Matern32": (8, 3)}[k], form)
    X, Xi = _rows(np.random.default_rng(5), mod, 777)
    post = mod["post"]
    # xi = 0: (0, 0, 1/2) exactly; all tied: the first index
    zero = eng.predict_slopes(post, X, np.zeros_like(Xi))
    assert np.all(host(zero["mu"]) == 0.0) and np.all(host(zero["var"]) == 0.0) and np.all(host(zero["prob"]) == 0.5)
    assert zero["best_idx"] == 0 and zero["best_val"] == 0.5
    # -xi: -mu_s bit for bit, var_s bitwise, p(-xi) + p(xi) = 1 to 1 ulp
    fw, bw = eng.predict_slopes(post, X, Xi), eng.predict_slopes(post, X, -Xi)
    assert np.array_equal(_bits(host(fw["mu"])), _bits(-host(bw["mu"])))
    assert np.array_equal(_bits(host(fw["var"])), _bits(host(bw["var"])))
    assert np.abs(host(fw["prob"]) + host(bw["prob"]) - 1.0).max() <= EPS
    # x on a design row: finite (and within the parity bound: _rows puts design rows first, see _parity)
    on = np.all(X[:16, None, :] == mod["X"][None, :, :], axis=2).any(axis=1)
    assert on.all() and np.all(np.isfinite(host(fw["mu"])[:16])) and np.all(host(fw["var"])[:16] > 0.0)
    # a repeated call is bitwise equal
    again = eng.predict_slopes(post, X, Xi)
    for k in ("mu", "var", "prob"):
        assert np.array_equal(_bits(host(fw[k])), _bits(host(again[k])))
    assert (fw["best_idx"], fw["best_val"]) == (again["best_idx"], again["best_val"])


# ---------------------------------------------------------------- 4. NaN rules, score kinds, the argmax
@pytest.mark.parametrize("form", ["node", "edge"])
def test_nan_rows_score_kinds_and_argmax(eng, form):
    from ppbo_amd.engine import SLOPE_MEAN, SLOPE_PROB, SLOPE_VARIANCE
    mod = _fitted("Matern52_kernel", 6, 8, 3, form)
    post = mod["post"]
    X, Xi = _rows(np.random.default_rng(10), mod, 601)
    X[400], Xi[400] = X[200], Xi[200]              # duplicate rows: a tie goes to the first
    clean = eng.predict_slopes(post, X, Xi)
    assert all(host(clean[k])[400] == host(clean[k])[200] for k in ("mu", "var", "prob"))
    X[3, 2], Xi[10, 0], X[599, 5], Xi[300, 1] = np.nan, np.nan, np.inf, -np.inf
    bad = np.zeros(601, dtype=bool)
    bad[[3, 10, 599, 300]] = True
    for kind, key in ((SLOPE_MEAN, "mu"), (SLOPE_VARIANCE, "var"), (SLOPE_PROB, "prob")):
        out = eng.predict_slopes(post, X, Xi, score=kind, want_score=True)
        sc = host(out["score"])
        assert np.array_equal(sc, host(out[key]), equal_nan=True)
        for k in ("mu", "var", "prob"):
            v = host(out[k])
            assert np.all(np.isnan(v[bad])) and np.array_equal(_bits(v[~bad]), _bits(host(clean[k])[~bad]))
        assert out["best_idx"] == int(np.nanargmax(sc)) and out["best_val"] == np.nanmax(sc)
        assert not bad[out["best_idx"]]
    # the tie of the duplicates, made the winner: the first of them comes back
    Xw, Xiw = X[[5, 200, 7, 400]], Xi[[5, 200, 7, 400]] * np.array([[0.0], [1.0], [0.0], [1.0]])
    tie = eng.predict_slopes(post, Xw, Xiw, score=SLOPE_VARIANCE)
    assert tie["best_idx"] == 1 and host(tie["var"])[1] == host(tie["var"])[3]
    # nothing but NaN rows: (NaN, -1)
    none = eng.predict_slopes(post, X[[3, 10, 599]], Xi[[3, 10, 599]])
    assert none["best_idx"] == -1 and np.isnan(none["best_val"])
    # the mean alone needs no operator: a model without G, bit for bit the mean of the full call
    bare = eng.mean_posterior(mod["X"], mod["th"], mod["kernel"], mod["m"], post.alpha)
    mean = eng.predict_slopes(bare, X, Xi, score=SLOPE_MEAN, want_var=False, want_prob=False, want_score=True)
    assert mean["var"] is None and mean["prob"] is None
    assert np.array_equal(host(mean["mu"])[~bad], host(clean["mu"])[~bad]) and np.all(np.isnan(host(mean["mu"])[bad]))
    assert mean["best_idx"] == int(np.nanargmax(host(mean["score"])))


# ---------------------------------------------------------------- 5. sensitivity
@pytest.mark.parametrize("which", ["radial", "camphor_ard"])
def test_sensitivity_is_D_unit_slopes(eng, which):
    mod = _fitted_camphor_ard() if which == "camphor_ard" else _fitted("SE_kernel", 6, 8, 3, "node")
    D = mod["X"].shape[1]
    xstar = np.random.default_rng(2).random(D)
    gp = _stub_gp(eng, mod, xstar)
    mu, var, p = gp.sensitivity()
    assert mu.shape == var.shape == p.shape == (D,)
    for d in range(D):
        one = gp.slope_pred(xstar, np.eye(D)[d])
        assert (one[0][0], one[1][0], one[2][0]) == (mu[d], var[d], p[d])
    other = np.random.default_rng(3).random(D)
    assert np.array_equal(gp.sensitivity(other)[0], gp.slope_pred(np.tile(other, (D, 1)), np.eye(D))[0])
    # the coordinate slopes are the posterior mean's gradient
    _, grad = eng.mean_grad(mod["post"], xstar[None, :])
    g = sn.slope_column(np.tile(xstar, (D, 1)), np.eye(D), mod["X"], mod["th"], mod["kernel"])
    assert np.max(np.abs(mu - host(grad)[0]) / (np.abs(g) @ np.abs(mod["alpha"]))) <= TOL


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_context_usable(eng):
    from ppbo_amd.engine import SLOPE_MEAN, SLOPE_PROB, SLOPE_VARIANCE, _ptr
    mod = _fitted("SE_kernel", 6, 8, 3, "node")
    post = mod["post"]
    X, Xi = _rows(np.random.default_rng(11), mod, 100)
    before = eng.predict_slopes(post, X, Xi)
    dx, dxi, mu, var = eng.dev(X), eng.dev(Xi), eng.empty(100), eng.empty(100)
    md, md32, bare = eng._model(post, True), eng._model(post, True, kstar_fp32=True), eng._model(post, False)
    nolam = eng._model(post, True)
    nolam.d_lam_diag = 0

    def call(model, a, b, M, kind, d_var=None, d_prob=None):
        rc = eng.lib.ppbo_predict_slopes(eng.ctx, C.byref(model) if model is not None else None, _ptr(a), _ptr(b), M, kind,
                                         _ptr(mu), _ptr(d_var), _ptr(d_prob), None, None, None, eng._stream())
        return rc, eng._err()

    for args in ((None, dx, dxi, 100, SLOPE_PROB), (md, None, dxi, 100, SLOPE_PROB), (md, dx, None, 100, SLOPE_PROB),
                 (md, dx, dxi, 0, SLOPE_PROB), (md, dx, dxi, -5, SLOPE_PROB), (md, dx, dxi, 2 ** 31, SLOPE_PROB),
                 (md, dx, dxi, 100, 3), (md, dx, dxi, 100, -1), (md32, dx, dxi, 100, SLOPE_PROB),
                 (bare, dx, dxi, 100, SLOPE_PROB), (bare, dx, dxi, 100, SLOPE_VARIANCE), (bare, dx, dxi, 100, SLOPE_MEAN, var),
                 (bare, dx, dxi, 100, SLOPE_MEAN, None, var), (nolam, dx, dxi, 100, SLOPE_PROB)):
        rc, msg = call(*args)
        assert rc != 0 and "invalid argument" in msg, (args[3:5], rc, msg)
    assert call(bare, dx, dxi, 100, SLOPE_MEAN)[0] == 0          # the mean alone: no operator needed
    assert call(md, dx, dxi, 100, SLOPE_PROB)[0] == 0
    after = eng.predict_slopes(post, X, Xi)
    for k in ("mu", "var", "prob"):
        assert np.array_equal(host(before[k]), host(after[k]))
    with pytest.raises(ValueError, match="predict_slopes"):
        eng.predict_slopes(post, X, Xi[:50])
    with pytest.raises(ValueError, match="predict_slopes"):
        eng.predict_slopes(post, X[:, :5], Xi[:, :5])
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = None
    with pytest.raises(RuntimeError, match="posterior covariance unavailable"):
        gp.slope_pred(X[0], Xi[0])
