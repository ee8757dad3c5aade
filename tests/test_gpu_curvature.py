"""GPU: curvatures -- ppbo_predict_curvatures / Engine.predict_curvatures / GPModel.curvature_pred / sharpness /
mean_hessian against the NumPy statement (tests/curvature_numpy.py: analytic second derivatives on direct differences,
the oracle's dense variance operator; itself checked by central differences in tests/test_curvature_host.py), the exact
identities of the construction, the NaN rules, the argmax and the refusals.  The fits are the cached small ones of
tests/test_gpu_slopes.py.

Bound (TOL = 1e-6, the package's parity standard), per row: |mu_c - ref| against sum_j |c_j alpha_j| (the mean is a sum
that cancels down from it), |var_c - ref| against the prior term (the variance is a difference that cancels down from
it).  p is held to the device's own (mu_c, var_c) at 4 eps; its distance from the reference's p is printed.

Measured on MI355X (the worst row over all cases; profiles/r18_curvature.txt has them case by case): mean 1.2e-9 (camphor
on cam_small; the radial kernels 6.0e-10), variance 1.6e-9 (Matern-5/2, D = 20, N = 78), |p - ref| 9.1e-11; with
accelerations (SE, D = 11) 1.9e-13 / 6.7e-13; the camphor-ARD model through d_Xa 4.1e-15 / 1.4e-15; xi' H xi of
mean_hessian against mu_c 5.5e-15 (camphor; radial and ARD <= 5.9e-16)."""
import ctypes as C

import numpy as np
import pytest

import curvature_numpy as cn
from test_gpu_slopes import _fitted, _fitted_camphor, _fitted_camphor_ard, _rows, _stub_gp, host

pytestmark = pytest.mark.gpu

RADIAL = ("SE_kernel", "RQ_kernel", "Matern52_kernel")
TOL = 1e-6                # the package's parity tolerance (README, "Parity")
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _errors(mod, X, Xi, mu, var, p, Xa=None):
    """The three error measures of the module docstring for device results (mu, var, p) on the rows (X, Xi[, Xa])."""
    mu0, var0, c = cn.curvature_reference(X, Xi, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"], Xa)
    e_mu = np.max(np.abs(mu - mu0) / (np.abs(c) @ np.abs(mod["alpha"])))
    e_var = np.max(np.abs(var - var0) / cn.curvature_prior(Xi, mod["th"], mod["kernel"], Xa))
    e_p = np.abs(p - cn.curvature_probability(mu0, var0)).max()
    return e_mu, e_var, e_p


def _parity(eng, mod, M=257, seed=3, label=""):
    X, Xi = _rows(np.random.default_rng(seed), mod, M)
    out = eng.predict_curvatures(mod["post"], X, Xi)
    mu, var, p = host(out["mu"]), host(out["var"]), host(out["prob"])
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var)) and np.all(np.isfinite(p))
    e_mu, e_var, e_p = _errors(mod, X, Xi, mu, var, p)
    print(f"curvature parity {label} M={M}: |mu_c - ref| / sum|c alpha| = {e_mu:.2e}, |var_c - ref| / prior = {e_var:.2e}, "
          f"|p - ref| = {e_p:.2e}")
    assert e_mu <= TOL and e_var <= TOL
    assert np.abs(p - cn.curvature_probability(mu, var)).max() <= 4 * EPS
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
    """More than one row split in the K* launch: stars of 41 rows (staged in two steps of KS_RJ = 32 rows), and N = 800 in
    50 splits of four stars."""
    _parity(eng, _fitted("RQ_kernel", 6, n_q, m, form), label=f"RQ D=6 N={n_q * (m + 1)} {form}")


# ---------------------------------------------------------------- 2. the coordinate maps
@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_ard(eng, form):
    _parity(eng, _fitted("Matern52_kernel", 6, 3, 25, form, ard=True), label=f"Matern52 ARD D=6 N=78 {form}")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_camphor(eng, form):
    _parity(eng, _fitted_camphor(form), label=f"camphor cam_small {form}")


def test_parity_camphor_ard_through_curvature_pred(eng):
    """SE on the 11 embedded columns with x~ = e(x), xi~ = J_e(x) xi and the acceleration e'', against the six-coordinate
    statement, which does not know the embedding: the test of d_Xa."""
    mod = _fitted_camphor_ard()
    X, Xi = _rows(np.random.default_rng(4), mod, 257)
    mu, var, p = _stub_gp(eng, mod).curvature_pred(X, Xi)
    e_mu, e_var, e_p = _errors(mod, X, Xi, mu, var, p)
    print(f"curvature parity camphor ARD (curvature_pred) M=257: |mu_c - ref| / sum|c alpha| = {e_mu:.2e}, "
          f"|var_c - ref| / prior = {e_var:.2e}, |p - ref| = {e_p:.2e}")
    assert e_mu <= TOL and e_var <= TOL
    assert np.abs(p - cn.curvature_probability(mu, var)).max() <= 4 * EPS
    import torch
    dmu, dvar, dp = _stub_gp(eng, mod).curvature_pred(torch.as_tensor(X[:5], device=eng.device), torch.as_tensor(Xi[:5], device=eng.device))
    assert np.array_equal(dmu, mu[:5]) and np.array_equal(dvar, var[:5]) and np.array_equal(dp, p[:5])
    one = _stub_gp(eng, mod).curvature_pred(X[7], Xi[7])
    assert all(v.shape == (1,) for v in one) and (one[0][0], one[1][0], one[2][0]) == (mu[7], var[7], p[7])


# ---------------------------------------------------------------- 3. the acceleration at the C level
def _c_call(eng, model, X, Xi, Xa, M, kind, mu=None, var=None, prob=None):
    from ppbo_amd.engine import _ptr
    rc = eng.lib.ppbo_predict_curvatures(eng.ctx, C.byref(model) if model is not None else None, _ptr(X), _ptr(Xi), _ptr(Xa),
                                         M, kind, _ptr(mu), _ptr(var), _ptr(prob), None, None, None, eng._stream())
    return rc, eng._err()


@pytest.mark.parametrize("form", ["node", "edge"])
def test_acceleration_on_an_se_model(eng, form):
    """D = 11 (the bucket 12, the embedding's): random accelerations against the curved-path statement; a non-finite
    acceleration makes its own row NaN and no other; D = 17 with d_Xa is refused."""
    from ppbo_amd.engine import CURV_PROB
    mod = _fitted("SE_kernel", 11, 8, 3, form)
    M = 257
    rng = np.random.default_rng(21)
    X, Xi = _rows(rng, mod, M)
    Xa = rng.standard_normal((M, 11)) * 10.0 ** rng.uniform(-2.0, 2.0, (M, 1))
    md = eng._model(mod["post"], True)
    mu, var, p = eng.empty(M), eng.empty(M), eng.empty(M)
    rc, msg = _c_call(eng, md, eng.dev(X), eng.dev(Xi), eng.dev(Xa), M, CURV_PROB, mu, var, p)
    assert rc == 0, msg
    mu, var, p = host(mu), host(var), host(p)
    e_mu, e_var, e_p = _errors(mod, X, Xi, mu, var, p, Xa)
    print(f"curvature parity SE D=11 N=32 {form} with accelerations M={M}: |mu_c - ref| / sum|c alpha| = {e_mu:.2e}, "
          f"|var_c - ref| / prior = {e_var:.2e}, |p - ref| = {e_p:.2e}")
    assert e_mu <= TOL and e_var <= TOL
    assert np.abs(p - cn.curvature_probability(mu, var)).max() <= 4 * EPS
    # a zero acceleration is the straight line, bit for bit; the accelerations above are not
    straight = eng.predict_curvatures(mod["post"], X, Xi)
    z = [eng.empty(M) for _ in range(3)]
    assert _c_call(eng, md, eng.dev(X), eng.dev(Xi), eng.dev(np.zeros_like(Xa)), M, CURV_PROB, *z)[0] == 0
    for k, v in zip(("mu", "var", "prob"), z):
        assert np.array_equal(_bits(host(v)), _bits(host(straight[k])))
    assert not np.array_equal(mu, host(straight["mu"]))
    # NaN / inf in the acceleration
    Xb = Xa.copy()
    Xb[5, 3], Xb[200, 10] = np.nan, -np.inf
    b = [eng.empty(M) for _ in range(3)]
    assert _c_call(eng, md, eng.dev(X), eng.dev(Xi), eng.dev(Xb), M, CURV_PROB, *b)[0] == 0
    bad = np.zeros(M, dtype=bool)
    bad[[5, 200]] = True
    for v, clean in zip(b, (mu, var, p)):
        v = host(v)
        assert np.all(np.isnan(v[bad])) and np.array_equal(_bits(v[~bad]), _bits(clean[~bad]))
    # D = 17: no instance holds three vectors there
    big = _fitted("SE_kernel", 17, 8, 3, form)
    X17, Xi17 = _rows(rng, big, 10)
    md17 = eng._model(big["post"], True)
    o = [eng.empty(10) for _ in range(3)]
    rc, msg = _c_call(eng, md17, eng.dev(X17), eng.dev(Xi17), eng.dev(np.ones_like(X17)), 10, CURV_PROB, *o)
    assert rc != 0 and "invalid argument" in msg
    assert _c_call(eng, md17, eng.dev(X17), eng.dev(Xi17), None, 10, CURV_PROB, *o)[0] == 0
    e_mu, e_var, _ = _errors(big, X17, Xi17, *(host(v) for v in o))
    assert e_mu <= TOL and e_var <= TOL


# ---------------------------------------------------------------- 4. batch independence
@pytest.mark.parametrize("form", ["node", "edge"])
def test_workgroup_edges_and_batch_independence(eng, form):
    """M = 1, 255, 256, 257 (the edges of the KS_THREADS workgroup): parity, and the same rows inside a larger batch are
    bitwise what they are in a smaller one."""
    mod = _fitted("RQ_kernel", 6, 3, 25, form)
    X, Xi, big = _parity(eng, mod, M=257, label=f"RQ D=6 N=78 {form}")
    for M in (1, 255, 256):
        out = eng.predict_curvatures(mod["post"], X[:M], Xi[:M])
        mu, var, p = host(out["mu"]), host(out["var"]), host(out["prob"])
        e_mu, e_var, _ = _errors(mod, X[:M], Xi[:M], mu, var, p)
        assert e_mu <= TOL and e_var <= TOL
        for k, v in (("mu", mu), ("var", var), ("prob", p)):
            assert np.array_equal(_bits(v), _bits(host(big[k])[:M]))
        assert out["best_idx"] == int(np.argmax(p)) and out["best_val"] == p.max()


def test_chunk_boundary(eng):
    """65536 + 5 rows at N = 32: the rows on either side of the chunk boundary are bitwise the same rows predicted alone."""
    mod = _fitted("SE_kernel", 6, 8, 3, "node")
    M = 65536 + 5
    X, Xi = _rows(np.random.default_rng(9), mod, M)
    out = eng.predict_curvatures(mod["post"], X, Xi, want_score=True)
    mu, var, p = host(out["mu"]), host(out["var"]), host(out["prob"])
    sel = np.r_[0:300, 65536 - 40:M]
    e_mu, e_var, e_p = _errors(mod, X[sel], Xi[sel], mu[sel], var[sel], p[sel])
    print(f"curvature parity SE D=6 N=32 node M={M} (rows at the chunk boundary): |mu_c - ref| / sum|c alpha| = {e_mu:.2e}, "
          f"|var_c - ref| / prior = {e_var:.2e}, |p - ref| = {e_p:.2e}")
    assert e_mu <= TOL and e_var <= TOL
    assert np.array_equal(host(out["score"]), p)
    assert out["best_idx"] == int(np.argmax(p)) and out["best_val"] == p.max()
    for rows in (np.arange(65536 - 40, M), np.arange(65536, M), np.arange(300), np.array([M - 1])):
        alone = eng.predict_curvatures(mod["post"], X[rows], Xi[rows])
        for k, v in (("mu", mu), ("var", var), ("prob", p)):
            assert np.array_equal(_bits(host(alone[k])), _bits(v[rows]))
    # the winner moved into the second chunk: the index that comes back is the global row
    i = int(np.argmax(p))
    X[[i, M - 1]], Xi[[i, M - 1]] = X[[M - 1, i]], Xi[[M - 1, i]]
    moved = eng.predict_curvatures(mod["post"], X, Xi, want_mu=False, want_var=False, want_prob=False)
    assert moved["best_val"] == p[i]
    assert moved["best_idx"] == (M - 1 if np.count_nonzero(p == p[i]) == 1 else min(M - 1, int(np.flatnonzero(p == p[i])[0])))


# ---------------------------------------------------------------- 5. exact identities (d_Xa NULL)
def _identity_model(which):
    if which.startswith("camphor"):
        return _fitted_camphor(which.split("-")[1])
    k, form = which.split("-")
    return _fitted(k + "_kernel", {"SE": 6, "RQ": 20, "Matern52": 40}[k], *{"SE": (8, 3), "RQ": (3, 25), "Matern52": (8, 3)}[k], form)


@pytest.mark.parametrize("which", ["SE-node", "RQ-edge", "Matern52-node", "SE-edge", "camphor-node", "camphor-edge"])
def test_exact_identities(eng, which):
    mod = _identity_model(which)
    X, Xi = _rows(np.random.default_rng(5), mod, 777)
    post = mod["post"]
    # xi = 0: (0, 0, 1/2) exactly; all tied: the first index
    zero = eng.predict_curvatures(post, X, np.zeros_like(Xi))
    assert np.all(host(zero["mu"]) == 0.0) and np.all(host(zero["var"]) == 0.0) and np.all(host(zero["prob"]) == 0.5)
    assert zero["best_idx"] == 0 and zero["best_val"] == 0.5
    # -xi: all three bitwise unchanged
    fw, bw = eng.predict_curvatures(post, X, Xi), eng.predict_curvatures(post, X, -Xi)
    for k in ("mu", "var", "prob"):
        assert np.array_equal(_bits(host(fw[k])), _bits(host(bw[k])))
    # 2 xi: 4 mu_c and 16 var_c bit for bit (the radial kernels: every term is homogeneous in xi)
    if not which.startswith("camphor"):
        tw = eng.predict_curvatures(post, X, 2.0 * Xi)
        assert np.array_equal(_bits(host(tw["mu"])), _bits(4.0 * host(fw["mu"])))
        assert np.array_equal(_bits(host(tw["var"])), _bits(16.0 * host(fw["var"])))
    # x on a design row: finite (and within the parity bound: _rows puts design rows first, see _parity)
    on = np.all(X[:16, None, :] == mod["X"][None, :, :], axis=2).any(axis=1)
    assert on.all() and np.all(np.isfinite(host(fw["mu"])[:16])) and np.all(host(fw["var"])[:16] > 0.0)
    # a repeated call is bitwise equal
    again = eng.predict_curvatures(post, X, Xi)
    for k in ("mu", "var", "prob"):
        assert np.array_equal(_bits(host(fw[k])), _bits(host(again[k])))
    assert (fw["best_idx"], fw["best_val"]) == (again["best_idx"], again["best_val"])


@pytest.mark.parametrize("which", ["radial", "ard", "camphor", "camphor_ard"])
def test_mean_hessian(eng, which):
    """Symmetric, and xi' H xi is mu_c(xi) within TOL of sum |c_j alpha_j|; needs no variance operator."""
    mod = {"radial": lambda: _fitted("RQ_kernel", 6, 8, 3, "node"), "ard": lambda: _fitted("Matern52_kernel", 6, 3, 25, "node", ard=True),
           "camphor": lambda: _fitted_camphor("node"), "camphor_ard": _fitted_camphor_ard}[which]()
    D = mod["X"].shape[1] if which != "camphor_ard" else 6
    x = np.random.default_rng(2).random(D)
    gp = _stub_gp(eng, mod, x)
    H = gp.mean_hessian()
    assert H.shape == (D, D) and np.array_equal(H, H.T)
    assert np.array_equal(np.diag(H), gp.sharpness()[0])
    Xi = np.random.default_rng(3).standard_normal((40, D))
    mu = gp.curvature_pred(np.tile(x, (40, 1)), Xi)[0]
    c = cn.curvature_column(np.tile(x, (40, 1)), Xi, mod["X"], mod["th"], mod["kernel"])
    e = np.max(np.abs(np.einsum("ia,ab,ib->i", Xi, H, Xi) - mu) / (np.abs(c) @ np.abs(mod["alpha"])))
    print(f"curvature mean_hessian {which}: |xi' H xi - mu_c| / sum|c alpha| = {e:.2e}")
    assert e <= TOL
    other = np.random.default_rng(4).random(D)
    assert not np.array_equal(gp.mean_hessian(other), H)
    if which == "radial":
        # a posterior without G serves
        bare = eng.mean_posterior(mod["X"], mod["th"], mod["kernel"], mod["m"], mod["post"].alpha)
        gp2 = _stub_gp(eng, dict(post=bare), x)
        assert np.array_equal(gp2.mean_hessian(), H)


# ---------------------------------------------------------------- 6. NaN rules, score kinds, the argmax
@pytest.mark.parametrize("form", ["node", "edge"])
def test_nan_rows_score_kinds_and_argmax(eng, form):
    from ppbo_amd.engine import CURV_MEAN, CURV_PROB, CURV_VARIANCE
    mod = _fitted("Matern52_kernel", 6, 8, 3, form)
    post = mod["post"]
    X, Xi = _rows(np.random.default_rng(10), mod, 601)
    X[400], Xi[400] = X[200], Xi[200]              # duplicate rows: a tie goes to the first
    clean = eng.predict_curvatures(post, X, Xi)
    assert all(host(clean[k])[400] == host(clean[k])[200] for k in ("mu", "var", "prob"))
    X[3, 2], Xi[10, 0], X[599, 5], Xi[300, 1] = np.nan, np.nan, np.inf, -np.inf
    bad = np.zeros(601, dtype=bool)
    bad[[3, 10, 599, 300]] = True
    for kind, key in ((CURV_MEAN, "mu"), (CURV_VARIANCE, "var"), (CURV_PROB, "prob")):
        out = eng.predict_curvatures(post, X, Xi, score=kind, want_score=True)
        sc = host(out["score"])
        assert np.array_equal(sc, host(out[key]), equal_nan=True)
        for k in ("mu", "var", "prob"):
            v = host(out[k])
            assert np.all(np.isnan(v[bad])) and np.array_equal(_bits(v[~bad]), _bits(host(clean[k])[~bad]))
        assert out["best_idx"] == int(np.nanargmax(sc)) and out["best_val"] == np.nanmax(sc)
        assert not bad[out["best_idx"]]
    # the tie of the duplicates, made the winner: the first of them comes back
    Xw, Xiw = X[[5, 200, 7, 400]], Xi[[5, 200, 7, 400]] * np.array([[0.0], [1.0], [0.0], [1.0]])
    tie = eng.predict_curvatures(post, Xw, Xiw, score=CURV_VARIANCE)
    assert tie["best_idx"] == 1 and host(tie["var"])[1] == host(tie["var"])[3]
    # nothing but NaN rows: (NaN, -1)
    none = eng.predict_curvatures(post, X[[3, 10, 599]], Xi[[3, 10, 599]])
    assert none["best_idx"] == -1 and np.isnan(none["best_val"])
    # the mean alone needs no operator: a model without G, bit for bit the mean of the full call
    bare = eng.mean_posterior(mod["X"], mod["th"], mod["kernel"], mod["m"], post.alpha)
    mean = eng.predict_curvatures(bare, X, Xi, score=CURV_MEAN, want_var=False, want_prob=False, want_score=True)
    assert mean["var"] is None and mean["prob"] is None
    assert np.array_equal(host(mean["mu"])[~bad], host(clean["mu"])[~bad]) and np.all(np.isnan(host(mean["mu"])[bad]))
    assert mean["best_idx"] == int(np.nanargmax(host(mean["score"])))


# ---------------------------------------------------------------- 7. sharpness
@pytest.mark.parametrize("which", ["radial", "camphor_ard"])
def test_sharpness_is_D_unit_curvatures(eng, which):
    mod = _fitted_camphor_ard() if which == "camphor_ard" else _fitted("SE_kernel", 6, 8, 3, "node")
    D = 6
    xstar = np.random.default_rng(2).random(D)
    gp = _stub_gp(eng, mod, xstar)
    mu, var, p = gp.sharpness()
    assert mu.shape == var.shape == p.shape == (D,)
    for d in range(D):
        one = gp.curvature_pred(xstar, np.eye(D)[d])
        assert (one[0][0], one[1][0], one[2][0]) == (mu[d], var[d], p[d])
    other = np.random.default_rng(3).random(D)
    assert np.array_equal(gp.sharpness(other)[0], gp.curvature_pred(np.tile(other, (D, 1)), np.eye(D))[0])
    e_mu, e_var, _ = _errors(mod, np.tile(xstar, (D, 1)), np.eye(D), mu, var, p)
    assert e_mu <= TOL and e_var <= TOL


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_context_usable(eng):
    from ppbo_amd.engine import CURV_MEAN, CURV_PROB, CURV_VARIANCE
    mod = _fitted("SE_kernel", 6, 8, 3, "node")
    post = mod["post"]
    X, Xi = _rows(np.random.default_rng(11), mod, 100)
    before = eng.predict_curvatures(post, X, Xi)
    dx, dxi, mu, var = eng.dev(X), eng.dev(Xi), eng.empty(100), eng.empty(100)
    md, md32, bare = eng._model(post, True), eng._model(post, True, kstar_fp32=True), eng._model(post, False)
    nolam = eng._model(post, True)
    nolam.d_lam_diag = 0
    m32 = _fitted("Matern32_kernel", 6, 8, 3, "node")
    md_m32 = eng._model(m32["post"], True)
    big = _fitted("SE_kernel", 20, 3, 25, "node")
    md_big = eng._model(big["post"], True)
    dx20 = eng.dev(np.zeros((100, 20)))
    cam = _fitted_camphor("node")
    md_cam = eng._model(cam["post"], True)

    def call(model, a, b, M, kind, d_var=None, d_prob=None, acc=None):
        return _c_call(eng, model, a, b, acc, M, kind, mu, d_var, d_prob)

    for args in ((None, dx, dxi, 100, CURV_PROB), (md, None, dxi, 100, CURV_PROB), (md, dx, None, 100, CURV_PROB),
                 (md, dx, dxi, 0, CURV_PROB), (md, dx, dxi, -5, CURV_PROB), (md, dx, dxi, 2 ** 31, CURV_PROB),
                 (md, dx, dxi, 100, 3), (md, dx, dxi, 100, -1), (md32, dx, dxi, 100, CURV_PROB),
                 (bare, dx, dxi, 100, CURV_PROB), (bare, dx, dxi, 100, CURV_VARIANCE), (bare, dx, dxi, 100, CURV_MEAN, var),
                 (bare, dx, dxi, 100, CURV_MEAN, None, var), (nolam, dx, dxi, 100, CURV_PROB),
                 (md_m32, dx, dxi, 100, CURV_PROB), (md_m32, dx, dxi, 100, CURV_MEAN),
                 (md_big, dx20, dx20, 100, CURV_PROB, None, None, dx20), (md_cam, dx, dxi, 100, CURV_PROB, None, None, dxi)):
        rc, msg = call(*args)
        assert rc != 0 and "invalid argument" in msg, (args[3:5], rc, msg)
    assert call(bare, dx, dxi, 100, CURV_MEAN)[0] == 0          # the mean alone: no operator needed
    assert call(md, dx, dxi, 100, CURV_PROB)[0] == 0
    assert call(md, dx, dxi, 100, CURV_PROB, None, None, dxi)[0] == 0     # D = 6 takes accelerations
    assert call(md_big, dx20, dx20, 100, CURV_PROB)[0] == 0
    assert call(md_cam, dx, dxi, 100, CURV_PROB)[0] == 0
    after = eng.predict_curvatures(post, X, Xi)
    for k in ("mu", "var", "prob"):
        assert np.array_equal(_bits(host(before[k])), _bits(host(after[k])))
    with pytest.raises(ValueError, match="predict_curvatures"):
        eng.predict_curvatures(post, X, Xi[:50])
    with pytest.raises(ValueError, match="predict_curvatures"):
        eng.predict_curvatures(post, X[:, :5], Xi[:, :5])
    with pytest.raises(ValueError, match="predict_curvatures"):
        eng.predict_curvatures(m32["post"], X, Xi)
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = None
    with pytest.raises(RuntimeError, match="posterior covariance unavailable"):
        gp.curvature_pred(X[0], Xi[0])
