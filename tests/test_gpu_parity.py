"""GPU parity tests: every C-ABI entry point against the CPU oracle and the golden
vectors produced by the reference.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import dense_ref as dr
from conftest import golden_names
from oracle import ppbo_oracle as orc

pytestmark = pytest.mark.gpu

ALL = golden_names()
FITTED = [n for n in ("smoke", "rq", "cam_small", "c2", "c4", "c3", "c5") if n in ALL]


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
    """Relative difference IN THE MAX NORM: max|a - b| / max|b| (not elementwise).  That is the norm every "relative"
    tolerance of this file is stated in -- north_star's "within 1e-5 relative" included: posterior means change sign
    across a candidate set and variances go to ~1e-6 sigma_f^2 at the design points, so an elementwise ratio would be
    dominated by the entries whose reference value is a rounding residue.  Variances are additionally held to an
    absolute bound in units of sigma_f^2 where they are tested."""
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b)))


# ---------------------------------------------------------------- dense engine
@pytest.mark.parametrize("shape", [(128, 128, 16), (130, 75, 33), (256, 384, 64), (70, 70, 2048), (513, 129, 257)])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_dgemm(eng, shape, ta, tb):
    M, N, K = shape
    rng = np.random.default_rng(M * 7 + N * 3 + K + ta * 2 + tb)
    A = rng.standard_normal((K, M) if ta else (M, K))
    B = rng.standard_normal((N, K) if tb else (K, N))
    C0 = rng.standard_normal((M, N))
    ref = 1.5 * (A.T if ta else A) @ (B.T if tb else B) - 0.5 * C0
    Cd = eng.dev(C0.copy())
    out = eng.dgemm(A, B, bool(ta), bool(tb), alpha=1.5, beta=-0.5, C_out=Cd)
    assert rel(host(out), ref) < 1e-13


def test_dgemm_mfma_layout_is_not_transposed(eng):
    """A = I with an asymmetric B catches a swapped C/D register map."""
    n = 128
    B = np.arange(n * n, dtype=np.float64).reshape(n, n)
    out = host(eng.dgemm(np.eye(n), B))
    assert np.array_equal(out, B)


@pytest.mark.parametrize("N", [1, 17, 63, 64, 65, 100, 129, 200, 512, 650, 1031, 2500, 4200])
def test_potrf_and_inverse(eng, N):
    rng = np.random.default_rng(N)
    Q = rng.standard_normal((N, N))
    A = Q @ Q.T + N * np.eye(N)
    L = np.tril(host(eng.potrf_(eng.dev(A.copy()))))
    assert rel(L, np.linalg.cholesky(A)) < 1e-12
    Ai = host(eng.pd_inverse(A))
    assert np.abs(Ai @ A - np.eye(N)).max() < 1e-10
    assert np.abs(Ai - Ai.T).max() <= 1e-12 * np.abs(Ai).max()


@pytest.mark.parametrize("N", [1, 15, 257, 1000, 2048])
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("lower", [False, True])
def test_dgemv(eng, N, trans, lower):
    rng = np.random.default_rng(N + 2 * trans + lower)
    A = rng.standard_normal((N, N))
    x = rng.standard_normal(N)
    y = host(eng.dgemv(A, x, trans=trans, lower=lower))
    Ae = np.tril(A) if lower else A
    ref = (Ae.T if trans else Ae) @ x
    assert np.abs(y - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()) * np.sqrt(N)
    y2 = host(eng.dgemv(A, x, trans=trans, lower=lower))
    assert np.array_equal(y, y2)            # fixed summation order: bitwise reproducible


@pytest.mark.parametrize("bad", [0, 63, 64, 150, 199])
def test_potrf_reports_not_pd(eng, bad):
    """LAPACK's info: the 1-based order of the first leading minor that is not positive definite."""
    from ppbo_amd.engine import NotPositiveDefinite
    N = 200
    A = np.eye(N) + 0.01
    A[bad, bad] = -1.0
    with pytest.raises(NotPositiveDefinite) as ei:
        eng.potrf_(eng.dev(A))
    assert ei.value.info == bad + 1


@pytest.mark.parametrize("kind", ["negative", "zero", "nan"])
def test_potrf_failure_column_is_lapacks(eng, kind):
    """Round 6: the slab factor no longer tests every pivot -- a pivot that is not positive poisons everything right of it
    with NaN, the LAST pivot of a 16-column slab tells, and only then the slab's pivots are scanned.  Every position class
    of a slab (first / inner / last column, first / later slab of a 64-column block, first / later block), a negative, an
    exactly zero and a NaN pivot: `info` is LAPACK's (netlib's, where the NaN is concerned)."""
    from scipy.linalg import lapack
    from ppbo_amd.engine import NotPositiveDefinite
    N = 150
    rng = np.random.default_rng(5)
    for bad in (0, 1, 15, 16, 17, 31, 32, 47, 48, 62, 63, 64, 65, 79, 80, 127, 128, 143, 149):
        if kind == "zero":
            A = np.diag(1.0 + rng.random(N))            # diagonal: the pivot is the entry itself, exactly
            A[bad, bad] = 0.0
        else:
            Q = rng.standard_normal((N, N))
            A = Q @ Q.T + N * np.eye(N)
            A[bad, bad] = -3.0 if kind == "negative" else np.nan
        info_ref = bad + 1          # netlib dpotrf2: ajj <= 0 or isnan(ajj); the OpenBLAS under SciPy lets a NaN pivot pass
        if kind != "nan":
            assert lapack.dpotrf(np.tril(A), lower=1)[1] == info_ref
        with pytest.raises(NotPositiveDefinite) as ei:
            eng.potrf_(eng.dev(A))
        assert ei.value.info == info_ref, (kind, bad)
    # and the context factors a good matrix right after
    Q = rng.standard_normal((N, N))
    A = Q @ Q.T + N * np.eye(N)
    assert rel(np.tril(host(eng.potrf_(eng.dev(A.copy())))), np.linalg.cholesky(A)) < 1e-12


@pytest.mark.parametrize("N,pad", [(200, 8), (257, 3)])
def test_potrf_with_leading_dimension(eng, N, pad):
    """lda > N (and odd): the factor lands in the view, the padding columns are untouched."""
    rng = np.random.default_rng(N + pad)
    Q = rng.standard_normal((N, N))
    A = Q @ Q.T + N * np.eye(N)
    buf = eng.dev(np.full((N, N + pad), 7.0))
    view = buf[:, :N]
    view.copy_(eng.dev(A))
    eng.potrf_(view)
    out = host(buf)
    assert rel(np.tril(out[:, :N]), np.linalg.cholesky(A)) < 1e-12
    assert np.all(out[:, N:] == 7.0)


# ---------------------------------------------------------------- K1 / K2
@pytest.mark.parametrize("name", ALL)
def test_gram_vs_reference_golden(eng, golden, name):
    g = golden(name)
    S = host(eng.gram(g["X"], g["theta"], str(g["kernel"])))
    c = g["Sigma_corner"].shape[0]
    assert rel(S[:c, :c], g["Sigma_corner"]) < 1e-12
    assert rel(S.sum(axis=1), g["Sigma_rowsum"]) < 1e-12
    assert rel(S[g["Sigma_ii"], g["Sigma_jj"]], g["Sigma_samples"]) < 1e-12
    assert np.array_equal(S, S.T)
    if int(g["N"]) <= 1024:
        assert rel(S, orc.gram(g["X"], g["theta"], str(g["kernel"]))) < 1e-12


@pytest.mark.parametrize("kernel,D", [("SE_kernel", 5), ("RQ_kernel", 7), ("camphor_copper_kernel", 6)])
@pytest.mark.parametrize("n1,n2", [(1, 1), (3, 130), (200, 77), (129, 64)])
def test_cross_cov_ragged(eng, kernel, D, n1, n2):
    rng = np.random.default_rng(n1 * 1000 + n2)
    X1, X2 = rng.random((n1, D)), rng.random((n2, D))
    th = [0.05, 0.31, 0.7]
    K = host(eng.cross_cov(X1, X2, th, kernel))
    assert rel(K, orc.cross_cov(X1, X2, th, kernel)) < 1e-12


def test_gram_odd_sizes(eng):
    rng = np.random.default_rng(3)
    for N, D in [(1, 2), (63, 3), (65, 4), (257, 9)]:
        X = rng.random((N, D))
        S = host(eng.gram(X, [0.1, 0.4, 1.3], "SE_kernel"))
        assert rel(S, orc.gram(X, [0.1, 0.4, 1.3], "SE_kernel")) < 1e-12


# ---------------------------------------------------------------- K5
@pytest.mark.parametrize("name", ALL)
def test_laplace_terms_vs_reference_golden(eng, golden, name):
    g = golden(name)
    m, sig = int(g["m"]), float(g["theta"][0])
    for k in range(g["lap_f"].shape[0]):
        T, beta, ld, lo = eng.laplace_terms(g["lap_f"][k], m, sig)
        assert abs(T - g["lap_Tlik"][k]) <= 1e-12 * max(1.0, abs(g["lap_Tlik"][k]))
        assert np.abs(host(beta) - g["lap_beta"][k]).max() <= 1e-12 * max(1.0, np.abs(g["lap_beta"][k]).max())
        scale = max(1e-300, np.abs(g["lap_diag"][k]).max())
        assert np.abs(host(ld) - g["lap_diag"][k]).max() <= 1e-12 * scale
        assert np.abs(host(lo) - g["lap_off"][k]).max() <= 1e-12 * scale


@pytest.mark.parametrize("m", [1, 5, 25, 31, 63, 100])
def test_laplace_terms_general_m(eng, m):
    rng = np.random.default_rng(m)
    n_q = 7
    f = rng.standard_normal(n_q * (m + 1)) * 0.2
    T, beta, ld, lo = eng.laplace_terms(f, m, 0.07)
    assert abs(T - (-orc.sum_phi0(f, m, 0.07).sum() / m)) < 1e-12
    assert np.abs(host(beta) - orc.beta_vector(f, m, 0.07)).max() < 1e-11
    d0, o0 = orc.lambda_compact(f, m, 0.07)
    assert np.abs(host(ld) - d0).max() <= 1e-12 * np.abs(d0).max()
    assert np.abs(host(lo) - o0).max() <= 1e-12 * np.abs(d0).max()


# ---------------------------------------------------------------- fit
def _sinv(eng, g):
    S = eng.gram(g["X"], g["theta"], str(g["kernel"]))
    return S, eng.pd_inverse(S)


@pytest.mark.parametrize("name", FITTED)
def test_T_and_grad(eng, golden, name):
    g = golden(name)
    m, sig = int(g["m"]), float(g["theta"][0])
    _, Sinv = _sinv(eng, g)
    Sinv_h = host(Sinv)
    for k in range(g["lap_f"].shape[0]):
        f = g["lap_f"][k]
        T, grad = eng.T_and_grad(Sinv, f, m, sig)
        assert abs(T - g["lap_T"][k]) <= 1e-7 * max(1.0, abs(g["lap_T"][k]))
        gscale = max(np.abs(Sinv_h @ f).max(), 1e-300)
        assert np.abs(host(grad) - g["lap_grad"][k]).max() <= 1e-6 * gscale + 1e-9


@pytest.mark.parametrize("name", FITTED)
def test_fit_fmap_vs_reference(eng, golden, name):
    g = golden(name)
    m, sig = int(g["m"]), float(g["theta"][0])
    _, Sinv = _sinv(eng, g)
    fmap, st = eng.fit_fmap(Sinv, g["f_init"], m, sig, gtol=1e-6)
    f = host(fmap)
    # reference-evaluated gradient norm must not exceed the reference's own (two-level parity)
    _, grad = eng.T_and_grad(Sinv, f, m, sig)
    gn = np.linalg.norm(host(grad))
    assert gn <= max(float(g["gradnorm_fMAP"]), 2e-6)
    # distance: 1e-5 max|f| plus the reference's own Newton gap |P g_ref| (it stops at gtol 1e-4)
    post = eng.posterior(g["X"], g["theta"], str(g["kernel"]), Sinv, g["fMAP"], m, want_P=True)
    _, gref = eng.T_and_grad(Sinv, g["fMAP"], m, sig)
    ref_gap = np.abs(host(post.P) @ host(gref)).max()
    assert np.abs(f - g["fMAP"]).max() <= 1e-5 * np.abs(g["fMAP"]).max() + 1.5 * ref_gap
    assert st["T"] >= float(g["T_fMAP"]) - 1e-7 * max(1.0, abs(float(g["T_fMAP"])))


# ---------------------------------------------------------------- predict
def _posterior(eng, g, want_P=False):
    _, Sinv = _sinv(eng, g)
    return eng.posterior(g["X"], g["theta"], str(g["kernel"]), Sinv, g["fMAP"], int(g["m"]), want_P=want_P), Sinv


@pytest.mark.parametrize("name", FITTED)
def test_predict_mean_var_vs_reference(eng, golden, name):
    from ppbo_amd.engine import SCORE_MEAN
    g = golden(name)
    post, _ = _posterior(eng, g)
    out = eng.predict(post, g["Xc"], score=SCORE_MEAN, want_score=True)
    mu, var = host(out["mu"]), host(out["var"])
    sf2 = float(g["theta"][2]) ** 2
    assert rel(mu, g["mu"]) < 1e-6                       # north_star: 1e-5
    assert np.abs(var - g["var"]).max() <= 1e-6 * sf2    # north_star: 1e-5 relative
    assert rel(host(post.alpha), g["alpha"]) < 1e-6
    assert out["best_idx"] == int(np.argmax(host(out["score"])))
    assert out["best_val"] == host(out["score"]).max()
    one = eng.predict(post, g["Xc"][:16], want_var=False)
    assert rel(host(one["mu"]), g["mu_pred16"]) < 1e-6


@pytest.mark.parametrize("name", [n for n in FITTED if n != "c5"])
def test_posterior_covariance_vs_reference(eng, golden, name):
    g = golden(name)
    post, _ = _posterior(eng, g, want_P=True)
    P = host(post.P)
    c = g["P_corner"].shape[0]
    scale = np.abs(g["P_diag"]).max()
    assert np.abs(np.diag(P) - g["P_diag"]).max() <= 1e-6 * scale
    assert np.abs(P[:c, :c] - g["P_corner"]).max() <= 1e-6 * scale


@pytest.mark.parametrize("name", FITTED)
def test_mean_grad_vs_oracle(eng, golden, name):
    """ppbo_mean_grad: mu against the reference's golden means, the gradient against the oracle's analytic
    derivative (itself pinned by central differences in the CPU suite)."""
    g = golden(name)
    post, _ = _posterior(eng, g)
    Xc = g["Xc"][:96]
    mu, grad = eng.mean_grad(post, Xc)
    mu0, grad0 = orc.mean_grad(Xc, g["X"], g["theta"], host(post.alpha), str(g["kernel"]))
    assert rel(host(mu), mu0) < 1e-9
    assert rel(host(mu), g["mu"][:96]) < 1e-5
    assert np.abs(host(grad) - grad0).max() <= 1e-9 * max(np.abs(grad0).max(), 1e-300)


def test_mean_grad_ragged_and_errors(eng, golden):
    g = golden("smoke")
    post, _ = _posterior(eng, g)
    mu, grad = eng.mean_grad(post, g["Xc"][:1])
    assert mu.shape == (1,) and grad.shape == (1, int(g["D"]))
    mu0, grad0 = orc.mean_grad(g["Xc"][:1], g["X"], g["theta"], host(post.alpha), str(g["kernel"]))
    assert rel(host(grad), grad0) < 1e-9
    import ctypes as C
    assert eng.lib.ppbo_mean_grad(eng.ctx, None, None, 1, None, None, None) < 0


@pytest.mark.parametrize("name", FITTED)
def test_predict_cov_line_vs_reference(eng, golden, name):
    g = golden(name)
    post, _ = _posterior(eng, g)
    mu, cov = eng.predict_cov(post, g["line_grid"])
    sf2 = float(g["theta"][2]) ** 2
    assert rel(host(mu), g["line_mu"]) < 1e-6
    assert np.abs(host(cov) - g["line_cov"]).max() <= 1e-6 * sf2


@pytest.mark.parametrize("name", [n for n in ("smoke", "c2", "c3") if n in ALL])
def test_line_acq_matches_oracle_with_same_draws(eng, golden, name):
    g = golden(name)
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
    # line 0 is the reference's own grid: statistical agreement with its Monte Carlo value
    zz = rng.standard_normal((4000, G))
    e_big, _ = eng.line_acq(post, grid[:1], zz, mustar, jitter=jit)
    smp = orc.line_samples(g["line_mu"], g["line_cov"], zz, jit).max(axis=1)
    se = np.std(np.maximum(smp - mustar, 0)) * np.sqrt(2 / 4000)
    assert abs(float(host(e_big)[0]) - float(g["line_ei_ref4000"])) <= 4 * se + 1e-12


def test_argmax_first_occurrence_and_scores(eng, golden):
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    g = golden("smoke")
    post, _ = _posterior(eng, g)
    Xc = np.concatenate([g["Xc"], g["Xc"]])      # every score appears twice -> first index must win
    out = eng.predict(post, Xc, want_score=True)
    assert out["best_idx"] == int(np.argmax(host(out["score"]))) < g["Xc"].shape[0]
    mustar = float(np.max(g["mu"]))
    ei = eng.predict(post, g["Xc"], score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True)
    want = orc.pointwise_ei(host(ei["mu"]), host(ei["var"]), mustar)
    assert np.abs(host(ei["score"]) - want).max() <= 1e-10 * max(1e-12, np.abs(want).max())
    assert ei["best_idx"] == int(np.argmax(host(ei["score"])))
    vs = eng.predict(post, g["Xc"], score=SCORE_VARIANCE, want_score=True)
    assert np.array_equal(host(vs["score"]), host(vs["var"]))


# ---------------------------------------------------------------- RFF
@pytest.mark.parametrize("name", [n for n in ("smoke", "c2", "c3") if n in ALL])
def test_rff_vs_reference(eng, golden, name):
    g = golden(name)
    m, sig, sf = int(g["m"]), float(g["theta"][0]), float(g["theta"][2])
    Phi = eng.rff_project(g["X"], g["rff_W"], g["rff_b"], sf)
    Ph = host(Phi)
    fc, c = g["rff_Phi_corner"].shape
    assert rel(Ph[:fc, :c], g["rff_Phi_corner"]) < 1e-11
    assert rel(Ph.sum(axis=1), g["rff_Phi_rowsum"]) < 1e-10
    assert rel(Ph.sum(axis=0), g["rff_Phi_colsum"]) < 1e-10
    S, gr, hd = eng.rff_terms(Phi, g["rff_omega"], m, sig)
    assert abs(S - float(g["rff_S"])) <= 1e-10 * abs(float(g["rff_S"]))
    assert rel(host(gr), g["rff_Sgrad"]) < 1e-9
    assert rel(host(hd), g["rff_Shdiag"]) < 1e-9
    sc, bv, bi = eng.rff_score(g["Xc"], g["rff_W"], g["rff_b"], sf, g["rff_omega"])
    assert rel(host(sc), g["rff_scores"]) < 1e-9
    assert bi == int(np.argmax(host(sc))) and bv == host(sc).max()


@pytest.mark.parametrize("N,F,D", [(1, 1, 1), (63, 65, 3), (130, 70, 7), (257, 130, 20), (1000, 300, 33), (514, 4100, 6)])
@pytest.mark.parametrize("nt", ["1", "2", "4"])
def test_rff_project_ragged_shapes(N, F, D, nt):
    """Odd N takes the 8-byte store path, even N the 16-byte row-pair path; every strip length; F, N, D ragged
    against the 64-wide tiles and the depth buckets; phases far outside the branch-free cosine's range take the
    library path behind the wave-uniform branch."""
    import os
    from ppbo_amd.engine import Engine
    os.environ["PPBO_RFF_NT"] = nt
    try:
        e = Engine(0)                      # the knob is read once per ctx
    finally:
        os.environ.pop("PPBO_RFF_NT", None)
    rng = np.random.default_rng(N + F + D)
    X = rng.random((N, D))
    W = rng.standard_normal((F, D)) / 0.1
    b = rng.uniform(0, 2 * np.pi, F)
    if F > 2:
        W[1] *= 1e6                          # |w.x| ~ 1e7: beyond the fast range
        b[2] = 3e7
    Phi = host(e.rff_project(X, W, b, 0.7))
    ref = orc.rff_features(X, W, b, 0.7)
    assert Phi.shape == (F, N)
    # a phase of 1e7 carries 1e7 * eps of argument rounding in ANY double evaluation of w.x + b
    tol = np.full((F, 1), 1e-12)
    if F > 2:
        tol[1] = tol[2] = 1e-8
    assert np.all(np.abs(Phi - ref) <= tol * np.sqrt(2 * 0.49 / F) * 10 + 1e-16)
    om = rng.standard_normal(F)
    sc, bv, bi = e.rff_score(X, W, b, 0.7, om)
    assert np.abs(host(sc) - ref.T @ om).max() <= 1e-7 * np.abs(ref.T @ om).max() + 1e-12
    e.close()


# ---------------------------------------------------------------- full-size properties (BASELINE config C3)
@pytest.mark.skipif("c3" not in ALL, reason="c3 fixture missing")
def test_full_size_c3_properties(eng, golden):
    """N=2048, D=20, M=65536: chunked scoring equals per-slice scoring, argmax equals
    np.argmax of the returned scores, and a random subsample matches the oracle."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    g = golden("c3")
    post, Sinv = _posterior(eng, g)
    M = 65536
    Xc = np.random.default_rng(1).random((M, int(g["D"])))
    mustar = float(np.max(g["mu"]))
    full = eng.predict(post, Xc, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True)
    sc = host(full["score"])
    assert full["best_idx"] == int(np.argmax(sc)) and full["best_val"] == sc.max()
    part = eng.predict(post, Xc[30000:31000], score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True)
    # independent of how the candidate set is tiled / split (only the partial-sum grouping differs)
    assert np.allclose(host(part["mu"]), host(full["mu"])[30000:31000], rtol=0, atol=1e-12)
    assert np.allclose(host(part["var"]), host(full["var"])[30000:31000], rtol=0, atol=1e-12)
    idx = np.random.default_rng(2).choice(M, 256, replace=False)
    sf2 = float(g["theta"][2]) ** 2
    # the oracle from the CPU alone: Sigma^-1, P and the variance operator from orc.gram (a wrong device Sigma^-1
    # would cancel out of an oracle built on it)
    cpu = dr.CpuModel(g["X"], g["theta"], str(g["kernel"]), int(g["m"]), g["fMAP"])
    mu0, var0 = cpu.mean_var(Xc[idx])
    assert rel(host(full["mu"])[idx], mu0) < 1e-6
    assert np.abs(host(full["var"])[idx] - var0).max() <= 1e-6 * sf2
    # and the identity check on the device's own Sigma^-1
    Sinv_h = host(Sinv)
    P = orc.posterior_covariance(Sinv_h, g["fMAP"], int(g["m"]), float(g["theta"][0]))
    lam = orc.lambda_dense(g["fMAP"], int(g["m"]), float(g["theta"][0]))
    A = orc.variance_operator(Sinv_h, P, faithful=False, lam=lam)
    mu0, var0 = orc.predict_mean_var(Xc[idx], g["X"], g["theta"], Sinv_h @ g["fMAP"], A)
    assert rel(host(full["mu"])[idx], mu0) < 1e-6
    assert np.abs(host(full["var"])[idx] - var0).max() <= 1e-6 * sf2


# ---------------------------------------------------------------- general m / sizes without a reference fixture
@pytest.mark.parametrize("m,n_q,D,kernel", [(1, 40, 2, "SE_kernel"), (5, 13, 3, "RQ_kernel"), (25, 6, 2, "SE_kernel"),
                                            (25, 25, 2, "SE_kernel"), (63, 3, 4, "SE_kernel")])
def test_pipeline_general_m_vs_oracle(eng, m, n_q, D, kernel):
    """Whole device pipeline (Gram, inverse, fit, posterior, predict, covariance) against the oracle for
    star sizes that do not divide the 128-row MFMA tiles (the reference's default is m=25)."""
    th = [0.2, 0.3, 0.5]
    X = orc.synthetic_design(n_q, D, m=m, seed=3)
    N = X.shape[0]
    S0 = orc.gram(X, th, kernel)
    Sinv0 = orc.pd_inverse(S0)
    f_init = np.random.default_rng(2).multivariate_normal(np.zeros(N), S0, method="cholesky")
    f0, _ = orc.fit_fmap_trust_exact(f_init, Sinv0, m, th[0], gtol=1e-9)
    S = eng.gram(X, th, kernel)
    Sinv = eng.pd_inverse(S)
    assert rel(host(Sinv), Sinv0) < 1e-6
    fm, st = eng.fit_fmap(Sinv, f_init, m, th[0], gtol=1e-8)
    assert np.abs(host(fm) - f0).max() <= 5e-6 * np.abs(f0).max()     # two optimisers, cond(Sigma) ~ 1e7
    post = eng.posterior(X, th, kernel, Sinv, f0, m, want_P=True)
    P0 = orc.posterior_covariance(Sinv0, f0, m, th[0])
    assert rel(host(post.P), P0) < 1e-6
    Xc = np.random.default_rng(4).random((300, D))
    A0 = orc.variance_operator(Sinv0, P0, faithful=False, lam=orc.lambda_dense(f0, m, th[0]))
    mu0, var0 = orc.predict_mean_var(Xc, X, th, Sinv0 @ f0, A0, kernel)
    out = eng.predict(post, Xc)
    assert rel(host(out["mu"]), mu0) < 1e-7
    assert np.abs(host(out["var"]) - var0).max() <= 1e-7 * th[2] ** 2
    mu1, cov1 = eng.predict_cov(post, Xc[:70])
    _, cov0 = orc.mu_sigma_pred(Xc[:70], X, th, Sinv0, f0, P0, kernel, faithful=False, A=A0)
    assert np.abs(host(cov1) - cov0).max() <= 1e-7 * th[2] ** 2
    # the line acquisitions at this star size: the covariance's data term takes the ONE-SIDED Lambda form of
    # line_cov_kernel (stars do not coincide with its 32-row chunks) -- against the oracle on the oracle's covariance
    rng = np.random.default_rng(6)
    B, G, Sd = 7, 70, 96
    xis = np.eye(D)[rng.integers(0, D, B)]
    xs = rng.random((B, D)) * (xis == 0)
    al = np.sort(np.clip(np.linspace(0.005, 0.995, G) + rng.normal(0, 0.01, (B, G)), 0, 1), axis=1)
    z = rng.standard_normal((Sd, G))
    mustar, jit = float(mu0.max()), 1e-9 * th[2] ** 2
    ei, vm = eng.line_acq_xi(post, xis, xs, al, z, mustar, jitter=jit)
    for b in range(B):
        grid = al[b][:, None] * xis[b][None, :] + xs[b][None, :]
        mu_b, cov_b = orc.mu_sigma_pred(grid, X, th, Sinv0, f0, P0, kernel, faithful=False, A=A0)
        e0 = orc.line_ei(mu_b, cov_b, z, mustar, jitter=jit)
        v0 = orc.line_varmax(mu_b, cov_b, z, jitter=jit)
        assert abs(float(host(ei)[b]) - e0) <= 1e-6 * max(abs(e0), 1e-3 * th[2])
        assert abs(float(host(vm)[b]) - v0) <= 1e-5 * max(abs(v0), 1e-6 * th[2] ** 2)


def test_c5_size_camphor_properties(eng):
    """BASELINE config 5 shape: camphor-copper kernel, D=6, N=4096 (m=31).  No reference fixture at this
    size (the reference's own fit takes hours): device fit, then prediction against the oracle on a subsample."""
    th, m, D, n_q = [0.05, 0.26, 0.1], 31, 6, 128
    kernel = "camphor_copper_kernel"
    X = orc.synthetic_design(n_q, D, m=m, seed=5)
    N = X.shape[0]
    S = eng.gram(X, th, kernel)
    Sh = host(S)
    assert np.array_equal(Sh, Sh.T)
    ii = np.random.default_rng(0).integers(0, N, 300)
    Kraw = orc.cross_cov(X[ii], X[ii], th, kernel)
    off = ~np.eye(len(ii), dtype=bool) & (ii[:, None] != ii[None, :])
    assert np.abs(Sh[np.ix_(ii, ii)][off] - (1 - 1e-6) * Kraw[off]).max() <= 1e-12 * th[2] ** 2
    Sinv = eng.pd_inverse(S)
    f_init = host(eng.dgemv(eng.potrf_(S.clone()), np.random.default_rng(2).standard_normal(N), lower=True))
    fm, st = eng.fit_fmap(Sinv, f_init, m, th[0], gtol=1e-5)
    assert st["converged"]
    post = eng.posterior(X, th, kernel, Sinv, fm, m, want_P=True)
    Xc = np.random.default_rng(1).random((4096, D))
    out = eng.predict(post, Xc)
    sub = np.random.default_rng(3).choice(4096, 64, replace=False)
    f = host(fm)
    # the oracle from the CPU alone at the device's f_MAP (the point the posterior is taken at; the fit is checked by
    # its convergence): Sigma^-1, P and the variance operator from orc.gram, no device intermediate
    cpu = dr.CpuModel(X, th, kernel, m, f)
    mu0, var0 = cpu.mean_var(Xc[sub])
    assert rel(host(out["mu"])[sub], mu0) < 1e-6
    assert np.abs(host(out["var"])[sub] - var0).max() <= 1e-6 * th[2] ** 2
    # and the identity checks on the device's own Sigma^-1 / P
    K = orc.cross_cov(X, Xc[sub], th, kernel)
    Sinv_h, P_h = host(Sinv), host(post.P)
    mu0 = K.T @ (Sinv_h @ f)
    lam = orc.lambda_dense(f, m, th[0])
    W = -lam
    A0 = W - W @ P_h @ W
    var0 = th[2] ** 2 - np.einsum("ij,ij->j", K, A0 @ K)
    assert rel(host(out["mu"])[sub], mu0) < 1e-6
    assert np.abs(host(out["var"])[sub] - var0).max() <= 1e-6 * th[2] ** 2
    assert np.abs(Sinv_h @ Sh - np.eye(N)).max() < 1e-5


# ---------------------------------------------------------------- a-9: LU / evidence
@pytest.mark.parametrize("N", [1, 5, 15, 16, 17, 31, 32, 33, 64, 100, 257, 513, 1024, 1025, 1500, 2048, 2300])
def test_lu_slogdet_matches_lapack_pivoting(eng, N):
    import scipy.linalg
    rng = np.random.default_rng(N)
    A = rng.standard_normal((N, N))
    A[rng.integers(0, N, max(1, N // 3)), :] *= -3.0
    P, L, U = scipy.linalg.lu(A)
    sgn_ref = np.prod(np.sign(np.diag(U)))
    ld_ref = np.sum(np.log(np.abs(np.diag(U))))
    Ad = eng.dev(A.copy())
    sgn, ld, info = eng.lu_slogdet_(Ad)
    assert info == 0
    assert sgn == sgn_ref                                  # pivot sequence (hence the signs of diag U) as LAPACK
    assert abs(ld - ld_ref) <= 1e-10 * max(1.0, abs(ld_ref))
    Uh = np.triu(host(Ad))
    assert np.abs(np.abs(np.diag(Uh)) - np.abs(np.diag(U))).max() <= 1e-9 * np.abs(np.diag(U)).max()


@pytest.mark.parametrize("name", [n for n in ("smoke", "rq") if n in ALL])
def test_evidence_vs_reference(golden, name):
    """GPModel.evidence on the device against the reference's values (same start vectors via a patched draw)."""
    from test_gpu_dropin import _model
    g = golden(name)
    gp, st = _model(g)
    gp.set_theta(); gp.update_Sigma(gp.theta); gp.update_Sigma_inv(gp.theta)
    for th, f0, v in zip(g["ev_theta"], g["ev_finit"], g["ev_value"]):
        gp._draw_prior = lambda f0=f0: gp.eng.dev(f0)
        mine = gp.evidence(list(th), None)
        assert abs(mine - float(v)) <= 1e-5 * max(1.0, abs(float(v))), (list(th), mine, float(v))


# ---------------------------------------------------------------- error conventions of the C-ABI
def test_error_codes_and_messages(eng, golden):
    import ctypes as C
    from ppbo_amd.engine import NotPositiveDefinite
    g = golden("smoke")
    X = eng.dev(g["X"])
    with pytest.raises(RuntimeError, match="camphor kernel needs D == 6"):
        eng.gram(X, g["theta"], "camphor_copper_kernel")
    with pytest.raises(RuntimeError, match="n_q\\*\\(m\\+1\\)"):
        eng.laplace_terms(np.zeros(65), 31, 0.1)
    S = eng.gram(X, g["theta"])
    Sinv = eng.pd_inverse(S)
    # every pseudo-observation sqrt(2) sigma above its observation maximises Lambda's weights:
    # Sigma^-1 - Lambda is then indefinite (min eigenvalue -1.06 here); the reference prints and keeps the
    # old posterior (gp_model.py:118-120)
    f_bad = np.where(np.arange(X.shape[0]) % (int(g["m"]) + 1) != 0, 1.414 * float(g["theta"][0]), 0.0)
    with pytest.raises(NotPositiveDefinite):
        eng.posterior(X, g["theta"], "SE_kernel", Sinv, f_bad, int(g["m"]))
    # null pointers / bad sizes are status codes, never crashes
    assert eng.lib.ppbo_gram(eng.ctx, 0, None, 4, 2, (C.c_double * 3)(0.1, 0.3, 0.5), 1e-6, None, None) < 0
    assert eng.lib.ppbo_predict(eng.ctx, None, None, 10, 0, 0.0, None, None, None, None, None, None) < 0
    buf = C.create_string_buffer(256)
    eng.lib.ppbo_last_error(eng.ctx, buf, 256)
    assert b"invalid argument" in buf.value
    # per-kernel event timing hooks
    eng.profile(True)
    eng.gram(X, g["theta"])
    ms, n = eng.profile_read("gram")
    assert n == 1 and ms > 0
    eng.profile(False)
    with pytest.raises(RuntimeError, match="unknown profile name"):
        eng.profile_read("nope")


@pytest.mark.parametrize("method", ["whitened", "trust-region"])
def test_dropin_posterior_not_psd_prints_and_continues(golden, capsys, method):
    """src/gp_model.py:118-120: a posterior precision that is not positive definite prints the reference's line and
    keeps the previous posterior covariance -- on the one-call update (ppbo_gp_fit reports info = 2 and no posterior)
    and on the call-by-call one (ppbo_posterior raises NotPositiveDefinite)."""
    from test_gpu_dropin import _model
    g = golden("smoke")
    gp, st = _model(g)
    gp.fMAP_method = method
    gp.turn_initialization_off()
    np.random.seed(2)
    gp.update_model()
    assert gp.fit_log[-1]["method"].startswith(method)
    old_post = gp._post
    assert old_post is not None
    # force an indefinite posterior precision on the next update
    f_bad = np.where(np.arange(gp.N) % (gp.m + 1) != 0, 1.414 * float(gp.theta[0]), 0.0)
    from ppbo_amd.engine import NotPositiveDefinite
    with pytest.raises(NotPositiveDefinite):       # the C path itself says so for this f
        gp.eng.posterior(gp._dX, gp.theta, gp.kernel.__name__, gp._dSigma_inv, f_bad, gp.m)
    real_fit, real_gp_fit = gp.eng.fit_fmap, gp.eng.gp_fit
    gp.eng.fit_fmap = lambda *a, **k: (gp.eng.dev(f_bad),
                                       dict(iterations=0, n_cholesky=0, converged=False, T=-1.0, gradnorm=1.0))

    def fake_gp_fit(*a, **k):                      # what ppbo_gp_fit hands back when Sigma^-1 - Lambda is not PD
        r = real_gp_fit(*a, **k)
        r.update(fMAP=gp.eng.dev(f_bad), post=None, info=2)
        return r

    gp.eng.gp_fit = fake_gp_fit
    try:
        gp.update_model()
    finally:
        gp.eng.fit_fmap, gp.eng.gp_fit = real_fit, real_gp_fit
    assert "Posterior covariance matrix is not PSD" in capsys.readouterr().out
    assert gp._post is old_post
    assert np.array_equal(gp.fMAP, f_bad)
    assert gp._post_mean is not old_post and gp._post_mean.G is None      # the mean follows the new f_MAP


@pytest.mark.skipif("c4" not in ALL, reason="c4 fixture missing")
def test_c4_sharded_search_equals_single_search(eng, golden):
    """BASELINE config 4 shape (N=1024, D=10, M=262144): scoring the 8 contiguous shards separately and
    combining the 16-byte records (what the 8 ranks do through RCCL) gives the single-GPU argmax."""
    import torch
    from ppbo_amd.dist import combine_best, shard_bounds
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    g = golden("c4")
    post, _ = _posterior(eng, g)
    M, world = 262144, 8
    Xc = eng.dev(np.random.default_rng(1).random((M, int(g["D"]))))
    Xc[1000] = Xc[200000]                        # a cross-shard tie: the lower global index must win
    mustar = float(np.max(g["mu"]))
    full = eng.predict(post, Xc, score=SCORE_POINTWISE_EI, mustar=mustar, want_score=True)   # 4 chunks of 65536
    sc = host(full["score"])
    assert full["best_idx"] == int(np.argmax(sc)) and full["best_val"] == sc.max()
    vals, idxs = [], []
    for r in range(world):
        lo, hi = shard_bounds(M, r, world)
        out = eng.predict(post, Xc[lo:hi], score=SCORE_POINTWISE_EI, mustar=mustar, want_mu=False, want_var=False)
        vals.append(out["best_val"])
        idxs.append(out["best_idx"] + lo)
    v, i = combine_best(torch.tensor(vals, dtype=torch.float64), torch.tensor(idxs))
    # same winner; the value may differ in the last bit (the row-split partial sums are grouped per launch size)
    assert i == full["best_idx"] and abs(v - full["best_val"]) <= 1e-12 * abs(full["best_val"])


@pytest.mark.parametrize("G", [90, 128])
def test_line_acq_long_grids(eng, golden, G):
    """G up to the documented 128 points per line: beyond ~89 the per-line Cholesky needs more than the default
    64 KB of dynamic LDS (133 KB at G = 128), which the library raises per ctx; G = 129 is an argument error."""
    g = golden("smoke")
    post, _ = _posterior(eng, g)
    D = int(g["D"])
    rng = np.random.default_rng(G)
    al = np.linspace(0.005, 0.995, G)
    grids = []
    for b in range(3):
        xi = np.zeros(D); xi[b % D] = 1.0
        x = rng.random(D); x[b % D] = 0.0
        grids.append(orc.line_grid(xi, x, al))
    grid = np.stack(grids)
    z = rng.standard_normal((150, G))
    sf2 = float(g["theta"][2]) ** 2
    mustar, jit = float(g["line_mustar"]), 1e-9 * sf2
    ei, vm = eng.line_acq(post, grid, z, mustar, jitter=jit)
    for b in range(3):
        mu_b, cov_b = eng.predict_cov(post, grid[b])
        e0 = orc.line_ei(host(mu_b), host(cov_b), z, mustar, jitter=jit)
        v0 = orc.line_varmax(host(mu_b), host(cov_b), z, jitter=jit)
        assert abs(host(ei)[b] - e0) <= 1e-6 * max(abs(e0), 1e-3 * np.sqrt(sf2))
        assert abs(host(vm)[b] - v0) <= 1e-5 * max(abs(v0), 1e-6 * sf2)
    with pytest.raises(RuntimeError, match="G <= 128"):
        eng.line_acq(post, np.zeros((1, 129, D)), rng.standard_normal((10, 129)), mustar)


@pytest.mark.parametrize("B,G,S", [(1, 1, 1), (1, 70, 4800), (2, 15, 63), (3, 16, 64), (5, 17, 65), (7, 33, 1000), (40, 70, 150),
                                   (64, 70, 1201), (300, 48, 97), (530, 20, 40)])
def test_line_acq_shapes(eng, golden, B, G, S):
    """The Monte-Carlo kernel splits the draws of a line over workgroups when the batch is small, pads grids to
    multiples of 16 and draws to multiples of 16 per split, and chunks batches above 512 lines: every combination
    of few / many lines, ragged G and ragged S against the oracle on the same draws (a few lines per case)."""
    g = golden("smoke")
    post, _ = _posterior(eng, g)
    D = int(g["D"])
    rng = np.random.default_rng(1000 * B + 10 * G + S)
    al = np.sort(rng.random(G))
    xis = np.zeros((B, D)); xis[np.arange(B), rng.integers(0, D, B)] = 1.0
    xs = rng.random((B, D)) * (xis == 0)
    grid = al[None, :, None] * xis[:, None, :] + xs[:, None, :]
    z = rng.standard_normal((S, G))
    sf2 = float(g["theta"][2]) ** 2
    mustar, jit = float(g["line_mustar"]), 1e-9 * sf2
    ei, vm = eng.line_acq(post, grid, z, mustar, jitter=jit)
    ei, vm = host(ei), host(vm)
    assert ei.shape == (B,) and np.all(np.isfinite(ei)) and np.all(np.isfinite(vm)) and np.all(ei >= 0) and np.all(vm >= -1e-12 * sf2)
    for b in sorted(set([0, B // 2, B - 1])):
        mu_b, cov_b = eng.predict_cov(post, grid[b])
        e0 = orc.line_ei(host(mu_b), host(cov_b), z, mustar, jitter=jit)
        v0 = orc.line_varmax(host(mu_b), host(cov_b), z, jitter=jit)
        assert abs(ei[b] - e0) <= 1e-6 * max(abs(e0), 1e-3 * np.sqrt(sf2)), (b, ei[b], e0)
        assert abs(vm[b] - v0) <= 1e-5 * max(abs(v0), 1e-6 * sf2), (b, vm[b], v0)
    # identical lines give identical values wherever they sit in the batch (split / chunk independent)
    if B >= 3:
        grid2 = grid.copy(); grid2[-1] = grid[0]
        ei2, vm2 = eng.line_acq(post, grid2, z, mustar, jitter=jit)
        assert host(ei2)[-1] == host(ei2)[0] and host(vm2)[-1] == host(vm2)[0]


def test_line_acq_chunk_edge(eng, golden):
    """513 lines = a chunk of 512 and a chunk of one: the last line of the first chunk and the only line of the second
    (and line 0) against the oracle on the same draws, at the tolerances of test_line_acq_shapes (whose batches above 512
    lines check their first, middle and last line only)."""
    g = golden("smoke")
    post, _ = _posterior(eng, g)
    B, G, S, D = 513, 3, 65, int(g["D"])
    rng = np.random.default_rng(513)
    al = np.sort(rng.random(G))
    xis = np.zeros((B, D)); xis[np.arange(B), rng.integers(0, D, B)] = 1.0
    xs = rng.random((B, D)) * (xis == 0)
    grid = al[None, :, None] * xis[:, None, :] + xs[:, None, :]
    z = rng.standard_normal((S, G))
    sf2 = float(g["theta"][2]) ** 2
    mustar, jit = float(g["line_mustar"]), 1e-9 * sf2
    ei, vm = eng.line_acq(post, grid, z, mustar, jitter=jit)
    ei, vm = host(ei), host(vm)
    assert ei.shape == (B,) and vm.shape == (B,)
    for b in (0, 511, 512):
        mu_b, cov_b = eng.predict_cov(post, grid[b])
        e0 = orc.line_ei(host(mu_b), host(cov_b), z, mustar, jitter=jit)
        v0 = orc.line_varmax(host(mu_b), host(cov_b), z, jitter=jit)
        assert abs(ei[b] - e0) <= 1e-6 * max(abs(e0), 1e-3 * np.sqrt(sf2)), (b, ei[b], e0)
        assert abs(vm[b] - v0) <= 1e-5 * max(abs(v0), 1e-6 * sf2), (b, vm[b], v0)


@pytest.mark.parametrize("m,n_q,B,G", [(25, 10, 40, 70), (25, 7, 3, 70), (9, 13, 33, 64), (30, 5, 50, 48), (25, 21, 30, 70), (40, 5, 30, 70),
                                       (1, 100, 8, 70), (15, 12, 35, 70), (33, 6, 30, 17), (25, 24, 600, 16)])
def test_line_acq_ragged_star_sizes(eng, m, n_q, B, G):
    """Line acquisitions on posteriors whose star size divides neither the chunk depth nor the row tile (m = 25 is the
    reference's default): from B G >= 2048 grid points on, Y = G K* runs on the zero-framed G with K* and Y padded to
    whole tiles; below, on the model's own array through the guarded loop.  Both against the full covariance
    (ppbo_predict_cov) + the oracle's Monte-Carlo statements on the same draws."""
    D = 4
    th = [0.3, 0.6, 0.8]
    X = orc.synthetic_design(n_q, D, m=m, seed=7 * m + n_q)
    N = X.shape[0]
    S0 = orc.gram(X, th, "SE_kernel")
    Sinv0 = orc.pd_inverse(S0)
    f_init = np.random.default_rng(m).multivariate_normal(np.zeros(N), S0, method="cholesky")
    f0, _ = orc.fit_fmap_trust_exact(f_init, Sinv0, m, th[0], gtol=1e-9)
    post = eng.posterior(X, th, "SE_kernel", eng.pd_inverse(eng.gram(X, th, "SE_kernel")), f0, m)
    rng = np.random.default_rng(B * G + m)
    al = np.sort(rng.random(G))
    xis = np.zeros((B, D)); xis[np.arange(B), rng.integers(0, D, B)] = 1.0
    xs = rng.random((B, D)) * (xis == 0)
    grid = al[None, :, None] * xis[:, None, :] + xs[:, None, :]
    z = rng.standard_normal((150, G))
    sf2 = th[2] ** 2
    mu_all = host(eng.predict(post, grid.reshape(-1, D), want_var=False, want_best=False)["mu"])
    mustar, jit = float(mu_all.max()) - 0.05, 1e-9 * sf2
    ei, vm = eng.line_acq(post, grid, z, mustar, jitter=jit)
    ei2, vm2 = eng.line_acq_xi(post, xis, xs, al, z, mustar, jitter=jit)
    assert np.array_equal(host(ei), host(ei2)) and np.array_equal(host(vm), host(vm2))
    ei, vm = host(ei), host(vm)
    P0 = orc.posterior_covariance(Sinv0, f0, m, th[0])
    A0 = orc.variance_operator(Sinv0, P0, faithful=False, lam=orc.lambda_dense(f0, m, th[0]))
    for b in sorted(set([0, B // 2, B - 1])):
        mu_b, cov_b = eng.predict_cov(post, grid[b])
        Ks = orc.cross_cov(X, grid[b], th, "SE_kernel")
        cov0 = orc.gram(grid[b], th, "SE_kernel") - Ks.T @ A0 @ Ks      # the reference's Sigma_pred (gp_model.py:441-452)
        assert np.abs(host(cov_b) - cov0).max() <= 1e-7 * sf2
        e0 = orc.line_ei(host(mu_b), host(cov_b), z, mustar, jitter=jit)
        v0 = orc.line_varmax(host(mu_b), host(cov_b), z, jitter=jit)
        assert abs(ei[b] - e0) <= 1e-6 * max(abs(e0), 1e-3 * np.sqrt(sf2)), (b, ei[b], e0)
        assert abs(vm[b] - v0) <= 1e-5 * max(abs(v0), 1e-6 * sf2), (b, vm[b], v0)


@pytest.mark.parametrize("D", [1, 11, 13, 17, 23, 24, 30, 33, 47, 48, 50, 64])
@pytest.mark.parametrize("kernel", ["SE_kernel", "RQ_kernel"])
def test_every_dimension_bucket(eng, D, kernel):
    """The kernels are specialised on the padded dimension (4 .. 64 in nine buckets for Gram / K* / RFF): one small
    end-to-end check per bucket edge against the oracle -- Gram, cross-covariance, posterior mean / variance of a
    Laplace posterior, the analytic mean gradient and the RFF features."""
    m, n_q = 5, 9
    th = [0.2, 0.3 * np.sqrt(D), 0.5]            # length scale grows with sqrt(D) so that the kernel does not vanish
    X = orc.synthetic_design(n_q, D, m=m, seed=D)
    N = X.shape[0]
    S0 = orc.gram(X, th, kernel)
    assert rel(host(eng.gram(X, th, kernel)), S0) < 1e-12
    Xc = np.random.default_rng(D).random((130, D))
    assert rel(host(eng.cross_cov(X, Xc, th, kernel)), orc.cross_cov(X, Xc, th, kernel)) < 1e-12
    Sinv0 = orc.pd_inverse(S0)
    f_init = np.random.default_rng(2).multivariate_normal(np.zeros(N), S0, method="cholesky")
    f0, _ = orc.fit_fmap_trust_exact(f_init, Sinv0, m, th[0], gtol=1e-9)
    Sinv = eng.pd_inverse(eng.gram(X, th, kernel))
    post = eng.posterior(X, th, kernel, Sinv, f0, m)
    P0 = orc.posterior_covariance(Sinv0, f0, m, th[0])
    A0 = orc.variance_operator(Sinv0, P0, faithful=False, lam=orc.lambda_dense(f0, m, th[0]))
    mu0, var0 = orc.predict_mean_var(Xc, X, th, Sinv0 @ f0, A0, kernel)
    out = eng.predict(post, Xc)
    assert rel(host(out["mu"]), mu0) < 1e-7
    assert np.abs(host(out["var"]) - var0).max() <= 1e-7 * th[2] ** 2
    o32 = eng.predict(post, Xc, want_best=False, kstar_fp32=True)      # the fp32-K* report path: buckets 6 / 20 / 64
    assert np.abs(host(o32["mu"]) - mu0).max() <= 1e-3 * np.abs(mu0).max()
    assert np.abs(host(o32["var"]) - var0).max() <= 1e-2 * th[2] ** 2
    mu_g, grad = eng.mean_grad(post, Xc[:17])
    mu1, g1 = orc.mean_grad(Xc[:17], X, th, Sinv0 @ f0, kernel)
    assert rel(host(mu_g), mu1) < 1e-7
    assert np.abs(host(grad) - g1).max() <= 1e-7 * max(np.abs(g1).max(), 1e-12)
    if kernel == "SE_kernel":
        F = 70
        W = np.random.default_rng(3).standard_normal((F, D)) / th[1]
        b = np.random.default_rng(4).uniform(0, 2 * np.pi, F)
        assert np.abs(host(eng.rff_project(X, W, b, th[2])) - orc.rff_features(X, W, b, th[2])).max() <= 1e-12


@pytest.mark.parametrize("m", [1, 3, 7, 15, 31, 63, 127])
def test_variance_contraction_fast_path_star_sizes(eng, m):
    """N = 256 and M = 256 are whole tiles, so the variance contraction takes the lean (aligned, in-bounds) main loop
    with its per-wavefront K limit at every star size m + 1 that divides the 128-row tile: mean and variance against
    the oracle's dense operator."""
    D = 3
    n_q = 256 // (m + 1)
    th = [0.3, 0.6, 0.8]
    X = orc.synthetic_design(n_q, D, m=m, seed=m)
    N = X.shape[0]
    assert N == 256
    S0 = orc.gram(X, th, "SE_kernel")
    Sinv0 = orc.pd_inverse(S0)
    f_init = np.random.default_rng(m).multivariate_normal(np.zeros(N), S0, method="cholesky")
    f0, _ = orc.fit_fmap_trust_exact(f_init, Sinv0, m, th[0], gtol=1e-9)
    post = eng.posterior(X, th, "SE_kernel", eng.pd_inverse(eng.gram(X, th, "SE_kernel")), f0, m)
    P0 = orc.posterior_covariance(Sinv0, f0, m, th[0])
    A0 = orc.variance_operator(Sinv0, P0, faithful=False, lam=orc.lambda_dense(f0, m, th[0]))
    Xc = np.random.default_rng(100 + m).random((256, D))
    mu0, var0 = orc.predict_mean_var(Xc, X, th, Sinv0 @ f0, A0, "SE_kernel")
    out = eng.predict(post, Xc)
    assert rel(host(out["mu"]), mu0) < 1e-7
    assert np.abs(host(out["var"]) - var0).max() <= 1e-7 * th[2] ** 2


@pytest.mark.parametrize("m,n_q,M", [(25, 5, 100), (25, 10, 257), (25, 21, 1000), (9, 13, 129), (2, 43, 128), (30, 9, 640),
                                     (25, 40, 1111), (40, 7, 300), (12, 20, 4097), (25, 10, 2500), (9, 13, 2048), (25, 3, 2049)])
def test_variance_contraction_ragged_shapes(eng, m, n_q, M):
    """Star sizes that divide neither the 16-deep chunk nor the 128-row tile (m = 25 is the reference's default,
    src/ppbo_settings.py:14: N = 26 n_q), N off every tile edge, candidate counts off the 128-column tile: the
    quadratic form then runs on a zero-framed copy of G with K* padded to whole tiles (predict_passes) so that every
    workgroup takes the unguarded loop.  Mean, variance, score and the argmax against the oracle's dense operator."""
    D = 4
    th = [0.3, 0.6, 0.8]
    X = orc.synthetic_design(n_q, D, m=m, seed=100 * m + n_q)
    N = X.shape[0]
    assert N == n_q * (m + 1)
    S0 = orc.gram(X, th, "SE_kernel")
    Sinv0 = orc.pd_inverse(S0)
    f_init = np.random.default_rng(m).multivariate_normal(np.zeros(N), S0, method="cholesky")
    f0, _ = orc.fit_fmap_trust_exact(f_init, Sinv0, m, th[0], gtol=1e-9)
    post = eng.posterior(X, th, "SE_kernel", eng.pd_inverse(eng.gram(X, th, "SE_kernel")), f0, m)
    P0 = orc.posterior_covariance(Sinv0, f0, m, th[0])
    A0 = orc.variance_operator(Sinv0, P0, faithful=False, lam=orc.lambda_dense(f0, m, th[0]))
    Xc = np.random.default_rng(100 + m).random((M, D))
    mu0, var0 = orc.predict_mean_var(Xc, X, th, Sinv0 @ f0, A0, "SE_kernel")
    mustar = float(np.max(mu0)) - 0.1
    out = eng.predict(post, Xc, score=1, mustar=mustar, want_score=True)      # PPBO_SCORE_POINTWISE_EI
    assert rel(host(out["mu"]), mu0) < 1e-7
    assert np.abs(host(out["var"]) - var0).max() <= 1e-7 * th[2] ** 2
    sc = host(out["score"])
    assert out["best_idx"] == int(np.argmax(sc)) and out["best_val"] == sc[out["best_idx"]]
    sc0 = orc.pointwise_ei(mu0, var0, mustar)
    assert np.abs(sc - sc0).max() <= 1e-6 * max(np.abs(sc0).max(), 1e-12)
    # the same candidates in two calls of other lengths (other padding, other tile counts): the same bits
    k = M // 2 + 1
    a, b = eng.predict(post, Xc[:k], want_best=False), eng.predict(post, Xc[k:], want_best=False)
    assert np.array_equal(np.concatenate([host(a["var"]), host(b["var"])]), host(out["var"]))
    assert np.array_equal(np.concatenate([host(a["mu"]), host(b["mu"])]), host(out["mu"]))


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 256, 320, 449, 512, 650, 1031, 2048, 2500, 2816, 3000])
def test_factor_triangular_inverse_and_inverse_together(eng, N):
    """ppbo_pd_inverse_ex hands back L, L^-1 and A^-1 from ONE enqueue (factorization, recursive-doubling triangular
    inverse, L^-T L^-1; the info word is read once at the end).  Checked entry by entry: L^-1 L = I, zeros above the
    diagonal, A^-1 = L^-T L^-1; ragged last blocks and 1, 2, 3, 4 blocks included; a failed factorization is reported
    with its leading minor and leaves the ctx usable."""
    rng = np.random.default_rng(N)
    Q = rng.standard_normal((N, N))
    A = Q @ Q.T + N * np.eye(N)
    Ai, Li, L = eng.pd_inverse_factors3(A)
    Ai, Li, L = host(Ai), host(Li), np.tril(host(L))
    assert rel(L, np.linalg.cholesky(A)) < 1e-12
    assert np.array_equal(np.triu(Li, 1), np.zeros_like(Li))
    assert np.abs(Li @ L - np.eye(N)).max() < 1e-11
    assert rel(Li, np.linalg.inv(np.linalg.cholesky(A))) < 1e-11
    assert np.abs(Ai - Li.T @ Li).max() <= 1e-12 * np.abs(Ai).max()
    # a matrix that is not positive definite: the call says so (and which leading minor), whatever the inverse roles did
    if N >= 3:
        B = A.copy()
        bad = max(1, (2 * N) // 3)
        B[bad, bad] = -1.0
        from ppbo_amd.engine import NotPositiveDefinite
        with pytest.raises(NotPositiveDefinite) as ei:
            eng.pd_inverse_factors3(B)
        assert ei.value.info == bad + 1
    # and the next call on the same ctx is unaffected
    Ai2 = host(eng.pd_inverse(A))
    assert np.array_equal(Ai2, Ai)


@pytest.mark.parametrize("name", [n for n in ("smoke", "c2", "c3") if n in ALL])
@pytest.mark.parametrize("per_line", [False, True])
def test_line_acq_xi_forms_the_grid_on_the_device(eng, golden, name, per_line):
    """ppbo_line_acq_xi(xi, x, alpha) = ppbo_line_acq on the grid alpha * xi + x built by the host
    (FeedbackProcessing.xi_grid with is_scaled, src/feedback_processing.py:57-107): same bits, with one abscissa
    vector shared by all lines and with one per line; more lines than one chunk of 512 included."""
    g = golden(name)
    post, _ = _posterior(eng, g)
    D = int(g["D"])
    rng = np.random.default_rng(7)
    B, G, S = (700 if name == "smoke" else 96), 70, 64
    xis = rng.random((B, D)) * (rng.random((B, D)) < 0.5)
    xis[np.arange(B), rng.integers(0, D, B)] = 1.0
    xs = rng.random((B, D)) * (xis == 0)
    base = np.linspace(0.005, 0.995, G)
    alphas = np.sort(np.clip(base + rng.normal(0, 0.01, (B, G) if per_line else G), 0.0, 1.0), axis=-1)
    grid = (alphas[:, :, None] if per_line else alphas[None, :, None]) * xis[:, None, :] + xs[:, None, :]
    z = rng.standard_normal((S, G))
    mustar = float(np.max(g["mu"]))
    jit = 1e-10 * float(g["theta"][2]) ** 2
    ei0, vm0 = eng.line_acq(post, grid, z, mustar, jitter=jit)
    ei1, vm1 = eng.line_acq_xi(post, xis, xs, alphas, z, mustar, jitter=jit)
    assert np.array_equal(host(ei0), host(ei1)) and np.array_equal(host(vm0), host(vm1))
    with pytest.raises(ValueError):
        eng.line_acq_xi(post, xis, xs[:-1], alphas, z, mustar)
