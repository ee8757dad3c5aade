"""GPU: batches of posterior maximiser samples -- ppbo_rff_score_multi against the oracle column by column (all three D
buckets, ragged sizes, phases beyond the fast cosine's range, bitwise repeatable), ppbo_rff_search_multi sample by
sample against the host value, the screen and the single-sample search, Hsampler.sample_xstars for every kernel against
return_xstar and an L-BFGS-B reference, the device draws of omega, the refusals, and the full C5 size."""
import ctypes as C
import types

import numpy as np
import pytest
import scipy.optimize
import torch

from conftest import load_golden
from oracle import ppbo_oracle as orc

pytestmark = pytest.mark.gpu

CAP = 1024                       # PPBO_RFF_MULTI_MAX_S


@pytest.fixture(scope="module")
def eng():
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _case(name):
    """(X, theta, kernel, m, xstars_local) of a fixture; 'matern52' and 'ard_se' are the rq design under those kernels."""
    base = {"matern52": "rq", "ard_se": "rq"}.get(name, name)
    g = load_golden(base)
    if base == "camphor_ard/spread":
        th = [float(g["theta_sf"][0]), np.asarray(g["theta_l"], dtype=float), float(g["theta_sf"][1])]
        kern = "camphor_copper_ard_kernel"
    else:
        th = [float(v) for v in g["theta"]]
        kern = str(g["kernel"])
    if name == "matern52":
        kern = "Matern52_kernel"
    elif name == "ard_se":
        kern = "SE_kernel"
        th[1] = np.array([0.2, 0.35, 0.5, 0.8])
    loc = g["Xc"][np.argsort(g["mu"])[-4:]]
    return g["X"], th, kern, int(g["m"]), loc


def _sampler(eng, name, F, seed):
    from ppbo_amd.random_fourier_sampler import Hsampler
    X, th, kern, m, loc = _case(name)
    N, D = X.shape
    gp = types.SimpleNamespace(eng=eng, D=D, m=m, X=X, xstar=loc[-1], xstars_local=loc, n_gausshermite_sample_points=None,
                               obs_indices=np.arange(0, N, m + 1), kernel=types.SimpleNamespace(__name__=kern), theta=th)
    hs = Hsampler(gp, F)
    np.random.seed(seed)
    hs.generate_basis()
    return hs


def _oracle_scores(Xc, W, b, sf, Om, chunk=4096):
    """orc.rff_score for every column of Omega^T at once, in candidate chunks: [S, M]."""
    out = np.empty((Om.shape[0], Xc.shape[0]))
    for c0 in range(0, Xc.shape[0], chunk):
        out[:, c0:c0 + chunk] = orc.rff_score(Xc[c0:c0 + chunk], W, b, sf, Om.T).T
    return out


# ---------------------------------------------------------------- 1. the multi-score kernel
@pytest.mark.parametrize("D", [6, 20, 40])
@pytest.mark.parametrize("S,F", [(1, 1000), (17, 4096), (256, 4096)])
def test_score_multi_matches_oracle(eng, D, S, F):
    rng = np.random.default_rng(100 * D + S)
    M = 65536 + 123
    Xc, W, b = rng.random((M, D)), rng.standard_normal((F, D)) / 0.3, rng.uniform(0, 2 * np.pi, F)
    Om = rng.standard_normal((S, F))
    sc = eng.rff_score_multi(Xc, W, b, 0.7, Om)
    assert tuple(sc.shape) == (S, M)
    got = sc.cpu().numpy()
    want = _oracle_scores(Xc, W, b, 0.7, Om)
    assert np.all(np.abs(got - want).max(axis=1) <= 1e-9 * np.abs(want).max(axis=1)), np.abs(got - want).max()
    # one fixed summation order: a second call is bitwise equal
    assert torch.equal(sc, eng.rff_score_multi(Xc, W, b, 0.7, Om))


def test_score_multi_large_phases(eng):
    """Rows of W scaled so that some phases exceed RFF_COS_FAST_RANGE (1.6e6): the library cosine takes them."""
    rng = np.random.default_rng(7)
    M, D, F, S = 4096 + 17, 6, 1000, 19
    Xc, W, b = rng.random((M, D)), rng.standard_normal((F, D)), rng.uniform(0, 2 * np.pi, F)
    W[::7] *= 2e6
    ph = Xc @ W.T + b
    assert (np.abs(ph) >= 1.6e6).any()
    Om = rng.standard_normal((S, F))
    got = eng.rff_score_multi(Xc, W, b, 0.5, Om).cpu().numpy()
    want = _oracle_scores(Xc, W, b, 0.5, Om)
    assert np.all(np.abs(got - want).max(axis=1) <= 1e-9 * np.abs(want).max(axis=1)), np.abs(got - want).max()


# ---------------------------------------------------------------- 2. the batched search, sample by sample
@pytest.mark.parametrize("D", [6, 20])
@pytest.mark.parametrize("S", [1, 33])
def test_search_multi_per_sample(eng, D, S):
    rng = np.random.default_rng(10 * D + S)
    M, F, K, sf = 8192 + 5, 1024, 16, 0.6
    cand, W, b = rng.random((M, D)), rng.standard_normal((F, D)) / 0.3, rng.uniform(0, 2 * np.pi, F)
    Om = rng.standard_normal((S, F))
    x, v, found = eng.rff_search_multi(cand, W, b, sf, Om, K=K, iters=100)
    assert x.shape == (S, K, D) and v.shape == (S, K) and found.shape == (S,)
    sc = eng.rff_score_multi(cand, W, b, sf, Om).cpu().numpy()
    amp = np.sqrt(2.0 * sf ** 2 / F)
    for k in range(S):
        n = int(found[k])
        assert 1 <= n <= K
        assert np.all(v[k, n:] == -np.inf)
        xk, vk = x[k, :n], v[k, :n]
        assert np.all((xk >= 0) & (xk <= 1))
        host = amp * np.cos(xk @ W.T + b) @ Om[k]
        assert np.all(np.abs(host - vk) <= 1e-12 * np.abs(vk)), np.abs(host - vk).max()
        best = vk.max()
        assert best >= sc[k].max() - 1e-12 * abs(sc[k].max())
        _, v1 = eng.rff_search(cand, W, b, sf, Om[k], K=K, iters=100)
        assert best >= v1.max() - 1e-6 * abs(v1.max()), (k, best, v1.max())


# ---------------------------------------------------------------- 3. Hsampler.sample_xstars for every kernel
def _scipy_multistart(hs, om, n=16, seed=0):
    """L-BFGS-B on -phi(x)^T omega in the caller's box from the perturbed local maxima and uniform starts."""
    rng = np.random.default_rng(seed)
    loc = np.atleast_2d(hs.GP_xstars_local)
    D = loc.shape[1]
    starts = [np.clip(p + 0.01 * rng.random(D), 0, 1) for p in loc] + list(rng.random((n - len(loc), D)))
    best = -np.inf
    for x0 in starts:
        r = scipy.optimize.minimize(lambda x: -float(hs.phi(x) @ om), x0, jac=lambda x: -(hs.Dphi(x).T @ om),
                                    method="L-BFGS-B", bounds=((0, 1),) * D, options={"maxiter": 5000})
        best = max(best, float(hs.phi(np.clip(r.x, 0, 1)) @ om))
    return best


@pytest.mark.parametrize("name", ["c3", "matern52", "rq", "ard_se", "cam_small", "camphor_ard/spread"])
def test_sample_xstars_every_kernel(eng, name):
    F, n = 1024, 6
    hs = _sampler(eng, name, F, 20)
    camphor = hs._camphor() is not None
    Om = np.random.default_rng(21).standard_normal((n, F))
    hs._xstar_candidates()                      # the resident pool is drawn on first use: before the seeded calls
    np.random.seed(22)
    X, V = hs.sample_xstars(n, omegas=Om)
    Dout = 6 if camphor else hs.D
    assert X.shape == (n, Dout) and V.shape == (n,)
    assert np.all((X >= 0) & (X <= 1)) and np.all(np.isfinite(V))
    for k in range(n):
        assert abs(float(hs.phi(X[k]) @ Om[k]) - V[k]) <= 1e-12 * abs(V[k])
    for k in (0, n - 1):
        np.random.seed(22)                      # the same candidates as the batch
        xs = hs.return_xstar(Om[k])
        v1 = float(hs.phi(xs) @ Om[k])
        assert V[k] >= v1 - 1e-6 * abs(v1), (k, V[k], v1)
        if camphor:
            ref = _scipy_multistart(hs, Om[k])
        else:
            np.random.seed(23)
            _, ref = orc.rff_return_xstar(hs.W, hs.b.ravel(), hs.theta[2], Om[k], hs.GP_xstars_local)
        assert V[k] >= ref - 1e-6 * abs(ref), (k, V[k], ref)


# ---------------------------------------------------------------- 4. device draws of omega
def test_sample_omegas(eng):
    from ppbo_amd.random_fourier_sampler import omega_draws_host
    F, n = 512, 4096
    hs = _sampler(eng, "rq", F, 30)
    with pytest.raises(RuntimeError):
        hs.sample_omegas(4, seed=1)             # no covariance yet
    hs.update_phi_X()
    np.random.seed(31)
    hs.update_omega_MAP()
    hs.update_covariancematrix()
    assert hs.cov_diag is not None
    a, b2, c = hs.sample_omegas(n, seed=5), hs.sample_omegas(n, seed=5), hs.sample_omegas(n, seed=6)
    assert tuple(a.shape) == (n, F)
    assert torch.equal(a, b2) and not torch.equal(a, c)
    Om = a.cpu().numpy()
    z = eng.randn(5, n, F).cpu().numpy()        # the same normals: the draw is the host formula on them
    want = omega_draws_host(hs.omega_MAP, hs.cov_diag, z)
    assert np.all(np.abs(Om - want) <= 4e-16 * (np.abs(hs.omega_MAP) + np.sqrt(hs.cov_diag) * np.abs(z)))
    # mean and variance per feature within 5 standard errors: F = 512 features x 2 statistics = 1024 z bounds, each
    # exceeded with probability ~6e-7 for a normal statistic
    mean, var = Om.mean(axis=0), Om.var(axis=0, ddof=1)
    zm = (mean - hs.omega_MAP) / np.sqrt(hs.cov_diag / n)
    zv = (var - hs.cov_diag) / (hs.cov_diag * np.sqrt(2.0 / (n - 1)))
    assert np.abs(zm).max() <= 5.0 and np.abs(zv).max() <= 5.0, (np.abs(zm).max(), np.abs(zv).max())
    # seed=None draws the seed from NumPy's global stream
    np.random.seed(32)
    d1 = hs.sample_omegas(3)
    np.random.seed(32)
    assert torch.equal(d1, hs.sample_omegas(3))


# ---------------------------------------------------------------- 5. refusals
def test_multi_refusals(eng):
    from ppbo_amd import _lib
    rng = np.random.default_rng(40)
    M, D, F = 256, 6, 64
    cand, W, b, Om = rng.random((M, D)), rng.standard_normal((F, D)), rng.random(F), rng.standard_normal((3, F))
    for kw in (dict(omegas=np.zeros((0, F))), dict(omegas=np.zeros((CAP + 1, F))), dict(K=0), dict(K=1025),
               dict(omegas=rng.standard_normal((3, F + 1)))):
        args = dict(cand=cand, W=W, b=b, sigma_f=0.5, omegas=Om)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.rff_search_multi(**args)
    with pytest.raises(ValueError):
        eng.rff_search_multi(rng.random((M, 65)), rng.standard_normal((F, 65)), b, 0.5, Om)
    with pytest.raises(ValueError):
        eng.rff_score_multi(cand, W, b, 0.5, np.zeros((0, F)))
    with pytest.raises(ValueError):                     # a camphor basis is [F, 11]
        eng.rff_search_multi_camphor(cand, np.full(6, 0.3), W, b, 0.5, Om)
    # the C-ABI itself
    dc, dW, db, dO = eng.dev(cand), eng.dev(W), eng.dev(b), eng.dev(Om)
    xs, vals, fnd = eng.empty(4 * 1025 * 65), eng.empty(4 * 1025), torch.zeros(4, dtype=torch.int32, device=eng.device)
    sc = eng.empty(4 * M)
    p = (lambda t: None if t is None else C.c_void_p(t.data_ptr()))

    def search(S=3, K=8, Dv=D, cand_p=dc, x_p=xs, f_p=fnd):
        return eng.lib.ppbo_rff_search_multi(eng.ctx, p(cand_p), M, Dv, p(dW), F, p(db), 0.5, p(dO), None, S, K, 0.05, 10, 1e-10,
                                             p(x_p), p(vals), p(f_p), eng._stream())

    assert search() == 0
    for kw in (dict(S=0), dict(S=CAP + 1), dict(K=0), dict(K=1025), dict(Dv=65), dict(cand_p=None), dict(x_p=None),
               dict(f_p=None)):
        assert search(**kw) != 0, kw
        assert "invalid argument" in eng._err(), kw
    for S in (0, CAP + 1):
        assert eng.lib.ppbo_rff_score_multi(eng.ctx, p(dc), M, D, p(dW), F, p(db), 0.5, p(dO), S, p(sc), eng._stream()) != 0
        assert "invalid argument" in eng._err()
    l = np.full(6, 0.3)
    dp = C.POINTER(C.c_double)
    bad_l = np.array([0.3, 0.3, -0.1, 0.3, 0.3, 0.3])
    W11 = eng.dev(rng.standard_normal((F, 11)))
    for ll, S, K in ((bad_l, 3, 8), (l, 0, 8), (l, 3, 1025)):
        co = _lib.Coords(_lib.COORDS_CAMPHOR, ll.ctypes.data_as(dp), None)
        rc = eng.lib.ppbo_rff_search_multi(eng.ctx, p(dc), M, 6, p(W11), F, p(db), 0.5, p(dO), co, S, K, 0.05, 10, 1e-10,
                                           p(xs), p(vals), p(fnd), eng._stream())
        assert rc != 0 and "invalid argument" in eng._err()
    assert search() == 0                                # the context is still usable
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. full size and chunking
def test_c5_camphor_sample_xstars_256(eng):
    F = 8192
    hs = _sampler(eng, "c5", F, 50)
    hs.update_phi_X()
    np.random.seed(51)
    hs.update_omega_MAP()
    hs.update_covariancematrix()
    assert hs.cov_diag is not None
    np.random.seed(52)
    X, V = hs.sample_xstars(256)
    assert X.shape == (256, 6) and V.shape == (256,)
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(V)) and np.all((X >= 0) & (X <= 1))


def test_sample_xstars_chunks_over_the_cap(eng):
    F, n = 256, CAP + 5
    hs = _sampler(eng, "rq", F, 60)
    Om = np.random.default_rng(61).standard_normal((n, F))
    hs._xstar_candidates()                      # the resident pool is drawn on first use: before the seeded calls
    np.random.seed(62)
    X, V = hs.sample_xstars(n, omegas=Om, starts=4)
    assert X.shape == (n, 4) and V.shape == (n,) and np.all(np.isfinite(V))
    # the second chunk's rows are its own samples': a row of it matches a one-sample batch on the same candidates
    np.random.seed(62)
    X1, V1 = hs.sample_xstars(1, omegas=Om[n - 1:], starts=4)
    assert abs(V1[0] - V[n - 1]) <= 1e-9 * abs(V1[0])
