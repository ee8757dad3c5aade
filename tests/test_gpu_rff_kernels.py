"""GPU: Hsampler with the RQ and camphor-copper bases -- Phi(X) on the device against the NumPy form, the weight-space
terms and omega_MAP against the oracle, the maximiser of one sample (ppbo_rff_search: for RQ as it is, with the camphor
coordinate map for the camphor kernels, in the caller's coordinates), its argument checks, and the C5 cycle with camphor features."""
import ctypes as C
import types

import numpy as np
import pytest
import scipy.optimize

from conftest import load_golden
from oracle import ppbo_oracle as orc

pytestmark = pytest.mark.gpu

CAM = "camphor_copper_ard_kernel"


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def eng():
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _case(name):
    """(X, theta, kernel, m, xstars_local) of a fixture; camphor_ard/spread as the per-coordinate kernel."""
    g = load_golden(name)
    if name == "camphor_ard/spread":
        th = [float(g["theta_sf"][0]), np.asarray(g["theta_l"], dtype=float), float(g["theta_sf"][1])]
        kern = CAM
    else:
        th = [float(v) for v in g["theta"]]
        kern = str(g["kernel"])
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


def _embedded(hs, X):
    from ppbo_amd.random_fourier_sampler import camphor_embed_host
    l = hs._camphor()
    return X if l is None else camphor_embed_host(X, l)


FIXTURES = ["rq", "cam_small", "camphor_ard/spread", "c5"]


@pytest.mark.parametrize("name", FIXTURES)
def test_phi_X_and_terms(eng, name):
    F = 512
    hs = _sampler(eng, name, F, 1)
    assert hs.W.shape == (F, 11 if name != "rq" else 4)
    hs.update_phi_X()
    Phi0 = orc.rff_features(_embedded(hs, hs.X), hs.W, hs.b.ravel(), hs.theta[2])
    assert np.abs(hs.phi_X - Phi0).max() <= 1e-10 * np.abs(Phi0).max()
    om = np.random.default_rng(2).standard_normal(F)
    S0, g0, h0 = orc.rff_terms(Phi0, om, hs.m, hs.theta[0])
    assert abs(hs.S(om, hs.theta) - S0) <= 1e-9 * abs(S0)
    assert np.abs(hs.S_grad(om, hs.theta) - g0).max() <= 1e-9 * np.abs(g0).max()
    assert np.abs(hs.S_hessian_diag(om, hs.theta) - h0).max() <= 1e-9 * np.abs(h0).max()
    if name == "c5":
        return                                   # the dense trust-exact oracle at N = 4096: covered at the small sizes
    np.random.seed(3)
    hs.update_omega_MAP()
    np.random.seed(3)
    om0 = np.random.randn(F)
    ref = orc.rff_omega_map(Phi0, om0, hs.m, hs.theta[0])
    _, gr, hr = orc.rff_terms(Phi0, ref, hs.m, hs.theta[0])
    gap = np.abs(gr / hr).max()                  # the oracle's own Newton gap at its stopping point
    assert np.abs(hs.omega_MAP - ref).max() <= 1e-4 * np.abs(ref).max() + 1.5 * gap


def test_rq_return_xstar_at_least_as_good_as_reference(eng):
    F = 1024
    hs = _sampler(eng, "rq", F, 4)
    hs.update_phi_X()
    om = np.random.default_rng(5).standard_normal(F)
    np.random.seed(6)
    xr, vr = orc.rff_return_xstar(hs.W, hs.b.ravel(), hs.theta[2], om, hs.GP_xstars_local)
    np.random.seed(7)
    xs = hs.return_xstar(om)
    assert xs.shape == (4,) and np.all((xs >= 0) & (xs <= 1))
    val = float(hs.phi(xs) @ om)
    assert val >= vr - 1e-6 * abs(vr), (val, vr)


def _scipy_multistart(hs, om, n=16, seed=0):
    """L-BFGS-B on -phi(x)^T omega in the caller's box from the perturbed local maxima and uniform starts."""
    rng = np.random.default_rng(seed)
    loc = np.atleast_2d(hs.GP_xstars_local)
    starts = [np.clip(p + 0.01 * rng.random(6), 0, 1) for p in loc] + list(rng.random((n - len(loc), 6)))
    best = -np.inf
    for x0 in starts:
        r = scipy.optimize.minimize(lambda x: -float(hs.phi(x) @ om), x0, jac=lambda x: -(hs.Dphi(x).T @ om),
                                    method="L-BFGS-B", bounds=((0, 1),) * 6, options={"maxiter": 5000})
        best = max(best, float(hs.phi(np.clip(r.x, 0, 1)) @ om))
    return best


@pytest.mark.parametrize("name", ["cam_small", "camphor_ard/spread", "c5"])
def test_camphor_return_xstar(eng, name):
    F = 1024
    hs = _sampler(eng, name, F, 8)
    hs.update_phi_X()
    om = np.random.default_rng(9).standard_normal(F)
    np.random.seed(10)
    xs = hs.return_xstar(om)
    assert xs.shape == (6,) and np.all((xs >= 0) & (xs <= 1))
    val = float(hs.phi(xs) @ om)
    ref = _scipy_multistart(hs, om)
    assert val >= ref - 1e-6 * abs(ref), (val, ref)
    # the entry point itself: every refined maximum in the box, its value phi(x)^T omega as the host computes it
    cand = np.random.default_rng(11).random((8192, 6))
    x, v = eng.rff_search_camphor(cand, hs._camphor(), hs.W, hs.b.ravel(), hs.theta[2], om, K=16, iters=100)
    assert len(v) > 0 and np.all((x >= 0) & (x <= 1))
    for xi, vi in zip(x, v):
        assert abs(float(hs.phi(xi) @ om) - vi) <= 1e-12 * abs(vi)
    # the screen and the ascent agree: no refined value below the best screened candidate's
    sc, _, _ = hs.score_candidates(cand, om)
    assert np.abs(sc - orc.rff_score(_embedded(hs, cand), hs.W, hs.b.ravel(), hs.theta[2], om)).max() <= 1e-9 * np.abs(sc).max()
    assert v.max() >= sc.max() - 1e-12 * abs(sc.max())


@pytest.mark.parametrize("name", ["cam_small", "camphor_ard/spread"])
def test_camphor_return_xstar_for_dim(eng, name):
    F = 512
    hs = _sampler(eng, name, F, 12)
    om = np.random.default_rng(13).standard_normal(F)
    x_ref = np.random.default_rng(14).random(6)
    for dim in range(1, 7):
        xo = hs.return_xstar_for_dim(om, dim, x_ref.copy())
        others = [d for d in range(6) if d != dim - 1]
        assert np.array_equal(xo[others], x_ref[others]) and 0.0 <= xo[dim - 1] <= 1.0
        grid = np.tile(x_ref, (4096, 1))
        grid[:, dim - 1] = np.linspace(0, 1, 4096)
        vals = orc.rff_score(_embedded(hs, grid), hs.W, hs.b.ravel(), hs.theta[2], om)
        assert float(hs.phi(xo) @ om) >= vals.max() - 1e-9 * np.abs(vals).max()


def test_rff_search_camphor_rejects_bad_arguments(eng):
    from ppbo_amd import _lib
    F, M = 64, 256
    rng = np.random.default_rng(15)
    cand, W, b, om = eng.dev(rng.random((M, 6))), eng.dev(rng.standard_normal((F, 11))), eng.dev(rng.random(F)), eng.dev(rng.standard_normal(F))
    xs, vals = eng.empty(1025, 6), eng.empty(1025)
    found = C.c_int(0)
    dp = C.POINTER(C.c_double)
    good = np.array([0.3, 0.3, 0.35, 0.3, 0.3, 0.3])

    def call(l=good, cand_p=cand, W_p=W, K=8, x_p=xs):
        co = _lib.Coords(_lib.COORDS_CAMPHOR, l.ctypes.data_as(dp) if l is not None else None, None)
        p = (lambda t: None if t is None else C.c_void_p(t.data_ptr()))
        return eng.lib.ppbo_rff_search(eng.ctx, p(cand_p), M, 6, p(W_p), F, p(b), 0.5, p(om), co, K, 0.05, 10, 1e-10,
                                       p(x_p), p(vals), C.byref(found), eng._stream())

    assert call() == 0 and 0 < found.value <= 8
    for bad in (np.array([0.3, 0.3, -0.1, 0.3, 0.3, 0.3]), np.array([0.3, np.nan, 0.3, 0.3, 0.3, 0.3]),
                np.array([0.3, 0.3, 0.3, 0.3, 0.3, 0.0]), None):
        assert call(l=bad) != 0
        assert "invalid argument" in eng._err()
    for kw in (dict(cand_p=None), dict(W_p=None), dict(x_p=None), dict(K=0), dict(K=1025)):
        assert call(**kw) != 0, kw
        assert "invalid argument" in eng._err()
    assert call() == 0                           # the context is still usable


def test_c5_camphor_features_full_cycle(eng):
    """Config 5's 8192 RFF with the camphor basis: basis, Phi(X), omega_MAP, covariance and sample_xstar."""
    F = 8192
    hs = _sampler(eng, "c5", F, 16)
    assert hs.W.shape == (F, 11)
    hs.update_phi_X()
    c = 64
    Phi0 = orc.rff_features(_embedded(hs, hs.X[:c]), hs.W, hs.b.ravel(), hs.theta[2])
    assert np.abs(hs.phi_X[:, :c] - Phi0).max() <= 1e-10 * np.abs(Phi0).max()
    np.random.seed(17)
    hs.update_omega_MAP()
    assert np.all(np.isfinite(hs.omega_MAP)) and np.isfinite(hs.omega_MAP_stats["S"])
    hs.update_covariancematrix()
    assert hs.cov_diag is not None and np.all(hs.cov_diag > 0)
    xs = hs.sample_xstar()
    assert xs.shape == (6,) and np.all((xs >= 0) & (xs <= 1)) and np.all(np.isfinite(xs))
