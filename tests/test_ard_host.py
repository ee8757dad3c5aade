"""CPU: per-dimension length scales (ARD) -- the three new entry points of the C-ABI, the one validation function of
theta[1], the RFF basis draws with a vector of length scales, and the length-scale prior summed over the dimensions.
No reference counterpart (GPy ARD=True, scikit-learn's anisotropic kernels)."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import scipy.stats

from conftest import ROOT

# what works in the caller's coordinates of an ARD model: the entries that read ppbo_model.coords (PPBO_COORDS_SCALED)
NEW = ("ppbo_scale_points", "ppbo_mean_search_multi", "ppbo_mean_ascent")
RADIAL = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")


def ard_closed_form(X1, X2, theta, kernel):
    """k(x, x') with r^2 = sum_d (x_d - x'_d)^2 / l_d^2 from direct differences, into each radial kernel's formula
    (RQ: alpha = 2, src/kernels.py:27-34; Matern: a = sqrt(2 nu) r)."""
    X1, X2 = np.atleast_2d(X1), np.atleast_2d(X2)
    l = np.broadcast_to(np.asarray(theta[1], dtype=float), (X1.shape[1],))
    r2 = (((X1[:, None, :] - X2[None, :, :]) / l) ** 2).sum(-1)
    sf2 = float(theta[2]) ** 2
    if kernel == "SE_kernel":
        return sf2 * np.exp(-0.5 * r2)
    if kernel == "RQ_kernel":
        return sf2 * (1.0 + r2 / 4.0) ** -2
    nu = 2.5 if kernel == "Matern52_kernel" else 1.5
    a = np.sqrt(2.0 * nu * r2)
    return sf2 * ((1.0 + a + a * a / 3.0) if nu == 2.5 else (1.0 + a)) * np.exp(-a)


def test_header_and_signatures_list_the_new_entry_points():
    from ppbo_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    for name in NEW:
        assert re.search(r"PPBO_API int " + name + r"\(", hdr), name
        assert name in _lib.SIGNATURES, name
    assert "no reference counterpart" in hdr
    assert _lib.ABI_VERSION == 9


def test_library_exports_the_new_entry_points():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libppbo_hip.so is not built (build() runs before the suite)")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert name in syms, name


@pytest.mark.parametrize("kernel", RADIAL)
def test_validation_accepts_scalar_and_vector(kernel):
    from ppbo_amd.engine import lengthscales
    assert lengthscales([0.1, 0.3, 1.0], 4, kernel) is None
    assert lengthscales([0.1, np.float64(0.3), 1.0], 4, kernel) is None
    v = lengthscales([0.1, [0.2, 0.2, 0.2, 0.2], 1.0], 4, kernel)
    assert isinstance(v, np.ndarray) and v.shape == (4,) and v.dtype == np.float64   # equal entries: still a vector


@pytest.mark.parametrize("bad, D, kernel", [
    ([0.5, 1.0, 2.0, 0.3, 0.1, 1.0], 6, "camphor_copper_kernel"),
    ([0.5, 1.0, 2.0], 4, "SE_kernel"),
    ([0.5, 1.0, 2.0, 0.3, 0.1], 4, "Matern52_kernel"),
    ([[0.5, 1.0], [2.0, 0.3]], 4, "SE_kernel"),
    ([0.5, 0.0, 2.0, 0.3], 4, "RQ_kernel"),
    ([0.5, -1.0, 2.0, 0.3], 4, "Matern32_kernel"),
    ([0.5, np.nan, 2.0, 0.3], 4, "SE_kernel"),
    ([0.5, np.inf, 2.0, 0.3], 4, "SE_kernel"),
])
def test_validation_rejects(bad, D, kernel):
    from ppbo_amd.engine import lengthscales
    with pytest.raises(ValueError):
        lengthscales([0.1, bad, 1.0], D, kernel)


def test_theta_key_holds_a_vector():
    from ppbo_amd.engine import theta_key
    assert theta_key([1, 0.5, 2]) == (1.0, 0.5, 2.0)
    k = theta_key([1, np.array([0.5, 0.25]), 2])
    assert k == (1.0, (0.5, 0.25), 2.0) and hash(k) == hash((1.0, (0.5, 0.25), 2.0))
    assert theta_key([1, np.array([0.5, 0.25]), 2]) != theta_key([1, np.array([0.5, 0.5]), 2])


def _sampler(kernel, theta, D, F):
    from ppbo_amd.random_fourier_sampler import Hsampler
    gp = types.SimpleNamespace(eng=object(), D=D, m=1, X=np.zeros((2, D)), xstar=None, xstars_local=None,
                               n_gausshermite_sample_points=0, obs_indices=[0], kernel=types.SimpleNamespace(__name__=kernel),
                               theta=theta)
    return Hsampler(gp, nFeatures=F)


def test_se_basis_column_spread_follows_one_over_l():
    l = np.array([0.05, 0.1, 0.4, 1.0, 2.5])
    np.random.seed(5)
    hs = _sampler("SE_kernel", [0.1, l, 1.0], len(l), 8192)
    hs.generate_basis()
    sd = hs.W.std(axis=0)
    assert np.all(np.abs(sd * l - 1.0) <= 0.05), sd * l


def test_matern_spectral_draw_column_spread_follows_one_over_l():
    from ppbo_amd.random_fourier_sampler import matern_spectral_draw
    l = np.array([0.05, 0.2, 0.7, 3.0])
    for nu in (2.5, 1.5):
        rng = np.random.RandomState(3)
        W = matern_spectral_draw(8192, len(l), l, nu, rng=rng)
        # the same draws with l = 1: column d of the ARD draw is exactly that column divided by l_d
        W1 = matern_spectral_draw(8192, len(l), 1.0, nu, rng=np.random.RandomState(3))
        assert np.allclose(W * l, W1, rtol=1e-15, atol=0)
        # per-column spread proportional to 1 / l_d: a robust scale (the Student-t tail at nu = 3/2 has no variance)
        iqr = np.subtract(*np.percentile(W, [75, 25], axis=0))
        ratio = iqr * l / np.mean(iqr * l)
        assert np.all(np.abs(ratio - 1.0) <= 0.05), ratio


def test_scalar_se_draw_order_unchanged():
    np.random.seed(17)
    hs = _sampler("SE_kernel", [0.1, 0.3, 1.0], 4, 64)
    hs.generate_basis()
    np.random.seed(17)
    W = np.random.randn(64, 4) / 0.3
    b = np.random.uniform(low=0, high=2 * np.pi, size=64)[:, None]
    assert np.array_equal(hs.W, W) and np.array_equal(hs.b, b)
    np.random.seed(17)
    hv = _sampler("SE_kernel", [0.1, np.full(4, 0.3), 1.0], 4, 64)
    hv.generate_basis()
    assert np.array_equal(hv.W, W) and np.array_equal(hv.b, b)       # the vector takes the same draws


def test_ard_prior_is_the_sum_over_dimensions():
    from ppbo_amd.gp_model import log_prior
    l = np.array([0.05, 0.2, 0.31, 1.4])
    th = [1.0, l, 0.8]
    lp0 = np.log(scipy.stats.lognorm.pdf(1.0, s=1, scale=np.exp(1)))
    lp2 = np.log(scipy.stats.lognorm.pdf(0.8, s=0.5, scale=np.exp(1.7)))
    per_dim = np.log(scipy.stats.lognorm.pdf(l, s=0.5, scale=np.exp(-1.4)))
    assert abs(log_prior(th) - (lp0 + per_dim.sum() + lp2)) <= 1e-12 * abs(log_prior(th))
    # a scalar l: the reference's three terms (src/gp_model.py:287-290), bit for bit
    ref = (np.log(scipy.stats.lognorm.pdf(1.0, s=1, scale=np.exp(1)))
           + np.log(scipy.stats.lognorm.pdf(0.31, s=0.5, scale=np.exp(-1.4)))
           + np.log(scipy.stats.lognorm.pdf(0.8, s=0.5, scale=np.exp(1.7))))
    assert log_prior([1.0, 0.31, 0.8]) == ref
    # equal entries: the scalar value plus (D - 1) log p(l)
    lpl = np.log(scipy.stats.lognorm.pdf(0.31, s=0.5, scale=np.exp(-1.4)))
    assert abs(log_prior([1.0, np.full(4, 0.31), 0.8]) - (ref + 3 * lpl)) <= 1e-12 * abs(ref)


def test_closed_form_against_sklearn():
    kern = pytest.importorskip("sklearn.gaussian_process.kernels")
    rng = np.random.default_rng(1)
    X1, X2 = rng.random((13, 5)), rng.random((9, 5))
    l = np.array([0.05, 0.3, 0.7, 1.1, 2.0])
    th = [0.1, l, 1.3]
    sf2 = th[2] ** 2
    assert np.abs(ard_closed_form(X1, X2, th, "SE_kernel") - sf2 * kern.RBF(l)(X1, X2)).max() <= 1e-14 * sf2
    for name, nu in (("Matern52_kernel", 2.5), ("Matern32_kernel", 1.5)):
        ref = sf2 * kern.Matern(l, nu=nu)(X1, X2)
        assert np.abs(ard_closed_form(X1, X2, th, name) - ref).max() <= 1e-13 * sf2
    # RQ with alpha = 2: sklearn's RationalQuadratic takes a scalar l; on l-scaled inputs it is the ARD form
    ref = sf2 * kern.RationalQuadratic(length_scale=1.0, alpha=2.0)(X1 / l, X2 / l)
    assert np.abs(ard_closed_form(X1, X2, th, "RQ_kernel") - ref).max() <= 1e-13 * sf2


def test_gpmodel_refuses_camphor_with_a_vector():
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    st = PPBO_settings(D=6, bounds=((0, 1),) * 6, xi_acquisition_function="PCD", kernel="camphor_copper_kernel",
                       theta_initial=[0.001, np.full(6, 0.26), 0.1], verbose=False)
    with pytest.raises(ValueError):
        GPModel(st, engine=object())
