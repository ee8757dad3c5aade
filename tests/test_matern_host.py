"""CPU: the Matern-5/2 and Matern-3/2 kernels -- the NumPy statement every GPU test compares against, its gradient,
the fixtures under tests/golden/matern/, name resolution through every layer, and the Student-t spectral draw of the
random-Fourier-feature basis.  No reference counterpart: GPy / scikit-learn Matern(nu)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from oracle import ppbo_oracle as orc

NU = {"Matern52_kernel": 2.5, "Matern32_kernel": 1.5}
FIXTURES = ["matern/m52_small", "matern/m32_small", "matern/m52_c2"]


def matern(X1, X2, theta, kernel):
    """k(x, x') from direct differences: a = sqrt(2 nu) r / l."""
    X1, X2 = np.atleast_2d(X1), np.atleast_2d(X2)
    r = np.sqrt(((X1[:, None, :] - X2[None, :, :]) ** 2).sum(-1))
    a = np.sqrt(2.0 * NU[kernel]) * r / theta[1]
    poly = 1.0 + a + a * a / 3.0 if kernel == "Matern52_kernel" else 1.0 + a
    return theta[2] ** 2 * poly * np.exp(-a)


def matern_grad(x, X, theta, kernel):
    """d k(x, X_i) / d x  [N, D]: -sf^2 (c^2/3) (1 + a) e^-a (x - X_i) for 5/2, -sf^2 c^2 e^-a (x - X_i) for 3/2."""
    diff = x[None, :] - X
    c = np.sqrt(2.0 * NU[kernel]) / theta[1]
    a = c * np.sqrt((diff ** 2).sum(-1))
    e = np.exp(-a)
    fac = -(theta[2] ** 2) * (c * c / 3.0) * (1.0 + a) * e if kernel == "Matern52_kernel" else -(theta[2] ** 2) * c * c * e
    return fac[:, None] * diff


@pytest.mark.parametrize("kernel", list(NU))
@pytest.mark.parametrize("D", [1, 3, 7])
def test_value_against_sklearn(kernel, D):
    kern = pytest.importorskip("sklearn.gaussian_process.kernels")
    rng = np.random.default_rng(D)
    X1, X2 = rng.random((23, D)), rng.random((19, D))
    X2[0] = X1[0]                                   # r = 0 included
    th = [0.05, 0.31, 0.7]
    ref = th[2] ** 2 * kern.Matern(length_scale=th[1], nu=NU[kernel])(X1, X2)
    assert np.abs(matern(X1, X2, th, kernel) - ref).max() <= 1e-13 * th[2] ** 2


@pytest.mark.parametrize("kernel", list(NU))
def test_gradient_against_central_differences(kernel):
    rng = np.random.default_rng(3)
    D = 4
    X = rng.random((30, D))
    th = [0.05, 0.42, 1.3]
    for x in (rng.random(D), X[5] + 1e-3 * rng.standard_normal(D)):
        g = matern_grad(x, X, th, kernel)
        h = 1e-6
        for d in range(D):
            e = np.zeros(D)
            e[d] = h
            fd = (matern(x + e, X, th, kernel) - matern(x - e, X, th, kernel))[0] / (2 * h)
            assert np.abs(g[:, d] - fd).max() <= 1e-7 * th[2] ** 2 / th[1] ** 2
    # finite at r = 0, and zero there
    assert np.all(matern_grad(X[0], X, th, kernel)[0] == 0.0)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_sigma_matches_closed_form(name):
    g = load_golden(name)
    kernel = str(g["kernel"])
    K = matern(g["X"], g["X"], g["theta"], kernel)
    S = orc.regularize_covariance(K, orc.SHRINKAGE)
    sf2 = float(g["theta"][2]) ** 2
    # the fixtures were built with the reference's expansion-form r^2: entries agree to its rounding
    assert np.abs(S[g["Sigma_ii"], g["Sigma_jj"]] - g["Sigma_samples"]).max() <= 1e-12 * sf2
    c = g["Sigma_corner"].shape[0]
    assert np.abs(S[:c, :c] - g["Sigma_corner"]).max() <= 1e-12 * sf2
    assert np.abs(matern(g["X"], g["X"][:c], g["theta"], kernel) - g["Kraw_cols"]).max() <= 1e-12 * sf2


def test_names_resolve_through_every_layer():
    from ppbo_amd import _lib, kernels
    from ppbo_amd.ppbo_settings import PPBO_settings
    assert _lib.KERNEL_IDS["Matern52_kernel"] == 3 and _lib.KERNEL_IDS["Matern32_kernel"] == 4
    # the ids are the header's
    hdr = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert int(re.search(r"PPBO_KERNEL_MATERN52\s*=\s*(\d+)", hdr).group(1)) == 3
    assert int(re.search(r"PPBO_KERNEL_MATERN32\s*=\s*(\d+)", hdr).group(1)) == 4
    for name in NU:
        fn = kernels.BY_NAME[name]
        assert fn.__name__ == name
        st = PPBO_settings(D=3, bounds=((0, 1),) * 3, xi_acquisition_function="PCD", kernel=name, verbose=False)
        assert st.kernel == name and kernels.BY_NAME[st.kernel] is fn


@pytest.mark.parametrize("kernel", list(NU))
def test_student_t_draw_second_moment(kernel):
    from ppbo_amd.random_fourier_sampler import matern_spectral_draw
    nu, D, l, F = NU[kernel], 5, 0.3, 400000
    W = matern_spectral_draw(F, D, l, nu, rng=np.random.default_rng(1))
    assert W.shape == (F, D)
    sq = (W ** 2).sum(1)
    if nu > 2:     # |w|^2 has a finite variance when 2 nu > 4: a 5-sigma bound on the mean
        want = D * (2 * nu / (2 * nu - 2)) / l ** 2
        assert abs(sq.mean() - want) <= 5 * sq.std() / np.sqrt(F)
    else:          # nu = 3/2: E|w|^2 is finite but |w|^2 has no variance; hold the mean loosely
        want = D * (2 * nu / (2 * nu - 2)) / l ** 2
        assert abs(sq.mean() - want) <= 0.1 * want


@pytest.mark.parametrize("kernel", list(NU))
def test_cosine_basis_approaches_the_kernel(kernel):
    from ppbo_amd.random_fourier_sampler import matern_spectral_draw
    rng = np.random.default_rng(7)
    F, D = 2 ** 16, 3
    th = [0.05, 0.35, 0.8]
    W = matern_spectral_draw(F, D, th[1], NU[kernel], rng=rng)
    b = rng.uniform(0, 2 * np.pi, F)
    X = rng.random((12, D))
    Phi = np.sqrt(2 * th[2] ** 2 / F) * np.cos(W @ X.T + b[:, None])     # [F, N], the Hsampler basis
    err = np.abs(Phi.T @ Phi - matern(X, X, th, kernel)).max()
    assert err <= 5 * th[2] ** 2 * np.sqrt(2 / F), err


def test_se_basis_draw_order_unchanged():
    """The SE branch of generate_basis draws W then b from the global stream exactly as before."""
    from ppbo_amd.random_fourier_sampler import Hsampler
    hs = Hsampler.__new__(Hsampler)
    hs.kernel, hs.nFeatures, hs.D, hs.theta = "SE_kernel", 64, 3, [0.1, 0.4, 1.0]
    np.random.seed(5)
    hs.generate_basis()
    np.random.seed(5)
    W = np.random.randn(64, 3) / 0.4
    b = np.random.uniform(low=0, high=2 * np.pi, size=64)[:, None]
    assert np.array_equal(hs.W, W) and np.array_equal(hs.b, b)
