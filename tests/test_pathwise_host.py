"""CPU: pathwise posterior samples -- the NumPy restatement (tests/pathwise_numpy.py) against itself, the oracle and central
differences; the public surface (header, ctypes prototypes, Engine / Hsampler attributes) and the refusals that are
decided on the host."""
import os
import re
import types

import numpy as np
import pytest

import pathwise_numpy as pw
from oracle import ppbo_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ppbo_path_score_multi", "ppbo_path_search_multi")


def _design():
    """The design of the first measurement: synthetic_design(12, 3, m=15, seed=1), SE, theta = [0.05, 0.3, 1.0]."""
    th, m = [0.05, 0.3, 1.0], 15
    X = orc.synthetic_design(12, 3, m=m, seed=1)
    Sinv = orc.pd_inverse(orc.gram(X, th))
    fmap = orc.fit_fmap_newton(np.random.RandomState(2).randn(X.shape[0]) * 0.1, Sinv, m, th[0])
    fmap = fmap[0] if isinstance(fmap, tuple) else fmap
    P = orc.posterior_covariance(Sinv, fmap, m, th[0])
    return X, th, m, Sinv, fmap, P


def _basis(F, D, l, seed):
    rs = np.random.RandomState(seed)
    return rs.randn(F, D) / l, rs.uniform(0, 2 * np.pi, F)


def test_closed_form_variance_tends_to_the_gp_posterior():
    """diag C (exact for a basis) against oracle.predict_mean_var's variance at 200 uniform points.  Measured ratio
    C_ii / var:  F = 2000: 0.905 .. 1.045 (worst |ratio - 1| 0.095);  F = 16000: 0.946 .. 1.012 (worst 0.054).  The gap
    is the RFF error of the prior, O(1 / sqrt(F)) (sqrt(8) = 2.8 between the two widths; measured 1.8 with one basis
    each): a property of the construction, not of the code.  Asserted: the NumPy GP mean and variance equal the
    oracle's, and the worst gap shrinks from F = 2000 to F = 16000."""
    X, th, m, Sinv, fmap, P = _design()
    Xq = np.random.RandomState(3).rand(200, 3)
    A = orc.variance_operator(Sinv, P, True)
    mu, var = orc.predict_mean_var(Xq, X, th, Sinv @ fmap, A)
    # two evaluations of k Sigma^-1 k (direct differences here, the oracle's expansion) agree to rounding on the sum of
    # absolute terms: Sigma^-1 has entries of 1e5 .. 1e6 that cancel to O(1)
    K, _ = pw.kernel_matrix(Xq, X, th, "SE_kernel")
    cancel = ((K @ np.abs(Sinv)) * K).sum(axis=1).max()
    assert np.abs(pw.gp_var(Xq, X, th, "SE_kernel", Sinv, P) - var).max() <= 1e-13 * cancel
    assert np.abs(pw.path_mean(Xq, X, th, "SE_kernel", Sinv, fmap) - mu).max() <= 1e-9 * np.abs(mu).max()
    gaps = {}
    for F in (2000, 16000):
        W, b = _basis(F, 3, th[1], 4)
        ratio = pw.path_var(Xq, W, b, X, th, "SE_kernel", Sinv, P) / var
        gaps[F] = np.abs(ratio - 1.0).max()
        print(f"F = {F}: C_ii / var in {ratio.min():.3f} .. {ratio.max():.3f}")
    assert gaps[16000] < gaps[2000]


def test_draw_assembly_has_the_closed_form_moments():
    """assemble + paths on NumPy normals: sample mean and variance of 4000 paths against path_mean / path_var, within
    5 standard errors (40 points x 2 statistics)."""
    X, th, m, Sinv, fmap, P = _design()
    N, F, S = X.shape[0], 500, 4000
    W, b = _basis(F, 3, th[1], 5)
    Phi = pw.features(X, W, b, th[2])
    rs = np.random.RandomState(6)
    L = np.linalg.cholesky((P + P.T) / 2)
    z, w = rs.randn(S, N), rs.randn(S, F)
    Fs, V = pw.assemble(z, w, fmap, L, Phi, Sinv)
    Xq = np.random.RandomState(7).rand(40, 3)
    G = pw.paths(Xq, w, V, W, b, X, th, "SE_kernel")
    C = pw.path_var(Xq, W, b, X, th, "SE_kernel", Sinv, P, Phi)
    assert np.allclose(C, np.diag(pw.path_cov(Xq, W, b, X, th, "SE_kernel", Sinv, P, Phi)), rtol=1e-10)
    assert np.all(np.abs(G.mean(axis=0) - pw.path_mean(Xq, X, th, "SE_kernel", Sinv, fmap)) <= 5 * np.sqrt(C / S))
    assert np.all(np.abs(G.var(axis=0, ddof=1) / C - 1.0) <= 5 * np.sqrt(2.0 / S))


@pytest.mark.parametrize("kernel", pw.KERNELS)
@pytest.mark.parametrize("ard", [False, True])
def test_path_gradient_against_central_differences(kernel, ard):
    rs = np.random.RandomState(11)
    N, D, F = 40, 5, 64
    th = [0.05, np.array([0.2, 0.3, 0.5, 0.8, 0.4]) if ard else 0.35, 0.7]
    X, x = rs.rand(N, D), rs.rand(D)
    W, b = rs.randn(F, D) / th[1], rs.uniform(0, 2 * np.pi, F)
    w, v = rs.randn(F), 30.0 * rs.randn(N)
    g = pw.path_grad(x, w, v, W, b, X, th, kernel)
    h = 1e-6
    num = np.array([(pw.paths(x + h * e, w, v, W, b, X, th, kernel)[0, 0] - pw.paths(x - h * e, w, v, W, b, X, th, kernel)[0, 0])
                    / (2 * h) for e in np.eye(D)])
    scale = pw.paths_abs(x, w, v, W, b, X, th, kernel)[0, 0]
    # central differences: truncation h^2 g''' / 6 and rounding eps scale / h, both far below 1e-6 of the gradient's scale
    assert np.abs(g - num).max() <= 1e-6 * max(np.abs(g).max(), scale), (g, num)


# ---------------------------------------------------------------- the public surface
def test_header_and_prototypes_list_the_new_entry_points():
    from ppbo_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ppbo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(", txt))
    for s in NEW_SYMBOLS:
        assert s in declared, f"include/ppbo_hip.h does not declare {s}"
        assert s in _lib.SIGNATURES, f"ctypes binding lacks {s}"
    assert len(_lib.SIGNATURES["ppbo_path_score_multi"]) == 16 and len(_lib.SIGNATURES["ppbo_path_search_multi"]) == 23
    # the version script exports the ppbo_ prefix: nothing to list per symbol
    assert "ppbo_*" in open(os.path.join(ROOT, "ppbo_amd", "csrc", "libppbo_hip.map")).read()


def test_library_exports_the_new_entry_points():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)


def _host_sampler(kernel="SE_kernel", D=3, theta=(0.05, 0.3, 1.0), **fit):
    """An Hsampler on a stand-in engine that has no device: every refusal below must come before the first device call."""
    from ppbo_amd.random_fourier_sampler import Hsampler
    X = np.random.RandomState(0).rand(8, D)
    gp = types.SimpleNamespace(D=D, m=3, X=X, xstar=X[0], xstars_local=X[:2], n_gausshermite_sample_points=None,
                               obs_indices=np.arange(0, 8, 4), kernel=types.SimpleNamespace(__name__=kernel),
                               theta=list(theta), **fit)
    hs = Hsampler(gp, 16, engine=types.SimpleNamespace(device="none"))
    hs.W = np.zeros((16, 11 if kernel.startswith("camphor") else D))
    hs.b = np.zeros((16, 1))
    return hs


def test_sampler_surface_and_host_refusals():
    from ppbo_amd import random_fourier_sampler as rfs
    from ppbo_amd.engine import Engine
    assert hasattr(rfs, "PosteriorPaths") and hasattr(rfs.Hsampler, "sample_paths")
    assert hasattr(Engine, "path_score_multi") and hasattr(Engine, "path_search_multi")
    hs = _host_sampler()
    with pytest.raises(ValueError, match="posterior"):
        hs.sample_xstars(4, posterior="other")
    with pytest.raises(RuntimeError, match="no fitted posterior"):          # a GP model without a fit
        hs.sample_paths(4, seed=1)
    with pytest.raises(RuntimeError, match="no fitted posterior"):
        hs.sample_xstars(4, seed=1, posterior="pathwise")
    with pytest.raises(ValueError):
        hs.sample_xstars(4, omegas=np.zeros((4, 16)), posterior="pathwise")
    for kern in ("camphor_copper_kernel", "camphor_copper_ard_kernel"):
        cam = _host_sampler(kern, 6)
        with pytest.raises(NotImplementedError, match=kern):
            cam.sample_paths(4, seed=1)
    # a fit of another design
    N = 8
    other = _host_sampler(Sigma_inv=np.eye(N + 1), fMAP=np.zeros(N + 1), posterior_covariance=np.eye(N + 1))
    with pytest.raises(RuntimeError, match="design"):
        other.sample_paths(4, seed=1)


def test_engine_argument_checks_run_on_shapes_alone():
    from ppbo_amd.engine import Engine, RFF_MULTI_MAX_S
    D, F, N, S = 4, 32, 10, 3
    z = np.zeros
    ok = dict(what="path_score_multi", D=D, W=z((F, D)), b=z(F), Wp=z((S, F)), V=z((S, N)), X=z((N, D)),
              kernel="SE_kernel", theta=[0.05, 0.3, 1.0])
    assert Engine._path_widths(**ok) == (F, S, N, None)
    ard = Engine._path_widths(**dict(ok, theta=[0.05, np.array([0.2, 0.4, 0.5, 1.0]), 1.0]))
    assert np.allclose(ard[3], [5.0, 2.5, 2.0, 1.0])
    for bad in (dict(V=z((S, N + 1))), dict(V=z((S + 1, N))), dict(V=z(N)), dict(Wp=z((0, F)), V=z((0, N))),
                dict(Wp=z((RFF_MULTI_MAX_S + 1, F)), V=z((RFF_MULTI_MAX_S + 1, N))), dict(K=0), dict(K=1025),
                dict(X=z((N, D + 1))), dict(kernel="camphor_copper_kernel"), dict(Wp=z((S, F + 1))),
                dict(D=65, W=z((F, 65)), X=z((N, 65))), dict(theta=[0.05, np.array([0.2, 0.4]), 1.0])):
        with pytest.raises(ValueError):
            Engine._path_widths(**dict(ok, **bad))
