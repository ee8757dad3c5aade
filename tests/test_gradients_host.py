"""CPU: the gradient surface (ppbo_predict_gradients / Engine.predict_gradients / GPModel.gradient_pred, xstar_covariance,
loosest_direction, active_subspace) -- the NumPy statement tests/gradients_numpy.py against the slope statement (which
tests/test_slopes_host.py holds to central differences), its symmetry and definiteness, the prior constants, the engine's
pull-back of a camphor_copper_ard_kernel model, the binding table and the refusals decided before a device is touched."""
import os
import re

import numpy as np
import pytest

import gradients_numpy as gn
import slopes_numpy as sn
from oracle import ppbo_oracle as orc
from test_slopes_host import RADIAL, _case, _stub_engine, _stub_post

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, False) for k in RADIAL] + [("Matern52_kernel", True), (sn.CAMPHOR, False), (sn.CAMPHOR_ARD, True)]


@pytest.mark.parametrize("kernel,ard", CASES)
def test_projections_are_the_slope_statement(kernel, ard):
    """xi' m = mu_s and xi' C xi = var_s for random xi of every length: the bound is rounding alone, 1e-12 of what each
    number cancels down from (the prior term, resp. sum_j |g_j alpha_j|)."""
    X, theta, m, alpha, A, Xq, Xi = _case(kernel, ard)
    mean, C, _ = gn.gradient_reference(Xq, X, theta, kernel, alpha, A)
    mu, var, g = sn.slope_reference(Xq, Xi, X, theta, kernel, alpha, A)
    e_mu = np.max(np.abs(np.einsum("id,id->i", mean, Xi) - mu) / (np.abs(g) @ np.abs(alpha)))
    e_var = np.max(np.abs(np.einsum("id,ide,ie->i", Xi, C, Xi) - var) / sn.slope_prior(Xi, theta, kernel))
    print(f"gradients statement {kernel} ard={ard}: |xi'm - mu_s| / sum|g alpha| = {e_mu:.2e}, |xi'C xi - var_s| / prior = {e_var:.2e}")
    assert e_mu <= 1e-12 and e_var <= 1e-12


@pytest.mark.parametrize("kernel,ard", CASES)
def test_reference_covariance_is_symmetric_and_positive(kernel, ard):
    X, theta, m, alpha, A, Xq, _ = _case(kernel, ard)
    _, C, _ = gn.gradient_reference(Xq, X, theta, kernel, alpha, A)
    scale = gn.cov_scale(theta, kernel, X.shape[1])
    assert np.max(np.abs(C - C.transpose(0, 2, 1)) / scale) <= 1e-14
    low = np.linalg.eigvalsh(0.5 * (C + C.transpose(0, 2, 1))).min() / gn.prior_diagonal(theta, kernel, X.shape[1]).max()
    print(f"gradients statement {kernel} ard={ard}: smallest eigenvalue / largest prior entry = {low:.3e}")
    assert low > 0.0
    # data only ever remove variance: P - C is positive semi-definite
    gone = np.diag(gn.prior_diagonal(theta, kernel, X.shape[1]))[None] - C
    assert np.linalg.eigvalsh(0.5 * (gone + gone.transpose(0, 2, 1))).min() >= -1e-12 * scale.max()


def test_prior_constants():
    sf, l = 0.7, 0.4
    for kernel, c in zip(RADIAL, (1.0, 1.0, 5.0 / 3.0, 3.0)):
        want = c * sf ** 2 / l ** 2
        assert np.abs(gn.prior_diagonal([0.05, l, sf], kernel, 5) - want).max() <= 4e-16 * want
    ls = np.array([0.4, 0.6, 0.5, 1.0, 0.8, 0.7])
    want = sf ** 2 * np.where(np.arange(6) == 2, 1.0, 4 * np.pi ** 2) / ls ** 2
    assert np.abs(gn.prior_diagonal([0.05, ls, sf], sn.CAMPHOR_ARD, 6) - want).max() <= 4e-16 * want.max()
    want = sf ** 2 * np.where(np.arange(6) == 2, 1.0 / (l + 0.05) ** 2, 4 * np.pi ** 2 / l ** 2)
    assert np.abs(gn.prior_diagonal([0.05, l, sf], sn.CAMPHOR, 6) - want).max() <= 4e-16 * want.max()
    # an ARD model in the device's coordinates (s . x, l = 1) and the engine's map back: S P S
    ls4 = np.array([0.3, 0.5, 0.25, 0.6])
    assert np.abs(gn.prior_diagonal([0.05, 1.0, sf], "SE_kernel", 4) / ls4 ** 2 - gn.prior_diagonal([0.05, ls4, sf], "SE_kernel", 4)).max() <= 1e-14


def test_camphor_ard_pull_back():
    """The engine's J'm and J'CJ of the 11-column statement (SE, l = 1, on embedded rows) against the six-coordinate one."""
    import torch
    from ppbo_amd.engine import camphor_embed_directions, camphor_embed_jacobians, camphor_pull_back
    from ppbo_amd.random_fourier_sampler import camphor_embed_host
    X, theta, m, alpha, A, Xq, Xi = _case(sn.CAMPHOR_ARD, True)
    ls = np.asarray(theta[1])
    J = camphor_embed_jacobians(torch.as_tensor(Xq), ls).numpy()
    assert J.shape == (40, 11, 6)
    assert np.abs(np.einsum("ice,ie->ic", J, Xi) - camphor_embed_directions(Xq, Xi, ls)).max() <= 1e-13 * np.abs(J).max() * np.abs(Xi).max()
    m11, C11, _ = gn.gradient_reference(camphor_embed_host(Xq, ls), camphor_embed_host(X, ls), [theta[0], 1.0, theta[2]], "SE_kernel", alpha, A)
    m6, C6, g6 = gn.gradient_reference(Xq, X, theta, sn.CAMPHOR_ARD, alpha, A)
    pm, pc = camphor_pull_back(torch.as_tensor(Xq), ls, torch.as_tensor(m11), torch.as_tensor(C11))
    e_m = np.max(np.abs(pm.numpy() - m6) / gn.mean_scale(g6, alpha))
    e_c = np.max(np.abs(pc.numpy() - C6) / gn.cov_scale(theta, sn.CAMPHOR_ARD, 6))
    print(f"gradients camphor ARD pull-back: mean {e_m:.2e}, covariance {e_c:.2e}")
    assert e_m <= 1e-13 and e_c <= 1e-13
    assert torch.equal(pc, pc.transpose(1, 2))
    only_m, none = camphor_pull_back(torch.as_tensor(Xq), ls, torch.as_tensor(m11), None)
    assert none is None and torch.equal(only_m, pm)


def test_delta_method_and_active_subspace_statements():
    rng = np.random.default_rng(0)
    B = rng.standard_normal((5, 5))
    H, C = -(B @ B.T + np.eye(5)), B.T @ B
    Hi = np.linalg.inv(H)
    want = Hi @ C @ Hi
    assert np.abs(gn.xstar_covariance(H, C) - want).max() <= 1e-12 * np.abs(want).max()
    m, Cs = rng.standard_normal((7, 5)), np.tile(C, (7, 1, 1))
    want = sum(np.outer(v, v) for v in m) / 7 + C
    assert np.abs(gn.active_matrix(m, Cs) - want).max() <= 1e-14 * np.abs(want).max()
    w, V = gn.active_subspace(m, Cs)
    assert np.all(np.diff(w) <= 0) and np.abs(V @ want @ V.T - np.diag(w)).max() <= 1e-12 * w[0]


def test_rotated_ridge_leads_the_active_subspace():
    """gradients_numpy.ridge_design: the NumPy statement alone, on an oracle fit, finds the one direction the design varies
    in (4.2 degrees; the GPU test holds GPModel.active_subspace on the device's fit of the same design to 10)."""
    R = gn.RIDGE
    X, u = gn.ridge_design()
    Sinv = orc.pd_inverse(orc.regularize_covariance(sn.cross(X, X, R["theta"], R["kernel"]), orc.SHRINKAGE))
    f, _ = orc.fit_fmap_newton(np.zeros(X.shape[0]), Sinv, R["m"], R["theta"][0], gtol=1e-10, maxiter=500)
    alpha, A = sn.operator_from_fit(X, R["theta"], R["kernel"], R["m"], f)
    m, C, _ = gn.gradient_reference(gn.ridge_points(), X, R["theta"], R["kernel"], alpha, A)
    w, V = gn.active_subspace(m, C)
    angle = gn.angle_degrees(V[0], u)
    print(f"gradients ridge: angle {angle:.2f} degrees, eigenvalues {w[0]:.3f} {w[1]:.3f}")
    assert angle <= 5.0 and w[0] >= 1.1 * w[1]


# ---------------------------------------------------------------- the plumbing
def test_binding_header_and_constants():
    from ppbo_amd import _lib, engine
    assert _lib.ABI_VERSION == 9
    assert len(_lib.SIGNATURES["ppbo_predict_gradients"]) == 12
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "ppbo_predict_gradients" in set(re.findall(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(", code))
    assert re.search(r"PPBO_GRAD_NONE\s*=\s*0\s*,\s*PPBO_GRAD_TRACE\s*=\s*1\s*,\s*PPBO_GRAD_NORM2\s*=\s*2", code)
    sig = re.search(r"ppbo_predict_gradients\s*\(([^)]*)\)", code).group(1)
    assert [a.split()[-1].lstrip("*") for a in sig.split(",")] == ["ctx", "model", "d_X", "M", "h_metric", "score_kind", "d_mean",
                                                                  "d_cov", "d_score", "h_best_val", "h_best_idx", "stream"]
    assert (_lib.GRAD_NONE, _lib.GRAD_TRACE, _lib.GRAD_NORM2) == (0, 1, 2)
    assert (engine.GRAD_NONE, engine.GRAD_TRACE, engine.GRAD_NORM2) == (0, 1, 2)
    assert hasattr(engine.Engine, "predict_gradients")
    from ppbo_amd.gp_model import GPModel
    for name in ("gradient_pred", "xstar_covariance", "loosest_direction", "active_subspace"):
        assert hasattr(GPModel, name)


def test_library_exports_the_entry_point():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    assert hasattr(_lib.load(), "ppbo_predict_gradients")


@pytest.mark.parametrize("camphor", [False, True])
def test_predict_gradients_refuses_shapes_before_the_device(camphor):
    eng = _stub_engine()
    D = 6 if camphor else 4
    post = _stub_post(camphor, D)
    z = np.zeros
    for X in (z((5, D + 1)), z((5, D - 1)), z(D), z((0, D)), z((5, D, 1)), z((5, 11))):
        with pytest.raises(ValueError, match="predict_gradients"):
            eng.predict_gradients(post, X)
    for score in (3, -1):
        with pytest.raises(ValueError, match="score kind"):
            eng.predict_gradients(post, z((5, D)), score=score)


def test_gpmodel_refusals():
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = None
    with pytest.raises(RuntimeError) as a:
        gp.gradient_pred(np.zeros(3))
    with pytest.raises(RuntimeError) as b:
        gp.mu_Sigma_pred(np.zeros((2, 3)))
    assert str(a.value) == str(b.value)
    with pytest.raises(RuntimeError):
        gp.active_subspace(X=np.zeros((2, 3)))
    gp._post = _stub_post(False, 4)
    gp._post.G = object()
    gp.eng = _stub_engine()
    for X in (np.zeros(5), np.zeros((3, 5)), np.zeros((0, 4))):
        with pytest.raises(ValueError, match="predict_gradients"):
            gp.gradient_pred(X)
    with pytest.raises(ValueError, match="predict_gradients"):
        gp.active_subspace(X=np.zeros((3, 5)))
