"""CPU: the functional surface (ppbo_predict_functionals / Engine.predict_functionals / GPModel.functional_pred and its
layers) -- the NumPy statement against the reference's dense covariance, the rearranged prior term against the dense
one, the binding table, and the refusals that are decided on shapes before anything reaches a device."""
import os
import re
import types

import numpy as np
import pytest

import functionals_numpy as fn
import pairs_numpy as pn
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIAL = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")
EPS = np.finfo(float).eps


def _theta(kernel, D):
    return [0.05, 0.3 * np.sqrt(D / 6.0), 0.7] if kernel != pn.CAMPHOR else [0.05, 0.6, 0.7]


@pytest.mark.parametrize("kernel", RADIAL + (pn.CAMPHOR,))
@pytest.mark.parametrize("G", [1, 2, 3, 17, 64])
def test_rearranged_prior_equals_the_dense_sum(kernel, G):
    """sf^2 (sum w)^2 - 2 sum_{g<h} w_g w_h (sf^2 - k) against sum_{g,h} w_g w_h k on random groups: two orders of the same
    G^2 products of O(1) kernel values, so they differ by rounding alone -- at most G^2 terms of half an ulp of
    sf^2 |w_g| |w_h| each way, G eps sf^2 (sum |w|)^2 with room to spare.  Anything more is a wrong term."""
    rng = np.random.default_rng(17 * G + len(kernel))
    D, M = 6, 40
    th = _theta(kernel, D)
    Xg = rng.random((M, G, D))
    if G > 2:
        Xg[:5, 1] = Xg[:5, 0]                                  # coincident points
        Xg[5:10, 2] = Xg[5:10, 0] + 1e-6 * rng.standard_normal((5, D))
    sf2 = th[2] ** 2
    for w in (rng.standard_normal((M, G)), np.full(G, 1.0 / G), rng.standard_normal(G)):
        dense, rearr = fn.dense_prior(Xg, w, th, kernel), fn.rearranged_prior(Xg, w, th, kernel)
        scale = sf2 * np.abs(np.broadcast_to(w, (M, G))).sum(axis=1) ** 2
        assert np.all(np.abs(dense - rearr) <= 4 * G * EPS * scale), np.max(np.abs(dense - rearr) / scale)


@pytest.mark.parametrize("kernel", RADIAL)
def test_rearranged_prior_keeps_the_digits_of_a_contrast(kernel):
    """A contrast (sum w = 0) on a cloud of radius 1e-4: w' K w ~ 1e-8 sf^2.  In longdouble the dense sum is the yardstick;
    the rearranged float64 term stays within 1e-10 of it RELATIVELY, where the float64 dense sum keeps ~1e-8."""
    rng = np.random.default_rng(5)
    D, G, M = 6, 9, 50
    th = _theta(kernel, D)
    x = rng.random((M, 1, D))
    u = rng.standard_normal((M, G - 1, D))
    cloud = x + 1e-4 * u / np.linalg.norm(u, axis=2, keepdims=True)
    Xg = np.concatenate([cloud, x], axis=1)
    w = np.concatenate([np.full(G - 1, 1.0 / (G - 1)), [-1.0]])
    rearr = fn.rearranged_prior(Xg, w, th, kernel)
    # yardstick: the rearrangement itself in extended precision (sum w = 0 exactly: only the pair terms remain), with
    # 1 - k / sf^2 from its Taylor-safe forms; against it the float64 result must agree to rounding of its own terms
    s = np.zeros(M, dtype=np.longdouble)
    for g in range(G):
        for h in range(g + 1, G):
            s += np.longdouble(w[g] * w[h]) * fn.one_minus_kernel(Xg[:, g], Xg[:, h], th, kernel).astype(np.longdouble)
    want = (np.longdouble(th[2]) ** 2 * (-2.0 * s)).astype(float)
    assert np.all(want > 0.0)
    assert np.max(np.abs(rearr - want) / want) <= 1e-10
    assert np.all(rearr > 0.0)


def test_identities_of_the_rearranged_prior():
    rng = np.random.default_rng(2)
    th = _theta("SE_kernel", 4)
    a = rng.random((7, 1, 4))
    same = np.concatenate([a, a], axis=1)
    assert np.all(fn.rearranged_prior(same, [1.0, -1.0], th, "SE_kernel") == 0.0)
    Xg = rng.random((7, 5, 4))
    assert np.all(fn.rearranged_prior(Xg, np.zeros(5), th, "SE_kernel") == 0.0)
    w = rng.standard_normal(5)
    p = fn.rearranged_prior(Xg, w, th, "SE_kernel")
    assert np.array_equal(fn.rearranged_prior(Xg, -w, th, "SE_kernel"), p)
    assert np.array_equal(fn.rearranged_prior(Xg, 2 * w, th, "SE_kernel"), 4 * p)
    # G = 1: the prior variance of one point
    assert np.allclose(fn.rearranged_prior(Xg[:, :1], [1.0], th, "SE_kernel"), th[2] ** 2, rtol=0, atol=0)


@pytest.mark.parametrize("name", ["smoke", "rq"])
def test_reference_tied_to_mu_Sigma_preds_dense_covariance(name):
    """The goldens hold the reference's mu_Sigma_pred on its 70-point line grid (line_mu, line_cov).  For groups drawn from
    that grid, w' line_cov w = var - s w' K w + s sf^2 |w|^2 (the reference shrinks its prior block by s = 1e-6, diagonal
    back to sf^2) and w' line_mu = mu.  Bound: the package's 1e-6, normalised as the GPU tests normalise."""
    g = load_golden(name)
    X, th, kernel, m = g["X"], [float(v) for v in g["theta"]], str(g["kernel"]), int(g["m"])
    alpha, A = pn.operator_from_fit(X, th, kernel, m, g["fMAP"])
    rng = np.random.default_rng(31)
    M, G = 24, 7
    idx = np.stack([rng.choice(70, G, replace=False) for _ in range(M)])
    W = rng.standard_normal((M, G))
    W[:8] = 1.0 / G
    W[8:16] -= W[8:16].mean(axis=1, keepdims=True)
    Xg = g["line_grid"][idx]
    mu, var = fn.functional_reference(Xg, W, X, th, kernel, alpha, A)
    s, sf2 = 1e-6, th[2] ** 2
    C = g["line_cov"]
    want_var = np.array([W[i] @ C[np.ix_(idx[i], idx[i])] @ W[i] for i in range(M)])
    want_mu = np.array([W[i] @ g["line_mu"][idx[i]] for i in range(M)])
    got_var = var - s * fn.dense_prior(Xg, W, th, kernel) + s * sf2 * (W * W).sum(axis=1)
    scale = sf2 * np.abs(W).sum(axis=1) ** 2
    e_var, e_mu = np.max(np.abs(got_var - want_var) / scale), np.abs(mu - want_mu).max() / np.abs(want_mu).max()
    print(f"functional reference against mu_Sigma_pred {name}: var {e_var:.2e}, mu {e_mu:.2e}")
    assert e_var <= 1e-6 and e_mu <= 1e-6


def test_reference_reduces_to_the_duel_and_the_point():
    g = load_golden("smoke")
    X, th, kernel, m = g["X"], [float(v) for v in g["theta"]], str(g["kernel"]), int(g["m"])
    alpha, A = pn.operator_from_fit(X, th, kernel, m, g["fMAP"])
    rng = np.random.default_rng(3)
    Xa, Xb = rng.random((20, 3)), rng.random((20, 3))
    mu_d, var_d = pn.pair_reference(Xa, Xb, X, th, kernel, alpha, A)
    mu, var = fn.functional_reference(np.stack([Xa, Xb], axis=1), [1.0, -1.0], X, th, kernel, alpha, A)
    assert np.allclose(mu, mu_d, rtol=0, atol=1e-12 * np.abs(mu_d).max()) and np.allclose(var, var_d, rtol=0, atol=1e-12)
    p = fn.threshold_probability([1.0, 0.0, -1.0, 0.3, np.nan], [0.0, 0.0, 0.0, 0.09, 1.0], 0.0)
    assert list(p[:3]) == [1.0, 0.5, 0.0] and abs(p[3] - 0.8413447460685429) <= 2 * EPS and np.isnan(p[4])
    assert fn.threshold_probability(0.3, 0.0, 0.3) == 0.5


def test_binding_header_and_constants():
    from ppbo_amd import _lib, engine
    assert _lib.ABI_VERSION == 9
    assert "ppbo_predict_functionals" in _lib.SIGNATURES and len(_lib.SIGNATURES["ppbo_predict_functionals"]) == 16
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", txt)
    assert re.search(r"#define\s+PPBO_FUNCTIONAL_MAX_G\s+64\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "ppbo_predict_functionals" in set(re.findall(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(", code))
    proto = re.search(r"ppbo_predict_functionals\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(proto.split(",")) == 16 and "w_stride" in proto and "threshold" in proto
    assert re.search(r"PPBO_FUNCTIONAL_MEAN\s*=\s*0\s*,\s*PPBO_FUNCTIONAL_VARIANCE\s*=\s*1\s*,\s*PPBO_FUNCTIONAL_PROB\s*=\s*2", code)
    assert (_lib.FUNCTIONAL_MEAN, _lib.FUNCTIONAL_VARIANCE, _lib.FUNCTIONAL_PROB, _lib.FUNCTIONAL_MAX_G) == (0, 1, 2, 64)
    assert (engine.FUNCTIONAL_MEAN, engine.FUNCTIONAL_VARIANCE, engine.FUNCTIONAL_PROB) == (0, 1, 2)
    # the version script exports the C-ABI by its prefix
    ver = open(os.path.join(ROOT, "ppbo_amd", "csrc", "libppbo_hip.map")).read()
    assert re.search(r"global:[^;]*\bppbo_\*", ver)
    assert hasattr(engine.Engine, "predict_functionals")
    from ppbo_amd.gp_model import GPModel
    for name in ("functional_pred", "average_pred", "contrast_pred", "robust_xstar"):
        assert hasattr(GPModel, name)


def test_library_exports_the_entry_point():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    assert hasattr(_lib.load(), "ppbo_predict_functionals")


class _NoDevice:
    """Stands where the library handle would: any call through it is a failure of the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the refusal came after a device call ({name})")


def _stub_engine():
    from ppbo_amd.engine import Engine
    eng = Engine.__new__(Engine)          # no ctx, no library: nothing below may touch either
    eng.lib, eng.ctx, eng.device = _NoDevice(), None, "none"
    eng.dev = lambda a, dtype=None: (_ for _ in ()).throw(AssertionError("the refusal came after an upload"))
    return eng


@pytest.mark.parametrize("camphor", [False, True])
def test_predict_functionals_refuses_shapes_before_the_device(camphor):
    from ppbo_amd.engine import Posterior
    eng = _stub_engine()
    D = 6 if camphor else 4
    post = Posterior("SE_kernel", (0.05, 0.3, 1.0), 3, types.SimpleNamespace(shape=(8, 11 if camphor else D)), None, None,
                     None, None, camphor=np.ones(6) if camphor else None)
    z = np.zeros
    for Xg, w in ((z((5, D)), z(D)), (z((5, 3, D + 1)), z(3)), (z((0, 3, D)), z(3)), (z((5, 0, D)), z(0)),
                  (z((5, 65, D)), z(65)), (z((5, 3, D)), z(4)), (z((5, 3, D)), z((4, 3))), (z((5, 3, D)), z((5, 3, 1))),
                  (z((5, 3, D)), z((3, 5))), (z((5, 3, D, 1)), z(3)), (z((5, 3, D)), 1.0)):
        with pytest.raises(ValueError, match="predict_functionals"):
            eng.predict_functionals(post, Xg, w)
    with pytest.raises(ValueError, match="score kind"):
        eng.predict_functionals(post, z((5, 3, D)), z(3), score=3)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="threshold"):
            eng.predict_functionals(post, z((5, 3, D)), z(3), threshold=bad)


def test_layers_without_a_posterior_raise_mu_Sigma_preds_error():
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = None
    with pytest.raises(RuntimeError) as a:
        gp.functional_pred(np.zeros((2, 3, 3)), np.ones(3))
    with pytest.raises(RuntimeError) as b:
        gp.mu_Sigma_pred(np.zeros((2, 3)))
    assert str(a.value) == str(b.value)
