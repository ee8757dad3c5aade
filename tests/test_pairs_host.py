"""CPU: the duel surface (ppbo_predict_pairs / Engine.predict_pairs / GPModel.preference_pred) -- the NumPy statement of
the win probability, the binding table, and the refusals that are decided on shapes before anything reaches a device."""
import os
import re
import types

import numpy as np
import pytest
import scipy.stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_preference_probability_against_scipy():
    from ppbo_amd.misc import preference_probability
    sigma = 0.05
    mu, var = np.meshgrid(np.linspace(-3.0, 3.0, 61), np.concatenate([[-1e-3, -1e-12, 0.0], np.logspace(-12, 1, 27)]))
    p = preference_probability(mu, var, sigma)
    ref = scipy.stats.norm.cdf(mu / np.sqrt(2 * sigma ** 2 + np.maximum(var, 0.0)))
    assert p.shape == mu.shape
    assert np.abs(p - ref).max() <= 4 * np.finfo(float).eps
    # a negative variance is clipped: the same value as at 0
    assert np.array_equal(preference_probability(mu[0], np.full(61, -0.5), sigma), preference_probability(mu[0], np.zeros(61), sigma))
    # a tie is exactly one half, whatever the variance, and the two sides of a duel sum to one
    assert np.all(preference_probability(np.zeros(30), var[:, 0], sigma) == 0.5)
    assert np.abs(p + preference_probability(-mu, var, sigma) - 1.0).max() <= 2 * np.finfo(float).eps
    # no noise and no variance: the sign of the mean decides
    assert list(preference_probability([-1.0, 0.0, 2.0], [0.0, 0.0, -1.0], 0.0)) == [0.0, 0.5, 1.0]
    assert np.isnan(preference_probability(np.nan, 1.0, sigma)) and np.isnan(preference_probability(1.0, np.nan, sigma))
    assert preference_probability(0.3, 0.1, sigma).shape == ()


def test_binding_header_and_constants():
    from ppbo_amd import _lib, engine
    assert _lib.ABI_VERSION == 9
    assert "ppbo_predict_pairs" in _lib.SIGNATURES and len(_lib.SIGNATURES["ppbo_predict_pairs"]) == 13
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "ppbo_predict_pairs" in set(re.findall(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(", code))
    assert re.search(r"PPBO_PAIR_MEAN\s*=\s*0\s*,\s*PPBO_PAIR_VARIANCE\s*=\s*1\s*,\s*PPBO_PAIR_PROB\s*=\s*2", code)
    assert (_lib.PAIR_MEAN, _lib.PAIR_VARIANCE, _lib.PAIR_PROB) == (0, 1, 2)
    assert (engine.PAIR_MEAN, engine.PAIR_VARIANCE, engine.PAIR_PROB) == (0, 1, 2)
    assert hasattr(engine.Engine, "predict_pairs")
    from ppbo_amd.gp_model import GPModel
    assert hasattr(GPModel, "preference_pred")


def test_library_exports_the_entry_point():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    assert hasattr(_lib.load(), "ppbo_predict_pairs")


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
def test_predict_pairs_refuses_shapes_before_the_device(camphor):
    from ppbo_amd.engine import Posterior
    eng = _stub_engine()
    D = 6 if camphor else 4
    post = Posterior("SE_kernel", (0.05, 0.3, 1.0), 3, types.SimpleNamespace(shape=(8, 11 if camphor else D)), None, None,
                     None, None, camphor=np.ones(6) if camphor else None)
    z = np.zeros
    for Xa, Xb in ((z((5, D)), z((4, D))), (z((5, D)), z((5, D + 1))), (z((5, D + 1)), z((5, D + 1))), (z(D), z(D)),
                   (z((0, D)), z((0, D))), (z((5, D, 1)), z((5, D, 1)))):
        with pytest.raises(ValueError, match="predict_pairs"):
            eng.predict_pairs(post, Xa, Xb)
    with pytest.raises(ValueError, match="score kind"):
        eng.predict_pairs(post, z((5, D)), z((5, D)), score=3)


def test_preference_pred_without_a_posterior_is_mu_Sigma_preds_error():
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = None
    with pytest.raises(RuntimeError) as a:
        gp.preference_pred(np.zeros(3), np.ones(3))
    with pytest.raises(RuntimeError) as b:
        gp.mu_Sigma_pred(np.zeros((2, 3)))
    assert str(a.value) == str(b.value)
