"""CPU: the tournament surface (ppbo_predict_tournament / Engine.predict_tournament / GPModel.tournament_pred, borda_pred,
ranking_pred) -- the NumPy statement against the duel's own (pairs_numpy), the row reductions, the binding table, and the
refusals that are decided on shapes before anything reaches a device."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import pairs_numpy as pn
import tournament_numpy as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy(kernel, D=4, n_q=3, m=5, seed=0):
    """A small design with a symmetric operator A of the right scale and a random alpha (no fit: the identities below hold
    for any symmetric A)."""
    rng = np.random.default_rng(seed)
    X = rng.random((n_q * (m + 1), D))
    th = [0.05, 0.4, 0.7]
    K = pn.cross(X, X, th, kernel)
    A = np.linalg.inv(K + 0.1 * np.eye(len(X)))
    return X, th, rng.standard_normal(len(X)), 0.5 * (A + A.T)


@pytest.mark.parametrize("kernel", ["SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel"])
def test_reference_var_d_is_the_duels_own(kernel):
    """var_d0 = var_a0 + var_b0 - 2 cov0 against pairs_numpy.pair_reference on the Ma Mb expanded pairs (which forms the
    difference column directly): 1e-12 sf^2; the means likewise."""
    X, th, alpha, A = _toy(kernel)
    rng = np.random.default_rng(1)
    Xa, Xb = rng.random((17, X.shape[1])), rng.random((9, X.shape[1]))
    Xa[0], Xb[1], Xb[2] = X[3], X[5], Xa[4]                       # design rows on either side, one identical point
    ref = tn.tournament_reference(Xa, Xb, X, th, kernel, alpha, A)
    mu_d, var_d = pn.pair_reference(np.repeat(Xa, len(Xb), axis=0), np.tile(Xb, (len(Xa), 1)), X, th, kernel, alpha, A)
    sf2 = th[2] ** 2
    assert np.abs(ref["var_d"].ravel() - var_d).max() <= 1e-12 * sf2
    assert np.abs((ref["mu_a"][:, None] - ref["mu_b"][None, :]).ravel() - mu_d).max() <= 1e-12 * np.abs(mu_d).max()
    assert abs(ref["var_d"][4, 2]) <= 1e-12 * sf2                 # a == b
    p = tn.win_matrix(ref, th[0])
    assert p.shape == (17, 9) and abs(p[4, 2] - 0.5) <= 1e-9


def test_reductions_on_a_hand_made_matrix():
    P = np.array([[0.5, 0.25, 1.0], [0.1, 0.9, 0.2], [0.75, 0.75, 0.75], [0.0, np.nan, 1.0]])
    b, w = tn.scores(P, tn.BORDA), tn.scores(P, tn.WORST)
    assert np.array_equal(b[:3], [(0.5 + 0.25 + 1.0) / 3, (0.1 + 0.9 + 0.2) / 3, 0.75]) and np.isnan(b[3])
    assert np.array_equal(w[:3], [0.25, 0.1, 0.75]) and np.isnan(w[3])
    assert tn.best(b) == (0.75, 2) and tn.best(w) == (0.75, 2)       # NaN never wins
    assert tn.best(np.array([0.3, 0.7, 0.7])) == (0.7, 1)            # the first index of equal scores
    v, i = tn.best(np.array([np.nan, np.nan]))
    assert np.isnan(v) and i == -1
    with pytest.raises(ValueError):
        tn.scores(P, 2)


def test_binding_header_and_constants():
    from ppbo_amd import _lib, engine
    assert _lib.ABI_VERSION == 9
    assert len(_lib.SIGNATURES["ppbo_predict_tournament"]) == 17
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", txt)
    assert re.search(r"#define\s+PPBO_TOURNAMENT_MAX_B\s+1024\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "ppbo_predict_tournament" in set(re.findall(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(", code))
    assert re.search(r"PPBO_TOURNAMENT_BORDA\s*=\s*0\s*,\s*PPBO_TOURNAMENT_WORST\s*=\s*1", code)
    assert (_lib.TOURNAMENT_BORDA, _lib.TOURNAMENT_WORST, _lib.TOURNAMENT_MAX_B) == (0, 1, 1024)
    assert (engine.TOURNAMENT_BORDA, engine.TOURNAMENT_WORST, engine.TOURNAMENT_MAX_B) == (0, 1, 1024)
    # the header states the formulas and the accuracy note
    comment = txt[txt.index("---- tournaments"):txt.index("#define PPBO_TOURNAMENT_MAX_B")]
    for needle in ("u_b = (Lambda + M'M) k_b", "var_a + var_b - 2 cov", "ABSOLUTE", "ppbo_predict_pairs remains the tool",
                   "poisons the field"):
        assert needle in comment, needle


def test_library_exports_the_entry_point():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    assert hasattr(_lib.load(), "ppbo_predict_tournament")


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
def test_predict_tournament_refuses_shapes_before_the_device(camphor):
    from ppbo_amd.engine import Posterior
    eng = _stub_engine()
    D = 6 if camphor else 4
    post = Posterior("SE_kernel", (0.05, 0.3, 1.0), 3, types.SimpleNamespace(shape=(8, 11 if camphor else D)), None, None,
                     None, None, camphor=np.ones(6) if camphor else None)
    z = np.zeros
    for Xa, Xb in ((z((5, D)), z((4, D + 1))), (z((5, D + 1)), z((4, D))), (z(D), z((4, D))), (z((5, D)), z(D)),
                   (z((0, D)), z((4, D))), (z((5, D)), z((0, D))), (z((5, D, 1)), z((4, D))), (z((5, D)), z((1025, D)))):
        with pytest.raises(ValueError, match="predict_tournament"):
            eng.predict_tournament(post, Xa, Xb)
    with pytest.raises(ValueError, match="score kind"):
        eng.predict_tournament(post, z((5, D)), z((4, D)), score=2)
    assert eng._tournament_shapes(post, z((5, D)), z((1024, D))) == (5, 1024)     # the cap itself is taken


def test_gpmodel_surface():
    from ppbo_amd.gp_model import GPModel
    assert list(inspect.signature(GPModel.tournament_pred).parameters) == ["self", "XA", "XB"]
    sig = inspect.signature(GPModel.borda_pred)
    assert list(sig.parameters) == ["self", "X", "field", "n_field", "seed"]
    assert (sig.parameters["field"].default, sig.parameters["n_field"].default, sig.parameters["seed"].default) == (None, 256, None)
    assert list(inspect.signature(GPModel.ranking_pred).parameters) == ["self", "X_items"]
    gp = GPModel.__new__(GPModel)
    gp.D = 5
    f1, f2, f3 = gp.default_field(256, seed=11), gp.default_field(256, seed=11), gp.default_field(256, seed=12)
    assert f1.shape == (256, 5) and np.array_equal(f1, f2) and not np.array_equal(f1, f3)
    assert f1.min() >= 0.0 and f1.max() < 1.0
    assert gp.default_field(7, seed=0).shape == (7, 5)


def test_predictions_without_a_posterior_are_mu_Sigma_preds_error():
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post, gp.D = None, 3
    with pytest.raises(RuntimeError) as ref:
        gp.mu_Sigma_pred(np.zeros((2, 3)))
    for call in (lambda: gp.tournament_pred(np.zeros((2, 3)), np.ones((2, 3))), lambda: gp.borda_pred(np.zeros((2, 3)), seed=0),
                 lambda: gp.ranking_pred(np.zeros((2, 3)))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == str(ref.value)
