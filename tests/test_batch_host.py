"""CPU: the shortlist surface (ppbo_search_batch / Engine.search_batch / GPModel.shortlist) -- the column-wise NumPy
statement (tests/batch_numpy.py) against independent DENSE conditioning (the M x M predictive covariance, the Schur
complement by np.linalg.solve, a greedy loop written directly on the matrix), the binding table, and the refusals that
are decided before anything reaches a device."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import batch_numpy as bn
import pairs_numpy as pn
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, Q = 300, 8


def _golden_model(name):
    g = load_golden(name)
    X, th, kernel, m = g["X"], [float(v) for v in g["theta"]], str(g["kernel"]), int(g["m"])
    alpha, A = pn.operator_from_fit(X, th, kernel, m, g["fMAP"])
    rng = np.random.default_rng(5)
    Xc = rng.random((M, X.shape[1]))
    Xc[:6] = X[rng.integers(0, len(X), 6)]            # a few design rows among the candidates
    return dict(X=X, th=th, kernel=kernel, alpha=alpha, A=A, Xc=Xc)


@pytest.fixture(scope="module", params=["smoke", "rq"])
def dense(request):
    """The model with the dense predictive covariance of its M candidates (only this test file forms one)."""
    mod = _golden_model(request.param)
    Kc = pn.cross(mod["Xc"], mod["X"], mod["th"], mod["kernel"])
    C = pn.cross(mod["Xc"], mod["Xc"], mod["th"], mod["kernel"]) - Kc @ mod["A"] @ Kc.T
    mod.update(C=0.5 * (C + C.T), mu=Kc @ mod["alpha"])
    return mod


def _args(mod):
    return mod["Xc"], mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"]


def _dense_greedy(C, mu, q, kind, mustar, noise_var):
    """Greedy picks by conditioning the dense covariance matrix itself after every pick."""
    C = C.copy()
    taken = np.zeros(len(mu), dtype=bool)
    picks = []
    for _ in range(q):
        sc = np.where(taken, -np.inf, bn.score_value(mu, np.diag(C), kind, mustar))
        p = int(np.argmax(sc))
        picks.append(p)
        taken[p] = True
        C = C - np.outer(C[:, p], C[p, :]) / (C[p, p] + noise_var)
    return np.array(picks), np.diag(C)


@pytest.mark.parametrize("kind", [bn.EI, bn.VARIANCE])
@pytest.mark.parametrize("noisy", [False, True])
def test_var_cond_is_the_schur_complement(dense, kind, noisy):
    """var_cond = diag(C - C[:, P] (C[P, P] + tau^2 I)^-1 C[P, :]) by np.linalg.solve on the dense covariance: 1e-9 sf^2
    (the picked block at tau = 0 is conditioned like the design's own Gramian, 1e4 .. 1e6)."""
    mod = dense
    sf2 = mod["th"][2] ** 2
    tau2 = mod["th"][0] ** 2 if noisy else 0.0
    mustar = float(np.quantile(mod["mu"], 0.9))
    out = bn.greedy(*_args(mod), Q, kind, mustar, tau2)
    P = out["idx"]
    assert (P >= 0).all() and len(set(P.tolist())) == Q
    C = mod["C"]
    S = C[np.ix_(P, P)] + tau2 * np.eye(Q)
    schur = np.diag(C) - np.einsum("ij,ji->i", C[:, P], np.linalg.solve(S, C[P, :]))
    assert np.abs(out["var"] - np.diag(C)).max() <= 1e-12 * sf2
    assert np.abs(out["mu"] - mod["mu"]).max() == 0.0
    assert np.abs(out["var_cond"] - np.maximum(schur, 0.0)).max() <= 1e-9 * sf2
    if not noisy:
        assert out["var_cond"][P].max() <= 1e-9 * sf2               # an exactly observed point has no variance left
    else:
        assert out["var_cond"][P].min() > 0.0
    # a replay of the same picks is the same loop
    rep = bn.replay(P, *_args(mod), kind, mustar, tau2)
    assert np.array_equal(rep["var_cond"], out["var_cond"]) and np.array_equal(rep["score"], out["score"])


@pytest.mark.parametrize("kind", [bn.EI, bn.VARIANCE])
@pytest.mark.parametrize("noisy", [False, True])
def test_picks_are_the_dense_greedys(dense, kind, noisy):
    mod = dense
    tau2 = mod["th"][0] ** 2 if noisy else 0.0
    mustar = float(np.quantile(mod["mu"], 0.9))
    out = bn.greedy(*_args(mod), Q, kind, mustar, tau2)
    picks, var_q = _dense_greedy(mod["C"], mod["mu"], Q, kind, mustar, tau2)
    assert out["gap"].min() > 1e-9, out["gap"]                      # the comparison of indices is meaningful
    assert np.array_equal(out["idx"], picks)
    assert np.abs(out["var_cond"] - np.maximum(var_q, 0.0)).max() <= 1e-9 * mod["th"][2] ** 2
    assert np.all(np.diff(out["score"]) <= 1e-12) or kind == bn.EI  # the largest variance left can only shrink


def test_exhaustion_nan_rows_and_huge_noise():
    mod = _golden_model("smoke")
    few = bn.greedy(mod["Xc"][:5], *_args(mod)[1:], 8, bn.VARIANCE, 0.0, 0.0)
    assert sorted(few["idx"][:5].tolist()) == [0, 1, 2, 3, 4] and (few["idx"][5:] == -1).all()
    assert np.isnan(few["score"][5:]).all() and not np.isnan(few["score"][:5]).any()
    Xb = mod["Xc"][:40].copy()
    Xb[7, 1] = np.nan
    clean = bn.greedy(np.delete(Xb, 7, axis=0), *_args(mod)[1:], 6, bn.EI, 0.1, 0.0)
    bad = bn.greedy(Xb, *_args(mod)[1:], 6, bn.EI, 0.1, 0.0)
    assert 7 not in bad["idx"] and np.isnan(bad["var_cond"][7]) and np.isnan(bad["mu"][7])
    assert np.abs(np.delete(bad["var_cond"], 7) - clean["var_cond"]).max() <= 1e-12 * mod["th"][2] ** 2
    allnan = bn.greedy(np.full((4, 3), np.nan), *_args(mod)[1:], 3, bn.EI, 0.0, 0.0)
    assert (allnan["idx"] == -1).all() and np.isnan(allnan["score"]).all()
    # nothing is conditioned under a huge noise: the q best scores in stable order, the variance untouched
    huge = bn.greedy(*_args(mod), Q, bn.EI, 0.1, 1e300)
    sc = bn.score_value(huge["mu"], huge["var"], bn.EI, 0.1)
    assert np.array_equal(huge["idx"], np.argsort(-sc, kind="stable")[:Q])
    assert np.array_equal(huge["var_cond"], huge["var"])


def test_binding_header_and_constants():
    from ppbo_amd import _lib, engine
    assert _lib.ABI_VERSION == 9
    assert len(_lib.SIGNATURES["ppbo_search_batch"]) == 14
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", txt)
    assert re.search(r"#define\s+PPBO_BATCH_MAX_Q\s+64\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "ppbo_search_batch" in set(re.findall(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(", code))
    assert _lib.BATCH_MAX_Q == engine.BATCH_MAX_Q == 64
    comment = txt[txt.index("---- shortlists"):txt.index("#define PPBO_BATCH_MAX_Q")]
    for needle in ("u_b = (Lambda + M'M) k_b", "max(var_j[c] - V_j[c]^2, 0)", "PPBO_SCORE_MEAN is refused", "bitwise equal",
                   "formed AGAIN per", "batch_step", "batch_field"):
        assert needle in comment, needle


def test_library_exports_the_entry_point():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    assert hasattr(_lib.load(), "ppbo_search_batch")


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
def test_search_batch_refuses_before_the_device(camphor):
    from ppbo_amd.engine import SCORE_MEAN, SCORE_VARIANCE, Posterior
    eng = _stub_engine()
    D = 6 if camphor else 4
    post = Posterior("SE_kernel", (0.05, 0.3, 1.0), 3, types.SimpleNamespace(shape=(8, 11 if camphor else D)), None, None,
                     None, None, camphor=np.ones(6) if camphor else None)
    z = np.zeros
    for Xc in (z((5, D + 1)), z(D), z((0, D)), z((5, D, 1))):
        with pytest.raises(ValueError, match="search_batch"):
            eng.search_batch(post, Xc, 4)
    for q in (0, -1, 65, 2.5):
        with pytest.raises(ValueError, match="search_batch"):
            eng.search_batch(post, z((5, D)), q)
    with pytest.raises(ValueError, match="score kind"):
        eng.search_batch(post, z((5, D)), 4, score=SCORE_MEAN)
    with pytest.raises(ValueError, match="score kind"):
        eng.search_batch(post, z((5, D)), 4, score=7)
    for nv in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise_var"):
            eng.search_batch(post, z((5, D)), 4, score=SCORE_VARIANCE, noise_var=nv)


def test_gpmodel_surface():
    from ppbo_amd.gp_model import GPModel
    sig = inspect.signature(GPModel.shortlist)
    assert list(sig.parameters) == ["self", "q", "score", "X_cand", "noise_var"]
    assert [sig.parameters[k].default for k in ("q", "score", "X_cand", "noise_var")] == [8, "EI", None, None]
    for needle in ("choice_pred", "ranking_pred", "tournament_pred"):
        assert needle in GPModel.shortlist.__doc__, needle
    gp = GPModel.__new__(GPModel)
    gp._post, gp.D = None, 3
    with pytest.raises(ValueError, match="shortlist"):
        gp.shortlist(score="mean")
    with pytest.raises(RuntimeError) as ref:
        gp.mu_Sigma_pred(np.zeros((2, 3)))
    with pytest.raises(RuntimeError) as e:
        gp.shortlist(X_cand=np.zeros((4, 3)))
    assert str(e.value) == str(ref.value)
