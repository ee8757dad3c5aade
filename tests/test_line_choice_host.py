"""CPU: the answer-prediction surface (ppbo_line_choice / Engine.line_choice / GPModel.answer_pred, choice_pred) -- the
NumPy statement of the model against the duel's closed form, the binding table, and the refusals that are decided on
shapes before anything reaches a device."""
import fnmatch
import os
import re
import types

import numpy as np
import pytest

import choice_numpy as cn
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"ppbo_line_choice": 15, "ppbo_line_choice_xi": 18}       # arguments of each


def test_restatement_against_the_duel_closed_form():
    """G = 2: the share of draws that pick point 0 is Phi(mu_d / sqrt(2 sigma^2 + var_d)) within 5 binomial standard
    errors, on pairs of the smoke fixture's line (strongly and weakly correlated, near ties and clear wins)."""
    g = load_golden("smoke")
    mu, cov, sigma = g["line_mu"], g["line_cov"], float(g["theta"][0])
    rng = np.random.default_rng(20)
    S = 200000
    z, e = rng.standard_normal((S, 2)), rng.standard_normal((S, 2))
    best = int(np.argmax(mu))
    pairs = [(0, 69), (10, 11), (best, (best + 35) % 70), (best, (best + 1) % 70), (30, 30), (69, 0)]
    for a, b in pairs:
        idx = [a, b]
        m2, c2 = mu[idx], cov[np.ix_(idx, idx)]
        for sd in (sigma, 0.0, 10.0 * sigma):
            jit = 1e-9 * float(g["theta"][2]) ** 2
            _, count, prob = cn.choice(m2, c2, z, e, sd, jit)
            p = cn.pair_closed_form(m2, c2, sd, jit)
            assert count.sum() == S and prob[0] + prob[1] == 1.0
            assert abs(prob[0] - p) <= 5.0 * np.sqrt(p * (1.0 - p) / S) + 1e-12, (a, b, sd, prob[0], p)


def test_restatement_rules():
    """Ties go to the lower index, the counts are the histogram of the choices, and the noise enters scaled."""
    mu, cov = np.zeros(3), np.zeros((3, 3))
    z = np.ones((4, 3))
    c, count, prob = cn.choice(mu, cov + np.eye(3), z)                 # u equal in every column: index 0
    assert list(c) == [0, 0, 0, 0] and list(count) == [4, 0, 0] and list(prob) == [1.0, 0.0, 0.0]
    e = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 2.0], [3.0, 0.0, 3.0], [0.0, 0.0, 0.0]])
    c, count, _ = cn.choice(mu, np.eye(3), z, e, 0.5)
    assert list(c) == [1, 2, 0, 0] and list(count) == [2, 1, 1]
    assert np.array_equal(cn.utilities(mu, np.eye(3), z, e, 0.5), 1.0 + 0.5 * e)
    assert np.array_equal(cn.top_two_gap(np.array([[1.0, 4.0, 2.5], [2.0, 2.0, 0.0]])), [1.5, 0.0])
    assert np.all(np.isinf(cn.top_two_gap(np.zeros((3, 1)))))


def test_binding_header_and_version_script():
    from ppbo_amd import _lib, engine
    assert _lib.ABI_VERSION == 9
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(([^)]*)\)", code)}
    script = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "ppbo_amd", "csrc", "libppbo_hip.map")).read(), flags=re.S)
    exported = [p.strip() for p in re.search(r"global:(.*?)local:", script, flags=re.S).group(1).split(";") if p.strip()]
    for name, nargs in ENTRIES.items():
        assert name in declared, f"{name} is not declared in include/ppbo_hip.h"
        assert len(declared[name].split(",")) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), f"{name} is not in the version script"
    # the header comment states the model and its rules
    comment = txt[txt.index("choice probabilities"):txt.index("PPBO_API int ppbo_line_choice(")]
    for word in ("noise_sd", "jitter", "LOWER index", "NaN never wins", "-1", "ppbo_predict_pairs", "invalid argument"):
        assert word in comment, word
    assert hasattr(engine.Engine, "line_choice") and hasattr(engine.Engine, "line_choice_xi")
    from ppbo_amd.gp_model import GPModel
    assert hasattr(GPModel, "answer_pred") and hasattr(GPModel, "choice_pred")


def test_library_exports_the_entry_points():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    lib = _lib.load()
    assert lib.ppbo_abi_version() == 9
    for name in ENTRIES:
        assert hasattr(lib, name)


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
def test_line_choice_refuses_shapes_before_the_device(camphor):
    from ppbo_amd.engine import Posterior
    eng = _stub_engine()
    D = 6 if camphor else 4
    post = Posterior("SE_kernel", (0.05, 0.3, 1.0), 3, types.SimpleNamespace(shape=(8, 11 if camphor else D)), None, None,
                     None, None, camphor=np.ones(6) if camphor else None)
    z = np.zeros
    bad = [dict(grid=z((3, 7, D + 1)), z=z((5, 7))),                       # width
           dict(grid=z((7, D)), z=z((5, 7))),                              # not [B, G, D]
           dict(grid=z((0, 7, D)), z=z((5, 7))),                           # no group
           dict(grid=z((3, 0, D)), z=z((5, 0))),                           # no point
           dict(grid=z((3, 129, D)), z=z((5, 129))),                       # G > 128
           dict(grid=z((3, 7, D)), z=z((5, 8))),                           # draws of another width
           dict(grid=z((3, 7, D)), z=z((0, 7))),                           # no draw
           dict(grid=z((3, 7, D)), z=z(7)),                                # draws not [S, G]
           dict(grid=z((3, 7, D)), z=z((5, 7)), e=z((4, 7))),              # noise draws of another shape
           dict(grid=z((3, 7, D)), z=z((5, 7))),                           # noise_sd = theta[0] > 0 without e
           dict(grid=z((3, 7, D)), z=z((5, 7)), e=z((5, 7)), noise_sd=-1.0),
           dict(grid=z((3, 7, D)), z=z((5, 7)), e=z((5, 7)), noise_sd=np.nan),
           dict(grid=z((3, 7, D)), z=z((5, 7)), e=z((5, 7)), noise_sd=np.inf),
           dict(grid=z((3, 7, D)), z=z((5, 7)), e=z((5, 7)), jitter=-1e-9),
           dict(grid=z((3, 7, D)), z=z((5, 7)), e=z((5, 7)), jitter=np.nan)]
    for kw in bad:
        with pytest.raises(ValueError, match="line_choice"):
            eng.line_choice(post, kw.pop("grid"), kw.pop("z"), **kw)
    xi, x, al = z((3, D)), z((3, D)), z(7)
    bad_xi = [dict(xis=z((3, D + 1)), xs=z((3, D + 1))), dict(xis=xi, xs=z((2, D))), dict(xis=z(D), xs=z(D)),
              dict(alphas=z((2, 7))), dict(alphas=z((3, 7, 1))), dict(alphas=z(129), z=z((5, 129)), e=z((5, 129))),
              dict(z=z((5, 6))), dict(e=None), dict(noise_sd=-0.5), dict(jitter=np.inf), dict(xis=z((0, D)), xs=z((0, D)))]
    for kw in bad_xi:
        a = dict(xis=xi, xs=x, alphas=al, z=z((5, 7)), e=z((5, 7)))
        a.update(kw)
        with pytest.raises(ValueError, match="line_choice_xi"):
            eng.line_choice_xi(post, **a)


def _stub_gp(D=3):
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = types.SimpleNamespace(G=object())
    gp.D, gp.theta, gp.COVARIANCE_SHRINKAGE, gp.eng = D, [0.05, 0.3, 1.0], 1e-6, _NoDevice()
    return gp


def test_answer_pred_and_choice_pred_refuse_before_the_device():
    gp = _stub_gp(3)
    z = np.zeros
    for kw in (dict(xi=z(4), x=z(4)), dict(xi=z(3), x=z((1, 3))), dict(xi=z((2, 3)), x=z((3, 3))), dict(xi=z((2, 2, 3)), x=z((2, 2, 3))),
               dict(xi=z((0, 3)), x=z((0, 3))), dict(xi=z(3), x=z(3), alphas=z((2, 5))), dict(xi=z(3), x=z(3), alphas=z(0)),
               dict(xi=z(3), x=z(3), alphas=z(129)), dict(xi=z(3), x=z(3), n_draws=0)):
        with pytest.raises(ValueError, match="answer_pred|n_draws"):
            gp.answer_pred(**kw)
    for kw in (dict(X_items=z(3)), dict(X_items=z((5, 4))), dict(X_items=z((129, 3))), dict(X_items=z((0, 3))),
               dict(X_items=z((0, 5, 3))), dict(X_items=z((2, 129, 3))), dict(X_items=z((2, 2, 5, 3))),
               dict(X_items=z((5, 3)), n_draws=-4)):
        with pytest.raises(ValueError, match="choice_pred|n_draws"):
            gp.choice_pred(**kw)


def test_without_a_variance_posterior_it_is_mu_Sigma_preds_error():
    from ppbo_amd.gp_model import GPModel
    for post in (None, types.SimpleNamespace(G=None)):
        gp = GPModel.__new__(GPModel)
        gp._post, gp.D = post, 3
        with pytest.raises(RuntimeError) as ref:
            gp.mu_Sigma_pred(np.zeros((2, 3)))
        with pytest.raises(RuntimeError) as a:
            gp.answer_pred(np.ones(3), np.zeros(3))
        with pytest.raises(RuntimeError) as c:
            gp.choice_pred(np.zeros((4, 3)))
        assert str(a.value) == str(c.value) == str(ref.value)
