"""CPU: the answer scores (ppbo_loo_answers / ppbo_score_answers, GPModel.loo_pred and its companions) -- the NumPy
statement (tests/loo_numpy.py) against itself by a second route, against exact leave-one-query-out refits and on a design
with one flipped answer, and the surface: header, binding table, sources, workspace slots, and the refusals that are decided
before anything reaches a device."""
import functools
import os
import re
import types

import numpy as np
import pytest

import loo_numpy as ln
from conftest import load_golden
from oracle import ppbo_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"ppbo_loo_answers": 18, "ppbo_score_answers": 13}       # arguments of each
THETA = [0.05, 0.3, 0.5]                                           # the flipped design's hyper-parameters
FLIPPED = 5


def _posterior(X, f, m, theta, kernel):
    Sinv = orc.pd_inverse(orc.gram(X, theta, kernel))
    return orc.posterior_covariance(Sinv, f, m, theta[0])


@pytest.mark.parametrize("name", ["smoke", "rq", "cam_small", "c2"])
def test_schur_route_against_dense_route(name):
    """The cavity from the star's block alone equals the one from all of Q = P^-1 with Lambda_q added to that block:
    covariance <= 1e-7 max|C_q|, mean <= 1e-8; every cavity of these fixtures is positive definite."""
    g = load_golden(name)
    X, m, th, f = g["X"], int(g["m"]), [float(v) for v in g["theta"]], g["fMAP"].ravel()
    P = _posterior(X, f, m, th, str(g["kernel"]))
    r = ln.loo(P, f, m, th[0])
    assert np.all(r["info"] == 0) and np.all(r["min_eig"] > 0.0), (r["info"], r["min_eig"].min())
    b = m + 1
    worst_c = worst_m = 0.0
    for q in range(len(f) // b):
        I = slice(q * b, (q + 1) * b)
        md, Cd = ln.cavity_dense(P, f, q, m, th[0])
        worst_c = max(worst_c, np.abs(Cd - r["cav_cov"][q]).max() / np.abs(r["cav_cov"][q]).max())
        worst_m = max(worst_m, np.abs(md - r["cav_mean"][I]).max())
    print(f"{name}: cavity block route against dense route: cov {worst_c:.2e} (rel), mean {worst_m:.2e}; "
          f"min eig of the cavity precisions {r['min_eig'].min():.3g}")
    assert worst_c <= 1e-7 and worst_m <= 1e-8


def test_agreement_is_one_plus_the_expected_log_likelihood():
    """a = mean_j p_j = 1 + E[l], by the statement's own draws to within 5 standard errors of that sample."""
    g = load_golden("smoke")
    m, th, f = int(g["m"]), [float(v) for v in g["theta"]], g["fMAP"].ravel()
    P = _posterior(g["X"], f, m, th, str(g["kernel"]))
    r = ln.loo(P, f, m, th[0])
    b = m + 1
    z = np.random.default_rng(7).standard_normal((20000, b))
    for q in range(len(f) // b):
        I = slice(q * b, (q + 1) * b)
        l = ln.ell(ln.draws(r["cav_mean"][I], r["cav_cov"][q], z), th[0])
        se = l.std(ddof=1) / np.sqrt(len(l))
        assert abs(1.0 + l.mean() - r["agree"][q]) <= 5.0 * se + 1e-12, (q, 1.0 + l.mean(), r["agree"][q], se)


@functools.lru_cache(maxsize=None)
def _flipped_fit(flip):
    """The 12-query design (one answer replaced by the worst point of its line where flip is set), fitted by the oracle."""
    m = 15
    X = ln.flipped_design(12, m, 2, 3, flip)
    Sig = orc.gram(X, THETA, "SE_kernel")
    Sinv = orc.pd_inverse(Sig)
    f, _ = orc.fit_fmap_trust_exact(np.zeros(len(X)), Sinv, m, THETA[0], maxiter=500)
    P = orc.posterior_covariance(Sinv, f, m, THETA[0])
    z = np.random.default_rng(0).standard_normal((4096, m + 1))
    return dict(X=X, m=m, Sig=Sig, f=f, P=P, loo=ln.loo(P, f, m, THETA[0], z))


def test_a_flipped_answer_is_the_minimum_of_both_scores():
    """Query 5 answered with the worst point of its line: the argmin of lpd and of the agreement, each by >= 0.05."""
    r = _flipped_fit(FLIPPED)["loo"]
    for key in ("lpd", "agree"):
        s = r[key]
        order = np.argsort(s)
        print(f"flipped design, {key}: query {order[0]} at {s[order[0]]:.3f}, runner-up {order[1]} at {s[order[1]]:.3f}")
        assert order[0] == FLIPPED
        assert s[order[1]] - s[order[0]] >= 0.05


@pytest.mark.parametrize("flip", [None, FLIPPED])
def test_cavity_agreement_against_exact_refits(flip):
    """The cavity's agreement against the agreement under a REFIT without the query (its own f_MAP and posterior on the
    kept rows, then the prediction at the left-out star): max|difference| <= 0.06."""
    d = _flipped_fit(flip)
    X, m, Sig, f = d["X"], d["m"], d["Sig"], d["f"]
    b, N = m + 1, len(d["f"])
    worst = 0.0
    for q in range(N // b):
        keep = np.r_[0:q * b, (q + 1) * b:N]
        I = np.arange(q * b, (q + 1) * b)
        S11i = orc.pd_inverse(Sig[np.ix_(keep, keep)])
        # from the full fit's f restricted to the kept rows (trust-exact from zeros produced NaNs on the reduced designs)
        f1, _ = orc.fit_fmap_trust_exact(f[keep], S11i, m, THETA[0], maxiter=500)
        P1 = orc.posterior_covariance(S11i, f1, m, THETA[0])
        Ks = Sig[np.ix_(I, keep)]
        mu = Ks @ (S11i @ f1)
        C = Sig[np.ix_(I, I)] - Ks @ (S11i - S11i @ P1 @ S11i) @ Ks.T
        worst = max(worst, abs(ln.answer_scores(mu, C, THETA[0])["agree"] - d["loo"]["agree"][q]))
    print(f"flip={flip}: cavity agreement against refits: max|diff| = {worst:.4f}")
    assert worst <= 0.06


def test_status_of_the_statement():
    """A block of P with a negative diagonal entry is info 1; a cavity made indefinite (large P, Delta = -1, small sigma) is
    info 2; both NaN."""
    b, sigma = 4, 0.01
    f = np.array([sigma, 0.0, 0.0, 0.0])                     # Delta_j = -1: w_j < 0
    mq, Cq, info, K = ln.cavity(100.0 * np.eye(b), f, sigma)
    assert info == 2 and np.isnan(mq).all() and np.isnan(Cq).all() and np.linalg.eigvalsh(K).min() < 0.0
    Pb = np.eye(b)
    Pb[2, 2] = -1.0
    assert ln.cavity(Pb, f, sigma)[2] == 1
    assert ln.cavity(np.eye(b), np.zeros(b), 1.0)[2] == 0


# ------------------------------------------------------------------------------------------------------ the surface
def test_header_binding_sources_and_slots():
    from ppbo_amd import _lib, build, engine
    from ppbo_amd.gp_model import GPModel
    assert _lib.ABI_VERSION == 9
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(([^)]*)\)", code)}
    for name, nargs in ENTRIES.items():
        assert name in declared, f"{name} is not declared in include/ppbo_hip.h"
        assert len(declared[name].split(",")) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs
        assert not name.endswith(("_edge", "_scaled", "_camphor"))
    comment = txt[txt.index("scoring the answers"):txt.index("PPBO_API int ppbo_loo_answers(")]
    for word in ("src/gp_model.py:176-226", "no reference counterpart", "ppbo_loo_answers", "ppbo_score_answers",
                 "invalid argument", "d_info", "jitter", "ppbo_randn"):
        assert word in comment, word
    assert "answers.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "answers.hip"))
    common = open(os.path.join(ROOT, "ppbo_amd", "csrc", "common.h")).read()
    slots = re.search(r"enum \{ (WS_KSTAR = 0.*?), WS_COUNT \}", common).group(1).split(",")
    assert len(slots) == 37
    for meth in ("loo_answers", "score_answers"):
        assert hasattr(engine.Engine, meth)
    for meth in ("loo_pred", "inconsistent_answers", "answers_score", "loo_score"):
        assert hasattr(GPModel, meth)


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


def test_engine_refuses_before_the_device():
    from ppbo_amd.engine import Posterior
    eng = _stub_engine()
    z = np.zeros
    ok = dict(P=z((8, 8)), f=z(8), m=3, sigma=0.1, z=z((5, 4)))
    bad = [dict(P=z((8, 7))), dict(P=z(8)), dict(f=z(7)), dict(m=0), dict(m=2), dict(m=128), dict(sigma=0.0),
           dict(sigma=-1.0), dict(sigma=np.nan), dict(sigma=np.inf), dict(jitter=-1e-9), dict(jitter=np.nan),
           dict(z=z((5, 3))), dict(z=z((0, 4))), dict(z=z(4)), dict(z=None, S=-1), dict(P=z((0, 0)), f=z(0))]
    for kw in bad:
        a = dict(ok)
        a.update(kw)
        with pytest.raises(ValueError, match="loo_answers"):
            eng.loo_answers(**a)
    post = Posterior("SE_kernel", (0.05, 0.3, 1.0), 3, types.SimpleNamespace(shape=(8, 4)), None, None, None, None)
    for kw in (dict(groups=z((3, 4))), dict(groups=z((3, 5, 3))), dict(groups=z((0, 5, 4))), dict(groups=z((3, 1, 4))),
               dict(groups=z((3, 129, 4)), z=z((5, 129))), dict(groups=z((3, 5, 4)), z=z((5, 4))),
               dict(groups=z((3, 5, 4)), z=z((0, 5))), dict(groups=z((3, 5, 4)), S=-2),
               dict(groups=z((3, 5, 4)), z=z((5, 5)), jitter=-1.0), dict(groups=z((3, 5, 4)), z=z((5, 5)), jitter=np.inf)):
        with pytest.raises(ValueError, match="score_answers"):
            eng.score_answers(post, **kw)


def test_gp_model_refuses_before_the_device():
    from ppbo_amd.gp_model import GPModel
    gp = GPModel.__new__(GPModel)
    gp._post = types.SimpleNamespace(G=object(), P=object())
    gp.D, gp.m, gp.theta, gp.COVARIANCE_SHRINKAGE, gp.eng = 3, 4, [0.05, 0.3, 1.0], 1e-6, _NoDevice()
    z = np.zeros
    for kw in (dict(X_stars=z(3)), dict(X_stars=z((5, 4))), dict(X_stars=z((7, 3))), dict(X_stars=z((0, 3))),
               dict(X_stars=z((2, 5, 3))), dict(X_stars=z((10, 3)), n_draws=0)):
        with pytest.raises(ValueError, match="answers_score|n_draws"):
            gp.answers_score(**kw)
    for post in (None, types.SimpleNamespace(G=None)):
        gp._post = post
        with pytest.raises(RuntimeError) as ref:
            gp.mu_Sigma_pred(np.zeros((2, 3)))
        for call in (lambda: gp.loo_pred(), lambda: gp.inconsistent_answers(2), lambda: gp.answers_score(z((10, 3))),
                     lambda: gp.loo_score()):
            with pytest.raises(RuntimeError) as e:
                call()
            assert str(e.value) == str(ref.value)
