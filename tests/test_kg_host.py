"""CPU: the knowledge-gradient surface (ppbo_kg_envelope, ppbo_predict_kg / Engine.kg_envelope, Engine.predict_kg /
GPModel.kg_field, GPModel.knowledge_gradient) -- the binding table, the refusals decided on shapes alone, and the two
NumPy statements of the envelope (tests/kg_numpy.py) against each other and against closed forms.

Between the two statements the bound is 1e-15 (max|a| + max|b|): they sum the same kinks in the same order and differ
only where a near-degenerate line is kept by one and dropped by the other, a term of the size of its rounding."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import kg_numpy as kn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scale(a, b):
    return np.abs(a).max() + np.abs(b).max()


# ---------------------------------------------------------------- 1. the surface
def test_binding_header_and_constants():
    from ppbo_amd import _lib, engine
    assert _lib.ABI_VERSION == 9
    assert len(_lib.SIGNATURES["ppbo_kg_envelope"]) == 13 and len(_lib.SIGNATURES["ppbo_predict_kg"]) == 16
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", txt)
    assert re.search(r"#define\s+PPBO_KG_MAX_B\s+1024\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\bint\s+(ppbo_[a-z_A-Z0-9]+)\s*\(", code))
    assert {"ppbo_kg_envelope", "ppbo_predict_kg"} <= names
    assert _lib.KG_MAX_B == engine.KG_MAX_B == 1024
    comment = txt[txt.index("---- knowledge gradient"):txt.index("#define PPBO_KG_MAX_B")]
    for needle in ("Frazier, Powell and Dayanik 2009", "s_i = sqrt(v_i + tau^2)", "psi(c) = phi(c) - c Phi(-c)",
                   "NOT the answer to a preference query", "a counted loop", "SET of its lines", "poisons the field",
                   "should hold the current", "\"kg\""):
        assert needle in comment, needle
    # the version script exports the C-ABI by its prefix: the new entries need no line of their own
    assert "global: ppbo_*;" in open(os.path.join(ROOT, "ppbo_amd", "csrc", "libppbo_hip.map")).read()
    # the new profile slot at the end of its enum, the new source in the build
    common = open(os.path.join(ROOT, "ppbo_amd", "csrc", "common.h")).read()
    assert re.search(r"PF_ACQ_GRAD,\s*PF_KG,\s*PF_COUNT", common)
    assert re.search(r'"acq_grad",\s*"kg"\s*\}', open(os.path.join(ROOT, "ppbo_amd", "csrc", "capi.hip")).read())
    from ppbo_amd.build import SOURCES
    assert "kg.hip" in SOURCES


def test_library_exports_the_entry_points():
    from ppbo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from ppbo_amd.build import build
        build(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "ppbo_kg_envelope") and hasattr(lib, "ppbo_predict_kg")
    assert lib.ppbo_abi_version() == 9


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
def test_predict_kg_refuses_before_the_device(camphor):
    from ppbo_amd.engine import Posterior
    eng = _stub_engine()
    D = 6 if camphor else 4
    post = Posterior("SE_kernel", (0.05, 0.3, 1.0), 3, types.SimpleNamespace(shape=(8, 11 if camphor else D)), None, None,
                     None, None, camphor=np.ones(6) if camphor else None)
    z = np.zeros
    for Xa, Xb in ((z((5, D)), z((4, D + 1))), (z((5, D + 1)), z((4, D))), (z(D), z((4, D))), (z((5, D)), z(D)),
                   (z((0, D)), z((4, D))), (z((5, D)), z((0, D))), (z((5, D, 1)), z((4, D))), (z((5, D)), z((1025, D)))):
        with pytest.raises(ValueError, match="predict_tournament"):       # the shape checks are the tournament's
            eng.predict_kg(post, Xa, Xb)
    for nv in (-1e-300, -1.0, np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match="noise_var"):
            eng.predict_kg(post, z((5, D)), z((4, D)), noise_var=nv)


def test_kg_envelope_refuses_before_the_device():
    eng = _stub_engine()
    z = np.zeros
    for a, s in ((z((3, 1)), z((5, 3))), (z(3), z(3)), (z(3), z((5, 4))), (z(3), z((0, 3))), (z(0), z((5, 0))),
                 (z(1025), z((2, 1025))), (z(3), z((5, 3, 1)))):
        with pytest.raises(ValueError, match="kg_envelope"):
            eng.kg_envelope(a, s)
    for sa, sb in ((z(5), None), (None, z(5)), (z(4), z(5)), (z(5), z((5, 1)))):
        with pytest.raises(ValueError, match="kg_envelope"):
            eng.kg_envelope(z(3), z((5, 3)), sa, sb)


def test_engine_and_gpmodel_surface():
    from ppbo_amd.engine import Engine
    from ppbo_amd.gp_model import GPModel
    sig = inspect.signature(Engine.predict_kg)
    assert list(sig.parameters) == ["self", "post", "Xa", "Xb", "noise_var", "want_kinks", "want_best"]
    assert [sig.parameters[k].default for k in ("noise_var", "want_kinks", "want_best")] == [None, False, True]
    sig = inspect.signature(Engine.kg_envelope)
    assert list(sig.parameters) == ["self", "a", "slopes", "self_a", "self_b"]
    assert (sig.parameters["self_a"].default, sig.parameters["self_b"].default) == (None, None)
    sig = inspect.signature(GPModel.kg_field)
    assert list(sig.parameters) == ["self", "n"] and sig.parameters["n"].default == 64
    sig = inspect.signature(GPModel.knowledge_gradient)
    assert list(sig.parameters) == ["self", "X_cand", "field", "noise_var"]
    assert all(p.default is None for k, p in sig.parameters.items() if k != "self")
    assert "MUST be in the field" in GPModel.kg_field.__doc__ and "inflates" in GPModel.kg_field.__doc__
    doc = " ".join(GPModel.knowledge_gradient.__doc__.split())
    assert "shortlist's convention" in doc and "NOT the answer to a preference query" in doc
    gp = GPModel.__new__(GPModel)
    gp.D, gp.xstar, gp.xstars_local = 3, None, None
    with pytest.raises(RuntimeError, match="kg_field"):
        gp.kg_field()
    gp.xstar = np.array([0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="kg_field"):
        gp.kg_field(0)
    with pytest.raises(ValueError, match="kg_field"):
        gp.kg_field(1025)
    # xstar first, then the local maxima: a field that they fill needs no shortlist (and no device)
    gp.xstars_local = np.arange(12.0).reshape(4, 3) / 12.0
    f = gp.kg_field(3)
    assert f.shape == (3, 3) and np.array_equal(f[0], gp.xstar) and np.array_equal(f[1:], gp.xstars_local[:2])
    assert np.array_equal(gp.kg_field(1), gp.xstar.reshape(1, 3))


# ---------------------------------------------------------------- 2. the two statements against each other
def _agree(a, b, what):
    k1, n1 = kn.kg_stack(a, b)
    k2, n2 = kn.kg_march(a, b)
    assert abs(k1 - k2) <= 1e-15 * _scale(a, b), (what, k1, k2, n1, n2)
    assert 0 <= n2 <= len(a) - 1 and 0 <= n1 <= len(a) - 1
    return k2, n2


def test_statements_agree_on_random_lines():
    rng = np.random.default_rng(0)
    worst = 0.0
    for case in range(300):
        n = int(rng.integers(1, 200))
        a = rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2)
        b = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)
        k1, k2 = kn.kg_stack(a, b)[0], kn.kg_march(a, b)[0]
        worst = max(worst, abs(k1 - k2) / _scale(a, b))
        _agree(a, b, case)
    print(f"stack against march, random lines: worst {worst:.2e} of max|a| + max|b|")


def test_statements_agree_on_gp_shaped_lines():
    """Slopes that are a smooth function of the intercepts' positions plus a common sign: a handful of kinks among many
    lines, the shape ppbo_predict_kg feeds the kernel."""
    rng = np.random.default_rng(1)
    for case in range(100):
        n = int(rng.choice([16, 64, 256, 1024]))
        x = rng.random(n)
        a = np.sin(6.0 * x + rng.uniform(0, 6)) + 0.3 * rng.standard_normal(n)
        b = 0.2 * np.exp(-0.5 * ((x - rng.random()) / 0.2) ** 2) * rng.choice([-1.0, 1.0]) + 1e-3 * rng.standard_normal(n)
        kg, kinks = _agree(a, b, case)
        assert kinks <= 40


def test_statements_agree_on_integer_lines():
    """Small integers: equal slopes, equal intercepts and three lines through one point in most rows."""
    rng = np.random.default_rng(2)
    for case in range(300):
        n = int(rng.integers(1, 40))
        a, b = rng.integers(-3, 4, n).astype(float), rng.integers(-3, 4, n).astype(float)
        kg, kinks = _agree(a, b, case)
        assert kinks <= len(np.unique(b)) - 1


def test_tangent_family_every_line_is_on_the_envelope():
    a, b = kn.tangents(40)
    kg, kinks = _agree(a, b, "tangents")
    assert kinks == 39 and kn.kg_stack(a, b)[1] == 39
    assert kg > 0.0
    assert kn.kg_march(*kn.tangents(1024))[1] == 1023 and kn.kg_stack(*kn.tangents(1024))[1] == 1023


def test_two_lines_closed_form():
    rng = np.random.default_rng(3)
    for _ in range(200):
        a, b = rng.standard_normal(2), rng.standard_normal(2)
        db = abs(b[1] - b[0])
        want = db * kn.psi(abs((a[0] - a[1]) / (b[1] - b[0])))
        for fn in (kn.kg_stack, kn.kg_march):
            kg, kinks = fn(a, b)
            assert kinks == 1 and abs(kg - want) <= 1e-15 * _scale(a, b)
    assert kn.kg_march([1.0, 2.0], [0.5, 0.5]) == (0.0, 0)          # parallel: the lower one never shows
    assert kn.kg_march([1.0], [3.0]) == (0.0, 0)
    assert kn.psi(0.0) == kn.INV_SQRT_2PI and kn.psi(40.0) == 0.0 and kn.psi(np.inf) == 0.0


def test_against_dense_quadrature():
    """E[max] by a dense trapezoid on [-10, 10]: an independent third statement, to the quadrature's own 1e-6."""
    rng = np.random.default_rng(4)
    z = np.linspace(-10.0, 10.0, 200001)
    w = np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) * (z[1] - z[0])
    for _ in range(10):
        n = int(rng.integers(2, 30))
        a, b = rng.standard_normal(n), rng.standard_normal(n)
        h = np.max(a[:, None] + b[:, None] * z[None, :], axis=0)
        want = np.sum(h * w) - a.max()
        assert abs(kn.kg_march(a, b)[0] - want) <= 1e-6 * _scale(a, b)


# ---------------------------------------------------------------- 3. properties of the march
def test_march_is_bitwise_invariant_under_permutation_and_duplication():
    rng = np.random.default_rng(5)
    for case in range(100):
        n = int(rng.integers(2, 120))
        if case % 2:
            a, b = rng.integers(-3, 4, n).astype(float), rng.integers(-3, 4, n).astype(float)
        else:
            a, b = rng.standard_normal(n), rng.standard_normal(n)
        ref = kn.kg_march(a, b)
        p = rng.permutation(n)
        assert kn.kg_march(a[p], b[p]) == ref
        assert kn.kg_march(np.tile(a, 2), np.tile(b, 2)) == ref
        q = rng.integers(0, n, 3 * n)                                # some lines three times, some not at all ...
        full = np.concatenate([np.arange(n), q])                     # ... on top of every line once
        assert kn.kg_march(a[full], b[full]) == ref


def test_kg_is_nonnegative_and_monotone_in_the_slope_scale():
    rng = np.random.default_rng(6)
    for _ in range(100):
        n = int(rng.integers(1, 80))
        a, b = rng.standard_normal(n), rng.standard_normal(n)
        prev = 0.0
        for f in (0.0, 1e-3, 0.1, 0.5, 1.0, 2.0, 10.0):
            kg = kn.kg_march(a, f * b)[0]
            assert kg >= 0.0
            assert kg >= prev - 1e-15 * _scale(a, f * b), (f, kg, prev)
            prev = kg
    assert kn.kg_march(rng.standard_normal(9), np.zeros(9)) == (0.0, 0)


def test_nan_rules_and_the_row_helpers():
    a, b = np.array([0.0, 1.0, 2.0]), np.array([1.0, 0.0, -1.0])
    for bad in (np.nan, np.inf, -np.inf):
        for arr in (0, 1):
            x = [a.copy(), b.copy()]
            x[arr][1] = bad
            for fn in (kn.kg_stack, kn.kg_march):
                kg, kinks = fn(*x)
                assert np.isnan(kg) and kinks == 0
    slopes = np.array([[1.0, 0.0, -1.0], [np.nan, 0.0, 1.0], [0.5, 0.5, 0.5]])
    kg, kinks = kn.rows(a, slopes)
    # (row 0: the three lines meet in (1, 1) -- one kink, from the flattest line straight to the steepest)
    assert np.isnan(kg[1]) and kg[0] > 0.0 and kg[2] == 0.0 and list(kinks) == [1, 0, 0]
    assert kn.best(kg) == (kg[0], 0) and kn.best([np.nan, np.nan])[1] == -1
    kg2, _ = kn.rows(a, slopes, self_a=np.array([5.0, 5.0, 5.0]), self_b=np.array([0.0, 0.0, 2.0]))
    assert kg2[0] < kg[0] and np.isnan(kg2[1]) and kg2[2] > 0.0
    # the lines of a posterior: s = 0 gives slopes 0, a NaN variance a NaN row
    la, ls, sa, sb = kn.lines_from_posterior([1.0, 2.0, 3.0], [0.0, 4.0, np.nan], [0.5, 0.7], [[0.0, 0.0], [1.0, 2.0], [1.0, 1.0]], 0.0)
    assert np.array_equal(ls[0], [0.0, 0.0]) and sb[0] == 0.0 and np.array_equal(ls[1], [0.5, 1.0]) and sb[1] == 2.0
    assert np.all(np.isnan(ls[2])) and np.isnan(sb[2])
    kg3, _ = kn.rows(la, ls, sa, sb)
    assert kg3[0] == 0.0 and kg3[1] > 0.0 and np.isnan(kg3[2])
    # a field point that is the candidate (coordinates and mean) takes the own line's slope; equal coordinates alone do not
    Xa, Xb = np.array([[0.1, 0.2], [0.3, 0.4]]), np.array([[0.3, 0.4], [0.1, 0.2], [0.1, 0.25]])
    _, ls, _, sb = kn.lines_from_posterior([1.0, 2.0], [4.0, 9.0], [2.0, 1.5, 1.0], [[1.0, 1.9, 0.5], [2.9, 1.0, 0.5]], 0.0, Xa, Xb)
    assert np.array_equal(ls, [[0.5, 0.95, 0.25], [3.0, 1.0 / 3.0, 0.5 / 3.0]]) and np.array_equal(sb, [2.0, 3.0])
