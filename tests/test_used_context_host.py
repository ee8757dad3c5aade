"""CPU: the tables of tests/used_context_cases.py -- what tests/test_gpu_used_context.py relies on without checking it there."""
import os
import re

import numpy as np
import pytest

import used_context_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(uc.CASES)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def _flat(text):
    """A C comment block as running text: line breaks, the leading ' * ' and runs of blanks become one blank."""
    return re.sub(r"\s+", " ", re.sub(r"\n\s*\*\s", " ", text))


def test_the_tile_constants_are_the_code_s():
    predict, fused = _read("ppbo_amd", "csrc", "predict.hip"), _read("ppbo_amd", "csrc", "fused.hip")
    assert "ldk = (Mc_max + 127) & ~127" in predict and uc.CAND_TILE == 128
    assert "M >= 2048" in predict and uc.GPAD_FROM == 2048
    assert f"GRAD_CHUNK = {uc.GRAD_CHUNK};" in predict and f"LC_MAXROWS = {uc.LINE_ROWS};" in predict
    assert f"constexpr int BK = {uc.K_CHUNK};" in _read("ppbo_amd", "csrc", "gemm_f64.h")
    assert f"constexpr int FS_BN = {uc.FUSED_BN};" in fused
    assert f"constexpr int NB = {uc.DENSE_NB};" in _read("ppbo_amd", "csrc", "linalg.hip")
    assert f"constexpr int TS = {uc.DENSE_NB};" in _read("ppbo_amd", "csrc", "gram.hip")
    assert f"constexpr int TS = {uc.DENSE_NB};" in _read("ppbo_amd", "csrc", "rff.hip")
    assert f"constexpr int LNB = {uc.LU_NB};" in _read("ppbo_amd", "csrc", "lu.hip")
    assert f"(n + {uc.POINT_BLOCK - 1}) / {uc.POINT_BLOCK}" in _read("ppbo_amd", "csrc", "camphor.hip")


@pytest.mark.parametrize("name", NAMES)
def test_the_larger_history_dominates_and_leaves_other_tile_counts(name):
    """Strictly larger in every dimension that sizes a workspace, and another number of tiles or chunks."""
    case = uc.CASES[name]
    small, large = case.dims["checked"], case.dims["larger"]
    assert set(small) == set(large) and small
    assert all(large[k] > small[k] for k in small), (small, large)
    assert case.sizes("nonfinite") is large
    ts, tl = uc.tiles(small), uc.tiles(large)
    assert ts and ts != tl and all(tl[k] >= ts[k] for k in ts), (ts, tl)


@pytest.mark.parametrize("name", NAMES)
def test_the_smaller_history_is_a_legal_call(name):
    """The smallest sizes: nothing above the checked call's, N = n_q (m + 1) wherever the entry has a design."""
    case = uc.CASES[name]
    small, checked = case.dims["smaller"], case.dims["checked"]
    assert set(small) == set(checked)
    assert all(1 <= small[k] <= checked[k] for k in small) and any(small[k] < checked[k] for k in small)
    if case.legal is not None:
        n_q, m, N = case.legal
        assert n_q >= 1 and m >= 1 and N == n_q * (m + 1)
    for v in ("checked", "larger", "smaller"):
        d = case.dims[v]
        if "n_q" in d:
            assert d["N"] == d["n_q"] * (d["m"] + 1), (v, d)
        elif "m" in d:
            assert d["N"] % (d["m"] + 1) == 0, (v, d)


@pytest.mark.parametrize("name", NAMES)
def test_the_non_finite_input_is_documented(name):
    """Every non-finite history names the header line (quoted: it must be there) or the test that sends the input, or says
    that it sends finite 1e300 entries where the entry documents no non-finite input."""
    doc = uc.CASES[name].doc
    assert doc.startswith(("include/ppbo_hip.h:", "tests/", "finite but huge (1e300)", "a NaN entry of f", "takes sizes only")), doc
    header = _flat(_read("include", "ppbo_hip.h"))
    if doc.startswith("include/ppbo_hip.h: '"):
        quoted = re.search(r"'(.*)'", doc).group(1)
        assert _flat(quoted) in header, quoted
    elif doc.startswith("include/ppbo_hip.h:"):
        assert "PPBO_ERR_NOT_PD" in doc and "PPBO_ERR_NOT_PD" in header
    for path, test in re.findall(r"(tests/\w+\.py)::(\w+)", doc):
        assert f"def {test}(" in _read(*path.split("/")), (path, test)


def test_the_neighbours_sequences_hold_every_call_and_alternate_the_families():
    seen = []
    for env in uc.envs():
        seq = uc.neighbours(env)
        assert seq and all(uc.CASES[n].env == env for n in seq)
        fam = [uc.CASES[n].family for n in seq]
        for i in range(1, len(seq)):
            left = set(fam[i:])
            assert fam[i] != fam[i - 1] or left == {fam[i]}, (env, i, seq[i - 1], seq[i])
        seen += seq
    assert sorted(seen) == sorted(NAMES) and len(set(seen)) == len(seen)
    # the default engine's sequence starts fit, predict, RFF, LU, predictors, lines, ..., and comes back to the fit
    fam = [uc.CASES[n].family for n in uc.neighbours()]
    n = len(uc.FAMILY_ORDER)
    assert tuple(fam[:n]) == uc.FAMILY_ORDER and fam[n] == "fit"
    shared = {"WS_SMALL", "WS_VEC", "WS_LINALG", "WS_PART", "WS_KSTAR", "WS_TRANSPOSE"}
    for slot in shared:
        users = {uc.CASES[c].family for c in uc.neighbours() if slot in uc.CASES[c].slots}
        assert len(users) >= 2, (slot, users)


def test_every_case_has_a_call_and_a_reference():
    for case in uc.CASES.values():
        assert callable(case.run) and callable(case.ref) and case.family in uc.FAMILY_ORDER
        assert set(case.dims) == {"checked", "larger", "smaller"}


def test_every_slot_is_reached_or_has_a_reason():
    enum = re.search(r"enum \{ (WS_KSTAR = 0.*?), WS_COUNT \}", _read("ppbo_amd", "csrc", "common.h")).group(1)
    slots = [s.split("=")[0].strip() for s in enum.split(",")]
    assert len(slots) == 37
    reached = uc.reached()
    assert reached <= set(slots), reached - set(slots)
    assert set(slots) - reached == set(uc.UNREACHED), (set(slots) - reached, set(uc.UNREACHED))
    table = _read("tests", "test_gpu_used_context.py").split('"""')[1]
    assert all(s in table for s in slots)


@pytest.mark.parametrize("key", list(uc.MODELS))
@pytest.mark.parametrize("variant", ["checked", "larger", "smaller"])
def test_the_hand_built_posteriors(key, variant):
    """The layout of synth_post() and of operator() (tests/test_gpu_kstar_star.py), and the dense operator A: the variance
    prior - k' A k is the form's own sum sf^2 + k' Lambda k + |G k|^2 (node) or + |H E|^2 (edge), and stays positive."""
    import pairs_numpy as pn
    mod = uc.model(key, variant)
    N, mb, n_q = mod.N, mod.m + 1, mod.n_q
    assert N == n_q * mb and np.all(mod.lo[::mb] == 0.0) and np.all(mod.ld < 0.0)
    i, j = np.indices((N, N))
    if mod.form == uc.FORM_EDGE:
        assert np.all(mod.G[j > i] == 0.0) and np.all(mod.G[:n_q] == 0.0) and np.all(mod.G[:, :n_q] == 0.0)
    else:
        assert np.all(mod.G[j // mb > i // mb] == 0.0)
    Xc = uc.points(np.random.default_rng(0), mod, 40, "checked")
    K = pn.cross(Xc, mod.X, mod.theta, mod.kernel).T                       # [N, M]
    Ks = K.reshape(n_q, mb, -1)
    ko, lds, los = Ks[:, :1, :], mod.ld.reshape(n_q, mb, 1), mod.lo.reshape(n_q, mb, 1)
    t = (lds[:, :1] * ko ** 2).sum((0, 1)) + (Ks[:, 1:] * (lds[:, 1:] * Ks[:, 1:] + 2.0 * los[:, 1:] * ko)).sum((0, 1))
    if mod.form == uc.FORM_EDGE:
        E = np.zeros_like(K)
        E[n_q:] = (los[:, 1:] * (Ks[:, 1:] - ko)).reshape(n_q * mod.m, -1)
        Y = mod.G @ E
    else:
        Y = mod.G @ K
    var0 = mod.sf2 + t + (Y ** 2).sum(0)
    mu, var = mod.mean_var(Xc)
    assert np.abs(var - var0).max() <= 1e-12 * mod.sf2 and np.abs(mu - K.T @ mod.alpha).max() == 0.0
    assert var.min() > 0.05 * mod.sf2
    assert np.all(np.isnan(uc.points(np.random.default_rng(0), mod, 40, "nonfinite")[::7, 0]))


def test_the_references_preconditions():
    """What the GPU references assume of their seeded inputs, checked where it costs nothing: no near-tied pivot in the LU
    matrices, a projection-sized and a pruning-sized design of the stated shapes, inputs that are functions of (case,
    variant) alone."""
    import scipy.linalg
    import lu_ref as lr
    for n in (33, 257):
        lu, _ = scipy.linalg.lu_factor(lr.scaled_gaussian(n, n))
        assert lr.pivot_gap(lu) >= 1e-8
    assert uc.FITTED["prune"]["checked"][:3] == (3, 31, 20) and uc.FITTED["proj"]["checked"][:3] == (16, 25, 2)
    a, b = uc.rng_of("x", "larger").random(3), uc.rng_of("x", "nonfinite").random(3)
    assert np.array_equal(a, b) and not np.array_equal(a, uc.rng_of("x", "checked").random(3))
    assert uc.model("A", "checked") is uc.model("A", "checked")
