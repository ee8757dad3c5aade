"""GPU: tournaments -- ppbo_predict_tournament / Engine.predict_tournament / GPModel.tournament_pred, borda_pred and
ranking_pred against the NumPy statement (tests/tournament_numpy.py on pairs_numpy's kernels and the oracle's dense
variance operator), the exact identities of the construction, the existing duel entry, the shapes that take other
branches, NaN rows and columns, and the refusals.  The star design of test_gpu_pairs: n_q = 7, m = 25, N = 182.

Worst errors measured on MI355X are recorded in DESIGN.md section 7 ("Tournaments")."""
import ctypes as C
import functools

import numpy as np
import pytest

import slopes_numpy as sn
import tournament_numpy as tn
from test_gpu_pairs import RADIAL, TOL, _fitted, _fitted_golden, _forms, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _sets(rng, mod, Ma, Mb):
    """Candidates and opponents in the box: uniform points, a few design rows in either set."""
    N, D = mod["X"].shape
    Xa, Xb = rng.random((Ma, D)), rng.random((Mb, D))
    ka, kb = min(8, Ma // 4), min(4, Mb // 4)
    Xa[:ka] = mod["X"][rng.integers(0, N, ka)]
    Xb[:kb] = mod["X"][rng.integers(0, N, kb)]
    return Xa, Xb


def _full(eng, post, Xa, Xb, **kw):
    from ppbo_amd.engine import TOURNAMENT_BORDA
    kw.setdefault("score", TOURNAMENT_BORDA)
    out = eng.predict_tournament(post, Xa, Xb, want_cov=True, want_prob=True, **kw)
    return {k: (host(v) if hasattr(v, "cpu") else v) for k, v in out.items()}


def _parity(eng, mod, Ma=300, Mb=200, seed=3, label="", cross=None):
    from ppbo_amd.engine import TOURNAMENT_WORST
    Xa, Xb = _sets(np.random.default_rng(seed), mod, Ma, Mb)
    out = _full(eng, mod["post"], Xa, Xb)
    worst = eng.predict_tournament(mod["post"], Xa, Xb, score=TOURNAMENT_WORST)
    kw = {} if cross is None else dict(cross=cross)
    ref = tn.tournament_reference(Xa, Xb, mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"], **kw)
    p0 = tn.win_matrix(ref, mod["th"][0])
    sf2 = float(mod["th"][2]) ** 2
    mx = max(np.abs(ref["mu_a"]).max(), np.abs(ref["mu_b"]).max())
    var_d = out["var_a"][:, None] + out["var_b"][None, :] - 2.0 * out["cov"]
    e = dict(mu=max(np.abs(out["mu_a"] - ref["mu_a"]).max(), np.abs(out["mu_b"] - ref["mu_b"]).max()) / mx,
             var=max(np.abs(out["var_a"] - ref["var_a"]).max(), np.abs(out["var_b"] - ref["var_b"]).max()) / sf2,
             cov=np.abs(out["cov"] - ref["cov"]).max() / sf2, var_d=np.abs(var_d - ref["var_d"]).max() / sf2,
             p=np.abs(out["prob"] - p0).max(), borda=np.abs(out["score"] - tn.scores(p0, tn.BORDA)).max(),
             worst=np.abs(host(worst["score"]) - tn.scores(p0, tn.WORST)).max())
    print(f"tournament parity {label}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), e
    for o, sc in ((out, out["score"]), (worst, host(worst["score"]))):
        assert o["best_idx"] == int(np.argmax(sc)) and o["best_val"] == sc.max()


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("D", [6, 20, 40])
@pytest.mark.parametrize("kernel", RADIAL)
def test_parity_radial(eng, kernel, D, form):
    """Ma = 300 against Mb = 200: two opponent tiles, the last one ragged.  Figures measured on MI355X: this test's
    docstring is the pointer, DESIGN.md section 7 holds them."""
    _parity(eng, _fitted(kernel, D, _forms()[form]), label=f"{kernel} D={D} {form}")


def test_parity_ard(eng):
    _parity(eng, _fitted("Matern52_kernel", 6, None, ard=True), label="Matern52 ARD D=6")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_camphor(eng, form):
    """kernel id 2: the small opponent tile whatever Mb is (7 tiles of 32 here)."""
    _parity(eng, _fitted_golden("cam_small", _forms()[form]), label=f"camphor cam_small {form}")


def test_parity_camphor_ard(eng):
    """camphor_ard/spread: embedded rows (D = 11, SE) behind Engine._points."""
    from test_gpu_marginals import _fitted_camphor_ard_golden
    _parity(eng, _fitted_camphor_ard_golden(), label="camphor ARD camphor_ard/spread", cross=sn.cross)


# ---------------------------------------------------------------- 2. exact identities
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("Matern52_kernel", 20), ("RQ_kernel", 40)])
def test_exact_identities(eng, kernel, D, form):
    from ppbo_amd.engine import TOURNAMENT_WORST
    mod = _fitted(kernel, D, _forms()[form])
    post = mod["post"]
    Xa, Xb = _sets(np.random.default_rng(5), mod, 777, 200)
    out = _full(eng, post, Xa, Xb)
    pa, pb = eng.predict(post, Xa), eng.predict(post, Xb)
    assert np.array_equal(out["mu_a"], host(pa["mu"])) and np.array_equal(out["var_a"], host(pa["var"]))
    assert np.array_equal(out["mu_b"], host(pb["mu"])) and np.array_equal(out["var_b"], host(pb["var"]))
    again = _full(eng, post, Xa, Xb)
    for k in ("mu_a", "var_a", "mu_b", "var_b", "cov", "prob", "score"):
        assert np.array_equal(out[k], again[k]), k
    assert (out["best_idx"], out["best_val"]) == (again["best_idx"], again["best_val"])
    # a row's outputs do not depend on the other rows of the call
    head = _full(eng, post, Xa[:100], Xb)
    for k in ("mu_a", "var_a", "cov", "prob", "score"):
        assert np.array_equal(out[k][:100], head[k]), k
    # the scores do not depend on whether the matrices are written
    lean = eng.predict_tournament(post, Xa, Xb)
    assert lean["cov"] is None and lean["prob"] is None
    assert np.array_equal(host(lean["score"]), out["score"])
    assert (lean["best_idx"], lean["best_val"]) == (out["best_idx"], out["best_val"])
    # the reductions against the returned matrix
    assert np.abs(out["score"] - tn.scores(out["prob"], tn.BORDA)).max() <= 1e-15 * Xb.shape[0]
    for kw in (dict(want_prob=True), dict()):
        worst = eng.predict_tournament(post, Xa, Xb, score=TOURNAMENT_WORST, **kw)
        assert np.array_equal(host(worst["score"]), out["prob"].min(axis=1))
        assert worst["best_idx"] == int(np.argmax(out["prob"].min(axis=1)))


# ---------------------------------------------------------------- 3. against the existing duel entry
def _against_pairs(eng, mod, Xa, Xb, label):
    out = _full(eng, mod["post"], Xa, Xb)
    Ma, Mb = len(Xa), len(Xb)
    duel = eng.predict_pairs(mod["post"], np.repeat(Xa, Mb, axis=0), np.tile(Xb, (Ma, 1)), want_best=False)
    var_d = out["var_a"][:, None] + out["var_b"][None, :] - 2.0 * out["cov"]
    sf2 = float(mod["th"][2]) ** 2
    e_p = np.abs(out["prob"] - host(duel["prob"]).reshape(Ma, Mb)).max()
    e_v = np.abs(var_d - host(duel["var"]).reshape(Ma, Mb)).max() / sf2
    print(f"tournament against predict_pairs {label}: |p - duel| = {e_p:.2e}, |var_d - duel| / sf2 = {e_v:.2e}")
    assert e_p <= TOL and e_v <= TOL
    return out, var_d


@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("Matern32_kernel", 20)])
def test_against_predict_pairs(eng, kernel, D, form):
    mod = _fitted(kernel, D, _forms()[form])
    rng = np.random.default_rng(14)
    Xa, Xb = _sets(rng, mod, 777, 33)
    _against_pairs(eng, mod, Xa, Xb, f"{kernel} D={D} {form} 777 x 33")
    _against_pairs(eng, mod, Xa[:50], Xb[:1], f"{kernel} D={D} {form} 50 x 1")
    # opponents taken from the candidates: identical points are a tie
    idx = rng.choice(100, 20, replace=False)
    out, var_d = _against_pairs(eng, mod, Xa[:100], Xa[idx], f"{kernel} D={D} {form} Xb in Xa")
    sf2 = float(mod["th"][2]) ** 2
    tie_p, tie_v = out["prob"][idx, np.arange(20)], var_d[idx, np.arange(20)]
    print(f"  identical points: |p - 1/2| <= {np.abs(tie_p - 0.5).max():.2e}, var_d in [{tie_v.min():.2e}, {tie_v.max():.2e}]")
    assert np.abs(tie_p - 0.5).max() <= TOL and tie_v.max() <= TOL * sf2
    assert tie_v.min() >= 0.0 and var_d.min() >= 0.0      # cov is clipped at (var_a + var_b) / 2
    # swapping the sets
    ab, ba = _full(eng, mod["post"], Xa[:100], Xb), _full(eng, mod["post"], Xb, Xa[:100])
    assert np.abs(ab["prob"] + ba["prob"].T - 1.0).max() <= TOL
    assert np.abs(ab["cov"] - ba["cov"].T).max() <= TOL * sf2


# ---------------------------------------------------------------- 4. shapes where the kernel can go wrong
@pytest.mark.parametrize("form", ["node", "edge"])
def test_chunk_boundary(eng, form):
    """Ma = 65536 + 5 against Mb = 3: 64 rows on each side of the boundary against a small call, bit for bit (the small
    model splits its mean sums the same way whatever the size of the call)."""
    mod = _fitted("SE_kernel", 6, _forms()[form])
    Ma = 65536 + 5
    rng = np.random.default_rng(15)
    Xa, Xb = rng.random((Ma, 6)), rng.random((3, 6))
    out = _full(eng, mod["post"], Xa, Xb)
    rows = np.r_[65536 - 64:65536, 65536:Ma, 0:59]            # 64 before, the 5 behind, 59 from the start
    small = _full(eng, mod["post"], Xa[rows], Xb)
    for k in ("mu_a", "var_a", "cov", "prob", "score"):
        assert np.array_equal(out[k][rows], small[k]), k
    assert out["best_idx"] == int(np.argmax(out["score"])) and out["best_val"] == out["score"].max()
    # the winner moved behind the boundary: the index that comes back is the global row
    i, j = out["best_idx"], 65536 + 3
    Xa[[i, j]] = Xa[[j, i]]
    moved = eng.predict_tournament(mod["post"], Xa, Xb)
    assert moved["best_val"] == out["best_val"]
    assert moved["best_idx"] == int(np.argmax(host(moved["score"])))


@pytest.mark.parametrize("form", ["node", "edge"])
def test_field_at_the_cap(eng, form):
    mod = _fitted("RQ_kernel", 6, _forms()[form])
    _parity(eng, mod, Ma=40, Mb=1024, seed=16, label=f"RQ D=6 {form} 40 x 1024")
    with pytest.raises(ValueError, match="predict_tournament"):
        eng.predict_tournament(mod["post"], np.zeros((4, 6)), np.zeros((1025, 6)))


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_c2(eng, form):
    """N = 512: the K loop spans 32 chunks and four candidate row tiles' worth of design rows."""
    _parity(eng, _fitted_golden("c2", _forms()[form]), Ma=200, Mb=40, seed=17, label=f"c2 {form} 200 x 40")


# ---------------------------------------------------------------- 5. NaN rows and columns, refusals
@pytest.mark.parametrize("form", ["node", "edge"])
def test_nan_rows_and_columns(eng, form):
    from ppbo_amd.engine import TOURNAMENT_WORST
    mod = _fitted("Matern52_kernel", 6, _forms()[form])
    Xa, Xb = _sets(np.random.default_rng(18), mod, 150, 70)
    clean = _full(eng, mod["post"], Xa, Xb)
    Xa_bad = Xa.copy()
    Xa_bad[11, 2], Xa_bad[140, 0] = np.nan, np.inf
    bad = np.zeros(150, dtype=bool)
    bad[[11, 140]] = True
    out = _full(eng, mod["post"], Xa_bad, Xb)
    for k in ("mu_a", "var_a", "cov", "prob", "score"):
        assert np.all(np.isnan(out[k][bad])), k
        assert np.array_equal(out[k][~bad], clean[k][~bad]), k
    assert not bad[out["best_idx"]] and out["best_val"] == np.nanmax(out["score"])
    assert out["best_idx"] == int(np.nanargmax(out["score"]))
    # a NaN opponent: its column, and every score
    Xb_bad = Xb.copy()
    Xb_bad[37, 4] = np.nan
    col = np.zeros(70, dtype=bool)
    col[37] = True
    for kind in (0, TOURNAMENT_WORST):
        out = _full(eng, mod["post"], Xa, Xb_bad, score=kind)
        assert np.isnan(out["mu_b"][37]) and np.isnan(out["var_b"][37])
        for k in ("cov", "prob"):
            assert np.all(np.isnan(out[k][:, col])) and np.array_equal(out[k][:, ~col], clean[k][:, ~col]), k
        assert np.all(np.isnan(out["score"]))
        assert out["best_idx"] == -1 and np.isnan(out["best_val"])


def test_refusals_leave_the_context_usable(eng):
    from ppbo_amd import _lib
    from ppbo_amd.engine import _ptr
    mod = _fitted("SE_kernel", 6, None)
    post = mod["post"]
    Xa, Xb = _sets(np.random.default_rng(19), mod, 100, 30)
    before = _full(eng, post, Xa, Xb)
    da, db = eng.dev(Xa), eng.dev(Xb)
    sentinel = -12345.0
    outs = [eng.empty(100).fill_(sentinel), eng.empty(100).fill_(sentinel), eng.empty(30).fill_(sentinel),
            eng.empty(30).fill_(sentinel), eng.empty(100, 30).fill_(sentinel), eng.empty(100, 30).fill_(sentinel),
            eng.empty(100).fill_(sentinel)]
    md, md32, bare = eng._model(post, True), eng._model(post, True, kstar_fp32=True), eng._model(post, False)
    nolam, badform = eng._model(post, True), eng._model(post, True)
    nolam.d_lam_off = 0
    badform.form = 2

    def call(model, a, b, Ma, Mb, kind):
        bv, bi = C.c_double(sentinel), C.c_int64(-7)
        rc = eng.lib.ppbo_predict_tournament(eng.ctx, C.byref(model) if model is not None else None, _ptr(a), Ma, _ptr(b), Mb,
                                             kind, *[_ptr(o) for o in outs], C.byref(bv), C.byref(bi), eng._stream())
        return rc, eng._err(), bv.value, bi.value

    for args in ((None, da, db, 100, 30, 0), (md, None, db, 100, 30, 0), (md, da, None, 100, 30, 0), (md, da, db, 0, 30, 0),
                 (md, da, db, -5, 30, 0), (md, da, db, 2 ** 31, 30, 0), (md, da, db, 100, 0, 0), (md, da, db, 100, -1, 0),
                 (md, da, db, 100, _lib.TOURNAMENT_MAX_B + 1, 0), (md, da, db, 100, 30, 2), (md, da, db, 100, 30, -1),
                 (md32, da, db, 100, 30, 0), (bare, da, db, 100, 30, 0), (nolam, da, db, 100, 30, 0),
                 (badform, da, db, 100, 30, 0)):
        rc, msg, bv, bi = call(*args)
        assert rc < 0 and msg.startswith("invalid argument"), (args[3:], rc, msg)
        assert (bv, bi) == (sentinel, -7)
    import torch
    torch.cuda.synchronize()
    assert all(bool((o == sentinel).all()) for o in outs)             # nothing was launched
    after = _full(eng, post, Xa, Xb)
    for k in ("mu_a", "var_a", "mu_b", "var_b", "cov", "prob", "score"):
        assert np.array_equal(before[k], after[k]), k


def test_profile_names(eng):
    """The cross product and the field pass are timed under stable names (one bracket per chunk / per call)."""
    import torch
    mod = _fitted("SE_kernel", 6, None)
    Xa, Xb = _sets(np.random.default_rng(21), mod, 50, 10)
    eng.profile(True)
    try:
        eng.predict_tournament(mod["post"], Xa, Xb)
        torch.cuda.synchronize()
        (t, n), (tf, nf) = eng.profile_read("tournament"), eng.profile_read("tournament_field")
    finally:
        eng.profile(False)
    assert (n, nf) == (1, 1) and t > 0.0 and tf > 0.0


# ---------------------------------------------------------------- 6. the GPModel surface
def test_gpmodel_ranking_and_borda():
    from test_gpu_pairs import _golden_gp
    from conftest import load_golden
    gp = _golden_gp(load_golden("rq"))
    rng = np.random.default_rng(20)
    items = rng.random((12, gp.D))
    P, borda, order = gp.ranking_pred(items)
    _, _, p = gp.preference_pred(np.repeat(items, 12, axis=0), np.tile(items, (12, 1)))
    print(f"ranking_pred: |P - preference_pred| = {np.abs(P - p.reshape(12, 12)).max():.2e}, "
          f"|diag - 1/2| = {np.abs(np.diag(P) - 0.5).max():.2e}")
    assert P.shape == (12, 12) and np.abs(P - p.reshape(12, 12)).max() <= TOL
    assert np.abs(np.diag(P) - 0.5).max() <= TOL
    assert np.abs(borda - tn.scores(P, tn.BORDA)).max() <= 12e-15
    assert np.array_equal(order, np.argsort(-borda, kind="stable")) and sorted(order) == list(range(12))
    X = rng.random((500, gp.D))
    score, winner = gp.borda_pred(X, seed=4)
    again, winner2 = gp.borda_pred(X, field=gp.default_field(256, seed=4))
    assert score.shape == (500,) and winner == int(np.argmax(score))
    assert np.array_equal(score, again) and winner2 == winner
    full = gp.tournament_pred(X[:20], gp.default_field(256, seed=4))
    assert full["prob"].shape == full["cov"].shape == (20, 256)
    assert np.array_equal(full["score"], score[:20])
    with pytest.raises(ValueError, match="ranking_pred"):
        gp.ranking_pred(rng.random((12, gp.D + 1)))
