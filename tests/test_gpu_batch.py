"""GPU: shortlists -- ppbo_search_batch / Engine.search_batch / GPModel.shortlist against the column-wise NumPy statement
(tests/batch_numpy.py on pairs_numpy's kernels and the oracle's dense variance operator), the exact identities of the
construction, the chunk boundary, exhaustion and NaN rows, the refusals, the profile names and the GPModel surface.
The star design of test_gpu_pairs: n_q = 7, m = 25, N = 182.

The picks are compared as INDICES.  What keeps that honest is asserted on the reference alone: at every pick the relative
gap between the best score and the runner-up exceeds GAP = 1e-5, ten times the parity tolerance.  The candidate seeds are
chosen so that it holds (SEED, below, with the cases where the reference is tied under every seed and what is checked
there), so no pick is excused.

Worst errors measured on MI355X are recorded in DESIGN.md section 7 ("Shortlists")."""
import ctypes as C

import numpy as np
import pytest

import batch_numpy as bn
import pairs_numpy as pn
import slopes_numpy as sn
from test_gpu_pairs import TOL, _fitted, _fitted_golden, _forms, host

pytestmark = pytest.mark.gpu

GAP = 1e-5
TINY = np.finfo(float).tiny

# The candidate seed of every parity case, chosen on the reference alone (tests/batch_numpy.py on the host statement of
# the fitted model, seeds 0 .. 39 tried): the first seed whose smallest relative gap over the picks exceeds 2e-5 at BOTH
# noise levels.  None: no seed has the gap, because the reference itself is tied there --
#   VARIANCE on SE D = 6, Matern-5/2 D = 40 and c2: far from the design the variance saturates at sigma_f^2; the largest
#     smallest-gap over the 40 seeds was 8.5e-6, 2.8e-6 and 6.5e-6 (medians 1.2e-6, 6e-7, 1.2e-6), and over 800 further seeds
#     1.3e-5 / 1.1e-5 (SE D = 6 node / edge, one seed each: too close to the bound to build on), 6.9e-6 and 8.6e-6
#   cam_small (l such that uniform candidates see the prior: mu = 0, var = sigma_f^2 exactly) and VARIANCE on
#     camphor_ard/spread: exact ties (gap 0) under VARIANCE, 1.6e-11 at most under EI
# -- and an index comparison would compare tie-breaks.  Those cases are checked through the reference's replay of the
# device's own picks instead (_parity_replayed): every pick is the reference's best at its turn to the parity tolerance,
# the leading picks up to the reference's first near-tie are the reference's own, and every quantity agrees with the
# replay.  No pick is excused in either form.
SEED = {("SE_kernel D=6 node", "EI"): 1, ("SE_kernel D=6 edge", "EI"): 0, ("SE_kernel D=6 node", "variance"): None,
        ("SE_kernel D=6 edge", "variance"): None, ("RQ_kernel D=20 node", "EI"): 1, ("RQ_kernel D=20 edge", "EI"): 0,
        ("RQ_kernel D=20 node", "variance"): 1, ("RQ_kernel D=20 edge", "variance"): 0,
        ("Matern52_kernel D=40 node", "EI"): 0, ("Matern52_kernel D=40 edge", "EI"): 0,
        ("Matern52_kernel D=40 node", "variance"): None, ("Matern52_kernel D=40 edge", "variance"): None,
        ("Matern32_kernel D=6 node", "EI"): 0, ("Matern32_kernel D=6 edge", "EI"): 0,
        ("Matern32_kernel D=6 node", "variance"): 4, ("Matern32_kernel D=6 edge", "variance"): 2,
        ("Matern52 ARD D=6", "EI"): 0, ("Matern52 ARD D=6", "variance"): 1,
        ("camphor cam_small node", "EI"): None, ("camphor cam_small edge", "EI"): None,
        ("camphor cam_small node", "variance"): None, ("camphor cam_small edge", "variance"): None,
        ("camphor ARD camphor_ard/spread", "EI"): 0, ("camphor ARD camphor_ard/spread", "variance"): None,
        ("c2 node", "EI"): 1, ("c2 edge", "EI"): 1, ("c2 node", "variance"): None, ("c2 edge", "variance"): None,
        ("RQ D=20 edge N=2080", "EI"): 0, ("RQ D=20 edge N=2080", "variance"): 0}
TIED_SEED = 5            # the candidates of the cases without a seed


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def _cands(rng, mod, M):
    """Candidates in the box: uniform points and a few design rows (test_gpu_tournament._sets)."""
    N, D = mod["X"].shape
    Xc = rng.random((M, D))
    k = min(8, M // 4)
    Xc[:k] = mod["X"][rng.integers(0, N, k)]
    return Xc


def _mustar(mod, cross):
    """The incumbent of EI: the largest posterior mean over the design rows (from the reference's own alpha)."""
    return float((cross(mod["X"], mod["X"], mod["th"], mod["kernel"]) @ mod["alpha"]).max())


def _host_args(mod):
    return mod["X"], mod["th"], mod["kernel"], mod["alpha"], mod["A"]


def _errors(out, ref, sf2):
    return dict(score=(np.abs(out["score"] - ref["score"]) / np.maximum(np.abs(ref["score"]), TINY)).max(),
                var_cond=np.abs(host(out["var_cond"]) - ref["var_cond"]).max() / sf2,
                mu=np.abs(host(out["mu"]) - ref["mu"]).max() / sf2, var=np.abs(host(out["var"]) - ref["var"]).max() / sf2)


def _parity_replayed(out, Xc, mod, q, kind, mustar, tau2, cross, sf2, tag):
    """A case whose reference is tied: the device's picks replayed in the reference."""
    picks = out["idx"]
    assert picks.min() >= 0 and len(set(picks.tolist())) == q
    ref = bn.greedy(Xc, *_host_args(mod), q, kind, mustar, tau2, cross=cross)
    near = np.flatnonzero(~(ref["gap"] > GAP))
    lead = int(near[0]) if near.size else q
    assert np.array_equal(picks[:lead], ref["idx"][:lead]), (lead, picks, ref["idx"])
    rep = bn.replay(picks, Xc, *_host_args(mod), kind, mustar, tau2, cross=cross)
    e = _errors(out, rep, sf2)
    print(f"shortlist parity {tag} (replayed; the reference's own picks for the first {lead}): worst shortfall of a pick "
          f"{max(0.0, -float(rep['gap'].min())):.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert rep["gap"].min() >= -TOL, rep["gap"]                    # every pick is the best of its turn
    assert all(v <= TOL for v in e.values()), e


def _parity(eng, mod, label, M=1500, q=16, cross=pn.cross):
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    sf2 = float(mod["th"][2]) ** 2
    mustar = _mustar(mod, cross)
    for kind, kname in ((SCORE_POINTWISE_EI, "EI"), (SCORE_VARIANCE, "variance")):
        seed = SEED[(label, kname)]
        Xc = _cands(np.random.default_rng(TIED_SEED if seed is None else seed), mod, M)
        for tau2 in (0.0, float(mod["th"][0]) ** 2):
            out = eng.search_batch(mod["post"], Xc, q, score=kind, mustar=mustar, noise_var=tau2, want_var_cond=True)
            tag = f"{label} {kname} tau2={tau2:.1e}"
            if seed is None:
                _parity_replayed(out, Xc, mod, q, kind, mustar, tau2, cross, sf2, tag)
                continue
            ref = bn.greedy(Xc, *_host_args(mod), q, kind, mustar, tau2, cross=cross)
            assert (ref["idx"] >= 0).all() and ref["gap"].min() > GAP, ref["gap"]      # on the reference alone
            e = _errors(out, ref, sf2)
            print(f"shortlist parity {tag} seed={seed} gap={ref['gap'].min():.1e}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
            assert np.array_equal(out["idx"], ref["idx"]), (out["idx"], ref["idx"])
            assert all(v <= TOL for v in e.values()), e


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("RQ_kernel", 20), ("Matern52_kernel", 40), ("Matern32_kernel", 6)])
def test_parity_radial(eng, kernel, D, form):
    """M = 1500 (off every tile edge), q = 16, EI and VARIANCE, tau^2 in {0, theta[0]^2}.  D = 6 in the node form takes the
    one-launch scoring path (a K* launch of the entry's own), the others the K* workspace of the scoring launches.
    Figures measured on MI355X: DESIGN.md section 7 holds them."""
    _parity(eng, _fitted(kernel, D, _forms()[form]), f"{kernel} D={D} {form}")


def test_parity_ard(eng):
    _parity(eng, _fitted("Matern52_kernel", 6, None, ard=True), "Matern52 ARD D=6")


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_camphor(eng, form):
    _parity(eng, _fitted_golden("cam_small", _forms()[form]), f"camphor cam_small {form}")


def test_parity_camphor_ard(eng):
    """camphor_ard/spread: embedded rows (D = 11, SE) behind Engine._points."""
    from test_gpu_marginals import _fitted_camphor_ard_golden
    _parity(eng, _fitted_camphor_ard_golden(), "camphor ARD camphor_ard/spread", cross=sn.cross)


@pytest.mark.parametrize("form", ["node", "edge"])
def test_parity_c2(eng, form):
    """N = 512: every wavefront of a step owns 32 rows of the K range."""
    _parity(eng, _fitted_golden("c2", _forms()[form]), f"c2 {form}")


def test_parity_padded_operands(eng):
    """N = 2080 (m = 25, n_q = 80): N is no multiple of the contraction's row tile, so the scoring launches pad their
    operands and the K* workspace is deeper than N."""
    _parity(eng, _fitted("RQ_kernel", 20, _forms()["edge"], n_q=80, m=25), "RQ D=20 edge N=2080", M=300, q=4)


# ---------------------------------------------------------------- 2. exact identities
@pytest.mark.parametrize("form", ["node", "edge"])
@pytest.mark.parametrize("kernel,D", [("SE_kernel", 6), ("Matern52_kernel", 20)])
def test_exact_identities(eng, kernel, D, form):
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    mod = _fitted(kernel, D, _forms()[form])
    post = mod["post"]
    sf2 = float(mod["th"][2]) ** 2
    mustar = _mustar(mod, pn.cross)
    Xc = _cands(np.random.default_rng(31), mod, 777)
    for kind in (SCORE_POINTWISE_EI, SCORE_VARIANCE):
        pred = eng.predict(post, Xc, score=kind, mustar=mustar, want_score=True)
        out = eng.search_batch(post, Xc, 16, score=kind, mustar=mustar, noise_var=0.0, want_var_cond=True)
        # mu, var and pick 0 are ppbo_predict's, bit for bit
        assert np.array_equal(host(out["mu"]), host(pred["mu"])) and np.array_equal(host(out["var"]), host(pred["var"]))
        assert (int(out["idx"][0]), float(out["score"][0])) == (pred["best_idx"], pred["best_val"])
        again = eng.search_batch(post, Xc, 16, score=kind, mustar=mustar, noise_var=0.0, want_var_cond=True)
        assert np.array_equal(out["idx"], again["idx"]) and np.array_equal(out["score"], again["score"])
        assert np.array_equal(host(out["var_cond"]), host(again["var_cond"]))
        assert len(set(out["idx"].tolist())) == 16 and out["idx"].min() >= 0
        # an exactly observed point has no variance left
        vc = host(out["var_cond"])
        assert vc[out["idx"]].max() <= TOL * sf2 and vc.min() >= 0.0
        assert np.all(vc <= host(out["var"]))
        # the picks do not depend on whether var_cond is written (the last pass is skipped without it)
        lean = eng.search_batch(post, Xc, 16, score=kind, mustar=mustar, noise_var=0.0)
        assert lean["var_cond"] is None
        assert np.array_equal(lean["idx"], out["idx"]) and np.array_equal(lean["score"], out["score"])
        # nothing is conditioned under a huge noise: the q best scores in stable order, the variance untouched
        huge = eng.search_batch(post, Xc, 16, score=kind, mustar=mustar, noise_var=1e300, want_var_cond=True)
        assert np.array_equal(host(huge["var_cond"]), host(pred["var"]))
        assert np.array_equal(huge["idx"], np.argsort(-host(pred["score"]), kind="stable")[:16])
        # q = 1 and q = 64
        one = eng.search_batch(post, Xc, 1, score=kind, mustar=mustar, noise_var=0.0, want_var_cond=True)
        assert (int(one["idx"][0]), float(one["score"][0])) == (pred["best_idx"], pred["best_val"])
        many = eng.search_batch(post, Xc, 64, score=kind, mustar=mustar, want_var_cond=True)
        assert len(set(many["idx"].tolist())) == 64 and many["idx"].min() >= 0
        assert np.array_equal(many["idx"][:1], out["idx"][:1])
        # the twin of a picked row: conditioned on its copy at tau = 0 it has no variance left either
        Xd = Xc.copy()
        p0 = int(out["idx"][0])
        Xd[700 if p0 != 700 else 600] = Xd[p0]
        twin = eng.search_batch(post, Xd, 1, score=kind, mustar=mustar, noise_var=0.0, want_var_cond=True)
        assert int(twin["idx"][0]) == min(p0, 700 if p0 != 700 else 600)
        assert host(twin["var_cond"])[[p0, 700 if p0 != 700 else 600]].max() <= TOL * sf2
    forced = np.tile(Xc[400], (3, 1))                             # three copies of one row: one is picked, all are known
    vc = host(eng.search_batch(post, forced, 1, score=SCORE_VARIANCE, noise_var=0.0, want_var_cond=True)["var_cond"])
    assert vc.max() <= TOL * sf2


# ---------------------------------------------------------------- 3. the chunk boundary
@pytest.mark.parametrize("form", ["node", "edge"])
def test_chunk_boundary(eng, form):
    """M = 65536 + 5, q = 6, EI: two chunks, the K* of each formed again per pick.  (Seed 5: the reference's smallest gap is
    6.9e-4 / 9.1e-4 in the node / edge form; under VARIANCE 65541 uniform candidates tie at 1e-7.)  Then the first winner
    moves behind the boundary: the global index follows, the scores stay."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI as EI
    mod = _fitted("SE_kernel", 6, _forms()[form])
    M, q = 65536 + 5, 6
    tau2, mustar = float(mod["th"][0]) ** 2, _mustar(mod, pn.cross)
    Xc = _cands(np.random.default_rng(5), mod, M)
    ref = bn.greedy(Xc, *_host_args(mod), q, EI, mustar, tau2)
    assert (ref["idx"] >= 0).all() and ref["gap"].min() > GAP, ref["gap"]
    out = eng.search_batch(mod["post"], Xc, q, score=EI, mustar=mustar, noise_var=tau2, want_var_cond=True)
    e = _errors(out, ref, float(mod["th"][2]) ** 2)
    print(f"shortlist chunk boundary {form} gap={ref['gap'].min():.1e}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert np.array_equal(out["idx"], ref["idx"]) and all(v <= TOL for v in e.values()), e
    i, j = int(out["idx"][0]), 65536 + 3
    assert j not in out["idx"]
    Xc[[i, j]] = Xc[[j, i]]
    moved = eng.search_batch(mod["post"], Xc, q, score=EI, mustar=mustar, noise_var=tau2)
    expect = np.where(out["idx"] == i, j, out["idx"])
    assert np.array_equal(moved["idx"], expect)
    assert np.array_equal(moved["score"], out["score"])


# ---------------------------------------------------------------- 4. exhaustion and NaN rows
@pytest.mark.parametrize("form", ["node", "edge"])
def test_exhaustion_and_nan(eng, form):
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    mod = _fitted("Matern52_kernel", 6, _forms()[form])
    post = mod["post"]
    Xc = _cands(np.random.default_rng(41), mod, 150)
    few = eng.search_batch(post, Xc[:5], 8, score=SCORE_VARIANCE, noise_var=0.0, want_var_cond=True)
    assert sorted(few["idx"][:5].tolist()) == [0, 1, 2, 3, 4] and (few["idx"][5:] == -1).all()
    assert not np.isnan(few["score"][:5]).any() and np.isnan(few["score"][5:]).all()
    for kind in (SCORE_POINTWISE_EI, SCORE_VARIANCE):
        clean = eng.search_batch(post, Xc, 8, score=kind, mustar=0.1, want_var_cond=True)
        bad = np.zeros(150, dtype=bool)
        # the clean run's first pick is made non-finite: it may never come back
        bad[[int(clean["idx"][0]), 140]] = True
        Xb = Xc.copy()
        Xb[int(clean["idx"][0]), 2], Xb[140, 0] = np.nan, np.inf
        out = eng.search_batch(post, Xb, 8, score=kind, mustar=0.1, want_var_cond=True)
        assert not bad[out["idx"]].any() and out["idx"].min() >= 0 and not np.isnan(out["score"]).any()
        for k in ("mu", "var", "var_cond"):
            assert np.all(np.isnan(host(out[k])[bad])) and not np.isnan(host(out[k])[~bad]).any(), k
        # the other rows are what a call without the two rows gives them
        rest = eng.search_batch(post, Xb[~bad], 8, score=kind, mustar=0.1, want_var_cond=True)
        assert np.array_equal(np.flatnonzero(~bad)[rest["idx"]], out["idx"])
        for k in ("mu", "var"):
            assert np.array_equal(host(out[k])[~bad], host(rest[k])), k
        assert np.abs(host(out["var_cond"])[~bad] - host(rest["var_cond"])).max() <= TOL * float(mod["th"][2]) ** 2
    allnan = eng.search_batch(post, np.full((7, 6), np.nan), 3, score=SCORE_VARIANCE, want_var_cond=True)
    assert (allnan["idx"] == -1).all() and np.isnan(allnan["score"]).all()
    assert np.isnan(host(allnan["var_cond"])).all()


# ---------------------------------------------------------------- 5. refusals
def test_engine_refusals(eng):
    from ppbo_amd.engine import SCORE_MEAN
    mod = _fitted("SE_kernel", 6, None)
    post, z = mod["post"], np.zeros
    for Xc in (z((5, 7)), z(6), z((0, 6)), z((5, 6, 1))):
        with pytest.raises(ValueError, match="search_batch"):
            eng.search_batch(post, Xc, 4)
    for q in (0, -1, 65):
        with pytest.raises(ValueError, match="search_batch"):
            eng.search_batch(post, z((5, 6)), q)
    with pytest.raises(ValueError, match="score kind"):
        eng.search_batch(post, z((5, 6)), 4, score=SCORE_MEAN)
    for nv in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise_var"):
            eng.search_batch(post, z((5, 6)), 4, noise_var=nv)


def test_refusals_leave_the_context_usable(eng):
    from ppbo_amd import _lib
    from ppbo_amd.engine import SCORE_MEAN, SCORE_POINTWISE_EI, _ptr
    mod = _fitted("SE_kernel", 6, None)
    post = mod["post"]
    Xc = _cands(np.random.default_rng(19), mod, 100)
    before = eng.search_batch(post, Xc, 5, want_var_cond=True)
    dc = eng.dev(Xc)
    sentinel = -12345.0
    outs = [eng.empty(100).fill_(sentinel) for _ in range(3)]
    md, md32, bare = eng._model(post, True), eng._model(post, True, kstar_fp32=True), eng._model(post, False)
    nolam, badform = eng._model(post, True), eng._model(post, True)
    nolam.d_lam_off = 0
    badform.form = 2
    EI = SCORE_POINTWISE_EI

    def call(model, x, M, kind, nv, q, with_idx=True):
        idx, sc = (C.c_int64 * 64)(*([-7] * 64)), (C.c_double * 64)(*([sentinel] * 64))
        rc = eng.lib.ppbo_search_batch(eng.ctx, C.byref(model) if model is not None else None, _ptr(x), M, kind, 0.0, nv, q,
                                       idx if with_idx else None, sc, *[_ptr(o) for o in outs], eng._stream())
        return rc, eng._err(), list(idx), list(sc)

    for args in ((None, dc, 100, EI, 0.0, 5), (md, None, 100, EI, 0.0, 5), (md, dc, 100, EI, 0.0, 5, False), (md, dc, 0, EI, 0.0, 5),
                 (md, dc, -5, EI, 0.0, 5), (md, dc, 2 ** 31, EI, 0.0, 5), (md, dc, 100, EI, 0.0, 0), (md, dc, 100, EI, 0.0, -1),
                 (md, dc, 100, EI, 0.0, _lib.BATCH_MAX_Q + 1), (md, dc, 100, EI, -1e-9, 5), (md, dc, 100, EI, float("nan"), 5),
                 (md, dc, 100, EI, float("inf"), 5), (md, dc, 100, SCORE_MEAN, 0.0, 5), (md, dc, 100, 3, 0.0, 5),
                 (md, dc, 100, -1, 0.0, 5), (md32, dc, 100, EI, 0.0, 5), (bare, dc, 100, EI, 0.0, 5), (nolam, dc, 100, EI, 0.0, 5),
                 (badform, dc, 100, EI, 0.0, 5)):
        rc, msg, idx, sc = call(*args)
        assert rc < 0 and msg.startswith("invalid argument"), (args[2:], rc, msg)
        assert idx == [-7] * 64 and sc == [sentinel] * 64
    import torch
    torch.cuda.synchronize()
    assert all(bool((o == sentinel).all()) for o in outs)             # nothing was launched
    rc, msg, idx, sc = call(md, dc, 100, EI, 1.7e308, 5)              # a huge finite noise is allowed
    assert rc == 0, msg
    after = eng.search_batch(post, Xc, 5, want_var_cond=True)
    assert np.array_equal(before["idx"], after["idx"]) and np.array_equal(before["score"], after["score"])
    assert np.array_equal(host(before["var_cond"]), host(after["var_cond"]))


# ---------------------------------------------------------------- 6. profile names
def test_profile_names(eng):
    """The streaming passes and the per-pick field passes are timed under stable names: one bracket per pass."""
    import torch
    mod = _fitted("SE_kernel", 20, None)
    Xc = _cands(np.random.default_rng(21), mod, 200)
    eng.profile(True)
    try:
        eng.search_batch(mod["post"], Xc, 4, want_var_cond=True)
        torch.cuda.synchronize()
        (t, n), (tf, nf) = eng.profile_read("batch_step"), eng.profile_read("batch_field")
    finally:
        eng.profile(False)
    assert (n, nf) == (4, 4) and t > 0.0 and tf > 0.0


# ---------------------------------------------------------------- 7. the GPModel surface
def test_gpmodel_shortlist():
    from conftest import load_golden
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    from test_gpu_pairs import _golden_gp
    gp = _golden_gp(load_golden("rq"))
    gp.mustar = 0.05
    rng = np.random.default_rng(20)
    cand = rng.random((2000, gp.D))
    X, idx, score = gp.shortlist(q=8, X_cand=cand)
    assert X.shape == (8, gp.D) and idx.shape == (8,) and score.shape == (8,)
    assert np.array_equal(X, cand[idx]) and len(set(idx.tolist())) == 8
    pred = gp.eng.predict(gp._post, cand, score=SCORE_POINTWISE_EI, mustar=0.05)
    assert (int(idx[0]), float(score[0])) == (pred["best_idx"], pred["best_val"])
    P, borda, order = gp.ranking_pred(X)
    assert P.shape == (8, 8) and sorted(order) == list(range(8))
    prob = gp.choice_pred(X, n_draws=512, seed=3)
    assert prob.shape == (8,) and np.all(np.isfinite(prob))
    Xv, idv, _ = gp.shortlist(q=8, score="variance", X_cand=cand)
    assert not np.array_equal(idv, idx)
    with pytest.raises(ValueError, match="shortlist"):
        gp.shortlist(score="mean", X_cand=cand)
    # the default candidates: the resident pool under a fresh rotation
    Xp, idp, scp = gp.shortlist(q=4)
    assert Xp.shape == (4, gp.D) and Xp.min() >= 0.0 and Xp.max() < 1.0 and len(set(idp.tolist())) == 4
    assert np.all(np.isfinite(scp))
    # fewer candidates than picks: the empty picks are dropped
    Xs, ids, _ = gp.shortlist(q=8, X_cand=cand[:3])
    assert Xs.shape == (3, gp.D) and sorted(ids.tolist()) == [0, 1, 2]
