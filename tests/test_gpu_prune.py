"""GPU: the pruned search (csrc/predict.hip) -- a call that asks only for the best record contracts the variance only for
the candidates that a certified bound cannot rule out.

The yardstick is the SAME call on an engine created with PPBO_PRUNE=0, today's launches: the record must agree bit for
bit, value and index, and with NumPy's argmax over the unpruned scores wherever the two best scores are more than 1e-9
apart.  What the pruning decided (the number of survivors, whether the chunk was pruned or fell back) comes from the
diagnostic entry ppbo_predict_prune_report, so that every case is known to walk the path it is meant to walk.

Models: real posteriors of star designs with 96 and 384 rows (edge form: the three-launch path at any size), hand-built
ones (random alpha, Lambda and operator: the bound holds for any operand) for the layout cases.
"""
import numpy as np
import pytest

from test_gpu_kstar_star import Hand, _engine, host, star_design
from test_gpu_var_projection import call_record, call_search, smooth_posterior

pytestmark = pytest.mark.gpu

EDGE = 1


@pytest.fixture(scope="module")
def on():
    e = _engine(PPBO_FUSED=0, PPBO_PRUNE=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def off():
    e = _engine(PPBO_FUSED=0, PPBO_PRUNE=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cap128():
    e = _engine(PPBO_FUSED=0, PPBO_PRUNE=1, PPBO_PRUNE_CAP=128)
    yield e
    e.close()


def real_posterior(eng, n_q, m, D, kernel, l, seed, off_line=False):
    """sigma = 1: Lambda stays a small perturbation of Sigma^-1 whatever the design (the posterior exists)."""
    rng = np.random.default_rng(seed)
    X = star_design(rng, n_q, m, D, "general")
    if off_line:
        X[(m + 1) + 3, 1] += 1e-9          # star 1 leaves its line: the per-row path of the K* pass
    th = [1.0, l, 1.3]
    S = eng.gram(X, th, kernel)
    f = 0.5 * eng.dgemv(eng.potrf_(S.clone()), rng.standard_normal(X.shape[0]), lower=True)
    return eng.posterior(X, th, kernel, eng.pd_inverse(S), f, m, form=EDGE), X, rng


_POSTS = {}


def posterior(eng, key):
    """(post, X, candidates pool) of a named model, built once (device tensors: shared by the engines of this file)."""
    if key not in _POSTS:
        n_q, m, D, kernel, l, off_line = {
            "d20_96": (3, 31, 20, "SE_kernel", 0.45, False),
            "d20_384": (12, 31, 20, "SE_kernel", 0.45, False),
            "d20_matern": (12, 31, 20, "Matern52_kernel", 0.6, False),
            "d20_offline": (3, 31, 20, "SE_kernel", 0.45, True),
            "d2_384": (12, 31, 2, "SE_kernel", 0.8, False),
            "d2_64": (2, 31, 2, "SE_kernel", 0.8, False),
        }[key]
        if key == "d2_384":     # sigma = 0.1, a Lambda that matters: the smooth design of test_gpu_var_projection.py
            post, rng = smooth_posterior(eng, n_q, m, D, kernel, l)
            X = host(post.X)
        else:
            post, X, rng = real_posterior(eng, n_q, m, D, kernel, l, seed=len(key) + n_q)
        # candidates around the design (where the posterior has something to say) and uniform ones
        near = X[rng.integers(0, X.shape[0], 1500)] + 0.05 * rng.standard_normal((1500, D))
        _POSTS[key] = (post, X, np.concatenate([near, rng.random((1500, D))])[rng.permutation(3000)])
    return _POSTS[key]


def same_record(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check(on, off, post, Xc, score, mustar, pj=None, want_pruned=None, label=""):
    """The record of the pruned engine against PPBO_PRUNE=0 (bitwise) and NumPy's argmax; returns the report."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    rec_on, rec_off = call_record(on, post, Xc, score, mustar, pj), call_record(off, post, Xc, score, mustar, pj)
    rep = on.prune_report(post, Xc[:65536], score, mustar, projection=pj)
    print(f"{label} M={Xc.shape[0]} score={score}: record {rec_on} / {rec_off}, n_surv {rep['n_surv']} pruned {rep['pruned']} "
          f"threshold {rep['threshold']:.6e}")
    assert same_record(rec_on, rec_off)
    assert same_record(call_search(on, post, Xc, score, mustar, pj), call_search(off, post, Xc, score, mustar, pj))
    full = off.predict(post, Xc, score=score, mustar=mustar, want_score=True, projection=pj)
    sc = host(full["score"])
    if np.isfinite(sc).any():
        top = np.sort(sc[np.isfinite(sc)])[-2:]
        if top.size < 2 or top[1] - top[0] > 1e-9:
            assert rec_on[1] == 1000 + int(np.nanargmax(sc)) and rec_on[0] == np.nanmax(sc)
    if Xc.shape[0] <= 65536:
        # the interval holds the unpruned score of every candidate (EI: to the rounding of the score expression)
        lo, hi = host(rep["s_lo"]), host(rep["s_hi"])
        ok = np.isfinite(sc)
        slack = 1e-12 * np.abs(sc[ok]).max() if (score == SCORE_POINTWISE_EI and ok.any()) else 0.0
        assert np.all(lo[ok] <= sc[ok] + slack) and np.all(hi[ok] >= sc[ok] - slack)
        assert np.all(np.isinf(hi[~ok]))
    if want_pruned is not None:
        assert rep["pruned"] == want_pruned
    return rep


@pytest.mark.parametrize("M", [300, 2049])
@pytest.mark.parametrize("key", ["d20_96", "d20_384", "d20_matern", "d20_offline"])
def test_few_survivors(on, off, key, M):
    """D = 20 with a short length scale: the bound rules out almost every candidate and the compact launch runs.
    d20_offline: one star off its line (the K* pass's per-row path accumulates the same sums)."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    post, X, pool = posterior(on, key)
    Xc = pool[:M]
    mu = host(off.predict(post, Xc)["mu"])
    rep = check(on, off, post, Xc, SCORE_POINTWISE_EI, float(np.sort(mu)[-3]), want_pruned=1, label=key)
    assert rep["n_surv"] <= M // 8
    check(on, off, post, Xc, SCORE_VARIANCE, 0.0, label=key)


def test_fallback_with_candidates_on_the_design(on, off):
    """D = 2, candidates on the design rows: the variance interval is wide, more than the capacity survive and the full
    contraction runs behind the plan."""
    from ppbo_amd.engine import SCORE_VARIANCE
    post, X, pool = posterior(on, "d2_384")
    Xc = np.concatenate([X, X[::-1], X[::2]])
    rep = check(on, off, post, Xc, SCORE_VARIANCE, 0.0, want_pruned=0, label="fallback")
    assert rep["n_surv"] > max(128, Xc.shape[0] // 8 // 128 * 128)


@pytest.mark.parametrize("n_best", [128, 129])
def test_survivor_counts_at_the_capacity_and_duplicated_best_rows(on, off, cap128, n_best):
    """The best candidate n_best times among candidates that the bound rules out, capacity 128: exactly 128 survivors
    take the compact launch, 129 overflow it and fall back.  The lowest of the duplicated rows wins either way."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    post, X, pool = posterior(on, "d20_384")
    mustar = float(np.sort(host(off.predict(post, pool)["mu"]))[-3])
    rep = on.prune_report(post, pool, SCORE_POINTWISE_EI, mustar)
    lo, hi = host(rep["s_lo"]), host(rep["s_hi"])
    best = int(np.argmax(lo))
    assert lo[best] == rep["threshold"] > 0.0
    out = np.flatnonzero(hi < 0.5 * lo[best])           # ruled out with room for any tolerance
    assert out.size >= 1000
    rng = np.random.default_rng(n_best)
    Xc = pool[out[:1000]].copy()
    at = np.sort(rng.choice(np.arange(7, 1000), n_best, replace=False))
    Xc[at] = pool[best]
    r = check(cap128, off, post, Xc, SCORE_POINTWISE_EI, mustar, want_pruned=1 if n_best == 128 else 0, label=f"n_best={n_best}")
    assert r["n_surv"] == n_best
    assert call_record(cap128, post, Xc, SCORE_POINTWISE_EI, mustar, None)[1] == 1000 + at[0]
    assert same_record(call_record(on, post, Xc, SCORE_POINTWISE_EI, mustar, None),
                       call_record(off, post, Xc, SCORE_POINTWISE_EI, mustar, None))


def test_two_chunks(on, off):
    """65536 + 130 candidates on a 64-row model: every chunk has its own threshold, plan and compaction."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    post, X, pool = posterior(on, "d2_64")
    rng = np.random.default_rng(3)
    Xc = rng.random((65536 + 130, 2))
    Xc[65536 + 77] = X[5] + 1e-3              # the winner of the EI search sits in the second chunk
    mu = host(off.predict(post, Xc[-130:])["mu"])
    for score, mustar in ((SCORE_POINTWISE_EI, float(np.sort(mu)[-2])), (SCORE_VARIANCE, 0.0)):
        a, b = call_record(on, post, Xc, score, mustar, None), call_record(off, post, Xc, score, mustar, None)
        print(f"two chunks score={score}: {a} / {b}")
        assert same_record(a, b)


def test_mean_takes_todays_path(on, off):
    from ppbo_amd.engine import SCORE_MEAN
    post, X, pool = posterior(on, "d20_96")
    assert same_record(call_record(on, post, pool[:300], SCORE_MEAN, 0.0, None), call_record(off, post, pool[:300], SCORE_MEAN, 0.0, None))
    with pytest.raises(RuntimeError):
        on.prune_report(post, pool[:300], SCORE_MEAN)


def test_with_a_projection_operand(on, off):
    """The dense projected operator T in the place of H: the block norms are T's, the compact launch the dense form's."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    post, X, pool = posterior(on, "d2_384")
    pj = off.project_variance(post, 1e-6)
    assert pj.rows > 0
    Xc = pool[:2049]
    mu = host(off.predict(post, Xc)["mu"])
    check(on, off, post, Xc, SCORE_POINTWISE_EI, float(np.sort(mu)[-3]), pj=pj, label="projected")
    check(on, off, post, Xc, SCORE_VARIANCE, 0.0, pj=pj, label="projected")
    post20, _, pool20 = posterior(on, "d20_384")
    pj20 = off.project_variance(post20, 1e-6)
    if pj20.rows > 0:
        mu = host(off.predict(post20, pool20[:2049])["mu"])
        check(on, off, post20, pool20[:2049], SCORE_POINTWISE_EI, float(np.sort(mu)[-3]), pj=pj20, want_pruned=1, label="projected d20")


def test_nan_candidates(on, off):
    """NaN coordinates in some candidates: they survive (s_hi = +inf), never win, and do not move the record.  In all of
    them: no threshold, the chunk falls back, the record is (NaN, -1)."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    post, X, pool = posterior(on, "d20_96")
    Xc = pool[:600].copy()
    Xc[[0, 77, 599], 3] = np.nan
    mu = host(off.predict(post, Xc)["mu"])
    rep = check(on, off, post, Xc, SCORE_POINTWISE_EI, float(np.sort(mu[np.isfinite(mu)])[-3]), want_pruned=1, label="some NaN")
    assert rep["n_surv"] >= 3
    Xc[:, 0] = np.nan
    for score in (SCORE_POINTWISE_EI, SCORE_VARIANCE):
        rep = check(on, off, post, Xc, score, 0.0, want_pruned=0, label="all NaN")
        rec = call_record(on, post, Xc, score, 0.0, None)
        assert np.isnan(rec[0]) and rec[1] == -1.0


def test_every_ei_underflows(on, off):
    """mustar far above every mean: every EI is 0, s_lo = s_hi = 0, everything survives and the chunk falls back; the
    first candidate wins the tie."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    post, X, pool = posterior(on, "d20_96")
    rep = check(on, off, post, pool[:300], SCORE_POINTWISE_EI, 1e6, want_pruned=0, label="underflow")
    assert rep["n_surv"] == 300
    rec = call_record(on, post, pool[:300], SCORE_POINTWISE_EI, 1e6, None)
    assert rec[0] == 0.0 and rec[1] == 1000.0


def test_a_call_that_asks_for_the_variance_is_todays(on, off):
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    post, X, pool = posterior(on, "d20_384")
    a = on.predict(post, pool[:2049], score=SCORE_POINTWISE_EI, mustar=0.1, want_score=True)
    b = off.predict(post, pool[:2049], score=SCORE_POINTWISE_EI, mustar=0.1, want_score=True)
    for k in ("mu", "var", "score"):
        assert np.array_equal(host(a[k]), host(b[k]))
    assert a["best_idx"] == b["best_idx"] and a["best_val"] == b["best_val"]
    # the best alone through ppbo_predict: the pruned path, the same record
    c = on.predict(post, pool[:2049], score=SCORE_POINTWISE_EI, mustar=0.1, want_mu=False, want_var=False)
    assert c["best_idx"] == b["best_idx"] and c["best_val"] == b["best_val"]


def test_report_bounds_the_exact_contraction(on, off):
    """u^2 >= the slab sum of the unpruned path on every candidate.  With VARIANCE s_lo is var_lo = sf2 + t itself, so the
    slab sum is var - s_lo up to the rounding of that one addition (half an ulp of var)."""
    from ppbo_amd.engine import SCORE_VARIANCE
    for key in ("d20_384", "d2_384"):
        post, X, pool = posterior(on, key)
        Xc = np.concatenate([pool[:1500], X[::5]])
        rep = on.prune_report(post, Xc, SCORE_VARIANCE)
        var = host(off.predict(post, Xc, score=SCORE_VARIANCE)["var"])
        u2, lo, hi = host(rep["u2"]), host(rep["s_lo"]), host(rep["s_hi"])
        q = var - lo
        print(f"{key}: u^2/q median {np.median(u2 / np.maximum(q, 1e-300)):.3g}, min of u^2 - q {np.min(u2 - q):.3e}, n_surv {rep['n_surv']}")
        assert np.all(lo <= var) and np.all(hi >= var)
        assert np.all(u2 >= q - 2.0 ** -52 * np.abs(var))


@pytest.mark.parametrize("form_case", ["collinear", "offline"])
def test_the_flagged_kstar_pass_stores_the_same_numbers(on, off, form_case):
    """K*, mu_part and t_part of the flagged K* instantiation against the unflagged one: one candidate per call, so the
    chunk is pruned with a single survivor and the record IS that candidate's score, formed from the flagged pass's K*
    column (gathered, contracted), mean and t sums.  Before every checked call the engine scores other candidates of the
    same shape, so that nothing stale in a workspace can stand in for a number the checked call failed to write."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    rng = np.random.default_rng(11)
    m, n_q, D = 7, 5, 6
    X = star_design(rng, n_q, m, D, "general", zero_row=True)
    if form_case == "offline":
        X[2 * (m + 1) + 3, 1] += 1e-9
    hand = Hand(rng, X, [1.0, 0.4, 1.1], "Matern52_kernel", m, EDGE)
    post = hand.on(on)
    Xc = np.concatenate([rng.random((24, D)), X[[0, 9, 17]]])
    full = off.predict(post, Xc, score=SCORE_POINTWISE_EI, mustar=0.3, want_score=True)
    var, ei = host(full["var"]), host(full["score"])
    for c in range(Xc.shape[0]):
        call_record(on, post, 1.0 - Xc[c:c + 1], SCORE_VARIANCE, 0.0, None)
        rv = call_record(on, post, Xc[c:c + 1], SCORE_VARIANCE, 0.0, None)
        re = call_record(on, post, Xc[c:c + 1], SCORE_POINTWISE_EI, 0.3, None)
        assert rv[0] == var[c] and re[0] == ei[c] and rv[1] == re[1] == 1000.0
    assert on.prune_report(post, Xc[:1], SCORE_VARIANCE)["pruned"] == 1
