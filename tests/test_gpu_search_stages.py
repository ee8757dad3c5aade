"""GPU: the two stages every maximiser search shares (ppbo_amd/csrc/meangrad.hip), each against its NumPy restatement
(tests/search_ref.py) instead of through the outcome of the whole search.

A.  Start selection, exact: every entry is run with iters = 0, which returns the picked starts and the value there; the
    scores come from the public scoring entry the search itself calls, the picks from search_ref.select_starts.  On
    lattice candidates (coordinates k / 2^p) every squared distance is exact, so the comparison is bitwise.
A'. The fp32 screening's scores are not exposed: properties of its picks.
B.  The ascent: iters = 0 .. 6 from the same starts against search_ref.bb_ascent.  A (start, n) pair is compared while all
    of the reference's branch margins exceed search_ref.MARGIN_MIN (at most 1/8 of a case's pairs may be left out); x is
    held to 100 times the reference's deviation from its own 1e-13-perturbed self (floored at 1e-10), values to
    1e-9 max|mu|, `it` exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import search_ref as sr
from oracle import ppbo_oracle as orc

pytestmark = pytest.mark.gpu

NEG = -np.inf
CAM = "camphor_copper_ard_kernel"
# D, M of the shape table: (G, Tg) = (1, 50), (3, 3000), (2, 2049: the last group has one member), (3, 1756: 96 KB of LDS),
# (80, 875: two scoring chunks, 143.6 KB of LDS), (4, 214: the widest rows)
SHAPES = [(3, 50), (1, 9000), (2, 4097), (6, 5267), (20, 70000), (64, 854)]


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def eng():
    from ppbo_amd.engine import get_engine
    return get_engine(0)


_MODELS = {}


def _model(eng, D, kernel="SE_kernel", l=None, n_q=10, m=4):
    """(post, X, theta, alpha) of a tiny synthetic model, fitted as test_searches_in_every_dimension_bucket fits its own;
    designs of 1024 rows are fitted on the device (the oracle's fit of 1024 unknowns takes over a minute)."""
    key = (D, kernel, None if l is None else tuple(np.ravel(l)), n_q, m)
    if key not in _MODELS:
        th = [0.1, 0.35 * np.sqrt(D) if l is None else l, 0.7]
        X = orc.synthetic_design(n_q, D, m=m, seed=100 + D)
        if X.shape[0] > 256:
            r = eng.gp_fit(X, th, kernel, m, np.random.default_rng(D).standard_normal(X.shape[0]), gtol=1e-6, start_is_whitened=True)
            post = r["post"]
            assert post is not None
        else:
            f0, _ = sr.host_fit(X, th, kernel, m, D)
            post = eng.posterior(X, th, kernel, eng.pd_inverse(eng.gram(X, th, kernel)), f0, m)
        _MODELS[key] = (post, X, th, host(post.alpha))
    return _MODELS[key]


def _mean_scores(eng, post, rows):
    """ppbo_predict, mean only, as ppbo_mean_search calls it; two calls are bitwise equal."""
    a = eng.predict(post, rows, want_var=False, want_best=False)["mu"]
    b = eng.predict(post, rows, want_var=False, want_best=False)["mu"]
    assert torch.equal(a, b) or np.array_equal(host(a), host(b), equal_nan=True)
    return host(a)


def _rff_scores(eng, rows, W, b, sf, omega):
    """ppbo_rff_score with no argmax record, as ppbo_rff_search calls it; two calls are bitwise equal."""
    from ppbo_amd.engine import _ptr
    rows, W, b, omega = eng.dev(rows), eng.dev(W), eng.dev(b).reshape(-1), eng.dev(omega).reshape(-1)
    out = []
    for _ in range(2):
        sc = eng.empty(rows.shape[0])
        rc = eng.lib.ppbo_rff_score(eng.ctx, _ptr(rows), rows.shape[0], rows.shape[1], _ptr(W), W.shape[0], _ptr(b), float(sf),
                                    _ptr(omega), _ptr(sc), None, None, eng._stream())
        eng._check(rc, "ppbo_rff_score")
        out.append(host(sc))
    assert np.array_equal(out[0], out[1])
    return out[0]


def _rff_search_raw(eng, cand, ls, W, b, sf, omega, K, sep, iters, tol):
    """ppbo_rff_search (ls: with the camphor coordinate map) with all K rows returned: x [K, D], val [K], found."""
    from ppbo_amd import _lib
    from ppbo_amd.engine import _ptr
    cand, W, b, omega = eng.dev(cand), eng.dev(W), eng.dev(b).reshape(-1), eng.dev(omega).reshape(-1)
    M, D = cand.shape
    xs, vals = torch.full((K, D), 7.0, dtype=torch.float64, device=eng.device), eng.empty(K)
    found = C.c_int(-1)
    co = None if ls is None else _lib.coords(_lib.COORDS_CAMPHOR, ls)
    rc = eng.lib.ppbo_rff_search(eng.ctx, _ptr(cand), M, D, _ptr(W), W.shape[0], _ptr(b), float(sf), _ptr(omega), co, int(K),
                                 float(sep), int(iters), float(tol), _ptr(xs), _ptr(vals), C.byref(found), eng._stream())
    eng._check(rc, "ppbo_rff_search")
    return host(xs), host(vals), found.value


def _check_picks(scores, cand, K, sep, xs, vals, count, what=""):
    """The device's picks at iters = 0 against the greedy rule on the same scores: the count, the rows bitwise and in
    order, the value of each row, -inf behind them.  Returns the reference's selection."""
    ref = sr.select_starts(scores, cand, K, sep)
    assert count == ref.count, (what, count, ref.count)
    assert np.array_equal(xs[:count], np.clip(cand[ref.idx], 0.0, 1.0)), (what, "rows", ref.idx[:8])
    fin = scores[np.isfinite(scores)]
    if count:
        assert np.abs(vals[:count] - scores[ref.idx]).max() <= 1e-9 * np.abs(fin).max() + 1e-14, what
    assert np.all(vals[count:] == NEG), what
    return ref


def _basis(D, F, seed, zero=False):
    rng = np.random.default_rng(seed)
    W = np.zeros((F, D)) if zero else rng.standard_normal((F, D)) / (0.35 * np.sqrt(D))
    return W, rng.uniform(0, 2 * np.pi, F), rng.standard_normal(F)


# =============================================================== A. selection, exact
def _mean_search0(eng, post, cand, K, sep):
    xs, mus = eng.mean_search(post, cand, K=K, sep=sep, iters=0, tol=1e-9, sync=False)      # all K rows
    n, _ = eng.mean_search(post, cand, K=K, sep=sep, iters=0, tol=1e-9)                      # h_found
    mus = host(mus)
    assert len(n) == int(np.isfinite(mus).sum())
    return host(xs), mus, len(n)


@pytest.mark.parametrize("D,M", SHAPES)
def test_mean_search_picks_on_the_shape_table(eng, D, M):
    post = _model(eng, D)[0]
    cand = sr.lattice(np.random.default_rng(D + M), M, D, 10)
    assert sr.group_shape(M, D) == dict(zip(SHAPES, [(1, 50), (3, 3000), (2, 2049), (3, 1756), (80, 875), (4, 214)]))[(D, M)]
    sc = _mean_scores(eng, post, cand)
    for K, sep in ((16, 0.25), (64, 0.25)) if M == 50 else ((32, 0.25 * np.sqrt(D)), (32, 0.0)):
        xs, mus, n = _mean_search0(eng, post, cand, K, sep)
        ref = _check_picks(sc, cand, K, sep, xs, mus, n, f"mean_search D={D} M={M} K={K} sep={sep}")
        assert 1 <= ref.count <= K and (ref.count == K if sep == 0.0 else True) and (ref.count < K if K == 64 else True)


@pytest.mark.parametrize("D,M", SHAPES)
def test_rff_search_picks_on_the_shape_table(eng, D, M):
    cand = sr.lattice(np.random.default_rng(2 * D + M), M, D, 10)
    W, b, om = _basis(D, 96, 3 + D)
    sc = _rff_scores(eng, cand, W, b, 0.7, om)
    for K, sep in ((16, 0.25), (64, 0.25)) if M == 50 else ((32, 0.25 * np.sqrt(D)), (32, 0.0)):
        xs, vals, n = _rff_search_raw(eng, cand, None, W, b, 0.7, om, K, sep, 0, 1e-10)
        ref = _check_picks(sc, cand, K, sep, xs, vals, n, f"rff_search D={D} M={M} K={K} sep={sep}")
        assert 1 <= ref.count <= K and (ref.count == K if sep == 0.0 else True) and (ref.count < K if K == 64 else True)


def test_strike_boundary_and_duplicate_ties(eng):
    """Lattice 1 / 16 at D = 3, M = 4000, sep = 0.25: thousands of pairs sit exactly at d2 == sep2 (a strike with < in
    place of <= keeps them) and duplicated rows tie bitwise."""
    post = _model(eng, 3)[0]
    cand = sr.lattice(np.random.default_rng(16), 4000, 3, 4)
    sc = _mean_scores(eng, post, cand)
    xs, mus, n = _mean_search0(eng, post, cand, 64, 0.25)
    ref = _check_picks(sc, cand, 64, 0.25, xs, mus, n, "mean_search boundary")
    assert ref.hits > 100 and ref.ties > 0 and ref.margin == 0.0
    W, b, om = _basis(3, 96, 5)
    sr_ = _rff_scores(eng, cand, W, b, 0.7, om)
    xs, vals, n = _rff_search_raw(eng, cand, None, W, b, 0.7, om, 64, 0.25, 0, 1e-10)
    ref = _check_picks(sr_, cand, 64, 0.25, xs, vals, n, "rff_search boundary")
    assert ref.hits > 100 and ref.ties > 0
    # sep = 0 strikes the winner and its duplicates only
    xs, mus, n = _mean_search0(eng, post, cand, 64, 0.0)
    ref = _check_picks(sc, cand, 64, 0.0, xs, mus, n, "mean_search sep = 0")
    assert ref.count == 64 and len(np.unique(xs, axis=0)) == 64


@pytest.mark.parametrize("D,M,p", [(3, 50, 4), (3, 4000, 4), (6, 5267, 3)])
def test_all_scores_tie(eng, D, M, p):
    """W = 0: every candidate scores a sum_f omega_f cos(b_f), so the picks are the groups' first rows in index order under
    the strikes -- every merge of the argmax (the DPP steps, the four rows of a wavefront, the 16 wave records) is decided
    by the index alone."""
    cand = sr.lattice(np.random.default_rng(M), M, D, p)
    W, b, om = _basis(D, 96, 9, zero=True)
    sc = _rff_scores(eng, cand, W, b, 0.7, om)
    assert np.all(sc == sc[0]) and np.isfinite(sc[0])
    xs, vals, n = _rff_search_raw(eng, cand, None, W, b, 0.7, om, 64, 0.25, 0, 1e-10)
    ref = _check_picks(sc, cand, 64, 0.25, xs, vals, n, "all-tie")
    assert ref.ties >= ref.count - 1 and np.all(np.diff(ref.idx) > 0) and ref.idx[0] == 0


@pytest.mark.parametrize("D,M", [(3, 50), (6, 5267)])
def test_nan_scores_never_start(eng, D, M):
    post = _model(eng, D)[0]
    rng = np.random.default_rng(D)
    cand = sr.lattice(rng, M, D, 10)
    G, Tg = sr.group_shape(M, D)
    bad = np.flatnonzero(rng.random(M) < 0.1)
    cand[bad, rng.integers(0, D, bad.size)] = np.nan                    # scattered
    cand[4 * G:5 * G] = np.nan                                          # a whole group
    sc = _mean_scores(eng, post, cand)
    assert np.isnan(sc[bad]).all() and np.isnan(sc[4 * G:5 * G]).all() and np.isfinite(np.delete(sc, np.r_[bad, 4 * G:5 * G])).all()
    pool, sh = cand, np.zeros((1, D))                                   # frac(x + 0) = x on [0, 1); a row with a 1.0 becomes 0.0
    pool = np.where(pool == 1.0, 0.5, pool)
    scp = _mean_scores(eng, post, pool)
    for K, sep in ((16, 0.25 * np.sqrt(D)), (16, 0.0)):
        xs, mus, n = _mean_search0(eng, post, cand, K, sep)
        ref = _check_picks(sc, cand, K, sep, xs, mus, n, "mean_search with NaN rows")
        assert ref.count >= 1 and np.isfinite(xs[:n]).all()
        xm, mm = eng.mean_search_multi(post, pool, sh, None, None, K=K, sep=sep, iters=0, screen_fp32=False)
        xm, mm = host(xm)[0], host(mm)[0]
        _check_picks(scp, pool, K, sep, xm, mm, int(np.isfinite(mm).sum()), "mean_search_multi with NaN rows")
    allnan = np.full((M, D), np.nan)
    xs, mus, n = _mean_search0(eng, post, allnan, 8, 0.1)
    assert n == 0 and np.all(mus == NEG)
    xm, mm = eng.mean_search_multi(post, allnan, sh, None, None, K=8, sep=0.1, iters=0, screen_fp32=False)
    assert np.all(host(mm) == NEG)


def _multi_case(eng, post, score_rows, D, M, E_rows, design, K, sep, seed, lattice_extra=True, T=3):
    """mean_search_multi (fp64 screening, iters = 0) of T trials against the rule, trial by trial.  score_rows(rows): the
    fp64 scores of caller-coordinate rows; design: the rows that extra = "design" stands for (caller coordinates)."""
    rng = np.random.default_rng(seed)
    pool, shifts = sr.lattice(rng, M, D, 10), sr.lattice(rng, T, D, 10)
    pool = np.where(pool == 1.0, 0.0, pool)
    extra = design if design is not None else (sr.lattice(rng, E_rows, D, 10) if E_rows else None)
    xprev = sr.lattice(rng, 1, D, 10)[0]
    xs, mus = eng.mean_search_multi(post, pool, shifts, "design" if design is not None else extra, xprev, K=K, sep=sep,
                                    iters=0, tol=1e-9, screen_fp32=False)
    xs, mus = host(xs), host(mus)
    refs = []
    for t in range(T):
        rows, n = sr.trial_rows(pool, shifts, t, extra, xprev)
        Mt = rows.shape[0]
        assert np.array_equal(rows[:M], host(eng.shift_points(pool, shifts[t])))
        sc = sr.trial_scores(score_rows(rows[:n]), Mt)
        cnt = int(np.isfinite(mus[t]).sum())
        assert np.all(np.isfinite(mus[t][:cnt]))                          # found rows come first
        refs.append(_check_picks(sc, rows, K, sep, xs[t], mus[t], cnt, f"trial {t}"))
        if not lattice_extra:
            assert refs[-1].margin > 1e-9, refs[-1].margin                # no strike decision within rounding of sep
    return refs


def test_mean_search_multi_picks(eng):
    post, X, th, _ = _model(eng, 3)
    sc = lambda rows: _mean_scores(eng, post, rows)                       # noqa: E731
    _multi_case(eng, post, sc, 3, 50, 5, None, 16, 0.25, 1)               # no thinning; extra rows + xprev in trial 0
    _multi_case(eng, post, sc, 3, 50, 0, X, 16, 0.3, 2, lattice_extra=False)              # extra = "design": the model's rows
    post6, X6, _, _ = _model(eng, 6)
    sc6 = lambda rows: _mean_scores(eng, post6, rows)                     # noqa: E731
    # Mt = 5266 + 7 = 5273: G = 3, 1758 groups; rows >= 5266 are absent in trials 1, 2 -- their last two groups hold
    # nothing but absent slots
    assert sr.group_shape(5273, 6) == (3, 1758)
    _multi_case(eng, post6, sc6, 6, 5266, 6, None, 32, 0.5, 3)
    _multi_case(eng, post6, sc6, 6, 5266, 0, X6, 32, 0.3 * np.sqrt(6) + 1e-3, 4, lattice_extra=False)


def test_mean_search_multi_picks_ard(eng):
    """Per-dimension length scales: sep, the box and the returned rows are in the caller's coordinates; "design" means the
    model's scaled rows divided by s, which are not lattice points."""
    ls = np.array([0.3, 0.5, 0.8, 1.1, 1.6])
    post, X, th, _ = _model(eng, 5, l=ls)
    assert post.scale is not None
    design = host(post.X) * (1.0 / post.scale)[None, :]                   # x~ (1 / s), the product the library forms
    sc = lambda rows: _mean_scores(eng, post, rows)                       # noqa: E731
    _multi_case(eng, post, sc, 5, 50, 0, design, 16, 0.3, 5, lattice_extra=False)
    _multi_case(eng, post, sc, 5, 50, 4, None, 16, 0.5, 6)
    assert sr.group_shape(6200 + 51, 5) == (3, 2084)
    _multi_case(eng, post, sc, 5, 6200, 0, design, 32, 0.3, 7, lattice_extra=False)


def test_mean_search_multi_picks_camphor(eng):
    """camphor_copper_ard_kernel: plain Euclidean distance in the six caller coordinates; "design" is the caller's rows."""
    post, X, th, _ = _model(eng, 6, kernel=CAM, l=sr.CAMPHOR_LS)
    sc = lambda rows: _mean_scores(eng, post, rows)                       # noqa: E731
    _multi_case(eng, post, sc, 6, 50, 0, X, 16, 0.3, 8, lattice_extra=False)
    _multi_case(eng, post, sc, 6, 5266, 6, None, 32, 0.5, 9)


def test_rff_search_camphor_picks(eng):
    rng = np.random.default_rng(12)
    W, b, om = rng.standard_normal((96, 11)), rng.uniform(0, 2 * np.pi, 96), rng.standard_normal(96)
    for M, K, sep in ((50, 16, 0.25), (5267, 32, 0.5)):
        cand = sr.lattice(rng, M, 6, 10)
        sc = _rff_scores(eng, eng.camphor_embed(cand, sr.CAMPHOR_LS), W, b, 0.7, om)
        xs, vals, n = _rff_search_raw(eng, cand, sr.CAMPHOR_LS, W, b, 0.7, om, K, sep, 0, 1e-10)
        _check_picks(sc, cand, K, sep, xs, vals, n, f"rff_search_camphor M={M}")


@pytest.mark.parametrize("S", [3, 65])
def test_rff_search_multi_picks_per_sample(eng, S):
    """Sample s picks from its own scores and reports its own count."""
    rng = np.random.default_rng(S)
    for D, M, K, sep in ((3, 50, 64, 0.25), (6, 5267, 24, 0.5)):
        cand = sr.lattice(rng, M, D, 10)
        W, b, _ = _basis(D, 96, 20 + D)
        Om = rng.standard_normal((S, 96))
        if D == 3:
            Om[1] = 0.0                                                   # one sample that ties everywhere
        sc = eng.rff_score_multi(cand, W, b, 0.7, Om)
        assert torch.equal(sc, eng.rff_score_multi(cand, W, b, 0.7, Om))
        sc = host(sc)
        x, v, found = eng.rff_search_multi(cand, W, b, 0.7, Om, K=K, sep=sep, iters=0, tol=1e-10)
        counts = set()
        for s in range(S):
            counts.add(_check_picks(sc[s], cand, K, sep, x[s], v[s], int(found[s]), f"sample {s}").count)
        if D == 3 and S == 65:
            assert len(counts) > 1 and max(counts) < K                    # the counts do differ between samples


def test_rff_search_multi_camphor_picks(eng):
    rng = np.random.default_rng(14)
    W, b, Om = rng.standard_normal((96, 11)), rng.uniform(0, 2 * np.pi, 96), rng.standard_normal((3, 96))
    for M, K, sep in ((50, 16, 0.25), (5267, 24, 0.5)):
        cand = sr.lattice(rng, M, 6, 10)
        sc = host(eng.rff_score_multi(eng.camphor_embed(cand, sr.CAMPHOR_LS), W, b, 0.7, Om))
        x, v, found = eng.rff_search_multi_camphor(cand, sr.CAMPHOR_LS, W, b, 0.7, Om, K=K, sep=sep, iters=0, tol=1e-10)
        for s in range(3):
            _check_picks(sc[s], cand, K, sep, x[s], v[s], int(found[s]), f"camphor sample {s}")


def _path_inputs(D, F, S, seed, ard):
    rng = np.random.default_rng(seed)
    X = orc.synthetic_design(10, D, m=4, seed=100 + D)
    th = [0.1, np.linspace(0.4, 1.4, D) if ard else 0.35 * np.sqrt(D), 0.7]
    W = rng.standard_normal((F, D)) / np.broadcast_to(np.asarray(th[1], dtype=float), (D,))
    return X, th, W, rng.uniform(0, 2 * np.pi, F), rng.standard_normal((S, F)), 0.3 * rng.standard_normal((S, X.shape[0]))


@pytest.mark.parametrize("ard", [False, True])
def test_path_search_multi_picks(eng, ard):
    rng = np.random.default_rng(15)
    for D, M, K, sep in ((3, 50, 16, 0.25), (6, 5267, 24, 0.5)):
        X, th, W, b, Wp, V = _path_inputs(D, 96, 2, 30 + D, ard)
        cand = sr.lattice(rng, M, D, 10)
        sc = eng.path_score_multi(cand, W, b, th, "SE_kernel", X, Wp, V)
        assert torch.equal(sc, eng.path_score_multi(cand, W, b, th, "SE_kernel", X, Wp, V))
        sc = host(sc)
        x, v, found = eng.path_search_multi(cand, W, b, th, "SE_kernel", X, Wp, V, K=K, sep=sep, iters=0, tol=1e-10)
        for s in range(2):
            _check_picks(sc[s], cand, K, sep, x[s], v[s], int(found[s]), f"path {s} ard={ard}")


# =============================================================== A'. fp32 screening: properties of the picks
@pytest.mark.parametrize("D,M", [(3, 50), (3, 4000), (6, 2600)])
def test_fp32_screening_picks_have_the_rules_properties(eng, D, M):
    post = _model(eng, D)[0]
    rng = np.random.default_rng(40 + D)
    assert M + 4 <= sr.select_capacity(D)                                 # no thinning: every row is a survivor
    pool, shifts = sr.lattice(rng, M, D, 10), sr.lattice(rng, 2, D, 10)
    pool = np.where(pool == 1.0, 0.0, pool)
    extra, xprev = sr.lattice(rng, 3, D, 10), sr.lattice(rng, 1, D, 10)[0]
    K, sep = 16, 0.25 * np.sqrt(D / 3.0)
    xs, mus = eng.mean_search_multi(post, pool, shifts, extra, xprev, K=K, sep=sep, iters=0, screen_fp32=True)
    xs, mus = host(xs), host(mus)
    for t in range(2):
        rows, n = sr.trial_rows(pool, shifts, t, extra, xprev)
        rows = rows[:n]
        mu = _mean_scores(eng, post, rows)
        ok = np.isfinite(mus[t])
        cnt = int(ok.sum())
        assert cnt >= 1 and np.all(ok[:cnt]) and np.all(mus[t][cnt:] == NEG)                    # found rows come first
        free = np.ones(n, dtype=bool)                                     # rows farther than sep from the earlier picks
        for k in range(cnt):
            hit = np.flatnonzero((rows == xs[t, k][None, :]).all(axis=1))
            assert hit.size >= 1, (t, k)                                  # bitwise a candidate row
            assert free[hit[0]], "within sep of an earlier pick"
            assert abs(mus[t, k] - mu[hit[0]]) <= 1e-9 * np.abs(mu).max() + 1e-14
            assert mu[hit[0]] >= mu[free].max() - 1e-5 * np.abs(mu).max(), (t, k)
            d2 = np.zeros(n)
            for d in range(D):
                dx = rows[:, d] - xs[t, k, d]
                d2 += dx * dx
            free &= d2 > sep * sep
        assert cnt == K or not free.any()


# =============================================================== B. the ascent, step by step
def _compare_ascent(label, run, fg, starts, tol, mu_scale, has_it=True):
    """run(n) -> (x [K, D], mu [K], it [K] or None) of the device after n iterations from `starts`."""
    s = sr.sensitivity(fg, starts, sr.ASCENT_ITERS, tol, mu_scale)
    bound = sr.x_bound(s.dev)
    assert s.flips == 0 and s.left_out <= 0.125, (label, s.flips, s.left_out)
    worst = np.zeros(sr.ASCENT_ITERS + 1)
    for n in range(sr.ASCENT_ITERS + 1):
        x, mu, it = run(n)
        keep = s.keep[:, n]
        if n == 0:
            assert np.array_equal(x, np.clip(starts, 0.0, 1.0)), label
        if has_it:
            assert np.array_equal(it[keep], s.its[keep, n]), (label, n, it, s.its[:, n])
        worst[n] = np.abs(x - s.xs[:, n])[keep].max()
        assert np.abs(mu - s.mus[:, n])[keep].max() <= 1e-9 * mu_scale + 1e-14, (label, n)
    print(f"STAGES {label} tol {tol:g}: |x_dev - x_ref| per n {np.array2string(worst, precision=1)}, bound "
          f"{np.array2string(bound, precision=1)}, left out {s.left_out:.3f}, it at n = {sr.ASCENT_ITERS}: "
          f"{np.bincount(s.its[:, -1], minlength=sr.ASCENT_ITERS + 1)}")
    assert np.all(worst <= bound), (label, worst, bound)
    return s


@pytest.mark.parametrize("tol", sr.TOLS)
@pytest.mark.parametrize("name", list(sr.MEAN_CASES))
def test_mean_ascent_steps(eng, name, tol):
    c = sr.MEAN_CASES[name]
    post, X, th, alpha = _model(eng, c["D"], c["kernel"], c.get("l"), c["n_q"], c["m"])
    fg = sr.mean_fg(X, th, c["kernel"], alpha)
    starts = sr.ascent_starts(c["D"], 7, fg)
    mu0 = np.array([fg(np.clip(s, 0, 1))[0] for s in starts])

    def run(n):
        x, mu, it = eng.mean_ascent(post, starts, iters=n, tol=tol)
        return host(x), host(mu), host(it)
    s = _compare_ascent(f"mean_ascent {name}", run, fg, starts, tol, np.abs(mu0).max())
    if tol > 1e-3:
        assert np.isin(s.its[:, -1], (1, 2)).any()                        # some starts do stop after a move or two


@pytest.mark.parametrize("name", list(sr.RFF_CASES))
def test_rff_ascent_steps(eng, name):
    cand, W, b, sf, Om, ls = sr.rff_case(name)
    om = Om[0]
    rows = cand if ls is None else eng.camphor_embed(cand, ls)
    sc = _rff_scores(eng, rows, W, b, sf, om)
    K = 24
    x0, v0, n0 = _rff_search_raw(eng, cand, ls, W, b, sf, om, K, 0.05, 0, 1e-10)
    ref = _check_picks(sc, cand, K, 0.05, x0, v0, n0, name)
    assert ref.count == K
    fg = sr.rff_fg(W, b, sf, om, ls)
    for tol in sr.TOLS:
        def run(n):
            x, v, cnt = _rff_search_raw(eng, cand, ls, W, b, sf, om, K, 0.05, n, tol)
            assert cnt == K
            return x, v, None
        _compare_ascent(f"rff_search {name}", run, fg, x0, tol, np.abs(sc).max(), has_it=False)


def test_rff_search_multi_ascent_follows_each_samples_weights(eng):
    """Workgroup s K + k climbs sample s's function from sample s's k-th start."""
    cand, W, b, sf, Om, _ = sr.rff_case("d6_f96", S=3)
    K = 8
    sc = host(eng.rff_score_multi(cand, W, b, sf, Om))
    x0, v0, f0 = eng.rff_search_multi(cand, W, b, sf, Om, K=K, sep=0.05, iters=0, tol=1e-9)
    runs = {n: eng.rff_search_multi(cand, W, b, sf, Om, K=K, sep=0.05, iters=n, tol=1e-9) for n in range(sr.ASCENT_ITERS + 1)}
    for s in range(3):
        assert _check_picks(sc[s], cand, K, 0.05, x0[s], v0[s], int(f0[s]), f"sample {s}").count == K
        _compare_ascent(f"rff_search_multi sample {s}", lambda n: (runs[n][0][s], runs[n][1][s], None),
                        sr.fg_rff(W, b, sf, Om[s]), x0[s], 1e-9, np.abs(sc[s]).max(), has_it=False)
    assert not np.array_equal(x0[0], x0[1])


@pytest.mark.parametrize("ard", [False, True])
def test_path_search_multi_ascent_steps(eng, ard):
    D, K = 6, 12
    X, th, W, b, Wp, V = _path_inputs(D, 96, 2, 50, ard)
    cand = np.random.default_rng(51).random((600, D))
    sc = host(eng.path_score_multi(cand, W, b, th, "SE_kernel", X, Wp, V))
    runs = {n: eng.path_search_multi(cand, W, b, th, "SE_kernel", X, Wp, V, K=K, sep=0.05, iters=n, tol=1e-9)
            for n in range(sr.ASCENT_ITERS + 1)}
    for s in range(2):
        x0 = runs[0][0][s]
        assert int(runs[0][2][s]) == K
        _compare_ascent(f"path_search_multi path {s} ard={ard}", lambda n: (runs[n][0][s], runs[n][1][s], None),
                        sr.fg_path(W, b, th, "SE_kernel", X, Wp[s], V[s]), x0, 1e-9, np.abs(sc[s]).max(), has_it=False)
