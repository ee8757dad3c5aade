"""GPU: the thin contraction of the pruned search (quadform_thin, csrc/predict.hip) -- a pruned chunk with at most THIN_MAX
survivors is contracted on 16-column tiles, one 16 x 16 accumulator tile per wavefront, in the place of the compact
launch's 128 x 128 tiles.

The yardstick is the SAME call on an engine created with PPBO_PRUNE=0: the record must agree bit for bit, value and
index.  Every case is also run on an engine with PPBO_PRUNE=1, PPBO_PRUNE_THIN=0 (the compact launch on its tiles), and
ppbo_predict_prune_report must say that the chunk was pruned with the intended number of survivors, so that no case
passes by falling back to the full launch.  Under SCORE_VARIANCE the record's value is the winner's variance itself: the
contraction's bits are compared directly.

How a survivor count is forced: the report of a pool of candidates gives every candidate's score interval; the candidate
with the largest lower bound sets the threshold, candidates whose upper bound clears it survive beside it, candidates
whose upper bound stays below it are ruled out, and copies of the best candidate fill the count up where the pool has
too few natural survivors (a copy carries the best candidate's interval).  The engines of this file take a survivor
capacity (PPBO_PRUNE_CAP) that makes the switch point reachable with about 2048 candidates.
"""
import numpy as np
import pytest

from test_gpu_kstar_star import Hand, _engine, host, star_design
from test_gpu_prune import posterior, real_posterior, same_record
from test_gpu_var_projection import call_record, call_search, smooth_posterior

pytestmark = pytest.mark.gpu

EDGE = 1
THIN_MAX = 256          # csrc/predict.hip
CAP = 4 * 320           # the thin path takes n_surv <= capacity / 4 (its workgroups are the compact launch's): 320 > THIN_MAX + 1


@pytest.fixture(scope="module")
def thin():
    e = _engine(PPBO_FUSED=0, PPBO_PRUNE=1, PPBO_PRUNE_CAP=CAP)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tile():
    e = _engine(PPBO_FUSED=0, PPBO_PRUNE=1, PPBO_PRUNE_CAP=CAP, PPBO_PRUNE_THIN=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def off():
    e = _engine(PPBO_FUSED=0, PPBO_PRUNE=0)
    yield e
    e.close()


_MODELS = {}


def model(eng, key):
    """(posterior, candidate pool, projection or None) of a named model, built once."""
    if key in _MODELS:
        return _MODELS[key]
    if key in ("d20_384", "d2_384", "d20_96"):                   # test_gpu_prune.py's models: 384 rows = three row tiles
        post, X, pool = posterior(eng, key)
    elif key == "d20_312":                                       # m = 25: 26-row stars, 312 rows in a zero frame of 384,
        post, X, rng = real_posterior(eng, 12, 25, 20, "SE_kernel", 0.45, seed=31)     # K extent padded to 320
        near = X[rng.integers(0, X.shape[0], 1500)] + 0.05 * rng.standard_normal((1500, 20))
        pool = np.concatenate([near, rng.random((1500, 20))])[rng.permutation(3000)]
    elif key == "d2_416":                                        # m = 25, the smallest ragged shape that takes a projection
        post, rng = smooth_posterior(eng, 16, 25, 2, "SE_kernel", 1.5)
        X = host(post.X)
        near = X[rng.integers(0, X.shape[0], 1500)] + 0.05 * rng.standard_normal((1500, 2))
        pool = np.concatenate([near, rng.random((1500, 2))])[rng.permutation(3000)]
    else:
        raise KeyError(key)
    pj = None
    if key in ("d2_384", "d2_416"):
        pj = eng.project_variance(post, 1e-6)
        assert pj.rows > 0
    _MODELS[key] = (post, pool, pj)
    return _MODELS[key]


def mustar_of(off, post, pool, score):
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    if score != SCORE_POINTWISE_EI:
        return 0.0
    return float(np.sort(host(off.predict(post, pool)["mu"]))[-3])


def forced(eng, post, pool, score, mustar, pj, n, n_out, seed=0):
    """Candidates of which exactly n survive: (Xc, positions of the survivors, how many of them are distinct rows)."""
    rep = eng.prune_report(post, pool, score, mustar, projection=pj)
    lo, hi = host(rep["s_lo"]), host(rep["s_hi"])
    fin = np.isfinite(lo) & np.isfinite(hi)
    best = int(np.argmax(np.where(fin, lo, -np.inf)))
    b = lo[best]
    assert b > 0.0
    # (the sums behind the bounds are split by the size of the call: 1e-9 relative is far above their rounding)
    keep = np.flatnonzero(fin & (hi > b * (1.0 + 1e-9)) & (lo < b * (1.0 - 1e-9)))
    keep = keep[keep != best][:n - 1]
    out = np.flatnonzero(fin & (hi < b * (1.0 - 1e-9)))[:n_out]
    rng = np.random.default_rng(seed + n)
    rows = np.concatenate([[best], keep, np.full(n - 1 - keep.size, best, dtype=np.int64)]).astype(np.int64)
    rows = rows[rng.permutation(n)]
    M = n + out.size
    at = np.sort(rng.choice(M, n, replace=False))
    idx = np.empty(M, dtype=np.int64)
    mask = np.zeros(M, dtype=bool)
    mask[at] = True
    idx[mask] = rows
    idx[~mask] = out
    return pool[idx].copy(), at, 1 + keep.size


def three_ways(thin, tile, off, post, Xc, score, mustar, pj, n_surv, label):
    """The record on the three engines, bit for bit; the thin engine's report says pruned with n_surv survivors."""
    rep = thin.prune_report(post, Xc[:65536], score, mustar, projection=pj)
    a, b, c = (call_record(e, post, Xc, score, mustar, pj) for e in (thin, tile, off))
    print(f"{label} M={Xc.shape[0]} score={score}: thin {a} tile {b} off {c}, n_surv {rep['n_surv']} pruned {rep['pruned']}")
    assert rep["pruned"] == 1 and rep["n_surv"] == n_surv
    assert same_record(a, c) and same_record(b, c)
    assert np.isfinite(c[0]) and c[1] >= 1000.0
    assert call_search(thin, post, Xc, score, mustar, pj) == call_search(off, post, Xc, score, mustar, pj)
    return a


COUNTS = [1, 15, 16, 17, 2 * 16 + 1, THIN_MAX, THIN_MAX + 1]


@pytest.mark.parametrize("n", COUNTS)
def test_survivor_counts_edge_form(thin, tile, off, n):
    """The edge form without a projection, 384 rows (three row tiles add to a column), pointwise EI: survivor counts around
    a column group, several groups and the switch point, with about 1750 ruled-out candidates between the survivors."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    post, pool, _ = model(thin, "d20_384")
    mustar = mustar_of(off, post, pool, SCORE_POINTWISE_EI)
    Xc, at, distinct = forced(thin, post, pool, SCORE_POINTWISE_EI, mustar, None, n, 1750)
    assert Xc.shape[0] >= n + 1000
    three_ways(thin, tile, off, post, Xc, SCORE_POINTWISE_EI, mustar, None, n, f"edge n={n} ({distinct} distinct)")


@pytest.mark.parametrize("score_name", ["ei", "variance"])
@pytest.mark.parametrize("key", ["d2_384", "d2_416"])
@pytest.mark.parametrize("n", [1, 17, 2 * 16 + 1])
def test_survivor_counts_dense_form(thin, tile, off, key, n, score_name):
    """The projected operator T (every row runs the whole K range) on the smooth designs: D = 2 leaves wide intervals, so
    the survivors are distinct candidates.  d2_416: 26-row stars, padded K extent.  Then the winner leaves and the search
    runs again, three times: more than one column's bits reach the record."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    score = SCORE_POINTWISE_EI if score_name == "ei" else SCORE_VARIANCE
    post, pool, pj = model(thin, key)
    mustar = mustar_of(off, post, pool, score)
    Xc, at, distinct = forced(thin, post, pool, score, mustar, pj, n, 200)
    rec = three_ways(thin, tile, off, post, Xc, score, mustar, pj, n, f"dense {key} n={n} ({distinct} distinct)")
    for _ in range(3):
        if Xc.shape[0] < 2:
            break
        Xc = np.delete(Xc, int(rec[1]) - 1000, axis=0)
        a, c = call_record(thin, post, Xc, score, mustar, pj), call_record(off, post, Xc, score, mustar, pj)
        assert same_record(a, c)
        rec = c
        if not np.isfinite(rec[0]):
            break


@pytest.mark.parametrize("score_name", ["ei", "variance"])
@pytest.mark.parametrize("n", [1, 17])
def test_rows_that_are_no_whole_tile(thin, tile, off, n, score_name):
    """m = 25, N = 26 x 12 = 312 in the edge form: the last row tile ends in the zero frame, the K extent is padded to 320
    and every 32-row group of the operator ends its K range at its own rows."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI, SCORE_VARIANCE
    score = SCORE_POINTWISE_EI if score_name == "ei" else SCORE_VARIANCE
    post, pool, _ = model(thin, "d20_312")
    mustar = mustar_of(off, post, pool, score)
    Xc, at, distinct = forced(thin, post, pool, score, mustar, None, n, 300)
    three_ways(thin, tile, off, post, Xc, score, mustar, None, n, f"ragged n={n} ({distinct} distinct)")


def test_single_candidates_variance_bits(thin, tile, off):
    """One candidate per call on a hand-built edge-form posterior of 312 rows (a random lower-triangular operator: every row
    group's K cut matters): the chunk is pruned with one survivor and the record IS that candidate's variance."""
    from ppbo_amd.engine import SCORE_VARIANCE
    rng = np.random.default_rng(5)
    m, n_q, D = 25, 12, 6
    X = star_design(rng, n_q, m, D, "general")
    post = Hand(rng, X, [1.0, 0.4, 1.1], "Matern52_kernel", m, EDGE).on(thin)
    Xc = np.concatenate([rng.random((9, D)), X[[0, 27, 311]]])
    var = host(off.predict(post, Xc, score=SCORE_VARIANCE)["var"])
    for c in range(Xc.shape[0]):
        call_record(thin, post, 1.0 - Xc[c:c + 1], SCORE_VARIANCE, 0.0, None)      # (nothing stale can stand in)
        a = call_record(thin, post, Xc[c:c + 1], SCORE_VARIANCE, 0.0, None)
        b = call_record(tile, post, Xc[c:c + 1], SCORE_VARIANCE, 0.0, None)
        assert a[0] == var[c] and b[0] == var[c] and a[1] == b[1] == 1000.0
    rep = thin.prune_report(post, Xc[:1], SCORE_VARIANCE)
    assert rep["pruned"] == 1 and rep["n_surv"] == 1


@pytest.mark.parametrize("key", ["d20_384", "d20_312"])
def test_a_nan_candidate_beside_the_survivors(thin, tile, off, key):
    """A candidate with a NaN coordinate right behind the best one: it survives (s_hi = +inf) into the best candidate's
    column group, its whole K* column is NaN -- also beyond the K cut of every early row group of the edge form -- and it
    never scores.  The columns around it keep their bits.
    (A non-finite K* entry in a candidate's LATE rows alone cannot be made through the library's entries: K* comes from
    the K* pass, and whatever makes one of its entries non-finite makes the candidate's mean non-finite too.)"""
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    post, pool, _ = model(thin, key)
    mustar = mustar_of(off, post, pool, SCORE_POINTWISE_EI)
    Xc, at, _ = forced(thin, post, pool, SCORE_POINTWISE_EI, mustar, None, 17, 300)
    win = int(call_record(off, post, Xc, SCORE_POINTWISE_EI, mustar, None)[1]) - 1000
    Xn = np.insert(Xc, win + 1, Xc[win], axis=0)
    Xn[win + 1, 3] = np.nan
    rec = three_ways(thin, tile, off, post, Xn, SCORE_POINTWISE_EI, mustar, None, 18, f"NaN beside the best ({key})")
    assert rec[1] == 1000.0 + win


def test_two_chunks(thin, tile, off):
    """65536 + 128 candidates on the 96-row model: a thin chunk, the chunk boundary, and a second chunk of one column tile
    with a plan of its own; the winner sits in the second chunk."""
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    post, pool, _ = model(thin, "d20_96")
    rng = np.random.default_rng(9)
    Xc = pool[rng.integers(0, pool.shape[0], 65536 + 128)] + 0.02 * rng.standard_normal((65536 + 128, pool.shape[1]))
    mu = host(off.predict(post, Xc)["mu"])
    Xc[65536 + 77] = Xc[int(np.argmax(mu))]
    mustar = float(np.sort(mu)[-40])
    rep = thin.prune_report(post, Xc[:65536], SCORE_POINTWISE_EI, mustar)
    a, b, c = (call_record(e, post, Xc, SCORE_POINTWISE_EI, mustar, None) for e in (thin, tile, off))
    print(f"two chunks: thin {a} tile {b} off {c}, first chunk n_surv {rep['n_surv']} pruned {rep['pruned']}")
    assert rep["pruned"] == 1 and 1 <= rep["n_surv"] <= THIN_MAX
    assert same_record(a, c) and same_record(b, c)
