"""CPU: the NumPy references of the searches' start selection and ascent (tests/search_ref.py) are right -- the greedy
rule against an independent statement of it, the capacity numbers the source quotes, the ascent on closed forms, the
objectives against central differences, and the references' own sensitivity on the start sets
tests/test_gpu_search_stages.py uses (which measures it again with its own fitted models and holds the device to
search_ref.x_bound of it: 100 times the deviation, floored at 1e-10)."""
import numpy as np
import pytest

import search_ref as sr
from oracle import ppbo_oracle as orc


# ---------------------------------------------------------------- selection
def test_capacity_numbers_of_the_source():
    """meangrad.hip quotes 2633 survivors at D = 6 and 877 at D = 20 (144 * 1024 bytes over 8 + 8 D), 4096 up to D = 3 and
    never fewer than 64; the shape table of tests/test_gpu_search_stages.py follows from them."""
    assert [sr.select_capacity(D) for D in (1, 2, 3, 4, 6, 20, 64)] == [4096, 4096, 4096, 3686, 2633, 877, 283]
    assert sr.select_capacity(400) == 64
    shapes = {(3, 50): (1, 50), (1, 9000): (3, 3000), (2, 4097): (2, 2049), (6, 5267): (3, 1756), (20, 70000): (80, 875),
              (64, 854): (4, 214)}
    for (D, M), gt in shapes.items():
        assert sr.group_shape(M, D) == gt
    assert 1756 * 7 * 8 > 96 * 1024 and 875 * 21 * 8 == 147000


def _inputs(rng, M, D, kind):
    cand = sr.lattice(rng, M, D, 4) if kind == "lattice" else rng.random((M, D))
    sc = rng.standard_normal(M)
    if kind == "lattice":
        sc = np.round(sc * 4) / 4                           # many ties
    sc[rng.random(M) < 0.05] = np.nan
    sc[rng.random(M) < 0.05] = -np.inf
    return sc, cand


@pytest.mark.parametrize("kind", ["lattice", "uniform"])
@pytest.mark.parametrize("D,M", [(3, 1), (3, 50), (3, 4000), (3, 4096), (3, 4097), (3, 8193), (6, 2633), (6, 2634), (6, 5267),
                                 (20, 877), (20, 1755), (64, 854)])
def test_select_starts_is_the_greedy_rule(kind, D, M):
    rng = np.random.default_rng(100 * D + M)
    sc, cand = _inputs(rng, M, D, kind)
    cap = sr.select_capacity(D)
    for K, sep in ((16, 0.25), (64, 0.25 * np.sqrt(D)), (5000 if M <= 50 else 300, 0.0), (8, 10.0)):
        sel = sr.select_starts(sc, cand, K, sep)
        ref = sr.greedy_by_sorting(sc, cand, K, sep)
        assert sel.count == len(ref) <= min(K, cap, M) and np.array_equal(sel.idx, ref), (K, sep)
        assert np.all(np.isfinite(sc[sel.idx]))
        if sep == 10.0:
            assert sel.count <= 1
    if kind == "lattice" and M >= 4000:
        sel = sr.select_starts(sc, cand, 64, 0.25)
        assert sel.hits > 0 and sel.ties > 0 and sel.margin == 0.0      # the boundary and ties are actually met


def test_thinning_edges():
    # first maximum under strict >, NaN never wins, all-NaN and all -inf groups yield -inf, the ragged last group
    D = 3
    cap = sr.select_capacity(D)
    M = 2 * cap + 2                                         # G = 3, the last group has one member
    G, Tg = sr.group_shape(M, D)
    assert (G, Tg) == (3, 2732) and M - (Tg - 1) * G == 1
    sc = np.zeros(M)
    sc[0:3] = [1.0, 1.0, 0.5]                               # tie: the first
    sc[3:6] = [np.nan, 2.0, np.nan]
    sc[6:9] = np.nan
    sc[9:12] = -np.inf
    sc[-2:] = [5.0, 4.0]                                    # the 5 belongs to the group before
    gv, gi = sr.thin(sc, D)
    assert list(gi[:4]) == [0, 4, 6, 9] and list(gv[:4]) == [1.0, 2.0, -np.inf, -np.inf]
    assert gi[-1] == M - 1 and gv[-1] == 4.0 and gi[-2] == M - 2 and gv[-2] == 5.0
    cand = np.random.default_rng(0).random((M, D))
    sel = sr.select_starts(np.full(M, np.nan), cand, 8, 0.1)
    assert sel.count == 0 and sel.idx.size == 0 and sel.margin == np.inf
    # sep = 0 strikes the winner and its duplicates only
    cand[5] = cand[2]
    sc = -np.arange(M, dtype=float)
    sc[5] = sc[2] = 7.0
    sel = sr.select_starts(sc[:100], cand[:100], 4, 0.0)
    assert list(sel.idx) == [2, 0, 1, 3] and sel.ties == 1


def test_trial_rows():
    rng = np.random.default_rng(2)
    pool, shifts, extra, xp = rng.random((10, 3)), rng.random((3, 3)), rng.random((4, 3)), rng.random(3)
    r0, n0 = sr.trial_rows(pool, shifts, 0, extra, xp)
    r2, n2 = sr.trial_rows(pool, shifts, 2, extra, xp)
    assert r0.shape == r2.shape == (15, 3) and (n0, n2) == (15, 10)
    assert np.array_equal(r0[:10], (pool + shifts[0]) - np.floor(pool + shifts[0])) and np.all((r0[:10] >= 0) & (r0[:10] < 1))
    assert np.array_equal(r0[10:14], extra) and np.array_equal(r0[14], xp)
    assert np.array_equal(sr.trial_scores(np.ones(10), 15), np.r_[np.ones(10), np.full(5, -np.inf)])
    r, n = sr.trial_rows(pool, shifts, 1)
    assert r.shape == (10, 3) and n == 10


# ---------------------------------------------------------------- the ascent on closed forms
def test_ascent_on_a_concave_quadratic_is_newton_at_the_second_move():
    a, c = 3.0, 0.6
    fg = lambda x: (-0.5 * a * float((x - c) @ (x - c)), -a * (x - c))      # noqa: E731
    r = sr.bb_ascent(fg, np.array([0.2]), 4, 1e-12)
    assert abs(r.xs[1, 0] - 0.22) <= 1e-15                   # the first move is 0.02 long
    assert abs(r.xs[2, 0] - c) <= 1e-15                      # s.s / -(s.y) = 1 / a: the Newton step
    assert r.it == 2 and np.array_equal(r.its, [0, 1, 2, 2, 2])      # then |pg| step < tol: no further move is evaluated


def test_ascent_ends_on_the_face_when_the_maximiser_is_outside():
    c = np.array([1.5, 0.4])
    fg = lambda x: (-0.5 * float((x - c) @ (x - c)), -(x - c))              # noqa: E731
    r = sr.bb_ascent(fg, np.array([0.5, 0.1]), 20, 1e-9)
    assert r.x[0] == 1.0 and abs(r.x[1] - 0.4) <= 1e-12
    assert np.all(sr._project(r.x, fg(r.x)[1]) == [0.0, fg(r.x)[1][1]]) and abs(fg(r.x)[1][1]) <= 1e-9
    assert r.it < 20 and r.it == r.its[-1] and np.all(np.diff(r.its) >= 0)
    # a start outside the box is clipped before anything is evaluated
    r0 = sr.bb_ascent(fg, np.array([-0.3, 1.7]), 0, 1e-9)
    assert np.array_equal(r0.x, [0.0, 1.0]) and r0.it == 0 and r0.mu == fg(np.array([0.0, 1.0]))[0] and r0.xs.shape == (1, 2)


def test_rejected_move_quarters_the_step_and_keeps_x():
    # a narrow peak: the first move of 0.02 overshoots it
    fg = lambda x: (-0.5 * 1e4 * float((x - 0.501) @ (x - 0.501)), -1e4 * (x - 0.501))     # noqa: E731
    r = sr.bb_ascent(fg, np.array([0.5]), 3, 1e-12)
    assert r.xs[1, 0] == 0.5 and r.its[1] == 1               # rejected, counted
    assert r.xs[2, 0] == 0.5 and r.its[2] == 2               # 0.005: rejected again
    assert abs(r.xs[3, 0] - 0.50125) <= 1e-15                # 0.00125: accepted
    assert np.all(np.isinf(r.margins[:2, 1])) and np.isfinite(r.margins[2, 1])


def test_doubling_where_the_curvature_is_not_positive():
    fg = lambda x: (float(x.sum()), np.ones_like(x))         # noqa: E731  (linear: y = 0, curv = 0)
    r = sr.bb_ascent(fg, np.array([0.1, 0.1]), 3, 1e-12)
    d = np.diff(r.xs[:, 0])
    assert np.allclose(d, 0.02 / np.sqrt(2) * np.array([1, 2, 4]), rtol=1e-12)


# ---------------------------------------------------------------- objectives against central differences
def _check_grad(fg, D, seed, h=1e-6, rtol=1e-6):
    rng = np.random.default_rng(seed)
    for x in 0.1 + 0.8 * rng.random((3, D)):
        mu, g = fg(x)
        num = np.array([(fg(x + h * e)[0] - fg(x - h * e)[0]) / (2 * h) for e in np.eye(D)])
        assert np.abs(num - g).max() <= rtol * max(np.abs(g).max(), abs(mu)), (np.abs(num - g).max(), np.abs(g).max())


@pytest.mark.parametrize("name", [n for n in sr.MEAN_CASES if not n.endswith("_tall")])
def test_mean_objectives_against_central_differences(name):
    X, th, kernel, m = sr.mean_case(name)
    alpha = np.random.default_rng(1).standard_normal(X.shape[0])
    _check_grad(sr.mean_fg(X, th, kernel, alpha), X.shape[1], 3)


def test_closed_forms_agree_with_each_other():
    rng = np.random.default_rng(5)
    X, alpha, x = rng.random((40, 4)), rng.standard_normal(40), rng.random(4)
    th = [0.1, 0.6, 0.8]
    for a, b in ((sr.fg_matern52(X, th, alpha), sr.fg_ard(X, th, alpha, "Matern52_kernel")),
                 (sr.fg_mean(X, th, alpha, "SE_kernel"), sr.fg_ard(X, [0.1, np.full(4, 0.6), 0.8], alpha, "SE_kernel")),
                 (sr.fg_mean(X, th, alpha, "RQ_kernel"), sr.fg_ard(X, th, alpha, "RQ_kernel"))):
        (m1, g1), (m2, g2) = a(x), b(x)
        assert abs(m1 - m2) <= 1e-12 * np.abs(alpha).sum() and np.abs(g1 - g2).max() <= 1e-11 * np.abs(alpha).sum()
    X6, x6 = rng.random((40, 6)), rng.random(6)
    (m1, g1) = sr.fg_mean(X6, [0.1, 0.4, 0.8], alpha, "camphor_copper_kernel")(x6)
    (m2, g2) = sr.fg_camphor_ard(X6, 0.4 + np.array([0, 0, 0.05, 0, 0, 0]), 0.8, alpha)(x6)
    assert abs(m1 - m2) <= 1e-12 * np.abs(alpha).sum() and np.abs(g1 - g2).max() <= 1e-10 * np.abs(alpha).sum()


@pytest.mark.parametrize("name", list(sr.RFF_CASES))
def test_rff_objectives_against_central_differences(name):
    cand, W, b, sf, om, ls = sr.rff_case(name)
    fg = sr.rff_fg(W, b, sf, om[0], ls)
    _check_grad(fg, cand.shape[1], 4, h=1e-6, rtol=1e-5)
    if ls is None:
        assert abs(fg(cand[0])[0] - orc.rff_score(cand[:1], W, b, sf, om[0])[0]) <= 1e-13


def test_path_objective_against_central_differences_and_pathwise_numpy():
    import pathwise_numpy as pw
    rng = np.random.default_rng(8)
    D, F, N = 4, 64, 30
    X, W, b = rng.random((N, D)), rng.standard_normal((F, D)) / 0.5, rng.uniform(0, 2 * np.pi, F)
    w, v, x = rng.standard_normal(F), rng.standard_normal(N), rng.random(D)
    for th in ([0.1, 0.5, 0.7], [0.1, np.array([0.3, 0.5, 0.8, 1.2]), 0.7]):
        for kernel in ("SE_kernel", "Matern52_kernel"):
            fg = sr.fg_path(W, b, th, kernel, X, w, v)
            _check_grad(fg, D, 2, rtol=1e-5)
            mu, g = fg(x)
            assert abs(mu - pw.paths(x[None], w, v, W, b, X, th, kernel)[0, 0]) <= 1e-12 * (np.abs(w).sum() + np.abs(v).sum())
            assert np.abs(g - pw.path_grad(x, w, v, W, b, X, th, kernel)).max() <= 1e-11 * (np.abs(w).sum() + np.abs(v).sum())


# ---------------------------------------------------------------- the references' own sensitivity
def _alpha(name, X, th, kernel, m):
    if name.endswith("_tall"):
        # (the oracle's fit of 1024 unknowns takes over a minute: unit normal weights here, so these two cases show the
        # method, not the GPU test's numbers; tests/test_gpu_search_stages.py measures the same quantities again with the
        # weights of its device-fitted model and asserts the same limits on them)
        return np.random.default_rng(X.shape[1]).standard_normal(X.shape[0])
    f0, Sinv0 = sr.host_fit(X, th, kernel, m, X.shape[1])
    return Sinv0 @ f0


def _report(label, s):
    print(f"{label}: largest |x - x'| per n {np.array2string(s.dev, precision=1)}, flips {s.flips}, left out {s.left_out:.3f}, "
          f"it at n = {sr.ASCENT_ITERS}: {np.bincount(s.its[:, -1], minlength=sr.ASCENT_ITERS + 1)}")


@pytest.mark.parametrize("tol", sr.TOLS)
@pytest.mark.parametrize("name", list(sr.MEAN_CASES))
def test_mean_ascent_references_are_stable_on_their_starts(name, tol):
    """The reference against its 1e-13-perturbed self from the 24 starts of each case: no branch flips among the kept
    (start, n) pairs, at most one eighth of the pairs is left out, and the bound derived from the deviation stays at or
    below 1e-6 (a deviation of at most 1e-8), four orders below the 1e-2 by which a wrong step rule moves x."""
    X, th, kernel, m = sr.mean_case(name)
    fg = sr.mean_fg(X, th, kernel, _alpha(name, X, th, kernel, m))
    starts = sr.ascent_starts(X.shape[1], 7, fg)
    mu0 = np.array([fg(np.clip(s, 0, 1))[0] for s in starts])
    s = sr.sensitivity(fg, starts, sr.ASCENT_ITERS, tol, np.abs(mu0).max())
    _report(f"{name} tol {tol:g}", s)
    assert s.flips == 0 and s.left_out <= 0.125
    assert sr.x_bound(s.dev).max() <= 1e-6
    if tol > 1e-3:
        assert np.isin(s.its[:, -1], (1, 2)).any()           # the large tolerance does stop some starts early


@pytest.mark.parametrize("name", list(sr.RFF_CASES))
def test_rff_ascent_references_are_stable(name):
    cand, W, b, sf, om, ls = sr.rff_case(name)
    fg = sr.rff_fg(W, b, sf, om[0], ls)
    sc = np.array([fg(c)[0] for c in cand])
    sel = sr.select_starts(sc, cand, 24, 0.05)
    assert sel.count == 24
    for tol in sr.TOLS:
        s = sr.sensitivity(fg, cand[sel.idx], sr.ASCENT_ITERS, tol, np.abs(sc).max())
        _report(f"rff {name} tol {tol:g}", s)
        assert s.flips == 0 and s.left_out <= 0.125 and sr.x_bound(s.dev).max() <= 1e-6
