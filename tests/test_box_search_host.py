"""CPU: the NumPy reference of the searches inside boxes (tests/box_search_numpy.py) is right and stable -- the boxed
ascent is search_ref.bb_ascent in the unit box state for state, it honours a box on closed forms, and on the start sets
tests/test_gpu_box_search.py uses it holds the project's limits against its own 1e-13-perturbed self (no branch flips
among the kept pairs, at most 1/8 of the pairs left out, a bound on x of at most 1e-6)."""
import os
import re

import numpy as np
import pytest

import box_search_numpy as bx
import search_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES = {}


def _case(name):
    """(fg, starts, mu_scale, D) of a mean case: the weights of test_search_ref_host.py (unit normal for the tall designs,
    whose host fit takes over a minute; the GPU test measures again on its device-fitted weights)."""
    if name not in _CASES:
        X, th, kernel, m = sr.mean_case(name)
        D = X.shape[1]
        if name.endswith("_tall"):
            alpha = np.random.default_rng(D).standard_normal(X.shape[0])
        else:
            f0, Sinv0 = sr.host_fit(X, th, kernel, m, D)
            alpha = Sinv0 @ f0
        fg = sr.mean_fg(X, th, kernel, alpha)
        starts = sr.ascent_starts(D, 7, fg)
        mu0 = np.array([fg(np.clip(s, 0, 1))[0] for s in starts])
        _CASES[name] = (fg, starts, float(np.abs(mu0).max()), D)
    return _CASES[name]


@pytest.mark.parametrize("box,tol", bx.CONFIGS)
@pytest.mark.parametrize("name", list(sr.MEAN_CASES))
def test_boxed_reference_is_stable_on_its_starts(name, box, tol):
    fg, starts, scale, D = _case(name)
    lo, hi = bx.boxes(D)[box]
    s = bx.sensitivity_box(fg, starts, lo, hi, sr.ASCENT_ITERS, tol, scale)
    print(f"{name} / {box} tol {tol:g}: largest |x - x'| per n {np.array2string(s.dev, precision=1)}, flips {s.flips}, "
          f"left out {s.left_out:.3f}, it at n = {sr.ASCENT_ITERS}: {np.bincount(s.its[:, -1], minlength=sr.ASCENT_ITERS + 1)}")
    assert s.flips == 0
    assert s.left_out <= 0.125
    assert sr.x_bound(s.dev).max() <= 1e-6
    assert np.all((s.xs >= lo) & (s.xs <= hi))
    if tol > 1e-3 and box == "unit":
        assert np.isin(s.its[:, -1], (1, 2)).any()           # the large tolerance does stop some starts early


@pytest.mark.parametrize("tol", sr.TOLS)
@pytest.mark.parametrize("name", ["se_d3", "rq_d10", "ard_se_d5", "camphor_ard"])
def test_unit_box_is_bb_ascent_state_for_state(name, tol):
    fg, starts, scale, D = _case(name)
    lo, hi = bx.boxes(D)["unit"]
    for s0 in starts:
        a, b = sr.bb_ascent(fg, s0, sr.ASCENT_ITERS, tol, scale), bx.bb_ascent_box(fg, s0, lo, hi, sr.ASCENT_ITERS, tol, scale)
        assert np.array_equal(a.xs, b.xs) and np.array_equal(a.mus, b.mus) and np.array_equal(a.its, b.its)
        assert np.array_equal(a.margins, b.margins) and a.it == b.it and a.mu == b.mu


def test_boxes_are_the_five_of_the_issue():
    for D in (3, 6, 20):
        b = bx.boxes(D)
        assert tuple(b) == bx.BOX_NAMES
        rng = np.random.default_rng(5 + D)
        v = 0.1 + 0.8 * rng.random(D)
        fixed = np.arange(D) % 3 == 1
        lo, hi = b["fixed3"]
        assert np.array_equal(lo[fixed], v[fixed]) and np.array_equal(hi[fixed], v[fixed])
        assert np.all(lo[~fixed] == 0.0) and np.all(hi[~fixed] == 1.0)
        assert b["slab"][0][0] == 0.5 and b["slab"][1][0] == 0.5 + 2.0 ** -10
        rlo = 0.6 * rng.random(D)
        assert np.array_equal(b["ragged"][0], rlo) and np.array_equal(b["ragged"][1], rlo + 0.05 + 0.35 * rng.random(D))
        for lo, hi in b.values():
            assert np.all((0.0 <= lo) & (lo <= hi) & (hi <= 1.0))


def test_box_on_closed_forms():
    c = np.array([0.9, 0.4, 0.3])
    fg = lambda x: (-0.5 * float((x - c) @ (x - c)), -(x - c))              # noqa: E731
    lo, hi = np.array([0.2, 0.25, 0.6]), np.array([0.7, 0.25, 0.8])
    r = bx.bb_ascent_box(fg, np.array([0.0, 0.9, 0.7]), lo, hi, 30, 1e-9)
    # the maximiser of the box: the face 0.7, the fixed 0.25, the face 0.6
    assert np.array_equal(r.x, [0.7, 0.25, 0.6]) and np.all(r.xs[:, 1] == 0.25)
    assert np.array_equal(r.xs[0], [0.2, 0.25, 0.7])                        # the start is clipped before anything is evaluated
    assert np.all(bx.project_box(r.x, fg(r.x)[1], lo, hi) == 0.0) and r.it < 30
    # the first move is 0.02 of the longest side (0.5), along the unprojected gradient's norm
    g0 = fg(r.xs[0])[1]
    pg0 = bx.project_box(r.xs[0], g0, lo, hi)
    assert np.allclose(r.xs[1] - r.xs[0], 0.02 * 0.5 / np.sqrt((g0 * g0).sum()) * pg0, rtol=1e-12, atol=0)
    # a box of one point: the point, the mean there, no iteration
    p = np.array([0.3, 0.6, 0.1])
    r = bx.bb_ascent_box(fg, np.array([0.9, 0.9, 0.9]), p, p, 10, 0.0)
    assert np.array_equal(r.x, p) and r.it == 0 and r.mu == fg(p)[0] and np.all(r.its == 0)


def test_some_starts_stop_after_a_move_or_two_at_the_large_tolerance():
    for name in ("se_d3", "camphor"):
        fg, starts, scale, D = _case(name)
        for box in ("unit", "fixed3", "slab"):
            lo, hi = bx.boxes(D)[box]
            its = bx.ascend_all_box(fg, starts, lo, hi, sr.ASCENT_ITERS, 1e-2, scale)[2][:, -1]
            assert (its <= 2).any(), (name, box, its)


def test_box_rows():
    rng = np.random.default_rng(3)
    pool, shifts = rng.random((10, 3)), rng.random((2, 3))
    unit = (np.zeros(3), np.ones(3))
    for t in range(2):
        assert np.array_equal(bx.box_rows(pool, shifts[t], *unit), sr.trial_rows(pool, shifts, t)[0])
    assert np.array_equal(bx.box_rows(pool, None, *unit), pool)
    lo, hi = np.array([0.25, 0.5, 0.0]), np.array([0.75, 0.5, 1.0])
    seeds = np.array([[0.0, 0.9, 0.3], [0.5, 0.1, 1.5]])
    rows = bx.box_rows(pool, shifts[0], lo, hi, seeds)
    assert rows.shape == (12, 3) and np.all((rows >= lo) & (rows <= hi)) and np.all(rows[:, 1] == 0.5)
    assert np.array_equal(rows[10:], [[0.25, 0.5, 0.3], [0.5, 0.5, 1.0]])
    u = (pool + shifts[0]) - np.floor(pool + shifts[0])
    assert np.array_equal(rows[:10, 0], 0.25 + 0.5 * u[:, 0]) and np.array_equal(rows[:10, 2], u[:, 2])


def test_header_declares_both_entries_at_abi_8():
    h = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"#define\s+PPBO_ABI_VERSION\s+9\b", h)
    for name in ("ppbo_mean_ascent_boxes", "ppbo_mean_search_boxes"):
        assert re.search(r"PPBO_API\s+int\s+" + name + r"\s*\(", h), name
    from ppbo_amd import _lib
    assert _lib.ABI_VERSION == 9
    assert len(_lib.SIGNATURES["ppbo_mean_ascent_boxes"]) == 13 and len(_lib.SIGNATURES["ppbo_mean_search_boxes"]) == 18
