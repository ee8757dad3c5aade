"""CPU: every closed-form ingredient of tests/marginals_numpy.py (the statement ppbo_predict_marginals is held to) against
tensor Gauss-Legendre quadrature of the NumPy kernel itself, the camphor factors against the oracle's kernel, the Python
refusals and the canonical form of a call's rows.  No device.

Settings of the quadrature (not to be loosened: l below 0.2 needs more nodes): SE-ARD l = (0.2, 0.45, 1.3) at D = 3 with
40 nodes per axis, the periodic factor at l = 0.26 with 200 nodes.  Bound 1e-12 relative."""
import itertools
import os
import re

import numpy as np
import pytest

import marginals_numpy as mn
from oracle import ppbo_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-12
L3 = np.array([0.2, 0.45, 1.3])
PER3 = np.zeros(3, dtype=int)
SF2 = 0.7 ** 2


def gauss_legendre(n):
    """Nodes and weights on [0, 1]."""
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


# ---------------------------------------------------------------- 1. the per-axis integrals
@pytest.mark.parametrize("l,periodic,n", [(0.2, 0, 40), (0.45, 0, 40), (1.3, 0, 40), (0.26, 1, 200), (0.31, 1, 200), (1.0, 1, 200)])
def test_axis_integrals(l, periodic, n):
    x, w = gauss_legendre(n)
    c = np.array([0.0, 0.013, 0.37, 0.5, 0.81, 1.0])
    I_q = (w[:, None] * mn.factor(x[:, None] - c[None, :], l, periodic)).sum(axis=0)
    I = mn.axis_integral(c, l, periodic)
    A_q = w @ mn.factor(x[:, None] - x[None, :], l, periodic) @ w
    A = mn.axis_double_integral(l, periodic)
    e_I, e_A = np.max(np.abs(I - I_q) / I_q), abs(A - A_q) / A_q
    print(f"axis integrals l={l} periodic={periodic}: I {e_I:.1e}, A {e_A:.1e}")
    assert e_I <= BOUND and e_A <= BOUND


def test_scaled_bessel_is_not_a_product_of_two_factors():
    """At l = 0.03 (a = 1111) exp(-a) underflows against I0(a) overflowing; ive stays finite and matches quadrature."""
    l = 0.03
    x, w = gauss_legendre(400)
    I_q = w @ mn.factor(x - 0.3, l, 1)
    assert np.isfinite(mn.axis_double_integral(l, 1)) and abs(mn.axis_double_integral(l, 1) - I_q) <= 1e-10 * I_q


# ---------------------------------------------------------------- 2. the three columns, orders 0, 1, 2
def _raw_column_by_quadrature(kept, X, l, periodic, n):
    """int k((t_J, u), x_j) du over the axes that are not kept: the full tensor grid through product_kernel itself."""
    D = X.shape[1]
    x, w = gauss_legendre(n)
    free = [d for d in range(D) if d not in kept]
    grids = np.meshgrid(*[x for _ in free], indexing="ij") if free else []
    wts = np.ones(1)
    for _ in free:
        wts = np.multiply.outer(wts, w)
    pts = np.zeros((max(1, x.size ** len(free)), D))
    for k, d in enumerate(free):
        pts[:, d] = grids[k].reshape(-1)
    for d, tv in kept.items():
        pts[:, d] = tv
    return wts.reshape(-1) @ mn.product_kernel(pts, X, l, periodic, SF2)


def _columns_by_quadrature(row, tv, X, l, periodic, n):
    kept = {d: tv[k] for k, d in enumerate(row) if d >= 0}
    raw = _raw_column_by_quadrature(kept, X, l, periodic, n)
    zero = _raw_column_by_quadrature({}, X, l, periodic, n)
    out = {mn.RAW: raw, mn.CENTRED: raw - zero}
    if len(kept) == 2:
        (d, td), (e, te) = kept.items()
        out[mn.INTERACTION] = (raw - _raw_column_by_quadrature({d: td}, X, l, periodic, n)
                               - _raw_column_by_quadrature({e: te}, X, l, periodic, n) + zero)
    return out


def test_columns_against_tensor_quadrature():
    rng = np.random.default_rng(0)
    X = rng.random((7, 3))
    X[0] = [0.0, 1.0, 0.5]
    worst = {}
    for row, tv in (((-1, -1), (0.0, 0.0)), ((0, -1), (0.3, 0.0)), ((2, -1), (1.0, 0.0)), ((1, -1), (0.0, 0.0)),
                    ((0, 1), (0.2, 0.9)), ((0, 2), (0.0, 1.0)), ((1, 2), (0.55, 0.41))):
        ref = _columns_by_quadrature(row, tv, X, L3, PER3, 40)
        for effect, cq in ref.items():
            c = mn.marginal_column(np.array([row]), np.array([tv]), X, L3, PER3, SF2, effect)[0]
            scale = np.abs(ref[mn.RAW]).max()
            e = np.abs(c - cq).max() / scale
            worst[(effect, sum(d >= 0 for d in row))] = max(worst.get((effect, sum(d >= 0 for d in row)), 0.0), e)
    print("columns against quadrature (effect, order): " + ", ".join(f"{k}: {v:.1e}" for k, v in sorted(worst.items())))
    assert max(worst.values()) <= BOUND
    # an order-0 row under CENTRED is the zero functional
    assert np.all(mn.marginal_column(np.array([[-1, -1]]), np.zeros((1, 2)), X, L3, PER3, SF2, mn.CENTRED) == 0.0)


def test_periodic_column_against_quadrature():
    """A periodic axis beside an SE one (l = 0.26, 0.45) and two periodic ones (l = 0.26, 0.31) at D = 2, 200 nodes per
    averaged axis; the scale of a row is the larger of its RAW column and the order-0 column it is centred by."""
    X = np.random.default_rng(1).random((5, 2))
    worst = 0.0
    for l, per in ((np.array([0.26, 0.45]), np.array([1, 0])), (np.array([0.26, 0.31]), np.array([1, 1]))):
        for row, tv in (((-1, -1), (0.0, 0.0)), ((0, -1), (0.7, 0.0)), ((1, -1), (0.15, 0.0)), ((0, 1), (0.4, 0.6))):
            ref = _columns_by_quadrature(row, tv, X, l, per, 200)
            scale = max(np.abs(ref[mn.RAW]).max(), np.abs(ref[mn.RAW] - ref[mn.CENTRED]).max())
            for effect, cq in ref.items():
                c = mn.marginal_column(np.array([row]), np.array([tv]), X, l, per, SF2, effect)[0]
                worst = max(worst, np.abs(c - cq).max() / scale)
    print(f"columns with periodic axes against quadrature: {worst:.1e}")
    assert worst <= BOUND


# ---------------------------------------------------------------- 3. the three prior terms
def _measures(row, tv, effect, D):
    """The functional of a row as signed RAW marginals: [(sign, {axis: value})]."""
    kept = {d: tv[k] for k, d in enumerate(row) if d >= 0}
    if effect == mn.RAW:
        return [(1.0, kept)]
    if effect == mn.CENTRED:
        return [(1.0, kept), (-1.0, {})]
    (d, td), (e, te) = kept.items()
    return [(1.0, kept), (-1.0, {d: td}), (-1.0, {e: te}), (1.0, {})]


def _cov_factorised(ka, kb, l, periodic, n):
    """Cov(f_Ja(ta), f_Jb(tb)) under the prior: the tensor Gauss-Legendre sum over both arguments.  Nodes, weights and
    the kernel are all products over the axes, so the sum factorises exactly into one small sum per axis."""
    x, w = gauss_legendre(n)
    out = SF2
    for d in range(len(l)):
        na, wa = (np.array([ka[d]]), np.ones(1)) if d in ka else (x, w)
        nb, wb = (np.array([kb[d]]), np.ones(1)) if d in kb else (x, w)
        out *= wa @ mn.factor(na[:, None] - nb[None, :], l[d], periodic[d]) @ wb
    return out


def _cov_full_tensor(ka, kb, l, periodic, n):
    """The same sum with nothing factorised: both tensor grids through product_kernel (small D and n only)."""
    x, w = gauss_legendre(n)

    def grid(k):
        free = [d for d in range(len(l)) if d not in k]
        pts = np.zeros((x.size ** len(free), len(l)))
        wt = np.ones(1)
        for i, d in enumerate(free):
            pts[:, d] = np.meshgrid(*[x for _ in free], indexing="ij")[i].reshape(-1)
            wt = np.multiply.outer(wt, w)
        for d, tv in k.items():
            pts[:, d] = tv
        return pts, wt.reshape(-1)

    (pa, wa), (pb, wb) = grid(ka), grid(kb)
    return wa @ mn.product_kernel(pa, pb, l, periodic, SF2) @ wb


def _prior_by_quadrature(row, tv, effect, l, periodic, n, cov):
    ms = _measures(row, tv, effect, len(l))
    return sum(sa * sb * cov(ka, kb, l, periodic, n) for (sa, ka), (sb, kb) in itertools.product(ms, ms))


ROWS = (((-1, -1), (0.0, 0.0)), ((0, -1), (0.3, 0.0)), ((2, -1), (1.0, 0.0)), ((0, 1), (0.2, 0.9)), ((0, 2), (0.0, 1.0)),
        ((1, 2), (0.55, 0.41)))


def test_priors_against_tensor_quadrature():
    worst = 0.0
    for row, tv in ROWS:
        for effect in (mn.RAW, mn.CENTRED, mn.INTERACTION):
            if effect == mn.INTERACTION and row[1] < 0:
                continue
            pr = mn.marginal_prior(np.array([row]), np.array([tv]), L3, PER3, SF2, effect)[0]
            pq = _prior_by_quadrature(row, tv, effect, L3, PER3, 40, _cov_factorised)
            scale = _cov_factorised({d: tv[k] for k, d in enumerate(row) if d >= 0}, {d: tv[k] for k, d in enumerate(row) if d >= 0},
                                    L3, PER3, 40)
            worst = max(worst, abs(pr - pq) / scale)
    print(f"prior terms against quadrature, relative to the RAW prior of the row: {worst:.1e}")
    assert worst <= BOUND
    assert mn.marginal_prior(np.array([[-1, -1]]), np.zeros((1, 2)), L3, PER3, SF2, mn.CENTRED)[0] == 0.0


def test_factorised_quadrature_is_the_full_tensor_sum():
    """At D = 2, 12 nodes: the factorised sum against both grids through product_kernel, every pair of measures."""
    l, per = np.array([0.45, 1.3]), np.array([0, 1])
    for ka, kb in itertools.product(({}, {0: 0.3}, {1: 0.8}, {0: 0.1, 1: 0.6}), repeat=2):
        a, b = _cov_factorised(ka, kb, l, per, 12), _cov_full_tensor(ka, kb, l, per, 12)
        assert abs(a - b) <= 1e-14 * abs(b)


def test_covariance_of_a_column_is_its_prior():
    """var = prior - c' A c needs prior = Cov(L f, L f) and c_j = Cov(L f, f(x_j)): the column at a design row placed ON the
    kept axes' values, averaged as the row averages, is the prior (RAW, order 2 at D = 2: the kernel itself)."""
    l, per = np.array([0.45, 1.3]), np.zeros(2, dtype=int)
    pt = np.array([[0.2, 0.7]])
    c = mn.marginal_column(np.array([[0, 1]]), pt, pt, l, per, SF2, mn.RAW)[0, 0]
    assert abs(c - SF2) <= 1e-15 and abs(mn.marginal_prior(np.array([[0, 1]]), pt, l, per, SF2, mn.RAW)[0] - SF2) <= 1e-15


# ---------------------------------------------------------------- 4. the camphor factors are the oracle's kernel
def test_camphor_factors_against_the_oracle():
    rng = np.random.default_rng(2)
    theta = [0.001, 0.26, 0.1]
    l, per = mn.axes_of(theta, mn.CAMPHOR, 6)
    Xa, Xb = rng.random((40, 6)), rng.random((30, 6))
    k0 = orc.camphor_copper_kernel(Xa, Xb, theta)
    assert np.abs(mn.product_kernel(Xa, Xb, l, per, theta[2] ** 2) - k0).max() <= 1e-14 * theta[2] ** 2
    # axis pairs: points that differ in two coordinates only
    base = rng.random(6)
    for d, e in itertools.combinations(range(6), 2):
        a, b = np.tile(base, (9, 1)), base.reshape(1, 6)
        a[:, d], a[:, e] = rng.random(9), rng.random(9)
        ref = orc.camphor_copper_kernel(a, b, theta)[:, 0]
        mine = theta[2] ** 2 * mn.factor(a[:, d] - base[d], l[d], per[d]) * mn.factor(a[:, e] - base[e], l[e], per[e])
        assert np.abs(mine - ref).max() <= 1e-14 * theta[2] ** 2, (d, e)
    # SE, scalar and per-dimension length scales, through the statement the other entries are held to
    import pairs_numpy as pn
    for th in ([0.05, 0.3, 0.7], [0.05, np.array([0.2, 0.45, 1.3, 0.6]), 0.7]):
        l, per = mn.axes_of(th, "SE_kernel", 4)
        A, B = rng.random((20, 4)), rng.random((10, 4))
        assert np.abs(mn.product_kernel(A, B, l, per, 0.49) - pn.cross(A, B, th, "SE_kernel")).max() <= 1e-14


# ---------------------------------------------------------------- 5. Python refusals, canonical rows, the binding
def test_python_refusals():
    from ppbo_amd.engine import EFFECT_CENTRED, EFFECT_INTERACTION, marginal_axis_params, marginal_rows
    for kernel in ("RQ_kernel", "Matern52_kernel", "Matern32_kernel"):
        with pytest.raises(ValueError, match="average_pred"):
            marginal_axis_params(kernel, (0.05, 0.3, 0.7), 4)
    with pytest.raises(ValueError, match="length scales"):
        marginal_axis_params("SE_kernel", (0.05, 0.3, 0.7), 65)
    l, per, i0 = marginal_axis_params("camphor_copper_kernel", (0.001, 0.26, 0.1), 6)
    assert np.allclose(l, [0.26, 0.26, 0.31, 0.26, 0.26, 0.26]) and list(per) == [1, 1, 0, 1, 1, 1]
    assert np.array_equal(i0, [mn.axis_integral(0.0, v, 1) for v in l])
    l, per, _ = marginal_axis_params("SE_kernel", (0.05, (0.2, 0.4), 0.7), 2, scale=np.array([5.0, 2.5]))
    assert np.allclose(l, [0.2, 0.4]) and not per.any()
    l, per, _ = marginal_axis_params("camphor_copper_ard_kernel", None, 11, camphor=np.arange(1.0, 7.0))
    assert np.array_equal(l, np.arange(1.0, 7.0)) and list(per) == [1, 1, 0, 1, 1, 1]
    for dims, t, eff in (([[4, -1]], [[0.1, 0.0]], EFFECT_CENTRED), ([[-2, -1]], [[0.1, 0.0]], EFFECT_CENTRED),
                         ([[1, 1]], [[0.1, 0.2]], EFFECT_CENTRED), ([[-1, 2]], [[0.1, 0.2]], EFFECT_CENTRED),
                         ([[1, -1]], [[0.1, 0.2]], EFFECT_INTERACTION), ([[-1, -1]], [[0.1, 0.2]], EFFECT_INTERACTION),
                         ([[0, 1, 2]], [[0.1, 0.2, 0.3]], EFFECT_CENTRED), ([[0, 1]], [[0.1]], EFFECT_CENTRED),
                         ([[0.5, 1]], [[0.1, 0.2]], EFFECT_CENTRED)):
        with pytest.raises(ValueError, match="predict_marginals"):
            marginal_rows(dims, t, 4, eff)


def test_rows_are_canonical_whatever_order_the_caller_gave():
    from ppbo_amd.engine import EFFECT_CENTRED, marginal_rows
    a = marginal_rows([[3, 1], [0, 2], [2, -1], [-1, -1]], [[0.3, 0.1], [0.5, 0.6], [0.2, 9.0], [7.0, 8.0]], 4, EFFECT_CENTRED)
    b = marginal_rows([[1, 3], [2, 0], [2, -1], [-1, -1]], [[0.1, 0.3], [0.6, 0.5], [0.2, 0.0], [0.0, 0.0]], 4, EFFECT_CENTRED)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].dtype == np.int32 and np.array_equal(a[0], [[1, 3], [0, 2], [2, -1], [-1, -1]])
    one = marginal_rows([2, 0, 1], [0.1, 0.2, 0.3], 4, EFFECT_CENTRED)          # [M]: one axis per row
    assert np.array_equal(one[0], [[2, -1], [0, -1], [1, -1]]) and np.array_equal(one[1][:, 0], [0.1, 0.2, 0.3])
    # ... whatever M is: two entries are TWO order-1 rows, never one order-2 row; that one is [[d, e]]
    two = marginal_rows([0, 1], [0.3, 0.4], 4, EFFECT_CENTRED)
    assert np.array_equal(two[0], [[0, -1], [1, -1]]) and np.array_equal(two[1], [[0.3, 0.0], [0.4, 0.0]])
    same = marginal_rows(np.full(2, 3), [0.0, 1.0], 4, EFFECT_CENTRED)          # main_effect on a two-point grid
    assert np.array_equal(same[0], [[3, -1], [3, -1]]) and np.array_equal(same[1][:, 0], [0.0, 1.0])
    col = marginal_rows(np.full((2, 1), 3), [[0.0], [1.0]], 4, EFFECT_CENTRED)
    assert np.array_equal(col[0], same[0]) and np.array_equal(col[1], same[1])
    pair = marginal_rows([[0, 1]], [[0.3, 0.4]], 4, EFFECT_CENTRED)
    assert np.array_equal(pair[0], [[0, 1]]) and np.array_equal(pair[1], [[0.3, 0.4]])
    single = marginal_rows([2], [0.5], 4, EFFECT_CENTRED)
    assert np.array_equal(single[0], [[2, -1]]) and np.array_equal(marginal_rows(2, 0.5, 4, EFFECT_CENTRED)[0], single[0])
    from ppbo_amd.engine import EFFECT_INTERACTION
    with pytest.raises(ValueError, match="two axes"):                           # [d, e] is two order-1 rows: no interaction
        marginal_rows([0, 1], [0.3, 0.4], 4, EFFECT_INTERACTION)
    with pytest.raises(ValueError, match="shape"):
        marginal_rows([0, 1], [[0.3, 0.4]], 4, EFFECT_CENTRED)


def test_main_effect_passes_one_axis_per_row_on_any_grid():
    """GPModel.main_effect and interaction_effect hand over [T, 1] / [T, 2] rows: a two-point grid stays two rows."""
    from ppbo_amd.gp_model import GPModel
    seen = []

    class Stub(GPModel):
        def marginal_pred(self, dims, t, effect="centred"):
            from ppbo_amd.engine import EFFECTS, marginal_rows
            d, tt = marginal_rows(dims, t, 4, EFFECTS[effect])
            seen.append((d, tt))
            return (np.zeros(len(d)),) * 3

    gp = Stub.__new__(Stub)
    for grid in ([0.0, 1.0], [0.5], np.linspace(0.0, 1.0, 5)):
        g, mu, _, _ = gp.main_effect(3, grid)
        d, tt = seen[-1]
        assert mu.shape == (len(grid),) and np.array_equal(d, np.tile([3, -1], (len(grid), 1))) and np.array_equal(tt[:, 0], g)
    out = gp.interaction_effect(1, 2, [0.0, 1.0], [0.25])
    d, tt = seen[-1]
    assert out[0].shape == (2, 1) and np.array_equal(d, [[1, 2], [1, 2]]) and np.array_equal(tt, [[0.0, 0.25], [1.0, 0.25]])
    # the statement itself is symmetric in the order
    X = np.random.default_rng(3).random((6, 4))
    l, per = np.array([0.2, 0.45, 1.3, 0.6]), np.zeros(4, dtype=int)
    for eff in (mn.RAW, mn.CENTRED, mn.INTERACTION):
        c1 = mn.marginal_column([[3, 1]], [[0.3, 0.1]], X, l, per, 1.0, eff)
        c2 = mn.marginal_column([[1, 3]], [[0.1, 0.3]], X, l, per, 1.0, eff)
        assert np.allclose(c1, c2, rtol=0, atol=1e-16)


def test_binding_and_header():
    from ppbo_amd import _lib
    assert "ppbo_predict_marginals" in _lib.SIGNATURES and len(_lib.SIGNATURES["ppbo_predict_marginals"]) == 15
    assert (_lib.EFFECT_RAW, _lib.EFFECT_CENTRED, _lib.EFFECT_INTERACTION) == (0, 1, 2)
    txt = open(os.path.join(ROOT, "include", "ppbo_hip.h")).read()
    assert re.search(r"PPBO_EFFECT_RAW = 0, PPBO_EFFECT_CENTRED = 1, PPBO_EFFECT_INTERACTION = 2", txt)
    assert "typedef struct ppbo_marginal_axes" in txt and "DOES NOT CHECK" in txt
    assert re.search(r"#define PPBO_ABI_VERSION 9\b", txt)
    fields = [f[0] for f in _lib.MarginalAxes._fields_]
    assert fields == ["Dc", "d_Xu", "h_l", "h_periodic", "h_I0"]
