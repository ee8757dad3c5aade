"""The references and bounds of tests/lu_ref.py against LAPACK, long double arithmetic and closed forms, on the CPU:
what tests/test_gpu_lu.py holds the device's LU to is shown to be sound here first."""
import numpy as np
import pytest
import scipy.linalg

import lu_ref as lr
from oracle import ppbo_oracle as orc

GAP = 1e-8          # no pivot decision of a test matrix may be closer than this: a different pivot is then never legitimate


def lapack(A):
    lu, piv = scipy.linalg.lu_factor(A)
    return lu, piv.astype(np.int64)


@pytest.mark.parametrize("n", [1, 2, 5, 16, 17, 100, 257])
def test_getf2_is_lapack_on_gaussian(n):
    A = lr.scaled_gaussian(n, n)
    lu, piv = lapack(A)
    mine, mypiv, info = lr.getf2(A)
    assert info == 0 and np.array_equal(mypiv, piv)
    assert lr.backward_ratio(A, mine, mypiv) <= 1.0
    assert lr.backward_ratio(A, lu, piv) <= 1.0
    ld, ldpiv, _ = lr.getf2(A, np.longdouble)
    assert np.array_equal(ldpiv, piv) and lr.backward_ratio(A, ld.astype(np.float64), ldpiv) <= 1.0


@pytest.mark.parametrize("n", [150, 700, 1100])
def test_getf2_is_lapack_on_ties(n):
    A, expect, _ = lr.tie_case(n)
    lu, piv = lapack(A)
    mine, mypiv, info = lr.getf2(A)
    assert info == 0 and np.array_equal(mypiv, piv)
    assert [(c, int(mypiv[c])) for c, _ in expect] == expect
    rows = lr.sample_rows(n)
    assert lr.backward_ratio(A, mine, mypiv, rows) <= 1.0
    assert lr.backward_ratio(A, lu, piv, rows) <= 1.0


@pytest.mark.parametrize("n,sizes", [(150, (2, 3, 17, 40)), (700, (2, 70, 129, 300))])
def test_drawn_ties_take_the_first_row(n, sizes):
    """tie_matrix with the tied rows and signs drawn: LAPACK and getf2 both take the first tied row."""
    A, expect, tied = lr.tie_matrix(n, sizes, np.random.default_rng(n))
    assert len(expect) == len(sizes) + 1 and all(want == min(rows) for (_, want), (_, rows) in zip(expect, tied))
    lu, piv = lapack(A)
    mine, mypiv, info = lr.getf2(A)
    assert info == 0 and np.array_equal(mypiv, piv)
    for col, want in expect:
        assert piv[col] == want and np.array_equal(mine[col, col:], A[want, col:])
    assert np.count_nonzero(A[np.tril_indices(n, -1)] == 0) >= sum(s * (n - sum(sizes[:i + 1])) for i, s in enumerate(sizes))


@pytest.mark.parametrize("n", sorted(lr.TIE_CASES))
def test_lapack_takes_the_first_tied_row(n):
    """On every tie matrix of the device test: the tie is exact and maximal when its column is reached, LAPACK takes the
    smallest tied row, and row col of U is that row of A bit for bit."""
    A, expect, tied = lr.tie_case(n)
    lu, piv = lapack(A)
    assert len(expect) == len(tied) >= 2
    for (col, want), (_, rows) in zip(expect, tied):
        assert want == min(rows) and piv[col] == want
        assert np.array_equal(lu[col, col:], A[want, col:])
        assert np.all(np.abs(A[list(rows), col]) == 1.5) and len({tuple(A[r, col + 1:]) for r in rows}) == len(rows)
        others = np.setdiff1d(np.arange(col, n), rows)
        assert np.all(np.abs(A[others, col]) <= 0.5)
    assert np.array_equal(lr.recover_rows(A, lu), lr.perm_of(piv))


def test_tie_cases_reach_every_class():
    """Every column of a panel, the first and the last panel, every panel kernel; tied rows in one wavefront, in two, in
    one thread of the two-row panel (t and t + 1024), and in the memory-resident panel one thread and > 1024 rows apart;
    ties of opposite sign."""
    feats, opposite = set(), False
    for n in lr.TIE_CASES:
        A, _, tied = lr.tie_case(n)
        for col, rows in tied:
            feats |= lr.tie_features(n, col, rows)
            opposite |= len(set(np.sign(A[list(rows), col]))) == 2
    want = {("J", j) for j in range(16)} | {"first_panel", "last_panel", "reg256", "reg512", "reg1024", "reg2048", "mem"}
    want |= {(c, w) for c in ("reg256", "reg512", "reg1024", "reg2048", "mem") for w in ("same_wave", "other_wave")}
    want |= {("reg2048", "same_thread"), ("mem", "same_thread"), ("mem", "far")}
    assert want <= feats, sorted(map(str, want - feats))
    assert opposite


@pytest.mark.parametrize("n", lr.ZERO_SIZES)
def test_getf2_info_is_lapack_on_zero_pivots(n):
    for cols in lr.zero_cases(n):
        A = lr.zero_pivot_matrix(n, cols, np.random.default_rng(n + cols[-1]))
        lu, piv, info = scipy.linalg.lapack.dgetrf(A)
        assert info == min(cols) + 1
        assert np.all(np.diag(lu)[list(cols)] == 0) and np.count_nonzero(np.diag(lu) == 0) == len(cols)
        if n <= 600 or len(cols) == 2:
            assert lr.backward_ratio(A, lu, piv, lr.sample_rows(n)) <= 1.0
        if n <= 600:
            mine, mypiv, myinfo = lr.getf2(A)
            assert myinfo == info and np.array_equal(mypiv, piv)
            assert np.all(np.diag(mine)[list(cols)] == 0)


def test_getf2_divides_by_a_subnormal_pivot():
    """The multipliers under a subnormal pivot are the exact quotients k / 8.  (No LAPACK beside it: the optimised
    libraries differ in what they do below the smallest normal number.)"""
    A, p = lr.tiny_pivot_matrix(100, 20, 30, np.random.default_rng(0))
    mine, mypiv, info = lr.getf2(A)
    assert info == 0 and mypiv[20] == p
    assert mine[20, 20] == A[p, 20] == -2.0 ** -1060 and abs(A[p, 20]) < lr.SFMIN
    with np.errstate(over="ignore"):
        assert np.isinf(1.0 / A[p, 20])
    perm = lr.perm_of(mypiv)
    mult = A[perm[21:50], 20] / A[p, 20]
    assert np.array_equal(mine[21:50, 20], mult) and np.array_equal(mult * 8, np.rint(mult * 8)) and np.abs(mult).max() < 1
    assert np.count_nonzero(mult) > 20 and np.all(mine[50:, 20] == 0)
    assert lr.backward_ratio(A, mine, mypiv) <= 1.0


def test_product_ld_is_a_long_double_product():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((37, 300)) * np.exp(6 * rng.standard_normal((37, 300)))
    B = rng.standard_normal((300, 41)) * np.exp(6 * rng.standard_normal((300, 41)))
    want = A.astype(np.longdouble) @ B.astype(np.longdouble)
    mag = np.abs(A) @ np.abs(B)
    assert np.abs(lr.product_ld(A, B) - want).max() <= (300 * 2.0 ** -63 * mag).max()
    assert np.all(np.abs(lr.product_ld(A, B) - want) <= 300 * 2.0 ** -63 * mag)


def test_backward_ratio_sees_one_wrong_entry():
    A = lr.scaled_gaussian(257, 3)
    lu, piv = lapack(A)
    assert lr.backward_ratio(A, lu, piv) <= 1.0
    bad = lu.copy()
    bad[200, 100] *= 1.0 + 1e-9                        # one multiplier off in the 9th digit
    assert lr.backward_ratio(A, bad, piv, [200]) > 1.0
    assert lr.backward_ratio(A, bad, piv, [199]) <= 1.0
    wrong = piv.copy()
    wrong[5], wrong[6] = piv[6], piv[5]
    assert lr.backward_ratio(A, lu, wrong) > 1.0


def test_recover_rows_is_the_permutation():
    for n, seed in ((1, 0), (33, 1), (300, 2)):
        A = lr.scaled_gaussian(n, seed)
        lu, piv = lapack(A)
        assert np.array_equal(lr.recover_rows(A, lu), lr.perm_of(piv))
        assert np.array_equal(lr.apply_piv(A, piv), A[lr.perm_of(piv)])
    with pytest.raises(AssertionError):
        lr.recover_rows(A, np.roll(lu, 1, axis=1))


@pytest.mark.parametrize("n", lr.GAUSS_SIZES)
def test_gaussian_cases_have_no_near_tie(n, capsys):
    """The matrices of the device's pivot-sequence test: smallest relative pivot gap >= 1e-8, and LAPACK's own figures."""
    A = lr.scaled_gaussian(n, n)
    lu, piv = lapack(A)
    gap = lr.pivot_gap(lu)
    ratio = lr.backward_ratio(A, lu, piv, lr.sample_rows(n))
    with capsys.disabled():
        print(f"\nLUFIG host gaussian N={n} gap={gap:.3g} lapack_backward_ratio={ratio:.3g}", end="")
    assert gap >= GAP
    assert ratio <= 1.0
    if n <= 513:
        ld, ldpiv, _ = lr.getf2(A, np.longdouble)
        assert np.array_equal(ldpiv, piv)
        err = abs(float(lr.u_slogdet(lu)[1] - lr.u_slogdet(ld)[1]))
        bound = lr.logdet_bound(A, lu, piv)
        with capsys.disabled():
            print(f" lapack_logdet_err/bound={err / bound:.3g} (bound {bound:.3g})", end="")
        assert err <= bound and lr.u_slogdet(lu)[0] == lr.u_slogdet(ld)[0]


def test_pivot_gap_is_the_gap():
    A = np.array([[1.0, 2.0, 0.0], [4.0, 1.0, 1.0], [3.0, 5.0, 2.0]])
    lu, piv = lapack(A)
    # step 0: 4 against 3 -> 1/4; step 1: rows (1.75, -.25) and (4.25, 1.25) -> 1 - 1.75 / 4.25
    assert np.isclose(lr.pivot_gap(lu), 0.25)
    A[2, 0] = 4.0 * (1 - 1e-9)
    assert np.isclose(lr.pivot_gap(lapack(A)[0]), 1e-9, rtol=1e-6)


# ------------------------------------------------------------------------------------------------------ I + Sigma Lambda
def test_star_lambda_dense_is_the_oracles():
    rng = np.random.default_rng(0)
    for n_q, m in ((1, 1), (3, 2), (4, 25)):
        f = rng.standard_normal(n_q * (m + 1))
        d, o = orc.lambda_compact(f, m, 0.3)
        assert np.array_equal(lr.star_lambda_dense(d, o, m), orc.lambda_dense(f, m, 0.3))
        o2 = o.copy()
        o2[:: m + 1] = 9.0
        assert np.array_equal(lr.star_lambda_dense(d, o2, m), orc.lambda_dense(f, m, 0.3))
    lam = lr.star_lambda_dense([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [0, 7.0, 8.0, 0, 9.0, 10.0], 2)
    want = np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    want[0, 1] = want[1, 0] = 7.0
    want[0, 2] = want[2, 0] = 8.0
    want[3, 4] = want[4, 3] = 9.0
    want[3, 5] = want[5, 3] = 10.0
    assert np.array_equal(lam, want)


@pytest.mark.parametrize("seed", [2, 3])
def test_exact_case_reference(seed, capsys):
    d, f = lr.exact_case(seed=seed)
    M = np.eye(d.size) + lr.star_lambda_dense(d, f, 25)
    assert np.array_equal(M, lr.ipsl_dense(np.eye(d.size), d, f, 25)) and np.array_equal(M, np.rint(M))
    lu, piv = lapack(M)
    ld, ldpiv, info = lr.getf2(M, np.longdouble)
    assert info == 0 and np.array_equal(piv, ldpiv) and lr.pivot_gap(lu) >= GAP
    assert np.count_nonzero(piv != np.arange(d.size)) >= 10
    err, bound = abs(float(lr.u_slogdet(lu)[1] - lr.u_slogdet(ld)[1])), lr.logdet_bound(M, lu, piv)
    with capsys.disabled():
        print(f"\nLUFIG host exact seed={seed} lapack_logdet_err/bound={err / bound:.3g} (bound {bound:.3g})", end="")
    assert err <= bound and lr.u_slogdet(lu)[0] == lr.u_slogdet(ld)[0]


@pytest.mark.parametrize("m", lr.ONE_HOT_M)
def test_one_hot_closed_forms(m, capsys):
    """det(I + S Lambda) of a one-entry Lambda in closed form against the dense determinant: LAPACK's within logdet_bound
    for every case, long double elimination where that is cheap."""
    S = lr.one_hot_sigma(m)
    n = S.shape[0]
    assert n == lr.ONE_HOT_NQ * (m + 1) and n % 256 != 0 and not np.allclose(S, S.T)
    worst = 0.0
    for name, d, f, closed in lr.one_hot_cases(m):
        det = closed(S.astype(np.longdouble))
        M = lr.ipsl_dense(S, d, f, m)
        lu, piv = lapack(M)
        assert lr.pivot_gap(lu) >= GAP, name
        sgn, ld = lr.u_slogdet(lu)
        bound = lr.logdet_bound(M, lu, piv)
        assert sgn * lr.piv_sign(piv) == np.sign(det), name
        err = abs(float(ld - np.log(np.abs(det))))
        assert err <= bound, (name, err, bound)
        worst = max(worst, err / bound)
        if n <= 182:
            Sl, lam = S.astype(np.longdouble), lr.star_lambda_dense(d, f, m).astype(np.longdouble)
            full, fpiv, _ = lr.getf2(np.eye(n, dtype=np.longdouble) + Sl @ lam, np.longdouble)
            s2, l2 = lr.u_slogdet(full)
            assert s2 * lr.piv_sign(fpiv) == np.sign(det), name
            assert abs(l2 - np.log(np.abs(det))) <= 64 * n * 2.0 ** -64 * max(1.0, abs(l2)) + bound * 2.0 ** -10, name
        if name.startswith("off_on_obs"):
            assert det == 1 and np.array_equal(M, np.eye(n))
        else:
            assert abs(det - 1) > 1e-3, name
    with capsys.disabled():
        print(f"\nLUFIG host one_hot m={m} N={n} lapack_logdet_err/bound={worst:.3g}", end="")


@pytest.mark.parametrize("case", lr.REAL_CASES, ids=lambda c: f"{c[2][:2]}-{c[0]}x{c[1]}-{c[3]}")
def test_real_cases_lapack_within_logdet_bound(case, capsys):
    Sigma, d, o = lr.real_case(*case)
    m = case[1]
    M = lr.ipsl_dense(Sigma, d, o, m)
    lu, piv = lapack(M)
    ld, ldpiv, info = lr.getf2(M, np.longdouble)
    assert info == 0 and np.array_equal(piv, ldpiv) and lr.pivot_gap(lu) >= GAP
    if case[3] < 0.01:
        assert np.count_nonzero(d == 0) > 10 and np.count_nonzero(d) > 10     # some weights underflow, not all
    else:
        assert np.all(d != 0)
    err, bound = abs(float(lr.u_slogdet(lu)[1] - lr.u_slogdet(ld)[1])), lr.logdet_bound(M, lu, piv)
    with capsys.disabled():
        print(f"\nLUFIG host real {case} N={M.shape[0]} lapack_logdet_err/bound={err / bound:.3g} (bound {bound:.3g})",
              end="")
    assert err <= bound and lr.u_slogdet(lu)[0] == lr.u_slogdet(ld)[0]
