"""The LU behind the evidence (ppbo_amd/csrc/lu.hip) on the device, through Engine.lu_slogdet_ and Engine.laplace_logdet:
pivot ties, the whole pivot sequence and the componentwise backward error on every panel path, zero and subnormal
pivots, row strides, and the matrix I + Sigma Lambda itself.  The references and bounds are tests/lu_ref.py's, shown to be
sound on the CPU by tests/test_lu_ref_host.py.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest
import scipy.linalg

import lu_ref as lr

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU; the HIP path has no CPU fallback")
    from ppbo_amd.engine import get_engine
    return get_engine(0)


def host(t):
    return t.detach().cpu().numpy()


def factor(eng, A, pad=0):
    """(sign, logdet, info, packed) of the device's in-place LU of A, run on a view of row stride N + pad whose padding
    must come back untouched."""
    n = A.shape[0]
    buf = np.full((n, n + pad), SENTINEL)
    buf[:, :n] = A
    d = eng.dev(buf)
    view = d[:, :n]
    assert view.stride(0) == n + pad and view.data_ptr() == d.data_ptr()
    sgn, ld, info = eng.lu_slogdet_(view)
    out = host(d)
    assert np.all(out[:, n:] == SENTINEL)
    return sgn, ld, info, np.ascontiguousarray(out[:, :n])


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def lapack(A):
    lu, piv = scipy.linalg.lu_factor(A)
    return lu, piv.astype(np.int64)


def say(capsys, text):
    with capsys.disabled():
        print("\nLUFIG gpu " + text, end="")


# ------------------------------------------------------------------------------------------------------------ 1. ties
@pytest.mark.parametrize("n", sorted(lr.TIE_CASES))
def test_pivot_ties_take_the_first_row(eng, n, capsys):
    """Exact ties of the pivot candidates (tests/lu_ref.py: TIE_CASES; test_tie_cases_reach_every_class lists what they
    reach): the smallest tied row wins at every tie, read off row col of U, which is that row of A bit for bit; the
    sign and the whole permutation are the reference's (getf2 up to N = 1100, beyond it LAPACK, which
    test_getf2_is_lapack_on_ties and test_lapack_takes_the_first_tied_row show to be the same on these matrices)."""
    A, expect, tied = lr.tie_case(n)
    if n <= 1100:
        ref, piv, info_ref = lr.getf2(A)
        assert info_ref == 0
    else:
        ref, piv = lapack(A)
    feats = set()
    for col, rows in tied:
        feats |= lr.tie_features(n, col, rows)
    assert lr.panel_class(n, 0) in feats and len(expect) == len(tied) >= 3
    sgn, ld, info, packed = factor(eng, A)
    assert info == 0
    for (col, want), (_, rows) in zip(expect, tied):
        got = [r for r in rows if np.array_equal(packed[col, col:], A[r, col:])]
        assert got == [want], (col, rows, got, sorted(map(str, lr.tie_features(n, col, rows))))
    assert sgn == lr.u_slogdet(ref)[0]
    assert np.array_equal(lr.recover_rows(A, packed), lr.perm_of(piv))
    ratio = lr.backward_ratio(A, packed, piv, lr.sample_rows(n))
    say(capsys, f"ties N={n} backward_ratio={ratio:.3g}")
    assert ratio <= 1.0


def test_tie_cases_reach_every_class():
    """What the five tie matrices reach together, asserted here as well as on the CPU."""
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


# ------------------------------------------------------------------------- 2. pivot sequence and backward error, all paths
def _gauss_ref(n):
    A = lr.scaled_gaussian(n, n)
    lu, piv = lapack(A)
    return A, lu, piv, lr.logdet_bound(A, lu, piv), lr.pivot_gap(lu)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", lr.GAUSS_SIZES)
def test_pivot_sequence_and_backward_error(eng, n, pad, capsys):
    """Gaussian matrices with a third of the rows scaled by -3 (no pivot decision closer than 1e-8: asserted here and in
    test_gaussian_cases_have_no_near_tie), contiguous and as a view of row stride N + 3: LAPACK's permutation, the
    componentwise backward bound on the sampled rows, the logdet within twice logdet_bound of LAPACK's (either side
    carries the bound once)."""
    A, lu, piv, bound, gap = cached(("gauss", n), lambda: _gauss_ref(n))
    assert gap >= 1e-8
    sgn, ld, info, packed = factor(eng, A, pad)
    assert info == 0
    assert np.array_equal(lr.recover_rows(A, packed), lr.perm_of(piv))
    ratio = lr.backward_ratio(A, packed, piv, lr.sample_rows(n))
    s_ref, ld_ref = lr.u_slogdet(lu)
    err = abs(ld - ld_ref)
    say(capsys, f"gaussian N={n} lda=N+{pad} backward_ratio={ratio:.3g} logdet_err/bound={err / bound:.3g}")
    assert ratio <= 1.0
    assert sgn == s_ref
    assert err <= 2.0 * bound


# ------------------------------------------------------------------------------------------------------- 3. zero pivots
@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("n", lr.ZERO_SIZES)
def test_zero_pivots(eng, n, case, capsys):
    """Columns that are exactly zero at and below the diagonal when the elimination reaches them: info is the first of
    them (LAPACK's), the logdet -inf, the factorization goes on as LAPACK's does -- same permutation, zeros on exactly
    those diagonal entries, every other u_ii of LAPACK's sign and inside the componentwise backward bound of its row --
    and the context factors a regular matrix correctly right afterwards."""
    cols = lr.zero_cases(n)[case]
    A = lr.zero_pivot_matrix(n, cols, np.random.default_rng(n + cols[-1]))
    lu, piv, info_ref = scipy.linalg.lapack.dgetrf(A)
    assert info_ref == min(cols) + 1
    sgn, ld, info, packed = factor(eng, A)
    assert info == info_ref
    assert ld == -np.inf
    du, dr = np.diag(packed), np.diag(lu)
    assert np.all(du[list(cols)] == 0) and np.array_equal(np.sign(du), np.sign(dr))
    assert sgn == lr.u_slogdet(lu)[0]
    assert np.array_equal(lr.recover_rows(A, packed), lr.perm_of(piv))
    ratio = lr.backward_ratio(A, packed, piv, lr.sample_rows(n))
    say(capsys, f"zero N={n} cols={cols} backward_ratio={ratio:.3g}")
    assert ratio <= 1.0
    B, blu, bpiv, bound, _ = cached(("gauss", 257), lambda: _gauss_ref(257))
    sgn, ld, info, packed = factor(eng, B)
    assert info == 0 and sgn == lr.u_slogdet(blu)[0] and abs(ld - lr.u_slogdet(blu)[1]) <= 2.0 * bound
    assert np.array_equal(lr.recover_rows(B, packed), lr.perm_of(bpiv))


# ------------------------------------------------------------------------------------------------------- 4. tiny pivots
@pytest.mark.parametrize("n,col,size", [(100, 20, 30), (600, 37, 40), (1100, 5, 30), (2100, 16, 30)],
                         ids=["reg256", "reg1024", "reg2048", "mem"])
def test_subnormal_pivot_divides(eng, n, col, size):
    """A pivot of -2^-1060 over entries k 2^-1063: its reciprocal is infinite, the multipliers are the exact k / 8."""
    A, p = lr.tiny_pivot_matrix(n, col, size, np.random.default_rng(n))
    assert lr.panel_class(n, col) == {100: "reg256", 600: "reg1024", 1100: "reg2048", 2100: "mem"}[n]
    ref, piv, info_ref = lr.getf2(A)
    assert info_ref == 0 and piv[col] == p
    sgn, ld, info, packed = factor(eng, A)
    assert info == 0 and np.isfinite(ld)
    perm = lr.recover_rows(A, packed)
    assert np.array_equal(perm, lr.perm_of(piv))
    assert packed[col, col] == A[p, col] == -2.0 ** -1060
    rows = np.arange(col + 1, col + size)
    assert np.array_equal(packed[rows, col], A[perm[rows], col] / A[p, col])
    assert np.all(packed[col + size:, col] == 0)
    assert sgn == lr.u_slogdet(ref)[0]


# ---------------------------------------------------------------------------------------------------- 5. I + Sigma Lambda
@pytest.mark.parametrize("seed", [2, 3])
def test_ipsl_exact_integers(eng, seed, capsys):
    """Sigma = I and a small-integer Lambda: the device's matrix is I + Lambda without a rounding."""
    m = 25
    d, f = lr.exact_case(seed=seed)
    n = d.size
    M = np.eye(n) + lr.star_lambda_dense(d, f, m)
    lu, piv = lapack(M)
    ref, rpiv, info_ref = lr.getf2(M, np.longdouble)
    assert info_ref == 0 and np.array_equal(piv, rpiv) and lr.pivot_gap(lu) >= 1e-8
    bound = lr.logdet_bound(M, lu, piv)
    sgn, ld, info = eng.laplace_logdet(eng.dev(np.eye(n)), eng.dev(d), eng.dev(f), m)
    s_ref, ld_ref = lr.u_slogdet(ref)
    err = abs(float(ld - ld_ref))
    say(capsys, f"exact seed={seed} N={n} logdet_err/bound={err / bound:.3g}")
    assert info == 0 and sgn == s_ref
    assert err <= bound


@pytest.mark.parametrize("j", [0, 27, 77, 78, 181])
def test_ipsl_exact_zero_column(eng, j):
    """lam_diag[j] = -1 alone under Sigma = I: column j of I + Lambda is exactly zero, info = j + 1."""
    m, n = 25, 182
    d = np.zeros(n)
    d[j] = -1.0
    sgn, ld, info = eng.laplace_logdet(eng.dev(np.eye(n)), eng.dev(d), eng.dev(np.zeros(n)), m)
    assert info == j + 1 and ld == -np.inf and sgn == 1.0


@pytest.mark.parametrize("m", lr.ONE_HOT_M)
def test_ipsl_one_hot(eng, m, capsys):
    """One non-zero weight and a NON-symmetric Gaussian Sigma (a transposed read, a wrong star offset or a mishandled
    last star changes the determinant): det(I + Sigma Lambda) in closed form, in long double, for the first, a middle
    and the last star.  The sign of U's diagonal is the determinant's times that of LAPACK's permutation."""
    S = lr.one_hot_sigma(m)
    Sd = eng.dev(S)
    worst = 0.0
    for name, d, f, closed in lr.one_hot_cases(m):
        det = closed(S.astype(np.longdouble))
        M = lr.ipsl_dense(S, d, f, m)
        lu, piv = lapack(M)
        assert lr.pivot_gap(lu) >= 1e-8, name
        bound = lr.logdet_bound(M, lu, piv)
        sgn, ld, info = eng.laplace_logdet(Sd, eng.dev(d), eng.dev(f), m)
        err = abs(float(ld - np.log(np.abs(det))))
        worst = max(worst, err / bound)
        assert info == 0, name
        assert sgn == float(np.sign(det)) * lr.piv_sign(piv), name
        assert err <= bound, (name, err, bound)
        if name.startswith("off_on_obs"):
            assert ld == 0.0 and sgn == 1.0, name
    say(capsys, f"one_hot m={m} N={S.shape[0]} logdet_err/bound={worst:.3g}")


@pytest.mark.parametrize("case", lr.REAL_CASES, ids=lambda c: f"{c[2][:2]}-{c[0]}x{c[1]}-{c[3]}")
def test_ipsl_real(eng, case, capsys):
    """Sigma a regularised Gram matrix, Lambda at a prior draw (the last case with sigma so small that most weights
    underflow to exactly 0): sign and logdet of the long double elimination of the dense matrix."""
    Sigma, d, o = lr.real_case(*case)
    m = case[1]
    M = lr.ipsl_dense(Sigma, d, o, m)
    lu, piv = lapack(M)
    ref, rpiv, info_ref = lr.getf2(M, np.longdouble)
    assert info_ref == 0 and np.array_equal(piv, rpiv) and lr.pivot_gap(lu) >= 1e-8
    bound = lr.logdet_bound(M, lu, piv)
    sgn, ld, info = eng.laplace_logdet(eng.dev(Sigma), eng.dev(d), eng.dev(o), m)
    s_ref, ld_ref = lr.u_slogdet(ref)
    err = abs(float(ld - ld_ref))
    say(capsys, f"real {case} N={M.shape[0]} logdet_err/bound={err / bound:.3g} (bound {bound:.3g})")
    assert info == 0 and sgn == s_ref
    assert err <= bound
