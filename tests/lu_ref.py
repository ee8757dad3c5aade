"""CPU references for the LU behind the evidence (ppbo_amd/csrc/lu.hip) -- test infrastructure only.

Everything here is NumPy / SciPy on host arrays: no device tensor is ever an input.  tests/test_lu_ref_host.py shows that
the references and the bounds are sound (against LAPACK and against closed forms) before tests/test_gpu_lu.py judges the
device by them.

Conventions: `packed` is the in-place result of an LU (unit lower L strictly below the diagonal, U on and above it),
`piv` the 0-based row interchanges of LAPACK (row k was swapped with row piv[k] at step k), `info` LAPACK's: 0, or the
1-based index of the first exactly zero pivot."""
import numpy as np

U = 2.0 ** -53          # unit roundoff of fp64
LNB = 16                # the device's panel width
SFMIN = 2.2250738585072014e-308


def gamma(k):
    """k u / (1 - k u)."""
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------------------------------------------- the factorization
def getf2(A, dtype=np.float64):
    """Unblocked LU with partial pivoting in `dtype` (float64 or longdouble): the pivot of column k is the FIRST row of
    maximal |entry| at and below the diagonal; a zero pivot is skipped (the first one recorded in info) and the
    factorization goes on; the multipliers are quotients.  Returns (packed, piv, info).  Rows past the last non-zero
    multiplier are not touched (a - 0 u = a), which keeps block triangular matrices cheap."""
    a = np.array(A, dtype=dtype, copy=True)
    n = a.shape[0]
    piv = np.arange(n)
    info = 0
    buf = np.empty((n, n), dtype=dtype)
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))           # argmax: the first maximal element
        piv[k] = p
        if p != k:
            a[[k, p]] = a[[p, k]]
        if a[k, k] == 0:
            info = info or k + 1
            continue
        a[k + 1:, k] /= a[k, k]
        nz = np.flatnonzero(a[k + 1:, k])
        if nz.size:
            hi = k + 2 + int(nz[-1])
            w = buf[: hi - k - 1, : n - k - 1]
            np.multiply.outer(a[k + 1:hi, k], a[k, k + 1:], out=w)
            v = a[k + 1:hi, k + 1:]
            np.subtract(v, w, out=v)
    return a, piv, info


def apply_piv(A, piv):
    """P A: the interchanges piv applied to the rows of A in order."""
    return A[perm_of(piv)]


def perm_of(piv):
    """The row permutation of the interchanges piv: (P A)[i] = A[perm[i]]."""
    perm = np.arange(len(piv))
    for k, p in enumerate(piv):
        if p != k:
            perm[k], perm[p] = perm[p], perm[k]
    return perm


def piv_sign(piv):
    """det P."""
    return -1.0 if int(np.count_nonzero(np.asarray(piv) != np.arange(len(piv)))) & 1 else 1.0


def split(packed):
    n = packed.shape[0]
    return np.tril(packed, -1) + np.eye(n, dtype=packed.dtype), np.triu(packed)


def u_slogdet(packed):
    """(prod sign(u_ii), sum log|u_ii|): the value the evidence uses (the sign of P is NOT in it); a zero on the diagonal
    does not change the sign, as on the device, and gives -inf."""
    d = np.diag(packed)
    with np.errstate(divide="ignore"):
        ld = np.sum(np.log(np.abs(d)))
    return (-1.0 if int(np.count_nonzero(d < 0)) & 1 else 1.0), ld


def pivot_gap(packed):
    """The smallest relative gap between the pivot and the second-best candidate of its column over all steps of the
    factorization `packed` records: the candidates of step k are u_kk and l_ik u_kk, so the gap is 1 - max_i |l_ik|.
    Steps with a zero pivot are left out."""
    n = packed.shape[0]
    L = np.abs(np.tril(packed, -1))
    ok = np.diag(packed)[: n - 1] != 0
    if n < 2 or not ok.any():
        return 1.0
    return float((1.0 - L[:, : n - 1].max(axis=0))[ok].min())


# ----------------------------------------------------------------------------------------------------------- the bounds
def sample_rows(n, tile=LNB):
    """Rows to hold a factorization of n rows to: the first and last row of every 16-row panel and every row of the last,
    partial panel (dense_ref.edge_indices with the panel as the tile)."""
    idx = set()
    for t0 in range(0, n, tile):
        idx.add(t0)
        idx.add(min(t0 + tile, n) - 1)
    idx.update(range((n - 1) // tile * tile, n))
    return np.array(sorted(idx), dtype=np.int64)


def _slices(X, axis, bits):
    """X as a sum of fp64 arrays whose entries along `axis` are multiples of one power of two with at most `bits` bits."""
    X = np.array(X, dtype=np.float64, copy=True)
    out = []
    while True:
        mu = np.abs(X).max(axis=axis, keepdims=True)
        if not mu.any():
            return out
        _, e = np.frexp(mu)                                 # |X| < 2^e along the axis
        sigma = np.where(mu > 0, np.ldexp(0.75, e + 54 - bits), 0.0)
        hi = (X + sigma) - sigma                            # X rounded to a multiple of 2^(e + 1 - bits); X - hi is exact
        out.append(hi)
        X -= hi
        if len(out) > 64:
            raise ValueError("range of the entries too wide to slice")


def product_ld(A, B):
    """A @ B of fp64 matrices to long double accuracy at the speed of fp64 products: the rows of A and the columns of B
    are cut into slices of b bits on a common power of two with 2 b + log2 K <= 53, so every slice product is a sum of
    integers below 2^53 times a power of two -- exact in fp64 in any order -- and only their sum is rounded, in long
    double.  (Plain long double products run without BLAS: minutes at N = 2000.)"""
    K = A.shape[1]
    bits = (53 - max(1, int(np.ceil(np.log2(K))))) // 2
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.longdouble)
    sb = _slices(B, 0, bits)
    for a in _slices(A, 1, bits):
        for b in sb:
            acc += a @ b
    return acc


def backward_ratio(A, packed, piv, rows=None):
    """max over the given rows i and all j of |(L U - P A)_ij| / (gamma(N + 2) (|L| |U|)_ij), L U to long double accuracy.
    Higham's componentwise backward bound for Gaussian elimination, |L U - P A| <= gamma_N |L| |U|, holds for any order of
    the sums; the 2 more roundings pay for multipliers formed as a_ik * (1 / u_kk).  <= 1 passes.  An entry with
    (|L| |U|)_ij = 0 must be reproduced exactly."""
    n = A.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    L, Um = split(np.asarray(packed, dtype=np.float64))
    err = np.abs(product_ld(L[rows], Um) - apply_piv(A, piv)[rows].astype(np.longdouble)).astype(np.float64)
    mag = gamma(n + 2) * (np.abs(L[rows]) @ np.abs(Um))
    ratio = np.where(mag > 0, err / np.where(mag > 0, mag, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())


def logdet_bound(M, packed, piv):
    """Bound on |sum log|u_ii| - log|det M|| of an fp64 LU of M, to first order: the computed factors are exact for
    P M + E with |E| <= gamma(N + 2) |L| |U|, and d log|det| = tr((P M)^-1 E), so the error is at most
    gamma(N + 2) sum_ij |(P M)^-1|_ji (|L| |U|)_ij; the sum of N logarithms adds N u max|log|u_ii||.
    packed / piv: LAPACK's fp64 factors of M."""
    n = M.shape[0]
    L, Um = split(np.asarray(packed, dtype=np.float64))
    inv = np.linalg.inv(apply_piv(M, piv))
    mag = np.abs(L) @ np.abs(Um)
    d = np.abs(np.diag(Um))
    return float(gamma(n + 2) * np.sum(np.abs(inv).T * mag) + n * U * np.abs(np.log(d)).max())


def recover_rows(A, packed):
    """The row permutation an in-place LU used, from its output alone: row i of L U is row perm[i] of A up to rounding,
    so perm[i] is the row of A nearest to it.  Raises if the nearest rows are not a permutation."""
    L, Um = split(np.asarray(packed, dtype=np.float64))
    LU = L @ Um
    d2 = (LU * LU).sum(1)[:, None] - 2.0 * (LU @ A.T) + (A * A).sum(1)[None, :]
    perm = np.argmin(d2, axis=1)
    if not np.array_equal(np.sort(perm), np.arange(A.shape[0])):
        raise AssertionError("the rows of L U do not match the rows of A one to one")
    return perm


# ------------------------------------------------------------------------------------------------------------- matrices
def _block_starts(n, block_sizes):
    sizes = [int(s) for s in block_sizes]
    if sum(sizes) > n or min(sizes, default=1) < 1:
        raise ValueError("block sizes")
    if sum(sizes) < n:
        sizes.append(n - sum(sizes))
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int), sizes


def block_upper(n, block_sizes, rng):
    """Gaussian n x n matrix with exact zeros below its diagonal blocks (sizes in order from row 0; what they leave of n
    is one last block).  Returns (A, starts, sizes)."""
    starts, sizes = _block_starts(n, block_sizes)
    A = rng.standard_normal((n, n))
    for c0, s in zip(starts, sizes):
        A[c0 + s:, c0:c0 + s] = 0.0
    return A, starts, sizes


def tie_matrix(n, block_sizes, rng, ties=None):
    """Block upper triangular matrix whose diagonal blocks of size >= 2 start with an exact pivot tie.

    The multipliers from a block into the rows below it are exactly 0, so every block's first column reaches its
    elimination step bit for bit as written, whatever the blocking or the order of the sums: +-1.5 in two or more rows of
    the block, |x| <= 0.5 in the others.  ties: {block index: (row offsets in the block, signs)} where the caller wants to
    choose; elsewhere 2 or 3 rows and their signs are drawn.  Returns (A, [(col, expected_row)], [(col, tied rows)]): the
    expected pivot is the smallest tied row, and row `col` of the device's U right of the diagonal is then the original
    A[expected_row, col:] bit for bit (the tied rows differ there, they are Gaussian)."""
    A, starts, sizes = block_upper(n, block_sizes, rng)
    ties = ties or {}
    expect, tied = [], []
    for b, (c0, s) in enumerate(zip(starts, sizes)):
        if s < 2:
            continue
        if b in ties:
            offs, signs = ties[b]
        else:
            k = min(s, int(rng.integers(2, 4)))
            offs = np.sort(rng.choice(s, k, replace=False))
            signs = rng.choice([-1.0, 1.0], k)
        offs = np.asarray(offs, dtype=int)
        if len(set(offs.tolist())) < 2 or offs.min() < 0 or offs.max() >= s:
            raise ValueError("tied rows")
        A[c0:c0 + s, c0] = rng.uniform(-0.5, 0.5, s)
        A[c0 + offs, c0] = 1.5 * np.asarray(signs, dtype=float)
        expect.append((int(c0), int(c0 + offs.min())))
        tied.append((int(c0), tuple(int(c0 + o) for o in offs)))
    return A, expect, tied


def zero_pivot_matrix(n, cols, rng):
    """Block upper triangular Gaussian matrix in which every column of `cols` starts a diagonal block and is exactly zero
    at and below the diagonal (so it still is when the elimination reaches it); blocks are at most 48 columns wide
    otherwise.  LAPACK's info is min(cols) + 1."""
    cols = sorted(int(c) for c in cols)
    cuts = sorted(set(range(0, n, 48)) | set(cols))
    sizes = [b - a for a, b in zip(cuts, cuts[1:] + [n])]
    A, _, _ = block_upper(n, sizes, rng)
    for c in cols:
        A[c:, c] = 0.0
    return A


def tiny_pivot_matrix(n, col, size, rng, e=-1060):
    """Block upper triangular Gaussian matrix with a diagonal block of `size` rows at column `col` whose first column is
    subnormal: -2^e in the block's 3rd row (the pivot) and k 2^(e-3), |k| <= 7, in the others, so the multipliers are the
    exactly representable -k / 8 -- and 1 / pivot overflows.  The blocks after it are 48 wide.  Returns (A, pivot row)."""
    rest = n - col - size
    A, _, _ = block_upper(n, ([col] if col else []) + [size] + [48] * (rest // 48), rng)
    A[col:col + size, col] = np.ldexp(rng.integers(-7, 8, size).astype(float), e - 3)
    A[col + 2, col] = -np.ldexp(1.0, e)
    return A, col + 2


def star_lambda_dense(lam_diag, lam_off, m):
    """The dense N x N Lambda of the star layout (include/ppbo_hip.h): rows q (m + 1) are the observations, the m rows
    after each its pseudo-observations j, with Lambda[j, j] = lam_diag[j] and Lambda[obs(j), j] = Lambda[j, obs(j)] =
    lam_off[j]; lam_off on observation rows is ignored."""
    lam_diag, lam_off = np.asarray(lam_diag), np.asarray(lam_off)
    n = lam_diag.shape[0]
    lam = np.diag(lam_diag).astype(np.result_type(lam_diag, lam_off))
    j = np.arange(n)
    pse = j[j % (m + 1) != 0]
    obs = pse // (m + 1) * (m + 1)
    lam[obs, pse] = lam_off[pse]
    lam[pse, obs] = lam_off[pse]
    return lam


# ------------------------------------------------------------------------------------ where a tie sits in the device's LU
def panel_class(n, col):
    """The panel kernel that factors column col of an n x n matrix, by the rows left at its panel's start:
    'reg256', 'reg512', 'reg1024' (a thread owns one row), 'reg2048' (two rows, t and t + 1024) or 'mem'."""
    rem = n - col // LNB * LNB
    for lim in (256, 512, 1024, 2048):
        if rem <= lim:
            return f"reg{lim}"
    return "mem"


def tie_features(n, col, rows):
    """What a tie at column col between `rows` of an n x n matrix exercises on the device: its panel kernel, its column
    in the panel, first / last panel, and how the tied rows are spread over threads and wavefronts."""
    k0 = col // LNB * LNB
    cls = panel_class(n, col)
    if cls == "mem":
        thread = [(r - col) % 1024 for r in rows]          # the memory-resident panel strides from the diagonal
    else:
        thread = [(r - k0) % min(int(cls[3:]), 1024) for r in rows]
    f = {cls, ("J", col - k0)}
    if k0 == 0:
        f.add("first_panel")
    if k0 + LNB >= n:
        f.add("last_panel")
    for i in range(len(rows)):
        for j in range(i + 1, len(rows)):
            if thread[i] == thread[j]:
                f.add((cls, "same_thread"))
            elif thread[i] // 64 == thread[j] // 64:
                f.add((cls, "same_wave"))
            else:
                f.add((cls, "other_wave"))
            if cls == "mem" and abs(rows[i] - rows[j]) > 1024:
                f.add((cls, "far"))
    return f


# Tie cases of the device test: n -> (block sizes, {block: (tied row offsets, signs)}, seed).  tests/test_lu_ref_host.py
# asserts that together they reach every class the device distinguishes.
TIE_CASES = {
    150: ([2, 3, 17, 40, 82, 3, 3], {0: ((0, 1), (1, -1)), 4: ((0, 70), (-1, 1)), 6: ((1, 2), (-1, -1))}, 1),
    700: ([17] * 16 + [129, 297, 2], {16: ((5, 80, 128), (1, -1, 1)), 17: ((0, 290), (-1, -1))}, 2),
    1100: ([5, 1075, 20], {0: ((1, 3), (-1, 1)), 1: ((2, 1026), (1, -1))}, 3),
    2100: ([3, 40, 1100, 957], {0: ((0, 2), (1, 1)), 1: ((4, 9), (1, -1)), 2: ((0, 1024, 1090), (-1, 1, -1)),
                                3: ((0, 700), (1, -1))}, 4),
    2200: ([20, 150, 6, 1100, 924], {0: ((0, 5), (-1, 1)), 1: ((1, 100), (1, 1)), 2: ((0, 4), (1, -1)),
                                     3: ((3, 500, 1027), (1, -1, -1)), 4: ((7, 8), (-1, 1))}, 5),
}


def tie_case(n):
    sizes, ties, seed = TIE_CASES[n]
    return tie_matrix(n, sizes, np.random.default_rng(seed), ties)


def scaled_gaussian(n, seed):
    """The Gaussian matrix of test_lu_slogdet_matches_lapack_pivoting: a third of the rows scaled by -3."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A[rng.integers(0, n, max(1, n // 3)), :] *= -3.0
    return A


# ------------------------------------------------------------------------------------------------- I + Sigma Lambda cases
ONE_HOT_M = (1, 2, 25, 63, 100)
ONE_HOT_NQ = 7


def one_hot_cases(m, n_q=ONE_HOT_NQ):
    """(name, lam_diag, lam_off, closed form of det(I + S Lambda) as a function of S) for the first, a middle and the
    last star: one diagonal weight on a pseudo row and on an observation row, one edge weight, and an edge weight on an
    observation row (ignored: det = 1)."""
    n = n_q * (m + 1)
    out = []
    for q in (0, n_q // 2, n_q - 1):
        o = q * (m + 1)
        j = o + m                                # the star's last pseudo row: the matrix's last row for the last star
        for name, row, w in (("diag_pseudo", j, 0.7), ("diag_obs", o, -1.3)):
            d, f = np.zeros(n), np.zeros(n)
            d[row] = w
            out.append((f"{name}_q{q}", d, f, lambda S, row=row, w=w: 1 + w * S[row, row]))
        d, f = np.zeros(n), np.zeros(n)
        f[j] = v = -0.9
        out.append((f"off_q{q}", d, f,
                    lambda S, j=j, o=o, v=v: (1 + v * S[j, o]) * (1 + v * S[o, j]) - v * v * S[j, j] * S[o, o]))
        d, f = np.zeros(n), np.zeros(n)
        f[o] = 2.5
        out.append((f"off_on_obs_q{q}", d, f, lambda S: S.dtype.type(1)))
    return out


def one_hot_sigma(m, n_q=ONE_HOT_NQ):
    n = n_q * (m + 1)
    return np.random.default_rng(1000 + m).standard_normal((n, n))


def ipsl_dense(Sigma, lam_diag, lam_off, m):
    """I + Sigma Lambda in fp64, Lambda dense."""
    return np.eye(Sigma.shape[0]) + Sigma @ star_lambda_dense(lam_diag, lam_off, m)


def exact_case(n_q=7, m=25, seed=0):
    """(lam_diag, lam_off) of small integers for Sigma = I: I + Sigma Lambda = I + Lambda without a rounding.  The edge
    weights of a star are +-(1 .. m) in a drawn order -- equal magnitudes would tie pivot candidates exactly -- and the
    observation's diagonal is larger than all of them."""
    rng = np.random.default_rng(seed)
    n = n_q * (m + 1)
    d = rng.choice([-4, -3, -2, 1, 2, 3, 4], n).astype(float)
    d[:: m + 1] = rng.integers(m + 5, m + 15, n_q)
    f = np.zeros((n_q, m + 1))
    for q in range(n_q):
        f[q, 1:] = rng.permutation(np.arange(1, m + 1)) * rng.choice([-1.0, 1.0], m)
    return d, f.ravel()


REAL_CASES = [(n_q, m, kernel, 0.3) for n_q, m in ((8, 25), (16, 31), (40, 25)) for kernel in ("SE_kernel", "Matern52_kernel")]
REAL_CASES.append((8, 25, "SE_kernel", 2e-3))            # Delta = df / sigma beyond 55: weights underflow to exactly 0


def real_case(n_q, m, kernel, sigma):
    """(Sigma, lam_diag, lam_off) of a seeded design: Sigma the regularised Gram matrix, Lambda at a draw f ~ N(0, Sigma)."""
    from oracle import ppbo_oracle as orc
    from test_matern_host import matern
    X = orc.synthetic_design(n_q, 3, m=m, seed=n_q + m)
    theta = [sigma, 0.4, 1.0]
    if kernel in orc.KERNELS:
        Sigma = orc.gram(X, theta, kernel)
    else:
        Sigma = orc.regularize_covariance(matern(X, X, theta, kernel), orc.SHRINKAGE)
    f = np.linalg.cholesky(Sigma) @ np.random.default_rng(7 * n_q + m).standard_normal(Sigma.shape[0])
    d, o = orc.lambda_compact(f, m, sigma)
    return Sigma, d, o


ZERO_SIZES = (100, 600, 2100)


def zero_cases(n):
    """Zero columns of the device test for an n x n matrix: column 0, inside a panel, the last column of a panel, the
    first column of a later panel, column n - 1, and two at once (the first inside the first panels)."""
    k0 = n // 2 // LNB * LNB
    return [(0,), (k0 + 5,), (k0 + 15,), (k0 + 16,), (n - 1,), (21, k0 + 5)]


GAUSS_SIZES = (257, 513, 1025, 2049, 2065)
