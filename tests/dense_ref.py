"""CPU references for the dense-product tests (tests/test_gpu_dense_products.py) -- test infrastructure only.

Everything here is NumPy on host arrays: no device tensor is ever an input.  The helpers evaluate a reference on a
SUBSET of a large output (rows / columns that hold every tile edge, whole lines of a batch) so that products of
thousands of rows can be checked entry by entry without forming the whole result on the CPU; tests/test_dense_ref_host.py
shows on small cases that the subsets equal the full computation."""
import numpy as np

from oracle import ppbo_oracle as orc

U = 2.0 ** -53          # unit roundoff of fp64


def edge_indices(n, tile=32, last=128, extra=0, seed=0):
    """Sorted distinct indices in [0, n): the first and last index of every `tile`-wide tile (every edge of the 32, 64
    and 128 tiles of the GEMM engine for tile = 32), every index of the last, partial `last`-wide tile, and `extra`
    random indices besides."""
    idx = set()
    for t0 in range(0, n, tile):
        idx.add(t0)
        idx.add(min(t0 + tile, n) - 1)
    idx.update(range((n - 1) // last * last, n))
    if extra:
        idx.update(np.random.default_rng(seed).integers(0, n, extra).tolist())
    return np.array(sorted(idx), dtype=np.int64)


def op(X, trans):
    return X.T if trans else X


def gemm_reference(A, B, C0, alpha, beta, ta, tb, rows, cols):
    """(ref, bound) for C = alpha op(A) op(B) + beta C0 on the entries rows x cols.  ref: long-double dot products;
    bound: the componentwise error bound of an fp64 product of depth K in any summation order,
    2 K u (|alpha| (|op(A)| |op(B)|)_ij + |beta| |C0_ij|) (max(K, 1): the one rounding of beta C0 when K = 0).
    beta == 0: C0 is not read (it may hold NaN)."""
    a, b = op(A, ta)[rows], op(B, tb)[:, cols]
    K = a.shape[1]
    ref = float(alpha) * (a.astype(np.longdouble) @ b.astype(np.longdouble))
    mag = abs(alpha) * (np.abs(a) @ np.abs(b))
    if beta != 0.0:
        c = C0[np.ix_(rows, cols)]
        ref = ref + np.longdouble(beta) * c.astype(np.longdouble)
        mag = mag + abs(beta) * np.abs(c)
    return ref, 2.0 * max(K, 1) * U * mag


def gemm_errors(out, ref, bound):
    """max |out - ref| / bound over the sampled entries (<= 1 passes) and the worst absolute error."""
    err = np.abs(out.astype(np.longdouble) - ref).astype(np.float64)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()), float(err.max())


class CpuModel:
    """The posterior of (X, theta, kernel, m, f) built on the CPU without any device intermediate:
    orc.gram -> orc.pd_inverse -> orc.posterior_covariance -> orc.variance_operator (Woodbury form)."""

    def __init__(self, X, theta, kernel, m, f):
        self.X, self.theta, self.kernel, self.m = np.asarray(X, float), [float(t) for t in theta], kernel, int(m)
        self.f = np.asarray(f, float)
        self.Sigma = orc.gram(self.X, self.theta, kernel)
        self.Sinv = orc.pd_inverse(self.Sigma)
        self.lam = orc.lambda_dense(self.f, self.m, self.theta[0])
        self.P = orc.posterior_covariance(self.Sinv, self.f, self.m, self.theta[0])
        self.A = orc.variance_operator(self.Sinv, self.P, faithful=False, lam=self.lam)
        self.alpha = self.Sinv @ self.f

    def mean(self, Xc):
        return orc.cross_cov(self.X, Xc, self.theta, self.kernel).T @ self.alpha

    def mean_var(self, Xc):
        return orc.predict_mean_var(Xc, self.X, self.theta, self.alpha, self.A, self.kernel)

    def cov_entries(self, Xc, rows, cols):
        """Entries rows x cols of the M x M predictive covariance of orc.mu_sigma_pred (faithful=False): the prior
        block with the reference's shrink toward tr(K)/M I over ALL M points, minus K*_r' A K*_c."""
        Xc = np.asarray(Xc, float)
        M = Xc.shape[0]
        kern = orc.KERNELS[self.kernel]
        dg = np.concatenate([np.diag(kern(Xc[i:i + 256], Xc[i:i + 256], self.theta)) for i in range(0, M, 256)])
        dg = np.where(dg < 0, 1e-7, dg)
        prior = (1.0 - orc.SHRINKAGE) * kern(Xc[rows], Xc[cols], self.theta)
        prior = prior + orc.SHRINKAGE * (dg.sum() / M) * (rows[:, None] == cols[None, :])
        Kr = orc.cross_cov(self.X, Xc[rows], self.theta, self.kernel)
        Kc = orc.cross_cov(self.X, Xc[cols], self.theta, self.kernel)
        return prior - Kr.T @ (self.A @ Kc)

    def line_acq(self, xis, xs, alphas, z, mustar, jitter, lines):
        """orc.line_ei / orc.line_varmax of the given lines of a batch {alphas[b] * xis[b] + xs[b]} (alphas [G] or
        [B, G]), each on its own orc.mu_sigma_pred covariance and the draws z."""
        ei, vm = [], []
        for b in lines:
            al = alphas[b] if np.ndim(alphas) == 2 else alphas
            grid = orc.line_grid(xis[b], xs[b], al)
            mu, cov = orc.mu_sigma_pred(grid, self.X, self.theta, self.Sinv, self.f, self.P, self.kernel, faithful=False,
                                        A=self.A)
            ei.append(orc.line_ei(mu, cov, z, mustar, jitter=jitter))
            vm.append(orc.line_varmax(mu, cov, z, jitter=jitter))
        return np.array(ei), np.array(vm)


def line_y_chunk(points):
    """Column tiles per chunk of the line acquisition's Y = G K* for a batch of `points` grid points when
    PPBO_LINE_Y_CHUNK is not set: equal chunks of at most 72 128-column tiles (ppbo_amd/csrc/predict.hip)."""
    tiles = (points + 127) // 128
    chunks = (tiles + 71) // 72
    return (tiles + chunks - 1) // chunks


def line_picks(B, G, chunk_tiles=(), n=64, seed=0):
    """About n line indices of a batch of B lines of G points: the first and the last line, every line whose points
    straddle a chunk boundary (a multiple of 128 c columns for c in chunk_tiles), then lines that straddle a 128-column
    tile boundary, then random lines, in that order of preference."""
    first = lambda b: b * G
    last = lambda b: b * G + G - 1
    pick = [0, B - 1]
    for c in chunk_tiles:
        w = 128 * c
        pick += [b for b in range(B) if first(b) // w != last(b) // w]
    tile = [b for b in range(B) if first(b) // 128 != last(b) // 128]
    rng = np.random.default_rng(seed)
    out = list(dict.fromkeys(pick))
    for b in rng.permutation(tile).tolist() + rng.permutation(B).tolist():
        if len(out) >= n:
            break
        if b not in out:
            out.append(b)
    return np.array(sorted(out), dtype=np.int64)
