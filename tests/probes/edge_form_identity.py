"""NumPy statement of the edge-form variance operator (ppbo_posterior with PPBO_FORM_EDGE, include/ppbo_hip.h).

Lambda = sum over the star edges (obs_q, j) of w_j (e_obs - e_j)(e_obs - e_j)' (lam_diag[j] = w_j, lam_off[j] = -w_j,
lam_diag[obs] = the star's sum), B = Sigma^-1 - Lambda, P = B^-1.  With D the E x N edge incidence and e = diag(w) D k*:
    k*' Lambda P Lambda k* = e' (D P D') e = |H e|^2,   H = L22^-1,
L the Cholesky factor of Btilde = Dbar^-T B Dbar^-1 in the coordinates [n_q observation values; E edge differences,
star-major] and L22 its trailing E x E block.  Btilde is written entry by entry the way form_edge_kernel does (star sums of
Sigma^-1 and the edge diagonal lam_off), then checked against the dense congruence and the node form |R Lambda k*|^2.

    python tests/probes/edge_form_identity.py
"""
import numpy as np


def star_lambda(f, m, sigma):
    """lam_diag, lam_off of laplace_kernel (fit.hip) for a latent vector f (the weights' signs vary)."""
    N, mblk = f.size, m + 1
    c = 1.0 / (m * sigma * sigma)
    ld, lo = np.zeros(N), np.zeros(N)
    for o in range(0, N, mblk):
        d = (f[o + 1:o + mblk] - f[o]) / sigma
        w = 0.5 * c * d * np.exp(-0.25 * d * d) / np.sqrt(4 * np.pi)
        ld[o + 1:o + mblk], lo[o + 1:o + mblk] = w, -w
        ld[o] = w.sum()
    return ld, lo


def lambda_dense(ld, lo, m):
    N, mblk = ld.size, m + 1
    L = np.diag(ld)
    for o in range(0, N, mblk):
        L[o, o + 1:o + mblk] = lo[o + 1:o + mblk]
        L[o + 1:o + mblk, o] = lo[o + 1:o + mblk]
    return L


def edge_nodes(N, m):
    mblk, n_q = m + 1, N // (m + 1)
    return np.array([q * mblk + 1 + t for q in range(n_q) for t in range(m)])


def btilde(Sinv, lo, m):
    """form_edge_kernel: [U, -T[j]'; -T[j], Sinv[edges, edges] + diag(lam_off[edges])]."""
    N, mblk = Sinv.shape[0], m + 1
    n_q = N // mblk
    T = Sinv.reshape(N, n_q, mblk).sum(axis=2)            # T[i][q] = star q's sum of row i
    U = T.reshape(n_q, mblk, n_q).sum(axis=1)             # U[p][q] = 1_p' Sinv 1_q
    j = edge_nodes(N, m)
    Bt = np.empty((N, N))
    Bt[:n_q, :n_q] = U
    Bt[:n_q, n_q:] = -T[j].T
    Bt[n_q:, :n_q] = -T[j]
    Bt[n_q:, n_q:] = Sinv[np.ix_(j, j)] + np.diag(lo[j])
    return Bt


def edge_operator(Sinv, lo, m):
    """H [N, N] in the library's layout: zero observation rows / columns, L22^-1 at (n_q, n_q)."""
    N, n_q = Sinv.shape[0], Sinv.shape[0] // (m + 1)
    L = np.linalg.cholesky(btilde(Sinv, lo, m))
    H = np.zeros((N, N))
    H[n_q:, n_q:] = np.tril(np.linalg.inv(L[n_q:, n_q:]))
    return H


def edge_kstar(K, lo, m):
    """kstar_kernel's edge epilogue: row n_q + q m + t = lam_off[j] (k*_j - k*_obs), rows [0, n_q) zero.  K: [N, M]."""
    N, mblk = K.shape[0], m + 1
    n_q = N // mblk
    j = edge_nodes(N, m)
    E = np.zeros_like(K)
    E[n_q:] = lo[j, None] * (K[j] - K[(j // mblk) * mblk])
    return E


def dbar(N, m):
    mblk, n_q = m + 1, N // (m + 1)
    Db = np.zeros((N, N))
    for q in range(n_q):
        Db[q, q * mblk] = 1.0
    for e, j in enumerate(edge_nodes(N, m)):
        Db[n_q + e, (j // mblk) * mblk] = 1.0
        Db[n_q + e, j] = -1.0
    return Db


def check(n_q=5, m=7, D=3, M=40, seed=0):
    rng = np.random.default_rng(seed)
    N = n_q * (m + 1)
    X = rng.random((N, D))
    Sigma = np.exp(-0.5 * ((X[:, None] - X[None]) ** 2).sum(-1) / 0.3 ** 2) + 1e-3 * np.eye(N)
    Sinv = np.linalg.inv(Sigma)
    Sinv = 0.5 * (Sinv + Sinv.T)
    f = np.linalg.cholesky(Sigma) @ rng.standard_normal(N)
    ld, lo = star_lambda(f, m, 0.5)
    Lam = lambda_dense(ld, lo, m)
    B = Sinv - Lam
    Db = dbar(N, m)
    Dbi = np.linalg.inv(Db)
    ref = Dbi.T @ B @ Dbi
    Bt = btilde(Sinv, lo, m)
    scale = np.abs(ref).max()
    assert np.abs(Bt - ref).max() <= 1e-9 * scale, np.abs(Bt - ref).max() / scale
    # the variance term in both forms
    Xc = rng.random((M, D))
    K = np.exp(-0.5 * ((X[:, None] - Xc[None]) ** 2).sum(-1) / 0.3 ** 2)           # [N, M]
    R = np.linalg.inv(np.linalg.cholesky(B))
    node = ((R @ Lam @ K) ** 2).sum(0)
    H = edge_operator(Sinv, lo, m)
    edge = ((H @ edge_kstar(K, lo, m)) ** 2).sum(0)
    dense = np.einsum("im,ij,jm->m", K, Lam @ np.linalg.inv(B) @ Lam, K)
    assert np.abs(edge - dense).max() <= 1e-9 * max(1.0, np.abs(dense).max())
    assert np.abs(node - dense).max() <= 1e-9 * max(1.0, np.abs(dense).max())
    # H is lower triangular and zero outside [n_q, N)
    assert not np.triu(H, 1).any() and not H[:n_q].any() and not H[:, :n_q].any()
    return np.abs(edge - node).max()


if __name__ == "__main__":
    for args in ((5, 7, 3), (4, 31, 6), (3, 25, 2)):
        print(args, "max |edge - node| =", check(*args))
