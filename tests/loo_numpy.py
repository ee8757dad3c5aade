"""NumPy statement of the answer scores (ppbo_loo_answers / ppbo_score_answers, GPModel.loo_pred / answers_score) -- test
infrastructure: it imports neither the product nor its kernels.

A star holds b = m + 1 rows, row 0 the point the user chose.  With sigma = theta[0], Delta_j = (f_j - f_0) / sigma and
phi2 the N(0, 2) density:
    w_j      = Delta_j phi2(Delta_j) / (2 m sigma^2)
    Lambda_q = sum_j w_j (e_0 - e_j)(e_0 - e_j)'
    g_q      : g_0 = sum_j phi2(Delta_j) / (sigma m),  g_j = -phi2(Delta_j) / (sigma m)
    cavity   : K_q = P_II^-1 + Lambda_q,  C_q = K_q^-1,  m_q = f_I - C_q g_q
and a group N(mu, C) is scored by
    p_j  = Phi((mu_0 - mu_j) / sqrt(2 sigma^2 + C_00 + C_jj - 2 C_0j))
    a    = mean_j p_j
    lpd  = log mean_s exp l(mu + L z_s),  l(f) = -(1/m) sum_j Phi((f_j - f_0) / (sigma sqrt 2)),  L L' = sym(C) + jitter I."""
import math

import numpy as np
from scipy.special import ndtr

_INV_SQRT_4PI = 1.0 / math.sqrt(4.0 * math.pi)


def site(f_star, sigma):
    """(Lambda_q [b, b], g_q [b]) of one star from its rows of f."""
    f_star = np.asarray(f_star, dtype=np.float64)
    b = f_star.size
    m = b - 1
    delta = (f_star[1:] - f_star[0]) / sigma
    p2 = _INV_SQRT_4PI * np.exp(-0.25 * delta * delta)
    w = delta * p2 / (2.0 * m * sigma ** 2)
    lam = np.zeros((b, b))
    lam[0, 0] = w.sum()
    lam[np.arange(1, b), np.arange(1, b)] = w
    lam[0, 1:] = -w
    lam[1:, 0] = -w
    g = np.empty(b)
    g[0] = p2.sum() / (sigma * m)
    g[1:] = -p2 / (sigma * m)
    return lam, g


def _inv_spd_ext(A):
    """The inverse of a symmetric positive definite matrix in extended precision (np.longdouble: Cholesky, the factor's
    inverse by forward substitution, L^-T L^-1), or None where a pivot is not positive (a NaN included)."""
    A = np.asarray(A, dtype=np.longdouble)
    A = 0.5 * (A + A.T)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Li = np.zeros((n, n), dtype=np.longdouble)
    for i in range(n):
        e = np.zeros(n, dtype=np.longdouble)
        e[i] = 1
        Li[i] = (e - L[i, :i] @ Li[:i]) / L[i, i]
    return Li.T @ Li


def cavity(P_block, f_star, sigma):
    """(m_q [b], C_q [b, b], info, K_q) of one star: info 0 fine, 1 P_II not positive definite, 2 the cavity is not (mean
    and covariance NaN then).

    The two inversions and m_q = f_I - C_q g_q run in extended precision and are rounded once at the end.  In fp64
    (np.linalg.inv twice) the statement itself loses m_q where a star falls back to the prior mean: on the cam_small fixture
    m_q cancels from max|f| = 7.0e-3 to max|m_q| = 1.9e-8 at cond(P_II) = 1.6e7, and against 60-digit linear algebra (mpmath)
    the fp64 statement is off by 1.1e-12 there -- 5.8e-5 of max|m_q| -- and this one by 5.6e-15, 2.9e-7 of max|m_q| (its
    covariance by 3.6e-13 of max|C_q|); on the other stars of that fixture by at most 2.4e-16."""
    P_block = np.asarray(P_block, dtype=np.float64)
    f_star = np.asarray(f_star, dtype=np.float64)
    b = f_star.size
    nan = (np.full(b, np.nan), np.full((b, b), np.nan))
    Pinv = _inv_spd_ext(P_block)
    if Pinv is None:
        return nan + (1, None)
    lam, g = site(f_star, sigma)
    K = Pinv + lam.astype(np.longdouble)
    K = 0.5 * (K + K.T)
    C = _inv_spd_ext(K)
    if C is None:
        return nan + (2, K.astype(np.float64))
    mq = f_star.astype(np.longdouble) - C @ g.astype(np.longdouble)
    return mq.astype(np.float64), C.astype(np.float64), 0, K.astype(np.float64)


def cavity_dense(P, f, q, m, sigma):
    """The same cavity by the dense route: Lambda_q added to the star's block of Q = P^-1, all of it inverted."""
    b = m + 1
    I = slice(q * b, (q + 1) * b)
    lam, g = site(f[I], sigma)
    Q = np.linalg.inv(P)
    Q[I, I] += lam
    Pm = np.linalg.inv(Q)
    e = np.zeros(len(f))
    e[I] = g
    return (f - Pm @ e)[I], Pm[I, I]


def edge_probs(mu, C, sigma):
    """p_j [m] of a group: ppbo_predict_pairs' rule, its den = 0 branch included."""
    mu, C = np.asarray(mu, dtype=np.float64), np.asarray(C, dtype=np.float64)
    C = 0.5 * (C + C.T)
    var = C[0, 0] + np.diag(C)[1:] - 2.0 * C[0, 1:]
    d = mu[0] - mu[1:]
    den = np.sqrt(2.0 * sigma ** 2 + np.maximum(var, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        zz = np.where(den > 0.0, d / den, np.where(d > 0.0, np.inf, np.where(d < 0.0, -np.inf, 0.0)))
    return np.where(np.isnan(var) | np.isnan(d), np.nan, ndtr(zz))


def ell(F, sigma):
    """l(f) for every row of F [S, b]."""
    m = F.shape[1] - 1
    return -ndtr((F[:, 1:] - F[:, :1]) / (sigma * math.sqrt(2.0))).sum(axis=1) / m


def draws(mu, C, z, jitter=0.0):
    """mu + L z_s [S, b], L the lower Cholesky factor of sym(C) + jitter I."""
    b = len(mu)
    L = np.linalg.cholesky(0.5 * (C + C.T) + jitter * np.eye(b))
    return np.asarray(mu)[None, :] + np.asarray(z) @ L.T


def answer_scores(mu, C, sigma, z=None, jitter=0.0):
    """dict(edge [m], agree, lpd (None without draws)) of one group; all NaN where the mean holds a NaN."""
    mu = np.asarray(mu, dtype=np.float64)
    if np.isnan(mu).any():
        return dict(edge=np.full(len(mu) - 1, np.nan), agree=np.nan, lpd=None if z is None else np.nan)
    p = edge_probs(mu, C, sigma)
    lpd = None
    if z is not None:
        lpd = math.log(np.exp(ell(draws(mu, C, z, jitter), sigma)).mean())
    return dict(edge=p, agree=float(p.mean()), lpd=lpd)


def loo(P, f, m, sigma, z=None, jitter=0.0):
    """Every star of (P, f): dict(lpd [n_q] or None, agree [n_q], edge [N] (row q b: a_q, rows q b + j: p_j), cav_mean
    [N], cav_var [N], cav_cov [n_q, b, b], info [n_q], min_eig [n_q] of the cavity precision)."""
    P, f = np.asarray(P, dtype=np.float64), np.asarray(f, dtype=np.float64).ravel()
    b = m + 1
    N = f.size
    n_q = N // b
    out = dict(lpd=None if z is None else np.empty(n_q), agree=np.empty(n_q), edge=np.empty(N), cav_mean=np.empty(N),
               cav_var=np.empty(N), cav_cov=np.empty((n_q, b, b)), info=np.zeros(n_q, dtype=np.int32),
               min_eig=np.full(n_q, np.nan))
    for q in range(n_q):
        I = slice(q * b, (q + 1) * b)
        mq, Cq, info, K = cavity(P[I, I], f[I], sigma)
        out["info"][q] = info
        if K is not None:
            out["min_eig"][q] = np.linalg.eigvalsh(K).min()
        out["cav_mean"][I], out["cav_cov"][q], out["cav_var"][I] = mq, Cq, np.diag(Cq)
        sc = answer_scores(mq, Cq, sigma, z, jitter)
        out["agree"][q] = sc["agree"]
        out["edge"][I] = np.concatenate([[sc["agree"]], sc["edge"]])
        if z is not None:
            out["lpd"][q] = sc["lpd"]
    return out


def heldout(mus, covs, sigma, z=None, jitter=0.0):
    """Groups with given means [B, G] and covariances [B, G, G]: dict(lpd [B] or None, agree [B], edge [B, G] (column 0: a))."""
    B, G = np.shape(mus)
    out = dict(lpd=None if z is None else np.empty(B), agree=np.empty(B), edge=np.empty((B, G)))
    for k in range(B):
        sc = answer_scores(mus[k], covs[k], sigma, z, jitter)
        out["agree"][k] = sc["agree"]
        out["edge"][k] = np.concatenate([[sc["agree"]], sc["edge"]])
        if z is not None:
            out["lpd"][k] = sc["lpd"]
    return out


def lpd_quadrature_m1(mu, C, sigma, n=200):
    """m = 1: lpd by 1-D Gauss-Hermite -- l depends on d = f_1 - f_0 ~ N(mu_1 - mu_0, C_00 + C_11 - 2 C_01) alone."""
    x, w = np.polynomial.hermite.hermgauss(n)
    md = mu[1] - mu[0]
    vd = C[0, 0] + C[1, 1] - C[0, 1] - C[1, 0]
    d = md + math.sqrt(2.0 * max(vd, 0.0)) * x
    return math.log((w * np.exp(-ndtr(d / (sigma * math.sqrt(2.0))))).sum() / math.sqrt(math.pi))


def flipped_design(n_q=12, m=15, D=2, seed=3, flip=None):
    """The design of the flipped-answer tests: utility -|x - 0.6|^2, query q moves axis q mod D through a random point;
    the answer is the best of m + 40 sorted abscissae (the WORST for query `flip`), beside m of the others."""
    rng = np.random.default_rng(seed)

    def u(x):
        return -np.sum((x - 0.6) ** 2, -1)

    rows = []
    for q in range(n_q):
        x = rng.random(D)
        d = q % D
        a = np.sort(rng.random(m + 40))
        pts = np.tile(x, (len(a), 1))
        pts[:, d] = a
        k = np.argmax(u(pts))
        if q == flip:
            k = np.argmin(u(pts))
        others = rng.choice(np.delete(np.arange(len(a)), k), m, replace=False)
        rows.append(pts[k])
        rows.extend(pts[others])
    return np.array(rows)
