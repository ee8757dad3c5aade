"""NumPy statement of the pruned search (csrc/predict.hip: block_norm_kernel, the flagged kstar_kernel, prune_bounds_kernel,
prune_select_kernel), on the edge-form pieces of tests/probes/edge_form_identity.py.

For a candidate with K* column k, e = edge_kstar(k) its edge-layout column and op the operand the contraction reads (the
edge operator H, or a projected T in the same column layout):
    var   = sf2 + t + q,   t = k' Lambda k,   q = |op e|^2 >= 0
    sig_s = ||op[:, n_q + s m : n_q + (s + 1) m]||_F                     (one per star s)
    u     = sum_s sig_s |e_s|  >=  |op e|                                (Cauchy-Schwarz per star, triangle inequality)
    var_lo = sf2 + t,   var_hi = var_lo + (1 + 2^-20) u^2
Pointwise EI and VARIANCE do not decrease in var at a fixed mean, so s_lo = score(mu, var_lo) <= score <= s_hi =
score(mu, var_hi).  The threshold b is the largest s_lo; a candidate survives unless s_hi + tol < b, with
tol = 2^-36 max (|mu - mustar| + sqrt(var_hi)) for EI and 0 for VARIANCE.  Candidates with a non-finite sum always survive
and set no threshold.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "probes"))
from edge_form_identity import edge_kstar, edge_operator, lambda_dense, star_lambda  # noqa: E402,F401

EI, VARIANCE = "ei", "variance"
_erfc = np.vectorize(math.erfc, otypes=[float])


def block_norms(op, n_q, m):
    """sig [n_q]: the Frobenius norm of op's column block of every star (edge column layout)."""
    return np.array([np.sqrt((op[:, n_q + s * m:n_q + (s + 1) * m] ** 2).sum()) for s in range(n_q)])


def u_bound(E, sig, n_q, m):
    """u [M] = sum_s sig_s |E_s| for the edge-layout columns E [N, M]."""
    Es = E[n_q:n_q + n_q * m].reshape(n_q, m, -1)
    return (sig[:, None] * np.sqrt((Es ** 2).sum(1))).sum(0)


def score(mu, var, kind, mustar=0.0):
    """score_kernel's expression: the variance itself, or the pointwise expected improvement over mustar."""
    mu, var = np.asarray(mu, float), np.asarray(var, float)
    if kind == VARIANCE:
        return np.where(np.isnan(mu), np.nan, var)
    d = mu - mustar
    sd = np.sqrt(np.maximum(var, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd > 0.0, d / np.where(sd > 0.0, sd, 1.0), 0.0)
        ei = d * 0.5 * _erfc(-z / math.sqrt(2.0)) + sd * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return np.where(np.isnan(mu), np.nan, np.where(sd > 0.0, ei, np.maximum(d, 0.0)))


def interval(mu, t, u, sf2, kind, mustar=0.0):
    """(var_lo, var_hi, s_lo, s_hi) per candidate."""
    var_lo = sf2 + t
    var_hi = var_lo + (1.0 + 2.0 ** -20) * u * u
    return var_lo, var_hi, score(mu, var_lo, kind, mustar), score(mu, var_hi, kind, mustar)


def select(mu, var_hi, s_lo, s_hi, kind, mustar=0.0):
    """(threshold, tol, survivors ascending).  A candidate with a non-finite figure survives and sets no threshold."""
    ok = np.isfinite(mu) & np.isfinite(var_hi) & np.isfinite(s_lo) & np.isfinite(s_hi)
    if not ok.any():
        return -np.inf, 0.0, np.arange(mu.size)
    b = s_lo[ok].max()
    tol = 0.0
    if kind == EI:
        tol = 2.0 ** -36 * (np.abs(mu[ok] - mustar) + np.sqrt(np.maximum(var_hi[ok], 0.0))).max()
    hi = np.where(ok, s_hi, np.inf)
    return b, tol, np.flatnonzero(~(hi + tol < b))


def prune(K, alpha, ld, lo, op, m, sf2, kind, mustar=0.0):
    """Everything for the K* columns K [N, M] of a model (alpha, Lambda = (ld, lo) in star form, operand op):
    dict(mu, var, q, u, s_lo, s_hi, score, threshold, tol, survivors)."""
    N = K.shape[0]
    n_q = N // (m + 1)
    Lam = lambda_dense(ld, lo, m)
    E = edge_kstar(K, lo, m)
    mu = K.T @ alpha
    t = np.einsum("im,ij,jm->m", K, Lam, K)
    q = ((op @ E) ** 2).sum(0)
    u = u_bound(E, block_norms(op, n_q, m), n_q, m)
    var_lo, var_hi, s_lo, s_hi = interval(mu, t, u, sf2, kind, mustar)
    b, tol, surv = select(mu, var_hi, s_lo, s_hi, kind, mustar)
    var = sf2 + t + q
    return dict(mu=mu, var=var, q=q, u=u, s_lo=s_lo, s_hi=s_hi, score=score(mu, var, kind, mustar), threshold=b,
                tol=tol, survivors=surv)
