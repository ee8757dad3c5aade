"""NumPy statement of a linear functional L f = sum_g w_g f(x_g) under the Laplace posterior (ppbo_predict_functionals,
GPModel.functional_pred) -- test infrastructure only.  With c = sum_g w_g k(x_g, X):

    mu = c' alpha,     var = w' K w - c' A c,     A = Sigma^-1 - Sigma^-1 P Sigma^-1  (pairs_numpy.operator_from_fit)

functional_reference forms w' K w as the PLAIN dense double sum over (g, h), diagonal included; rearranged_prior is the
host statement of the device's arrangement, sf^2 (sum w)^2 - 2 sum_{g<h} w_g w_h (sf^2 - k(x_g, x_h)) with the bracket in a
form that does not cancel.  The two are different sums of the same quantity: test_functionals_host.py holds them together."""
from __future__ import annotations

import numpy as np
import scipy.special

import pairs_numpy as pn
import slopes_numpy as sn


def _cross(Xq, X, theta, kernel):
    """pairs_numpy.cross; the per-coordinate camphor kernel (six length scales in theta[1]) through slopes_numpy.cross."""
    return sn.cross(Xq, X, theta, kernel) if kernel == sn.CAMPHOR_ARD else pn.cross(Xq, X, theta, kernel)


def _pair(Xa, Xb, theta, kernel):
    """pairs_numpy.pair_kernel; the per-coordinate camphor kernel from the same direct differences."""
    if kernel != sn.CAMPHOR_ARD:
        return pn.pair_kernel(Xa, Xb, theta, kernel)
    d, l = np.asarray(Xa, dtype=float) - np.asarray(Xb, dtype=float), sn.camphor_ls(theta)
    e = 0.5 * d[:, 2] ** 2 / l[2] ** 2 + sum(2.0 * np.sin(np.pi * d[:, k]) ** 2 / l[k] ** 2 for k in sn.PERIODIC)
    return float(theta[2]) ** 2 * np.exp(-e)


def _weights(w, M, G):
    w = np.asarray(w, dtype=float)
    if w.shape == (G,):
        return np.broadcast_to(w, (M, G))
    if w.shape == (M, G):
        return w
    raise ValueError(f"weights of shape {w.shape} for {M} groups of {G} points")


def functional_column(Xg, w, X, theta, kernel):
    """c [M, N] = sum_g w_g k(x_g, X), added in the order of g."""
    Xg = np.asarray(Xg, dtype=float)
    M, G, _ = Xg.shape
    W = _weights(w, M, G)
    c = np.zeros((M, np.shape(X)[0]))
    for g in range(G):
        c += W[:, g:g + 1] * _cross(Xg[:, g], X, theta, kernel)
    return c


def dense_prior(Xg, w, theta, kernel):
    """w' K w [M]: the plain double sum over all G^2 pairs (pairs_numpy.pair_kernel, direct differences)."""
    Xg = np.asarray(Xg, dtype=float)
    M, G, _ = Xg.shape
    W = _weights(w, M, G)
    out = np.zeros(M)
    for g in range(G):
        for h in range(G):
            out += W[:, g] * W[:, h] * _pair(Xg[:, g], Xg[:, h], theta, kernel)
    return out


def one_minus_kernel(Xa, Xb, theta, kernel):
    """1 - k(a_i, b_i) / sf^2 [M] from the direct differences, in forms that do not cancel at small distances."""
    Xa, Xb = np.atleast_2d(np.asarray(Xa, dtype=float)), np.atleast_2d(np.asarray(Xb, dtype=float))
    if kernel == pn.CAMPHOR:
        l = float(theta[1])
        ad = np.abs(Xa - Xb)
        e = sum(2.0 * np.sin(np.pi * ad[:, k]) ** 2 / l ** 2 for k in (0, 1, 3, 4, 5)) + 0.5 * ad[:, 2] ** 2 / (l + 0.05) ** 2
        return -np.expm1(-e)
    d = (Xa - Xb) / np.broadcast_to(np.asarray(theta[1], dtype=float), (Xa.shape[1],))
    r2 = (d * d).sum(axis=1)
    if kernel == "SE_kernel":
        return -np.expm1(-0.5 * r2)
    if kernel == "RQ_kernel":
        u = r2 / 4.0
        return u * (2.0 + u) / (1.0 + u) ** 2
    wq = {"Matern52_kernel": 1.0 / 3.0, "Matern32_kernel": 0.0}[kernel]
    a = np.sqrt((5.0 if kernel == "Matern52_kernel" else 3.0) * r2)
    # 1 - (1 + a + wq a^2) e^-a = e^-a (e^a - 1 - a - wq a^2); the bracket below a = 1 by its series
    small = a < 1.0
    series = (0.5 - wq) * a * a
    for k in range(3, 25):
        series = series + a ** k / scipy.special.factorial(k)
    return np.where(small, series * np.exp(-a), 1.0 - (1.0 + a + wq * a * a) * np.exp(-a))


def rearranged_prior(Xg, w, theta, kernel):
    """w' K w [M] in the device's arrangement: sf^2 (sum w)^2 - 2 sf^2 sum_{g<h} w_g w_h (1 - k(x_g, x_h) / sf^2)."""
    Xg = np.asarray(Xg, dtype=float)
    M, G, _ = Xg.shape
    W = _weights(w, M, G)
    s = np.zeros(M)
    for g in range(G):
        for h in range(g + 1, G):
            s += W[:, g] * W[:, h] * one_minus_kernel(Xg[:, g], Xg[:, h], theta, kernel)
    return float(theta[2]) ** 2 * (W.sum(axis=1) ** 2 - 2.0 * s)


def functional_reference(Xg, w, X, theta, kernel, alpha, A):
    """(mu, var) [M] of L f = sum_g w_g f(Xg[i, g]); w is [G] (one row for all groups) or [M, G]."""
    c = functional_column(Xg, w, X, theta, kernel)
    mu = c @ np.asarray(alpha, dtype=float)
    var = dense_prior(Xg, w, theta, kernel) - np.einsum("ij,ij->i", c, c @ A)
    return mu, var


def threshold_probability(mu, var, threshold=0.0):
    """P(L f > threshold) = Phi((mu - threshold) / sqrt(max(var, 0))); no variance: the sign decides, a tie is 1/2."""
    mu, var = np.asarray(mu, dtype=float), np.asarray(var, dtype=float)
    sd = np.sqrt(np.maximum(var, 0.0))
    d = mu - threshold
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd > 0.0, d / sd, np.where(d > 0.0, np.inf, np.where(d < 0.0, -np.inf, 0.0)))
    p = 0.5 * scipy.special.erfc(-z / np.sqrt(2.0))
    return np.where(np.isnan(mu) | np.isnan(var), np.nan, p)
