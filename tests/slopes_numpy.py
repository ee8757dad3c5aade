"""NumPy statement of a slope under the Laplace posterior (ppbo_predict_slopes, GPModel.slope_pred) -- test
infrastructure only, no device input.  For a point x and a direction xi, with the column

    g_j = d/da k(x + a xi, x_j) at a = 0

    mu_s = g' alpha,     var_s = prior - g' A g,     A = Sigma^-1 - Sigma^-1 P Sigma^-1  (oracle.variance_operator)
    prior = xi' (d^2 k / dx dx')(x, x) xi,     p = Phi(mu_s / sqrt(max(var_s, 0)))

the dense form tests/pairs_numpy.py uses for duels.  Every derivative is analytic, from direct differences:

    radial kernels (scalar or per-dimension length scales l_d), k = sf^2 kappa(rho^2), rho^2 = sum_d ((x_d - x_jd) / l_d)^2:
        g_j = 2 sf^2 kappa'(rho_j^2) sum_d (x_d - x_jd) xi_d / l_d^2,     prior = -2 kappa'(0) sf^2 sum_d (xi_d / l_d)^2
    camphor-copper (six length scales l_d; the scalar-l kernel is the profile (l, l, l + 0.05, l, l, l)), k = sf^2 e^-s,
    s = sum_{d != 2} 2 sin^2(pi D_d) / l_d^2 + D_2^2 / (2 l_2^2),  D = x - x_j:
        g_j = -k_j (sum_{d != 2} (2 pi / l_d^2) sin(2 pi D_d) xi_d + D_2 xi_2 / l_2^2)
        prior = sf^2 (sum_{d != 2} 4 pi^2 xi_d^2 / l_d^2 + xi_2^2 / l_2^2)

tests/test_slopes_host.py confirms g, mu_s and var_s (and with them the constants kappa'(0) and the camphor prior) by
central differences of the dense kernel and its posterior."""
from __future__ import annotations

import numpy as np
from scipy.special import ndtr

from evgrad_numpy import kappa

CAMPHOR = "camphor_copper_kernel"
CAMPHOR_ARD = "camphor_copper_ard_kernel"
PERIODIC = (0, 1, 3, 4, 5)


def camphor_ls(theta):
    l = theta[1]
    return float(l) + np.array([0.0, 0.0, 0.05, 0.0, 0.0, 0.0]) if np.ndim(l) == 0 else np.asarray(l, dtype=float)


def _ls(theta, D):
    return np.broadcast_to(np.asarray(theta[1], dtype=float), (D,)).astype(float)


def cross(Xq, X, theta, kernel):
    """k(x_c, x_i) [M, N] from direct differences (all five kernels and the per-coordinate camphor kernel)."""
    Xq, X = np.atleast_2d(np.asarray(Xq, dtype=float)), np.atleast_2d(np.asarray(X, dtype=float))
    sf2 = float(theta[2]) ** 2
    d = Xq[:, None, :] - X[None, :, :]
    if kernel in (CAMPHOR, CAMPHOR_ARD):
        l = camphor_ls(theta)
        s = 0.5 * d[:, :, 2] ** 2 / l[2] ** 2
        for k in PERIODIC:
            s = s + 2.0 * np.sin(np.pi * d[:, :, k]) ** 2 / l[k] ** 2
        return sf2 * np.exp(-s)
    d = d / _ls(theta, Xq.shape[1])
    return sf2 * kappa((d * d).sum(axis=2), kernel)[0]


def slope_column(Xq, Xi, X, theta, kernel):
    """g [M, N]: g[i, j] = d/da k(Xq[i] + a Xi[i], X[j]) at a = 0."""
    Xq, Xi, X = (np.atleast_2d(np.asarray(a, dtype=float)) for a in (Xq, Xi, X))
    sf2 = float(theta[2]) ** 2
    d = Xq[:, None, :] - X[None, :, :]
    if kernel in (CAMPHOR, CAMPHOR_ARD):
        l = camphor_ls(theta)
        ds = d[:, :, 2] * Xi[:, None, 2] / l[2] ** 2
        for k in PERIODIC:
            ds = ds + (2.0 * np.pi / l[k] ** 2) * np.sin(2.0 * np.pi * d[:, :, k]) * Xi[:, None, k]
        return -cross(Xq, X, theta, kernel) * ds
    l = _ls(theta, Xq.shape[1])
    r2 = ((d / l) ** 2).sum(axis=2)
    return 2.0 * sf2 * kappa(r2, kernel)[1] * (d * (Xi / l ** 2)[:, None, :]).sum(axis=2)


def slope_prior(Xi, theta, kernel):
    """xi' (d^2 k / dx dx')(x, x) xi [M] (the kernels are stationary: no x)."""
    Xi = np.atleast_2d(np.asarray(Xi, dtype=float))
    sf2 = float(theta[2]) ** 2
    if kernel in (CAMPHOR, CAMPHOR_ARD):
        l = camphor_ls(theta)
        w = np.full(6, 4.0 * np.pi ** 2) / l ** 2
        w[2] = 1.0 / l[2] ** 2
        return sf2 * (Xi ** 2 * w).sum(axis=1)
    l = _ls(theta, Xi.shape[1])
    return -2.0 * float(kappa(np.zeros(1), kernel)[1][0]) * sf2 * ((Xi / l) ** 2).sum(axis=1)


def slope_reference(Xq, Xi, X, theta, kernel, alpha, A):
    """(mu_s, var_s, g) of the rows (Xq[i], Xi[i]): g is returned for the error measures (sum_j |g_j alpha_j|)."""
    g = slope_column(Xq, Xi, X, theta, kernel)
    mu = g @ np.asarray(alpha, dtype=float)
    var = slope_prior(Xi, theta, kernel) - np.einsum("ij,ij->i", g, g @ A)
    return mu, var, g


def slope_probability(mu_s, var_s):
    """P(slope > 0) = Phi(mu_s / sqrt(max(var_s, 0))): no noise term; without variance the sign of mu_s decides and a
    tie is 1/2; NaN in, NaN out."""
    mu = np.asarray(mu_s, dtype=float)
    sd = np.sqrt(np.maximum(np.asarray(var_s, dtype=float), 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd > 0.0, mu / sd, np.where(mu > 0.0, np.inf, np.where(mu < 0.0, -np.inf, 0.0)))
    z = np.where(np.isnan(mu) | np.isnan(sd), np.nan, z)
    return ndtr(z)


def operator_from_fit(X, theta, kernel, m, f_map):
    """(alpha, A) on the host from the design and f_MAP alone, as pairs_numpy.operator_from_fit: Sigma^-1 by the oracle's
    inverse of the shrunk Gramian (direct differences), P and A by the oracle."""
    from oracle import ppbo_oracle as orc
    S = orc.regularize_covariance(cross(X, X, theta, kernel), orc.SHRINKAGE)
    Sinv = orc.pd_inverse(S)
    P = orc.posterior_covariance(Sinv, f_map, m, float(theta[0]))
    return Sinv @ np.asarray(f_map, dtype=float), orc.variance_operator(Sinv, P, True)
