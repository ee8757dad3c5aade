"""NumPy statement of a curvature under the Laplace posterior (ppbo_predict_curvatures, GPModel.curvature_pred) -- test
infrastructure only, no device input.  For a path gamma with gamma(0) = x, gamma'(0) = xi, gamma''(0) = acc (a straight
line: acc = 0), with the column

    c_j = d^2/da^2 k(gamma(a), x_j) at a = 0

    mu_c = c' alpha,     var_c = prior - c' A c,     A = Sigma^-1 - Sigma^-1 P Sigma^-1  (oracle.variance_operator)
    prior = Var[d^2/da^2 f(gamma(a))],     p = P(curvature < 0) = Phi(-mu_c / sqrt(max(var_c, 0)))

the dense form tests/slopes_numpy.py uses for slopes.  Every derivative is analytic, from direct differences:

    radial kernels (scalar or per-dimension length scales l_d), k = sf^2 kappa(rho^2), rho^2 = sum_d ((x_d - x_jd) / l_d)^2,
    b_j = sum_d (x_d - x_jd) xi_d / l_d^2, n2 = sum_d (xi_d / l_d)^2:
        c_j = sf^2 (4 kappa''(rho_j^2) b_j^2 + 2 kappa'(rho_j^2) (n2 + sum_d (x_d - x_jd) acc_d / l_d^2))
        prior = 12 kappa''(0) sf^2 n2^2 - 2 kappa'(0) sf^2 sum_d (acc_d / l_d)^2
        (12 kappa''(0) = 3 (SE), 9/2 (RQ), 25 (Matern-5/2); Matern-3/2 has no kappa''(0): refused)
    camphor-copper in the caller's six coordinates (six length scales l_d; the scalar-l kernel is the profile
    (l, l, l + 0.05, l, l, l)), k = sf^2 e^-s, s = sum_{d != 2} 2 sin^2(pi D_d) / l_d^2 + D_2^2 / (2 l_2^2), D = x - x_j,
    straight lines only:
        c_j = k_j ((ds_j/da)^2 - d^2 s_j/da^2),     ds_j/da as slopes_numpy,
        d^2 s_j/da^2 = sum_{d != 2} (4 pi^2 / l_d^2) cos(2 pi D_d) xi_d^2 + xi_2^2 / l_2^2
        prior = sf^2 (12 A^2 + 16 pi^4 sum_{d != 2} xi_d^4 / l_d^2),   A = sum_{d != 2} 2 pi^2 xi_d^2 / l_d^2 + xi_2^2 / (2 l_2^2)
        (s(t xi) = A t^2 - sum_{d != 2} (2 pi^4 xi_d^4 / (3 l_d^2)) t^4 + ..., and the prior is the fourth derivative of
        e^-s at 0)

tests/test_curvature_host.py confirms the column by central differences of slopes_numpy.slope_column and the prior by
second central differences of the column in the design point; the six-coordinate camphor form does not know the
eleven-column embedding, so it is the check of the acceleration path."""
from __future__ import annotations

import numpy as np

from evgrad_numpy import kappa
from slopes_numpy import CAMPHOR, CAMPHOR_ARD, PERIODIC, _ls, camphor_ls, cross, operator_from_fit, slope_probability  # noqa: F401


def kappa2(r2, kernel):
    """kappa''(rho^2) = d^2 kappa / d(rho^2)^2 of SE, RQ (alpha = 2) and Matern-5/2."""
    if kernel == "SE_kernel":
        return 0.25 * np.exp(-0.5 * r2)
    if kernel == "RQ_kernel":
        return 0.375 * (1.0 + r2 / 4.0) ** -4
    if kernel == "Matern52_kernel":
        return (25.0 / 12.0) * np.exp(-np.sqrt(5.0 * r2))
    raise ValueError(f"no curvature for {kernel}")


def curvature_column(Xq, Xi, X, theta, kernel, Xa=None):
    """c [M, N]: c[i, j] = d^2/da^2 k(gamma_i(a), X[j]) at a = 0, gamma_i(a) = Xq[i] + a Xi[i] + a^2 Xa[i] / 2."""
    Xq, Xi, X = (np.atleast_2d(np.asarray(a, dtype=float)) for a in (Xq, Xi, X))
    sf2 = float(theta[2]) ** 2
    d = Xq[:, None, :] - X[None, :, :]
    if kernel in (CAMPHOR, CAMPHOR_ARD):
        if Xa is not None:
            raise ValueError("camphor-copper in six coordinates: straight lines only")
        l = camphor_ls(theta)
        ds = d[:, :, 2] * Xi[:, None, 2] / l[2] ** 2
        d2s = np.broadcast_to((Xi[:, None, 2] / l[2]) ** 2, ds.shape).copy()
        for k in PERIODIC:
            ds = ds + (2.0 * np.pi / l[k] ** 2) * np.sin(2.0 * np.pi * d[:, :, k]) * Xi[:, None, k]
            d2s = d2s + (4.0 * np.pi ** 2 / l[k] ** 2) * np.cos(2.0 * np.pi * d[:, :, k]) * Xi[:, None, k] ** 2
        return cross(Xq, X, theta, kernel) * (ds * ds - d2s)
    l = _ls(theta, Xq.shape[1])
    r2 = ((d / l) ** 2).sum(axis=2)
    b = (d * (Xi / l ** 2)[:, None, :]).sum(axis=2)
    n2 = ((Xi / l) ** 2).sum(axis=1)[:, None]
    if Xa is not None:
        n2 = n2 + (d * (np.atleast_2d(np.asarray(Xa, dtype=float)) / l ** 2)[:, None, :]).sum(axis=2)
    return sf2 * (4.0 * kappa2(r2, kernel) * b * b + 2.0 * kappa(r2, kernel)[1] * n2)


def curvature_prior(Xi, theta, kernel, Xa=None):
    """Var[d^2/da^2 f(gamma(a))] at a = 0 under the prior [M] (the kernels are stationary: no x, no cross term)."""
    Xi = np.atleast_2d(np.asarray(Xi, dtype=float))
    sf2 = float(theta[2]) ** 2
    if kernel in (CAMPHOR, CAMPHOR_ARD):
        if Xa is not None:
            raise ValueError("camphor-copper in six coordinates: straight lines only")
        l = camphor_ls(theta)
        per = list(PERIODIC)
        A = (2.0 * np.pi ** 2 * Xi[:, per] ** 2 / l[per] ** 2).sum(axis=1) + 0.5 * (Xi[:, 2] / l[2]) ** 2
        return sf2 * (12.0 * A * A + 16.0 * np.pi ** 4 * (Xi[:, per] ** 4 / l[per] ** 2).sum(axis=1))
    l = _ls(theta, Xi.shape[1])
    n2 = ((Xi / l) ** 2).sum(axis=1)
    out = 12.0 * float(kappa2(np.zeros(1), kernel)[0]) * sf2 * n2 * n2
    if Xa is not None:
        out = out - 2.0 * float(kappa(np.zeros(1), kernel)[1][0]) * sf2 * ((np.atleast_2d(np.asarray(Xa, dtype=float)) / l) ** 2).sum(axis=1)
    return out


def curvature_reference(Xq, Xi, X, theta, kernel, alpha, A, Xa=None):
    """(mu_c, var_c, c) of the rows (Xq[i], Xi[i][, Xa[i]]): c is returned for the error measures (sum_j |c_j alpha_j|)."""
    c = curvature_column(Xq, Xi, X, theta, kernel, Xa)
    mu = c @ np.asarray(alpha, dtype=float)
    var = curvature_prior(Xi, theta, kernel, Xa) - np.einsum("ij,ij->i", c, c @ A)
    return mu, var, c


def curvature_probability(mu_c, var_c):
    """P(curvature < 0) = Phi(-mu_c / sqrt(max(var_c, 0))): no noise term; without variance the sign of mu_c decides and
    mu_c = 0 gives 1/2; NaN in, NaN out."""
    return slope_probability(-np.asarray(mu_c, dtype=float), var_c)
