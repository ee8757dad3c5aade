"""NumPy statement of a duel under the Laplace posterior (ppbo_predict_pairs, GPModel.preference_pred) -- test
infrastructure only.  With d = k(a, X) - k(b, X):

    mu_d = d' alpha,     var_d = 2 sf^2 - 2 k(a, b) - d' A d,     A = Sigma^-1 - Sigma^-1 P Sigma^-1  (oracle.variance_operator)

Every kernel value comes from direct differences (the radial families through pathwise_numpy.kernel_matrix, scalar or
per-dimension length scales; the camphor-copper kernel is the oracle's, which is written on differences)."""
from __future__ import annotations

import numpy as np

import pathwise_numpy as pw
from evgrad_numpy import kappa
from oracle import ppbo_oracle as orc

CAMPHOR = "camphor_copper_kernel"


def cross(Xq, X, theta, kernel):
    """k(x_c, x_i) [M, N] from direct differences."""
    if kernel == CAMPHOR:
        return orc.camphor_copper_kernel(np.asarray(Xq, dtype=float), np.asarray(X, dtype=float), theta)
    return pw.kernel_matrix(Xq, X, theta, kernel)[0]


def pair_kernel(Xa, Xb, theta, kernel):
    """k(a_i, b_i) [M] from the direct differences a_i - b_i."""
    Xa, Xb = np.atleast_2d(np.asarray(Xa, dtype=float)), np.atleast_2d(np.asarray(Xb, dtype=float))
    sf2 = float(theta[2]) ** 2
    if kernel == CAMPHOR:
        l = float(theta[1])
        ad = np.abs(Xa - Xb)
        e = sum(2.0 * np.sin(np.pi * ad[:, k]) ** 2 / l ** 2 for k in (0, 1, 3, 4, 5)) + 0.5 * ad[:, 2] ** 2 / (l + 0.05) ** 2
        return sf2 * np.exp(-e)
    d = (Xa - Xb) / np.broadcast_to(np.asarray(theta[1], dtype=float), (Xa.shape[1],))
    return sf2 * kappa((d * d).sum(axis=1), kernel)[0]


def operator_from_fit(X, theta, kernel, m, f_map):
    """(alpha, A) on the host from the design and f_MAP alone: Sigma^-1 by the oracle's inverse of the shrunk Gramian
    (direct differences), P and A by the oracle -- nothing of the device's inverse or operator enters."""
    S = orc.regularize_covariance(cross(X, X, theta, kernel), orc.SHRINKAGE)
    Sinv = orc.pd_inverse(S)
    P = orc.posterior_covariance(Sinv, f_map, m, float(theta[0]))
    return Sinv @ np.asarray(f_map, dtype=float), orc.variance_operator(Sinv, P, True)


def pair_reference(Xa, Xb, X, theta, kernel, alpha, A):
    """(mu_d, var_d) [M] of the duels (Xa[i], Xb[i])."""
    d = cross(Xa, X, theta, kernel) - cross(Xb, X, theta, kernel)            # [M, N]
    mu = d @ np.asarray(alpha, dtype=float)
    var = 2.0 * float(theta[2]) ** 2 - 2.0 * pair_kernel(Xa, Xb, theta, kernel) - np.einsum("ij,ij->i", d, d @ A)
    return mu, var
