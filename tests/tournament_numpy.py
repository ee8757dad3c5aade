"""NumPy statement of a tournament under the Laplace posterior (ppbo_predict_tournament, GPModel.tournament_pred) -- test
infrastructure only.  With (alpha, A) of pairs_numpy.operator_from_fit, k_a = k(a, X) and k_b = k(b, X):

    mu(x) = k_x' alpha,   var(x) = sf^2 - k_x' A k_x,   cov(a, b) = k(a, b) - k_a' A k_b,
    var_d(a, b) = var_a + var_b - 2 cov(a, b),   p(a > b) = preference_probability(mu_a - mu_b, var_d, sigma)

Every kernel value comes from direct differences (pairs_numpy.cross / pathwise_numpy.kernel_matrix)."""
from __future__ import annotations

import numpy as np

import pairs_numpy as pn
import pathwise_numpy as pw  # noqa: F401  (the radial kernels behind pairs_numpy.cross)

BORDA, WORST = 0, 1


def tournament_reference(Xa, Xb, X, theta, kernel, alpha, A, cross=pn.cross):
    """dict(mu_a, var_a [Ma], mu_b, var_b [Mb], cov, var_d [Ma, Mb]) of every a_i against every b_j.  cross(Xq, X, theta,
    kernel) -> k [len(Xq), len(X)]: pairs_numpy.cross, or slopes_numpy.cross for the per-coordinate camphor kernel."""
    Xa, Xb = np.atleast_2d(np.asarray(Xa, dtype=float)), np.atleast_2d(np.asarray(Xb, dtype=float))
    alpha, A = np.asarray(alpha, dtype=float), np.asarray(A, dtype=float)
    sf2 = float(theta[2]) ** 2
    Ka, Kb = cross(Xa, X, theta, kernel), cross(Xb, X, theta, kernel)                # [Ma, N], [Mb, N]
    AKb = A @ Kb.T                                                                    # [N, Mb]
    var_a = sf2 - np.einsum("ij,ij->i", Ka, Ka @ A)
    var_b = sf2 - np.einsum("ij,ji->i", Kb, AKb)
    cov = cross(Xa, Xb, theta, kernel) - Ka @ AKb
    return dict(mu_a=Ka @ alpha, var_a=var_a, mu_b=Kb @ alpha, var_b=var_b, cov=cov,
                var_d=var_a[:, None] + var_b[None, :] - 2.0 * cov)


def win_matrix(ref, sigma):
    """p0 [Ma, Mb] of a tournament_reference by misc.preference_probability."""
    from ppbo_amd.misc import preference_probability
    return preference_probability(ref["mu_a"][:, None] - ref["mu_b"][None, :], ref["var_d"], sigma)


def scores(prob, kind=BORDA):
    """The row reductions: BORDA the mean of a row (summed in index order), WORST its minimum; NaN propagates in both."""
    prob = np.atleast_2d(np.asarray(prob, dtype=float))
    if kind == BORDA:
        s = np.zeros(prob.shape[0])
        for j in range(prob.shape[1]):
            s = s + prob[:, j]
        return s / prob.shape[1]
    if kind == WORST:
        return prob.min(axis=1)
    raise ValueError(f"unknown score kind {kind}")


def best(score):
    """(largest score, its first index); NaN never wins; (nan, -1) when nothing scored."""
    score = np.asarray(score, dtype=float)
    ok = ~np.isnan(score)
    if not ok.any():
        return float("nan"), -1
    i = int(np.argmax(np.where(ok, score, -np.inf)))
    return float(score[i]), i
