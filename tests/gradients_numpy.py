"""NumPy statement of the gradient's posterior (ppbo_predict_gradients, Engine.predict_gradients, GPModel.gradient_pred)
-- test infrastructure only, no device input.  For a point x, with the D columns

    g_d = d k(x, X) / d x_d = slopes_numpy.slope_column(x, e_d)          (analytic, from direct differences)

    grad f(x) ~ N(m, C),     m_d = g_d' alpha,     C_de = P_de - g_d' A g_e,     P = diag(slopes_numpy.slope_prior(e_d))

with (alpha, A) of slopes_numpy.operator_from_fit and A symmetrised, (A + A') / 2 (the oracle's A is asymmetric at about
3e-10, and the device's operator is symmetric by construction).  The slope statement of tests/slopes_numpy.py -- held to
central differences in tests/test_slopes_host.py -- is its projection: xi' m = mu_s and xi' C xi = var_s.

Beside it the two consumers: the delta-method covariance of the optimum, H^-1 C H^-1, and the active-subspace matrix
mean_i(m_i m_i' + C_i)."""
from __future__ import annotations

import numpy as np

import slopes_numpy as sn


def gradient_columns(Xq, X, theta, kernel):
    """g [M, D, N]: g[i, d, j] = d k(Xq[i], X[j]) / d x_d."""
    Xq = np.atleast_2d(np.asarray(Xq, dtype=float))
    M, D = Xq.shape
    E = np.eye(D)
    return np.stack([sn.slope_column(Xq, np.tile(E[d], (M, 1)), X, theta, kernel) for d in range(D)], axis=1)


def prior_diagonal(theta, kernel, D):
    """The diagonal [D] of the unshrunk prior (d^2 k / dx dx')(x, x); its off-diagonal entries are zero."""
    return sn.slope_prior(np.eye(D), theta, kernel)


def gradient_reference(Xq, X, theta, kernel, alpha, A):
    """(m [M, D], C [M, D, D], g [M, D, N]): g is returned for the error measures (sum_j |g_jd alpha_j|)."""
    g = gradient_columns(Xq, X, theta, kernel)
    As = 0.5 * (np.asarray(A, dtype=float) + np.asarray(A, dtype=float).T)
    m = g @ np.asarray(alpha, dtype=float)
    C = np.diag(prior_diagonal(theta, kernel, g.shape[1]))[None, :, :] - np.einsum("idj,jk,iek->ide", g, As, g)
    return m, C, g


def mean_scale(g, alpha):
    """sum_j |g_jd alpha_j| [M, D]: what the mean of a gradient entry cancels down from."""
    return np.abs(g) @ np.abs(np.asarray(alpha, dtype=float))


def cov_scale(theta, kernel, D):
    """sqrt(P_dd P_ee) [D, D]: what a covariance entry cancels down from."""
    p = prior_diagonal(theta, kernel, D)
    return np.sqrt(np.outer(p, p))


def xstar_covariance(H, C):
    """The delta method: x* ~ N(x, H^-1 C H^-1) for the mean Hessian H and the gradient's covariance C at the peak."""
    return np.linalg.solve(H, np.linalg.solve(H, C).T)


def active_matrix(m, C):
    """E_x[grad f grad f'] over the given points: mean_i(m_i m_i' + C_i) [D, D]."""
    m, C = np.asarray(m, dtype=float), np.asarray(C, dtype=float)
    return (m[:, :, None] * m[:, None, :] + C).mean(axis=0)


RIDGE = dict(D=4, n_q=64, m=3, seed=1, theta=[1.0, 0.3 * np.sqrt(4 / 6.0), 0.7], kernel="SE_kernel")


def ridge_design(D=RIDGE["D"], n_q=RIDGE["n_q"], m=RIDGE["m"], seed=RIDGE["seed"]):
    """(X [n_q (m + 1), D], u): a star design that varies in ONE rotated direction only -- every row is c + t u with c the
    centre of the box, u a random unit vector and t uniform on the segment inside the box; the chosen row of a star (its
    first) is the one nearest the peak at t = 0.1 t_max.  The prior of a gradient is isotropic and data only remove
    variance along u, so u leads the active subspace only where the squared mean slope outweighs that loss: with the
    parameters of RIDGE (noise 1.0 against sigma_f = 0.7, 64 stars) the NumPy statement puts the leading eigenvector of
    mean_i(m_i m_i' + C_i) over 256 uniform points at 4.2 degrees from u, eigenvalues 10.29 against 8.99 (checked in
    tests/test_gradients_host.py)."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(D)
    u /= np.linalg.norm(u)
    tmax = 0.45 / np.abs(u).max()
    rows = []
    for _ in range(n_q):
        t = rng.uniform(-tmax, tmax, m + 1)
        t = t[np.argsort(np.abs(t - 0.1 * tmax))]
        rows += [0.5 + ti * u for ti in t]
    return np.array(rows), u


def ridge_points(D=RIDGE["D"], M=256):
    return np.random.default_rng(5).random((M, D))


def angle_degrees(v, u):
    return float(np.degrees(np.arccos(min(1.0, abs(float(np.dot(v, u))) / (np.linalg.norm(v) * np.linalg.norm(u))))))


def active_subspace(m, C):
    """(eigenvalues, eigenvectors as rows) of active_matrix, largest first."""
    A = active_matrix(m, C)
    w, V = np.linalg.eigh(0.5 * (A + A.T))
    order = np.argsort(w)[::-1]
    return w[order], V[:, order].T
