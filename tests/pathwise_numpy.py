"""NumPy restatement of pathwise (decoupled) posterior sampling on the Laplace posterior (DESIGN.md 7,
Hsampler.sample_paths, ppbo_path_score_multi / ppbo_path_search_multi) -- test infrastructure only.

    g_s(x) = phi(x)^T w_s + k(x, X) v_s,     v_s = Sigma^-1 (f_s - Phi(X)^T w_s),     f_s = f_MAP + L z_s,  L L^T = P

The kernels are written out here from direct differences of x / l (the four radial families, scalar or per-dimension
length scales); Phi is [F, N] as the sampler stores it, Phi[f, n] = sqrt(2 sf^2 / F) cos(w_f . x_n + b_f)."""
from __future__ import annotations

import numpy as np

from evgrad_numpy import kappa

KERNELS = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")


def _ls(theta, D):
    return np.broadcast_to(np.asarray(theta[1], dtype=float), (D,)).astype(float)


def kernel_matrix(A, B, theta, kernel):
    """k(a_i, b_j) [len(A), len(B)] and the scaled differences (a_i - b_j) / l [len(A), len(B), D]."""
    A, B = np.atleast_2d(np.asarray(A, dtype=float)), np.atleast_2d(np.asarray(B, dtype=float))
    l = _ls(theta, A.shape[1])
    d = A[:, None, :] / l - B[None, :, :] / l
    k, _ = kappa((d * d).sum(axis=2), kernel)
    return float(theta[2]) ** 2 * k, d


def features(Xq, W, b, sigma_f):
    """Phi(Xq) [F, M]."""
    Xq = np.atleast_2d(np.asarray(Xq, dtype=float))
    W = np.asarray(W, dtype=float)
    return np.sqrt(2.0 * float(sigma_f) ** 2 / W.shape[0]) * np.cos(W @ Xq.T + np.asarray(b, dtype=float).ravel()[:, None])


def assemble(z, w, f_map, L, Phi, Sigma_inv):
    """(F_s [S, N], V [S, N]) from given normals z [S, N] and prior weights w [S, F]: f_s = f_MAP + L z_s,
    v_s = Sigma^-1 (f_s - Phi^T w_s) (Sigma^-1 symmetric)."""
    Fs = np.asarray(f_map, dtype=float)[None, :] + np.asarray(z, dtype=float) @ np.asarray(L, dtype=float).T
    return Fs, (Fs - np.asarray(w, dtype=float) @ Phi) @ Sigma_inv


def paths(Xq, w, V, W, b, X, theta, kernel):
    """g_s(x_c) [S, M]."""
    K, _ = kernel_matrix(Xq, X, theta, kernel)
    return np.atleast_2d(w) @ features(Xq, W, b, theta[2]) + np.atleast_2d(V) @ K.T


def paths_abs(Xq, w, V, W, b, X, theta, kernel):
    """sum_f |w_sf phi_f(x_c)| + sum_i |v_si| k(x_c, x_i) [S, M]: the scale rounding errors of g_s are measured against
    (k v cancels heavily when |v| is large)."""
    K, _ = kernel_matrix(Xq, X, theta, kernel)
    return np.abs(np.atleast_2d(w)) @ np.abs(features(Xq, W, b, theta[2])) + np.abs(np.atleast_2d(V)) @ K.T


def path_grad(x, w, v, W, b, X, theta, kernel):
    """d g_s / d x [D] of one path (w [F], v [N]) at one point x [D]."""
    x = np.asarray(x, dtype=float).ravel()
    W = np.asarray(W, dtype=float)
    F, D = W.shape
    l = _ls(theta, D)
    amp = np.sqrt(2.0 * float(theta[2]) ** 2 / F)
    gf = -amp * (np.sin(W @ x + np.asarray(b, dtype=float).ravel()) * np.asarray(w, dtype=float)) @ W
    d = (x[None, :] - np.asarray(X, dtype=float)) / l                    # [N, D]
    _, dk = kappa((d * d).sum(axis=1), kernel)                           # d kappa / d rho^2
    gk = (2.0 * float(theta[2]) ** 2 * (np.asarray(v, dtype=float) * dk)) @ (d / l)
    return gf + gk


def path_cov(Xq, W, b, X, theta, kernel, Sigma_inv, P, Phi=None):
    """The closed-form covariance of g_s for THIS basis, C(x, x') = r(x)^T r(x') + k(x, X) Sigma^-1 P Sigma^-1 k(X, x'),
    r(x) = phi(x) - Phi(X) Sigma^-1 k(X, x): [M, M].  The mean is path_mean."""
    K, _ = kernel_matrix(Xq, X, theta, kernel)                           # [M, N]
    Phi = features(X, W, b, theta[2]) if Phi is None else Phi
    B = Sigma_inv @ K.T                                                  # [N, M]
    R = features(Xq, W, b, theta[2]) - Phi @ B                           # [F, M]
    return R.T @ R + B.T @ P @ B


def path_var(Xq, W, b, X, theta, kernel, Sigma_inv, P, Phi=None):
    """diag of path_cov without forming the [M, M] matrix."""
    K, _ = kernel_matrix(Xq, X, theta, kernel)
    Phi = features(X, W, b, theta[2]) if Phi is None else Phi
    B = Sigma_inv @ K.T
    R = features(Xq, W, b, theta[2]) - Phi @ B
    return (R * R).sum(axis=0) + (B * (P @ B)).sum(axis=0)


def path_mean(Xq, X, theta, kernel, Sigma_inv, f_map):
    """E g_s(x) = k(x, X) Sigma^-1 f_MAP (the prior halves cancel in expectation): the GP posterior mean."""
    K, _ = kernel_matrix(Xq, X, theta, kernel)
    return K @ (Sigma_inv @ np.asarray(f_map, dtype=float))


def gp_var(Xq, X, theta, kernel, Sigma_inv, P):
    """The GP posterior variance k(x, x) - k(x, X) (Sigma^-1 - Sigma^-1 P Sigma^-1) k(X, x) (what C tends to as F grows)."""
    K, _ = kernel_matrix(Xq, X, theta, kernel)
    B = Sigma_inv @ K.T
    return float(theta[2]) ** 2 - (K.T * B).sum(axis=0) + (B * (P @ B)).sum(axis=0)
