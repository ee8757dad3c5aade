"""NumPy restatement of the Laplace-evidence gradient (ppbo_evidence_grad) -- test infrastructure only.

The objective is the reference's evidence with its quirks (src/gp_model.py:278-319, oracle.ppbo_oracle.evidence):
E = T(f) - 1/2 s_U log|det A| + log p(theta), A = I + Sigma Lambda(f), s_U = prod sign(u_kk) of A's LU with LAPACK's
pivoting, sigma fixed.  Kernels are written out here (the oracle has no Matern and no per-dimension length scales); the
Gram matrix goes through the oracle's shrink."""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg

from oracle import ppbo_oracle as orc

SHRINK = 1e-6
_PRIOR_L = (0.5, -1.4)          # lognormal (s, log scale) of each length scale (src/gp_model.py:287-290)
_PRIOR_SF = (0.5, 1.7)          # ... of sigma_f


def _ls(theta, D):
    return np.broadcast_to(np.asarray(theta[1], dtype=float), (D,)).astype(float)


def kappa(r2, kernel):
    """kappa(rho^2) and kappa'(rho^2) = d kappa / d rho^2 of the four radial kernels (RQ: alpha = 2)."""
    if kernel == "SE_kernel":
        k = np.exp(-0.5 * r2)
        return k, -0.5 * k
    if kernel == "RQ_kernel":
        t = 1.0 + r2 / 4.0
        return t ** -2, -0.5 * t ** -3
    if kernel == "Matern52_kernel":
        a = np.sqrt(5.0 * r2)
        e = np.exp(-a)
        return (1.0 + a + a * a / 3.0) * e, -(5.0 / 6.0) * (1.0 + a) * e
    if kernel == "Matern32_kernel":
        a = np.sqrt(3.0 * r2)
        e = np.exp(-a)
        return (1.0 + a) * e, -1.5 * e
    raise ValueError(kernel)


def sigma_matrix(X, theta, kernel):
    """Sigma = (1 - eps) K + eps tr(K)/N I (the reference's shrink), K from direct differences of X / l."""
    Xs = X / _ls(theta, X.shape[1])
    r2 = orc.sqdist_direct(Xs, Xs)
    K = float(theta[2]) ** 2 * kappa(r2, kernel)[0]
    return orc.regularize_covariance(K, SHRINK)


def log_prior(theta):
    l = np.atleast_1d(np.asarray(theta[1], dtype=float))
    def lognorm(x, s, mu):
        return -np.log(x) - math.log(s * math.sqrt(2.0 * math.pi)) - (np.log(x) - mu) ** 2 / (2.0 * s * s)
    return float(lognorm(float(theta[0]), 1.0, 1.0) + np.sum(lognorm(l, *_PRIOR_L)) + lognorm(float(theta[2]), *_PRIOR_SF))


def log_prior_grad(theta):
    """d log p / d (l, sigma_f): each lognormal term gives -(1 + (ln x - ln scale) / s^2) / x."""
    l = np.asarray(theta[1], dtype=float)
    gl = -(1.0 + (np.log(l) - _PRIOR_L[1]) / _PRIOR_L[0] ** 2) / l
    sf = float(theta[2])
    gsf = -(1.0 + (math.log(sf) - _PRIOR_SF[1]) / _PRIOR_SF[0] ** 2) / sf
    return np.append(np.ravel(gl), gsf)


def slogdet_lu(A):
    """(s_U, sum log|u_kk|, sign det A) with scipy's LU (LAPACK getrf pivoting)."""
    _, _, U = scipy.linalg.lu(A)
    du = np.diag(U)
    return float(np.prod(np.sign(du))), float(np.sum(np.log(np.abs(du)))), float(np.sign(np.linalg.det(A)))


def evidence_value(X, theta, kernel, m, f):
    """E at a given f (no fit): T(f) - 1/2 s_U log|det A| + log p."""
    Sig = sigma_matrix(X, theta, kernel)
    Sinv = np.linalg.inv(Sig)
    Lam = orc.lambda_dense(f, m, theta[0])
    sU, ld, _ = slogdet_lu(np.eye(len(f)) + Sig @ Lam)
    return orc.T_value(f, Sinv, m, theta[0]) - 0.5 * sU * ld + log_prior(theta)


def fit(X, theta, kernel, m, f0, gtol=1e-12):
    Sinv = np.linalg.inv(sigma_matrix(X, theta, kernel))
    f, _ = orc.fit_fmap_newton(f0, Sinv, m, theta[0], gtol=gtol, maxiter=500)
    return f


def evidence(X, theta, kernel, m, f0, gtol=1e-12):
    """(E, f_MAP) with f_MAP Newton-converged from f0."""
    f = fit(X, theta, kernel, m, f0, gtol)
    return evidence_value(X, theta, kernel, m, f), f


def evidence_grad(X, theta, kernel, m, f, with_prior=True, sign=None):
    """dE/d(l, sigma_f) at f = f_MAP (l a scalar: one entry; a vector: D entries), and s_U (`sign` replaces s_U)."""
    sigma, sf = float(theta[0]), float(theta[2])
    N, D = X.shape
    l = _ls(theta, D)
    Xs = X / l
    Sig = sigma_matrix(X, theta, kernel)
    Sinv = np.linalg.inv(Sig)
    alpha = Sinv @ f
    Lam = orc.lambda_dense(f, m, sigma)
    A = np.eye(N) + Sig @ Lam
    sU, _, _ = slogdet_lu(A)
    if sign is not None:
        sU = sign
    Ainv = np.linalg.inv(A)
    Z = Lam @ Ainv
    C = Ainv @ Sig
    v = np.zeros(N)
    for q in range(N // (m + 1)):
        i = q * (m + 1)
        for j in range(i + 1, i + m + 1):
            dl = (f[j] - f[i]) / sigma
            hp = orc.var2_normal_pdf(dl) * (1.0 - 0.5 * dl * dl) / (2.0 * m * sigma ** 2)
            t = hp / sigma * (C[i, i] + C[j, j] - C[i, j] - C[j, i])
            v[j] += t
            v[i] -= t
    Q = Sinv - Lam
    w = Sinv @ np.linalg.solve(Q, v)
    W = 0.5 * np.outer(alpha, alpha) - 0.5 * sU * Z - 0.5 * sU * np.outer(w, alpha)
    kp = kappa(orc.sqdist_direct(Xs, Xs), kernel)[1]
    gl = np.empty(D)
    for d in range(D):
        dx2 = (Xs[:, d][:, None] - Xs[:, d][None, :]) ** 2
        gl[d] = np.sum(W * (-2.0 * (1.0 - SHRINK) * sf * sf * kp * dx2 / l[d]))
    if np.ndim(theta[1]) == 0:
        gl = np.array([gl.sum()])
    g = np.append(gl, np.sum(W * (2.0 * Sig / sf)))
    if with_prior:
        g = g + log_prior_grad(theta)
    return g, sU


def with_params(theta, p):
    """theta with (l..., sigma_f) replaced by the flat vector p (scalar l when theta[1] is a scalar)."""
    if np.ndim(theta[1]) == 0:
        return [theta[0], float(p[0]), float(p[-1])]
    return [theta[0], np.asarray(p[:-1], dtype=float), float(p[-1])]


def params(theta):
    return np.append(np.ravel(np.asarray(theta[1], dtype=float)), float(theta[2]))
