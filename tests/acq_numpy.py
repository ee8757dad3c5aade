"""NumPy statement of the acquisition gradients (ppbo_acq_grad, ppbo_acq_ascent, GPModel.acquisition_grad) -- test
infrastructure only, no device input.  For a point x, with the column k = k(x, X) and its Jacobian J = dk/dx [N, D]:

    mu = k' alpha,           grad mu  = J' alpha
    var = sf^2 - k' A k,     grad var = 2 J' u,   u = -A k        A = Sigma^-1 - Sigma^-1 P Sigma^-1 (oracle.variance_operator)

(-A is the Lambda + M'M of the device, so u is its adjoint column), and the score of ppbo_predict with its gradient:

    MEAN       mu                                                  grad mu
    VARIANCE   var                                                 grad var
    EI         d Phi(z) + sd phi(z), d = mu - mu*, z = d / sd      Phi(z) grad mu + phi(z) grad var / (2 sd)
               sd = sqrt(max(var, 0)) > 0;   sd = 0: max(d, 0)     grad mu where d > 0, else 0

Every derivative is analytic, from direct differences (the Jacobians are those of tests/slopes_numpy.slope_column, before
the contraction with a direction):

    radial kernels (scalar or per-dimension l_d), k = sf^2 kappa(rho^2):   J_jd = 2 sf^2 kappa'(rho_j^2) (x_d - x_jd) / l_d^2
    camphor-copper (six l_d; scalar l = the profile (l, l, l + 0.05, l, l, l)):
        J_jd = -k_j (2 pi / l_d^2) sin(2 pi (x_d - x_jd)) for a periodic d,   -k_j (x_2 - x_j2) / l_2^2 for d = 2

tests/test_acq_host.py confirms mu, var, the score and the three gradients by central differences."""
from __future__ import annotations

import numpy as np
from scipy.special import ndtr

import slopes_numpy as sn
from evgrad_numpy import kappa

MEAN, EI, VARIANCE = 0, 1, 2          # PPBO_SCORE_MEAN, PPBO_SCORE_POINTWISE_EI, PPBO_SCORE_VARIANCE
INV_SQRT_2PI = 0.3989422804014327


def jacobian(Xq, X, theta, kernel):
    """J [M, N, D]: J[i, j, d] = d k(Xq[i], X[j]) / d x_d."""
    Xq, X = np.atleast_2d(np.asarray(Xq, dtype=float)), np.atleast_2d(np.asarray(X, dtype=float))
    sf2 = float(theta[2]) ** 2
    d = Xq[:, None, :] - X[None, :, :]
    if kernel in (sn.CAMPHOR, sn.CAMPHOR_ARD):
        l = sn.camphor_ls(theta)
        fac = (2.0 * np.pi / l ** 2) * np.sin(2.0 * np.pi * d)
        fac[:, :, 2] = d[:, :, 2] / l[2] ** 2
        return -sn.cross(Xq, X, theta, kernel)[:, :, None] * fac
    l = sn._ls(theta, Xq.shape[1])
    r2 = ((d / l) ** 2).sum(axis=2)
    return (2.0 * sf2 * kappa(r2, kernel)[1])[:, :, None] * (d / l ** 2)


def score_value(mu, var, kind, mustar=0.0):
    """score_value of csrc/score.h on arrays."""
    mu, var = np.asarray(mu, dtype=float), np.asarray(var, dtype=float)
    if kind == MEAN:
        return mu.copy()
    if kind == VARIANCE:
        return np.where(np.isnan(mu), mu, var)
    d, sd = mu - mustar, np.sqrt(np.maximum(var, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = d / sd
        ei = d * ndtr(z) + sd * INV_SQRT_2PI * np.exp(-0.5 * z * z)
    return np.where(np.isnan(mu), mu, np.where(sd > 0.0, ei, np.maximum(d, 0.0)))


def score_weights(mu, var, kind, mustar=0.0):
    """(a, b) with grad score = a grad mu + b grad var."""
    mu, var = np.asarray(mu, dtype=float), np.asarray(var, dtype=float)
    if kind == MEAN:
        return np.ones_like(mu), np.zeros_like(mu)
    if kind == VARIANCE:
        return np.zeros_like(mu), np.ones_like(mu)
    d, sd = mu - mustar, np.sqrt(np.maximum(var, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = d / sd
        a, b = ndtr(z), INV_SQRT_2PI * np.exp(-0.5 * z * z) / (2.0 * sd)
    pos = sd > 0.0
    return np.where(pos, a, (d > 0.0).astype(float)), np.where(pos, b, 0.0)


def acq_reference(Xq, X, theta, kernel, alpha, A, kind=EI, mustar=0.0):
    """dict(mu, var, score [M], grad_mu, grad_var, grad_score [M, D]) and the sums of absolute terms the device's results
    are held against: abs_mu = sum_j |k_j alpha_j| [M], abs_gmu[i, d] = sum_j |J_jd alpha_j|, abs_gvar[i, d] =
    2 sum_j |J_jd| |u_j|."""
    alpha, A = np.asarray(alpha, dtype=float), np.asarray(A, dtype=float)
    k = sn.cross(Xq, X, theta, kernel)
    J = jacobian(Xq, X, theta, kernel)
    u = -(k @ A)
    mu = k @ alpha
    var = float(theta[2]) ** 2 + np.einsum("ij,ij->i", k, u)
    gmu = np.einsum("ijd,j->id", J, alpha)
    gvar = 2.0 * np.einsum("ijd,ij->id", J, u)
    a, b = score_weights(mu, var, kind, mustar)
    return dict(mu=mu, var=var, score=score_value(mu, var, kind, mustar), grad_mu=gmu, grad_var=gvar,
                grad_score=a[:, None] * gmu + b[:, None] * gvar, u=u, abs_mu=np.abs(k) @ np.abs(alpha),
                abs_gmu=np.einsum("ijd,j->id", np.abs(J), np.abs(alpha)),
                abs_gvar=2.0 * np.einsum("ijd,ij->id", np.abs(J), np.abs(u)))


def acq_fg(X, theta, kernel, alpha, A, kind, mustar):
    """fg(x) -> (score, grad score) of one point: the objective of tests/box_search_numpy.bb_ascent_box."""
    def f(x):
        r = acq_reference(np.asarray(x, dtype=float)[None, :], X, theta, kernel, alpha, A, kind, mustar)
        return float(r["score"][0]), r["grad_score"][0]
    return f


# ---------------------------------------------------------------------------------------------- the ascent comparison
# The cases of the step-by-step comparison of ppbo_acq_ascent (tests/test_gpu_acq.py) and of its pre-check on the
# reference alone (tests/test_acq_host.py): (kernel, D, n_q, m) of a tests/test_gpu_slopes._fitted model, the score kind,
# a box of tests/box_search_numpy.boxes and the seed of the 24 starts.
ASCENT_CASES = {
    "SE-6-EI-unit": ("SE_kernel", 6, 8, 3, EI, "unit", 1),
    "SE-6-variance-fixed3": ("SE_kernel", 6, 8, 3, VARIANCE, "fixed3", 2),
    "SE-20-EI-inner": ("SE_kernel", 20, 3, 25, EI, "inner", 3),
    "SE-20-variance-unit": ("SE_kernel", 20, 3, 25, VARIANCE, "unit", 4),
}


def ascent_design(case):
    """(X, theta, kernel, m): the design and theta tests/test_gpu_slopes._fitted gives the case's model (the same
    generator, the same draws)."""
    from test_gpu_slopes import RADIAL, _star_design
    kernel, D, n_q, m = ASCENT_CASES[case][:4]
    rng = np.random.default_rng(1000 * D + 10 * n_q + m + 7 * RADIAL.index(kernel))
    return _star_design(rng, n_q, D, m), [0.05, 0.3 * np.sqrt(D / 6.0), 0.7], kernel, m


def ascent_setup(case):
    """(kind, lo, hi, starts [24, D]) of a case: search_ref.ascent_starts (interior, outside, on faces, corners)."""
    import box_search_numpy as bsn
    import search_ref as sr
    _, D, _, _, kind, box, seed = ASCENT_CASES[case]
    lo, hi = bsn.boxes(D)[box]
    return kind, lo, hi, sr.ascent_starts(D, seed)


def best_design_mean(X, theta, kernel, alpha):
    """mu* of the tests: the largest posterior mean over the design rows."""
    return float((sn.cross(X, X, theta, kernel) @ np.asarray(alpha, dtype=float)).max())
