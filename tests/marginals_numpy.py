"""NumPy statement of main effects and interactions under the Laplace posterior (ppbo_predict_marginals,
GPModel.marginal_pred) -- test infrastructure only, no device input.

The kernels it covers are products over the unit-box coordinates, k(x, x') = sf^2 prod_d kappa_d(x_d - x'_d):

    an SE axis        kappa_d(D) = exp(-D^2 / (2 l_d^2))
    a periodic axis   kappa_d(D) = exp(-2 sin^2(pi D) / l_d^2)        (the camphor-copper kernel's, every axis but the third)

Per-axis integrals over [0, 1] (a = 1 / l^2, ive the exponentially scaled Bessel function):

    I_d(c) = int kappa_d(u - c) du       l sqrt(pi/2) (erf((1 - c) / (sqrt2 l)) + erf(c / (sqrt2 l)))      | ive(0, a)
    A_d    = int int kappa_d(u - u')     2 (l sqrt(pi/2) erf(1 / (sqrt2 l)) - l^2 (1 - exp(-1 / (2 l^2))))  | ive(0, a)

Per design row j: Q_jd = I_d(x_jd), P_j = sf^2 prod_d Q_jd.  A row of the call keeps the axes J (|J| <= 2) at the values t:
r_d = kappa_d(t_d - x_jd) / Q_jd.  With S = sf^2 prod_{d not in J} A_d, a_d = I_d(t_d), b_d = 1 - 2 a_d + A_d:

    RAW           f_J(t) = int f dx_-J               c_j = P_j prod_J r_d            prior = S
    CENTRED       f_J(t) - fbar                      c_j = P_j (prod_J r_d - 1)      prior = S (1 - 2 prod_J a_d + prod_J A_d)
    INTERACTION   f_de - f_d - f_e + fbar            c_j = P_j (r_d - 1)(r_e - 1)    prior = S b_d b_e

    mu = c' alpha,     var = prior - c' A c,     A = Sigma^-1 - Sigma^-1 P Sigma^-1  (pairs_numpy.operator_from_fit),

formed from the column as tests/functionals_numpy.py forms them.  tests/test_marginals_host.py confirms every ingredient by
tensor Gauss-Legendre quadrature of product_kernel itself."""
from __future__ import annotations

import numpy as np
from scipy.special import erf, ive

import functionals_numpy as fn

RAW, CENTRED, INTERACTION = 0, 1, 2
CAMPHOR = "camphor_copper_kernel"
CAMPHOR_ARD = "camphor_copper_ard_kernel"
CAMPHOR_PERIODIC = np.array([1, 1, 0, 1, 1, 1])


def axes_of(theta, kernel, D):
    """(l [D], periodic [D]) of a product kernel by the project's kernel names; ValueError for the radial ones."""
    if kernel == CAMPHOR:
        return float(theta[1]) + np.array([0.0, 0.0, 0.05, 0.0, 0.0, 0.0]), CAMPHOR_PERIODIC.copy()
    if kernel == CAMPHOR_ARD:
        l = theta[1]
        l = float(l) + np.array([0.0, 0.0, 0.05, 0.0, 0.0, 0.0]) if np.ndim(l) == 0 else np.asarray(l, dtype=float)
        return l, CAMPHOR_PERIODIC.copy()
    if kernel == "SE_kernel":
        return np.broadcast_to(np.asarray(theta[1], dtype=float), (D,)).astype(float), np.zeros(D, dtype=int)
    raise ValueError(f"{kernel} is not a product over coordinates")


def factor(delta, l, periodic):
    """kappa_d at the differences delta."""
    delta = np.asarray(delta, dtype=float)
    return np.exp(-2.0 * np.sin(np.pi * delta) ** 2 / l ** 2) if periodic else np.exp(-0.5 * delta ** 2 / l ** 2)


def product_kernel(Xa, Xb, l, periodic, sf2):
    """k(a_i, b_j) [Ma, Mb] as the product of the axis factors on direct differences."""
    Xa, Xb = np.atleast_2d(np.asarray(Xa, dtype=float)), np.atleast_2d(np.asarray(Xb, dtype=float))
    k = np.full((Xa.shape[0], Xb.shape[0]), float(sf2))
    for d in range(Xa.shape[1]):
        k = k * factor(Xa[:, None, d] - Xb[None, :, d], l[d], periodic[d])
    return k


def axis_integral(c, l, periodic):
    """I_d(c) = int_0^1 kappa_d(u - c) du."""
    c = np.asarray(c, dtype=float)
    if periodic:
        return np.full(c.shape, ive(0, 1.0 / l ** 2))
    return l * np.sqrt(np.pi / 2.0) * (erf((1.0 - c) / (np.sqrt(2.0) * l)) + erf(c / (np.sqrt(2.0) * l)))


def axis_double_integral(l, periodic):
    """A_d = int_0^1 int_0^1 kappa_d(u - u') du du'."""
    if periodic:
        return float(ive(0, 1.0 / l ** 2))
    return 2.0 * (l * np.sqrt(np.pi / 2.0) * erf(1.0 / (np.sqrt(2.0) * l)) + l ** 2 * np.expm1(-0.5 / l ** 2))


def _rows(dims, t):
    dims, t = np.asarray(dims, dtype=int), np.asarray(t, dtype=float)
    if dims.ndim == 1:
        dims, t = dims.reshape(1, -1), t.reshape(1, -1)
    return dims, t


def marginal_column(dims, t, X, l, periodic, sf2, effect):
    """c [M, N] of the rows (dims [M, 2] with -1 = unused, t [M, 2])."""
    dims, t = _rows(dims, t)
    X = np.asarray(X, dtype=float)
    N, D = X.shape
    Q = np.stack([axis_integral(X[:, d], l[d], periodic[d]) for d in range(D)], axis=1)      # [N, D]
    P = float(sf2) * np.prod(Q, axis=1)
    c = np.zeros((dims.shape[0], N))
    for i, (row, tv) in enumerate(zip(dims, t)):
        r = [factor(tv[k] - X[:, d], l[d], periodic[d]) / Q[:, d] for k, d in enumerate(row) if d >= 0]
        if effect == INTERACTION:
            f = (r[0] - 1.0) * (r[1] - 1.0)
        else:
            f = np.prod(r, axis=0) if r else np.ones(N)
            if effect == CENTRED:
                f = f - 1.0
        c[i] = P * f
    return c


def marginal_prior(dims, t, l, periodic, sf2, effect):
    """The prior variance [M] of the functional of each row."""
    dims, t = _rows(dims, t)
    D = len(l)
    A = np.array([axis_double_integral(l[d], periodic[d]) for d in range(D)])
    out = np.zeros(dims.shape[0])
    for i, (row, tv) in enumerate(zip(dims, t)):
        kept = [(d, tv[k]) for k, d in enumerate(row) if d >= 0]
        S = float(sf2) * np.prod([A[d] for d in range(D) if d not in [k[0] for k in kept]])
        a = [float(axis_integral(tt, l[d], periodic[d])) for d, tt in kept]
        Ak = [A[d] for d, _ in kept]
        if effect == RAW:
            out[i] = S
        elif effect == CENTRED:
            out[i] = S * (1.0 - 2.0 * np.prod(a) + np.prod(Ak))
        else:
            out[i] = S * (1.0 - 2.0 * a[0] + Ak[0]) * (1.0 - 2.0 * a[1] + Ak[1])
    return out


def marginal_reference(dims, t, X, theta, kernel, alpha, A, effect):
    """(mu, var, c) of the rows: mu = c' alpha, var = prior - c' A c."""
    X = np.asarray(X, dtype=float)
    l, periodic = axes_of(theta, kernel, X.shape[1])
    sf2 = float(theta[2]) ** 2
    c = marginal_column(dims, t, X, l, periodic, sf2, effect)
    mu = c @ np.asarray(alpha, dtype=float)
    var = marginal_prior(dims, t, l, periodic, sf2, effect) - np.einsum("ij,ij->i", c, c @ A)
    return mu, var, c


def sign_probability(mu, var):
    """P(L f > 0) = Phi(mu / sqrt(max(var, 0))); no variance: the sign decides, a tie is 1/2."""
    return fn.threshold_probability(mu, var, 0.0)
