"""NumPy statement of a greedy shortlist under the conditioned variance (ppbo_search_batch, Engine.search_batch,
GPModel.shortlist) -- test infrastructure only.  Column-wise: no M x M matrix is ever formed.  With (alpha, A) of
pairs_numpy.operator_from_fit and k_c = k(c, X), as in tournament_numpy:

    mu(c) = k_c' alpha,   var_0(c) = sf^2 - k_c' A k_c,   cov_0(c, p) = k(c, p) - k_c' A k_p

and for j = 0 .. q - 1, with tau^2 = noise_var:

    p_j        = the first index of the largest score(mu[c], var_j[c]) over the candidates not picked yet (NaN never wins)
    c_j[c]     = cov_0(c, p_j) - sum_{i<j} V_i[c] V_i[p_j]
    V_j[c]     = c_j[c] / sqrt(var_j[p_j] + tau^2)        (0 where the denominator is 0)
    var_j+1[c] = max(var_j[c] - V_j[c]^2, 0)

Every kernel value comes from direct differences (pairs_numpy.cross, or slopes_numpy.cross through `cross`)."""
from __future__ import annotations

import numpy as np
from scipy.special import erfc

import pairs_numpy as pn

MEAN, EI, VARIANCE = 0, 1, 2


def score_value(mu, var, kind, mustar):
    """The score of ppbo_predict from a mean and a variance: EI = d Phi(z) + sd phi(z), d = mu - mustar, sd =
    sqrt(max(var, 0)), z = d / sd, and max(d, 0) where sd = 0; VARIANCE = var; a NaN mean never scores."""
    mu, var = np.asarray(mu, dtype=float), np.asarray(var, dtype=float)
    if kind == VARIANCE:
        sc = var.copy()
    elif kind == EI:
        d = mu - mustar
        sd = np.sqrt(np.maximum(var, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(sd > 0.0, d / np.where(sd > 0.0, sd, 1.0), 0.0)
        sc = np.where(sd > 0.0, d * 0.5 * erfc(-z / np.sqrt(2.0)) + sd * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi),
                      np.maximum(d, 0.0))
    else:
        raise ValueError(f"unknown score kind {kind}")
    return np.where(np.isnan(mu), np.nan, sc)


def _prior(Xc, X, theta, kernel, alpha, A, cross):
    """(Kc [M, N], Kc A [M, N], mu [M], var_0 [M])."""
    Kc = cross(Xc, X, theta, kernel)
    KA = Kc @ np.asarray(A, dtype=float)
    return Kc, KA, Kc @ np.asarray(alpha, dtype=float), float(theta[2]) ** 2 - np.einsum("ij,ij->i", Kc, KA)


def _run(Xc, X, theta, kernel, alpha, A, q, kind, mustar, noise_var, cross, forced):
    Xc = np.atleast_2d(np.asarray(Xc, dtype=float))
    M = Xc.shape[0]
    Kc, KA, mu, var0 = _prior(Xc, X, theta, kernel, alpha, A, cross)
    var = var0.copy()
    V = np.zeros((q, M))
    picks, scores, gaps = np.full(q, -1, dtype=np.int64), np.full(q, np.nan), np.full(q, np.nan)
    taken = np.zeros(M, dtype=bool)
    for j in range(q):
        sc = score_value(mu, var, kind, mustar)
        ok = ~np.isnan(sc) & ~taken
        if not ok.any():
            break
        masked = np.where(ok, sc, -np.inf)
        pj = int(np.argmax(masked)) if forced is None else int(forced[j])
        if pj < 0:
            break
        picks[j], scores[j] = pj, sc[pj]
        rest = masked.copy()
        rest[pj] = -np.inf
        if np.isfinite(rest.max()):
            # the relative gap between the best and the runner-up: what keeps an index comparison honest
            gaps[j] = (sc[pj] - rest.max()) / max(abs(sc[pj]), np.finfo(float).tiny)
        else:
            gaps[j] = np.inf
        taken[pj] = True
        cj = cross(Xc, Xc[pj:pj + 1], theta, kernel)[:, 0] - KA @ Kc[pj]
        for i in range(j):
            cj = cj - V[i] * V[i, pj]
        den = var[pj] + noise_var
        V[j] = cj / np.sqrt(den) if den > 0.0 else 0.0
        nv = var - V[j] * V[j]
        var = np.where(np.isnan(nv), nv, np.maximum(nv, 0.0))
    return dict(idx=picks, score=scores, var_cond=var, gap=gaps, mu=mu, var=var0)


def greedy(Xc, X, theta, kernel, alpha, A, q, kind, mustar, noise_var, cross=pn.cross):
    """The greedy loop: dict(idx [q] int64, score [q], var_cond [M], gap [q], mu [M], var [M]); (-1, NaN) once nothing
    scoreable is left.  gap[j] is the relative distance of pick j's score to the runner-up's (inf when there is none)."""
    return _run(Xc, X, theta, kernel, alpha, A, q, kind, mustar, noise_var, cross, None)


def replay(picks, Xc, X, theta, kernel, alpha, A, kind, mustar, noise_var, cross=pn.cross):
    """The same quantities conditioned on a GIVEN pick sequence (score[j] = the score of picks[j] at its turn)."""
    picks = np.asarray(picks, dtype=np.int64)
    return _run(Xc, X, theta, kernel, alpha, A, len(picks), kind, mustar, noise_var, cross, picks)
