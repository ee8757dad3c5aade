"""NumPy statement of the answer to a query (ppbo_line_choice, GPModel.answer_pred / choice_pred) -- test infrastructure
only.  In draw s the user sees

    u[s] = mu + L z[s] + noise_sd e[s],     L L' = 0.5 (cov + cov') + jitter I     (oracle.line_samples)

and picks argmax_g u[s, g] (np.argmax: of equal values the first).  For G = 2 the probability of picking point 0 is the
duel's closed form Phi(mu_d / sqrt(2 noise_sd^2 + var_d)), mu_d = mu_0 - mu_1, var_d = C_00 + C_11 - 2 C_01."""
from __future__ import annotations

import numpy as np
import scipy.stats

from oracle import ppbo_oracle as orc


def utilities(mu, cov, z, e=None, noise_sd=0.0, jitter=0.0):
    """u [S, G] for stored standard-normal z [S, G] and e [S, G] (None: no noise)."""
    u = orc.line_samples(np.asarray(mu, dtype=float), np.asarray(cov, dtype=float), np.asarray(z, dtype=float), jitter)
    if e is not None and noise_sd != 0.0:
        u = u + float(noise_sd) * np.asarray(e, dtype=float)
    return u


def choice(mu, cov, z, e=None, noise_sd=0.0, jitter=0.0):
    """(choice [S], count [G], prob [G]) of the S draws."""
    u = utilities(mu, cov, z, e, noise_sd, jitter)
    c = u.argmax(axis=1)
    count = np.bincount(c, minlength=u.shape[1])
    return c, count, count / u.shape[0]


def top_two_gap(u):
    """max - second largest of every row of u [S, G] (inf for G = 1)."""
    if u.shape[1] < 2:
        return np.full(u.shape[0], np.inf)
    top = np.partition(u, -2, axis=1)[:, -2:]
    return top[:, 1] - top[:, 0]


def pair_closed_form(mu, cov, noise_sd, jitter=0.0):
    """P(point 0 is picked) for G = 2, exactly."""
    mu, C = np.asarray(mu, dtype=float), np.asarray(cov, dtype=float)
    C = 0.5 * (C + C.T) + jitter * np.eye(2)
    var_d = C[0, 0] + C[1, 1] - 2.0 * C[0, 1]
    return float(scipy.stats.norm.cdf((mu[0] - mu[1]) / np.sqrt(2.0 * float(noise_sd) ** 2 + max(var_d, 0.0))))
