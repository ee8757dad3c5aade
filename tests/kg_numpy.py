"""NumPy statements of the knowledge gradient for correlated beliefs (ppbo_kg_envelope, ppbo_predict_kg) -- test support.

For lines a_j + b_j z and Z ~ N(0, 1):  KG = E[max_j (a_j + b_j Z)] - max_j a_j = sum_k (beta_{k+1} - beta_k) psi(|c_k|)
over the kinks c_k of the upper envelope, beta the slopes on either side, psi(c) = phi(c) - c Phi(-c).  Two independent
statements of the envelope:

  kg_stack   lines sorted by slope, the classical stack scan (a line leaves the stack when the new one overtakes its
             predecessor no later than it did itself)
  kg_march   gift wrapping, the device kernel's statement: from the line of the smallest slope to the steeper line that
             crosses the current one first; every choice a minimum or a maximum over the lines

Both return (kg, kinks) for one row of lines; `rows` applies either to the rows of a slope matrix.
"""
import math

import numpy as np

SQRT2 = math.sqrt(2.0)
INV_SQRT_2PI = 0.39894228040143267794


def psi(c):
    """phi(c) - c Phi(-c) for c >= 0, Phi(-c) = erfc(c / sqrt 2) / 2 formed directly; 0 from c = 40 on (both terms are) and
    never negative (the terms cancel to phi(c) / c^2)."""
    c = float(c)
    if not c < 40.0:
        return 0.0
    return max(INV_SQRT_2PI * math.exp(-0.5 * c * c) - c * (0.5 * math.erfc(c / SQRT2)), 0.0)


def _finite(a, b):
    return bool(np.all(np.isfinite(a)) and np.all(np.isfinite(b)))


def kg_stack(a, b):
    """(kg, kinks) by the sorted-slope stack scan."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    if not _finite(a, b):
        return float("nan"), 0
    order = np.lexsort((-a, b))                      # by slope, of equal slopes the largest intercept first
    sa, sb = [], []                                  # the stack
    cross = []                                       # cross[k]: where stack line k + 1 overtakes line k
    last = None
    for j in order:
        if last is not None and b[j] == last:
            continue                                 # a parallel line below one already seen
        last = b[j]
        aj, bj = float(a[j]), float(b[j])
        while sa:
            c = (sa[-1] - aj) / (bj - sb[-1])
            if cross and c <= cross[-1]:
                sa.pop(), sb.pop(), cross.pop()      # the top is overtaken before (or as) it gets on top itself
                continue
            cross.append(c)
            break
        sa.append(aj), sb.append(bj)
    kg = 0.0
    for k, c in enumerate(cross):
        kg += (sb[k + 1] - sb[k]) * psi(abs(c))
    return kg, len(cross)


def kg_march(a, b):
    """(kg, kinks) by the march of the device kernel: every reduction a minimum or a maximum over the lines, the sum in
    march order, a counted loop of at most len(a) passes."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    if not _finite(a, b):
        return float("nan"), 0
    bcur = b.min()
    acur = a[b == bcur].max()
    kg, kinks = 0.0, 0
    for _ in range(len(a)):
        up = b > bcur
        if not up.any():
            break
        with np.errstate(over="ignore"):
            c = np.where(up, (acur - a) / np.where(up, b - bcur, 1.0), np.inf)
        cmin = c.min()
        sel = up & (c == cmin)
        bsel = b[sel].max()
        asel = a[sel & (b == bsel)].max()
        kg += (bsel - bcur) * psi(abs(cmin))
        acur, bcur = asel, bsel
        kinks += 1
    else:
        raise AssertionError("the march did not end within its count")
    return kg, kinks


def rows(a, slopes, self_a=None, self_b=None, fn=kg_march):
    """(kg [Ma], kinks [Ma]) of the rows of slopes [Ma, Mb] over the shared intercepts a [Mb], each row with its own line
    (self_a[i], self_b[i]) when given."""
    a, slopes = np.asarray(a, dtype=float), np.asarray(slopes, dtype=float)
    kg, kinks = np.empty(len(slopes)), np.empty(len(slopes), dtype=np.int64)
    for i, s in enumerate(slopes):
        la, lb = (a, s) if self_a is None else (np.append(a, self_a[i]), np.append(s, self_b[i]))
        kg[i], kinks[i] = fn(la, lb)
    return kg, kinks


def lines_from_posterior(mu_a, var_a, mu_b, cov, noise_var, Xa=None, Xb=None):
    """(a, slopes, self_a, self_b) of ppbo_predict_kg from the posterior of the candidates and the field: s = sqrt(max(var,
    0) + tau^2), field lines (mu_b[j], cov[i, j] / s_i), own line (mu_a[i], max(var_i, 0) / s_i); s = 0 gives slopes 0.
    With the points Xa [Ma, D], Xb [Mb, D]: a field point that IS candidate i (equal coordinates and an equal mean) takes
    the own line's slope -- cov(a, a) is var(a)."""
    mu_a, var_a, cov = np.asarray(mu_a, dtype=float), np.asarray(var_a, dtype=float), np.asarray(cov, dtype=float)
    mu_b = np.asarray(mu_b, dtype=float)
    v = np.where(np.isnan(var_a), var_a, np.maximum(var_a, 0.0))
    s = np.sqrt(v + noise_var)
    with np.errstate(divide="ignore", invalid="ignore"):
        slopes = np.where((s == 0.0)[:, None] & ~np.isnan(cov), 0.0, cov / s[:, None])
        self_b = np.where(s == 0.0, 0.0, v / s)
    if Xa is not None:
        Xa, Xb = np.asarray(Xa, dtype=float), np.asarray(Xb, dtype=float)
        same = mu_a[:, None] == mu_b[None, :]
        for d in range(Xa.shape[1]):
            same &= Xa[:, d][:, None] == Xb[:, d][None, :]
        slopes = np.where(same, self_b[:, None], slopes)
    return mu_b, slopes, mu_a, self_b


def best(kg):
    """(value, first index) of the largest non-NaN entry; (NaN, -1) when there is none."""
    kg = np.asarray(kg, dtype=float)
    if np.all(np.isnan(kg)):
        return float("nan"), -1
    i = int(np.nanargmax(kg))
    return float(kg[i]), i


def tangents(n, lo=-3.0, hi=3.0):
    """(a, b): the lines -t^2 / 2 + t z for n values of t in [lo, hi], the tangents of the convex z^2 / 2 -- every line is
    on the envelope, n - 1 kinks (at the midpoints of neighbouring t)."""
    t = np.linspace(lo, hi, n)
    return -0.5 * t * t, t
