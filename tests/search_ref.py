"""NumPy restatement of the two stages every maximiser search shares (ppbo_amd/csrc/meangrad.hip) -- test
infrastructure only, no device code.

    start selection   select_capacity, thin, select_starts, trial_rows   (group_max_kernel, select_starts_kernel,
                                                                          StartSelection, TrialCands)
    ascent            bb_ascent, sensitivity                             (bb_ascent_kernel)
    objectives        fg_mean, fg_matern52, fg_ard, fg_camphor_ard, fg_rff, fg_rff_camphor, fg_path
    inputs            lattice, ascent_starts, host_fit, mean_case, rff_case

The selection is exact: it is fed the device's own scores and compares row indices.  The ascent is followed for a few
iterations, with the margin of every branch it takes, so that a test can leave out a start whose branch a rounding error
could flip and hold the rest to a bound measured here (sensitivity)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from evgrad_numpy import kappa
from oracle import ppbo_oracle as orc

PERIODIC = (0, 1, 3, 4, 5)
# a (start, n) pair is compared only while every branch margin up to n exceeds these: relative |mu_new - mu|, the
# cosine |curv| / (|s| |y|), | |pg| step - tol | / tol
MARGIN_MIN = np.array([1e-10, 1e-6, 1e-3])


# ---------------------------------------------------------------------------------------------- start selection
def select_capacity(D):
    """Survivors of the thinning: as many as fit one workgroup's LDS (144 KB) next to their D coordinates."""
    return min(4096, max(64, 147456 // (8 + 8 * int(D))))


def group_shape(M, D):
    """(G rows per group, Tg groups) for M scored rows."""
    cap = select_capacity(D)
    G = -(-int(M) // cap)
    return G, -(-int(M) // G)


def thin(scores, D):
    """(gval [Tg], gidx [Tg]): each group of G consecutive rows keeps its first maximum under strict >; NaN never wins; a
    group with nothing above -inf keeps (-inf, its first row)."""
    s = np.asarray(scores, dtype=np.float64).ravel()
    M = s.size
    G, Tg = group_shape(M, D)
    pad = np.full(Tg * G, -np.inf)
    pad[:M] = np.where(np.isnan(s), -np.inf, s)
    pad = pad.reshape(Tg, G)
    j = np.argmax(pad, axis=1)                    # first occurrence of the maximum
    return pad[np.arange(Tg), j], np.arange(Tg) * G + j


Selection = namedtuple("Selection", "idx count margin ties hits")


def select_starts(scores, cand, K, sep):
    """The greedy rule on the thinned survivors: at most K picks, each the first maximum among the live survivors; after
    a pick every live survivor with sum_d dx^2 <= sep^2 is struck (the winner too).  Returns the picked ROW indices in
    order, their number, the smallest |d2 - sep2| ever compared (inf if nothing was), the number of picks at which
    another live survivor tied the winner's score, and the number of comparisons with d2 == sep2 exactly."""
    cand = np.asarray(cand, dtype=np.float64)
    D = cand.shape[1]
    gval, gidx = thin(scores, D)
    sv = gval.copy()
    xc = cand[gidx]
    sep2 = float(sep) * float(sep)
    idx, margin, ties, hits = [], np.inf, 0, 0
    for _ in range(int(K)):
        w = int(np.argmax(sv))
        if not sv[w] > -np.inf:
            break
        idx.append(int(gidx[w]))
        live = np.flatnonzero(sv > -np.inf)
        ties += int((sv[live] == sv[w]).sum() > 1)
        d2 = np.zeros(live.size)
        for d in range(D):                        # the device's order of summation
            dx = xc[live, d] - xc[w, d]
            d2 += dx * dx
        margin = min(margin, float(np.abs(d2 - sep2).min()))
        hits += int((d2 == sep2).sum())
        sv[live[d2 <= sep2]] = -np.inf
    return Selection(np.asarray(idx, dtype=np.int64), len(idx), margin, ties, hits)


def greedy_by_sorting(scores, cand, K, sep):
    """The same rule stated independently, thinning included: a plain loop over the groups of G consecutive rows keeps
    each group's first row whose score no other row of the group exceeds (NaN counts as -inf); the survivors above -inf
    are sorted by (-score, index) and each is accepted iff it is MORE than sep away from every accepted one, until K are."""
    cand = np.asarray(cand, dtype=np.float64)
    s = [(-np.inf if np.isnan(v) else float(v)) for v in np.asarray(scores, dtype=np.float64).ravel()]
    M = len(s)
    cap = min(4096, max(64, (144 * 1024) // (8 * (1 + cand.shape[1]))))
    G = (M + cap - 1) // cap
    surv = []
    for lo in range(0, M, G):
        grp = s[lo:lo + G]
        top = max(grp)
        if top > -np.inf:
            surv.append((-top, lo + grp.index(top)))
    acc = []
    for _, i in sorted(surv):
        if len(acc) == int(K):
            break
        if all(float(((cand[i] - cand[a]) ** 2).sum()) > float(sep) * float(sep) for a in acc):
            acc.append(i)
    return np.asarray(acc, dtype=np.int64)


def trial_rows(pool, shifts, t, extra=None, xprev=None):
    """(rows [Mt, D], n): the candidates of trial t of ppbo_mean_search_multi.  Rows < M are frac(pool + shifts[t]); trial
    0 also carries the extra rows followed by xprev (n = Mt = M + E); in later trials those E slots are absent (n = M,
    their rows are zero here and they score -inf).  Grouping uses Mt in every trial."""
    pool = np.asarray(pool, dtype=np.float64)
    v = pool + np.asarray(shifts, dtype=np.float64)[t][None, :]
    rows = [v - np.floor(v)]
    tail = []
    if extra is not None:
        tail.append(np.asarray(extra, dtype=np.float64))
    if xprev is not None:
        tail.append(np.asarray(xprev, dtype=np.float64).reshape(1, -1))
    E = sum(a.shape[0] for a in tail)
    if t == 0:
        rows += tail
    elif E:
        rows.append(np.zeros((E, pool.shape[1])))
    return np.vstack(rows), pool.shape[0] + (E if t == 0 else 0)


def trial_scores(mu_present, Mt):
    """The score vector of a trial: the n present rows' scores, -inf in the absent slots."""
    out = np.full(int(Mt), -np.inf)
    out[:len(mu_present)] = mu_present
    return out


def lattice(rng, M, D, p):
    """M rows of D coordinates k / 2^p, k = 0 .. 2^p: differences, their squares and sums of up to 64 of them are exact
    in double, so no order of summation and no fused multiply-add can change a strike decision."""
    return rng.integers(0, 2 ** p + 1, size=(M, D)).astype(np.float64) / float(2 ** p)


# ---------------------------------------------------------------------------------------------- ascent
Ascent = namedtuple("Ascent", "x mu it xs mus its margins")


def _project(x, g):
    return np.where(((x <= 0.0) & (g < 0.0)) | ((x >= 1.0) & (g > 0.0)), 0.0, g)


def bb_ascent(fg, x0, iters, tol, mu_scale=None):
    """The iteration of bb_ascent_kernel from one start; fg(x) -> (mu, grad).  Returns the final x, mu and it, the states
    after n = 0 .. iters iterations (xs [iters + 1, D], mus, its; a stopped start repeats its last state) and the branch
    margins of iteration n -> n + 1 (margins [iters, 3]: relative |mu_new - mu| (against mu_scale, else the larger of the
    two), |curv| / (|s| |y|) of an accepted move, | |pg| step - tol | / tol; inf where the branch was not taken)."""
    x = np.clip(np.asarray(x0, dtype=np.float64), 0.0, 1.0)
    mu, g = fg(x)
    g = np.asarray(g, dtype=np.float64)
    step = 0.02 / max(float(np.sqrt((g * g).sum())), 1e-300)      # the unprojected norm
    xs, mus, its = [x.copy()], [float(mu)], [0]
    margins = np.full((int(iters), 3), np.inf)
    it, stopped = 0, False
    for n in range(int(iters)):
        if not stopped:
            pg = _project(x, g)
            pn = float(np.sqrt((pg * pg).sum()))
            if tol > 0:
                margins[n, 2] = abs(pn * step - tol) / tol
            if not (pn * step >= tol):
                stopped = True
            else:
                xn = np.clip(x + step * pg, 0.0, 1.0)
                mun, gnew = fg(xn)
                gnew = np.asarray(gnew, dtype=np.float64)
                ok = mun >= mu
                scale = mu_scale if mu_scale is not None else max(abs(mu), abs(mun), 1e-300)
                margins[n, 0] = abs(mun - mu) / scale
                s, y = xn - x, gnew - g
                curv, ss = -float((s * y).sum()), float((s * s).sum())
                if ok:
                    margins[n, 1] = abs(curv) / max(np.sqrt(ss) * float(np.sqrt((y * y).sum())), 1e-300)
                    step = ss / max(curv, 1e-300) if curv > 0.0 else 2.0 * step
                    x, g, mu = xn, gnew, mun
                else:
                    step = 0.25 * step
                it += 1
        xs.append(x.copy()); mus.append(float(mu)); its.append(it)
    return Ascent(x, float(mu), it, np.asarray(xs), np.asarray(mus), np.asarray(its), margins)


def ascend_all(fg, starts, iters, tol, mu_scale=None):
    """bb_ascent from every row of starts: xs [K, iters + 1, D], mus [K, iters + 1], its [K, iters + 1], margins
    [K, iters, 3]."""
    runs = [bb_ascent(fg, s, iters, tol, mu_scale) for s in np.atleast_2d(starts)]
    return (np.stack([r.xs for r in runs]), np.stack([r.mus for r in runs]), np.stack([r.its for r in runs]),
            np.stack([r.margins for r in runs]))


def kept_pairs(margins):
    """keep [K, iters + 1]: (start, n) is compared iff every branch margin of iterations < n exceeds MARGIN_MIN."""
    K, iters, _ = margins.shape
    good = np.all(margins > MARGIN_MIN[None, None, :], axis=2)
    keep = np.ones((K, iters + 1), dtype=bool)
    keep[:, 1:] = np.logical_and.accumulate(good, axis=1)
    return keep


def perturbed(fg, rng, rel=1e-13, mu_scale=None):
    """fg with mu and the gradient disturbed by rel (uniform in [-rel, rel]): of mu_scale (else |mu|) and of max |g|."""
    def f(x):
        mu, g = fg(x)
        g = np.asarray(g, dtype=np.float64)
        ms = mu_scale if mu_scale is not None else abs(mu)
        return (mu + rel * rng.uniform(-1, 1) * ms, g + rel * rng.uniform(-1, 1, g.shape) * np.abs(g).max())
    return f


Sensitivity = namedtuple("Sensitivity", "xs mus its keep dev flips left_out")


def sensitivity(fg, starts, iters, tol, mu_scale=None, seeds=(101, 202)):
    """The reference against its 1e-13-perturbed self (one run per seed): dev [iters + 1] the largest |x - x'|_inf over
    the kept starts after n iterations, flips the number of kept (start, n) pairs whose `it` differs, left_out the share
    of pairs the margins exclude."""
    xs, mus, its, margins = ascend_all(fg, starts, iters, tol, mu_scale)
    keep = kept_pairs(margins)
    dev, flips = np.zeros(iters + 1), 0
    for seed in seeds:
        xp, _, ip, _ = ascend_all(perturbed(fg, np.random.default_rng(seed), 1e-13, mu_scale), starts, iters, tol, mu_scale)
        d = np.abs(xp - xs).max(axis=2)
        dev = np.maximum(dev, np.where(keep, d, 0.0).max(axis=0))
        flips += int(((ip != its) & keep).sum())
    return Sensitivity(xs, mus, its, keep, dev, flips, 1.0 - keep.mean())


def x_bound(dev):
    """The bound on |x_device - x_ref|_inf after n iterations: 100 times the reference's own deviation under a relative
    1e-13 (the device's mean and gradient agree with the oracle to a few 1e-12, not 1e-13), floored at 1e-10."""
    return np.maximum(100.0 * np.asarray(dev), 1e-10)


def ascent_starts(D, seed, fg=None):
    """24 starts: 12 interior, 4 outside the box (the clip), 4 on faces, 4 corners.  With fg, four of the interior ones are
    moved next to a maximiser of fg (the reference's own, 0.004 .. 0.04 away): from there the first move of 0.02 overshoots
    or nearly arrives, so a stopping tolerance of 1e-2 ends them after one or two evaluated moves."""
    rng = np.random.default_rng(seed)
    inner = 0.05 + 0.9 * rng.random((12, D))
    if fg is not None:
        for r, dist in enumerate((0.004, 0.013, 0.035, 0.04)):
            u = rng.standard_normal(D)
            inner[r] = np.clip(bb_ascent(fg, inner[r], 60, 1e-12).x + dist * u / np.sqrt((u * u).sum()), 0.0, 1.0)
    out = rng.random((4, D))
    for r in range(4):
        j = rng.integers(0, D)
        out[r, j] = (-0.2, 1.3, -1e-3, 1.0 + 1e-9)[r]
        if D > 1:
            out[r, (j + 1) % D] = (1.25, -0.5, 0.5, 0.25)[r]
    face = 0.05 + 0.9 * rng.random((4, D))
    for r in range(4):
        face[r, rng.integers(0, D)] = float(r % 2)
        face[r, rng.integers(0, D)] = float((r // 2) % 2)
    corner = rng.integers(0, 2, size=(4, D)).astype(np.float64)
    return np.vstack([inner, out, face, corner])


# ---------------------------------------------------------------------------------------------- objectives
def fg_mean(X, theta, alpha, kernel):
    """Posterior mean and gradient by the oracle (SE_kernel, RQ_kernel, camphor_copper_kernel)."""
    def f(x):
        mu, g = orc.mean_grad(x[None, :], X, theta, alpha, kernel)
        return float(mu[0]), g[0]
    return f


def fg_matern52(X, theta, alpha):
    """Matern-5/2 in closed form: k = sf^2 (1 + a + a^2 / 3) e^-a, a = sqrt(5) r / l;
    dk / dx = -sf^2 (5 / (3 l^2)) (1 + a) e^-a (x - x_i)."""
    l, sf2 = float(theta[1]), float(theta[2]) ** 2

    def f(x):
        d = x[None, :] - X
        a = np.sqrt(5.0 * (d * d).sum(axis=1)) / l
        e = np.exp(-a)
        mu = float((alpha * sf2 * (1.0 + a + a * a / 3.0) * e).sum())
        return mu, -(alpha * sf2 * (5.0 / (3.0 * l * l)) * (1.0 + a) * e) @ d
    return f


def fg_ard(X, theta, alpha, kernel):
    """A radial kernel with theta[1] a scalar or one length scale per coordinate, in the caller's coordinates:
    k = sf^2 kappa(rho^2), rho^2 = sum_d ((x_d - x_i,d) / l_d)^2, dk / dx_d = 2 sf^2 kappa'(rho^2) (x_d - x_i,d) / l_d^2."""
    X = np.asarray(X, dtype=np.float64)
    l = np.broadcast_to(np.asarray(theta[1], dtype=np.float64), (X.shape[1],))
    sf2 = float(theta[2]) ** 2

    def f(x):
        d = (x[None, :] - X) / l
        k, dk = kappa((d * d).sum(axis=1), kernel)
        return float(sf2 * (alpha * k).sum()), (2.0 * sf2 * (alpha * dk)) @ (d / l)
    return f


def fg_camphor_ard(Xc, l, sf, alpha):
    """camphor-copper with six length scales in the caller's coordinates: k = sf^2 exp(-sum_periodic 2 sin^2(pi dx) / l_d^2
    - dz^2 / (2 l_2^2))."""
    l = np.asarray(l, dtype=np.float64)

    def f(x):
        d = x[None, :] - Xc
        s = 0.5 * d[:, 2] ** 2 / l[2] ** 2
        for j in PERIODIC:
            s = s + 2.0 * np.sin(np.pi * d[:, j]) ** 2 / l[j] ** 2
        w = alpha * (sf * sf) * np.exp(-s)
        fac = -(2.0 * np.pi / l ** 2)[None, :] * np.sin(2.0 * np.pi * d)
        fac[:, 2] = -d[:, 2] / l[2] ** 2
        return float(w.sum()), w @ fac
    return f


def fg_rff(W, b, sigma_f, omega):
    """One posterior sample in weight space: a sum_f omega_f cos(w_f.x + b_f), a = sqrt(2 sf^2 / F)."""
    W, b, omega = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64).ravel(), np.asarray(omega, dtype=np.float64).ravel()
    a = np.sqrt(2.0 * float(sigma_f) ** 2 / W.shape[0])

    def f(x):
        ph = W @ x + b
        return float(a * (omega @ np.cos(ph))), -a * ((omega * np.sin(ph)) @ W)
    return f


def camphor_embed(x, l):
    """e(x) [11] in the column order (c0, s0, c1, s1, z, c3, s3, c4, s4, c5, s5) and de / dx [11, 6]."""
    e, J, c = np.zeros(11), np.zeros((11, 6)), 0
    for d in range(6):
        if d == 2:
            e[c] = x[2] / l[2]
            J[c, 2] = 1.0 / l[2]
            c += 1
        else:
            cs, sn = np.cos(2 * np.pi * x[d]) / l[d], np.sin(2 * np.pi * x[d]) / l[d]
            e[c], e[c + 1] = cs, sn
            J[c, d], J[c + 1, d] = -2 * np.pi * sn, 2 * np.pi * cs
            c += 2
    return e, J


def fg_rff_camphor(W, b, sigma_f, omega, l):
    """fg_rff over a camphor basis W [F, 11] on the embedding, in the caller's six coordinates."""
    inner = fg_rff(W, b, sigma_f, omega)
    l = np.asarray(l, dtype=np.float64)

    def f(x):
        e, J = camphor_embed(x, l)
        v, ge = inner(e)
        return v, ge @ J
    return f


def fg_path(W, b, theta, kernel, X, w, v):
    """One pathwise sample: the feature half (weights w) plus the kernel half (weights v over the design X), theta[1] a
    scalar or per-dimension length scales; everything in the caller's coordinates."""
    fa, fb = fg_rff(W, b, theta[2], w), fg_ard(X, theta, np.asarray(v, dtype=np.float64), kernel)

    def f(x):
        (m1, g1), (m2, g2) = fa(x), fb(x)
        return m1 + m2, g1 + g2
    return f


# ---------------------------------------------------------------------------------------------- models
def host_gram(X, theta, kernel):
    """The shrunk Gram matrix on the host: the oracle's for its three kernels, else from direct differences."""
    if kernel in orc.KERNELS and np.ndim(theta[1]) == 0:
        return orc.gram(X, theta, kernel)
    if kernel == "camphor_copper_ard_kernel":
        l = np.asarray(theta[1], dtype=np.float64)
        s = np.zeros((X.shape[0], X.shape[0]))
        for d in range(6):
            dx = X[:, d][:, None] - X[:, d][None, :]
            s += 2.0 * np.sin(np.pi * np.abs(dx)) ** 2 / l[d] ** 2 if d != 2 else 0.5 * dx * dx / l[2] ** 2
        return orc.regularize_covariance(float(theta[2]) ** 2 * np.exp(-s), orc.SHRINKAGE)
    Xs = X / np.broadcast_to(np.asarray(theta[1], dtype=np.float64), (X.shape[1],))
    return orc.regularize_covariance(float(theta[2]) ** 2 * kappa(orc.sqdist_direct(Xs, Xs), kernel)[0], orc.SHRINKAGE)


def host_fit(X, theta, kernel, m, seed):
    """(f_MAP, Sigma^-1) of a tiny synthetic model on the host, as test_searches_in_every_dimension_bucket fits its own: a
    prior draw for the start, the oracle's trust-region fit."""
    S0 = host_gram(X, theta, kernel)
    Sinv0 = orc.pd_inverse(S0)
    f_init = np.random.default_rng(seed).multivariate_normal(np.zeros(X.shape[0]), S0, method="cholesky")
    f0, _ = orc.fit_fmap_trust_exact(f_init, Sinv0, m, theta[0], gtol=1e-9)
    return f0, Sinv0


# ---------------------------------------------------------------------------------------------- the ascent cases
# one per compiled (DP, NT) shape of the mean ascent, then camphor-copper (the reference kernel), ARD in the caller's
# coordinates and camphor-copper with six length scales; tall designs (N = 1024) take the wide workgroups
CAMPHOR_LS = np.array([0.3, 0.4, 0.5, 0.6, 0.8, 1.0])
MEAN_CASES = {
    "se_d3": dict(D=3, kernel="SE_kernel", n_q=10, m=4),                       # (8, 256)
    "rq_d10": dict(D=10, kernel="RQ_kernel", n_q=10, m=4),                     # (24, 256)
    "matern52_d33": dict(D=33, kernel="Matern52_kernel", n_q=10, m=4),         # (64, 256)
    "se_d6_tall": dict(D=6, kernel="SE_kernel", n_q=32, m=31),                 # (8, 1024)
    "se_d20_tall": dict(D=20, kernel="SE_kernel", n_q=32, m=31),               # (24, 512)
    "camphor": dict(D=6, kernel="camphor_copper_kernel", n_q=10, m=4, l=1.0),
    "ard_se_d5": dict(D=5, kernel="SE_kernel", n_q=10, m=4, l=np.array([0.3, 0.5, 0.8, 1.1, 1.6])),
    "camphor_ard": dict(D=6, kernel="camphor_copper_ard_kernel", n_q=10, m=4, l=CAMPHOR_LS),
}
TOLS = (1e-9, 1e-2)              # the suite's stopping tolerance, and one at which some starts stop after a move or two
ASCENT_ITERS = 6


def mean_case(name):
    """(X, theta, kernel, m) of a mean-ascent case."""
    c = MEAN_CASES[name]
    D = c["D"]
    th = [0.1, c.get("l", 0.35 * np.sqrt(D)), 0.7]
    return orc.synthetic_design(c["n_q"], D, m=c["m"], seed=100 + D), th, c["kernel"], c["m"]


def mean_fg(X, theta, kernel, alpha):
    """The objective of a mean-ascent case in the caller's coordinates, from the design, theta and Sigma^-1 f_MAP."""
    if kernel == "camphor_copper_ard_kernel":
        return fg_camphor_ard(X, theta[1], theta[2], alpha)
    if np.ndim(theta[1]) > 0:
        return fg_ard(X, theta, alpha, kernel)
    if kernel == "Matern52_kernel":
        return fg_matern52(X, theta, alpha)
    return fg_mean(X, theta, alpha, kernel)


RFF_CASES = {                    # D (caller coordinates), F, camphor basis
    "d6_f96": (6, 96, False), "d6_f1024": (6, 1024, False), "d20_f1024": (20, 1024, False), "d33_f96": (33, 96, False),
    "camphor_f96": (6, 96, True), "camphor_f1024": (6, 1024, True),
}


def rff_case(name, S=1):
    """(cand [600, D], W, b, sigma_f, omegas [S, F], ls or None) of an RFF ascent case."""
    D, F, cam = RFF_CASES[name]
    rng = np.random.default_rng(1000 + 7 * D + F + int(cam))
    W = rng.standard_normal((F, 11)) if cam else rng.standard_normal((F, D)) / (0.35 * np.sqrt(D))
    return rng.random((600, D)), W, rng.uniform(0, 2 * np.pi, F), 0.7, rng.standard_normal((S, F)), (CAMPHOR_LS if cam else None)


def rff_fg(W, b, sigma_f, omega, ls):
    return fg_rff(W, b, sigma_f, omega) if ls is None else fg_rff_camphor(W, b, sigma_f, omega, ls)
