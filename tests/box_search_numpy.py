"""NumPy restatement of the searches inside boxes (ppbo_mean_ascent_boxes, ppbo_mean_search_boxes in
ppbo_amd/csrc/meangrad.hip) -- test infrastructure only, no device code.  It extends tests/search_ref.py:

    ascent       bb_ascent_box, ascend_all_box, sensitivity_box     (bb_ascent_box_kernel)
    candidates   box_rows                                           (BoxCands, box_coord)
    inputs       boxes

bb_ascent_box is search_ref.bb_ascent with the box's three changes -- the clip to [lo, hi], the projection at lo and hi,
the first step of 0.02 times the longest side -- and the same branch margins; with lo = 0, hi = 1 it is bb_ascent state for
state."""
from __future__ import annotations

import numpy as np

import search_ref as sr

BOX_NAMES = ("unit", "inner", "fixed3", "slab", "ragged")
# the configurations of the ascent tests: every box at the suite's tolerance; at 1e-2 the boxes whose longest side is 1
# (in `inner` the first move is 0.02 * 0.5 = 1e-2 exactly, so the stopping decision sits on the tolerance itself and
# the margin rule drops up to 43 % of the pairs; in `ragged` every start stops at once)
CONFIGS = [(b, 1e-9) for b in BOX_NAMES] + [(b, 1e-2) for b in ("unit", "fixed3", "slab")]


def boxes(D):
    """The five test boxes {name: (lo [D], hi [D])}."""
    rng = np.random.default_rng(5 + D)
    v = 0.1 + 0.8 * rng.random(D)
    rlo = 0.6 * rng.random(D)
    rhi = rlo + 0.05 + 0.35 * rng.random(D)
    fixed = np.arange(D) % 3 == 1
    slab_lo, slab_hi = np.zeros(D), np.ones(D)
    slab_lo[0], slab_hi[0] = 0.5, 0.5 + 2.0 ** -10
    return {
        "unit": (np.zeros(D), np.ones(D)),
        "inner": (np.full(D, 0.2), np.full(D, 0.7)),
        "fixed3": (np.where(fixed, v, 0.0), np.where(fixed, v, 1.0)),
        "slab": (slab_lo, slab_hi),
        "ragged": (rlo, rhi),
    }


def project_box(x, g, lo, hi):
    return np.where(((x <= lo) & (g < 0.0)) | ((x >= hi) & (g > 0.0)), 0.0, g)


def bb_ascent_box(fg, x0, lo, hi, iters, tol, mu_scale=None):
    """The iteration of bb_ascent_box_kernel from one start inside [lo, hi]; returns search_ref.Ascent (states after
    n = 0 .. iters iterations and the branch margins, as search_ref.bb_ascent)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    wmax = float((hi - lo).max())
    x = np.clip(np.asarray(x0, dtype=np.float64), lo, hi)
    mu, g = fg(x)
    g = np.asarray(g, dtype=np.float64)
    step = (0.02 * wmax) / max(float(np.sqrt((g * g).sum())), 1e-300)      # the unprojected norm
    xs, mus, its = [x.copy()], [float(mu)], [0]
    margins = np.full((int(iters), 3), np.inf)
    it, stopped = 0, False
    for n in range(int(iters)):
        if not stopped:
            pg = project_box(x, g, lo, hi)
            pn = float(np.sqrt((pg * pg).sum()))
            if tol > 0:
                margins[n, 2] = abs(pn * step - tol) / tol
            if not (pn * step >= tol) or not (wmax > 0.0):
                stopped = True
            else:
                xn = np.clip(x + step * pg, lo, hi)
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
    return sr.Ascent(x, float(mu), it, np.asarray(xs), np.asarray(mus), np.asarray(its), margins)


def ascend_all_box(fg, starts, lo, hi, iters, tol, mu_scale=None):
    """bb_ascent_box from every row of starts, stacked as search_ref.ascend_all."""
    runs = [bb_ascent_box(fg, s, lo, hi, iters, tol, mu_scale) for s in np.atleast_2d(starts)]
    return (np.stack([r.xs for r in runs]), np.stack([r.mus for r in runs]), np.stack([r.its for r in runs]),
            np.stack([r.margins for r in runs]))


def sensitivity_box(fg, starts, lo, hi, iters, tol, mu_scale=None, seeds=(101, 202)):
    """search_ref.sensitivity of the boxed reference: against its 1e-13-perturbed self, one run per seed."""
    xs, mus, its, margins = ascend_all_box(fg, starts, lo, hi, iters, tol, mu_scale)
    keep = sr.kept_pairs(margins)
    dev, flips = np.zeros(iters + 1), 0
    for seed in seeds:
        xp, _, ip, _ = ascend_all_box(sr.perturbed(fg, np.random.default_rng(seed), 1e-13, mu_scale), starts, lo, hi, iters, tol,
                                      mu_scale)
        d = np.abs(xp - xs).max(axis=2)
        dev = np.maximum(dev, np.where(keep, d, 0.0).max(axis=0))
        flips += int(((ip != its) & keep).sum())
    return sr.Sensitivity(xs, mus, its, keep, dev, flips, 1.0 - keep.mean())


def box_rows(pool, shift, lo, hi, seeds=None):
    """rows [M + S, D]: the candidates of one trial of ppbo_mean_search_boxes.  Rows < M are lo + (hi - lo) u with
    u = frac(pool + shift) (u = pool when shift is None) -- the device forms fma(hi - lo, u, lo), which is the same number
    wherever the product is exact (lattice inputs, the unit box) and within an ulp of it elsewhere; the S seed rows
    follow, clipped into the box."""
    pool = np.asarray(pool, dtype=np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    u = pool
    if shift is not None:
        v = pool + np.asarray(shift, dtype=np.float64)[None, :]
        u = v - np.floor(v)
    rows = [lo[None, :] + (hi - lo)[None, :] * u]
    if seeds is not None and len(seeds):
        rows.append(np.clip(np.asarray(seeds, dtype=np.float64).reshape(-1, pool.shape[1]), lo, hi))
    return np.vstack(rows)
